"""Host-side mirror of the reference's Ruby API over the C ABI.

``RawMap`` mirrors the C glue class ``Blurrily::RawMap`` (ext/blurrily/map_ext.c:206-229:
``new``/``load``, ``put/3``, ``delete/1``, ``save/1``, ``find/2``, ``stats/0``, ``close/0``,
``ClosedError``); ``Map`` mirrors ``Blurrily::Map`` (lib/blurrily/map.rb:8-47: string
normalisation, default weight/limit, clean-path save elision).  Same names, same argument
meaning, same error behaviour -- so tests read like spec/blurrily/map_spec.rb.

Every method reads: check open, convert the arguments, call the C function by name, shape the result.  What the
conversions and the shaping share is in the helpers below, once each.

The image has no Ruby; INTEGRATION.md shows the Ruby side of the same boundary.
"""
import ctypes as C
import os
import re
import unicodedata
from contextlib import contextmanager as _contextmanager
from errno import ERANGE as _ERANGE

import numpy as np

from . import _native
from .defaults import LIMIT_DEFAULT

_U32_MAX = 0xFFFFFFFF
_NO_BYTES = C.create_string_buffer(1)


class ClosedError(RuntimeError):
    """Blurrily::RawMap::ClosedError (map_ext.c:216)."""


def _raise_errno(path=None):
    err = C.get_errno()
    raise OSError(err, os.strerror(err), path)


def _check(res, path=None):
    """The result of a C call that can fail: negative -> OSError from errno (with the path where one is given)."""
    if res < 0:
        _raise_errno(path)
    return res


def _u32(value, what):
    """NUM2UINT (map_ext.c:85-86): reject what does not fit an unsigned 32-bit integer."""
    v = int(value)
    if not 0 <= v <= _U32_MAX:
        raise OverflowError(f"{what} {value!r} out of range of unsigned int")
    return v


def _permille(value):
    mp = _u32(value, "min_permille")
    if mp > 1000:
        raise ValueError(f"min_permille {value!r} above 1000")
    return mp


def _floors(floors):
    """The floors of a cluster_levels call: 1 .. CLUSTER_MAX_LEVELS per-mille values, strictly ascending."""
    fl = [_permille(f) for f in floors]
    if not 1 <= len(fl) <= _native.CLUSTER_MAX_LEVELS:
        raise ValueError(f"{len(fl)} floors: one call takes 1 to {_native.CLUSTER_MAX_LEVELS}")
    if any(a >= b for a, b in zip(fl, fl[1:])):
        raise ValueError(f"floors {fl!r} not strictly ascending")
    return np.array(fl, dtype=np.uint32)


def _find_limit(limit):
    """The single finds' limit (map_ext.c:131-146), as the C function takes it."""
    limit = int(limit)
    if not -(1 << 31) <= limit <= _U32_MAX:
        raise OverflowError("limit out of range")
    if limit > 0x7FFFFFFF:
        limit -= 1 << 32                      # NUM2UINT into an `int` (map_ext.c:135)
    if limit <= 0:
        limit = LIMIT_DEFAULT                 # map_ext.c:142-146
    return limit & 0xFFFF                     # uint16_t parameter (storage.h:110)


def _batch_limit(limit):
    """The batched methods' limit: the uint16_t parameter, nothing else."""
    return int(limit) & 0xFFFF


def _pack(needles):
    """list of bytes -> (packed bytes buffer, uint64 offsets[n+1])."""
    offsets = np.zeros(len(needles) + 1, dtype=np.uint64)
    if needles:
        offsets[1:] = np.cumsum([len(b) for b in needles], dtype=np.uint64)
    return b"".join(needles), offsets


def _needles(packed, offsets):
    """Packed needles as the C side takes them: (pointer to the bytes, contiguous uint64 offsets[n + 1], n).  Needles
    that are all empty have no bytes to point to and get a dummy byte (NULL with n > 0 is an argument error to some
    entries); NULL only for n == 0.  `packed` and an `offsets` that is already right are not copied: the caller's
    stay alive through the call."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    buf = packed if isinstance(packed, np.ndarray) else np.frombuffer(packed, dtype=np.uint8)
    return buf.ctypes.data if buf.size else (C.addressof(_NO_BYTES) if n > 0 else None), offsets, n


def _blocks(n, limit, row_ntri=False, per_needle=0):
    """What a batched find fills: rows[n, max(limit, 1), 3], counts[n], with `row_ntri` a word per row
    [n, max(limit, 1)], and `per_needle` more blocks of [n]; all uint32.  Returns (what to hand back -- rows and
    row_ntri cut to [:, :limit] --, the pointers for the C call in the same order)."""
    room = max(limit, 1)
    full = [np.zeros((n, room, 3), dtype=np.uint32), np.zeros(n, dtype=np.uint32)]
    if row_ntri:
        full.append(np.zeros((n, room), dtype=np.uint32))
    full += [np.zeros(n, dtype=np.uint32) for _ in range(per_needle)]
    return tuple(a[:, :limit] if a.ndim > 1 else a for a in full), [a.ctypes.data for a in full]


def _call_growing(call, cap, needed, row=(), dtype=np.uint32):
    """``call(pointer, cap)`` into a buffer of `cap` rows (np.empty: only the pages written are committed); when the
    library answers ERANGE it has reported the room it needs (``needed()``), and the call is made once more with
    that.  Returns the buffer filled."""
    while True:
        buf = np.empty((cap,) + row, dtype=dtype)
        if call(buf.ctypes.data, cap) == 0:
            return buf
        if C.get_errno() != _ERANGE or needed() <= cap:
            _raise_errno()
        cap = needed()


def _lists(rows, counts, row_ntri=None):
    """rows[n, limit, 3] and counts[n] -> n lists of ``[ref, matches, weight]``; with row_ntri[n, limit], of
    ``[ref, matches, weight, R]``."""
    if row_ntri is None:
        return [rows[i, :c].tolist() for i, c in enumerate(counts.tolist())]
    return [[r + [t] for r, t in zip(rows[i, :c].tolist(), row_ntri[i, :c].tolist())]
            for i, c in enumerate(counts.tolist())]


class RawMap:
    """Thin object wrapper over a ``trigram_map`` handle (map_ext.c)."""

    ClosedError = ClosedError

    def __init__(self, _handle=None):
        self._lib = _native.lib()
        if _handle is None:
            _handle = C.c_void_p()
            _check(self._lib.blurrily_storage_new(C.byref(_handle)))          # map_ext.c:49-50
        self._h = _handle
        self._closed = False

    # -- construction ---------------------------------------------------------------
    @classmethod
    def load(cls, path):
        """map_ext.c:59-71 -- Errno::* on failure (ENOENT, EPROTO ...)."""
        h = C.c_void_p()
        _check(_native.lib().blurrily_storage_load(C.byref(h), os.fsencode(path)), path)
        obj = cls.__new__(cls)
        RawMap.__init__(obj, _handle=h)
        return obj

    def __del__(self):                                              # blurrily_free, map_ext.c:25-32
        try:
            if not getattr(self, "_closed", True) and self._h:
                self._lib.blurrily_storage_close(C.byref(self._h))
                self._closed = True
        except Exception:
            pass

    def _check_open(self):
        if self._closed:
            raise ClosedError("Map was freed")                      # map_ext.c:11-16

    # -- reference surface ----------------------------------------------------------
    def put(self, needle, reference, weight):
        """map_ext.c:81-95 -> blurrily_storage_put.  Returns #trigrams added (0 for a dup ref)."""
        self._check_open()
        res = self._lib.blurrily_storage_put(self._h, _as_bytes(needle), _u32(reference, "reference"),
                                             _u32(weight, "weight"))
        assert res >= 0
        return res

    def delete(self, reference):
        """map_ext.c:99-111."""
        self._check_open()
        res = self._lib.blurrily_storage_delete(self._h, _u32(reference, "reference"))
        assert res >= 0
        return res

    def save(self, path):
        """map_ext.c:115-127."""
        self._check_open()
        _check(self._lib.blurrily_storage_save(self._h, os.fsencode(path)), path)
        return None

    def find(self, needle, limit):
        """map_ext.c:131-162: limit <= 0 -> LIMIT_DEFAULT; rows ``[ref, matches, weight]``."""
        self._check_open()
        c_limit = _find_limit(limit)
        rows = (_native.TrigramMatch * max(c_limit, 1))()
        res = _check(self._lib.blurrily_storage_find(self._h, _as_bytes(needle), c_limit, rows))
        return [[rows[k].reference, rows[k].matches, rows[k].weight] for k in range(res)]

    def stats(self):
        """map_ext.c:167-184."""
        self._check_open()
        st = _native.TrigramStat()
        res = self._lib.blurrily_storage_stats(self._h, C.byref(st))
        assert res >= 0
        return {"references": st.references, "trigrams": st.trigrams}

    def close(self):
        """map_ext.c:188-202."""
        self._check_open()
        _check(self._lib.blurrily_storage_close(C.byref(self._h)))
        self._closed = True
        return None

    # -- batched extensions (no reference counterpart) -------------------------------
    def put_many(self, needles, references, weights=None):
        """Same as ``put`` for each element, in order; returns total trigrams added."""
        self._check_open()
        packed, offsets = _pack([_as_bytes(s) for s in needles])
        refs = np.ascontiguousarray(references, dtype=np.uint32)
        wts = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint32)
        return self.put_many_packed(packed, offsets, refs, wts)

    def put_many_packed(self, packed, offsets, refs, weights=None):
        self._check_open()
        data, offsets, _ = _needles(packed, offsets)
        return _check(self._lib.blurrily_storage_put_many(
            self._h, data, offsets.ctypes.data, refs.ctypes.data, None if weights is None else weights.ctypes.data,
            len(refs)))

    def find_batch_packed(self, packed, offsets, limit):
        """n finds in one GPU batch.  Returns (rows[n, limit, 3] uint32, counts[n] uint32)."""
        self._check_open()
        limit = _batch_limit(limit)
        data, offsets, n = _needles(packed, offsets)
        out, ptrs = _blocks(n, limit)
        _check(self._lib.blurrily_storage_find_batch(self._h, data, offsets.ctypes.data, n, limit, *ptrs))
        return out

    def find_batch_raw_packed(self, packed, offsets, limit):
        """find_batch_packed over un-normalised ASCII needles: normalize_string runs on the device
        (blurrily_storage_find_batch_raw).  Returns (rows, counts, non_ascii[n] uint32)."""
        self._check_open()
        limit = _batch_limit(limit)
        data, offsets, n = _needles(packed, offsets)
        out, ptrs = _blocks(n, limit, per_needle=1)
        _check(self._lib.blurrily_storage_find_batch_raw(self._h, data, offsets.ctypes.data, n, limit, *ptrs))
        return out

    # -- by reference (reference storage.h:72-87's commented-out get; find what is like a stored entry) ---------
    def _refs(self, references):
        refs = np.asarray(references)
        if refs.ndim != 1:
            raise ValueError("references must be one-dimensional")
        if refs.dtype != np.uint32:
            refs = np.array([_u32(r, "reference") for r in refs.tolist()], dtype=np.uint32)
        return np.ascontiguousarray(refs)

    def get(self, reference):
        """``(weight, codes)`` of a stored reference -- its trigram codes ascending, what the tokeniser gives for the
        string it was put with -- or None when the map does not hold it (blurrily_storage_get)."""
        self._check_open()
        codes = np.zeros(28 * 28 * 28, dtype=np.uint16)
        weight = C.c_uint32(0)
        res = _check(self._lib.blurrily_storage_get(self._h, _u32(reference, "reference"), C.byref(weight), len(codes),
                                                    codes.ctypes.data))
        if res == 0:
            return None
        return int(weight.value), codes[:res].tolist()

    def get_batch(self, references):
        """``get`` for every reference at once: ``(weights[n], code_offsets[n + 1], codes)`` -- reference i's codes are
        ``codes[code_offsets[i]:code_offsets[i + 1]]``, an empty range when the map does not hold it (weight 0)."""
        self._check_open()
        refs = self._refs(references)
        n = len(refs)
        # each distinct reference once: their codes together are at most the map's trigram count (the library's
        # extraction also reads each once), so one call always fits
        uniq, inv = np.unique(refs, return_inverse=True)
        n_u = len(uniq)
        w_u = np.zeros(n_u, dtype=np.uint32)
        offs_u = np.zeros(n_u + 1, dtype=np.uint64)
        codes_u = _call_growing(
            lambda codes, cap: self._lib.blurrily_storage_get_batch(
                self._h, uniq.ctypes.data if n_u else None, n_u, w_u.ctypes.data, offs_u.ctypes.data, codes, cap),
            max(1, min(self.stats()["trigrams"], n_u * 28 * 28 * 28)), lambda: int(offs_u[n_u]), dtype=np.uint16)
        # back to the caller's order, duplicates included
        starts = offs_u[:-1].astype(np.int64)[inv]
        lens = np.diff(offs_u.astype(np.int64))[inv]
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(lens)
        at = np.repeat(starts - offs[:-1].astype(np.int64), lens) + np.arange(int(offs[n]), dtype=np.int64)
        return w_u[inv], offs, codes_u[at]

    def find_batch_by_reference(self, references, limit):
        """Find what is like each stored reference: element i is ``find(s_i, limit)`` for the string reference i was put
        with (the reference itself among the rows, normally first; none for a reference the map does not hold).
        Returns (rows[n, limit, 3] uint32, counts[n] uint32, nb_trigrams[n] uint32)."""
        self._check_open()
        refs = self._refs(references)
        n = len(refs)
        limit = _batch_limit(limit)
        out, ptrs = _blocks(n, limit, per_needle=1)
        _check(self._lib.blurrily_storage_find_references(self._h, refs.ctypes.data if n else None, n, limit, *ptrs))
        return out

    def find_by_reference(self, reference, limit):
        """``find``'s rows for the string `reference` was put with ([] when the map does not hold it); `limit` as find's."""
        self._check_open()
        c_limit = _find_limit(limit)
        rows, counts, _ = RawMap.find_batch_by_reference(self, [_u32(reference, "reference")], c_limit)
        return rows[0, :counts[0]].tolist()

    # -- scoped find (no reference counterpart: the reference keeps one map per scope, map_group.rb) -----------
    def scope(self, references):
        """A ``Scope`` of these references (a fixed set; duplicates count once, references the map does not hold are
        ignored).  Nothing reaches the GPU until its first scoped find."""
        self._check_open()
        refs = self._refs(references if isinstance(references, np.ndarray) else list(references))
        h = C.c_void_p()
        _check(self._lib.blurrily_scope_new(self._h, refs.ctypes.data if len(refs) else None, len(refs), C.byref(h)))
        return Scope(self, h, np.unique(refs))

    def _own(self, scope):
        """`scope`, checked: a Scope of this map, and open."""
        if scope._map is not self:
            raise ValueError("the scope belongs to another map")
        scope._check_open()
        return scope

    @_contextmanager
    def _scopes_of(self, scopes):
        """``with self._scopes_of(scopes) as scs``: a Scope for each element -- a plain iterable of references is made
        into a scope for this one call, and closed on the way out (also when making a later one fails)."""
        once = []
        try:
            scs = []
            for s in scopes:
                if isinstance(s, Scope):
                    scs.append(self._own(s))
                else:
                    once.append(self.scope(s))
                    scs.append(once[-1])
            yield scs
        finally:
            for sc in once:
                sc.close()

    @staticmethod
    def _handles(scs):
        """The scopes' handles as the ``blurrily_scope*`` array of the each-in entries (NULL for none)."""
        return (C.c_void_p * len(scs))(*[sc._h.value for sc in scs]) if scs else None

    def find_batch_in(self, scope, packed, offsets, limit):
        """``find_batch_packed`` among the scope's members only.  Returns (rows[n, limit, 3] uint32, counts[n] uint32)."""
        self._check_open()
        if not isinstance(scope, Scope):
            with self.scope(scope) as one_shot:
                return RawMap.find_batch_in(self, one_shot, packed, offsets, limit)
        sc = self._own(scope)
        limit = _batch_limit(limit)
        data, offsets, n = _needles(packed, offsets)
        out, ptrs = _blocks(n, limit)
        _check(self._lib.blurrily_storage_find_batch_in(self._h, sc._h, data, offsets.ctypes.data, n, limit, *ptrs))
        return out

    # -- a scope per needle -----------------------------------------------------------------
    @staticmethod
    def _which(which, n):
        """uint32[n]: a scope index per needle, None -> NO_SCOPE (the whole map)."""
        if len(which) != n:
            raise ValueError(f"which has {len(which)} elements for {n} needles")
        if isinstance(which, np.ndarray) and which.dtype == np.uint32:
            return np.ascontiguousarray(which)
        return np.array([_native.NO_SCOPE if w is None else _u32(w, "scope index") for w in which], dtype=np.uint32)

    def find_batch_each_in(self, scopes, which, packed, offsets, limit):
        """``find_batch_packed`` with a scope per needle: needle i among ``scopes[which[i]]`` only, or the whole map when
        ``which[i]`` is None.  Returns (rows[n, limit, 3] uint32, counts[n] uint32)."""
        self._check_open()
        which = self._which(which, len(offsets) - 1)
        with self._scopes_of(scopes) as scs:
            limit = _batch_limit(limit)
            data, offsets, n = _needles(packed, offsets)
            out, ptrs = _blocks(n, limit)
            _check(self._lib.blurrily_storage_find_batch_each_in(
                self._h, self._handles(scs), len(scs), which.ctypes.data if n else None, data, offsets.ctypes.data, n,
                limit, *ptrs))
            return out

    def find_batch_by_reference_each_in(self, scopes, which, references, limit):
        """``find_batch_by_reference`` with a scope per reference, as ``find_batch_each_in``.
        Returns (rows[n, limit, 3] uint32, counts[n] uint32, nb_trigrams[n] uint32)."""
        self._check_open()
        refs = self._refs(references)
        n = len(refs)
        which = self._which(which, n)
        with self._scopes_of(scopes) as scs:
            limit = _batch_limit(limit)
            out, ptrs = _blocks(n, limit, per_needle=1)
            _check(self._lib.blurrily_storage_find_references_each_in(
                self._h, self._handles(scs), len(scs), which.ctypes.data if n else None,
                refs.ctypes.data if n else None, n, limit, *ptrs))
            return out

    def join_within(self, scopes, limit):
        """The blocked self-join: every member of every scope searched among its own scope (``find_by_reference``
        restricted to it), in one GPU batch.  Returns (references[k] uint32, which[k] uint32: the scope of each,
        rows: k lists of [ref, matches, weight]) over the members the map holds, scope after scope."""
        self._check_open()
        with self._scopes_of(scopes) as scs:
            parts = [sc._refs if sc._refs is not None else np.zeros(0, np.uint32) for sc in scs]
            refs = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)
            which = np.repeat(np.arange(len(parts), dtype=np.uint32), [len(p) for p in parts])
            rows, counts, ntri = self.find_batch_by_reference_each_in(scs, which, refs, limit)
        held = np.nonzero(ntri)[0]
        return refs[held], which[held], _lists(rows[held], counts[held])

    def find_in(self, scope, needle, limit):
        """``find`` among the scope's members only (rows ``[ref, matches, weight]``); `limit` as find's."""
        self._check_open()
        c_limit = _find_limit(limit)
        if not isinstance(scope, Scope):
            with self.scope(scope) as one_shot:
                return RawMap.find_in(self, one_shot, needle, limit)
        sc = self._own(scope)
        rows = (_native.TrigramMatch * max(c_limit, 1))()
        res = _check(self._lib.blurrily_storage_find_in(self._h, sc._h, _as_bytes(needle), c_limit, rows))
        return [[rows[k].reference, rows[k].matches, rows[k].weight] for k in range(res)]

    # -- threshold find (no reference counterpart): every row at or above a bar of matches -------------------------
    @staticmethod
    def _bar(min_matches, min_permille):
        return _u32(min_matches, "min_matches"), _permille(min_permille)

    @staticmethod
    def _above(call, n):
        """One threshold call ``call(rows, cap, row_off)`` with room for a guessed number of rows (and for the exact
        number if that was too few).  Returns (rows[R, 3] uint32, row_off[n + 1] uint64)."""
        row_off = np.zeros(n + 1, dtype=np.uint64)
        rows = _call_growing(lambda rows, cap: call(rows, cap, row_off.ctypes.data), max(1024, 16 * n),
                             lambda: int(row_off[n]), row=(3,))
        return rows[:int(row_off[n])], row_off

    def find_batch_above_packed(self, packed, offsets, min_matches=0, min_permille=0):
        """Every row of each needle with at least its bar of matches, bar = max(1, min_matches, ceil(min_permille * T /
        1000)) for a needle of T distinct trigrams, in find's order.  Returns (rows[R, 3] uint32, row_off[n + 1]
        uint64): needle i's rows are rows[row_off[i]:row_off[i + 1]]."""
        self._check_open()
        mm, mp = self._bar(min_matches, min_permille)
        data, offsets, n = _needles(packed, offsets)
        return self._above(lambda rows, cap, off: self._lib.blurrily_storage_find_batch_above(
            self._h, data, offsets.ctypes.data, n, mm, mp, rows, cap, off), n)

    def find_above(self, needle, min_matches=0, min_permille=0):
        """``find_batch_above_packed`` for one needle: a list of ``[ref, matches, weight]``."""
        self._check_open()
        mm, mp = self._bar(min_matches, min_permille)
        s = _as_bytes(needle)
        total = C.c_uint64(0)
        rows = _call_growing(lambda rows, cap: self._lib.blurrily_storage_find_above(
            self._h, s, mm, mp, rows, cap, C.byref(total)), 1024, lambda: total.value, row=(3,))
        return rows[:total.value].tolist()

    def find_batch_by_reference_above(self, references, min_matches=0, min_permille=0):
        """``find_batch_above_packed`` for stored references (each among its own rows; none for a reference the map
        does not hold).  Returns (rows[R, 3] uint32, row_off[n + 1] uint64, nb_trigrams[n] uint32)."""
        self._check_open()
        mm, mp = self._bar(min_matches, min_permille)
        refs = self._refs(references)
        n = len(refs)
        ntri = np.zeros(n, dtype=np.uint32)
        rows, row_off = self._above(lambda rows, cap, off: self._lib.blurrily_storage_find_references_above(
            self._h, refs.ctypes.data if n else None, n, mm, mp, rows, cap, off, ntri.ctypes.data), n)
        return rows, row_off, ntri

    def join_above(self, references, min_matches=0, min_permille=0):
        """The threshold self-join: every held reference's rows at or above its bar, as arrays.  Returns (refs[k]
        uint32: the references the map holds, in the order given; row_off[k + 1] uint64; rows[R, 3] uint32)."""
        rows, row_off, ntri = self.find_batch_by_reference_above(references, min_matches, min_permille)
        refs = self._refs(references)
        held = np.nonzero(ntri)[0]
        counts = np.diff(row_off.astype(np.int64))[held]
        off = np.zeros(len(held) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(counts)
        if len(held) == len(refs):
            return refs, off, rows
        at = np.repeat(row_off[:-1].astype(np.int64)[held] - off[:-1].astype(np.int64), counts) + \
            np.arange(int(off[-1]), dtype=np.int64)
        return refs[held], off, rows[at]

    # -- similarity find (no reference counterpart): the best rows by trigram Jaccard similarity --------------------
    def find_batch_similar_packed(self, packed, offsets, limit, min_permille=0):
        """The best `limit` rows of each needle by trigram Jaccard similarity J = m / (T + R - m), at or above
        min_permille / 1000; J descending, then find's order.  Returns (rows[n, limit, 3] uint32, counts[n] uint32,
        row_ntri[n, limit] uint32: each row's R)."""
        self._check_open()
        mp = _permille(min_permille)
        data, offsets, n = _needles(packed, offsets)
        limit = _batch_limit(limit)
        out, ptrs = _blocks(n, limit, row_ntri=True)
        _check(self._lib.blurrily_storage_find_batch_similar(self._h, data, offsets.ctypes.data, n, limit, mp, *ptrs))
        return out

    def find_similar(self, needle, limit, min_permille=0):
        """``find_batch_similar_packed`` for one needle: a list of ``[ref, matches, weight, R]``; `limit` as find's."""
        self._check_open()
        mp = _permille(min_permille)
        c_limit = _find_limit(limit)
        rows = np.zeros((max(c_limit, 1), 3), dtype=np.uint32)
        ntri = np.zeros(max(c_limit, 1), dtype=np.uint32)
        res = _check(self._lib.blurrily_storage_find_similar(self._h, _as_bytes(needle), c_limit, mp, rows.ctypes.data,
                                                             ntri.ctypes.data))
        return [r + [t] for r, t in zip(rows[:res].tolist(), ntri[:res].tolist())]

    def find_batch_by_reference_similar(self, references, limit, min_permille=0):
        """``find_batch_similar_packed`` for stored references (each its own row at similarity 1; none for a reference
        the map does not hold).  Returns (rows[n, limit, 3] uint32, counts[n] uint32, row_ntri[n, limit] uint32,
        nb_trigrams[n] uint32)."""
        self._check_open()
        mp = _permille(min_permille)
        refs = self._refs(references)
        n = len(refs)
        limit = _batch_limit(limit)
        out, ptrs = _blocks(n, limit, row_ntri=True, per_needle=1)
        _check(self._lib.blurrily_storage_find_references_similar(self._h, refs.ctypes.data if n else None, n, limit,
                                                                  mp, *ptrs))
        return out

    # -- scoped similarity find: the similarity find among a scope's members -------------------
    def find_batch_similar_in_packed(self, scope, packed, offsets, limit, min_permille=0):
        """``find_batch_similar_packed`` among the scope's members only (a ``Scope`` or an iterable of references).
        Returns (rows[n, limit, 3] uint32, counts[n] uint32, row_ntri[n, limit] uint32)."""
        self._check_open()
        mp = _permille(min_permille)
        if not isinstance(scope, Scope):
            with self.scope(scope) as one_shot:
                return RawMap.find_batch_similar_in_packed(self, one_shot, packed, offsets, limit, mp)
        sc = self._own(scope)
        data, offsets, n = _needles(packed, offsets)
        limit = _batch_limit(limit)
        out, ptrs = _blocks(n, limit, row_ntri=True)
        _check(self._lib.blurrily_storage_find_batch_similar_in(self._h, sc._h, data, offsets.ctypes.data, n, limit, mp,
                                                                *ptrs))
        return out

    def find_similar_in(self, scope, needle, limit, min_permille=0):
        """``find_similar`` among the scope's members only: a list of ``[ref, matches, weight, R]``."""
        self._check_open()
        mp = _permille(min_permille)
        c_limit = _find_limit(limit)
        if not isinstance(scope, Scope):
            with self.scope(scope) as one_shot:
                return RawMap.find_similar_in(self, one_shot, needle, limit, mp)
        sc = self._own(scope)
        rows = np.zeros((max(c_limit, 1), 3), dtype=np.uint32)
        ntri = np.zeros(max(c_limit, 1), dtype=np.uint32)
        res = _check(self._lib.blurrily_storage_find_similar_in(self._h, sc._h, _as_bytes(needle), c_limit, mp,
                                                                rows.ctypes.data, ntri.ctypes.data))
        return [r + [t] for r, t in zip(rows[:res].tolist(), ntri[:res].tolist())]

    def find_batch_similar_each_in(self, scopes, which, packed, offsets, limit, min_permille=0):
        """``find_batch_similar_packed`` with a scope per needle: needle i among ``scopes[which[i]]`` only, or the whole
        map when ``which[i]`` is None.  Returns (rows[n, limit, 3] uint32, counts[n] uint32, row_ntri[n, limit])."""
        self._check_open()
        mp = _permille(min_permille)
        which = self._which(which, len(offsets) - 1)
        with self._scopes_of(scopes) as scs:
            limit = _batch_limit(limit)
            data, offsets, n = _needles(packed, offsets)
            out, ptrs = _blocks(n, limit, row_ntri=True)
            _check(self._lib.blurrily_storage_find_batch_similar_each_in(
                self._h, self._handles(scs), len(scs), which.ctypes.data if n else None, data, offsets.ctypes.data, n,
                limit, mp, *ptrs))
            return out

    def find_batch_by_reference_similar_each_in(self, scopes, which, references, limit, min_permille=0):
        """``find_batch_by_reference_similar`` with a scope per reference.  Returns (rows[n, limit, 3] uint32,
        counts[n] uint32, row_ntri[n, limit] uint32, nb_trigrams[n] uint32)."""
        self._check_open()
        mp = _permille(min_permille)
        refs = self._refs(references)
        n = len(refs)
        which = self._which(which, n)
        with self._scopes_of(scopes) as scs:
            limit = _batch_limit(limit)
            out, ptrs = _blocks(n, limit, row_ntri=True, per_needle=1)
            _check(self._lib.blurrily_storage_find_references_similar_each_in(
                self._h, self._handles(scs), len(scs), which.ctypes.data if n else None,
                refs.ctypes.data if n else None, n, limit, mp, *ptrs))
            return out

    def join_similar_within(self, scopes, limit, min_permille=0):
        """The blocked similarity self-join: every member of every scope ranked by similarity among its own scope, in
        one GPU batch.  Returns (references[k] uint32, which[k] uint32: the scope of each, rows: k lists of
        [ref, matches, weight, R]) over the members the map holds, scope after scope."""
        self._check_open()
        with self._scopes_of(scopes) as scs:
            parts = [sc._refs if sc._refs is not None else np.zeros(0, np.uint32) for sc in scs]
            refs = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)
            which = np.repeat(np.arange(len(parts), dtype=np.uint32), [len(p) for p in parts])
            rows, counts, rntri, ntri = self.find_batch_by_reference_similar_each_in(scs, which, refs, limit,
                                                                                     min_permille)
        held = np.nonzero(ntri)[0]
        return refs[held], which[held], _lists(rows[held], counts[held], rntri[held])

    # -- scoped threshold find: the threshold find among a scope's members -----------------------
    def find_batch_above_in_packed(self, scope, packed, offsets, min_matches=0, min_permille=0):
        """``find_batch_above_packed`` among the scope's members only (a ``Scope`` or an iterable of references).
        Returns (rows[R, 3] uint32, row_off[n + 1] uint64)."""
        self._check_open()
        mm, mp = self._bar(min_matches, min_permille)
        if not isinstance(scope, Scope):
            with self.scope(scope) as one_shot:
                return RawMap.find_batch_above_in_packed(self, one_shot, packed, offsets, mm, mp)
        sc = self._own(scope)
        data, offsets, n = _needles(packed, offsets)
        return self._above(lambda rows, cap, off: self._lib.blurrily_storage_find_batch_above_in(
            self._h, sc._h, data, offsets.ctypes.data, n, mm, mp, rows, cap, off), n)

    def find_above_in(self, scope, needle, min_matches=0, min_permille=0):
        """``find_above`` among the scope's members only: a list of ``[ref, matches, weight]``."""
        self._check_open()
        mm, mp = self._bar(min_matches, min_permille)
        if not isinstance(scope, Scope):
            with self.scope(scope) as one_shot:
                return RawMap.find_above_in(self, one_shot, needle, mm, mp)
        sc = self._own(scope)
        s = _as_bytes(needle)
        total = C.c_uint64(0)
        rows = _call_growing(lambda rows, cap: self._lib.blurrily_storage_find_above_in(
            self._h, sc._h, s, mm, mp, rows, cap, C.byref(total)), 1024, lambda: total.value, row=(3,))
        return rows[:total.value].tolist()

    def find_batch_above_each_in(self, scopes, which, packed, offsets, min_matches=0, min_permille=0):
        """``find_batch_above_packed`` with a scope per needle: needle i among ``scopes[which[i]]`` only, or the whole
        map when ``which[i]`` is None.  Returns (rows[R, 3] uint32, row_off[n + 1] uint64)."""
        self._check_open()
        mm, mp = self._bar(min_matches, min_permille)
        which = self._which(which, len(offsets) - 1)
        with self._scopes_of(scopes) as scs:
            data, offsets, n = _needles(packed, offsets)
            return self._above(lambda rows, cap, off: self._lib.blurrily_storage_find_batch_above_each_in(
                self._h, self._handles(scs), len(scs), which.ctypes.data if n else None, data, offsets.ctypes.data, n,
                mm, mp, rows, cap, off), n)

    def find_batch_by_reference_above_each_in(self, scopes, which, references, min_matches=0, min_permille=0):
        """``find_batch_by_reference_above`` with a scope per reference.  Returns (rows[R, 3] uint32,
        row_off[n + 1] uint64, nb_trigrams[n] uint32)."""
        self._check_open()
        mm, mp = self._bar(min_matches, min_permille)
        refs = self._refs(references)
        n = len(refs)
        which = self._which(which, n)
        ntri = np.zeros(n, dtype=np.uint32)
        with self._scopes_of(scopes) as scs:
            rows, row_off = self._above(lambda rows, cap, off: self._lib.blurrily_storage_find_references_above_each_in(
                self._h, self._handles(scs), len(scs), which.ctypes.data if n else None,
                refs.ctypes.data if n else None, n, mm, mp, rows, cap, off, ntri.ctypes.data), n)
        return rows, row_off, ntri

    def join_above_within(self, scopes, min_matches=0, min_permille=0):
        """The blocked threshold self-join: every member of every scope with all the members of its own scope at or above
        its bar, in one GPU batch.  Returns (refs[k] uint32, which[k] uint32: the scope of each, row_off[k + 1] uint64,
        rows[R, 3] uint32) over the members the map holds, scope after scope."""
        self._check_open()
        with self._scopes_of(scopes) as scs:
            parts = [sc._refs if sc._refs is not None else np.zeros(0, np.uint32) for sc in scs]
            refs = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)
            which = np.repeat(np.arange(len(parts), dtype=np.uint32), [len(p) for p in parts])
            rows, row_off, ntri = self.find_batch_by_reference_above_each_in(scs, which, refs, min_matches, min_permille)
        held = np.nonzero(ntri)[0]                       # (a reference the map does not hold has no rows: nothing to cut)
        off = np.zeros(len(held) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(np.diff(row_off.astype(np.int64))[held])
        return refs[held], which[held], off, rows

    # -- clusters (no reference counterpart): connected components of the similarity self-join ----------------------
    def cluster(self, references, min_permille):
        """Single-linkage clusters of the stored references under "J >= min_permille / 1000" (blurrily_storage_cluster).
        Returns (labels[n] uint32: the smallest reference of each reference's component, ``_native.NO_CLUSTER`` for
        one the map does not hold; the number of components; the number of edges, each pair once)."""
        self._check_open()
        mp = _permille(min_permille)
        refs = self._refs(references)
        n = len(refs)
        labels = np.zeros(n, dtype=np.uint32)
        n_clusters, n_edges = C.c_uint32(0), C.c_uint64(0)
        _check(self._lib.blurrily_storage_cluster(self._h, refs.ctypes.data if n else None, n, mp,
                                                  labels.ctypes.data if n else None, C.byref(n_clusters),
                                                  C.byref(n_edges)))
        return labels, int(n_clusters.value), int(n_edges.value)

    def cluster_levels(self, references, floors):
        """``cluster`` at several floors (strictly ascending, at most ``_native.CLUSTER_MAX_LEVELS``) from one sweep of
        the device (blurrily_storage_cluster_levels).  Returns (labels[K, n] uint32, n_clusters[K] int64, n_edges[K]
        int64): row k is what ``cluster(references, floors[k])`` returns."""
        self._check_open()
        fl = _floors(floors)
        refs = self._refs(references)
        n, k = len(refs), len(fl)
        labels = np.zeros((k, n), dtype=np.uint32)
        n_clusters, n_edges = np.zeros(k, dtype=np.uint32), np.zeros(k, dtype=np.uint64)
        _check(self._lib.blurrily_storage_cluster_levels(self._h, refs.ctypes.data if n else None, n, fl.ctypes.data, k,
                                                         labels.ctypes.data if n else None, n_clusters.ctypes.data,
                                                         n_edges.ctypes.data))
        return labels, n_clusters.astype(np.int64), n_edges.astype(np.int64)

    def cluster_profile(self, references, floors):
        """What a caller picks a floor by: per floor ``{floor, n_clusters, n_edges, largest, singletons}`` -- the
        components, the edges, the nodes of the largest component and the components of one node -- from one
        ``cluster_levels`` call and numpy over its labels."""
        floors = list(floors)
        refs = np.unique(self._refs(references))               # (a reference listed twice is one node)
        labels, n_clusters, n_edges = self.cluster_levels(refs, floors)
        profile = []
        for k, floor in enumerate(floors):
            _, sizes = np.unique(labels[k][labels[k] != _native.NO_CLUSTER], return_counts=True)
            profile.append({"floor": int(floor), "n_clusters": int(n_clusters[k]), "n_edges": int(n_edges[k]),
                            "largest": int(sizes.max()) if len(sizes) else 0, "singletons": int((sizes == 1).sum())})
        return profile

    def cluster_centres(self, references, min_permille, attached=True):
        """``cluster`` with what tells a tight group from a chain (blurrily_storage_cluster_centres).  Returns (labels[n],
        degrees[n] uint32: each reference's edges; centres[n] uint32: the reference with the most edges in its
        component, the smallest among equals, ``_native.NO_CLUSTER`` for one the map does not hold; attached[n] uint8:
        1 for a centre and for a reference that shares an edge with its centre -- None with ``attached=False``, which
        spares the device its second sweep; the number of components; the number of edges)."""
        self._check_open()
        mp = _permille(min_permille)
        refs = self._refs(references)
        n = len(refs)
        labels, degrees, centres = (np.zeros(n, dtype=np.uint32) for _ in range(3))
        att = np.zeros(n, dtype=np.uint8) if attached else None
        n_clusters, n_edges = C.c_uint32(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data if n else None
        _check(self._lib.blurrily_storage_cluster_centres(self._h, ptr(refs), n, mp, ptr(labels), ptr(degrees),
                                                          ptr(centres), ptr(att) if attached else None,
                                                          C.byref(n_clusters), C.byref(n_edges)))
        return labels, degrees, centres, att, int(n_clusters.value), int(n_edges.value)

    def cluster_shapes(self, references, min_permille):
        """The components of two or more references, ordered by label: ``{label, size, edges, centre, attached, star}``
        each -- its nodes, its edges, its centre, how many of its nodes are the centre or share an edge with it, and
        whether all do (a star: every member is directly similar to the centre; otherwise a chain to look at again).
        Numpy over one ``cluster_centres`` call."""
        refs = np.unique(self._refs(references))               # (a reference listed twice is one node)
        labels, degrees, centres, att, _, _ = self.cluster_centres(refs, min_permille)
        held = labels != _native.NO_CLUSTER
        labels, degrees, centres, att = labels[held], degrees[held], centres[held], att[held]
        uniq, first, which, sizes = np.unique(labels, return_index=True, return_inverse=True, return_counts=True)
        edges = np.bincount(which, weights=degrees.astype(np.float64), minlength=len(uniq)).astype(np.int64) // 2
        marked = np.bincount(which, weights=att.astype(np.float64), minlength=len(uniq)).astype(np.int64)
        return [{"label": int(uniq[k]), "size": int(sizes[k]), "edges": int(edges[k]), "centre": int(centres[first[k]]),
                 "attached": int(marked[k]), "star": bool(marked[k] == sizes[k])}
                for k in np.nonzero(sizes >= 2)[0].tolist()]

    def duplicates(self, references, min_permille):
        """The clusters of two or more references: a list of lists of references, each ascending, ordered by label."""
        refs = self._refs(references)
        labels, _, _ = self.cluster(refs, min_permille)
        refs, at = np.unique(refs, return_index=True)
        labels = labels[at]
        held = labels != _native.NO_CLUSTER
        refs, labels = refs[held], labels[held]
        order = np.argsort(labels, kind="stable")               # (refs ascending within a label)
        _, starts, sizes = np.unique(labels[order], return_index=True, return_counts=True)
        return [refs[order[s:s + k]].tolist() for s, k in zip(starts.tolist(), sizes.tolist()) if k >= 2]

    def cluster_cores(self, references, min_permille, min_degree):
        """Density-based clusters over ``cluster``'s edges (blurrily_storage_cluster_cores): a reference with at least
        ``min_degree`` edges is a core, only edges between cores unite, a reference that is no core joins the cluster
        of its core neighbour with the most edges (the smallest among equals) as a border, or is noise.  Returns
        (labels[n] uint32: the smallest core of the cluster, a noise reference itself, ``_native.NO_CLUSTER`` for one
        the map does not hold; degrees[n] uint32; kinds[n] uint8: ``_native.KIND_NONE``, ``KIND_NOISE``,
        ``KIND_BORDER``, ``KIND_CORE``; the number of clusters; the number of edges; the edges between cores)."""
        self._check_open()
        mp = _permille(min_permille)
        md = _u32(min_degree, "min_degree")
        refs = self._refs(references)
        n = len(refs)
        labels, degrees = (np.zeros(n, dtype=np.uint32) for _ in range(2))
        kinds = np.zeros(n, dtype=np.uint8)
        n_clusters, n_edges, n_core_edges = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data if n else None
        _check(self._lib.blurrily_storage_cluster_cores(self._h, ptr(refs), n, mp, md, ptr(labels), ptr(degrees),
                                                        ptr(kinds), C.byref(n_clusters), C.byref(n_edges),
                                                        C.byref(n_core_edges)))
        return labels, degrees, kinds, int(n_clusters.value), int(n_edges.value), int(n_core_edges.value)

    def dense_duplicates(self, references, min_permille, min_degree):
        """The clusters of ``cluster_cores``: a list of lists of references, cores and borders, each ascending,
        ordered by label; noise is left out.  Numpy over one ``cluster_cores`` call."""
        refs = np.unique(self._refs(references))               # (a reference listed twice is one node)
        labels, _, kinds, _, _, _ = self.cluster_cores(refs, min_permille, min_degree)
        member = kinds >= _native.KIND_BORDER
        refs, labels = refs[member], labels[member]
        order = np.argsort(labels, kind="stable")               # (refs ascending within a label)
        _, starts, sizes = np.unique(labels[order], return_index=True, return_counts=True)
        return [refs[order[s:s + k]].tolist() for s, k in zip(starts.tolist(), sizes.tolist())]

    def cluster_extend(self, old_refs, old_labels, new_refs, min_permille):
        """The clusters of ``old_refs`` and ``new_refs`` together, from the labels the caller holds for the old ones
        (blurrily_storage_cluster_extend): only the new references sweep the map, the old ones start from
        ``old_labels``.  With ``old_labels`` from ``cluster(old_refs, min_permille)`` on the map as it is now and the
        lists disjoint, the result is ``cluster``'s over both lists; a group that lost a member to a delete is
        re-clustered on its own first (``cluster`` over its remaining members).  Returns (labels_old[n_old] uint32,
        labels_new[n_new] uint32, the number of components, the number of edges with a new end, each once)."""
        self._check_open()
        mp = _permille(min_permille)
        old, new = self._refs(old_refs), self._refs(new_refs)
        seeds = self._refs(old_labels)
        if len(seeds) != len(old):
            raise ValueError(f"{len(seeds)} old labels for {len(old)} old references")
        labels_old, labels_new = np.zeros(len(old), dtype=np.uint32), np.zeros(len(new), dtype=np.uint32)
        n_clusters, n_edges = C.c_uint32(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data if len(a) else None
        _check(self._lib.blurrily_storage_cluster_extend(self._h, ptr(old), ptr(seeds), len(old), ptr(new), len(new), mp,
                                                         ptr(labels_old), ptr(labels_new), C.byref(n_clusters),
                                                         C.byref(n_edges)))
        return labels_old, labels_new, int(n_clusters.value), int(n_edges.value)

    def cluster_changes(self, old_refs, old_labels, labels_old):
        """What a database update after ``cluster_extend`` needs: (the old references whose label moved, their new
        labels), in the list's order.  Numpy only."""
        old, was, now = self._refs(old_refs), self._refs(old_labels), self._refs(labels_old)
        if not len(old) == len(was) == len(now):
            raise ValueError("old_refs, old_labels and labels_old differ in length")
        moved = was != now
        return old[moved], now[moved]

    def cluster_within(self, references, blocks, min_permille):
        """``cluster`` within blocks (blurrily_storage_cluster_within): ``blocks[i]`` is a 32-bit key for
        ``references[i]``, and only references under one key are ever joined.  One call serves all blocks.  Returns
        (labels[n] uint32, the number of components over all blocks, the number of within-block edges): what one
        ``cluster`` call per block gives, the counts summed."""
        self._check_open()
        mp = _permille(min_permille)
        refs, keys = self._refs(references), self._refs(blocks)
        if len(keys) != len(refs):
            raise ValueError(f"{len(keys)} block keys for {len(refs)} references")
        n = len(refs)
        labels = np.zeros(n, dtype=np.uint32)
        n_clusters, n_edges = C.c_uint32(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data if n else None
        _check(self._lib.blurrily_storage_cluster_within(self._h, ptr(refs), ptr(keys), n, mp, ptr(labels),
                                                         C.byref(n_clusters), C.byref(n_edges)))
        return labels, int(n_clusters.value), int(n_edges.value)

    def duplicates_within(self, references, blocks, min_permille):
        """The within-block clusters of two or more references, as ``duplicates`` gives them: a list of lists of
        references, each ascending, ordered by label."""
        refs = self._refs(references)
        labels, _, _ = self.cluster_within(refs, blocks, min_permille)
        refs, at = np.unique(refs, return_index=True)
        labels = labels[at]
        held = labels != _native.NO_CLUSTER
        refs, labels = refs[held], labels[held]
        order = np.argsort(labels, kind="stable")               # (refs ascending within a label)
        _, starts, sizes = np.unique(labels[order], return_index=True, return_counts=True)
        return [refs[order[s:s + k]].tolist() for s, k in zip(starts.tolist(), sizes.tolist()) if k >= 2]

    def cluster_cores_within(self, references, blocks, min_permille, min_degree):
        """``cluster_cores`` within blocks (blurrily_storage_cluster_cores_within): ``blocks[i]`` is a 32-bit key for
        ``references[i]``, an edge needs both ends under one key, and a degree counts those edges only, so a core, a
        border's anchor and a cluster never reach across a key.  One call serves all blocks.  Returns (labels[n]
        uint32, degrees[n] uint32, kinds[n] uint8, the number of clusters, the number of within-block edges, the edges
        between cores) as ``cluster_cores`` gives them: what one ``cluster_cores`` call per block gives, put back in
        place, the counts summed."""
        self._check_open()
        mp = _permille(min_permille)
        md = _u32(min_degree, "min_degree")
        refs, keys = self._refs(references), self._refs(blocks)
        if len(keys) != len(refs):
            raise ValueError(f"{len(keys)} block keys for {len(refs)} references")
        n = len(refs)
        labels, degrees = (np.zeros(n, dtype=np.uint32) for _ in range(2))
        kinds = np.zeros(n, dtype=np.uint8)
        n_clusters, n_edges, n_core_edges = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data if n else None
        _check(self._lib.blurrily_storage_cluster_cores_within(self._h, ptr(refs), ptr(keys), n, mp, md, ptr(labels),
                                                               ptr(degrees), ptr(kinds), C.byref(n_clusters),
                                                               C.byref(n_edges), C.byref(n_core_edges)))
        return labels, degrees, kinds, int(n_clusters.value), int(n_edges.value), int(n_core_edges.value)

    def dense_duplicates_within(self, references, blocks, min_permille, min_degree):
        """The clusters of ``cluster_cores_within``, as ``dense_duplicates`` gives them: a list of lists of references,
        cores and borders, each ascending, ordered by label; noise is left out.  Numpy over one call."""
        refs = self._refs(references)
        labels, _, kinds, _, _, _ = self.cluster_cores_within(refs, blocks, min_permille, min_degree)
        refs, at = np.unique(refs, return_index=True)           # (a reference listed twice is one node)
        labels, kinds = labels[at], kinds[at]
        member = kinds >= _native.KIND_BORDER
        refs, labels = refs[member], labels[member]
        order = np.argsort(labels, kind="stable")               # (refs ascending within a label)
        _, starts, sizes = np.unique(labels[order], return_index=True, return_counts=True)
        return [refs[order[s:s + k]].tolist() for s, k in zip(starts.tolist(), sizes.tolist())]

    def cluster_tree(self, references, min_permille):
        """The single-linkage dendrogram of ``cluster`` at per-mille resolution (blurrily_storage_cluster_tree): the
        maximum spanning forest of the edges at or above ``min_permille``, an edge's height being its similarity in
        whole per mille, rounded down.  Returns (labels[n] uint32, n_clusters and n_edges as ``cluster`` gives them at
        ``min_permille``, and between them merges[k, 3] uint32: rows ``[a, b, permille]`` with a < b, sorted by height
        descending, then a, then b; k is the nodes minus the components) as ``(labels, merges, n_clusters, n_edges)``.
        ``cut_tree`` gives the labels at any higher floor without another call."""
        self._check_open()
        mp = _permille(min_permille)
        refs = self._refs(references)
        n = len(refs)
        labels = np.zeros(n, dtype=np.uint32)
        merges = np.zeros((n, 3), dtype=np.uint32)
        n_merges, n_clusters, n_edges = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data if n else None
        _check(self._lib.blurrily_storage_cluster_tree(self._h, ptr(refs), n, mp, ptr(labels), ptr(merges),
                                                       C.byref(n_merges), C.byref(n_clusters), C.byref(n_edges)))
        return labels, merges[:int(n_merges.value)].copy(), int(n_clusters.value), int(n_edges.value)

    @staticmethod
    def cut_tree(references, labels, merges, floor, min_permille=0):
        """The labels ``cluster(references, floor)`` would give, from a ``cluster_tree`` result alone: union-find in
        numpy over the merges with ``permille >= floor``.  ``labels`` are the tree's (they tell which references the
        map holds), ``min_permille`` the floor the tree was made at: the tree knows no edge below it, so a cut there
        is refused (ValueError), as is one above 1000.  Needs no map and no GPU."""
        floor, low = _permille(floor), _permille(min_permille)
        if floor < low:
            raise ValueError(f"floor {floor} below the tree's {low}: its edges are not in the tree")
        refs, labels = np.asarray(references, dtype=np.uint32), np.asarray(labels, dtype=np.uint32)
        merges = np.asarray(merges, dtype=np.uint32).reshape(-1, 3)
        if refs.ndim != 1 or labels.shape != refs.shape:
            raise ValueError("references and labels must be one-dimensional and of one length")
        held = labels != _native.NO_CLUSTER
        nodes = np.unique(refs[held])                             # ascending: the lowest index is the lowest reference
        kept = merges[merges[:, 2] >= floor]
        a, b = np.searchsorted(nodes, kept[:, 0]), np.searchsorted(nodes, kept[:, 1])
        if len(kept) and (max(a.max(), b.max()) >= len(nodes) or (nodes[a] != kept[:, 0]).any() or (nodes[b] != kept[:, 1]).any()):
            raise ValueError("a merge names a reference that the labels do not hold")
        label = np.arange(len(nodes), dtype=np.int64)
        while len(kept):                                          # lowest-label propagation with pointer jumping
            low_of = np.minimum(label[a], label[b])
            nxt = label.copy()
            np.minimum.at(nxt, a, low_of)
            np.minimum.at(nxt, b, low_of)
            nxt = nxt[nxt]
            if np.array_equal(nxt, label):
                break
            label = nxt
        out = np.full(len(refs), _native.NO_CLUSTER, dtype=np.uint32)
        out[held] = nodes[label[np.searchsorted(nodes, refs[held])]]
        return out

    @staticmethod
    def _records(merges, what):
        """Tree records as a contiguous uint32[k, 3]; values that do not fit are refused, as ``_refs`` refuses them."""
        rows = np.asarray(merges)
        if rows.size == 0:
            return np.zeros((0, 3), dtype=np.uint32)
        if rows.ndim != 2 or rows.shape[1] != 3:
            raise ValueError(f"{what} must be rows of [a, b, permille]")
        if rows.dtype != np.uint32:
            rows = np.array([_u32(v, what) for v in rows.reshape(-1).tolist()], dtype=np.uint32).reshape(-1, 3)
        return np.ascontiguousarray(rows)

    def cluster_tree_extend(self, old_refs, old_merges, new_refs, min_permille):
        """The tree of ``old_refs`` and ``new_refs`` together, from the records the caller holds for the old ones
        (blurrily_storage_cluster_tree_extend): only the new references sweep the map, the old ones are spoken for by
        ``old_merges``.  With ``old_merges`` from ``cluster_tree(old_refs, f)`` for some ``f <= min_permille`` on old
        rows unchanged since, the lists disjoint and every reference held, the result is ``cluster_tree``'s over both
        lists at ``min_permille``; a component that lost a member to a delete is re-treed on its own first.  Returns
        ``(labels_old, labels_new, merges, n_clusters, n_edges)``: merges[k, 3] uint32 as ``cluster_tree`` gives them,
        n_edges the edges with a new end, each once.  ``cut_tree`` and ``merge_profile`` take the records as they
        are; ``tree_changes`` tells which of the caller's to delete and to insert."""
        self._check_open()
        mp = _permille(min_permille)
        old, new = self._refs(old_refs), self._refs(new_refs)
        records = self._records(old_merges, "old_merges")
        if len(records) > len(old):
            raise ValueError(f"{len(records)} old records for {len(old)} old references: a forest has fewer")
        if len(records) and ((records[:, 0] >= records[:, 1]).any() or (records[:, 2] > 1000).any()):
            raise ValueError("an old record needs a < b and permille <= 1000")
        n = len(old) + len(new)
        labels_old, labels_new = np.zeros(len(old), dtype=np.uint32), np.zeros(len(new), dtype=np.uint32)
        merges = np.zeros((n, 3), dtype=np.uint32)
        n_merges, n_clusters, n_edges = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data if len(a) else None
        _check(self._lib.blurrily_storage_cluster_tree_extend(self._h, ptr(old), len(old), ptr(records), len(records),
                                                              ptr(new), len(new), mp, ptr(labels_old), ptr(labels_new),
                                                              ptr(merges), C.byref(n_merges), C.byref(n_clusters),
                                                              C.byref(n_edges)))
        return labels_old, labels_new, merges[:int(n_merges.value)].copy(), int(n_clusters.value), int(n_edges.value)

    @staticmethod
    def tree_changes(old_merges, merges):
        """What a database update after ``cluster_tree_extend`` needs: ``(removed, added)``, uint32[r, 3] and
        uint32[s, 3] -- the records of ``old_merges`` that ``merges`` no longer holds and the records of ``merges``
        that ``old_merges`` did not hold, whole rows compared, each in the tree's order (height descending, then a,
        then b).  Needs no map and no GPU."""
        was, now = RawMap._records(old_merges, "old_merges"), RawMap._records(merges, "merges")
        # equal rows get one number: whole records are compared, the height included
        _, number = np.unique(np.concatenate([was, now]), axis=0, return_inverse=True)
        number = number.reshape(-1)
        gone = ~np.isin(number[:len(was)], number[len(was):])
        come = ~np.isin(number[len(was):], number[:len(was)])

        def ordered(rows):
            return rows[np.lexsort((rows[:, 1], rows[:, 0], 1000 - rows[:, 2].astype(np.int64)))]

        return ordered(was[gone]), ordered(now[come])

    def cluster_core_tree(self, references, min_permille, min_degree):
        """The dendrogram of ``cluster_cores``' cores at every floor from ``min_permille`` up
        (blurrily_storage_cluster_core_tree).  A node's core height is the ``min_degree``-th largest height among its
        edges, and an edge between two nodes that have one joins them at the least of its own height and theirs.
        Returns ``(labels, core_permille, merges, n_clusters, n_edges, n_core_edges)``: labels[n] and core_permille[n]
        uint32 (``_native.NO_CORE`` for a reference the map does not hold or a node of fewer than ``min_degree`` edges),
        merges[k, 3] uint32 rows ``[a, b, permille]`` as ``cluster_tree`` gives them, and ``cluster_cores``' three
        counts at ``(min_permille, min_degree)``.  ``cut_core_tree`` gives the cores and their labels at any higher
        floor without another call."""
        self._check_open()
        mp = _permille(min_permille)
        md = _u32(min_degree, "min_degree")
        refs = self._refs(references)
        n = len(refs)
        labels, core_permille = (np.zeros(n, dtype=np.uint32) for _ in range(2))
        merges = np.zeros((n, 3), dtype=np.uint32)
        n_merges, n_clusters, n_edges, n_core_edges = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data if n else None
        _check(self._lib.blurrily_storage_cluster_core_tree(self._h, ptr(refs), n, mp, md, ptr(labels),
                                                            ptr(core_permille), ptr(merges), C.byref(n_merges),
                                                            C.byref(n_clusters), C.byref(n_edges),
                                                            C.byref(n_core_edges)))
        return (labels, core_permille, merges[:int(n_merges.value)].copy(), int(n_clusters.value), int(n_edges.value),
                int(n_core_edges.value))

    @staticmethod
    def cut_core_tree(references, labels, core_permille, merges, floor, min_permille=0):
        """What ``cluster_cores(references, floor, min_degree)`` says of the cores, from a ``cluster_core_tree`` result
        alone: ``(labels_at_floor, is_core)``.  A reference is a core at ``floor`` when its core height is at least
        ``floor``; the cores are labelled by the smallest reference of their component under the merges with
        ``permille >= floor``, every other node by its own reference (its anchor needs its degree at that floor,
        which the tree does not hold), and a reference that is no node keeps ``NO_CLUSTER``.  ``min_permille`` is the
        floor the tree was made at; a cut below it or above 1000 is refused (ValueError).  Needs no map and no GPU."""
        core = np.asarray(core_permille, dtype=np.uint32)
        refs = np.asarray(references, dtype=np.uint32)
        if core.shape != refs.shape:
            raise ValueError("references and core_permille must be of one length")
        cut = RawMap.cut_tree(refs, labels, merges, floor, min_permille)   # (checks the rest)
        is_core = (core != _native.NO_CORE) & (core >= _permille(floor)) & (cut != _native.NO_CLUSTER)
        merges = np.asarray(merges, dtype=np.uint32).reshape(-1, 3)
        kept = merges[merges[:, 2] >= floor]
        if not np.isin(kept[:, :2], refs[is_core]).all():
            raise ValueError("a merge at this floor names a reference that is no core there")
        held = cut != _native.NO_CLUSTER
        return np.where(is_core | ~held, cut, refs), is_core

    def cluster_tree_within(self, references, blocks, min_permille):
        """``cluster_tree`` within blocks (blurrily_storage_cluster_tree_within): ``blocks[i]`` is a 32-bit key for
        ``references[i]``, and only references under one key are ever joined.  One call serves all blocks.  Returns
        ``(labels, merges, n_clusters, n_edges)``: labels[n] uint32, n_clusters and n_edges as ``cluster_within`` gives
        them at ``min_permille``, and merges[k, 3] uint32 as ``cluster_tree`` gives them -- what one ``cluster_tree``
        call per block gives, the records merged into one list in the tree's order.  ``cut_tree`` gives
        ``cluster_within``'s labels at any higher floor without another call, ``merge_profile`` takes the records as
        they are, and ``tree_by_block`` splits them by key."""
        self._check_open()
        mp = _permille(min_permille)
        refs, keys = self._refs(references), self._refs(blocks)
        if len(keys) != len(refs):
            raise ValueError(f"{len(keys)} block keys for {len(refs)} references")
        n = len(refs)
        labels = np.zeros(n, dtype=np.uint32)
        merges = np.zeros((n, 3), dtype=np.uint32)
        n_merges, n_clusters, n_edges = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        ptr = lambda a: a.ctypes.data if n else None
        _check(self._lib.blurrily_storage_cluster_tree_within(self._h, ptr(refs), ptr(keys), n, mp, ptr(labels),
                                                              ptr(merges), C.byref(n_merges), C.byref(n_clusters),
                                                              C.byref(n_edges)))
        return labels, merges[:int(n_merges.value)].copy(), int(n_clusters.value), int(n_edges.value)

    @staticmethod
    def tree_by_block(merges, references, blocks):
        """A ``cluster_tree_within`` result split by block, for the caller who stores a tree per block:
        ``{key: merges rows}``, uint32[k, 3] each, in the tree's order (the order the records come in).  Only keys with
        a record appear.  ValueError for a record whose ends carry two keys or name a reference that is not listed.
        Needs no map and no GPU."""
        rows = RawMap._records(merges, "merges")
        refs, keys = np.asarray(references, dtype=np.uint32), np.asarray(blocks, dtype=np.uint32)
        if refs.ndim != 1 or keys.shape != refs.shape:
            raise ValueError("references and blocks must be one-dimensional and of one length")
        if not len(rows):
            return {}
        listed, at = np.unique(refs, return_index=True)
        ends = np.searchsorted(listed, rows[:, :2])
        if len(listed) == 0 or (listed[np.minimum(ends, len(listed) - 1)] != rows[:, :2]).any():
            raise ValueError("a record names a reference that is not listed")
        key = keys[at][ends]
        if (key[:, 0] != key[:, 1]).any():
            raise ValueError("a record joins references under two keys")
        return {int(k): rows[key[:, 0] == k] for k in np.unique(key[:, 0]).tolist()}

    def _cluster_edges_call(self, references, min_permille, blocks):
        """What the two edge methods share: ``(call(rows, cap, n_edges), n)`` for the unblocked symbol
        (``blocks`` None) or the blocked one."""
        self._check_open()
        mp = _permille(min_permille)
        refs = self._refs(references)
        n = len(refs)
        ptr = lambda a: a.ctypes.data if n else None
        if blocks is None:
            return (lambda rows, cap, n_edges: self._lib.blurrily_storage_cluster_edges(
                self._h, ptr(refs), n, mp, rows, cap, n_edges)), n
        keys = self._refs(blocks)
        if len(keys) != n:
            raise ValueError(f"{len(keys)} block keys for {n} references")
        return (lambda rows, cap, n_edges: self._lib.blurrily_storage_cluster_edges_within(
            self._h, ptr(refs), ptr(keys), n, mp, rows, cap, n_edges)), n

    def cluster_edges(self, references, min_permille, blocks=None, capacity=None):
        """The edges of ``cluster``'s graph themselves (blurrily_storage_cluster_edges), or with ``blocks`` of
        ``cluster_within``'s (blurrily_storage_cluster_edges_within): edges[E, 3] uint32, one row ``[a, b, permille]``
        per pair of listed references at or above ``min_permille``, a < b, permille the similarity in whole per mille
        rounded down, sorted as ``cluster_tree``'s merges are (height descending, then a, then b).  E is ``cluster``'s
        n_edges.  The first call has room for ``capacity`` records (default ``max(1024, 8 n)``); if there are more, one
        more call is made with the room the first reported.  OSError EOVERFLOW when the edges outnumber option
        "cluster_edges_max": raise the floor, block or split the list.  ``tree_by_block``, ``cut_tree`` (with
        ``cluster``'s labels) and ``merge_profile`` take the records as they are; ``adjacency`` turns them into
        neighbour lists."""
        call, n = self._cluster_edges_call(references, min_permille, blocks)
        total = C.c_uint64(0)
        first = max(1024, 8 * n) if capacity is None else int(capacity)
        if not 0 <= first < 1 << 64:
            raise OverflowError(f"capacity {capacity!r} out of range of uint64_t")
        rows = _call_growing(lambda rows, cap: call(rows, cap, C.byref(total)), first, lambda: int(total.value), row=(3,))
        return rows[:int(total.value)]

    def cluster_edge_count(self, references, min_permille, blocks=None):
        """How many records ``cluster_edges`` would return, without sorting or fetching them: no buffer is handed."""
        call, _ = self._cluster_edges_call(references, min_permille, blocks)
        total = C.c_uint64(0)
        _check(call(None, 0, C.byref(total)))
        return int(total.value)

    def _cluster_edges_two_call(self, symbol, first, second, min_permille):
        """What the extend and between methods share: ``(call(rows, cap, n_edges), n)`` over two lists."""
        self._check_open()
        mp = _permille(min_permille)
        one, two = self._refs(first), self._refs(second)
        ptr = lambda a: a.ctypes.data if len(a) else None
        fn = getattr(self._lib, symbol)
        return (lambda rows, cap, n_edges: fn(self._h, ptr(one), len(one), ptr(two), len(two), mp, rows, cap,
                                              n_edges)), len(one) + len(two)

    def _cluster_edges_two(self, symbol, first, second, min_permille, capacity):
        call, n = self._cluster_edges_two_call(symbol, first, second, min_permille)
        total = C.c_uint64(0)
        start = max(1024, 8 * n) if capacity is None else int(capacity)
        if not 0 <= start < 1 << 64:
            raise OverflowError(f"capacity {capacity!r} out of range of uint64_t")
        rows = _call_growing(lambda rows, cap: call(rows, cap, C.byref(total)), start, lambda: int(total.value), row=(3,))
        return rows[:int(total.value)]

    def _cluster_edge_count_two(self, symbol, first, second, min_permille):
        call, _ = self._cluster_edges_two_call(symbol, first, second, min_permille)
        total = C.c_uint64(0)
        _check(call(None, 0, C.byref(total)))
        return int(total.value)

    def cluster_edges_extend(self, old_refs, new_refs, min_permille, capacity=None):
        """The ``cluster_edges`` records over both lists that have at least one end in ``new_refs``, each once
        (blurrily_storage_cluster_edges_extend): only the new references sweep the map.  A reference both lists name
        is new.  ``merge_edges(cluster_edges(old minus new), this)`` is ``cluster_edges(old and new)`` byte for byte:
        how an edge list is kept current after a put.  E is ``cluster_extend``'s n_edges.  Records, order, ``capacity``
        and EOVERFLOW are ``cluster_edges``'; ``adjacency``, ``cut_tree`` and ``merge_profile`` take the records as
        they are."""
        return self._cluster_edges_two("blurrily_storage_cluster_edges_extend", old_refs, new_refs, min_permille, capacity)

    def cluster_edge_count_extend(self, old_refs, new_refs, min_permille):
        """How many records ``cluster_edges_extend`` would return: no buffer is handed, nothing is sorted."""
        return self._cluster_edge_count_two("blurrily_storage_cluster_edges_extend", old_refs, new_refs, min_permille)

    def cluster_edges_between(self, left, right, min_permille, capacity=None):
        """Record linkage: the ``cluster_edges`` records with exactly one end in ``left`` and one in ``right``
        (blurrily_storage_cluster_edges_between).  A reference both lists name is on the right only.  The side with
        fewer distinct references sweeps the map, whichever way round the lists are given, and for disjoint lists
        both ways round give identical bytes.  ``cluster_edges_extend(l, r)`` is this merged with ``cluster_edges(r)``.
        Records, order, ``capacity`` and EOVERFLOW are ``cluster_edges``'.  ``adjacency(records, left + right)`` takes
        them as they are: a left row's first neighbour is its best link (the records come best first); ``cut_tree``
        and ``merge_profile`` take them too."""
        return self._cluster_edges_two("blurrily_storage_cluster_edges_between", left, right, min_permille, capacity)

    def cluster_edge_count_between(self, left, right, min_permille):
        """How many records ``cluster_edges_between`` would return: no buffer is handed, nothing is sorted."""
        return self._cluster_edge_count_two("blurrily_storage_cluster_edges_between", left, right, min_permille)

    @staticmethod
    def merge_edges(*record_lists):
        """Edge record lists, each in ``cluster_edges``' total order (permille descending, then a, then b), as one
        list in that order: uint32[E, 3].  How a caller keeps an edge list current:
        ``merge_edges(held, cluster_edges_extend(old, new, floor))``.  ValueError for a list that is not in order or
        for a record present twice, in one list or in two.  Needs no map and no GPU."""
        lists = [RawMap._records(rows, "edges") for rows in record_lists]
        for rows in lists:
            if len(rows) > 1:
                prev, nxt = rows[:-1], rows[1:]
                eq = lambda c: prev[:, c] == nxt[:, c]
                before = (prev[:, 2] > nxt[:, 2]) | (eq(2) & ((prev[:, 0] < nxt[:, 0]) | (eq(0) & (prev[:, 1] < nxt[:, 1]))))
                if not before.all():
                    raise ValueError("a record list is not in order (permille descending, then a, then b), or holds "
                                     "a record twice")
        if not sum(len(rows) for rows in lists):
            return np.zeros((0, 3), dtype=np.uint32)
        rows = np.concatenate(lists)
        rows = np.ascontiguousarray(rows[np.lexsort((rows[:, 1], rows[:, 0], -rows[:, 2].astype(np.int64)))])
        if len(rows) > 1 and (rows[1:] == rows[:-1]).all(axis=1).any():
            raise ValueError("a record is present twice")
        return rows

    @staticmethod
    def adjacency(edges, references):
        """``cluster_edges`` records (``cluster_edges_extend``'s and ``cluster_edges_between``'s too: of a left row's
        neighbours the first is its best link) as neighbour lists, what a caller's own graph code starts from:
        ``(row_off uint64[n + 1], neighbour uint32[2 E], permille uint32[2 E])``, one row per element of ``references``
        -- element i's neighbours are ``neighbour[row_off[i]:row_off[i + 1]]`` with their similarities beside them, in
        the records' order.  A repeated reference gets the same row each time it is listed (so the rows add up to more
        than 2 E then); one that no record names gets an empty row.  ValueError for a record that names a reference
        which is not listed.  Needs no map and no GPU."""
        rows = RawMap._records(edges, "edges")
        refs = np.asarray(references, dtype=np.uint32)
        if refs.ndim != 1:
            raise ValueError("references must be one-dimensional")
        listed = np.unique(refs)
        ends = np.searchsorted(listed, rows[:, :2])
        if len(rows) and (len(listed) == 0 or (listed[np.minimum(ends, len(listed) - 1)] != rows[:, :2]).any()):
            raise ValueError("a record names a reference that is not listed")
        # every record twice, once from each end, kept in the records' order per end
        src = np.concatenate([ends[:, 0], ends[:, 1]]) if len(rows) else np.zeros(0, dtype=np.int64)
        dst = np.concatenate([rows[:, 1], rows[:, 0]])
        sim = np.concatenate([rows[:, 2], rows[:, 2]])
        at = np.concatenate([np.arange(len(rows)), np.arange(len(rows))])
        order = np.lexsort((at, src))
        dst, sim = dst[order], sim[order]
        start = np.zeros(len(listed) + 1, dtype=np.int64)
        np.cumsum(np.bincount(src, minlength=len(listed)), out=start[1:])
        if len(listed) == len(refs) and (listed == refs).all():    # (the list is its own numbering: nothing to gather)
            return start.astype(np.uint64), dst.astype(np.uint32), sim.astype(np.uint32)
        node = np.searchsorted(listed, refs)
        size = start[node + 1] - start[node]
        row_off = np.zeros(len(refs) + 1, dtype=np.int64)
        np.cumsum(size, out=row_off[1:])
        pick = np.repeat(start[node] - row_off[:-1], size) + np.arange(row_off[-1])
        return row_off.astype(np.uint64), dst[pick].astype(np.uint32), sim[pick].astype(np.uint32)

    @staticmethod
    def merge_profile(merges, nodes=None):
        """What a caller slides the cut by: per distinct height of a ``cluster_tree`` result, highest first,
        ``{permille, merges, n_clusters}`` -- the merges at or above it and the clusters a cut there leaves among
        ``nodes`` references (default: the references the merges name, so singletons are left out).  (It counts
        records: for ``cluster_edges`` records, which are no forest, ``merges`` is the edges at or above each height
        and ``n_clusters`` means nothing.)"""
        merges = np.asarray(merges, dtype=np.uint32).reshape(-1, 3)
        if nodes is None:
            nodes = len(np.unique(merges[:, :2]))
        heights, counts = np.unique(merges[:, 2], return_counts=True)
        done = np.cumsum(counts[::-1])
        return [{"permille": int(h), "merges": int(k), "n_clusters": int(nodes) - int(k)}
                for h, k in zip(heights[::-1].tolist(), done.tolist())]

    def sync_device(self):
        self._check_open()
        _check(self._lib.blurrily_storage_sync_device(self._h))

    def device_info(self):
        self._check_open()
        info = _native.DeviceInfo()
        self._lib.blurrily_storage_device_info(self._h, C.byref(info))
        return {f: getattr(info, f) for f, _ in info._fields_}

    def set_timing(self, enabled):
        self._check_open()
        self._lib.blurrily_storage_set_timing(self._h, 1 if enabled else 0)

    STAT_NAMES = ("posting_entries", "steps", "table_words", "tasks", "compactions", "resweeps",
                  "units", "probes")

    def set_stats(self, enabled):
        """Request counters of the find kernels on/off (include/blurrily_storage.h)."""
        self._check_open()
        self._lib.blurrily_storage_set_stats(self._h, 1 if enabled else 0)

    # bits of find_path_flags() (csrc/find_kernels.h: kPath*)
    PATH_FLAGS = ("nibble", "byte", "cold_start", "resweep", "compaction", "skipped", "ring_overflow", "pipelined",
                  "wide", "chunked", "ranged", "multi_pass", "tombstone", "own_only", "ws_task", "ws_left_out",
                  "ws_robust", "ws_cand_overflow", "ws_pool_overflow", "ws_wide", "ws_table_walk", "nm_left_out", "small")

    def find_path_flags(self, n):
        """Per needle of the last find call made while set_stats(True): which kernel paths its find took
        (uint32 array; bit i = PATH_FLAGS[i])."""
        self._check_open()
        out = np.zeros(n, dtype=np.uint32)
        _check(self._lib.blurrily_storage_find_path_flags(self._h, out.ctypes.data, n))
        return out

    def last_kernels(self):
        """Names of the find kernels the last batched find launched, in launch order (blurrily_storage_last_kernels)."""
        self._check_open()
        buf = C.create_string_buffer(512)
        need = self._lib.blurrily_storage_last_kernels(self._h, buf, len(buf))
        if need >= len(buf):                              # (a call of many launches: the whole list, not its first 511 bytes)
            buf = C.create_string_buffer(need + 1)
            self._lib.blurrily_storage_last_kernels(self._h, buf, len(buf))
        return [k for k in buf.value.decode().split("+") if k]

    def tune(self, packed, offsets, n, limit):
        """Measure now which sweep serves batches of n needles at this limit (blurrily_storage_tune): the needles
        given, repeated up to n, go through every sweep the class can take."""
        self._check_open()
        data, offsets, n_given = _needles(packed, offsets)
        _check(self._lib.blurrily_storage_tune(self._h, data, offsets.ctypes.data, n_given, n, limit))

    def set_option(self, key, value):
        """A tunable of this map (include/blurrily_storage.h: blurrily_storage_set_option)."""
        self._check_open()
        _check(self._lib.blurrily_storage_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        self._check_open()
        out = C.c_longlong(0)
        _check(self._lib.blurrily_storage_get_option(self._h, key.encode(), C.byref(out)))
        return int(out.value)

    def find_stats(self):
        """Counters of the last find call made while set_stats(True): a dict by STAT_NAMES."""
        self._check_open()
        out = (C.c_uint64 * 8)()
        _check(self._lib.blurrily_storage_find_stats(self._h, out))
        return dict(zip(self.STAT_NAMES, (int(v) for v in out)))

    @property
    def handle(self):
        self._check_open()
        return self._h


class Scope:
    """A fixed set of references of one map (``RawMap.scope``): finds with ``find_in`` / ``find_batch_in`` return rows
    of its members only.  Membership is read at each find: deleted members are not found, members put later are."""

    ClosedError = ClosedError

    def __init__(self, owner, handle, refs=None):
        self._lib = owner._lib
        self._map = owner
        self._h = handle
        self._refs = refs                               # its references, sorted and distinct
        self._closed = False

    def _check_open(self):
        if self._closed:
            raise ClosedError("Scope was closed")
        self._map._check_open()

    def members(self):
        """How many of the scope's references the map holds now."""
        self._check_open()
        held = C.c_uint32()
        _check(self._lib.blurrily_scope_members(self._h, C.byref(held)))
        return held.value

    def close(self):
        if self._closed:
            return None
        self._closed = True
        _check(self._lib.blurrily_scope_close(C.byref(self._h)))    # (it never touches the map)
        return None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        if not getattr(self, "_closed", True):
            self._lib.blurrily_scope_close(C.byref(self._h))
            self._closed = True


def set_process_option(key, value):
    """A process-wide tunable ("host_threads", "build_trace"; include/blurrily_storage.h)."""
    _check(_native.lib().blurrily_storage_set_option(None, key.encode(), int(value)))


def _as_bytes(s):
    """StringValuePtr: the C side sees the bytes up to the first NUL."""
    if isinstance(s, bytes):
        return s
    return str(s).encode("utf-8")


_PLAIN = re.compile(r"^([a-z ])+$", re.M)       # Ruby's ^ and $ are line anchors (map.rb:42)
_ASCII_UPPER = {c: c + 32 for c in range(ord("A"), ord("Z") + 1)}


def normalize_string(needle):
    """lib/blurrily/map.rb:40-47.

    downcase -> unless only ``[a-z ]``: NFKD, drop non-ASCII, non ``[a-z]`` -> space ->
    squeeze whitespace, strip.  ``downcase`` is ASCII-only, as on the Rubies the reference
    supports (.travis.yml:1-5: 1.9.3-2.2.0).  NFKD comes from Python's ``unicodedata``;
    the reference uses ActiveSupport 4.2's tables (Gemfile.lock:11) -- parity on non-ASCII
    input is pinned only by spec/blurrily/map_spec.rb:55-59 (``'@€%é'`` -> ``'e'``).
    """
    result = str(needle).translate(_ASCII_UPPER)
    if not _PLAIN.search(result):
        result = unicodedata.normalize("NFKD", result)
        result = re.sub(r"[^\x00-\x7F]", "", result)
        result = re.sub(r"[^a-z]", " ", result)
    result = re.sub(r"[ \t\r\n\f\v]+", " ", result)
    return result.strip(" \t\r\n\f\v").rstrip("\0 \t\r\n\f\v")


def _limit_or_default(limit):
    """Blurrily::Map's batched counterparts: a limit <= 0 means the default, as find's does."""
    limit = int(limit)
    return limit if limit > 0 else LIMIT_DEFAULT


def _normalised(needles):
    """The needles as ``find`` would send them, packed: (packed, offsets)."""
    return _pack([_as_bytes(normalize_string(s)) for s in needles])


class Map(RawMap):
    """Blurrily::Map (lib/blurrily/map.rb:6-48)."""

    def __init__(self, _handle=None):
        super().__init__(_handle)
        self._clean_path = None

    def put(self, needle, reference, weight=None):                  # map.rb:8-13
        weight = 0 if weight is None else weight
        needle = normalize_string(needle)
        self._clean_path = None
        return super().put(needle, reference, weight)

    def find(self, needle, limit=LIMIT_DEFAULT):                    # map.rb:15-18
        return super().find(normalize_string(needle), limit)

    def delete(self, reference):                                    # map.rb:20-23
        self._clean_path = None
        return super().delete(reference)

    def save(self, path):                                           # map.rb:25-30
        path = os.fspath(path)
        if self._clean_path == path:
            return None
        super().save(path)
        self._clean_path = path
        return None

    @classmethod
    def load(cls, path):                                            # map.rb:32-36
        obj = super().load(path)
        obj._clean_path = os.fspath(path)
        return obj

    # batched counterparts: each element behaves exactly like the single call
    def put_many(self, needles, references, weights=None):
        self._clean_path = None
        return super().put_many([normalize_string(s) for s in needles], references, weights)

    def find_by_reference(self, reference, limit=LIMIT_DEFAULT):
        return super().find_by_reference(reference, limit)

    def dense_tree(self, references, min_permille, min_degree):
        """``cluster_core_tree`` over the references as a set: ``(refs, labels, core_permille, merges)``, refs
        ascending without repeats -- what ``cut_core_tree`` takes, the counts left out."""
        refs = np.unique(self._refs(references))
        return (refs,) + super().cluster_core_tree(refs, min_permille, min_degree)[:3]

    def find_batch_by_reference(self, references, limit=LIMIT_DEFAULT):
        """``[self.find_by_reference(r, limit) for r in references]`` in one GPU batch."""
        rows, counts, _ = super().find_batch_by_reference(references, _limit_or_default(limit))
        return _lists(rows, counts)

    def find_in(self, scope, needle, limit=LIMIT_DEFAULT):
        """``find`` among the references of `scope` (a ``Scope`` or an iterable of references) only."""
        return super().find_in(scope, normalize_string(needle), limit)

    def find_batch_in(self, scope, needles, limit=LIMIT_DEFAULT):
        """``[self.find_in(scope, s, limit) for s in needles]`` in one GPU batch."""
        limit = _limit_or_default(limit)
        return _lists(*super().find_batch_in(scope, *_normalised(needles), limit))

    def find_batch_each_in(self, scopes, which, needles, limit=LIMIT_DEFAULT):
        """``[self.find_in(scopes[w], s, limit) if w is not None else self.find(s, limit) for s, w in zip(needles,
        which)]`` in one GPU batch."""
        limit = _limit_or_default(limit)
        return _lists(*super().find_batch_each_in(scopes, which, *_normalised(needles), limit))

    def join_within(self, scopes, limit=LIMIT_DEFAULT):
        return super().join_within(scopes, _limit_or_default(limit))

    def find_above(self, needle, min_matches=0, min_permille=0):
        """Every row of the normalised needle at or above its bar (``RawMap.find_above``)."""
        return super().find_above(normalize_string(needle), min_matches, min_permille)

    def find_batch_above(self, needles, min_matches=0, min_permille=0):
        """``[self.find_above(s, min_matches, min_permille) for s in needles]`` in one GPU batch."""
        rows, row_off = super().find_batch_above_packed(*_normalised(needles), min_matches, min_permille)
        return [rows[lo:hi].tolist() for lo, hi in zip(row_off[:-1].tolist(), row_off[1:].tolist())]

    def find_above_in(self, scope, needle, min_matches=0, min_permille=0):
        """``find_above`` among the references of `scope` (a ``Scope`` or an iterable of references) only."""
        return super().find_above_in(scope, normalize_string(needle), min_matches, min_permille)

    def find_batch_above_in(self, scope, needles, min_matches=0, min_permille=0):
        """``[self.find_above_in(scope, s, min_matches, min_permille) for s in needles]`` in one GPU batch."""
        rows, row_off = super().find_batch_above_in_packed(scope, *_normalised(needles), min_matches, min_permille)
        return [rows[lo:hi].tolist() for lo, hi in zip(row_off[:-1].tolist(), row_off[1:].tolist())]

    def find_batch_above_each_in(self, scopes, which, needles, min_matches=0, min_permille=0):
        """``[self.find_above_in(scopes[w], s, ...) if w is not None else self.find_above(s, ...) for s, w in
        zip(needles, which)]`` in one GPU batch."""
        rows, row_off = super().find_batch_above_each_in(scopes, which, *_normalised(needles), min_matches,
                                                         min_permille)
        return [rows[lo:hi].tolist() for lo, hi in zip(row_off[:-1].tolist(), row_off[1:].tolist())]

    def join_above_within(self, scopes, min_matches=0, min_permille=0):
        return super().join_above_within(scopes, min_matches, min_permille)

    def find_similar(self, needle, limit=LIMIT_DEFAULT, min_permille=0):
        """The best rows of the normalised needle by trigram Jaccard similarity (``RawMap.find_similar``): a list of
        ``[ref, matches, weight, R]``."""
        return super().find_similar(normalize_string(needle), limit, min_permille)

    def find_batch_similar(self, needles, limit=LIMIT_DEFAULT, min_permille=0):
        """``[self.find_similar(s, limit, min_permille) for s in needles]`` in one GPU batch."""
        limit = _limit_or_default(limit)
        return _lists(*super().find_batch_similar_packed(*_normalised(needles), limit, min_permille))

    def find_similar_in(self, scope, needle, limit=LIMIT_DEFAULT, min_permille=0):
        """``find_similar`` among the references of `scope` (a ``Scope`` or an iterable of references) only."""
        return super().find_similar_in(scope, normalize_string(needle), limit, min_permille)

    def find_batch_similar_each_in(self, scopes, which, needles, limit=LIMIT_DEFAULT, min_permille=0):
        """``[self.find_similar_in(scopes[w], s, limit, min_permille) if w is not None else self.find_similar(s, limit,
        min_permille) for s, w in zip(needles, which)]`` in one GPU batch."""
        limit = _limit_or_default(limit)
        return _lists(*super().find_batch_similar_each_in(scopes, which, *_normalised(needles), limit, min_permille))

    def join_similar_within(self, scopes, limit=LIMIT_DEFAULT, min_permille=0):
        return super().join_similar_within(scopes, _limit_or_default(limit), min_permille)

    def find_batch(self, needles, limit=LIMIT_DEFAULT):
        """``[self.find(s, limit) for s in needles]`` in one GPU batch."""
        limit = _limit_or_default(limit)
        # ASCII needles go to the GPU as they are (normalize_string runs there); the others are
        # normalised here first -- NFKD is host work -- and pass through the device step unchanged
        raw = []
        for s in needles:
            b = _as_bytes(s)
            raw.append(b if b.isascii() else _as_bytes(normalize_string(b.decode("utf-8", "replace")
                                                                        if isinstance(s, bytes) else s)))
        rows, counts, flags = self.find_batch_raw_packed(*_pack(raw), limit)
        assert not flags.any()
        return _lists(rows, counts)
