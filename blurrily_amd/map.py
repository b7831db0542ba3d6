"""Host-side mirror of the reference's Ruby API over the C ABI.

``RawMap`` mirrors the C glue class ``Blurrily::RawMap`` (ext/blurrily/map_ext.c:206-229:
``new``/``load``, ``put/3``, ``delete/1``, ``save/1``, ``find/2``, ``stats/0``, ``close/0``,
``ClosedError``); ``Map`` mirrors ``Blurrily::Map`` (lib/blurrily/map.rb:8-47: string
normalisation, default weight/limit, clean-path save elision).  Same names, same argument
meaning, same error behaviour -- so tests read like spec/blurrily/map_spec.rb.

Every method reads: check open, convert the arguments, call the C function by name, shape the result.  What the
conversions and the shaping share is in ``_marshal.py``, once each; the cluster methods are ``map_clusters.py``'s, and
what works on their results without a map is ``cluster_records.py``'s (``RawMap`` carries both).

The image has no Ruby; INTEGRATION.md shows the Ruby side of the same boundary.
"""
import ctypes as C
import os
import re
import unicodedata
from contextlib import contextmanager as _contextmanager

import numpy as np

from . import _native
from . import cluster_records as _cluster_records
from ._marshal import (_as_bytes, _batch_limit, _blocks, _call_growing, _check, _find_limit, _held_offsets, _lists,
                       _match_lists, _match_rows, _members_of, _needles, _pack, _permille, _ptr, _records, _refs,
                       _refs_with_keys, _similar_lists, _similar_rows, _slices, _u32)
from .defaults import LIMIT_DEFAULT
from .map_clusters import ClusterMethods as _ClusterMethods


class ClosedError(RuntimeError):
    """Blurrily::RawMap::ClosedError (map_ext.c:216)."""


class RawMap(_ClusterMethods):
    """Thin object wrapper over a ``trigram_map`` handle (map_ext.c)."""

    ClosedError = ClosedError
    _refs, _records = staticmethod(_refs), staticmethod(_records)
    # what works on the cluster methods' results, without a map or a GPU (cluster_records.py)
    cut_tree = staticmethod(_cluster_records.cut_tree)
    cut_core_tree = staticmethod(_cluster_records.cut_core_tree)
    tree_changes = staticmethod(_cluster_records.tree_changes)
    tree_by_block = staticmethod(_cluster_records.tree_by_block)
    merge_edges = staticmethod(_cluster_records.merge_edges)
    adjacency = staticmethod(_cluster_records.adjacency)
    merge_profile = staticmethod(_cluster_records.merge_profile)

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
        rows = _match_rows(c_limit)()
        return _match_lists(rows, self._lib.blurrily_storage_find(self._h, _as_bytes(needle), c_limit, rows))

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
        refs = _refs(references)
        n = len(refs)
        # each distinct reference once: their codes together are at most the map's trigram count (the library's
        # extraction also reads each once), so one call always fits
        uniq, inv = np.unique(refs, return_inverse=True)
        n_u = len(uniq)
        w_u = np.zeros(n_u, dtype=np.uint32)
        offs_u = np.zeros(n_u + 1, dtype=np.uint64)
        codes_u = _call_growing(
            lambda codes, cap: self._lib.blurrily_storage_get_batch(
                self._h, _ptr(uniq), n_u, w_u.ctypes.data, offs_u.ctypes.data, codes, cap),
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
        refs = _refs(references)
        n = len(refs)
        limit = _batch_limit(limit)
        out, ptrs = _blocks(n, limit, per_needle=1)
        _check(self._lib.blurrily_storage_find_references(self._h, _ptr(refs), n, limit, *ptrs))
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
        refs = _refs(references if isinstance(references, np.ndarray) else list(references))
        h = C.c_void_p()
        _check(self._lib.blurrily_scope_new(self._h, _ptr(refs), len(refs), C.byref(h)))
        return Scope(self, h, np.unique(refs))

    def _one_shot(self, method, scope, *args):
        """``method(self, scope, *args)`` with `scope`, an iterable of references, made a Scope for this one call.  The
        caller names RawMap's own method, so that a subclass's override is not entered twice.  (The Scope's own
        ``with``: a generator context manager here cost a single find 1.6 us.)"""
        with self.scope(scope) as one_shot:
            return method(self, one_shot, *args)

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
            return self._one_shot(RawMap.find_batch_in, scope, packed, offsets, limit)
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
                self._h, self._handles(scs), len(scs), _ptr(which), data, offsets.ctypes.data, n,
                limit, *ptrs))
            return out

    def find_batch_by_reference_each_in(self, scopes, which, references, limit):
        """``find_batch_by_reference`` with a scope per reference, as ``find_batch_each_in``.
        Returns (rows[n, limit, 3] uint32, counts[n] uint32, nb_trigrams[n] uint32)."""
        self._check_open()
        refs = _refs(references)
        n = len(refs)
        which = self._which(which, n)
        with self._scopes_of(scopes) as scs:
            limit = _batch_limit(limit)
            out, ptrs = _blocks(n, limit, per_needle=1)
            _check(self._lib.blurrily_storage_find_references_each_in(
                self._h, self._handles(scs), len(scs), _ptr(which), _ptr(refs), n, limit, *ptrs))
            return out

    def join_within(self, scopes, limit):
        """The blocked self-join: every member of every scope searched among its own scope (``find_by_reference``
        restricted to it), in one GPU batch.  Returns (references[k] uint32, which[k] uint32: the scope of each,
        rows: k lists of [ref, matches, weight]) over the members the map holds, scope after scope."""
        self._check_open()
        with self._scopes_of(scopes) as scs:
            refs, which = _members_of(scs)
            rows, counts, ntri = self.find_batch_by_reference_each_in(scs, which, refs, limit)
        held = np.nonzero(ntri)[0]
        return refs[held], which[held], _lists(rows[held], counts[held])

    def find_in(self, scope, needle, limit):
        """``find`` among the scope's members only (rows ``[ref, matches, weight]``); `limit` as find's."""
        self._check_open()
        c_limit = _find_limit(limit)
        if not isinstance(scope, Scope):
            return self._one_shot(RawMap.find_in, scope, needle, limit)
        sc = self._own(scope)
        rows = _match_rows(c_limit)()
        return _match_lists(rows, self._lib.blurrily_storage_find_in(self._h, sc._h, _as_bytes(needle), c_limit, rows))

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
        return _call_growing(lambda rows, cap, total: self._lib.blurrily_storage_find_above(
            self._h, s, mm, mp, rows, cap, total), 1024, row=(3,)).tolist()

    def find_batch_by_reference_above(self, references, min_matches=0, min_permille=0):
        """``find_batch_above_packed`` for stored references (each among its own rows; none for a reference the map
        does not hold).  Returns (rows[R, 3] uint32, row_off[n + 1] uint64, nb_trigrams[n] uint32)."""
        self._check_open()
        mm, mp = self._bar(min_matches, min_permille)
        refs = _refs(references)
        n = len(refs)
        ntri = np.zeros(n, dtype=np.uint32)
        rows, row_off = self._above(lambda rows, cap, off: self._lib.blurrily_storage_find_references_above(
            self._h, _ptr(refs), n, mm, mp, rows, cap, off, ntri.ctypes.data), n)
        return rows, row_off, ntri

    def join_above(self, references, min_matches=0, min_permille=0):
        """The threshold self-join: every held reference's rows at or above its bar, as arrays.  Returns (refs[k]
        uint32: the references the map holds, in the order given; row_off[k + 1] uint64; rows[R, 3] uint32)."""
        rows, row_off, ntri = self.find_batch_by_reference_above(references, min_matches, min_permille)
        refs = _refs(references)
        held, counts, off = _held_offsets(row_off, ntri)
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
        rows, ntri = _similar_rows(c_limit)
        return _similar_lists(rows, ntri, self._lib.blurrily_storage_find_similar(
            self._h, _as_bytes(needle), c_limit, mp, rows.ctypes.data, ntri.ctypes.data))

    def find_batch_by_reference_similar(self, references, limit, min_permille=0):
        """``find_batch_similar_packed`` for stored references (each its own row at similarity 1; none for a reference
        the map does not hold).  Returns (rows[n, limit, 3] uint32, counts[n] uint32, row_ntri[n, limit] uint32,
        nb_trigrams[n] uint32)."""
        self._check_open()
        mp = _permille(min_permille)
        refs = _refs(references)
        n = len(refs)
        limit = _batch_limit(limit)
        out, ptrs = _blocks(n, limit, row_ntri=True, per_needle=1)
        _check(self._lib.blurrily_storage_find_references_similar(self._h, _ptr(refs), n, limit,
                                                                  mp, *ptrs))
        return out

    # -- scoped similarity find: the similarity find among a scope's members -------------------
    def find_batch_similar_in_packed(self, scope, packed, offsets, limit, min_permille=0):
        """``find_batch_similar_packed`` among the scope's members only (a ``Scope`` or an iterable of references).
        Returns (rows[n, limit, 3] uint32, counts[n] uint32, row_ntri[n, limit] uint32)."""
        self._check_open()
        mp = _permille(min_permille)
        if not isinstance(scope, Scope):
            return self._one_shot(RawMap.find_batch_similar_in_packed, scope, packed, offsets, limit, mp)
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
            return self._one_shot(RawMap.find_similar_in, scope, needle, limit, mp)
        sc = self._own(scope)
        rows, ntri = _similar_rows(c_limit)
        return _similar_lists(rows, ntri, self._lib.blurrily_storage_find_similar_in(
            self._h, sc._h, _as_bytes(needle), c_limit, mp, rows.ctypes.data, ntri.ctypes.data))

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
                self._h, self._handles(scs), len(scs), _ptr(which), data, offsets.ctypes.data, n,
                limit, mp, *ptrs))
            return out

    def find_batch_by_reference_similar_each_in(self, scopes, which, references, limit, min_permille=0):
        """``find_batch_by_reference_similar`` with a scope per reference.  Returns (rows[n, limit, 3] uint32,
        counts[n] uint32, row_ntri[n, limit] uint32, nb_trigrams[n] uint32)."""
        self._check_open()
        mp = _permille(min_permille)
        refs = _refs(references)
        n = len(refs)
        which = self._which(which, n)
        with self._scopes_of(scopes) as scs:
            limit = _batch_limit(limit)
            out, ptrs = _blocks(n, limit, row_ntri=True, per_needle=1)
            _check(self._lib.blurrily_storage_find_references_similar_each_in(
                self._h, self._handles(scs), len(scs), _ptr(which), _ptr(refs), n, limit, mp, *ptrs))
            return out

    def join_similar_within(self, scopes, limit, min_permille=0):
        """The blocked similarity self-join: every member of every scope ranked by similarity among its own scope, in
        one GPU batch.  Returns (references[k] uint32, which[k] uint32: the scope of each, rows: k lists of
        [ref, matches, weight, R]) over the members the map holds, scope after scope."""
        self._check_open()
        with self._scopes_of(scopes) as scs:
            refs, which = _members_of(scs)
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
            return self._one_shot(RawMap.find_batch_above_in_packed, scope, packed, offsets, mm, mp)
        sc = self._own(scope)
        data, offsets, n = _needles(packed, offsets)
        return self._above(lambda rows, cap, off: self._lib.blurrily_storage_find_batch_above_in(
            self._h, sc._h, data, offsets.ctypes.data, n, mm, mp, rows, cap, off), n)

    def find_above_in(self, scope, needle, min_matches=0, min_permille=0):
        """``find_above`` among the scope's members only: a list of ``[ref, matches, weight]``."""
        self._check_open()
        mm, mp = self._bar(min_matches, min_permille)
        if not isinstance(scope, Scope):
            return self._one_shot(RawMap.find_above_in, scope, needle, mm, mp)
        sc = self._own(scope)
        s = _as_bytes(needle)
        return _call_growing(lambda rows, cap, total: self._lib.blurrily_storage_find_above_in(
            self._h, sc._h, s, mm, mp, rows, cap, total), 1024, row=(3,)).tolist()

    def find_batch_above_each_in(self, scopes, which, packed, offsets, min_matches=0, min_permille=0):
        """``find_batch_above_packed`` with a scope per needle: needle i among ``scopes[which[i]]`` only, or the whole
        map when ``which[i]`` is None.  Returns (rows[R, 3] uint32, row_off[n + 1] uint64)."""
        self._check_open()
        mm, mp = self._bar(min_matches, min_permille)
        which = self._which(which, len(offsets) - 1)
        with self._scopes_of(scopes) as scs:
            data, offsets, n = _needles(packed, offsets)
            return self._above(lambda rows, cap, off: self._lib.blurrily_storage_find_batch_above_each_in(
                self._h, self._handles(scs), len(scs), _ptr(which), data, offsets.ctypes.data, n,
                mm, mp, rows, cap, off), n)

    def find_batch_by_reference_above_each_in(self, scopes, which, references, min_matches=0, min_permille=0):
        """``find_batch_by_reference_above`` with a scope per reference.  Returns (rows[R, 3] uint32,
        row_off[n + 1] uint64, nb_trigrams[n] uint32)."""
        self._check_open()
        mm, mp = self._bar(min_matches, min_permille)
        refs = _refs(references)
        n = len(refs)
        which = self._which(which, n)
        ntri = np.zeros(n, dtype=np.uint32)
        with self._scopes_of(scopes) as scs:
            rows, row_off = self._above(lambda rows, cap, off: self._lib.blurrily_storage_find_references_above_each_in(
                self._h, self._handles(scs), len(scs), _ptr(which), _ptr(refs), n, mm, mp, rows, cap,
                off, ntri.ctypes.data), n)
        return rows, row_off, ntri

    def join_above_within(self, scopes, min_matches=0, min_permille=0):
        """The blocked threshold self-join: every member of every scope with all the members of its own scope at or above
        its bar, in one GPU batch.  Returns (refs[k] uint32, which[k] uint32: the scope of each, row_off[k + 1] uint64,
        rows[R, 3] uint32) over the members the map holds, scope after scope."""
        self._check_open()
        with self._scopes_of(scopes) as scs:
            refs, which = _members_of(scs)
            rows, row_off, ntri = self.find_batch_by_reference_above_each_in(scs, which, refs, min_matches, min_permille)
        held, _, off = _held_offsets(row_off, ntri)      # (a reference the map does not hold has no rows: nothing to cut)
        return refs[held], which[held], off, rows

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
        refs = np.unique(_refs(references))
        return (refs,) + super().cluster_core_tree(refs, min_permille, min_degree)[:3]

    def dense_tree_within(self, references, blocks, min_permille, min_degree):
        """``cluster_core_tree_within`` over the (reference, key) pairs as a set: ``(refs, keys, labels, core_permille,
        merges)``, refs ascending without repeats, each with its key -- what ``cut_core_tree`` and ``tree_by_block``
        take, the counts left out.  ValueError for a reference that carries two keys."""
        refs, keys = _refs_with_keys(references, blocks)
        refs, at, number = np.unique(refs, return_index=True, return_inverse=True)
        if (keys[at][number.reshape(-1)] != keys).any():
            raise ValueError("a reference is listed under two block keys")
        keys = keys[at]
        return (refs, keys) + super().cluster_core_tree_within(refs, keys, min_permille, min_degree)[:3]

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
        return _slices(rows, row_off)

    def find_above_in(self, scope, needle, min_matches=0, min_permille=0):
        """``find_above`` among the references of `scope` (a ``Scope`` or an iterable of references) only."""
        return super().find_above_in(scope, normalize_string(needle), min_matches, min_permille)

    def find_batch_above_in(self, scope, needles, min_matches=0, min_permille=0):
        """``[self.find_above_in(scope, s, min_matches, min_permille) for s in needles]`` in one GPU batch."""
        rows, row_off = super().find_batch_above_in_packed(scope, *_normalised(needles), min_matches, min_permille)
        return _slices(rows, row_off)

    def find_batch_above_each_in(self, scopes, which, needles, min_matches=0, min_permille=0):
        """``[self.find_above_in(scopes[w], s, ...) if w is not None else self.find_above(s, ...) for s, w in
        zip(needles, which)]`` in one GPU batch."""
        rows, row_off = super().find_batch_above_each_in(scopes, which, *_normalised(needles), min_matches,
                                                         min_permille)
        return _slices(rows, row_off)

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
