"""What the methods of ``map.py`` and ``map_clusters.py`` share of a call across the C ABI, once each: the result check,
the argument conversions, the buffers a call fills and how they are cut and listed.  Functions only: nothing here knows
a map, and which C function is called stands in the method that calls it (DESIGN.md sections 2 and 43).
"""
import ctypes as C
import os
from errno import ERANGE as _ERANGE
from functools import lru_cache

import numpy as np

from . import _native
from .defaults import LIMIT_DEFAULT

_U32_MAX = 0xFFFFFFFF
_NO_BYTES = C.create_string_buffer(1)


def _raise_errno(path=None):
    err = C.get_errno()
    raise OSError(err, os.strerror(err), path)


def _check(res, path=None):
    """The result of a C call that can fail: negative -> OSError from errno (with the path where one is given)."""
    if res < 0:
        _raise_errno(path)
    return res


def _as_bytes(s):
    """StringValuePtr: the C side sees the bytes up to the first NUL."""
    if isinstance(s, bytes):
        return s
    return str(s).encode("utf-8")


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


# -- lists in ------------------------------------------------------------------------------------------------------
def _refs(references):
    """A list of references (or of labels, or of block keys) as a contiguous one-dimensional uint32 array; one that is
    already that goes as it is."""
    refs = np.asarray(references)
    if refs.ndim != 1:
        raise ValueError("references must be one-dimensional")
    if refs.dtype != np.uint32:
        refs = np.array([_u32(r, "reference") for r in refs.tolist()], dtype=np.uint32)
    return np.ascontiguousarray(refs)


def _refs_with_keys(references, blocks):
    """Listed references with a block key each: (refs, keys), both as ``_refs`` gives them."""
    refs, keys = _refs(references), _refs(blocks)
    if len(keys) != len(refs):
        raise ValueError(f"{len(keys)} block keys for {len(refs)} references")
    return refs, keys


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


def _ptr(a):
    """An array's address for the C call; NULL for no array and for an empty one (the size, not the length: labels[K, 0]
    has K rows and nothing to point to)."""
    return None if a is None or a.size == 0 else a.ctypes.data


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


def _members_of(scs):
    """The members of these scopes, scope after scope: (refs[k] uint32, which[k] uint32: the scope of each)."""
    parts = [sc._refs if sc._refs is not None else np.zeros(0, np.uint32) for sc in scs]
    refs = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)
    return refs, np.repeat(np.arange(len(parts), dtype=np.uint32), [len(p) for p in parts])


# -- what a call fills -----------------------------------------------------------------------------------------------
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


@lru_cache(maxsize=None)
def _match_rows(c_limit):
    """The type of what a single find fills: ``trigram_match`` rows, room for one where the limit is none.  (Kept per
    limit: making the array type anew cost a single find 0.07 us.)"""
    return _native.TrigramMatch * max(c_limit, 1)


def _match_lists(rows, res):
    """A single find's result `res` checked, and that many of its rows as ``[ref, matches, weight]``."""
    return [[rows[k].reference, rows[k].matches, rows[k].weight] for k in range(_check(res))]


def _similar_rows(c_limit):
    """What a single similarity find fills: (rows[room, 3], row_ntri[room]) uint32."""
    room = max(c_limit, 1)
    return np.zeros((room, 3), dtype=np.uint32), np.zeros(room, dtype=np.uint32)


def _similar_lists(rows, ntri, res):
    """A single similarity find's result `res` checked, and that many rows as ``[ref, matches, weight, R]``."""
    res = _check(res)
    return [r + [t] for r, t in zip(rows[:res].tolist(), ntri[:res].tolist())]


def _counters(*widths):
    """The counters a call writes by reference: a ``c_uint32`` or ``c_uint64`` per width given, zeroed."""
    return [(C.c_uint32 if w == 32 else C.c_uint64)(0) for w in widths]


def _byrefs(counters):
    return [C.byref(c) for c in counters]


def _ints(counters):
    return tuple(int(c.value) for c in counters)


def _merges(n):
    """Room for the records of a tree over n references: uint32[n, 3] (a forest has fewer)."""
    return np.zeros((n, 3), dtype=np.uint32)


def _merged(merges, counters):
    """(A tree call's records cut to its first counter, n_merges, as an array of their own; the other counters ...)."""
    k, *rest = _ints(counters)
    return (merges[:k].copy(),) + tuple(rest)


def _call_growing(call, cap, needed=None, row=(), dtype=np.uint32):
    """``call(pointer, cap)`` into a buffer of `cap` rows (np.empty: only the pages written are committed); when the
    library answers ERANGE it has reported the room it needs (``needed()``), and the call is made once more with
    that.  Returns the buffer filled.  Without `needed` the library reports the rows in a ``uint64_t`` by reference --
    ``call(pointer, cap, total)``: a single threshold find, the edge records -- and the buffer comes back cut to them."""
    total = None
    if needed is None:
        total = C.c_uint64(0)
        ref, needed = C.byref(total), lambda: total.value
    while True:
        buf = np.empty((cap,) + row, dtype=dtype)
        if total is None:
            if call(buf.ctypes.data, cap) == 0:
                return buf
        elif call(buf.ctypes.data, cap, ref) == 0:
            return buf[:total.value]
        if C.get_errno() != _ERANGE or needed() <= cap:
            _raise_errno()
        cap = needed()


def _edge_records(call, n, capacity):
    """The edge-record protocol over n listed references: room for `capacity` records first (default max(1024, 8 n)),
    once more with what the library reported if they are more."""
    first = max(1024, 8 * n) if capacity is None else int(capacity)
    if not 0 <= first < 1 << 64:
        raise OverflowError(f"capacity {capacity!r} out of range of uint64_t")
    return _call_growing(call, first, row=(3,))


def _edge_count(call):
    """The count-only call of the same entries: no buffer is handed, the total alone comes back."""
    total = C.c_uint64(0)
    _check(call(None, 0, C.byref(total)))
    return int(total.value)


# -- rows out ------------------------------------------------------------------------------------------------------
def _lists(rows, counts, row_ntri=None):
    """rows[n, limit, 3] and counts[n] -> n lists of ``[ref, matches, weight]``; with row_ntri[n, limit], of
    ``[ref, matches, weight, R]``."""
    if row_ntri is None:
        return [rows[i, :c].tolist() for i, c in enumerate(counts.tolist())]
    return [[r + [t] for r, t in zip(rows[i, :c].tolist(), row_ntri[i, :c].tolist())]
            for i, c in enumerate(counts.tolist())]


def _slices(rows, row_off):
    """rows[R, 3] and row_off[n + 1] -> n lists of rows: list i is rows[row_off[i]:row_off[i + 1]]."""
    return [rows[lo:hi].tolist() for lo, hi in zip(row_off[:-1].tolist(), row_off[1:].tolist())]


def _held_offsets(row_off, ntri):
    """Of a by-reference threshold result, the references the map holds: (held: their indices, counts: their rows
    each, off[len(held) + 1] uint64: their row offsets once the others' empty ranges are left out)."""
    held = np.nonzero(ntri)[0]
    counts = np.diff(row_off.astype(np.int64))[held]
    off = np.zeros(len(held) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(counts)
    return held, counts, off
