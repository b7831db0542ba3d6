"""What the Python binding hands the C ABI, recorded without a GPU: a recording object stands where `_lib` stands in a
RawMap, a Map and their Scopes, every public method is driven through a grid of arguments, and each driven call is one
JSON line -- the method and its arguments, every C call it made (symbol, scalars, for each pointer NULL or the dtype,
shape and contents of what it points to on entry, for each by-reference argument its type) and what came back or was
raised.  The first lines are the signatures of every public attribute of RawMap, Map and Scope and the public names of
blurrily_amd.map.  Only the public surface and the `_lib` attribute are used, so the same file runs on two checkouts of
the binding: a change that moves no C call and no exception gives byte-identical output (``cmp``).

    python tools/python_calls.py > calls.jsonl          # (for the other side: the same file in that checkout's tools/)

The library answers canned values: outputs filled with a fixed pattern, counters 2, 3, 4 ..., and once per growing entry
-1 with ERANGE and a larger needed count, so that the second call is seen.  The last line says how many calls were driven
and made, and which symbols of `_native._ENTRIES` that the binding names were never called.
"""
import ctypes as C
import errno
import glob
import inspect
import json
import os
import re
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blurrily_amd.map as map_module                                    # noqa: E402
from blurrily_amd import Map, RawMap, _native                             # noqa: E402
from blurrily_amd.map import Scope, _pack                                 # noqa: E402

P = "blurrily_storage_"
_ROWS = ">rows:u4[n,max(limit,1),3] >counts:u4[n]"
_SIM = _ROWS + " >rntri:u4[n,max(limit,1)]"
_NEEDLES = "packed offsets:u8[n+1]"
_EACH = "h arr n_scopes which:u4[n]"
_TWO = "h one:u4[n1] n1 two:u4[n2] n2 mp ~rows:u4[cap,3] cap &"
# symbol -> its arguments in order.  `h` the map, `sc` a scope's handle, `&` by reference, `str` bytes, `arr` a ctypes
# array, a bare name a scalar, `name:dtype[shape]` an input array, `>` an output the caller zeroed (shown on entry, then
# filled), `~` an output handed uninitialised (shape only), `packed` the needles' bytes (their length is offsets[-1])
SPEC = {
    P + "close": "&", P + "save": "h str", P + "put": "h str reference weight", P + "delete": "h reference",
    P + "find": "h str limit arr", P + "stats": "h &", P + "sync_device": "h", P + "device_info": "h &",
    P + "set_timing": "h on", P + "set_stats": "h on", P + "find_path_flags": "h >out:u4[n] n",
    P + "last_kernels": "h arr size", P + "tune": f"h {_NEEDLES} n n_batch limit", P + "set_option": "h str value",
    P + "get_option": "h str &", P + "find_stats": "h arr",
    P + "put_many": f"h {_NEEDLES} refs:u4[n] weights:u4[n] n",
    P + "find_batch": f"h {_NEEDLES} n limit {_ROWS}", P + "find_batch_raw": f"h {_NEEDLES} n limit {_ROWS} >flags:u4[n]",
    P + "get": "h reference & cap >codes:u2[cap]",
    P + "get_batch": "h refs:u4[n] n >weights:u4[n] >row_off:u8[n+1] ~rows:u2[cap] cap",
    P + "find_references": f"h refs:u4[n] n limit {_ROWS} >ntri:u4[n]",
    "blurrily_scope_new": "h refs:u4[n] n &", "blurrily_scope_close": "&", "blurrily_scope_members": "sc &",
    P + "find_in": "h sc str limit arr", P + "find_batch_in": f"h sc {_NEEDLES} n limit {_ROWS}",
    P + "find_batch_each_in": f"{_EACH} {_NEEDLES} n limit {_ROWS}",
    P + "find_references_each_in": f"{_EACH} refs:u4[n] n limit {_ROWS} >ntri:u4[n]",
    P + "find_batch_above": f"h {_NEEDLES} n mm mp ~rows:u4[cap,3] cap >row_off:u8[n+1]",
    P + "find_above": "h str mm mp ~rows:u4[cap,3] cap &",
    P + "find_references_above": "h refs:u4[n] n mm mp ~rows:u4[cap,3] cap >row_off:u8[n+1] >ntri:u4[n]",
    P + "find_batch_similar": f"h {_NEEDLES} n limit mp {_SIM}",
    P + "find_similar": "h str limit mp >rows:u4[max(limit,1),3] >ntri:u4[max(limit,1)]",
    P + "find_references_similar": f"h refs:u4[n] n limit mp {_SIM} >ntri:u4[n]",
    P + "find_batch_similar_in": f"h sc {_NEEDLES} n limit mp {_SIM}",
    P + "find_similar_in": "h sc str limit mp >rows:u4[max(limit,1),3] >ntri:u4[max(limit,1)]",
    P + "find_batch_similar_each_in": f"{_EACH} {_NEEDLES} n limit mp {_SIM}",
    P + "find_references_similar_each_in": f"{_EACH} refs:u4[n] n limit mp {_SIM} >ntri:u4[n]",
    P + "find_batch_above_in": f"h sc {_NEEDLES} n mm mp ~rows:u4[cap,3] cap >row_off:u8[n+1]",
    P + "find_above_in": "h sc str mm mp ~rows:u4[cap,3] cap &",
    P + "find_batch_above_each_in": f"{_EACH} {_NEEDLES} n mm mp ~rows:u4[cap,3] cap >row_off:u8[n+1]",
    P + "find_references_above_each_in": f"{_EACH} refs:u4[n] n mm mp ~rows:u4[cap,3] cap >row_off:u8[n+1] >ntri:u4[n]",
    P + "cluster": "h refs:u4[n] n mp >labels:u4[n] & &",
    P + "cluster_levels": "h refs:u4[n] n floors:u4[k] k >labels:u4[k,n] >n_clusters:u4[k] >n_edges:u8[k]",
    P + "cluster_centres": "h refs:u4[n] n mp >labels:u4[n] >degrees:u4[n] >centres:u4[n] >attached:u1[n] & &",
    P + "cluster_cores": "h refs:u4[n] n mp md >labels:u4[n] >degrees:u4[n] >kinds:u1[n] & & &",
    P + "cluster_extend": "h old:u4[n1] seeds:u4[n1] n1 new:u4[n2] n2 mp >labels_old:u4[n1] >labels_new:u4[n2] & &",
    P + "cluster_within": "h refs:u4[n] keys:u4[n] n mp >labels:u4[n] & &",
    P + "cluster_extend_within": "h old:u4[n1] old_keys:u4[n1] seeds:u4[n1] n1 new:u4[n2] new_keys:u4[n2] n2 mp "
                                 ">labels_old:u4[n1] >labels_new:u4[n2] & &",
    P + "cluster_cores_within": "h refs:u4[n] keys:u4[n] n mp md >labels:u4[n] >degrees:u4[n] >kinds:u1[n] & & &",
    P + "cluster_tree": "h refs:u4[n] n mp >labels:u4[n] >merges:u4[n,3] & & &",
    P + "cluster_tree_extend": "h old:u4[n1] n1 records:u4[nr,3] nr new:u4[n2] n2 mp >labels_old:u4[n1] "
                               ">labels_new:u4[n2] >merges:u4[n1+n2,3] & & &",
    P + "cluster_core_tree": "h refs:u4[n] n mp md >labels:u4[n] >core:u4[n] >merges:u4[n,3] & & & &",
    P + "cluster_tree_within": "h refs:u4[n] keys:u4[n] n mp >labels:u4[n] >merges:u4[n,3] & & &",
    P + "cluster_core_tree_within": "h refs:u4[n] keys:u4[n] n mp md >labels:u4[n] >core:u4[n] >merges:u4[n,3] & & & &",
    P + "cluster_edges": "h refs:u4[n] n mp ~rows:u4[cap,3] cap &",
    P + "cluster_edges_within": "h refs:u4[n] keys:u4[n] n mp ~rows:u4[cap,3] cap &",
    P + "cluster_edges_extend": _TWO, P + "cluster_edges_between": _TWO,
}
RETURNS = {P + "put": 5, P + "delete": 1, P + "put_many": 7, P + "get": 3}       # (everything else answers 0)


def show(x):
    """A value as JSON holds it: arrays as dtype, shape and contents (a checksum for a large one)."""
    if isinstance(x, C.Array):                                             # (a buffer of characters or of rows: its size)
        plain = not issubclass(x._type_, (C.c_char, C.Structure))
        return {"ctypes": type(x).__name__, "values": list(x)} if plain else {"ctypes": type(x).__name__}
    if isinstance(x, np.ndarray):
        a = x
        body = a.tolist() if a.size <= 256 else "crc32 %08x" % zlib.crc32(np.ascontiguousarray(a).tobytes())
        return {"dtype": str(a.dtype), "shape": list(a.shape), "data": body}
    if isinstance(x, np.generic):
        return {"dtype": str(x.dtype), "value": x.item()}
    if isinstance(x, bytes):
        return {"bytes": x.decode("latin1")}
    if isinstance(x, (list, tuple)):
        return {"tuple": [show(v) for v in x]} if isinstance(x, tuple) else [show(v) for v in x]
    if isinstance(x, dict):
        return {str(k): show(v) for k, v in x.items()}
    if isinstance(x, Scope):
        return "Scope"
    if x is None or isinstance(x, (bool, int, str)):
        return x
    return repr(x) if isinstance(x, float) else f"<{type(x).__name__}>"


def _view(address, dtype, shape):
    size = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    return np.frombuffer((C.c_char * size).from_address(address), dtype=dtype).reshape(shape)


class Recorder:
    """Stands where the library stands: every entry point records what it is handed and answers canned values."""

    def __init__(self):
        self.calls, self.seen, self.grown, self.fail, self.scopes = [], set(), set(), False, 1000

    def __getattr__(self, symbol):
        if symbol not in SPEC:
            raise AttributeError(symbol)
        return lambda *args: self._call(symbol, args)

    def _call(self, symbol, args):
        spec = SPEC[symbol].split()
        assert len(spec) == len(args), (symbol, len(spec), len(args))
        self.seen.add(symbol)
        env = {"max": max}
        for tok, a in zip(spec, args):                                   # scalars first: the shapes are made of them
            if tok.isidentifier() and tok not in ("h", "sc", "str", "arr", "packed"):
                env[tok] = int(a)
        shown, arrays, refs = [], {}, []
        for tok, a in zip(spec, args):
            if tok == "h":
                shown.append("map" if isinstance(a, C.c_void_p) else show(a))
            elif tok == "sc":
                shown.append(f"scope {a.value}")
            elif tok == "&":
                refs.append(a._obj)
                shown.append("&" + type(a._obj).__name__)
            elif tok == "str":
                shown.append(show(a))
            elif tok == "arr":
                shown.append("NULL" if a is None else show(a))
            elif tok == "packed":
                shown.append(None)                                         # (after its offsets, below)
            elif ":" in tok:
                name, dtype, shape = re.fullmatch(r"[>~]?(\w+):(\w+)\[(.*)\]", tok).groups()
                shape = eval(f"({shape},)", env)
                if a is None:
                    shown.append("NULL")
                elif tok[0] == "~":
                    arrays[name] = (a, dtype, shape)
                    shown.append({"dtype": str(np.dtype(dtype)), "shape": list(shape), "data": "uninitialised"})
                else:
                    arrays[name] = (a, dtype, shape)
                    shown.append(show(_view(a, dtype, shape)))
            else:
                shown.append(env[tok])
        if "packed" in spec:
            at, a = spec.index("packed"), args[spec.index("packed")]
            size = int(_view(*arrays["offsets"])[-1])
            shown[at] = "NULL" if a is None else {"bytes": bytes(_view(a, "u1", (size,))).decode("latin1")}
        self.calls.append({"symbol": symbol, "args": shown})
        return self._answer(symbol, spec, args, env, arrays, refs)

    def _answer(self, symbol, spec, args, env, arrays, refs):
        if self.fail:
            C.set_errno(errno.EINVAL)
            return -1
        for tok in spec:                                                  # every output filled, offsets ascending
            if tok[0] in ">~" and tok[1:].split(":")[0] in arrays:
                name = tok[1:].split(":")[0]
                out = _view(*arrays[name])
                if out.size <= 1 << 16:
                    out.reshape(-1)[:] = np.arange(out.size) * 2 if name == "row_off" else np.arange(out.size) % 3
        for k, obj in enumerate(refs):                                    # counters 2, 3, 4 ...; a new scope's handle
            if isinstance(obj, C.c_void_p):
                self.scopes += symbol.endswith("scope_new")
                obj.value = self.scopes if symbol.endswith("scope_new") else None
            elif isinstance(obj, _native.TrigramStat):
                obj.references, obj.trigrams = 3, 50
            elif not isinstance(obj, C.Structure):
                obj.value = 2 + k
        if symbol == P + "last_kernels":
            if symbol not in self.grown:                                  # once: a list longer than the buffer
                self.grown.add(symbol)
                return 600
            args[1].value = b"find_kernel+select_kernel"
            return len(args[1].value)
        if symbol in (P + "find", P + "find_in"):
            k = min(max(env["limit"], 1), 2)
            for i in range(k):
                args[-1][i].reference, args[-1][i].matches, args[-1][i].weight = 7 + i, 5 - i, i
            return k
        if symbol in (P + "find_similar", P + "find_similar_in"):
            return min(max(env["limit"], 1), 2)
        if "cap" in env and symbol != P + "get":                          # the growing entries: rows, cap and a needed count
            rows = arrays.get("rows")
            needed = min(env["cap"], 4) if rows else 4
            if rows and symbol not in self.grown:                         # once each: ERANGE, five more needed
                self.grown.add(symbol)
                needed = env["cap"] + 5
                C.set_errno(errno.ERANGE)
            if "row_off" in arrays:
                off = _view(*arrays["row_off"])
                needed = max(needed, int(off[-1])) if needed > env["cap"] else int(off[-1])
                off[-1] = needed
            else:
                refs[-1].value = needed
            return -1 if needed > env["cap"] else 0
        return RETURNS.get(symbol, 0)


REFS = [3, 1, 4, 1, 5]                                                   # (every list of BASE that goes with another has five)
PACKED = _pack([b"abc", b"", b"san jose", b"a", b"san jose"])
U32 = lambda v: np.array(v, dtype=np.uint32)
BASE = dict(needle="san jose", limit=10, reference=7, weight=2, references=REFS, min_permille=500, min_degree=2,
            min_matches=1, blocks=[1, 1, 2, 1, 2], capacity=None, floors=[300, 600], attached=True, old_refs=[1, 2, 3],
            old_labels=[1, 1, 3], labels_old=[1, 1, 1], new_refs=[8, 9], old_merges=[[1, 2, 700]], left=[1, 2, 3],
            old_blocks=[1, 1, 2], new_blocks=[1, 2],
            right=[8, 9], scope="held", scopes=["held", "list"], which=[0, None, 1, 1, None], packed=PACKED[0], offsets=PACKED[1],
            needles=["São Paulo", "", "abc", "A b\tC", "é"], refs=U32(REFS), weights=None, path="/nonexistent/blurrily.trigrams",
            key="one_taken", value=1, enabled=True, n=3, labels=[1, 1, 4, 1, 5], merges=[[1, 4, 800], [1, 5, 600]],
            floor=700, core_permille=[900, 800, 900, 800, 0xFFFFFFFF], edges=[[1, 3, 900], [1, 4, 800]], nodes=None,
            record_lists=([[1, 3, 900]], [[1, 4, 800]]))
_MERGES = [[], [[2, 1, 700]], [[1, 2, 1001]], [[1, 2, 9], [1, 3, 8], [2, 3, 7], [1, 2, 6]], U32([[1, 3, 900]]),
           [[1, 2]], [[1, 2, -1]], np.array([[1, 2, 700]], dtype=np.int64), [[1, 2, 700], [1, 3, 900]]]
_LIST = [[], [7], U32(REFS), np.array(REFS, dtype=np.int64), np.array(REFS, dtype=np.uint8), np.array(REFS, dtype=np.float64),
         [[1, 2]], U32([[1, 2], [3, 4]]), [-1], [1 << 32], U32([]), U32(np.arange(10))[::2], (3, 1)]
_PERMILLE = [0, 1, 1000, 1001, -1, 1 << 32]
_KEYS = [[1] * 4, [1] * 6, [1, 2, 3, 4, 1 << 32], [1, 2, 3, 4, -1], U32([1, 1, 2, 1, 2]), []]
# per parameter, the values tried in its place (a dict sets several parameters at once), the others at BASE
GRID = dict(
    limit=[-(1 << 31) - 1, -1, 0, 1, 10, 65535, 65536, 70000, 1 << 31, (1 << 32) - 1, 1 << 32],
    needle=["", "a", b"by\xfftes", "São Paulo", "A b\tC"], reference=[0, -1, 0xFFFFFFFF, 1 << 32],
    weight=[0, -1, 1 << 32, None], references=_LIST, old_refs=_LIST[:1] + _LIST[6:10], new_refs=_LIST[:4] + _LIST[6:10],
    left=_LIST[:3] + _LIST[8:10], right=_LIST[:3] + _LIST[8:10], old_labels=[[], [1, 1], [1, 1, 1, 1], [1, 1, -1], U32([1, 1, 3])],
    labels_old=[[], [1, 1], U32([1, 2, 3])], min_permille=_PERMILLE, floor=_PERMILLE, min_matches=[0, 5, -1, 1 << 32],
    min_degree=[0, 1, 0xFFFFFFFF, -1, 1 << 32], blocks=_KEYS + [None], old_blocks=[[], [1] * 4, [1, 2, -1], U32([1, 1, 2])],
    new_blocks=[[], [1], [1, 1 << 32], U32([1, 2])], capacity=[None, 0, 3, 2000, 1 << 64, -1],
    floors=[[], [500], [100 * k for k in range(1, 10)], [500, 500], [600, 300], [1001], [0, 1000]], attached=[False],
    old_merges=_MERGES, merges=_MERGES, edges=_MERGES, record_lists=[(), (_MERGES[3],), (_MERGES[8], _MERGES[8])],
    scope=["held", "list", "empty", "array", "foreign", "closed"],
    scopes=[[], ["held"], ["list"], ["held", "foreign"], ["closed", "held"], ["empty", "array", "held"]],
    which=[[0, 1], [0] * 6, U32([0, 1, 0, 1, 0]), [None] * 5, [0, -1, 1, 1, 1], [0, 1 << 32, 1, 1, 1]],
    packed=[dict(zip(("packed", "offsets"), _pack([]))) | {"which": []}, dict(zip(("packed", "offsets"), _pack([b""] * 5))),
            dict(packed=np.frombuffer(PACKED[0], dtype=np.uint8)), dict(offsets=PACKED[1].tolist()),
            dict(offsets=PACKED[1].astype(np.int64))],
    needles=[[""] * 5, [b"by\xfftes", "é", "x", "y", "z"], dict(needles=[], which=[]), dict(needles=["abc"], which=[None])],
    weights=[REFS, U32(REFS)], labels=[[], [1, 1], U32([1, 1, 4, 1, 5]), [1, 1, 4, 1, 0xFFFFFFFF]],
    core_permille=[[], [900], U32([0, 0, 0, 0, 0])], nodes=[0, 9], key=["", "no_such_option"], value=[0, -1, 1 << 40],
    enabled=[False, 0], n=[0, 1], path=["", b"/nonexistent/bytes"])
EMPTY = dict(references=[], blocks=[], old_refs=[], old_labels=[], labels_old=[], new_refs=[], old_merges=[], left=[], right=[],
             scopes=[], which=[], packed=b"", offsets=[0], needles=[], refs=U32([]), labels=[], merges=[], core_permille=[],
             edges=[], record_lists=(), floors=[], scope="empty", old_blocks=[], new_blocks=[])
# put_many trusts its lists to be of one length: a grid over one of them alone would have the library read past the other
ALONE = {("put_many", "references"), ("put_many", "needles"), ("put_many_packed", "packed")}
LAST = ("close",)                                                        # (a map is closed after everything else)


class Driver:
    def __init__(self, out):
        self.out, self.rec, self.driven, self.made = out, Recorder(), 0, 0

    def target(self, cls):
        """An object of `cls` over the recorder, with a held and a closed scope of its own and a scope of another map."""
        obj, other = cls(), cls()
        obj._lib = other._lib = self.rec
        named = {"held": obj.scope([1, 2, 3]), "closed": obj.scope([1]), "foreign": other.scope([1, 2]),
                 "list": [2, 3, 2], "empty": [], "array": U32([5, 6])}
        named["closed"].close()
        return obj, named

    def drive(self, what, fn, kwargs, named):
        sig = inspect.signature(fn)
        args, kw = [], {}
        for p in sig.parameters.values():
            v = kwargs[p.name]
            if p.name in ("scope", "scopes"):                             # (by name: the objects are the target's own)
                v = named[v] if p.name == "scope" else [named[s] for s in v]
            if p.kind == p.VAR_POSITIONAL:
                args += list(v)
            else:
                kw[p.name] = v
        self.rec.calls = []
        line = {"call": what, "args": {k: show(v) for k, v in kwargs.items() if k in sig.parameters}}
        try:
            got = fn(*args, **kw)
            if isinstance(got, Scope):                                   # (closed at once: nothing left to the collector)
                got.close()
            line["returned"] = show(got)
        except Exception as e:                                            # noqa: BLE001 -- whatever is raised is the record
            line["raised"] = [type(e).__name__, str(e)]
        line["c_calls"] = self.rec.calls
        self.driven, self.made = self.driven + 1, self.made + len(self.rec.calls)
        self.out.write(json.dumps(line, sort_keys=True) + "\n")

    def methods(self, obj):
        names = [n for n in sorted(dir(type(obj))) if not n.startswith("_") and n not in LAST
                 and inspect.isroutine(getattr(type(obj), n))]
        return [(n, getattr(obj, n)) for n in names + [n for n in LAST if hasattr(obj, n)]]

    def all_of(self, cls):
        obj, named = self.target(cls)
        for name, fn in self.methods(obj):
            if name in LAST:
                continue
            params = [p for p in inspect.signature(fn).parameters]
            base = {p: BASE[p] for p in params}
            what = f"{cls.__name__}.{name}"
            bases = [base] + ([base | {"blocks": None}] if "capacity" in params else [])   # (cluster_edges' two symbols)
            for base in bases:
                self.drive(what, fn, base, named)
                for p in params:
                    for v in GRID.get(p, []) if (name, p) not in ALONE else []:
                        self.drive(what, fn, base | (v if isinstance(v, dict) else {p: v}), named)
            base = bases[0]
            if set(params) & set(EMPTY):
                self.drive(what + " (nothing listed)", fn, base | {p: EMPTY[p] for p in params if p in EMPTY}, named)
            self.rec.fail = True                                          # the library refuses: EINVAL
            self.drive(what + " (refused)", fn, base, named)
            self.rec.fail = False
        for label in ("held", "closed", "foreign"):                       # the scopes' own surface
            for name, fn in self.methods(named[label]):
                self.drive(f"{cls.__name__} {label} Scope.{name}", fn, {}, named)
        held = obj.scope([4])
        self.drive(f"{cls.__name__}.close", obj.close, {}, named)
        for of, what in ((obj, f"closed {cls.__name__}."), (held, f"closed {cls.__name__}'s Scope.")):
            for name, fn in self.methods(of):
                self.drive(what + name, fn, {p: BASE[p] for p in inspect.signature(fn).parameters}, named)
        held.close()


def signatures(out):
    for cls in (RawMap, Map, Scope):
        for name in sorted(n for n in dir(cls) if not n.startswith("_")):
            attr, static = getattr(cls, name), inspect.getattr_static(cls, name)
            sig = str(inspect.signature(attr)) if callable(attr) and not inspect.isclass(attr) else ""
            out.write(json.dumps({"signature": f"{cls.__name__}.{name}{sig}", "kind": type(static).__name__}) + "\n")
    out.write(json.dumps({"blurrily_amd.map": sorted(n for n in dir(map_module) if not n.startswith("_"))}) + "\n")


def main():
    out = sys.stdout
    signatures(out)
    d = Driver(out)
    for cls in (RawMap, Map):
        d.all_of(cls)
    source = "".join(open(f).read() for f in glob.glob(os.path.join(os.path.dirname(map_module.__file__), "*.py"))
                     if os.path.basename(f).startswith(("map.", "map_clusters.", "_marshal.")))
    named = set(re.findall(r"blurrily_(?:storage|scope)_\w+", source)) & set(_native._ENTRIES)
    out.write(json.dumps({"driven": d.driven, "c_calls": d.made, "symbols_called": len(d.rec.seen),
                          "never_called": sorted(named - d.rec.seen)}) + "\n")


if __name__ == "__main__":
    main()
