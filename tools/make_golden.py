#!/usr/bin/env python3
"""Generate tests/golden/ref_*.json from the reference's own C compiled in place (and its headers).

Runs only where the reference tree is ($BLURRILY_REF_EXT, default /root/reference/ext/blurrily; oracle/_ref
must be built: `make -C oracle`).  The fixtures are data -- seeded inputs, or the seeds they are rebuilt from
(tests/helpers.py), and the outputs the reference produced for them -- so that no test needs the reference tree.

    python tools/make_golden.py

How a haystack reaches the reference: this repo's blurrily_storage_put/save write a
`.trigrams` file; the reference's blurrily_storage_load maps it (oracle/ref_shim.c).  The
reference's find and tokeniser then produce the expected values stored here.
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import workloads as W  # noqa: E402
from blurrily_amd import RawMap  # noqa: E402
import helpers as H  # noqa: E402
from helpers import GOLDEN, Reference, golden_haystack  # noqa: E402

REF_EXT = os.environ.get("BLURRILY_REF_EXT", "/root/reference/ext/blurrily")
# the gem's own flags (ext/blurrily/extconf.rb:4-13)
REF_FLAGS = ["-std=c99", "-DPLATFORM_LINUX", "-D_XOPEN_SOURCE=700", "-D_GNU_SOURCE=1", "-D_FILE_OFFSET_BITS=64"]


def case(name, kind, n, hay_seed, q_seed, n_q, limit, refs="seq", weights="zero"):
    meta = {"kind": kind, "n": n, "seed": hay_seed, "refs": refs, "weights": weights, "ref_seed": hay_seed}
    hay, off, ref_arr, w_arr = golden_haystack(meta)
    m = RawMap()
    m.put_many_packed(hay, off, ref_arr, w_arr)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "h.trigrams")
        m.save(path)
        ref = Reference(path)
        q, qo = W.queries(hay, off, n_q, q_seed)
        needles = W.unpack(q, qo) + [b"", b"zzzz", b"a", b"the quick brown fox"]
        expected = [ref.find(nd, limit) for nd in needles]
        stats = ref.stats()
        ref.close()
    out = {
        "generator": "tools/make_golden.py (reference C: oracle/_ref/libblurrily_ref.so)",
        "haystack": meta,
        "stats": stats, "limit": limit,
        "needles_hex": [nd.hex() for nd in needles],
        "expected": expected,
    }
    with open(os.path.join(GOLDEN, f"ref_find_{name}.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(name, len(needles), "needles")


def tokeniser_vectors():
    rng = np.random.default_rng(42)
    needles = [b"", b"london", b"new york", b"a", b"aa", b"aaa", b"aaaa", b"port au prince", b"  ", b"a  b",
               b"Mixed CASE", b"caf\xc3\xa9", b"***", b"z" * 40, b"abcdefghijklmnopqrstuvwxyz" * 6]
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz  *-AZ\xc3\xa9", dtype=np.uint8)
    for _ in range(200):
        ln = int(rng.integers(0, 40))
        needles.append(bytes(rng.choice(alphabet, size=ln).tolist()).replace(b"\0", b"a"))
    out = {"generator": "tools/make_golden.py (blurrily_tokeniser_parse_string of the reference)",
           "vectors": [{"needle_hex": nd.hex(), "codes": Reference.tokenise(nd)} for nd in needles]}
    with open(os.path.join(GOLDEN, "ref_tokeniser.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("tokeniser", len(needles), "vectors")


def _reference_answers(m, needles, limit):
    """Save m, load the file with the reference, find every needle: (stats, digests of the rows)."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "h.trigrams")
        m.save(path)
        ref = Reference(path)
        out = ref.stats(), [H.rows_digest(ref.find(nd, limit)) for nd in needles]
        ref.close()
    return out


def recorded():
    """tests/golden/ref_recorded.json: the reference's answers for the seeded inputs of tests/helpers.py."""
    out = {"generator": "tools/make_golden.py (reference C: oracle/_ref/libblurrily_ref.so)",
           "digests": "tests/helpers.py: rows_digest, codes_digest",
           "tokeniser": [H.codes_digest(Reference.tokenise(nd)) for nd in H.tokeniser_needles()]}
    for key, cases, inputs in (("oracle_cases", H.ORACLE_CASES, H.oracle_case_inputs),
                               ("hip_cases", H.HIP_CASES, H.hip_case_inputs)):
        out[key] = {}
        for kind, n, limit in cases:
            hay, off, needles = inputs(kind, n)
            m = RawMap()
            m.put_many_packed(hay, off, np.arange(1, n + 1, dtype=np.uint32))
            stats, digests = _reference_answers(m, needles, limit)
            out[key][H.case_key(kind, n, limit)] = {"stats": stats, "rows": digests}
            m.close()
            print(key, kind, n, len(needles), "needles")
    out["head_cases"] = {}
    for kind in ("geonames", "skewed"):
        hay, off, q, qo = H.head_case_inputs(kind)
        m = RawMap()
        m.put_many_packed(hay, off, np.arange(1, len(off), dtype=np.uint32))
        needles = W.unpack(q, qo)[:60]
        out["head_cases"][kind] = [_reference_answers(m, needles, limit)[1] for limit in H.HEAD_LIMITS]
        m.close()
    out["tiny_cases"] = []
    for entries, needle, limit in H.tiny_haystack_cases():
        m = RawMap()
        for i, (s, w) in enumerate(entries):
            m.put(s, i + 1, w)
        stats, digests = _reference_answers(m, [needle] + [s for s, _ in entries[:5]], limit)
        out["tiny_cases"].append({"stats": stats, "rows": digests})
        m.close()
    m = H.resave_haystack()
    with tempfile.TemporaryDirectory() as d:
        ours, theirs = os.path.join(d, "ours.trigrams"), os.path.join(d, "theirs.trigrams")
        m.save(ours)
        ref = Reference(ours)
        stats = ref.stats()
        assert ref.save(theirs) == 0
        ref.close()
        out["resave"] = {"stats": stats, "md5": hashlib.md5(open(theirs, "rb").read()).hexdigest()}
    with open(os.path.join(GOLDEN, H.RECORDED), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("recorded", len(out["tiny_cases"]), "tiny cases")


def abi():
    """tests/golden/ref_abi.json: what the tests hold this repository's header and Ruby glue to -- the nine
    prototypes of the reference's storage.h as gcc prints them (-aux-info), the types its typedefs name, the
    layout of its result row and stats, and the methods the gem's Init_map_ext defines (map_ext.c)."""
    with tempfile.TemporaryDirectory() as d:
        src, info, exe = os.path.join(d, "abi.c"), os.path.join(d, "abi.txt"), os.path.join(d, "abi")
        layout = ["sizeof(trigram_match_t)", "offsetof(trigram_match_t, reference)", "offsetof(trigram_match_t, matches)",
                  "offsetof(trigram_match_t, weight)", "sizeof(trigram_stat_t)", "offsetof(trigram_stat_t, references)",
                  "offsetof(trigram_stat_t, trigrams)"]
        typedefs = {"trigram_map": "struct trigram_map_t*", "trigram_match": "struct trigram_match_t*",
                    "trigram_match_t": "struct trigram_match_t", "trigram_stat_t": "struct trigram_stat_t"}
        body = ['#include "storage.h"', "#include <stddef.h>", "#include <stdio.h>"]
        body += [f"typedef char td_{i}[__builtin_types_compatible_p({a}, {b}) ? 1 : -1];"
                 for i, (a, b) in enumerate(typedefs.items())]
        body.append("int main(void) {")
        body += [f'  printf("%zu\\n", (size_t)({e}));' for e in layout]
        body.append("  return 0; }")
        open(src, "w").write("\n".join(body) + "\n")
        subprocess.run(["gcc", *REF_FLAGS, "-I", REF_EXT, "-aux-info", info, "-o", exe, src], check=True)
        values = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
        prototypes = [re.sub(r"^/\*.*?\*/\s*", "", ln).strip() for ln in open(info)
                      if "/storage.h:" in ln and "blurrily_storage_" in ln]
    assert len(prototypes) == 9, prototypes
    glue = open(os.path.join(REF_EXT, "map_ext.c")).read()
    out = {"generator": "tools/make_golden.py (gcc -aux-info over the reference's ext/blurrily/storage.h)",
           "prototypes": prototypes, "typedefs": typedefs,
           "layout": {k: int(v) for k, v in zip(layout, values)},
           "gem_methods": re.findall(r'rb_define_method\(klass,\s*"(\w+)"', glue),
           "gem_initialiser": "void Init_map_ext(void)" if re.search(r"\bvoid\s+Init_map_ext\s*\(\s*void\s*\)\s*\{", glue)
           else None}
    assert out["gem_initialiser"] and out["gem_methods"]
    with open(os.path.join(GOLDEN, H.ABI), "w") as f:
        json.dump(out, f, indent=1)
    print("abi", len(prototypes), "prototypes,", len(out["gem_methods"]), "gem methods")


if __name__ == "__main__":
    assert Reference.available(), "build oracle/_ref first (make -C oracle) -- needs /root/reference"
    os.makedirs(GOLDEN, exist_ok=True)
    tokeniser_vectors()
    case("words3k", "words", 3000, 21, 22, 120, 10)
    case("words3k_limit100", "words", 3000, 21, 23, 40, 100)
    case("geo20k", "geonames", 20000, 31, 32, 120, 10)
    case("skewed_ties", "skewed", 8000, 41, 42, 80, 25, refs="sparse", weights="small")
    recorded()
    abi()
