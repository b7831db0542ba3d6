"""The map tests/test_gpu_dense_cluster_trees.py runs the three tree entries on: tests/dense_case.py's held strings and
weights unchanged, and from reference 300 000 on five chain families.  dense_case.py's families are six-member
near-cliques, each one component after the first Boruvka round at every floor, so on that map nothing with a left-out
slice or a 16-bit half window ever runs a tree's later rounds.  A chain is a sliding window: for each width of
dense_case.FAMILY_WORDS (12, 25, 45, 70, 110), width + 11 random words of the haystack, and twelve members held, member
i being words [i, i + width) joined by spaces.  Neighbours are the most alike, members two or three apart are still above
the lower floors, and a chain needs two or three merging rounds on its own.  The chain members' weights are random from a
fixed seed, so they fall into both windows and both halves of the first.

`host()` is numpy and Oracle.tokenise only; `build()` adds the map.  tests/test_dense_tree_case.py proves on the host the
conditions the GPU tests lean on.  If a re-seeded generator ever breaks one of them, change the seeds, not the
assertion."""
from types import SimpleNamespace

import numpy as np

import dense_case as D
import dense_truths as DT
from cluster_tree_within_truth import BlockedTruth

CHAIN_REF0 = 300000
CHAIN_MEMBERS = 12
CHAIN_SEED, WEIGHT_SEED = 71, 29


def chain_of(words, width):
    return [b" ".join(words[i:i + width]) for i in range(CHAIN_MEMBERS)]


def key_chains(refs):
    """dense_truths.key_families with each chain under a key of its own (100 + its index)."""
    refs = np.asarray(refs, dtype=np.uint32)
    chain = refs >= CHAIN_REF0
    return np.where(chain, 100 + (refs - np.where(chain, CHAIN_REF0, 0)) // CHAIN_MEMBERS,
                    DT.key_families(np.where(chain, 0, refs))).astype(np.uint32)


_HOST = {}


def host():
    """dense_case.Host over both; .chains: the five chains' first references, .chain(first): its twelve."""
    if "h" in _HOST:
        return _HOST["h"]
    base = D.host()
    words = base.strings[:D.N_WORDS]
    held = dict(base.held)
    rng = np.random.default_rng(CHAIN_SEED)
    chains, ref = [], CHAIN_REF0
    for width in D.FAMILY_WORDS:
        chains.append(ref)
        drawn = [words[int(i)] for i in rng.integers(0, D.N_WORDS, size=width + CHAIN_MEMBERS - 1)]
        for s in chain_of(drawn, width):
            held[ref] = s
            ref += 1
    assert int(base.refs[-1]) < CHAIN_REF0                        # (the chains sort behind: the held weights keep their places)
    more = np.random.default_rng(WEIGHT_SEED).integers(1, 1 << 20, size=ref - CHAIN_REF0).astype(np.uint32)
    h = D.Host(held, np.concatenate([base.weights, more]), base.heads, D.DENSE_MIN)
    h.chains = chains
    h.chain = lambda first: list(range(first, first + CHAIN_MEMBERS))
    h.members = np.array([r for first in chains for r in h.chain(first)], dtype=np.uint32)
    assert all(h.held[int(r)] == base.held[int(r)] for r in base.refs[::997]) and len(h.refs) == len(base.refs) + len(h.members)
    D.assert_inputs(h)
    _HOST["h"] = h
    return h


def position(h, ref):
    """Where a reference lies in the sweep's order: an edge is found from its end at the higher position."""
    w, r = h.loc[int(ref)]
    return w * D.WINDOW_RANKS + r


def inputs(h):
    """dense_truths.inputs on the larger map -- the pair, p_star, the floors, the family -- with the 60 chain references
    appended to both lists."""
    c = DT.inputs(h)
    c.lists = {name: np.concatenate([listed, h.members]) for name, listed in c.lists.items()}
    c.chains = h.members
    # the first two members of the widest chain: neighbours, so an edge at every floor used, under different parities
    c.parity_edge = (h.chains[-1], h.chains[-1] + 1)
    return c


def handmade_expectations(c):
    """What dense_truths.handmade() must give, from m = 6, T = 12, R = 6 (the glued string and a copy meet at exactly
    500, the copies each other at 1000): tree {floor: records}, core {(floor, min_degree): {reference: core height}},
    own_key (the glued string under a key of its own)."""
    NO_CORE = 0xFFFFFFFF
    copies = list(range(2, 72))
    among = [[2, r, 1000] for r in copies[1:]]                    # the 69 records at 1000, in the total order
    rest = {100: NO_CORE, 101: NO_CORE}

    def core(glued, copy):
        return {1: glued, **{r: copy for r in copies}, **rest}

    return SimpleNamespace(
        tree={500: among + [[1, 2, 500]], 501: among},
        # a copy's edges: 69 at 1000 and, at floor 500, one at 500; the glued string's: 70 at 500, none at 501 -- so at
        # (500, 69) its 69th largest is 500, and it is without a core height beside copies at 1000 only at (501, 69)
        core={(500, 70): core(500, 500), (500, 69): core(500, 1000), (501, 69): core(NO_CORE, 1000),
              (501, 70): core(NO_CORE, NO_CORE)},
        own_key=(np.asarray(c.refs) == 1).astype(np.uint32))


CORE_HIGH = 1001 - 32                                          # from here on the core heights take one sweep, below it two


def core_cases(c):
    """The (floor, min_degree) of the core tree: five whose first bracket of heights takes two sweeps and one that takes
    one."""
    return ((200, 2), (200, 4), (350, 3), (600, 2), (c.p_star, 5), (CORE_HIGH, 2))


def truths(h, c):
    """name -> a cluster_truth.Truth per list (a Truth keeps one list's pairs), the tokenisation shared."""
    import copy
    kept = {}

    def truth(name):
        if name not in kept:
            kept[name] = copy.copy(h.truth)
            kept[name]._pairs = {}
        return kept[name]

    return truth


def blocked_on(truth, listed, blocks):
    """cluster_tree_within_truth.blocked(held, listed, blocks) over a Truth that has tokenised the held strings already:
    its BlockedTruth with the tokenisation shared, and the pairs that `truth` keeps at this moment (of the same list, if
    it has been asked: BlockedTruth.pairs() filters those; whatever either is asked later is its own)."""
    b = BlockedTruth.__new__(BlockedTruth)
    b.__dict__ = dict(truth.__dict__)
    key_of = dict(zip(np.asarray(listed).tolist(), np.asarray(blocks).tolist()))
    b.key = np.array([key_of.get(int(r), -1 - i) for i, r in enumerate(b.refs)], dtype=np.int64)   # (unlisted: a key of its own)
    return b


def build():
    """(the map, the Host).  The caller closes the map."""
    from blurrily_amd import RawMap
    from blurrily_amd.map import _pack
    h = host()
    m = RawMap()
    m.set_option("dense_min", D.DENSE_MIN)                       # before the first put: changing it later forces a rebuild
    m.put_many_packed(*_pack(h.strings), h.refs, h.weights)
    m.sync_device()
    info = m.device_info()
    assert info["n_windows"] == 2, info["n_windows"]
    assert info["n_bitmaps"] >= h.n_dense_pairs() > 1000, (info["n_bitmaps"], h.n_dense_pairs())
    return m, h
