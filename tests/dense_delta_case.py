"""The map tests/test_gpu_dense_delta_*.py run every sweep on: tests/dense_case.py's held strings and weights unchanged as
the base image ("dense_min" 64 set before the first put, then sync_device()), and on top of it a fixed list of mutations
that leaves a delta image with dense slices of its own and tombstones behind the base image's bitmaps.  The other dense
files build their maps with one bulk put, so every sweep of theirs runs on the base image with an empty log; the suite's
delta-image and tombstone tests put a few strings under the default "dense_min", so their delta image has no bitmap at
all.  Here the two meet.

The files that run on it: tests/test_gpu_dense_delta_finds.py and tests/test_gpu_dense_delta_plain_find.py (the finds),
tests/test_gpu_dense_delta_clusters.py (cluster, levels, centres, cores, within, extend),
tests/test_gpu_dense_delta_trees.py (the four tree entries), tests/test_gpu_dense_delta_edges.py (the edge lists: plain,
blocked, extend and between) and tests/test_gpu_dense_delta_blocked.py (cores, core tree and extend within blocks).

The mutations, in order (`Host.steps`; one generator, default_rng(83), throughout):

  pending phrases   150 of the 70 000 base words are the vocabulary; 3 000 phrases of three vocabulary words each, from
                    reference 400 000 on, random weights.  A small vocabulary is what makes a delta dense.
  delta families    two dense_case.family_of families each of 12, 25, 45, 70 and 110 distinct vocabulary words, six members
                    a family, from reference 500 000 on: every head has more than 64 dense slices in the delta's one window.
  tombstones        of a narrow and of a wide base family the head's twin (head + 1: its matches with the head include all
                    of the head's left-out slices), and every 233rd base word.
  moved rows        of two other base families head + 2 is deleted and put again as the head's text + b" moved" with a new
                    weight: a tombstoned base rank and a delta node whose neighbours sit behind the base's bitmaps.  One
                    more reference is put and deleted again (erased from the delta, no tombstone).
  the exact bar     tests/dense_truths.py's hand-made case as pending puts: seventy copies of a word and, at the highest
                    delta position, the word glued to another; one copy is deleted again.  The word's six trigrams are the
                    glued string's only dense slices in the delta, its bar at floor 500 is 6 of its 12: L = t - 1.

`host()` is everything the host knows (numpy, Oracle.tokenise, cluster_truth.Truth; nothing of the library): what is held
now, and each image's layout -- the base's as built (deleted ranks stay in its postings and bitmaps), the delta's
dense_case.locate over the pending puts alone with postings by the same rule.  `build()` adds the map.
tests/test_dense_delta_case.py proves on the host the conditions the GPU files lean on.  If a re-seeded generator ever
breaks one of them, change the seed, not the assertion.

Not covered: a delta of more than one window, or with ranks of 32 768 and more, needs a base of 2.1 M / 4.2 M references
(the log's budget is a 64th of the base), which is too slow for this suite.  DeviceInfo.n_bitmaps counts the base image's
bitmaps only, so that the delta's are there is known from the host's postings alone."""
from types import SimpleNamespace

import numpy as np

import dense_case as D
import dense_truths as DT
from cluster_truth import Truth

SEED = 83
N_VOCAB, N_PHRASES, PHRASE_WORDS = 150, 3000, 3
PHRASE_REF0, FAMILY_REF0, HANDMADE_REF0, GONE_REF = 400000, 500000, 600000, 700000
FAMILIES_EACH = 2
WORDS_DELETED_EVERY = 233
TWIN_FAMILIES = (0, 9)                                         # base families (12 and 70 words) whose head + 1 is deleted
MOVED_FAMILIES = (3, 13)                                       # ... (25 and 110 words) whose head + 2 is deleted and put again
COPIES = 70
WORD, OTHER = b"klmno", b"pqrst"
TOP_WEIGHT = 1 << 20                                           # above every random weight: the highest position of its image
LOG_BUDGET = 4096                                              # map_log.hip: max(4096, n_refs / 64)
PAIR_FAMILY, PAIR_MEMBERS = 9, (4, 5)                          # the delta family (110 words) whose pair gives p*


class Host:
    """What the host knows of the mutated map.

    held {reference: string} and weight_of {reference: weight} as they should be now; refs (ascending), strings and
    weights side by side; truth (cluster_truth.Truth over held).  base: dense_case.host()'s Host, the base image as built.
    delta: a dense_case.Host over the pending puts alone (loc, postings, dense, dense_padded of the delta image).
    pending {reference: (string, weight)}; tombstones: the base references deleted since the build, in order; steps: the
    mutations as ("put", refs, strings, weights) / ("delete", refs)."""

    def __init__(self, base):
        self.base = base
        self.held = dict(base.held)
        self.weight_of = dict(zip(base.refs.tolist(), base.weights.tolist()))
        self.pending, self.tombstones, self.steps = {}, [], []

    # ---- the mutations, as the log of map_log.hip books them ----
    def put(self, refs, strings, weights):
        refs, weights = [int(r) for r in refs], [int(w) for w in weights]
        for r, s, w in zip(refs, strings, weights):
            assert r not in self.held and len(s) >= 1                # (a held reference's put is ignored: none here)
            self.held[r], self.weight_of[r], self.pending[r] = s, w, (s, w)
        self.steps.append(("put", np.array(refs, dtype=np.uint32), list(strings), np.array(weights, dtype=np.uint32)))

    def delete(self, refs):
        refs = [int(r) for r in refs]
        for r in refs:
            del self.held[r], self.weight_of[r]
            if self.pending.pop(r, None) is None:                   # never reached the base image: erased, no tombstone
                assert r in self.base.held and r not in self.tombstones
                self.tombstones.append(r)
        self.steps.append(("delete", np.array(refs, dtype=np.uint32)))

    def finish(self):
        self.refs = np.array(sorted(self.held), dtype=np.uint32)
        self.strings = [self.held[int(r)] for r in self.refs]
        self.weights = np.array([self.weight_of[int(r)] for r in self.refs], dtype=np.uint32)
        now = D.Host(self.held, self.weights, [], D.DENSE_MIN)      # (its loc and postings are of no image: dropped)
        self.truth, self._now = now.truth, now
        del now.loc, now.postings
        p_refs = sorted(self.pending)
        self.delta = D.Host({r: self.pending[r][0] for r in p_refs}, [self.pending[r][1] for r in p_refs],
                            self.delta_heads, D.DENSE_MIN)
        self.deleted = set(self.tombstones)
        self.base_windows = max(w for w, _ in self.base.loc.values()) + 1

    # ---- the strings ----
    def T(self, ref):
        return self._now.T(int(ref))

    def codes(self, ref):
        return self._now.codes(int(ref))

    def permille(self, a, b):
        return self._now.permille(int(a), int(b))

    def family(self, head):
        return list(range(head, head + D.MEMBERS))

    # ---- the images ----
    def image(self, ref):
        """0: a row of the base image, 1: of the delta image (a held reference)."""
        assert int(ref) in self.held
        return 1 if int(ref) in self.pending else 0

    def at(self, ref):
        """(image, window, in-window rank) of a held reference."""
        i = self.image(ref)
        return (i,) + (self.delta if i else self.base).loc[int(ref)]

    def position(self, ref):
        """Where a held reference lies in the sweeps' order -- the delta image behind the base's windows: an edge is
        found from its end at the higher position."""
        i, w, r = self.at(ref)
        return (i * self.base_windows + w) * D.WINDOW_RANKS + r

    def dense(self, ref, image, window=0):
        """The slices of a held reference's codes that are dense in a window of an image, by the index's rule (postings
        padded to a multiple of 8 reach "dense_min"; a base image's postings keep its deleted ranks)."""
        post = (self.delta if image else self.base).postings[window][self.codes(ref)]
        return int(((post + 7) // 8 * 8 >= D.DENSE_MIN).sum())


_HOST = {}


def host():
    if "h" in _HOST:
        return _HOST["h"]
    base = D.host()
    words = base.strings[:D.N_WORDS]
    assert int(base.refs[D.N_WORDS - 1]) == D.N_WORDS < D.FAMILY_REF0 <= int(base.refs[D.N_WORDS])
    h = Host(base)
    rng = np.random.default_rng(SEED)
    weights = lambda n: rng.integers(1, TOP_WEIGHT, size=n)

    # pending phrases
    vocab = [words[int(i)] for i in rng.choice(D.N_WORDS, N_VOCAB, replace=False)]
    phrases = [b" ".join(vocab[int(j)] for j in rng.integers(0, N_VOCAB, size=PHRASE_WORDS)) for _ in range(N_PHRASES)]
    h.phrases = np.arange(PHRASE_REF0, PHRASE_REF0 + N_PHRASES, dtype=np.uint32)
    h.put(h.phrases, phrases, weights(N_PHRASES))

    # delta families
    h.delta_heads, strings = [], []
    for k in D.FAMILY_WORDS:
        for _ in range(FAMILIES_EACH):
            h.delta_heads.append(FAMILY_REF0 + len(strings))
            strings += D.family_of([vocab[int(j)] for j in rng.choice(N_VOCAB, k, replace=False)])
    h.delta_family = np.arange(FAMILY_REF0, FAMILY_REF0 + len(strings), dtype=np.uint32)
    h.put(h.delta_family, strings, weights(len(strings)))

    # tombstones behind bitmaps
    h.base_heads = list(base.heads)
    h.base_family = np.array([r for x in base.heads for r in h.family(x)], dtype=np.uint32)
    h.twin_heads = [base.heads[k] for k in TWIN_FAMILIES]
    h.twins = [x + 1 for x in h.twin_heads]
    assert all(base.held[x] == base.held[x + 1] for x in h.twin_heads)
    h.delete(h.twins)
    h.words_deleted = base.refs[:D.N_WORDS][::WORDS_DELETED_EVERY].copy()
    h.delete(h.words_deleted)

    # moved rows, and a reference put and deleted again
    h.moved_heads = [base.heads[k] for k in MOVED_FAMILIES]
    h.moved = [x + 2 for x in h.moved_heads]
    h.delete(h.moved)
    h.put(h.moved, [base.held[x] + b" moved" for x in h.moved_heads], weights(len(h.moved)))
    h.put([GONE_REF], [vocab[0] + b" " + vocab[1]], weights(1))
    h.delete([GONE_REF])

    # the exact bar, in the delta
    glued = HANDMADE_REF0
    copies = np.arange(HANDMADE_REF0 + 1, HANDMADE_REF0 + 1 + COPIES, dtype=np.uint32)
    h.put(copies, [WORD] * COPIES, np.ones(COPIES, dtype=np.uint32))
    h.put([glued], [WORD + b" " + OTHER], [TOP_WEIGHT])
    h.copy_deleted = int(copies[COPIES // 2])
    h.delete([h.copy_deleted])
    h.handmade = SimpleNamespace(glued=glued, copies=copies, held_copies=copies[copies != h.copy_deleted],
                                 listed=np.concatenate([[glued], copies]).astype(np.uint32))
    h.finish()
    assert_inputs(h)
    _HOST["h"] = h
    return h


def assert_inputs(h):
    """The conditions on the inputs that every user of the map relies on (tests/test_dense_delta_case.py has the rest)."""
    assert len(h.pending) + len(h.tombstones) <= LOG_BUDGET, (len(h.pending), len(h.tombstones))
    assert len(h.pending) == N_PHRASES + len(h.delta_family) + len(h.moved) + COPIES
    assert len(h.tombstones) == len(h.twins) + len(h.words_deleted) + len(h.moved)
    assert max(w for w, _ in h.delta.loc.values()) == 0 and len(h.delta.loc) < D.HALF      # one window, its lower half
    assert all(h.delta.dense_padded(x, 0) > D.MAX_DENSE for x in h.delta_heads)
    assert any(h.T(x) <= 255 for x in h.delta_heads) and sum(h.T(x) > 255 for x in h.delta_heads) >= 3
    g = h.handmade
    assert h.delta.loc[g.glued][1] == len(h.pending) - 1           # the glued string at the delta's highest position
    assert (h.T(g.glued), h.T(int(g.copies[0]))) == (12, 6) and h.permille(g.glued, int(g.copies[0])) == 500
    assert set(h.codes(int(g.copies[0])).tolist()) < set(h.codes(g.glued).tolist())
    # the word's six are the glued string's only dense slices in the delta; its bar at floor 500 leaves five of them out
    post = h.delta.postings[0]
    assert h.delta.dense_padded(g.glued, 0) == 6 and ((post[h.codes(int(g.copies[0]))] + 7) // 8 * 8 >= D.DENSE_MIN).all()
    assert DT.floor_bar(12, 500) - 1 == 5 < 6


def inputs(h):
    """The lists, the floors and the wide delta pair whose permille p* gives the last two floors: lists {"short", "long",
    "handmade"} (`short`: the delta families, the base families -- their moved rows, which are nodes of the delta now, and
    their deleted twins among them -- and every 97th base word, deleted or not; `long`: with every pending phrase; a listed
    reference that is not held is no node), pair (low, high) by delta position, p_star, floors."""
    words = h.base.refs[:D.N_WORDS]
    short = np.concatenate([h.delta_family, h.base_family, words[::97]])
    assert set(h.moved) | set(h.twins) <= set(h.base_family.tolist())   # (the moved rows are base family members)
    assert len(set(short.tolist())) == len(short)
    lists = {"short": short, "long": np.concatenate([short, h.phrases]), "handmade": h.handmade.listed}
    head = h.delta_heads[PAIR_FAMILY]
    low, high = (head + k for k in PAIR_MEMBERS)
    if h.position(low) > h.position(high):
        low, high = high, low
    p_star = h.permille(low, high)
    floors = tuple(sorted(DT.FIXED_FLOORS + (p_star, p_star + 1)))
    return SimpleNamespace(lists=lists, pair=(low, high), p_star=p_star, floors=floors, words=words)


def find_needles(h):
    """The finds' needles: the delta heads, the base heads, a moved row's text, two strings that are not held, b"",
    b"a", the glued string and its word, and 40 base words."""
    heads = [h.held[x] for x in h.delta_heads] + [h.held[x] for x in h.base_heads]
    wide = h.held[h.delta_heads[-1]]
    other = [wide + b" qq", wide[len(wide) // 3:2 * len(wide) // 3]]
    assert not set(other) & set(h.held.values())
    words = h.base.strings[:D.N_WORDS]
    g = h.handmade
    return heads + [h.held[h.moved[1]]] + other + [b"", b"a", h.held[g.glued], WORD] + words[::len(words) // 40][:40]


def key_families(refs):
    """Each family under a key of its own (10 + its index for the base's, 40 + its index for the delta's; a moved row
    stays with its base family, so those blocks hold nodes of both images), everything else -- base words, pending
    phrases, the hand-made case -- under three (by ref // 7), each of them a block of both images."""
    refs = np.asarray(refs, dtype=np.uint32)
    delta = (refs >= FAMILY_REF0) & (refs < HANDMADE_REF0)
    base = (refs >= D.FAMILY_REF0) & (refs < PHRASE_REF0)
    keys = (refs // 7) % 3
    keys = np.where(base, 10 + (refs - np.where(base, D.FAMILY_REF0, 0)) // D.MEMBERS, keys)
    return np.where(delta, 40 + (refs - np.where(delta, FAMILY_REF0, 0)) // D.MEMBERS, keys).astype(np.uint32)


def truths(h):
    """name -> a cluster_truth.Truth over what is held now, one per list (a Truth keeps one list's pairs), the
    tokenisation shared."""
    import copy
    kept = {}

    def truth(name):
        if name not in kept:
            kept[name] = copy.copy(h.truth)
            kept[name]._pairs = {}
        return kept[name]

    return truth


class KeepingTruth(Truth):
    """A cluster_truth.Truth that keeps every list's pairs, not the last one's alone: cluster_edges_extend_truth.Split
    asks for three lists' (both, the old alone, the new alone) at every floor."""

    def pairs(self, listed, least=0):
        nodes = np.nonzero(np.isin(self.refs, np.asarray(listed, dtype=np.int64)) & (self.R > 0))[0]
        key = (nodes.tobytes(), least)
        if key not in self._kept:
            self._kept[key] = super().pairs(listed, least)
        return self._kept[key]


def keeping_truth(h):
    """A KeepingTruth over what is held now, the tokenisation shared with h.truth."""
    t = KeepingTruth.__new__(KeepingTruth)
    t.__dict__ = dict(h.truth.__dict__, _pairs={}, _kept={})
    return t


def keys_of(name):
    """The two key functions of the blocked entries: dense_truths.key_pairs (two blocks of both images, about half a
    list each) and key_families."""
    return {"pairs": DT.key_pairs, "families": key_families}[name]


def blocked_truth(c, name, keys):
    """The cluster_tree_within_truth.BlockedTruth of a list of `c` (inputs() with .truth) under a key function, made
    once: over the list's own truth, the tokenisation shared."""
    from cluster_core_tree_within_truth import blocked_over
    kept = c.__dict__.setdefault("_blocked_truths", {})
    if (name, keys) not in kept:
        kept[name, keys] = blocked_over(c.truth(name), c.lists[name], keys_of(keys)(c.lists[name]))
    return kept[name, keys]


def by_image(h, listed):
    """(in_base, in_delta): a list split by the image its references lie in -- the pending puts, the moved rows among
    them, against the rest.  The deleted, listed among the base's, are no nodes."""
    listed = np.asarray(listed, dtype=np.uint32)
    pending = np.isin(listed, np.array(sorted(h.pending), dtype=np.uint32))
    return listed[~pending], listed[pending]


def by_seven(listed):
    """(old, new): every reference that is a multiple of 7 new, the rest old -- nodes of both images on either side."""
    listed = np.asarray(listed, dtype=np.uint32)
    return listed[listed % 7 != 0], listed[listed % 7 == 0]


def delta_ends(h, records):
    """Per record (a, b, permille) of held references: how many of its two ends lie in the delta image."""
    records = np.asarray(records, dtype=np.uint32).reshape(-1, 3)
    return np.isin(records[:, :2], np.array(sorted(h.pending), dtype=np.uint32)).sum(axis=1)


def kinds(h, records):
    """(delta-delta, base-delta, base-base) records."""
    ends = delta_ends(h, records)
    return tuple(int((ends == k).sum()) for k in (2, 1, 0))


def across_in_a_block(h, records, keys):
    """The records with an end in each image and both ends under one key of the key function `keys`."""
    records = np.asarray(records, dtype=np.uint32).reshape(-1, 3)
    one = (delta_ends(h, records) == 1) & (keys_of(keys)(records[:, 0]) == keys_of(keys)(records[:, 1]))
    return records[one]


def fold(m):
    """Fold the log into a rebuilt base image: "dense_min" to 72 and back to 64 marks the image for a rebuild by the
    next call (options.hip), and 64 is what it is rebuilt with."""
    m.set_option("dense_min", 72)
    m.set_option("dense_min", D.DENSE_MIN)


def assert_folded(m):
    info = m.device_info()
    assert (info["base_builds"], info["n_pending"], info["n_tombstones"]) == (2, 0, 0), info


def thrice(c, name, call):
    """Three calls, identical bytes; the call and its first answer are kept under `name` for the fold test."""
    one, two, three = call(), call(), call()
    DT._same_bytes(one, two)
    DT._same_bytes(one, three)
    assert name not in c.recorded, name
    c.recorded[name] = (call, one)
    return one


def fold_and_compare(c, at_least):
    """The last test of a GPU file: nothing so far has folded the log; after the fold every kept call answers from one
    image, without tombstones, with the bytes it gave from two."""
    assert_log(c.m, c.h)
    assert len(c.recorded) >= at_least, len(c.recorded)
    fold(c.m)
    for name, (call, before) in c.recorded.items():
        try:
            DT._same_bytes(before, call())
        except AssertionError as e:
            raise AssertionError(f"{name}: other bytes after the fold") from e
        assert_folded(c.m)


def gpu_case(options=None, before=None):
    """build() and inputs() for a GPU file's module fixture, with the lists' sizes checked against the device: on the
    base image `short` gives a needle two workgroups and `long` one; the delta image has one window."""
    import torch
    m, h = build(options, before)
    c = inputs(h)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # windows_per_workgroup: per = max(1, n_windows * nodes / (8 CUs)), at most n_windows
    assert 2 * len(c.lists["short"]) < 8 * cus, (len(c.lists["short"]), cus)     # per == 1: two workgroups a needle
    assert len(c.lists["long"]) >= 8 * cus, (len(c.lists["long"]), cus)          # per == 2: one
    c.m, c.h, c.cus, c.truth, c.recorded = m, h, cus, truths(h), {}
    return c


def apply(target, steps):
    """Replay the mutations on a map or an oracle (put(string, reference, weight) and delete(reference))."""
    for step in steps:
        if step[0] == "put":
            for r, s, w in zip(step[1].tolist(), step[2], step[3].tolist()):
                target.put(s, r, w)
        else:
            for r in step[1].tolist():
                target.delete(r)


def build(options=None, before=None):
    """(the map, the Host).  options: set before the first put, beside "dense_min"; before(m): called on the synced base
    image in front of the first mutation.  The caller closes the map."""
    from blurrily_amd import RawMap
    from blurrily_amd.map import _pack
    h = host()
    m = RawMap()
    for k, v in dict(options or {}, dense_min=D.DENSE_MIN).items():   # before the first put: changing it later forces a rebuild
        m.set_option(k, v)
    m.put_many_packed(*_pack(h.base.strings), h.base.refs, h.base.weights)
    m.sync_device()
    assert m.device_info()["n_windows"] == 2
    if before is not None:
        before(m)
    for step in h.steps:
        if step[0] == "put":
            assert m.put_many_packed(*_pack(step[2]), step[1], step[3]) > 0
        else:
            for r in step[1].tolist():
                assert m.delete(r) > 0
    assert_log(m, h)
    return m, h


def assert_log(m, h):
    """One base build, and the log holds what the host counts: within its budget, so that no find folds it."""
    info = m.device_info()
    assert info["base_builds"] == 1, info
    assert (info["n_pending"], info["n_tombstones"]) == (len(h.pending), len(h.tombstones)), info
    assert info["n_pending"] + info["n_tombstones"] <= LOG_BUDGET
