"""Crafted vocabularies and frames for Frame::ComputeBoW (k_bow_words, k_bow_reduce; reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h
:1127-1196, :1218-1262): frames past 1024 keypoints (k_bow_reduce's `per` >= 2), the capacities where the summed weights move from LDS into the
output array, weights whose sums depend on the order of the additions, stopped words, every weighting x scoring, levels_up at and past the
tree's depth, and children lists that need several rounds of 16 lanes.  A case is dict(name, vocab, frames, capacity, levels_up);
docs/history/r25_bow_edges.md lists what each reaches."""
import numpy as np

from test_bow import make_vocab

POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.uint16)
REDUCE_THREADS = 1024        # k_bow.hip: kReduceThreads


def descend(v, desc, levels_up):
    """TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup) for all features at once: (leaf node, node at level L - levels_up)
    per feature.  The nearest child, the first one on ties (np.argmin returns the first minimum)."""
    parent = np.asarray(v["parent"])
    n = len(parent)
    order = np.argsort(parent[1:], kind="stable") + 1             # the children of every node, in node order
    counts = np.bincount(parent[1:], minlength=n)
    off = np.r_[0, np.cumsum(counts)]
    node = np.zeros(len(desc), np.int64); nid = np.zeros(len(desc), np.int64)
    level = 0
    while True:
        act = np.nonzero(counts[node] > 0)[0]
        if not len(act):
            return node, nid
        level += 1
        for p in np.unique(node[act]):
            idx = act[node[act] == p]
            kids = order[off[p]:off[p + 1]]
            for c in range(0, len(idx), 2048):
                part = idx[c:c + 2048]
                d = POPCOUNT[desc[part][:, None, :] ^ v["desc"][kids][None, :, :]].sum(2)
                node[part] = kids[d.argmin(1)]
        if level == v["L"] - levels_up:
            nid[act] = node[act]


def word_ids(v):
    """node -> word id: the leaves in node order (:1409-1415)"""
    return np.cumsum(np.asarray(v["is_leaf"], np.int64)) - 1


def sort_size(n):
    """k_bow_reduce: the power of two its sorts run on for a frame of n keypoints / the launch's Pmax for a capacity"""
    P = 64
    while P < n:
        P <<= 1
    return P


def per_thread(n):
    return (sort_size(n) + REDUCE_THREADS - 1) // REDUCE_THREADS


def wsum_in_output_array(capacity):
    """k_bow_reduce keeps the summed weights in LDS while Pmax <= 8192, else in the output array itself"""
    return sort_size(capacity) > 8192


# ---- vocabularies ----

def exponent_weights(v, rng, spread=30):
    """word weights with binary exponents over 2^-spread ... 2^spread and full mantissas: any other order of a sum of them gives another double"""
    n = len(v["parent"])
    w = rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-spread, spread + 1, n).astype(np.float64))
    return dict(v, weight=np.where(np.asarray(v["is_leaf"]) > 0, w, 0.0))


def with_modes(v, scoring, weighting):
    return dict(v, scoring=scoring, weighting=weighting)


def tree(parent, is_leaf, desc, weight, k, L, scoring=0, weighting=0):
    return dict(k=k, L=L, scoring=scoring, weighting=weighting, parent=np.array(parent, np.int32), is_leaf=np.array(is_leaf, np.uint8),
                desc=np.ascontiguousarray(desc, np.uint8), weight=np.array(weight, np.float64))


def twenty_children(rng):
    """one node with 20 children, child 17 equal to child 2: the tie spans the two rounds of 16 lanes, the first wins"""
    desc = rng.integers(0, 256, (21, 32), dtype=np.uint8)
    desc[1 + 17] = desc[1 + 2]
    return tree([0] * 21, [0] + [1] * 20, desc, np.r_[0.0, rng.uniform(0.5, 4.0, 20)], k=20, L=1)


def wide_children(rng):
    """root -> A, B.  A has 256 children (the rank byte's last value is 255) and a descriptor that equals its child 255; B's 256 children are all
    the complement of B's own descriptor: a feature equal to B's descriptor is 256 bits from every child, the largest key there is."""
    x = rng.integers(0, 256, 32, dtype=np.uint8); D = rng.integers(0, 256, 32, dtype=np.uint8)
    kids_a = rng.integers(0, 256, (256, 32), dtype=np.uint8); kids_a[255] = x
    desc = np.concatenate([np.zeros((1, 32), np.uint8), x[None], (~D)[None], kids_a, np.repeat(D[None], 256, 0)])
    parent = [0, 0, 0] + [1] * 256 + [2] * 256
    return tree(parent, [0, 0, 0] + [1] * 512, desc, np.r_[0.0, 0.0, 0.0, rng.uniform(0.5, 4.0, 512)], k=20, L=2), x, ~D


# ---- frames ----

def near_leaves(v, rng, n, hot=0.3):
    """n descriptors near vocabulary leaves (a share `hot` of them near a handful of leaves, so words repeat), a tenth pure noise"""
    leaves = np.nonzero(v["is_leaf"])[0]
    d = v["desc"][rng.choice(leaves, n)].copy()
    nh = int(n * hot)
    d[:nh] = v["desc"][rng.choice(leaves[: max(4, len(leaves) // 50)], nh)]
    flips = rng.integers(0, 256, (n, 6)); nflip = rng.integers(0, 7, n)
    for j in range(6):
        on = nflip > j
        d[on, flips[on, j] >> 3] ^= (1 << (flips[on, j] & 7)).astype(np.uint8)
    d[n - n // 10:] = rng.integers(0, 256, (n // 10, 32), dtype=np.uint8)
    return d[rng.permutation(n)]


def distinct_words(v, rng, n):
    """n descriptors that fall into n different, unstopped words"""
    pool = near_leaves(v, rng, 6 * n, hot=0.0)
    leaf, _ = descend(v, pool, 0)
    _, first = np.unique(leaf, return_index=True)
    first = np.sort(first[np.asarray(v["weight"])[leaf[first]] > 0])
    assert len(first) >= n
    return pool[first[:n]]


FRAME_SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3000]
MODES = [(w, s) for w in (0, 1, 2, 3) for s in (0, 1, 5)]      # weighting TF_IDF, TF, IDF, BINARY x scoring L1_NORM, L2_NORM, DOT_PRODUCT


def cases():
    rng = np.random.default_rng(2500)
    out = []
    base = exponent_weights(make_vocab(rng, k=10, L=3), rng)
    add = lambda name, v, frames, capacity, levels_up: out.append(dict(name=name, vocab=v, frames=frames, capacity=capacity, levels_up=levels_up))
    add("frame_sizes", base, [near_leaves(base, rng, n) for n in FRAME_SIZES], 3000, 1)
    add("capacity_8192", base, [near_leaves(base, rng, 8192), near_leaves(base, rng, 1500)], 8192, 2)
    add("capacity_8193", with_modes(base, 1, 0), [near_leaves(base, rng, 1500), near_leaves(base, rng, 8193), near_leaves(base, rng, 0)], 8193, 2)
    add("capacity_16384", base, [near_leaves(base, rng, 16384), near_leaves(base, rng, 1500)], 16384, 2)
    # one word holds the whole frame: DOT_PRODUCT leaves the sum itself in the output (divided by the one word)
    one = near_leaves(base, rng, 40, hot=0.0)
    one = one[np.asarray(base["weight"])[descend(base, one, 0)[0]] > 0][:1]
    add("one_hot_word", with_modes(base, 5, 0), [np.repeat(one, 1500, 0)], 1500, 1)
    mixed = np.concatenate([np.repeat(one, 700, 0), near_leaves(base, rng, 800)])[rng.permutation(1500)]
    add("hot_word_l1", base, [mixed], 1500, 1)
    add("hot_word_l2", with_modes(base, 1, 1), [mixed], 1500, 1)
    big = exponent_weights(make_vocab(rng, k=10, L=4, stop_frac=0.02), rng)
    add("own_words", big, [distinct_words(big, rng, 1500)], 1500, 2)
    # stopped words
    add("all_stopped", dict(base, weight=np.zeros(len(base["parent"]))), [near_leaves(base, rng, 500), near_leaves(base, rng, 1100)], 1100, 1)
    half = np.asarray(base["weight"]).copy(); half[(word_ids(base) % 2 == 1) & (np.asarray(base["is_leaf"]) > 0)] = 0.0
    add("every_second_stopped", dict(base, weight=half), [near_leaves(base, rng, 500)], 600, 1)
    small = exponent_weights(make_vocab(rng, k=6, L=3), rng, spread=8)
    frame = near_leaves(small, rng, 200)
    for w, s in MODES:
        add("modes_w%d_s%d" % (w, s), with_modes(small, s, w), [frame], 256, 2)
    ragged = make_vocab(rng, k=4, L=4, ragged=True)
    frame = near_leaves(ragged, rng, 300)
    for lu in (0, 1, 3, 4, 6):                # L = 4: the leaf's level, ..., the root's children, the root, the root
        add("levels_up_%d" % lu, ragged, [frame], 300, lu)
    v20 = twenty_children(rng)
    add("twenty_children", v20, [np.concatenate([np.repeat(v20["desc"][3:4], 5, 0), np.repeat(v20["desc"][18:19], 5, 0), near_leaves(v20, rng, 60)])], 70, 0)
    wide, x, notd = wide_children(rng)
    add("wide_children", wide, [np.concatenate([x[None], notd[None], near_leaves(wide, rng, 40, hot=0.0), x[None], notd[None]])], 64, 1)
    return out
