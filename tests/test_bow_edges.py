"""Frame::ComputeBoW (k_bow_words, k_bow_reduce) on crafted vocabularies and frames (tests/bow_scenes.py).  CPU: the oracle equals an independent
statement on every case, the cases reach what they are for (frames whose sorts run at every size up to 16384, `per` up to 16, the summed
weights in the output array, a word segment across thread blocks, order-sensitive sums).  GPU: compute_bow_device against the oracle on every
case: ids, weights byte for byte, both FeatureVector columns, both counts.  docs/history/r25_bow_edges.md has the tables."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import extractorb_amd as X
import bow_scenes as B
from test_bow import brute_bow

CASES = B.cases()
BY_NAME = dict((c["name"], c) for c in CASES)


@functools.lru_cache(maxsize=None)
def want(name, f):
    c = BY_NAME[name]
    got = O.compute_bow(c["vocab"], c["frames"][f], c["levels_up"])
    for a in got:
        a.setflags(write=False)
    return got


@pytest.mark.parametrize("name", list(BY_NAME))
def test_oracle_equals_statement_on_every_case(name):
    c = BY_NAME[name]
    for f, d in enumerate(c["frames"]):
        wid, ww, fn, fi = want(name, f)
        keys, vals, bfn, bfi = brute_bow(c["vocab"], d, c["levels_up"])
        assert wid.tolist() == keys and fn.tolist() == bfn and fi.tolist() == bfi, (name, f)
        assert ww.tolist() == vals, (name, f)                    # the same doubles: the same order of additions


def test_cases_reach_what_they_are_for():
    sizes = BY_NAME["frame_sizes"]
    assert [len(d) for d in sizes["frames"]] == B.FRAME_SIZES and sizes["capacity"] == 3000
    assert sorted(set(B.sort_size(n) for n in B.FRAME_SIZES)) == [64, 128, 1024, 2048, 4096] and max(B.per_thread(n) for n in B.FRAME_SIZES) == 4
    assert [B.per_thread(n) for n in (1024, 1025, 2049)] == [1, 2, 4]
    # capacities: the summed weights live in LDS up to 8192 slots and in the output array beyond
    assert [B.wsum_in_output_array(BY_NAME[n]["capacity"]) for n in ("capacity_8192", "capacity_8193", "capacity_16384")] == [False, True, True]
    assert [B.sort_size(c) for c in (8192, 8193, 16384)] == [8192, 16384, 16384]
    for n in ("capacity_8192", "capacity_8193", "capacity_16384"):
        c = BY_NAME[n]
        lens = [len(d) for d in c["frames"]]
        assert max(lens) == c["capacity"] and 1500 in lens      # one frame filled to the capacity, the others sort at a smaller size
    assert B.per_thread(16384) == 16
    # a word segment longer than four threads' blocks
    for n, least in (("one_hot_word", 1500), ("hot_word_l1", 700), ("hot_word_l2", 700)):
        c = BY_NAME[n]
        leaf, _ = B.descend(c["vocab"], c["frames"][0], 0)
        assert np.bincount(leaf).max() >= least > 4 * B.per_thread(1500)
    assert len(want("one_hot_word", 0)[0]) == 1 and len(want("hot_word_l1", 0)[0]) > 100
    assert len(want("own_words", 0)[0]) == 1500 == len(BY_NAME["own_words"]["frames"][0])      # W = N
    # stopped words
    for f in (0, 1):
        wid, ww, fn, fi = want("all_stopped", f)
        assert len(wid) == 0 and len(fi) == 0 and len(BY_NAME["all_stopped"]["frames"][f]) > 0
    wid, ww, fn, fi = want("every_second_stopped", 0)
    assert (wid % 2 == 0).all() and 100 < len(fi) < 450
    # levels_up: the leaf itself, ..., the root's children, the root
    rag = BY_NAME["levels_up_0"]["vocab"]
    level = np.asarray(rag["level"])
    fn = dict((lu, want("levels_up_%d" % lu, 0)[2]) for lu in (0, 1, 3, 4, 6))
    assert (fn[4] == 0).all() and (fn[6] == 0).all() and set(level[fn[3]]) == {1}
    assert set(level[fn[0]]) == {0, 4} and (fn[0] == 0).any() and set(level[fn[1]]) == {0, 3}      # 0: leaves above the node level keep the root's id
    assert all(np.asarray(rag["is_leaf"])[fn[0][fn[0] > 0]])
    # children
    wid = want("twenty_children", 0)[0]
    assert 2 in wid and 17 not in wid
    leaf, _ = B.descend(BY_NAME["wide_children"]["vocab"], BY_NAME["wide_children"]["frames"][0], 0)
    assert leaf[0] == 3 + 255 and leaf[1] == 3 + 256 and leaf[-2] == 3 + 255 and leaf[-1] == 3 + 256      # A's child 255; the first of B's children
    assert len(set(c["name"] for c in CASES if c["name"].startswith("modes_"))) == 12


def _pairwise(x):
    return x[0] if len(x) == 1 else _pairwise(x[: len(x) // 2]) + _pairwise(x[len(x) // 2:])


def _sequential(x):
    s = 0.0
    for a in x:
        s = s + a
    return s


def test_the_weights_are_order_sensitive():
    """the sums the kernel must form in the reference's order give other doubles in any other order: otherwise the cases prove nothing"""
    c = BY_NAME["one_hot_word"]
    leaf, _ = B.descend(c["vocab"], c["frames"][0], 0)
    w = float(c["vocab"]["weight"][leaf[0]])
    seq = _sequential([w] * 1500)
    assert seq != 1500 * w and seq != _pairwise([w] * 1500)
    assert want("one_hot_word", 0)[1].tolist() == [seq]          # DOT_PRODUCT with one word: the sum itself
    for name in ("hot_word_l1", "hot_word_l2"):
        c = BY_NAME[name]
        leaf, _ = B.descend(c["vocab"], c["frames"][0], 0)
        hot = np.bincount(leaf).argmax(); n = int((leaf == hot).sum()); w = float(c["vocab"]["weight"][hot])
        assert _sequential([w] * n) != n * w and _sequential([w] * n) != _pairwise([w] * n)
    for name in ("hot_word_l1", "own_words", "frame_sizes"):      # the norm over the words, ascending: not the descending sum, not a pairwise one
        c = BY_NAME[name]
        d = c["frames"][-1]
        leaf, _ = B.descend(c["vocab"], d, 0)
        sums = {}                                                # the words' summed weights before the normalisation
        for i in range(len(d)):
            w = float(c["vocab"]["weight"][leaf[i]])
            if w > 0:
                sums[leaf[i]] = sums[leaf[i]] + w if leaf[i] in sums else w
        vals = [sums[k] for k in sorted(sums)]                   # (word ids ascend with the leaves' node numbers)
        assert len(vals) > 100 and _sequential(vals) != _sequential(vals[::-1]) and _sequential(vals) != _pairwise(vals), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BY_NAME))
def test_gpu_bow_case_equals_oracle(name):
    import torch
    c = BY_NAME[name]
    cap, frames = c["capacity"], c["frames"]
    if name.startswith("capacity_"):      # which launches ran k_bow_reduce with the summed weights in the output array
        assert B.wsum_in_output_array(cap) == (cap > 8192) and max(len(d) for d in frames) == cap
    n = len(frames)
    desc = np.zeros((n, cap, 32), np.uint8)
    for f, d in enumerate(frames):
        desc[f, :len(d)] = d
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_wid = torch.full((n, cap), -7, dtype=torch.int32, device="cuda"); d_ww = torch.full((n, cap), -7.0, dtype=torch.float64, device="cuda")
    d_nw = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_fn = torch.full((n, cap), -7, dtype=torch.int32, device="cuda"); d_fi = torch.full((n, cap), -7, dtype=torch.int32, device="cuda")
    d_nf = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ex = X.ORBextractor(1000)
    ex.compute_bow_device(X.Vocabulary(arrays=c["vocab"]), n, dev(desc), dev(np.array([len(d) for d in frames], np.int32)), cap, d_wid, d_ww, d_nw, d_fn,
                          d_fi, d_nf, levels_up=c["levels_up"])
    ex.synchronize()
    nw, nf = d_nw.cpu().numpy(), d_nf.cpu().numpy()
    g_wid, g_ww, g_fn, g_fi = d_wid.cpu().numpy(), d_ww.cpu().numpy(), d_fn.cpu().numpy(), d_fi.cpu().numpy()
    for f in range(n):
        wid, ww, fn, fi = want(name, f)
        assert (int(nw[f]), int(nf[f])) == (len(wid), len(fi)), (name, f)
        assert g_wid[f, :len(wid)].astype(np.uint32).tolist() == wid.tolist(), (name, f)
        assert g_ww[f, :len(wid)].tobytes() == ww.tobytes(), "%s frame %d: weights differ (order of additions?)" % (name, f)
        assert g_fn[f, :len(fi)].astype(np.uint32).tolist() == fn.tolist() and g_fi[f, :len(fi)].astype(np.uint32).tolist() == fi.tolist(), (name, f)
