#!/usr/bin/env python3
"""Times orbx_search_by_bow_two_eyes_device (ORBmatcher::SearchByBoW for two-camera frames, reference src/ORBmatcher.cc:269-471) with HIP
events around many calls, as one search and as a batch of searches, next to the one-eye entry orbx_search_by_bow_device on the same frames
(keyframe left eye -> frame left eye), and in both of its forms: the frame pair's descriptors staged in LDS (the default at this capacity)
and read from L2 (test aid "two_eyes_bow_stage" = 0).  The three are timed alternately, round after round, and the median over the rounds is
reported, with the shader clock sampled beside the timed work.

Synthetic frames at the capacity of a 1200-feature extractor, 1200 features per eye: 40 % of a keyframe's right descriptors are copies of
left ones, frame descriptors are noisy copies of keyframe descriptors of either eye in the same vocabulary node (100 nodes, the count at
levelsup = 4 of a k = 10, L = 6 vocabulary), 80 % of the keyframe features hold a MapPoint.  Prints one JSON line.
usage: two_eyes_bow_rate.py [--pairs 256] [--rounds 7] [--calls 200]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import extractorb_amd as X  # noqa: E402

N_NODES = 100


def feature_vectors(node, cap):
    """(node, index) order per frame: [B, n] node ids -> padded node / index columns"""
    B, n = node.shape
    fn = np.zeros((B, cap), np.uint32); fi = np.zeros((B, cap), np.uint32)
    order = np.argsort(node, axis=1, kind="stable")
    fn[:, :n] = np.take_along_axis(node, order, 1); fi[:, :n] = order
    return fn, fi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256, help="searches of the batch call")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200, help="calls of one search inside one timed span (the batch call: a tenth)")
    a = ap.parse_args()
    import torch
    rng = np.random.default_rng(1)
    P, n = a.pairs, 1200
    ex = X.ORBextractor(1200)
    X.debug_set_option("two_eyes_bow_stage", 0)
    try:
        ex_l2 = X.ORBextractor(1200)
    finally:
        X.debug_set_option("two_eyes_bow_stage", -1)
    cap = ex.capacity
    st = torch.cuda.current_stream().cuda_stream
    ex.set_stream(st); ex_l2.set_stream(st)
    # batch pair 2p = keyframe pair of search p, 2p + 1 = its frame pair; frame 2X = left eye, 2X + 1 = right eye of pair X
    B = 4 * P
    desc = np.zeros((B, cap, 32), np.uint8); node = np.zeros((B, n), np.uint32)
    kps = np.zeros((B, cap), X.KEYPOINT_DTYPE)
    for p in range(P):
        kl, kr, fl = 4 * p, 4 * p + 1, 4 * p + 2
        dk = rng.integers(0, 256, (2 * n, 32), dtype=np.uint8); nk = rng.integers(1, N_NODES + 1, 2 * n).astype(np.uint32)
        twin = np.nonzero(rng.random(n) < 0.4)[0]; of = rng.integers(0, n, len(twin))
        dk[n + twin] = dk[of]; nk[n + twin] = nk[of]
        src = rng.integers(0, 2 * n, 2 * n)
        df = dk[src] ^ np.packbits(rng.random((2 * n, 256)) < 0.06, axis=1)       # ~15 flipped bits
        nf = nk[src].copy()
        wrong = rng.random(2 * n) < 0.15
        nf[wrong] = rng.integers(1, N_NODES + 1, wrong.sum())
        ak = rng.uniform(0, 360, 2 * n).astype(np.float32)
        af = np.mod(ak[src] + rng.normal(12, 4, 2 * n), 360).astype(np.float32); af[af >= 360] = 0
        desc[kl, :n], desc[kr, :n], desc[fl, :n], desc[fl + 1, :n] = dk[:n], dk[n:], df[:n], df[n:]
        node[kl], node[kr], node[fl], node[fl + 1] = nk[:n], nk[n:], nf[:n], nf[n:]
        kps["angle"][kl, :n], kps["angle"][kr, :n], kps["angle"][fl, :n], kps["angle"][fl + 1, :n] = ak[:n], ak[n:], af[:n], af[n:]
    fn, fi = feature_vectors(node, cap)
    flags2 = (rng.random((P, 2, cap)) < 0.8).astype(np.uint8)
    flags1 = np.ascontiguousarray(flags2[:, 0])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    d_fn, d_fi, d_nf = dev(fn.view(np.int32)), dev(fi.view(np.int32)), dev(np.full(B, n, np.int32))
    d_k, d_d, d_n = dev(kps.view(np.uint8)), dev(desc), dev(np.full(B, n, np.int32))
    d_f2, d_f1 = dev(flags2), dev(flags1)
    d_m2 = torch.zeros((P, 2, cap), dtype=torch.int32, device="cuda"); d_m1 = torch.zeros((P, cap), dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(P, dtype=torch.int32, device="cuda")

    def two(e):
        return lambda np_: e.search_by_bow_two_eyes_device(np_, (0, 2), (1, 2), d_fn, d_fi, d_nf, d_f2, d_k, d_d, d_n, cap, d_m2, d_nm)

    def one(np_):      # keyframe left eye (frame 4p) against the frame's left eye (frame 4p + 2)
        ex.search_by_bow_device(np_, (0, 4), (2, 4), d_fn, d_fi, d_nf, d_f1, d_k, d_d, d_n, cap, d_m1, d_nm)

    forms = [("two_eyes_staged", two(ex)), ("two_eyes_l2", two(ex_l2)), ("one_eye", one)]
    out = dict(tool="two_eyes_bow_rate", source_hash=X.source_hash(), capacity=cap, features_per_eye=n, nodes=N_NODES, searches_batch=P,
               rounds=a.rounds, calls_per_span=a.calls, note="us per call: median over the rounds of (events around `calls` calls) / calls")
    two(ex)(P); torch.cuda.synchronize()
    m_staged, n_staged = d_m2.clone(), d_nm.clone()
    out["matches_mean_two_eyes"] = float(d_nm.float().mean())
    out["matches_right_eye_mean"] = float((d_m2[:, 1] >= 0).sum()) / P
    two(ex_l2)(P); torch.cuda.synchronize()
    out["forms_agree"] = bool(torch.equal(m_staged, d_m2) and torch.equal(n_staged, d_nm))
    one(P); torch.cuda.synchronize()
    out["matches_mean_one_eye"] = float(d_nm.float().mean())
    slot = 0
    for label, np_, calls in (("1", 1, a.calls), ("batch", P, max(a.calls // 10, 5))):
        ts = {name: [] for name, _ in forms}
        for name, fn_ in forms:                          # warm-up of every shape the timed spans use
            for _ in range(3):
                fn_(np_)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, fn_ in forms:                      # alternating: a drift of the machine lands on all three
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for c in range(calls):
                    fn_(np_)
                    if c == calls // 2 and slot < 60:
                        ex.clock_probe(slot); slot += 1
                e1.record()
                torch.cuda.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1000.0 / calls)
        for name, v in ts.items():
            out["%s_us_%s" % (name, label)] = round(float(np.median(v)), 2)
            out["%s_us_%s_minmax" % (name, label)] = [round(min(v), 2), round(max(v), 2)]
    ghz = ex.clock_read(slot)
    out["shader_clock_ghz_minmax"] = [round(float(min(ghz)), 3), round(float(max(ghz)), 3)]
    for label in ("1", "batch"):
        out["ratio_two_eyes_over_one_eye_%s" % label] = round(out["two_eyes_staged_us_%s" % label] / out["one_eye_us_%s" % label], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
