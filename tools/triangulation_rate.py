#!/usr/bin/env python3
"""Times orbx_search_for_triangulation_device (ORBmatcher::SearchForTriangulation, reference src/ORBmatcher.cc:965-1206) with HIP events
around many calls, in three shapes: one pair, one keyframe against 20 neighbours (kf1_step = 0, LocalMapping::CreateNewMapPoints' shape)
and a batch of pairs; and, in the same process on the same frames and flags, orbx_search_by_bow_keyframes_device (the keyframe-to-keyframe
SearchByBoW, existing code) as the yardstick.  The two are timed alternately, round after round, and the median over the rounds is reported,
with the shader clock sampled beside the timed work.

Synthetic keyframes at the capacity of a 1200-feature extractor, 1200 features each in ~100 vocabulary nodes: keyframe 2's descriptors are
noisy copies (~15 flipped bits) of keyframe 1's in the same node (15 % in another node), places follow a sideways motion through a pinhole
camera (a quarter of keyframe 2's pushed off their epipolar line), 40 % of the features hold a MapPoint, 30 % have mvuRight >= 0.
Prints one JSON line.  usage: triangulation_rate.py [--pairs 256] [--neighbours 20] [--rounds 7] [--calls 200]"""
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
    ap.add_argument("--pairs", type=int, default=256, help="pairs of the batch call")
    ap.add_argument("--neighbours", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200, help="calls of one pair inside one timed span (the larger shapes: a tenth)")
    a = ap.parse_args()
    import torch
    rng = np.random.default_rng(1)
    P, n = max(a.pairs, a.neighbours), 1200
    ex = X.ORBextractor(1200)
    cap = ex.capacity
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    sf = ex.mvScaleFactor
    # frame 2p = keyframe 1 of pair p, 2p + 1 = its keyframe 2; with kf1_step = 0 frame 0 meets frames 1, 3, 5, ... (other scenes' second
    # keyframes: as many candidates per node, fewer true correspondences)
    B = 2 * P
    fx, cx, cy = 500.0, 320.0, 240.0
    ang, t = 0.03, np.array([-0.5, 0.03, 0.02])
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    Kin = np.linalg.inv(np.array([[fx, 0, cx], [0, fx, cy], [0, 0, 1]]))
    t12 = -R.T @ t
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F12 = (Kin.T @ tx @ R.T @ Kin).astype(np.float32)
    ep = np.array([fx * t[0] / t[2] + cx, fx * t[1] / t[2] + cy], np.float32)
    desc = np.zeros((B, cap, 32), np.uint8); node = np.zeros((B, n), np.uint32)
    kps = np.zeros((B, cap), X.KEYPOINT_DTYPE)
    for p in range(P):
        Xw = np.c_[rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(4, 12, n)]
        X2 = Xw @ R.T + t
        o1 = rng.integers(0, 8, n); o2 = np.clip(o1 + rng.integers(-1, 2, n), 0, 7)
        p1 = np.c_[fx * Xw[:, 0] / Xw[:, 2] + cx, fx * Xw[:, 1] / Xw[:, 2] + cy] + rng.normal(0, 0.3, (n, 2)) * sf[o1][:, None]
        p2 = np.c_[fx * X2[:, 0] / X2[:, 2] + cx, fx * X2[:, 1] / X2[:, 2] + cy] + rng.normal(0, 0.5, (n, 2)) * sf[o2][:, None]
        off = rng.random(n) < 0.25
        p2[off] += rng.normal(0, 12, (int(off.sum()), 2))
        d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8); n1 = rng.integers(1, N_NODES + 1, n).astype(np.uint32)
        perm = rng.permutation(n)
        d2 = d1[perm] ^ np.packbits(rng.random((n, 256)) < 0.06, axis=1)          # ~15 flipped bits
        n2 = n1[perm].copy()
        wrong = rng.random(n) < 0.15
        n2[wrong] = rng.integers(1, N_NODES + 1, int(wrong.sum()))
        a1 = rng.uniform(0, 360, n).astype(np.float32)
        a2 = np.mod(a1[perm] - rng.normal(12, 4, n), 360).astype(np.float32); a2[a2 >= 360] = 0
        k1, k2 = 2 * p, 2 * p + 1
        desc[k1, :n], desc[k2, :n] = d1, d2
        node[k1], node[k2] = n1, n2
        kps["x"][k1, :n], kps["y"][k1, :n], kps["angle"][k1, :n], kps["octave"][k1, :n] = p1[:, 0], p1[:, 1], a1, o1
        kps["x"][k2, :n], kps["y"][k2, :n], kps["angle"][k2, :n], kps["octave"][k2, :n] = p2[perm, 0], p2[perm, 1], a2, o2[perm]
    fn, fi = feature_vectors(node, cap)
    flags1 = (rng.random((P, cap)) < 0.4).astype(np.uint8); flags2 = (rng.random((P, cap)) < 0.4).astype(np.uint8)
    ur = np.where(rng.random((B, cap)) < 0.3, 10.0, -1.0).astype(np.float32)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    d_fn, d_fi, d_nf = dev(fn.view(np.int32)), dev(fi.view(np.int32)), dev(np.full(B, n, np.int32))
    d_k, d_d, d_n, d_ur = dev(kps.view(np.uint8)), dev(desc), dev(np.full(B, n, np.int32)), dev(ur)
    d_f1, d_f2 = dev(flags1), dev(flags2)
    d_F, d_e = dev(np.tile(F12.reshape(1, 9), (P, 1))), dev(np.tile(ep.reshape(1, 2), (P, 1)))
    d_m = torch.zeros((P, cap), dtype=torch.int32, device="cuda"); d_p = torch.zeros((P, cap, 2), dtype=torch.int32, device="cuda")
    d_mb = torch.zeros((P, cap), dtype=torch.int32, device="cuda"); d_nm = torch.zeros(P, dtype=torch.int32, device="cuda")

    def tri(np_, kf1_step):
        ex.search_for_triangulation_device(np_, (0, kf1_step), (1, 2), d_fn, d_fi, d_nf, d_f1, d_f2, d_k, d_ur, d_d, d_n, cap, d_F, d_e, d_m, d_p, d_nm)

    def bow(np_, kf1_step):      # the yardstick: SearchByBoW(pKF1, pKF2) on the same frames (its candidates HOLD a MapPoint: flags inverted to keep the candidate count)
        ex.search_by_bow_keyframes_device(np_, (0, kf1_step), (1, 2), d_fn, d_fi, d_nf, d_g1, d_g2, d_k, d_d, d_n, cap, d_mb, d_nm)

    d_g1, d_g2 = dev(1 - flags1), dev(1 - flags2)
    forms = [("triangulation", tri), ("bow_keyframes", bow)]
    out = dict(tool="triangulation_rate", source_hash=X.source_hash(), capacity=cap, features=n, nodes=N_NODES, pairs_batch=a.pairs,
               neighbours=a.neighbours, rounds=a.rounds, calls_per_span=a.calls,
               note="us per call: median over the rounds of (events around `calls` calls) / calls")
    tri(a.pairs, 2); torch.cuda.synchronize()
    out["matches_mean_triangulation"] = float(d_nm[:a.pairs].float().mean())
    bow(a.pairs, 2); torch.cuda.synchronize()
    out["matches_mean_bow_keyframes"] = float(d_nm[:a.pairs].float().mean())
    slot = 0
    for label, np_, step, calls in (("1", 1, 2, a.calls), ("neighbours", a.neighbours, 0, max(a.calls // 10, 5)), ("batch", a.pairs, 2, max(a.calls // 10, 5))):
        ts = {name: [] for name, _ in forms}
        for name, fn_ in forms:                          # warm-up of every shape the timed spans use
            for _ in range(3):
                fn_(np_, step)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, fn_ in forms:                      # alternating: a drift of the machine lands on both
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for c in range(calls):
                    fn_(np_, step)
                    if c == calls // 2 and slot < 60:
                        ex.clock_probe(slot); slot += 1
                e1.record()
                torch.cuda.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1000.0 / calls)
        for name, v in ts.items():
            out["%s_us_%s" % (name, label)] = round(float(np.median(v)), 2)
            out["%s_us_%s_minmax" % (name, label)] = [round(min(v), 2), round(max(v), 2)]
        out["ratio_triangulation_over_bow_%s" % label] = round(out["triangulation_us_%s" % label] / out["bow_keyframes_us_%s" % label], 2)
    ghz = ex.clock_read(slot)
    out["shader_clock_ghz_minmax"] = [round(float(min(ghz)), 3), round(float(max(ghz)), 3)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
