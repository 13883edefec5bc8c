#!/usr/bin/env python3
"""Times orbx_search_by_projection_two_eyes_device (ORBmatcher::SearchByProjection for two-camera frames, reference src/ORBmatcher.cc:44-213)
with HIP events, as one pair and as a batch of pairs, next to the one-eye entry orbx_search_by_projection_device (ratio mode, no mvuRight)
on the same left frames.  Synthetic frames: random raw keypoints per eye (1200-feature extractor capacity), 60 % of the left keypoints
paired with a right keypoint by consistent maps, one MapPoint per left keypoint up to query_capacity, both requests on, 90 % of them with
observations; grids from orbx_frame_finish_two_eyes_device.  Prints one JSON line.  usage: two_eyes_search_rate.py [--pairs 256] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import extractorb_amd as X  # noqa: E402

ROWS, COLS = 480, 640
PROJ_QUERY = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("radius", "<f4"), ("min_level", "<i4"), ("max_level", "<i4"),
                       ("flags", "<i4"), ("angle", "<f4")])


def frames(rng, B, cap, n):
    k = np.zeros((B, cap), X.KEYPOINT_DTYPE)
    k["x"][:, :n] = rng.uniform(0, COLS, (B, n)); k["y"][:, :n] = rng.uniform(0, ROWS, (B, n))
    k["octave"][:, :n] = rng.integers(0, 8, (B, n)); k["size"], k["class_id"] = 31, -1
    d = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    return k, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--query-capacity", type=int, default=2048)
    a = ap.parse_args()
    import torch
    rng = np.random.default_rng(1)
    ex = X.ORBextractor(1200, max_batch=2)
    cap, qcap, P = ex.capacity, a.query_capacity, a.pairs
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    n = min(1200, cap)
    k, d = frames(rng, 2 * P, cap, n)
    scale = np.asarray(X.compute_tables(1200, 1.2, 8)["scale_factors"], np.float32)
    l2r = np.full((2 * P, cap), -1, np.int32); r2l = np.full((2 * P, cap), -1, np.int32)
    nq = min(qcap, n)
    q = np.zeros((P, qcap, 2), PROJ_QUERY); qd = np.zeros((P, qcap, 32), np.uint8)
    for p in range(P):
        L, R = 2 * p, 2 * p + 1
        paired = rng.permutation(n)[:int(0.6 * n)]
        right = rng.permutation(n)[:len(paired)]
        k["x"][R, right] = k["x"][L, paired] - rng.uniform(5, 40, len(paired)); k["y"][R, right] = k["y"][L, paired]
        k["octave"][R, right] = k["octave"][L, paired]; d[R, right] = d[L, paired]
        l2r[L, paired], r2l[R, right] = right, paired
        t = np.arange(nq)
        lv = k["octave"][L, t]
        q[p, :nq, 0]["u"] = k["x"][L, t] + rng.uniform(-2, 2, nq); q[p, :nq, 0]["v"] = k["y"][L, t] + rng.uniform(-2, 2, nq)
        q[p, :nq, 0]["radius"] = np.float32(4.0 * 5.0) * scale[lv]
        partner = np.where(l2r[L, t] >= 0, l2r[L, t], rng.integers(0, n, nq))
        q[p, :nq, 1]["u"] = k["x"][R, partner] + rng.uniform(-2, 2, nq); q[p, :nq, 1]["v"] = k["y"][R, partner] + rng.uniform(-2, 2, nq)
        q[p, :nq, 1]["radius"] = np.float32(4.0) * scale[k["octave"][R, partner]]
        obs = np.where(rng.random(nq) < 0.9, 2, 0)
        for e, lvl in ((0, lv), (1, k["octave"][R, partner])):
            q[p, :nq, e]["min_level"], q[p, :nq, e]["max_level"], q[p, :nq, e]["flags"] = lvl - 1, lvl, 1 | obs
        qd[p, :nq] = d[L, t] ^ (rng.random((nq, 32)) < 0.04).astype(np.uint8)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    d_k, d_d = dev(k.view(np.uint8)), dev(d)
    d_n = dev(np.full(2 * P, n, np.int32))
    bounds = np.array([0, COLS, 0, ROWS], np.float32)
    cam = X.camera(fx=500.0, fy=500.0, cx=320.0, cy=240.0)
    d_un = torch.zeros_like(d_k); d_off = torch.zeros((2 * P, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    d_idx = torch.zeros((2 * P, cap), dtype=torch.int32, device="cuda"); d_nin = torch.zeros(2 * P, dtype=torch.int32, device="cuda")
    ex.frame_finish_two_eyes_device(P, d_k, d_n, cap, cam, bounds, d_un, d_off, d_idx, d_nin)
    d_q, d_qd, d_nq = dev(q.view(np.uint8)), dev(qd), dev(np.full(P, nq, np.int32))
    d_l2r, d_r2l = dev(l2r), dev(r2l)
    q1 = np.ascontiguousarray(q[:, :, 0])
    d_q1 = dev(q1.view(np.uint8))
    d_occ2 = torch.zeros((P, 2, cap), dtype=torch.uint8, device="cuda"); d_occ1 = torch.zeros((P, cap), dtype=torch.uint8, device="cuda")
    d_m2 = torch.zeros((P, 2, cap), dtype=torch.int32, device="cuda"); d_m1 = torch.zeros((P, cap), dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(P, dtype=torch.int32, device="cuda")

    def two(np_):
        d_occ2.zero_()
        ex.search_by_projection_two_eyes_device(np_, (0, 1), d_q, d_qd, (0, 1), d_nq, qcap, d_k, d_d, d_n, cap, d_off, d_idx, bounds, d_l2r, d_r2l,
                                                d_occ2, 0.8, d_m2, d_nm)

    def one(np_):
        d_occ1.zero_()
        ex.search_by_projection_device(np_, (0, 2), d_q1, d_qd, (0, 1), d_nq, qcap, d_k, d_d, d_n, cap, d_off, d_idx, bounds, None, d_occ1, True,
                                       0.8, False, d_m1, d_nm)

    def timed(fn, np_):
        fn(np_)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(np_); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1000.0)
        return float(np.median(ts))

    import ctypes as C
    st = (C.c_int * 4)()
    X.load_library().orbx_debug_two_eyes_search_stats(st)
    out = dict(tool="two_eyes_search_rate", source_hash=X.source_hash(), capacity=cap, query_capacity=qcap, keypoints_per_eye=n, mappoints=nq,
               pairs=P, reps=a.reps, note="median of reps; each timed span includes a small occupancy-reset memset")
    out["two_eyes_us_1pair"] = timed(two, 1)
    X.load_library().orbx_debug_two_eyes_search_stats(st)
    two(1); torch.cuda.synchronize(); X.load_library().orbx_debug_two_eyes_search_stats(st)
    out["two_eyes_rounds_pair0"], out["two_eyes_walk_pair0"] = st[0], st[1]
    out["two_eyes_us_batch"] = timed(two, P)
    out["one_eye_us_1pair"] = timed(one, 1)
    out["one_eye_us_batch"] = timed(one, P)
    two(P); torch.cuda.synchronize()
    out["two_eyes_matches_mean"] = float(d_nm.float().mean())
    X.load_library().orbx_debug_two_eyes_search_stats(st)
    out["two_eyes_pairs_walked_last_call"] = st[2]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
