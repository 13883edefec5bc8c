#!/usr/bin/env python3
"""Times orbx_search_last_frame_two_eyes_device (ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, ...) for two-camera frames, reference
src/ORBmatcher.cc:1961-2177) with HIP events, as one pair and as a batch of pairs, next to what a caller could approximate without it: two
launches of the one-eye entry orbx_search_by_projection_device (ratio_mode 0, rotation histogram per launch), one over the left frames with
the L requests and one over the right frames with the R requests - no suppression of R, two histograms.  Also times the front half
(orbx_project_last_frame_two_eyes_device).  Synthetic rigs: random raw keypoints per eye at the 1200-feature extractor's capacity, ~1000
MapPoints per last rig aimed at a current keypoint in each eye (th = 7 windows), 85 % of them with observations; grids from
orbx_frame_finish_two_eyes_device.  Prints one JSON line.  usage: last_frame_two_eyes_rate.py [--pairs 256] [--reps 20] [--mappoints 1000]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import extractorb_amd as X  # noqa: E402

SIDE = 512
CAM = X.camera_kb8(190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504, 0.0034823894022493434,
                   0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mappoints", type=int, default=1000)
    a = ap.parse_args()
    import torch
    rng = np.random.default_rng(1)
    ex = X.ORBextractor(1200, max_batch=2)
    cap, P, M = ex.capacity, a.pairs, a.mappoints
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    n, B = cap, 2 * a.pairs
    scale = np.asarray(X.compute_tables(1200, 1.2, 8)["scale_factors"], np.float32)
    k = np.zeros((B, cap), X.KEYPOINT_DTYPE)
    k["x"] = rng.uniform(0, SIDE, (B, n)); k["y"] = rng.uniform(0, SIDE, (B, n)); k["octave"] = rng.integers(0, 8, (B, n))
    k["angle"] = rng.uniform(0, 360, (B, n)); k["size"], k["class_id"] = 31, -1
    d = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    q = np.zeros((P, 2 * cap, 2), X.PROJ_QUERY_DTYPE); qd = np.zeros((P, 2 * cap, 32), np.uint8)
    for p in range(P):
        j = np.sort(rng.permutation(2 * cap)[:M])             # the request slots that hold a MapPoint
        obs = np.where(rng.random(M) < 0.85, 2, 0)
        for e in (0, 1):
            t = rng.integers(0, n, M)
            lv = k["octave"][2 * p + e, t]
            r = np.zeros(M, X.PROJ_QUERY_DTYPE)               # (a field of q[p, j, e] is a field of a copy: fill a record array, assign it whole)
            r["u"] = k["x"][2 * p + e, t] + rng.uniform(-3, 3, M); r["v"] = k["y"][2 * p + e, t] + rng.uniform(-3, 3, M)
            r["radius"] = np.float32(7.0) * scale[lv]
            r["min_level"], r["max_level"], r["flags"] = lv - 1, lv + 1, 1 | obs
            r["angle"] = (k["angle"][2 * p + e, t] + rng.uniform(0, 10, M)) % 360
            q[p, j, e] = r
            if e == 0:
                qd[p, j] = d[2 * p, t] ^ (rng.random((M, 32)) < 0.04).astype(np.uint8)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    d_k, d_d, d_n = dev(k.view(np.uint8)), dev(d), dev(np.full(B, n, np.int32))
    bounds = np.array([0, SIDE, 0, SIDE], np.float32)
    d_un = torch.zeros_like(d_k); d_off = torch.zeros((B, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    d_idx = torch.zeros((B, cap), dtype=torch.int32, device="cuda"); d_nin = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.frame_finish_two_eyes_device(P, d_k, d_n, cap, X.camera(190.98, 190.97, 254.93, 256.9), bounds, d_un, d_off, d_idx, d_nin)
    assert int((q["flags"] & 1).sum()) == 2 * P * M
    d_q, d_qd = dev(q.view(np.uint8)), dev(qd)
    d_qe = [dev(np.ascontiguousarray(q[:, :, e]).view(np.uint8)) for e in (0, 1)]
    d_occ = torch.zeros((P, 2, cap), dtype=torch.uint8, device="cuda"); d_occ1 = [torch.zeros((P, cap), dtype=torch.uint8, device="cuda") for _ in (0, 1)]
    d_m = torch.zeros((P, 2, cap), dtype=torch.int32, device="cuda"); d_m1 = [torch.zeros((P, cap), dtype=torch.int32, device="cuda") for _ in (0, 1)]
    d_nm = torch.zeros(P, dtype=torch.int32, device="cuda"); d_nm1 = [torch.zeros(P, dtype=torch.int32, device="cuda") for _ in (0, 1)]
    # the front half's inputs: every request slot of a last rig holds a MapPoint in front of the rig
    world = np.stack([rng.uniform(-4, 4, (B, cap)), rng.uniform(-4, 4, (B, cap)), rng.uniform(1, 8, (B, cap))], 2).astype(np.float32)
    poses = np.tile(np.eye(3, 4, dtype=np.float32), (P + 1, 1, 1)); poses[:, 2, 3] = np.arange(P + 1) * 0.01
    trl = np.eye(3, 4, dtype=np.float32); trl[0, 3] = -0.1
    d_fl, d_w, d_p = dev(np.full((B, cap), 3, np.uint8)), dev(world), dev(poses)
    d_fq = torch.zeros((P, 2 * cap, 2, 32), dtype=torch.uint8, device="cuda")

    def new(np_):
        d_occ.zero_()
        ex.search_last_frame_two_eyes_device(np_, (0, 1), d_q, d_qd, d_k, d_d, d_n, cap, d_off, d_idx, bounds, d_occ, True, d_m, d_nm)

    def two_launches(np_):
        for e in (0, 1):
            d_occ1[e].zero_()
            ex.search_by_projection_device(np_, (e, 2), d_qe[e], d_qd, (0, 1), None, 2 * cap, d_k, d_d, d_n, cap, d_off, d_idx, bounds, None,
                                           d_occ1[e], False, 0.9, True, d_m1[e], d_nm1[e])

    def front(np_):
        ex.project_last_frame_two_eyes_device(min(np_, P - 1) or 1, (0, 1), (1, 1), d_k, d_n, cap, d_fl, d_w, d_p, trl, CAM, bounds, 0.1, 7.0, False, d_fq)

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

    st = (C.c_int * 4)(); st1 = (C.c_int * 4)()
    out = dict(tool="last_frame_two_eyes_rate", source_hash=X.source_hash(), capacity=cap, keypoints_per_eye=n, mappoints=M, pairs=P, reps=a.reps,
               note="median of reps, microseconds; each search span includes its occupancy-reset memsets (one for the new entry, two for the two launches)")
    out["new_us_1pair"] = timed(new, 1)
    out["new_us_batch"] = timed(new, P)
    X.load_library().orbx_debug_last_frame_two_eyes_stats(st)
    out["new_rounds_pair0"], out["new_ticks_stage_scan_rounds_pair0"] = st[0], [st[1], st[2], st[3]]
    out["new_matches_mean"] = float(d_nm.float().mean())
    out["two_launches_us_1pair"] = timed(two_launches, 1)
    out["two_launches_us_batch"] = timed(two_launches, P)
    X.load_library().orbx_debug_search_rounds(st1)
    out["one_eye_rounds_pair0_right_launch"] = st1[0]
    out["two_launches_matches_mean"] = float((d_nm1[0] + d_nm1[1]).float().mean())
    out["front_half_us_batch"] = timed(front, P)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
