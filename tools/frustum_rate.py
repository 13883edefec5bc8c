#!/usr/bin/env python3
"""Times orbx_frustum_requests_device (Frame::isInFrustum over a local map plus the prelude of the local-map projection search, reference
src/Frame.cc:493-570, src/Tracking.cc:2941-2959, src/ORBmatcher.cc:50-73) with HIP events around spans of calls, in three shapes:
  1 x 4096, 1 x 16384 and 8 x 4096 MapPoints (pairs x list length; one list per pair, one frame for all)
Beside each, in the same run and alternately:
  search   orbx_search_by_projection_device (k_search_proj, ratio_mode 1) on the requests the entry produced - what the front half feeds.
           With one pair the search is given query_capacity = the request count rounded up to 256 (the requests are compacted, and with one
           pair any capacity at or above the count addresses the same slots); with several pairs it must be mp_capacity.
  project  orbx_project_last_frame_device (k_project_last) at the same count of keypoints - the front half of the frame-to-frame search,
           one thread per keypoint over as many workgroups as it takes, no compaction: the yardstick for "one workgroup per list".
A span is `calls` calls between two events; the figure is the median over `rounds` spans (21 x 20 by default) after three warm-up calls.
No threshold: a measuring tool.  Prints one JSON line.

The scene: P uniform in [-6, 6] x [-4, 4] x [-1, 12] around a camera near the origin, mfMaxDistance in [2, 20], normals along the viewing ray
plus noise (about a quarter of a list reaches a request); the frame holds 1200 keypoints anywhere in 640 x 480.
usage: frustum_rate.py [--rounds 21] [--calls 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import extractorb_amd as X  # noqa: E402

CAM = (520.0, 520.0, 320.0, 240.0)
BOUNDS = np.array([0, 640, 0, 480], np.float32)
SHAPES = (("1x4096", 1, 4096), ("1x16384", 1, 16384), ("8x4096", 8, 4096))


def grid_of(x, y):
    """AssignFeaturesToGrid as CSR (cells x * 48 + y, push order)"""
    px = np.floor(x * np.float32(0.1) + 0.5).astype(np.int64); py = np.floor(y * np.float32(0.1) + 0.5).astype(np.int64)
    inside = (px >= 0) & (px < 64) & (py >= 0) & (py < 48)
    cell = np.where(inside, px * 48 + py, 64 * 48)
    order = np.argsort(cell, kind="stable")[:int(inside.sum())]
    off = np.zeros(64 * 48 + 1, np.int32); off[1:] = np.cumsum(np.bincount(cell[inside], minlength=64 * 48))
    return off, order.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    import torch
    rng = np.random.default_rng(4)
    ex = X.ORBextractor(1200)
    cap, n = ex.capacity, 1200
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")      # noqa: E731
    kps = np.zeros((1, cap), X.KEYPOINT_DTYPE); desc = rng.integers(0, 256, (1, cap, 32), dtype=np.uint8)
    kps["x"][0, :n] = rng.uniform(2, 638, n); kps["y"][0, :n] = rng.uniform(2, 478, n)
    kps["octave"][0, :n] = np.minimum(rng.geometric(0.35, n) - 1, 7)
    off, order = grid_of(kps["x"][0, :n], kps["y"][0, :n])
    idx = np.zeros((1, cap), np.int32); idx[0, :len(order)] = order
    d_k, d_d, d_n, d_off, d_idx = dev(kps.view(np.uint8)), dev(desc), dev(np.full(1, n, np.int32)), dev(off[None, :]), dev(idx)
    pose = np.array([[1, 0, 0, 0.07], [0, 1, 0, -0.03], [0, 0, 1, 0.1]], np.float32)
    cam = X.camera(*CAM)

    def lists(pairs, m):
        world = np.stack([rng.uniform(-6, 6, (pairs, m)), rng.uniform(-4, 4, (pairs, m)), rng.uniform(-1, 12, (pairs, m))], 2)
        PO = world + pose[:, 3].astype(np.float64)
        nrm = PO / np.linalg.norm(PO, axis=2, keepdims=True) + 0.6 * rng.standard_normal((pairs, m, 3))
        nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
        mf = rng.uniform(2, 20, (pairs, m))
        dist = np.stack([0.8 * mf / 1.2 ** 7, 1.2 * mf, mf], 2)
        flags = (rng.random((pairs, m)) < 0.93).astype(np.uint8) | ((rng.random((pairs, m)) < 0.8).astype(np.uint8) << 1)
        return [dev(world.astype(np.float32)), dev(nrm.astype(np.float32)), dev(dist.astype(np.float32)),
                dev(rng.integers(0, 256, (pairs, m, 32), dtype=np.uint8)), dev(flags)]

    shapes = {}
    for label, pairs, m in SHAPES:
        bufs = lists(pairs, m)
        outs = dict(q=torch.zeros((pairs, m, 32), dtype=torch.uint8, device="cuda"), qd=torch.zeros((pairs, m, 32), dtype=torch.uint8, device="cuda"),
                    src=i32(pairs, m), nq=i32(pairs), tr=torch.zeros((pairs, m, 28), dtype=torch.uint8, device="cuda"), nin=i32(pairs),
                    matches=i32(pairs, cap), nm=i32(pairs), pq=torch.zeros((pairs, m, 32), dtype=torch.uint8, device="cuda"))
        # k_project_last's inputs at the same count: `pairs` frames of m keypoints, each projected under its own pose
        lk = np.zeros((pairs, m), X.KEYPOINT_DTYPE); lk["octave"] = rng.integers(0, 8, (pairs, m))
        last = dict(k=dev(lk.view(np.uint8)), n=dev(np.full(pairs, m, np.int32)), poses=dev(np.tile(pose.reshape(1, 12), (pairs, 1))))
        shapes[label] = dict(pairs=pairs, m=m, bufs=bufs, outs=outs, last=last, qcap=m)

    def frustum(s):
        (w, nv, dist, md, fl), o = s["bufs"], s["outs"]
        ex.frustum_requests_device(s["pairs"], (0, 0), (0, 1), w, nv, dist, md, None, None, s["m"], fl, s["last"]["poses"], cam, BOUNDS, o["q"], o["qd"],
                                   o["src"], o["nq"], o["tr"], o["nin"], mode=X.FRUSTUM_LOCAL_MAP, mbf=40.0, th=1.0)

    def search(s):
        o = s["outs"]
        ex.search_by_projection_device(s["pairs"], (0, 0), o["q"], o["qd"], (0, 1), o["nq"], s["qcap"], d_k, d_d, d_n, cap, d_off, d_idx, BOUNDS, None, None,
                                       True, 0.8, False, o["matches"], o["nm"])

    def project(s):
        (w, _, _, _, fl), o, l = s["bufs"], s["outs"], s["last"]
        ex.project_last_frame_device(s["pairs"], (0, 1), (0, 1), l["k"], l["k"], l["n"], s["m"], fl, w, l["poses"], cam, BOUNDS, 40.0, 0.08, 15.0, True, o["pq"])

    out = dict(tool="frustum_rate", source_hash=X.source_hash(), capacity=cap, keypoints=n, rounds=a.rounds, calls_per_span=a.calls,
               note="us per call: median over the rounds of (events around `calls` calls) / calls; frustum = k_frustum (one workgroup of 1024 "
                    "threads per list), search = k_search_proj (ratio_mode 1) on the requests it produced, project = k_project_last at the same count")
    for label, s in shapes.items():
        frustum(s)
        torch.cuda.synchronize()
        nq = s["outs"]["nq"].cpu().numpy()
        if s["pairs"] == 1:
            s["qcap"] = max(256, (int(nq[0]) + 255) // 256 * 256)
        for _ in range(3):
            frustum(s); search(s); project(s)
        torch.cuda.synchronize()
        out["shape_%s" % label] = dict(pairs=s["pairs"], mappoints=s["m"], requests_per_pair=round(float(nq.mean()), 1), search_query_capacity=s["qcap"],
                                       in_view_per_pair=round(float(s["outs"]["nin"].float().mean()), 1),
                                       matches_per_pair=round(float(s["outs"]["nm"].float().mean()), 1), search_rounds_pair0=int(ex_rounds()[0]),
                                       exits=np.bincount(s["outs"]["tr"].cpu().numpy().reshape(-1, 28)[:, 24:].copy().view(np.int32).ravel(), minlength=7).tolist())
    calls = dict(("%s_%s" % (k, label), (f, s)) for label, s in shapes.items() for k, f in (("frustum", frustum), ("search", search), ("project", project)))
    ts = {k: [] for k in calls}
    slot = 0
    for _ in range(a.rounds):
        for k, (f, s) in calls.items():                      # alternating: a drift of the machine lands on all of them
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for c in range(a.calls):
                f(s)
                if c == a.calls // 2 and slot < 60:
                    ex.clock_probe(slot); slot += 1
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1000.0 / a.calls)
    for k, v in ts.items():
        out["us_%s" % k] = round(float(np.median(v)), 2)
        out["us_%s_minmax" % k] = [round(min(v), 2), round(max(v), 2)]
    ghz = ex.clock_read(slot)
    out["shader_clock_ghz_minmax"] = [round(float(min(ghz)), 3), round(float(max(ghz)), 3)]
    print(json.dumps(out))


def ex_rounds():
    import ctypes as C
    r = (C.c_int * 4)()
    X.load_library().orbx_debug_search_rounds(r)
    return list(r)


if __name__ == "__main__":
    main()
