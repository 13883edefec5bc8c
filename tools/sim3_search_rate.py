#!/usr/bin/env python3
"""Times orbx_search_by_projection_sim3_device (the Sim3 overloads of ORBmatcher::SearchByProjection, reference src/ORBmatcher.cc:473-586 and
:588-704) with HIP events around many calls, in two shapes of LoopClosing:
  A  4 loop candidates x 2000 MapPoints into one keyframe of capacity 1302 (kf_step = 0), th 8, ratio 1.5, the second overload's projection
  B  one candidate x 8000 MapPoints, th 3, ratio 1.5, the first overload's projection
Beside each, orbx_fuse_device(reproj_check = 0) on the SAME data and with the same th is timed as the yardstick, alternately in the same run:
that call is the same front end and the same window scan without the closing, so the difference is the price of the sequential rule (the key
lists, the settling workgroup, its rounds).  Rounds and re-scans of the search are reported beside the times.  No threshold: a measuring tool.

Synthetic keyframe at the capacity of a 1200-feature extractor, 1200 keypoints anywhere in a 640 x 480 image; 60 % of a list's MapPoints sit
on a keypoint (a pixel of noise per level, ~12 flipped descriptor bits, the keypoint's level), so in shape B four MapPoints want every second
keypoint; the others are anywhere in front of the camera; 85 % of the flags are set.  All pairs of shape A carry the keyframe's own pose (the
Fuse entry takes its pose per frame).  Prints one JSON line.  usage: sim3_search_rate.py [--rounds 7] [--calls 100]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import extractorb_amd as X  # noqa: E402

CAM = (458.654, 457.296, 317.215, 238.375)
BOUNDS = np.array([0, 640, 0, 480], np.float32)


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    a = ap.parse_args()
    import torch
    rng = np.random.default_rng(4)
    ex = X.ORBextractor(1200)
    cap, n = ex.capacity, 1200
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    sf = np.asarray(ex.mvScaleFactor, np.float64)
    kps = np.zeros((1, cap), X.KEYPOINT_DTYPE); desc = rng.integers(0, 256, (1, cap, 32), dtype=np.uint8)
    depth = rng.uniform(2, 9, n)
    kps["x"][0, :n] = rng.uniform(2, 638, n); kps["y"][0, :n] = rng.uniform(2, 478, n)
    kps["octave"][0, :n] = np.minimum(rng.geometric(0.35, n) - 1, 7)
    off, order = grid_of(kps["x"][0, :n], kps["y"][0, :n])
    idx = np.zeros((1, cap), np.int32); idx[0, :len(order)] = order
    ax, ay = rng.normal(0, 0.03, 2)
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    R = Rx @ Ry; t = rng.normal(0, 0.15, 3)
    pose = np.concatenate([R, t[:, None]], axis=1).astype(np.float32)

    def mappoints(m):
        j = rng.integers(0, n, m); on = rng.random(m) < 0.6
        o = np.where(on, kps["octave"][0, j], rng.integers(0, 8, m))
        z = np.where(on, depth[j], rng.uniform(1, 9, m))
        px = np.where(on, kps["x"][0, j] + rng.normal(0, 0.9, m) * sf[o], rng.uniform(-60, 700, m))
        py = np.where(on, kps["y"][0, j] + rng.normal(0, 0.9, m) * sf[o], rng.uniform(-40, 520, m))
        xc = np.stack([(px - CAM[2]) / CAM[0] * z, (py - CAM[3]) / CAM[1] * z, z], 1)
        world = (xc - t) @ R
        Ow = -R.T @ t
        d = np.linalg.norm(world - Ow, axis=1)
        mf = d * sf[o] * rng.uniform(0.93, 0.999, m)
        mdesc = np.where(on[:, None], desc[0, j] ^ np.packbits(rng.random((m, 256)) < 0.05, axis=1), rng.integers(0, 256, (m, 32), dtype=np.uint8))
        return (world.astype(np.float32), ((world - Ow) / d[:, None]).astype(np.float32),
                np.stack([0.8 * mf / sf[7], 1.2 * mf, mf], 1).astype(np.float32), mdesc.astype(np.uint8))

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    d_k, d_d, d_n = dev(kps.view(np.uint8)), dev(desc), dev(np.full(1, n, np.int32))
    d_off, d_idx = dev(off[None, :]), dev(idx)
    cam = X.camera(*CAM)
    shapes = {}
    for label, pairs, m, th, projection in (("A", 4, 2000, 8.0, 1), ("B", 1, 8000, 3.0, 0)):
        parts = [mappoints(m) for _ in range(pairs)]
        bufs = [dev(np.stack([p[k] for p in parts])) for k in range(4)] + [dev((rng.random((pairs, m)) < 0.85).astype(np.uint8))]
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")      # noqa: E731
        outs = dict(matches=i32(pairs, cap), mi=i32(pairs, m), md=i32(pairs, m), ex=torch.zeros((pairs, m), dtype=torch.uint8, device="cuda"), nm=i32(pairs),
                    bi=i32(pairs, m), bd=i32(pairs, m), fex=torch.zeros((pairs, m), dtype=torch.uint8, device="cuda"), nf=i32(pairs))
        shapes[label] = (pairs, m, th, projection, bufs, outs, dev(np.tile(pose.reshape(1, 12), (pairs, 1))))

    def search(label):
        pairs, m, th, projection, (w, nv, dist, md, fl), o, d_pose = shapes[label]
        ex.search_by_projection_sim3_device(pairs, (0, 0), (0, 1), w, nv, dist, md, None, m, fl, d_pose, d_k, d_d, d_n, cap, d_off, d_idx, BOUNDS, cam,
                                            None, o["matches"], o["mi"], o["md"], o["ex"], o["nm"], projection=projection, th=th, th_low=50,
                                            ratio_hamming=1.5)

    def fuse(label):
        pairs, m, th, projection, (w, nv, dist, md, fl), o, d_pose = shapes[label]
        ex.fuse_device(pairs, (0, 0), (0, 1), w, nv, dist, md, None, m, fl, d_pose, d_k, None, d_d, d_n, cap, d_off, d_idx, BOUNDS, cam, 0.0,
                       o["bi"], o["bd"], o["fex"], o["nf"], th=th, th_low=75, reproj_check=False)

    out = dict(tool="sim3_search_rate", source_hash=X.source_hash(), capacity=cap, keypoints=n, rounds=a.rounds, calls_per_span=a.calls,
               note="us per call: median over the rounds of (events around `calls` calls) / calls; search = k_sim3_window + k_sim3_settle, "
                    "fuse = memset + k_fuse with reproj_check 0 on the same data (the yardstick: no closing)")
    for label in shapes:
        pairs, m, th, projection, _, o, _ = shapes[label]
        for _ in range(3):
            search(label); fuse(label)
        torch.cuda.synchronize()
        st = ex.debug_sim3_search_stats()
        out["shape_%s" % label] = dict(pairs=pairs, mappoints=m, th=th, projection=projection, matches_per_pair=round(float(o["nm"].float().mean()), 1),
                                       fused_per_pair=round(float(o["nf"].float().mean()), 1), rounds_pair0=st[0], rescans=st[1], settle_ticks_pair0=st[2],
                                       exits=np.bincount(o["ex"].cpu().numpy().ravel(), minlength=8).tolist())
    calls = dict(("%s_%s" % (k, label), (f, label)) for label in shapes for k, f in (("search", search), ("fuse", fuse)))
    ts = {k: [] for k in calls}
    slot = 0
    for _ in range(a.rounds):
        for k, (f, label) in calls.items():                  # alternating: a drift of the machine lands on all four
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for c in range(a.calls):
                f(label)
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


if __name__ == "__main__":
    main()
