#!/usr/bin/env python3
"""Times orbx_fuse_device (the search half of ORBmatcher::Fuse, reference src/ORBmatcher.cc:1399-1609) with HIP events around many calls, in
the two shapes of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:729-837):
  A  the current keyframe's 1000 MapPoints into 30 neighbour keyframes (mp_step = 0), capacity 1302
  B  30 000 candidate MapPoints into one keyframe
The shapes are timed alternately, round after round; the median over the rounds and the smallest and largest round are reported, with the
shader clock sampled beside the timed work.

Synthetic keyframes at the capacity of a 1200-feature extractor, 1200 keypoints each anywhere in a 640 x 480 image, 65 % with mvuRight >= 0;
60 % of a list's MapPoints sit on a keypoint of ONE of the keyframes (a pixel of noise per level, ~12 flipped descriptor bits, the keypoint's
level), the others are anywhere in front of the camera; 85 % of the flags are set.  In shape A a MapPoint so meets its keypoint in one of the 30
keyframes and an arbitrary window in the others.  Prints one JSON line.  usage: fuse_rate.py [--rounds 7] [--calls 100]"""
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
MBF = 47.9


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
    rng = np.random.default_rng(3)
    ex = X.ORBextractor(1200)
    cap, n, B = ex.capacity, 1200, 30
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    sf = np.asarray(ex.mvScaleFactor, np.float64)
    kps = np.zeros((B, cap), X.KEYPOINT_DTYPE); desc = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8); ur = np.full((B, cap), -1, np.float32)
    off = np.zeros((B, 64 * 48 + 1), np.int32); idx = np.zeros((B, cap), np.int32); poses = np.zeros((B, 3, 4))
    depth = rng.uniform(2, 9, (B, n))
    for f in range(B):
        kps["x"][f, :n] = rng.uniform(2, 638, n); kps["y"][f, :n] = rng.uniform(2, 478, n)
        kps["octave"][f, :n] = np.minimum(rng.geometric(0.35, n) - 1, 7)
        ur[f, :n] = np.where(rng.random(n) < 0.65, kps["x"][f, :n] - MBF / depth[f], -1)
        off[f], order = grid_of(kps["x"][f, :n], kps["y"][f, :n]); idx[f, :len(order)] = order
        ax, ay = rng.normal(0, 0.03, 2)
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        poses[f, :, :3] = Rx @ Ry; poses[f, :, 3] = rng.normal(0, 0.15, 3)

    def mappoints(m, frames):
        """m MapPoints, each built on a keyframe drawn from `frames`"""
        f = rng.choice(frames, m); j = rng.integers(0, n, m); on = rng.random(m) < 0.6
        o = np.where(on, kps["octave"][f, j], rng.integers(0, 8, m))
        z = np.where(on, depth[f, j], rng.uniform(1, 9, m))
        px = np.where(on, kps["x"][f, j] + rng.normal(0, 0.9, m) * sf[o], rng.uniform(-60, 700, m))
        py = np.where(on, kps["y"][f, j] + rng.normal(0, 0.9, m) * sf[o], rng.uniform(-40, 520, m))
        xc = np.stack([(px - CAM[2]) / CAM[0] * z, (py - CAM[3]) / CAM[1] * z, z], 1)
        R, t = poses[f, :, :3], poses[f, :, 3]
        world = np.einsum("mji,mj->mi", R, xc - t)
        Ow = -np.einsum("mji,mj->mi", R, t)
        d = np.linalg.norm(world - Ow, axis=1)
        mf = d * sf[o] * rng.uniform(0.93, 0.999, m)
        mdesc = np.where(on[:, None], desc[f, j] ^ np.packbits(rng.random((m, 256)) < 0.05, axis=1), rng.integers(0, 256, (m, 32), dtype=np.uint8))
        return (world.astype(np.float32), ((world - Ow) / d[:, None]).astype(np.float32),
                np.stack([0.8 * mf / sf[7], 1.2 * mf, mf], 1).astype(np.float32), mdesc.astype(np.uint8))

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    d_k, d_d, d_ur, d_n = dev(kps.view(np.uint8)), dev(desc), dev(ur), dev(np.full(B, n, np.int32))
    d_off, d_idx, d_pose = dev(off), dev(idx), dev(poses.astype(np.float32))
    cam = X.camera(*CAM)
    shapes = {}
    for label, pairs, m, frames in (("A", B, 1000, np.arange(B)), ("B", 1, 30000, np.arange(1))):
        w, nv, dist, md = mappoints(m, frames)
        bufs = [dev(w), dev(nv), dev(dist), dev(md), dev((rng.random((pairs, m)) < 0.85).astype(np.uint8))]
        outs = [torch.zeros((pairs, m), dtype=torch.int32, device="cuda"), torch.zeros((pairs, m), dtype=torch.int32, device="cuda"),
                torch.zeros((pairs, m), dtype=torch.uint8, device="cuda"), torch.zeros(pairs, dtype=torch.int32, device="cuda")]
        shapes[label] = (pairs, m, bufs, outs)

    def call(label):
        pairs, m, (w, nv, dist, md, fl), (bi, bd, exits, nf) = shapes[label]
        ex.fuse_device(pairs, (0, 1), (0, 0), w, nv, dist, md, None, m, fl, d_pose, d_k, d_ur, d_d, d_n, cap, d_off, d_idx, BOUNDS, cam, MBF, bi, bd, exits, nf)

    out = dict(tool="fuse_rate", source_hash=X.source_hash(), capacity=cap, keypoints=n, rounds=a.rounds, calls_per_span=a.calls,
               note="us per call (memset of d_n_fused + k_fuse): median over the rounds of (events around `calls` calls) / calls")
    for label in shapes:
        pairs, m, _, outs = shapes[label]
        for _ in range(3):
            call(label)
        torch.cuda.synchronize()
        out["shape_%s" % label] = dict(pairs=pairs, mappoints=m, fused_per_pair=round(float(outs[3].float().mean()), 1),
                                       exits=np.bincount(outs[2].cpu().numpy().ravel(), minlength=8).tolist())
    ts = {label: [] for label in shapes}
    slot = 0
    for _ in range(a.rounds):
        for label in ts:                                     # alternating: a drift of the machine lands on both
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for c in range(a.calls):
                call(label)
                if c == a.calls // 2 and slot < 60:
                    ex.clock_probe(slot); slot += 1
            e1.record()
            torch.cuda.synchronize()
            ts[label].append(e0.elapsed_time(e1) * 1000.0 / a.calls)
    for label, v in ts.items():
        out["us_%s" % label] = round(float(np.median(v)), 2)
        out["us_%s_minmax" % label] = [round(min(v), 2), round(max(v), 2)]
        out["us_%s_rounds" % label] = [round(x, 2) for x in v]
    ghz = ex.clock_read(slot)
    out["shader_clock_ghz_minmax"] = [round(float(min(ghz)), 3), round(float(max(ghz)), 3)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
