#!/usr/bin/env python3
"""Times orbx_frustum_requests_two_eyes_device (Frame::isInFrustumChecks per eye over a local map plus the prelude of the local-map projection
search for two-camera rigs, reference src/Frame.cc:571-581, :1181-1254, src/Tracking.cc:2941-2959, src/ORBmatcher.cc:50-73, :145-151) with
HIP events around spans of calls, in three shapes:
  1 x 4096, 1 x 16384 and 8 x 4096 MapPoints (pairs x list length; one list per pair, one rig pose for all)
Beside each, in the same process and alternately:
  one_eye  orbx_frustum_requests_device (k_frustum: one workgroup per list, the pinhole statement) on the same lists - the yardstick;
  search   orbx_search_by_projection_two_eyes_device on the slots the entry produced, with the query_capacity the entry was given: the count
           the list produced rounded up to 256, capped by what the search's LDS holds beside the frame (slots beyond it are dropped by the
           entry and reported in d_n_wanted).
A span is `calls` calls between two events; the figure is the median over `rounds` spans (21 x 20 by default) after three warm-up calls, with
the smallest and the largest, and a shader-clock sample.  No threshold: a measuring tool.  Prints one JSON line.

The scene: P uniform in [-6, 6] x [-4, 4] x [-1, 12] around a rig near the origin (10 cm baseline, a hundredth of a radian between the eyes),
mfMaxDistance in [2, 20], normals along the viewing ray plus noise; each eye holds 1200 keypoints anywhere in 512 x 512.
usage: frustum_two_eyes_rate.py [--rounds 21] [--calls 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import extractorb_amd as X  # noqa: E402

CAM_L = X.camera_kb8(190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504,
                     0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182)
CAM_R = X.camera_kb8(190.44236969414825, 190.4344384721956, 252.59949716835982, 254.91723064636983,
                     0.0034003170790442797, 0.001766278153469831, -0.00266312569781606, 0.0003299517423931039)
PINHOLE = (190.0, 190.0, 256.0, 256.0)
BOUNDS = np.array([0, 512, 0, 512], np.float32)
SHAPES = (("1x4096", 1, 4096), ("1x16384", 1, 16384), ("8x4096", 8, 4096))


def grid_of(x, y):
    """AssignFeaturesToGrid as CSR (cells x * 48 + y, push order) for the 512 x 512 bounds"""
    px = np.floor(x * np.float32(64.0 / 512.0) + 0.5).astype(np.int64); py = np.floor(y * np.float32(48.0 / 512.0) + 0.5).astype(np.int64)
    inside = (px >= 0) & (px < 64) & (py >= 0) & (py < 48)
    cell = np.where(inside, px * 48 + py, 64 * 48)
    order = np.argsort(cell, kind="stable")[:int(inside.sum())]
    off = np.zeros(64 * 48 + 1, np.int32); off[1:] = np.cumsum(np.bincount(cell[inside], minlength=64 * 48))
    return off, order.astype(np.int32)


def rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


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
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")       # noqa: E731
    # one rig frame: device frames 0 (left eye) and 1 (right eye)
    kps = np.zeros((2, cap), X.KEYPOINT_DTYPE); desc = rng.integers(0, 256, (2, cap, 32), dtype=np.uint8)
    off = np.zeros((2, 64 * 48 + 1), np.int32); idx = np.zeros((2, cap), np.int32)
    for e in (0, 1):
        kps["x"][e, :n] = rng.uniform(2, 510, n); kps["y"][e, :n] = rng.uniform(2, 510, n)
        kps["octave"][e, :n] = np.minimum(rng.geometric(0.35, n) - 1, 7)
        off[e], order = grid_of(kps["x"][e, :n], kps["y"][e, :n])
        idx[e, :len(order)] = order
    d_k, d_d, d_n, d_off, d_idx = dev(kps.view(np.uint8)), dev(desc), dev(np.full(2, n, np.int32)), dev(off), dev(idx)
    pose = np.array([[1, 0, 0, 0.07], [0, 1, 0, -0.03], [0, 0, 1, 0.1]], np.float32)
    Rrl = rot_y(-0.01)
    trl = np.concatenate([Rrl, [[-0.1], [0.001], [0.002]]], 1).astype(np.float32)
    tlr = np.concatenate([Rrl.T, (-Rrl.T @ trl[:, 3].astype(np.float64)).reshape(3, 1)], 1).astype(np.float32)
    # the largest query_capacity the search's LDS holds beside the frame (include/orbx.h: 100 B per keypoint of an eye, 8 per MapPoint, 12 392 B)
    qcap_max = (160 * 1024 - 512 - 12392 - 100 * ((cap + 3) & ~3)) // 8 // 256 * 256

    def lists(pairs, m):
        world = np.stack([rng.uniform(-6, 6, (pairs, m)), rng.uniform(-4, 4, (pairs, m)), rng.uniform(-1, 12, (pairs, m))], 2)
        PO = world + pose[:, 3].astype(np.float64)
        nrm = PO / np.linalg.norm(PO, axis=2, keepdims=True) + 0.6 * rng.standard_normal((pairs, m, 3))
        nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
        mf = rng.uniform(2, 20, (pairs, m))
        dist = np.stack([0.8 * mf / 1.2 ** 7, 1.2 * mf, mf], 2)
        flags = (rng.random((pairs, m)) < 0.93).astype(np.uint8) | ((rng.random((pairs, m)) < 0.8).astype(np.uint8) << 1)
        return [dev(world.astype(np.float32)), dev(nrm.astype(np.float32)), dev(dist.astype(np.float32)),
                dev(rng.integers(0, 256, (pairs, m, 32), dtype=np.uint8)), dev(flags), dev(rng.uniform(0, 12, (pairs, m)).astype(np.float32))]

    shapes = {}
    for label, pairs, m in SHAPES:
        outs = dict(q=u8(pairs, m, 2, 32), qd=u8(pairs, m, 32), src=i32(pairs, m), nq=i32(pairs), nw=i32(pairs), tr=u8(pairs, m, 2, 28), nin=i32(pairs),
                    q1=u8(pairs, m, 32), qd1=u8(pairs, m, 32), src1=i32(pairs, m), nq1=i32(pairs), tr1=u8(pairs, m, 28), nin1=i32(pairs),
                    matches=i32(pairs, 2, cap), nm=i32(pairs))
        shapes[label] = dict(pairs=pairs, m=m, bufs=lists(pairs, m), outs=outs, poses=dev(np.tile(pose.reshape(1, 12), (pairs, 1))), qcap=m)

    def two_eyes(s):
        (w, nv, dist, md, fl, prev), o = s["bufs"], s["outs"]
        ex.frustum_requests_two_eyes_device(s["pairs"], (0, 0), (0, 1), w, nv, dist, md, None, s["m"], fl, prev, s["poses"], trl, tlr, CAM_L, CAM_R, BOUNDS,
                                            s["qcap"], o["q"], o["qd"], o["src"], o["nq"], o["nw"], o["tr"], o["nin"], th=1.0, far_points=True,
                                            th_far_points=10.0)

    def one_eye(s):
        (w, nv, dist, md, fl, _), o = s["bufs"], s["outs"]
        ex.frustum_requests_device(s["pairs"], (0, 0), (0, 1), w, nv, dist, md, None, None, s["m"], fl, s["poses"], X.camera(*PINHOLE), BOUNDS, o["q1"],
                                   o["qd1"], o["src1"], o["nq1"], o["tr1"], o["nin1"], mode=X.FRUSTUM_LOCAL_MAP, mbf=40.0, th=1.0, far_points=True,
                                   th_far_points=10.0)

    def search(s):
        o = s["outs"]
        ex.search_by_projection_two_eyes_device(s["pairs"], (0, 0), o["q"], o["qd"], (0, 1), o["nq"], s["qcap"], d_k, d_d, d_n, cap, d_off, d_idx, BOUNDS,
                                                None, None, None, 0.8, o["matches"], o["nm"])

    out = dict(tool="frustum_two_eyes_rate", source_hash=X.source_hash(), capacity=cap, keypoints_per_eye=n, rounds=a.rounds, calls_per_span=a.calls,
               search_query_capacity_max=qcap_max,
               note="us per call: median over the rounds of (events around `calls` calls) / calls; two_eyes = k_frustum_two_eyes_check + "
                    "k_frustum_two_eyes_place (ceil(mappoints / 256) workgroups of 512 threads per pair, two launches), one_eye = k_frustum (one "
                    "workgroup of 1024 threads per list, pinhole) on the same lists, search = the two-eye projection search on the produced slots")
    for label, s in shapes.items():
        two_eyes(s)                                          # query_capacity = mappoints: the count the list produces
        torch.cuda.synchronize()
        wanted = s["outs"]["nw"].cpu().numpy()
        s["qcap"] = int(min(max(256, (int(wanted.max()) + 255) // 256 * 256), qcap_max, s["m"]))
        for _ in range(3):
            two_eyes(s); one_eye(s); search(s)
        torch.cuda.synchronize()
        tr = s["outs"]["tr"].cpu().numpy().reshape(-1, 2, 28)[:, :, 24:].copy().view(np.int32).reshape(-1, 2)
        out["shape_%s" % label] = dict(pairs=s["pairs"], mappoints=s["m"], slots_wanted_per_pair=round(float(wanted.mean()), 1), query_capacity=s["qcap"],
                                       slots_written_per_pair=round(float(s["outs"]["nq"].float().mean()), 1),
                                       in_view_per_pair=round(float(s["outs"]["nin"].float().mean()), 1),
                                       one_eye_requests_per_pair=round(float(s["outs"]["nq1"].float().mean()), 1),
                                       matches_per_pair=round(float(s["outs"]["nm"].float().mean()), 1),
                                       exits_left=np.bincount(tr[:, 0], minlength=7).tolist(), exits_right=np.bincount(tr[:, 1], minlength=7).tolist())
    calls = dict(("%s_%s" % (k, label), (f, s)) for label, s in shapes.items() for k, f in (("two_eyes", two_eyes), ("one_eye", one_eye), ("search", search)))
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


if __name__ == "__main__":
    main()
