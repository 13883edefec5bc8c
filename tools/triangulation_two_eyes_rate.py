#!/usr/bin/env python3
"""Times orbx_search_for_triangulation_two_eyes_device (ORBmatcher::SearchForTriangulation on two-camera keyframes, reference
src/ORBmatcher.cc:965-1206 with the branches :994-1004 and :1099-1129) at the real size - 1302 keypoints per eye, one keyframe against 4
neighbours, a 300-node vocabulary (the scene of tests/test_search_triangulation_two_eyes_gpu.py) - with events around many calls, and beside
it orbx_search_for_triangulation_device on the same keypoint counts: every rig as ONE frame of 2604 stacked keypoints with the stacked
FeatureVector, F12 of the left-left pose through a pinhole of the fisheye's focal length (what it accepts is not compared: the yardstick is
its time on as many candidates).  The medians over the rounds are reported.  Run it under `rocprofv3 --kernel-trace --stats -- python
tools/triangulation_two_eyes_rate.py --calls 20 --rounds 3` for the per-kernel table.
torch is asked for the GPU BEFORE the library is loaded: a process whose first HIP call is the library's leaves torch without a device.
Prints one JSON line.  usage: triangulation_two_eyes_rate.py [--rounds 7] [--calls 100]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "no GPU"
    torch.zeros(1, device="cuda")                       # torch's runtime first
    import extractorb_amd as X
    import triangulation_two_eyes_scenes as S
    import triangulation_two_eyes_walk as W

    def dev(x):
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.view(np.uint8) if x.dtype.fields else x).cuda()

    s = S.make(21, cap=1302, n_points=1500, rigs=5, nan_rig=-1, skew=0.02, nodes=300, dup=40, decoys=8)
    pairs = [(0, b) for b in (1, 2, 3, 4)]
    cap, P = 1302, len(pairs)
    d = dict((k, dev(v)) for k, v in S.pack(s, pairs, cap).items())
    ex = X.ORBextractor(1000, 1.2, 8)
    m12 = torch.zeros((P, 2, cap), dtype=torch.int32, device="cuda"); out_pairs = torch.zeros((P, 2 * cap, 2), dtype=torch.int32, device="cuda")
    n = torch.zeros(P, dtype=torch.int32, device="cuda")
    cams = (X.camera_kb8(*s["cams"][0]), X.camera_kb8(*s["cams"][1]))

    def two_eyes(n_pairs):
        ex.search_for_triangulation_two_eyes_device(n_pairs, (0, 0), (1, 1), d["fn"], d["fi"], d["nfeat"], d["fl1"], d["fl2"], d["poses"], s["tlr"],
                                                    cams[0], cams[1], d["kps"], d["desc"], d["nout"], cap, m12, out_pairs, n)

    # the one-camera yardstick: rig X as one frame of the stacked keypoints
    cap1 = 2 * cap
    R = len(s["kfs"])
    kps1 = np.zeros((R, cap1), X.KEYPOINT_DTYPE); desc1 = np.zeros((R, cap1, 32), np.uint8)
    fn1 = np.zeros((R, cap1), np.uint32); fi1 = np.zeros((R, cap1), np.uint32); n1 = np.zeros(R, np.int32)
    for x, kf in enumerate(s["kfs"]):
        fv = W.stacked_feature_vector(kf)
        k = np.concatenate([e["kps"] for e in kf["eyes"]]); dd = np.concatenate([e["desc"] for e in kf["eyes"]])
        kps1[x, :len(k)] = k; desc1[x, :len(k)] = dd; n1[x] = len(k)
        nodes = np.array([node for node, lst in fv for _ in lst], np.uint32); idx = np.array([i for _, lst in fv for i in lst], np.uint32)
        fn1[x, :len(idx)] = nodes; fi1[x, :len(idx)] = idx
    f12 = np.zeros((P, 9), np.float32); ep = np.zeros((P, 2), np.float32)
    K = np.array([[190.97, 0, 254.93], [0, 190.97, 256.9], [0, 0, 1]]); Kin = np.linalg.inv(K)
    for p, (x, y) in enumerate(pairs):
        R12, t12 = S.relative64(s["kfs"][x]["pose"], s["kfs"][y]["pose"], 0, 0)
        tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
        f12[p] = (Kin.T @ tx @ R12 @ Kin).reshape(9)
        c2 = K @ (-R12.T @ t12); ep[p] = c2[:2] / c2[2]
    fl = np.zeros((P, cap1), np.uint8)
    g = dict(kps=dev(kps1), desc=dev(desc1), fn=dev(fn1), fi=dev(fi1), n=dev(n1), f12=dev(f12), ep=dev(ep), fl=dev(fl))
    m1 = torch.zeros((P, cap1), dtype=torch.int32, device="cuda"); p1 = torch.zeros((P, cap1, 2), dtype=torch.int32, device="cuda")

    def one_camera(n_pairs):
        ex.search_for_triangulation_device(n_pairs, (0, 0), (1, 1), g["fn"], g["fi"], g["n"], g["fl"], g["fl"], g["kps"], None, g["desc"], g["n"], cap1,
                                           g["f12"], g["ep"], m1, p1, n)

    ex.set_stream(torch.cuda.current_stream().cuda_stream)

    def span(fn, n_pairs):
        fn(n_pairs); torch.cuda.synchronize()
        t = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn(n_pairs)
            e1.record(); torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 1000.0 / a.calls)
        return float(np.median(t))

    out = dict(two_eyes_1_pair_us=span(two_eyes, 1), two_eyes_4_pairs_us=span(two_eyes, 4), one_camera_1_pair_us=span(one_camera, 1),
               one_camera_4_pairs_us=span(one_camera, 4), keypoints_per_eye=cap, rounds=a.rounds, calls=a.calls)
    ex.search_triangulation_two_eyes_count(True)          # (the timed calls above ran without the counters)
    two_eyes(4); ex.synchronize()
    out["matches"] = n.cpu().numpy().tolist()
    out["triangulations"], out["within_th_low"] = ex.search_triangulation_two_eyes_stats()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
