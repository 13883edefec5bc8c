#!/usr/bin/env python3
"""Times orbx_stereo_fisheye_match_device (Frame::ComputeStereoFishEyeMatches, reference src/Frame.cc:1139-1179) at the real size - 1302
keypoints per eye, 1152 x 1150 lapping rows (the scene of tests/test_stereo_fisheye_gpu.py, its four rigs repeated) - for 1, 16 and 256 rigs
per call, with events around many calls; the medians over the rounds are reported.  Beside it:
  * the same call on rigs whose right descriptors are all equal (d0 = d1 on every row: nothing passes the ratio test, so no wave enters
    stage B): the difference is stage B's share;
  * orbx_kb8_triangulate_device over as many pairs as passed the ratio test: the floor of stage B;
  * the kernel's source compiled for the host, one thread (tests/cpp/stereo_fisheye_host_check.cpp): what a caller pays today, without
    the copies;
  * orbx_extract_batch_device of as many 640 x 480 frames (1200 features), so the reader sees what share of a frame this step is.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/stereo_fisheye_rate.py --calls 20 --rounds 3` for the per-kernel table.
torch is asked for the GPU BEFORE the library is loaded: a process whose first HIP call is the library's leaves torch without a device.
Prints one JSON line.  usage: stereo_fisheye_rate.py [--rounds 7] [--calls 50] [--rigs 1,16,256]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rigs", default="1,16,256")
    a = ap.parse_args()
    shapes = [int(v) for v in a.rigs.split(",")]
    import torch
    assert torch.cuda.is_available(), "no GPU"
    torch.zeros(1, device="cuda")                       # torch's runtime first
    import extractorb_amd as X
    import stereo_fisheye_scenes as SC
    import test_stereo_fisheye as T
    from extractorb_amd import synth

    def dev(x):
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.view(np.uint8) if x.dtype.fields else x).cuda()

    cap, R = 1302, max(shapes)
    rigs = SC.make_real(31)
    packed = SC.pack(rigs, cap)
    reps = (R + len(rigs) - 1) // len(rigs)
    d = dict((k, dev(np.concatenate([v] * reps)[:2 * R])) for k, v in packed.items())
    flat = packed["desc"].copy(); flat[1::2] = 0x5a     # every right descriptor the same: d0 = d1, the ratio test rejects every row
    d_flat = dev(np.concatenate([flat] * reps)[:2 * R])
    ex = X.ORBextractor(1200, 1.2, 8, max_width=640, max_height=480, max_batch=2 * min(R, 64))
    l2r = torch.zeros((2 * R, cap), dtype=torch.int32, device="cuda"); r2l = torch.zeros_like(l2r)
    depth = torch.zeros((2 * R, cap), device="cuda"); x3d = torch.zeros((2 * R, cap, 3), device="cuda")
    n = torch.zeros(R, dtype=torch.int32, device="cuda"); nd = torch.zeros(R, dtype=torch.int32, device="cuda")
    cams = (X.camera_kb8(*SC.CAMS[0]), X.camera_kb8(*SC.CAMS[1]))
    ex.set_stream(torch.cuda.current_stream().cuda_stream)

    def match(n_rigs, desc=None):
        ex.stereo_fisheye_match_device(n_rigs, (0, 1), d["kps"], d["desc"] if desc is None else desc, d["nout"], d["mono"], cap, SC.TLR, cams[0], cams[1],
                                       l2r, r2l, depth, x3d, n, nd)

    def span(fn, calls=None):
        calls = calls or a.calls
        fn(); torch.cuda.synchronize()
        t = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record(); torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 1000.0 / calls)
        return float(np.median(t))

    out = dict(keypoints_per_eye=cap, rounds=a.rounds, calls=a.calls)
    match(R); ex.synchronize()
    passed = nd.cpu().numpy()
    out["matches_per_rig"] = n.cpu().numpy()[:4].tolist(); out["ratio_passes_per_rig"] = passed[:4].tolist()
    # the floor of stage B: the parent's triangulation kernel over as many pairs
    uv = dev(np.random.default_rng(0).uniform(60, 450, (int(passed.sum()), 2)).astype(np.float32))
    z = torch.zeros(int(passed.sum()), device="cuda"); x = torch.zeros((int(passed.sum()), 3), device="cuda")
    for r in shapes:
        calls = max(5, a.calls // max(1, r // 16))
        pairs = int(passed[:r].sum())
        full = span(lambda: match(r), calls); stage_a = span(lambda: match(r, d_flat), calls)
        floor = span(lambda: ex.kb8_triangulate_device(pairs, uv, uv, SC.CAMS[0], SC.CAMS[1], SC.TLR[:, :3], SC.TLR[:, 3], 1.0, 1.0, z, x), calls)
        out["rigs_%d" % r] = dict(call_us=full, per_rig_us=full / r, no_survivor_call_us=stage_a, stage_b_share=(full - stage_a) / full,
                                  kb8_triangulate_pairs=pairs, kb8_triangulate_us=floor)
    # the extraction of the same rigs' frames (two per rig), in batches of at most 128 frames
    frames = 2 * min(R, 64)
    img = dev(np.stack([synth.frames("textured", i % 8, 1, 480, 640)[0] for i in range(frames)]))
    ecap = ex.capacity
    ek = torch.zeros((frames, ecap, 28), dtype=torch.uint8, device="cuda"); ed = torch.zeros((frames, ecap, 32), dtype=torch.uint8, device="cuda")
    en = torch.zeros(frames, dtype=torch.int32, device="cuda"); em = torch.zeros(frames, dtype=torch.int32, device="cuda")
    for r in shapes:
        f = 2 * min(r, 64)
        t = span(lambda: ex.extract_batch_device(img, f, 480, 640, ek, ed, en, em, ecap), max(5, a.calls // max(1, r // 4)))
        out["rigs_%d" % r]["extract_frames"] = f
        out["rigs_%d" % r]["extract_per_rig_us"] = t / (f // 2)
    out["extract_capacity"] = ecap
    # the host-compiled kernel, one thread
    host = T.build_host(tempfile.mkdtemp())
    T.host_run(host, rigs, cap)
    t0 = time.perf_counter()
    for _ in range(3):
        T.host_run(host, rigs, cap)
    out["host_one_thread_per_rig_us"] = (time.perf_counter() - t0) / 3 / len(rigs) * 1e6
    print(json.dumps(out))


if __name__ == "__main__":
    main()
