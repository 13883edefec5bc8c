#!/usr/bin/env python3
"""Times orbx_reconstruct_two_views_device (TwoViewReconstruction::Reconstruct, reference src/TwoViewReconstruction.cc:39-125) at the
monocular initialisation's size: frames of 1000 keypoints, 300 of them matched (the scene generator of tests/two_view_scenes.py: general
depth, 0.3 px noise, 10 % gross outliers), 200 iterations, for 1, 16 and 256 pairs per call - every pair names the same two frames and has
its own draws - with events around back-to-back calls; the medians over the rounds are reported.  Beside it the same header compiled for
the host on one thread (tests/cpp/two_view_host_check.cpp): what a caller pays today, without the copies of the match table and the
points.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/two_view_rate.py --calls 5 --rounds 2 --pairs 16` for the
per-kernel split.  torch is asked for the GPU BEFORE the library is loaded.
Prints one JSON line.  usage: two_view_rate.py [--rounds 7] [--calls 20] [--pairs 1,16,256] [--shape 1] [--no-host]"""
import argparse
import ctypes as C
import json
import os
import subprocess
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--pairs", default="1,16,256")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--shape", type=int, default=1, help="the hypothesis kernel: 1 rows over the lanes (default), 0 one lane out of LDS")
    a = ap.parse_args()
    shapes = [int(v) for v in a.pairs.split(",")]
    import torch
    assert torch.cuda.is_available(), "no GPU"
    torch.zeros(1, device="cuda")                       # torch's runtime first
    import extractorb_amd as X
    import two_view_scenes as SC
    import two_view_walk as TW

    s = SC.make("general", 300, 1, iterations=200, pairs=max(shapes), shape="twice", cap=1000, n_keys=1000)
    ex = X.ORBextractor(1000, 1.2, 8)
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    ex.two_view_shape(a.shape)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8) if v.dtype.fields else np.ascontiguousarray(v)).cuda()
    o = SC.poisoned_outputs(s)
    d = dict((k, dev(v)) for k, v in o.items())
    kps, n_out, rnd, cam = dev(s["kps"]), dev(s["n_out"]), dev(s["rand"]), X.camera(*s["cam"])

    def call(P):
        ex.reconstruct_two_views_device(P, s["frames1"], s["frames2"], kps, n_out, s["cap"], d["matches"], d["n_matches"], cam, rnd, d["result"],
                                        d["p3d"], d["tri"], iterations=200, prune=False)

    def span(fn, calls):
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

    out = dict(keypoints=1000, matches=int(s["n_matches"][0]), iterations=200, shape=a.shape, rounds=a.rounds, calls=a.calls, us_per_call={})
    for P in shapes:
        out["us_per_call"][str(P)] = round(span(lambda: call(P), a.calls), 1)
    torch.cuda.synchronize()
    status = d["result"].cpu().numpy().view(SC.RESULT_DTYPE).reshape(-1)["status"]
    out["statuses"] = dict((TW.STATUS[v], int((status == v).sum())) for v in np.unique(status))
    if not a.no_host:
        with tempfile.TemporaryDirectory() as td:
            so = os.path.join(td, "libtwo_view_host.so")
            inc = ["-I" + os.path.join(ROOT, *q) for q in (("tests", "cpp"), ("tests", "cpp", "host_shim"), ("extractorb_amd", "csrc"), ("include",))]
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", *inc,
                                   os.path.join(ROOT, "tests", "cpp", "two_view_host_check.cpp"), "-o", so])
            L = C.CDLL(so)
            VP = C.c_void_p
            L.tv_host.argtypes = [C.c_int] * 5 + [VP, VP, C.c_int, VP, VP, VP, C.c_float, C.c_int, C.c_float, C.c_int, C.c_float, VP, C.c_int, VP, VP, VP]
            L.tv_host.restype = None
            h = SC.poisoned_outputs(s)
            ptr = lambda v: v.ctypes.data_as(VP)
            cam4 = np.array(s["cam"], np.float32)
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                L.tv_host(1, 0, 0, 1, 0, ptr(s["kps"]), ptr(s["n_out"]), s["cap"], ptr(h["matches"]), ptr(h["n_matches"]), ptr(cam4), 1.0, 200, 1.0, 50, 0.5,
                          ptr(s["rand"]), 0, ptr(h["result"]), ptr(h["p3d"]), ptr(h["tri"]))
                t.append((time.perf_counter() - t0) * 1e6)
            out["host_one_thread_us_per_pair"] = round(float(np.median(t)), 1)
            out["host_equals_device_pair_0"] = bool(h["result"][:1].tobytes() == d["result"].cpu().numpy().view(SC.RESULT_DTYPE).reshape(-1)[:1].tobytes())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
