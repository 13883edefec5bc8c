#!/usr/bin/env python3
"""Times orbx_optimize_pose_device (Optimizer::PoseOptimization, reference src/Optimizer.cc:854-1168) at the tracker's size: problems of 300
correspondences (the scene generator of tests/pose_optimization_scenes.py: Pinhole, half of the keypoints with a right-eye column, 30 %
gross outliers), for 1, 16 and 256 problems per call, with events around back-to-back calls on the handle's stream.  A call optimises IN
PLACE, so every timed call starts from the poses and flags of the call before it - from an optimised pose the LM stops earlier.  The tool
therefore copies the initial poses back (device to device, on the same stream) in front of every call and reports that copy's time, timed
alone in alternating rounds, beside the call's.  Beside it the same header compiled for the host on one thread
(tests/cpp/pose_optimization_host_check.cpp).  THAT IS NOT g2o: it is this library's own statement with its own summation order and 6x6
solve, compiled with g++ -O2, and the only CPU form of it that exists; no number here says how long the reference takes.
torch is asked for the GPU BEFORE the library is loaded.  Prints one JSON line and writes the report (--out).
usage: pose_optimization_rate.py [--rounds 9] [--calls 20] [--problems 1,16,256] [--out profiles/r26_pose_optimization.md] [--no-host]"""
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
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--problems", default="1,16,256")
    ap.add_argument("--correspondences", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_pose_optimization.md"))
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    shapes = [int(v) for v in a.problems.split(",")]
    import torch
    assert torch.cuda.is_available(), "no GPU"
    torch.zeros(1, device="cuda")                       # torch's runtime first
    import extractorb_amd as X
    import pose_optimization_scenes as SC
    import pose_optimization_walk as PW

    s = SC.make([a.correspondences] * max(shapes), stereo=True, seed=99)
    ex = X.ORBextractor(1000, 1.2, SC.NLEVELS)
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8) if v.dtype.fields else np.ascontiguousarray(v)).cuda()
    o = SC.poisoned_outputs(s)
    d = dict((k, dev(v)) for k, v in o.items())
    ins = dict((k, dev(s[k])) for k in ("problems", "kps", "n_out", "u_right", "matches", "world"))
    initial = dev(s["poses"])

    def call(P, solve=True):
        d["poses"][:P * 12].copy_(initial[:P * 12])
        if solve:
            ex.optimize_pose_device(P, (0, 1), ins["problems"], ins["kps"], ins["n_out"], ins["u_right"], s["cap"], ins["matches"], ins["world"],
                                    len(s["world"]), d["poses"], d["outlier"], d["result"])

    def span(P, solve):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            call(P, solve)
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / a.calls

    out = dict(correspondences=a.correspondences, rounds=a.rounds, calls=a.calls, us_per_call={}, copy_us={}, spread={})
    for P in shapes:
        call(P); torch.cuda.synchronize()
        t = {True: [], False: []}
        for _ in range(a.rounds):
            for solve in (True, False):                         # alternating: a drift of the clocks falls on both alike
                t[solve].append(span(P, solve))
        both, copy = float(np.median(t[True])), float(np.median(t[False]))
        out["us_per_call"][str(P)] = round(both - copy, 1)
        out["copy_us"][str(P)] = round(copy, 1)
        out["spread"][str(P)] = [round(min(t[True]) - copy, 1), round(max(t[True]) - copy, 1)]
    call(max(shapes)); torch.cuda.synchronize()
    res = d["result"].cpu().numpy().view(SC.RESULT_DTYPE).reshape(-1)
    out["statuses"] = dict((PW.STATUS[v], int((res["status"] == v).sum())) for v in np.unique(res["status"]))
    out["median_lm_iterations"] = float(np.median(res["its"].sum(axis=1)))
    out["median_trials"] = float(np.median(res["trials"].sum(axis=1)))
    out["median_outliers"] = float(np.median(res["n_bad"]))
    if not a.no_host:
        with tempfile.TemporaryDirectory() as td:
            so = os.path.join(td, "libpose_optimization_host.so")
            inc = ["-I" + os.path.join(ROOT, *q) for q in (("tests", "cpp"), ("tests", "cpp", "host_shim"), ("extractorb_amd", "csrc"), ("include",))]
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", *inc,
                                   os.path.join(ROOT, "tests", "cpp", "pose_optimization_host_check.cpp"), "-o", so])
            L = C.CDLL(so)
            VP = C.c_void_p
            L.po_host.argtypes = [C.c_int] * 4 + [VP] * 4 + [C.c_int, VP, VP, C.c_int, C.c_int, VP, VP, VP]
            L.po_host.restype = None
            ptr = lambda v: v.ctypes.data_as(VP)
            t = []
            for _ in range(5):
                h = SC.poisoned_outputs(s)
                t0 = time.perf_counter()
                L.po_host(1, 0, 1, 1, ptr(s["problems"]), ptr(s["kps"]), ptr(s["n_out"]), ptr(s["u_right"]), s["cap"], ptr(s["matches"]), ptr(s["world"]),
                          len(s["world"]), SC.NLEVELS, ptr(h["poses"]), ptr(h["outlier"]), ptr(h["result"]))
                t.append((time.perf_counter() - t0) * 1e6)
            out["host_one_thread_us_per_problem"] = round(float(np.median(t)), 1)
            out["host_equals_device_problem_0"] = bool(h["result"][:1].tobytes() == res[:1].tobytes())
    print(json.dumps(out))
    lines = ["# orbx_optimize_pose_device: first timing (tools/pose_optimization_rate.py)", "",
             "Problems of %d correspondences (Pinhole, about half of them stereo edges, 30 %% gross outliers); HIP events around %d back-to-back calls,"
             % (a.correspondences, a.calls),
             "the median of %d alternating rounds.  Every call starts from the initial poses: a device-to-device copy in front of it, timed alone" % a.rounds,
             "in the alternate rounds and subtracted.", "",
             "| problems | call, us | per problem, us | min .. max | the copy, us |", "|---|---|---|---|---|"]
    for P in shapes:
        tot = out["us_per_call"][str(P)]
        lines.append("| %d | %.1f | %.1f | %.1f .. %.1f | %.1f |" % (P, tot, tot / P, out["spread"][str(P)][0], out["spread"][str(P)][1], out["copy_us"][str(P)]))
    lines += ["", "The largest call: statuses %s; medians per problem: %.0f LM iterations and %.0f trials over the four rounds, %.0f outliers."
              % (out["statuses"], out["median_lm_iterations"], out["median_trials"], out["median_outliers"]),
              "One workgroup of 256 lanes per problem, one launch per call (k_pose_optimization.hip)."]
    if not a.no_host:
        lines += ["", "The same header on one host thread, one problem: %.1f us (result row equal to the device's: %s).  That is this library's own"
                  % (out["host_one_thread_us_per_problem"], out["host_equals_device_problem_0"]),
                  "statement compiled with g++ -O2 - its summation order, its Cholesky - and NOT g2o: no number here is the reference's time."]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
