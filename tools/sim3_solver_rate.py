#!/usr/bin/env python3
"""Times orbx_sim3_solve_device (Sim3Solver, reference src/Sim3Solver.cc as src/LoopClosing.cc:673-684 runs it) at the loop closer's size:
problems of about 60 correspondences among 1000 slots (the scene generator of tests/sim3_solver_scenes.py: half of them gross outliers),
0.99 / 15 / 300, for 1, 16 and 256 problems per call, with events around back-to-back calls on the handle's stream.  The three kernels are
timed by difference: orbx_debug_sim3_solve_steps launches prepare alone, prepare + hypotheses, or all three, and the rounds ALTERNATE between
the three forms so that a drift of the clocks falls on all of them alike; the medians over the rounds are reported.  Beside it the same
header compiled for the host on one thread (tests/cpp/sim3_solver_host_check.cpp): what a caller pays today, without the copies.
torch is asked for the GPU BEFORE the library is loaded.  Prints one JSON line and writes the report (--out).
usage: sim3_solver_rate.py [--rounds 9] [--calls 20] [--problems 1,16,256] [--out profiles/r24_sim3_solver.md] [--no-host]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_sim3_solver.md"))
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    shapes = [int(v) for v in a.problems.split(",")]
    import torch
    assert torch.cuda.is_available(), "no GPU"
    torch.zeros(1, device="cuda")                       # torch's runtime first
    import extractorb_amd as X
    import sim3_solver_scenes as SC
    import sim3_solver_walk as SW

    s = SC.make([60 + (i % 5) for i in range(max(shapes))], 99, cap=1000, n1=1000)
    ex = X.ORBextractor(1000, 1.2, SC.NLEVELS)
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8) if v.dtype.fields else np.ascontiguousarray(v)).cuda()
    o = SC.poisoned_outputs(s)
    d = dict((k, dev(v)) for k, v in o.items())
    ins = [dev(s[k]) for k in ("problems", "x1w", "x2w", "oct1", "oct2", "rand")]

    def call(P):
        ex.sim3_solve_device(P, ins[0], s["cap"], ins[1], ins[2], ins[3], ins[4], ins[5], d["result"], d["inliers"], 0.99, 15, 300)

    def span(P):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            call(P)
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / a.calls

    out = dict(slots=1000, correspondences="60 .. 64", iterations=300, rounds=a.rounds, calls=a.calls, us_per_call={}, steps_us={})
    try:
        for P in shapes:
            call(P); torch.cuda.synchronize()
            t = {1: [], 3: [], 7: []}
            for _ in range(a.rounds):
                for mask in (7, 1, 3):                          # alternating: every round times all three forms
                    ex.sim3_solve_steps(mask)
                    t[mask].append(span(P))
            m = dict((k, float(np.median(v))) for k, v in t.items())
            out["us_per_call"][str(P)] = round(m[7], 1)
            out["steps_us"][str(P)] = dict(prepare=round(m[1], 1), hypotheses=round(m[3] - m[1], 1), decide=round(m[7] - m[3], 1),
                                           spread_all_three=[round(min(t[7]), 1), round(max(t[7]), 1)])
    finally:
        ex.sim3_solve_steps(7)
    call(max(shapes)); torch.cuda.synchronize()
    res = d["result"].cpu().numpy().view(SC.RESULT_DTYPE).reshape(-1)
    out["statuses"] = dict((SW.STATUS[v], int((res["status"] == v).sum())) for v in np.unique(res["status"]))
    out["median_iterations_run"] = float(np.median(res["iterations"]))
    out["max_its"] = [int(res["max_its"].min()), int(res["max_its"].max())]
    if not a.no_host:
        with tempfile.TemporaryDirectory() as td:
            so = os.path.join(td, "libsim3_solver_host.so")
            inc = ["-I" + os.path.join(ROOT, *q) for q in (("tests", "cpp"), ("tests", "cpp", "host_shim"), ("extractorb_amd", "csrc"), ("include",))]
            subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", *inc,
                                   os.path.join(ROOT, "tests", "cpp", "sim3_solver_host_check.cpp"), "-o", so])
            L = C.CDLL(so)
            VP = C.c_void_p
            L.ss_host.argtypes = [C.c_int, VP, C.c_int, VP, VP, VP, VP, C.c_double, C.c_int, C.c_int, C.c_int, VP, VP, VP]
            L.ss_host.restype = None
            h = SC.poisoned_outputs(s)
            ptr = lambda v: v.ctypes.data_as(VP)
            t = []
            for _ in range(5):
                t0 = time.perf_counter()
                L.ss_host(1, ptr(s["problems"]), s["cap"], ptr(s["x1w"]), ptr(s["x2w"]), ptr(s["oct1"]), ptr(s["oct2"]), 0.99, 15, 300, SC.NLEVELS,
                          ptr(s["rand"]), ptr(h["result"]), ptr(h["inliers"]))
                t.append((time.perf_counter() - t0) * 1e6)
            out["host_one_thread_us_per_problem_all_iterations"] = round(float(np.median(t)), 1)
            out["host_equals_device_problem_0"] = bool(h["result"][:1].tobytes() == res[:1].tobytes())
    print(json.dumps(out))
    lines = ["# orbx_sim3_solve_device: first timing (tools/sim3_solver_rate.py)", "",
             "Problems of 60 .. 64 correspondences among 1000 slots, half of them gross outliers, 0.99 / 15 / 300 (mRansacMaxIts %d .. %d); HIP events"
             % tuple(out["max_its"]),
             "around %d back-to-back calls, the median of %d alternating rounds.  The steps are differences of calls that launch one, two or"
             % (a.calls, a.rounds),
             "all three kernels (orbx_debug_sim3_solve_steps).", "",
             "| problems | call, us | per problem, us | prepare | hypotheses | decide | all three, min .. max |", "|---|---|---|---|---|---|---|"]
    for P in shapes:
        st, tot = out["steps_us"][str(P)], out["us_per_call"][str(P)]
        share = lambda v: "%.1f us (%.0f %%)" % (v, 100.0 * v / tot)
        lines.append("| %d | %.1f | %.1f | %s | %s | %s | %.1f .. %.1f |" % (P, tot, tot / P, share(st["prepare"]), share(st["hypotheses"]), share(st["decide"]),
                                                                        st["spread_all_three"][0], st["spread_all_three"][1]))
    longest = lambda P: max(("prepare", "hypotheses", "decide"), key=lambda k: out["steps_us"][str(P)][k])
    lines += ["", "A call of %d problem(s) waits longest for `%s`, one of %d for `%s`: a small call is three launches of similar length (each mostly"
              % (shapes[0], longest(shapes[0]), shapes[-1], longest(shapes[-1])), "launch and one short wave), a large one is the hypotheses."]
    lines += ["", "Statuses of the largest call: %s; median mnIterations at the return %.0f." % (out["statuses"], out["median_iterations_run"])]
    if not a.no_host:
        lines += ["", "The same header on one host thread, one problem, every iteration evaluated as the kernels do: %.1f us (result row equal to the"
                  % out["host_one_thread_us_per_problem_all_iterations"], "device's: %s)." % out["host_equals_device_problem_0"]]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
