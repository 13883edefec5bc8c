#!/usr/bin/env python3
"""Times orbx_covisibility_device (KeyFrame::UpdateConnections and the vote of Tracking::UpdateLocalKeyFrames, reference src/KeyFrame.cc:388-511,
src/Tracking.cc:3030-3102) and orbx_keyframe_redundancy_device (the test of LocalMapping::KeyFrameCulling, src/LocalMapping.cc:977-1043) at a
tracker's and a mapper's sizes: 1 and 64 subjects of about 1000 slots, MapPoints with lists of about 8 observations, against 256 and 2048
keyframes (a map of n_frames * slots / 8 MapPoints, each seen from neighbouring keyframes), with events around back-to-back calls on the handle's stream.  The scenes are tests/covisibility_scenes.seeded_vote /
seeded_redundancy.  Every timed call does the same work: the entries read tables and overwrite their own outputs.  Beside them the same
header compiled for the host on one thread (tests/cpp/covisibility_host_check.cpp: cv_time, rd_time).  THAT IS NOT the reference's walk:
the reference counts into a std::map and sorts a vector of the counts that reach th; the header clears and scans a counter per keyframe
and, for the vote, ranks all keys of the call first (n_frames squared compares), compiled with g++ -O2.  The comparison says what the
device costs, not what it saves.
A window of back-to-back calls is bounded by the device or by the host's enqueue rate, whichever is slower: the tool also times the enqueue
loop alone on the host clock (before the synchronise); the kernels' own times come from a kernel trace of this tool, in a run of its own.
torch is asked for the GPU BEFORE the library is loaded.  Prints one JSON line; --out FILE also writes the table (profiles/
r34_covisibility.md holds one such table and the reading of it: the tool never writes there by itself).
usage: covisibility_rate.py [--rounds 7] [--calls 100] [--frames 256,2048] [--subjects 1,64] [--slots 1000] [--only all|vote|redundancy] [--out FILE] [--no-host]"""
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
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--frames", default="256,2048")
    ap.add_argument("--subjects", default="1,64")
    ap.add_argument("--slots", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--only", default="all", choices=["all", "vote", "redundancy"])
    a = ap.parse_args()
    frames, subjects = [int(v) for v in a.frames.split(",")], [int(v) for v in a.subjects.split(",")]
    import torch
    assert torch.cuda.is_available(), "no GPU"
    torch.zeros(1, device="cuda")                       # torch's runtime first
    import extractorb_amd as X
    import covisibility_scenes as SC
    import covisibility_walk as CW
    call, download, upload = SC.call, SC.download, SC.upload

    ex = X.ORBextractor(1000, 1.2, 8)
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    host = None
    if not a.no_host:
        td = tempfile.mkdtemp()
        so = os.path.join(td, "libcovisibility_host.so")
        inc = ["-I" + os.path.join(ROOT, *q) for q in (("tests", "cpp"), ("tests", "cpp", "host_shim"), ("extractorb_amd", "csrc"), ("include",))]
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", *inc,
                               os.path.join(ROOT, "tests", "cpp", "covisibility_host_check.cpp"), "-o", so])
        host = C.CDLL(so)
        VP = C.c_void_p
        host.cv_time.argtypes = [C.c_int, C.c_int, C.c_int, VP, VP, VP, C.c_int, VP, VP, VP, C.c_int, VP, VP, C.c_int, VP, VP, C.c_int, C.c_int, VP, VP, VP, VP, VP]
        host.rd_time.argtypes = [C.c_int, C.c_int, VP, VP, VP, VP, C.c_int, VP, VP, VP, C.c_int, VP, VP, C.c_int, VP, VP]
        host.cv_time.restype = host.rd_time.restype = C.c_double
    ptr = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    lens = (8, 9, 7, 8, 6, 10, 8, 8)
    out = dict(slots=a.slots, list_lengths=lens, rounds=a.rounds, calls=a.calls, rows=[])

    def timed(s):
        d, ins = upload(s)
        torch.cuda.synchronize()
        call(ex, s, d, ins); torch.cuda.synchronize()
        t, enq = [], []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            h0 = time.perf_counter()
            for _ in range(a.calls):
                call(ex, s, d, ins)
            enq.append((time.perf_counter() - h0) * 1e6 / a.calls)      # the host's share: the calls return before the kernels end
            e1.record(); torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 1000.0 / a.calls)
        return download(s, d), dict(us_per_call=round(float(np.median(t)), 1), min_us=round(min(t), 1), max_us=round(max(t), 1),
                                    enqueue_us=round(float(np.median(enq)), 1))

    for nf in frames:
        n_points = max(2 * a.slots, nf * a.slots // 8)      # a keyframe sees about `slots` MapPoints, a MapPoint is seen from about 8
        for ns in subjects:
            for tag, mode in ((("UPDATE_CONNECTIONS", CW.UPDATE_CONNECTIONS), ("LOCAL_KEYFRAMES", CW.LOCAL_KEYFRAMES)) if a.only != "redundancy" else ()):
                s = SC.seeded_vote(nf + ns, mode, nf, a.slots, ns, lens=lens, th=15, conn_capacity=nf, n_points=n_points)
                got, row = timed(s)
                r = got["result"]
                row.update(entry=tag, n_frames=nf, subjects=ns, median_counter=float(np.median(r["n_counter"])), median_ordered=float(np.median(r["n_ordered"])),
                           statuses=dict((CW.STATUS[v], int((r["status"] == v).sum())) for v in np.unique(r["status"])))
                if host is not None:
                    h = SC.poisoned_outputs(s)
                    sec = host.cv_time(3, s["mode"], s["n_points"], ptr(s["obs_off"]), ptr(s["obs"]), ptr(s["mp_flags"]), nf, ptr(s["kf_flags"]), ptr(s["kf_map"]),
                                       ptr(s["kf_key"]), ns, ptr(s["subject_mp"]), ptr(s["subject_n"]), s["capacity"], ptr(s["subject_kf"]), ptr(s["subject_map"]),
                                       s["th"], s["conn_capacity"], ptr(h["counter_kf"]), ptr(h["counter_w"]), ptr(h["ordered_kf"]), ptr(h["ordered_w"]), ptr(h["result"]))
                    row["host_one_thread_us_per_call"] = round(sec * 1e6, 1)
                    row["host_equals_device"] = SC.differences(got, h) == []
                out["rows"].append(row)
            if a.only == "vote":
                continue
            s = SC.seeded_redundancy(nf + ns, nf, a.slots, ns, lens=lens, monocular=True, n_points=n_points)
            got, row = timed(s)
            r = got["result"]
            row.update(entry="REDUNDANCY", n_frames=nf, subjects=ns, median_counter=float(np.median(r["n_mps"])), median_ordered=float(np.median(r["n_redundant"])),
                       statuses=dict((CW.REDUNDANCY_STATUS[v], int((r["status"] == v).sum())) for v in np.unique(r["status"])))
            if host is not None:
                h = SC.poisoned_outputs(s)
                sec = host.rd_time(3, s["n_points"], ptr(s["obs_off"]), ptr(s["obs"]), ptr(s["mp_flags"]), ptr(s["mp_nobs"]), nf, ptr(s["kf_flags"]), ptr(s["kps_un"]),
                                   ptr(s["n_out"]), ns, ptr(s["subject_mp"]), ptr(s["subject_n"]), s["capacity"], ptr(s["subject_kf"]), ptr(h["result"]))
                row["host_one_thread_us_per_call"] = round(sec * 1e6, 1)
                row["host_equals_device"] = h["result"].tobytes() == got["result"].tobytes()
            out["rows"].append(row)
    print(json.dumps(out))
    lines = ["# orbx_covisibility_device and orbx_keyframe_redundancy_device: first timing (tools/covisibility_rate.py)", "",
             "Subjects of %d slots, MapPoints with lists of %d .. %d observations; HIP events around %d back-to-back calls, the median of %d rounds;"
             % (a.slots, min(lens), max(lens), a.calls, a.rounds),
             "`enqueue` is the host clock around the same calls before the synchronise.  The host column is the same header on one host thread, g++ -O2.", "",
             "| entry | n_frames | subjects | call, us | per subject, us | min .. max | enqueue, us | counter / ordered, or nMPs / redundant (median) | host, us | host per subject, us | equal |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["rows"]:
        hu = r.get("host_one_thread_us_per_call")
        lines.append("| %s | %d | %d | %.1f | %.1f | %.1f .. %.1f | %.1f | %.0f / %.0f | %s | %s | %s |"
                     % (r["entry"], r["n_frames"], r["subjects"], r["us_per_call"], r["us_per_call"] / r["subjects"], r["min_us"], r["max_us"], r["enqueue_us"],
                        r["median_counter"], r["median_ordered"], "-" if hu is None else "%.0f" % hu, "-" if hu is None else "%.0f" % (hu / r["subjects"]),
                        r.get("host_equals_device", "-")))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
