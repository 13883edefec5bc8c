#!/usr/bin/env python3
"""Times orbx_update_map_points_device and orbx_update_map_points_two_eyes_device (MapPoint::ComputeDistinctiveDescriptors and
MapPoint::UpdateNormalAndDepth, reference src/MapPoint.cc:330-403, :427-494) with what = 3 on the working-size scene of
tests/map_point_update_scenes.py - a batch of 32 frames at capacity 2024, lists with a mean of about 6 entries and a tail into the hundreds -
for 256, 2048 and 16384 points per call, with events around back-to-back calls; the medians over the rounds are reported.  Beside it:
  * the kernel's statement compiled for the host, one thread (tests/cpp/map_point_update_host_check.cpp), on host arrays;
  * the D2H copy of the batch's descriptor rows (d_desc of all frames, into pinned memory) that this host path needs first, since
    mDescriptors live in HBM here: host thread + copy is the path the entry replaces.
One (form, size) per process, so that a caller can put every GPU step under a time limit of its own:
  for f in one_camera two_eyes; do for n in 256 2048 16384; do timeout -k 10 300 python tools/map_point_update_rate.py --form $f --points $n || break 2; done; done
torch is asked for the GPU BEFORE the library is loaded: a process whose first HIP call is the library's leaves torch without a device.
Prints one JSON line.  usage: map_point_update_rate.py --form one_camera|two_eyes --points N [--tail 24] [--rounds 7] [--calls 2000]"""
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
    ap.add_argument("--form", choices=("one_camera", "two_eyes"), default="one_camera")
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--tail", type=int, default=24, help="lists of 65 .. 400 entries in the call (0: no list above 40 entries)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2000, help="calls per timed window at 2048 points and below (fewer above, never under 50)")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "no GPU"
    torch.zeros(1, device="cuda")                       # torch's runtime first
    import map_point_update_scenes as SC
    import test_map_point_update as T
    import test_map_point_update_gpu as G

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
        return float(np.median(t)), float(min(t)), float(max(t))

    s = SC.working(a.form == "two_eyes", points=a.points, tail=a.tail)
    n = np.diff(s["obs_off"])
    ex = G.extractor()
    dv, out = G.upload(s), G.poisoned(s)
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    calls = max(50, a.calls // max(1, a.points // 2048))
    call_us, call_min, call_max = span(lambda: G.call(ex, s, dv, 3, out), calls)
    status = out["status"].cpu().numpy()
    # the D2H copy of the descriptor rows the host path needs: the batch's d_desc into pinned memory
    pinned = torch.empty(dv["desc"].shape, dtype=torch.uint8).pin_memory()
    copy_us = span(lambda: pinned.copy_(dv["desc"], non_blocking=True), 200)[0]
    host = T.build_host(tempfile.mkdtemp())
    T.host_update(host, s)
    reps = 3 if a.points <= 2048 else 1
    t0 = time.perf_counter()
    for _ in range(reps):
        T.host_update(host, s)
    host_us = (time.perf_counter() - t0) / reps * 1e6
    print(json.dumps(dict(form=a.form, points=a.points, tail=a.tail, entries=int(n.sum()), mean_entries=float(n.mean()), longest=int(n.max()),
                          lists_above_64=int((n > 64).sum()), rounds=a.rounds, calls=calls, call_us=call_us, call_us_min=call_min, call_us_max=call_max, per_point_us=call_us / a.points,
                          host_one_thread_us=host_us, desc_d2h_us=copy_us, desc_d2h_bytes=int(pinned.numel()), host_plus_copy_us=host_us + copy_us,
                          status_counts=np.bincount(status, minlength=5).tolist())))


if __name__ == "__main__":
    main()
