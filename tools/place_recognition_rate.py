#!/usr/bin/env python3
"""Times orbx_detect_candidates_device (KeyFrameDatabase::DetectNBestCandidates / DetectRelocalizationCandidates, reference
src/KeyFrameDatabase.cc:612-780, :783-895) at a loop closer's sizes: databases of 256, 2048 and 8192 keyframes (8192 is the largest the entry
takes) of about 300 words each, 1 and 64 queries per call, both modes, with events around back-to-back calls on the handle's stream.  The
scenes are tests/place_recognition_scenes.seeded's: rows drawn from places, so that several rows pass the word threshold.  A call rewrites
the scored entries of its score rows with the values they already hold, so every timed call does the same work.  Beside it the same header
compiled for the host on one thread (tests/cpp/place_recognition_host_check.cpp: pr_time).  THAT IS NOT the reference's inverted-file walk:
it is this library's pair form - every (query, row) pair is searched - compiled with g++ -O2.  The inverted file visits only the rows that
share a word and does less work per query, so the comparison says what the device costs, not what it saves.
A window of back-to-back calls is bounded by the device or by the host's enqueue rate, whichever is slower: the tool also times the enqueue
loop alone on the host clock (before the synchronise), and the kernels' own times come from a kernel trace of this tool, in a run of its own.
torch is asked for the GPU BEFORE the library is loaded.  Prints one JSON line; --out FILE also writes the table (profiles/
r31_place_recognition.md holds one such table and the reading of it: the tool never writes there by itself).
usage: place_recognition_rate.py [--rounds 7] [--calls 100] [--db 256,2048,8192] [--queries 1,64] [--modes N_BEST,RELOCALIZATION] [--out FILE] [--no-host]"""
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
    ap.add_argument("--db", default="256,2048,8192")
    ap.add_argument("--queries", default="1,64")
    ap.add_argument("--words", type=int, default=300)
    ap.add_argument("--modes", default="N_BEST,RELOCALIZATION")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    dbs, queries = [int(v) for v in a.db.split(",")], [int(v) for v in a.queries.split(",")]
    import torch
    assert torch.cuda.is_available(), "no GPU"
    torch.zeros(1, device="cuda")                       # torch's runtime first
    import extractorb_amd as X
    import place_recognition_scenes as SC
    import place_recognition_walk as PW
    from test_bow import make_vocab
    call, download, upload = SC.call, SC.download, SC.upload

    ex = X.ORBextractor(1000, 1.2, 8)
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    voc = X.Vocabulary(arrays=make_vocab(np.random.default_rng(3), k=3, L=2))
    host = None
    if not a.no_host:
        td = tempfile.mkdtemp()
        so = os.path.join(td, "libplace_recognition_host.so")
        inc = ["-I" + os.path.join(ROOT, *q) for q in (("tests", "cpp"), ("tests", "cpp", "host_shim"), ("extractorb_amd", "csrc"), ("include",))]
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", *inc,
                               os.path.join(ROOT, "tests", "cpp", "place_recognition_host_check.cpp"), "-o", so])
        host = C.CDLL(so)
        VP = C.c_void_p
        host.pr_time.argtypes = [C.c_int, C.c_int, C.c_int, VP, VP, VP, C.c_int, VP, VP, VP, C.c_int, VP, VP, VP, C.c_int, VP, C.c_int, VP, VP, VP, VP, VP,
                                 C.c_int]
        host.pr_time.restype = C.c_double
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    words = a.words
    cap = words + words // 15
    out = dict(words=words, capacity=cap, rounds=a.rounds, calls=a.calls, rows=[])
    for n_db in dbs:
        for mode, tag in [(m, t) for m, t in ((PW.N_BEST, "N_BEST"), (PW.RELOCALIZATION, "RELOCALIZATION")) if t in a.modes.split(",")]:
            base = SC.seeded(n_db, mode, n_db, [words, words - 40, words + words // 15], max(queries), cap, places=max(1, n_db // 16), query_words=words,
                             cand_capacity=n_db)
            base["connected"] = None                        # pr_time takes none; the connected test is one byte per pair
            for nq in queries:
                s = dict(base, n_queries=nq, q_map=base["q_map"][:nq].copy(), score_in=base["score_in"][:nq].copy())
                d, ins = upload(s)
                torch.cuda.synchronize()
                call(ex, voc, s, d, ins); torch.cuda.synchronize()
                t, enq = [], []
                for _ in range(a.rounds):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    h0 = time.perf_counter()
                    for _ in range(a.calls):
                        call(ex, voc, s, d, ins)
                    enq.append((time.perf_counter() - h0) * 1e6 / a.calls)      # the host's share: the calls return before the kernels end
                    e1.record(); torch.cuda.synchronize()
                    t.append(e0.elapsed_time(e1) * 1000.0 / a.calls)
                got = download(s, d)
                r = got["result"]
                row = dict(mode=tag, n_db=n_db, queries=nq, us_per_call=round(float(np.median(t)), 1), min_us=round(min(t), 1), max_us=round(max(t), 1), enqueue_us=round(float(np.median(enq)), 1),
                           median_sharing=float(np.median(r["n_sharing"])), median_scored=float(np.median(r["n_scored"])),
                           statuses=dict((PW.STATUS[v], int((r["status"] == v).sum())) for v in np.unique(r["status"])))
                if host is not None and (nq == 1 or n_db <= 2048):
                    h = SC.poisoned_outputs(s)
                    sec = host.pr_time(1 if nq > 1 else 3, s["mode"], n_db, ptr(s["db_ids"]), ptr(s["db_w"]), ptr(s["db_n"]), cap, ptr(s["db_map"]),
                                       ptr(s["db_flags"]), ptr(s["db_covis"]), nq, ptr(s["q_ids"]), ptr(s["q_w"]), ptr(s["q_n"]), s["q_capacity"],
                                       ptr(s["q_map"]), s["n_candidates"], ptr(h["score"]), ptr(h["result"]), ptr(h["loop"]), ptr(h["merge"]),
                                       ptr(h["cand"]), s["cand_capacity"])
                    row["host_one_thread_us_per_call"] = round(sec * 1e6, 1)
                    row["host_equals_device"] = all(h[k].tobytes() == got[k].tobytes() for k in ("result", "loop", "merge", "cand", "score"))
                out["rows"].append(row)
    print(json.dumps(out))
    lines = ["# orbx_detect_candidates_device: first timing (tools/place_recognition_rate.py)", "",
             "Databases of keyframes of about %d words (capacity %d), rows drawn from places of sixteen keyframes; HIP events around %d back-to-back"
             % (words, cap, a.calls),
             "calls, the median of %d rounds; `enqueue` is the host clock around the same calls before the synchronise.  The host column is the same" % a.rounds,
             "header (the pair form) on one host thread, g++ -O2.", "",
             "| mode | n_db | queries | call, us | per query, us | min .. max | enqueue, us | rows sharing / scored (median) | host, us | host per query, us | equal |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["rows"]:
        hu = r.get("host_one_thread_us_per_call")
        lines.append("| %s | %d | %d | %.1f | %.1f | %.1f .. %.1f | %.1f | %.0f / %.0f | %s | %s | %s |"
                     % (r["mode"], r["n_db"], r["queries"], r["us_per_call"], r["us_per_call"] / r["queries"], r["min_us"], r["max_us"], r["enqueue_us"], r["median_sharing"],
                        r["median_scored"], "-" if hu is None else "%.0f" % hu, "-" if hu is None else "%.0f" % (hu / r["queries"]),
                        r.get("host_equals_device", "-")))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
