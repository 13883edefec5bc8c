#!/usr/bin/env python3
"""Seeded soak of the matcher rows on the GPU box: the parity tests of tests/test_search_projection.py, tests/test_search_bow.py,
tests/test_search_init.py, tests/test_search_init_edges.py, tests/test_stereo_edges.py, tests/test_search_triangulation.py, tests/test_fuse_gpu.py, tests/test_fuse_two_eyes_gpu.py and tests/test_search_triangulation_two_eyes_gpu.py bodies re-run with seeds outside the committed parametrisation.
usage: fuzz_matchers.py [n_seeds] [first_seed]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

n, s0 = (int(sys.argv[1]) if len(sys.argv) > 1 else 20), (int(sys.argv[2]) if len(sys.argv) > 2 else 1000)
import test_search_projection as P
import test_search_bow as W
import test_search_init as I
import test_search_triangulation as T
import test_stereo_edges as E
import test_search_init_edges as IE
import test_fuse_gpu as FU
import test_fuse_two_eyes_gpu as FU2
import test_search_triangulation_two_eyes_gpu as T2
from extractorb_amd import synth
t0 = time.time()
done = 0
for k in range(n):
    seed = s0 + k
    rng = np.random.default_rng(seed)
    ratio, stereo, check = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    P.test_gpu_search_equals_oracle_on_random_scenes(seed, ratio, stereo, check and not ratio, int(rng.choice([100, 64, 100])))
    big = rng.random() < 0.3          # the list-less kernel variant
    P.test_gpu_search_settles_crowded_requests_like_the_walk(seed, ratio, 2200 if big else 1024, 1500 if big else 768)
    case = dict(seed=seed, nnratio=float(rng.choice([0.6, 0.7, 0.9])), th_low=int(rng.choice([50, 100])), check=bool(rng.integers(0, 2)),
                n_nodes=int(rng.choice([3, 60, 400, 2000])), tie_heavy=bool(rng.random() < 0.3))
    W.test_gpu_search_by_bow_equals_oracle(case)
    W.test_gpu_keyframe_search_by_bow_equals_oracle(case)
    if k % 5 == 0:      # SearchForInitialization on a freshly extracted stream (heavier: six frames through the HIP path and the oracle)
        frames = synth.frames(["textured", "noise", "sparse", "natural"][int(rng.integers(0, 4))], seed, 6, 480, 640)
        I.run_gpu_pairs(frames, ((0, 1), (1, 1), 5), I.PINHOLE, int(rng.choice([300, 1000, 2000, 5000])), int(rng.choice([30, 100, 300])),
                        float(rng.choice([0.6, 0.9, 1.3])), bool(rng.integers(0, 2)), rounds=int(rng.integers(1, 3)))
    trng = np.random.default_rng(seed + 77)      # (a generator of its own: the draws of the cases above stay what they were)
    T.check_gpu_on_seed(seed, only_stereo=bool(trng.random() < 0.2), coarse=bool(trng.integers(0, 2)), th_low=int(trng.choice([50, 100])),
                        check_orientation=bool(trng.integers(0, 2)))
    E.check_gpu_on_seed(seed)      # ComputeStereoMatches on the crafted scenes of this seed (ties, gates, borders, empty stripe, zero disparity)
    IE.check_gpu_on_seed(seed)     # SearchForInitialization on the crafted scenes of this seed (ladders, cascades, crowds, histogram ties, cell edges)
    FU.check_gpu_on_seed(seed, reproj_check=bool(trng.integers(0, 2)), th=float(trng.choice([3.0, 3.0, 5.0])))      # the search half of Fuse, one list into three keyframes
    frng = np.random.default_rng(seed + 177)     # (again a generator of its own)
    FU2.check_gpu_on_seed(seed, th=float(frng.choice([3.0, 3.0, 4.0])))      # Fuse on two-camera keyframes: one list into both eyes of three rigs
    T2.check_gpu_on_seed(seed, coarse=bool(frng.random() < 0.2), th_low=int(frng.choice([50, 50, 30])),
                         check_orientation=bool(frng.integers(0, 2)))      # SearchForTriangulation on two-camera keyframes: one rig against three
    done += 1
print("matcher soak: %d seeds x 10 matcher parity bodies (+ SearchForInitialization every fifth seed) bit-exact, %.0f s" % (done, time.time() - t0))
