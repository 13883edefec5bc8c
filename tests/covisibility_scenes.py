"""Scenes for orbx_covisibility_device and orbx_keyframe_redundancy_device: plain arrays in the entries' layout, crafted ones - one per rule
of the reference the entries have to keep (docs/history/r34_covisibility.md lists them) - and seeded ones at the sizes where the kernels can
go wrong.  A scene is a dict (kind "vote" or "redundancy"); case(name) builds it, case_expected(name) walks it ONCE with
tests/covisibility_walk.py; both are cached and nothing changes them afterwards."""
import functools

import numpy as np

import covisibility_walk as CW

f32 = np.float32
UPDATE, LOCAL = CW.UPDATE_CONNECTIONS, CW.LOCAL_KEYFRAMES
POISON = CW.POISON
MAX_FRAMES, MAX_CAPACITY = 8192, 163280                  # the entries' launch-time bounds (include/orbx.h)
VOTE_OUTPUTS = ("result", "counter_kf", "counter_w", "ordered_kf", "ordered_w")
REDUNDANCY_OUTPUTS = ("result", "slot_state")


def poisoned_outputs(s):
    return CW.poisoned_vote_outputs(s) if s["kind"] == "vote" else CW.poisoned_redundancy_outputs(s)


def differences(got, want):
    """the outputs that are not equal byte for byte"""
    return [k for k in want if got[k].tobytes() != want[k].tobytes()]


def reversed_keys(n):
    """addresses in the order opposite to the frames'"""
    return (np.uint64(0x7f0000001000) + np.uint64(0x1e0) * np.arange(n, dtype=np.uint64))[::-1].copy()


def permuted_keys(n, seed):
    """addresses in a random order, the top bit set in some: the order is unsigned"""
    rng = np.random.default_rng(seed)
    keys = np.uint64(0x560000000000) + np.uint64(0x90) * rng.permutation(n).astype(np.uint64)
    keys[::5] |= np.uint64(1 << 63)
    return keys


def csr(points, rng, rows=None):
    off = np.zeros(len(points) + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in points])
    obs = np.zeros((int(off[-1]), 2), np.int32)
    o = 0
    for m, p in enumerate(points):
        for e in p:
            f, row = e if isinstance(e, tuple) else (e, int(rng.integers(0, 1 << 20)) if rows is None else int(rng.integers(0, rows)))
            obs[o] = (f, row)
            o += 1
    return off, obs


def subject_rows(subjects, capacity, rng, n_points):
    mp = rng.integers(-1, max(n_points, 1), (len(subjects), capacity)).astype(np.int32)       # the slots past N hold junk
    n = np.zeros(len(subjects), np.int32)
    for j, sub in enumerate(subjects):
        n[j] = sub.get("n", len(sub["mp"]))
        mp[j, :len(sub["mp"])] = sub["mp"]
    return mp, n


def votes(counts, first=0):
    """MapPoints (lists of observing frames) in which frame f stands counts[f] times, and their indices from `first` on"""
    pts = [[f for f, c in counts.items() if c > k] for k in range(max(counts.values()))]
    return pts, list(range(first, first + len(pts)))


def craft_vote(mode, n_frames, points, subjects, keys=None, kf_flags=None, kf_map=None, mp_bad=(), th=15, conn_capacity=None, capacity=None, seed=0):
    """points: lists of observing frames; subjects: dict(mp=[MapPoint indices or -1], kf=-1, map=0, n=len(mp))"""
    rng = np.random.default_rng(seed)
    capacity = capacity or max([len(sub["mp"]) for sub in subjects] + [1])
    off, obs = csr(points, rng)
    mp, n = subject_rows(subjects, capacity, rng, len(points))
    flags = np.zeros(len(points), np.uint8)
    flags[list(mp_bad)] = 1
    flags |= (rng.integers(0, 128, len(points)) << 1).astype(np.uint8)                       # only bit 0 is read
    kff = np.zeros(n_frames, np.uint8) if kf_flags is None else np.asarray(kf_flags, np.uint8)
    return dict(kind="vote", mode=mode, n_points=len(points), obs_off=off, obs=obs, mp_flags=flags, n_frames=n_frames, kf_flags=kff,
                kf_map=np.zeros(n_frames, np.int32) if kf_map is None else np.asarray(kf_map, np.int32),
                kf_key=reversed_keys(n_frames) if keys is None else np.asarray(keys, np.uint64), n_subjects=len(subjects), subject_mp=mp, subject_n=n,
                capacity=capacity, subject_kf=np.array([sub.get("kf", -1) for sub in subjects], np.int32),
                subject_map=np.array([sub.get("map", 0) for sub in subjects], np.int32), th=th,
                conn_capacity=n_frames if conn_capacity is None else conn_capacity)


def neighbourhood_points(rng, n_points, n_frames, lens, width=6):
    """MapPoint m is seen from frames around a centre that moves with m: subjects that take a band of MapPoints share many observers"""
    pts = []
    for m in range(n_points):
        L = min(int(lens[m % len(lens)]), n_frames)
        c = (m * n_frames) // max(n_points, 1)
        pool = np.arange(max(0, c - width), min(n_frames, c + width + 1))
        if L > len(pool):
            pool = np.arange(n_frames)
        pts.append([int(f) for f in rng.permutation(pool)[:L]])
    return pts


def seeded_vote(seed, mode, n_frames, N, n_subjects, lens=(8, 5, 4, 1, 0, 7, 9, 6), keys="permuted", n_points=None, conn_capacity=None, th=6,
                long_list=0, capacity=None):
    rng = np.random.default_rng(seed)
    n_points = n_points or max(4, 2 * N)
    pts = neighbourhood_points(rng, n_points, n_frames, lens)
    if long_list:
        pts[n_points // 2] = [int(f) for f in rng.permutation(n_frames)[:long_list]]
    subjects = []
    for j in range(n_subjects):
        kf = int(rng.integers(0, n_frames))
        first = min(max(0, (kf * n_points) // n_frames - N // 2), max(0, n_points - N))
        band = [first + (i % max(1, min(N, n_points))) for i in range(N)]
        mp = [(-1 if rng.random() < 0.15 else int(rng.integers(0, n_points)) if rng.random() < 0.1 else band[i]) for i in range(N)]
        if long_list and N:
            mp[0] = n_points // 2
        subjects.append(dict(mp=mp, kf=kf, map=int(j % 5 == 4)))
    kf_flags = (rng.random(n_frames) < 0.05).astype(np.uint8) | (rng.integers(0, 64, n_frames) << 2).astype(np.uint8)
    kf_map = (np.arange(n_frames) % 11 == 5).astype(np.int32)
    key = reversed_keys(n_frames) if keys == "reversed" else permuted_keys(n_frames, seed)
    s = craft_vote(mode, n_frames, pts, subjects, key, kf_flags, kf_map, mp_bad=[m for m in range(n_points) if rng.random() < 0.05], th=th,
                   conn_capacity=conn_capacity, capacity=capacity or max(N, 1) + 3, seed=seed)
    return s


def craft_redundancy(n_frames, capacity, points, subjects, octaves=None, depth=None, th_depth=4.0, kf_flags=None, mp_bad=(), nobs=None,
                     n_out=None, monocular=True, th_obs=3, redundant_th=0.9, seed=0, default_octave=0):
    """points: lists of (frame, row); subjects: dict(kf, mp=[...]); octaves {(frame, row): octave}; depth {(frame, slot): depth}; nobs {m: n}"""
    rng = np.random.default_rng(seed)
    off, obs = csr(points, rng, rows=capacity)
    mp, n = subject_rows(subjects, capacity, rng, len(points))
    kps = np.zeros((n_frames, capacity), CW.KEYPOINT_DTYPE)
    kps["x"] = rng.random((n_frames, capacity)) * 600
    kps["octave"], kps["class_id"] = default_octave, -1
    for (f, row), o in (octaves or {}).items():
        kps["octave"][f, row] = o
    d = np.ones((n_frames, capacity), f32)
    for (f, i), v in (depth or {}).items():
        d[f, i] = v
    flags = np.zeros(len(points), np.uint8)
    flags[list(mp_bad)] = 1
    mp_nobs = None
    if nobs is not None:
        mp_nobs = np.diff(off).astype(np.int32)
        for m, v in nobs.items():
            mp_nobs[m] = v
    return dict(kind="redundancy", n_points=len(points), obs_off=off, obs=obs, mp_flags=flags, mp_nobs=mp_nobs, n_frames=n_frames,
                kf_flags=np.zeros(n_frames, np.uint8) if kf_flags is None else np.asarray(kf_flags, np.uint8), kps_un=kps,
                n_out=np.full(n_frames, capacity, np.int32) if n_out is None else np.asarray(n_out, np.int32), depth=d,
                th_depth=np.full(n_frames, th_depth, f32), n_subjects=len(subjects), subject_mp=mp, subject_n=n, capacity=capacity,
                subject_kf=np.array([sub["kf"] for sub in subjects], np.int32), monocular=monocular, th_obs=th_obs, redundant_th=f32(redundant_th))


def seeded_redundancy(seed, n_frames, N, n_subjects, lens=(8, 5, 4, 1, 0, 7, 9, 6), monocular=True, redundant_th=0.9, with_nobs=True, long_list=0,
                      n_points=None):
    rng = np.random.default_rng(seed)
    capacity = max(N, 1) + 2
    n_points = n_points or max(4, 2 * N)
    n_out = rng.integers(max(1, capacity - 3), capacity + 1, n_frames).astype(np.int32)
    frames = neighbourhood_points(rng, n_points, n_frames, lens)
    if long_list:
        frames[1] = [int(f) for f in rng.permutation(n_frames)[:long_list]]
    pts = [[(f, int(rng.integers(0, n_out[f]))) for f in p] for p in frames]
    subjects = []
    for j in range(n_subjects):
        kf = int(rng.integers(0, n_frames))
        first = min(max(0, (kf * n_points) // n_frames - N // 2), max(0, n_points - N))
        mp = [(-1 if rng.random() < 0.15 else first + (i % max(1, min(N, n_points)))) for i in range(N)]
        if long_list and N:
            mp[0] = 1
        subjects.append(dict(kf=kf, mp=mp))
    s = craft_redundancy(n_frames, capacity, pts, subjects, kf_flags=((rng.random(n_frames) < 0.08).astype(np.uint8) | (np.arange(n_frames) == 0) * 2),
                         mp_bad=[m for m in range(n_points) if rng.random() < 0.05], n_out=n_out, monocular=monocular, redundant_th=redundant_th, seed=seed)
    s["kps_un"]["octave"] = rng.integers(0, 8, (n_frames, capacity))
    s["depth"] = (rng.random((n_frames, capacity)) * 7 - 1).astype(f32)
    if with_nobs:
        s["mp_nobs"] = (np.diff(s["obs_off"]) + rng.integers(0, 4, n_points)).astype(np.int32)
    return s


# ---- crafted: the vote --------------------------------------------------------------------------------------------------------------------------
def th_14_15_16():
    pts, idx = votes({1: 14, 2: 15, 3: 16})
    return craft_vote(UPDATE, 5, pts, [dict(mp=idx, kf=0)])


def none_reach_th_tie():
    """counts 5, 5, 3: no count >= 15, the single pair is the first of the two fives in KEY order - frame 2, whose key is smaller"""
    pts, idx = votes({1: 5, 2: 5, 3: 3})
    return craft_vote(UPDATE, 4, pts, [dict(mp=idx, kf=0)])


def three_equal_weights():
    pts, idx = votes({1: 20, 2: 25, 3: 20, 4: 16, 5: 20, 6: 3})
    return craft_vote(UPDATE, 7, pts, [dict(mp=idx, kf=0)], keys=[50, 30, 90, 10, 70, 20, 60])


def empty_counter():
    """the first subject's MapPoints are seen by nobody else; the second subject is answered"""
    pts, idx = votes({1: 3})
    return craft_vote(UPDATE, 3, [[0], [0], []] + pts, [dict(mp=[0, 1, -1, 2], kf=0), dict(mp=[3, 4, 5], kf=0)])


def point_in_two_slots():
    return craft_vote(UPDATE, 3, [[1, 2], [2]], [dict(mp=[0, 1, 0, -1, 0], kf=0)])


def bad_map_point():
    return craft_vote(UPDATE, 3, [[1, 2], [2], [1]], [dict(mp=[0, 1, 2], kf=0)], mp_bad=[0])


def bad_observer(mode):
    """frame 2 is bad and holds the largest count"""
    pts, idx = votes({1: 16, 2: 18, 3: 4})
    return craft_vote(mode, 4, pts, [dict(mp=idx, kf=0)], kf_flags=[0, 0, 1, 0])


def other_map_and_self(mode):
    """frame 3 lives in another map; frame 0 is the subject and observes every MapPoint"""
    pts, idx = votes({0: 17, 1: 16, 3: 17, 2: 2})
    return craft_vote(mode, 4, pts, [dict(mp=idx, kf=0, map=0)], kf_map=[0, 0, 0, 1])


def conn_capacity(cc):
    pts, idx = votes({1: 20, 2: 18, 3: 17, 4: 16, 5: 2})
    return craft_vote(UPDATE, 6, pts, [dict(mp=idx, kf=0)], conn_capacity=cc)


def counter_longer_than_ordered(cc):
    """five keyframes in the counter, two in the ordered list: a capacity of 3 truncates the one and not the other"""
    pts, idx = votes({1: 20, 2: 18, 3: 1, 4: 1, 5: 2})
    return craft_vote(UPDATE, 6, pts, [dict(mp=idx, kf=0)], conn_capacity=cc)


def duplicate_keys():
    pts, idx = votes({1: 20, 2: 18})
    return craft_vote(UPDATE, 300, pts, [dict(mp=idx, kf=0), dict(mp=idx[:3], kf=4)], keys=[7 + 3 * (f if f != 299 else 2) for f in range(300)])


def bad_index(kind, mode=UPDATE):
    """two subjects: the first reads one index outside its table, the second is answered"""
    pts, idx = votes({1: 16, 2: 3})
    s = craft_vote(mode, 3, pts + [[1, 2], [1]], [dict(mp=idx + [16], kf=0), dict(mp=idx[1:15], kf=0)])      # MapPoints 0, 15, 16: the first subject's alone
    if kind == "mp_high":
        s["subject_mp"][0, 5] = s["n_points"]
    elif kind == "mp_negative":
        s["subject_mp"][0, 5] = -2
    elif kind == "offset_negative":
        s["obs_off"][0] = -1
    elif kind == "offset_decreasing":                        # MapPoint 16's list ends in front of its start
        s["obs_off"][17] = s["obs_off"][16] - 1
    elif kind == "offset_past_total":
        s["obs_off"][16] = s["obs_off"][18] + 5               # MapPoint 15's
    elif kind == "frame_high":
        s["obs"][int(s["obs_off"][16]), 0] = 3
    elif kind == "frame_negative":
        s["obs"][int(s["obs_off"][16]), 0] = -1
    elif kind == "subject_kf":
        s["subject_kf"][0] = 3
    elif kind == "bad_map_point_unchecked":                  # a bad MapPoint's list is not read: junk in it is no bad index
        s["mp_flags"][16] |= 1
        s["obs"][int(s["obs_off"][16]), 0] = 77
    return s


# ---- crafted: redundancy ------------------------------------------------------------------------------------------------------------------------
def seen_by(slot, others, subject=0, rows=None):
    """a MapPoint in `slot` of the subject (frame `subject`) and at row r of the other frames"""
    return [(subject, slot)] + [(f, (rows or {}).get(f, slot)) for f in others]


def observations_3_and_4():
    """slot 0: five observers, Observations() 3: not examined.  slot 1: the same, Observations() 4: redundant.  slot 2: three observers and a
    stereo count of 6: examined, two others: counted only"""
    pts = [seen_by(0, [1, 2, 3, 4]), seen_by(1, [1, 2, 3, 4]), seen_by(2, [1, 2])]
    return craft_redundancy(5, 4, pts, [dict(kf=0, mp=[0, 1, 2])], nobs={0: 3, 1: 4, 2: 6})


def octave_edges():
    """the subject's octave is 2.  slot 0: four others at octave 3 (= octave_i + 1): redundant.  slot 1: three at 3 and one at 4: three qualify"""
    pts = [seen_by(0, [1, 2, 3, 4]), seen_by(1, [1, 2, 3, 4])]
    octv = {(0, 0): 2, (0, 1): 2}
    octv.update({(f, 0): 3 for f in (1, 2, 3, 4)})
    octv.update({(f, 1): 3 for f in (1, 2, 3)})
    octv[(4, 1)] = 4
    return craft_redundancy(5, 3, pts, [dict(kf=0, mp=[0, 1])], octaves=octv, default_octave=7)


def subject_one_of_four():
    """slot 0: the subject and three others; slot 1: the subject and four others, one of them bad"""
    pts = [seen_by(0, [1, 2, 3]), seen_by(1, [1, 2, 3, 4])]
    return craft_redundancy(5, 2, pts, [dict(kf=0, mp=[0, 1])], kf_flags=[0, 0, 0, 0, 1])


def depth_edges():
    pts = [seen_by(i, [1, 2, 3, 4]) for i in range(7)]
    th = f32(4.0)
    d = {(0, 0): th, (0, 1): np.nextafter(th, f32(9)), (0, 2): f32(-0.0), (0, 3): f32(-1e-30), (0, 4): f32(np.nan), (0, 5): f32(0.0), (0, 6): np.nextafter(th, f32(0))}
    return craft_redundancy(5, 7, pts, [dict(kf=0, mp=list(range(7)))], depth=d, th_depth=4.0, monocular=False)


def share(n_mps, n_redundant, th, monocular=True):
    """n_mps counted slots of which n_redundant are redundant"""
    pts = [seen_by(i, [1, 2, 3, 4] if i < n_redundant else [1]) for i in range(n_mps)]
    return craft_redundancy(5, max(n_mps, 1), pts, [dict(kf=0, mp=list(range(n_mps)))], redundant_th=th, monocular=monocular)


def initial_and_bad():
    pts = [seen_by(0, [1, 2, 3, 4], subject=f) for f in (0, 1, 2)]
    pts[1] = [(1, 0), (0, 0), (2, 0), (3, 0), (4, 0)]
    pts[2] = [(2, 0), (0, 0), (1, 0), (3, 0), (4, 0)]
    return craft_redundancy(5, 2, pts, [dict(kf=0, mp=[0]), dict(kf=1, mp=[1]), dict(kf=2, mp=[2]), dict(kf=3, mp=[-1, -1])], kf_flags=[2, 1, 0, 3, 0])


def redundancy_bad_index(kind):
    pts = [seen_by(0, [1, 2, 3, 4]), seen_by(1, [1, 2, 3, 4]), [(1, 0)]]
    s = craft_redundancy(5, 3, pts, [dict(kf=0, mp=[0, 1, 2]), dict(kf=0, mp=[1, -1, 2])], n_out=[3, 3, 3, 3, 2], nobs={2: 9})
    first = int(s["obs_off"][0])
    if kind == "row_high":
        s["obs"][first + 1, 1] = 3
    elif kind == "row_negative":
        s["obs"][first + 1, 1] = -1
    elif kind == "row_past_n_out":                           # frame 4 holds two keypoints
        s["obs"][first + 4, 1] = 2
    elif kind == "frame_high":
        s["obs"][first + 2, 0] = 5
    elif kind == "subject_kf_high":
        s["subject_kf"][0] = 5
    elif kind == "subject_kf_negative":
        s["subject_kf"][0] = -1
    elif kind == "mp_high":
        s["subject_mp"][0, 0] = 3
    elif kind == "offset_decreasing":
        s["obs_off"][0] = s["obs_off"][1] + 1
    elif kind == "not_examined_unchecked":                   # Observations() 3: the list is not walked, junk in it is no bad index
        s["mp_nobs"][0] = 3
        s["obs"][first + 1, 1] = 99
    return s


VOTE_BAD = ("mp_high", "mp_negative", "offset_negative", "offset_decreasing", "offset_past_total", "frame_high", "frame_negative", "subject_kf")
REDUNDANCY_BAD = ("row_high", "row_negative", "row_past_n_out", "frame_high", "subject_kf_high", "subject_kf_negative", "mp_high", "offset_decreasing")

CASES = {
    "update_th_14_15_16": th_14_15_16,
    "update_none_reach_th_tie": none_reach_th_tie,
    "update_three_equal_weights": three_equal_weights,
    "update_empty_counter": empty_counter,
    "update_point_in_two_slots": point_in_two_slots,
    "update_bad_map_point": bad_map_point,
    "update_bad_observer": lambda: bad_observer(UPDATE),
    "local_bad_observer": lambda: bad_observer(LOCAL),
    "update_other_map_and_self": lambda: other_map_and_self(UPDATE),
    "local_other_map_and_self": lambda: other_map_and_self(LOCAL),
    "update_conn_capacity_exact": lambda: conn_capacity(5),
    "update_conn_capacity_one_short": lambda: conn_capacity(4),
    "update_conn_capacity_ordered_fits": lambda: counter_longer_than_ordered(3),
    "update_conn_capacity_0": lambda: conn_capacity(0),
    "update_duplicate_keys": duplicate_keys,
    "update_bad_map_point_unchecked": lambda: bad_index("bad_map_point_unchecked"),
    "local_bad_frame_high": lambda: bad_index("frame_high", LOCAL),
    "local_subject_kf_ignored": lambda: bad_index("subject_kf", LOCAL),
    "redundancy_observations_3_and_4": observations_3_and_4,
    "redundancy_octave_edges": octave_edges,
    "redundancy_subject_one_of_four": subject_one_of_four,
    "redundancy_depth_edges": depth_edges,
    "redundancy_10_9": lambda: share(10, 9, 0.9),
    "redundancy_10_10": lambda: share(10, 10, 0.9),
    "redundancy_half_7_4": lambda: share(7, 4, 0.5, monocular=False),
    "redundancy_half_7_3": lambda: share(7, 3, 0.5, monocular=False),
    "redundancy_no_map_points": lambda: share(0, 0, 0.9),
    "redundancy_initial_and_bad": initial_and_bad,
    "redundancy_not_examined_unchecked": lambda: redundancy_bad_index("not_examined_unchecked"),
}
for _k in VOTE_BAD:
    CASES["update_bad_" + _k] = functools.partial(bad_index, _k)
for _k in REDUNDANCY_BAD:
    CASES["redundancy_bad_" + _k] = functools.partial(redundancy_bad_index, _k)
# seeded: n_frames 1, 2, 63, 64, 65, 257 and the LDS bound; N 0, 1, 63, 64, 65, 300; 1, 3 and 17 subjects; lists of 0, 1, 4, 5, 64, 65 and 3000
SEEDED_FRAMES = (1, 2, 63, 64, 65, 257)
SEEDED_N = (0, 1, 63, 64, 65, 300)
for _i, (_nf, _n) in enumerate(zip(SEEDED_FRAMES, SEEDED_N)):
    for _tag, _mode in (("update", UPDATE), ("local", LOCAL)):
        CASES["%s_frames%d_n%d" % (_tag, _nf, _n)] = functools.partial(seeded_vote, 10 + _i, _mode, _nf, _n, (1, 3, 17)[_i % 3],
                                                                       keys="reversed" if _i % 2 else "permuted")
    CASES["redundancy_frames%d_n%d" % (_nf, _n)] = functools.partial(seeded_redundancy, 20 + _i, _nf, _n, (1, 3, 17)[_i % 3], monocular=bool(_i % 2),
                                                                     redundant_th=0.5 if _i % 3 == 0 else 0.9, with_nobs=_i != 2)
CASES["update_frames257_n300_x17"] = functools.partial(seeded_vote, 31, UPDATE, 257, 300, 17, lens=(64, 65, 5, 4, 1, 0, 8), th=15)
CASES["local_frames257_n300_x17"] = functools.partial(seeded_vote, 32, LOCAL, 257, 300, 17, lens=(64, 65, 5, 4, 1, 0, 8))
CASES["update_frames257_short"] = functools.partial(seeded_vote, 33, UPDATE, 257, 300, 3, lens=(64, 65, 5, 4), conn_capacity=7)
CASES["update_frames%d" % MAX_FRAMES] = functools.partial(seeded_vote, 34, UPDATE, MAX_FRAMES, 300, 3, lens=(8, 64, 5, 65, 4), long_list=3000, th=2)
CASES["local_frames%d" % MAX_FRAMES] = functools.partial(seeded_vote, 35, LOCAL, MAX_FRAMES, 300, 3, lens=(8, 64, 5, 65, 4), long_list=3000)
CASES["redundancy_frames257_n300_x17"] = functools.partial(seeded_redundancy, 36, 257, 300, 17, lens=(64, 65, 5, 4, 1, 0, 8), monocular=False)
CASES["redundancy_frames4000_long_list"] = functools.partial(seeded_redundancy, 37, 4000, 65, 3, lens=(8, 5, 4), long_list=3000)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def case_expected(name):
    return CW.walk_scene(case(name))


# ---- the scenes on a device (tests/test_covisibility_gpu.py, tools/covisibility_rate.py) --------------------------------------------------------
VOTE_INPUTS = ("obs_off", "obs", "mp_flags", "kf_flags", "kf_map", "kf_key", "subject_mp", "subject_n", "subject_kf", "subject_map")
REDUNDANCY_INPUTS = ("obs_off", "obs", "mp_flags", "mp_nobs", "kf_flags", "kps_un", "n_out", "depth", "th_depth", "subject_mp", "subject_n", "subject_kf")


def to_device(a):
    """an array as a device tensor; an array without elements as one element, so that its pointer is not NULL"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.fields:
        a = a.view(np.uint8)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.size == 0:
        a = np.zeros(1, a.dtype)
    return torch.from_numpy(a).cuda()


def upload(s):
    """(poisoned outputs, inputs) of a scene as device tensors"""
    o = poisoned_outputs(s)
    names = VOTE_INPUTS if s["kind"] == "vote" else REDUNDANCY_INPUTS
    return dict((k, to_device(v)) for k, v in o.items()), dict((k, None if s[k] is None else to_device(s[k])) for k in names)


def call(ex, s, d, ins, **change):
    if s["kind"] == "vote":
        args = dict(mode=s["mode"], n_points=s["n_points"], d_obs_off=ins["obs_off"], d_obs=ins["obs"], d_mp_flags=ins["mp_flags"], n_frames=s["n_frames"],
                    d_kf_flags=ins["kf_flags"], d_kf_key=ins["kf_key"], n_subjects=s["n_subjects"], d_subject_mp=ins["subject_mp"],
                    d_subject_n=ins["subject_n"], capacity=s["capacity"], conn_capacity=s["conn_capacity"], d_counter_kf=d["counter_kf"],
                    d_counter_w=d["counter_w"], d_result=d["result"], d_kf_map_id=ins["kf_map"], d_subject_kf=ins["subject_kf"],
                    d_subject_map_id=ins["subject_map"], th=s["th"], d_ordered_kf=d["ordered_kf"], d_ordered_w=d["ordered_w"])
        ex.covisibility_device(**dict(args, **change))
    else:
        args = dict(n_points=s["n_points"], d_obs_off=ins["obs_off"], d_obs=ins["obs"], d_mp_flags=ins["mp_flags"], n_frames=s["n_frames"],
                    d_kf_flags=ins["kf_flags"], d_kps_un=ins["kps_un"], d_n_out=ins["n_out"], n_subjects=s["n_subjects"], d_subject_mp=ins["subject_mp"],
                    d_subject_n=ins["subject_n"], capacity=s["capacity"], d_subject_kf=ins["subject_kf"], d_result=d["result"],
                    monocular=bool(s["monocular"]), d_depth=ins["depth"], d_th_depth=ins["th_depth"], d_mp_nobs=ins["mp_nobs"], th_obs=s["th_obs"],
                    redundant_th=float(s["redundant_th"]), d_slot_state=d["slot_state"])
        ex.keyframe_redundancy_device(**dict(args, **change))


def download(s, d):
    o = poisoned_outputs(s)
    return dict((k, np.frombuffer(d[k].cpu().numpy().tobytes()[:o[k].nbytes], o[k].dtype).reshape(o[k].shape)) for k in o)
