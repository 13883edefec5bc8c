"""Scenes for the MapPoint update (tests/test_map_point_update.py without a GPU, tests/test_map_point_update_gpu.py with one): a batch of
8 device frames at capacity 32 - eight one-camera keyframes or four rigs - and lists of MapPoints over it, as the arrays of the C entries.
  base(two_eyes, seed)             the frames: random descriptors, octaves, poses, N per frame; mTlr far from the identity
  with_points(base, points, ...)   the CSR arrays of a list of points, each dict(entries=[(frame, row[, flag])], ref=, name=)
  lengths(two_eyes)                lists of 0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 129, 1024 and 1025 entries, short and long interleaved
  crafted(two_eyes)                median ties, bad keyframes, bad indices, the two-eye reference centre, octaves outside the table
  working(two_eyes, seed)          2048 points over 32 frames at capacity 2024, a mean of about 6 entries and a tail into the hundreds"""
import numpy as np

f32 = np.float32
CAPACITY, FRAMES, NLEVELS = 32, 8, 8
# mTlr far from the identity (a rotation of 37 degrees about y and a translation of decimetres): a right centre taken for a left one shows
TLR = np.array([[0.8, 0.0, 0.6, 0.4], [0.0, 1.0, 0.0, -0.2], [-0.6, 0.0, 0.8, 0.1]], f32)


def scale_factors(nlevels=NLEVELS, factor=1.2):
    from fuse_walk import tables
    return tables(factor, nlevels)["scale"]


def rotation(rng, angle):
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def base(two_eyes, seed, capacity=CAPACITY, frames=FRAMES, nlevels=NLEVELS):
    rng = np.random.default_rng(seed)
    n_kf = frames // 2 if two_eyes else frames
    poses = np.zeros((n_kf, 3, 4), f32)
    for k in range(n_kf):
        poses[k, :, :3] = rotation(rng, rng.uniform(-0.5, 0.5)); poses[k, :, 3] = rng.uniform(-2, 2, 3)
    n_out = rng.integers(capacity * 5 // 8, capacity + 1, frames).astype(np.int32)
    n_out[frames - 1] = capacity
    return dict(two_eyes=two_eyes, capacity=capacity, nlevels=nlevels, scale=scale_factors(nlevels), tlr=TLR if two_eyes else None, poses=poses,
                n_out=n_out, desc=rng.integers(0, 256, (frames, capacity, 32)).astype(np.uint8),
                octave=rng.integers(0, nlevels, (frames, capacity)).astype(np.int32), rng=rng)


def with_points(b, points, n_slots=None, slot=None, no_flags=False):
    """points: dicts(entries = [(frame, row) or (frame, row, flag)], ref = position of mpRefKF's entry).  slot: None (= m) or a list"""
    s = dict(b)
    off = np.zeros(len(points) + 1, np.int32)
    obs, flags = [], []
    for m, pt in enumerate(points):
        off[m + 1] = off[m] + len(pt["entries"])
        obs += [(e[0], e[1]) for e in pt["entries"]]
        flags += [e[2] if len(e) > 2 else 0 for e in pt["entries"]]
    n_slots = n_slots or len(points)
    rng = np.random.default_rng(1234 + len(points))
    s.update(obs_off=off, obs=np.array(obs, np.int32).reshape(-1, 2), flags=None if no_flags else np.array(flags, np.uint8),
             ref=np.array([pt.get("ref", 0) for pt in points], np.int32), slot=None if slot is None else np.array(slot, np.int32),
             world=(rng.uniform(-6, 6, (n_slots, 3)) + np.array([0, 0, 14.0])).astype(f32),
             names=dict((pt["name"], m) for m, pt in enumerate(points) if "name" in pt))
    return s


def random_entries(b, rng, n, flagged=0.0):
    fr = rng.integers(0, len(b["n_out"]), n)
    rows = (rng.random(n) * b["n_out"][fr]).astype(np.int64)
    fl = (rng.random(n) < flagged).astype(np.int64)
    return [(int(f), int(r), int(x)) for f, r, x in zip(fr, rows, fl)]


LENGTHS = (1024, 1, 65, 2, 0, 17, 3, 129, 16, 4, 64, 15, 1025, 63, 5, 33, 2, 70, 7, 1, 16, 0, 64, 9)      # short and long as neighbours; 24 points: two workgroups


def lengths(two_eyes, seed=3, flagged=0.2):
    b = base(two_eyes, seed)
    rng = b["rng"]
    pts = []
    for n in LENGTHS:
        e = random_entries(b, rng, n, flagged)
        pts.append(dict(entries=e, ref=int(rng.integers(0, n)) if n else 0, name="len%d" % n))
    return b, pts


def flip(d, bits):
    d = d.copy()
    for k in bits:
        d[k >> 3] ^= 1 << (k & 7)
    return d


def crafted(two_eyes, seed=5):
    """the named points of the GPU test.  Descriptor rows 0 .. 15 of the last frame are written by hand"""
    b = base(two_eyes, seed)
    rng = b["rng"]
    F = FRAMES - 1
    D = b["desc"][F]
    c = D[0].copy()
    D[1] = flip(c, range(0, 40)); D[2] = flip(c, range(40, 80)); D[3] = flip(c, range(80, 120)); D[4] = flip(c, range(120, 160))
    D[5] = c; D[6] = c                                               # duplicates of row 0
    D[7] = flip(c, range(0, 3)); D[8] = flip(c, range(200, 256))     # near row 0; an outlier
    b["n_out"][0] = 20
    B = len(b["n_out"])
    some = lambda n: [(f, r) for f, r, _ in random_entries(b, rng, n)]
    pts = [
        # several rows share the least median (0: three copies among five, rank 2); the first of them is position 1
        dict(name="duplicates", entries=[(F, 8), (F, 0), (F, 5), (F, 6), (F, 1)], ref=2),
        # three entries, one outlier: the two near ones tie on their mutual distance, the first wins
        dict(name="outlier", entries=[(F, 0), (F, 7), (F, 8)], ref=1),
        # four spokes at 40 bits from the hub, 80 from one another: the hub's median (rank 2 of 5) is 40, a spoke's 80; the hub is LAST
        dict(name="best_last", entries=[(F, 1), (F, 2), (F, 3), (F, 4), (F, 0)], ref=0),
        # the same with the hub flagged bad: a spoke wins, and the normal still counts five entries
        dict(name="some_flagged", entries=[(F, 1), (F, 2, 1), (F, 3), (F, 4), (F, 0, 1)], ref=4),
        dict(name="all_flagged", entries=[(f, r, 1) for f, r in some(6)], ref=3),
        dict(name="plain", entries=some(7), ref=5),
        dict(name="frame_minus_one", entries=some(3) + [(-1, 0)] + some(2), ref=0),
        dict(name="frame_past", entries=some(2) + [(B, 0)], ref=0),
        dict(name="row_past", entries=[(0, int(b["n_out"][0]))] + some(4), ref=1),
        dict(name="ref_minus_one", entries=some(4), ref=-1),
        dict(name="ref_past", entries=some(4), ref=4),
        dict(name="flagged_bad_row", entries=some(3) + [(0, -1, 1)], ref=0),      # a flagged entry is checked as well
        dict(name="single", entries=[(2, 3)], ref=0),
        dict(name="pair", entries=[(2, 3), (5, 1)], ref=1),
    ]
    # octaves outside the table on the reference entry
    b["octave"][1, 2] = -1; b["octave"][1, 3] = b["nlevels"]; b["octave"][1, 4] = b["nlevels"] - 1; b["octave"][1, 5] = 0
    pts += [dict(name="octave_minus_one", entries=[(3, 1), (1, 2), (4, 0)], ref=1), dict(name="octave_nlevels", entries=[(1, 3), (3, 1), (4, 0)], ref=0),
            dict(name="octave_last", entries=[(1, 4), (3, 1), (4, 0)], ref=0), dict(name="octave_zero", entries=[(3, 1), (1, 5), (4, 0)], ref=1)]
    if two_eyes:
        pts += [
            # seen by both eyes of rig 1: the left entry, then the right one; mpRefKF is that rig, d_ref its left entry
            dict(name="both_eyes", entries=[(0, 4), (2, 7), (3, 9), (6, 1)], ref=1),
            # seen by right eyes only, d_ref on a right entry: the reference centre is the rig's LEFT centre all the same
            dict(name="right_only", entries=[(1, 4), (3, 9), (5, 2), (7, 11)], ref=1),
        ]
    return b, pts


def working(two_eyes, seed=17, points=2048, frames=32, capacity=2024, tail=24):
    b = base(two_eyes, seed, capacity=capacity, frames=frames)
    rng = b["rng"]
    n = np.minimum(rng.geometric(1 / 5.0, points) + 1, 40)           # a mean of about 6 ...
    long_ = rng.choice(points, tail, replace=False)
    n[long_] = rng.integers(65, 400, tail)                           # ... and a tail into the hundreds (tail = 0: none, for the rate tool)
    mid = rng.choice(points, tail // 3, replace=False)
    n[mid] = rng.integers(17, 65, tail // 3)
    pts = []
    for k in n:
        pts.append(dict(entries=random_entries(b, rng, int(k), 0.05), ref=int(rng.integers(0, k))))
    return with_points(b, pts, slot=rng.permutation(points).tolist())
