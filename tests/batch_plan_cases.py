"""The calls the launch-plan tests share (tests/test_batch_plan.py on the CPU, tests/test_batch_plan_gpu.py and tools/record_batch_plan_forms.py on
the device): switch sets, shapes, the rows run with a real handle, the wider CPU-only grid, and how a row becomes a case line of
tests/cpp/batch_plan_check.cpp.

A row is (switch set, shape, steps); a step is (B, stages, profiling) with stages 3 = a whole extraction, 1 = the pyramid part alone
(orbx_compute_pyramid), 2 = the rest on the pyramid the handle holds (orbx_compute_keypoints_octree); the steps of a row run back to back on one
handle, so a back-only step sees what the step before it left."""

MAX_BATCH = 16
SHAPES = {"qvga": dict(rows=240, cols=320, nf=300), "vga": dict(rows=480, cols=640, nf=1000),
          "hd720": dict(rows=720, cols=1280, nf=1500), "hd1080": dict(rows=1080, cols=1920, nf=2000)}      # (the last two: CPU grid only)

SWITCH_SETS = {
    "default": {},
    "nofuse": {"ORBX_FUSE_SMALL": "0"},
    "pb": {"ORBX_PATCH_BLUR": "1", "ORBX_BLUR_SPLIT": "0"},
    "pbsplit": {"ORBX_PATCH_BLUR": "1"},
    "big": {"ORBX_SPLIT_MIN_MPX": "0"},
    "big_nofuse": {"ORBX_SPLIT_MIN_MPX": "0", "ORBX_FUSE_SMALL": "0"},
    "big_leaf8": {"ORBX_SPLIT_MIN_MPX": "0", "ORBX_LEAF_FRAMES": "8"},
    "big_split0": {"ORBX_SPLIT_MIN_MPX": "0", "ORBX_SPLIT": "0"},
    "leaf8": {"ORBX_LEAF_FRAMES": "8"},
    "oct256": {"ORBX_OCT_THREADS": "256"},
    "oct512": {"ORBX_OCT_THREADS": "512"},
    "oct1024": {"ORBX_OCT_THREADS": "1024"},
    "oct512r": {"ORBX_OCT_THREADS": "512", "ORBX_OCT_ROOMY": "1"},
    "pyr0": {"ORBX_PYR_COLS": "0"},
    "wide0": {"ORBX_FAST_WIDE": "0"},
    "wide1": {"ORBX_FAST_WIDE": "1"},
}
CPU_ONLY_SETS = {      # (forms that need more frames than the device rows take, or switches whose effect shows in no report)
    "split3": {"ORBX_SPLIT": "3"},
    "big_split3": {"ORBX_SPLIT_MIN_MPX": "0", "ORBX_SPLIT": "3"},
    "nopb": {"ORBX_PATCH_BLUR": "0"},
    "split2": {"ORBX_PATCH_BLUR": "1", "ORBX_BLUR_SPLIT": "2"},
    "leaf0": {"ORBX_LEAF_FRAMES": "0"},
    "bytewise": {"ORBX_RESIZE_BYTEWISE": "1"},
    "pyr1": {"ORBX_PYR_COLS": "1"},
    "roomy": {"ORBX_OCT_ROOMY": "1"},
    "shape4": {"aid:pyr_cols_shape": "4"},
}

FULL, FRONT, BACK = 3, 1, 2
WHOLE = lambda B: [(B, FULL, 0)]
FRONT_THEN_BACK = [(1, FRONT, 0), (1, BACK, 0)]

# The rows run on the device (B <= 16).  At 256 CUs: 640x480 has 815 FAST cells and cuts of 192 / 99 / 48 / 24 regions, 320x240 145 cells and
# 48 / 24 / 12 / 6 regions; a cut needs 192 workgroups, a shape with a CU per workgroup 256, a workgroup per FAST cell 1024 cells per call.
GPU_ROWS = [
    ("default", "vga", WHOLE(1)),             # blur in the FAST launch (form 1), cut 40, shape 6, k_fast_wide, 256-thread resident quad-tree
    ("default", "vga", WHOLE(2)),             # cut 56 (198 regions), shape 6; 1630 cells: k_fast
    ("default", "vga", WHOLE(3)),             # cut 56, 297 workgroups: shape 1
    ("default", "vga", WHOLE(4)),             # cut 80 (192), shape 4
    ("default", "vga", WHOLE(7)),             # cut 80
    ("default", "vga", WHOLE(8)),             # cut 112 (192)
    ("default", "vga", WHOLE(16)),
    ("default", "qvga", WHOLE(1)),            # ROIs beyond 45 px: k_blur in 8-row blocks (form 0), no k_fast_wide
    ("default", "qvga", WHOLE(7)),            # 1015 cells: a workgroup per cell ...
    ("default", "qvga", WHOLE(8)),            # ... 1160: not
    ("default", "qvga", WHOLE(16)),
    ("default", "vga", FRONT_THEN_BACK),      # a back-only pass after form 1: the FAST launch carries the owed blur
    ("default", "vga", [(1, FRONT, 0), (1, BACK, 1)]),      # ... with profiling switched on in between: the owed blur as a launch of its own
    ("default", "vga", [(1, FULL, 1)]),       # a profiled call: k_blur (form 0)
    ("default", "vga", [(1, FULL, 0), (1, BACK, 0)]),      # a back-only pass after a whole call
    ("nofuse", "vga", WHOLE(1)),
    ("nofuse", "vga", FRONT_THEN_BACK),       # ... after form 0
    ("pb", "vga", WHOLE(1)),
    ("pb", "vga", FRONT_THEN_BACK),           # ... after form 3
    ("pb", "qvga", WHOLE(3)),
    ("pbsplit", "vga", WHOLE(2)),             # form 5, the automatic split level 3
    ("pbsplit", "vga", FRONT_THEN_BACK),      # ... after form 5
    ("pbsplit", "qvga", WHOLE(1)),
    ("big", "qvga", WHOLE(2)),                # a big batch: blur on the side stream, staggered tails
    ("big", "qvga", WHOLE(5)),                # unequal halves
    ("big", "qvga", WHOLE(16)),
    ("big", "vga", WHOLE(16)),                # the blur rides in the FAST launch: no staggered tails
    ("big_nofuse", "vga", WHOLE(4)),          # per-keypoint blur by the big-batch ratio, split at level 3, both overlaps
    ("big_leaf8", "qvga", WHOLE(16)),         # the second half past the leaf tables: 1024-thread resident quad-tree
    ("big_leaf8", "qvga", WHOLE(9)),
    ("big_split0", "qvga", WHOLE(4)),         # a big batch with every overlap switched off
    ("leaf8", "vga", WHOLE(8)),
    ("leaf8", "vga", WHOLE(9)),               # past the leaf tables
    ("oct256", "vga", WHOLE(1)), ("oct512", "vga", WHOLE(1)), ("oct1024", "vga", WHOLE(1)), ("oct512r", "vga", WHOLE(1)),
    ("pyr0", "vga", WHOLE(2)),                # one launch per level
    ("wide0", "vga", WHOLE(1)),
    ("wide1", "vga", WHOLE(4)),
]

# B on either side of every threshold in numCUs at 256 CUs, for the shapes above: cuts (regions x B >= 192, > 3072), shapes (<= 256), a workgroup
# per cell (cells x B <= 1024), resident quad-trees (8 B <= 256, 8 B x 256 <= 768 x 256), the roomy build (8 B <= 1024), the blur's row blocks
# (lanes x B >= 131072), the leaf tables (128), big batches (120 Mpx of pyramid)
GRID_B = [1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 16, 17, 21, 22, 31, 32, 33, 42, 43, 62, 63, 64, 65, 96, 97, 126, 127, 128, 129, 256, 257, 384, 512]


def cpu_rows():
    """the device rows, every switch set over the grid of B for every shape (a handle for up to 512 frames), and back-only passes after each"""
    rows = [(s, shape, steps, MAX_BATCH) for s, shape, steps in GPU_ROWS]
    every = dict(SWITCH_SETS, **CPU_ONLY_SETS)
    for shape in SHAPES:
        for s in every:
            for B in GRID_B:
                rows.append((s, shape, WHOLE(B), 512))
            rows.append((s, shape, FRONT_THEN_BACK, 512))
            rows.append((s, shape, [(1, FRONT, 0), (1, BACK, 1)], 512))
            rows.append((s, shape, [(64, FULL, 1)], 512))
    return rows


def switches(name):
    return dict(SWITCH_SETS, **CPU_ONLY_SETS)[name]


def policy_tokens(env, max_batch, num_cus):
    """LaunchPolicy as orbx_create fills it from the switches (include/orbx.h), as tokens of the check program.  The leaf
    tables cover ORBX_LEAF_FRAMES frames (128) but no more than the handle's max_batch."""
    e = lambda k, d: int(env.get(k, d))
    return dict(numCUs=num_cus, pyrCols=e("ORBX_PYR_COLS", -1), fastWide=e("ORBX_FAST_WIDE", -1), patchBlur=e("ORBX_PATCH_BLUR", -1),
                blurSplit=e("ORBX_BLUR_SPLIT", -1), colsShape=e("aid:pyr_cols_shape", -1), splitMode=e("ORBX_SPLIT", 1), fuseSmall=e("ORBX_FUSE_SMALL", 1),
                splitMinPixels=int(float(env.get("ORBX_SPLIT_MIN_MPX", "120")) * 1e6), leafFrames=max(0, min(e("ORBX_LEAF_FRAMES", 128), max_batch)),
                octForced=e("ORBX_OCT_THREADS", 0), octRoomy=int("ORBX_OCT_ROOMY" in env), bytewise=int("ORBX_RESIZE_BYTEWISE" in env), arena=0)


def case_lines(row, num_cus):
    """one line of the check program per step of the row; steps after the first take the state the line before left (prev=1)"""
    name, shape, steps, max_batch = row
    tok = dict(SHAPES[shape], nlevels=8, sf=1.2, maxB=max_batch, **policy_tokens(switches(name), max_batch, num_cus))
    return [" ".join("%s=%s" % kv for kv in dict(tok, B=B, stages=stages, profiling=prof, prev=int(i > 0)).items()) for i, (B, stages, prof) in enumerate(steps)]


def reported_fields(stages):
    """what a step of these stages writes of the handle's report: the front part the pyramid form, its cut and the resize slot's kernel, the back
    part the FAST and quad-tree slots'; the blur form and its split level are the handle's after either"""
    return (["pyr_form", "cut_px", "resize"] if stages & FRONT else []) + ["blur_form", "split_level"] + (["fast", "octree"] if stages & BACK else [])


# ---- on the device (the recording tool and the GPU test) ----------------------------------------------------------------------------------
def run_gpu_rows(make_extractor, frames_of, on_step=None):
    """Runs GPU_ROWS: make_extractor(set name, shape name) -> ORBextractor (created with the set's switches, max_batch = MAX_BATCH),
    frames_of(shape name) -> uint8 [MAX_BATCH, rows, cols].  Returns per row the list of what each step reported (reported_fields);
    on_step(row index, step index, extractor, result) sees every step's result (a list of per-frame tuples, or the per-level keypoints of a
    back-only pass, or None after a pyramid alone)."""
    S_RESIZE, S_FAST, S_OCTREE = 1, 3, 4      # profile slots (include/orbx.h)
    out = []
    for r, (name, shape, steps) in enumerate(GPU_ROWS):
        ex = make_extractor(name, shape)
        fr = frames_of(shape)
        rec = []
        for i, (B, stages, prof) in enumerate(steps):
            ex.profile(bool(prof))
            if stages == FULL:
                res = ex.extract_batch(fr[:B])
            elif stages == FRONT:
                res = ex.ComputePyramid(fr[0])
            else:
                res = ex.ComputeKeyPointsOctTree()
            pyr_form, cut_px, blur_form = ex.last_forms()
            name_of = lambda slot: ex._L.orbx_profile_kernel_name_of(ex._h, slot).decode()
            seen = dict(pyr_form=pyr_form, cut_px=cut_px, blur_form=blur_form, split_level=ex._L.orbx_debug_last_split_level(ex._h),
                        resize=name_of(S_RESIZE), fast=name_of(S_FAST), octree=name_of(S_OCTREE))
            rec.append({k: seen[k] for k in reported_fields(stages)})
            if on_step:
                on_step(r, i, ex, res)
        ex.profile(False)
        out.append(rec)
    return out
