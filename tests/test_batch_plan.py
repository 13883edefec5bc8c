"""The launch policy of the extraction path without a GPU: tests/cpp/batch_plan_check.cpp prints the plans extractorb_amd/csrc/orbx_batch_plan.hpp
makes (planGeometry, planBatch, planFront, planBack) for case lines; here they are compared

  * with tests/golden/batch_plan_forms.json, what the library of the commit before the header existed reported on an MI355X for the same calls
    (tools/record_batch_plan_forms.py: forms, cut, split level, kernel names), and
  * over a grid of frame counts on either side of every threshold, shapes and switch sets, with an independent statement in Python of the
    rules for what no report shows: the side-stream blur, the staggered tails and their first half, the workgroup shape of k_pyr_cols, the leaf
    tables, the owed blur (carried by the FAST launch or launched in front of it), the blur table a front part launches, the per-level
    quad-tree sizes.

The grid must cross every decision: every boolean and every enumerated field of the three plans takes each of its values in some line."""
import json
import os
import subprocess

import pytest

import batch_plan_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "extractorb_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "batch_plan_forms.json")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bpc") / "batch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "batch_plan_check.cpp"), "-o", exe])
    return exe


def plans(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_the_plans_report_what_the_library_reported_on_the_device(checker, golden):
    assert golden["max_batch"] == P.MAX_BATCH and len(golden["rows"]) == len(P.GPU_ROWS)
    lines, where = [], []
    for r, (row, rec) in enumerate(zip(P.GPU_ROWS, golden["rows"])):
        assert (rec["set"], rec["shape"], [tuple(s) for s in rec["steps"]]) == (row[0], row[1], [tuple(s) for s in row[2]]), "row %d: the table was recorded for other rows" % r
        for i, line in enumerate(P.case_lines(row + (P.MAX_BATCH,), golden["numCUs"])):
            lines.append(line); where.append((r, i))
    for (r, i), plan in zip(where, plans(checker, lines)):
        stages = P.GPU_ROWS[r][2][i][1]
        got = {k: plan["reported"][k] for k in P.reported_fields(stages)}
        assert got == golden["rows"][r]["reported"][i], "row %d %s step %d" % (r, P.GPU_ROWS[r], i)


# ---- the rules no report shows, stated once more (the thresholds are those of the comments in orbx_batch_plan.hpp) ----
def expect_unreported(tok, step, plan, owed_before):
    """tok: the policy tokens of the line; step: (B, stages, profiling); plan: the program's output; owed_before: the blur the earlier call left owed"""
    B, stages, prof = step
    G, cus = plan["geom"], tok["numCUs"]
    lanes32 = sum(-(-h // 32) * -(-w // 4) for w, h in zip(G["w"], G["h"]))      # four columns a lane, 32-row blocks
    fills_chip = lambda Bn: lanes32 * Bn >= 2 * 4 * 64 * cus                    # two waves per SIMD
    rides = lambda Bn: not fills_chip(Bn) and not prof and tok["fuseSmall"] and max(G["maxRoiW"], G["maxRoiH"]) <= 45 and not G["big"]
    big_batch = G["sumPixels"] * B >= tok["splitMinPixels"]
    whole = stages == P.FULL
    want = dict(bigBatch=big_batch, blurSide=tok["splitMode"] != 0 and big_batch and not prof and whole)
    small_frame = tok["rows"] * tok["cols"] <= 512 * 1024
    want["stagger"] = whole and big_batch and not prof and B >= 2 and not rides(B) and (tok["splitMode"] == 3 or (tok["splitMode"] == 1 and small_frame))
    want["B0"] = (B + 1) // 2 if want["stagger"] else B
    front = None
    if stages & P.FRONT:
        f = plan["front"]
        front = dict(blurOwed=f["blurForm"] == 1)
        if f["cut"] >= 0:
            wgs = G["cuts"][f["cut"]]["regions"] * B
            front["colsShape"] = tok["colsShape"] if tok["colsShape"] > 0 else ((6 if f["cutPx"] <= 56 else 4) if wgs <= cus else 1)
        table = {5: 2, 3: -1, 1: -1, 0: 0 if fills_chip(B) else 1}[f["blurForm"]]
        front.update(blurTable=table, blurBlockRows={-1: 0, 0: 32, 1: 8, 2: 32}[table])
    back = []
    if stages & P.BACK:
        owed = front["blurOwed"] if front else owed_before
        halves = [(0, want["B0"]), (want["B0"], B - want["B0"])] if want["stagger"] else [(0, B)]
        for f0, Bn in halves:
            carry = owed and rides(Bn)
            back.append(dict(f0=f0, Bn=Bn, leafTables=tok["leafFrames"] > 0 and f0 + Bn <= tok["leafFrames"] and not G["big"], carry=carry, blurFirst=owed and not carry))
            owed = False
    return want, front, back


def test_the_unreported_rules_over_the_grid_and_the_grid_crosses_every_decision(checker):
    rows = P.cpu_rows()
    lines, where = [], []
    for r, row in enumerate(rows):
        for i, line in enumerate(P.case_lines(row, 256)):
            lines.append(line); where.append((r, i))
    out = plans(checker, lines)
    seen = {}
    note = lambda k, v: seen.setdefault(k, set()).add(v)
    owed = False
    for (r, i), line, plan in zip(where, lines, out):
        name, shape, steps, max_batch = rows[r]
        tok = {k: float(v) if "." in v else int(v) for k, v in (t.split("=") for t in line.split())}
        what = "%s %s max_batch %d step %d %s" % (name, shape, max_batch, i, steps[i])
        want, front, back = expect_unreported(tok, steps[i], plan, owed if i else False)
        assert {k: plan["batch"][k] for k in want} == {k: int(v) for k, v in want.items()}, what
        b = plan["batch"]
        assert b["splitL"] == 0 or b["patchBlur"], what
        for k, v in b.items():
            if k != "B0": note("batch." + k, v if k != "splitL" else bool(v))
        if front is not None:
            f = plan["front"]
            assert {k: f[k] for k in front} == {k: int(v) for k, v in front.items()}, what
            assert f["pyrForm"] == (0 if f["cut"] >= 0 else 1) and f["resizeKernel"] == ("k_pyr_cols" if f["cut"] >= 0 else "k_resize"), what
            assert (f["blurForm"] in (3, 5)) == bool(b["patchBlur"]) and (f["blurForm"] == 5) == bool(b["splitL"]), what
            for k in ("cutPx", "pyrForm", "colsShape", "resizeKernel", "blurForm", "blurTable", "blurBlockRows", "blurOwed"):
                note("front." + k, f[k])
        else:
            assert "front" not in plan, what
        assert len(plan.get("back", [])) == len(back), what
        for got, exp in zip(plan.get("back", []), back):
            assert {k: got[k] for k in exp} == {k: int(v) for k, v in exp.items()}, what
            assert len(set(got["octT"])) == 1 and len(got["octT"]) == plan["geom"]["nlevels"], what      # one size for every level ...
            T, roomy = got["octT"][0], got["roomy"]
            assert got["octKernel"] == "k_octree_%d%s" % (T, "r" if roomy else ""), what                 # ... the one the kernel's name carries
            assert got["fastKernel"] == ("k_fast_wide" if got["wide"] and max(plan["geom"]["maxRoiW"], plan["geom"]["maxRoiH"]) <= 45 else "k_fast"), what
            for k in ("leafTables", "carry", "blurFirst", "wide", "fastKernel", "roomy"):
                note("back." + k, got[k])
            note("back.octT", (T, roomy))
        owed = bool(plan["left"]["blurOwed"])
    both = {0, 1}
    for k in ("batch.bigBatch", "batch.patchBlur", "batch.blurSide", "batch.stagger", "front.blurOwed", "back.leafTables", "back.carry", "back.blurFirst", "back.wide", "back.roomy", "front.pyrForm"):
        assert seen[k] == both, (k, seen[k])
    assert seen["batch.splitL"] == {False, True}
    assert seen["front.blurForm"] == {0, 1, 3, 5} and seen["front.blurTable"] == {-1, 0, 1, 2} and seen["front.blurBlockRows"] == {0, 8, 32}
    assert seen["front.colsShape"] == {0, 1, 4, 6} and seen["front.cutPx"] >= {0, 40, 56, 80, 112}
    assert seen["front.resizeKernel"] == {"k_pyr_cols", "k_resize"} and seen["back.fastKernel"] == {"k_fast", "k_fast_wide"}
    assert seen["back.octT"] == {(T, r) for T in (256, 512, 1024) for r in (0, 1)}, seen["back.octT"]


def test_a_back_only_pass_repeats_the_blur_form_of_the_call_before(checker):
    """after each blur form: per keypoint again where no blurred level exists (3), split at the same level (5), from the blurred levels else"""
    base = "rows=480 cols=640 nf=1000 maxB=1 leafFrames=1 B=1 stages=2 "
    cases = [(0, 0), (1, 0), (3, 0), (5, 3), (5, 2)]
    out = plans(checker, [base + "lastBlurForm=%d lastSplitLevel=%d blurSplit=4" % c for c in cases])
    for (form, split), plan in zip(cases, out):
        assert plan["batch"]["patchBlur"] == int(form in (3, 5)) and plan["batch"]["splitL"] == split, (form, split, plan["batch"])
        assert plan["left"]["lastBlurForm"] == form and plan["reported"]["split_level"] == split


def test_the_quad_tree_build_with_its_node_arrays_in_hbm_has_one_name(checker):
    out = plans(checker, ["rows=480 cols=640 nf=25000 arena=1 B=%d octRoomy=%d" % c for c in ((1, 0), (64, 0), (1, 1))])
    assert [o["back"][0]["octKernel"] for o in out] == ["k_octree_1024g"] * 3


def test_the_geometry_plan(checker):
    """the split level: automatic (the first level whose patches hold more than 1.5 x its pixels, if those levels hold a quarter of the
    features), pinned, off, and never a level the pyramid does not have; the quad-tree size by image area; table [2] empty without a split"""
    line = lambda shape, **kw: " ".join("%s=%s" % kv for kv in dict(P.SHAPES[shape], **kw).items())
    out = plans(checker, [line("vga"), line("hd720"), line("hd1080"), line("vga", blurSplit=0), line("vga", blurSplit=5), line("vga", blurSplit=8),
                          line("vga", octForced=1024), line("vga", octForced=300), line("qvga")])
    gp = [o["geometryPlan"] for o in out]
    assert [g["splitLevel"] for g in gp] == [3, 0, 0, 0, 5, 0, 3, 3, 2]
    assert [g["octThreads"] for g in gp] == [256, 512, 1024, 256, 256, 256, 1024, 256, 256]
    for o, g in zip(out, gp):
        w, h = o["geom"]["w"], o["geom"]["h"]
        lanes = lambda rows, l0: sum(-(-hh // rows) * -(-ww // 4) for ww, hh in list(zip(w, h))[l0:])
        assert g["nBlurLanes"] == [lanes(32, 0), lanes(8, 0), lanes(32, g["splitLevel"]) if g["splitLevel"] else 0]
        assert g["blurItemOff"] == [0, g["nBlurItems"][0], g["nBlurItems"][0] + g["nBlurItems"][1]]
        assert g["blurLaneOff"] == [0, g["nBlurLanes"][0], g["nBlurLanes"][0] + g["nBlurLanes"][1]]


def test_the_header_and_the_kernel_file_state_the_same_roi_limit():
    """orbx_batch_plan.hpp is host only and cannot call k_fast.hip's fastCanCarryBlur: both say 45 x 45"""
    assert "bool fastCanCarryBlur(int maxRoiW, int maxRoiH) { return maxRoiW <= 45 && maxRoiH <= 45; }" in open(os.path.join(CSRC, "k_fast.hip")).read()
    assert "inline bool roiFitsFastTile(const FrameGeom& g) { return g.maxRoiW <= 45 && g.maxRoiH <= 45; }" in open(os.path.join(CSRC, "orbx_batch_plan.hpp")).read()


def test_no_bare_blur_form_number_is_left_in_the_host_files():
    import re
    for f in ("orbx_api.cpp", "orbx_debug.cpp"):
        code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
        assert not re.findall(r"lastBlurForm\s*[=!]=\s*\d", code), f
