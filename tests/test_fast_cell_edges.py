"""The FAST cells (k_fast<48,45>, k_fast<72,69>, k_fast_wide, with and without the blur's lanes, the two-dword build, leaf tables on and off) on
crafted scenes (tests/fast_cell_scenes.py).
CPU: the statement equals the oracle, in order, on every scene under every parameter set, and every planted probe is kept (or not) at the
threshold and with the response the scene's own text says; every named mutant of the statement is told apart by a named scene, or is shown
equivalent; the scenes hold the cell sizes, item counts, misalignments and masks they exist for; the host-only launch plan gives the
(shape, switch set) pairs every form.  GPU: debug_candidates in order against the statement, the whole result against the oracle, under
every switch set, in batches, and around degenerate calls.  docs/history/r29_fast_cell_edges.md has the tables."""
import functools
import os
import subprocess

import numpy as np
import pytest

import extractorb_amd as X
import fast_cell_scenes as S
import test_batch_plan as TBP

SCENES = S.crafted_scenes()
SWEEP = S.sweep_scenes()
BY_NAME = dict((s["name"], s) for s in SCENES + SWEEP)

# mutant -> the scene that tells it from the statement (test_every_mutant_is_caught_by_its_scene)
CAUGHT_BY = {
    "fast_ge": "threshold_steps", "arc_8": "arc_positions", "arc_10": "arc_positions", "arc_no_wrap": "arc_positions", "bright_only": "arc_positions",
    "dark_only": "arc_positions", "score_over_all_arcs_min": "arc_positions", "nms_ge": "nms_ties", "nms_4": "nms_ties", "nms_across_cells": "nms_ties",
    "no_retry": "threshold_steps", "retry_before_nms": "plateau_forces_retry", "retry_per_level": "threshold_steps", "response_is_score": "extremes",
    "interior_from_2": "cell_edges_62x62", "interior_to_max_minus_2": "cell_edges_62x62", "cell_floor": "cell_edges_62x153",
    "cell_w_35": "cell_edges_62x156", "order_level_raster": "nms_ties", "order_column_major": "nms_ties",
}
# mutants no scene can tell apart, and why
EQUIVALENT = {
    "nms_sees_sub_threshold": "a kept corner has S > t; a neighbour that is no corner at t has S <= t, so its score never reaches the corner's",
    "skip_x_minus3": "a column with maxBorderX - 6 <= iniX < maxBorderX - 3 has an ROI of 4 to 6 columns, on which cv::FAST evaluates nothing",
}


@functools.lru_cache(maxsize=None)
def expected(name, ini, mn, level=0):
    s = BY_NAME[name]
    return S.statement(S.oracle(s["img"], s["nlevels"], ini, mn)["levels"][level], ini, mn)


def test_scene_names_are_unique_and_small():
    assert len(BY_NAME) == len(SCENES) + len(SWEEP)
    for s in SCENES + SWEEP:
        assert s["img"].size <= 30000 or s["name"] in ("skipped_cells", "big"), s["name"]
        assert s["img"].dtype == np.uint8 and all(1 <= t <= 254 for p in s["params"] for t in p)


def test_the_smallest_frame_and_the_mirror_of_the_cell_list():
    """62 rows (or columns) is the least makeFrameGeom accepts; the mirror of its cell list agrees with the library's own report for every
    shape used here"""
    assert S.cell_geometry(62, 62) is not None and S.cell_geometry(61, 62) is None and S.cell_geometry(62, 61) is None
    X.compute_cell_grid(62, 62, 0, 1.2, 1)
    for shape in ((61, 62), (62, 61)):
        with pytest.raises(X.OrbxError):
            X.compute_cell_grid(shape[0], shape[1], 0, 1.2, 1)
    for s in SCENES + SWEEP:
        rows, cols = s["img"].shape
        g, lib = S.cell_geometry(rows, cols), X.compute_cell_grid(rows, cols, 0, 1.2, s["nlevels"])
        assert (g["nCols"], g["nRows"], g["wCell"], g["hCell"], len(g["cells"]), sum(c["cap"] for c in g["cells"])) == \
               (lib["n_cols"], lib["n_rows"], lib["w_cell"], lib["h_cell"], lib["n_cells"], lib["cand_cap"]), s["name"]
        # the statement visits the same cells
        cells = expected(s["name"], *s["params"][0])[1]
        assert [(c["i"], c["j"]) for c in cells] == [(c["i"], c["j"]) for c in g["cells"]], s["name"]


def test_scenes_hold_the_cell_shapes_they_are_for():
    geo = {s["name"]: S.cell_geometry(*s["img"].shape) for s in SCENES + SWEEP}
    cells = lambda names: [c for n in names for c in geo[n]["cells"]]
    # one-column frames 62 ... 91 wide: ROIs of 30 ... 59 columns, 24 ... 53 evaluated, 6 ... 14 items per row, either tile
    sweep = [geo["sweep_62x%d" % w] for w in range(62, 92)]
    assert [g["cells"][0]["roiW"] for g in sweep] == list(range(30, 60)) and all(len(g["cells"]) == 1 for g in sweep)
    assert [g["tile"] for g in sweep] == ["48x45"] * 16 + ["72x69"] * 14
    assert {g["cells"][0]["nq"] for g in sweep} == set(range(6, 15)) and {g["cells"][0]["last"] for g in sweep} == {1, 2, 3, 4}
    assert {c["roiH"] for n in geo if n.startswith("sweep_") for c in geo[n]["cells"]} >= {30, 38, 45, 46, 48, 59}
    # the first dword of a row is always whole: the interior starts on a tile dword (kFastTileShift = 1), so maskFirst is all ones
    assert {c["first"] for g in geo.values() for c in g["cells"]} == {0}
    # four columns of 31 at rectW 121 ... 124: every byte misalignment of the staged ROI, the clipped last cell at every width mod 4
    for w in (153, 154, 155, 156):
        g = geo["cell_edges_62x%d" % w]
        assert [c["gsh"] for c in g["cells"]] == [3, 2, 1, 0] and [c["cw"] for c in g["cells"]] == [31, 31, 31, w - 131]
    assert {geo["cell_edges_62x%d" % w]["cells"][-1]["last"] for w in (153, 154, 155, 156)} == {1, 2, 3, 4}
    # a lane keeps its item column (8 items per row: 64 % nq == 0) in cells 29 ... 32 wide, under either tile; every other width re-deals the lanes
    edges = cells(n for n in geo if n.startswith("cell_edges_"))
    assert {c["cw"] for c in edges if c["sx64"] == 0} == {29, 30, 31, 32} and {c["cw"] for c in edges if c["sx64"] != 0} >= {22, 23, 24, 25, 26, 27}
    assert geo["sweep_80x68"]["tile"] == "72x69" and geo["sweep_80x68"]["cells"][0]["nq"] == 8 and geo["cell_edges_62x68"]["tile"] == "48x45"
    # k_fast_wide's second trip: more than 256 items in a cell that fits the small tile
    for name in ("dense_104x104", "dense_106x108", "dense_graded_110x110"):
        assert geo[name]["tile"] == "48x45" and max(c["items"] for c in geo[name]["cells"]) > 256, name
    assert [(c["cw"], c["ch"]) for n in ("dense_104x104", "dense_106x108", "dense_graded_110x110") for c in geo[n]["cells"][:1]] == [(36, 36), (38, 37), (39, 39)]
    assert [c["cw"] for c in geo["dense_104x104"]["cells"]] == [36, 30, 36, 30]      # (the second column's ROI ends at the rectangle)
    assert max(c["items"] for n in ("dense_63x152", "nms_ties", "arc_positions") for c in geo[n]["cells"]) <= 256
    # the skipped column and the narrow last cell
    g = geo["skipped_cells"]
    assert g["nCols"] == 26 and [c["j"] for c in g["cells"]] == list(range(25)) and g["cells"][-1]["x0"] - S.MINB + 3 + g["cells"][-1]["cw"] - 1 == 777
    g = geo["big"]
    assert g["nCols"] == 138 and len(g["cells"]) == 135 and g["cells"][-1]["cw"] == 8 and g["rectW"] > 4096


@pytest.mark.parametrize("name", [s["name"] for s in SCENES + SWEEP])
def test_statement_equals_oracle_on_every_scene(name):
    s = BY_NAME[name]
    for ini, mn in s["params"]:
        want = S.oracle(s["img"], s["nlevels"], ini, mn)
        for l in range(s["nlevels"]):
            cands, cells = S.statement(want["levels"][l], ini, mn)
            assert cands == S.as_tuples(want["candidates"][l]), (name, ini, mn, l)
            assert sum(c["count"] for c in cells) == len(cands)
        # what the scene's own text promises of each probe: kept or not, the cell's threshold, the response
        cands, cells = expected(name, ini, mn)
        kept = S.kept_map(cands, cells)
        for p in s["probes"]:
            if p["params"] == (ini, mn):
                got = kept.get((p["x"], p["y"]))
                assert (got is not None) == p["kept"], (name, ini, mn, p)
                if p["kept"]:
                    assert got == (p["resp"], p["th"]), (name, ini, mn, p, got)
        if "counts" in s:
            assert [c["count"] for c in cells] == s["counts"][(ini, mn)], (name, ini, mn)


def test_scenes_reach_what_they_are_for():
    """properties of the answers that the scenes exist for (a scene that lost its branch must not pass silently)"""
    counts = lambda name, p=(20, 7), l=0: [c["count"] for c in expected(name, p[0], p[1], l)[1]]
    ths = lambda name, p=(20, 7): [c["th"] for c in expected(name, p[0], p[1])[1]]
    assert counts("threshold_steps") == [10, 1, 0, 2] and ths("threshold_steps") == [7, 20, 7, 20]
    assert counts("plateau_forces_retry") == [1, 1] and ths("plateau_forces_retry") == [7, 20]
    assert [r for _, _, r in expected("extremes", 254, 253)[0]] == [254, 254] and len(expected("extremes", 7, 20)[0]) == 5
    assert len([p for p in BY_NAME["arc_positions"]["probes"] if p["kept"]]) == 52 and len(BY_NAME["arc_positions"]["probes"]) == 84
    # more than 64 keys in a cell under each tile and in k_fast_wide's two-trip cells; the graded lattices keep about two fifths, from the first call
    print("dense counts:", {n: counts(n) for n in BY_NAME if n.startswith("dense_")})
    assert counts("dense_63x84") == [108] and counts("dense_63x152") == [72, 72, 72, 60] and min(counts("dense_104x104")) > 64
    assert max(counts("dense_106x108")) > 64 and counts("dense_skew_63x84")[0] > 64      # (the skew lattice: dots on odd and even rows)
    assert counts("dense_graded_63x84") == [43] and counts("dense_graded_63x152") == [29, 29, 29, 24] and set(ths("dense_graded_63x152")) == {20}
    for name, flat in (("dense_graded_63x84", "dense_63x84"), ("dense_graded_63x152", "dense_63x152")):      # ... while the retry would have kept them all
        s = BY_NAME[name]
        weak = S.statement(s["img"], 200, 7)
        assert [c["count"] for c in weak[1]] == counts(flat) and set(c["th"] for c in weak[1]) == {7}
    g = expected("dense_graded_110x110", 20, 7)
    assert min(c["count"] for c in g[1]) >= 48 and len(S.statement(BY_NAME["dense_graded_110x110"]["img"], 200, 7)[0]) > 4 * 64
    # three levels, every one with keys
    assert all(sum(counts("levels_3", l=l)) > 40 for l in range(3))
    # the skipped column: nothing from the strip, the two last evaluated columns kept
    xs = [x for x, _, _ in expected("skipped_cells", 20, 7)[0]]
    assert max(xs) == 777 and 776 in xs
    xs = [x for x, _, _ in expected("big", 20, 7)[0]]
    assert min(xs) == 3 and max(xs) == 4164 and {4095, 4096, 4097} <= set(xs) and 7 in ths("big") and counts("big")[32] == 2
    for r, w in S.CELL_EDGE_SHAPES:
        name = "cell_edges_%dx%d" % (r, w)
        assert counts(name) == [4] * len(S.cell_geometry(r, w)["cells"]), name
    # degenerate frames give nothing
    for s in (S.flat(63, 152), S.corners_outside_only(63, 152)):
        assert S.statement(s["img"], 20, 7)[0] == [] and len(S.oracle(s["img"], 1, 20, 7)["result"][1]) == 0
    assert S.score_map(S.corners_outside_only(63, 152)["img"]).max() == 60


def test_every_mutant_is_caught_by_its_scene():
    assert set(CAUGHT_BY) | set(EQUIVALENT) == set(S.MUTANTS) and not set(CAUGHT_BY) & set(EQUIVALENT)
    caught = {}
    for mutant in S.MUTANTS:
        for s in SCENES:
            for ini, mn in s["params"]:
                want = S.oracle(s["img"], s["nlevels"], ini, mn)
                for l in range(s["nlevels"]):
                    if S.statement(want["levels"][l], ini, mn, mutant=mutant)[0] != expected(s["name"], ini, mn, l)[0]:
                        caught.setdefault(mutant, set()).add(s["name"])
    print("mutants caught by:", dict((k, sorted(v)) for k, v in caught.items()))
    for mutant, where in CAUGHT_BY.items():
        assert where in caught.get(mutant, ()), (mutant, sorted(caught.get(mutant, ())))
    for mutant in EQUIVALENT:
        assert mutant not in caught, (mutant, caught.get(mutant))
    # the mutations the oracle carries too: the same candidates on the named scene
    for mutant, number in S.ORACLE_MUTATION.items():
        s = BY_NAME["skipped_cells" if mutant == "skip_x_minus3" else CAUGHT_BY[mutant]]
        differs = False
        for ini, mn in s["params"]:
            o = S.oracle(s["img"], s["nlevels"], ini, mn, mutation=number)
            assert S.as_tuples(o["candidates"][0]) == S.statement(s["img"], ini, mn, mutant=mutant)[0], (mutant, ini, mn)
            differs |= o["candidates"][0].tobytes() != S.oracle(s["img"], s["nlevels"], ini, mn)["candidates"][0].tobytes()
        assert differs == (mutant not in EQUIVALENT), mutant


# ---- which launch form every (scene shape, switch set) takes: the host-only plan (orbx_batch_plan.hpp) ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fce") / "batch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + TBP.CSRC, "-I" + os.path.join(TBP.ROOT, "include"),
                           os.path.join(TBP.ROOT, "tests", "cpp", "batch_plan_check.cpp"), "-o", exe])
    return exe


def shapes_of_the_device_tests():
    return sorted({(s["img"].shape[0], s["img"].shape[1], s["nlevels"]) for s in SCENES + SWEEP})


def test_the_plan_gives_the_scenes_every_form(checker):
    rows_, lines = [], []
    for rows, cols, nlevels in shapes_of_the_device_tests():
        for name, sw in S.SWITCH_SETS.items():
            rows_.append((rows, cols, nlevels, name)); lines.append(S.plan_line(rows, cols, nlevels, sw))
    seen, table = set(), {}
    for (rows, cols, nlevels, name), plan in zip(rows_, TBP.plans(checker, lines)):
        back = plan["back"]
        assert len(back) == 1
        b, G = back[0], plan["geom"]
        tile = "48x45" if max(G["maxRoiW"], G["maxRoiH"]) <= 45 else "72x69"
        form = (b["fastKernel"], tile, bool(b["carry"]), bool(G["big"]), bool(b["leafTables"]))
        if nlevels == 1:
            assert form == S.expected_form(rows, cols, nlevels, S.SWITCH_SETS[name]), (rows, cols, name, form)
            assert tile == S.cell_geometry(rows, cols)["tile"]
        assert bool(b["carry"]) == (plan["front"]["blurForm"] == 1) and not plan["batch"]["patchBlur"], (rows, cols, name)
        seen.add(form); table.setdefault(form, []).append((rows, cols, name))
    print("forms:", {k: len(v) for k, v in table.items()})
    kernels = {(k, t, c, big) for k, t, c, big, _ in seen}
    assert kernels >= {("k_fast", "48x45", True, False), ("k_fast", "48x45", False, False), ("k_fast", "72x69", False, False),
                       ("k_fast_wide", "48x45", True, False), ("k_fast_wide", "48x45", False, False), ("k_fast", "48x45", False, True)}
    assert {leaf for *_, leaf in seen} == {False, True}
    for k, t in (("k_fast", "48x45"), ("k_fast", "72x69"), ("k_fast_wide", "48x45")):
        assert {leaf for kk, tt, _, big, leaf in seen if (kk, tt) == (k, t) and not big} == {False, True}, (k, t)


def test_the_leaf_tables_reach_both_branches():
    """nLeafLocal: the leaf cells a FAST cell touches are collected in LDS when they fit the kernel's table, else every key goes to L2.  On these
    frames a leaf cell is 1 to 3 px wide, so most cells take the second branch; arc_positions (75 x 90 px roots) takes the first in both kernels,
    nms_ties (60 x 60 px roots) both, cell by cell.  skipped_cells has 25 roots: no leaf tables for that level."""
    reach = {s["name"]: S.leaf_branches(*s["img"].shape) for s in SCENES + SWEEP if s["nlevels"] == 1 and s["name"] != "big"}
    assert reach["arc_positions"] == {"k_fast": {"lds"}, "k_fast_wide": {"lds"}}
    assert reach["nms_ties"] == {"k_fast": {"l2", "lds"}, "k_fast_wide": {"l2", "lds"}}
    print("leaf branches:", {n: r for n, r in reach.items() if not n.startswith("sweep_")})
    assert reach["dense_63x152"] == {"k_fast": {"l2"}, "k_fast_wide": {"l2"}} and reach["dense_63x84"]["k_fast"] == {"l2"}
    assert reach["skipped_cells"]["k_fast"] == {"off"}
    for k in ("k_fast", "k_fast_wide"):
        assert set().union(*(r[k] for r in reach.values())) == {"lds", "l2", "off"}, k
    assert any(S.cell_geometry(*BY_NAME[n]["img"].shape)["tile"] == "72x69" and "l2" in r["k_fast"] for n, r in reach.items())


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _device(switches, monkeypatch):
    for k, v in S.SWITCH_SETS[switches].items():
        monkeypatch.setenv(k, v)
    X.debug_set_option("poison", 0xA5)
    X.debug_set_option("lds_pollute", 0xC3)
    return S.Device(X)


def _check_form(dev, ex, shape, nlevels, switches, B=1):
    kernel, tile, carry, big, leaf = S.expected_form(shape[0], shape[1], nlevels, S.SWITCH_SETS[switches], B)
    assert dev.fast_kernel(ex) == kernel, (shape, switches, dev.fast_kernel(ex))
    assert (ex.last_forms()[2] == 1) == carry, (shape, switches, ex.last_forms())


@pytest.mark.gpu
@pytest.mark.parametrize("switches", list(S.SWITCH_SETS))
def test_gpu_crafted_scenes_under_every_switch_set(switches, monkeypatch):
    """every scene under every parameter set it has: the candidates of every level in order against the statement, the result and the per-level
    keypoints against the oracle, over poisoned buffers; the launch takes the form the plan names"""
    dev = _device(switches, monkeypatch)
    wrong = []      # every scene runs, so that a failure names all the scenes that notice (a HIP error is no AssertionError: it ends the test at once)
    for s in SCENES + SWEEP:
        rows, cols = s["img"].shape
        for ini, mn in s["params"]:
            ex = dev.handle(rows, cols, s["nlevels"], ini, mn)
            out = ex(s["img"])
            if s["nlevels"] == 1:
                _check_form(dev, ex, (rows, cols), 1, switches)
            try:
                S.check_frame(ex, out, 0, s["img"], s["nlevels"], ini, mn, "%s %s %s" % (s["name"], (ini, mn), switches))
            except AssertionError as e:
                wrong.append("%s %s: %s" % (s["name"], (ini, mn), str(e).splitlines()[0][:160]))
    assert not wrong, "%d scene runs differ [%s]:\n%s" % (len(wrong), " ".join(sorted({w.split()[0] for w in wrong})), "\n".join(wrong))


@pytest.mark.gpu
@pytest.mark.parametrize("switches", ["default", "wide0", "wide0_nofuse", "leaf0"])
def test_gpu_batches(switches, monkeypatch):
    """three different scenes of one shape in one call, then one scene three times: per-frame segments and counts; equal frames, equal bytes"""
    dev = _device(switches, monkeypatch)
    for names in (("threshold_steps", "dense_63x152", "dense_graded_63x152"), ("dense_graded_63x152",) * 3, ("dense_63x84", "dense_graded_63x84", "dense_63x84")):
        frames = np.stack([BY_NAME[n]["img"] for n in names])
        rows, cols = frames.shape[1:]
        ex = dev.handle(rows, cols, 1, 20, 7, max_batch=3)
        for rep in range(2):
            out = ex.extract_batch(frames)
            _check_form(dev, ex, (rows, cols), 1, switches, B=3)
            for f, n in enumerate(names):
                S.check_frame(ex, out[f], f, frames[f], 1, 20, 7, "%s frame %d of %s, call %d, %s" % (n, f, names, rep, switches))
            for f, g in ((f, g) for f in range(3) for g in range(f) if names[f] == names[g]):
                assert ex.debug_candidates(0, f).tobytes() == ex.debug_candidates(0, g).tobytes()
                assert out[f][1].tobytes() == out[g][1].tobytes() and np.array_equal(out[f][2], out[g][2])


@pytest.mark.gpu
@pytest.mark.parametrize("switches", ["default", "wide0", "leaf0"])
@pytest.mark.parametrize("shape", [(63, 152), (63, 84)])
def test_gpu_degenerate_calls_between_normal_ones(shape, switches, monkeypatch):
    """on one handle: a normal frame, a flat frame (every count 0), the normal frame, a frame whose only corners lie outside the evaluated
    pixels, the normal frame again"""
    dev = _device(switches, monkeypatch)
    normal = BY_NAME["dense_graded_%dx%d" % shape]["img"]
    ex = dev.handle(shape[0], shape[1], 1, 20, 7)
    for step, img in enumerate((normal, S.flat(*shape)["img"], normal, S.corners_outside_only(*shape)["img"], normal)):
        out = ex(img)
        S.check_frame(ex, out, 0, img, 1, 20, 7, "step %d %s %s" % (step, shape, switches))
        if step in (1, 3):
            assert len(ex.debug_candidates(0)) == 0 and out[0] == 0 and len(out[1]) == 0 and out[2].shape == (0, 32)
        else:
            assert len(out[1]) > 20
