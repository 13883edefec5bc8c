"""The launch-plan rows (tests/batch_plan_cases.py: GPU_ROWS) with a real handle: every call reports the forms, the split level and the kernel
names of tests/golden/batch_plan_forms.json - what the library of the commit before csrc/orbx_batch_plan.hpp existed reported for the same calls -
and gives, whatever form it took, the results of serial single-frame extractions byte for byte (a back-only pass: their per-level keypoints).
One handle per switch set and shape, 320 x 240 x 300 features and 640 x 480 x 1000, at most 16 frames per call."""
import json
import os

import pytest

import extractorb_amd as X
from extractorb_amd import synth
from helpers import assert_same_result
import batch_plan_cases as P

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_plan_forms.json")


@pytest.fixture(scope="module")
def serial():
    """per shape: the frames and what a one-frame handle with the default switches makes of each (mono, keypoints, descriptors, per level)"""
    out = {}
    for shape in ("qvga", "vga"):
        s = P.SHAPES[shape]
        fr = synth.frames("textured", 40, P.MAX_BATCH, s["rows"], s["cols"])
        one = X.ORBextractor(s["nf"], max_width=s["cols"], max_height=s["rows"])
        out[shape] = fr, [one(fr[f]) for f in range(P.MAX_BATCH)]
    return out


def test_every_row_reports_the_recorded_forms_and_gives_the_serial_results(serial):
    import torch
    golden = json.load(open(GOLDEN))
    assert golden["numCUs"] == torch.cuda.get_device_properties(0).multi_processor_count, "the table was recorded on a device with another CU count"
    made = {}
    mp = pytest.MonkeyPatch()

    def make(name, shape):
        if (name, shape) not in made:
            with mp.context() as m:
                for k, v in P.switches(name).items():
                    m.setenv(k, v)
                s = P.SHAPES[shape]
                made[name, shape] = X.ORBextractor(s["nf"], max_width=s["cols"], max_height=s["rows"], max_batch=P.MAX_BATCH)
        return made[name, shape]

    def check(r, i, ex, res):
        name, shape, steps = P.GPU_ROWS[r]
        B, stages, _ = steps[i]
        want = serial[shape][1]
        what = "row %d (%s, %s) step %d %s" % (r, name, shape, i, steps[i])
        if stages == P.FULL:
            for f in range(B):
                assert_same_result(res[f][:3], want[f][:3], "%s frame %d" % (what, f))
                assert all(a.tobytes() == b.tobytes() for a, b in zip(res[f][3], want[f][3])), "%s frame %d: per-level keypoints" % (what, f)
        elif stages == P.BACK:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(res, want[0][3])), "%s: per-level keypoints of the back-only pass" % what

    got = P.run_gpu_rows(make, lambda shape: serial[shape][0], check)
    for r, (g, rec) in enumerate(zip(got, golden["rows"])):
        assert (rec["set"], rec["shape"], [tuple(s) for s in rec["steps"]]) == (P.GPU_ROWS[r][0], P.GPU_ROWS[r][1], [tuple(s) for s in P.GPU_ROWS[r][2]])
        assert g == rec["reported"], "row %d %s" % (r, P.GPU_ROWS[r])
