#!/usr/bin/env python3
"""Records what the library reports for the launch-plan rows (tests/batch_plan_cases.py: GPU_ROWS) on the device: the pyramid form, cut and blur
form of orbx_debug_last_forms, orbx_debug_last_split_level, the kernel names of the resize, FAST and quad-tree slots, and the device's CU count.
tests/golden/batch_plan_forms.json is this recording made with the library of the commit BEFORE the plan header existed (tools/ab_build.sh,
ORBX_LIBRARY=build/ab/liborbx_head.so); a recording of the working tree's library must be identical to it.
usage (GPU box): [ORBX_LIBRARY=...] python tools/record_batch_plan_forms.py OUT.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import extractorb_amd as X
from extractorb_amd import synth
import batch_plan_cases as P


def main(out):
    made = {}

    def make(name, shape):
        if (name, shape) not in made:
            env = P.switches(name)
            for k in [k for k in os.environ if k.startswith("ORBX_") and k not in ("ORBX_LIBRARY",)]:
                del os.environ[k]
            os.environ.update({k: v for k, v in env.items() if not k.startswith("aid:")})
            s = P.SHAPES[shape]
            made[name, shape] = X.ORBextractor(s["nf"], max_width=s["cols"], max_height=s["rows"], max_batch=P.MAX_BATCH)
        return made[name, shape]

    frames = {shape: synth.frames("textured", 40, P.MAX_BATCH, P.SHAPES[shape]["rows"], P.SHAPES[shape]["cols"]) for shape in ("qvga", "vga")}
    rec = P.run_gpu_rows(make, frames.__getitem__)
    rows = [dict(set=name, shape=shape, steps=[list(s) for s in steps], reported=r) for (name, shape, steps), r in zip(P.GPU_ROWS, rec)]
    with open(out, "w") as f:
        json.dump(dict(numCUs=torch.cuda.get_device_properties(0).multi_processor_count, max_batch=P.MAX_BATCH, rows=rows), f, indent=1)
        f.write("\n")
    print("%d rows -> %s" % (len(rows), out))


if __name__ == "__main__":
    main(sys.argv[1])
