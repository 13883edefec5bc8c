"""The kernels of extractorb_amd/csrc/k_triangulate_match_two_eyes.hip in the SHIPPED library, read from its code objects
(tools/isa/kernel_table.py): no scratch, no spilled register of either kind, no FLAT instruction.  tests/test_kernel_table.py holds every
kernel to the checked-in table; this holds these to zero whatever the table says."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "isa"))
import kernel_table as KT  # noqa: E402
import extractorb_amd as X  # noqa: E402


def test_no_scratch_no_spills_no_flat():
    if not os.path.exists(os.path.join(KT.LLVM, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    table = KT.table(X.library_path())
    names = ["k_search_triangulation_two_eyes<0>", "k_search_triangulation_two_eyes<1>", "k_kb8_unproject", "k_kb8_triangulate"]
    for k in names:
        v = table[k]
        print(k, v)
        assert v["scratch_bytes"] == 0 and v["scratch_ops"] == 0 and v["sgpr_spill"] == 0 and v["vgpr_spill"] == 0 and v["flat"] == 0, (k, v)
        assert v["vgpr"] <= 256 and v["agpr"] == 0
