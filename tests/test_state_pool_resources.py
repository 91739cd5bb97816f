"""Register use of k_state_save / k_state_restore (dm_device.h, in the object of the reset / query / probe family), from the compiler's resource remarks
(deepmimic_amd/csrc/build/k_f32_11.o.res, written by `make`), by the pattern of tests/test_build_resources.py: every fp32 instantiation -- one per class of
DM_MISC_CLASSES -- spills no vector register and uses no scratch; k_state_save is a copy and uses no LDS."""
import os
import re

import pytest

BUILD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimic_amd", "csrc", "build")


@pytest.mark.parametrize("kernel,mangled", [("k_state_save", "_ZN3dmk12k_state_saveIf"), ("k_state_restore", "_ZN3dmk15k_state_restoreIf")])
def test_state_pool_kernels_do_not_spill_or_use_scratch_in_float(kernel, mangled):
    path = os.path.join(BUILD, "k_f32_11.o.res")
    if not os.path.exists(path):
        pytest.skip("no resource remarks (libdm_hip.so not built here)")
    blocks = re.split(r"remark: Function Name: ", open(path).read())
    mine = [b for b in blocks if b.startswith(mangled)]
    assert len(mine) >= 5, [b.split(" ")[0] for b in blocks[1:]]          # Biped, BipedObj, Large, LargeTree, BipedTree
    for b in mine:
        get = lambda pat: int(re.search(pat, b).group(1))
        assert get(r"VGPRs Spill: (\d+)") == 0 and get(r"ScratchSize \[bytes/lane\]: (\d+)") == 0, b.split(" ")[0]
        if kernel == "k_state_save":
            assert get(r"LDS Size \[bytes/block\]: (\d+)") == 0, b.split(" ")[0]
