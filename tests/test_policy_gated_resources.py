"""Register / LDS budget of the gated one-launch actor (k_policy_fused<.., true>, deepmimic_amd/csrc/dm_policy.h) from the resource remarks and the disassembly
of the shipped object, in the style of tests/test_build_resources.py: two workgroups per CU, and no scratch instruction inside the k loops over the weight
stream.  Skipped when the library was not built in this checkout."""
import os
import re
import subprocess
import tempfile

import pytest

from test_build_resources import BUILD, LLVM_BIN

GATED_FUSED = re.compile(r"k_policy_fusedILi(8|12)ELi(2|4)ELb1E")


def test_gated_fused_kernels_fit_two_workgroups_per_cu():
    path = os.path.join(BUILD, "dm_host.o.res")
    if not os.path.exists(path):
        pytest.skip("no resource remarks (libdm_hip.so not built here)")
    blocks = re.split(r"remark: Function Name: ", open(path).read())[1:]
    mine = [b for b in blocks if GATED_FUSED.search(b.split()[0])]
    assert len(mine) == 4, [b.split()[0] for b in blocks]
    for b in mine:
        get = lambda pat: int(re.search(pat, b).group(1))
        # 160 KB of LDS per CU, two workgroups of four waves: 80 KB and 256 VGPRs each
        assert get(r"Occupancy \[waves/SIMD\]: (\d+)") == 2 and get(r"LDS Size \[bytes/block\]: (\d+)") <= 81920 and get(r"\bVGPRs: (\d+)") <= 256, b[:600]
        # measured: 0 spilled VGPRs at K1 = 256, 2 / 4 at K1 = 384, 136 .. 152 bytes of scratch per lane, touched in the gate prologue and the head only (below)
        assert get(r"VGPRs Spill: (\d+)") <= 8 and get(r"ScratchSize \[bytes/lane\]: (\d+)") <= 192, b[:600]


def test_no_scratch_instruction_inside_the_k_loops_of_the_gated_fused_kernels():
    """The kernel has ten barriers: observations, goal block, c, e_i (the gate prologue), one per layer-1 chunk, h2, logp.  Everything that walks the weight stream
    -- the four chunks with their gated epilogues and the gated layer-2 epilogue -- lies between the fourth and the ninth; the few scratch accesses of the shipped
    build sit in the gate prologue and, at K1 = 384, in the head."""
    obj = os.path.join(BUILD, "dm_host.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM_BIN, "llvm-objdump")):
        pytest.skip("no object / no LLVM tools here")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "x.fat"), os.path.join(d, "x.co")
        subprocess.check_call([os.path.join(LLVM_BIN, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
        subprocess.check_call([os.path.join(LLVM_BIN, "clang-offload-bundler"), "--type=o", "--unbundle", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        txt = subprocess.check_output([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
    kernels, cur = {}, None
    for line in txt.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = kernels.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(line.split("//")[0].strip())
    mine = {n: b for n, b in kernels.items() if GATED_FUSED.search(n)}
    assert len(mine) == 4, list(kernels)
    for n, body in mine.items():
        bar = [i for i, ins in enumerate(body) if ins.startswith("s_barrier")]
        assert len(bar) == 10, (n, bar)
        mfma = [i for i, ins in enumerate(body) if ins.startswith("v_mfma") and bar[3] < i < bar[8]]
        assert len(mfma) >= 4 * (8 * 8 + 128 + 32) + 64, (n, len(mfma))          # the stream's MFMAs are all in there
        inside = [(i, ins) for i, ins in enumerate(body) if ins.startswith(("scratch_", "buffer_")) and bar[3] < i < bar[8]]
        assert not inside, (n, inside[:8])
