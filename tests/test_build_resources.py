"""Register / scratch budget of the compiled step kernels, read from the resource remarks the build leaves next to every object
(deepmimic_amd/csrc/build/k_f32_<family>.o.res, written by `make`: -Rpass-analysis=kernel-resource-usage).  A production kernel that
starts spilling is a silent 1.7x (dog3d: one divergent store in the level buffer of the tree factor cost 389 spilled VGPRs and nobody
saw it until the next profile) -- this holds the budgets the measurements in DESIGN.md section 6 / 7 were taken at.  Skipped when the
library was not built in this checkout."""
import os
import re

import pytest

BUILD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimic_amd", "csrc", "build")


def _res(family, prec="f32"):
    path = os.path.join(BUILD, "k_%s_%d.o.res" % (prec, family))
    if not os.path.exists(path):
        pytest.skip("no resource remarks (libdm_hip.so not built here)")
    txt = open(path).read()
    out = {}
    for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                     ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
        vals = [int(v) for v in re.findall(pat, txt)]
        assert vals, (path, key)
        out[key] = max(vals) if key != "occupancy" else min(vals)
    return out


# family ids: deepmimic_amd/csrc/dm_kernels.cpp
@pytest.mark.parametrize("family,what,occupancy,lds_max", [
    (0, "two characters per wavefront, plain (the headline kernel)", 2, 20480),
    (1, "two characters per wavefront, AMP / goal / perturbation instantiation", 2, 20480),
    (7, "ClsLarge, AMP", 2, 20480),
    (12, "ClsLargeTree (dog3d on its compiled topology), plain", 2, 20480),
    (13, "ClsLargeTree, AMP (dog3d imitate_amp)", 2, 20480),
])
def test_production_kernels_do_not_spill_vector_registers(family, what, occupancy, lds_max):
    r = _res(family)
    if family in (0, 1):
        # round 6: the borrowed-lane path (DuoSim lane borrowing, a rare branch of the update loop) shares the two-per-wave kernels' register file: measured 1 / 7 spilled
        # VGPRs (29 / 42 before that path re-read the lanes' candidate tables behind itself: 10 MB of prologue spill stores per 4096-env launch).  The hot path is held
        # free of scratch by the disassembly test below; here the budget
        # round 6, second pass: the y = L^-1 J^T loop without its per-dof `k < D` branches (DuoSim::YFULL) keeps both look-ahead sets honest -- measured 33 / 13: spilled
        # in the prologue, reloaded in the epilogue and inside the beyond-32-rows region only (the disassembly test below holds that), -2 % kernel time in the same-box A/B
        assert r["spill"] <= (40 if family == 0 else 16), (what, r)
    else:
        assert r["spill"] == 0, (what, r)
    assert r["occupancy"] == occupancy and r["lds"] <= lds_max, (what, r)          # 160 KB LDS per CU: 8 (16) waves need <= 20480 (10240) B each


LLVM_BIN = "/opt/rocm/lib/llvm/bin"


def _disassemble(family, prec="f32"):
    """the gfx950 code object of one kernel family, disassembled (llvm-objcopy -> clang-offload-bundler -> llvm-objdump, NOTES.md)"""
    import subprocess
    import tempfile
    obj = os.path.join(BUILD, "k_%s_%d.o" % (prec, family))
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
    return kernels


def test_no_scratch_access_on_the_hot_path_of_the_headline_and_dog_kernels():
    """`ScratchSize` > 0 in the resource remarks does not say whether an instruction touches scratch.  From the disassembly of the shipped objects:
    * family 12 (dog3d, ClsLargeTree plain): not one scratch_ / buffer_ instruction in the step kernel;
    * family 0 (the headline two-per-wave kernel): inside the update loop -- between the first and the last s_setprio, priorities are only set there -- every
      scratch access lies in the borrowed-lane region (bracketed by `s_nop 13` / `s_nop 14`, DM_REGION_MARK), and none of them is a store: the spilled values
      are written once in the prologue."""
    dog = _disassemble(12)
    k = [v for n, v in dog.items() if "k_env_step" in n and "ClsLargeTree" in n]
    assert k, list(dog)
    for body in k:
        assert not [i for i in body if i.startswith(("scratch_", "buffer_"))]
    duo = [v for n, v in _disassemble(0).items() if "k_env_step_duo" in n]
    assert len(duo) == 1
    body = duo[0]
    prio = [i for i, ins in enumerate(body) if ins.startswith("s_setprio")]
    a = [i for i, ins in enumerate(body) if re.match(r"s_nop 13$", ins)]
    b = [i for i, ins in enumerate(body) if re.match(r"s_nop 14$", ins)]
    assert len(a) == 1 and len(b) == 1 and a[0] < b[0], (a, b)
    scr = [(i, ins) for i, ins in enumerate(body) if ins.startswith("scratch_")]
    in_loop = [(i, ins) for i, ins in scr if prio[0] <= i <= prio[-1]]
    for i, ins in in_loop:          # (none at all in the shipped build: the borrowed-lane path re-reads the lanes' candidate tables behind itself instead of keeping them alive)
        assert a[0] < i < b[0] and ins.startswith("scratch_load"), (i, ins, a, b)
    assert not [ins for i, ins in scr if ins.startswith("buffer_")]
    assert all(ins.startswith("scratch_load") or i < prio[0] for i, ins in scr)       # stores: prologue only


@pytest.mark.parametrize("family,what,spill_max", [
    (3, "ClsBiped one per wavefront, plain: 20 spilled VGPRs in the prologue / epilogue (DESIGN.md section 6)", 24),
    (6, "ClsLarge (dense dog3d, DM_TREE=0), plain: 4 (DESIGN.md section 6)", 8),
    (4, "ClsBiped AMP (odd batches of the task scenes; round 5: + the draw-tape lookups of the one-env drop-in, 11 -> 21, all in the rare draw / reset paths)", 24),
    (9, "ClsBipedObj (dribble_amp, one per wavefront)", 16),
    (24, "ClsBipedObj two per wavefront (round 6, dribble_amp's default): measured 30", 40),
    (18, "ClsBiped, DM-physics v2 (round 5: 32 -> 35 with the draw-tape lookups and the per-clip cycle boundary of the kinematic character, both in rare paths)", 40),
])
def test_secondary_kernels_stay_inside_their_measured_spill_budget(family, what, spill_max):
    r = _res(family)
    assert r["spill"] <= spill_max, (what, r)


@pytest.mark.parametrize("prec,real,scratch_max", [("f32", "f", 0), ("f64", "d", 272)])
def test_wave_probe_kernel_keeps_its_operands_in_registers(prec, real, scratch_max):
    """k_wave_probe (dm_wave_probe.h, in the object of the reset / query / probe family) measures the primitives as the step kernels use them only while its row files,
    Gram operands and accumulators stay in VGPRs: no spill in either precision, no scratch in float.  In double the 272 bytes are the `out[i]` of the fp64 Gram bodies' own
    `#pragma unroll 1` row loop (32 doubles and a pair), the primitive as it is written."""
    path = os.path.join(BUILD, "k_%s_11.o.res" % prec)
    if not os.path.exists(path):
        pytest.skip("no resource remarks (libdm_hip.so not built here)")
    blocks = re.split(r"remark: Function Name: ", open(path).read())
    mine = [b for b in blocks if b.startswith("_ZN3dmw12k_wave_probeI%sEE" % real)]
    assert len(mine) == 1, [b.split(" ")[0] for b in blocks[1:]]
    get = lambda pat: int(re.search(pat, mine[0]).group(1))
    assert get(r"VGPRs Spill: (\d+)") == 0 and get(r"SGPRs Spill: (\d+)") == 0
    assert get(r"ScratchSize \[bytes/lane\]: (\d+)") <= scratch_max and get(r"LDS Size \[bytes/block\]: (\d+)") == 0


def test_committed_counter_files_carry_the_kernel_source_stamp():
    """bench.py quotes HBM traffic and VALU figures from COMMITTED rocprofv3 counter files (PMC passes serialise the kernels, so they cannot be taken inside
    the timed run).  Each file carries the hash of the device sources it was taken on and the bench line says whether that is what it runs
    (`roofline.traffic_source_current`, `roofline.valu.source_current`): a kernel change can no longer keep quoting old counters silently (VERDICT r3,
    weak #5).  Here: the newest files are stamped; a stale stamp is a warning, not a failure (kernels change before they are re-profiled)."""
    import glob
    import json
    import os
    import sys
    import warnings
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    cur = bench.kernel_source_sha1()
    assert cur and len(cur) == 40
    newest = sorted(glob.glob(os.path.join(root, "profiles", "r*_traffic.json")))[-1]
    t = json.load(open(newest))
    assert "kernel_source_sha1" in t, newest
    tr, src = bench.measured_traffic("humanoid3d_walk", 4096, "k_env_step_duo")
    assert src == os.path.relpath(newest, root) and tr > 9.9e6
    if t["kernel_source_sha1"] != cur:
        warnings.warn("%s was taken on other device sources than the tree holds: re-run tools/gpu_round_profile.sh + tools/collect_profiles.py" % os.path.basename(newest))
    else:
        assert bench.measured_traffic.current is True
