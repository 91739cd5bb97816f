"""Every kernel family of libdm_hip.so against the oracle, with the family that ran reported by the library.

libdm_hip.so is one object per (precision, kernel family): the table of deepmimic_amd/csrc/dm_families.h, from which both Makefiles take their objects, each with
code generation flags of its own (NOLICM_IDS, SCHED_IDS) and all from one source: which loops a kernel runs is a property of its class and template
arguments (ClsBipedTree::PIPE = false: the tree loops without the LDS look-ahead; DuoSim::YFULL = false in the tap instantiation, family 2: the
y = L^-1 J^T loops with their per-dof tests), so the emulator library runs, per class and per kernel, the loops of the GPU objects.  dm_get_debug
"family" names the family of the last step launch (dm_host.cpp launch_step), so each row of FAMILIES below asserts that its configuration ran the
object it claims before it compares that object with the oracle.

* ledger (CPU): FAMILIES covers every step family of the table and of both Makefiles' objects, FAMILY11 every class of the reset / query / probe family;
* dispatch (CPU, emulator): each row's configuration reports its id, and so do the documented one-per-wavefront fallbacks;
* build rules (CPU): no compile rule of either Makefile passes a -D that could fork a template between objects, no header keeps an overridable knob;
* loop variants (CPU, emulator): the tree rows, the dense class and the two-per-wave tap family -- through both of its beyond-32-rows paths -- against the oracle;
* parity (GPU): each row x {f32, f64} on the HIP objects, sampled envs re-synchronised from the device before every control step.
"""
import os
import re
import subprocess
from dataclasses import dataclass, field

import numpy as np
import pytest

import parity_common as pc
from deepmimic_amd import core, model, streams
from deepmimic_amd.core import BatchEnv
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepmimic_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
DRIBBLE = "amp_dribble_zombie"


@dataclass(frozen=True)
class Row:
    """One step family: the configuration that selects it, the oracle check that holds it, its bounds.
    kind: "sampled" (parity_common.sampled_compare, stream A2 actions, auto-reset on), "goal" (parity_common.goal_rollout_compare: the dribble scene's
    ball and goal draws), "probe3" (the profiled control step of dm_probe 3, open loop, against sampled oracles).
    taps: the debug taps are armed (dm_probe 0) before the first step: the one-per-wavefront step then runs its tap instantiation."""
    asset: str
    n: int                      # envs of the GPU context: even on two-per-wavefront rows (both halves of every pair sampled), odd on one-per-wavefront rows
    kind: str = "sampled"
    pack: int = 0               # BatchEnv wave_packing
    physics: int = 1
    env: tuple = ()             # environment switches read by dm_create
    rot_fail: bool = False      # enable_root_rot_fail: selects the AMP instantiation on the plain imitate scene
    taps: bool = False
    f32_wc: tuple = ()          # f32, sampled rows: (|reward - fp64 oracle|, relative state difference) allowed on well-conditioned steps
    note: str = field(default="", compare=False)


HUM, DOG = "humanoid3d_walk", "dog3d_pace"
DENSE, BTREE = (("DM_TREE", "0"),), (("DM_TREE_BIPED", "1"),)
# f32_wc: twice the worst |reward - fp64 oracle| and relative state difference measured on MI355X over the sampled steps on which the oracle's own
# fp32 build stays within 1e-6 of its fp64 build (test_family_parity_gpu: all N envs, 8 control steps; measured reward / state: 0, 1: 2.95e-6 / 1.47e-3;
# 2: 4.61e-6 / 1.71e-3; 3, 4: 4.92e-6 / 1.17e-3; 5: 4.86e-6 / 1.17e-3; 6-8: 1.84e-6 / 1.59e-3; 12-14: 1.42e-5 / 1.26e-3; 15-17: 3.78e-6 / 2.09e-3;
# 18: 3.46e-6 / 1.23e-3; 19: 2.38e-5 / 2.58e-2; 20: 3.71e-6 / 1.71e-3; 21: 2.26e-6 / 1.31e-3; 22: 2.85e-6 / 2.04e-3).  Measured f64 worst case on
# every sampled row: reward 2.9e-8 (the float32 rounding of the output), relative state 5.5e-8.
FAMILIES = {
    0: Row(HUM, 10, f32_wc=(6.0e-06, 3.0e-03), note="two-per-wave plain"),
    1: Row(HUM, 10, rot_fail=True, f32_wc=(6.0e-06, 3.0e-03), note="two-per-wave AMP instantiation"),
    2: Row(HUM, 10, kind="probe3", f32_wc=(9.3e-06, 3.5e-03), note="two-per-wave taps (dm_probe 3): y loops with their per-dof tests"),
    3: Row(HUM, 9, f32_wc=(9.9e-06, 2.4e-03), note="ClsBiped plain: odd N falls back to one per wave"),
    4: Row(HUM, 9, rot_fail=True, f32_wc=(9.9e-06, 2.4e-03), note="ClsBiped AMP instantiation"),
    5: Row(HUM, 9, taps=True, f32_wc=(9.8e-06, 2.4e-03), note="ClsBiped taps"),
    6: Row(DOG, 9, env=DENSE, f32_wc=(3.7e-06, 3.2e-03), note="ClsLarge plain (dense dog)"),
    7: Row(DOG, 9, env=DENSE, rot_fail=True, f32_wc=(3.7e-06, 3.2e-03), note="ClsLarge AMP instantiation"),
    8: Row(DOG, 9, env=DENSE, taps=True, f32_wc=(3.7e-06, 3.2e-03), note="ClsLarge taps"),
    9: Row(DRIBBLE, 9, kind="goal", pack=1, note="ClsBipedObj one per wave"),
    10: Row(DRIBBLE, 9, kind="goal", pack=1, taps=True, note="ClsBipedObj taps"),
    12: Row(DOG, 9, f32_wc=(2.9e-05, 2.6e-03), note="ClsLargeTree plain"),
    13: Row(DOG, 9, rot_fail=True, f32_wc=(2.9e-05, 2.6e-03), note="ClsLargeTree AMP instantiation"),
    14: Row(DOG, 9, taps=True, f32_wc=(2.9e-05, 2.6e-03), note="ClsLargeTree taps"),
    15: Row(HUM, 9, env=BTREE, f32_wc=(7.6e-06, 4.2e-03), note="ClsBipedTree plain (tree loops without the look-ahead)"),
    16: Row(HUM, 9, env=BTREE, rot_fail=True, f32_wc=(7.6e-06, 4.2e-03), note="ClsBipedTree AMP instantiation (no look-ahead)"),
    17: Row(HUM, 9, env=BTREE, taps=True, f32_wc=(7.6e-06, 4.2e-03), note="ClsBipedTree taps (no look-ahead)"),
    18: Row(HUM, 9, physics=2, f32_wc=(7.0e-06, 2.5e-03), note="ClsBiped DM-physics v2"),
    19: Row(DOG, 9, env=DENSE, physics=2, f32_wc=(4.8e-05, 5.2e-02), note="ClsLarge DM-physics v2"),
    20: Row(DOG, 9, physics=2, f32_wc=(7.5e-06, 3.5e-03), note="ClsLargeTree DM-physics v2"),
    21: Row(HUM, 9, env=BTREE, physics=2, f32_wc=(4.6e-06, 2.7e-03), note="ClsBipedTree DM-physics v2 (no look-ahead)"),
    22: Row(HUM, 10, physics=2, f32_wc=(5.8e-06, 4.1e-03), note="two-per-wave DM-physics v2"),
    23: Row(DRIBBLE, 9, kind="goal", pack=1, physics=2, note="ClsBipedObj DM-physics v2"),
    24: Row(DRIBBLE, 10, kind="goal", pack=2, note="two-per-wave biped + free body"),
}
PRECISIONS = (32, 64)
# family 11: reset / query / probe of every class (dm_host.cpp LaunchTable) and the AMP expert, which every biped class shares with ClsBiped
FAMILY11 = {
    "ClsBiped": ("misc", "expert"), "ClsBipedObj": ("misc",), "ClsLarge": ("misc", "expert"), "ClsLargeTree": ("misc",), "ClsBipedTree": ("misc",),
}
# f64, every live sampled step (the bounds of the existing f64 parity tests); f32 ceilings of tests/test_parity_4096.py on the other steps
F64_REWARD, F64_STATE = 1e-6, 1e-5
F32_CEIL_REWARD, F32_ILL = 2e-2, 2e-5


# ---------------------------------------------------------------------------------------------------------------------------------- helpers
def _tables(row):
    t = model.load_asset(row.asset)
    if row.rot_fail:
        t.cfg.enable_root_rot_fail = True
    return t


def _env(row, prec, lib, monkeypatch, n=None, **kw):
    for k, v in row.env:
        monkeypatch.setenv(k, v)
    t = _tables(row)
    env = BatchEnv(t, row.n if n is None else n, precision=prec, lib_path=lib, wave_packing=row.pack, physics=row.physics, seed=3, **kw)
    return t, env


def _family(env):
    f = env.debug("family")
    assert (f == f[0]).all(), f
    return int(f[0])


def run_row(fid, prec, lib, monkeypatch, n=None, steps=8):
    """Run row `fid` against the oracle; asserts the reported family first.  Returns the measurements."""
    row = FAMILIES[fid]
    if row.kind == "goal":
        for k, v in row.env:
            monkeypatch.setenv(k, v)
        keep = []

        def on_env(e):
            keep.append(e)
            if row.taps:
                e.probe(0, pc.DT)
        w = pc.goal_rollout_compare(_tables(row), prec, lib, steps=steps, n=row.n if n is None else n, seed=5, wave_packing=row.pack,
                                    physics=row.physics, on_env=on_env)
        assert _family(keep[0]) == fid
        return dict(kind="goal", w=w)
    t, env = _env(row, prec, lib, monkeypatch, n=n)
    N = env.N
    o = Oracle(t)
    kt = streams.reset_phase(np.arange(N), o.duration)
    env.reset(kin_times=kt, max_times=np.inf)
    assert _family(env) == -1          # dm_create / dm_reset launch no step kernel
    if row.taps:
        env.probe(0, pc.DT)
    kw = dict(physics=row.physics, get_manifolds=env.get_manifolds, max_contacts=env.max_contacts) if row.physics == 2 else {}
    if row.kind == "probe3":
        def step():
            env.probe(3, pc.DT)        # one profiled control step: open loop, auto-reset, the tap instantiation of the two-per-wave kernel
            return env.query()         # (no env ends in this window: asserted below, so the query reads what the step left)
        res = pc.sampled_compare(env.get_state, step, t, np.arange(N), steps, conditioning=(prec == 32))
    else:
        orc = Oracle(t)
        acts = lambda k, st0: streams.stream_a2(pc.tracking_actions(t, st0["clocks"][:, 0], oracle=orc), np.arange(N), k)
        step = lambda a: env.step(a, pc.DT, 20, auto_reset=True)
        res = pc.sampled_compare(env.get_state, step, t, np.arange(N), steps, conditioning=(prec == 32), actions=acts, **kw)
    assert _family(env) == fid, (_family(env), fid)
    dr, ds, alive, ok, ends = res[:5]
    if row.kind == "probe3":
        assert ends == 0
    out = dict(kind="sampled", dr=dr, ds=ds, alive=alive, ok=ok, ends=ends)
    if prec == 32:
        out["d32"] = res[5]
    env.close()
    return out


def check_f64(fid, m):
    if m["kind"] == "goal":
        w = m["w"]
        assert w["flags_ok"] and w["reward"] < F64_REWARD and w["state"] < F64_STATE and w["ball"] < 1e-6, w
        return dict(reward=w["reward"], state=w["state"])
    dr, ds, alive = m["dr"], m["ds"], m["alive"]
    assert m["ok"], "terminate / valid / episode_end differ from the oracle"
    assert alive.mean() > 0.5
    live, sl = dr[alive], ds[alive & np.isfinite(ds)]
    assert live.max() < F64_REWARD and sl.max(initial=0.0) < F64_STATE, (live.max(), sl.max(initial=0.0))
    assert dr[~alive].max(initial=0.0) < 1e-6
    return dict(reward=float(live.max()), state=float(sl.max(initial=0.0)))


def check_f32(fid, m):
    row = FAMILIES[fid]
    if m["kind"] == "goal":
        # free-running rollouts: the bounds of tests/test_goal_scenes.py::test_dribble_scene_gpu / test_dribble_scene_physics_2_gpu
        w = m["w"]
        assert w["flags_ok"] and w["reward_mean"] < 2e-3 and w["ball"] < (2e-2 if row.physics == 1 else 5e-2), w
        return dict(reward=w["reward"], reward_mean=w["reward_mean"], state=w["state"])
    dr, ds, alive, d32 = m["dr"], m["ds"], m["alive"], m["d32"]
    assert m["ok"], "terminate / valid / episode_end differ from the oracle"
    assert alive.mean() > 0.5
    wc = alive & (d32 < 1e-6)          # steps single precision itself holds: the oracle's fp32 build within 1e-6 of its fp64 build
    ill = alive & ~wc
    assert wc.sum() >= alive.sum() // 2, (wc.sum(), alive.sum())
    worst, worst_s = float(dr[wc].max()), float(ds[wc & np.isfinite(ds)].max(initial=0.0))
    assert worst <= row.f32_wc[0], "family %d: well-conditioned f32 rewards %.3g from the fp64 oracle (bound %.3g)" % (fid, worst, row.f32_wc[0])
    assert worst_s <= row.f32_wc[1], "family %d: well-conditioned f32 states %.3g from the fp64 oracle (bound %.3g)" % (fid, worst_s, row.f32_wc[1])
    # the other steps: the ceilings of tests/test_parity_4096.py (beyond 1e-3 only where the oracle's own fp32 build misses its fp64 self by > 2e-5)
    assert dr[alive].max() < F32_CEIL_REWARD
    for k, j in np.argwhere(ill & (dr > 1e-3)):
        assert d32[k, j] > F32_ILL, (k, j, dr[k, j], d32[k, j])
    sl = ds[alive & np.isfinite(ds)]
    assert sl.mean() < 5e-3 and sl.max() < 0.3, (sl.mean(), sl.max())
    return dict(reward=worst, state=worst_s, ill=int(ill.sum()))


# ---------------------------------------------------------------------------------------------------------------------------------- ledger
def _makefile_var(path, name):
    txt = open(path).read()
    m = re.search(r"^%s\s*\??=\s*(.*)$" % name, txt, re.M)
    assert m, (path, name)
    return m.group(1).split()


def _table():
    """dm_families.h: ({step family id: (characters per wavefront, class, variant)}, id of the reset / query / probe family, its classes, the expert classes)"""
    src = open(os.path.join(CSRC, "dm_families.h")).read()
    rows = re.findall(r"^\s*F\((\d+),\s*([12]),\s*(\w+),\s*(SV_\w+)\)", src, re.M)
    step = {int(i): (int(pack), cls, v) for i, pack, cls, v in rows}
    assert len(step) == len(rows), "a family id has two rows"
    misc = int(re.search(r"^#define DM_MISC_FAMILY (\d+)", src, re.M).group(1))
    classes = {n: set(re.findall(r"\b%s\((\w+)\)" % x, re.search(r"^#define DM_%s_CLASSES\(%s\)(.*)$" % (n, x), src, re.M).group(1))) for n, x in (("MISC", "M"), ("EXPERT", "E"))}
    return step, misc, classes["MISC"], classes["EXPERT"]


TWO_PER_WAVE = tuple(sorted(i for i, (pack, _, _) in _table()[0].items() if pack == 2))


def _built_families(mk_dir):
    """the family ids a Makefile builds kernel objects for (dry run of a full build): {32: ids, 64: ids}"""
    out = subprocess.run(["make", "-C", mk_dir, "-n", "-B"], check=True, capture_output=True, text=True).stdout
    return {prec: {int(i) for i in re.findall(r"-o \S*/k_f%d_(\d+)\.o\b" % prec, out)} for prec in PRECISIONS}


def test_ledger_covers_every_family():
    """a family added to the table (dm_families.h) fails here until FAMILIES has a row (configuration, oracle check, bounds) for it"""
    step, misc_id, misc, expert = _table()
    kids = set(step) | {misc_id}
    for mk_dir in (CSRC, EMU):
        for prec, ids in _built_families(mk_dir).items():
            assert ids == kids, "%s builds f%d objects for %s, the table has %s" % (os.path.relpath(mk_dir, ROOT), prec, sorted(ids), sorted(kids))
    assert misc_id == 11 and misc_id not in step
    for prec in PRECISIONS:
        missing = sorted(set(step) - set(FAMILIES))
        assert not missing, "step families without a parity row (f%d): %s" % (prec, missing)
    assert set(FAMILIES) <= set(step), sorted(set(FAMILIES) - set(step))
    for fid, row in FAMILIES.items():
        assert row.kind in ("sampled", "goal", "probe3") and row.n >= 8
        assert row.n % 2 == (0 if fid in TWO_PER_WAVE else 1), "family %d: pairs need an even N, one-per-wave rows an odd one" % fid
        if row.kind != "goal":
            assert len(row.f32_wc) == 2 and 0 < row.f32_wc[0] <= 1e-4 and 0 < row.f32_wc[1] < 0.3, "family %d needs its measured f32 bounds" % fid
    assert misc == set(FAMILY11), sorted(misc ^ set(FAMILY11))
    assert expert == {c for c, what in FAMILY11.items() if "expert" in what}


def _recipe_lines(path):
    """the recipe lines (commands) of a Makefile, continuation lines joined"""
    txt = open(path).read().replace("\\\n", " ")
    return [l for l in txt.split("\n") if l.startswith("\t")]


def test_no_rule_defines_a_source_variant():
    """One template instantiation has one body in every object of the GPU library and of the emulator library: no compile rule of either Makefile passes
    a -D other than the translation unit's own (precision, family) and the emulator switch, nor a variable that could smuggle one in per family; no
    header under deepmimic_amd/csrc keeps an `#ifndef DM_X / #define DM_X` default for a -D to override (DM_HD, the host / device qualifier, apart)."""
    allowed = {"DM_EMU", "DM_TU_F64", "DM_TU_ID"}
    for mk in (os.path.join(CSRC, "Makefile"), os.path.join(EMU, "Makefile")):
        txt = open(mk).read()
        recipes = _recipe_lines(mk)
        assert any("dm_kernels.cpp" in l for l in recipes), mk
        # every variable and function a recipe expands is looked through too (HIPFLAGS, CXXFLAGS, licmflag, ...)
        names = set(re.findall(r"\$\((?:call )?(\w+)", "\n".join(recipes)))
        defs = [m.group(2) for m in re.finditer(r"^(\w+)\s*[?:+]?=(.*)$", txt, re.M) if m.group(1) in names]
        for text in recipes + defs:
            for d in re.findall(r"(?<![\w-])-D\s*(\w+)", text):
                assert d in allowed, "%s passes -D%s: make it a class property or a constant (dm_types.h)" % (os.path.relpath(mk, ROOT), d)
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".h", ".cpp")):
            continue
        src = open(os.path.join(CSRC, f)).read()
        knobs = [n for n in re.findall(r"^\s*#\s*ifndef\s+(DM_\w+)", src, re.M) if n != "DM_HD" and re.search(r"^\s*#\s*define\s+%s\b" % n, src, re.M)]
        assert not knobs, "%s keeps overridable knobs %s" % (f, knobs)
    for var in ("NOLICM_IDS", "SCHED_IDS"):
        ids = {int(i) for i in _makefile_var(os.path.join(CSRC, "Makefile"), var)}
        assert ids <= _built_families(CSRC)[32], var


# ---------------------------------------------------------------------------------------------------------------------------------- dispatch (CPU)
def _one_step(env):
    a = np.zeros((env.N, env.A), np.float32)
    env.step(a, pc.DT, 1)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("fid", sorted(FAMILIES))
def test_dispatch_reports_family(emu_lib, monkeypatch, fid, prec):
    row = FAMILIES[fid]
    n = 2 if row.n % 2 == 0 else 3
    t, env = _env(row, prec, emu_lib, monkeypatch, n=n)
    env.reset() if row.kind == "goal" else env.reset(kin_times=np.zeros(n), max_times=np.inf)
    assert _family(env) == -1
    if row.taps:
        env.probe(0, pc.DT)
    if row.kind == "probe3":
        env.probe(3, pc.DT)
    else:
        _one_step(env)
    assert _family(env) == fid, (_family(env), fid, row.note)
    env.close()


def _amp(name):
    t = model.load_asset(name)
    t.cfg.scene = "imitate_amp"
    return t


@pytest.mark.parametrize("case,want", [
    ("subset", 3), ("tape", 3), ("duo_off", 3), ("pack1", 3), ("taps_even", 5), ("probe3_pack1", 5), ("probe3_v2", 5),
    ("rotfail_subset", 4), ("rotfail_tape", 4), ("amp_even", 1), ("amp_odd", 4), ("amp_dog", 13), ("amp_dog_dense", 7),
    ("amp_tree_biped", 16), ("dribble_subset", 9), ("dribble_duo_obj_off", 9), ("dribble_v2_even", 23), ("probe3_dog", 14),
])
def test_dispatch_fallbacks(emu_lib, monkeypatch, case, want):
    """the documented one-per-wavefront fallbacks of the two-per-wave kernels, and the AMP scenes' instantiations"""
    t = model.load_asset(HUM)
    kw = {}
    if case.startswith("rotfail"):
        t.cfg.enable_root_rot_fail = True
    if case.startswith("amp"):
        t = _amp(DOG if "dog" in case else HUM)
    if case.startswith("dribble") or case == "probe3_dog":
        t = model.load_asset(DRIBBLE if case.startswith("dribble") else DOG)
    if case == "duo_off":
        monkeypatch.setenv("DM_DUO", "0")
    if case in ("amp_dog_dense",):
        monkeypatch.setenv("DM_TREE", "0")
    if case == "amp_tree_biped":
        monkeypatch.setenv("DM_TREE_BIPED", "1")
    if case == "dribble_duo_obj_off":
        monkeypatch.setenv("DM_DUO_OBJ", "0")
    if case in ("pack1", "probe3_pack1"):
        kw["wave_packing"] = 1
    if case.endswith("v2_even") or case == "probe3_v2":
        kw["physics"] = 2
    n = 3 if case in ("amp_odd", "amp_tree_biped") else 4      # (ClsBipedTree: even batches of default packing stay two per wavefront, dm_host.cpp setup)
    env = BatchEnv(t, n, precision=64, lib_path=emu_lib, seed=3, **kw)
    env.reset() if case.startswith("dribble") else env.reset(kin_times=np.zeros(n), max_times=np.inf)
    a = np.zeros((n, env.A), np.float32)
    if case.endswith("subset"):
        env.step_envs([0, 1], a[:2], pc.DT, 1)
    elif case.endswith("tape"):
        env.set_draw_tape(np.zeros((n, core.TAPE_STRIDE)))
        env.step(a, pc.DT, 1)
    elif case.startswith("probe3"):
        env.probe(3, pc.DT)
    elif case == "taps_even":
        env.probe(0, pc.DT)
        env.step(a, pc.DT, 1)
    else:
        env.step(a, pc.DT, 1)
    assert _family(env) == want, (case, _family(env))
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------- loop variants (CPU)
def _emu_row(fid, lib, monkeypatch, steps=3):
    row = FAMILIES[fid]
    m = run_row(fid, 64, lib, monkeypatch, n=(2 if row.n % 2 == 0 else 3), steps=steps)
    return check_f64(fid, m)


@pytest.mark.parametrize("fid", [6, 7, 8, 19])
def test_dense_large_class_emulator(emu_lib, monkeypatch, fid):
    """ClsLarge (DM_TREE=0): the dense class of any character up to 23 links / 64 dof that is not a compiled topology"""
    _emu_row(fid, emu_lib, monkeypatch)
    if FAMILIES[fid].taps:
        monkeypatch.setenv("DM_TREE", "0")
        pc.check_dynamics(DOG, 64, emu_lib, rtol=1e-11)
        pc.check_spd(DOG, 64, emu_lib, rtol=1e-9)


@pytest.mark.parametrize("fid", [15, 16, 17, 21, 12, 13, 14, 20])
def test_tree_rows_on_their_own_loops(emu_lib, monkeypatch, fid):
    """the tree classes, each on the loops its GPU objects run: ClsBipedTree (15, 16, 17, 21) without the LDS look-ahead, ClsLargeTree (12, 13, 14, 20)
    with it.  (The two other combinations -- the dog without the look-ahead, the humanoid with it -- are in no library any more.)"""
    _emu_row(fid, emu_lib, monkeypatch)
    if fid == 17:
        monkeypatch.setenv("DM_TREE_BIPED", "1")
        pc.check_dynamics(HUM, 64, emu_lib, rtol=1e-11)
        pc.check_substep(HUM, 64, emu_lib, tol_vel=1e-8, tol_pose=1e-10, lift=-0.03)


def test_duo_tap_family_on_its_own_loops(emu_lib, monkeypatch):
    """family 2, the tap instantiation of the two-per-wave kernel (DuoSim::YFULL = false: y loops with their per-dof tests): the profiled control step, and the
    heavy-contact rollout stepped by dm_probe 3 + query() -- the only route to that instantiation -- through the borrowed-lane path and the 64-lane fallback.
    The A2 rollout runs family 0 on family 0's own loops.
    dm_probe 3 steps with auto_reset and end_early on, the oracles mirror the resets (parity_common.batch_rollout_compare).  Under it the lifts -0.08 / -0.3 end the
    lifted characters' episodes inside the first control step (a fall contact): both paths run, but what is compared of those two envs in that step is the
    first observation of their next episode.  So a second set, found on the emulator: -0.07 on envs 0, 1 and 3 puts pair 0 (two heavy characters, more than 64
    rows together) on the 64-lane fallback and pair 1 (env 3 beyond 32 rows beside a light partner) on borrowed lanes in the first control step, and no episode ends:
    all four envs are compared with their oracles through and after those substeps."""
    _emu_row(2, emu_lib, monkeypatch)
    dr, ds, ok, _ = pc.action_rollout_compare(HUM, 64, emu_lib, 2, "A2", [0.0, 0.37], wave_packing=2)
    assert ok and dr.max() < 1e-6 and ds.max() < 1e-5, (dr, ds)
    for lifts, live in (([-0.08, 0.0, 0.0, -0.3], False), ([-0.07, -0.07, 0.0, -0.07], True)):
        fam, st = [], {}

        def probe3(env):
            env.probe(3, pc.DT)
            fam.append(_family(env))
            return env.query()
        dr, ds, ok = pc.batch_rollout_compare(HUM, 64, emu_lib, steps=2, t0s=[0.0, 0.4, 0.2, 0.6], wave_packing=2, lifts=lifts, stats=st, step=probe3)
        first = st["steps"][0]
        print("lifts %s: per step borrowed %s fallback %s resets %s, reward diff %s state diff %s" % (
            lifts, [x["borrowed"].tolist() for x in st["steps"]], [x["fallback"].tolist() for x in st["steps"]], [x["reset"].tolist() for x in st["steps"]], dr, ds))
        assert fam == [2, 2], fam
        assert first["borrowed"].max() > 0 and first["fallback"].max() > 0, st["steps"]         # both beyond-32-rows paths, on these loops
        if live:
            assert not any(x["reset"].any() for x in st["steps"]), st["steps"]
            assert (first["fallback"][:2] > 0).all() and (first["borrowed"][2:] > 0).all(), st["steps"]
        assert ok and dr.max() < 1e-6 and ds.max() < 1e-4, (dr, ds)       # (heavy contact: the pairs through the borrowed-lane path and the 64-lane fallback)


# ---------------------------------------------------------------------------------------------------------------------------------- parity (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("fid", sorted(FAMILIES))
def test_family_parity_gpu(hip_lib, monkeypatch, fid, prec):
    m = run_row(fid, prec, hip_lib, monkeypatch)
    got = check_f64(fid, m) if prec == 64 else check_f32(fid, m)
    print("FAMILY %2d f%d reported %2d %s" % (fid, prec, fid, " ".join("%s=%.3g" % kv for kv in got.items())))
    row = FAMILIES[fid]
    if row.taps and row.kind == "sampled":
        # the tap family's class through the component probes (reset / query / probe family 11): bounds of tests/test_parity_gpu.py
        for k, v in row.env:
            monkeypatch.setenv(k, v)
        pc.check_dynamics(row.asset, prec, hip_lib, rtol=1e-11 if prec == 64 else 5e-5)
        pc.check_spd(row.asset, prec, hip_lib, rtol=1e-9 if prec == 64 else 5e-3)
