"""The contact step against its impulse-momentum identity (tests/impulse_identity.py): oracle, emulator and MI355X on the same cases.

Parity tests hold the kernels to the oracle, but the oracle's substep was written from the same reading of Bullet: a wrong lever
arm, sign or friction direction would sit in both.  The identity needs neither: its reference side is H, C and numerical link
Jacobians of code pinned to the reference sources, plus the contact points.  Being a residual it holds the float32 heavy-contact
paths (borrowed lanes, 64-lane fallback, overflow rows) to a few units of roundoff where a state comparison has to be loose.

Routes
* tap: one character per wave, k_env_probe: set_state, set_tau, probe(1, h), then the vstar / lambda / rows taps and get_state.
  Full residual, null-space residual, (**), and the exact box inequalities on lambda.
* production: the step kernel of the requested packing without taps, tables with num_sim_substeps = 1 so that update(h, 1) is one
  substep of length h; tau is read back.  N^T [H (v' - v) - h (tau - C)] = 0, the lambda-free form.  wave_packing = 1 is the control.

Cases (CASES): states are rows of parity_common.random_states(seed, vel_scale) lifted per env; seeds, rows and lifts were searched
on the float64 oracle so that the conditions of `build_case` hold (clamp inactive below 0.9 of its value, codimension >= 6, the
contents each case names); a case that stops meeting them is re-seeded, never relaxed.

Bounds: impulse_identity.bound(D, precision) = 8 D u, derived in that module.  float32 additionally: the worst ratio of a case on
the device at most MARGIN32 = 8 times the worst ratio of the same case on the oracle's own float32 build, computed live.

Sharpness (test_sharpness_*): corruptions of the reference side -- a contact point moved by 1 cm, the sign of body b of a self
contact flipped, t1 and t2 of one contact exchanged -- push the full residual from 1e-16 beyond 1e-6.  In the null-space form the
moved point and the flipped sign are caught (the perturbed columns leave the span); exchanging t1 and t2 permutes two columns of B
and leaves its range, hence N, unchanged: that corruption is visible to the full form only, which is why the tap route asserts both.
"""
from dataclasses import dataclass

import numpy as np
import pytest

import impulse_identity as ii
import parity_common as pc
from deepmimic_amd import model
from deepmimic_amd.core import BatchEnv
from oracle_lib import Oracle

HUM, DOG, DRIBBLE = "humanoid3d_walk", "dog3d_pace", "amp_dribble_zombie"
H_STEP = 1.0 / 1200
MARGIN32 = 8.0
BALL_SEED = 7
TWO_PER_WAVE = (0, 1, 2, 22, 24)          # dm_families.h rows with two characters per wavefront (tests/test_kernel_families.py derives the same set)


@dataclass(frozen=True)
class Case:
    asset: str
    picks: tuple                 # per env (seed, row of random_states(n = 4, seed), lift)
    vel_scale: float = 0.3
    tau_scale: float = 20.0
    balls: tuple = ()            # dribble scene, per env: ("ground",) | ("link", link, direction, ball velocity)
    duo: str = ""                # what the two-per-wave route must report: "" | "borrowed" | "fallback"
    min_rows: int = 0            # every env named in `heavy` has more rows than this
    heavy: tuple = ()
    need_self: bool = False      # at least one env with a self contact


CASES = {
    # lift +2 m: no ground contact; envs 1 and 2 carry self contacts, all four the limit rows
    "airborne": Case(HUM, ((3, 0, 2.0), (3, 1, 2.0), (3, 2, 2.0), (3, 3, 2.0)), need_self=True),
    # lift 0: one or two feet on the ground, env 2 a self contact as well
    "light": Case(HUM, ((0, 0, 0.0), (0, 1, 0.0), (0, 2, 0.0), (0, 3, 0.0)), need_self=True),
    # a character beyond 32 rows (within 48) beside a light partner (pair within 64): heavy in the lower half of pair 0 and in the upper half of pair 1
    "borrowed": Case(HUM, ((11, 1, -0.08), (3, 0, 0.0), (3, 3, 0.0), (11, 0, -0.12)), duo="borrowed", min_rows=32, heavy=(0, 3)),
    # both pairs beyond 64 rows together: the 64-lane fallback
    "fallback": Case(HUM, ((11, 1, -0.08), (4, 0, -0.12), (11, 2, -0.05), (14, 2, -0.12)), duo="fallback", min_rows=32, heavy=(0, 1, 2, 3)),
    # the dog pressed 2-3 cm into the ground: more than 32 rows on the one-per-wave kernel (rows beyond its register file in the overflow block); its smallest
    # link inertias are 1.5e-4 kg m^2, so the torques stay small enough for v* to keep away from the clamp
    "dog_press": Case(DOG, ((8, 2, -0.03), (14, 1, -0.02), (19, 0, -0.03), (19, 0, 0.0)), vel_scale=0.1, tau_scale=0.2, min_rows=32, heavy=(0, 1, 2)),
    # biped + ball (the system is H extended by the sphere's mass block): the ball rolling on the ground away from the character; against the right shin;
    # against the right foot; kicked at the chest of an airborne character
    "ball": Case(DRIBBLE, ((BALL_SEED, 0, 0.0), (BALL_SEED, 1, 0.0), (BALL_SEED, 2, 0.0), (BALL_SEED, 3, 2.0)),
                 balls=(("ground",), ("link", 4, (1.0, 0.0, 0.2), (-1.0, 0.0, 0.0)), ("link", 5, (1.0, 1.0, 0.0), (-2.0, 0.0, 0.0)), ("link", 1, (1.0, 0.0, 0.0), (-4.0, 0.5, 0.0)))),
}
GPU_PRECISIONS = (64, 32)

_CACHE = {}


def _tables(asset, one_substep=False):
    t = model.load_asset(asset)
    if one_substep:
        t.cfg.num_sim_substeps = 1
    return t


def _place_ball(o, t, q, v, link, u, pen=0.003):
    """the ball centre on the ray com(link) + s u at which the ball penetrates the link's capsule model by ~pen: s walks in from 0.8 m in 1 mm steps until the
    oracle lists a (link, ball) contact, then goes `pen` plus that contact's distance further"""
    u = np.asarray(u, dtype=np.float64); u = u / np.linalg.norm(u)
    o.set_sim_state(q, v)
    com = o.links()[link, 0:3].copy()
    b = np.zeros(13); b[3] = 1.0
    for s in np.arange(0.8, 0.0, -0.001):
        b[0:3] = com + s * u
        o.set_sim_state(q, v); o.set_ball(b); o.set_tau(np.zeros(o.P)); o.substep(H_STEP)
        cl = o.contact_list_ex()
        hit = cl[(cl[:, 9] == 1) & (cl[:, 0] == link)] if len(cl) else cl
        if len(hit):
            return com + (s - pen - float(hit[0, 2])) * u
    raise AssertionError("the ball never touches link %d" % link)


def build_case(name):
    """states, torques, the float64 oracle's step and the reference side per env; asserts the conditions the case was searched for"""
    if name in _CACHE:
        return _CACHE[name]
    c = CASES[name]
    t = _tables(c.asset)
    o = Oracle(t)
    idx = pc.dof_index(t)
    Q, V, TAU, BALL = [], [], [], []
    for e, (seed, row, lift) in enumerate(c.picks):
        P, Vs, _ = pc.random_states(t, o, 4, seed=seed, vel_scale=c.vel_scale)
        q = P[row].copy(); q[1] += lift
        tau = c.tau_scale * np.random.default_rng(seed + 1000).normal(size=(4, len(idx)))[row]; tau[:6] = 0
        Q.append(q); V.append(Vs[row]); TAU.append(tau)
        if c.balls:
            spec = c.balls[e]
            b = np.zeros(13); b[3] = 1.0
            if spec[0] == "ground":          # resting on the ground 3 m from the character, rolling slowly
                b[0:3] = [q[0] + 3.0, ii.cfg_of(o, "ball_radius") - 0.001, q[2]]; b[7:13] = [0.3, 0.0, 0.1, 0.0, 0.5, 0.0]
            else:
                b[0:3] = _place_ball(o, t, q, Vs[row], spec[1], spec[2]); b[7:10] = spec[3]; b[10:13] = [0.0, 0.0, 2.0]
            BALL.append(b)
    refs = [ii.reference_step(o, t, Q[e], V[e], TAU[e], H_STEP, BALL[e] if c.balls else None) for e in range(len(Q))]
    case = dict(name=name, cfg=c, t=t, idx=idx, Q=np.array(Q), V=np.array(V), TAU=np.array(TAU), BALL=np.array(BALL) if c.balls else None, refs=refs, D=len(idx))
    check_conditions(case, refs)
    _CACHE[name] = case
    return case


def check_conditions(case, refs):
    """not measurements: what makes the identity applicable and the case what it claims to be (float64 oracle)"""
    c = case["cfg"]
    for e, r in enumerate(refs):
        m = max(np.abs(r["vstar"] / r["clamp"]).max(), np.abs(r["v1"] / r["clamp"]).max())
        assert m < 0.9, "%s env %d: a coordinate velocity at %.2f of its clamp: re-seed" % (case["name"], e, m)
        N, rank = ii.nullspace(r["B"])
        assert N.shape[1] >= 6, "%s env %d: codimension %d" % (case["name"], e, N.shape[1])
        assert r["rows"] == r["B"].shape[1] == r["meta"]["n_lim"] + 3 * r["ncontacts"]
    assert len(c.heavy) >= (2 if c.duo else 0)
    for e in c.heavy:
        assert refs[e]["rows"] > c.min_rows, (case["name"], e, refs[e]["rows"])
    if c.need_self:
        assert any(r["nself"] > 0 for r in refs)
    if c.balls:
        for r, spec in zip(refs, c.balls):
            kinds = r["contacts"][:, 9].astype(int).tolist()
            assert (2 in kinds) if spec[0] == "ground" else any(k == 1 and int(l) == spec[1] for k, l in zip(kinds, r["contacts"][:, 0])), (case["name"], spec, kinds)
    if c.duo == "borrowed":
        for e in c.heavy:
            assert 32 < refs[e]["rows"] <= 48 and refs[e]["rows"] + refs[e ^ 1]["rows"] <= 64 and refs[e ^ 1]["rows"] <= 32
    if c.duo == "fallback":
        for e in c.heavy:
            assert refs[e]["rows"] > 48 or refs[e]["rows"] + refs[e ^ 1]["rows"] > 64


# ---------------------------------------------------------------------------------------------------------------- routes
def run_oracle(case, variant):
    """the case on the oracle build `variant`: per env v*, v', lambda, rows, contacts, the ball's v'"""
    o = Oracle(case["t"], variant=variant)
    idx, out = case["idx"], []
    for e in range(len(case["Q"])):
        o.set_sim_state(case["Q"][e], case["V"][e])
        if case["BALL"] is not None:
            o.set_ball(case["BALL"][e])
        tp = np.zeros(o.P); tp[idx] = case["TAU"][e]; o.set_tau(tp)
        o.substep(H_STEP)
        out.append(dict(vstar=o.vstar()[idx], v1=o.sim_state()[1][idx], lam=o.lambdas(), rows=o.num_rows(), nc=o.num_contacts(),
                        ball_v1=o.ball_state()[7:13].copy() if case["BALL"] is not None else None))
    return out


def run_tap(case, lib, prec):
    n = len(case["Q"])
    env = BatchEnv(case["t"], n, precision=prec, lib_path=lib, wave_packing=1)
    env.set_state(pose=case["Q"], vel=case["V"])
    if case["BALL"] is not None:
        env.set_obj_state(case["BALL"])
    env.set_tau(case["TAU"])
    env.probe(1, H_STEP)
    vstar, lam, rows, st = env.debug("vstar"), env.debug("lambda"), env.debug("rows"), env.get_state()
    ob = env.get_obj_state() if case["BALL"] is not None else None
    env.close()
    return [dict(vstar=vstar[e], v1=st["vel"][e][case["idx"]], lam=lam[e][:int(rows[e][0])], rows=int(rows[e][0]), nc=int(rows[e][1]),
                 ball_v1=None if ob is None else ob[e][7:13]) for e in range(n)]


def run_production(case, lib, prec, pack):
    """one update(h, 1) of the step kernel without taps (tables with one substep per update); returns per env v', the tau the kernel applied, the ball's v',
    and the family / borrowed / fallback counters"""
    n = len(case["Q"])
    t1 = _tables(case["cfg"].asset, one_substep=True)
    env = BatchEnv(t1, n, precision=prec, lib_path=lib, wave_packing=pack)
    st0 = env.get_state()
    env.set_state(pose=case["Q"], vel=case["V"], tar=case["Q"], kin=st0["kin"], clocks=st0["clocks"])      # (kin / clocks: zeroes the path counters)
    if case["BALL"] is not None:
        env.set_obj_state(case["BALL"])
    env.update(H_STEP, 1)
    tau, st = env.debug("tau"), env.get_state()
    fam, bor, fb = env.debug("family"), env.debug("borrowed"), env.debug("fallback")
    ob = env.get_obj_state() if case["BALL"] is not None else None
    env.close()
    outs = [dict(v1=st["vel"][e][case["idx"]], tau=tau[e], ball_v1=None if ob is None else ob[e][7:13]) for e in range(n)]
    return outs, dict(family=int(fam[0]), borrowed=bor, fallback=fb)


# ---------------------------------------------------------------------------------------------------------------- evaluation
def tap_worst(case, outs, precision, counts=True):
    """worst ratio of each kind over the envs of a case; asserts row / contact counts against the float64 oracle and the lambda boxes"""
    worst = dict(full=0.0, null=0.0, vstar=0.0)
    for e, (r, o) in enumerate(zip(case["refs"], outs)):
        if counts:
            assert (o["rows"], o["nc"]) == (r["rows"], r["ncontacts"]), (case["name"], e, o["rows"], o["nc"], r["rows"], r["ncontacts"])
        got = ii.ratios(r, o["vstar"], o["v1"], o["lam"], o["ball_v1"])
        for k in worst:
            worst[k] = max(worst[k], got[k])
        bad = ii.lambda_box_violations(r, o["lam"], precision)
        assert not bad, (case["name"], e, bad)
    return worst


def production_refs(case, outs):
    """the reference side at the torque the kernel applied (float64 oracle); the conditions are asserted again for that torque"""
    o = Oracle(case["t"])
    refs = []
    for e, x in enumerate(outs):
        assert np.all(x["tau"][:6] == 0), "root torque"
        refs.append(ii.reference_step(o, case["t"], case["Q"][e], case["V"][e], x["tau"], H_STEP, None if case["BALL"] is None else case["BALL"][e]))
    check_conditions(case, refs)
    return refs


def step_ratio(r, v1, ball_v1=None):
    ball = None if r["ball_pos"] is None else (np.diag(r["He"])[-6:], ball_v1, r["ball_vstar"])
    return ii.residual_step_nullspace(r["H"], r["C"], r["v"], v1, r["tau"], r["h"], r["B"], ball)[1]


def production_worst(case, outs, precision):
    refs = production_refs(case, outs)
    worst = max(step_ratio(r, x["v1"], x["ball_v1"]) for r, x in zip(refs, outs))
    worst32 = None
    if precision == 32:      # the same step on the oracle's own float32 build, under the torque the kernel applied
        o32 = Oracle(case["t"], variant="f32"); idx = case["idx"]; worst32 = 0.0
        for e, (r, x) in enumerate(zip(refs, outs)):
            o32.set_sim_state(case["Q"][e], case["V"][e])
            if case["BALL"] is not None:
                o32.set_ball(case["BALL"][e])
            tp = np.zeros(o32.P); tp[idx] = x["tau"]; o32.set_tau(tp); o32.substep(H_STEP)
            assert (o32.num_rows(), o32.num_contacts()) == (r["rows"], r["ncontacts"])
            worst32 = max(worst32, step_ratio(r, o32.sim_state()[1][idx], o32.ball_state()[7:13] if case["BALL"] is not None else None))
    return worst, worst32


def check_tap(case, outs, precision, label):
    w = tap_worst(case, outs, precision)
    bnd = ii.bound(case["D"], precision)
    line = "IDENTITY %-10s %-22s f%d tap: full %.2e null %.2e vstar %.2e (bound %.2e)" % (case["name"], label, precision, w["full"], w["null"], w["vstar"], bnd)
    if precision == 32:
        w32 = tap_worst(case, run_oracle(case, "f32"), 32)
        line += " | oracle f32: full %.2e null %.2e vstar %.2e" % (w32["full"], w32["null"], w32["vstar"])
    print(line)
    if case["name"] == "airborne":          # nothing external touches the character: total linear and angular momentum, by name
        for e, (r, o) in enumerate(zip(case["refs"], outs)):
            for nm, (val, scale) in ii.root_momentum_rows(r["H"], o["v1"], o["vstar"]).items():
                assert abs(val) <= bnd * scale, "%s env %d: %s changed by %.3e (scale %.3e)" % (label, e, nm, val, scale)
    for k in ("full", "null", "vstar"):
        assert w[k] <= bnd, (case["name"], label, k, w[k], bnd)
        if precision == 32 and label != "oracle":
            assert w[k] <= MARGIN32 * w32[k], "%s %s: %s ratio %.3e beyond %g x the oracle's float32 build (%.3e)" % (case["name"], label, k, w[k], MARGIN32, w32[k])
    return w


def check_production(case, lib, precision, pack, label):
    outs, info = run_production(case, lib, precision, pack)
    w, w32 = production_worst(case, outs, precision)
    bnd = ii.bound(case["D"], precision)
    print("IDENTITY %-10s %-22s f%d pack %d family %d borrowed %s fallback %s: step null %.2e (bound %.2e)%s" % (
        case["name"], label, precision, pack, info["family"], info["borrowed"].astype(int).tolist(), info["fallback"].astype(int).tolist(), w, bnd,
        "" if w32 is None else " | oracle f32: %.2e" % w32))
    if pack == 2:
        assert info["family"] in TWO_PER_WAVE, info
        duo = case["cfg"].duo
        if duo == "borrowed":
            assert (info["borrowed"] > 0).all() and (info["fallback"] == 0).all(), info
        elif duo == "fallback":
            assert (info["fallback"] > 0).all(), info
        else:
            assert (info["borrowed"] == 0).all() and (info["fallback"] == 0).all(), info
    else:
        assert info["family"] not in TWO_PER_WAVE, info
    assert w <= bnd, (case["name"], label, w, bnd)
    if precision == 32:
        assert w <= MARGIN32 * w32, "%s %s: step ratio %.3e beyond %g x the oracle's float32 build (%.3e)" % (case["name"], label, w, MARGIN32, w32)


# ---------------------------------------------------------------------------------------------------------------- CPU: helper, oracle
def _sharp_ref():
    """an env of the light case with a self contact and ground contacts, active impulses on both"""
    case = build_case("light")
    r = next(r for r in case["refs"] if r["nself"] > 0 and r["ncontacts"] > r["nself"])
    assert np.abs(r["lam"]).max() > 0
    return case, r


def _corrupted(case, r, corrupt):
    o = Oracle(case["t"])
    B, _ = ii.constraint_span(case["t"], r["LJ"], r["coms"], r["q"], r["contacts"], ii.cfg_of(o, "friction"), corrupt=corrupt)
    full = ii.residual_full(r["H"], r["v1"], r["vstar"], B, r["lam"])[1]
    null = ii.residual_nullspace(r["H"], r["v1"], r["vstar"], B)[1]
    return full, null


def test_sharpness_of_the_reference_side(oracle_built):
    case, r = _sharp_ref()
    clean_f, clean_n = _corrupted(case, r, None)
    assert clean_f < 1e-15 and clean_n < 1e-15, (clean_f, clean_n)
    lam, meta = r["lam"], r["meta"]
    nl, nc = meta["n_lim"], meta["nc"]
    ground = next(c for c in range(nc) if r["contacts"][c][1] < 0 and lam[nl + c] > 0)
    selfc = next(c for c in range(nc) if r["contacts"][c][1] >= 0 and lam[nl + c] > 0)
    # the friction pair of `ground` must be active and unequal for the exchange to matter
    assert abs(lam[nl + nc + 2 * ground] - lam[nl + nc + 2 * ground + 1]) > 1e-6 * abs(lam).max()
    res = {}
    res["point"] = _corrupted(case, r, ("point", ground, np.array([0.01, 0.0, 0.0])))
    res["flip_b"] = _corrupted(case, r, ("flip_b", selfc))
    res["swap"] = _corrupted(case, r, ("swap", ground))
    print("SHARPNESS clean full %.1e null %.1e; " % (clean_f, clean_n) + "; ".join("%s full %.1e null %.1e" % (k, f, n) for k, (f, n) in res.items()))
    for k, (f, n) in res.items():
        assert f > 1e-6, (k, f)
    # null-space form: the moved point and the flipped sign leave the span; exchanging t1 and t2 permutes columns and does not
    assert res["point"][1] > 1e-6 and res["flip_b"][1] > 1e-6, res
    assert res["swap"][1] < 1e-15, res


def test_sharpness_of_the_implementation_side(oracle_built):
    """an implementation whose impulses or velocities are off in the ninth digit misses the float64 bound: one impulse scaled by 1 + 1e-9 (full form), the
    new velocity scaled by 1 + 1e-9 (all three forms that read it), v* scaled by 1 + 1e-9 ((**))"""
    case, r = _sharp_ref()
    bnd = ii.bound(case["D"], 64)
    lam = r["lam"].copy(); lam[np.argmax(np.abs(lam))] *= 1 + 1e-9
    bad_lam = ii.ratios(r, r["vstar"], r["v1"], lam)
    bad_v1 = ii.ratios(r, r["vstar"], r["v1"] * (1 + 1e-9), r["lam"])
    bad_vs = ii.ratios(r, r["vstar"] * (1 + 1e-9), r["v1"], r["lam"])
    step = ii.residual_step_nullspace(r["H"], r["C"], r["v"], r["v1"] * (1 + 1e-9), r["tau"], r["h"], r["B"])[1]
    print("SHARPNESS implementation side (bound %.1e): lambda full %.1e; v' full %.1e null %.1e step %.1e; v* vstar %.1e" % (
        bnd, bad_lam["full"], bad_v1["full"], bad_v1["null"], step, bad_vs["vstar"]))
    assert bad_lam["full"] > bnd and bad_v1["full"] > bnd and bad_v1["null"] > bnd and step > bnd and bad_vs["vstar"] > bnd


@pytest.mark.parametrize("name", sorted(CASES))
def test_identity_oracle(oracle_built, name):
    """the float64 oracle (the identity holds for the restated physics at these states), then its float32 build against the hard bound"""
    case = build_case(name)
    outs = [dict(vstar=r["vstar"], v1=r["v1"], lam=r["lam"], rows=r["rows"], nc=r["ncontacts"], ball_v1=r.get("ball_v1")) for r in case["refs"]]
    check_tap(case, outs, 64, "oracle")
    check_tap(case, run_oracle(case, "f32"), 32, "oracle")


def test_airborne_momentum_by_name(oracle_built):
    """no external impulse on an airborne character: the six root rows of (*) are the change of total linear and angular momentum by the internal (self
    contact, joint limit) impulses, each zero to roundoff"""
    case = build_case("airborne")
    assert all(r["ncontacts"] == r["nself"] for r in case["refs"]) and any(np.abs(r["lam"]).max() > 0 for r in case["refs"])
    for e, r in enumerate(case["refs"]):
        for nm, (val, scale) in ii.root_momentum_rows(r["H"], r["v1"], r["vstar"]).items():
            assert abs(val) <= ii.bound(case["D"], 64) * scale, "env %d: %s changed by %.3e (scale %.3e)" % (e, nm, val, scale)


# ---------------------------------------------------------------------------------------------------------------- emulator (CPU)
@pytest.mark.parametrize("prec", (64, 32))
@pytest.mark.parametrize("name", sorted(CASES))
def test_identity_tap_emulator(emu_lib, name, prec):
    case = build_case(name)
    check_tap(case, run_tap(case, emu_lib, prec), prec, "emulator")


# (the dog has no two-per-wave kernel: its case runs one per wave only)
PRODUCTION = [(name, prec, pack) for name in sorted(CASES) for prec in (64, 32) for pack in (2, 1) if not (CASES[name].asset == DOG and pack == 2)]


@pytest.mark.parametrize("name,prec,pack", PRODUCTION)
def test_identity_production_emulator(emu_lib, name, prec, pack):
    case = build_case(name)
    check_production(case, emu_lib, prec, pack, "emulator")


# ---------------------------------------------------------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("prec", GPU_PRECISIONS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_identity_tap_gpu(hip_lib, name, prec):
    case = build_case(name)
    check_tap(case, run_tap(case, hip_lib, prec), prec, "MI355X")


@pytest.mark.gpu
@pytest.mark.parametrize("name,prec,pack", PRODUCTION)
def test_identity_production_gpu(hip_lib, name, prec, pack):
    case = build_case(name)
    check_production(case, hip_lib, prec, pack, "MI355X")
