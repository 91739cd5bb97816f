"""Contact generation against exact geometry (tests/contact_geometry.py), on every step route.

Every other check of the rigid-body step compares one restatement of the collision code with another (kernel == oracle, line for line) or takes its
contact points from the oracle's own list (tests/test_step_identity.py).  Here the contact LIST -- which pairs, in which slots, at what distance, along
which normal, at a pair of points that really are closest points -- is compared with an independent float64 reference that shares only the definitions
of DESIGN.md section 4, at the smallest states at which the routine can go wrong.  The states are built or were searched ON THE REFERENCE and every
property a case is named for is asserted on the reference (`CONDITIONS`), never on the code under test.

Routes (one substep from the set state; the reference is fed `Oracle.links()` of the float64 oracle at that state):
* the float64 oracle and its float32 build (`contact_list_ex`);
* tap route, one character per wavefront: `dm_probe 1`, taps "contacts" + "rows" (BatchEnv.contacts); the same under DM-physics v2, where the
  ground contacts of the first substep are one support point per link (contact_geometry.contacts(manifold_first=True));
* tap route, two per wavefront: `dm_probe 5` (one update of the tap instantiation of the two-per-wave kernel, family 2 asserted), DuoSim's own copy
  of the ground-candidate loop and its double-buffered pair loop;
* production (no taps; one `dm_update` of tables with one substep per update): the contact bit mask of flags[:, 1], both packings, the plain, AMP
  and v2 instantiations; under v2 `dm_get_manifolds` after each of 6 updates.

What is asserted per slot: count, (link a, link b, kind) and order exactly; `dist` to the tolerance; for a ground slot x to the tolerance and
n == (0, 1, 0) exactly; for a pair x is NOT compared with a point: ca = x + (r_a + dist / 2) n and cb = x - (r_b + dist / 2) n are recovered and each must
lie on its segment, | |ca - cb| - d_min | within the tolerance (SegDist.residual) -- that proves a pair of closest points and is the right statement
where the minimiser is not unique; n within tol / d_axis where the axes are more than 1e-3 apart; where they meet (d = 0) n == (0, 1, 0) exactly in
float64, finite and of unit length within 4 u in float32.

Tolerances.  float64: 1e-12 absolute (quantities of O(1) m, the project's oracle-vs-reference convention).  float32: no number is fixed.  The float32
build of the oracle is measured per case against the reference; a device route may be MARGIN32 = 8 times worse (computed live, as in
tests/test_step_identity.py), where the oracle's own figure counts for at least u * scale (the rounding of ONE stored coordinate of that size: a smaller
measured error is luck), and everything sits under the hard bound `hard_bound32`.  Decisions: every candidate and pair of every case keeps
|dist - thr| and |y - report_dist| at least 100 gates away (`check_margins`), the designated exact tie excepted.

Found with it (docs/HISTORY.md section 31): for parallel axes (denom <= 1e-12) the segment routine started from s = 0 whatever the geometry, which put the
pair of axes converging towards the s = 1 end 2 L sin(angle) too far (float64: 4.0e-8 m at 1e-7 rad) -- fixed in kernels and oracle (`near_parallel`,
both signs).  Not asserted, because the geometry does not determine it: the normal of an interior pair of skew axes closer to parallel than 1e-3
(condition L / (d angle)); build_case refuses a case that would rest on one.

Sharpness: `test_mutants_are_caught` runs eight wrong variants of the reference over the same cases; each must change a slot list or move a figure by
more than 100 times the float32 hard bound on at least one case.
"""
from dataclasses import dataclass

import numpy as np
import pytest

import contact_geometry as cg
from deepmimic_amd import model
from deepmimic_amd.core import BatchEnv
from oracle_lib import Oracle
from test_physics_validity import box_tables

HUM, DOG, DRIBBLE = "humanoid3d_walk", "dog3d_pace", "amp_dribble_zombie"
H_STEP = 1.0 / 1200
U32 = 2.0 ** -24
TOL64 = 1e-12
MARGIN32 = 8.0
C_CHAIN = 128.0
TWO_PER_WAVE = (0, 1, 2, 22, 24)
UP = np.array([0.0, 1.0, 0.0])


def hard_bound32(scale):
    """C_CHAIN u scale, scale = |com|_max + L_max of the case.  C_CHAIN = 128 counts the roundings a contact figure passes through, each on a quantity
    bounded by `scale`: forward kinematics, at most 8 links deep (the dog's toes), per level the quaternion to its matrix (4), the product with the
    parent's rotation (3 products + 2 sums), the attach point rotated and added (3 + 1): 12 x 8 = 96; the contact routine: the segment ends (5), r (1),
    five dot products folded into s and t (10 + 6), the two points (4), their difference and its norm (1 + 5), the radii (2), x (2): about 32."""
    return C_CHAIN * U32 * scale


# ---------------------------------------------------------------------------------------------------------------- poses
def quat(axis, angle):
    a = np.asarray(axis, dtype=np.float64); a = a / np.linalg.norm(a)
    return np.r_[np.cos(angle / 2), np.sin(angle / 2) * a]


def qmul(a, b):
    w1, x1, y1, z1 = a; w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def make_pose(t, root_pos, root_rot=(1, 0, 0, 0), joints=None):
    """pose vector: identity joint rotations / zero angles but for `joints` {link: quaternion | angle}"""
    q = np.zeros(t.pose_dim); q[0:3] = root_pos; q[3:7] = root_rot
    for j in range(1, t.num_joints):
        off, ty = int(t.joint_mat[j, model.JD_PARAM_OFFSET]), int(t.joint_mat[j, model.JD_TYPE])
        if ty == model.JT_SPHERICAL:
            q[off] = 1.0
    for j, v in (joints or {}).items():
        off, ty = int(t.joint_mat[j, model.JD_PARAM_OFFSET]), int(t.joint_mat[j, model.JD_TYPE])
        if ty == model.JT_SPHERICAL:
            v = np.asarray(v, dtype=np.float64); q[off:off + 4] = v if v[0] >= 0 else -v
        else:
            q[off] = float(v)
    return q


def random_pose(t, seed, y):
    rng = np.random.default_rng(seed)
    rot = lambda: (lambda x: x / np.linalg.norm(x))(rng.normal(size=4))
    return make_pose(t, (0.0, y, 0.0), rot(), {j: (rot() if int(t.joint_mat[j, model.JD_TYPE]) == model.JT_SPHERICAL else rng.uniform(-1, 1)) for j in range(1, t.num_joints)})


# ---------------------------------------------------------------------------------------------------------------- the synthetic character
# root box (0) | arm A: capsule 1, sphere 2, box 3 | arm B: capsule 4, sphere 5, box 6, all on spherical joints.  The two capsules are centred on their joints,
# 0.16 m apart with radius 0.1: pair (1, 4) touches in EVERY pose and its region of (s, t) is set by the two rotations alone.  Non-adjacent pairs of every kind:
# capsule-capsule (1, 4), sphere-capsule (2, 4) (1, 5), box-capsule (1, 3) (1, 6) (3, 4), sphere-box (2, 6) (3, 5), box-box (3, 6) (0, 3) (0, 6), sphere-sphere (2, 5).
# Thresholds 0.02 R: capsule 6 mm, sphere 2 mm, arm box 3.5 mm, root box 4.1 mm.
SYN_PARENT = (-1, 0, 1, 2, 0, 4, 5)
SYN_ATTACH = {1: (-0.08, 0, 0), 2: (0, -0.32, 0), 3: (0, -0.12, 0), 4: (0.08, 0, 0), 5: (0, -0.32, 0), 6: (0, -0.12, 0)}
SYN_BODY = {0: (model.SH_BOX, (0.3, 0.2, 0.2), (0, 0, 0)), 1: (model.SH_CAPSULE, (0.2, 0.4, 0), (0, 0, 0)), 2: (model.SH_SPHERE, (0.2, 0.2, 0.2), (0, 0, 0)),
            3: (model.SH_BOX, (0.1, 0.3, 0.16), (0, -0.1, 0)), 4: (model.SH_CAPSULE, (0.2, 0.4, 0), (0, 0, 0)), 5: (model.SH_SPHERE, (0.2, 0.2, 0.2), (0, 0, 0)),
            6: (model.SH_BOX, (0.1, 0.3, 0.16), (0, -0.1, 0))}
SYN_Y = 1.5


def synth_tables():
    J = len(SYN_PARENT)
    jm = np.zeros((J, 19))
    off = 0
    for j in range(J):
        d = model._joint_desc_default()
        d[model.JD_TYPE] = model.JT_NONE if j == 0 else model.JT_SPHERICAL; d[model.JD_PARENT] = SYN_PARENT[j]; d[model.JD_TORQUE_LIM] = 100.0
        d[model.JD_AX:model.JD_AZ + 1] = SYN_ATTACH.get(j, (0, 0, 0)); d[model.JD_PARAM_OFFSET] = off
        off += model.joint_param_size(int(d[model.JD_TYPE]), j == 0)
        jm[j] = d
    bd = np.zeros((J, 17))
    for j, (sh, p, a) in SYN_BODY.items():
        d = model._body_def_default()
        d[model.BD_SHAPE] = sh; d[model.BD_MASS] = 2.0; d[model.BD_COLGROUP] = 1; d[model.BD_P0:model.BD_P2 + 1] = p; d[model.BD_AX:model.BD_AZ + 1] = a
        bd[j] = d
    cfg = model.SceneConfig(); cfg.enable_char_contact_fall = False; cfg.enable_fall_end = False
    t = model.SceneTables(joint_mat=jm, body_defs=bd, pd_params=np.zeros((J, 2)), frames=np.zeros((2, off + 1)), loop=True, cfg=cfg, joint_names=["j%d" % j for j in range(J)])
    pose = make_pose(t, (0.0, SYN_Y, 0.0))
    t.frames = np.array([np.r_[0.5, pose], np.r_[0.5, pose]])
    return t


# ---------------------------------------------------------------------------------------------------------------- cases
@dataclass
class Built:
    name: str
    t: object
    parents: list
    Q: np.ndarray
    BALL: object
    cfg: object              # cg.Config
    links: list              # per env Oracle.links() of the float64 oracle
    refs: list               # per env (rows, info) of the reference
    scale: float
    duo: bool                # the two-per-wave kernels serve this character
    tie: bool = False        # the designated exact tie: exempt from the margin rule


_CACHE, _TABLES = {}, {}


def tables_of(asset, one_substep=False):
    key = (asset, one_substep)
    if key not in _TABLES:
        t = synth_tables() if asset == "synth" else (box_tables() if asset == "box" else model.load_asset(asset))
        if one_substep:
            t.cfg.num_sim_substeps = 1
        _TABLES[key] = t
    return _TABLES[key]


def reference_of(b, e, **kw):
    return cg.contacts(b.links[e], b.t.body_defs, b.parents, b.cfg, ball=None if b.BALL is None else b.BALL[e][0:3], **kw)


def build_case(name):
    if name in _CACHE:
        return _CACHE[name]
    asset, max_contacts, make = CASES[name]
    t = tables_of(asset)
    o = Oracle(t)
    Q, BALL = make(t, o)
    Q = np.array(Q)
    parents = [int(x) for x in t.joint_mat[:, model.JD_PARENT]]
    cfg = cg.Config(max_contacts=max_contacts, report_dist=0.001, ball_radius=float(t.cfg.ball_radius) if BALL is not None else 0.0)
    links = []
    for q in Q:
        o.set_sim_state(q, np.zeros(o.P)); links.append(o.links().copy())
    b = Built(name, t, parents, Q, None if BALL is None else np.array(BALL), cfg, links, [], 0.0, duo=asset in (HUM, DRIBBLE) and len(Q) % 2 == 0, tie=name == "box_tie")
    b.refs = [reference_of(b, e) for e in range(len(Q))]
    ext = max(2 * cg.shape_radius(*cg.shape_of(bd)) for bd in t.body_defs)
    b.scale = max(float(np.abs(l[:, 0:3]).max()) for l in links) + ext
    CONDITIONS[name](b)
    check_margins(b, 100 * TOL64)
    # Where both closest points are interior the pair sits at u / sin^2(angle) in (s, t) and its normal at u L / (d sin(angle)): an interior minimiser of axes
    # closer to parallel than 1e-3 has no normal to 1e-12 in float64, whatever the routine.  No case may rest on one.
    for e, (rows, info) in enumerate(b.refs):
        for p in info["pairs"]:
            sd = p["sd"]
            if p["active"] and sd.unique and sd.region(1e-6) == ("i", "i") and sd.dmin > 1e-3:
                assert sd.sin_angle >= 1e-3, (name, e, p["i"], p["j"], sd.sin_angle)
    _CACHE[name] = b
    return b


def margins(b):
    """the least |dist - thr| over every ground candidate, link pair and ball test of the case, and the least |y - report_dist|"""
    m_thr, m_rep = np.inf, np.inf
    for rows, info in b.refs:
        for j, _, y in info["cand"]:
            m_thr = min(m_thr, abs(y - info["thr"][j])); m_rep = min(m_rep, abs(y - b.cfg.report_dist))
        for p in info["pairs"]:
            m_thr = min(m_thr, abs(p["dist"] - p["thr"]))
        if info["n_active_ground_uncut"] > b.cfg.max_contacts:          # the cut: the depths that decide it differ by the margin, or are EXACTLY equal (the designated tie)
            ys = sorted(y for j, _, y in info["cand"] if y < info["thr"][j])
            gap = ys[b.cfg.max_contacts] - ys[b.cfg.max_contacts - 1]
            if not (b.tie and gap == 0.0):
                m_thr = min(m_thr, gap)
        for p in info["ball"]:
            m_thr = min(m_thr, abs(p["dist"] - p["thr"]))
    return m_thr, m_rep


def check_margins(b, least):
    m_thr, m_rep = margins(b)
    assert m_thr >= least and m_rep >= least, "%s: a decision %.3e / %.3e from its threshold, need %.3e: move the state" % (b.name, m_thr, m_rep, least)


# ---- builders: (poses, balls or None).  Numbers that were searched carry the condition they were searched for in CONDITIONS.
def _syn(joints=None, root_rot=(1, 0, 0, 0)):
    return lambda t: make_pose(t, (0.0, SYN_Y, 0.0), root_rot, joints)


def make_special(t, o):
    """constructed poses of the synthetic character, one per env"""
    Q = [make_pose(t, (0.0, SYN_Y, 0.0))]                                                    # 0 all identity: capsules 1 | 4 exactly parallel and level; spheres 2 | 5 touch; (2, 4) and (1, 5) point against segment
    Q.append(make_pose(t, (0.0, SYN_Y, 0.0), joints={1: quat((0, 0, 1), -np.pi / 6), 4: quat((0, 0, 1), np.pi / 6)}))     # 1 the axes of 1 and 4 meet 0.16 m up each segment
    # 2, 3: sphere 2 (thr 2 mm) against capsule 4 (thr 6 mm) at +1 mm and at +4 mm: arm A swung about z until the reference reads that distance
    for want in (0.001, 0.004):
        Q.append(make_pose(t, (0.0, SYN_Y, 0.0), joints={1: quat((0, 0, 1), _solve_swing(t, o, want))}))
    Q.append(make_pose(t, (0.0, SYN_Y, 0.0), joints={1: quat((1, 0, 0), np.pi / 2), 4: quat((0, 0, 1), np.pi / 2)}))     # 4 perpendicular axes through both centres
    phi = np.arcsin(0.041 / 0.64)                                                            # 5 both arms swung out: spheres 2 | 5 one millimetre apart, inside their 2 mm threshold
    Q.append(make_pose(t, (0.0, SYN_Y, 0.0), joints={1: quat((0, 0, 1), -phi), 4: quat((0, 0, 1), phi)}))
    return Q, None


def _solve_swing(t, o, want):
    """the angle about z of joint 1 at which sphere 2 is `want` from capsule 4 (bisection on the reference, on the side where the arm swings away)"""
    par = list(SYN_PARENT)
    def dist(a):
        o.set_sim_state(make_pose(t, (0.0, SYN_Y, 0.0), joints={1: quat((0, 0, 1), a)}), np.zeros(o.P))
        return cg.pair_of(cg.contacts(o.links(), t.body_defs, par, cg.Config())[1], 2, 4)["dist"]
    lo, hi = 0.0, -0.3                    # dist(0) = 0 (touching), dist(-0.3) > 4 mm: swinging towards -x moves the sphere away
    assert dist(lo) < want < dist(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if dist(mid) < want else (lo, mid)
    return 0.5 * (lo + hi)


NEAR_PARALLEL = tuple((sg, ang) for sg in (1, -1) for ang in (1e-3, 1e-5, 1e-7))


def make_near_parallel(t, o):
    """capsule 4 turned about z by +-angle: the two axes stay in one plane and converge towards one end, where the unique closest pair sits: the end s = t = 0
    for +, s = t = 1 for -.  (Turned about x instead the axes are skew with the closest pair at both centres, and every pair along the overlap is within
    (L angle)^2 / 2 d of the minimum: the normal is then not determined to the accuracy of the distance, and no case uses it -- build_case.)"""
    return [make_pose(t, (0.0, SYN_Y, 0.0), joints={4: quat((0, 0, 1), sg * ang)}) for sg, ang in NEAR_PARALLEL], None


REGION_SEEDS = (313, 6, 17)          # searched for cond_regions: the nine regions and the five pair kinds among the active pairs, margins kept


def make_regions(t, o):
    return [random_pose(t, s, SYN_Y) for s in REGION_SEEDS], None


def make_box_tie(t, o):
    """the box set down with identity rotation (four corners at y = 0 exactly, in float32 too), and two controls: tipped about z (two corners deeper), yawed (still tied)"""
    return [make_pose(t, (0.0, 0.2, 0.0)), make_pose(t, (0.0, 0.19, 0.0), quat((0, 0, 1), 0.01)), make_pose(t, (0.3, 0.2, -0.2), quat((0, 1, 0), 0.5)), make_pose(t, (0.0, 0.199, 0.0), quat((0, 0, 1), -0.02))], None


# ---- humanoid (both packings).  Numbers found by search on the reference; what they were searched for is asserted in the conditions.
LEGS_ABDUCTION = 0.0462300832928121           # hips turned in by this much: the mirrored shins 2 mm into each other at their lower ends
HAND_ON_THIGH = {6: (0.41504886, 0.89114599, 0.03926654), 7: 0.35737765}           # right shoulder (rotation vector), right elbow: the right hand 4 mm into the left thigh
FOREARMS = {6: (1.12379619, 1.94187251, 0.06676532), 7: 0.30139685, 12: (-0.00354108, 1.0156283, -1.3615769), 13: 0.36346554}       # the forearms crossed mid-segment, 4 mm in
LYING = dict(roll=0.17, pitch=0.03, y=0.03, joints={3: ((1, 0, 0), 0.13), 9: ((1, 0, 0), -0.21), 6: ((1, 0, 0), -0.3), 12: ((1, 0, 0), 0.37), 4: -0.2, 10: -0.35, 7: 0.3, 13: 0.5})
STAND_Y = 0.8805538903217855                  # legs together, the soles 2 mm into the ground
AIR_Y = 2.0


def rotvec(v):
    v = np.asarray(v, dtype=np.float64); a = float(np.linalg.norm(v))
    return quat(v / a, a) if a > 0 else np.array([1.0, 0, 0, 0])


def _arms(spec):
    return {j: (rotvec(v) if isinstance(v, tuple) else v) for j, v in spec.items()}


def _legs():
    return {3: quat((1, 0, 0), LEGS_ABDUCTION), 9: quat((1, 0, 0), -LEGS_ABDUCTION)}


def _lying(t):
    rr = qmul(quat((0, 0, 1), LYING["pitch"]), qmul(quat((1, 0, 0), LYING["roll"]), quat((0, 0, 1), -np.pi / 2)))
    return make_pose(t, (0.0, LYING["y"], 0.0), rr, {j: (quat(*v) if isinstance(v, tuple) else v) for j, v in LYING["joints"].items()})


def make_hum_pairs(t, o):
    """0 mirrored legs brought together, 1 the right hand on the left thigh, 2 forearm across forearm (all airborne), 3 lying on the back, rolled and pressed in"""
    return [make_pose(t, (0.0, AIR_Y, 0.0), joints=_legs()), make_pose(t, (0.0, AIR_Y, 0.0), joints=_arms(HAND_ON_THIGH)),
            make_pose(t, (0.0, AIR_Y, 0.0), joints=_arms(FOREARMS)), _lying(t)], None


def make_hum_slots(t, o):
    """standing with the legs together and the right hand on the left thigh: 4 ground contacts and 4 active pairs for 6 slots; the same turned about the vertical"""
    jj = dict(_legs()); jj.update(_arms(HAND_ON_THIGH))
    return [make_pose(t, (0.0, STAND_Y, 0.0), joints=jj), make_pose(t, (0.4, STAND_Y, -0.3), quat((0, 1, 0), 0.7), jj)], None


# ---- dog (the class with the bounding-sphere cull): curled poses, seeds searched for the largest |com_i - com_j| / (brad_i + brad_j) among ACTIVE pairs and for many pairs
DOG_SEEDS = (160, 267, 209, 467)


def curled_dog(t, seed, scale=0.9):
    rng = np.random.default_rng(seed)
    jj = {}
    for j in range(1, t.num_joints):
        ty = int(t.joint_mat[j, model.JD_TYPE])
        if ty == model.JT_SPHERICAL:
            jj[j] = rotvec(rng.normal(size=3) * scale)
        elif ty == model.JT_REVOLUTE:
            jj[j] = rng.uniform(-2.0, 0.0)
    return make_pose(t, (0.0, AIR_Y, 0.0), joints=jj)


def make_dog(t, o):
    return [curled_dog(t, s) for s in DOG_SEEDS], None


# ---- biped + ball
SHIN = 4


def _ball(c):
    b = np.zeros(13); b[0:3] = c; b[3] = 1.0
    return b


def make_ball(t, o):
    """0 the ball resting on the ground away from the airborne character, 1 against the right shin mid-segment, 2 against its lower end cap, 3 its centre on the shin's axis"""
    q = make_pose(t, (0.0, AIR_Y, 0.0))
    o.set_sim_state(q, np.zeros(o.P))
    l = o.links()[SHIN]
    com, R = l[0:3], l[3:12].reshape(3, 3)
    axis, perp = R @ np.array([0.0, 1.0, 0.0]), R @ np.array([1.0, 0.0, 0.0])
    half, r = cg.link_capsule(*cg.shape_of(t.body_defs[SHIN]))
    hl, rb = float(np.linalg.norm(half)), float(t.cfg.ball_radius)
    slant = (-0.8 * axis + 0.6 * perp)
    balls = [_ball((3.0, rb - 0.001, 0.5)), _ball(com + (r + rb - 0.002) * perp), _ball(com - hl * axis + (r + rb - 0.002) * slant), _ball(com + 0.05 * axis)]
    return [q] * 4, balls


BALL_SLOTS_MC = 9


def make_ball_slots(t, o):
    """standing (4 ground contacts + 4 active pairs) with one slot left, the ball on the ground AND against the right foot: the ball-ground contact takes the slot"""
    jj = dict(_legs()); jj.update(_arms(HAND_ON_THIGH))
    q = make_pose(t, (0.0, STAND_Y, 0.0), joints=jj)
    o.set_sim_state(q, np.zeros(o.P))
    foot = o.links()[5][0:3]
    rb = float(t.cfg.ball_radius)
    return [q, q], [_ball((foot[0] + 0.19, rb - 0.001, foot[2])), _ball((foot[0] + 0.19, rb - 0.0015, foot[2] + 0.01))]


CASES = {
    "special": ("synth", 20, make_special),
    "near_parallel": ("synth", 20, make_near_parallel),
    "regions": ("synth", 20, make_regions),
    "box_tie": ("box", 3, make_box_tie),
    "hum_pairs": (HUM, 20, make_hum_pairs),
    "hum_slots": (HUM, 6, make_hum_slots),
    "dog": (DOG, 20, make_dog),
    "ball": (DRIBBLE, 20, make_ball),
    "ball_slots": (DRIBBLE, BALL_SLOTS_MC, make_ball_slots),
}
CONDITIONS = {}


# ---- conditions: what each case is named for, on the reference
def _active(info, i, j):
    return cg.pair_of(info, i, j)["active"]


def _angle(sd):
    u, v = sd.p1 - sd.p0, sd.q1 - sd.q0
    return float(np.arctan2(np.linalg.norm(np.cross(u, v)), abs(u @ v)))


def cond_special(b):
    infos = [r[1] for r in b.refs]
    p = cg.pair_of(infos[0], 1, 4)                               # exactly parallel, overlapping: the minimiser is not unique
    assert p["active"] and not p["sd"].unique and _angle(p["sd"]) == 0.0
    p = cg.pair_of(infos[0], 2, 5)                               # point against point
    assert p["active"] and np.array_equal(p["sd"].p0, p["sd"].p1) and np.array_equal(p["sd"].q0, p["sd"].q1)
    p = cg.pair_of(infos[0], 2, 4)                               # point (link a) against segment: a <= eps
    assert p["active"] and np.array_equal(p["sd"].p0, p["sd"].p1) and not np.array_equal(p["sd"].q0, p["sd"].q1)
    p = cg.pair_of(infos[0], 1, 5)                               # segment against point (link b): e <= eps
    assert p["active"] and np.array_equal(p["sd"].q0, p["sd"].q1) and not np.array_equal(p["sd"].p0, p["sd"].p1)
    p = cg.pair_of(infos[1], 1, 4)                               # intersecting axes: d = 0, the normal is the fallback
    assert p["active"] and p["sd"].dmin < 1e-15 and p["sd"].region() == ("i", "i")
    row = next(r for r in b.refs[1][0] if (int(r[0]), int(r[1])) == (1, 4))
    assert np.array_equal(row[6:9], UP)
    inside, outside = cg.pair_of(infos[2], 2, 4), cg.pair_of(infos[3], 2, 4)      # thresholds 2 mm | 6 mm: below the smaller, between the two
    assert inside["thr_j"] >= 2 * inside["thr_i"]
    assert inside["active"] and abs(inside["dist"] - 0.001) < 1e-9 and inside["dist"] < inside["thr"]
    assert not outside["active"] and abs(outside["dist"] - 0.004) < 1e-9 and min(outside["thr_i"], outside["thr_j"]) < outside["dist"] < max(outside["thr_i"], outside["thr_j"])
    assert cg.pair_of(infos[4], 1, 4)["sd"].region(1e-6) == ("i", "i")
    p = cg.pair_of(infos[5], 2, 5)                               # separated and active: the centres are farther apart than the two radii, only the threshold term keeps the pair from a cull
    assert p["active"] and abs(p["dist"] - 0.001) < 1e-12 and p["sd"].dmin > p["ra"] + p["rb"] and p["cull_ratio"] < 1
    assert all(len(r[0]) < b.cfg.max_contacts and not r[1]["active_ground"] for r in b.refs)


def cond_near_parallel(b):
    """the relative angle, a unique closest pair at the converging end -- which is the end s = 0 for +, s = 1 for - -- and a normal the geometry determines"""
    for (sg, ang), (rows, info) in zip(NEAR_PARALLEL, b.refs):
        p = cg.pair_of(info, 1, 4); sd = p["sd"]
        assert p["active"] and abs(_angle(sd) / ang - 1) < 1e-6 and sd.unique, (sg, ang, _angle(sd))
        assert sd.region(1e-5) == ((0, 0) if sg > 0 else (1, 1)), (sg, ang, sd.s, sd.t)
        far = np.linalg.norm((sd.p1 if sg > 0 else sd.p0) - (sd.q1 if sg > 0 else sd.q0))          # the other end is farther by 2 L sin(angle) (L = 0.2)
        assert abs((far - sd.dmin) / (0.4 * np.sin(ang)) - 1) < 1e-3, (far - sd.dmin, ang)


def cond_regions(b):
    """all nine combinations of s in {0, interior, 1} x t in {0, interior, 1} among the ACTIVE pairs of two proper segments, and every pair kind"""
    seen, kinds = set(), set()
    shape = lambda j: cg.shape_of(b.t.body_defs[j])[0]
    for rows, info in b.refs:
        assert len(rows) < b.cfg.max_contacts
        for p in info["pairs"]:
            if p["active"]:
                kinds.add(tuple(sorted((shape(p["i"]), shape(p["j"])))))
                sd = p["sd"]
                if not np.array_equal(sd.p0, sd.p1) and not np.array_equal(sd.q0, sd.q1) and sd.unique:
                    # the class must be robust: the parameter 1e-3 inside its class
                    for tol in (1e-9, 1e-3):
                        assert sd.region(tol) == sd.region(), (p["i"], p["j"], sd.s, sd.t)
                    seen.add(sd.region())
    assert seen == {(a, c) for a in (0, "i", 1) for c in (0, "i", 1)}, sorted(map(str, seen))
    B, C, S = cg.SH_BOX, cg.SH_CAPSULE, cg.SH_SPHERE
    assert {(C, C), (C, S), (B, C), (B, S), (B, B)} <= kinds, kinds


def cond_box_tie(b):
    rows, info = b.refs[0]
    ys = [y for _, _, y in info["cand"]]
    assert [k for k, y in enumerate(ys) if y == 0.0] == [2, 3, 6, 7] and info["n_active_ground_uncut"] == 4      # four corners exactly on the plane
    assert info["active_ground"] == [2, 3, 6]                                                                    # the three lower indices
    assert np.float32(0.2) - np.float32(0.5 * 0.4) == 0                                                          # ... and the tie is exact in float32 too
    for rows, info in b.refs:
        assert info["n_active_ground_uncut"] == 4 and len(rows) == 3
    assert b.refs[1][1]["active_ground"] != [2, 3, 6]                                                            # the tipped control keeps other corners


def cond_hum_pairs(b):
    infos = [r[1] for r in b.refs]
    shins, thighs = cg.pair_of(infos[0], 4, 10), cg.pair_of(infos[0], 3, 9)
    assert shins["active"] and shins["sd"].sin_angle < 0.1 and thighs["sd"].sin_angle < 0.1           # near-parallel mirrored pairs (2 x the abduction)
    assert cg.pair_of(infos[1], 8, 9)["active"]                                                         # the right hand on the left thigh
    arms = cg.pair_of(infos[2], 7, 13)
    assert arms["active"] and arms["sd"].region(0.05) == ("i", "i") and arms["sd"].sin_angle > 0.5      # forearm across forearm
    rows, info = b.refs[3]                                                                              # lying: more candidates than slots, at distinct depths, no slot for a pair
    ys = sorted(y for j, _, y in info["cand"] if y < info["thr"][j])
    assert info["n_active_ground_uncut"] > b.cfg.max_contacts and min(np.diff(ys)) > 1e-4 and info["n_active_pairs"] > 0
    assert len(rows) == b.cfg.max_contacts and (rows[:, 1] == -1).all() and (rows[:, 9] == 0).all()
    assert all(not r[1]["active_ground"] for r in b.refs[:3])


def cond_hum_slots(b):
    for rows, info in b.refs:
        k = info["n_active_ground_uncut"]
        assert 0 < k < b.cfg.max_contacts and info["n_active_pairs"] > b.cfg.max_contacts - k and len(rows) == b.cfg.max_contacts
        act = [(p["i"], p["j"]) for p in info["pairs"] if p["active"]]
        assert [(int(r[0]), int(r[1])) for r in rows[k:]] == act[:b.cfg.max_contacts - k]            # the first pairs in pair order


DOG_MAX_RATIO = 0.97          # the largest |com_i - com_j| / (brad_i + brad_j) of an active pair in these poses (a record, not a gate: 0.9726)


def cond_dog(b):
    ratios = [p["cull_ratio"] for rows, info in b.refs for p in info["pairs"] if p["active"]]
    print("CONTACTS dog: %d active pairs, cull ratios up to %.4f" % (len(ratios), max(ratios)))
    assert max(ratios) > DOG_MAX_RATIO and max(r[1]["n_active_pairs"] for r in b.refs) >= 10 and all(r < 1.0 for r in ratios)
    assert all(len(r[0]) < b.cfg.max_contacts for r in b.refs)


def cond_ball(b):
    kinds = [[(int(r[0]), int(r[9])) for r in rows] for rows, _ in b.refs]
    assert kinds[0] == [(-1, 2)]                                                                    # resting on the ground
    mid, cap, axis = (b.refs[e][1]["ball"][1 + SHIN] for e in (1, 2, 3))
    assert (SHIN, 1) in kinds[1] and mid["sd"].region(0.05)[0] == "i"                               # mid-segment
    assert (SHIN, 1) in kinds[2] and cap["sd"].region()[0] == 1                                     # the end cap
    assert (SHIN, 1) in kinds[3] and axis["sd"].dmin < 1e-15                                        # centre on the axis: the fallback normal
    row = next(r for r in b.refs[3][0] if (int(r[0]), int(r[9])) == (SHIN, 1))
    assert np.array_equal(row[6:9], UP)


def cond_ball_slots(b):
    for rows, info in b.refs:
        nb = sum(1 for p in info["ball"] if p["dist"] < p["thr"])
        assert info["n_active_ground_uncut"] + info["n_active_pairs"] == b.cfg.max_contacts - 1 and nb >= 2, (info["n_active_ground_uncut"], info["n_active_pairs"], nb)
        assert len(rows) == b.cfg.max_contacts and int(rows[-1][9]) == 2 and all(int(r[9]) == 0 for r in rows[:-1])


CONDITIONS.update(hum_pairs=cond_hum_pairs, hum_slots=cond_hum_slots, dog=cond_dog, ball=cond_ball, ball_slots=cond_ball_slots)
CONDITIONS.update(near_parallel=cond_near_parallel, special=cond_special, regions=cond_regions, box_tie=cond_box_tie)


# ---------------------------------------------------------------------------------------------------------------- routes
def run_oracle(b, variant, physics=1):
    o = Oracle(b.t, variant=variant, max_contacts=v2_max_contacts(b) if physics == 2 else b.cfg.max_contacts, physics=physics)
    lists, masks = [], []
    for e, q in enumerate(b.Q):
        o.set_sim_state(q, np.zeros(o.P))
        if physics == 2:
            o.set_manifolds(np.zeros((o.J, 25)))
        if b.BALL is not None:
            o.set_ball(b.BALL[e])
        o.set_tau(np.zeros(o.P)); o.substep(H_STEP)
        lists.append(o.contact_list_ex()); masks.append(int(sum(int(c) << j for j, c in enumerate(o.contacts()))))
    return lists, masks


def _env(b, lib, prec, one_substep=False, **kw):
    asset = CASES[b.name][0]
    env = BatchEnv(tables_of(asset, one_substep) if one_substep else b.t, len(b.Q), precision=prec, lib_path=lib, max_contacts=b.cfg.max_contacts, **kw)
    assert env.max_contacts == (v2_max_contacts(b) if kw.get("physics", 1) == 2 else b.cfg.max_contacts)
    st0 = env.get_state()
    env.set_state(pose=b.Q, vel=np.zeros_like(b.Q), tar=b.Q, kin=st0["kin"], clocks=st0["clocks"])
    if b.BALL is not None:
        env.set_obj_state(b.BALL)
    return env


def run_tap(b, lib, prec, physics=1):
    """one character per wavefront: dm_probe 1"""
    env = _env(b, lib, prec, wave_packing=1, physics=physics)
    env.set_tau(np.zeros((len(b.Q), env.D)))
    env.probe(1, H_STEP)
    cs, mask = env.contacts(), env.get_state()["flags"][:, 1].copy()
    env.close()
    return cs, [int(x) for x in mask]


def run_tap_duo(b, lib, prec):
    """two characters per wavefront: one update of the tap instantiation of the two-per-wave kernel (dm_probe 5; tables with one substep per update)"""
    env = _env(b, lib, prec, one_substep=True, wave_packing=2)
    env.probe(5, H_STEP)
    fam = env.debug("family")
    cs, mask = env.contacts(), env.get_state()["flags"][:, 1].copy()
    env.close()
    assert int(fam[0]) == 2, fam
    return cs, [int(x) for x in mask]


def run_production(b, lib, prec, pack, variant):
    """no taps: one dm_update of the step kernel (tables with one substep per update); the contact mask and the family that ran"""
    asset = CASES[b.name][0]
    t1 = tables_of(asset, True)
    kw = {}
    if variant == "amp":          # the AMP instantiation: any of its switches selects it; the root-rotation fail test leaves the contact mask alone
        import copy
        t1 = copy.deepcopy(t1); t1.cfg.enable_root_rot_fail = True
    env = BatchEnv(t1, len(b.Q), precision=prec, lib_path=lib, max_contacts=b.cfg.max_contacts, wave_packing=pack, physics=2 if variant == "v2" else 1)
    st0 = env.get_state()
    env.set_state(pose=b.Q, vel=np.zeros_like(b.Q), tar=b.Q, kin=st0["kin"], clocks=st0["clocks"])
    if b.BALL is not None:
        env.set_obj_state(b.BALL)
    env.update(H_STEP, 1)
    mask, fam = env.get_state()["flags"][:, 1].copy(), int(env.debug("family")[0])
    env.close()
    return [int(x) for x in mask], fam


# ---------------------------------------------------------------------------------------------------------------- evaluation
def compare(b, e, got, prec, label, ref=None):
    """structure exactly; returns the errors {dist, pt, n} of env e in metres (n scaled by the axis distance)"""
    rows, info = ref if ref is not None else b.refs[e]
    assert got.shape == rows.shape, "%s %s env %d: %d slots, reference %d\n%s\n%s" % (b.name, label, e, len(got), len(rows), got[:, [0, 1, 9]], rows[:, [0, 1, 9]])
    assert np.array_equal(got[:, [0, 1, 9]], rows[:, [0, 1, 9]]), "%s %s env %d: slots\n%s\nreference\n%s" % (b.name, label, e, got[:, [0, 1, 9]], rows[:, [0, 1, 9]])
    err = dict(dist=0.0, pt=0.0, n=0.0)
    for r, g in zip(rows, got):
        la, lb, kind = int(r[0]), int(r[1]), int(r[9])
        err["dist"] = max(err["dist"], abs(g[2] - r[2]))
        if (kind == 0 and lb < 0) or kind == 2:                 # against the ground: the point itself, the normal exactly
            assert np.array_equal(g[6:9], UP), (b.name, label, e, g)
            err["pt"] = max(err["pt"], float(np.abs(g[3:6] - r[3:6]).max()))
            continue
        p = cg.pair_of(info, la, lb) if kind == 0 else info["ball"][1 + la]
        sd, n = p["sd"], g[6:9]
        ca, cb = g[3:6] + (p["ra"] + g[2] / 2) * n, g[3:6] - (p["rb"] + g[2] / 2) * n
        err["pt"] = max(err["pt"], sd.residual(ca, cb))
        if sd.dmin > 1e-3:
            err["n"] = max(err["n"], float(np.abs(n - r[6:9]).max()) * sd.dmin)
        elif sd.dmin < 1e-12:                                   # the axes meet
            if prec == 64:
                assert np.array_equal(n, UP), (b.name, label, e, n)
            else:
                assert np.all(np.isfinite(n)) and abs(float(np.linalg.norm(n)) - 1) <= 4 * U32, (b.name, label, e, n)
        else:
            raise AssertionError("%s env %d pair (%d, %d): axis distance %.3e is neither a contact of two separate axes nor d = 0" % (b.name, e, la, lb, sd.dmin))
    return err


def worst(b, lists, prec, label, refs=None):
    w = dict(dist=0.0, pt=0.0, n=0.0)
    for e, got in enumerate(lists):
        err = compare(b, e, got, prec, label, None if refs is None else refs[e])
        for k in w:
            w[k] = max(w[k], err[k])
    return w


def gate32(b, w32):
    """per figure: MARGIN32 x the float32 oracle's error (at least u * scale), under the hard bound"""
    return {k: min(MARGIN32 * max(w32[k], U32 * b.scale), hard_bound32(b.scale)) for k in w32}


def check_route(b, lists, masks, prec, label, refs=None, want_masks=None):
    w = worst(b, lists, prec, label, refs)
    line = "CONTACTS %-12s %-22s f%d: dist %.2e pt %.2e n %.2e" % (b.name, label, prec, w["dist"], w["pt"], w["n"])
    if prec == 64:
        print(line + " (tol %.0e)" % TOL64)
        for k in w:
            assert w[k] <= TOL64, (b.name, label, k, w[k])
    else:
        o32, _ = run_oracle(b, "f32", physics=2 if refs is not None else 1)
        w32 = worst(b, o32, 32, "oracle f32", refs)
        g = gate32(b, w32)
        print(line + " | oracle f32: dist %.2e pt %.2e n %.2e | gate %.2e %.2e %.2e, hard bound %.2e" % (w32["dist"], w32["pt"], w32["n"], g["dist"], g["pt"], g["n"], hard_bound32(b.scale)))
        check_margins(b, 100 * max(g.values()))
        for k in w32:
            assert w32[k] <= hard_bound32(b.scale), (b.name, "oracle f32", k, w32[k])
        if label != "oracle":
            for k in w:
                assert w[k] <= g[k], "%s %s: %s error %.3e beyond the gate %.3e (oracle float32 %.3e)" % (b.name, label, k, w[k], g[k], w32[k])
    if masks is not None:
        want = want_masks if want_masks is not None else [cg.contact_mask(r[1]) for r in b.refs]
        assert masks == want, (b.name, label, masks, want)
    return w


def v2_max_contacts(b):
    """DM-physics v2 carries both rows of every revolute limit: 64 rows leave (64 - 2 limits) / 3 contacts"""
    jm = b.t.joint_mat
    nlim = sum(1 for j in range(1, len(jm)) if int(jm[j, model.JD_TYPE]) == model.JT_REVOLUTE and jm[j, model.JD_LL0] <= jm[j, model.JD_LH0])
    return min(b.cfg.max_contacts, (64 - 2 * nlim) // 3)


def v2_refs(b):
    import dataclasses
    cfg = dataclasses.replace(b.cfg, max_contacts=v2_max_contacts(b))
    return [cg.contacts(b.links[e], b.t.body_defs, b.parents, cfg, ball=None if b.BALL is None else b.BALL[e][0:3], manifold_first=True) for e in range(len(b.Q))]


# ---------------------------------------------------------------------------------------------------------------- CPU: the reference itself
def _grid_min(p0, p1, q0, q1, n=401):
    s = np.linspace(0.0, 1.0, n)
    P = p0[None, :] + s[:, None] * (p1 - p0)[None, :]
    Qp = q0[None, :] + s[:, None] * (q1 - q0)[None, :]
    return float(np.sqrt(((P[:, None, :] - Qp[None, :, :]) ** 2).sum(-1)).min())


def designated_segments():
    """segment pairs of the constructed cases, as plain geometry: every region of (s, t), parallel, near-parallel, degenerate, intersecting"""
    z, x, y = np.zeros(3), np.array([1.0, 0, 0]), np.array([0, 1.0, 0])
    S = {}
    for a, sa in ((0, -1.5), ("i", 0.5), (1, 2.5)):              # q's foot point on p's line before, inside, past p; p's on q's likewise: the nine regions
        for c, tc in ((0, -1.5), ("i", 0.5), (1, 2.5)):
            w = np.array([0, 0, 1.0])
            S["region_%s%s" % (a, c)] = (z, x, sa * x + 0.3 * y - tc * w, sa * x + 0.3 * y - tc * w + w)
    S["parallel_overlap"] = (z, x, 0.2 * y + 0.5 * x, 0.2 * y + 1.5 * x)
    S["parallel_apart"] = (z, x, 0.2 * y + 2 * x, 0.2 * y + 3 * x)
    S["antiparallel"] = (z, x, 0.2 * y + 0.7 * x, 0.2 * y - 0.3 * x)
    for ang in (1e-3, 1e-5, 1e-7):
        S["near_parallel_%g" % ang] = (z - 0.5 * x, 0.5 * x, 0.2 * y - 0.5 * np.array([np.cos(ang), 0, np.sin(ang)]), 0.2 * y + 0.5 * np.array([np.cos(ang), 0, np.sin(ang)]))
    S["point_segment"] = (0.3 * y + 0.4 * x, 0.3 * y + 0.4 * x, z, x)
    S["segment_point"] = (z, x, 0.3 * y + 1.4 * x, 0.3 * y + 1.4 * x)
    S["point_point"] = (y, y, x, x)
    S["intersecting"] = (z - x, x, -y, y)
    S["touching_end"] = (z, x, x, x + y)
    return S


def test_reference_segment_distance_against_a_dense_grid():
    """the enumeration is <= the minimum over a 401 x 401 grid of (s, t) and within the grid's resolution of it: a grid point lies within 1 / 800 of any (s, t) in
    each parameter and the distance is Lipschitz with constants |u| and |v|, so grid_min - d_min <= (|u| + |v|) / 800"""
    rng = np.random.default_rng(5)
    pairs = [tuple(rng.normal(size=3) * sc for sc in rng.uniform(0.05, 1.0, size=4)) for _ in range(200)] + list(designated_segments().values())
    for p0, p1, q0, q1 in pairs:
        sd = cg.segment_distance(p0, p1, q0, q1)
        g = _grid_min(*(np.asarray(v, dtype=np.float64) for v in (p0, p1, q0, q1)))
        res = (np.linalg.norm(np.subtract(p1, p0)) + np.linalg.norm(np.subtract(q1, q0))) / 800
        assert sd.dmin <= g + 1e-15 and g - sd.dmin <= res + 1e-15, (p0, p1, q0, q1, sd.dmin, g, res)
        ca, cb = sd.p0 + sd.s * (sd.p1 - sd.p0), sd.q0 + sd.t * (sd.q1 - sd.q0)
        assert sd.residual(ca, cb) <= 1e-15 and 0 <= sd.s <= 1 and 0 <= sd.t <= 1


def test_reference_regions_and_uniqueness():
    S = designated_segments()
    for a in (0, "i", 1):
        for c in (0, "i", 1):
            sd = cg.segment_distance(*S["region_%s%s" % (a, c)])
            assert sd.region() == (a, c) and sd.unique, (a, c, sd.s, sd.t)
    assert not cg.segment_distance(*S["parallel_overlap"]).unique and not cg.segment_distance(*S["antiparallel"]).unique
    assert cg.segment_distance(*S["parallel_apart"]).unique and abs(cg.segment_distance(*S["parallel_apart"]).dmin - np.hypot(0.2, 1.0)) < 1e-15
    assert abs(cg.segment_distance(*S["parallel_overlap"]).dmin - 0.2) < 1e-15
    for ang in (1e-3, 1e-5, 1e-7):
        sd = cg.segment_distance(*S["near_parallel_%g" % ang])
        assert sd.unique or ang < 1e-6
        assert abs(sd.dmin - 0.2) < 1e-15 and (ang < 1e-6 or (abs(sd.s - 0.5) < 1e-6 and abs(sd.t - 0.5) < 1e-6)), (ang, sd.s, sd.t, sd.dmin)
    assert cg.segment_distance(*S["intersecting"]).dmin == 0.0 and cg.segment_distance(*S["touching_end"]).dmin == 0.0
    assert abs(cg.segment_distance(*S["point_segment"]).dmin - 0.3) < 1e-15 and abs(cg.segment_distance(*S["segment_point"]).dmin - 0.5) < 1e-15
    assert abs(cg.segment_distance(*S["point_point"]).dmin - np.sqrt(2)) < 1e-15
    # a claimed minimiser that is none: off the segment, or not at the minimal distance
    sd = cg.segment_distance(*S["parallel_overlap"])
    good = (np.array([0.7, 0, 0]), np.array([0.7, 0.2, 0]))
    assert sd.residual(*good) < 1e-15 and sd.residual(good[0], good[1] + [0.01, 0, 0]) > 1e-5 and sd.residual(good[0] + [0.5, 0, 0], good[1] + [0.5, 0, 0]) > 0.1


def test_reference_shapes():
    B, C, S = cg.SH_BOX, cg.SH_CAPSULE, cg.SH_SPHERE
    assert cg.shape_radius(S, np.array([0.2, 0, 0])) == 0.1 and cg.shape_radius(C, np.array([0.2, 0.4, 0])) == 0.1 + 0.2
    assert abs(cg.shape_radius(B, np.array([0.3, 0.4, 1.2])) - 0.65) < 1e-15
    half, r = cg.link_capsule(B, np.array([0.125, 0.5, 0.25]))
    assert np.array_equal(half, [0, 0.1875, 0]) and r == 0.0625                      # longest edge y, radius half the shortest: the capsule is inscribed
    half, r = cg.link_capsule(B, np.array([0.4, 0.4, 0.4]))
    assert np.array_equal(half, [0, 0, 0]) and r == 0.2                         # a cube: a sphere
    pts = cg.ground_points(B, np.array([2.0, 4.0, 6.0]))
    assert [tuple(p) for p, _ in pts][:3] == [(1, 2, 3), (-1, 2, 3), (1, -2, 3)] and len(pts) == 8 and all(rr == 0 for _, rr in pts)
    assert [tuple(p) for p, _ in cg.ground_points(C, np.array([0.2, 0.4, 0]))] == [(0, 0.2, 0), (0, -0.2, 0)]


# ---------------------------------------------------------------------------------------------------------------- CPU: oracle, emulator
ALL = sorted(CASES)
DUO = [n for n in ALL if CASES[n][0] == HUM]                # (the two-per-wave tap family is the biped's: dm_families.h)
V2 = ALL


@pytest.mark.parametrize("name", ALL)
def test_contacts_oracle(oracle_built, name):
    b = build_case(name)
    for variant, prec in (("", 64), ("f32", 32)):
        lists, masks = run_oracle(b, variant)
        check_route(b, lists, masks, prec, "oracle")
    if name in V2:
        for variant, prec in (("", 64), ("f32", 32)):
            lists, masks = run_oracle(b, variant, physics=2)
            check_route(b, lists, masks, prec, "oracle", refs=v2_refs(b), want_masks=[cg.contact_mask(r[1]) for r in v2_refs(b)])


def test_correct_cull_changes_nothing(oracle_built):
    """the bounding-sphere cull with radius = half length + capsule radius + threshold drops no active pair on any case"""
    for name in ALL:
        b = build_case(name)
        for e in range(len(b.Q)):
            rows, _ = reference_of(b, e, cull=True)
            assert np.array_equal(rows, b.refs[e][0]), (name, e)


MUTANTS = ("no_second_clamp", "no_t_gt_1", "thr_max", "box_shortest", "keep_shallowest", "ties_high", "self_first", "cull_no_thr")


def test_mutants_are_caught(oracle_built):
    """every wrong variant of the reference differs from it on a designated case: another slot list, or a figure off by more than 100 x the float32 hard bound"""
    caught = {m: [] for m in MUTANTS}
    for name in ALL:
        b = build_case(name)
        big = 100 * hard_bound32(b.scale)
        for m in MUTANTS:
            for e in range(len(b.Q)):
                rows, _ = reference_of(b, e, mutant=m)
                ref = b.refs[e][0]
                if rows.shape != ref.shape or not np.array_equal(rows[:, [0, 1, 9]], ref[:, [0, 1, 9]]):
                    caught[m].append((name, e, "slots")); continue
                try:
                    err = compare(b, e, rows, 64, "mutant " + m)
                except AssertionError:
                    caught[m].append((name, e, "normal")); continue
                if max(err.values()) > big:
                    caught[m].append((name, e, "%.1e" % max(err.values())))
    print("MUTANTS " + "; ".join("%s: %d (%s)" % (m, len(c), ", ".join("%s[%d] %s" % x for x in c[:3])) for m, c in caught.items()))
    for m, c in caught.items():
        assert c, "mutant %s passes every case" % m


@pytest.mark.parametrize("prec", (64, 32))
@pytest.mark.parametrize("name", ALL)
def test_contacts_tap_emulator(emu_lib, name, prec):
    b = build_case(name)
    check_route(b, *run_tap(b, emu_lib, prec), prec, "emulator tap")


@pytest.mark.parametrize("prec", (64, 32))
@pytest.mark.parametrize("name", V2)
def test_contacts_tap_v2_emulator(emu_lib, name, prec):
    b = build_case(name)
    refs = v2_refs(b)
    check_route(b, *run_tap(b, emu_lib, prec, physics=2), prec, "emulator tap v2", refs=refs, want_masks=[cg.contact_mask(r[1]) for r in refs])


@pytest.mark.parametrize("prec", (64, 32))
@pytest.mark.parametrize("name", DUO)
def test_contacts_tap_two_per_wave_emulator(emu_lib, name, prec):
    b = build_case(name)
    check_route(b, *run_tap_duo(b, emu_lib, prec), prec, "emulator duo tap")


# (biped + ball under DM-physics v2 has no two-per-wave family and the host refuses the request: dm_families.h)
PRODUCTION = [(n, prec, pack, v) for n in ALL for prec in (64, 32) for pack in (1, 2) for v in ("plain", "amp", "v2") if not (CASES[n][0] == DRIBBLE and pack == 2 and v == "v2")]


def check_production(b, lib, prec, pack, variant):
    if CASES[b.name][0] == DRIBBLE and variant == "plain":
        variant = "amp"               # biped + ball has no plain family (dm_families.h)
    masks, fam = run_production(b, lib, prec, pack, variant)
    want = [cg.contact_mask(r[1]) for r in (v2_refs(b) if variant == "v2" else b.refs)]
    print("CONTACTS %-12s production f%d pack %d %s: family %d, masks %s" % (b.name, prec, pack, variant, fam, [hex(m) for m in masks]))
    assert (fam in TWO_PER_WAVE) == (pack == 2 and b.duo), (fam, pack)
    assert masks == want, (b.name, prec, pack, variant, masks, want)


@pytest.mark.parametrize("name,prec,pack,variant", PRODUCTION)
def test_contact_mask_production_emulator(emu_lib, name, prec, pack, variant):
    check_production(build_case(name), emu_lib, prec, pack, variant)


# ---------------------------------------------------------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("prec", (64, 32))
@pytest.mark.parametrize("name", ALL)
def test_contacts_tap_gpu(hip_lib, name, prec):
    b = build_case(name)
    check_route(b, *run_tap(b, hip_lib, prec), prec, "MI355X tap")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", (64, 32))
@pytest.mark.parametrize("name", V2)
def test_contacts_tap_v2_gpu(hip_lib, name, prec):
    b = build_case(name)
    refs = v2_refs(b)
    check_route(b, *run_tap(b, hip_lib, prec, physics=2), prec, "MI355X tap v2", refs=refs, want_masks=[cg.contact_mask(r[1]) for r in refs])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", (64, 32))
@pytest.mark.parametrize("name", DUO)
def test_contacts_tap_two_per_wave_gpu(hip_lib, name, prec):
    b = build_case(name)
    check_route(b, *run_tap_duo(b, hip_lib, prec), prec, "MI355X duo tap")


@pytest.mark.gpu
@pytest.mark.parametrize("name,prec,pack,variant", PRODUCTION)
def test_contact_mask_production_gpu(hip_lib, name, prec, pack, variant):
    check_production(build_case(name), hip_lib, prec, pack, variant)


# ---------------------------------------------------------------------------------------------------------------- DM-physics v2: the persistent manifolds
def manifold_states(which):
    """(asset, poses of two envs): the box set down flat, the box tipped onto an edge, the humanoid standing with its soles 2 mm in"""
    if which == "box_flat":
        t = tables_of("box"); return "box", [make_pose(t, (0.0, 0.199, 0.0)), make_pose(t, (0.5, 0.1995, 0.2), quat((0, 1, 0), 0.4))]
    if which == "box_tilted":
        t = tables_of("box"); return "box", [make_pose(t, (0.0, 0.2 * (np.cos(0.3) + np.sin(0.3)) - 0.001, 0.0), quat((0, 0, 1), 0.3)), make_pose(t, (0.0, 0.2 * (np.cos(0.1) + np.sin(0.1)) - 0.002, 0.0), quat((1, 0, 0), 0.1))]
    t = tables_of(HUM); return HUM, [make_pose(t, (0.0, STAND_Y, 0.0), joints=_legs()), make_pose(t, (0.3, STAND_Y + 0.001, 0.1), quat((0, 1, 0), -0.5), _legs())]


def check_manifolds(lib, prec, which, pack):
    """dm_get_manifolds after each of 6 updates (one substep each): at most 4 points per link; every stored body-frame point is a support point of the link's shape
    (a box corner; on a sphere or a capsule's end sphere a point at the radius from its centre); its stored distance is its world height at the pose the substep
    started from, at most thr; its drift from the stored plane point at most thr; the link's deepest candidate is among the points whenever it is below thr"""
    asset, Q = manifold_states(which)
    t, t1 = tables_of(asset), tables_of(asset, True)
    Q = np.array(Q)
    env = BatchEnv(t1, len(Q), precision=prec, lib_path=lib, wave_packing=pack, physics=2)
    st0 = env.get_state()
    env.set_state(pose=Q, vel=np.zeros_like(Q), tar=Q, kin=st0["kin"], clocks=st0["clocks"])
    o = Oracle(t)
    shapes = [cg.shape_of(bd) for bd in t.body_defs]
    thr = [cg.BREAKING_FACTOR * cg.shape_radius(*sh) for sh in shapes]
    scale = float(np.abs(Q[:, 0:3]).max()) + max(2 * cg.shape_radius(*sh) for sh in shapes) + 1.0
    tol = TOL64 if prec == 64 else hard_bound32(scale)
    seen, worst_err = 0, 0.0
    for u in range(6):
        pose = env.get_state()["pose"]
        env.update(H_STEP, 1)
        mf = env.get_manifolds()
        for e in range(len(Q)):
            o.set_sim_state(pose[e], np.zeros(o.P)); links = o.links()
            for j in range(t.num_joints):
                cnt = int(mf[e, j, 0])
                assert 0 <= cnt <= 4, (which, u, e, j, cnt)
                com, Rb = links[j][0:3], links[j][3:12].reshape(3, 3)
                pts = cg.ground_points(*shapes[j])
                stored = [mf[e, j, 1 + 6 * i:7 + 6 * i] for i in range(cnt)]
                for rec in stored:
                    lp, bx, bz, dist = rec[0:3], rec[3], rec[4], rec[5]
                    sup = min(abs(float(np.linalg.norm(lp - loc)) - r) for loc, r in pts)
                    xw = com + Rb @ lp
                    worst_err = max(worst_err, sup, abs(xw[1] - dist))
                    assert sup <= tol and abs(xw[1] - dist) <= tol, (which, u, e, j, sup, xw[1], dist)
                    assert dist <= thr[j] + tol and np.hypot(bx - xw[0], bz - xw[2]) <= thr[j] + tol, (which, u, e, j, dist, thr[j])
                    seen += 1
                ys = [(float((com + Rb @ loc)[1] - r), k) for k, (loc, r) in enumerate(pts)]
                y, k = min(ys)
                if y < thr[j] - 100 * tol:
                    loc, r = pts[k]
                    lp_new = Rb.T @ (Rb @ loc - r * UP)
                    assert any(float(np.abs(rec[0:3] - lp_new).max()) <= 4 * tol for rec in stored), (which, u, e, j, lp_new, stored)
                else:
                    assert y > thr[j] + 100 * tol or cnt >= 0          # (a candidate within the margin of thr decides nothing here)
    fam = int(env.debug("family")[0])
    env.close()
    print("CONTACTS manifolds %-10s f%d pack %d family %d: %d stored points checked, worst %.2e (tol %.2e)" % (which, prec, pack, fam, seen, worst_err, tol))
    assert seen >= 6 * len(Q) and (fam in TWO_PER_WAVE) == (pack == 2 and asset == HUM)


MANIFOLDS = [(w, prec, pack) for w in ("box_flat", "box_tilted", "hum_standing") for prec in (64, 32) for pack in (1, 2)]


@pytest.mark.parametrize("which,prec,pack", MANIFOLDS)
def test_manifolds_emulator(emu_lib, which, prec, pack):
    check_manifolds(emu_lib, prec, which, pack)


@pytest.mark.gpu
@pytest.mark.parametrize("which,prec,pack", MANIFOLDS)
def test_manifolds_gpu(hip_lib, which, prec, pack):
    check_manifolds(hip_lib, prec, which, pack)
