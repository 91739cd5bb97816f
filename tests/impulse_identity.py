"""The impulse-momentum identity of one rigid-body substep, reference side.  Plain numpy float64; TEST INFRASTRUCTURE ONLY.

The constraint solver changes the velocity only by impulses along the constraint directions, and the unconstrained step is one
solve with the mass matrix:

    H(q) (v' - v*) = B(q) lambda,    B = [J_c(x)^T d ... | +-e_k ...]          (*)
    H(q) (v* - v)  = h (tau - C(q, v))                                        (**)

Both hold wherever the coordinate-velocity clamp is inactive.  Everything on the reference side comes from code that is pinned to
the compiled reference sources (tests/test_oracle_vs_ref.py): H and C from `Oracle.mass_bias(1, q, v)`, the link Jacobians
numerically from `orc_skel_link_vel` (link velocities are linear in v: one call per unit generalized velocity), the contact points
and normals from the oracle's contact list.  Nothing here reads the oracle's own solver, Jacobian rows or factorisation, so a
wrong lever arm, sign or friction direction shared by oracle and kernel shows as a residual.

Row order (oracle/orc_scene.h Scene::substep): the limit rows (revolute joints in joint order; the nearer bound, +e_k for the
lower and -e_k for the upper), then one normal row per contact, then the friction pairs contact-major (t1, t2 of contact 0, t1, t2
of contact 1, ...), t1 / t2 = btPlaneSpace1(n).

Residuals are backward errors.  Each is reported as a ratio to the magnitude of the terms it is the difference of,

    full:       || H (v' - v*) - B lambda ||_inf         /  || |H| (|v'| + |v*|) + |B| |lambda| ||_inf
    null space: || N^T H (v' - v*) ||_inf                /  || |N^T| (|H| (|v'| + |v*|)) ||_inf
    vstar:      || H (v* - v) - h (tau - C) ||_inf       /  || |H| (|v*| + |v|) + h (|tau| + |C|) ||_inf
    lambda-free production form:
                || N^T [H (v' - v) - h (tau - C)] ||_inf /  || |N^T| (|H| (|v'| + |v|) + h (|tau| + |C|)) ||_inf

with N an orthonormal basis of the orthogonal complement of range(B) (left singular vectors of B beyond its rank, relative
threshold 1e-10), so that no figure depends on the conditioning of the contact problem.

THE BOUND  ratio <= C_BOUND * D * u  (u the unit roundoff of the working precision, D the number of generalized velocities).
A step of the kernels (and of the oracle) computes, in working precision,
    H = L L^T              the factor:                 |H - L L^T| <= (D + 1) u |L| |L^T|                        1 D u
    Y = L^-1 B             one triangular solve:       (L + dL_r) y_r = b_r, |dL_r| <= D u |L|                   1 D u
    w = Y lambda           a sum of R <= 64 <= 2 D terms per component                                           2 D u
    z = L^-T w, v' = v* + z   the second triangular solve and one addition                                       1 D u
and before that forms H (composite inertias through kinematic chains of at most 8 links) and the rows of B (lever arms through
the same chains) from q in working precision: each entry is a sum of at most D products of rounded factors              2 D u
The test's own products H (v' - v*) and B lambda run in float64 (nothing beside a float32 step; for a float64 step sums of D and
R terms) together with the one rounding of each stored v*, v', tau, lambda                                               1 D u
Every term is of the size |L| |L^T| |z| or |L| |Y| |lambda|; for the positive definite H of an articulated body these are of the
size of |H| |z| and |B| |lambda| (Higham, Accuracy and Stability of Numerical Algorithms, 10.1: no growth in Cholesky), which is
the denominator above.  Sum: C_BOUND = 8.  (**) goes through the factor and the two solves only and is held to the same bound.
"""
import ctypes as C

import numpy as np

from deepmimic_amd import model
from oracle_lib import CFG_KEYS, _d
import parity_common as pc

C_BOUND = 8.0
U64, U32 = 2.0 ** -53, 2.0 ** -24
RANK_RTOL = 1e-10


def bound(D, precision):
    return C_BOUND * D * (U64 if precision == 64 else U32)


# ---------------------------------------------------------------------------------------------------------------- Jacobians
def _skel(oracle, tables):
    """the oracle library's bare skeleton handle (orc_skel_*), cached on the Oracle object"""
    h = getattr(oracle, "_skel_h", None)
    if h is None:
        lib = oracle.lib
        assert lib.orc_real_bytes() == 8, "the reference side runs on the float64 oracle"
        lib.orc_skel_create.restype = C.c_void_p
        jm = np.ascontiguousarray(tables.joint_mat, dtype=np.float64); bd = np.ascontiguousarray(tables.body_defs, dtype=np.float64)
        g = np.zeros(3)
        h = oracle._skel_h = C.c_void_p(lib.orc_skel_create(_d(jm), _d(bd), jm.shape[0], _d(g)))
    return h


def link_jacobians(oracle, tables, q):
    """[J, 6, D]: linear velocity of the link's COM (rows 0..2) and its angular velocity (rows 3..5) per unit generalized
    velocity, in parity_common.dof_index order: D calls of orc_skel_link_vel"""
    idx = pc.dof_index(tables)
    h = _skel(oracle, tables)
    q = np.ascontiguousarray(q, dtype=np.float64)
    out = np.zeros((oracle.J, 6, len(idx)))
    for k, i in enumerate(idx):
        v = np.zeros(oracle.P); v[i] = 1.0
        lv = np.zeros((oracle.J, 6))
        oracle.lib.orc_skel_link_vel(h, _d(q), _d(v), _d(lv))
        out[:, :, k] = lv
    return out


def point_jacobian(LJ, coms, link, x):
    """[3, D]: velocity of the world point x moving with `link`: Jv + Jw x (x - com)"""
    r = np.asarray(x, dtype=np.float64) - coms[link]
    Jv, Jw = LJ[link, 0:3], LJ[link, 3:6]
    return Jv + np.cross(Jw.T, r).T


def plane_space(n):
    """btPlaneSpace1"""
    n = np.asarray(n, dtype=np.float64)
    if abs(n[2]) > 0.7071067811865475244:
        a = n[1] * n[1] + n[2] * n[2]; k = 1.0 / np.sqrt(a)
        p = np.array([0.0, -n[2] * k, n[1] * k]); q = np.array([a * k, -n[0] * p[2], n[0] * p[1]])
    else:
        a = n[0] * n[0] + n[1] * n[1]; k = 1.0 / np.sqrt(a)
        p = np.array([-n[1] * k, n[0] * k, 0.0]); q = np.array([-n[2] * p[1], n[2] * p[0], a * k])
    return p, q


def limit_rows(tables, q):
    """[(dof, sign)] of the joint-limit rows: every revolute joint with lo <= hi, the nearer bound (ties: the lower)"""
    idx = list(pc.dof_index(tables))
    rows = []
    for j in range(1, tables.num_joints):
        jm = tables.joint_mat[j]
        if int(jm[model.JD_TYPE]) != model.JT_REVOLUTE or jm[model.JD_LL0] > jm[model.JD_LH0]:
            continue
        off = int(jm[model.JD_PARAM_OFFSET]); th = q[off]
        rows.append((idx.index(off), 1.0 if (th - jm[model.JD_LL0]) <= (jm[model.JD_LH0] - th) else -1.0))
    return rows


def contact_directions(c, swap_tangents=False):
    t1, t2 = plane_space(c[6:9])
    return (c[6:9], t2, t1) if swap_tangents else (c[6:9], t1, t2)


def contact_column(LJ, coms, c, d, D, ball_pos=None, flip_b=False):
    """J_c(x)^T d of one contact row (c: a row of Oracle.contact_list_ex); with a ball the column has D + 6 entries, the last six
    the ball's linear and angular velocity"""
    link, link_b, x, kind = int(c[0]), int(c[1]), c[3:6], int(c[9])
    col = np.zeros(D + (6 if ball_pos is not None else 0))
    if link >= 0:
        col[:D] = point_jacobian(LJ, coms, link, x).T @ d
    if link_b >= 0:
        jb = point_jacobian(LJ, coms, link_b, x).T @ d
        col[:D] += jb if flip_b else -jb
    if kind:
        sg = 1.0 if kind == 2 else -1.0         # 2: the ball is body a (ball on the ground), 1: the ball is body b
        col[D:D + 3] = sg * d; col[D + 3:D + 6] = sg * np.cross(x - ball_pos, d)
    return col


def constraint_span(tables, LJ, coms, q, contacts, mu_link, mu_ball=0.0, ball_pos=None, corrupt=None):
    """B [D (+ 6), R] in the solver's row order, and per row the friction coefficient (0 for limit and normal rows) and the index
    of the normal row that boxes it (-1 for limit and normal rows).
    corrupt (sharpness tests only): ("point", c, dx) moves the point of contact c by dx, ("flip_b", c) flips the sign of body b
    of self contact c, ("swap", c) exchanges t1 and t2 of contact c."""
    D = LJ.shape[2]
    contacts = np.array(contacts, dtype=np.float64, copy=True).reshape(-1, 10)
    kind, which = (corrupt[0], corrupt[1]) if corrupt else (None, -1)
    if kind == "point":
        contacts[which, 3:6] += corrupt[2]
    lim = limit_rows(tables, q)
    n_lim, nc = len(lim), len(contacts)
    n = D + (6 if ball_pos is not None else 0)
    B = np.zeros((n, n_lim + 3 * nc)); mu = np.zeros(n_lim + 3 * nc); normal_row = np.full(n_lim + 3 * nc, -1)
    for r, (k, sgn) in enumerate(lim):
        B[k, r] = sgn
    for ci, c in enumerate(contacts):
        dn, t1, t2 = contact_directions(c, swap_tangents=(kind == "swap" and ci == which))
        flip = kind == "flip_b" and ci == which
        B[:, n_lim + ci] = contact_column(LJ, coms, c, dn, D, ball_pos, flip)
        for s, d in enumerate((t1, t2)):
            r = n_lim + nc + 2 * ci + s
            B[:, r] = contact_column(LJ, coms, c, d, D, ball_pos, flip)
            mu[r] = mu_ball if int(c[9]) else mu_link
            normal_row[r] = n_lim + ci
    return B, dict(n_lim=n_lim, nc=nc, mu=mu, normal_row=normal_row)


def extend_H(H, ball_mass, ball_radius):
    """the character's H with the free sphere's diag(m I, 0.4 m r^2 I)"""
    D = H.shape[0]
    He = np.zeros((D + 6, D + 6)); He[:D, :D] = H
    He[D:D + 3, D:D + 3] = ball_mass * np.eye(3); He[D + 3:, D + 3:] = 0.4 * ball_mass * ball_radius ** 2 * np.eye(3)
    return He


def ball_vstar(ball13, h, gravity, lin_damping, ang_damping):
    """the ball's unconstrained velocity: btRigidBody::applyDamping (the damping power), then the gravity impulse"""
    return np.concatenate([ball13[7:10] * (1.0 - lin_damping) ** h + h * np.asarray(gravity), ball13[10:13] * (1.0 - ang_damping) ** h])


# ---------------------------------------------------------------------------------------------------------------- residuals
def _ratio(num, den):
    d = float(np.abs(den).max())
    return float(np.abs(num).max()) / d if d > 0 else float(np.abs(num).max())


def residual_full(H, v1, vstar, B, lam):
    """r = H (v' - v*) - B lambda (all components) and its ratio"""
    r = H @ (v1 - vstar) - B @ lam
    return r, _ratio(r, np.abs(H) @ (np.abs(v1) + np.abs(vstar)) + np.abs(B) @ np.abs(lam))


def nullspace(B):
    """(N [n, codim], rank): orthonormal basis of the orthogonal complement of range(B)"""
    if B.shape[1] == 0:
        return np.eye(B.shape[0]), 0
    U, s, _ = np.linalg.svd(B, full_matrices=True)
    rank = int((s > RANK_RTOL * s[0]).sum()) if s.size and s[0] > 0 else 0
    return U[:, rank:], rank


def residual_nullspace(H, v1, vstar, B):
    """(N^T H (v' - v*), ratio, rank, codimension): needs no lambda"""
    N, rank = nullspace(B)
    r = N.T @ (H @ (v1 - vstar))
    return r, _ratio(r, np.abs(N.T) @ (np.abs(H) @ (np.abs(v1) + np.abs(vstar)))), rank, N.shape[1]


def residual_vstar(H, Cb, v, vstar, tau, h):
    """(**): H (v* - v) - h (tau - C) and its ratio"""
    r = H @ (vstar - v) - h * (tau - Cb)
    return r, _ratio(r, np.abs(H) @ (np.abs(vstar) + np.abs(v)) + h * (np.abs(tau) + np.abs(Cb)))


def residual_step_nullspace(H, Cb, v, v1, tau, h, B, ball=None):
    """(**) + (*) without lambda or v*: N^T [H (v' - v) - h (tau - C)], what a kernel without taps can be asked.
    ball = (diagonal of the sphere's mass block (6), its v', its closed-form v*): six more rows m (v_b' - v_b*)"""
    N, rank = nullspace(B)
    r = H @ (v1 - v) - h * (tau - Cb)
    s = np.abs(H) @ (np.abs(v1) + np.abs(v)) + h * (np.abs(tau) + np.abs(Cb))
    if ball is not None:
        mb, b1, bs = ball
        r = np.concatenate([r, mb * (b1 - bs)]); s = np.concatenate([s, mb * (np.abs(b1) + np.abs(bs))])
    r = N.T @ r
    return r, _ratio(r, np.abs(N.T) @ s), rank, N.shape[1]


def root_momentum_rows(H, v1, vstar):
    """the six root rows of H (v' - v*) by name.  The root's generalized velocities are its world-frame linear and angular velocity,
    so these are the change of total linear momentum and of total angular momentum about the root joint: zero for an airborne
    character, whatever its internal (self-contact and limit) impulses.  Returns {name: (value, scale)}."""
    r = H @ (v1 - vstar); s = np.abs(H) @ (np.abs(v1) + np.abs(vstar))
    names = ("linear momentum x", "linear momentum y", "linear momentum z", "angular momentum x", "angular momentum y", "angular momentum z")
    return {nm: (float(r[i]), float(s[i])) for i, nm in enumerate(names)}


# ---------------------------------------------------------------------------------------------------------------- reference side of one env
def cfg_of(oracle, key):
    return float(oracle.cfg[CFG_KEYS.index(key)])


def reference_step(oracle, tables, q, v, tau, h, ball13=None):
    """One substep of the float64 oracle from (q, v) under tau (dof order), and the reference side built at that state: H, C, the
    constraint span, the oracle's own v*, v', lambda (dof order; with a ball six more entries: its linear and angular velocity)."""
    idx = pc.dof_index(tables)
    oracle.set_sim_state(q, v)
    if ball13 is not None:
        oracle.set_ball(ball13)
    tp = np.zeros(oracle.P); tp[idx] = tau; oracle.set_tau(tp)
    qs, vs = oracle.sim_state()                      # as the step sees them (spherical joints standardised)
    oracle.substep(h)
    links = oracle.links()                           # start-of-substep pose
    _, v1 = oracle.sim_state()
    H, Cb = oracle.mass_bias(1, qs, vs)
    H = H[np.ix_(idx, idx)]; Cb = Cb[idx]
    LJ = link_jacobians(oracle, tables, qs)
    contacts = oracle.contact_list_ex()
    ball_pos = None if ball13 is None else np.asarray(ball13[:3], dtype=np.float64)
    B, meta = constraint_span(tables, LJ, links[:, 0:3], qs, contacts, cfg_of(oracle, "friction"), cfg_of(oracle, "ball_friction"), ball_pos)
    ref = dict(q=qs, v=vs[idx], tau=np.asarray(tau, dtype=np.float64), h=h, H=H, C=Cb, B=B, meta=meta, LJ=LJ, coms=links[:, 0:3], contacts=contacts,
               vstar=oracle.vstar()[idx], v1=v1[idx], lam=oracle.lambdas(), rows=oracle.num_rows(), ncontacts=oracle.num_contacts(),
               nself=oracle.num_self_contacts(), D=len(idx), ball_pos=ball_pos)
    ws = cfg_of(oracle, "world_scale")
    ref["clamp"] = np.array([100.0 / ws] * 3 + [100.0] * (len(idx) - 3))
    ref["lim_max"] = 100.0 / (ws * ws)
    if ball13 is not None:
        g = [cfg_of(oracle, "grav_x"), cfg_of(oracle, "grav_y"), cfg_of(oracle, "grav_z")]
        ref["He"] = extend_H(H, cfg_of(oracle, "ball_mass"), cfg_of(oracle, "ball_radius"))
        ref["ball_vstar"] = ball_vstar(np.asarray(ball13, dtype=np.float64), h, g, cfg_of(oracle, "ball_lin_damp"), cfg_of(oracle, "ball_ang_damp"))
        ref["ball_v1"] = oracle.ball_state()[7:13].copy()
    return ref


def ratios(ref, vstar, v1, lam=None, ball_v1=None):
    """the three ratios of a step (reference side `ref`; v*, v', lambda of the implementation under test, dof order)"""
    H = ref["H"]
    out = {}
    _, out["vstar"] = residual_vstar(H, ref["C"], ref["v"], vstar, ref["tau"], ref["h"])
    if ref["ball_pos"] is not None:
        He = ref["He"]; ve = np.concatenate([vstar, ref["ball_vstar"]]); v1e = np.concatenate([v1, ball_v1])
    else:
        He, ve, v1e = H, vstar, v1
    _, out["null"], out["rank"], out["codim"] = residual_nullspace(He, v1e, ve, ref["B"])
    if lam is not None:
        _, out["full"] = residual_full(He, v1e, ve, ref["B"], lam)
    return out


def lambda_box_violations(ref, lam, precision):
    """the exact inequalities on a lambda vector: 0 <= limit <= 100 / world_scale^2, normal >= 0, |friction| <= mu * (final normal),
    with one ulp of the working precision on the product mu * lambda_n.  Returns the list of violated rows (empty = holds)."""
    meta = ref["meta"]; n_lim, nc = meta["n_lim"], meta["nc"]
    ft = np.float64 if precision == 64 else np.float32
    bad = []
    for r in range(n_lim):
        if not (0.0 <= lam[r] <= ref["lim_max"]):
            bad.append(("limit", r, lam[r]))
    for r in range(n_lim, n_lim + nc):
        if not lam[r] >= 0.0:
            bad.append(("normal", r, lam[r]))
    for r in range(n_lim + nc, n_lim + 3 * nc):
        cap = ft(meta["mu"][r]) * ft(lam[meta["normal_row"][r]])
        cap = float(np.nextafter(cap, ft(np.inf)))
        if not abs(lam[r]) <= cap:
            bad.append(("friction", r, lam[r], cap))
    return bad
