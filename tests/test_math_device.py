"""The helpers of deepmimic_amd/csrc/dm_math.h, one at a time, at the inputs on which they branch -- through dm_math_probe (include/dm_hip.h,
deepmimic_amd/csrc/dm_math_probe.h), which runs ONE dmk:: helper per launch on rows of the caller's inputs, in float or in double.

Every case runs on the emulator library (the same source under g++) and, marked gpu, on libdm_hip.so, in both precisions.  The reference is plain numpy float64 written
here, evaluated on the inputs AFTER they were rounded to the helper's type, so only the helper's own arithmetic is measured.

Tolerances are forward-error bounds written next to each case, c_op * u * scale with u = 2^-24 (float) or 2^-53 (double):
  * a sum of products is held to gamma_k * S, gamma_k = k u / (1 - k u), k = the longest chain of roundings in the helper's expression and S the same expression
    evaluated on absolute values with every subtraction turned into an addition (`absval`) -- the textbook running bound, it holds for any association and for any
    choice of fused multiply-adds;
  * sqrt and division count 1 ulp = 2 u, the libm calls (sin, cos, atan2, acos) the 2 ulp = 4 u that ROCm documents for them; fmod is exact;
  * in double the reference is as inexact as the helper: each libm term counts 3 ulp there (`LIBM`) and every other rounding twice (`R`);
  * a wrapped angle carries the distance of the type's 2 pi from the real one (`D2PI`: 1.75e-7 in float = 0.37 ulp(2 pi)) once per turn taken off;
  * dm_sincos (float): see `sincos_bounds`.
None of them comes from what the helpers returned.  Each check prints its worst error and worst error / bound (pytest -s); docs/HISTORY.md section 20 tabulates them.

Where float and double may legitimately take different branches (the eps of quat_to_rotvec, the 1e-4 of quat_theta, 1e-6 of the exponentials) inputs whose float64
discriminant lies within 8 ulp(Real) of the threshold are dropped, and the case asserts that this is under 1 % of its rows (in fact none: the inputs keep clear).
qslerp and an angle on +-pi need no exclusion: either branch is right there and the comparison says so (up to the quaternion's sign / modulo 2 pi; for qslerp the
bound is widened by the distance between the reference's two branches, about theta^2 / 16)."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from deepmimic_amd import math_probe as mp
from deepmimic_amd.core import load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = {0: 2.0 ** -24, 1: 2.0 ** -53}
REAL = {0: np.float32, 1: np.float64}
LIBM = {0: 4.0, 1: 6.0}                     # units of u per libm call: 2 ulp of the helper's (+ 1 ulp of the reference's own in double)
# the unit of every other rounding: in double the float64 reference rounds the same expression as often as the helper does (and, without fused multiply-adds,
# differently), so each rounding counts twice; against a float helper the reference's own error is 2^-29 of the bound
R = {0: U[0], 1: 2 * U[1]}
PI, TWO_PI = np.pi, 2 * np.pi
# |2 pi as the type holds it - 2 pi|: float from the double (exact enough), double from the next digits of pi
D2PI = {0: abs(float(np.float32(TWO_PI)) - TWO_PI), 1: 2.4492935982947064e-16}
PI_FRAC = Fraction("3.14159265358979323846264338327950288419716939937510582097494459")
MAX_ROWS = 65536


# ---------------------------------------------------------------- plumbing
def rnd(x, f64):
    """x as the helper's type holds it, widened back"""
    return np.asarray(x, np.float64).astype(REAL[f64]).astype(np.float64)


def neighbour(x, f64, steps):
    """the value `steps` representable numbers of the helper's type away from x"""
    v = np.asarray(x, np.float64).astype(REAL[f64])
    to = REAL[f64](np.inf if steps > 0 else -np.inf)
    for _ in range(abs(steps)):
        v = np.nextafter(v, to)
    return v.astype(np.float64)


def ulp(x, f64):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(REAL[f64])).astype(np.float64)


def gamma(k, f64):
    return k * R[f64] / (1 - k * R[f64])


class Probe:
    """rows [n, <= IN] float64 -> [n, OUT] float64 through dm_math_probe of `lib_path`; host arrays on the emulator, torch tensors on the GPU"""

    def __init__(self, lib_path, gpu):
        self.lib_path, self.gpu, self.name = lib_path, gpu, "gpu" if gpu else "emulator"

    def raw(self, op, f64, n, inp, fill=np.nan):
        rows = inp.shape[0]
        assert 1 <= rows <= MAX_ROWS and inp.shape[1] == mp.IN and inp.dtype == np.float64
        if self.gpu:
            import torch
            d_in = torch.from_numpy(np.ascontiguousarray(inp)).cuda()
            d_out = torch.full((rows, mp.OUT), float(fill), dtype=torch.float64, device="cuda")
            mp.math_probe(op, f64, n, d_in.data_ptr(), d_out.data_ptr(), stream=int(torch.cuda.current_stream().cuda_stream), lib_path=self.lib_path)
            torch.cuda.synchronize()
            return d_out.cpu().numpy()
        inp = np.ascontiguousarray(inp)
        out = np.full((rows, mp.OUT), fill, np.float64)
        mp.math_probe(op, f64, n, inp.ctypes.data, out.ctypes.data, lib_path=self.lib_path)
        return out

    def __call__(self, op, f64, *cols):
        """cols: arrays [n] or [n, k], laid side by side into the row"""
        cols = [np.asarray(c, np.float64).reshape(len(c), -1) for c in cols]
        n = cols[0].shape[0]
        inp = np.zeros((n, mp.IN))
        flat = np.concatenate(cols, axis=1)
        inp[:, :flat.shape[1]] = flat
        out = self.raw(op, f64, n, inp)
        assert np.isfinite(out).all(), "%s: a row was not written or is not finite" % op
        return out


def hold(probe, f64, what, err, bound, rows=None):
    """assert err <= bound elementwise; print the worst figures first"""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    assert err.size > 0 and np.isfinite(err).all() and np.isfinite(bound).all() and (bound >= 0).all(), what
    ratio = np.where(err > 0, err / np.where(bound > 0, bound, 1e-300), 0.0)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print("MATHDEV %-8s f%d %-34s rows %6d  worst |err| %.3e (%.2f u)  worst err/bound %.3f" %
          (probe.name, 64 if f64 else 32, what, err.shape[0], err.max(), err.max() / U[f64], ratio[i]))
    assert ratio[i] <= 1.0, "%s: |err| %.3e > bound %.3e at %s%s" % (what, err[i], bound[i], i, "" if rows is None else " input %r" % (rows[i[0]],))


def keep_clear(what, disc, threshold, f64):
    """mask of the rows whose float64 discriminant is more than 8 ulp(Real) away from `threshold`; at most 1 % may be dropped"""
    clear = np.abs(disc - threshold) > 8 * ulp(threshold, f64)
    dropped = 1.0 - clear.mean()
    print("MATHDEV excluded %-30s f%d %.4f %%" % (what, 64 if f64 else 32, 100 * dropped))
    assert dropped <= 0.01, "%s: %.2f %% of the rows lie on the threshold" % (what, 100 * dropped)
    return clear


class absval:
    """the arithmetic of a bound: every subtraction an addition, every negation dropped (operands are passed as absolute values)"""
    sub = staticmethod(np.add)
    neg = staticmethod(lambda a: a)


class exact:
    sub = staticmethod(np.subtract)
    neg = staticmethod(np.negative)


def value_and_scale(f, *args):
    return f(exact, *args), f(absval, *[np.abs(a) for a in args])


def unit_rows(rng, n, k):
    v = rng.standard_normal((n, k))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def axis_angle_quat(axis, angle):
    return np.concatenate([np.cos(0.5 * angle)[:, None], np.sin(0.5 * angle)[:, None] * axis], axis=1)


def exp_quat(rv):
    """exact exponential of a rotation vector in float64 (the series below 1e-4: its next term is th^4 / 3840)"""
    th = np.linalg.norm(rv, axis=1)
    k = np.where(th < 1e-4, 0.5 - th * th / 48.0, np.sin(0.5 * th) / np.where(th > 0, th, 1.0))
    return np.concatenate([np.cos(0.5 * th)[:, None], k[:, None] * rv], axis=1)


def mod_2pi(d):
    """|d| reduced by the nearest multiple of 2 pi"""
    return np.abs(d - TWO_PI * np.rint(d / TWO_PI))


# ---------------------------------------------------------------- dm_sincos, rot_y, rot_z
PIO2_HI = float(np.float32(PI / 2))                               # the first Cody-Waite constant of dm_sincos(float)
PIO2_MID = (PI / 2 - PIO2_HI) + 6.123233995736766e-17             # pi / 2 - PIO2_HI to double precision (-4.3711390e-8)
# what the three constants of the reduction leave of pi / 2 (the second and third as dm_math.h writes them): 6e-17 per quadrant
PIO2_RESIDUE = abs(-PIO2_MID - float(np.float32(4.3711388287e-08)) - float(np.float32(1.7763568394e-15)))


def sincos_bounds(x, f64, exact_first=True):
    """(sin x, cos x, bound on the sin, bound on the cos) for x already rounded to the type.
    double: libm.  float, dm_sincos: k = rint(x 2 / pi) and r = x - k pi / 2 the exact reduced argument (|r| <= pi / 4 + 2 u |k|); three fused steps reduce x:
      r1 = fl(x - k c1) with c1 = PIO2_HI: ONE rounding of the exact v1 = x - k c1 = r - k 4.37e-8, i.e. at most half an ulp of v1 (taken exactly, `e1`);
      r2, r3: one rounding each of a value of size |r|: 2 u |r|; the constants' own residue is |k| PIO2_RESIDUE;
    the error of r reaches the result times |dy/dr| <= 1.  The polynomial: its last fma rounds the result, u |y|; the terms inside are rounded products of size
    r^3 / 6 (sin), r^2 / 2 and r^4 / 24 (cos) with a handful of roundings each: u (|y| + 2 r^2) covers them (1 - r^2 / 2 <= |y| + r^2 for the cos).  Together
        |err| <= e1 + u (2 |y| + 2 |r| + 2 r^2)            <= 5.1 u for |x| <= 1e4,  and e1 + 4 u |r| <= u (5 |r| + |k| 4.4e-8) next to a zero of y.
    Where the float k may differ from the double one (|r| at pi / 4) v1 is a binade's width different at most: 1 % more.
    exact_first=False, for an argument that is itself only known to a few ulps: e1 as its own bound u |v1| <= u (|r| + |k| 4.3712e-8)."""
    s, c = np.sin(x), np.cos(x)
    if f64:
        return s, c, (LIBM[1] / 2) * ulp(s, 1), (LIBM[1] / 2) * ulp(c, 1)
    u = U[0]
    k = np.rint(x * (2 / PI))
    v1 = x - k * PIO2_HI                                           # exact in double: k has 13 bits, PIO2_HI 24
    r = np.abs(v1 - k * PIO2_MID)
    e1 = np.where(v1 != 0, np.ldexp(1.0, np.frexp(v1)[1] - 1 - 24), 0.0) if exact_first else 1.01 * u * (r + np.abs(k) * 4.3712e-8)
    common = (e1 + np.abs(k) * PIO2_RESIDUE + u * (2 * r + 2 * r * r)) * np.where(r > 0.78, 1.01, 1.0)
    return s, c, common + 2 * u * np.abs(s), common + 2 * u * np.abs(c)


def sincos_inputs(f64):
    """(a) k pi / 2 rounded to the type for every k in [-6400, 6400] with its +-1 and +-2 neighbours: the quadrant select at both signs of k and every value of
    k & 1, k & 2, (k + 1) & 2, on both sides of each boundary of the reduction; (b) +-0, the smallest denormal, 1e-30, 20 000 uniform draws in +-1e4"""
    base = rnd(np.arange(-6400, 6401) * (PI / 2), f64)
    sweep = np.concatenate([neighbour(base, f64, s) for s in (-2, -1, 0, 1, 2)])
    tiny = np.finfo(REAL[f64]).smallest_subnormal
    rng = np.random.default_rng(20)
    rest = rnd(np.concatenate([[0.0, -0.0, tiny, -tiny, 1e-30, -1e-30, 1e4, -1e4], rng.uniform(-1e4, 1e4, 20000)]), f64)
    assert len(sweep) <= MAX_ROWS
    return [("k pi/2 sweep", sweep), ("zeros, denormal, uniform", rest)]


def case_sincos(probe, f64):
    for label, x in sincos_inputs(f64):
        out = probe("SINCOS", f64, x)
        s, c, bs, bc = sincos_bounds(x, f64)
        hold(probe, f64, "dm_sincos sin, " + label, np.abs(out[:, 0] - s), bs, x)
        hold(probe, f64, "dm_sincos cos, " + label, np.abs(out[:, 1] - c), bc, x)
        assert (out[:, 2:] == 0).all()


def rot_expected(which, x, f64):
    """the written-out matrices: rot_y = [c 0 s; 0 1 0; -s 0 c] (m[2] = +s, m[6] = -s), rot_z = [c -s 0; s c 0; 0 0 1]; 0 and 1 are exact"""
    s, c, bs, bc = sincos_bounds(x, f64)
    o, z = np.ones_like(x), np.zeros_like(x)
    if which == "ROT_Y":
        want, bound = [c, z, s, z, o, z, -s, z, c], [bc, z, bs, z, z, z, bs, z, bc]
    else:
        want, bound = [c, -s, z, s, c, z, z, z, o], [bc, bs, z, bs, bc, z, z, z, z]
    return np.stack(want, 1), np.stack(bound, 1)


def case_rot(which):
    def case(probe, f64):
        for label, x in sincos_inputs(f64):
            out = probe(which, f64, x)
            want, bound = rot_expected(which, x, f64)
            hold(probe, f64, "%s, %s" % (which.lower(), label), np.abs(out[:, :9] - want), bound, x)
    return case


# ---------------------------------------------------------------- normalize_angle
def case_normalize_angle(probe, f64):
    """+-pi as the type holds it and its neighbours, k 2 pi +- an ulp for |k| <= 3, 0, +-1e3, 256 uniform draws in +-1e3.  The result lies in [-pi_Real, pi_Real] and
    equals the input modulo 2 pi: out - in is reduced by the nearest multiple of a 60-digit 2 pi in rational arithmetic (what sin and cos of the difference would say,
    without their rounding), so on a boundary either sign is right.  fmod is exact but takes off q turns of the TYPE's 2 pi, and the wrap one more: (|q| + 1) D2PI,
    plus the wrap's rounding u pi."""
    pi_r = float(REAL[f64](PI))
    two_pi_r = float(REAL[f64](TWO_PI))
    x = [0.0, 1e3, -1e3]
    for s in (-2, -1, 0, 1, 2):
        x += [float(neighbour(pi_r, f64, s)), float(neighbour(-pi_r, f64, s))]
    for k in range(-3, 4):
        x += [float(neighbour(k * TWO_PI, f64, s)) for s in (-1, 0, 1)]
    x = rnd(np.concatenate([x, np.random.default_rng(21).uniform(-1e3, 1e3, 256)]), f64)
    out = probe("NORMALIZE_ANGLE", f64, x)[:, 0]
    assert (out >= -pi_r).all() and (out <= pi_r).all(), "normalize_angle left [-pi, pi]: %r" % (x[(out < -pi_r) | (out > pi_r)],)
    two_pi = 2 * PI_FRAC
    resid = np.empty(len(x))
    for i in range(len(x)):
        d = Fraction(float(out[i])) - Fraction(float(x[i]))
        resid[i] = abs(float(d - two_pi * round(d / two_pi)))
    q = np.abs(np.trunc(x / two_pi_r))
    hold(probe, f64, "normalize_angle modulo 2 pi", resid, (q + 1) * D2PI[f64] + U[f64] * PI, x)
    inside = np.abs(x) <= pi_r
    assert (out[inside] == x[inside]).all()                        # an angle already inside comes back bit for bit


# ---------------------------------------------------------------- the algebraic helpers
def f_cross(a, x, y):
    return np.stack([a.sub(x[:, 1] * y[:, 2], x[:, 2] * y[:, 1]), a.sub(x[:, 2] * y[:, 0], x[:, 0] * y[:, 2]), a.sub(x[:, 0] * y[:, 1], x[:, 1] * y[:, 0])], 1)


def f_cross_add(a, c, x, y):
    return np.stack([a.sub(c[:, 0] + x[:, 1] * y[:, 2], x[:, 2] * y[:, 1]), a.sub(c[:, 1] + x[:, 2] * y[:, 0], x[:, 0] * y[:, 2]),
                     a.sub(c[:, 2] + x[:, 0] * y[:, 1], x[:, 1] * y[:, 0])], 1)


def f_qmul(a, p, q):
    pw, px, py, pz = p.T
    qw, qx, qy, qz = q.T
    return np.stack([a.sub(a.sub(a.sub(pw * qw, px * qx), py * qy), pz * qz), a.sub(pw * qx + px * qw + py * qz, pz * qy),
                     a.sub(pw * qy + py * qw + pz * qx, px * qz), a.sub(pw * qz + pz * qw + px * qy, py * qx)], 1)


def f_qrot(a, q, v):
    u = q[:, 1:]
    uv = 2 * f_cross(a, u, v)
    return v + q[:, :1] * uv + f_cross(a, u, uv)


def f_quat_to_rot(a, q):
    """cMathUtil::RotateMat(quat), divided by |q|^2"""
    w, x, y, z = q.T
    sw, sx, sy, sz = w * w, x * x, y * y, z * z
    inv = 1.0 / (sx + sy + sz + sw)
    m = [a.sub(a.sub(sx, sy), sz) + sw, 2 * a.sub(x * y, z * w), 2 * (x * z + y * w),
         2 * (x * y + z * w), a.sub(a.sub(sy, sx), sz) + sw, 2 * a.sub(y * z, x * w),
         2 * a.sub(x * z, y * w), 2 * (y * z + x * w), a.sub(a.sub(sz, sx), sy) + sw]
    return np.stack(m, 1) * inv[:, None]


def f_quat_diff_mul(a, q, o):
    """0.5 q (x) (0, omega)"""
    w, x, y, z = (0.5 * q).T
    ox, oy, oz = o.T
    return np.stack([a.sub(a.sub(a.neg(x * ox), y * oy), z * oz), a.sub(w * ox, z * oy) + y * oz, a.sub(z * ox + w * oy, x * oz), a.sub(x * oy, y * ox) + w * oz], 1)


def case_algebra(probe, f64):
    """4096 random rows each.  k of gamma_k: cross 2 (product, difference); cross_add, M v, M^T v, M M, quat_diff_mul 3 (product, two sums; the 0.5 is exact);
    qmul 4; qrot 6 (a cross on a cross: 2 + 2, times w or plus, plus); quat_to_rot 11 (square, three sums, times 1 / |q|^2 which carries the four of |q|^2 and a
    division of 1 ulp); qnormalize 7, relative (|q|^2: 4, halved by the sqrt of 1 ulp, a division of 1 ulp, a product)."""
    rng = np.random.default_rng(22)
    n = 4096
    v = lambda k=3: rnd(rng.standard_normal((n, k)) * 10.0 ** rng.uniform(-2, 2, (n, 1)), f64)
    a, b, c = v(), v(), v()
    val, S = value_and_scale(f_cross, a, b)
    hold(probe, f64, "cross", np.abs(probe("CROSS", f64, a, b)[:, :3] - val), gamma(2, f64) * S)
    val, S = value_and_scale(f_cross_add, c, a, b)
    hold(probe, f64, "cross_add vs c + a x b", np.abs(probe("CROSS_ADD", f64, c, a, b)[:, :3] - (c + np.cross(a, b))), gamma(3, f64) * S)
    A, B = v(9), v(9)
    A3, B3 = A.reshape(n, 3, 3), B.reshape(n, 3, 3)
    hold(probe, f64, "M3 * V3", np.abs(probe("M3_V3", f64, A, a)[:, :3] - np.einsum("nij,nj->ni", A3, a)), gamma(3, f64) * np.einsum("nij,nj->ni", np.abs(A3), np.abs(a)))
    hold(probe, f64, "tmul", np.abs(probe("TMUL", f64, A, a)[:, :3] - np.einsum("nji,nj->ni", A3, a)), gamma(3, f64) * np.einsum("nji,nj->ni", np.abs(A3), np.abs(a)))
    hold(probe, f64, "M3 * M3", np.abs(probe("M3_M3", f64, A, B)[:, :9] - np.einsum("nij,njk->nik", A3, B3).reshape(n, 9)),
         gamma(3, f64) * np.einsum("nij,njk->nik", np.abs(A3), np.abs(B3)).reshape(n, 9))
    p, q = rnd(unit_rows(rng, n, 4), f64), rnd(unit_rows(rng, n, 4), f64)
    val, S = value_and_scale(f_qmul, p, q)
    hold(probe, f64, "qmul", np.abs(probe("QMUL", f64, p, q)[:, :4] - val), gamma(4, f64) * S)
    val, S = value_and_scale(f_qrot, q, a)
    hold(probe, f64, "qrot", np.abs(probe("QROT", f64, q, a)[:, :3] - val), gamma(6, f64) * S)
    val, S = value_and_scale(f_quat_diff_mul, q, a)
    hold(probe, f64, "quat_diff_mul", np.abs(probe("QUAT_DIFF_MUL", f64, q, a)[:, :4] - val), gamma(3, f64) * S)
    for scale in (1e-3, 1.0, 1e3):                                  # quat_to_rot divides by |q|^2: any norm gives the rotation of q / |q|
        qs = rnd(scale * unit_rows(rng, n, 4), f64)
        val, S = value_and_scale(f_quat_to_rot, qs)
        out = probe("QUAT_TO_ROT", f64, qs)[:, :9]
        hold(probe, f64, "quat_to_rot, |q| = %g" % scale, np.abs(out - val), gamma(11, f64) * S)
        M = out.reshape(n, 3, 3)                                    # and it is a rotation: R R^T = 1 to 3 x 2 x the entries' bound (|R_ij| <= 1, S <= 1)
        hold(probe, f64, "quat_to_rot orthonormal, |q| = %g" % scale, np.abs(np.einsum("nij,nkj->nik", M, M) - np.eye(3)).reshape(n, 9), 6.5 * gamma(11, f64))
        out = probe("QNORMALIZE", f64, qs)[:, :4]
        want = qs / np.linalg.norm(qs, axis=1, keepdims=True)
        hold(probe, f64, "qnormalize, |q| = %g" % scale, np.abs(out - want), 7 * R[f64] * np.abs(want))
    # qstandardize is a sign choice: exact, and -0.0 < 0 is false, so w = -0.0 and w = 0 leave q as it is
    qz = q.copy()
    qz[:8, 0] = [-0.0, 0.0] * 4
    out = probe("QSTANDARDIZE", f64, qz)[:, :4]
    want = np.where(qz[:, :1] < 0, -qz, qz)
    assert (out == want).all() and (np.signbit(out) == np.signbit(want)).all() and (want[:, 0] >= 0).all() and np.signbit(out[0, 0]) and (out[:8, 1:] == qz[:8, 1:]).all()
    print("MATHDEV %-8s f%d qstandardize exact on %d rows" % (probe.name, 64 if f64 else 32, n))


# ---------------------------------------------------------------- quat_to_rotvec, quat_theta, calc_heading
def angle_classes(rng, per_class):
    """the angle in five classes: uniform in (0, 2 pi); small; just under pi; just over pi; just under 2 pi (w < 0 with a small rotation)"""
    t = lambda lo, hi: 10.0 ** rng.uniform(lo, hi, per_class)
    return np.concatenate([rng.uniform(0, TWO_PI, per_class), t(-7, -1), PI - t(-7, -1), PI + t(-7, -1), TWO_PI - t(-6, -1)])


def theta_reference(q, f64):
    """2 atan2(s, w) wrapped to [-pi, pi] in float64 and the bound on the helper's value of it.  s = |xyz| carries 3.5 u relative (three squares summed: 3, halved
    by the sqrt, whose own 1 ulp is 2), which reaches the angle as 2 ds w / (s^2 + w^2); atan2 LIBM u of its value, doubled exactly; an angle past pi loses one turn
    of the type's 2 pi: D2PI and the rounding of the difference.  So a rotation stored with w < 0 keeps an ABSOLUTE error of about ulp(2 pi) however small it is."""
    u = R[f64]
    w = q[:, 0]
    s = np.sqrt((q[:, 1:] ** 2).sum(axis=1))
    at = np.arctan2(s, w)
    near_pi = np.abs(2 * at - PI) < 0.25
    wrapped = 2 * at > PI
    th = np.where(wrapped, 2 * at - TWO_PI, 2 * at)
    d_th = 2 * 3.5 * u * s * np.abs(w) / (s * s + w * w) + 2 * LIBM[f64] * U[f64] * at + np.where(wrapped | near_pi, D2PI[f64] + u * PI, 0.0)
    return s, th, d_th, near_pi


def case_quat_to_rotvec(probe, f64):
    """random axes, the five angle classes, the identity and (-1, 0, 0, 0); eps = 1e-6 as every caller passes it (the small class straddles it).  The vector is
    (th / s) xyz: the angle's bound plus 6.5 u |th| (s again: 3.5, the division 2, the product 1).  Within 0.25 of pi the two sides are compared as rotations,
    through the float64 exponential and up to the quaternion's sign (half the vector's bound): +pi and -pi about one axis are one rotation."""
    rng = np.random.default_rng(23)
    per = 2048
    q = rnd(np.concatenate([axis_angle_quat(unit_rows(rng, 5 * per, 3), angle_classes(rng, per)), [[1, 0, 0, 0], [-1, 0, 0, 0]]]), f64)
    eps = float(REAL[f64](1e-6))
    out = probe("QUAT_TO_ROTVEC", f64, q, np.full(len(q), 1e-6))[:, :3]
    s, th, d_th, near_pi = theta_reference(q, f64)
    clear = keep_clear("quat_to_rotvec eps", s, eps, f64)
    zero = ~(s > eps)
    assert zero.sum() >= 100 and zero[-2:].all() and (out[zero & clear] == 0).all()
    want = np.where(zero[:, None], 0.0, (th / np.where(zero, 1.0, s))[:, None] * q[:, 1:])
    bound = (d_th + 6.5 * R[f64] * np.abs(th))[:, None]
    direct = clear & ~zero & ~near_pi
    assert direct.sum() > 2.5 * per and (q[direct, 0] < -0.99).sum() > per / 2            # the small rotations stored with w < 0 are compared directly
    hold(probe, f64, "quat_to_rotvec", np.abs(out - want)[direct], bound[direct] * np.ones(3), q[direct])
    hold(probe, f64, "quat_to_rotvec, w < -0.99", np.abs(out - want)[direct & (q[:, 0] < -0.99)], bound[direct & (q[:, 0] < -0.99)] * np.ones(3))
    hold(probe, f64, "quat_to_rotvec, small, w > 0", np.abs(out - want)[direct & (q[:, 0] > 0.99)], bound[direct & (q[:, 0] > 0.99)] * np.ones(3))
    rot = clear & near_pi
    assert rot.sum() > per
    qa, qb = exp_quat(out[rot]), exp_quat(want[rot])
    err = np.minimum(np.abs(qa - qb).max(axis=1), np.abs(qa + qb).max(axis=1))
    hold(probe, f64, "quat_to_rotvec near pi, as rotations", err, 0.5 * 1.01 * bound[rot, 0] + 4 * U[1], q[rot])


def case_quat_theta(probe, f64):
    """the same quaternions, and |sin(theta / 2)| on both sides of the helper's 1e-4 (0.5, 0.9, 1.1, 2 x 1e-4, both signs of w); compared modulo 2 pi (pi = -pi)"""
    rng = np.random.default_rng(24)
    per = 1024
    q = axis_angle_quat(unit_rows(rng, 5 * per, 3), angle_classes(rng, per))
    sh = np.repeat([0.5e-4, 0.9e-4, 1.1e-4, 2e-4], 32)
    edge = np.concatenate([np.sqrt(1 - sh * sh)[:, None] * np.tile([1.0, -1.0], len(sh) // 2)[:, None], sh[:, None] * unit_rows(rng, len(sh), 3)], axis=1)
    q = rnd(np.concatenate([q, edge, [[1, 0, 0, 0], [-1, 0, 0, 0]]]), f64)
    out = probe("QUAT_THETA", f64, q)[:, 0]
    s, th, d_th, _ = theta_reference(q, f64)
    clear = keep_clear("quat_theta 1e-4", s, 1e-4, f64)
    zero = ~(s > 1e-4)
    assert zero[clear].sum() >= 64 and (~zero[-130:-2]).sum() == 64 and (out[zero & clear] == 0).all()
    m = clear & ~zero
    hold(probe, f64, "quat_theta", mod_2pi(out - th)[m], d_th[m], q[m])


def case_calc_heading(probe, f64):
    """atan2(-d.z, d.x) of d = q (1, 0, 0) q^-1: 4096 random rotations and 65 headings about y from -pi to pi, where the heading is the angle itself.  d carries
    qrot's gamma_6 S per component; it turns the angle by |dd| / rho, rho = |(d.x, d.z)| (1.1: the arc sine up to 0.1, rows beyond that are dropped), atan2 adds LIBM u
    of its value; modulo 2 pi."""
    rng = np.random.default_rng(25)
    h = np.linspace(-PI, PI, 65)
    about_y = axis_angle_quat(np.tile([0.0, 1.0, 0.0], (65, 1)), h)
    q = rnd(np.concatenate([unit_rows(rng, 4096, 4), about_y]), f64)
    out = probe("CALC_HEADING", f64, q)[:, 0]
    ex = np.tile([1.0, 0.0, 0.0], (len(q), 1))
    d, S = value_and_scale(f_qrot, q, ex)
    rho = np.hypot(d[:, 0], d[:, 2])
    turn = gamma(6, f64) * np.hypot(S[:, 0], S[:, 2]) / rho
    ok = turn < 0.1
    assert ok.mean() >= 0.99
    want = np.arctan2(-d[:, 2], d[:, 0])
    hold(probe, f64, "calc_heading", mod_2pi(out - want)[ok], (1.1 * turn + LIBM[f64] * U[f64] * np.abs(want))[ok], q[ok])
    assert mod_2pi(out[-65:] - h).max() < 1e-5                      # (the reference's convention: a turn about +y by h is the heading h)


# ---------------------------------------------------------------- quat_exp, exp_map_to_quat
def exp_inputs(rng, f64, per):
    mags = [0.0, 1e-9, 9e-7, 1.1e-6, 1e-3, 1.0, PI - 1e-3, PI + 1e-3, 1.5 * PI, TWO_PI - 1e-3, TWO_PI + 1e-3, 3 * PI]
    rv = rnd(np.repeat(mags, per)[:, None] * unit_rows(rng, len(mags) * per, 3), f64)
    return rv, np.linalg.norm(rv, axis=1)


def case_quat_exp(probe, f64):
    """(cos(th / 2), sin(th / 2) / th rv) against the exact exponential.  th = |rv| carries 4 u relative (3.5 rounded up), th / 2 is exact; dm_sincos' own bound at
    th / 2 plus what 4 u th / 2 of argument does (times |sin| on the cos, |cos| on the sin); sh / th times rv_i: the sin's error, and 7 u |sh| (th again 4, the
    division 2, the product 1).  Below 1e-6 the series 0.5 - th^2 / 48 is 0.5 (1 + u): inside the same bound.  The output's norm is 1 to the Euclidean sum of those."""
    rv, th = exp_inputs(np.random.default_rng(26), f64, 64)
    keep_clear("quat_exp 1e-6", th, 1e-6, f64)
    out = probe("QUAT_EXP", f64, rv)[:, :4]
    u, half = R[f64], rnd(0.5 * th, f64)
    s, c, bs, bc = sincos_bounds(half, f64, exact_first=False)       # (the helper's own th / 2 is a few ulps from this one)
    bw = bc + 4 * u * half * np.abs(s)
    bv = bs + 4 * u * half * np.abs(c) + 7 * u * np.abs(s)
    want = exp_quat(rv)
    hold(probe, f64, "quat_exp w", np.abs(out[:, 0] - want[:, 0]), bw, rv)
    hold(probe, f64, "quat_exp xyz", np.abs(out[:, 1:] - want[:, 1:]), bv[:, None] * np.ones(3), rv)
    hold(probe, f64, "quat_exp norm", np.abs(np.linalg.norm(out, axis=1) - 1.0), bw + np.sqrt(3.0) * bv, rv)
    assert (out[th == 0] == [1, 0, 0, 0]).all()


def case_exp_map_to_quat(probe, f64):
    """cMathUtil::ExpMapToQuaternion's own branches in float64: identity unless |e| > 1e-6; ang = |e| wrapped to [-pi, pi]; (cos(ang / 2), sin(ang / 2) / |e| e) --
    for pi < |e| < 2 pi that is MINUS the exponential, the axis flipped and w > 0.  |e| carries 4 u relative; the wrap takes q + 1 turns of the type's 2 pi off and
    rounds: d_ang = 4 u |e| + (q + 1) D2PI + u pi; cos and sin LIBM u of their values plus d_ang / 2; sin / |e| times e_i another 7 u.  Compared with its sign
    everywhere except where |e| mod 2 pi is within 8 ulp of pi (3 pi is): +pi and -pi are both right there, and give q and -q."""
    rv, th = exp_inputs(np.random.default_rng(27), f64, 64)
    clear = keep_clear("exp_map_to_quat 1e-6", th, 1e-6, f64)
    out = probe("EXP_MAP_TO_QUAT", f64, rv)[:, :4]
    u = R[f64]
    n = np.fmod(th, TWO_PI)
    ang = np.where(n > PI, n - TWO_PI, n)
    ident = ~(th > 1e-6)
    want = np.where(ident[:, None], [1.0, 0, 0, 0], np.concatenate([np.cos(0.5 * ang)[:, None], (np.sin(0.5 * ang) / np.where(ident, 1.0, th))[:, None] * rv], axis=1))
    turns = np.trunc(th / TWO_PI)
    wraps = turns + (n > PI - 1e-2)
    d_ang = 4 * u * th + wraps * (D2PI[f64] + u * PI)
    bw = LIBM[f64] * U[f64] * np.abs(want[:, 0]) + 0.5 * d_ang * np.abs(np.sin(0.5 * ang))
    bv = LIBM[f64] * U[f64] * np.abs(np.sin(0.5 * ang)) + 0.5 * d_ang * np.abs(np.cos(0.5 * ang)) + 7 * u * np.abs(np.sin(0.5 * ang))
    bound = np.concatenate([bw[:, None], bv[:, None] * np.ones(3)], axis=1)
    assert (out[ident & clear] == [1, 0, 0, 0]).all() and ident.sum() == 3 * 64
    on_pi = np.abs(n - PI) <= 8 * ulp(PI, f64) + 4 * u * th
    assert on_pi.sum() <= 64 and (want[(th > PI + 1e-4) & (th < TWO_PI), 0] > 0).all() and not on_pi[th < 2 * PI].any()
    m = clear & ~ident & ~on_pi
    hold(probe, f64, "exp_map_to_quat", np.abs(out - want)[m], bound[m], rv[m])
    m = clear & on_pi
    err = np.minimum(np.abs(out - want), np.abs(out + want))[m]
    hold(probe, f64, "exp_map_to_quat, |e| = 3 pi, up to sign", err, bound[m] + 0.5 * d_ang[m, None], rv[m])


# ---------------------------------------------------------------- qslerp
def slerp_coefficients(ad, t, linear):
    th = np.arccos(np.minimum(ad, 1.0))
    st = np.where(linear, 1.0, np.sin(th))
    return np.where(linear, 1 - t, np.sin((1 - t) * th) / st), np.where(linear, t, np.sin(t * th) / st), th


def d_ratio(a, th, d_th):
    """bound on the change of sin(a th) / sin(th) over th +- d_th: its derivative is a (1 - a^2) th / 3 (1 + O(th^2)) <= 0.7 a (1 - a^2) th on (0, pi / 2]"""
    return 0.7 * a * (1 - a * a) * (th + d_th) * d_th


def case_qslerp(probe, f64):
    """Eigen's Quaternion::slerp in float64 with the threshold the library installs for the type (dm_host.cpp: 1 - 1e-6 float, 1 - epsilon double), passed the way
    the model tables hold it.  Pairs: random (dot of either sign); nearly equal above the threshold (the linear branch); theta in the decade below it; b = a; b = -a;
    every pair with b and with -b, at t in {0, 1, 0.5, random}.
    Bound: d = a . b carries gamma_4 (|a| . |b|) =: dd.  Linear branch: 1 - t rounds, u.  Else th = acos |d| moves by 2 dd / sin th + LIBM u th -- much, next to the
    threshold, hence the 2: th'^2 - th^2 = 2 dd gives |th' - th| <= 2 dd / th -- but s0 = sin((1 - t) th) / sin th hardly depends on th (`d_ratio`); what remains is the rounding of (1 - t) th (2 u of it), the two sines (LIBM u
    each, relative) and the division (2 u).  Then s0 a + s1 b: gamma_2.  Within 8 ulp of the threshold either branch is right: the bound grows by the distance
    between the reference's two branches."""
    rng = np.random.default_rng(28)
    u, r1 = U[f64], R[f64]
    thr = float(REAL[f64](1.0 - 1e-6)) if not f64 else 1.0 - np.finfo(np.float64).eps
    n = 512
    a = unit_rows(rng, n, 4)
    perp = unit_rows(rng, n, 4)
    perp -= (perp * a).sum(axis=1, keepdims=True) * a
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    toward = lambda th: np.cos(th)[:, None] * a + np.sin(th)[:, None] * perp
    gap = 1.0 - thr
    lo = gap + 16 * u
    below = np.sqrt(2 * rng.uniform(lo, max(10 * gap, lo + 12 * u), n))             # 1 - cos th = th^2 / 2: the decade under the threshold, clear of its 8 ulp
    above = np.sqrt(2 * rng.uniform(0, max(gap - 10 * u, 0), n))
    sets = [("random", unit_rows(rng, n, 4)), ("above the threshold", toward(above)), ("decade below the threshold", toward(below)), ("b = a", a.copy())]
    for label, b in sets:
        for sign in (1.0, -1.0):
            qa = rnd(np.tile(a, (4, 1)), f64)
            qb = rnd(np.tile(sign * b, (4, 1)), f64)
            t = rnd(np.concatenate([np.zeros(n), np.ones(n), np.full(n, 0.5), rng.uniform(0, 1, n)]), f64)
            out = probe("QSLERP", f64, qa, qb, t, np.full(4 * n, thr))[:, :4]
            d = (qa * qb).sum(axis=1)
            ad = np.abs(d)
            linear = ad >= thr
            if label == "decade below the threshold":
                assert not linear.any() and (1 - ad < 10 * gap + 40 * u).all() and keep_clear("qslerp " + label, ad, thr, f64).all()
            if label in ("above the threshold", "b = a"):
                assert f64 or linear.all()                      # (in double the threshold is two ulps under 1: b = a sits on it)
            if label == "random":
                assert (~linear).all() and (d < 0).sum() > n and (d > 0).sum() > n
            s0, s1, th = slerp_coefficients(ad, t, linear)
            l0, l1, _ = slerp_coefficients(ad, t, np.ones_like(linear))
            n0, n1, _ = slerp_coefficients(np.minimum(ad, thr - u), t, np.zeros_like(linear))
            on_edge = np.abs(ad - thr) <= 8 * ulp(thr, f64)
            dd = gamma(4, f64) * (np.abs(qa) * np.abs(qb)).sum(axis=1)
            d_th = 2 * dd / np.where(linear, 1.0, np.sin(th)) + LIBM[f64] * u * th
            rel = 4 * r1 + 2 * LIBM[f64] * u
            b0 = np.where(linear, r1, d_ratio(1 - t, th, d_th) + rel * np.abs(s0)) + np.where(on_edge, np.abs(l0 - n0), 0.0)
            b1 = np.where(linear, 0, d_ratio(t, th, d_th) + rel * np.abs(s1)) + np.where(on_edge, np.abs(l1 - n1), 0.0)
            flip = np.where(d < 0, -1.0, 1.0)
            want = s0[:, None] * qa + (flip * s1)[:, None] * qb
            bound = b0[:, None] * np.abs(qa) + b1[:, None] * np.abs(qb) + gamma(2, f64) * (np.abs(s0)[:, None] * np.abs(qa) + np.abs(s1)[:, None] * np.abs(qb))
            hold(probe, f64, "qslerp %s, %s" % (label, "b" if sign > 0 else "-b"), np.abs(out - want), bound, np.concatenate([qa, qb, t[:, None]], axis=1))
            if label == "b = a":                                # a to a, and a to -a, is a at every t
                hold(probe, f64, "qslerp %s stays a" % ("a, a" if sign > 0 else "a, -a"), np.abs(out - qa), bound + 2 * r1)


# ---------------------------------------------------------------- the cases on both libraries
CASES = dict(sincos=case_sincos, rot_y=case_rot("ROT_Y"), rot_z=case_rot("ROT_Z"), normalize_angle=case_normalize_angle, algebra=case_algebra,
             quat_to_rotvec=case_quat_to_rotvec, quat_theta=case_quat_theta, calc_heading=case_calc_heading, quat_exp=case_quat_exp,
             exp_map_to_quat=case_exp_map_to_quat, qslerp=case_qslerp)


@pytest.mark.parametrize("f64", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_helper_emulator(emu_lib, case, f64):
    CASES[case](Probe(emu_lib, gpu=False), f64)


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_helper_gpu(hip_lib, case, f64):
    CASES[case](Probe(hip_lib, gpu=True), f64)


def _launch_shape(probe, f64):
    """n in {1, 63, 64, 65}: a lone lane, a wave short of one lane, a full wave, a second workgroup of one lane; rows >= n keep the sentinel, every double of them"""
    rows = 130
    x = rnd(np.linspace(-9.0, 9.0, rows), f64)
    inp = np.zeros((rows, mp.IN))
    inp[:, 0] = x
    T = REAL[f64]
    m = np.fmod(x.astype(T), T(TWO_PI))                              # IEEE arithmetic in the type: fmod is exact, the wrap one correctly rounded sum
    want = np.where(m > T(PI), -T(TWO_PI) + m, np.where(m < -T(PI), T(TWO_PI) + m, m)).astype(np.float64)
    assert (want != x).sum() > 60 and (want < x).any() and (want > x).any()
    for n in (1, 63, 64, 65):
        out = probe.raw("NORMALIZE_ANGLE", f64, n, inp, fill=-77.0)
        assert (out[n:] == -77.0).all(), "n = %d: a row >= n was written" % n
        assert (out[:n, 1:] == 0).all() and (out[:n, 0] == want[:n]).all()          # each row is ITS input's angle


@pytest.mark.parametrize("f64", [0, 1])
def test_launch_shape_emulator(emu_lib, f64):
    _launch_shape(Probe(emu_lib, gpu=False), f64)


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [0, 1])
def test_launch_shape_gpu(hip_lib, f64):
    _launch_shape(Probe(hip_lib, gpu=True), f64)


def _argument_checks(lib_path):
    lib = load_library(lib_path)
    inp = np.zeros((4, mp.IN))
    out = np.full((4, mp.OUT), 7.0)
    good = dict(op=0, f64=0, n=4, in_ptr=inp.ctypes.data, out_ptr=out.ctypes.data, lib_path=lib_path)
    for bad in (dict(n=0), dict(n=-5), dict(in_ptr=0), dict(out_ptr=0), dict(op=-1), dict(op=len(mp.OPS)), dict(op=1000)):
        with pytest.raises(RuntimeError, match="dm_math_probe"):
            mp.math_probe(**dict(good, **bad))
        assert b"dm_math_probe" in lib.dm_last_error()
    assert (out == 7.0).all()           # nothing was launched


def test_argument_checks_emulator(emu_lib):
    _argument_checks(emu_lib)


@pytest.mark.gpu
def test_argument_checks_gpu(hip_lib):
    """host addresses: every call is refused before a launch, so none is dereferenced"""
    _argument_checks(hip_lib)


def test_binding_names_the_ops_of_the_header():
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    enum = re.search(r"enum \{ (DM_MOP_SINCOS = 0,[^}]*)\}", src).group(1)
    names = [s.strip().split(" ")[0] for s in enum.split(",")]
    assert names == ["DM_MOP_" + o for o in mp.OPS] + ["DM_MOP_COUNT"]
    assert int(re.search(r"#define DM_MATH_PROBE_IN (\d+)", src).group(1)) == mp.IN and int(re.search(r"#define DM_MATH_PROBE_OUT (\d+)", src).group(1)) == mp.OUT
    assert set(CASES) >= {"sincos", "qslerp"} and len(mp.OPS) == 21


def test_shipped_revolute_joints_have_limits():
    """what the comment at the rot_z call of dm_device.h (kinematics) rests on: the integrator never wraps a revolute angle and dm_sincos is measured for |x| <= 1e4;
    every revolute joint of the shipped characters has limits (lim_lo <= lim_hi: limit rows hold it there) within +-2 pi"""
    from deepmimic_amd import model
    seen = 0
    for f in sorted(os.listdir(model.ASSET_DIR)):
        if f.endswith(".json"):
            jm = model.load_asset(f[:-5]).joint_mat
            rev = jm[(jm[:, model.JD_TYPE] == model.JT_REVOLUTE) & (jm[:, model.JD_PARENT] >= 0)]
            seen += len(rev)
            assert (rev[:, model.JD_LL0] <= rev[:, model.JD_LH0]).all() and (np.abs(rev[:, [model.JD_LL0, model.JD_LH0]]) <= TWO_PI).all(), f
    assert seen > 0
