#!/usr/bin/env python
"""Golden vectors for the time-warp alignment kernel (deepmimic_amd/csrc/dm_time_warp.h) from the REFERENCE's own cDynamicTimeWarper, compiled into
oracle/_ref/libdm_ref.so (`ref_time_warp` of oracle/ref_glue.cpp, under cSceneImitateAMP::TimeWarpCost).  Run where oracle/_ref is built.
Writes tests/golden/time_warp_vectors.npz: for dim = 45 (the humanoid's 3J) and the dog's 3J one batch of envs with the sample counts COUNTS mixed, capacity CAPACITY --
the smallest counts at which the strip hand-over of the kernel (64 rows per strip), its ramp-up and its tail can go wrong.

Data: the simulated side is a random walk, the kinematic side the same walk re-timed by a random monotone index map plus a small walk of its own, so that the optimal
path leaves the diagonal (checked below against the diagonal's cost).  Every value is q / 256 with an int16 q (the file holds q): exactly representable in float32, so
that the float and the double kernel read the same numbers.  Only the first count[i] rows of env i are stored (rows past the count are never read).
Usage: python tests/golden/make_time_warp_vectors.py"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_lib                                       # noqa: E402
from deepmimic_amd import model                      # noqa: E402

COUNTS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 130)
CAPACITY = 140
SCALE = 256.0

lib = ref_lib.load("ref")
lib.ref_time_warp.restype = ctypes.c_double
rng = np.random.default_rng(20260417)
dims = (45, 3 * model.load_asset("dog3d_pace").num_joints)
out = {"capacity": np.array([CAPACITY], np.int32), "dims": np.array(dims, np.int32), "scale": np.array([SCALE])}
for dim in dims:
    order = rng.permutation(len(COUNTS))
    counts = np.array(COUNTS, np.int32)[order]
    rows0, rows1, want, diag = [], [], [], []
    for n in counts:
        base = np.cumsum(rng.integers(-32, 33, size=(2 * n + 2, dim)), axis=0) + rng.integers(-256, 257, size=dim)
        idx = np.minimum(np.cumsum(rng.integers(0, 3, size=n)), 2 * n + 1)                     # the kinematic side's clock: stalls, runs and double steps
        q0 = base[:n].astype(np.int16)
        q1 = (base[idx] + np.cumsum(rng.integers(-4, 5, size=(n, dim)), axis=0)).astype(np.int16)
        assert np.abs(base).max() < 32000
        d0, d1 = q0 / SCALE, q1 / SCALE
        assert np.array_equal(d0.astype(np.float32).astype(np.float64), d0) and np.array_equal(d1.astype(np.float32).astype(np.float64), d1)
        w = lib.ref_time_warp(ref_lib._d(ref_lib._arr(d0)), int(n), ref_lib._d(ref_lib._arr(d1)), int(n), int(dim), CAPACITY)
        dg = float(np.linalg.norm((d0 - d1).reshape(n, -1, 3), axis=2).mean(axis=1)[1:].sum())  # the cost of the diagonal path
        assert n < 63 or w < 0.9 * dg, (n, w, dg)                                                # the optimal path leaves the diagonal
        rows0.append(q0); rows1.append(q1); want.append(w); diag.append(dg)
    out["d%d/count" % dim] = counts
    out["d%d/sim" % dim] = np.concatenate(rows0); out["d%d/kin" % dim] = np.concatenate(rows1)
    out["d%d/want" % dim] = np.array(want); out["d%d/diag" % dim] = np.array(diag)
path = os.path.join(HERE, "time_warp_vectors.npz")
np.savez_compressed(path, **out)
print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")
