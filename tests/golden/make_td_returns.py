#!/usr/bin/env python
"""Golden vectors for the TD(lambda) kernel (deepmimic_amd/csrc/dm_returns.h) from the REFERENCE's own learning/rl_util.py (numpy only), imported from the
reference checkout in the build container.  Random [T, N] rollouts are cut into paths per env column; every path goes through the reference's compute_return
with val_t assembled by the end-of-path rules of learning/ppo_agent.py:251-266 -- behind a path's last step stands val_fail / val_succ (done with terminate
Fail / Succ), the critic on the terminal observation (done with Null) or, for a window cut at T, values[T] -- in float64 from the float32 inputs; gamma = 0 gives
the rewards back as ppo_agent.py:269-270 does.  A path that ended invalid is masked.  Writes tests/golden/td_returns.npz: inputs, expected float32 returns, masks.
Usage: python tests/golden/make_td_returns.py [/root/reference]"""
import os
import sys

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, os.path.join(REF, "learning"))
import rl_util as ref                                # noqa: E402  (the reference's file, unmodified)

SHAPES = [(T, N) for T in (1, 5, 7) for N in (3, 64, 65)]
PARAMS = [(0.95, 0.95), (0.95, 0.0), (0.95, 1.0), (0.0, 0.95)]
VAL_FAIL, VAL_SUCC = -0.3, 1.0 / (1.0 - 0.95)        # (ppo_agent.py: 0 and 1 / (1 - discount); a non-zero failure value shows in the bits)
NULL, FAIL, SUCC = 0, 1, 2

rng = np.random.default_rng(20261017)
out = {"shapes": np.array(SHAPES, np.int32), "params": np.array(PARAMS), "val_fail_succ": np.array([VAL_FAIL, VAL_SUCC])}


def column(T, c):
    """(done, terminate, valid) of env column c: the first seven columns are the named edge cases (clipped to the window), the rest random"""
    done, term, valid = np.zeros(T, np.int32), np.zeros(T, np.int32), np.ones(T, np.int32)

    def end(t, kind=NULL, ok=1):
        if 0 <= t < T:
            done[t], term[t], valid[t] = 1, kind, ok
    k = c % 10
    if k == 0:
        pass                                          # no done at all: one path, cut at T
    elif k == 1:
        end(0, NULL)                                  # done at t = 0
    elif k == 2:
        end(T - 1, FAIL)                              # done at t = T - 1
    elif k == 3:
        end(1, SUCC); end(2, NULL); end(3, FAIL)      # dones on consecutive steps, every kind of end
    elif k == 4:
        end(1, NULL); end(3, NULL, ok=0)              # one invalid episode in the middle (steps 2 .. 3)
    elif k == 5:
        end(2, FAIL, ok=0); end(T - 1, SUCC)          # one invalid episode running into t = 0
    elif k == 6:
        end(0, NULL, ok=0)                            # ... of one step
    else:
        for t in range(T):
            if rng.random() < 0.3:
                end(t, int(rng.integers(0, 3)), int(rng.random() > 0.25))
    return done, term, valid


for T, N in SHAPES:
    key = "T%d_N%d" % (T, N)
    rewards = rng.random((T, N)).astype(np.float32) + np.float32(0.01)
    values = (rng.normal(size=(T + 1, N)) * 3 + 5).astype(np.float32)
    term_values = (rng.normal(size=(T, N)) * 3 + 5).astype(np.float32)
    done, term, valid = (np.zeros((T, N), np.int32) for _ in range(3))
    for c in range(N):
        done[:, c], term[:, c], valid[:, c] = column(T, c)
    for name, a in (("rewards", rewards), ("values", values), ("term_values", term_values), ("done", done), ("terminate", term), ("valid", valid)):
        out[key + "/" + name] = a
    for p, (gamma, lam) in enumerate(PARAMS):
        ret, mask = np.zeros((T, N), np.float32), np.ones((T, N), np.int32)
        for c in range(N):
            t0 = 0
            while t0 < T:
                t1 = t0
                while t1 < T - 1 and not done[t1, c]:
                    t1 += 1                           # the step that closes the path: a done step, or the last of the window
                r = rewards[t0:t1 + 1, c].astype(np.float64)
                val_t = np.zeros(len(r) + 1)
                val_t[:len(r)] = values[t0:t1 + 1, c].astype(np.float64)
                if done[t1, c]:
                    val_t[-1] = VAL_FAIL if term[t1, c] == FAIL else VAL_SUCC if term[t1, c] == SUCC else float(term_values[t1, c])
                else:
                    val_t[-1] = float(values[T, c])
                new_vals = r.copy() if gamma == 0 else ref.compute_return(r, gamma, lam, val_t)
                ret[t0:t1 + 1, c] = new_vals.astype(np.float32)
                if done[t1, c] and not valid[t1, c]:
                    mask[t0:t1 + 1, c] = 0
                t0 = t1 + 1
        out["%s/returns%d" % (key, p)] = ret; out["%s/mask%d" % (key, p)] = mask
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "td_returns.npz"), **out)
print("wrote", len(out), "arrays")
