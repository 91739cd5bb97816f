"""Times of the device state pool's launches (k_state_save / k_state_restore of deepmimic_amd/csrc/dm_device.h, deepmimic_amd/state_pool.py) by the method of
tools/link_state_bench.py: one process, the arms alternating, whole calls bracketed by HIP events on the current stream (the ctypes launch path included), every
repetition kept, medians of `reps`.  Per scene (4096 humanoid3d_walk and 4096 dog3d_pace by default), at a mask of 1 % and of 100 % of the envs:
  save                                   dm_state_save, every env into its own slot
  restore_rewind[_states]                dm_state_restore, DM_POOL_REWIND, without / with states_dev (and goals_dev in a goal scene)
  restore_new_episode[_states]           the same with DM_POOL_NEW_EPISODE
  reset_where_100pct                     the yardstick: dm_reset_where at a full mask in the same bracket
next to the bytes each launch moves (record bytes read + written, observation rows written; from the layout) and the GB/s that makes.  A REWIND restore does a
subset of dm_reset_where's work (the same load and emit, no motion sample, no draw, no store), so its median is expected at or below the yardstick's; the output
says whether it is.  Also the host route of the same context, wall clock: BatchEnv.snapshot() + restore() of all envs.  A report; the comparison is recorded, not
asserted.  Writes one JSON object (default profiles/state_pool_bench.json).
usage: python tools/state_pool_bench.py [--N 4096] [--reps 100] [--warmup 10] [--scenes humanoid3d_walk dog3d_pace] [--out ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd import link_state as ls, model, state_pool as sp  # noqa: E402
from deepmimic_amd.vec_env import TorchVecEnv  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def quartiles(x):
    return [float(np.percentile(x, p)) for p in (25, 50, 75)]


def bench(scene, N, reps, warmup):
    env = TorchVecEnv(model.load_asset(scene), N, seed=1, deferred_reset=True)
    env.reset(); env._enter()
    e, dev, S, G = env.env, env.device, env.obs_dim, env.goal_dim
    pool = env.state_pool(N)
    slot_bytes, pp, bad = pool.slot_bytes, pool.data.data_ptr(), pool.bad.data_ptr()
    ids = torch.arange(N, dtype=torch.int32, device=dev)
    masks = {"1pct": torch.zeros(N, dtype=torch.int32, device=dev), "100pct": torch.ones(N, dtype=torch.int32, device=dev)}
    masks["1pct"][::100] = 1
    obs, goal = env.obs.data_ptr(), env.goal.data_ptr() if G else 0
    act = torch.zeros((N, env.act_dim), device=dev)
    for _ in range(3):
        env.step(act)                                       # states off the reference motion
    sp.save_device(e, pp, N, masks["100pct"].data_ptr(), ids.data_ptr(), bad)
    runs, moved = {}, {}
    row = 4 * (S + G)
    for share, m in masks.items():
        mp, n = m.data_ptr(), int(m.sum())
        runs["save_" + share] = lambda mp=mp: sp.save_device(e, pp, N, mp, ids.data_ptr(), bad)
        moved["save_" + share] = 2 * n * slot_bytes
        for mode, flag in (("rewind", sp.REWIND), ("new_episode", sp.NEW_EPISODE)):
            runs["restore_%s_%s" % (mode, share)] = lambda mp=mp, flag=flag: sp.restore_device(e, pp, N, mp, ids.data_ptr(), flag, 0, 0, bad)
            runs["restore_%s_states_%s" % (mode, share)] = lambda mp=mp, flag=flag: sp.restore_device(e, pp, N, mp, ids.data_ptr(), flag, obs, goal, bad)
            # read from the pool and written to the env rows, read again by the load; NEW_EPISODE stores the record back
            rec = (3 if mode == "rewind" else 4) * n * slot_bytes
            moved["restore_%s_%s" % (mode, share)] = rec
            moved["restore_%s_states_%s" % (mode, share)] = rec + n * row
    runs["reset_where_100pct"] = lambda: ls.reset_where_device(e, masks["100pct"].data_ptr(), obs, goal)
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in times.items()}
    host = []
    for _ in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        e.restore(e.snapshot()); e.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    pool_dims = sp.dims(e)
    env.close()
    yard = med["reset_where_100pct"]
    return dict(scene=scene, N=N, S=S, G=G, slot_bytes=slot_bytes, pool_dims=pool_dims, bytes_moved=moved,
                GB_per_s={k: moved[k] / (med[k] * 1e-6) / 1e9 for k in moved}, us_q25_median_q75={k: quartiles(v) for k, v in times.items()},
                rewind_100pct_over_reset_where_100pct=med["restore_rewind_states_100pct"] / yard,
                rewind_at_or_below_the_yardstick=bool(med["restore_rewind_states_100pct"] <= yard),
                host_snapshot_plus_restore_us_wall_clock=host, us_every_repetition=times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4096); ap.add_argument("--reps", type=int, default=100); ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scenes", nargs="+", default=["humanoid3d_walk", "dog3d_pace"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_pool_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("state_pool_bench needs a GPU (deepmimic_amd has no CPU path)")
    out = dict(what="the device state pool: microseconds per dm_state_save / dm_state_restore call (HIP events, alternating, the ctypes launch path included) at masks of "
                    "1 % and 100 % beside the bytes each launch moves (from the layout) and dm_reset_where at a full mask in the same bracket; the host "
                    "snapshot() + restore() of the same context by wall clock; a report, no gate",
               device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, scenes=[bench(s, a.N, a.reps, a.warmup) for s in a.scenes])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k in ("device", "reps")}))
    for u in out["scenes"]:
        print("%s N=%d slot %d B  us q25/median/q75:" % (u["scene"], u["N"], u["slot_bytes"]), json.dumps(u["us_q25_median_q75"]))
        print("  GB/s:", json.dumps(u["GB_per_s"]))
        print("  rewind(100 %%, states) / reset_where(100 %%) = %.3f; host snapshot + restore: %.0f us (median of %d)"
              % (u["rewind_100pct_over_reset_where_100pct"], float(np.median(u["host_snapshot_plus_restore_us_wall_clock"])), len(u["host_snapshot_plus_restore_us_wall_clock"])))


if __name__ == "__main__":
    main()
