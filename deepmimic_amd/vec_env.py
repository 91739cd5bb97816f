"""Device-resident vectorised env on top of the C-ABI (deepmimic_amd/core.py): observations, rewards and flags stay in HBM as
torch tensors, one kernel launch per 30 Hz control step, asynchronous on torch's current stream (whatever is current at each call) -- the way a GPU learner consumes
the path (the facade in compat/ is the drop-in for the reference's one-env-per-process driver; this is the batched form of the same
protocol: SetAction ; 20 x Update ; RecordState / CalcReward / CheckTerminate ; Reset of finished episodes, DeepMimic.py:62-80).

torch is plumbing here (device memory, streams); the stepping itself is libdm_hip.so.  From 4096 envs per GPU on, `TorchVecEnvGroups` (two env groups on their
own streams, below) is the faster form of the same thing: +2 ... 15 % depending on the scene (profiles/r04_bench_scenes_groups.json).

`--timer_type exp` scenes are served like the uniform timer since round 4: the in-kernel auto-reset draws min(min + Exp, max) (util/Timer.cpp:64-67)."""
from __future__ import annotations

import copy
from typing import Dict, Tuple

from .binding import stream_handle, tensor_arg
from .core import BatchEnv
from .episodes import EpisodeStats, decode_block, merge_blocks
from .kin_query import KinQuery, reset_where_at_device
from .link_state import KIN, SIM, LinkState, reset_where_device
from . import pushes as pu
from . import state_pool as sp
from .model import SceneTables
from .time_warp import TimeWarp, buffer_size, why_no_warper


class _EnvStatePool(sp.StatePool):
    """the StatePool of a TorchVecEnv: the calls go to torch's current stream, and a restore writes the env's `obs` / `goal` rows unless told otherwise"""

    def __init__(self, venv, slots: int):
        super().__init__(venv.env, slots, device=venv.device)
        self.venv = venv

    def save(self, mask, slots):
        self.venv._enter()
        return super().save(mask, slots)

    def restore(self, mask, slots, new_episode: bool = False, states=None, goals=None):
        v = self.venv
        v._enter()
        return super().restore(mask, slots, new_episode=new_episode, states=v.obs if states is None else states, goals=v.goal if goals is None else goals)


class TorchVecEnv:
    def __init__(self, tables: SceneTables, num_envs: int, device: str = "cuda:0", seed: int = 0, timestep: float = 1.0 / 600,
                 updates_per_step: int = 20, amp_obs: bool = False, terminal_obs: bool = True, episode_stats: bool = False, episode_bins: int = 0,
                 episode_bin_steps: int = 1, time_warp: bool = False, link_state: bool = False, kin_link_state: bool = False, deferred_reset: bool = False,
                 kin_lookahead=(), pushes: bool = False, **env_kwargs):
        """terminal_obs (default on): keep `terminal_obs` / `terminal_goal` tensors bound to the context (BatchEnv.set_terminal_outputs), handed out as
        info["terminal_obs"] / info["terminal_goal"] by `step`; off: the launches write nothing extra and the two keys are absent.
        episode_stats (default off: no extra launch, no extra key): `step` runs deepmimic_amd.episodes.EpisodeStats.update behind the step launch on the same
        stream and hands out info["episode_return"] / info["episode_length"]; `episode_totals()` reads the totals (and a length histogram of `episode_bins`
        bins of `episode_bin_steps` steps).
        time_warp (default off: no extra launch, no extra key; `--scene imitate_amp` with a finite episode length only, refused elsewhere): the test-mode return
        of the reference, cSceneImitateAMP::CalcRewardTimeWarp (deepmimic_amd/time_warp.py).  `step` samples every env in front of the step launch, aligns the
        envs whose episode ended behind it and hands out info["time_warp_return"]: float32 [N], the reward the reference's test mode pays at this step -- the
        alignment cost plus 1 per sample the episode fell short of the buffer where done[i] is set in THIS step, 0 elsewhere.  `reward` stays what the launch
        wrote.  With `episode_stats` as well the statistics accumulate time_warp_return IN PLACE OF reward (episode_return included), so that `episode_totals()`
        is the reference's Test_Return for these scenes.  Memory: N * 2 * capacity * 3J * sizeof(Real) for the samples, capacity = ceil(30 * episode length) + 2
        -- 0.89 GB for 4096 humanoids and 20 s episodes in fp32.
        link_state / kin_link_state / deferred_reset (all off by default: `step` launches and returns exactly what it does without them) serve tasks written in
        torch (deepmimic_amd/link_state.py has the column constants).
        link_state: `step` runs dm_link_state behind the step launch on the same stream and hands out info["link_state"] [N, J, 22], info["link_env"] [N, 8],
        info["pose"] / info["vel"] [N, P] and, where the scene has a ball, info["obj_state"] [N, 13] -- float32 tensors of the SIMULATED character; `link_names` names
        the J rows.  kin_link_state adds the same of the KINEMATIC character (the clip the env tracks) under "kin_link_state", "kin_link_env", "kin_pose", "kin_vel".
        `update_link_state()` refreshes the tensors from the context's current state at any time, e.g. behind `reset()`.
        WITHOUT deferred_reset the link-state rows of envs that are done in this step describe the first state of the NEW episode, as `obs` does: the launch has
        reset them already.  deferred_reset: `step` launches without the in-kernel auto-reset (ending an episode at the update that ends it, as before), takes the
        link states -- which then describe the END OF THE STEP for every env, finished ones included: the state a task reward has to see --, copies the `obs` /
        `goal` rows of done envs into `terminal_obs` / `terminal_goal` and resets the done envs with dm_reset_where, which overwrites those `obs` / `goal` rows with
        the new episode's.  (obs, reward, done, info) hold the same bytes as the auto-reset step's; it is three or four launches and two small torch kernels
        instead of one launch, with no host read.
        kin_lookahead=(o_1, ..., o_K) (default none: no extra launch, no extra key): offsets in seconds from every env's clip clock.  Wherever the kinematic link
        state is refreshed -- in `step` and in `update_link_state()` -- dm_kin_query samples the kinematic character at clock + o_k and hands out
        info["kin_ahead_link_state"] [N, K, J, 22], info["kin_ahead_link_env"] [N, K, 8], info["kin_ahead_pose"] / info["kin_ahead_vel"] [N, K, P]: the target
        frames a tracking policy is fed (deepmimic_amd/kin_query.py).  `kin_query()` asks for other times, clips or the clip's own frame; `set_start_sampler()`
        lets the task choose where new episodes start; `state_pool()` keeps whole env states on the device to rewind to or to start episodes from.
        pushes (default off: no extra launch, no extra key, the context as before): the task places forces on body parts (deepmimic_amd/pushes.py).  The env works
        on its own copy of the scene config with `task_pushes` set, so the context carries the perturbation rows; `push()` / `clear_pushes()` write them from
        device tensors, and `reset` and `step` refresh `pushes`, float32 [N, 2, 6] = per slot {link (-1: free), force xyz, duration, elapsed}, handed out as
        info["pushes"]: one dm_push_state launch.  With deferred_reset it is taken before the reset, like the link states: a finished env shows what was acting
        when its episode ended (the reset then clears its slots)."""
        import torch
        if pushes:
            tables = copy.copy(tables)
            tables.cfg = copy.copy(tables.cfg)
            tables.cfg.task_pushes = True
        self.torch = torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TorchVecEnv needs a GPU device (deepmimic_amd has no CPU path)")
        if time_warp and buffer_size(tables.cfg, tables.query_rate) is None:
            raise ValueError("time_warp=True: " + why_no_warper(tables.cfg))
        with torch.cuda.device(self.device):
            torch.zeros(1, device=self.device)                     # torch's context first (one HIP runtime in the process)
            self.env = BatchEnv(tables, num_envs, device_id=self.device.index or 0, seed=seed, **env_kwargs)
        self.n, self.obs_dim, self.act_dim, self.goal_dim = self.env.N, self.env.S, self.env.A, self.env.G
        self.timestep, self.updates = float(timestep), int(updates_per_step)
        f32, i32 = dict(dtype=torch.float32, device=self.device), dict(dtype=torch.int32, device=self.device)
        self.obs = torch.zeros((self.n, self.obs_dim), **f32); self.reward = torch.zeros(self.n, **f32)
        self.terminate = torch.zeros(self.n, **i32); self.valid = torch.zeros(self.n, **i32); self.episode_end = torch.zeros(self.n, **i32)
        self.amp_obs = torch.zeros((self.n, self.env.amp_size), **f32) if (amp_obs and self.env.amp_size) else None
        self.goal = torch.zeros((self.n, self.goal_dim), **f32) if self.goal_dim else None      # RecordGoal of the last step (goal scenes), device resident
        # observation / goal of the moment an episode ended, written by the launch that resets the env (rows of other envs keep what they held)
        self.terminal_obs = torch.zeros((self.n, self.obs_dim), **f32) if terminal_obs else None
        self.terminal_goal = torch.zeros((self.n, self.goal_dim), **f32) if (terminal_obs and self.goal_dim) else None
        if terminal_obs:
            self.env.set_terminal_outputs(self.terminal_obs.data_ptr(), self.terminal_goal.data_ptr() if self.terminal_goal is not None else 0)
        # the launches go to the caller's CURRENT torch stream (looked up at every call): ordered against the caller's work on both sides
        # without events (torch's default stream has the null handle; BatchEnv.set_stream maps it to the legacy default stream)
        self._stream_handle = None
        self.expert_draw_calls = 0                                  # amp_expert_draw's own call counter (the context's is the host routes')
        self.stats = None
        if episode_stats:
            self.stats = EpisodeStats(self.n, self.device, bins=episode_bins, bin_steps=episode_bin_steps, lib_path=env_kwargs.get("lib_path"))
            self.episode_return = torch.zeros(self.n, **f32); self.episode_length = torch.zeros(self.n, **i32)
        self.tw = None
        if time_warp:
            self.tw = TimeWarp(self.env, tables, device=self.device)
            self.time_warp_return = torch.zeros(self.n, **f32)
            self._tw_restart = torch.ones(self.n, **i32)            # envs reset since their last sample: all before the first step, `done` of the last step after it
        self.link_names = list(tables.joint_names)
        self.deferred_reset = bool(deferred_reset)
        self.ls = LinkState(self.env, SIM, device=self.device) if link_state else None
        self.kin_ls = LinkState(self.env, KIN, device=self.device) if kin_link_state else None
        self._done_i32 = torch.zeros(self.n, **i32) if deferred_reset else None      # dm_reset_where's mask
        offsets = [float(o) for o in kin_lookahead]
        self.kin_ahead = KinQuery(self.env, len(offsets), device=self.device) if offsets else None
        self.kin_ahead_times = torch.tensor(offsets, dtype=torch.float64, device=self.device) if offsets else None
        self._queries = {}                                          # kin_query(): one KinQuery per K
        self._clip_table = None
        self._start_sampler = None
        self.start_bad = None                                       # int32 [1], set_start_sampler: becomes 1 when a sampler handed in an invalid start
        self._pool = None                                           # state_pool(): the pool a start sampler's "slots" index
        self._pool_mask = None
        self.has_pushes = bool(self.env.has_pushes)                 # pushes=True, or a scene with a finite random schedule: push() / clear_pushes() work
        self.pushes = torch.zeros((self.n, pu.PUSH_SLOTS, pu.PUSH_W), **f32) if pushes else None
        self.push_bad = torch.zeros(1, **i32) if self.has_pushes else None      # int32 [1]: becomes 1 when a push() named an invalid value (read by check=True)
        self._push_all = None

    def _enter(self):
        h = stream_handle(self.device)
        if h != self._stream_handle:
            self.env.set_stream(h); self._stream_handle = h

    def _leave(self):
        pass

    def _launch(self, actions_ptr, n_updates, auto_reset, end_early=None):
        self.env.step_device(actions_ptr, self.obs.data_ptr(), self.reward.data_ptr(), self.terminate.data_ptr(), self.valid.data_ptr(),
                             self.episode_end.data_ptr(), timestep=self.timestep, n_updates=n_updates, auto_reset=auto_reset, end_early=end_early,
                             amp_ptr=self.amp_obs.data_ptr() if self.amp_obs is not None else 0)

    def reset(self):
        """Reset every env (clip time, episode length, clip and yaw drawn on the device) and return the first observations."""
        self._enter()
        self.env.reset()
        self._launch(0, 0, False)                                   # RecordState of the reset state, no update
        if self.pushes is not None:
            pu.push_state_device(self.env, self.pushes.data_ptr())
        self._leave()
        if self.stats is not None:
            self.stats.reset_carry()                                # episodes in flight are dropped, not counted
        if self.tw is not None:
            self._tw_restart.fill_(1)                               # every env starts its sample buffer over at the next step
        return self.obs

    def step(self, actions) -> Tuple["object", "object", "object", Dict[str, "object"]]:
        """One control step for every env.  `actions`: (N, A) float32 on this device.  Envs whose episode ended during the step are
        reset inside the launch; their `obs` row is already the first observation of the next episode, `reward` / `terminate` describe
        the step that ended (eTerminateNull 0 / Fail 1 / Succ 2; episode_end also covers the episode timer).  The observation (and, in a goal
        scene, the goal) such an env had when its episode ended -- the path-end state a critic bootstraps a timer end from, learning/ppo_agent.py:251-266 --
        is info["terminal_obs"] / info["terminal_goal"]: (N, S) / (N, G) tensors whose row i is meaningful where done[i] is set in THIS step (other
        rows keep what an earlier step left there).  deepmimic_amd.returns.td_lambda_returns turns a stacked rollout of these into critic targets.
        With `episode_stats`, info["episode_return"] / info["episode_length"] are the running return and length of the episode each env's step belongs to, this
        step included: the finished episode's figures where done[i] is set (deepmimic_amd/episodes.py).
        `done` = every env that was reset inside the launch: episode_end (cDeepMimicCore::IsEpisodeEnd) OR an INVALID episode (valid == 0:
        cSceneSimChar::CheckValidEpisode failed, a link velocity beyond 100 -- the reference's driver ends and DISCARDS such an episode,
        DeepMimic.py:62-80 / learning/rl_agent.py end_episode; info["valid"] tells the two apart).  A learner that bootstraps across a row with
        done == False can therefore never stitch two episodes together."""
        tensor_arg("actions", actions, self.device, self.torch.float32, [(self.n, self.act_dim)])
        self._enter()
        if self.tw is not None:
            self.tw.sample(self._tw_restart)                        # the state at entry of the control step (cRLSceneSimChar::PreUpdate)
        self._launch(actions.data_ptr(), self.updates, not self.deferred_reset, end_early=True)      # (an episode ends at the update that ends it, on both routes)
        info = {"terminate": self.terminate, "valid": self.valid}
        if self.amp_obs is not None:
            info["amp_obs"] = self.amp_obs
        if self.goal_dim:
            self.env.last_goals_device(self.goal.data_ptr())        # device-to-device on the same stream, behind the step kernel: no host sync
            info["goal"] = self.goal
        if self.terminal_obs is not None:
            info["terminal_obs"] = self.terminal_obs
            if self.terminal_goal is not None:
                info["terminal_goal"] = self.terminal_goal
        done = (self.episode_end != 0) | (self.valid == 0)
        self._link_info(info)                                       # (auto-reset: done envs are in their new episode; deferred: every env at the end of the step)
        if self.pushes is not None:
            pu.push_state_device(self.env, self.pushes.data_ptr())
            info["pushes"] = self.pushes
        if self.deferred_reset:
            # what the auto-reset launch does behind its outputs, as launches of their own: the rows of the moment the episode ended go to terminal_obs /
            # terminal_goal (other rows keep their bytes), then the done envs start their next episode and obs / goal get its first rows
            d = done.unsqueeze(1)
            if self.terminal_obs is not None:
                self.torch.where(d, self.obs, self.terminal_obs, out=self.terminal_obs)
                if self.terminal_goal is not None:
                    self.torch.where(d, self.goal, self.terminal_goal, out=self.terminal_goal)
            self._done_i32.copy_(done)
            if self._start_sampler is None:
                reset_where_device(self.env, self._done_i32.data_ptr(), self.obs.data_ptr(), self.goal.data_ptr() if self.goal_dim else 0)
            else:
                self._reset_at(self._start_sampler(self._done_i32, info))
        self._leave()
        if self.tw is not None:
            self._tw_restart.copy_(done)                            # (done is bool: its int32 form is both the alignment's selection and the next step's restart marks)
            self.tw.align(self._tw_restart, out=(self.time_warp_return, None), stream=self._stream_handle)
            info["time_warp_return"] = self.time_warp_return
        if self.stats is not None:
            self.stats.update(self.reward if self.tw is None else self.time_warp_return, self.terminate, done, self.valid, out=(self.episode_return, self.episode_length))
            info["episode_return"], info["episode_length"] = self.episode_return, self.episode_length
        return self.obs, self.reward, done, info

    def _link_info(self, info):
        for ls, prefix in ((self.ls, ""), (self.kin_ls, "kin_")):
            if ls is not None:
                info.update(ls.update().info(prefix))
        if self.kin_ahead is not None:
            info.update(self.kin_ahead.update(self.kin_ahead_times).info())

    def update_link_state(self) -> dict:
        """refresh the link-state tensors from the context's current state (e.g. behind `reset()`), on torch's current stream; returns them under their info keys"""
        if self.ls is None and self.kin_ls is None and self.kin_ahead is None:
            raise RuntimeError("update_link_state needs link_state=True, kin_link_state=True or kin_lookahead")
        self._enter()
        info = {}
        self._link_info(info)
        self._leave()
        return info

    def kin_query(self, times, clips=None, absolute: bool = False, identity_origin: bool = False) -> dict:
        """the kinematic character at `times` (float64 tensor on this device, [K] shared by all envs or [N, K]; offsets from every env's clip clock, or clip times
        with absolute=True -- only then may `clips`, int32 [N], name another clip of the dataset; identity_origin: the clip in its own frame), on torch's current
        stream: {"link_state" [N, K, J, 22], "link_env" [N, K, 8], "pose", "vel" [N, K, P]}.  The tensors belong to the env and are overwritten by the next
        call with the same K (deepmimic_amd/kin_query.py)."""
        K = int(times.shape[-1]) if times.dim() in (1, 2) else 0
        q = self._queries.get(K)
        if q is None:
            q = self._queries[K] = KinQuery(self.env, K, device=self.device)
        self._enter()
        q.update(times, clips, absolute=absolute, identity_origin=identity_origin)
        self._leave()
        return q.info(prefix="")

    def clip_table(self):
        """(durations, cdf) of the dataset's clips as float64 tensors [num_clips] on this device: what a start sampler scales its times by"""
        if self._clip_table is None:
            d, c = self.env.clip_table()
            self._clip_table = (self.torch.as_tensor(d, device=self.device), self.torch.as_tensor(c, device=self.device))
        return self._clip_table

    def set_start_sampler(self, fn):
        """let the task choose where new episodes start (deferred_reset=True only; None: back to the device's own draws).  `step` calls
        fn(done_i32, info) -> dict before it resets the done envs -- done_i32: int32 [N], 1 where the env's episode ended in this step; info: the step's info, link
        states included, describing the END of the step -- and resets through dm_reset_where_at with the dict's optional "clips" (int32 [N], -1: drawn), "times"
        (float64 [N] clip times, NaN: drawn) and "yaw" (float64 [N], NaN: the scene's rule) on this device; rows of envs that are not done are ignored.  An invalid
        value (clip id outside the dataset, negative or infinite time, infinite yaw) leaves that env as it is and sets `start_bad[0]`, which nobody reads on the
        way: check it when a run misbehaves.
        With a pool (`state_pool()`) the dict may hold "slots" (int32 [N], -1: none) instead of or beside the others: a done env with slots[i] >= 0 starts a new
        episode at the state stored in that slot (StatePool.restore(new_episode=True)) and the other done envs are reset as above -- two launches with disjoint
        masks.  A slot index outside the pool leaves the env as it is and sets the pool's `bad[0]`.  Not with time_warp=True (a ValueError in `step`): the
        sample buffer of a time-warp episode starts on the reference motion."""
        if not self.deferred_reset:
            raise ValueError("set_start_sampler needs deferred_reset=True: the in-kernel auto-reset draws every start on the device")
        self._start_sampler = fn
        if fn is not None and self.start_bad is None:
            self.start_bad = self.torch.zeros(1, dtype=self.torch.int32, device=self.device)

    def _reset_at(self, start):
        t = self.torch
        ptr = {}
        for key, dtype in (("clips", t.int32), ("times", t.float64), ("yaw", t.float64)):
            x = (start or {}).get(key)
            if x is not None:
                tensor_arg("start sampler's " + key, x, self.device, dtype, [(self.n,)])
            ptr[key] = x.data_ptr() if x is not None else 0
        unknown = set(start or {}) - {"clips", "times", "yaw", "slots"}
        if unknown:
            raise ValueError("start sampler: unknown keys %s" % sorted(unknown))
        mask, slots = self._done_i32, (start or {}).get("slots")
        if slots is not None:
            if self._pool is None:
                raise ValueError("start sampler's slots need a pool: call state_pool() first")
            if self.tw is not None:
                raise ValueError("start sampler's slots cannot be used with time_warp=True")
            tensor_arg("start sampler's slots", slots, self.device, t.int32, [(self.n,)])
            if self._pool_mask is None:
                self._pool_mask = (t.zeros_like(self._done_i32), t.zeros_like(self._done_i32))
            from_pool, mask = self._pool_mask
            t.mul(self._done_i32, slots >= 0, out=from_pool); t.sub(self._done_i32, from_pool, out=mask)
        reset_where_at_device(self.env, mask.data_ptr(), ptr["clips"], ptr["times"], ptr["yaw"], self.obs.data_ptr(),
                              self.goal.data_ptr() if self.goal_dim else 0, self.start_bad.data_ptr())
        if slots is not None:
            sp.restore_device(self.env, self._pool.data.data_ptr(), self._pool.slots, from_pool.data_ptr(), slots.data_ptr(), sp.NEW_EPISODE, self.obs.data_ptr(),
                              self.goal.data_ptr() if self.goal_dim else 0, self._pool.bad.data_ptr())

    def state_pool(self, slots: int):
        """a pool of `slots` whole env states on this device (deepmimic_amd/state_pool.py): `save(mask, slots)` and `restore(mask, slots, new_episode=False)` take
        int32 (or bool) tensors [N] and run on torch's current stream without a host read; a restore writes the `obs` / `goal` rows of the restored envs.  The
        pool made last is the one a start sampler's "slots" index (set_start_sampler)."""
        self._pool = _EnvStatePool(self, slots)
        return self._pool

    def push(self, mask, links, forces, durations, slots=None, frame: str = "world", check: bool = True):
        """place task-chosen forces (deepmimic_amd/pushes.py; include/dm_hip.h dm_push_where), on torch's current stream: for every env with mask[i] != 0 (int32 or
        bool [N]) the force forces[i] (float32 or float64 [N, 3], newtons) acts on body part links[i] (int32 [N], a row of `link_names`; -1 clears) for
        durations[i] seconds (float32 or float64 [N]; +inf: until the episode's reset) from the first scene update of the next `step` on.  slots: int32 [N], 0 / 1,
        or -1 / None for a free slot, else the one nearest its end.  frame "world", or "heading": the force is given in the character's heading frame (x forward)
        and keeps the world direction it has at the time of the call.  The tensors are converted on the device.  check (default on): one host read of the
        kernel's bad word, a ValueError when some selected env had an invalid value -- a link outside [-1, J), a non-finite force, a negative or NaN duration, a
        slot outside [-1, 2); that env kept every byte, the others were served.  check=False reads nothing (`push_bad` keeps the word)."""
        t = self.torch
        if not self.has_pushes:
            raise ValueError("this env has no perturbation rows: build it with TorchVecEnv(..., pushes=True)")
        flags = pu.frame_flag(frame)
        if isinstance(mask, t.Tensor) and mask.dtype == t.bool:
            mask = mask.to(t.int32)
        tensor_arg("mask", mask, self.device, t.int32, [(self.n,)])
        tensor_arg("links", links, self.device, t.int32, [(self.n,)])
        if slots is not None:
            tensor_arg("slots", slots, self.device, t.int32, [(self.n,)])
        for name, x, shape in (("forces", forces, (self.n, 3)), ("durations", durations, (self.n,))):
            if not isinstance(x, t.Tensor) or x.device != self.device or x.dtype not in (t.float32, t.float64) or tuple(x.shape) != shape:
                raise ValueError("%s must be a float32 or float64 tensor of shape %s on %s" % (name, shape, self.device))
        forces, durations = forces.to(t.float64).contiguous(), durations.to(t.float64).contiguous()
        self._enter()
        if check:
            self.push_bad.zero_()
        pu.push_where_device(self.env, mask.data_ptr(), links.data_ptr(), forces.data_ptr(), durations.data_ptr(), slots.data_ptr() if slots is not None else 0,
                             flags, self.push_bad.data_ptr())
        self._leave()
        if check and int(self.push_bad.item()):
            raise ValueError("push: an env had an invalid value (a link outside [-1, %d), a non-finite force, a negative or NaN duration, or a slot outside [-1, 2)); "
                             "it kept its pushes, the other envs were served" % self.env.J)

    def clear_pushes(self, mask=None):
        """free both push slots of the envs with mask[i] != 0 (int32 or bool [N]; None: of every env), on torch's current stream, no host read"""
        t = self.torch
        if not self.has_pushes:
            raise ValueError("this env has no perturbation rows: build it with TorchVecEnv(..., pushes=True)")
        if self._push_all is None:
            i32 = dict(dtype=t.int32, device=self.device)
            self._push_all = (t.ones(self.n, **i32), t.full((self.n,), -1, **i32), t.zeros((self.n, 3), dtype=t.float64, device=self.device),
                              t.zeros(self.n, dtype=t.float64, device=self.device))
        ones, minus, f0, d0 = self._push_all
        self.push(ones if mask is None else mask, minus, f0, d0, slots=minus, check=False)

    def episode_totals(self) -> dict:
        """figures of the episodes finished since construction or the last `stats.clear_totals()` (episodes.decode_block): one device-to-host copy"""
        if self.stats is None:
            raise RuntimeError("episode_totals needs episode_stats=True")
        return self.stats.totals()

    def amp_expert_draw(self, n: int, out=None, return_draws: bool = False):
        """n expert AMP observations (amp_agent.py:244-249: one per agent observation) whose clips and clip times are drawn on the device, on torch's current
        stream, no host read: an (n, amp_size) float32 tensor (`out` if given), and with `return_draws` the int32 clip ids and float64 clip times behind it.
        Call k of this method draws what call k of `BatchEnv.amp_expert` / `amp_expert_clips` draws on a context of the same seed; it keeps its own counter."""
        t = self.torch
        n, w = int(n), self.env.amp_size
        if n < 1:
            raise ValueError("n must be >= 1")
        if out is None:
            out = t.empty((n, w), dtype=t.float32, device=self.device)
        elif out.device != self.device or out.dtype != t.float32 or not out.is_contiguous() or out.numel() != n * w:
            raise ValueError("out must be a contiguous float32 (n, amp_size) tensor on %s" % self.device)
        clips = t.empty(n, dtype=t.int32, device=self.device) if return_draws else None
        times = t.empty(n, dtype=t.float64, device=self.device) if return_draws else None
        self._enter()
        self.env.amp_expert_draw_device(n, self.expert_draw_calls, out.data_ptr(), clips_out_ptr=clips.data_ptr() if return_draws else 0,
                                        times_out_ptr=times.data_ptr() if return_draws else 0)
        self._leave()
        self.expert_draw_calls += 1
        return (out, clips, times) if return_draws else out

    def close(self):
        self.env.close()


class TorchVecEnvGroups:
    """`TorchVecEnv` as G env groups on their own streams (deepmimic_amd/groups.py; round 4): the batch's tensors are shared, group g owns the rows
    `rows(g)`, and its control step runs on `stream(g)` -- a learner runs policy(g) on that stream right before `step_group(g, ...)` and works on
    another group meanwhile, the way double-buffered samplers do; the groups then drift apart in phase and fill each other's wave-time tail
    (closed loop with the on-device policy, 4096 humanoids: 2.14 M env-steps/s against 2.05 M with one launch per step, profiles/r04_policy_bench.json).
    `step(actions)` is the synchronous convenience: all groups, then the caller's current stream waits for them.  Env i follows the same trajectory
    as in a `TorchVecEnv` of the whole batch (draws are keyed by the global env id; tests/test_vec_env.py).
    `time_warp=True` as in `TorchVecEnv`: each group samples and aligns its rows of whole-batch buffers (N * 2 * capacity * 3J * sizeof(Real) bytes) on its own
    stream, info["time_warp_return"] is row for row what the ungrouped env hands out, and with `episode_stats` the statistics accumulate it in place of `reward`."""

    def __init__(self, tables: SceneTables, num_envs: int, groups: int = 2, device: str = "cuda:0", seed: int = 0, timestep: float = 1.0 / 600,
                 updates_per_step: int = 20, amp_obs: bool = False, terminal_obs: bool = True, episode_stats: bool = False, episode_bins: int = 0,
                 episode_bin_steps: int = 1, time_warp: bool = False, **env_kwargs):
        import torch
        from .groups import EnvGroups
        self.torch = torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TorchVecEnvGroups needs a GPU device (deepmimic_amd has no CPU path)")
        if time_warp and buffer_size(tables.cfg, tables.query_rate) is None:
            raise ValueError("time_warp=True: " + why_no_warper(tables.cfg))
        with torch.cuda.device(self.device):
            torch.zeros(1, device=self.device)
            self.g = EnvGroups(tables, num_envs, groups=groups, device_id=self.device.index or 0, seed=seed, **env_kwargs)
        self.G, self.n, self.obs_dim, self.act_dim = self.g.G, self.g.N, self.g.S, self.g.A
        self.goal_dim = self.g.envs[0].G
        self.timestep, self.updates = float(timestep), int(updates_per_step)
        f32, i32 = dict(dtype=torch.float32, device=self.device), dict(dtype=torch.int32, device=self.device)
        self.obs = torch.zeros((self.n, self.obs_dim), **f32); self.reward = torch.zeros(self.n, **f32)
        self.terminate = torch.zeros(self.n, **i32); self.valid = torch.zeros(self.n, **i32); self.episode_end = torch.zeros(self.n, **i32)
        self.amp_obs = torch.zeros((self.n, self.g.amp_size), **f32) if (amp_obs and self.g.amp_size) else None
        self.goal = torch.zeros((self.n, self.goal_dim), **f32) if self.goal_dim else None
        # terminal observation / goal as in TorchVecEnv: whole-batch tensors, each group's context bound to its own rows
        self.terminal_obs = torch.zeros((self.n, self.obs_dim), **f32) if terminal_obs else None
        self.terminal_goal = torch.zeros((self.n, self.goal_dim), **f32) if (terminal_obs and self.goal_dim) else None
        for g, e in enumerate(self.g.envs if terminal_obs else []):
            r = self.g.rows(g)
            e.set_terminal_outputs(self.terminal_obs[r].data_ptr(), self.terminal_goal[r].data_ptr() if self.terminal_goal is not None else 0)
        # the contexts' own streams (created back to back: distinct hardware queues), visible to torch as external streams
        self.streams = [torch.cuda.ExternalStream(e.own_stream(), device=self.device) for e in self.g.envs]
        # episode statistics as in TorchVecEnv: one EpisodeStats per group, on its rows of whole-batch carries and on its stream; totals merged in group order
        self.stats = None
        if episode_stats:
            self.episode_return = torch.zeros(self.n, **f32); self.episode_length = torch.zeros(self.n, **i32)
            self._acc_return = torch.zeros(self.n, dtype=torch.float64, device=self.device); self._acc_len = torch.zeros(self.n, **i32)
            self.stats = [EpisodeStats(self.g.count[g], self.device, bins=episode_bins, bin_steps=episode_bin_steps,
                                       lib_path=env_kwargs.get("lib_path"), carry=(self._acc_return[self.rows(g)], self._acc_len[self.rows(g)])) for g in range(self.G)]
        # the time-warp return as in TorchVecEnv: one TimeWarp per group, on its rows of whole-batch sample buffers and on its stream
        self.tw = None
        if time_warp:
            cap = buffer_size(tables.cfg, tables.query_rate)
            self.time_warp_return = torch.zeros(self.n, **f32); self._tw_restart = torch.ones(self.n, **i32)
            self._tw_samples = torch.zeros((self.n, 2, cap, 3 * self.g.J), dtype=torch.float64 if self.g.envs[0].precision == 64 else torch.float32, device=self.device)
            self._tw_count = torch.zeros(self.n, **i32)
            self.tw = [TimeWarp(self.g.envs[g], tables, device=self.device, buffers=(self._tw_samples[self.rows(g)], self._tw_count[self.rows(g)])) for g in range(self.G)]

    def rows(self, g: int) -> slice:
        return self.g.rows(g)

    def stream(self, g: int):
        return self.streams[g]

    def _launch(self, g, actions_ptr, n_updates, auto_reset):
        if self.tw is not None and n_updates:
            self.tw[g].sample(self._tw_restart[self.rows(g)])      # in front of the step launch, on the group's stream
        self.g.step_group_device(g, actions_ptr, self.obs.data_ptr(), self.reward.data_ptr(), self.terminate.data_ptr(), self.valid.data_ptr(),
                                 self.episode_end.data_ptr(), timestep=self.timestep, n_updates=n_updates, auto_reset=auto_reset,
                                 amp_ptr=self.amp_obs.data_ptr() if self.amp_obs is not None else 0)
        if self.goal is not None and n_updates:
            self.g.envs[g].last_goals_device(self.goal[self.rows(g)].data_ptr())      # device-to-device on the group's stream, behind its kernel

    def _info(self, r):
        info = {"terminate": self.terminate[r], "valid": self.valid[r]}
        if self.amp_obs is not None:
            info["amp_obs"] = self.amp_obs[r]
        if self.goal is not None:
            info["goal"] = self.goal[r]
        if self.terminal_obs is not None:       # rows meaningful where `done` is set in this step (TorchVecEnv.step)
            info["terminal_obs"] = self.terminal_obs[r]
            if self.terminal_goal is not None:
                info["terminal_goal"] = self.terminal_goal[r]
        if self.stats is not None:
            info["episode_return"], info["episode_length"] = self.episode_return[r], self.episode_length[r]
        if self.tw is not None:
            info["time_warp_return"] = self.time_warp_return[r]
        return info

    def _episode_update(self, g, done):
        """behind group g's step launch, on its rows: the time-warp return of the envs that ended, then EpisodeStats.update (on that return where there is one);
        the caller has made `stream(g)` torch's current stream"""
        r = self.rows(g)
        if self.tw is not None:
            self._tw_restart[r].copy_(done)
            self.tw[g].align(self._tw_restart[r], out=(self.time_warp_return[r], None), stream=self.streams[g].cuda_stream)
        if self.stats is not None:
            self.stats[g].update(self.reward[r] if self.tw is None else self.time_warp_return[r], self.terminate[r], done, self.valid[r],
                                 out=(self.episode_return[r], self.episode_length[r]))

    def reset(self):
        self.g.reset()
        cur = self.torch.cuda.current_stream(self.device)
        for g in range(self.G):
            self.streams[g].wait_stream(cur)      # reads of self.obs the caller still has queued on its stream come first (write-after-read)
            self._launch(g, 0, 0, False)
            if self.stats is not None or self.tw is not None:
                with self.torch.cuda.stream(self.streams[g]):
                    if self.stats is not None:
                        self.stats[g].reset_carry()   # episodes in flight are dropped, not counted
                    if self.tw is not None:
                        self._tw_restart[self.rows(g)].fill_(1)
        self._join()
        return self.obs

    def _check_actions(self, actions):
        tensor_arg("actions", actions, self.device, self.torch.float32, [(self.n, self.act_dim)])       # the whole batch's tensor

    def step_group(self, g: int, actions):
        """Control step of group g, asynchronous on `stream(g)`.  `actions`: the WHOLE batch's (N, A) tensor (the group reads its rows) written on
        `stream(g)` (or ordered before it by the caller).  Returns views of the group's rows: (obs, reward, done, info) -- valid on `stream(g)`."""
        t = self.torch
        self._check_actions(actions)
        self._launch(g, actions.data_ptr(), self.updates, True)
        r = self.rows(g)
        with t.cuda.stream(self.streams[g]):
            done = (self.episode_end[r] != 0) | (self.valid[r] == 0)
            if self.stats is not None or self.tw is not None:
                self._episode_update(g, done)
        return self.obs[r], self.reward[r], done, self._info(r)

    def _join(self):
        cur = self.torch.cuda.current_stream(self.device)
        for s in self.streams:
            cur.wait_stream(s)

    def step(self, actions):
        """all groups (each on its stream, ordered behind the caller's current stream), then the current stream waits for them"""
        self._check_actions(actions)             # (a float64 / transposed / CPU tensor would be read as raw fp32 rows)
        cur = self.torch.cuda.current_stream(self.device)
        for g in range(self.G):
            self.streams[g].wait_stream(cur)
            self._launch(g, actions.data_ptr(), self.updates, True)
            if self.stats is not None or self.tw is not None:
                r = self.rows(g)
                with self.torch.cuda.stream(self.streams[g]):
                    self._episode_update(g, (self.episode_end[r] != 0) | (self.valid[r] == 0))
        self._join()
        return self.obs, self.reward, (self.episode_end != 0) | (self.valid == 0), self._info(slice(None))

    def episode_totals(self) -> dict:
        """as TorchVecEnv.episode_totals: the groups' blocks merged in group order (the current stream waits for the groups' streams first)"""
        if self.stats is None:
            raise RuntimeError("episode_totals needs episode_stats=True")
        self._join()
        return decode_block(merge_blocks([s.raw() for s in self.stats]), self.stats[0].bin_steps)

    def close(self):
        self.g.close()
