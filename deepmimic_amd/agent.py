"""The learner: PPO and AMP agents that train end to end on the device pieces, from the reference's own agent files (learning/rl_agent.py, pg_agent.py,
ppo_agent.py, amp_agent.py; data/agents/*.txt).  One process owns a `TorchVecEnv` of N envs; an iteration is T control steps of all of them into a
device-resident `Rollout` (`collect`), one update over its T x N samples (`update`: for AMP the discriminator's data, its steps and the batch rewards first; then
critic values, TD(lambda), advantages and the minibatches of critic then actor) and the bookkeeping of rl_agent.py:485-546 with one log row (`iterate`).
INTEGRATION.md section 4 has the calls and what differs from the reference.

Every number the pieces are keyed by is a function of (seed, iteration, position): `keys(iteration)`.  Two agents with one seed on one scene produce the same bytes.
`collect` copies out of the env's tensors into the rollout (the actor alone writes straight into the slot): the env keeps one set of output buffers bound to its context.
The nets take the normalisers' statistics as float32 mean / std through `set_weights` -- the numbers a checkpoint holds -- so that a model written by `save_model`
evaluates bit for bit like the live nets when read back (`bind_policy` hands over float(1 / std64), an ulp away from 1 / float(std) in many columns): one host round trip
per iteration while samples < NormalizerSamples, none afterwards; the same read serves State_Mean / State_Std."""
from __future__ import annotations

import json
import math
import os
import time
from typing import Optional

import numpy as np

from . import amp_rewards, ppo_batch, replay, returns, tf_checkpoint, train
from .binding import stream_handle, tensor_arg
from .episodes import EpisodeStats
from .heads import Critic, Discriminator
from .normalizer import DeviceNormalizer
from .policy import Policy, random_weights

NETS = ("fc_2layers_1024units", "fc_2layers_gated_1024units")
AGENT_TYPES = ("PPO", "AMP")
ADV_EPS = 1e-5                   # ppo_agent.py:27
ACTOR_BOUND_LOSS_WEIGHT = 10.0   # ppo_agent.py:96

# key of the agent file -> (attribute, the reference's default, conversion); rl_agent.py:55-76, 233-268, pg_agent.py:124-127, ppo_agent.py:36-41, amp_agent.py:58-68, 108-139
_KEYS = {
    "ActorStepsize": ("actor_stepsize", 0.001, float), "ActorMomentum": ("actor_momentum", 0.9, float), "ActorWeightDecay": ("actor_weight_decay", 0.0, float),
    "ActorInitOutputScale": ("actor_init_output_scale", 1.0, float),
    "CriticStepsize": ("critic_stepsize", 0.01, float), "CriticMomentum": ("critic_momentum", 0.9, float), "CriticWeightDecay": ("critic_weight_decay", 0.0, float),
    "ItersPerUpdate": ("iters_per_update", 1, int), "Discount": ("discount", 0.95, float), "MiniBatchSize": ("mini_batch_size", 32, int),
    "ReplayBufferSize": ("replay_buffer_size", 50000, int), "InitSamples": ("init_samples", 1000, int), "NormalizerSamples": ("normalizer_samples", math.inf, float),
    "OutputIters": ("output_iters", 100, int), "IntOutputIters": ("int_output_iters", 100, int), "TestEpisodes": ("test_episodes", 0, int),
    "ExpAnnealSamples": ("exp_anneal_samples", 320000, float),
    "Epochs": ("epochs", 1, int), "BatchSize": ("batch_size", 1024, int), "RatioClip": ("ratio_clip", 0.2, float), "NormAdvClip": ("norm_adv_clip", 5.0, float),
    "TDLambda": ("td_lambda", 0.95, float), "TarClipFrac": ("tar_clip_frac", -1.0, float),
}
_AMP_KEYS = {
    "TaskRewardLerp": ("task_reward_lerp", 0.5, float), "DiscInitOutputScale": ("disc_init_output_scale", 1.0, float), "DiscWeightDecay": ("disc_weight_decay", 0.0, float),
    "DiscLogitRegWeight": ("disc_logit_reg_weight", 0.0, float), "DiscStepSize": ("disc_stepsize", 0.001, float), "DiscMomentum": ("disc_momentum", 0.9, float),
    "DiscBatchSize": ("disc_batch_size", 256, int), "DiscStepsPerBatch": ("disc_steps_per_batch", 1, int), "DiscExpertBufferSize": ("disc_expert_buffer_size", 100000, int),
    "DiscAgentBufferSize": ("disc_agent_buffer_size", 100000, int), "RewardScale": ("reward_scale", 1.0, float), "DiscGradPenalty": ("disc_grad_penalty", 0.0, float),
}
EXP_RATE_DEFAULT, EXP_NOISE_DEFAULT = 0.2, 0.1      # learning/exp_params.py:9-12


class AgentConfig:
    """The reference's agent JSON.  Attributes are the snake-case names of `_KEYS` / `_AMP_KEYS` plus agent_type, actor_net, critic_net, disc_net,
    exp_beg / exp_end ((rate, noise) pairs); a key that is absent has the reference's default.  `ignored`: the keys of the file no agent here reads (kept in `raw`)."""

    def __init__(self, d: dict):
        if not isinstance(d, dict):
            raise ValueError("an agent file is a JSON object")
        self.raw = dict(d)
        self.agent_type = d.get("AgentType")
        if self.agent_type not in AGENT_TYPES:
            raise ValueError("unsupported AgentType %r: this learner builds %s" % (self.agent_type, " and ".join(AGENT_TYPES)))
        amp = self.agent_type == "AMP"
        nets = [("ActorNet", "actor_net"), ("CriticNet", "critic_net")] + ([("DiscNet", "disc_net")] if amp else [])
        self.disc_net = None
        for key, attr in nets:
            if key not in d:
                raise ValueError("the agent file names no %s" % key)
            if d[key] not in NETS:
                raise ValueError("unsupported %s %r: the device nets are %s" % (key, d[key], " and ".join(NETS)))
            setattr(self, attr, d[key])
        if amp and self.disc_net != NETS[0]:
            raise ValueError("unsupported DiscNet %r: the AMP discriminator is the plain %s" % (self.disc_net, NETS[0]))
        table = dict(_KEYS)
        if amp:
            table.update(_AMP_KEYS)
        for key, (attr, default, conv) in table.items():
            setattr(self, attr, conv(d[key]) if key in d else default)
        def exp(key):
            e = d.get(key, {})
            return (float(e.get("Rate", EXP_RATE_DEFAULT)), float(e.get("Noise", EXP_NOISE_DEFAULT)))
        self.exp_beg, self.exp_end = exp("ExpParamsBeg"), exp("ExpParamsEnd")
        if self.exp_beg[1] != self.exp_end[1]:
            raise ValueError("ExpParamsBeg and ExpParamsEnd must name one Noise: the noise std does not change (rl_agent.py:277)")
        known = set(table) | {"AgentType", "ExpParamsBeg", "ExpParamsEnd"} | {k for k, _ in nets}
        self.ignored = sorted(k for k in d if k not in known)

    @classmethod
    def from_dict(cls, d: dict) -> "AgentConfig":
        return cls(d)

    @classmethod
    def from_file(cls, path: str) -> "AgentConfig":
        with open(path) as f:
            return cls(json.load(f))

    def exp_params(self, samples) -> tuple:
        """(rate, noise) after `samples` samples: rl_agent.py:345-349, ExpParams.lerp"""
        t = float(np.clip(float(samples) / self.exp_anneal_samples, 0.0, 1.0))
        return tuple((1 - t) * b + t * e for b, e in zip(self.exp_beg, self.exp_end))


def _mix(seed: int, tag: int) -> int:
    """splitmix64 of seed + tag: the seeds the agent hands out"""
    z = (int(seed) * 0x9E3779B97F4A7C15 + (int(tag) + 1) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    return z ^ (z >> 31)


_TAG_ACTOR, _TAG_GATHER, _TAG_AGENT_STORE, _TAG_EXPERT_STORE, _TAG_ENV, _TAG_INIT = range(6)


class Rollout:
    """T control steps of N envs on the device, time-major: obs / goal [T + 1, N, .] (row T: behind the last step), act, logp, flags, reward (the env's), terminate,
    done, valid, terminal_obs / terminal_goal [T, N, .], amp_obs [T, N, AMP] (AMP agents)"""

    def __init__(self, T, N, S, G, A, AMP, device):
        import torch
        f32, i32 = dict(dtype=torch.float32, device=device), dict(dtype=torch.int32, device=device)
        self.T, self.N = T, N
        self.obs = torch.zeros((T + 1, N, S), **f32); self.goal = torch.zeros((T + 1, N, G), **f32) if G else None
        self.act = torch.zeros((T, N, A), **f32); self.logp = torch.zeros((T, N), **f32); self.flags = torch.zeros((T, N), **i32)
        self.reward = torch.zeros((T, N), **f32)
        self.terminate, self.done, self.valid = (torch.zeros((T, N), **i32) for _ in range(3))
        self.terminal_obs = torch.zeros((T, N, S), **f32); self.terminal_goal = torch.zeros((T, N, G), **f32) if G else None
        self.amp_obs = torch.zeros((T, N, AMP), **f32) if AMP else None


# the variables of a net under <scope>/main/<net>/ by the key of the weights dict
_NET_VARIABLES = {"w1": "0/dense/kernel", "b1": "0/dense/bias", "w2": "1/dense/kernel", "b2": "1/dense/bias"}
_OUT_LAYER = {"actor": "dist_gauss_diag/mean", "critic": "dense", "disc": "disc_logits"}

LOG_COLUMNS = ("Iteration", "Wall_Time", "Samples", "Train_Return", "Test_Return", "State_Mean", "State_Std", "Goal_Mean", "Goal_Std", "Exp_Rate", "Exp_Noise",
               "Critic_Loss", "Actor_Loss", "Clip_Frac", "Adv_Mean", "Adv_Std")
AMP_LOG_COLUMNS = ("Disc_Loss", "Disc_Acc_Expert", "Disc_Acc_Agent", "Disc_Prob", "Disc_Abs_Logit", "Disc_Reward_Mean", "Disc_Reward_Std", "Grad_Penalty", "Disc_Steps")
OPT_LOG_COLUMNS = ("Skipped_Steps", "Grad_Norm")


class PPOAgent:
    KIND = "PPO"

    def __init__(self, env, cfg: AgentConfig, rollout_steps: int = 32, seed: int = 0, mini_batch_size: Optional[int] = None, optimizer: str = "momentum",
                 init_from: Optional[str] = None, reward_fn=None, goal_fn=None, goal_dim: int = 0, push_fn=None, **opt):
        """env: a `TorchVecEnv` (an AMP agent: with amp_obs=True).  rollout_steps: T; a rollout is T x N samples, the file's BatchSize is logged next to it, not
        enforced.  mini_batch_size: M (None: the file's MiniBatchSize).  optimizer / **opt (max_grad_norm, skip_nonfinite, betas, eps): the trainers'.
        init_from: a checkpoint prefix whose nets and normalisers the agent starts from instead of random weights.
        reward_fn: a task written in torch -- a callable (info, reward) -> float32 [N] tensor on the env's device, called behind every env.step of `collect` with
        the step's info dict (info["link_state"] and the like with `TorchVecEnv(link_state=True, deferred_reset=True)`) and the env's reward; its result is stored
        in the rollout IN PLACE OF the env's reward (an AMP agent: in place of the task reward the style reward is blended with).  None: the env's reward.
        goal_fn / goal_dim: an observation written in torch -- goal_fn(info) -> float32 [N, goal_dim] on the env's device becomes the goal block of actor and
        critic, as the goal of a goal scene does (G = goal_dim: goal normaliser, rollout goal / terminal_goal, gated nets, checkpoints).  It needs a scene without
        a goal of its own and `TorchVecEnv(..., deferred_reset=True)` with link states or kin_lookahead (info is what `env.update_link_state()` returns, plus the
        step's keys behind a step).  Per step of `collect` and `test`: env.step; reward_fn and goal_fn on the end-of-step tensors -- that goal is the terminal
        goal where done; env.update_link_state(), after which the done envs show their new episode (the others the same bytes); goal_fn again: the goal the
        next action is taken from.
        push_fn: pushes chosen by the task -- a callable (info, t) -> None or a dict of `TorchVecEnv.push`'s arguments, called by `collect` before every env.step
        (t: the step of the rollout) and applied with env.push(**dict); it needs `TorchVecEnv(..., pushes=True)`.  info holds the tensors the action was computed
        from: the last step's info dict (empty before the first step behind a reset of every env) plus "obs", "goal" where there is one, and "pushes".
        pushes.RandomPushes is such a callable.  `test` does not push.  None: `collect` does what it did."""
        import torch
        self.torch = torch
        if cfg.agent_type != self.KIND:
            raise ValueError("%s built from an agent file of AgentType %s" % (type(self).__name__, cfg.agent_type))
        bad = [k for k in opt if k not in ("max_grad_norm", "skip_nonfinite", "betas", "eps")]
        if bad:
            raise TypeError("unknown optimiser option %s" % bad[0])
        self.env, self.cfg, self.seed = env, cfg, int(seed)
        self.reward_fn, self.goal_fn, self.push_fn = reward_fn, goal_fn, push_fn
        if push_fn is not None and not getattr(env, "has_pushes", False):
            raise ValueError("push_fn needs TorchVecEnv(..., pushes=True)")
        self._step_info = {}                                        # push_fn: the info dict of the last env.step
        self.device = env.device
        self.T, self.N, self.S, self.G, self.A = int(rollout_steps), env.n, env.obs_dim, env.goal_dim, env.act_dim
        if goal_fn is None and goal_dim:
            raise ValueError("goal_dim without goal_fn")
        if goal_fn is not None:
            if env.goal_dim:
                raise ValueError("goal_fn: the scene has a goal of its own (env.goal_dim = %d)" % env.goal_dim)
            if int(goal_dim) < 1:
                raise ValueError("goal_fn needs goal_dim >= 1")
            if not getattr(env, "deferred_reset", False):
                raise ValueError("goal_fn needs TorchVecEnv(..., deferred_reset=True): the terminal goal is computed from the end-of-step link states")
            self.G = int(goal_dim)
            self._goal = torch.zeros((self.N, self.G), dtype=torch.float32, device=self.device)        # the goal the next action is taken from
        self.AMP = 0
        if self.T < 1:
            raise ValueError("rollout_steps must be >= 1")
        self.M = int(cfg.mini_batch_size if mini_batch_size is None else mini_batch_size)
        if self.M < 1:
            raise ValueError("mini_batch_size must be >= 1")
        self.gated_actor, self.gated_critic = cfg.actor_net == NETS[1], cfg.critic_net == NETS[1]
        if (self.gated_actor or self.gated_critic) and not self.G:
            raise ValueError("%s gates on the goal: this scene has none" % NETS[1])
        self._opt = dict(optimizer=optimizer, **opt)
        self.iteration, self.samples, self.empty_rollouts = 0, 0, 0
        self.initialized = cfg.init_samples <= 0
        self.recording = cfg.normalizer_samples > 0
        self.exp_rate, self.exp_noise = cfg.exp_params(0)
        self.train_return, self.test_return = 0.0, 0.0
        self.log, self._t0, self._wall0 = [], time.time(), 0.0
        self._setup_scene()
        self._build_nets(init_from)
        self._build_rest()
        self.rollout = Rollout(self.T, self.N, self.S, self.G, self.A, self.AMP, self.device)
        self._zero_values = torch.zeros((self.T + 1, self.N), dtype=torch.float32, device=self.device)
        self._sums = torch.zeros(self._N_SUMS, dtype=torch.float64, device=self.device)
        self._norm_stats = None
        self._refresh_nets()
        self._begin(self.env.reset())

    # ---- construction
    def _setup_scene(self):
        offs = self.env.env.offsets_scales()
        self.a_mean, self.a_std = (-offs["action_offset"]).astype(np.float32), (1.0 / offs["action_scale"]).astype(np.float32)
        self.a_bound_min, self.a_bound_max = offs["action_min"].astype(np.float32), offs["action_max"].astype(np.float32)
        g = self.cfg.discount
        # rl_agent.py:385-423 with the scene's reward range [0, 1], fail 0, succ 1 (sim/DeepMimicCharController.cpp, scenes/RLScene.cpp)
        self.val_min, self.val_max = 0.0 / (1.0 - g), 1.0 / (1.0 - g)
        self.val_fail, self.val_succ = (0.0, 0.0) if g == 0 else (0.0 / (1.0 - g), 1.0 / (1.0 - g))
        dev = self.device.index or 0
        self.s_norm = DeviceNormalizer(self.S, groups_ids=offs["state_norm_groups"], device_id=dev)
        self.s_norm.set_mean_std(-offs["state_offset"], 1.0 / offs["state_scale"])
        self.g_norm = None
        if self.G:
            # cRLSceneSimChar::BuildGoalOffsetScale / BuildGoalNormGroups: offset 0, scale 1, every column a group of its own
            self.g_norm = DeviceNormalizer(self.G, device_id=dev)
            self.g_norm.set_mean_std(np.zeros(self.G), np.ones(self.G))

    def _norms(self) -> dict:
        return {k: n for k, n in (("s", self.s_norm), ("g", self.g_norm)) if n is not None}

    def _random_nets(self) -> dict:
        c = self.cfg
        init = _mix(self.seed, _TAG_INIT)
        SG = self.S + self.G
        actor = random_weights(SG, self.A, seed=init & 0x7FFFFFFF, init_output_scale=c.actor_init_output_scale, noise=self.exp_noise,
                               gated_goal_dim=self.G if self.gated_actor else 0)
        critic = random_weights(SG, 1, seed=(init >> 8) & 0x7FFFFFFF, gated_goal_dim=self.G if self.gated_critic else 0)
        lim = math.sqrt(6.0 / (critic["w2"].shape[1] + 1))      # pg_agent.py:166-168: the value layer is Xavier
        critic["w3"] = np.random.default_rng((init >> 16) & 0x7FFFFFFF).uniform(-lim, lim, size=critic["w3"].shape).astype(np.float32)
        return dict(actor=actor, critic=critic)

    def _checkpoint_nets(self, prefix: str) -> dict:
        gated = tf_checkpoint.is_gated_checkpoint(prefix)
        actor = (tf_checkpoint.gated_actor_weights if gated else tf_checkpoint.actor_weights)(prefix, state_dim=self.S)
        critic = tf_checkpoint.critic_weights(prefix, state_dim=self.S)
        if gated != self.gated_actor or ("gc_w" in critic) != self.gated_critic:
            raise ValueError("%s holds %s nets, the agent file names others" % (prefix, "gated" if gated else "plain"))
        return dict(actor=actor, critic=critic)

    def _build_nets(self, init_from):
        w = self._random_nets() if init_from is None else self._checkpoint_nets(init_from)
        if init_from is not None:
            a = w["actor"]
            for key, norm in (("s", self.s_norm), ("g", self.g_norm)):
                if norm is not None and key + "_mean" in a:
                    norm.set_mean_std(a[key + "_mean"], a[key + "_std"])
            if "a_mean" in a:
                self.a_mean, self.a_std = a["a_mean"].astype(np.float32), a["a_std"].astype(np.float32)
            self._load_extra_norms(w)
        self.logstd = np.asarray(w["actor"].get("logstd", np.full(self.A, math.log(self.exp_noise))), np.float32).copy()
        strip = lambda d: {k: v for k, v in d.items() if k not in ("s_mean", "s_std", "g_mean", "g_std", "a_mean", "a_std", "logstd")}
        dev = self.device.index or 0
        aw = strip(w["actor"]); aw.update(a_mean=self.a_mean, a_std=self.a_std, logstd=self.logstd)
        cw = strip(w["critic"])
        for d_, gated in ((aw, self.gated_actor), (cw, self.gated_critic)):
            if gated:
                d_["goal_dim"] = self.G
        self.actor = Policy(aw, device_id=dev)
        self.critic = Critic(cw, val_fail=self.val_fail, val_succ=self.val_succ, device_id=dev)
        c = self.cfg
        A_cls = train.GatedActorTrainer if self.gated_actor else train.ActorTrainer
        C_cls = train.GatedCriticTrainer if self.gated_critic else train.CriticTrainer
        self.actor_tr = A_cls.from_policy(self.actor, aw, stepsize=c.actor_stepsize, momentum=c.actor_momentum, weight_decay=c.actor_weight_decay, **self._opt)
        self.critic_tr = C_cls.from_policy(self.critic.net, cw, stepsize=c.critic_stepsize, momentum=c.critic_momentum, weight_decay=c.critic_weight_decay, **self._opt)
        self._build_extra_nets(w)

    def _load_extra_norms(self, w):
        pass

    def _build_extra_nets(self, w):
        pass

    def _build_rest(self):
        self.stats = EpisodeStats(self.N, self.device)

    def trainers(self) -> dict:
        return dict(actor=self.actor_tr, critic=self.critic_tr)

    _N_SUMS = 4       # minibatches, critic loss, actor loss, clip fraction

    # ---- the nets' input statistics
    def _obs_nets(self):
        return (self.actor, self.critic.net)

    def _refresh_nets(self):
        """the normalisers' statistics, as float32, into the nets (one host round trip; see the module text) and into the log's State_ / Goal_ columns"""
        st = {k: n.state_host() for k, n in self._norms().items()}
        self._norm_stats = st
        mean = np.concatenate([st[k]["mean"] for k in ("s", "g") if k in st]).astype(np.float32)
        std = np.concatenate([st[k]["std"] for k in ("s", "g") if k in st]).astype(np.float32)
        for net in self._obs_nets():
            net.set_weights(dict(s_mean=mean, s_std=std))

    def _set_noise(self, noise: float):
        if noise != self.exp_noise:
            self.exp_noise = noise
            self.logstd = np.full(self.A, math.log(noise), np.float32)
            self.actor.set_weights(dict(logstd=self.logstd))

    # ---- keys
    def disc_steps_max(self) -> int:
        return 0

    def keys(self, iteration: int) -> dict:
        """every seed, call counter, step index and gather epoch iteration `iteration` hands to a piece"""
        it = int(iteration)
        return dict(actor_seed=_mix(self.seed, _TAG_ACTOR), actor_step0=it * self.T, gather_seed=_mix(self.seed, _TAG_GATHER), gather_epoch0=it * self.cfg.epochs,
                    agent_store_seed=_mix(self.seed, _TAG_AGENT_STORE), expert_store_seed=_mix(self.seed, _TAG_EXPERT_STORE), append_call=it,
                    sample_call0=it * self.disc_steps_max(), expert_draw_call=it)

    def env_keys(self, key: int) -> np.ndarray:
        """the draw keys `restart_envs(key)` gives the N envs (below 2^53)"""
        base = _mix(_mix(self.seed, _TAG_ENV), int(key))
        return np.array([_mix(base, i) >> 11 for i in range(self.N)], dtype=np.uint64)

    def _begin(self, obs):
        """behind a reset of every env: the goal of the new episodes (the step launches keep it current from here on), no episode in flight"""
        if self.goal_fn is not None:
            self._goal.copy_(self._call_goal_fn(self.env.update_link_state()))
        elif self.G:
            self.env.goal.copy_(self.torch.from_numpy(np.ascontiguousarray(self.env.env.query_goal(), dtype=np.float32)))
        self.stats.reset_carry()
        self._step_info = {}

    def _call_goal_fn(self, info):
        return tensor_arg("goal_fn's result", self.goal_fn(info), self.device, self.torch.float32, [(self.N, self.G)], contiguous=False)

    def _cur_goal(self):
        """the goal block of the next forward pass: the env's (goal scenes) or goal_fn's"""
        return self._goal if self.goal_fn is not None else self.env.goal

    def _after_step(self, info):
        """goal_fn agents, behind env.step: (the terminal goal -- goal_fn on the end-of-step tensors, meaningful where done) and the next goal in self._goal --
        goal_fn behind update_link_state(), where the done envs show their new episode"""
        term = self._call_goal_fn(info).clone()
        info.update(self.env.update_link_state())
        self._goal.copy_(self._call_goal_fn(info))
        return term

    def restart_envs(self, key: int):
        """every env reset under a draw key derived from (seed, key): what `load_state` does with the iteration number, env state not being part of a checkpoint.
        (A scene without per-env draw rows -- one clip, no goal, no perturbations -- restarts its episode counters only.)"""
        self.env.env.set_env_keys(np.arange(self.N, dtype=np.int32), self.env_keys(key))
        self._begin(self.env.reset())

    # ---- sampling
    def collect(self) -> Rollout:
        env, ro, k = self.env, self.rollout, self.keys(self.iteration)
        stream = stream_handle(self.device)
        for n in self._norms().values():
            n.set_stream(stream)
        G = self.G
        for t in range(self.T):
            ro.obs[t].copy_(env.obs)
            if G:
                ro.goal[t].copy_(self._cur_goal())
            self.actor.forward_device_ex(ro.obs[t].data_ptr(), self.N, ro.act[t].data_ptr(), ro.goal[t].data_ptr() if G else 0, G, logp_ptr=ro.logp[t].data_ptr(),
                                         exp_flags_ptr=ro.flags[t].data_ptr(), exp_rate=self.exp_rate, sample=True, seed=k["actor_seed"], step=k["actor_step0"] + t,
                                         stream=stream)
            if self.push_fn is not None:
                self._push(ro, t)
            _, reward, done, info = env.step(ro.act[t])
            self._step_info = info
            if self.reward_fn is not None:
                reward = tensor_arg("reward_fn's result", self.reward_fn(info, reward), self.device, self.torch.float32, [(self.N,)], contiguous=False)
            ro.reward[t].copy_(reward); ro.terminate[t].copy_(info["terminate"]); ro.done[t].copy_(done); ro.valid[t].copy_(info["valid"])
            ro.terminal_obs[t].copy_(info["terminal_obs"])
            if G:
                ro.terminal_goal[t].copy_(info["terminal_goal"] if self.goal_fn is None else self._after_step(info))
            if ro.amp_obs is not None:
                ro.amp_obs[t].copy_(info["amp_obs"])
            if self.recording:                                       # rl_agent.py:463-476
                self.s_norm.record_device(ro.obs[t].data_ptr(), self.N)
                if G:
                    self.g_norm.record_device(ro.goal[t].data_ptr(), self.N)
        ro.obs[self.T].copy_(env.obs)
        if G:
            ro.goal[self.T].copy_(self._cur_goal())
        return ro

    def _push(self, ro, t):
        """push_fn in front of env.step: the tensors the action of step t was computed from, then the pushes it chose"""
        info = dict(self._step_info)
        info["obs"] = ro.obs[t]
        if self.G:
            info["goal"] = ro.goal[t]
        if getattr(self.env, "pushes", None) is not None:
            info["pushes"] = self.env.pushes
        push = self.push_fn(info, t)
        if push is not None:
            self.env.push(**push)

    # ---- the update
    def _valid_lists(self, ro):
        """which samples are valid depends on the flags alone: a TD pass over the env rewards with a zero critic hands out the mask, dm_ppo_advantages the list"""
        c = self.cfg
        _, mask0 = returns.td_lambda_returns_torch(ro.reward, self._zero_values, self._zero_values[:self.T], ro.terminate, ro.done, ro.valid, c.discount, c.td_lambda,
                                                   0.0, 0.0)
        return ppo_batch.advantages_torch(ro.reward, self._zero_values, mask0)

    def _rewards(self, ro, k, train_nets: bool):
        """(rewards [T, N] of the update, value bounds) -- PPO: the env's; returns None for a rollout without a valid sample"""
        return ro.reward, None

    def update(self, ro: Rollout, train_nets: bool = True) -> dict:
        """One update over `ro` under the keys of the current iteration.  train_nets False (an InitSamples rollout): the data side only -- counts, AMP stores and
        their normaliser -- no optimiser step.  Returns dict(n_valid, n_exp, minibatches)."""
        t, c, k = self.torch, self.cfg, self.keys(self.iteration)
        out = dict(n_valid=0, n_exp=0, minibatches=0)
        self._sums.zero_(); self._adv_stats = None; self._lists = None
        self._mark("disc")
        got = self._rewards(ro, k, train_nets)
        self._mark("values")
        if got is None:
            self.empty_rollouts += 1
            return out
        rewards, bounds = got
        self.stats.update(rewards, ro.terminate, ro.done, ro.valid, per_step=False)
        if not train_nets:
            out["n_valid"], out["n_exp"] = (self._valid_lists(ro) if self._lists is None else self._lists).counts_host()
            if not out["n_valid"]:
                self.empty_rollouts += 1
            return out
        ret, mask, values = returns.critic_returns_torch(self.critic, ro.obs, ro.goal, ro.terminal_obs, ro.terminal_goal, ro.terminate, ro.done, ro.valid, rewards,
                                                         c.discount, c.td_lambda, return_values=True, bounds=bounds)
        batch = ppo_batch.advantages_torch(ret, values, mask, ro.flags, adv_eps=ADV_EPS, norm_adv_clip=c.norm_adv_clip, val_min=self.val_min, val_max=self.val_max)
        self._adv_stats, self.last_batch = batch.stats, batch
        n_valid, n_exp = batch.counts_host()
        out.update(n_valid=n_valid, n_exp=n_exp)
        if not n_valid:
            self.empty_rollouts += 1
            return out
        G = self.G
        self._mark("minibatches")
        obs, goal = ro.obs[:self.T], (ro.goal[:self.T] if G else None)
        critic_cols = [obs] + ([goal] if G else []) + [batch.targets]
        actor_cols = [obs] + ([goal] if G else []) + [ro.act, ro.logp, batch.adv]
        sums = self._sums
        for e in range(c.epochs):
            for b in range(-(-n_valid // self.M)):
                cr = batch.gather("valid", b * self.M, self.M, k["gather_seed"], k["gather_epoch0"] + e, *critic_cols)
                self.critic_tr.grad(cr[0], cr[-1], goals=cr[1] if G else None); self.critic_tr.step()
                sums[0] += 1.0; sums[1] += self.critic_tr.stats()[0]
                if n_exp:                                            # (a rollout without an explored sample updates the critic only)
                    ar = batch.gather("exp", b * self.M, self.M, k["gather_seed"], k["gather_epoch0"] + e, *actor_cols)
                    self.actor_tr.grad(ar[0], ar[-3], ar[-2], ar[-1], goals=ar[1] if G else None, ratio_clip=c.ratio_clip, bound_weight=ACTOR_BOUND_LOSS_WEIGHT,
                                       a_bound_min=self.a_bound_min, a_bound_max=self.a_bound_max)
                    self.actor_tr.step()
                    s = self.actor_tr.stats()
                    sums[2] += t.abs(s[1] + ACTOR_BOUND_LOSS_WEIGHT * s[2]); sums[3] += s[3]
                out["minibatches"] += 1
        return out

    _lists = None
    _adv_stats = None
    last_batch = None            # the PPOBatch of the last training update (advantages, targets, the valid / explored lists)
    phase_mark = None            # a callable(name) called at the phase boundaries of an iteration (tools/agent_iteration_bench.py records a device event in it)

    def _mark(self, name: str):
        if self.phase_mark is not None:
            self.phase_mark(name)

    # ---- one iteration
    def iterate(self) -> dict:
        c = self.cfg
        rate, noise = self.exp_rate, self.exp_noise
        self.stats.clear_totals()
        self._mark("collect")
        ro = self.collect()
        trained = self.initialized
        info = self.update(ro, train_nets=trained)
        self._mark("bookkeeping")
        self.samples += info["n_valid"]
        if not self.initialized and self.samples >= c.init_samples:             # rl_agent.py:536-538
            self.initialized = True
        if self.recording:                                                      # rl_agent.py:540-542
            for n in self._all_norms():
                n.update()
            self._refresh_nets()
            self.recording = c.normalizer_samples > self.samples
        self.exp_rate, noise_next = c.exp_params(self.samples)                  # rl_agent.py:345-349: the next rollout's
        self._set_noise(noise_next)
        self.env.env.set_sample_count(self.samples)                             # the episode-length schedule of the scene (rl_agent.py:136)
        row = self._log_row(rate, noise, info, trained)
        self._mark("end")
        self.iteration += 1
        self.log.append(row)
        return row

    def update_losses(self) -> dict:
        """Critic_Loss, Actor_Loss and Clip_Frac of the last `update`, means over its minibatches: one host read"""
        b = self._sums.cpu().numpy()
        nb = max(b[0], 1.0)
        return {"Critic_Loss": float(b[1] / nb), "Actor_Loss": float(b[2] / nb), "Clip_Frac": float(b[3] / nb), "minibatches": int(b[0])}

    def train(self, iterations: int) -> list:
        return [self.iterate() for _ in range(int(iterations))]

    def _all_norms(self):
        return list(self._norms().values())

    # ---- the log
    def _log_block(self):
        """everything the log row reads from the device, as one float64 tensor: the sums over the minibatches, the advantage statistics, the episode totals
        (their int64 words bit-cast) and what `_extra_block` adds"""
        t = self.torch
        adv = self._adv_stats if self._adv_stats is not None else t.zeros(2, dtype=t.float64, device=self.device)
        parts = [self._sums, adv, self.stats.block.view(t.float64)] + self._extra_block()
        return t.cat(parts).cpu().numpy()

    def _extra_block(self) -> list:
        out = []
        for tr in self.trainers().values():
            if tr.opt_state is not None:
                out.append(tr.opt_state)
        return out

    def columns(self) -> tuple:
        measured = any(tr.opt_state is not None for tr in self.trainers().values())
        return LOG_COLUMNS + (OPT_LOG_COLUMNS if measured else ())

    def _log_row(self, rate, noise, info, trained) -> dict:
        from .episodes import TOTALS_WORDS, decode_block
        b = self._log_block()
        nb = max(b[0], 1.0)
        at = self._N_SUMS + 2
        totals = decode_block(b[at:at + TOTALS_WORDS + self.stats.bins].view(np.int64), self.stats.bin_steps)
        if totals["episodes"]:
            self.train_return = totals["mean_return"]               # rl_agent.py:460-461, over the episodes that finished in this rollout
        st = self._norm_stats
        row = {"Iteration": self.iteration, "Wall_Time": (self._wall0 + time.time() - self._t0) / 3600.0, "Samples": self.samples,
               "Train_Return": float(self.train_return), "Test_Return": float(self.test_return),
               "State_Mean": float(np.mean(st["s"]["mean"])), "State_Std": float(np.mean(st["s"]["std"])),
               "Goal_Mean": float(np.mean(st["g"]["mean"])) if "g" in st else 0.0, "Goal_Std": float(np.mean(st["g"]["std"])) if "g" in st else 0.0,
               "Exp_Rate": float(rate), "Exp_Noise": float(noise),
               "Critic_Loss": float(b[1] / nb), "Actor_Loss": float(b[2] / nb), "Clip_Frac": float(b[3] / nb), "Adv_Mean": float(b[self._N_SUMS]),
               "Adv_Std": float(b[self._N_SUMS + 1])}
        at = self._log_extra(row, b, at + TOTALS_WORDS + self.stats.bins, nb)
        words = []
        for tr in self.trainers().values():
            if tr.opt_state is not None:
                words.append(b[at:at + len(train.OPT_STATE)]); at += len(train.OPT_STATE)
        if words:
            row["Skipped_Steps"] = int(sum(w[train.OPT_STATE.index("skipped")] for w in words))
            row["Grad_Norm"] = float(words[0][train.OPT_STATE.index("norm")])           # the actor's last step
        return {k: row[k] for k in self.columns()}

    def _log_extra(self, row, b, at, nb) -> int:
        return at

    # ---- test episodes
    def test(self, episodes: int) -> float:
        """`episodes` finished episodes in test mode with the mode action (rl_agent.py:351-377); sets and returns Test_Return, then train mode and fresh envs"""
        t = self.torch
        episodes = int(episodes)
        if episodes < 1:
            raise ValueError("episodes must be >= 1")
        env, G = self.env, self.G
        st = EpisodeStats(self.N, self.device)
        env.env.set_mode(True); env.env.set_sample_count(self.samples, test_mode=True)
        self._begin(env.reset())
        actions = t.zeros((self.N, self.A), dtype=t.float32, device=self.device)
        stream = stream_handle(self.device)
        steps, done_eps, totals = 0, 0, None
        limit = 40 * 30 * max(1, -(-episodes // self.N)) + 64       # no episode of the reference's scenes outlasts 40 s of 30 Hz steps
        while done_eps < episodes and steps < limit:
            for _ in range(8):                                      # one host read per eight steps
                self.actor.forward_device_ex(env.obs.data_ptr(), self.N, actions.data_ptr(), self._cur_goal().data_ptr() if G else 0, G, sample=False, stream=stream)
                _, reward, done, info = env.step(actions)
                if self.goal_fn is not None:
                    self._after_step(info)
                st.update(reward, info["terminate"], done, info["valid"], per_step=False)
                steps += 1
            totals = st.totals()
            done_eps = totals["episodes"]
        if done_eps:
            self.test_return = float(totals["mean_return"])
        env.env.set_mode(False); env.env.set_sample_count(self.samples)
        self.restart_envs(self.iteration)
        return self.test_return

    # ---- saving
    def _host(self, x):
        return x.detach().cpu().numpy()

    def _net_tensors(self, name: str, views: dict, scope: str) -> dict:
        base = "%s/main/%s/" % (scope, name)
        out = {base + var: self._host(views[k]) for k, var in _NET_VARIABLES.items()}
        out[base + _OUT_LAYER[name] + "/kernel"] = self._host(views["w3"]); out[base + _OUT_LAYER[name] + "/bias"] = self._host(views["b3"])
        if "gc_w" in views:
            for key, var in tf_checkpoint.GATE_VARIABLES.items():
                out[base + var + "/kernel"] = self._host(views[key + "_w"]); out[base + var + "/bias"] = self._host(views[key + "_b"])
        return out

    def _norm_tensors(self, scope: str) -> dict:
        """{resource name: (mean, std, count)}"""
        st = {k: n.state_host() for k, n in self._norms().items()}
        lo, hi = self.val_min, self.val_max
        val_offset, val_scale = (-0.5 * (hi + lo), 2.0 / (hi - lo)) if (np.isfinite(lo) and np.isfinite(hi)) else (0.0, 1.0)       # rl_agent.py:394-403
        out = {"s_norm": (st["s"]["mean"], st["s"]["std"], st["s"]["count"]),
               "g_norm": (st["g"]["mean"], st["g"]["std"], st["g"]["count"]) if "g" in st else (np.zeros(0), np.zeros(0), 0),
               "a_norm": (self.a_mean, self.a_std, 0), "val_norm": (np.array([-val_offset]), np.array([1.0 / val_scale]), 0)}
        return out

    def _reward_scale(self):
        return None

    def checkpoint_tensors(self, scope: str = "agent") -> dict:
        """{variable name: array} of `save_model`: the fp32 masters, the normalisers and reward_scale under the names, shapes and dtypes of `tf_checkpoint.agent_variables`"""
        spec = tf_checkpoint.agent_variables(self.S, self.G, self.A, self.AMP, gated=self.gated_actor, reward_scale=self._reward_scale() is not None, scope=scope)
        out = {}
        for name, tr in self.trainers().items():
            out.update(self._net_tensors(name, tr.views(), scope))
        out[scope + "/main/actor/dist_gauss_diag/logstd/bias"] = self.logstd
        for n in spec:
            if "/logstd/bias_" in n:
                out[n] = np.full(spec[n][1], self.logstd[0], np.float32)        # the shipped files' leftover variables (tf_checkpoint.agent_variables)
        for res, (mean, std, count) in self._norm_tensors(scope).items():
            for suffix in ("", "_ph"):
                out["%s/resource/%s/mean%s" % (scope, res, suffix)] = np.asarray(mean, np.float64).astype(np.float32)
                out["%s/resource/%s/std%s" % (scope, res, suffix)] = np.asarray(std, np.float64).astype(np.float32)
                out["%s/resource/%s/count%s" % (scope, res, suffix)] = np.array([min(int(count), 2 ** 31 - 1)], np.int32)
        if self._reward_scale() is not None:
            out[scope + "/reward_scale"] = np.array([self._reward_scale()], np.float32)
        return out

    def save_model(self, prefix: str):
        """the nets and normalisers as a tf.train.Saver V2 checkpoint with the variable set of the shipped checkpoints of this agent kind"""
        tf_checkpoint.write_checkpoint(prefix, self.checkpoint_tensors())

    def _state_arrays(self) -> dict:
        out = dict(iteration=np.int64(self.iteration), samples=np.int64(self.samples), seed=np.int64(self.seed), empty_rollouts=np.int64(self.empty_rollouts),
                   initialized=np.int64(self.initialized), recording=np.int64(self.recording), exp=np.array([self.exp_rate, self.exp_noise]),
                   returns=np.array([self.train_return, self.test_return]), wall=np.float64(self._wall0 + time.time() - self._t0), logstd=self.logstd,
                   kind=np.array(self.KIND), shape=np.array([self.T, self.N, self.S, self.G, self.A, self.AMP, self.M], np.int64))
        for name, tr in self.trainers().items():
            out["buf_" + name] = self._host(tr.buf)
            if tr.opt_state is not None:
                out["opt_" + name] = self._host(tr.opt_state)
        for k, n in self._state_norms().items():
            st = n.state_host()
            for f in ("mean", "std", "mean_sq"):
                out["norm_%s_%s" % (k, f)] = st[f]
            out["norm_%s_count" % k] = np.int64(st["count"])
        out["ep_acc_return"], out["ep_acc_len"] = self._host(self.stats.acc_return), self._host(self.stats.acc_len)
        return out

    def _state_norms(self) -> dict:
        return self._norms()

    def save_state(self, path: str):
        """the whole learner in one .npz (see `load_state`); env state is not part of it"""
        with open(path, "wb") as f:
            np.savez(f, **self._state_arrays())

    def _set_state(self, z):
        t = self.torch
        want = np.array([self.T, self.N, self.S, self.G, self.A, self.AMP, self.M], np.int64)
        if str(z["kind"]) != self.KIND or not np.array_equal(z["shape"], want):
            raise ValueError("the saved learner is %s of (T, N, S, G, A, AMP, M) = %s, this one %s of %s" % (z["kind"], tuple(z["shape"]), self.KIND, tuple(want)))
        self.iteration, self.samples, self.empty_rollouts = int(z["iteration"]), int(z["samples"]), int(z["empty_rollouts"])
        self.initialized, self.recording = bool(z["initialized"]), bool(z["recording"])
        self.exp_rate = float(z["exp"][0]); self._set_noise(float(z["exp"][1]))
        self.train_return, self.test_return = float(z["returns"][0]), float(z["returns"][1])
        self._wall0, self._t0 = float(z["wall"]), time.time()
        for name, tr in self.trainers().items():
            if tuple(z["buf_" + name].shape) != tuple(tr.buf.shape) or (("opt_" + name) in z) != (tr.opt_state is not None):
                raise ValueError("the saved %s trainer was built with another optimiser" % name)
            tr.buf.copy_(t.from_numpy(z["buf_" + name]))
            if tr.opt_state is not None:
                tr.opt_state.copy_(t.from_numpy(z["opt_" + name]))
            tr.sync()
        for k, n in self._state_norms().items():
            n.set_state(z["norm_%s_mean" % k], z["norm_%s_std" % k], z["norm_%s_mean_sq" % k], int(z["norm_%s_count" % k]))
        self._refresh_nets()
        self.env.env.set_sample_count(self.samples)
        self.stats.acc_return.copy_(t.from_numpy(z["ep_acc_return"])); self.stats.acc_len.copy_(t.from_numpy(z["ep_acc_len"]))

    @classmethod
    def load_state(cls, env, cfg: AgentConfig, path: str, **kw):
        """the learner `save_state` wrote, on `env` (a fresh one of the same scene and size): trainers, normalisers, stores and counters as saved, the envs
        restarted under `restart_envs(iteration)`.  **kw: the constructor's optimizer / optimiser options, which must be the saved agent's."""
        with np.load(path, allow_pickle=False) as z:
            z = {k: z[k] for k in z.files}
        T, M = int(z["shape"][0]), int(z["shape"][6])
        agent = cls(env, cfg, rollout_steps=T, seed=int(z["seed"]), mini_batch_size=M, **kw)
        agent._set_state(z)
        agent.restart_envs(agent.iteration)
        return agent


class AMPAgent(PPOAgent):
    KIND = "AMP"
    _N_SUMS = PPOAgent._N_SUMS + 1 + len(train.DISC_STATS) + 1        # + discriminator steps, its eight statistics, Disc_Loss

    def __init__(self, env, cfg, *a, **kw):
        if getattr(env, "amp_obs", None) is None:
            raise ValueError("an AMP agent needs the AMP observations: TorchVecEnv(..., amp_obs=True) on an imitate_amp scene")
        self.disc_steps_done = 0
        super().__init__(env, cfg, *a, **kw)

    def _setup_scene(self):
        super()._setup_scene()
        self.AMP = self.env.env.amp_size
        # cSceneImitateAMP::GetAMPObsOffset / Scale / NormGroup: offset 0, scale 1, every column a group of its own
        self.amp_norm = DeviceNormalizer(self.AMP, device_id=self.device.index or 0)
        self.amp_norm.set_mean_std(np.zeros(self.AMP), np.ones(self.AMP))

    def _random_nets(self):
        w = super()._random_nets()
        w["disc"] = random_weights(self.AMP, 1, seed=(_mix(self.seed, _TAG_INIT) >> 24) & 0x7FFFFFFF, init_output_scale=self.cfg.disc_init_output_scale)
        return w

    def _checkpoint_nets(self, prefix):
        w = super()._checkpoint_nets(prefix)
        w["disc"] = tf_checkpoint.disc_weights(prefix)
        return w

    def _load_extra_norms(self, w):
        if "s_mean" in w["disc"]:
            self.amp_norm.set_mean_std(w["disc"]["s_mean"], w["disc"]["s_std"])

    def _build_extra_nets(self, w):
        c = self.cfg
        dw = {k: v for k, v in w["disc"].items() if k in train.KEYS}
        self.disc = Discriminator(dw, reward_scale=c.reward_scale, task_reward_lerp=c.task_reward_lerp if self.G else None, device_id=self.device.index or 0)
        self.disc_tr = train.DiscTrainer.from_policy(self.disc.net, dw, stepsize=c.disc_stepsize, momentum=c.disc_momentum, weight_decay=c.disc_weight_decay, **self._opt)

    def _build_rest(self):
        super()._build_rest()
        c, t = self.cfg, self.torch
        k = self.keys(0)
        # the task reward is blended in where the scene has a goal (cSceneTargetAMP::EnableAMPTaskReward), amp_agent.py:405-409
        self.amp = amp_rewards.AmpRewards(self.device, reward_scale=c.reward_scale, task_reward_lerp=c.task_reward_lerp if self.G else None, discount=c.discount)
        self.agent_store = replay.DeviceReplayStore(c.disc_agent_buffer_size, self.AMP, device=self.device, seed=k["agent_store_seed"])
        self.expert_store = replay.DeviceReplayStore(c.disc_expert_buffer_size, self.AMP, device=self.device, seed=k["expert_store_seed"])
        self._amp_packed = t.zeros((self.T * self.N, self.AMP), dtype=t.float32, device=self.device)
        self._expert = t.zeros((self.T * self.N, self.AMP), dtype=t.float32, device=self.device)

    def trainers(self):
        return dict(actor=self.actor_tr, critic=self.critic_tr, disc=self.disc_tr)

    def _all_norms(self):
        return super()._all_norms() + [self.amp_norm]

    def _state_norms(self):
        return dict(super()._state_norms(), amp=self.amp_norm)

    def _refresh_nets(self):
        super()._refresh_nets()
        st = self.amp_norm.state_host()
        self._norm_stats["amp"] = st
        self.disc.net.set_weights(dict(s_mean=st["mean"].astype(np.float32), s_std=st["std"].astype(np.float32)))

    def disc_steps_max(self) -> int:
        return -(-self.cfg.disc_steps_per_batch * self.T * self.N // self.cfg.disc_batch_size)

    def _rewards(self, ro, k, train_nets):
        c = self.cfg
        self.amp_norm.set_stream(stream_handle(self.device))
        lists = self._lists = self._valid_lists(ro)
        n_valid, _ = lists.counts_host()                             # the first count read of the iteration
        if not n_valid:
            return None
        # the discriminator's data (amp_agent.py:216-249, 287-292): the valid steps' observations into the agent store, as many expert rows into the expert store
        self.agent_store.append_calls = k["append_call"]; self.expert_store.append_calls = k["append_call"]
        self.agent_store.append_batch(ro.amp_obs, lists, packed=self._amp_packed)
        self.env.expert_draw_calls = k["expert_draw_call"]
        expert = self.env.amp_expert_draw(n_valid, out=self._expert[:n_valid])
        self.expert_store.append(expert)
        if self.recording:
            self.amp_norm.record_device(self._amp_packed.data_ptr(), n_valid); self.amp_norm.record_device(expert.data_ptr(), n_valid)
        if not train_nets:
            return ro.reward, None
        steps = -(-c.disc_steps_per_batch * n_valid // c.disc_batch_size)          # amp_agent.py:323-354
        sums, base = self._sums, PPOAgent._N_SUMS
        for b in range(steps):
            self.agent_store.sample_calls = self.expert_store.sample_calls = k["sample_call0"] + b
            agent_rows, expert_rows = self.agent_store.sample(c.disc_batch_size), self.expert_store.sample(c.disc_batch_size)
            self.disc_tr.grad(expert_rows, agent_rows, grad_penalty=c.disc_grad_penalty, logit_reg=c.disc_logit_reg_weight)
            self.disc_tr.step()
            sums[base] += 1.0; sums[base + 1:base + 1 + len(train.DISC_STATS)] += self.disc_tr.stats(); sums[base + 1 + len(train.DISC_STATS)] += self.disc_tr.loss()
        self.disc_steps_done += steps
        # the batch rewards (amp_agent.py:393-425): the whole rollout scored by the discriminator as it is now
        rewards, _ = self.amp.update_from_disc(self.disc, ro.amp_obs, ro.reward if self.G else None, ro.done, ro.valid)
        return rewards, self.amp

    def columns(self):
        base = super().columns()
        n = len(LOG_COLUMNS)
        return base[:n] + AMP_LOG_COLUMNS + base[n:]

    def _extra_block(self):
        return [self.amp.stats, self.amp.bounds.to(self.torch.float64)] + super()._extra_block()

    def _log_extra(self, row, b, at, nb):
        base = PPOAgent._N_SUMS
        nd = max(b[base], 1.0)
        d = dict(zip(train.DISC_STATS, b[base + 1:base + 1 + len(train.DISC_STATS)] / nd))
        row.update({"Disc_Loss": float(b[base + 1 + len(train.DISC_STATS)] / nd), "Disc_Acc_Expert": float(d["acc_expert"]), "Disc_Acc_Agent": float(d["acc_agent"]),
                    "Disc_Prob": float(d["prob_agent"]), "Disc_Abs_Logit": float(d["abs_logit_agent"]), "Disc_Reward_Mean": float(b[at + amp_rewards.STAT_MEAN]),
                    "Disc_Reward_Std": float(b[at + amp_rewards.STAT_STD]), "Grad_Penalty": float(d["grad_penalty"]), "Disc_Steps": int(self.disc_steps_done)})
        return at + amp_rewards.STATS_WORDS + 2

    def _norm_tensors(self, scope):
        out = super()._norm_tensors(scope)
        st = self.amp_norm.state_host()
        out["amp_obs_norm"] = (st["mean"], st["std"], st["count"])
        return out

    def _reward_scale(self):
        return self.cfg.reward_scale

    def _state_arrays(self):
        out = super()._state_arrays()
        out["amp_bounds"] = self._host(self.amp.bounds); out["disc_steps_done"] = np.int64(self.disc_steps_done)
        for name, st in (("agent", self.agent_store), ("expert", self.expert_store)):
            out["store_%s_buf" % name], out["store_%s_state" % name] = self._host(st.buf), self._host(st.state)
            out["store_%s_calls" % name] = np.array([st.append_calls, st.sample_calls], np.int64)
        out["expert_draw_calls"] = np.int64(self.env.expert_draw_calls)
        return out

    def _set_state(self, z):
        t = self.torch
        super()._set_state(z)
        self.amp.bounds.copy_(t.from_numpy(z["amp_bounds"])); self.disc_steps_done = int(z["disc_steps_done"])
        for name, st in (("agent", self.agent_store), ("expert", self.expert_store)):
            if tuple(z["store_%s_buf" % name].shape) != tuple(st.buf.shape):
                raise ValueError("the saved %s store holds %d rows, the agent file names %d" % (name, z["store_%s_buf" % name].shape[0], st.capacity))
            st.buf.copy_(t.from_numpy(z["store_%s_buf" % name])); st.state.copy_(t.from_numpy(z["store_%s_state" % name]))
            st.append_calls, st.sample_calls = (int(x) for x in z["store_%s_calls" % name])
        self.env.expert_draw_calls = int(z["expert_draw_calls"])


def make_agent(env, cfg: AgentConfig, **kw) -> PPOAgent:
    """the agent class the file's AgentType names"""
    return {"PPO": PPOAgent, "AMP": AMPAgent}[cfg.agent_type](env, cfg, **kw)


# ---- the log file (util/logger.py: Logger.dump_tabular left-aligns every cell in 25 characters, the header row first; numpy.genfromtxt(names=True) reads it)

def format_log_header(columns) -> str:
    return ("{:<25}" * len(columns)).format(*columns)


def format_log_row(columns, row: dict) -> str:
    return ("{:<25}" * len(columns)).format(*(str(row[k]) for k in columns))


def format_log_table(columns, row: dict) -> str:
    """Logger.print_tabular"""
    lines = ["-" * 39]
    for k in columns:
        v = row[k]
        lines.append("| %16s | %16s |" % (k, "%8.3g" % v if isinstance(v, float) else str(v)))
    return "\n".join(lines + ["-" * 39])


class LogFile:
    """`agent0_log.txt` as the reference's Logger.dump_tabular writes it: the header once, one row per call, flushed"""

    def __init__(self, path: str, columns):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.columns = tuple(columns)
        self.f = open(path, "w")
        self.f.write(format_log_header(self.columns) + "\n"); self.f.flush()

    def write(self, row: dict):
        self.f.write(format_log_row(self.columns, row) + "\n"); self.f.flush()

    def close(self):
        self.f.close()


# ---- the command line (DeepMimic_Optimizer.py / learning/rl_world.py:60-85)

def main(argv=None) -> int:
    import argparse
    from . import model
    from .vec_env import TorchVecEnv
    ap = argparse.ArgumentParser(prog="python -m deepmimic_amd.agent", description="train the agent an arg file names on one GPU")
    ap.add_argument("--arg_file", required=True); ap.add_argument("--data_root", default=".")
    ap.add_argument("--asset", default=None, help="a packaged scene (deepmimic_amd/assets/<name>.json) in place of the arg file's character / motion files")
    ap.add_argument("--num_envs", type=int, default=4096); ap.add_argument("--rollout_steps", type=int, default=32)
    ap.add_argument("--iterations", type=int, required=True); ap.add_argument("--mini_batch_size", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0); ap.add_argument("--optimizer", default="momentum"); ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    root = a.data_root
    rs = lambda p: p if os.path.isabs(p) else os.path.join(root, p)
    parser = model.ArgParser([])
    if not parser.load_file(rs(a.arg_file)):
        raise FileNotFoundError("Failed to load args from: %s" % a.arg_file)
    strings = lambda key: [s for s in (parser.get(key) or []) if s]
    agent_files, model_files = strings("agent_files"), strings("model_files")
    if len(agent_files) != 1:
        raise ValueError("--agent_files must name one agent file, got %d" % len(agent_files))
    out_dir, int_dir = parser.str("output_path", ""), parser.str("int_output_path", "")
    cfg = AgentConfig.from_file(rs(agent_files[0]))
    tables = model.load_asset(a.asset) if a.asset else model.load_scene_from_args(["--arg_file", a.arg_file], data_root=root)
    env = TorchVecEnv(tables, a.num_envs, device=a.device, seed=a.seed, amp_obs=cfg.agent_type == "AMP")
    agent = make_agent(env, cfg, rollout_steps=a.rollout_steps, seed=a.seed, mini_batch_size=a.mini_batch_size, optimizer=a.optimizer,
                       init_from=rs(model_files[0]) if model_files else None)
    print("%s agent: %d envs x %d steps = %d samples per update (BatchSize %d in the agent file), minibatches of %d" %
          (cfg.agent_type, agent.N, agent.T, agent.T * agent.N, cfg.batch_size, agent.M))
    if cfg.ignored:
        print("ignored keys: " + ", ".join(cfg.ignored))
    columns = agent.columns()
    log = LogFile(os.path.join(rs(out_dir), "agent0_log.txt"), columns) if out_dir else None
    for _ in range(a.iterations):
        it = agent.iteration
        if out_dir and it % cfg.output_iters == 0:                  # rl_agent.py:425-441
            agent.save_model(os.path.join(rs(out_dir), "agent0_model.ckpt"))
        if int_dir and it % cfg.int_output_iters == 0:
            agent.save_model(os.path.join(rs(int_dir), "agent0_models", "agent0_int_model_%010d.ckpt" % it))
        if cfg.test_episodes > 0 and it > 0 and it % cfg.int_output_iters == 0:           # rl_agent.py:528-529, 544-545: Test_Return of the rows that follow
            agent.test(cfg.test_episodes)
        row = agent.iterate()
        if it % cfg.output_iters == 0:
            print("Agent 0\n" + format_log_table(columns, row) + "\n", flush=True)
        if log is not None:
            log.write(row)
    if out_dir:
        agent.save_model(os.path.join(rs(out_dir), "agent0_model.ckpt"))
    if log is not None:
        log.close()
    env.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
