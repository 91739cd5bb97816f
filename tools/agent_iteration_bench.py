"""Where one learner iteration spends its time (deepmimic_amd/agent.py), on one GPU: PPO on humanoid3d_walk and AMP on amp_heading_zombie, 4096 envs, T = 32,
minibatches of 256 and of 4096.  Device events are recorded at the agent's phase marks -- collect | discriminator phase (the AMP data, its steps, the batch
rewards) | critic evaluations + TD(lambda) + advantages | minibatch loop | bookkeeping (normaliser update, the log row's reads) -- and around the whole iteration;
medians and quartiles over the timed iterations.  The host reads of an iteration lie inside the bracketed spans, so the spans are what the
iteration takes on the device's clock, idle gaps included.

Two bare loops give the kernels' own share, timed the same way in the same process: T x (actor forward + env step) with nothing else, and the trainers'
grad + step calls of one iteration on fixed minibatch tensors (critic and actor per minibatch, the discriminator per discriminator step).
`glue_share` = 1 - (bare step loop + bare trainer calls) / iteration: copies into the rollout, normalisers, stores and draws, the head evaluations, TD(lambda),
advantages, gathers, the statistics' torch arithmetic, launch gaps and host reads.

Writes one JSON object (default profiles/agent_iteration.json).
usage: python tools/agent_iteration_bench.py [--envs 4096] [--T 32] [--iters 20] [--warmup 3] [--out profiles/agent_iteration.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmimic_amd import agent, model  # noqa: E402
from deepmimic_amd.binding import stream_handle  # noqa: E402
from deepmimic_amd.vec_env import TorchVecEnv  # noqa: E402

PLAIN, GATED = agent.NETS
EXP = {"ExpParamsBeg": {"Rate": 1, "Noise": 0.05}, "ExpParamsEnd": {"Rate": 0.2, "Noise": 0.05}}
# data/agents/ct_agent_humanoid_ppo.txt and ct_agent_humanoid_amp_tasks.txt of the reference (the values, not the files: the tool runs without the checkout)
PPO = dict({"AgentType": "PPO", "ActorNet": PLAIN, "ActorStepsize": 2e-6, "ActorMomentum": 0.9, "ActorWeightDecay": 0.0005, "ActorInitOutputScale": 0.01,
            "CriticNet": PLAIN, "CriticStepsize": 0.0005, "CriticMomentum": 0.9, "CriticWeightDecay": 0, "Discount": 0.95, "BatchSize": 4096, "MiniBatchSize": 256,
            "Epochs": 1, "InitSamples": 1, "NormalizerSamples": 1000000, "RatioClip": 0.2, "NormAdvClip": 4, "TDLambda": 0.95, "OutputIters": 10,
            "ExpAnnealSamples": 64000000}, **EXP)
AMP = dict({"AgentType": "AMP", "ActorNet": GATED, "ActorStepsize": 4e-6, "ActorMomentum": 0.9, "ActorWeightDecay": 0.0005, "ActorInitOutputScale": 0.01,
            "CriticNet": GATED, "CriticStepsize": 2e-5, "CriticMomentum": 0.9, "CriticWeightDecay": 0, "Discount": 0.99, "BatchSize": 4096, "MiniBatchSize": 256,
            "Epochs": 1, "InitSamples": 1, "NormalizerSamples": 1000000, "RatioClip": 0.2, "NormAdvClip": 4, "TDLambda": 0.95, "TaskRewardLerp": 0.5,
            "DiscNet": PLAIN, "DiscInitOutputScale": 1, "DiscStepSize": 1e-5, "DiscMomentum": 0.9, "DiscWeightDecay": 0.0005, "DiscLogitRegWeight": 0.05,
            "DiscGradPenalty": 10, "DiscBatchSize": 256, "DiscStepsPerBatch": 2, "DiscExpertBufferSize": 100000, "DiscAgentBufferSize": 100000, "RewardScale": 2,
            "OutputIters": 10, "ExpAnnealSamples": 200000000}, **EXP)
CASES = {"ppo_walk": ("humanoid3d_walk", PPO), "amp_heading": ("amp_heading_zombie", AMP)}
PHASES = ("collect", "disc", "values", "minibatches", "bookkeeping")


def quartiles(x):
    return [float(np.percentile(x, p)) for p in (25, 50, 75)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)            # ms


def bare_step_loop(a):
    """T x (actor forward, env step) on the agent's env: no copy into a rollout, no normaliser"""
    env, G = a.env, a.G
    act = torch.zeros((a.N, a.A), dtype=torch.float32, device=a.device)
    stream = stream_handle(a.device)
    def run():
        for t in range(a.T):
            a.actor.forward_device_ex(env.obs.data_ptr(), a.N, act.data_ptr(), env.goal.data_ptr() if G else 0, G, exp_rate=a.exp_rate, sample=True, seed=11, step=t,
                                      stream=stream)
            a.env.env.step_device(act.data_ptr(), env.obs.data_ptr(), env.reward.data_ptr(), env.terminate.data_ptr(), env.valid.data_ptr(), env.episode_end.data_ptr(),
                                  timestep=env.timestep, n_updates=env.updates, auto_reset=True, amp_ptr=env.amp_obs.data_ptr() if env.amp_obs is not None else 0)
    return run


def bare_trainer_calls(a, info):
    """the grad + step calls of one iteration on fixed tensors, stepsize 0 so that the nets stay where they are: critic and actor per minibatch, the discriminator
    per discriminator step"""
    ro, G, M, c = a.rollout, a.G, a.M, a.cfg
    flat = lambda x: x[:a.T].reshape((a.T * a.N,) + tuple(x.shape[2:]))[:M].contiguous()
    obs, goal = flat(ro.obs), (flat(ro.goal) if G else None)
    act, logp = flat(ro.act), flat(ro.logp)
    targets, adv = torch.zeros(M, dtype=torch.float32, device=a.device), torch.ones(M, dtype=torch.float32, device=a.device)
    steps = 0
    if a.KIND == "AMP":
        steps = -(-c.disc_steps_per_batch * info["n_valid"] // c.disc_batch_size)
        rows_a, rows_e = a.agent_store.buf[:c.disc_batch_size].contiguous(), a.expert_store.buf[:c.disc_batch_size].contiguous()
    def run():
        keep = {n: tr.stepsize for n, tr in a.trainers().items()}
        for tr in a.trainers().values():
            tr.stepsize = 0.0
        for _ in range(steps):
            a.disc_tr.grad(rows_e, rows_a, grad_penalty=c.disc_grad_penalty, logit_reg=c.disc_logit_reg_weight); a.disc_tr.step()
        for _ in range(info["minibatches"]):
            a.critic_tr.grad(obs, targets, goals=goal); a.critic_tr.step()
            a.actor_tr.grad(obs, act, logp, adv, goals=goal, ratio_clip=c.ratio_clip, a_bound_min=a.a_bound_min, a_bound_max=a.a_bound_max); a.actor_tr.step()
        for n, tr in a.trainers().items():
            tr.stepsize = keep[n]
    return run


def run_case(name, M, envs, T, iters, warmup):
    asset, d = CASES[name]
    cfg = agent.AgentConfig.from_dict(d)
    env = TorchVecEnv(model.load_asset(asset), envs, seed=1, amp_obs=cfg.agent_type == "AMP")
    a = agent.make_agent(env, cfg, rollout_steps=T, seed=1, mini_batch_size=M)
    a.iterate()                                       # the InitSamples rollout: not an update
    marks = []
    a.phase_mark = lambda label: (marks.append((label, torch.cuda.Event(enable_timing=True))), marks[-1][1].record())
    spans, totals, walls = {p: [] for p in PHASES}, [], []
    for i in range(warmup + iters):
        marks.clear()
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        row = a.iterate()
        torch.cuda.synchronize()
        w1 = time.perf_counter()
        if i < warmup:
            continue
        labels = [m[0] for m in marks]
        assert labels == list(PHASES) + ["end"], labels
        for (label, e0), (_, e1) in zip(marks[:-1], marks[1:]):
            spans[label].append(e0.elapsed_time(e1))
        totals.append(marks[0][1].elapsed_time(marks[-1][1])); walls.append((w1 - w0) * 1e3)
    a.phase_mark = None
    info = dict(n_valid=a.last_batch.counts_host()[0], minibatches=cfg.epochs * -(-a.last_batch.counts_host()[0] // M))
    step_loop, trainer = bare_step_loop(a), bare_trainer_calls(a, info)
    bare = {"step_loop_ms": [], "trainer_calls_ms": []}
    for i in range(3 + 7):
        s, t = timed(step_loop), timed(trainer)
        if i >= 3:
            bare["step_loop_ms"].append(s); bare["trainer_calls_ms"].append(t)
    med = lambda x: float(np.median(x))
    total = med(totals)
    out = dict(case=name, agent=cfg.agent_type, asset=asset, envs=envs, T=T, M=M, samples_per_iteration=envs * T, minibatches_per_iteration=info["minibatches"],
               disc_steps_per_iteration=(-(-cfg.disc_steps_per_batch * info["n_valid"] // cfg.disc_batch_size) if cfg.agent_type == "AMP" else 0),
               iterations=iters, warmup=warmup, iteration_ms=quartiles(totals), iteration_wall_ms=quartiles(walls),
               phases_ms={p: quartiles(v) for p, v in spans.items()}, phase_share={p: med(v) / total for p, v in spans.items()},
               bare_step_loop_ms=quartiles(bare["step_loop_ms"]), bare_trainer_calls_ms=quartiles(bare["trainer_calls_ms"]),
               glue_share=1.0 - (med(bare["step_loop_ms"]) + med(bare["trainer_calls_ms"])) / total,
               samples_per_second=envs * T / (med(walls) * 1e-3), last_row={k: row[k] for k in ("Iteration", "Samples", "Train_Return", "Critic_Loss", "Actor_Loss")})
    env.close()
    return out


def write(res: dict, path: str):
    """one result per line, figures to six significant digits"""
    rnd = lambda o: float("%.6g" % o) if isinstance(o, float) else [rnd(x) for x in o] if isinstance(o, list) else {k: rnd(v) for k, v in o.items()} if isinstance(o, dict) else o
    head = {k: v for k, v in res.items() if k != "results"}
    with open(path, "w") as f:
        f.write(json.dumps(head)[:-1] + ', "results": [\n' + ",\n".join(" " + json.dumps(rnd(x)) for x in res["results"]) + "\n]}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096); ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="ppo_walk,amp_heading"); ap.add_argument("--minibatch", default="256,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agent_iteration.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("agent_iteration_bench needs the GPU: no HIP device is visible")
    res = dict(tool="tools/agent_iteration_bench.py", device=torch.cuda.get_device_name(0), unit="ms; [q25, median, q75]", results=[])
    for name in a.cases.split(","):
        for M in (int(x) for x in a.minibatch.split(",")):
            r = run_case(name, M, a.envs, a.T, a.iters, a.warmup)
            res["results"].append(r)
            print("%-12s M=%-5d iteration %8.1f ms  (%s)  bare steps %7.1f  bare trainers %7.1f  glue %.1f %%" %
                  (name, M, r["iteration_ms"][1], "  ".join("%s %.1f" % (p, r["phases_ms"][p][1]) for p in PHASES), r["bare_step_loop_ms"][1],
                   r["bare_trainer_calls_ms"][1], 100 * r["glue_share"]), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            write(res, a.out)


if __name__ == "__main__":
    main()
