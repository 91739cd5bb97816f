"""Two ranks on the CPU (gloo, the emulator build as the device; the launch pattern of tests/test_dist_gloo.py): each rank takes half of a 64-row minibatch through
ActorTrainer.grad, then dist.all_reduce_gradients and step(grad_scale=0.5) -- MPISolver.update_flatgrad.  Both ranks must hold identical masters, and those must be
the masters of a single process on all 64 rows up to fp32 summation order:

  g_i = -(adv ratio) / n and the bound term's weight / n are formed with n = 32 on a rank and n = 64 in the single process, a factor of exactly 2 that the bf16
  roundings of dz3, dz2, dz1 carry unchanged (a power of two).  So 0.5 (grad_rank0 + grad_rank1) and the single-process gradient are the same sums of the same bf16
  products, accumulated in fp32 in another order: 32 + 32 rows and one more addition against 64 rows in a chain.  Per entry |difference| <= 2 gamma_65 sum|a||b|
  (gamma_k = k u / (1 - k u), u = 2^-24, each side within gamma of the exact sum), computed below from the single process's own bf16 operands; through
  v = g and w -= stepsize v that is stepsize times as much, plus one ulp of w for the final rounding."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["DM_ROOT"]); sys.path.insert(0, os.path.join(os.environ["DM_ROOT"], "tests"))
import torch, torch.distributed as dist
from deepmimic_amd import train as tr
from deepmimic_amd.dist import all_reduce_gradients
from deepmimic_amd.policy import Policy
from test_train_dist import make_case
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
w, states, kw = make_case()
half = slice(32 * rank, 32 * rank + 32)
pol = Policy(w, lib_path=os.environ["DM_HIP_LIB"])
trn = tr.ActorTrainer.from_policy(pol, w, stepsize=0.05, momentum=0.9, device="cpu")
t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
trn.grad(t(states[half]), t(kw["actions"][half]), t(kw["old_logp"][half]), t(kw["adv"][half]), ratio_clip=kw["ratio_clip"], bound_weight=kw["bound_weight"],
         a_bound_min=kw["a_bound_min"], a_bound_max=kw["a_bound_max"])
all_reduce_gradients(trn)
trn.step(grad_scale=1.0 / world)
np.save(os.environ["DM_OUT"] + ".r%d.npy" % rank, trn.buf.numpy())
dist.barrier()
dist.destroy_process_group()
'''


def make_case():
    from test_train import NET_A, random_case
    w, states, A, kw = random_case(NET_A, 64, "actor", seed=21)
    return w, states, kw


def test_two_ranks_hold_the_single_process_masters(emu_lib, tmp_path):
    import torch
    from deepmimic_amd import train as tr
    from deepmimic_amd.policy import Policy
    from test_train import NET_A, U, gamma
    out = str(tmp_path / "train")
    script = tmp_path / "train_worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, DM_ROOT=ROOT, DM_HIP_LIB=emu_lib, DM_OUT=out, MASTER_ADDR="127.0.0.1", DM_ALLOW_EMULATOR="1")
    port = 35500 + (os.getpid() % 2000)
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)], env=env, timeout=600)
    a, b = np.load(out + ".r0.npy"), np.load(out + ".r1.npy")
    assert a.tobytes() == b.tobytes()                                 # masters, momentum and the reduced gradients, bit for bit on both ranks
    # the single process on all 64 rows
    w, states, kw = make_case()
    pol = Policy(w, lib_path=emu_lib)
    trn = tr.ActorTrainer.from_policy(pol, w, stepsize=0.05, momentum=0.9, device="cpu")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    trn.grad(t(states), t(kw["actions"]), t(kw["old_logp"]), t(kw["adv"]), ratio_clip=kw["ratio_clip"], bound_weight=kw["bound_weight"],
             a_bound_min=kw["a_bound_min"], a_bound_max=kw["a_bound_max"])
    n, (S, H1, H2, A) = 64, (NET_A["S"], NET_A["H1"], NET_A["H2"], NET_A["A"])
    lay = tr.workspace_layout(H1, H2, A, n)
    raw = trn._work.numpy().view(np.uint8)
    piece = lambda k: tr.bf16_value(raw[lay[k][0]:lay[k][0] + int(np.prod(lay[k][2])) * 2].view(np.uint16).reshape(lay[k][2])).astype(np.float64)
    acts = dict(w1=tr.bf16_value(tr.read_activations(pol, "s16", n))[:, :S], w2=tr.bf16_value(tr.read_activations(pol, "h1", n)), w3=tr.bf16_value(tr.read_activations(pol, "h2", n)))
    dz = dict(w1=piece("dz1"), w2=piece("dz2"), w3=piece("dz3")[:, :A])
    bound = {}
    for wk, bk in (("w1", "b1"), ("w2", "b2"), ("w3", "b3")):
        bound[wk] = 2 * gamma(65) * (np.abs(acts[wk].astype(np.float64)).T @ np.abs(dz[wk])); bound[bk] = 2 * gamma(65) * np.abs(dz[wk]).sum(axis=0)
    gbound = np.concatenate([bound[k].reshape(-1) for k in tr.KEYS])
    single_grads = trn.grads.numpy().copy()
    assert (np.abs(0.5 * a[2].astype(np.float64) - single_grads) <= gbound).all() and gbound.max() < 1e-4 * np.abs(single_grads).max()
    trn.step()
    single = trn.buf.numpy()
    assert (np.abs(a[1].astype(np.float64) - single[1]) <= gbound + 2 * U * np.abs(single[1])).all()                       # momentum = the scaled gradient (from zero)
    assert (np.abs(a[0].astype(np.float64) - single[0]) <= 0.05 * (gbound + 2 * U * np.abs(single[1])) + 2 * U * np.abs(single[0])).all()
    assert not np.array_equal(single[0], tr.pack_params(w))           # a step was taken
