"""Two ranks on the CPU (gloo, the emulator build as the device; the launch pattern of tests/test_train_dist.py): each rank holds its own gradient block,
dist.all_reduce_gradients sums them, then every rank takes the clipped Adam step with grad_scale = 1 / 2.  The norm is taken after the reduction, so both ranks clip
alike: they must end with identical masters, moments and state, and -- gloo's sum of two float32 arrays is one rounded addition per element, the same on both ranks
and in numpy -- those are, byte for byte, the arrays of a single process fed the summed gradients."""
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
from deepmimic_amd.dist import all_reduce_gradients
from test_train_optim_dist import make_trainer, rank_grads
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
trn = make_trainer(os.environ["DM_HIP_LIB"])
for it in range(2):
    trn.grads.copy_(torch.from_numpy(rank_grads(trn.P, it)[rank]))
    all_reduce_gradients(trn)
    trn.step(grad_scale=1.0 / world)
np.save(os.environ["DM_OUT"] + ".r%d.npy" % rank, trn.buf.numpy())
np.save(os.environ["DM_OUT"] + ".s%d.npy" % rank, trn.opt_state.numpy())
dist.barrier()
dist.destroy_process_group()
'''


def make_trainer(lib):
    from deepmimic_amd import train as tr
    from deepmimic_amd.policy import Policy
    from test_train import NET_A, net_weights
    w = net_weights(NET_A, seed=21)
    return tr.ActorTrainer.from_policy(Policy(w, lib_path=lib), w, stepsize=1e-3, weight_decay=1e-4, device="cpu", optimizer="adam", max_grad_norm=1.0, skip_nonfinite=True)


def rank_grads(P, it):
    rng = np.random.default_rng([31, it])
    return rng.standard_normal((2, P)).astype(np.float32)


def test_two_ranks_clip_alike_and_match_the_single_process(emu_lib, tmp_path):
    import torch
    out = str(tmp_path / "optim")
    script = tmp_path / "optim_worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, DM_ROOT=ROOT, DM_HIP_LIB=emu_lib, DM_OUT=out, MASTER_ADDR="127.0.0.1", DM_ALLOW_EMULATOR="1")
    port = 37500 + (os.getpid() % 2000)
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)], env=env, timeout=600)
    a, b = np.load(out + ".r0.npy"), np.load(out + ".r1.npy")
    sa, sb = np.load(out + ".s0.npy"), np.load(out + ".s1.npy")
    assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes()                # masters, both moments, the reduced gradients and the state on both ranks
    trn = make_trainer(emu_lib)
    start = trn.params.numpy().copy()
    for it in range(2):
        g = rank_grads(trn.P, it)
        trn.grads.copy_(torch.from_numpy(g[0] + g[1]))
        trn.step(grad_scale=0.5)
    assert trn.buf.numpy().tobytes() == a.tobytes() and trn.opt_state.numpy().tobytes() == sa.tobytes()
    assert sa[0] == 2 and sa[3] == 0 and sa[5] < 1.0 and not np.array_equal(a[0], start)          # two steps taken, none skipped, the clip was active
