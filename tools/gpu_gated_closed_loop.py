#!/usr/bin/env python
"""The closed loop of a task scene (actor -> control step, goal from the env) once with the plain actor and once with the gated actor its agent file names,
same process, same box: env steps per second of each.  Prints one JSON object; run on the GPU box.  SCENE (default amp_heading_zombie), ENVS (4096)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepmimic_amd import model                                # noqa: E402
from deepmimic_amd.policy import Policy, random_weights        # noqa: E402
from deepmimic_amd.vec_env import TorchVecEnv                  # noqa: E402

scene = os.environ.get("SCENE", "amp_heading_zombie"); n = int(os.environ.get("ENVS", "4096")); steps = 100
t = model.load_asset(scene)
out = {"scene": scene, "envs": n, "steps": steps}
for name in ("plain", "gated", "plain_again"):
    env = TorchVecEnv(t, n, seed=3)
    obs = env.reset()
    S, G, A = env.obs_dim, env.goal_dim, env.act_dim
    offs = env.env.offsets_scales()
    w = random_weights(S + G, A, seed=1, gated_goal_dim=G if name == "gated" else 0)
    w["s_mean"] = np.concatenate([-offs["state_offset"], np.zeros(G)]).astype(np.float32); w["s_std"] = np.concatenate([1.0 / offs["state_scale"], np.ones(G)]).astype(np.float32)
    w["a_mean"] = -offs["action_offset"].astype(np.float32); w["a_std"] = (1.0 / offs["action_scale"]).astype(np.float32)
    pol = Policy(w, s_clip=10.0)
    actions = torch.zeros((n, A), device=obs.device)
    goal = torch.from_numpy(env.env.query_goal()).to(obs.device).float().contiguous()
    for phase in range(2):                   # phase 0 warms up
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for k in range(steps if phase else 10):
            pol.forward_device_ex(obs.data_ptr(), n, actions.data_ptr(), goals_ptr=goal.data_ptr(), goal_dim=G, sample=True, seed=7, step=k)
            obs, reward, done, info = env.step(actions)
            goal = info["goal"]
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
    out[name] = {"env_steps_per_s": n * steps / dt, "ms_per_step": 1e3 * dt / steps, "path_gated": [pol.info()["path"], int(pol.info()["gated"])],
                 "finite": bool(torch.isfinite(obs).all().item())}
    pol.close(); env.close()
print(json.dumps(out))
