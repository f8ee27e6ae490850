"""Recurrent PPO's policy step on one GPU: the fused step (``fused_step=True``,
one agx_ppo_act_recurrent launch) against the torch modules (the switch off,
the default), in one process.

Two figures per shape, both host wall-clock with the device drained at the end
of a block, because both paths end in host reads: ``get_action`` (us per call,
blocks of CALLS calls) and one ``collect_rollouts_recurrent`` of T = 128 steps
on a SyntheticVecEnv (ms per rollout, the bootstrap value and GAE included).
After a warm-up, ROUNDS rounds alternate fused and torch.  Median and min-max
of the blocks.  Shapes: N in 64 / 128, obs 8, H in 64 / 128, L in 1 / 2,
default heads, Discrete(4) and Box(6).  ``--spaces`` times N = 64, H = 64, L = 1
over MultiDiscrete([3, 3]), MultiDiscrete([2] * 16), MultiBinary(4) and
MultiBinary(32), each beside the Discrete space of the same logit count.

  python tools/recurrent_step_time.py [--out FILE]    (default profiles/recurrent_step_time.json)
  python tools/recurrent_step_time.py --spaces [--out FILE]    (default profiles/recurrent_step_spaces.json)
  python tools/recurrent_step_time.py --shared [--out FILE]
      the same shapes and method for a shared-encoder agent (``share_encoders=True``): its fused step
      (agx_ppo_act_recurrent_shared) against its torch modules, and beside them, for information, the fused step
      of a separate-encoder agent of the same shape.  Added to --out under "cells_shared"; other keys are kept.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS, HS, LS, T = (64, 128), (64, 128), (1, 2), 128
CALLS = int(os.environ.get("CALLS", 50))
ROUNDS = int(os.environ.get("ROUNDS", 5))


def _stats(v, digits):
    return [round(sorted(v)[len(v) // 2], digits), round(min(v), digits), round(max(v), digits)]


SPACES = {"discrete6": dict(n_actions=6), "multidiscrete3x3": dict(nvec=[3, 3]), "discrete32": dict(n_actions=32),
          "multidiscrete2x16": dict(nvec=[2] * 16), "discrete4": dict(n_actions=4), "multibinary4": dict(n_binary=4),
          "multibinary32": dict(n_binary=32)}


def time_cell(N, H, L, env_kw, shared=False):
    import numpy as np
    import torch

    from agilerl_amd.algorithms.ppo import PPO
    from agilerl_amd.envs import SyntheticVecEnv
    from agilerl_amd.rollouts import collect_rollouts_recurrent

    def make(fused, share=shared):
        env = SyntheticVecEnv(N, obs_dim=8, p_done=1 / 50, seed=3, **env_kw)
        torch.manual_seed(N + H + L)
        agent = PPO(env.single_observation_space, env.single_action_space, recurrent=True, share_encoders=share,
                    num_envs=N, learn_step=T * N, fused_step=fused,
                    net_config={"encoder_config": {"hidden_state_size": H, "num_layers": L}})
        return agent, env

    variants = {"fused": make(True), "torch": make(False)}
    if shared:
        variants["separate_fused"] = make(True, False)
    obs = np.random.default_rng(0).standard_normal((N, 8)).astype(np.float32)

    def act(agent):
        hidden = agent.get_initial_hidden_state(N)
        for _ in range(CALLS):
            hidden = agent.get_action(obs, hidden_state=hidden)[4]

    for agent, env in variants.values():  # warm-up: allocator, kernels' first launches
        act(agent)
        collect_rollouts_recurrent(agent, env)
    assert variants["fused"][0]._act_counter > 0, "the fused step did not take this shape"
    step_us, roll_ms = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(ROUNDS):
        for name, (agent, env) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            act(agent)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            collect_rollouts_recurrent(agent, env)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            step_us[name].append(1e6 * (t1 - t0) / CALLS)
            roll_ms[name].append(1e3 * (t2 - t1))
    res = {"get_action_us": {k: _stats(v, 1) for k, v in step_us.items()},
           "rollout_T128_ms": {k: _stats(v, 2) for k, v in roll_ms.items()}}
    for key in res:  # true when the fused maximum lies below torch's minimum
        res[key]["fused_clear"] = res[key]["fused"][2] < res[key]["torch"][1]
    return res


if __name__ == "__main__":
    import torch

    assert torch.cuda.is_available(), "tools/recurrent_step_time.py measures on the GPU only"
    os.environ.pop("AGX_RECURRENT_STEP", None)
    spaces = "--spaces" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
        os.path.join(ROOT, "profiles", "recurrent_step_spaces.json" if spaces else "recurrent_step_time.json")
    shared = "--shared" in sys.argv
    result = {"calls_per_block": CALLS, "rounds": ROUNDS, "unit": "median, min, max (host wall-clock)",
              "fused": "fused_step=True", "torch": "the switch off (the parent commit's path)", "cells": {}}
    cells = [(f"{name}_N64_H64_L1", 64, 64, 1, kw) for name, kw in SPACES.items()] if spaces else \
        [(f"{name}_N{N}_H{H}_L{L}", N, H, L, kw) for name, kw in (("discrete4", dict(n_actions=4)),
                                                                  ("box6", dict(action_dim=6)))
         for N in NS for H in HS for L in LS]
    key = "cells"
    if shared:  # beside what the file holds
        key, kept = "cells_shared", result
        with open(out_path) as f:
            result = json.load(f)
        result[key] = {"fused": "share_encoders=True, fused_step=True", "torch": "share_encoders=True, the switch off",
                       "separate_fused": "share_encoders=False, fused_step=True (for information)",
                       **{k: kept[k] for k in ("calls_per_block", "rounds", "unit")}}
    for name, N, H, L, kw in cells:
        result[key][name] = time_cell(N, H, L, kw, shared)
        with open(out_path, "w") as f:  # after every cell: a run cut short keeps what it measured
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))
