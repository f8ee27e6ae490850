"""Timing of PPO for Box actions (DESIGN.md §4 "PPO for Box actions"):

  1. agx_ppo_act_gauss_graph per vector step, 8 agents x 128 envs, A = 6,
     default networks, against the categorical agx_ppo_act_graph at the same
     shape (the same forward, the categorical head);
  2. learn() of the Box population on the autograd learner (S = 2048, batch
     128, 4 epochs), against the same learner with the Gaussian loss written
     in plain torch ops;
  3. learn() of the same population through the fused Gaussian learner
     (agx_ppo_learn_gauss_graph) against (a) the autograd learner of 2. and
     (b) the categorical agx_ppo_learn_graph on a Discrete population with the
     same layer list and n_actions = A.

Device-event timing after a warm-up; each figure is the median of REPEATS
windows, the two versions of a pair alternating inside one process.  Not part
of bench.py.

Usage:  python tools/gauss_ppo_time.py [--only policy,learn,fused] [--out FILE.json]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPEATS = 7


def _window_ms(fn, calls: int) -> float:
    """Milliseconds per call of ``calls`` back-to-back calls (device events)."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def _pair(a, b, calls: int, warmup: int) -> tuple[dict, dict]:
    for _ in range(warmup):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REPEATS):
        ta.append(_window_ms(a, calls))
        tb.append(_window_ms(b, calls))
    rec = lambda t: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}  # noqa: E731
    return rec(ta), rec(tb)


def policy_step(P=8, N=128, A=6) -> dict:
    from agilerl_amd.algorithms.ppo import spec_from_net_config
    from agilerl_amd.envs import Box, Discrete
    from agilerl_amd.population.learner import graph_descriptor, policy_step_graph, policy_step_head
    from agilerl_amd.population.ppo_pop import PPOPopulation

    obs_space = Box(-np.inf, np.inf, (8,))
    gauss = PPOPopulation(spec_from_net_config(obs_space, Box(-1.0, 1.0, (A,)), None), P, N, learn_step=2 * N)
    cat = PPOPopulation(spec_from_net_config(obs_space, Discrete(A), None), P, N, learn_step=2 * N)
    cdesc = graph_descriptor(cat.spec)
    obs = torch.randn(P, N, 8, device="cuda")
    counter = [0]

    def run_gauss():
        counter[0] += 1
        policy_step_head(gauss, obs, N * 8, sample=True, counter=counter[0], actions=gauss.actions[:, 0],
                         log_probs=gauss.log_probs[:, 0], values=gauss.values[:, 0], out_agent_stride=gauss.T * N)

    def run_cat():
        counter[0] += 1
        policy_step_graph(cat, cdesc, obs, N * 8, sample=True, counter=counter[0], actions=cat.actions[:, 0],
                          log_probs=cat.log_probs[:, 0], values=cat.values[:, 0], out_agent_stride=cat.T * N)

    g, c = _pair(run_gauss, run_cat, calls=2000, warmup=200)
    return {"what": "policy step per vector step", "shape": f"{P} agents x {N} envs, A = {A}, default networks",
            "agx_ppo_act_gauss_graph": g, "agx_ppo_act_graph": c}


def learn(P=8, N=128, S=2048, A=6) -> dict:
    from agilerl_amd.algorithms.ppo import spec_from_net_config
    from agilerl_amd.envs import Box
    from agilerl_amd.population import ppo_pop
    from agilerl_amd.population.nets import gaussian
    from agilerl_amd.population.ppo_pop import PPOPopulation

    pop = PPOPopulation(spec_from_net_config(Box(-np.inf, np.inf, (8,)), Box(-1.0, 1.0, (A,)), None), P, N,
                        learn_step=S, batch_size=128, update_epochs=4, fused=False)  # the autograd learner
    pop.obs.normal_()
    for t in range(pop.T):
        pop.act_into(t)
    pop.rewards.normal_()
    pop.finish_rollout(torch.randn(P, N, 8, device="cuda"), torch.zeros(P, N, dtype=torch.uint8, device="cuda"))
    hip_fn = ppo_pop._PPOGaussLossFn

    class TorchLoss:
        """_PPOGaussLossFn's interface with the loss in plain torch ops."""

        @staticmethod
        def apply(mean, value, log_std, actions, old_logp, adv, ret, old_v, gidx, b, clip, vf, ent):
            Pn = mean.shape[0]
            logp, H = gaussian(mean, log_std.unsqueeze(1), actions[gidx].view(Pn, b, -1))
            olp, a, r, ov = (x[gidx].view(Pn, b) for x in (old_logp, adv, ret, old_v))
            lr_ = logp - olp
            ratio = lr_.exp()
            pg = torch.max(-a * ratio, -a * ratio.clamp(1 - clip, 1 + clip)).mean(1)
            vc = ov + (value - ov).clamp(-clip, clip)
            vl = 0.5 * torch.max((value - r) ** 2, (vc - r) ** 2).mean(1)
            loss = pg + vf * vl - ent * H.mean(1)
            with torch.no_grad():
                stats = torch.zeros(Pn, 8, device=mean.device)
                stats[:, 0] = loss
                stats[:, 4] = ((ratio - 1) - lr_).mean(1)
            return loss.sum(), stats

    def run(fn):
        def go():
            ppo_pop._PPOGaussLossFn = fn
            pop.learn()
        return go

    try:
        h, t = _pair(run(hip_fn), run(TorchLoss), calls=3, warmup=2)
    finally:
        ppo_pop._PPOGaussLossFn = hip_fn
    updates = pop.n_updates() // P
    return {"what": "learn() of the Box population", "shape": f"{P} agents, S = {S}, batch 128, 4 epochs "
            f"({updates} minibatch updates)", "hip_loss": h, "torch_loss": t}


def fused_learn(P=8, N=128, S=2048, A=6) -> dict:
    from agilerl_amd.algorithms.ppo import spec_from_net_config
    from agilerl_amd.envs import Box, Discrete
    from agilerl_amd.population.learner import GaussGraphLearner, GraphLearner
    from agilerl_amd.population.ppo_pop import PPOPopulation

    obs_space = Box(-np.inf, np.inf, (8,))
    kw = dict(learn_step=S, batch_size=128, update_epochs=4)
    box = PPOPopulation(spec_from_net_config(obs_space, Box(-1.0, 1.0, (A,)), None), P, N, **kw)
    cat = PPOPopulation(spec_from_net_config(obs_space, Discrete(A), None), P, N, **kw)
    for pop in (box, cat):
        pop.obs.normal_()
        for t in range(pop.T):
            pop.act_into(t)
        pop.rewards.normal_()
        pop.finish_rollout(torch.randn(P, N, 8, device="cuda"), torch.zeros(P, N, dtype=torch.uint8, device="cuda"))
    # the default networks are a compiled shape of agx_ppo_learn: pin the runtime-shape learner
    cat._fused = GraphLearner(cat)

    def run_torch():
        box.fused = False  # head_learn_descriptor() is None: _learn_torch
        try:
            box.learn()
        finally:
            box.fused = True

    f, c = _pair(box.learn, cat.learn, calls=20, warmup=5)
    assert isinstance(box._fused, GaussGraphLearner) and isinstance(cat._fused, GraphLearner)
    f2, t = _pair(box.learn, run_torch, calls=3, warmup=2)
    box.check_errors()
    cat.check_errors()
    updates = box.n_updates() // P
    return {"what": "learn() through the fused Gaussian learner", "shape": f"{P} agents x {N} envs, S = {S}, batch "
            f"128, 4 epochs ({updates} minibatch updates), A = {A}, default networks",
            "agx_ppo_learn_gauss_graph": f, "agx_ppo_learn_graph_categorical": c,
            "agx_ppo_learn_gauss_graph_beside_autograd": f2, "autograd_learner": t}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="policy,learn,fused", help="comma-separated: policy, learn, fused")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gauss_ppo_time.py needs the GPU: a CPU run says nothing about these times")
    np.random.seed(0)
    parts = {"policy": policy_step, "learn": learn, "fused": fused_learn}
    res = [parts[k]() for k in args.only.split(",")]
    for r in res:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
