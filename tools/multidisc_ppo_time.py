"""Timing of PPO for MultiDiscrete actions:

  1. agx_ppo_act_multi_graph per vector step, 8 agents x 128 envs, default
     networks, nvec = [4], [3, 3] and [2] * 16, each against the categorical
     agx_ppo_act_graph at the same logit count L = sum(nvec) (the same forward,
     one categorical head over all L logits);
  2. learn() of a MultiDiscrete population on the autograd learner (S = 2048,
     batch 128, 4 epochs) with the fused loss kernel
     (agx_ppo_multi_loss_fwd_bwd), against the same learner with the
     multi-categorical loss written in plain torch ops;
  3. learn() through the fused multi-categorical learner
     (agx_ppo_learn_multi_graph, ``multi_fused=True``) at the same shape for
     nvec = [3, 3] and [2] * 16, against (a) the autograd learner on the same
     population and (b) agx_ppo_learn_graph on a Discrete population with the
     same layer list and n_actions = L.

Device-event timing after a warm-up; each figure is the median of REPEATS
windows, the two versions of a pair alternating inside one process.  Not part
of bench.py.

Usage:  python tools/multidisc_ppo_time.py [--only policy,learn,fused] [--out FILE.json]
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
NVECS = [(4,), (3, 3), (2,) * 16]


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


def policy_step(nvec, P=8, N=128) -> dict:
    from agilerl_amd.algorithms.ppo import spec_from_net_config
    from agilerl_amd.envs import Box, Discrete, MultiDiscrete
    from agilerl_amd.population.learner import graph_descriptor, policy_step_graph, policy_step_head
    from agilerl_amd.population.ppo_pop import PPOPopulation

    obs_space = Box(-np.inf, np.inf, (8,))
    L = int(sum(nvec))
    multi = PPOPopulation(spec_from_net_config(obs_space, MultiDiscrete(nvec), None), P, N, learn_step=2 * N)
    cat = PPOPopulation(spec_from_net_config(obs_space, Discrete(L), None), P, N, learn_step=2 * N)
    cdesc = graph_descriptor(cat.spec)
    obs = torch.randn(P, N, 8, device="cuda")
    counter = [0]

    def run_multi():
        counter[0] += 1
        policy_step_head(multi, obs, N * 8, sample=True, counter=counter[0], actions=multi.actions[:, 0],
                         log_probs=multi.log_probs[:, 0], values=multi.values[:, 0], out_agent_stride=multi.T * N)

    def run_cat():
        counter[0] += 1
        policy_step_graph(cat, cdesc, obs, N * 8, sample=True, counter=counter[0], actions=cat.actions[:, 0],
                          log_probs=cat.log_probs[:, 0], values=cat.values[:, 0], out_agent_stride=cat.T * N)

    m, c = _pair(run_multi, run_cat, calls=2000, warmup=200)
    return {"what": "policy step per vector step", "shape": f"{P} agents x {N} envs, nvec = {list(nvec)} "
            f"(K = {len(nvec)}, L = {L}), default networks", "agx_ppo_act_multi_graph": m, "agx_ppo_act_graph": c,
            "ratio_of_medians": m["median_ms"] / c["median_ms"]}


def learn(P=8, N=128, S=2048, nvec=(3, 3)) -> dict:
    from agilerl_amd.algorithms.ppo import spec_from_net_config
    from agilerl_amd.envs import Box, MultiDiscrete
    from agilerl_amd.population import ppo_pop
    from agilerl_amd.population.nets import multi_categorical
    from agilerl_amd.population.ppo_pop import PPOPopulation

    pop = PPOPopulation(spec_from_net_config(Box(-np.inf, np.inf, (8,)), MultiDiscrete(nvec), None), P, N,
                        learn_step=S, batch_size=128, update_epochs=4)
    pop.obs.normal_()
    for t in range(pop.T):
        pop.act_into(t)
    pop.rewards.normal_()
    pop.finish_rollout(torch.randn(P, N, 8, device="cuda"), torch.zeros(P, N, dtype=torch.uint8, device="cuda"))
    hip_fn = ppo_pop._PPOMultiLossFn

    class TorchLoss:
        """_PPOMultiLossFn's interface with the loss in plain torch ops."""

        @staticmethod
        def apply(logits, value, head, actions, masks, old_logp, adv, ret, old_v, gidx, b, clip, vf, ent):
            Pn = logits.shape[0]
            mk = None if masks is None else masks[gidx].view(Pn, b, -1)
            logp, H = multi_categorical(logits, nvec, actions[gidx].view(Pn, b, -1), mk)
            olp, a, r, ov = (x[gidx].view(Pn, b) for x in (old_logp, adv, ret, old_v))
            lr_ = logp - olp
            ratio = lr_.exp()
            pg = torch.max(-a * ratio, -a * ratio.clamp(1 - clip, 1 + clip)).mean(1)
            vc = ov + (value - ov).clamp(-clip, clip)
            vl = 0.5 * torch.max((value - r) ** 2, (vc - r) ** 2).mean(1)
            loss = pg + vf * vl - ent * H.mean(1)
            with torch.no_grad():
                stats = torch.zeros(Pn, 8, device=logits.device)
                stats[:, 0] = loss
                stats[:, 4] = ((ratio - 1) - lr_).mean(1)
            return loss.sum(), stats

    def run(fn):
        def go():
            ppo_pop._PPOMultiLossFn = fn
            pop.learn()
        return go

    try:
        h, t = _pair(run(hip_fn), run(TorchLoss), calls=3, warmup=2)
    finally:
        ppo_pop._PPOMultiLossFn = hip_fn
    updates = pop.n_updates() // P
    return {"what": "learn() of the MultiDiscrete population", "shape": f"{P} agents, S = {S}, batch 128, 4 epochs "
            f"({updates} minibatch updates), nvec = {list(nvec)}", "hip_loss": h, "torch_loss": t}


def fused_learn(nvec, P=8, N=128, S=2048) -> dict:
    from agilerl_amd.algorithms.ppo import spec_from_net_config
    from agilerl_amd.envs import Box, Discrete, MultiDiscrete
    from agilerl_amd.population.learner import GraphLearner, MultiGraphLearner
    from agilerl_amd.population.ppo_pop import PPOPopulation

    obs_space = Box(-np.inf, np.inf, (8,))
    L = int(sum(nvec))
    kw = dict(learn_step=S, batch_size=128, update_epochs=4)
    multi = PPOPopulation(spec_from_net_config(obs_space, MultiDiscrete(nvec), None), P, N, multi_fused=True, **kw)
    cat = PPOPopulation(spec_from_net_config(obs_space, Discrete(L), None), P, N, **kw)
    for pop in (multi, cat):
        pop.obs.normal_()
        for t in range(pop.T):
            pop.act_into(t)
        pop.rewards.normal_()
        pop.finish_rollout(torch.randn(P, N, 8, device="cuda"), torch.zeros(P, N, dtype=torch.uint8, device="cuda"))
    # the default networks are a compiled shape of agx_ppo_learn: pin the runtime-shape learner
    cat._fused = GraphLearner(cat)

    def run_torch():
        multi.fused = False  # head_learn_descriptor() is None: _learn_torch
        try:
            multi.learn()
        finally:
            multi.fused = True

    f, c = _pair(multi.learn, cat.learn, calls=20, warmup=5)
    assert isinstance(multi._fused, MultiGraphLearner) and isinstance(cat._fused, GraphLearner)
    f2, t = _pair(multi.learn, run_torch, calls=3, warmup=2)
    multi.check_errors()
    cat.check_errors()
    updates = multi.n_updates() // P
    return {"what": "learn() through the fused multi-categorical learner", "shape": f"{P} agents x {N} envs, S = {S}, "
            f"batch 128, 4 epochs ({updates} minibatch updates), nvec = {list(nvec)} (K = {len(nvec)}, L = {L}), "
            "default networks", "agx_ppo_learn_multi_graph": f, "agx_ppo_learn_graph_categorical": c,
            "ratio_to_categorical": {"of_medians": f["median_ms"] / c["median_ms"],
                                     "min": f["min_ms"] / c["max_ms"], "max": f["max_ms"] / c["min_ms"]},
            "agx_ppo_learn_multi_graph_beside_autograd": f2, "autograd_learner": t}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="policy,learn,fused", help="comma-separated: policy, learn, fused")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/multidisc_ppo_time.py needs the GPU: a CPU run says nothing about these times")
    np.random.seed(0)
    res = []
    for k in args.only.split(","):
        if k == "policy":
            res += [policy_step(nvec) for nvec in NVECS]
        elif k == "learn":
            res.append(learn())
        elif k == "fused":
            res += [fused_learn(nvec) for nvec in ((3, 3), (2,) * 16)]
        else:
            raise SystemExit(f"unknown part {k!r}")
    for r in res:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
