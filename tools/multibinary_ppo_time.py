"""Timing of PPO for MultiBinary actions, 8 agents x 128 envs,
default networks, n = 4, 16 and 32 bits:

  1. agx_ppo_act_bern_graph per vector step against the categorical
     agx_ppo_act_graph at n_actions = n (the same forward, one categorical head
     over the n logits) and, for n = 16, against agx_ppo_act_multi_graph at
     nvec = [2] * 16 (the MultiDiscrete stand-in for 16 switches);
  2. learn() through the fused Bernoulli learner (agx_ppo_learn_bern_graph;
     S = 2048, batch 128, 4 epochs) against (a) agx_ppo_learn_graph on a
     Discrete population with the same layer list, (b) the autograd learner on
     the same population and, for n = 16, (c) agx_ppo_learn_multi_graph at
     nvec = [2] * 16.

Device-event timing after a warm-up; each figure is the median of REPEATS
windows, the versions of a group alternating inside one process.  Not part of
bench.py.

Usage:  python tools/multibinary_ppo_time.py [--only policy,fused] [--out FILE.json]
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
WIDTHS = [4, 16, 32]


def _window_ms(fn, calls: int) -> float:
    """Milliseconds per call of ``calls`` back-to-back calls (device events)."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def _group(fns: dict, calls: int, warmup: int) -> dict:
    """name -> {median, min, max} ms of every function, their windows alternating."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            t[k].append(_window_ms(fn, calls))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in t.items()}


def _ratio(a: dict, b: dict) -> dict:
    return {"of_medians": a["median_ms"] / b["median_ms"], "min": a["min_ms"] / b["max_ms"],
            "max": a["max_ms"] / b["min_ms"]}


def _spaces(n):
    from agilerl_amd.envs import Box, Discrete, MultiBinary, MultiDiscrete

    return Box(-np.inf, np.inf, (8,)), MultiBinary(n), Discrete(n), (MultiDiscrete((2,) * 16) if n == 16 else None)


def policy_step(n, P=8, N=128) -> dict:
    from agilerl_amd.algorithms.ppo import spec_from_net_config
    from agilerl_amd.population.learner import graph_descriptor, policy_step_graph, policy_step_head
    from agilerl_amd.population.ppo_pop import PPOPopulation

    obs_space, binary, discrete, stand_in = _spaces(n)
    bern = PPOPopulation(spec_from_net_config(obs_space, binary, None), P, N, learn_step=2 * N)
    cat = PPOPopulation(spec_from_net_config(obs_space, discrete, None), P, N, learn_step=2 * N)
    cdesc = graph_descriptor(cat.spec)
    obs = torch.randn(P, N, 8, device="cuda")
    counter = [0]

    def step(fn, pop, *desc):
        def go():
            counter[0] += 1
            fn(pop, *desc, obs, N * 8, sample=True, counter=counter[0], actions=pop.actions[:, 0],
               log_probs=pop.log_probs[:, 0], values=pop.values[:, 0], out_agent_stride=pop.T * N)
        return go

    fns = {"agx_ppo_act_bern_graph": step(policy_step_head, bern),
           "agx_ppo_act_graph": step(policy_step_graph, cat, cdesc)}
    if stand_in is not None:
        multi = PPOPopulation(spec_from_net_config(obs_space, stand_in, None), P, N, learn_step=2 * N)
        fns["agx_ppo_act_multi_graph_2x16"] = step(policy_step_head, multi)
    out = _group(fns, calls=2000, warmup=200)
    out.update(what="policy step per vector step", shape=f"{P} agents x {N} envs, n = {n} bits, default networks",
               ratio_to_categorical=_ratio(out["agx_ppo_act_bern_graph"], out["agx_ppo_act_graph"]))
    if stand_in is not None:
        out["ratio_to_multi_2x16"] = _ratio(out["agx_ppo_act_bern_graph"], out["agx_ppo_act_multi_graph_2x16"])
    return out


def fused_learn(n, P=8, N=128, S=2048) -> dict:
    from agilerl_amd.algorithms.ppo import spec_from_net_config
    from agilerl_amd.population.learner import BernGraphLearner, GraphLearner, MultiGraphLearner
    from agilerl_amd.population.ppo_pop import PPOPopulation

    obs_space, binary, discrete, stand_in = _spaces(n)
    kw = dict(learn_step=S, batch_size=128, update_epochs=4)
    bern = PPOPopulation(spec_from_net_config(obs_space, binary, None), P, N, **kw)
    cat = PPOPopulation(spec_from_net_config(obs_space, discrete, None), P, N, **kw)
    pops = [bern, cat]
    if stand_in is not None:
        multi = PPOPopulation(spec_from_net_config(obs_space, stand_in, None), P, N, multi_fused=True, **kw)
        pops.append(multi)
    for pop in pops:
        pop.obs.normal_()
        for t in range(pop.T):
            pop.act_into(t)
        pop.rewards.normal_()
        pop.finish_rollout(torch.randn(P, N, 8, device="cuda"), torch.zeros(P, N, dtype=torch.uint8, device="cuda"))
    # the default networks are a compiled shape of agx_ppo_learn: pin the runtime-shape learner
    cat._fused = GraphLearner(cat)

    def run_torch():
        bern.fused = False  # head_learn_descriptor() is None: _learn_torch
        try:
            bern.learn()
        finally:
            bern.fused = True

    fns = {"agx_ppo_learn_bern_graph": bern.learn, "agx_ppo_learn_graph_categorical": cat.learn}
    if stand_in is not None:
        fns["agx_ppo_learn_multi_graph_2x16"] = multi.learn
    out = _group(fns, calls=20, warmup=5)
    assert isinstance(bern._fused, BernGraphLearner) and isinstance(cat._fused, GraphLearner)
    assert stand_in is None or isinstance(multi._fused, MultiGraphLearner)
    beside = _group({"agx_ppo_learn_bern_graph_beside_autograd": bern.learn, "autograd_learner": run_torch},
                    calls=3, warmup=2)
    for pop in pops:
        pop.check_errors()
    updates = bern.n_updates() // P
    out.update(beside)
    out.update(what="learn() through the fused Bernoulli learner",
               shape=f"{P} agents x {N} envs, S = {S}, batch 128, 4 epochs ({updates} minibatch updates), n = {n} "
               "bits, default networks",
               ratio_to_categorical=_ratio(out["agx_ppo_learn_bern_graph"], out["agx_ppo_learn_graph_categorical"]))
    if stand_in is not None:
        out["ratio_to_multi_2x16"] = _ratio(out["agx_ppo_learn_bern_graph"], out["agx_ppo_learn_multi_graph_2x16"])
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="policy,fused", help="comma-separated: policy, fused")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/multibinary_ppo_time.py needs the GPU: a CPU run says nothing about these times")
    np.random.seed(0)
    res = []
    for k in args.only.split(","):
        if k == "policy":
            res += [policy_step(n) for n in WIDTHS]
        elif k == "fused":
            res += [fused_learn(n) for n in WIDTHS]
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
