"""Rollout and evaluation time of the non-categorical PPO heads (DESIGN.md
§4.5-4.7): 8 agents x 128 envs, T = 16, default networks, SyntheticVecEnv.

Per configuration (Box A = 6; MultiDiscrete [3, 3] and [2] * 16; MultiBinary
n = 4 and n = 32):

  1. collect() through the head's persistent launch
     (agx_ppo_rollout_*_graph_persistent, PopulationRunner.head_persistent)
     against the per-step path (AGX_PERSISTENT_ROLLOUT=0: one policy-step
     launch, a D2H copy, an event wait, three H2D copies and the accounting ops
     per vector step) and against the categorical
     agx_ppo_rollout_graph_persistent on a Discrete population with the same
     layer list at the same logit count (pinned to the runtime-shape kernels);
  2. one evaluation pass of max_steps = EVAL_STEPS vector steps, the same three.

Host clock around calls that end in a device synchronise; each figure is the
median (and range) of REPEATS windows after a warm-up, the versions of a
configuration alternating inside one process.  Not part of bench.py.

Usage:  python tools/vector_rollout_time.py [--only rollout,eval] [--out FILE.json]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPEATS = 9
P, N, T = 8, 128, 16
EVAL_STEPS = 64
CONFIGS = [("box_A6", "box", 6), ("multidiscrete_3x3", "multi", (3, 3)), ("multidiscrete_2x16", "multi", (2,) * 16),
           ("multibinary_4", "bern", 4), ("multibinary_32", "bern", 32)]


def _window_ms(fn, calls: int) -> float:
    """Milliseconds per call of ``calls`` calls, the device drained at both ends."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


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


def _runners(kind, arg):
    """(head persistent, head per-step, categorical persistent) runners of one configuration."""
    from agilerl_amd.algorithms.ppo import spec_from_net_config
    from agilerl_amd.envs import Box, Discrete, MultiBinary, MultiDiscrete, SyntheticVecEnv
    from agilerl_amd.population.ppo_pop import PPOPopulation
    from agilerl_amd.population.runner import PopulationRunner

    obs_space = Box(-np.inf, np.inf, (8,))
    if kind == "box":
        space, env_kw, logits = Box(-1.0, 1.0, (arg,)), dict(action_dim=arg), arg
    elif kind == "multi":
        space, env_kw, logits = MultiDiscrete(arg), dict(nvec=list(arg)), int(sum(arg))
    else:
        space, env_kw, logits = MultiBinary(arg), dict(n_binary=arg), arg

    def make(space, env_kw, mode, pin_graph=False):
        os.environ["AGX_PERSISTENT_ROLLOUT"] = mode
        pop = PPOPopulation(spec_from_net_config(obs_space, space, None), P, N, learn_step=T * N,
                            seeds=list(range(P)))
        if pin_graph:  # a compiled shape too runs the runtime-shape kernels here
            pop._desc = False
        return PopulationRunner(pop, SyntheticVecEnv(P * N, seed=3, **env_kw))

    head, step = make(space, env_kw, "1"), make(space, env_kw, "0")
    cat = make(Discrete(logits), {}, "1", pin_graph=True)
    assert head.head_persistent and not step.head_persistent and cat.graph_persistent and not cat.persistent
    return head, step, cat, logits


def rollout(name, kind, arg) -> dict:
    head, step, cat, logits = _runners(kind, arg)
    out = _group({"head_persistent": head.collect, "head_per_step": step.collect,
                  "categorical_graph_persistent": cat.collect}, calls=20, warmup=5)
    for r in (head, cat):
        assert int(r.ctl_h.view(torch.int32)[1]) == 0, "a persistent launch timed out"
    out.update(what="collect(): one rollout of T vector steps", config=name,
               shape=f"{P} agents x {N} envs, T = {T}, {logits} logits, default networks",
               ratio_to_per_step=_ratio(out["head_persistent"], out["head_per_step"]),
               ratio_to_categorical=_ratio(out["head_persistent"], out["categorical_graph_persistent"]))
    return out


def evaluation(name, kind, arg) -> dict:
    head, step, cat, logits = _runners(kind, arg)
    fns = {k: (lambda r=r: r.evaluate(loop=1, max_steps=EVAL_STEPS))
           for k, r in (("head_persistent", head), ("head_per_step", step), ("categorical_persistent", cat))}
    out = _group(fns, calls=5, warmup=2)
    out.update(what=f"evaluate(loop=1, max_steps={EVAL_STEPS}): one pass", config=name,
               shape=f"{P} agents x {N} envs, {EVAL_STEPS} vector steps, {logits} logits, default networks",
               note="categorical_persistent is the Discrete population's own pass (agx_ppo_eval_multi_persistent)",
               ratio_to_per_step=_ratio(out["head_persistent"], out["head_per_step"]),
               ratio_to_categorical=_ratio(out["head_persistent"], out["categorical_persistent"]))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="rollout,eval", help="comma-separated: rollout, eval")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/vector_rollout_time.py needs the GPU: a CPU run says nothing about these times")
    np.random.seed(0)
    res = []
    for k in args.only.split(","):
        if k not in ("rollout", "eval"):
            raise SystemExit(f"unknown part {k!r}")
        for cfg in CONFIGS:
            res.append(rollout(*cfg) if k == "rollout" else evaluation(*cfg))
            print(json.dumps(res[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
