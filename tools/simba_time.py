"""SimBa encoder forward + backward on one GPU: the split plan the library
chooses, the whole kernels (AGX_SIMBA_SPLIT=0) and the torch modules
(AGX_SIMBA=0), in one process.

Every variant is captured once (forward, then autograd.grad down to x and every
parameter) and replayed: after a warm-up, ROUNDS rounds that alternate the
variants, each a block of REPLAYS replays between two device events.  Median
and min-max of the blocks, in microseconds per replay.  Grid: H in 128 .. 496,
B in 64 / 256 / 1024, in = 8, out = 32, 2 blocks, scale 4.  Then DQN.learn at
H = 496, B = 64 under the same three settings (host clock around calls that end
in a device synchronise; the later calls replay its captured update).

  python tools/simba_time.py [--out FILE] [--plans] [--cells H:B,H:B...]
      --plans also times the candidate plans of candidates() per cell: the
      sweep agx_simba_choose_plan's table was set from.  One JSON line, also
      written to FILE (default profiles/simba_time.json).
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HS = (128, 160, 192, 224, 256, 320, 496)
BS = (64, 256, 1024)
REPLAYS = int(os.environ.get("REPLAYS", 100))
ROUNDS = int(os.environ.get("ROUNDS", 5))
WARMUP = 10


def candidates(H, B):
    """The plans tried per cell: S = 2, 4, 8, 16 with R = 1 and Q = 1, 2, 4 (within the row tiles), and
    S = 4, 8 with R = 2 and 4 where there are that many row tiles and the LDS fits."""
    nrt, nt = -(-B // 16), 4 * H // 16
    out = {(S, 1, Q) for S in (2, 4, 8, 16) if S <= nt for Q in (1, 2, 4) if Q <= nrt}
    for R in (2, 4):
        if nrt >= 4 * R and 4 * (2 * 16 * R * (H + 4) + 32 * R + 16 * R * 132 + 4) <= 160 * 1024:
            out |= {(S, R, min(4, nrt)) for S in (4, 8)}
    return sorted(out)


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _capture(fn):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    g.keep = keep  # the outputs live in the graph's pool
    for _ in range(WARMUP):
        g.replay()
    torch.cuda.synchronize()
    return g


def _blocks(fns, per_block):
    """us per call of every variant: ROUNDS alternating blocks -> (median, min, max)."""
    import torch

    us = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(per_block):
                fn()
            end.record()
            end.synchronize()
            us[name].append(1e3 * start.elapsed_time(end) / per_block)
    return {n: [round(sorted(v)[len(v) // 2], 1), round(min(v), 1), round(max(v), 1)] for n, v in us.items()}


def time_cell(H, B, with_plans):
    import torch

    from agilerl_amd.modules.simba import EvolvableSimBa, _plan, choose_plan, simba_encoder

    torch.manual_seed(H + B)
    net = EvolvableSimBa(8, 32, H, 2, output_activation="ReLU", scale_factor=4, device="cuda")
    params = list(net.parameters())
    x = torch.randn(B, 8, device="cuda").requires_grad_(True)
    g = torch.randn(B, 32, device="cuda")

    def step(plan):
        y = net.model(x) if plan == "torch" else simba_encoder(net, x, plan=plan)
        return torch.autograd.grad((y * g).sum(), [x] + params)

    chosen = choose_plan(_plan(net)[0], B)
    graphs = {"chosen": _capture(lambda: step(None)), "torch": _capture(lambda: step("torch"))}
    with _Env(AGX_SIMBA_SPLIT="0"):
        graphs["whole"] = _capture(lambda: step(None))
    if with_plans and not (B <= 256 and H <= 224):  # inside the whole kernels' range the choice is fixed
        for p in candidates(H, B):
            graphs["plan_%d_%d_%d" % p] = _capture(lambda p=p: step(p))
    res = _blocks({n: gr.replay for n, gr in graphs.items()}, REPLAYS)
    res["chosen_plan"] = list(chosen)
    return res


def time_dqn(H, B):
    import numpy as np
    import torch

    from agilerl_amd.algorithms import DQN
    from agilerl_amd.envs import Box, Discrete

    rng = np.random.default_rng(3)
    e = {"obs": rng.standard_normal((B, 8)).astype(np.float32), "action": rng.integers(0, 4, (B, 1)),
         "reward": rng.standard_normal((B, 1)).astype(np.float32),
         "next_obs": rng.standard_normal((B, 8)).astype(np.float32),
         "done": (rng.random((B, 1)) < 0.2).astype(np.float32)}
    cfg = {"simba": True, "encoder_config": {"hidden_size": H, "num_blocks": 2}}
    envs = {"chosen": {"AGX_SIMBA": "1"}, "whole": {"AGX_SIMBA": "1", "AGX_SIMBA_SPLIT": "0"},
            "torch": {"AGX_SIMBA": "0"}}
    agents = {}
    for name in envs:
        torch.manual_seed(7)
        agents[name] = DQN(Box(-np.inf, np.inf, (8,)), Discrete(4), batch_size=B, lr=1e-4, net_config=cfg)

    def learn(name):
        with _Env(**envs[name]):
            agents[name].learn(e)

    for name in envs:
        for _ in range(WARMUP):
            learn(name)
    torch.cuda.synchronize()
    us = {name: [] for name in envs}
    for _ in range(ROUNDS):
        for name in envs:
            t0 = time.perf_counter()
            for _ in range(REPLAYS):
                learn(name)
            torch.cuda.synchronize()
            us[name].append(1e6 * (time.perf_counter() - t0) / REPLAYS)
    return {n: [round(sorted(v)[len(v) // 2], 1), round(min(v), 1), round(max(v), 1)] for n, v in us.items()}


if __name__ == "__main__":
    import torch

    assert torch.cuda.is_available(), "tools/simba_time.py measures on the GPU only"
    cells = [(H, B) for H in HS for B in BS]
    if "--cells" in sys.argv:
        cells = [tuple(int(v) for v in c.split(":")) for c in sys.argv[sys.argv.index("--cells") + 1].split(",")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
        os.path.join(ROOT, "profiles", "simba_time.json")
    result = {"replays_per_block": REPLAYS, "rounds": ROUNDS, "unit": "us: median, min, max", "cells": {}}
    for H, B in cells:
        result["cells"][f"H{H}_B{B}"] = time_cell(H, B, "--plans" in sys.argv)
        with open(out_path, "w") as f:  # after every cell: a run cut short keeps what it measured
            json.dump(result, f, indent=1)
            f.write("\n")
    if "--no-dqn" not in sys.argv:
        result["dqn_learn_H496_B64"] = time_dqn(496, 64)
    print(json.dumps(result))
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
