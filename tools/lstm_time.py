"""EvolvableLSTM's nn.LSTM on one GPU: the fused sequence kernels (AGX_LSTM=1)
in their whole-sequence form (``fused``) and their split per-step form
(``split``, csrc/lstm_split.hip) against torch's nn.LSTM (AGX_LSTM=0), in one
process.

Three modes per cell: ``step`` (no-grad, T = 1, B = 128: the rollout's call),
``fwd`` (no-grad sequence) and ``fwdbwd`` (forward, then autograd.grad down to
x, h0, c0 and every parameter).  The fused and split variants are captured
once and replayed.  torch's nn.LSTM cannot be captured here (its hipBLASLt calls
refuse a capturing stream and the process dies), so it is called eagerly
and its figures include the host's launch work: they are an upper bound on
torch's device time, and no automatic bound of EvolvableLSTM.forward is taken
from them.  After a warm-up, ROUNDS rounds alternate fused, split and torch,
each a block of REPLAYS calls between two device events.  Median and min-max
of the blocks, in microseconds per call.  Grid: H in 64 / 128 / 144 / 256 / 512
x L in 1 / 2, and for the sequence modes T in 16 / 64 x B in 32 / 128; input
size 8.

A cell's ``fused_clear`` is true when the fused maximum lies below torch's
(eager) minimum, its ``split_clear`` when the split maximum lies below the
fused minimum: agx_lstm_choose_plan returns split for the widths at which that
holds in every sequence cell (``split_clear_widths`` in the result).

  python tools/lstm_time.py [--out FILE]    (default profiles/lstm_time.json)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HS, LS, TS, BS = (64, 128, 144, 256, 512), (1, 2), (16, 64), (32, 128)
REPLAYS = int(os.environ.get("REPLAYS", 20))
ROUNDS = int(os.environ.get("ROUNDS", 5))
WARMUP = 5


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


def _blocks(fns):
    """us per replay of every variant: ROUNDS alternating blocks -> [median, min, max]."""
    import torch

    us = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(REPLAYS):
                fn()
            end.record()
            end.synchronize()
            us[name].append(1e3 * start.elapsed_time(end) / REPLAYS)
    return {n: [round(sorted(v)[len(v) // 2], 1), round(min(v), 1), round(max(v), 1)] for n, v in us.items()}


def time_cell(H, L, B, T, grad):
    import torch

    from agilerl_amd.modules.lstm import EvolvableLSTM, lstm_sequence

    torch.manual_seed(H + L + B + T)
    net = EvolvableLSTM(8, H, 32, num_layers=L, max_layers=L + 1, device="cuda")
    params = list(net.lstm.parameters())
    x, h0, c0 = (torch.randn(*s, device="cuda").requires_grad_(grad) for s in ((B, T, 8), (L, B, H), (L, B, H)))
    gy = torch.randn(B, T, H, device="cuda")

    def run(plan):
        with torch.set_grad_enabled(grad):
            if plan:
                y, h_n, c_n = lstm_sequence(net, x, h0, c0, plan=plan)
            else:
                y, (h_n, c_n) = net.lstm(x, (h0, c0))
            if not grad:
                return y, h_n, c_n
            return torch.autograd.grad([(y * gy).sum() + h_n.sum() + c_n.sum()], [x, h0, c0] + params)

    for _ in range(WARMUP):
        run(None)
    res = _blocks({"fused": _capture(lambda: run("whole")).replay, "split": _capture(lambda: run("split")).replay,
                   "torch": lambda: run(None)})
    res["fused_clear"] = res["fused"][2] < res["torch"][1]
    res["split_clear"] = res["split"][2] < res["fused"][1]
    return res


if __name__ == "__main__":
    import torch

    assert torch.cuda.is_available(), "tools/lstm_time.py measures on the GPU only"
    os.environ["AGX_LSTM"] = "1"
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
        os.path.join(ROOT, "profiles", "lstm_time.json")
    cells = [("step", H, L, 128, 1) for H in HS for L in LS]
    cells += [(mode, H, L, B, T) for mode in ("fwd", "fwdbwd") for H in HS for L in LS for T in TS for B in BS]
    result = {"replays_per_block": REPLAYS, "rounds": ROUNDS, "unit": "us: median, min, max",
              "fused": "captured graph replay", "split": "captured graph replay", "torch": "eager calls",
              "cells": {}}
    for mode, H, L, B, T in cells:
        result["cells"][f"{mode}_H{H}_L{L}_B{B}_T{T}"] = time_cell(H, L, B, T, mode == "fwdbwd")
        seq = {H: [c["split_clear"] for k, c in result["cells"].items() if f"_H{H}_" in k and k[:4] != "step"]
               for H in HS}
        result["split_clear_widths"] = [H for H in HS if seq[H] and all(seq[H])]
        with open(out_path, "w") as f:  # after every cell: a run cut short keeps what it measured
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))
