"""TD3.learn per update on one GPU: the shipped path (agx_td3_smooth_actions,
agx_td3_critic_target, flat-buffer Adam and Polyak) against the plain-torch
update of tests/td3_twin.py on copies of the same networks (the baseline:
what the reference's learn costs on this GPU).  Default networks, 8-dim
observations, 6-dim actions, B = 64 and 256, one fixed device batch.

  python tools/td3_update_time.py
      updates/s of both paths per batch size: warm-up, then ROUNDS alternating
      blocks of UPDATES updates each, every block between two device events
      (learn returns its losses to the host, as the reference's API does, so
      a block's span includes those round trips); the median block is reported.
      One JSON line.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o td3 -- python tools/td3_update_time.py --markers
  python tools/td3_update_time.py --count DIR/.../td3_kernel_trace.csv
      launches per update: --markers runs UPDATES updates of each path per
      batch size between marker kernels (agx_debug_stream's stream_kernel<1>),
      --count divides the kernels of each window by UPDATES.
"""
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCHES = (64, 256)
UPDATES = int(os.environ.get("UPDATES", 200))
ROUNDS = int(os.environ.get("ROUNDS", 5))
WARMUP = 20


def setup(B):
    import torch

    from agilerl_amd.algorithms import TD3
    from agilerl_amd.envs import Box
    from tests.td3_twin import Twin

    torch.manual_seed(0)
    agent = TD3(Box(-float("inf"), float("inf"), (8,)), Box(-1.0, 1.0, (6,)), batch_size=B)
    twin = Twin.of(agent)
    g = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    batch = {"obs": r(B, 8), "action": torch.tanh(r(B, 6)), "reward": r(B, 1), "next_obs": r(B, 8),
             "done": (torch.rand(B, 1, device="cuda", generator=g) < 0.05).float()}
    return {"shipped": lambda: agent.learn(batch), "twin": lambda: twin.learn(batch)}


def time_paths():
    import torch

    out = {}
    for B in BATCHES:
        paths = setup(B)
        for fn in paths.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in paths}
        for _ in range(ROUNDS):
            for name, fn in paths.items():
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(UPDATES):
                    fn()
                end.record()
                end.synchronize()
                ms[name].append(start.elapsed_time(end) / UPDATES)
        for name, v in ms.items():
            v.sort()
            out[f"B{B}_{name}_updates_per_s"] = round(1e3 / v[len(v) // 2], 1)
            out[f"B{B}_{name}_ms_min_max"] = [round(v[0], 4), round(v[-1], 4)]
    print(json.dumps(out))


def run_markers():
    import torch

    from agilerl_amd import _lib

    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")

    def marker():
        torch.cuda.synchronize()
        _lib.call("agx_debug_stream", buf.data_ptr(), buf[32:].data_ptr(), 16, 1, 1, _lib.stream())
        torch.cuda.synchronize()

    for B in BATCHES:
        for fn in setup(B).values():  # windows in the order B64 shipped, B64 twin, B256 shipped, B256 twin
            for _ in range(WARMUP):
                fn()
            marker()
            for _ in range(UPDATES):
                fn()
            marker()


def count(path):
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(path)))
    marks = [i for i, (_, n) in enumerate(rows) if "stream_kernel<1>" in n]
    names = [f"B{B}_{p}" for B in BATCHES for p in ("shipped", "twin")]
    if len(marks) != 2 * len(names):
        sys.exit(f"{path}: {len(marks)} markers, expected {2 * len(names)}")
    out = {}
    for k, name in enumerate(names):
        win = rows[marks[2 * k] + 1:marks[2 * k + 1]]
        out[f"{name}_launches_per_update"] = round(len(win) / UPDATES, 1)
        out[f"{name}_agx_launches_per_update"] = round(sum("agx::" in n for _, n in win) / UPDATES, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    if "--count" in sys.argv:
        count(sys.argv[sys.argv.index("--count") + 1])
    elif "--markers" in sys.argv:
        run_markers()
    else:
        time_paths()
