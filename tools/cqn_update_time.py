"""CQN.learn per update on one GPU, and agx_cqn_loss alone.

The update: the shipped path replayed from its captured graph, the same path
eager (AGX_LEARN_GRAPH=0), and the plain-torch update of tests/cqn_twin.py on
copies of the same networks (the baseline: what the reference's learn costs on
this GPU), in one process, on one fixed device batch.  Default networks, 8-dim
observations, 4 actions, B = 64 and 256.

The kernel: agx_cqn_loss (with its sums, double = False) against the same
loss as torch ops with its backward pass down to Q(s), both replayed from a
captured graph, at 2^20 x 6 (the row-per-lane form) and 2^16 x 64 (the
row-per-wave form); GB/s over the algorithmic bytes (Q(s), Q_target(s') and
the gradient once each, plus the per-row vectors).  Every replay reads the
same 96 MB / 50 MB of inputs, which stay resident in the 256 MB Infinity
Cache for both paths: the figures are cache-warm, not HBM, figures.

  python tools/cqn_update_time.py [--out FILE]
      updates/s of the three paths per batch size: warm-up, then ROUNDS
      alternating blocks of UPDATES updates each, every block between two
      device events (learn returns its loss to the host, as the reference's
      API does, so a block's span includes those round trips); the median
      block and the range are reported.  Then the kernel numbers.  One JSON
      line (also written to FILE).

  rocprofv3 --kernel-trace --output-format csv -d DIR -o cqn -- python tools/cqn_update_time.py --markers
  python tools/cqn_update_time.py --count DIR/.../cqn_kernel_trace.csv
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
PATHS = ("captured", "eager", "twin")
KERNEL_SHAPES = ((1 << 20, 6), (1 << 16, 64))


def setup(B):
    import torch

    from agilerl_amd.algorithms import CQN
    from agilerl_amd.envs import Box, Discrete
    from tests.cqn_twin import Twin

    torch.manual_seed(0)
    agent = CQN(Box(-float("inf"), float("inf"), (8,)), Discrete(4), batch_size=B)
    eager, twin = agent.clone(), Twin.of(agent)
    g = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    batch = {"obs": r(B, 8), "action": torch.randint(0, 4, (B, 1), device="cuda", generator=g), "reward": r(B, 1),
             "next_obs": r(B, 8), "done": (torch.rand(B, 1, device="cuda", generator=g) < 0.05).float()}

    def eager_learn():
        os.environ["AGX_LEARN_GRAPH"] = "0"
        try:
            return eager.learn(batch)
        finally:
            os.environ.pop("AGX_LEARN_GRAPH", None)

    return {"captured": lambda: agent.learn(batch), "eager": eager_learn, "twin": lambda: twin.learn(batch)}


def _blocks(paths, per_block):
    """ms per call of every path: ROUNDS alternating blocks, sorted."""
    import torch

    ms = {name: [] for name in paths}
    for _ in range(ROUNDS):
        for name, fn in paths.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(per_block):
                fn()
            end.record()
            end.synchronize()
            ms[name].append(start.elapsed_time(end) / per_block)
    for v in ms.values():
        v.sort()
    return ms


def time_updates(out):
    import torch

    for B in BATCHES:
        paths = setup(B)
        for fn in paths.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        for name, v in _blocks(paths, UPDATES).items():
            out[f"B{B}_{name}_updates_per_s"] = round(1e3 / v[len(v) // 2], 1)
            out[f"B{B}_{name}_ms_min_max"] = [round(v[0], 4), round(v[-1], 4)]


def _torch_ops(q_cur, q_next_target, actions, rewards, dones, gamma):
    """The loss as torch ops (tests/cqn_twin.py cql_loss_torch) and its
    backward pass down to Q(s) -> (loss, dloss/dQ)."""
    import torch

    from tests.cqn_twin import cql_loss_torch

    q = q_cur.detach().requires_grad_(True)
    _, _, loss = cql_loss_torch(None, q_next_target, q, actions, rewards, dones, gamma, False)
    (grad,) = torch.autograd.grad(loss, q)
    return loss, grad


def time_kernel(out):
    import torch

    from agilerl_amd import kernels as K

    for B, A in KERNEL_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(2)
        q_cur = 3 * torch.randn(B, A, device="cuda", generator=g)
        q_next = 3 * torch.randn(B, A, device="cuda", generator=g)
        actions = torch.randint(0, A, (B, 1), device="cuda", generator=g)
        rewards = torch.randn(B, 1, device="cuda", generator=g)
        dones = (torch.rand(B, 1, device="cuda", generator=g) < 0.2).float()
        fns = {"agx": lambda: K.cqn_loss(q_cur, q_next, actions, rewards, dones, 0.99),
               "torch": lambda: _torch_ops(q_cur, q_next, actions, rewards, dones, 0.99)}
        graphs = {}
        for name, fn in fns.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                keep = fn()  # noqa: F841 - the outputs live in the graph's pool
            for _ in range(5):
                graphs[name].replay()
        torch.cuda.synchronize()
        nbytes = 3 * B * A * 4 + B * (8 + 4 + 4 + 4)
        for name, v in _blocks({n: gr.replay for n, gr in graphs.items()}, 20).items():
            med = v[len(v) // 2]
            out[f"kernel_{B}x{A}_{name}_us"] = round(med * 1e3, 2)
            out[f"kernel_{B}x{A}_{name}_us_min_max"] = [round(v[0] * 1e3, 2), round(v[-1] * 1e3, 2)]
            out[f"kernel_{B}x{A}_{name}_GBps"] = round(nbytes / (med * 1e-3) / 1e9, 1)


def run_markers():
    import torch

    from agilerl_amd import _lib

    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")

    def marker():
        torch.cuda.synchronize()
        _lib.call("agx_debug_stream", buf.data_ptr(), buf[32:].data_ptr(), 16, 1, 1, _lib.stream())
        torch.cuda.synchronize()

    for B in BATCHES:
        for fn in setup(B).values():  # windows in the order of PATHS per batch size
            for _ in range(WARMUP):
                fn()
            marker()
            for _ in range(UPDATES):
                fn()
            marker()


def count(path):
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(path)))
    marks = [i for i, (_, n) in enumerate(rows) if "stream_kernel<1>" in n]
    names = [f"B{B}_{p}" for B in BATCHES for p in PATHS]
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
        result = {"updates_per_block": UPDATES, "blocks": ROUNDS}
        time_updates(result)
        time_kernel(result)
        print(json.dumps(result))
        if "--out" in sys.argv:
            with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
