"""MATD3.learn per update on one GPU: the shipped path
(agx_matd3_critic_target, one agx_clip_adam launch per optimizer step over
flat buffers, one agx_polyak_segments launch per soft update) against the
plain-torch update of tests/test_matd3_gpu.py (``_reference_learn``, the
restatement of matd3.py:700-926) on copies of the same networks — the
baseline: what the reference's learn costs on this GPU.  Speaker-listener
shapes (two agents: obs 3 / 11, 3 / 5 discrete actions), default networks,
policy_freq 2, B = 64 and 256, one fixed device batch.  With policy_freq 2
every second update also steps the actors and the targets; every figure is
the mean over an even number of consecutive updates.

  python tools/matd3_update_time.py [--out profiles/matd3_update_time.json]
      updates/s of both paths per batch size: warm-up, then ROUNDS alternating
      blocks of UPDATES updates each, every block between two device events
      (learn returns its losses to the host, as the reference's API does, so
      a block's span includes those round trips); the median block is
      reported with the fastest and slowest.  One JSON line, also written to --out.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o matd3 -- python tools/matd3_update_time.py --markers
  python tools/matd3_update_time.py --count DIR/.../matd3_kernel_trace.csv [--out ...]
      launches per update: --markers runs UPDATES updates of each path per
      batch size between marker kernels (agx_debug_stream's stream_kernel<1>),
      --count divides the kernels of each window by UPDATES and merges the
      figures into --out.
"""
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (64, 256)
UPDATES = int(os.environ.get("UPDATES", 200))  # even: as many delayed updates as full ones
ROUNDS = int(os.environ.get("ROUNDS", 5))
WARMUP = 20
POLICY_FREQ = 2


def setup(B):
    import copy

    import torch

    from agilerl_amd.algorithms import MATD3
    from agilerl_amd.envs import SyntheticMultiAgentVecEnv
    from tests.test_matd3_gpu import GROUPS, _reference_learn

    env = SyntheticMultiAgentVecEnv(8)
    ids = env.agents
    torch.manual_seed(0)
    agent = MATD3([env.observation_spaces[a] for a in ids], [env.action_spaces[a] for a in ids], agent_ids=ids,
                  batch_size=B, vect_noise_dim=8, policy_freq=POLICY_FREQ)
    nets = copy.deepcopy(tuple(getattr(agent, g) for g in GROUPS))
    opts = tuple({a: torch.optim.Adam(nets[k][a].parameters(), lr=lr) for a in ids}
                 for k, lr in ((0, agent.lr_actor), (1, agent.lr_critic), (2, agent.lr_critic)))
    counter = dict.fromkeys(ids, 0)
    g = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    obs_dim = {a: env.observation_spaces[a].shape[0] for a in ids}
    batch = ({a: r(B, obs_dim[a]) for a in ids},
             {a: torch.softmax(r(B, agent.action_dims[a]), dim=-1) for a in ids},  # raw actions: the actors' outputs
             {a: r(B, 1) for a in ids},
             {a: r(B, obs_dim[a]) for a in ids},
             {a: (torch.rand(B, 1, device="cuda", generator=g) < 0.05).float() for a in ids})
    return {"shipped": lambda: agent.learn(batch),
            "twin": lambda: _reference_learn(agent, nets, opts, counter, batch)}


def _merge(path, figures):
    if not path:
        return
    old = json.load(open(path)) if os.path.exists(path) else {}
    old.update(figures)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(old, f, indent=1, sort_keys=True)
        f.write("\n")


def time_paths(out_path):
    import torch

    out = {"updates_per_block": UPDATES, "blocks": ROUNDS, "policy_freq": POLICY_FREQ,
           "device": torch.cuda.get_device_name(0)}
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
            out[f"B{B}_{name}_updates_per_s_min_max"] = [round(1e3 / v[-1], 1), round(1e3 / v[0], 1)]
            out[f"B{B}_{name}_ms_min_max"] = [round(v[0], 4), round(v[-1], 4)]
        out[f"B{B}_shipped_over_twin"] = round(out[f"B{B}_shipped_updates_per_s"] / out[f"B{B}_twin_updates_per_s"], 3)
    print(json.dumps(out))
    _merge(out_path, out)


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


def count(path, out_path):
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
    _merge(out_path, out)


if __name__ == "__main__":
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
        os.path.join(ROOT, "profiles", "matd3_update_time.json")
    if "--count" in sys.argv:
        count(sys.argv[sys.argv.index("--count") + 1], out_path)
    elif "--markers" in sys.argv:
        run_markers()
    else:
        time_paths(out_path)
