"""IPPO.learn per call on one GPU, on the three-agent speaker-listener shapes
(speaker_0: obs 3 / 3 actions; listener_0, listener_1: obs 11 / 5 actions, one
shared network), 128 envs, learn_step 2048 (T = 16), batch 128, 4 epochs,
default networks:

  (a) ``fused``  IPPO.learn as shipped: one upload and one bootstrap launch per
                 group, one agx_ippo_gae launch, then gather + per-minibatch
                 normalisation + learner (three launches) per group;
  (b) ``loop``   the same agent with AGX_IPPO_FUSED=0: the per-minibatch loop;
  (c) ``torch``  a plain-torch restatement of the reference's step
                 (ippo.py:644-836) on copies of the same networks in the same
                 process: GAE as T steps of CPU float32 ops, minibatches
                 through autograd, clip_grad_norm_ and torch.optim.Adam twice —
                 the baseline: what the reference's learn costs on this GPU;

and agx_ippo_gae alone (device events) against that T-step torch loop (host
clock; it runs on the CPU, where the reference runs it).

  python tools/ippo_time.py [--out profiles/ippo_time.json]
      warm-up, then ROUNDS alternating blocks of CALLS calls each; the median
      block is reported with the fastest and slowest.  learn returns its
      losses to the host, as the reference's API does, so a block's span
      includes that round trip.  One JSON line, also written to --out.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS = {"speaker_0": (3, 3), "listener_0": (11, 5), "listener_1": (11, 5)}
N, LEARN_STEP, BATCH, EPOCHS = 128, 2048, 128, 4
CALLS = int(os.environ.get("CALLS", 5))
ROUNDS = int(os.environ.get("ROUNDS", 5))
WARMUP = 2


def torch_gae(r, d, v, nv, nd, gamma, lam):
    import torch

    adv = torch.zeros_like(r)
    last = 0
    T = r.shape[0]
    for t in reversed(range(T)):
        nnt = 1.0 - (nd if t == T - 1 else d[t + 1])
        nxt = nv if t == T - 1 else v[t + 1]
        delta = r[t] + gamma * nxt * nnt - v[t]
        adv[t] = last = delta + gamma * lam * nnt * last
    return adv, adv + v


def setup():
    import numpy as np
    import torch

    from agilerl_amd.algorithms import IPPO
    from agilerl_amd.algorithms.ippo import assemble_rows
    from agilerl_amd.envs import Box, Discrete
    from agilerl_amd.population.nets import categorical

    ids = list(DIMS)
    agent = IPPO({a: Box(-np.inf, np.inf, (DIMS[a][0],)) for a in ids}, {a: Discrete(DIMS[a][1]) for a in ids},
                 agent_ids=ids, batch_size=BATCH, learn_step=LEARN_STEP, update_epochs=EPOCHS, lr=1e-4)
    T = -(LEARN_STEP // -N)
    rng = np.random.default_rng(0)
    f = np.float32
    exp = tuple({a: x(a) for a in ids} for x in (
        lambda a: rng.standard_normal((T, N, DIMS[a][0])).astype(f), lambda a: rng.integers(0, DIMS[a][1], (T, N)),
        lambda a: rng.uniform(-2.5, -0.3, (T, N)).astype(f), lambda a: rng.standard_normal((T, N)).astype(f),
        lambda a: (rng.random((T, N)) < 0.05).astype(f), lambda a: rng.standard_normal((T, N)).astype(f),
        lambda a: rng.standard_normal((N, DIMS[a][0])).astype(f), lambda a: (rng.random(N) < 0.05).astype(f)))

    # (c): each network's two halves as parameters of their own, with torch's Adam
    nets = {}
    for g, pop in agent.groups.items():
        ae = pop.spec.actor_end
        pa = torch.nn.Parameter(pop.params.data[0, :ae].clone())
        pc = torch.nn.Parameter(pop.params.data[0, ae:].clone())
        nets[g] = (pop.spec, pa, pc, torch.optim.Adam([pa], lr=agent.lr), torch.optim.Adam([pc], lr=agent.lr))

    def torch_learn():
        out = {}
        for g, (spec, pa, pc, oa, oc) in nets.items():
            members = agent._members(g)
            D = spec.obs_dim
            rows = lambda i, tail=(): torch.as_tensor(assemble_rows(exp[i], members, T, tail))  # noqa: E731
            with torch.no_grad():
                nobs = torch.as_tensor(assemble_rows(exp[6], members, None, (D,))).cuda()
                nv = spec.forward(torch.cat([pa, pc]).unsqueeze(0), nobs.unsqueeze(0))[1][0].cpu()
                v = rows(5)
                adv, ret = torch_gae(rows(3), rows(4), v, nv, torch.as_tensor(assemble_rows(exp[7], members, None)),
                                     agent.gamma, agent.gae_lambda)
            S = adv.numel()
            obs, act, lp = rows(0, (D,)).reshape(S, D).cuda(), rows(1).reshape(S).cuda(), rows(2).reshape(S).cuda()
            adv, ret, v = adv.reshape(S).cuda(), ret.reshape(S).cuda(), v.reshape(S).cuda()
            idx, mean_loss = np.arange(S), 0.0
            for _ in range(EPOCHS):
                np.random.shuffle(idx)
                for s in range(0, S, BATCH):
                    mb = torch.as_tensor(idx[s:s + BATCH]).cuda()
                    logits, value = spec.forward(torch.cat([pa, pc]).unsqueeze(0), obs[mb].unsqueeze(0))
                    logp_all, ent = categorical(logits[0])
                    logratio = logp_all.gather(-1, act[mb].unsqueeze(-1)).squeeze(-1) - lp[mb]
                    ratio = logratio.exp()
                    a = adv[mb]
                    a = (a - a.mean()) / (a.std() + 1e-8)
                    pg = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - agent.clip_coef, 1 + agent.clip_coef)).mean()
                    val = value[0]
                    vc = v[mb] + torch.clamp(val - v[mb], -agent.clip_coef, agent.clip_coef)
                    v_loss = 0.5 * torch.max((val - ret[mb]) ** 2, (vc - ret[mb]) ** 2).mean()
                    actor_loss, critic_loss = pg - agent.ent_coef * ent.mean(), v_loss * agent.vf_coef
                    oa.zero_grad()
                    actor_loss.backward()
                    torch.nn.utils.clip_grad_norm_([pa], agent.max_grad_norm)
                    oa.step()
                    oc.zero_grad()
                    critic_loss.backward()
                    torch.nn.utils.clip_grad_norm_([pc], agent.max_grad_norm)
                    oc.step()
                    mean_loss += actor_loss.item() + critic_loss.item()
            out[g] = mean_loss / (S * EPOCHS)
        return out

    def with_env(value, fn):
        def run():
            old = os.environ.get("AGX_IPPO_FUSED")
            os.environ["AGX_IPPO_FUSED"] = value
            try:
                return fn()
            finally:
                os.environ.pop("AGX_IPPO_FUSED") if old is None else os.environ.__setitem__("AGX_IPPO_FUSED", old)
        return run

    paths = {"fused": with_env("1", lambda: agent.learn(exp)), "loop": with_env("0", lambda: agent.learn(exp)),
             "torch": torch_learn}
    return agent, exp, paths, T


def main(out_path):
    import numpy as np
    import torch

    from agilerl_amd import kernels as K

    agent, exp, paths, T = setup()
    out = {"device": torch.cuda.get_device_name(0), "calls_per_block": CALLS, "blocks": ROUNDS,
           "shape": {"envs": N, "T": T, "batch": BATCH, "epochs": EPOCHS, "rows": {"speaker": T * N, "listener": 2 * T * N}}}
    for fn in paths.values():
        for _ in range(WARMUP):
            fn()
    assert set(agent.last_learn_paths.values()) == {"loop"}
    paths["fused"]()
    assert set(agent.last_learn_paths.values()) == {"fused"}
    torch.cuda.synchronize()
    ms = {name: [] for name in paths}
    for _ in range(ROUNDS):
        for name, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / CALLS)
    for name, v in ms.items():
        v.sort()
        out[f"learn_{name}_ms"] = round(v[len(v) // 2], 3)
        out[f"learn_{name}_ms_min_max"] = [round(v[0], 3), round(v[-1], 3)]
    out["learn_torch_over_fused"] = round(out["learn_torch_ms"] / out["learn_fused_ms"], 2)
    out["learn_loop_over_fused"] = round(out["learn_loop_ms"] / out["learn_fused_ms"], 2)

    # the GAE alone: both groups in one launch against the T-step torch loop on the CPU
    pops = list(agent.groups.values())
    segs = [(p.rewards[0], p.dones_f[0], p.values[0], p.next_value, p.next_done, p.advantages[0], p.returns[0])
            for p in pops]
    host = [tuple(t.cpu() for t in s[:5]) for s in segs]
    for _ in range(10):
        K.ippo_gae(segs, agent.gamma, agent.gae_lambda)
    dev_us, cpu_us = [], []
    for _ in range(ROUNDS):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(100):
            K.ippo_gae(segs, agent.gamma, agent.gae_lambda)
        end.record()
        end.synchronize()
        dev_us.append(start.elapsed_time(end) * 10)
        t0 = time.perf_counter()
        for _ in range(10):
            for h in host:
                torch_gae(*h, agent.gamma, agent.gae_lambda)
        cpu_us.append((time.perf_counter() - t0) * 1e5)
    for name, v in (("gae_agx_us", dev_us), ("gae_torch_cpu_us", cpu_us)):
        v.sort()
        out[name] = round(v[len(v) // 2], 2)
        out[name + "_min_max"] = [round(v[0], 2), round(v[-1], 2)]
    for s, h in zip(segs, host):  # the same bits
        adv, ret = torch_gae(*h, agent.gamma, agent.gae_lambda)
        assert torch.equal(adv, s[5].cpu()) and torch.equal(ret, s[6].cpu())
    out["gae_bit_equal_to_torch_loop"] = True
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else
         os.path.join(ROOT, "profiles", "ippo_time.json"))
