"""Recurrent PPO's truncated-BPTT data path and ``learn()`` on one GPU: T = 128 steps x N = 64 envs, obs 8,
Discrete(4), one LSTM layer of H = 64 per encoder, max_seq_len 16 (CHUNKED), 64 sequences per minibatch, 4 epochs.

  ``prepare``  prepare_sequence_tensors + one full pass of get_minibatch_sequences
      (a) ``agx``    agx_bptt_plan, one read-back, one agx_bptt_gather per minibatch;
      (b) ``torch``  a plain-torch restatement of rollout_buffer.py:676-922 on a CPU copy of the same buffer
                     (where the reference keeps it): the Python loops per env, episode and key, pad_sequence,
                     the padded and unpadded tensors moved to the GPU, Python index lists per minibatch;
  ``learn``    one learn() on the same buffer
      (a) ``agx``    PPO(recurrent=True).learn();
      (b) ``torch``  the restatement of ppo.py:923-1111 on a deep copy of the agent: (b)'s data path, three
                     masked index ops, the loss block and autograd's backward through them; same networks,
                     clips and Adam.

  python tools/bptt_time.py [--out profiles/bptt_time.json]
      warm-up, then ROUNDS alternating blocks of 100 (prepare) or 5 (learn) calls each, every call ended by a
      device synchronise; the median block per call is reported with the fastest and slowest.
      compute_returns_and_advantages (the
      GAE launch both learners need before each learn) is outside the timed span.  One JSON line, also
      written to --out.  Not measured: kernel times (no profiler run), other shapes, AGX_LSTM=1.

  python tools/bptt_time.py --heads [--out profiles/bptt_time.json]
      learn() on the same buffer with the fused heads (AGX_RECURRENT_LEARN) off, which is the path
      without them, and on, each with AGX_LSTM unset and AGX_LSTM=1: four settings of one agent in the same
      alternating blocks.  Added to --out under "learn_heads"; the file's other keys are kept.
  python tools/bptt_time.py --heads --space NAME [--out FILE]
      the same on another action space (SPACES: Discrete of 6 / 32 logits, MultiDiscrete([3, 3]) / ([2] * 16),
      MultiBinary(4) / (32)), under "learn_heads_NAME".
  python tools/bptt_time.py --heads --shared [--out profiles/bptt_time.json]
      the same four settings on a shared-encoder agent (``share_encoders=True``) and, for information,
      the two heads-on settings on a separate-encoder agent of the same shape in the same alternating blocks, under
      "learn_heads_shared".
"""
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, N, OBS, ACTIONS, H, MAX_SEQ_LEN, BATCH, EPOCHS = 128, 64, 8, 4, 64, 16, 64, 4
CALLS = {"prepare": int(os.environ.get("PREPARE_CALLS", 100)), "learn": int(os.environ.get("LEARN_CALLS", 5))}
ROUNDS = int(os.environ.get("ROUNDS", 5))


SPACES = {"discrete6": ("Discrete", 6), "multidiscrete3x3": ("MultiDiscrete", [3, 3]), "discrete32": ("Discrete", 32),
          "multidiscrete2x16": ("MultiDiscrete", [2] * 16), "multibinary4": ("MultiBinary", 4),
          "multibinary32": ("MultiBinary", 32)}


def setup(space=None, shared=False):
    import numpy as np
    import torch

    from agilerl_amd import envs
    from agilerl_amd.algorithms.ppo import PPO
    from agilerl_amd.envs import Box

    kind, arg = SPACES[space] if space else ("Discrete", ACTIONS)
    # the exclusive upper bounds of a step's random actions: [] (Discrete), [K] or [n]
    high = torch.tensor([2] * arg if kind == "MultiBinary" else arg)
    torch.manual_seed(0)
    agent = PPO(Box(-np.inf, np.inf, (OBS,)), getattr(envs, kind)(arg), recurrent=True, share_encoders=shared, num_envs=N,
                learn_step=T * N, max_seq_len=MAX_SEQ_LEN, batch_size=BATCH, update_epochs=EPOCHS,
                net_config={"encoder_config": {"hidden_state_size": H, "num_layers": 1}})
    buf, g = agent.rollout_buffer, torch.Generator().manual_seed(1)
    hidden = agent.get_initial_hidden_state(N)
    for _ in range(T):
        action = (torch.rand(N, *high.shape, generator=g) * high).long()
        buf.add(obs=torch.randn(N, OBS, generator=g), action=action,
                reward=torch.randn(N, generator=g), done=torch.rand(N, generator=g) < 0.03,
                value=torch.randn(N, generator=g), log_prob=-torch.rand(N, generator=g) - 0.5,
                hidden_state={k: 0.1 * torch.randn(v.shape, generator=g) for k, v in hidden.items()})
    return agent


def gae(agent):
    import torch

    agent.rollout_buffer.compute_returns_and_advantages(torch.zeros(N), torch.zeros(N))


def torch_prepare(host, max_seq_len, device):
    """rollout_buffer.py:722-843 on the CPU dict ``host`` -> (padded dict on ``device``, initial hidden states,
    unpadded dict on ``device``, unpadded_slices, S, L)."""
    import torch
    from torch.nn.utils.rnn import pad_sequence

    n_steps, n_envs = host["dones"].shape
    ends = []
    for env in range(n_envs):
        e = host["dones"][:, env].nonzero().squeeze(-1).tolist()
        if not e or e[-1] != n_steps - 1:
            e.append(n_steps - 1)
        ends.append(e)

    def sequences(data):
        out = []
        for env in range(n_envs):
            start = 0
            for end in ends[env]:
                ep = data[start:end + 1, env]
                if len(ep) >= max_seq_len:
                    out += [ep[c * max_seq_len:(c + 1) * max_seq_len] for c in range(max(1, len(ep) // max_seq_len))]
                else:
                    out.append(ep)
                start = end + 1
        return out

    slices = sequences(torch.arange(n_steps * n_envs).reshape(n_steps, n_envs))
    keys = {"observations": host["observations"], "actions": host["actions"],
            "pad_mask": torch.ones(n_steps, n_envs, dtype=torch.bool), **host["hidden_states"]}
    padded = {k: pad_sequence(sequences(v.clone()), batch_first=True) for k, v in keys.items()}
    S, L = padded["pad_mask"].shape
    initial = {k: padded.pop(k)[:, 0].clone().to(device) for k in host["hidden_states"]}
    padded = {k: v.flatten(0, 1).to(device) for k, v in padded.items()}
    unpadded = {k: host[k].flatten().to(device) for k in ("log_probs", "advantages", "values", "returns")}
    return padded, initial, unpadded, slices, S, L


def torch_minibatches(prep, batch):
    """rollout_buffer.py:845-922."""
    import torch

    padded, initial, unpadded, slices, S, L = prep
    indices, order = torch.arange(S * L).reshape(S, L), torch.randperm(S)
    for start in range(0, S, batch):
        ids = order[start:start + batch]
        rows = indices[ids].view(-1).to(unpadded["returns"].device)
        flat = torch.as_tensor([int(i) for j in ids.tolist() for i in slices[j].tolist()], device=rows.device)
        hidden = {k: v[ids.to(v.device)].clone().permute(1, 0, 2).contiguous() for k, v in initial.items()}
        yield {**{k: v[rows] for k, v in padded.items()}, "initial_hidden_states": hidden}, \
            {k: v[flat] for k, v in unpadded.items()}


def host_copy(agent):
    b = agent.rollout_buffer.buffer
    return {**{k: v.cpu() for k, v in b.items() if k != "hidden_states"},
            "hidden_states": {k: v.cpu() for k, v in b["hidden_states"].items()}}


def torch_learn(ref, host):
    """ppo.py:923-1111 (target_kl None) on the agent copy ``ref``."""
    import torch
    from torch.nn.utils import clip_grad_norm_

    adv = host["advantages"]
    host = {**host, "advantages": (adv - adv.mean()) / (adv.std() + 1e-8)}
    prep = torch_prepare(host, MAX_SEQ_LEN, ref.device)
    total, count = 0.0, 0
    for _ in range(EPOCHS):
        for p, u in torch_minibatches(prep, BATCH):
            logp, ent, value = ref.evaluate_actions(p["observations"], p["actions"].squeeze(-1),
                                                    hidden_state=p["initial_hidden_states"])
            m = p["pad_mask"]
            value, logp, ent = value[m], logp[m], ent[m].mean()
            ratio = torch.exp(logp - u["log_probs"])
            pg = torch.max(-u["advantages"] * ratio,
                           -u["advantages"] * torch.clamp(ratio, 1 - ref.clip_coef, 1 + ref.clip_coef)).mean()
            v_clip = u["values"] + torch.clamp(value - u["values"], -ref.clip_coef, ref.clip_coef)
            vl = torch.max((value - u["returns"]) ** 2, (v_clip - u["returns"]) ** 2).mean()
            loss = pg + ref.vf_coef * vl - ref.ent_coef * ent
            ref.optimizer.zero_grad()
            loss.backward()
            clip_grad_norm_(ref.actor.parameters(), ref.max_grad_norm)
            clip_grad_norm_(ref.critic.parameters(), ref.max_grad_norm)
            ref.optimizer.step()
            total, count = total + loss.item(), count + 1
    return total / count


def block(fn, before, calls):
    """Mean seconds per call of ``calls`` calls, each between two device synchronises; ``before`` is not timed."""
    import torch

    spans = []
    for _ in range(calls):
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        spans.append(time.perf_counter() - t0)
    return sum(spans) / len(spans)


def spread(v):
    return {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}


HEADS = {"heads off": (None, "0"), "heads on": (None, "1"), "AGX_LSTM=1, heads off": ("1", "0"),
         "AGX_LSTM=1, heads on": ("1", "1")}  # setting -> (AGX_LSTM, AGX_RECURRENT_LEARN)


def heads(out_path, space=None, shared=False):
    agents = dict.fromkeys(HEADS, setup(space, shared))
    if shared:
        sep = setup(space)
        agents.update({"separate encoders, " + s: sep for s in HEADS if s.endswith("heads on")})

    def learn(setting):
        agent = agents[setting]
        lstm, switch = HEADS[setting.replace("separate encoders, ", "")]
        os.environ.pop("AGX_LSTM", None)
        if lstm is not None:
            os.environ["AGX_LSTM"] = lstm
        os.environ["AGX_RECURRENT_LEARN"] = switch
        return block(agent.learn, lambda: gae(agent), CALLS["learn"])

    for setting in agents:  # warm-up of every setting
        learn(setting)
    times = {setting: [] for setting in agents}
    for _ in range(ROUNDS):  # alternating blocks
        for setting in agents:
            times[setting].append(1e3 * learn(setting))
    result = {}
    if out_path and os.path.exists(out_path):
        with open(out_path) as f:
            result = json.load(f)
    key = "learn_heads" + (f"_{space}" if space else "") + ("_shared" if shared else "")
    result[key] = {"unit": "ms per learn()", "calls_per_block": CALLS["learn"], "blocks": ROUNDS,
                             **{setting: spread(v) for setting, v in times.items()}}
    print(key, json.dumps(result[key]))
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if "--heads" in sys.argv:
        return heads(out_path, sys.argv[sys.argv.index("--space") + 1] if "--space" in sys.argv else None,
                     "--shared" in sys.argv)
    agent = setup()
    ref = copy.deepcopy(agent)
    ref.reinit_optimizers()
    gae(agent)
    host = host_copy(agent)
    buf = agent.rollout_buffer

    def agx_prepare():
        buf.prepare_sequence_tensors()
        for _ in buf.get_minibatch_sequences(BATCH):
            pass

    def ref_prepare():
        for _ in torch_minibatches(torch_prepare(host, MAX_SEQ_LEN, agent.device), BATCH):
            pass

    def agx_learn():
        agent.learn()

    def ref_learn():
        torch_learn(ref, host)

    pairs = {"prepare": ((agx_prepare, None), (ref_prepare, None)),
             "learn": ((agx_learn, lambda: gae(agent)), (ref_learn, None))}
    result = {"shape": dict(T=T, N=N, obs=OBS, actions=ACTIONS, H=H, layers=1, max_seq_len=MAX_SEQ_LEN,
                            batch_sequences=BATCH, epochs=EPOCHS),
              "sequences": None, "calls_per_block": CALLS, "blocks": ROUNDS, "unit": "ms per call"}
    for name, sides in pairs.items():
        for fn, before in sides:  # warm-up of both sides
            block(fn, before, min(CALLS[name], 5))
        times = {"agx": [], "torch": []}
        for _ in range(ROUNDS):  # alternating blocks
            for side, (fn, before) in zip(times, sides):
                times[side].append(1e3 * block(fn, before, CALLS[name]))
        result[name] = {s: spread(v) for s, v in times.items()}
    result["sequences"] = dict(S=buf.num_sequences, L=buf.max_sequence_length)
    result["not_measured"] = "kernel times (no profiler run), other shapes, AGX_LSTM=1"
    line = json.dumps(result)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
