"""The multi-categorical and Bernoulli heads of recurrent PPO's fused policy step (csrc/recurrent_policy.hip) and
learner head kernels (csrc/recurrent_heads.hip) against the same modules in float64 on the CPU.  Error measure and
bound as tests/test_lstm_gpu.py: max |a - ref| / max |ref| per tensor, at most 4 x the float32 CPU modules' own
error + 8 * 2^-23.  The largest ratios seen are in DESIGN 4.15 / 4.16."""

import numpy as np
import pytest
import torch

from agilerl_amd import kernels as K
from agilerl_amd.algorithms.ppo import PPO
from agilerl_amd.envs import Box, Discrete, MultiBinary, MultiDiscrete, SyntheticVecEnv
from agilerl_amd.modules.lstm import lstm_sequence
from agilerl_amd.networks.actors import StochasticActor
from agilerl_amd.networks.base import mlp_net_config
from agilerl_amd.networks.value_networks import ValueNetwork
from agilerl_amd.population.nets import bernoulli_head, multi_categorical
from tests import multibinary_twin as mb
from tests import multidisc_twin as md
from tests import test_recurrent_heads_gpu as heads
from tests import test_recurrent_step_gpu as step

pytestmark = pytest.mark.gpu

# (nvec or the number of bits, mask, N of the step, R of the heads, in, H, L, latent, actor head).  The masks make
# one logit (flat index 7 / 3) illegal in every row.
CASES = [((4,), False, 17, 15, 5, 48, 2, 32, [32]), ((1, 3), False, 1, 1, 3, 16, 1, 8, [16]),
         ((5, 13, 14), True, 33, 33, 8, 64, 1, 32, [64, 64]), ((2,) * 16, False, 17, 15, 4, 32, 1, 16, [32]),
         (1, False, 1, 1, 3, 16, 1, 8, [16]), (17, True, 33, 33, 5, 48, 2, 32, [32]), (32, False, 17, 15, 4, 32, 1, 16, [32])]
# On the CPU, over counters 1..8 of all seven cases, the float64 reference alone leaves out no (row, component,
# counter) triple (gap 1e-4) and no bit (|u - p| 1e-5) with this Philox key (cap: 2 %).
SEED = step.SEED
ZERO = (5, 6, 7, 20)  # heads rows with zero upstream gradients (R = 33)


def _build(case):
    """Networks on the CPU from a fixed seed; the step's (obs, hidden, mask); the heads' (h_top, actions, mask, ups)."""
    spec, masked, N, R, n_in, H, L, latent, head = case
    multi = isinstance(spec, tuple)
    A = sum(spec) if multi else spec
    torch.manual_seed(100 * A + N)
    rng = np.random.default_rng(A)
    obs_space, space = Box(-np.inf, np.inf, (n_in,)), MultiDiscrete(spec) if multi else MultiBinary(spec)
    enc = {"hidden_state_size": H, "num_layers": L, "output_activation": "ReLU"}
    actor = StochasticActor(obs_space, space, encoder_config=dict(enc), latent_dim=latent, max_latent_dim=128,
                            head_config=mlp_net_config(head, output_vanish=False), recurrent=True,
                            encoder_name="actor_encoder")
    critic = ValueNetwork(obs_space, encoder_config=dict(enc), latent_dim=latent, max_latent_dim=128,
                          head_config=mlp_net_config([16]), recurrent=True, encoder_name="critic_encoder")
    with torch.no_grad():
        for p in (*actor.parameters(), *critic.parameters()):
            if p.dim() == 1:
                p.add_(0.2 * torch.randn_like(p))
    if multi:
        actions = np.stack([rng.integers(0, n, R) for n in spec], -1)
        if masked:
            actions[actions[:, 1] == 2, 1] = 3  # flat index 7 is never taken
        masks = [md.random_mask(rng, N, spec), md.random_mask(rng, R, spec, keep=actions)]
    else:
        actions = rng.integers(0, 2, (R, A))
        if masked:
            actions[:, 3] = 0
        masks = [mb.random_mask(rng, N, A), mb.random_mask(rng, R, A, keep=actions)]
    for m in masks if masked else ():
        m[:, 7 if multi else 3] = 0
    masks = [torch.from_numpy(m) if masked else None for m in masks]
    ups = [torch.randn(R) for _ in range(3)]
    for u in ups:
        u[[z for z in ZERO if z < R]] = 0
    stepped = (torch.randn(N, n_in), {k: 0.5 * torch.randn(L, N, H) for k in step.KEYS}, masks[0])
    learned = ([0.5 * torch.randn(R, H), 0.5 * torch.randn(R, H)], torch.from_numpy(actions).float(), masks[1], ups)
    return (actor, critic), stepped, learned


def _to(dev, x):
    if isinstance(x, (list, tuple)):
        return [_to(dev, t) for t in x]
    return {k: v.to(dev) for k, v in x.items()} if isinstance(x, dict) else None if x is None else x.to(dev)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}")
def built(request):
    """Per case: float64 and float32 CPU references of the step and the heads, one launch of each (never modified)."""
    case = request.param
    nets, stepped, learned = _build(case)
    refs = [step._reference(*nets, *stepped, d) for d in (torch.float64, torch.float32)]
    cpu, nets = learned, _to("cuda", nets)
    names = heads._names(*nets)
    hrefs = [heads._reference(nets, *cpu, names, d) for d in (torch.float64, torch.float32)]
    stepped, learned = _to("cuda", stepped), _to("cuda", learned)
    res = K.ppo_act_recurrent(*nets, *stepped[:2], mask=stepped[2], seed=SEED, counter=1)
    return case, nets, stepped, refs, res, learned, names, hrefs, heads._launch(nets, *learned)


def test_step_parity_and_bits(built):
    case, (actor, critic), (obs, hidden, mask), (ref, base), res = built[:5]
    action = res["actions"].cpu()
    logp = (lambda lg: multi_categorical(lg, list(case[0]), action.long())[0]) if isinstance(case[0], tuple) else \
        (lambda lg: bernoulli_head(lg, action)[0])
    pairs = [("log_probs", res["log_probs"], logp(base["logits"]), logp(ref["logits"]))]
    pairs += [(k, res[k], base[k], ref[k]) for k in ("entropy", "values")]
    for name, got, b, r in pairs:
        e, e32 = step._err(got, r), step._err(b, r)
        print(f"{case[0]} {name}: fused {e:.3e} cpu32 {e32:.3e} ratio {e / max(e32, 2.0 ** -24):.2f}")
        assert e <= 4 * e32 + step.FLOOR, name
    with torch.no_grad():
        for net, name in ((actor, "actor_encoder"), (critic, "critic_encoder")):
            _, h_n, c_n = lstm_sequence(net.encoder, obs[:, None, :].contiguous(), hidden[f"{name}_h"],
                                        hidden[f"{name}_c"])
            assert torch.equal(res["hidden"][f"{name}_h"], h_n) and torch.equal(res["hidden"][f"{name}_c"], c_n)
    again = K.ppo_act_recurrent(actor, critic, obs, hidden, mask=mask, seed=SEED, counter=1)
    quiet = K.ppo_act_recurrent(actor, critic, obs, hidden, mask=mask, sample=False, seed=SEED, counter=1)
    assert all(torch.equal(u, v) for u, v in zip(step._flat(res), step._flat(again)))
    assert quiet["actions"] is None and quiet["log_probs"] is None
    assert all(torch.equal(u, v) for u, v in zip(step._flat(quiet), step._flat(res)[2:]))


def test_step_sampling_follows_the_streams(built, monkeypatch):
    case, (actor, critic), (obs, hidden, mask), (ref, _), res = built[:5]
    spec, N, logits = case[0], case[2], ref["logits"].numpy()
    left_out = total = 0
    for counter in range(1, 9):
        got = K.ppo_act_recurrent(actor, critic, obs, hidden, mask=mask, seed=SEED, counter=counter)["actions"]
        if isinstance(spec, tuple):
            want, gap = md.choices(md.gumbel_scores(logits[None], SEED, counter)[0], spec)
            sure = gap > 1e-4
        else:
            want, gap = mb.choices(logits, mb.uniforms(1, N, spec, SEED, counter)[0])
            sure = gap > 1e-5
        assert np.array_equal(got.cpu().numpy()[sure], want[sure].astype(np.float32))
        left_out, total = left_out + int((~sure).sum()), total + sure.size
    assert left_out <= 0.02 * total
    if spec == (4,):  # one component: Discrete(4)'s choices on the same key
        monkeypatch.setattr(actor, "action_space", Discrete(4))  # the binding takes the head kind from the space
        want = K.ppo_act_recurrent(actor, critic, obs, hidden, seed=SEED, counter=1)
        assert torch.equal(res["actions"], want["actions"])


def test_heads_parity_and_bits(built):
    case, nets, learned, names, (ref, base), got = built[0], built[1], *built[5:]
    heads._check(case[:4], ["log_prob", "entropy", "value"], got[0], base[0], ref[0])
    heads._check(case[:4], ["dh_top actor", "dh_top critic", *names], got[1], base[1], ref[1])
    zero = [z for z in ZERO if z < case[3]]
    assert not got[1][0][zero].any() and not got[1][1][zero].any()
    if case[1]:  # the logit that is illegal in every row: its row of the last layer's dW and db is exactly 0
        col = 7 if isinstance(case[0], tuple) else 3
        last = [g for n, g in zip(names, got[1][2:]) if n.startswith("actor.head_net")][-2:]
        assert last[0].shape[0] == last[1].shape[0] and not last[0][col].any() and not last[1][col].any()
        assert last[0].any(dim=1).sum() == last[0].shape[0] - 1
    again = heads._launch(nets, *learned)
    assert all(torch.equal(u, v) for u, v in zip(got[0] + got[1], again[0] + again[1]))


@pytest.mark.parametrize("env_kw", [dict(nvec=[3, 3]), dict(n_binary=4)], ids=["multidiscrete", "multibinary"])
def test_agent_end_to_end(env_kw, monkeypatch):
    from agilerl_amd.rollouts import collect_rollouts_recurrent

    def agent_and_env(**kw):
        env = SyntheticVecEnv(3, obs_dim=4, p_done=0.3, seed=1, **env_kw)
        torch.manual_seed(0)
        agent = PPO(Box(-np.inf, np.inf, (4,)), env.single_action_space, recurrent=True, share_encoders=False,
                    num_envs=3, learn_step=36, max_seq_len=4, batch_size=3, update_epochs=1,
                    net_config={"encoder_config": {"hidden_state_size": 16, "num_layers": 2}}, **kw)
        agent._act_seed = SEED
        return agent, env

    for var in ("AGX_RECURRENT_STEP", "AGX_RECURRENT_LEARN"):
        monkeypatch.delenv(var, raising=False)
    bufs = []
    for direct in (True, False):  # the launch writes the slot; get_action + buf.add from the same key and counters
        agent, env = agent_and_env(fused_step=True, fused_learn=True)
        if not direct:
            monkeypatch.setattr(agent.rollout_buffer, "fused_step", lambda *a, **k: None)
        collect_rollouts_recurrent(agent, env)
        assert agent._act_counter == 12 and K.recurrent_heads_params(agent.actor, agent.critic) is not None
        bufs.append(agent.rollout_buffer.buffer)
        assert np.isfinite(agent.learn())
    for k in ("actions", "log_probs", "values", "advantages"):
        assert torch.equal(bufs[0][k], bufs[1][k]), k
    action = agent.get_action(np.zeros((3, 4), np.float32), hidden_state=agent.get_initial_hidden_state(3))[0]
    assert action.shape == (3, bufs[0]["actions"].shape[-1]) and action.dtype == env.single_action_space.dtype

    plain, env = agent_and_env()  # both switches off: neither kernel may be called
    monkeypatch.setattr(K, "ppo_act_recurrent", None)
    monkeypatch.setattr(K, "recurrent_heads_forward", None)
    collect_rollouts_recurrent(plain, env)
    assert np.isfinite(plain.learn())
