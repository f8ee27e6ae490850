"""The fused recurrent policy step (csrc/recurrent_policy.hip) against the same modules in float64 on the CPU.

Error measure and bound as tests/test_lstm_gpu.py: max |a - ref| / max |ref| per tensor, at most 4 x the float32
CPU modules' own error against float64 on the same inputs, + 8 * 2^-23.  The largest ratios seen per case are in
DESIGN 4.15."""

import copy

import numpy as np
import pytest
import torch

from agilerl_amd import kernels as K
from agilerl_amd.algorithms.ppo import PPO
from agilerl_amd.envs import Box, Discrete, SyntheticVecEnv
from agilerl_amd.modules.lstm import lstm_sequence
from agilerl_amd.networks.actors import StochasticActor
from agilerl_amd.networks.base import mlp_net_config
from agilerl_amd.networks.value_networks import ValueNetwork
from agilerl_amd.population.nets import categorical, gaussian
from tests.gauss_twin import gauss_eps
from tests.multidisc_twin import gumbel_scores

pytestmark = pytest.mark.gpu

# (N, in, H, L, latent, actor head, A, kind): the issue's table
CASES = [(1, 3, 16, 1, 8, [16], 2, "discrete"), (17, 5, 48, 2, 32, [32], 5, "discrete+mask"),
         (16, 8, 64, 1, 32, [64, 64], 32, "discrete"), (33, 20, 128, 3, 128, [32], 6, "box"),
         (4, 9, 80, 1, 24, [16], 1, "box"), (4, 4, 512, 1, 32, [32], 3, "discrete")]
FLOOR = 8 * 2.0 ** -23
# the Philox key of every sampled launch here.  On the CPU, over counters 1..8 of cases 2 and 3, the float64
# reference's top-two Gumbel score gap stays above 1e-4 on all 136 + 128 rows with this seed (cap: 2 %).
SEED = 0x5EED5EED1234
KEYS = ("actor_encoder_h", "actor_encoder_c", "critic_encoder_h", "critic_encoder_c")


def _build(case, out_act="ReLU"):
    """(actor, critic) built on the CPU from a fixed seed (so the weights do not depend on the device) with
    every bias, LayerNorm affine and log_std moved off its initial value; obs, hidden states and mask."""
    N, n_in, H, L, latent, head, A, kind = case
    torch.manual_seed(1000 * case[0] + case[2])
    obs_space = Box(-np.inf, np.inf, (n_in,))
    act_space = Box(-1.0, 1.0, (A,)) if kind == "box" else Discrete(A)
    enc = {"hidden_state_size": H, "num_layers": L, "output_activation": out_act}
    actor = StochasticActor(obs_space, act_space, encoder_config=dict(enc), latent_dim=latent, max_latent_dim=128,
                            head_config=mlp_net_config(head, output_vanish=False), recurrent=True,
                            encoder_name="actor_encoder")
    critic = ValueNetwork(obs_space, encoder_config=dict(enc), latent_dim=latent, max_latent_dim=128,
                          head_config=mlp_net_config([16]), recurrent=True, encoder_name="critic_encoder")
    with torch.no_grad():
        for p in (*actor.parameters(), *critic.parameters()):
            if p.dim() == 1 or p.shape[0] == 1:
                p.add_(0.2 * torch.randn_like(p))
    obs = torch.randn(N, n_in)
    hidden = {k: 0.5 * torch.randn(L, N, H) for k in KEYS}
    mask = None
    if kind == "discrete+mask":
        mask = (torch.rand(N, A) > 0.4).to(torch.uint8)
        mask[:, 1] = 1
    return actor, critic, obs, hidden, mask


def _reference(actor, critic, obs, hidden, mask, dtype):
    """The modules on the CPU in ``dtype`` -> dict of float64 tensors: (masked) logits or means, entropy, value,
    the next states, log_std."""
    a, c = (copy.deepcopy(n).to("cpu", dtype) for n in (actor, critic))
    hid = {k: v.to(dtype) for k, v in hidden.items()}
    with torch.no_grad():
        latent, nh = a.extract_features(obs.to(dtype), hidden_state={k: hid[k] for k in KEYS[:2]})
        _, _, entropy = a.forward_head(latent, action_mask=mask, sample=False)
        value, nc = c(obs.to(dtype), hidden_state={k: hid[k] for k in KEYS[2:]})
    out = {"logits": a.head_net.logits, "entropy": entropy, "values": value.squeeze(-1), **nh, **nc}
    if not a.head_net.discrete:
        out["log_std"] = a.head_net.log_std.detach()
    return {k: v.double() for k, v in out.items()}


def _logp(ref, action):
    if "log_std" in ref:
        return gaussian(ref["logits"], ref["log_std"], action.double())[0]
    return categorical(ref["logits"])[0].gather(-1, action.long().reshape(-1, 1)).squeeze(-1)


def _cuda(actor, critic, obs, hidden, mask):
    return (actor.to("cuda"), critic.to("cuda"), obs.cuda(), {k: v.cuda() for k, v in hidden.items()},
            None if mask is None else mask.cuda())


def _flat(res):
    """Every output of a launch, in a fixed order."""
    return [res[k] for k in ("actions", "log_probs", "entropy", "values") if res[k] is not None] + \
        [res["hidden"][k] for k in KEYS]


def _err(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.fixture(scope="module", params=CASES, ids=str)
def built(request):
    """Per case: the CPU build, both references, the device copies and one sampled launch (never modified)."""
    parts = _build(request.param)
    ref, base = _reference(*parts, torch.float64), _reference(*parts, torch.float32)
    dev = _cuda(*parts)
    res = K.ppo_act_recurrent(*dev[:4], mask=dev[4], seed=SEED, counter=1)
    assert res is not None
    return request.param, dev, ref, base, res


def test_parity(built):
    case, _, ref, base, res = built
    action = res["actions"].cpu()
    action = action if "log_std" in ref else action[:, 0]
    pairs = [("log_probs", res["log_probs"], _logp(base, action), _logp(ref, action))]
    pairs += [(k, res[k], base[k], ref[k]) for k in ("entropy", "values")]
    pairs += [(k, res["hidden"][k], base[k], ref[k]) for k in KEYS]
    worst = []
    for name, got, b, r in pairs:
        e, e32 = _err(got, r), _err(b, r)
        print(f"{case} {name}: fused {e:.3e} cpu32 {e32:.3e} ratio {e / max(e32, 2.0 ** -24):.2f}")
        if e > 4 * e32 + FLOOR:
            worst.append((name, e, e32))
    assert not worst, worst


def test_state_bits(built):
    _, (actor, critic, obs, hidden, mask), _, _, res = built
    with torch.no_grad():
        for net, name in ((actor, "actor_encoder"), (critic, "critic_encoder")):
            _, h_n, c_n = lstm_sequence(net.encoder, obs[:, None, :].contiguous(), hidden[f"{name}_h"],
                                        hidden[f"{name}_c"])
            assert torch.equal(res["hidden"][f"{name}_h"], h_n) and torch.equal(res["hidden"][f"{name}_c"], c_n)
    again = K.ppo_act_recurrent(actor, critic, obs, hidden, mask=mask, seed=SEED, counter=1)
    assert all(torch.equal(u, v) for u, v in zip(_flat(res), _flat(again)))


def test_sampling_follows_the_streams(built):
    case, (actor, critic, obs, hidden, mask), ref, base, res = built
    N, A = case[0], case[6]
    if case[7] == "box":
        eps = torch.from_numpy(gauss_eps(np.arange(N)[:, None], np.arange(A)[None, :], SEED, 1))
        want, want32 = (r["logits"] + torch.exp(r["log_std"]) * eps for r in (ref, base))
        assert _err(res["actions"], want) <= 4 * _err(want32, want) + FLOOR
    elif case in (CASES[1], CASES[2]):
        close = 0
        for counter in range(1, 9):
            got = K.ppo_act_recurrent(actor, critic, obs, hidden, mask=mask, seed=SEED, counter=counter)
            scores = np.sort(gumbel_scores(ref["logits"].numpy()[None], SEED, counter)[0], axis=-1)
            sure = scores[:, -1] - scores[:, -2] > 1e-4
            close += int((~sure).sum())
            want = gumbel_scores(ref["logits"].numpy()[None], SEED, counter)[0].argmax(-1)
            assert np.array_equal(got["actions"][:, 0].cpu().numpy()[sure], want[sure].astype(np.float32))
        assert close <= 0.02 * 8 * N
    other = K.ppo_act_recurrent(actor, critic, obs, hidden, mask=mask, seed=SEED, counter=2)
    if N > 8:  # a handful of draws can coincide
        assert not torch.equal(other["actions"], res["actions"])
    quiet = K.ppo_act_recurrent(actor, critic, obs, hidden, mask=mask, sample=False, seed=SEED, counter=1)
    assert quiet["actions"] is None and quiet["log_probs"] is None
    assert all(torch.equal(u, v) for u, v in zip(_flat(quiet), _flat(res)[2:]))


def test_reset_rows(built):
    case, (actor, critic, obs, hidden, mask), _, _, res = built
    N, L, H = case[0], case[3], case[2]
    flags = torch.arange(N) % 3 == 0
    store = {k: torch.full((N, L, H), 7.0, device="cuda") for k in KEYS}
    got = K.ppo_act_recurrent(actor, critic, obs, hidden, mask=mask, seed=SEED, counter=1, reset=flags,
                              store_hidden=store, store_obs=(kept := torch.empty_like(obs)))
    zeroed = {k: v.clone() for k, v in hidden.items()}
    for v in zeroed.values():
        v[:, flags.cuda()] = 0
    want = K.ppo_act_recurrent(actor, critic, obs, zeroed, mask=mask, seed=SEED, counter=1)
    assert all(torch.equal(u, v) for u, v in zip(_flat(got), _flat(want)))
    keep = ~flags.cuda()
    assert all(torch.equal(u[..., keep, :] if u.dim() == 3 else u[keep], v[..., keep, :] if v.dim() == 3 else v[keep])
               for u, v in zip(_flat(got), _flat(res)))
    assert all(torch.equal(store[k], zeroed[k].permute(1, 0, 2)) for k in KEYS) and torch.equal(kept, obs)


def _agent(action_space, hidden_size=16, **kw):
    torch.manual_seed(0)
    agent = PPO(Box(-np.inf, np.inf, (4,)), action_space, recurrent=True, share_encoders=False, num_envs=3,
                learn_step=36, net_config={"encoder_config": {"hidden_state_size": hidden_size, "num_layers": 2}},
                **kw)
    agent._act_seed = SEED
    return agent


@pytest.mark.parametrize("action_dim", [None, 2], ids=["discrete", "box"])
def test_rollout_writes_the_slot(action_dim, monkeypatch):
    from agilerl_amd.rollouts import collect_rollouts_recurrent

    bufs = []
    for direct in (True, False):  # the launch writes the slot; get_action + buf.add from the same seed and counters
        env = SyntheticVecEnv(3, obs_dim=4, n_actions=3, p_done=0.3, seed=1, action_dim=action_dim)
        agent = _agent(env.single_action_space, fused_step=True)
        if not direct:
            monkeypatch.setattr(agent.rollout_buffer, "fused_step", lambda *a, **k: None)
        collect_rollouts_recurrent(agent, env)
        assert agent._act_counter == 12
        bufs.append(agent.rollout_buffer.buffer)
    for k in ("actions", "log_probs", "values", "observations", "rewards", "dones", "advantages"):
        assert torch.equal(bufs[0][k], bufs[1][k]), k
    after_done = bufs[0]["dones"][:-1].cpu()
    assert after_done.any()
    for k in KEYS:
        assert torch.equal(bufs[0]["hidden_states"][k], bufs[1]["hidden_states"][k])
        stored = bufs[0]["hidden_states"][k][1:].cpu()
        assert not stored[after_done].any() and stored[~after_done].any()


def test_fallbacks_and_switch(monkeypatch):
    monkeypatch.delenv("AGX_RECURRENT_STEP", raising=False)
    ok = _cuda(*_build(CASES[0]))
    assert K.ppo_act_recurrent(*ok[:4]) is not None
    ok[0].encoder.lstm.register_forward_hook(lambda *_: None)
    assert K.ppo_act_recurrent(*ok[:4]) is None
    assert K.ppo_act_recurrent(*_cuda(*_build((2, 3, 24, 1, 8, [16], 2, "discrete")))[:4]) is None
    assert K.ppo_act_recurrent(*_cuda(*_build(CASES[0], out_act="Sigmoid"))[:4]) is None
    obs = np.zeros((3, 4), np.float32)
    odd = _agent(Discrete(3), hidden_size=24, fused_step=True)  # H = 24: the torch modules act
    out = odd.get_action(obs, hidden_state=odd.get_initial_hidden_state(3))
    assert out[0].shape == out[3].shape == (3,) and odd._act_counter == 0

    def boom(*a, **k):
        raise AssertionError("the fused step is off by default")

    plain = _agent(Discrete(3))
    monkeypatch.setattr(K, "ppo_act_recurrent", boom)
    assert plain.get_action(obs, hidden_state=plain.get_initial_hidden_state(3))[0].shape == (3,)
    monkeypatch.setenv("AGX_RECURRENT_STEP", "0")
    forced = _agent(Discrete(3), fused_step=True)
    assert forced.get_action(obs, hidden_state=forced.get_initial_hidden_state(3))[0].shape == (3,)


def test_train_on_policy_fused(monkeypatch):
    from agilerl_amd.training.train_on_policy import train_on_policy
    from agilerl_amd.utils import create_population

    monkeypatch.setenv("AGX_RECURRENT_STEP", "1")
    env = SyntheticVecEnv(3, obs_dim=4, n_actions=3, p_done=0.3, seed=2)
    init_hp = dict(RECURRENT=True, SHARE_ENCODERS=False, MAX_SEQ_LEN=4, LEARN_STEP=12, BATCH_SIZE=2, UPDATE_EPOCHS=1)
    pop = create_population("PPO", {"encoder_config": {"hidden_state_size": 16, "num_layers": 1}}, init_hp,
                            env.single_observation_space, env.single_action_space, population_size=2, num_envs=3)
    pop, fitnesses = train_on_policy(env, "synthetic", "PPO", pop, max_steps=24, evo_steps=12, eval_steps=8,
                                     eval_loop=1, verbose=False)
    assert len(fitnesses) == 2 and np.isfinite(fitnesses).all() and all(a._act_counter > 0 for a in pop)
