"""The shared-encoder fused policy step (agx_ppo_act_recurrent_shared, csrc/recurrent_policy.hip) against the same
modules in float64 on the CPU, and bit for bit against the separate-encoder step on a critic whose encoder is a copy
of the actor's.

Error measure and bound as tests/test_lstm_gpu.py: max |a - ref| / max |ref| per tensor, at most 4 x the float32
CPU modules' own error against float64 on the same inputs, + 8 * 2^-23.  The largest ratios seen are in DESIGN 4.17."""

import copy

import numpy as np
import pytest
import torch

from agilerl_amd import kernels as K
from agilerl_amd.envs import Box, Discrete, MultiBinary, MultiDiscrete
from agilerl_amd.networks.actors import StochasticActor
from agilerl_amd.networks.base import mlp_net_config
from agilerl_amd.networks.value_networks import ValueNetwork

pytestmark = pytest.mark.gpu

# (N, in, H, L, latent, (actor head, its LayerNorm), (critic head, its LayerNorm), space, mask, output activation):
# the issue's table.  Every case also resets its first and last row (case 2: rows 0 and 16).
CASES = [(1, 3, 16, 1, 8, ([16], False), ([16], False), Discrete(2), False, "ReLU"),
         (17, 4, 48, 2, 24, ([32], True), ([16], False), Discrete(5), True, "ReLU"),
         (5, 8, 64, 1, 32, ([64, 64], False), ([16], False), Box(-1.0, 1.0, (6,)), False, "Tanh"),
         (33, 4, 32, 1, 16, ([16], False), ([24], True), MultiDiscrete([5, 13, 14]), True, "ReLU"),
         (3, 4, 16, 1, 16, ([16], False), ([16], False), MultiBinary(17), False, "ReLU"),
         (2, 4, 512, 1, 512, ([512], False), ([16], False), Discrete(3), False, "ReLU")]
FLOOR = 8 * 2.0 ** -23
SEED = 0x5EED5EED1234
KEYS = ("shared_encoder_h", "shared_encoder_c")
OUT = ("actions", "log_probs", "entropy", "values")


def shared_pair(n_in, H, L, latent, ahead, chead, space, out_act, seed):
    """(actor, critic, twin) on the CPU from a fixed seed: both networks on ``shared_encoder`` with every bias,
    LayerNorm affine and log_std moved off its initial value; ``twin`` is the critic on a ``critic_encoder`` of its
    own that is a copy of the actor's, for the separate-encoder kernels."""
    torch.manual_seed(seed)
    obs_space = Box(-np.inf, np.inf, (n_in,))
    enc = {"hidden_state_size": H, "num_layers": L, "output_activation": out_act}
    actor = StochasticActor(obs_space, space, encoder_config=dict(enc), latent_dim=latent, max_latent_dim=512,
                            head_config=mlp_net_config(ahead[0], layer_norm=ahead[1], output_vanish=False),
                            recurrent=True, encoder_name="shared_encoder")
    kw = dict(encoder_config=dict(enc), latent_dim=latent, max_latent_dim=512, recurrent=True,
              head_config=mlp_net_config(chead[0], layer_norm=chead[1]))
    critic = ValueNetwork(obs_space, encoder_name="shared_encoder", **kw)
    twin = ValueNetwork(obs_space, encoder_name="critic_encoder", **kw)
    with torch.no_grad():
        for p in (*actor.parameters(), *critic.head_net.parameters()):
            if p.dim() == 1 or p.shape[0] == 1:
                p.add_(0.2 * torch.randn_like(p))
    twin.encoder.load_state_dict({k.replace("shared", "critic"): v for k, v in actor.encoder.state_dict().items()})
    twin.head_net.load_state_dict(critic.head_net.state_dict())
    return actor, critic, twin


def legal_mask(space, rows):
    """A random mask [rows, A] with a legal logit in every component."""
    nvec = space.nvec if hasattr(space, "nvec") else [space.n]
    mask = torch.rand(rows, int(np.sum(nvec))) > 0.4
    mask[:, np.cumsum([0, *nvec[:-1]])] = True
    return mask


def _reference(actor, critic, obs, hidden, mask, action, dtype):
    """The shared branch of the reference's ``_get_action_and_values`` on the CPU in ``dtype`` -> float64 tensors."""
    a, c = (copy.deepcopy(n).to("cpu", dtype) for n in (actor, critic))
    with torch.no_grad():
        latent, nxt = a.extract_features(obs.to(dtype), hidden_state={k: v.to(dtype) for k, v in hidden.items()})
        _, _, entropy = a.forward_head(latent, action_mask=mask, sample=False)
        logp = a.action_log_prob(action[:, 0] if isinstance(a.action_space, Discrete) else action.to(dtype))
        out = {"log_probs": logp, "entropy": entropy, "values": c.forward_head(latent).squeeze(-1), **nxt}
    return {k: v.double() for k, v in out.items()}


def _flat(res, keys=KEYS):
    return [res[k] for k in OUT if res[k] is not None] + [res["hidden"][k] for k in keys]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: str(c[:5]))
def built(request):
    """Per case: the device copies, the inputs and one sampled launch (never modified)."""
    N, n_in, H, L, latent, ahead, chead, space, masked, out_act = request.param
    nets = shared_pair(n_in, H, L, latent, ahead, chead, space, out_act, 1000 * N + H)
    obs, hidden = torch.randn(N, n_in), {k: 0.5 * torch.randn(L, N, H) for k in KEYS}
    mask = legal_mask(space, N) if masked else None
    host = (obs, hidden, mask)
    dev = ([n.to("cuda") for n in nets], obs.cuda(), {k: v.cuda() for k, v in hidden.items()},
           None if mask is None else mask.cuda())
    res = K.ppo_act_recurrent(*dev[0][:2], dev[1], dev[2], mask=dev[3], seed=SEED, counter=1)
    assert res is not None and set(res["hidden"]) == set(KEYS)
    return request.param, host, dev, res


def test_parity(built):
    case, (obs, hidden, mask), ((actor, critic, _), *_), res = built
    ref, base = (_reference(actor, critic, obs, hidden, mask, res["actions"].cpu(), d)
                 for d in (torch.float64, torch.float32))
    bad = []
    for name in ref:
        got = res[name] if name in res else res["hidden"][name]
        e, e32 = (float((t.double().cpu() - ref[name]).abs().max() / ref[name].abs().max()) for t in (got, base[name]))
        print(f"{case[:5]} {name}: fused {e:.3e} cpu32 {e32:.3e} ratio {e / max(e32, 2.0 ** -24):.2f}")
        if not e <= 4 * e32 + FLOOR:
            bad.append((name, e, e32))
    assert not bad, bad


def test_bits_of_the_separate_step(built):
    _, _, ((actor, critic, twin), obs, hidden, mask), res = built
    both = {**hidden, "critic_encoder_h": hidden[KEYS[0]], "critic_encoder_c": hidden[KEYS[1]]}
    want = K.ppo_act_recurrent(actor, twin, obs, both, mask=mask, seed=SEED, counter=1)
    assert set(want["hidden"]) == set(both)
    assert all(torch.equal(u, v) for u, v in zip(_flat(res), _flat(want)))
    quiet = K.ppo_act_recurrent(actor, critic, obs, hidden, mask=mask, sample=False, seed=SEED, counter=1)
    assert quiet["actions"] is None and quiet["log_probs"] is None
    assert all(torch.equal(u, v) for u, v in zip(_flat(quiet), _flat(res)[2:]))


def test_reset_rows(built):
    case, _, ((actor, critic, _), obs, hidden, mask), res = built
    N, L, H = case[0], case[3], case[2]
    flags = torch.zeros(N, dtype=torch.bool)
    flags[[0, N - 1]] = True
    store = {k: torch.full((N, L, H), 7.0, device="cuda") for k in KEYS}
    got = K.ppo_act_recurrent(actor, critic, obs, hidden, mask=mask, seed=SEED, counter=1, reset=flags,
                              store_hidden=store, store_obs=(kept := torch.empty_like(obs)))
    zeroed = {k: v.clone() for k, v in hidden.items()}
    for v in zeroed.values():
        v[:, flags.cuda()] = 0
    want = K.ppo_act_recurrent(actor, critic, obs, zeroed, mask=mask, seed=SEED, counter=1)
    assert all(torch.equal(u, v) for u, v in zip(_flat(got), _flat(want)))
    assert all(torch.equal(store[k], zeroed[k].permute(1, 0, 2)) for k in KEYS) and torch.equal(kept, obs)
    keep = ~flags.cuda()
    assert all(torch.equal(u[..., keep, :] if u.dim() == 3 else u[keep], v[..., keep, :] if v.dim() == 3 else v[keep])
               for u, v in zip(_flat(got), _flat(res)))
