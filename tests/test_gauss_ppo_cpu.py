"""PPO for Box action spaces without a GPU: the Gaussian spec's layout, the
float64 restatements of tests/gauss_twin.py pinned to the reference
(tests/golden/gauss_*.npz), the reference noise sequence the GPU tests select,
architecture mutations carrying log_std, and the refusals."""

import json
import os

import numpy as np
import pytest
import torch

from tests import gauss_twin as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _specs(A=6, **kw):
    from agilerl_amd.population.nets import ActorCriticSpec, GaussianActorCriticSpec

    shape = dict(obs_dim=8, encoder_hidden=[64, 64], latent_dim=32, actor_hidden=[32], critic_hidden=[16])
    return GaussianActorCriticSpec(n_actions=A, **shape, **kw), ActorCriticSpec(n_actions=A, **shape)


# ---- spec layout ---------------------------------------------------------------- #
def test_gaussian_spec_layout():
    g, d = _specs(6, action_std_init=0.5)
    out = g.actor[-1]
    out_end = out.b + out.fout
    for lg, ld in zip(g.encoder + g.actor, d.encoder + d.actor):  # equal up to the actor's output layer
        assert (lg.w, lg.b, lg.g, lg.beta) == (ld.w, ld.b, ld.g, ld.beta)
    assert out_end == d.actor_end
    assert g.log_std == out_end and g.actor_end == out_end + 6 and g.n_params == d.n_params + 6
    assert g.group_offsets == [0, g.actor_end, g.n_params]  # log_std is an actor parameter (ppo.py:910-911)
    assert [lg.w - ld.w for lg, ld in zip(g.critic, d.critic)] == [6] * len(d.critic)
    keys = g.state_dict_keys()
    assert keys["actor.head_net.log_std"] == (g.log_std, (1, 6))
    assert set(keys) - {"actor.head_net.log_std"} == set(d.state_dict_keys())
    # the reference's actor.parameters() order (tests/golden/META_gauss.json): log_std before head_net._wrapped.*
    names = [k for k in keys if k.startswith("actor.head_net.")]
    meta = json.load(open(os.path.join(GOLDEN, "META_gauss.json")))
    assert ["actor." + n for n in meta["actor_parameter_order"][1:]] == names
    assert g.shape_key() != d.shape_key() and g.shape_key() != _specs(6, action_std_init=0.25)[0].shape_key()
    mean, value = g.forward(g.init_params(2), torch.zeros(2, 3, 8))
    assert mean.shape == (2, 3, 6) and value.shape == (2, 3)


def test_gaussian_spec_keeps_the_discrete_initialisation():
    """The layers draw from the generator exactly as today: against a tensor
    built by the Discrete spec's init_params (the code path as it stands)."""
    g, d = _specs(6, action_std_init=0.5)
    fg, fd = g.init_params(3, seeds=[7, 8, 9]), d.init_params(3, seeds=[7, 8, 9])
    a = d.actor_end
    assert torch.equal(fg[:, :a], fd[:, :a]) and torch.equal(fg[:, a + 6:], fd[:, a:])
    assert torch.equal(fg[:, a:a + 6], torch.full((3, 6), 0.5))
    # and the Discrete spec's own result does not depend on a Gaussian spec having been built
    assert torch.equal(fd, _specs(6)[1].init_params(3, seeds=[7, 8, 9]))


def test_gaussian_spec_never_reaches_the_categorical_descriptors():
    from agilerl_amd.population.learner import graph_descriptor, net_descriptor

    g, d = _specs(4)
    assert graph_descriptor(g) is None and net_descriptor(g) is None
    assert graph_descriptor(d) is not None
    desc = g.gauss_descriptor()
    assert desc is not None and desc.n_params == g.n_params and desc.n_actions == 4
    assert desc.critic_start == g.actor_end


def test_gaussian_helper_matches_restatement():
    from agilerl_amd.population.nets import gaussian

    rng = np.random.default_rng(0)
    mean, act = rng.standard_normal((2, 5, 3)), rng.standard_normal((2, 5, 3))
    ls = rng.uniform(-1, 0.5, (2, 1, 3))
    lp, H = gaussian(torch.tensor(mean), torch.tensor(ls), torch.tensor(act))
    elp, eH = G.logp_entropy(mean, ls, act)
    np.testing.assert_allclose(lp.numpy(), elp, rtol=1e-13)
    np.testing.assert_allclose(H.numpy(), eH, rtol=1e-13)


# ---- the restatement is the reference's ----------------------------------------------- #
@pytest.mark.parametrize("case", range(4))
def test_restatement_pinned_to_reference_goldens(case):
    """tests/gauss_twin.py loss_and_grads / logp_entropy (what the GPU tests
    compare the kernels with) against the reference's log_prob_continuous /
    entropy_continuous and torch autograd of the ppo.py:868-902 loss
    (tests/golden/gen_gauss_golden.py; float64 on float32-valued inputs, so
    only float64 rounding separates them)."""
    g = dict(np.load(os.path.join(GOLDEN, f"gauss_{case}.npz")))
    b, clip, vf, ent = int(g["b"]), float(g["clip"]), float(g["vf"]), float(g["ent"])
    r = G.loss_and_grads(g["mean"], g["value"], g["log_std"], g["actions"], g["old_logp"], g["adv"], g["ret"],
                         g["old_v"], g.get("index"), b, clip, vf, ent)
    for k in ("logp", "entropy", "g_mean", "g_value", "g_log_std"):
        np.testing.assert_allclose(r[k], g[k], rtol=1e-12, atol=1e-13, err_msg=k)
    np.testing.assert_allclose(r["stats"][:, 0], g["loss"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(r["stats"][:, 4], g["approx_kl"], rtol=1e-12, atol=1e-14)
    # the fixtures hold rows on the tie rules (gauss_twin.loss_inputs)
    S = g["mean"].shape[0]
    src = g["index"] if "index" in g else np.arange(S)
    if S >= 7:
        assert (g["adv"][src] == 0).any() and (g["value"] == g["old_v"][src]).any()
        assert (g["value"] - g["old_v"][src] == np.float32(clip)).any()


# ---- the noise reference ---------------------------------------------------------------- #
def test_philox_known_answer():
    """Philox4x32-10 known-answer vectors (Random123 kat_vectors)."""
    z = G.philox(0, 0, 0, 0, 0, 0)
    assert [int(x) for x in z] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    o = G.philox(f, f, f, f, f, f)
    assert [int(x) for x in o] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


@pytest.mark.parametrize("P,N,A", [(3, 21, 6), (2, 2048, 6)])
def test_noise_reference_sequence_at_the_gpu_tests_seed(P, N, A):
    """Conditions on the REFERENCE sequence the GPU test compares the kernel's
    samples with (its population's act_seed, gauss_twin.COUNTER): a sample mean
    within 4 / sqrt(n) and a variance within 4 sqrt(2 / n) of a standard
    normal's, and no u1 on an endpoint (ln u1 finite and non-zero)."""
    seed = (5 * 0x9E3779B97F4A7C15 + 0x5851F42D) & 0xFFFFFFFFFFFFFFFF  # PPOPopulation.act_seed at seed_base 5
    env = (np.arange(P)[:, None] * N + np.arange(N)[None, :])[:, :, None]
    d = np.arange(A)[None, None, :]
    u1, u2 = G.gauss_uniforms(env, d, seed, G.COUNTER)
    assert u1.dtype == np.float32 and u1.shape == (P, N, A)
    assert u1.min() > 0.0 and u1.max() < 1.0 and u2.min() > 0.0
    eps = G.gauss_eps(env, d, seed, G.COUNTER)
    n = eps.size
    assert abs(eps.mean()) <= 4 / np.sqrt(n)
    assert abs(eps.var() - 1.0) <= 4 * np.sqrt(2 / n)
    assert np.abs(eps).max() <= 5.9
    # dimensions 2k and 2k + 1 share a Philox block, other pairs do not
    x = G.gauss_uniforms(env, np.array([0, 1, 2])[None, None, :], seed, G.COUNTER)[0]
    assert not np.array_equal(x[..., 0], x[..., 1]) and not np.array_equal(x[..., 0], x[..., 2])


# ---- architecture mutations ---------------------------------------------------------------- #
@pytest.mark.parametrize("method", ["encoder.add_layer", "encoder.add_node", "head.add_layer", "head.add_node",
                                    "add_latent_node"])
def test_architecture_mutation_keeps_log_std(method):
    from agilerl_amd.population import arch
    from agilerl_amd.population.nets import GaussianActorCriticSpec

    g, _ = _specs(6, action_std_init=0.3, action_low=(-1.0,) * 6, action_high=(1.0,) * 6)
    flat = g.init_params(1, seeds=[4])[0]
    flat[g.log_std:g.log_std + 6] = torch.tensor([0.3, -0.7, 0.11, 0.0, 1.5, -2.25])
    torch.manual_seed(0)
    rng = np.random.default_rng(3)
    new_spec, new_flat, applied, _ = arch.mutate(g, flat, method, rng, np.random.default_rng(4))
    assert applied is not None and isinstance(new_spec, GaussianActorCriticSpec)
    assert new_spec.n_params != g.n_params and new_flat.numel() == new_spec.n_params
    assert new_spec.log_std == new_spec.actor[-1].b + 6 and new_spec.actor_end == new_spec.log_std + 6
    assert torch.equal(new_flat[new_spec.log_std:new_spec.log_std + 6], flat[g.log_std:g.log_std + 6])
    assert (new_spec.action_low, new_spec.action_high, new_spec.action_std_init) == ((-1.0,) * 6, (1.0,) * 6, 0.3)


# ---- refusals ------------------------------------------------------------------------------ #
def test_box_action_refusals():
    from agilerl_amd.algorithms.ppo import spec_from_net_config
    from agilerl_amd.envs import Box
    from agilerl_amd.population.nets import GaussianActorCriticSpec

    obs = Box(-np.inf, np.inf, (8,))
    ok = spec_from_net_config(obs, Box(-2.0, 3.0, (32,)), None, action_std_init=0.1)
    assert isinstance(ok, GaussianActorCriticSpec) and ok.n_actions == 32 and ok.action_std_init == 0.1
    assert ok.action_low == (-2.0,) * 32 and ok.action_high == (3.0,) * 32
    inf = spec_from_net_config(obs, Box(-np.inf, np.inf, (2,)), {"head_config": {"hidden_size": [24],
                                                                                 "output_activation": "Tanh"}})
    assert inf.action_high == (float("inf"),) * 2 and not inf.actor[-1].act  # the actor's output stays linear
    with pytest.raises(NotImplementedError, match="squash_output"):
        spec_from_net_config(obs, Box(-1.0, 1.0, (6,)), {"squash_output": True})
    with pytest.raises(NotImplementedError, match="32"):
        spec_from_net_config(obs, Box(-1.0, 1.0, (33,)), None)
    with pytest.raises(NotImplementedError, match="1-D"):
        spec_from_net_config(obs, Box(-1.0, 1.0, (2, 3)), None)
    with pytest.raises(NotImplementedError, match="image"):
        spec_from_net_config(Box(0, 255, (4, 84, 84), dtype=np.uint8), Box(-1.0, 1.0, (6,)), None)


def test_checkpoint_spaces_round_trip_box_bounds():
    from types import SimpleNamespace

    from agilerl_amd.algorithms import checkpoint as C
    from agilerl_amd.envs import Box

    act = Box(-1.0, 1.0, (3,))
    act.high[1] = np.inf
    agent = SimpleNamespace(algo="PPO", observation_space=Box(-np.inf, np.inf, (8,)), action_space=act,
                            action_std_init=0.4)
    ck = C.checkpoint_dict(agent, {}, {})
    assert ck["action_std_init"] == 0.4 and "n_actions" not in ck["spaces"]
    obs2, act2 = C.spaces(ck)
    assert obs2.shape == (8,) and np.array_equal(act2.low, act.low) and np.array_equal(act2.high, act.high)


def test_reference_adam_rekeyed_in_the_reference_parameter_order():
    """A reference PPO file's single Adam numbers its parameters in
    actor.parameters() order, where head_net.log_std precedes
    head_net._wrapped.* (distributions.py:152-156).  The spec's state-dict keys
    follow that order, so refckpt._adam_rows hands log_std its own moments."""
    from collections import OrderedDict

    from agilerl_amd.algorithms.refckpt import _adam_rows

    g, _ = _specs(3)
    keys = g.state_dict_keys()
    nets = {n: OrderedDict((k[len(n) + 1:], torch.zeros(sh)) for k, (_, sh) in keys.items() if k.startswith(n + "."))
            for n in ("actor", "critic")}
    names = list(nets["actor"])
    i = names.index("head_net.log_std")
    assert names[i - 1].startswith("encoder.") and names[i + 1].startswith("head_net._wrapped.")
    groups = [[torch.nn.Parameter(t.clone()) for t in nets[n].values()] for n in ("actor", "critic")]
    opt = torch.optim.Adam([{"params": p} for p in groups])
    for j, p in enumerate(groups[0] + groups[1]):
        p.grad = torch.full_like(p, float(j + 1))
    opt.step()
    rows = _adam_rows(opt.state_dict(), [("actor", nets["actor"]), ("critic", nets["critic"])])
    m = rows["exp_avg"]["actor.head_net.log_std"]
    assert tuple(m.shape) == (1, 3) and torch.allclose(m, torch.full((1, 3), 0.1 * (i + 1)))
