"""PPO for MultiDiscrete action spaces without a GPU: the float64 restatements
of tests/multidisc_twin.py pinned to the reference (tests/golden/
multidisc_*.npz), the spec's layout, the conditions on the seeded inputs the GPU
tests use, checkpoints and architecture mutations carrying nvec, and the
refusals."""

import json
import os

import numpy as np
import pytest
import torch

from tests import multidisc_twin as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_GOLDEN = 5
SHAPE = dict(obs_dim=8, encoder_hidden=[64, 64], latent_dim=32, actor_hidden=[32], critic_hidden=[16])


def _specs(nvec):
    from agilerl_amd.population.nets import ActorCriticSpec, MultiDiscreteActorCriticSpec

    L = int(sum(nvec))
    return MultiDiscreteActorCriticSpec(n_actions=L, nvec=tuple(nvec), **SHAPE), ActorCriticSpec(n_actions=L, **SHAPE)


# ---- the restatement is the reference's ----------------------------------------------- #
@pytest.mark.parametrize("case", range(N_GOLDEN))
def test_restatement_pinned_to_reference_goldens(case):
    """tests/multidisc_twin.py loss_and_grads / logp_entropy / masked (what the
    GPU tests compare the kernels with) against the reference's
    log_prob_multi_discrete / entropy_multi_discrete /
    apply_action_mask_discrete and torch autograd of the ppo.py:868-902 loss
    (tests/golden/gen_multidisc_golden.py; float64 on float32-valued inputs)."""
    g = dict(np.load(os.path.join(GOLDEN, f"multidisc_{case}.npz")))
    nvec = tuple(int(n) for n in g["nvec"])
    b, clip, vf, ent = int(g["b"]), float(g["clip"]), float(g["vf"]), float(g["ent"])
    r = M.loss_and_grads(g["logits"], g["value"], nvec, g["actions"], g.get("mask"), g["old_logp"], g["adv"],
                         g["ret"], g["old_v"], g.get("index"), b, clip, vf, ent)
    for k in ("logp", "entropy", "g_logits", "g_value"):
        np.testing.assert_allclose(r[k], g[k], rtol=1e-12, atol=1e-13, err_msg=k)
    np.testing.assert_allclose(r["stats"][:, 0], g["loss"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(r["stats"][:, 4], g["approx_kl"], rtol=1e-12, atol=1e-14)
    S = g["logits"].shape[0]
    src = g["index"] if "index" in g else np.arange(S)
    if "mask" in g:
        mk = g["mask"][src]
        np.testing.assert_array_equal(M.masked(g["logits"], mk), g["masked_logits"])
        assert (mk == 0).any() and (r["g_logits"][mk == 0] == 0).all() and (g["g_logits"][mk == 0] == 0).all()
    if S >= 7:  # the fixtures hold rows on the tie rules (gauss_twin.loss_inputs)
        assert (g["adv"][src] == 0).any() and (g["value"] == g["old_v"][src]).any()
        assert (g["value"] - g["old_v"][src] == np.float32(clip)).any()


def test_goldens_cover_the_required_cases():
    meta = json.load(open(os.path.join(GOLDEN, "META_multidisc.json")))
    cases = meta["cases"]
    assert len(cases) == N_GOLDEN and len({tuple(c[0]) for c in cases}) >= 4
    assert all(tuple(c[0]) in M.NVECS for c in cases)
    assert any(c[8] for c in cases) and any(c[3] is not None for c in cases) and any(c[1] * c[2] >= 7 for c in cases)


def test_torch_helper_matches_restatement():
    from agilerl_amd.population.nets import multi_categorical

    rng = np.random.default_rng(0)
    for nvec in M.NVECS:
        L = sum(nvec)
        lg = rng.standard_normal((2, 5, L))
        act = np.stack([rng.integers(0, n, (2, 5)) for n in nvec], -1)
        mask = M.random_mask(rng, 10, nvec, keep=act.reshape(10, -1)).reshape(2, 5, L)
        for mk in (None, mask):
            lp, H = multi_categorical(torch.tensor(lg), nvec, torch.tensor(act),
                                      None if mk is None else torch.tensor(mk))
            elp, eH = M.logp_entropy(lg, nvec, act, mk)
            np.testing.assert_allclose(lp.numpy(), elp, rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(H.numpy(), eH, rtol=1e-12, atol=1e-13)
    # a one-way component contributes log-prob 0 and entropy ~0
    lp, H = M.logp_entropy(np.array([[0.3]]), (1,), np.array([[0]]))
    assert lp[0] == 0.0 and abs(H[0]) < 2e-8


def test_gumbel_scores_use_the_flat_index_stream():
    """K = 1 and K > 1 draw the same uniforms for the same flat index; word
    j & 3 of block j >> 2, as agx_ppo_act's stream."""
    env = np.array([[5], [9]])
    u = M.gumbel_uniforms(env, np.arange(8)[None, :], M.SEED, M.COUNTER)
    assert u.dtype == np.float32 and u.shape == (2, 8) and u.min() > 0 and u.max() < 1
    from tests.gauss_twin import philox

    hi = (M.COUNTER >> 32) ^ (1 << 24)
    w = philox(np.uint64(9), 0, M.COUNTER & 0xFFFFFFFF, hi, M.SEED & 0xFFFFFFFF, M.SEED >> 32)
    assert u[1, 6] == (np.float32(int(w[2]) >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)
    lg = np.zeros((1, 2, 8))
    ch, gap = M.choices(M.gumbel_scores(lg, M.SEED, M.COUNTER), (3, 1, 4))
    assert ch.shape == (1, 2, 3) and (ch[..., 1] == 0).all() and np.isinf(gap[..., 1]).all()


# ---- spec ------------------------------------------------------------------------------ #
@pytest.mark.parametrize("nvec", M.NVECS)
def test_spec_shares_the_categorical_layout(nvec):
    m, d = _specs(nvec)
    assert m.head == "multidiscrete" and m.n_actions == sum(nvec) and m.nvec == tuple(nvec)
    assert m.n_params == d.n_params and m.group_offsets == d.group_offsets
    assert m.state_dict_keys() == d.state_dict_keys()  # parameter order and count: no extra parameters
    assert list(m.state_dict_keys()) == list(d.state_dict_keys())
    assert torch.equal(m.init_params(2, seeds=[3, 4]), d.init_params(2, seeds=[3, 4]))
    assert m.shape_key() != d.shape_key()
    h = m.multi_head()
    assert h.K == len(nvec) and list(h.nvec[:h.K]) == list(nvec)


def test_spec_never_reaches_the_categorical_descriptors():
    from agilerl_amd.population.learner import graph_descriptor, net_descriptor

    for nvec in ((4,), (3, 2)):  # K = 1 too
        m, d = _specs(nvec)
        assert graph_descriptor(m) is None and net_descriptor(m) is None
        assert graph_descriptor(d) is not None
        desc = m.multi_descriptor()
        assert desc is not None and desc.n_params == m.n_params and desc.n_actions == sum(nvec)


def test_spec_rejects_a_bad_nvec():
    from agilerl_amd.population.nets import MultiDiscreteActorCriticSpec

    for nvec, L in (((), 4), ((3, 0), 3), ((3, 2), 6)):
        with pytest.raises(ValueError):
            MultiDiscreteActorCriticSpec(n_actions=L, nvec=nvec, **SHAPE)


def test_spec_from_net_config_and_refusals():
    from agilerl_amd.algorithms.ppo import spec_from_net_config
    from agilerl_amd.envs import Box, Discrete, MultiDiscrete
    from agilerl_amd.population.nets import (ActorCriticSpec, GaussianActorCriticSpec,
                                             MultiDiscreteActorCriticSpec)

    obs = Box(-np.inf, np.inf, (8,))
    ok = spec_from_net_config(obs, MultiDiscrete([2] * 16), None)
    assert isinstance(ok, MultiDiscreteActorCriticSpec) and ok.n_actions == 32 and ok.nvec == (2,) * 16
    one = spec_from_net_config(obs, MultiDiscrete([5]), {"head_config": {"hidden_size": [24]}})
    assert isinstance(one, MultiDiscreteActorCriticSpec) and one.nvec == (5,) and one.actor_hidden == [24]
    sp = MultiDiscrete([3, 2])
    assert sp.shape == (2,) and sp.dtype == np.int64
    s = sp.sample()
    assert s.shape == (2,) and s.dtype == np.int64 and (s >= 0).all() and (s < sp.nvec).all()
    # a Discrete and a Box space still build the specs they build today
    d = spec_from_net_config(obs, Discrete(4), None)
    assert type(d) is ActorCriticSpec and d.head == "categorical" and d.n_actions == 4
    g = spec_from_net_config(obs, Box(-1.0, 1.0, (3,)), None, action_std_init=0.2)
    assert type(g) is GaussianActorCriticSpec and g.n_actions == 3
    with pytest.raises(NotImplementedError, match="32"):
        spec_from_net_config(obs, MultiDiscrete([16, 17]), None)
    with pytest.raises(NotImplementedError, match="1-D"):
        spec_from_net_config(obs, MultiDiscrete([[2, 2], [3, 3]]), None)
    with pytest.raises(NotImplementedError, match="image"):
        spec_from_net_config(Box(0, 255, (4, 84, 84), dtype=np.uint8), MultiDiscrete([3, 2]), None)

    class MultiBinary:  # gymnasium's has n and shape, no nvec
        n, shape = 4, (4,)

    with pytest.raises(NotImplementedError, match="MultiBinary"):
        spec_from_net_config(obs, MultiBinary(), None)


def test_synthetic_env_nvec():
    from agilerl_amd.envs import Discrete, MultiDiscrete, SyntheticVecEnv

    e = SyntheticVecEnv(4, nvec=(3, 2))
    assert isinstance(e.single_action_space, MultiDiscrete) and list(e.action_space.nvec) == [3, 2]
    obs, _ = e.reset()
    obs2, rew, term, trunc, _ = e.step(np.zeros((4, 2), np.int64))
    assert obs2.shape == (4, 8) and rew.shape == (4,)
    d = SyntheticVecEnv(4)  # the default is today's env
    assert isinstance(d.single_action_space, Discrete) and d.single_action_space.n == 4
    a, b = SyntheticVecEnv(4, seed=3), SyntheticVecEnv(4, seed=3, nvec=(2, 2))
    assert np.array_equal(a._obs, b._obs) and np.array_equal(a._rew, b._rew)
    with pytest.raises(ValueError):
        SyntheticVecEnv(4, nvec=(2,), action_dim=2)


def test_checkpoint_spaces_round_trip_nvec():
    from types import SimpleNamespace

    from agilerl_amd.algorithms import checkpoint as C
    from agilerl_amd.envs import Box, MultiDiscrete

    agent = SimpleNamespace(algo="PPO", observation_space=Box(-np.inf, np.inf, (8,)),
                            action_space=MultiDiscrete([5, 1, 4]))
    ck = C.checkpoint_dict(agent, {}, {})
    assert ck["spaces"] == {"obs_shape": [8], "nvec": [5, 1, 4]}
    obs2, act2 = C.spaces(ck)
    assert obs2.shape == (8,) and isinstance(act2, MultiDiscrete) and list(act2.nvec) == [5, 1, 4]


@pytest.mark.parametrize("method", ["encoder.add_layer", "encoder.add_node", "head.add_layer", "head.add_node",
                                    "add_latent_node"])
def test_architecture_mutation_keeps_the_output_width_and_nvec(method):
    from agilerl_amd.population import arch
    from agilerl_amd.population.nets import MultiDiscreteActorCriticSpec

    m, _ = _specs((3, 2, 4))
    flat = m.init_params(1, seeds=[4])[0]
    torch.manual_seed(0)
    new_spec, new_flat, applied, _ = arch.mutate(m, flat, method, np.random.default_rng(3), np.random.default_rng(4))
    assert applied is not None and isinstance(new_spec, MultiDiscreteActorCriticSpec)
    assert new_spec.n_params != m.n_params and new_flat.numel() == new_spec.n_params
    assert new_spec.nvec == (3, 2, 4) and new_spec.n_actions == 9 and new_spec.actor[-1].fout == 9
    assert new_spec.head == "multidiscrete" and new_spec.multi_descriptor() is not None


# ---- conditions on the seeded inputs of the GPU tests ------------------------------------- #
def test_gpu_test_inputs_meet_their_conditions():
    """tests/test_multidisc_ppo_gpu.py checks its own inputs on the device's
    logits; here the twin alone: with logits of the scale the GPU tests see
    (0.1-scaled output layer: |lg| well below 1) the share of (row, component)
    pairs whose float64 top-two Gumbel score gap is under 1e-4 stays far below
    1 % at the tests' seed and counter."""
    rng = np.random.default_rng(11)
    for nvec in ((3, 2), (7, 20, 5), (2,) * 16):
        for P, N in ((3, 21), (2, 2048)):
            lg = 0.3 * rng.standard_normal((P, N, sum(nvec)))
            _, gap = M.choices(M.gumbel_scores(lg, M.SEED, M.COUNTER), nvec)
            share = float((gap < 1e-4).mean())
            print(f"nvec {nvec} P {P} N {N}: excluded share {share:.5f}")
            assert share <= 0.01
