"""PPO for MultiBinary action spaces without a GPU: the float64 restatements of
tests/multibinary_twin.py pinned to the reference (tests/golden/
multibinary_*.npz) and to the MultiDiscrete restatement at nvec = [2] * n, the
spec's layout, the env option, checkpoints and architecture mutations carrying
the head, the conditions on the seeded inputs the GPU tests use, and the
refusals."""

import json
import os

import numpy as np
import pytest
import torch

from tests import multibinary_twin as B
from tests import multidisc_twin as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_GOLDEN = 5
SHAPE = dict(obs_dim=8, encoder_hidden=[64, 64], latent_dim=32, actor_hidden=[32], critic_hidden=[16])


def _specs(n):
    from agilerl_amd.population.nets import ActorCriticSpec, MultiBinaryActorCriticSpec

    return MultiBinaryActorCriticSpec(n_actions=n, **SHAPE), ActorCriticSpec(n_actions=n, **SHAPE)


# ---- the restatement is the reference's ----------------------------------------------- #
@pytest.mark.parametrize("case", range(N_GOLDEN))
def test_restatement_pinned_to_reference_goldens(case):
    """tests/multibinary_twin.py loss_and_grads / logp_entropy / masked against
    the reference's log_prob_multi_binary / entropy_multi_binary /
    apply_action_mask_discrete and torch autograd of the ppo.py:868-902 loss
    (tests/golden/gen_multibinary_golden.py; float64 on float32-valued inputs)."""
    g = dict(np.load(os.path.join(GOLDEN, f"multibinary_{case}.npz")))
    b, clip, vf, ent = int(g["b"]), float(g["clip"]), float(g["vf"]), float(g["ent"])
    assert g["logits"].shape[1] == int(g["n"])
    r = B.loss_and_grads(g["logits"], g["value"], g["actions"], g.get("mask"), g["old_logp"], g["adv"], g["ret"],
                         g["old_v"], g.get("index"), b, clip, vf, ent)
    for k in ("logp", "entropy", "g_logits", "g_value"):
        np.testing.assert_allclose(r[k], g[k], rtol=1e-12, atol=1e-13, err_msg=k)
    np.testing.assert_allclose(r["stats"][:, 0], g["loss"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(r["stats"][:, 4], g["approx_kl"], rtol=1e-12, atol=1e-14)
    S = g["logits"].shape[0]
    src = g["index"] if "index" in g else np.arange(S)
    if "mask" in g:
        mk = g["mask"][src]
        np.testing.assert_array_equal(B.masked(g["logits"], mk), g["masked_logits"])
        assert (mk == 0).any() and (r["g_logits"][mk == 0] == 0).all() and (g["g_logits"][mk == 0] == 0).all()
        assert (g["actions"][src][mk == 0] == 0).all()  # a stored 1-bit is legal
    if S >= 7:  # the fixtures hold rows on the tie rules (gauss_twin.loss_inputs)
        assert (g["adv"][src] == 0).any() and (g["value"] == g["old_v"][src]).any()
        assert (g["value"] - g["old_v"][src] == np.float32(clip)).any()


def test_goldens_cover_the_required_cases():
    meta = json.load(open(os.path.join(GOLDEN, "META_multibinary.json")))
    cases = [tuple(c[:4]) + (bool(c[8]),) for c in meta["cases"]]
    assert cases == [(1, 1, 1, None, False), (5, 5, 3, None, False), (16, 16, 2, 40, True), (17, 8, 2, None, True),
                     (32, 7, 2, 20, False)]
    assert all(c[0] in B.NS for c in cases)


@pytest.mark.parametrize("n", [n for n in B.NS if n <= 16])
def test_restatement_equals_multidiscrete_over_two_way_components(n):
    """A Bernoulli over logit l is the categorical over logits (0, l): equal
    log-prob and entropy (the entropy's 1e-8 sits inside the logarithm in both)."""
    rng = np.random.default_rng(n)
    lg = 1.5 * rng.standard_normal((7, n))
    act = rng.integers(0, 2, (7, n))
    pair = np.stack([np.zeros_like(lg), lg], -1).reshape(7, 2 * n)
    lp, H = B.logp_entropy(lg, act)
    elp, eH = M.logp_entropy(pair, (2,) * n, act)
    np.testing.assert_allclose(lp, elp, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(H, eH, rtol=1e-12, atol=1e-13)


def test_restatement_edge_cases():
    # a masked bit with stored action 0 contributes exactly 0; everything stays finite at |l| = 1e8
    lp, H = B.logp_entropy(np.array([[0.7, -0.2]]), np.array([[1, 0]]), np.array([[1, 0]]))
    lp1, H1 = B.logp_entropy(np.array([[0.7]]), np.array([[1]]))
    assert lp[0] == lp1[0] and abs(H[0] - H1[0]) < 2e-8
    for big in (1e8, -1e8):
        for a in (0, 1):
            lp, H = B.logp_entropy(np.array([[big]]), np.array([[a]]))
            assert np.isfinite(lp[0]) and np.isfinite(H[0])
    # a stored action other than 0 / 1 counts as 1
    lg = np.array([[0.3]])
    for odd in (7, -3):
        assert B.logp_entropy(lg, np.array([[odd]]))[0] == B.logp_entropy(lg, np.array([[1]]))[0]
    # the mode: a logit of exactly 0 gives 0; a masked bit is never 1
    assert B.mode(np.array([0.0, 1e-9, -1.0, 5.0]), np.array([1, 1, 1, 0])).tolist() == [0, 1, 0, 0]
    bits, _ = B.choices(np.full((1, 4), 30.0), np.full((1, 4), 0.5), np.array([[1, 0, 1, 0]]))
    assert bits.tolist() == [[1, 0, 1, 0]]


def test_torch_helper_matches_restatement():
    from agilerl_amd.population.nets import bernoulli_head

    rng = np.random.default_rng(0)
    for n in B.NS:
        lg = 1.5 * rng.standard_normal((2, 5, n))
        act = rng.integers(0, 2, (2, 5, n))
        mask = B.random_mask(rng, 10, n, keep=act.reshape(10, n)).reshape(2, 5, n)
        for mk in (None, mask):
            lp, H = bernoulli_head(torch.tensor(lg), torch.tensor(act), None if mk is None else torch.tensor(mk))
            elp, eH = B.logp_entropy(lg, act, mk)
            np.testing.assert_allclose(lp.numpy(), elp, rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(H.numpy(), eH, rtol=1e-12, atol=1e-13)
    # autograd of the helper is the hand gradient of the restatement (masked: exactly 0)
    r = B.loss_inputs(17, 8, 2, None, 9, 0.2, True)
    e = B.loss_and_grads(r["logits"], r["value"], r["actions"], r["mask"], r["old_logp"], r["adv"], r["ret"],
                         r["old_v"], None, 8, 0.2, 0.5, 0.01)
    from tests.gauss_twin import torch_loss

    t64 = lambda k: torch.tensor(r[k], dtype=torch.float64)  # noqa: E731
    lg, v = t64("logits").requires_grad_(True), t64("value").requires_grad_(True)
    lp, H = bernoulli_head(lg, torch.tensor(r["actions"]), torch.tensor(r["mask"]))
    total = 0
    for m in range(2):
        s = slice(8 * m, 8 * m + 8)
        total = total + torch_loss(lp[s], H[s], v[s], t64("old_logp")[s], t64("adv")[s], t64("ret")[s],
                                   t64("old_v")[s], 0.2, 0.5, 0.01)[0]
    total.backward()
    np.testing.assert_allclose(lg.grad.numpy(), e["g_logits"], rtol=1e-10, atol=1e-13)
    assert (lg.grad.numpy()[r["mask"] == 0] == 0).all()


def test_uniforms_are_the_multi_categorical_stream():
    u = B.uniforms(2, 3, 8, B.SEED, B.COUNTER, env_base=[5, 9])
    g = M.gumbel_uniforms(np.array([[9 + 2]]), np.arange(8)[None, :], B.SEED, B.COUNTER)
    assert u.shape == (2, 3, 8) and np.array_equal(u[1, 2], g[0].astype(np.float64))
    assert u.min() > 0 and u.max() < 1


# ---- spec ------------------------------------------------------------------------------ #
@pytest.mark.parametrize("n", B.NS)
def test_spec_shares_the_categorical_layout(n):
    m, d = _specs(n)
    assert m.head == "multibinary" and m.n_actions == n and m.actor[-1].fout == n
    assert m.n_params == d.n_params and m.group_offsets == d.group_offsets
    assert list(m.state_dict_keys()) == list(d.state_dict_keys()) and m.state_dict_keys() == d.state_dict_keys()
    assert torch.equal(m.init_params(2, seeds=[3, 4]), d.init_params(2, seeds=[3, 4]))
    assert m.shape_key() != d.shape_key()
    desc = m.bern_descriptor()
    assert desc is not None and desc.n_params == m.n_params and desc.n_actions == n
    assert m.bern_learn_descriptor() is not None


def test_spec_never_reaches_the_categorical_descriptors():
    from agilerl_amd.population.learner import graph_descriptor, net_descriptor

    m, d = _specs(4)
    assert graph_descriptor(m) is None and net_descriptor(m) is None
    assert graph_descriptor(d) is not None
    with pytest.raises(ValueError):
        _specs(0)
    with pytest.raises(ValueError):
        _specs(33)


def test_spec_from_net_config_and_refusals():
    from agilerl_amd.algorithms.ppo import spec_from_net_config
    from agilerl_amd.envs import Box, Discrete, MultiBinary, MultiDiscrete
    from agilerl_amd.population.nets import (ActorCriticSpec, MultiBinaryActorCriticSpec,
                                             MultiDiscreteActorCriticSpec)

    obs = Box(-np.inf, np.inf, (8,))
    sp = MultiBinary(4)
    assert sp.n == 4 and sp.shape == (4,) and sp.dtype == np.int8
    s = sp.sample()
    assert s.shape == (4,) and s.dtype == np.int8 and set(s.tolist()) <= {0, 1}
    ok = spec_from_net_config(obs, sp, None)
    assert type(ok) is MultiBinaryActorCriticSpec and ok.actor[-1].fout == 4 and ok.action_dtype == "int8"
    one = spec_from_net_config(obs, MultiBinary(32), {"head_config": {"hidden_size": [24]}})
    assert one.n_actions == 32 and one.actor_hidden == [24]
    assert spec_from_net_config(obs, MultiBinary(1), None).n_actions == 1

    class Other:  # duck-typed: the class name, an integer n, shape (n,), a dtype
        def __init__(self, n, shape, dtype=np.float32):
            self.n, self.shape, self.dtype = n, shape, dtype

    Other.__name__ = "MultiBinary"
    assert spec_from_net_config(obs, Other(3, (3,)), None).action_dtype == "float32"
    for bad in (Other((2, 3), (2, 3)), Other(33, (33,)), Other(0, (0,)), Other(3, (4,)), Other(3, (3,), None)):
        with pytest.raises(NotImplementedError, match="MultiBinary"):
            spec_from_net_config(obs, bad, None)
    with pytest.raises(NotImplementedError, match="MultiBinary"):
        spec_from_net_config(Box(0, 255, (4, 84, 84), dtype=np.uint8), MultiBinary(4), None)
    # the other spaces still build the specs they build today
    assert type(spec_from_net_config(obs, Discrete(4), None)) is ActorCriticSpec
    assert type(spec_from_net_config(obs, MultiDiscrete([2, 2]), None)) is MultiDiscreteActorCriticSpec


def test_synthetic_env_n_binary():
    from agilerl_amd.envs import Discrete, MultiBinary, SyntheticVecEnv

    e = SyntheticVecEnv(4, n_binary=5)
    assert isinstance(e.single_action_space, MultiBinary) and e.action_space.n == 5
    e.reset()
    obs2, rew, term, trunc, _ = e.step(np.zeros((4, 5), np.int8))
    assert obs2.shape == (4, 8) and rew.shape == (4,)
    assert isinstance(SyntheticVecEnv(4).single_action_space, Discrete)  # the default is today's env
    a, b = SyntheticVecEnv(4, seed=3), SyntheticVecEnv(4, seed=3, n_binary=6)
    assert np.array_equal(a._obs, b._obs) and np.array_equal(a._rew, b._rew) and np.array_equal(a._term, b._term)
    with pytest.raises(ValueError):
        SyntheticVecEnv(4, n_binary=2, action_dim=2)
    with pytest.raises(ValueError):
        SyntheticVecEnv(4, n_binary=2, nvec=(2,))


def test_checkpoint_spaces_round_trip_n_binary():
    from types import SimpleNamespace

    from agilerl_amd.algorithms import checkpoint as C
    from agilerl_amd.envs import Box, Discrete, MultiBinary

    agent = SimpleNamespace(algo="PPO", observation_space=Box(-np.inf, np.inf, (8,)), action_space=MultiBinary(6))
    ck = C.checkpoint_dict(agent, {}, {})
    assert ck["spaces"] == {"obs_shape": [8], "n_binary": 6}
    obs2, act2 = C.spaces(ck)
    assert obs2.shape == (8,) and isinstance(act2, MultiBinary) and act2.n == 6
    agent.action_space = Discrete(6)  # a Discrete space keeps its key
    assert C.checkpoint_dict(agent, {}, {})["spaces"] == {"obs_shape": [8], "n_actions": 6}


def test_reference_layout_checkpoint_names_multibinary():
    from agilerl_amd.algorithms import refckpt

    obs = refckpt._standin("gymnasium.spaces.box.Box")()
    obs.state = {"_shape": (8,)}
    act = refckpt._standin("gymnasium.spaces.multi_binary.MultiBinary")()
    act.state = {"n": 6, "_shape": (6,)}
    assert refckpt._space_shapes({"observation_space": obs, "action_space": act}) == {"obs_shape": [8], "n_binary": 6}
    act.state = {"n": (2, 3), "_shape": (2, 3)}
    assert refckpt._space_shapes({"observation_space": obs, "action_space": act}) is None


@pytest.mark.parametrize("method", ["encoder.add_layer", "encoder.add_node", "head.add_layer", "head.add_node",
                                    "add_latent_node"])
def test_architecture_mutation_keeps_the_head(method):
    from agilerl_amd.population import arch
    from agilerl_amd.population.nets import MultiBinaryActorCriticSpec

    m, _ = _specs(9)
    flat = m.init_params(1, seeds=[4])[0]
    torch.manual_seed(0)
    new_spec, new_flat, applied, _ = arch.mutate(m, flat, method, np.random.default_rng(3), np.random.default_rng(4))
    assert applied is not None and isinstance(new_spec, MultiBinaryActorCriticSpec)
    assert new_spec.n_params != m.n_params and new_flat.numel() == new_spec.n_params
    assert new_spec.n_actions == 9 and new_spec.actor[-1].fout == 9 and new_spec.action_dtype == "int8"
    assert new_spec.head == "multibinary" and new_spec.bern_descriptor() is not None


# ---- routing predicates (no device) ---------------------------------------------------- #
def _bare_population(spec, fused=True):
    from agilerl_amd.population.ppo_pop import PPOPopulation

    pop = PPOPopulation.__new__(PPOPopulation)
    pop.spec = spec
    head = getattr(spec, "head", "categorical")
    pop.gaussian, pop.multidiscrete = head == "gaussian", head == "multidiscrete"
    pop.fused, pop.multi_fused = fused, False
    pop._desc = pop._gdesc = pop._edesc = pop._gauss = pop._glearn = pop._mlearn = pop._multi = pop._mhead = None
    return pop


def test_fused_learner_is_the_default_and_can_be_switched_off(monkeypatch):
    monkeypatch.delenv("AGX_BERN_FUSED", raising=False)
    m, d = _specs(5)
    pop = _bare_population(m)
    assert pop.multibinary and pop.vector_int and pop.act_width == 5 and not pop.multidiscrete
    assert pop.bern_learn_descriptor() is not None and pop._fused_learner()
    assert pop.bern_learn_descriptor() is pop.bern_learn_descriptor()  # made once
    assert pop.learn_descriptor() is None and pop.fused_descriptor() is None and pop.eval_descriptor() is None
    assert pop.multi_learn_descriptor() is None and pop.gauss_learn_descriptor() is None
    assert not _bare_population(m, fused=False)._fused_learner()
    monkeypatch.setenv("AGX_BERN_FUSED", "0")
    assert _bare_population(m).bern_learn_descriptor() is None and not _bare_population(m)._fused_learner()
    cat = _bare_population(d)  # a Discrete population is untouched by the switch
    assert not cat.multibinary and cat.act_width == 1 and cat.bern_learn_descriptor() is None and cat._fused_learner()


# ---- conditions on the seeded inputs of the GPU tests ------------------------------------- #
def test_gpu_test_inputs_meet_their_conditions():
    """The sampled-step GPU test excludes a bit whose float64 |u - p| is under
    1e-4 and requires at most 1 % excluded; here the twin alone, at logits of
    the scale the GPU tests see and at their seed and counter (expected share
    2e-4)."""
    rng = np.random.default_rng(11)
    for n in (5, 17, 32):
        for P, N in ((3, 21), (2, 2048)):
            lg = 0.3 * rng.standard_normal((P, N, n))
            _, gap = B.choices(lg, B.uniforms(P, N, n, B.SEED, B.COUNTER))
            share = float((gap < 1e-4).mean())
            print(f"n {n} P {P} N {N}: excluded share {share:.5f}")
            assert share <= 0.01
