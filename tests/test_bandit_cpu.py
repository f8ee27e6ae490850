"""NeuralUCB / NeuralTS without a GPU: the float64 twin (tests/bandit_twin.py)
against every step the reference's own get_action produced
(tests/golden/bandit_*.npz), the CPU agent on the golden networks, the
closed-form gradient against the autograd loop, the ABI, the covariance rule
after an architecture mutation, clones, checkpoints, create_population,
BanditEnv against the reference's recorded outputs, and train_bandits.

The bound on every float32 result is 4 x max(err_ref, 1 float32 ulp of the
value), err_ref being the error of the reference's own float32 evaluation of
a step against float64 on the same inputs (META_bandit.json) —
test_cqn_gpu.py's convention.  It is a one-step figure, so every comparison
is one step deep: the twin is evaluated on the float32 matrix the code under
test held before the step.  (Two float32 runs of 64 steps drift apart by their
accumulated rounding, which a one-step error does not bound and which says
nothing about a single step.)  Actions are compared exactly, over the whole run: every
fixture step keeps the best two legal scores 64 x err_ref apart."""

import glob
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import bandit_twin as T

HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, "golden", "META_bandit.json")))
CASES = sorted(META["errors"])


def _mask(g, t):
    return g["mask"][t] if bool(g["masked"]) else None


def _single(case):
    return bool(META["shapes"][case][4])


# ---- the twin against the reference ------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_twin_matches_reference_golden(golden, case):
    g, err = golden(case), META["errors"][case]
    S = (float(g["lamb"]) * np.eye(g["h"].shape[2] + 1)).astype(np.float32)
    for t in range(len(g["action"])):
        step = T.select(T.gradients(g["h"][t]), g["mu"][t], S, _mask(g, t), float(g["gamma"]))
        assert step["action"] == int(g["action"][t]), (case, t)
        gap = err["gap"][t]
        if gap is not None:
            assert gap >= 64 * err["err_ref_scores"][t] and abs(step["gap"] - gap) <= 1e-9
        d_scores = np.abs(g["action_values"][t].astype(np.float64) - step["scores"])
        d_sigma = np.abs(g["sigma_inv"][t].astype(np.float64) - step["sigma_inv"])
        assert (d_scores <= T.bound(err["err_ref_scores"][t], step["scores"])).all(), (case, t, d_scores.max())
        assert (d_sigma <= T.bound(err["err_ref_sigma"][t], step["sigma_inv"])).all(), (case, t, d_sigma.max())
        # the recorded errors are this twin's distance from the reference (another float64 evaluation
        # differs by float64 rounding)
        assert abs(d_scores.max() - err["err_ref_scores"][t]) <= 1e-12
        assert abs(d_sigma.max() - err["err_ref_sigma"][t]) <= 1e-12
        S = g["sigma_inv"][t]  # the matrix the reference holds before the next step


def test_onehot_case_overrules_the_best_arm(golden):
    """The fixture does what it is for: the one legal arm is not the best."""
    g = golden("bandit_onehot")
    assert (g["mask"].sum(axis=1) == 1).all()
    assert any(int(np.argmax(g["action_values"][t])) != int(g["action"][t]) for t in range(len(g["action"])))
    assert all(g["mask"][t][int(g["action"][t])] == 1 for t in range(len(g["action"])))


def _golden_agent(g, case, cls=None, device="cpu"):
    from agilerl_amd.algorithms import NeuralUCB
    from agilerl_amd.envs import Box, Discrete
    from agilerl_amd.networks.base import mlp_net_config

    A, H = int(META["shapes"][case][0]), int(META["shapes"][case][1])
    net = META["net"]
    cfg = {"encoder_config": {"hidden_size": [net["encoder"]]}, "latent_dim": net["latent"],
           "head_config": mlp_net_config([H], layer_norm=False)}
    agent = (cls or NeuralUCB)(Box(-np.inf, np.inf, (net["obs"],)), Discrete(A), net_config=cfg,
                               gamma=float(g["gamma"]), lamb=float(g["lamb"]), device=device)
    params = list(agent.actor.parameters())
    assert len(params) == 8
    with torch.no_grad():
        for i, p in enumerate(params):
            p.copy_(torch.from_numpy(g[f"param_{i}"]))
    agent.init_params()
    return agent


@pytest.mark.parametrize("case", CASES)
def test_cpu_agent_matches_reference_golden(golden, case):
    g, err = golden(case), META["errors"][case]
    agent = _golden_agent(g, case)
    assert agent.closed_form() and agent.numel == g["h"].shape[2] + 1
    for t in range(len(g["action"])):
        # the twin restates the selection, not the network: it runs on the features this build's forward
        # gives (another matmul blocking may round mu or h an ulp away from the recorded ones)
        mu, h = (x.numpy() for x in agent.arm_features(agent._obs(g["context"][t])))
        np.testing.assert_allclose(mu, g["mu"][t], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(h, g["h"][t], rtol=1e-5, atol=1e-6)
        step = T.select(T.gradients(h), mu, agent.sigma_inv.numpy(), _mask(g, t), float(g["gamma"]))
        S = step["sigma_inv"]
        action = agent.get_action(g["context"][t], action_mask=_mask(g, t))
        assert isinstance(action, int) and action == int(g["action"][t]), (case, t)
        d = np.abs(agent.sigma_inv.numpy().astype(np.float64) - S)
        assert (d <= T.bound(err["err_ref_sigma"][t], S)).all(), (case, t, d.max())
        d = np.abs(agent.last_scores.numpy().astype(np.float64) - step["scores"])
        assert (d <= T.bound(err["err_ref_scores"][t], step["scores"])).all(), (case, t, d.max())


# ---- the closed-form gradient -------------------------------------------------------------------
def _env(arms=4, features=6, seed=3):
    from agilerl_amd.envs import SyntheticBanditEnv

    return SyntheticBanditEnv(arms=arms, features=features, seed=seed)


def test_closed_form_gradient_equals_autograd_bitwise():
    from agilerl_amd.algorithms import NeuralTS, NeuralUCB

    env = _env()
    for cls in (NeuralUCB, NeuralTS):
        torch.manual_seed(1)
        agent = cls(env.observation_space, env.action_space, device="cpu")
        assert agent.closed_form() and agent.numel == 33 and type(agent.exp_layer) is torch.nn.Linear
        assert not any(isinstance(m, torch.nn.LayerNorm) for m in agent.actor.encoder.modules())  # layer_norm=False
        for ctx in (env.reset(), env.reset()[:1]):  # every arm its row; one row repeated over the arms
            x = agent._obs(ctx)
            mu, h = agent.arm_features(x)
            mu_a, g_a = agent.arm_gradients(x)
            g = torch.cat([h * agent._scale, torch.full((4, 1), agent._scale)], dim=1)
            assert g.shape == g_a.shape == (4, 33) and torch.equal(g, g_a) and torch.equal(mu, mu_a)
            assert (h > 0).any()


def test_output_activation_selects_the_autograd_route(monkeypatch):
    from agilerl_amd import kernels as K
    from agilerl_amd.algorithms import NeuralUCB
    from agilerl_amd.networks.base import mlp_net_config

    env = _env()
    torch.manual_seed(2)
    agent = NeuralUCB(env.observation_space, env.action_space, device="cpu",
                      net_config={"head_config": mlp_net_config([32], output_activation="Tanh")})
    assert not agent.closed_form()
    seen = {}
    real = K.bandit_select_torch

    def spy(h, mu, sigma_inv, mask=None, **kw):
        seen.update(kw, g=h.clone(), mu=mu.clone(), S=sigma_inv.clone())
        return real(h, mu, sigma_inv, mask, **kw)

    monkeypatch.setattr(K, "bandit_select_torch", spy)
    ctx = env.reset()
    action = agent.get_action(ctx)
    assert seen["bias_one"] is False and seen["g"].shape == (4, 33)
    # the explicit g carries the activation's derivative: not [h, 1]
    _, h = agent.arm_features(agent._obs(ctx))
    assert not torch.equal(seen["g"][:, :32], h)
    step = T.select(seen["g"].numpy().astype(np.float64), seen["mu"].numpy(), seen["S"].numpy(), None, 1.0)
    assert action == step["action"]
    np.testing.assert_allclose(agent.sigma_inv.numpy(), step["sigma_inv"], rtol=0, atol=1e-6)


# ---- ABI -----------------------------------------------------------------------------------------
def test_abi_bandit_symbols_and_signatures():
    from agilerl_amd import _lib
    from tests.test_abi import header_arity

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lib = _lib.load(require_gpu=False)
    arity = header_arity()
    for name in ("agx_bandit_select", "agx_bandit_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == arity[name]
    from agilerl_amd import kernels as K

    header = open(os.path.join(os.path.dirname(HERE), "include", "agx_bandit.h")).read()
    for macro, value in (("AGX_BANDIT_RESIDENT_MAX_D", K.BANDIT_RESIDENT_MAX_D), ("AGX_BANDIT_MAX_D", K.BANDIT_MAX_D),
                         ("AGX_BANDIT_MAX_ARMS", K.BANDIT_MAX_ARMS)):
        assert f"#define {macro} {value}\n" in header
    assert lib.agx_bandit_workspace_bytes(10, 33) == 16
    assert lib.agx_bandit_workspace_bytes(7, 501) == (2 * 501 + 2 * 4 * 7) * 8  # u, w, 2 x 4 tiles of 7 partials
    assert lib.agx_bandit_workspace_bytes(1025, 33) == 0 and lib.agx_bandit_workspace_bytes(2, 1026) == 0
    # argument validation happens before any HIP call
    rc = lib.agx_bandit_select(None, 0, None, None, None, 1, 1, 1, 1.0, 1.0, 0, 0, None, None, None, None, None, None)
    assert rc == -1 and b"null pointer" in lib.agx_last_error()


# ---- the covariance after an architecture mutation ---------------------------------------------
def _numpy_rule(S, old, new, lamb):
    """np.delete / np.insert on a weight [1, old] + bias [1] layout."""
    S = np.array(S)
    if new < old:
        drop = list(range(new, old))
        S = np.delete(np.delete(S, drop, 0), drop, 1)
    elif new > old:
        at = [old] * (new - old)
        S = np.insert(np.insert(S, at, 0.0, 0), at, 0.0, 1)
        for i in range(old, new):
            S[i, i] = lamb
    return S


@pytest.mark.parametrize("method,delta", [("head_net.add_node", 16), ("head_net.remove_node", -16)])
def test_reinit_rule_on_a_resized_exploration_layer(method, delta):
    from agilerl_amd.algorithms import NeuralUCB
    from agilerl_amd.hpo.mutation import reinit_bandit_grads
    from agilerl_amd.networks.base import mlp_net_config

    env = _env()
    torch.manual_seed(4)
    agent = NeuralUCB(env.observation_space, env.action_space, device="cpu", lamb=0.5,
                      net_config={"head_config": mlp_net_config([48])})
    ctx = env.reset()
    for _ in range(6):
        ctx, _ = env.step(agent.get_action(ctx))
    before = agent.sigma_inv.numpy().copy()
    assert before.shape == (49, 49) and np.abs(before - 0.5 * np.eye(49)).max() > 1e-3
    old = agent._exp_sizes()
    assert old == {"weight": 48, "bias": 1}
    applied, _ = agent.actor.apply_mutation_dict(method, {"hidden_layer": 0, "numb_new_nodes": 16})
    assert applied == method
    agent._reinit_bandit_grads(old)
    agent.reinit_optimizers()
    H = 48 + delta
    want = _numpy_rule(before, 48, H, 0.5)
    assert agent.numel == H + 1 and agent.exp_layer is agent.actor.get_output_dense()
    np.testing.assert_array_equal(agent.sigma_inv.numpy(), want)
    np.testing.assert_array_equal(reinit_bandit_grads(before, old, {"weight": H, "bias": 1}, 0.5), want)
    assert torch.equal(agent.theta_0, torch.cat([p.detach().flatten() for p in agent.exp_layer.parameters()]))
    kept = min(48, H)
    np.testing.assert_array_equal(want[:kept, :kept], before[:kept, :kept])
    np.testing.assert_array_equal(want[-1, :kept], before[-1, :kept])  # the bias row moved with its column
    assert want[-1, -1] == before[-1, -1]
    if delta > 0:
        assert (np.diag(want)[48:H] == 0.5).all() and not want[48:H, :48].any()
    # a vanished parameter loses its rows, a new one gets lamb
    np.testing.assert_array_equal(reinit_bandit_grads(before, old, {"weight": 48}, 0.5), before[:48, :48])
    grown = reinit_bandit_grads(before[:48, :48], {"weight": 48}, old, 0.5)
    assert grown.shape == (49, 49) and grown[48, 48] == 0.5 and not grown[48, :48].any()
    assert isinstance(agent.get_action(ctx), int)  # the agent goes on with the new layer
    assert np.isfinite(agent.learn({"obs": torch.randn(8, 24), "reward": torch.rand(8, 1)}))


def test_architecture_mutation_through_mutations_keeps_the_covariance():
    from agilerl_amd.algorithms import NeuralUCB
    from agilerl_amd.hpo.mutation import Mutations

    env = _env()
    torch.manual_seed(5)
    agent = NeuralUCB(env.observation_space, env.action_space, device="cpu")
    ctx = env.reset()
    for _ in range(4):
        ctx, _ = env.step(agent.get_action(ctx))
    muts = Mutations(no_mutation=0, architecture=1, new_layer_prob=0.3, parameters=0, activation=0, rl_hp=0,
                     rand_seed=3)
    for _ in range(6):
        before, old_numel = agent.sigma_inv.clone(), agent.numel
        agent = muts.mutation([agent])[0]
        assert agent.mut not in (None, "None") and agent.exp_layer is agent.actor.get_output_dense()
        assert agent.sigma_inv.shape == (agent.numel, agent.numel)
        k = min(old_numel, agent.numel) - 1
        assert torch.equal(agent.sigma_inv[:k, :k], before[:k, :k])  # never reset to lamb * I
        assert list(agent.optimizer.param_groups[0]["params"])[0] is next(agent.actor.parameters())
        ctx, _ = env.step(agent.get_action(ctx))


# ---- clone, checkpoint, population ----------------------------------------------------------------
def _same_agent(a, b):
    sa, sb = a.actor.state_dict(), b.actor.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(a.sigma_inv, b.sigma_inv) and torch.equal(a.theta_0, b.theta_0)
    assert a.numel == b.numel and list(a.regret) == list(b.regret)
    assert int(a.ts_counter) == int(b.ts_counter) and a.noise_base == b.noise_base
    assert (a.lamb, a.reg, a.gamma, a.lr, a.batch_size, a.learn_step) == \
        (b.lamb, b.reg, b.gamma, b.lr, b.batch_size, b.learn_step)
    assert b.exp_layer is b.actor.get_output_dense() and a.exp_layer is not b.exp_layer


@pytest.mark.parametrize("name", ["NeuralUCB", "NeuralTS"])
def test_clone_and_checkpoint_round_trip(name, tmp_path):
    from agilerl_amd import algorithms
    from agilerl_amd.hpo.mutation import Mutations

    cls = getattr(algorithms, name)
    env = _env()
    torch.manual_seed(6)
    agent = cls(env.observation_space, env.action_space, device="cpu", lamb=2.0, reg=0.001, batch_size=8)
    ctx = env.reset()
    for _ in range(5):
        ctx, r = env.step(agent.get_action(ctx))
        agent.regret.append(agent.regret[-1] + 1 - r)
    agent.learn({"obs": torch.randn(8, 24), "reward": torch.rand(8, 1)})
    agent.fitness.append(1.5)
    for mutate in (False, True):
        if mutate:
            muts = Mutations(no_mutation=0, architecture=1, new_layer_prob=0.5, parameters=0, activation=0, rl_hp=0,
                             rand_seed=1)
            agent = muts.mutation([agent])[0]
            agent.learn({"obs": torch.randn(8, 24), "reward": torch.rand(8, 1)})
        clone = agent.clone(7)
        assert clone.index == 7 and clone.algo == name
        _same_agent(agent, clone)
        if name == "NeuralTS":
            assert clone.noise_seed != agent.noise_seed  # a new index: its own noise
        path = str(tmp_path / f"{name}_{mutate}.pt")
        agent.save_checkpoint(path)
        loaded = cls.load(path, device="cpu")
        _same_agent(agent, loaded)
        assert loaded.fitness == agent.fitness and loaded.steps == agent.steps and loaded.index == agent.index
        fresh = cls(env.observation_space, env.action_space, device="cpu")
        fresh.load_checkpoint(path)
        _same_agent(agent, fresh)
        # the copies act as the original does
        a, b = agent.clone(), loaded
        assert a.get_action(ctx) == b.get_action(ctx) and torch.equal(a.sigma_inv, b.sigma_inv)


def test_create_population_for_both_names():
    from agilerl_amd.hpo.registry import HyperparameterConfig, RLParameter
    from agilerl_amd.utils import create_population

    env = _env()
    hp = HyperparameterConfig(lr=RLParameter(min=1e-4, max=1e-2))
    INIT_HP = {"GAMMA": 0.5, "LAMBDA": 2.0, "REG": 0.001, "BATCH_SIZE": 16, "LR": 2e-3, "LEARN_STEP": 3}
    for algo, default_lr in (("NeuralUCB", 1e-3), ("NeuralTS", 3e-3)):
        pop = create_population(algo, None, INIT_HP, env.observation_space, env.action_space, hp_config=hp,
                                population_size=3, device="cpu")
        assert [a.index for a in pop] == [0, 1, 2] and all(a.algo == algo for a in pop)
        for a in pop:
            assert (a.gamma, a.lamb, a.reg, a.batch_size, a.lr, a.learn_step) == (0.5, 2.0, 0.001, 16, 2e-3, 3)
            assert torch.equal(a.sigma_inv, 2.0 * torch.eye(33)) and a.regret == [0] and a.registry.hp_config is hp
        assert create_population(algo, None, {}, env.observation_space, env.action_space, device="cpu")[0].lr == default_lr


# ---- the envs ----------------------------------------------------------------------------------------
def test_bandit_env_matches_reference_outputs(golden):
    import pandas as pd

    from agilerl_amd.wrappers import BanditEnv

    g = golden("bandit_env")
    for features, targets in ((g["features"], g["targets"]), (pd.DataFrame(g["features"]), pd.DataFrame(g["targets"]))):
        env = BanditEnv(features, targets)
        assert env.arms == int(g["n_arms"]) and env.context_dim == (int(g["context_dim"]),)
        random.seed(int(g["seed"]))
        contexts, rewards = [env.reset()], []
        for k in g["arms"]:
            ctx, r = env.step(int(k))
            contexts.append(ctx)
            rewards.append(r)
        np.testing.assert_array_equal(np.stack(contexts), g["contexts"])
        np.testing.assert_array_equal(np.asarray(rewards), g["rewards"])
    import agilerl_amd.wrappers.learning as L

    assert "pandas" not in vars(L) and "pd" not in vars(L)


def test_synthetic_bandit_env_is_seeded_and_learnable():
    a, b, c = _env(seed=9), _env(seed=9), _env(seed=10)
    ca, cb = a.reset(), b.reset()
    assert ca.shape == (4, 24) and ca.dtype == np.float32 and np.array_equal(ca, cb)
    assert not np.array_equal(ca, c.reset())
    state = np.random.get_state()[1].copy()
    for _ in range(20):
        row = ca[0, :6]
        for k in range(4):  # BanditEnv's layout: block k of row k
            want = np.zeros(24, np.float32)
            want[6 * k:6 * k + 6] = row
            assert np.array_equal(ca[k], want)
        target = int(np.argmax(a._w @ row.astype(np.float64)))  # a fixed function of the context
        ca, r = a.step(target)
        assert r == 1.0
        cb, r = b.step((target + 1) % 4)
        assert r == 0.0 and np.array_equal(ca, cb)
    assert np.array_equal(np.random.get_state()[1], state)  # nothing drawn from the global generator


# ---- the trainer ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["NeuralUCB", "NeuralTS"])
def test_train_bandits_cpu(algo, tmp_path):
    from agilerl_amd.components import ReplayBuffer
    from agilerl_amd.hpo.mutation import Mutations
    from agilerl_amd.hpo.registry import HyperparameterConfig, RLParameter
    from agilerl_amd.hpo.tournament import TournamentSelection
    from agilerl_amd.training import train_bandits
    from agilerl_amd.utils import create_population

    env = _env(arms=4, features=6)
    hp = HyperparameterConfig(lr=RLParameter(min=1e-4, max=1e-2), batch_size=RLParameter(min=8, max=32, dtype=int),
                              learn_step=RLParameter(min=1, max=4, dtype=int))
    np.random.seed(0)
    torch.manual_seed(0)
    pop = create_population(algo, None, {"BATCH_SIZE": 8}, env.observation_space, env.action_space, hp_config=hp,
                            population_size=2, device="cpu")
    memory = ReplayBuffer(500, device="cpu")
    muts = Mutations(no_mutation=0.1, architecture=0.3, new_layer_prob=0.2, parameters=0.3, activation=0, rl_hp=0.3,
                     rand_seed=1)
    ckpt = str(tmp_path / "pop")
    pop, fits = train_bandits(env, "synthetic", algo, pop, memory, max_steps=64, episode_steps=16, evo_steps=32,
                              eval_steps=8, eval_loop=1, tournament=TournamentSelection(2, True, 2, 1), mutation=muts,
                              checkpoint=32, checkpoint_path=ckpt, save_elite=True, elite_path=str(tmp_path / "elite"),
                              verbose=False)
    assert len(pop) == 2 and len(fits) == 4 and all(len(f) == 2 and np.isfinite(f).all() for f in fits)
    assert len(memory) == 2 * 64 and memory.storage["obs"].shape[1:] == (24,)  # context[action], not the context
    for agent in pop:
        assert agent.steps[-1] == 64 and len(agent.regret) == 1 + 64 and len(agent.scores) == 4
        assert all(0 <= b - a <= 1 for a, b in zip(agent.regret, agent.regret[1:]))
        assert agent.sigma_inv.shape == (agent.numel, agent.numel) and torch.isfinite(agent.sigma_inv).all()
        assert all(torch.isfinite(p).all() for p in agent.actor.parameters())
    files = sorted(os.path.basename(f) for f in glob.glob(ckpt + "_*.pt"))
    assert files == ["pop_0_32.pt", "pop_0_64.pt", "pop_1_32.pt", "pop_1_64.pt"]
    assert os.path.exists(str(tmp_path / "elite.pt"))
    from agilerl_amd import algorithms

    loaded = getattr(algorithms, algo).load(f"{ckpt}_0_64.pt", device="cpu")
    assert torch.equal(loaded.sigma_inv, pop[0].sigma_inv) and list(loaded.regret) == [float(x) for x in pop[0].regret]
