"""DDPG / TD3 without a GPU: the plain-torch twin (tests/td3_twin.py) pinned
to the reference's own TD3.learn / DDPG.learn outputs, the agents' mutation
hooks, exploration noise, the continuous synthetic env, and the argument
checks of the two libagx entry points (no launch)."""

import numpy as np
import pytest
import torch

from tests import td3_twin

TD3_CASES = ["td3_0", "td3_1", "td3_2"]
DDPG_CASES = ["ddpg_0", "ddpg_1"]


@pytest.mark.parametrize("case", TD3_CASES + DDPG_CASES)
def test_twin_matches_reference_golden(golden, case):
    """next_actions and y bit for bit; dL/dQ and the loss to f32 rounding."""
    g = golden(case)
    t = lambda k: torch.from_numpy(g[k])  # noqa: E731
    twin = "q2" in g
    na = td3_twin.smooth(t("mu"), t("noise"), t("low"), t("high"), float(g["noise_clip"]))
    np.testing.assert_array_equal(na.numpy(), g["next_actions"])
    q = [t(k).requires_grad_() for k in (("q1", "q2") if twin else ("q1",))]
    qn = [t(k) for k in (("qn1", "qn2") if twin else ("qn1",))]
    y, loss = td3_twin.critic_target(q, qn, t("r"), t("d"), float(g["gamma"]))
    np.testing.assert_array_equal(y.detach().numpy(), g["y"])
    loss.backward()
    for k, qk in enumerate(q):
        np.testing.assert_allclose(qk.grad.numpy(), g[f"g_q{k + 1}"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(loss.item(), float(g["critic_loss"]), rtol=1e-6, atol=0)


def _env(num_envs=4):
    from agilerl_amd.envs import SyntheticVecEnv

    return SyntheticVecEnv(num_envs, action_dim=3, action_low=-2.0, action_high=0.5)


def _agent(algo, env, **kw):
    from agilerl_amd import algorithms

    return getattr(algorithms, algo)(env.single_observation_space, env.single_action_space,
                                     vect_noise_dim=env.num_envs, device="cpu", **kw)


def _optimizers(agent):
    return [getattr(agent, t[2]) for t in agent._triples()]


@pytest.mark.parametrize("algo", ["DDPG", "TD3"])
def test_architecture_mutation_keeps_networks_in_step(algo):
    from agilerl_amd.algorithms.ddpg import _arch
    from agilerl_amd.hpo.mutation import Mutations

    agent = _agent(algo, _env())
    mutations = Mutations(0, 1.0, 0.5, 0, 0, 0, rand_seed=3)
    evals = [t[0] for t in agent._triples()]
    seen = set()
    for _ in range(6):
        shapes = {n: _arch(getattr(agent, n)) for n in evals}
        old_opts = _optimizers(agent)
        calls = []
        for n, opt in zip(evals, old_opts):
            net = getattr(agent, n)
            opt.state[next(net.parameters())]["step"] = torch.tensor(7.0)  # state for the old optimizers to lose
            net.__dict__.pop("apply_mutation_dict", None)

            def spy(method, mut_dict=None, _net=net, _n=n):
                out = type(_net).apply_mutation_dict(_net, method, mut_dict)
                calls.append((_n, method, mut_dict, out))
                return out

            net.apply_mutation_dict = spy
        [agent] = mutations.mutation([agent])
        # the actor first, then every critic with the method the actor applied and its mutation dict
        assert [c[0] for c in calls] == evals
        applied, mut_dict = calls[0][3]
        assert applied is not None and agent.mut == applied
        for _, method, given, out in calls[1:]:
            assert method == applied and given == mut_dict and out[0] == applied
        seen.add(applied)
        assert any(_arch(getattr(agent, n)) != shapes[n] for n in evals) or "remove" in applied
        for net, target, opt in agent._triples():
            eval_sd, target_sd = getattr(agent, net).state_dict(), getattr(agent, target).state_dict()
            assert list(eval_sd) == list(target_sd) and all(torch.equal(eval_sd[k], target_sd[k]) for k in eval_sd)
            fresh = getattr(agent, opt)
            assert all(fresh is not o for o in old_opts) and len(fresh.state) == 0
            params = list(getattr(agent, net).parameters())
            assert [id(p) for p in fresh.param_groups[0]["params"]] == [id(p) for p in params]
    assert len(seen) > 1


def test_lr_critic_mutation_remakes_both_critic_optimizers():
    from agilerl_amd.hpo.mutation import Mutations
    from agilerl_amd.hpo.registry import HyperparameterConfig, RLParameter

    hp = HyperparameterConfig(lr_critic=RLParameter(min=1e-4, max=1e-2))
    agent = _agent("TD3", _env(), hp_config=hp)
    actor_opt, c1, c2 = _optimizers(agent)
    p = next(agent.actor.parameters())
    actor_opt.state[p]["exp_avg"] = torch.ones_like(p)
    [agent] = Mutations(0, 0, 0.5, 0, 0, 1.0, rand_seed=1).mutation([agent])
    assert agent.mut == "lr_critic"
    assert agent.actor_optimizer is actor_opt and torch.equal(actor_opt.state[p]["exp_avg"], torch.ones_like(p))
    assert agent.critic_1_optimizer is not c1 and agent.critic_2_optimizer is not c2
    for opt, net in ((agent.critic_1_optimizer, agent.critic_1), (agent.critic_2_optimizer, agent.critic_2)):
        assert opt.param_groups[0]["lr"] == agent.lr_critic and len(opt.state) == 0
        assert [id(q) for q in opt.param_groups[0]["params"]] == [id(q) for q in net.parameters()]


def _reference_noise(state, O_U_noise, theta, dt, n, A):
    """td3.py:430-452 on ``state`` = dict(current_noise, mean_noise, expl_noise)."""
    if O_U_noise:
        noise = (state["current_noise"] + theta * (state["mean_noise"] - state["current_noise"]) * dt
                 + state["expl_noise"] * np.sqrt(dt) * np.random.normal(size=(n, A)))
        state["current_noise"] = noise
    else:
        noise = np.random.normal(state["mean_noise"], state["expl_noise"], size=(n, A))
    return noise.astype(np.float32)


@pytest.mark.parametrize("algo", ["DDPG", "TD3"])
@pytest.mark.parametrize("O_U_noise", [True, False])
def test_get_action_training_noise_matches_reference_formula(algo, O_U_noise):
    env = _env()
    agent = _agent(algo, env, O_U_noise=O_U_noise, expl_noise=0.3, mean_noise=0.05)
    n, A = env.num_envs, 3
    obs = [env.reset()[0]] + [env.step(None)[0] for _ in range(2)]
    with torch.no_grad():
        agent.actor.eval()
        mu = [agent.actor(torch.from_numpy(o)).numpy() for o in obs]
        agent.actor.train()
    np.random.seed(11)
    got = []
    for k, o in enumerate(obs):
        got.append(agent.get_action(o, training=True))
        if k == 0:
            agent.reset_action_noise([1])
    np.random.seed(11)
    state = dict(current_noise=np.zeros((n, A)), mean_noise=0.05 * np.ones((n, A)), expl_noise=0.3 * np.ones((n, A)))
    for k in range(3):
        want = (mu[k] + _reference_noise(state, O_U_noise, 0.15, 1e-2, n, A)).clip(-1, 1)
        np.testing.assert_array_equal(got[k], want)
        assert got[k].dtype == np.float32 and got[k].shape == (n, A)
        if k == 0:
            state["current_noise"][[1]] = state["mean_noise"][[1]]
    assert isinstance(agent.current_noise, np.ndarray) and isinstance(agent.expl_noise, np.ndarray)


@pytest.mark.parametrize("algo", ["DDPG", "TD3"])
def test_get_action_eval_lies_in_bounds(algo):
    env = _env()
    agent = _agent(algo, env)
    action = agent.get_action(env.reset()[0], training=False)
    assert action.shape == (env.num_envs, 3) and action.dtype == np.float32
    assert (action >= -2.0).all() and (action <= 0.5).all()


def test_synthetic_env_action_spaces():
    from agilerl_amd.envs import Box, Discrete, SyntheticVecEnv

    env = SyntheticVecEnv(2, action_dim=3)
    space = env.single_action_space
    assert isinstance(space, Box) and space.shape == (3,) and env.action_space is space
    assert (space.low == -1).all() and (space.high == 1).all() and space.low.dtype == np.float32
    space = SyntheticVecEnv(2, action_dim=2, action_low=-2.0, action_high=0.5).single_action_space
    assert (space.low == -2).all() and (space.high == 0.5).all()
    env = SyntheticVecEnv(2)
    assert isinstance(env.single_action_space, Discrete) and env.single_action_space.n == 4
    obs, rew, term, trunc, _ = SyntheticVecEnv(2, action_dim=3).step(np.zeros((2, 3), np.float32))
    assert obs.shape == (2, 8) and rew.shape == (2,)


def test_out_of_scope_arguments_raise():
    env = _env()
    for kw in (dict(share_encoders=True), dict(actor_network=torch.nn.Linear(8, 3))):
        with pytest.raises(NotImplementedError):
            _agent("TD3", env, **kw)
    from agilerl_amd.algorithms import DDPG
    from agilerl_amd.envs import Box, Discrete

    with pytest.raises(NotImplementedError):
        DDPG(Box(0, 1, (4, 8, 8)), env.single_action_space, device="cpu")
    with pytest.raises(AssertionError, match="DDPG only supports continuous action spaces."):
        DDPG(env.single_observation_space, Discrete(3), device="cpu")


def test_clone_and_checkpoint_round_trip_on_cpu(tmp_path):
    from agilerl_amd.hpo.mutation import Mutations

    env = _env()
    agent = _agent("TD3", env)
    [agent] = Mutations(0, 1.0, 0.5, 0, 0, 0, rand_seed=5).mutation([agent])  # a checkpoint of a mutated shape
    agent.fitness, agent.steps, agent.learn_counter = [1.5], [0, 40], 3
    clone = agent.clone(index=9)
    assert clone.index == 9 and clone.actor is not agent.actor
    path = str(tmp_path / "td3.pt")
    agent.save_checkpoint(path)
    other = _agent("TD3", env)
    other.load_checkpoint(path)
    for net, target, _ in agent._triples():
        for n in (net, target):
            a, b = getattr(agent, n).state_dict(), getattr(other, n).state_dict()
            assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert (other.fitness, other.steps, other.learn_counter, other.mut) == ([1.5], [0, 40], 3, agent.mut)
    with pytest.raises(ValueError):
        _agent("DDPG", env).load_checkpoint(path)


# ---- the two entry points' argument checks: status codes without a launch ------
@pytest.fixture(scope="module")
def lib():
    import os

    from agilerl_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load(require_gpu=False)


def test_td3_entry_points_check_arguments_before_any_launch(lib):
    one = 0x1000  # a non-NULL pointer that is never dereferenced: every call returns before a launch
    ok = lambda *a: lib.agx_td3_critic_target(*a)  # noqa: E731
    # B == 0: AGX_OK
    assert lib.agx_td3_smooth_actions(one, one, one, one, 0, 3, 0.5, one, None) == 0
    assert ok(one, one, one, one, one, one, 0, 0.99, None, None, None, one, one, None) == 0
    assert ok(one, None, one, None, one, one, 0, 0.99, None, None, None, one, one, None) == 0
    assert lib.agx_td3_workspace_bytes(0) == 0 and lib.agx_td3_workspace_bytes(257) == 2 * 2 * 8
    # bad arguments: AGX_EINVAL (-1) and a message
    assert ok(None, one, one, one, one, one, 4, 0.99, None, None, None, one, one, None) == -1
    assert b"agx_td3_critic_target" in lib.agx_last_error()
    assert ok(one, one, one, None, one, one, 4, 0.99, None, None, None, one, one, None) == -1
    assert b"go together" in lib.agx_last_error()
    assert ok(one, None, one, one, one, one, 4, 0.99, None, None, None, one, one, None) == -1
    assert ok(one, None, one, None, one, one, 4, 0.99, None, None, one, one, one, None) == -1  # g_q2 without q2
    assert ok(one, one, one, one, one, one, -1, 0.99, None, None, None, one, one, None) == -1
    assert lib.agx_td3_smooth_actions(None, one, one, one, 4, 3, 0.5, one, None) == -1
    assert lib.agx_td3_smooth_actions(one, one, one, one, 4, 0, 0.5, one, None) == -1
    assert b"agx_td3_smooth_actions" in lib.agx_last_error()
