"""CQN / train_offline without a GPU: the float64 twin (tests/cqn_twin.py)
pinned to the reference's own CQN.learn outputs (tests/golden/cqn_*.npz), the
replay fill of train_offline, its argument handling, the agent's constructor
keys and the argument checks of agx_cqn_loss (no launch)."""

import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests import cqn_twin

CASES = [f"cqn_{k}" for k in range(6)]
META = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "META_cqn.json")))

# Two float64 evaluations of one formula (the generator's torch ops, the twin's
# numpy ops) differ by float64 rounding, nine orders below the float32 errors
# recorded as err_ref: this is added so that the element that attains err_ref
# cannot miss by that rounding (without it the loss of cqn_2 misses its
# 3.6e-7 by 1.8e-15, one float64 ulp of the loss).
F64_SLACK = 1e-13


def _twin(g):
    return cqn_twin.cqn_loss_twin(g["q_next_online"], g["q_next_target"], g["q_cur"], g["a"], g["r"], g["d"],
                                  float(g["gamma"]), bool(g["double"]))


@pytest.mark.parametrize("case", CASES)
def test_twin_matches_reference_golden(golden, case):
    """y bit for bit; the float64 loss, terms and gradient within the
    reference's own float32 error (both measure the same f32-vs-f64 gap)."""
    g, err = golden(case), META["errors"][case]
    assert META["shapes"][case] == [g["q_cur"].shape[0], g["q_cur"].shape[1], bool(g["double"])]
    t = _twin(g)
    np.testing.assert_array_equal(t["y"], g["y"])
    scale = lambda v: F64_SLACK * max(1.0, abs(float(v)))  # noqa: E731
    assert abs(t["loss"] - float(g["loss"])) <= err["err_ref_loss"] + scale(t["loss"])
    for k in range(3):
        assert abs(t["terms"][k] - float(g["terms"][k])) <= err["err_ref_terms"][k] + scale(t["terms"][k]), k
    assert np.max(np.abs(t["grad"] - g["g_q"].astype(np.float64))) <= err["err_ref_grad"] + F64_SLACK


def test_golden_cases_are_the_issue_list():
    assert [tuple(META["shapes"][c]) for c in CASES] == [(1, 1, False), (33, 2, True), (64, 4, False),
                                                         (257, 6, True), (64, 33, False), (1024, 6, True)]
    assert sorted(META["groups"]) == sorted(CASES + ["cqn_nan"])


def test_twin_nan_pattern_matches_reference_golden(golden):
    g = golden("cqn_nan")
    t = _twin(g)
    np.testing.assert_array_equal(np.isnan(t["y"]), np.isnan(g["y"]))
    np.testing.assert_array_equal(np.isnan(t["grad"]), np.isnan(g["g_q"]))
    assert np.isnan(g["y"]).sum() == 1 and np.isnan(g["g_q"]).all(axis=1).sum() == 1
    assert np.isnan(t["loss"]) and np.isnan(float(g["loss"]))
    ok = ~np.isnan(g["y"])
    np.testing.assert_array_equal(t["y"][ok], g["y"][ok])


@pytest.mark.parametrize("B,A,double", [(1, 1, False), (33, 7, True), (64, 33, False), (257, 100, True)])
def test_twin_gradient_rows_sum_to_the_td_term(B, A, double):
    """softmax sums to 1 and the -1/(BA) terms to -1/B: a row of the gradient
    sums to (Q[a] - y) / B.  A dropped term shows here."""
    rec = cqn_twin.inputs(B, A)
    t = cqn_twin.cqn_loss_twin(**rec, double=double)
    qa = rec["q_cur"].astype(np.float64)[np.arange(B), rec["actions"]]
    want = (qa - t["y"].reshape(B).astype(np.float64)) / B
    np.testing.assert_allclose(t["grad"].sum(axis=1), want, rtol=0, atol=1e-14 * A)
    # and the float32 torch evaluation agrees with the twin to float32 rounding
    t32 = cqn_twin.cqn_loss_torch32(**rec, double=double)
    np.testing.assert_array_equal(t32["y"], t["y"])
    np.testing.assert_allclose(t32["grad"], t["grad"], rtol=0, atol=1e-6)
    assert abs(t32["loss"] - t["loss"]) <= 1e-5


def test_twin_one_action_and_infinite_rows():
    """A == 1: lse = Q exactly; an infinite row maximum shifts by 0."""
    rec = cqn_twin.inputs(5, 1)
    t = cqn_twin.cqn_loss_twin(**rec, double=False)
    np.testing.assert_array_equal(t["lse"], rec["q_cur"].astype(np.float64).reshape(5))
    rec = cqn_twin.inputs(4, 3)
    rec["q_cur"][1] = (-np.inf, 0.5, -np.inf)
    t = cqn_twin.cqn_loss_twin(**rec, double=False)
    assert t["lse"][1] == 0.5
    rec["q_cur"][1] = (np.inf, 0.5, 1.0)  # shifting by the maximum would give inf - inf
    t = cqn_twin.cqn_loss_twin(**rec, double=False)
    assert t["lse"][1] == np.inf


# ---- train_offline's fill ---------------------------------------------------------
def _dataset(n=50, obs_dim=3, n_actions=4, seed=0):
    rng = np.random.default_rng(seed)
    return {"observations": rng.standard_normal((n, obs_dim)).astype(np.float32),
            "actions": rng.integers(0, n_actions, n), "rewards": rng.standard_normal(n),
            "terminals": rng.random(n) < 0.2}


def _row_by_row(ds, max_size):
    """What the reference's fill (train_offline.py:177-201) leaves in a ring of max_size rows."""
    n = ds["rewards"].shape[0] - 1
    ring = {}
    for i in range(n):
        ring[i % max_size] = (ds["observations"][i], int(ds["actions"][i]), np.float32(ds["rewards"][i]),
                              ds["observations"][i + 1], float(bool(ds["terminals"][i])))
    return ring, n


class _H5Like:
    """A dataset object that only answers ``[...]``, as an h5py dataset read whole."""

    def __init__(self, a):
        self.a = a

    def __getitem__(self, key):
        assert key is Ellipsis
        return self.a


@pytest.mark.parametrize("max_size", [100, 20])
@pytest.mark.parametrize("h5", [False, True])
def test_fill_matches_row_by_row_fill(max_size, h5):
    from agilerl_amd.components import ReplayBuffer
    from agilerl_amd.training.train_offline import fill_memory

    ds = _dataset()
    memory = ReplayBuffer(max_size, device="cpu")
    calls = []
    add = memory.add
    memory.add = lambda data: (calls.append(1), add(data))[1]
    n = fill_memory(memory, {k: _H5Like(v) for k, v in ds.items()} if h5 else ds, 4)
    ring, want_n = _row_by_row(ds, max_size)
    assert n == want_n == 49 and len(memory) == min(49, max_size) and memory.counter == 49
    assert 1 <= len(calls) <= 4
    st = memory.storage
    assert st["action"].dtype == torch.int64 and st["obs"].dtype == torch.float32
    assert st["reward"].shape == (max_size, 1) and st["done"].shape == (max_size, 1)
    for slot, (o, a, r, no, d) in ring.items():
        np.testing.assert_array_equal(st["obs"][slot].numpy(), o)
        np.testing.assert_array_equal(st["next_obs"][slot].numpy(), no)
        assert int(st["action"][slot]) == a and float(st["reward"][slot]) == r and float(st["done"][slot]) == d
    assert memory._cursor == 49 % max_size


def test_fill_refuses_actions_outside_the_space():
    from agilerl_amd.components import ReplayBuffer
    from agilerl_amd.training.train_offline import fill_memory

    for bad in (4, -1, 1.5):
        ds = _dataset()
        ds["actions"] = ds["actions"].astype(np.float64)
        ds["actions"][7] = bad
        memory = ReplayBuffer(100, device="cpu")
        with pytest.raises(ValueError, match=r"integers in \[0, 4\)"):
            fill_memory(memory, ds, 4)
        assert len(memory) == 0
    ds = _dataset()
    ds["actions"][48] = 3  # the largest legal action, in the last row that is used
    ds["actions"][49] = 9  # the last row pairs with nothing: not read
    fill_memory(ReplayBuffer(100, device="cpu"), ds, 4)


class _Agent:
    """The least train_offline touches before its loop."""
    action_dim, device, batch_size, steps = 4, torch.device("cpu"), 8, [10]


def test_train_offline_refuses_what_it_does_not_do():
    from agilerl_amd.components import ReplayBuffer
    from agilerl_amd.training import train_offline

    ds = _dataset()
    with pytest.raises(NotImplementedError, match="minari"):
        train_offline(None, "env", None, "CQN", [_Agent()], ReplayBuffer(100, device="cpu"), minari_dataset_id="x/y-v0")
    with pytest.raises(NotImplementedError, match="swap_channels"):
        train_offline(None, "env", ds, "CQN", [_Agent()], ReplayBuffer(100, device="cpu"), swap_channels=True)


def test_train_offline_argument_warnings():
    """The reference's two inconsistent-argument warnings; max_steps already
    reached, so the call fills the buffer and returns."""
    from agilerl_amd.components import ReplayBuffer
    from agilerl_amd.training import train_offline

    ds = _dataset()
    memory = ReplayBuffer(100, device="cpu")
    with pytest.warns(UserWarning) as rec:
        pop, fits = train_offline(None, "env", ds, "CQN", [_Agent()], memory, max_steps=10, save_elite=False,
                                  elite_path="elite", checkpoint=None, checkpoint_path="ckpt", verbose=False)
    msgs = [str(w.message) for w in rec]
    assert any("'save_elite' set to False but 'elite_path'" in m for m in msgs)
    assert any("'checkpoint' set to None but 'checkpoint_path'" in m for m in msgs)
    assert fits == [] and len(pop) == 1 and len(memory) == 49
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        train_offline(None, "env", ds, "CQN", [_Agent()], ReplayBuffer(100, device="cpu"), max_steps=10,
                      verbose=False)


# ---- the agent -----------------------------------------------------------------------
def _spaces():
    from agilerl_amd.envs import SyntheticVecEnv

    env = SyntheticVecEnv(2)
    return env.single_observation_space, env.single_action_space


def test_create_population_and_from_init_hp_keys():
    from agilerl_amd.algorithms import CQN, DQN
    from agilerl_amd.utils import create_population

    obs, act = _spaces()
    INIT_HP = {"BATCH_SIZE": 32, "LR": 3e-4, "LEARN_STEP": 2, "GAMMA": 0.9, "TAU": 0.01, "DOUBLE": True}
    pop = create_population("CQN", None, INIT_HP, obs, act, population_size=3, device="cpu")
    assert [a.index for a in pop] == [0, 1, 2] and all(type(a) is CQN and a.algo == "CQN" for a in pop)
    a = pop[1]
    assert (a.batch_size, a.lr, a.learn_step, a.gamma, a.tau, a.double) == (32, 3e-4, 2, 0.9, 0.01, True)
    d = CQN(obs, act, device="cpu")  # the reference's defaults (cqn.py:57-76)
    assert (d.batch_size, d.lr, d.learn_step, d.gamma, d.tau, d.double, d.index) == (64, 1e-4, 5, 0.99, 1e-3, False, 0)
    assert d.get_lr_names() == ["lr"] and d.can_mutate_architecture
    assert not isinstance(d, DQN) and CQN.get_action is DQN.get_action and CQN.test is DQN.test
    with pytest.raises(NotImplementedError):
        CQN(obs, act, device="cpu", actor_network=torch.nn.Linear(8, 4))
    action = d.get_action(np.zeros((5, 8), np.float32))
    assert action.shape == (5,) and (0 <= action).all() and (action < 4).all()


def test_mutations_apply_to_cqn(tmp_path):
    from agilerl_amd.algorithms import CQN
    from agilerl_amd.hpo.mutation import Mutations

    obs, act = _spaces()
    agent = CQN(obs, act, device="cpu")
    before = agent.actor.activation
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # "not supported for ..." would be a warning
        [agent] = Mutations(0, 0, 0.5, 0, 1.0, 0, rand_seed=2).mutation([agent])
    assert agent.mut == "act" and agent.actor.activation != before
    assert agent.actor_target.activation == agent.actor.activation
    agent.fitness, agent.steps = [2.5], [0, 16]
    path = str(tmp_path / "cqn.pt")
    agent.save_checkpoint(path)
    other = CQN(obs, act, device="cpu")
    other.load_checkpoint(path)
    sd, osd = agent.actor.state_dict(), other.actor.state_dict()
    assert list(osd) == list(sd) and all(torch.equal(osd[k], sd[k]) for k in sd)
    assert (other.fitness, other.steps, other.mut) == ([2.5], [0, 16], "act")
    [agent] = Mutations(0, 1.0, 0.5, 0, 0, 0, rand_seed=3).mutation([agent])
    sd, tsd = agent.actor.state_dict(), agent.actor_target.state_dict()
    assert agent.mut not in ("act", "None") and list(sd) == list(tsd) and all(torch.equal(sd[k], tsd[k]) for k in sd)
    assert len(agent.optimizer.state) == 0
    assert [id(p) for p in agent.optimizer.param_groups[0]["params"]] == [id(p) for p in agent.actor.parameters()]


# ---- the entry point's argument checks: status codes without a launch ------------------
@pytest.fixture(scope="module")
def lib():
    from agilerl_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load(require_gpu=False)


def test_cqn_entry_point_checks_arguments_before_any_launch(lib):
    one = 0x1000  # a non-NULL pointer that is never dereferenced: every call returns before a launch
    call = lambda *a: lib.agx_cqn_loss(*a)  # noqa: E731
    # B == 0: AGX_OK
    assert call(None, one, one, one, one, one, 0, 4, 0.99, 0, one, one, one, None, one, None) == 0
    assert call(one, one, one, one, one, one, 0, 33, 0.99, 1, one, one, one, one, one, None) == 0
    assert lib.agx_cqn_workspace_bytes(0, 4) == 0
    assert lib.agx_cqn_workspace_bytes(257, 32) == 2 * 3 * 8    # row per lane: 256 rows a block
    assert lib.agx_cqn_workspace_bytes(257, 33) == 65 * 3 * 8   # row per wave: 4 rows a block
    assert lib.agx_cqn_workspace_bytes(1 << 20, 64) == 4096 * 3 * 8  # its grid is capped
    # bad arguments: AGX_EINVAL (-1) and a message
    assert call(None, None, one, one, one, one, 4, 4, 0.99, 0, one, one, one, None, one, None) == -1
    assert b"agx_cqn_loss" in lib.agx_last_error()
    assert call(None, one, one, one, one, one, 4, 4, 0.99, 1, one, one, one, None, one, None) == -1
    assert b"double_q" in lib.agx_last_error()
    assert call(None, one, one, one, one, one, 4, 4, 0.99, 0, one, None, one, None, one, None) == -1  # no g_q
    assert call(None, one, one, one, one, one, 4, 4, 0.99, 0, one, one, one, None, None, None) == -1  # no workspace
    assert call(None, one, one, one, one, one, -1, 4, 0.99, 0, one, one, one, None, one, None) == -1
    assert call(None, one, one, one, one, one, 4, 0, 0.99, 0, one, one, one, None, one, None) == -1
    assert call(None, one, one, one, one, one, 4, 65536, 0.99, 0, one, one, one, None, one, None) == -1
