"""CQN on the GPU: agx_cqn_loss against the reference's own outputs
(tests/golden/cqn_*.npz) and the float64 twin (tests/cqn_twin.py) at the
shapes where its two forms can go wrong, CQN.learn — eager, captured and
replayed — against the twin's plain-torch update on copies of the same
networks, and train_offline with tournament, mutations, checkpoints, the
elite file and clones.

The bound on every float32 result is 4 x max(err_ref, 1 float32 ulp of the
value), err_ref being the error of the reference's own float32 evaluation
against float64 on the same inputs (recorded in META_cqn.json for the golden
cases, computed here from torch's CPU ops for the others): the device's expf /
logf may be 2-ulp functions where the CPU's are 1-ulp ones, chained through
exp, sum and log.  A wrong or missing term is orders of magnitude larger."""

import json
import os

import numpy as np
import pytest
import torch

from tests import cqn_twin

pytestmark = pytest.mark.gpu

CASES = [f"cqn_{k}" for k in range(6)]
META = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "META_cqn.json")))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ulp(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def _bound(err_ref, value):
    return 4.0 * np.maximum(err_ref, _ulp(value))


def _call(rec, double, with_terms=True):
    from agilerl_amd import kernels as K

    return K.cqn_loss(_dev(rec["q_cur"]), _dev(rec["q_next_target"]), _dev(rec["actions"]), _dev(rec["rewards"]),
                      _dev(rec["dones"]), float(rec["gamma"]), q_next_online=_dev(rec["q_next_online"]),
                      double=double, with_terms=with_terms)


def _td_y(rec, double):
    from agilerl_amd import kernels as K

    y, _, _ = K.td_target(_dev(rec["q_next_target"]), _dev(rec["rewards"]), _dev(rec["dones"]), float(rec["gamma"]),
                          q_next_online=_dev(rec["q_next_online"]), double=double, with_loss=False)
    return y


def _check(tag, out, twin, err_loss, err_terms, err_grad):
    """Print each figure, then hold it to its bound."""
    y, g_q, loss, terms = (t.cpu().numpy() for t in out)
    d_loss = abs(float(loss[0]) - twin["loss"])
    d_terms = np.abs(terms.astype(np.float64) - twin["terms"])
    d_grad = np.abs(g_q.astype(np.float64) - twin["grad"])
    b_loss, b_terms, b_grad = _bound(err_loss, twin["loss"]), _bound(np.asarray(err_terms), twin["terms"]), \
        _bound(err_grad, twin["grad"])
    print(f"{tag}: loss err {d_loss:.3e} (bound {float(b_loss):.3e}), terms err {d_terms} (bound {b_terms}), "
          f"grad max err {d_grad.max():.3e} (err_ref {err_grad:.3e}, worst err/bound {np.max(d_grad / b_grad):.3f})")
    np.testing.assert_array_equal(y, twin["y"])
    assert d_loss <= b_loss
    assert (d_terms <= b_terms).all()
    assert (d_grad <= b_grad).all()


def _golden_rec(g):
    return dict(q_next_online=g["q_next_online"], q_next_target=g["q_next_target"], q_cur=g["q_cur"],
                actions=g["a"].reshape(-1), rewards=g["r"].reshape(-1), dones=g["d"].reshape(-1),
                gamma=float(g["gamma"]))


# ---- agx_cqn_loss ---------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_kernel_matches_reference_golden(golden, case):
    g, err = golden(case), META["errors"][case]
    rec, double = _golden_rec(g), bool(g["double"])
    out = _call(rec, double)
    np.testing.assert_array_equal(out[0].cpu().numpy(), g["y"])
    assert torch.equal(out[0], _td_y(rec, double))
    twin = cqn_twin.cqn_loss_twin(**rec, double=double)
    _check(case, out, twin, err["err_ref_loss"], err["err_ref_terms"], err["err_ref_grad"])
    # the reference's float32 outputs lie within the same distance
    assert abs(float(out[2]) - float(g["loss"])) <= _bound(err["err_ref_loss"], twin["loss"]) + err["err_ref_loss"]


def test_kernel_nan_case_matches_reference_golden(golden):
    g = golden("cqn_nan")
    rec = _golden_rec(g)
    y, g_q, loss, terms = (t.cpu().numpy() for t in _call(rec, bool(g["double"])))
    np.testing.assert_array_equal(np.isnan(y), np.isnan(g["y"]))
    np.testing.assert_array_equal(y[~np.isnan(y)], g["y"][~np.isnan(g["y"])])
    np.testing.assert_array_equal(np.isnan(g_q), np.isnan(g["g_q"]))
    assert np.isnan(g_q).all(axis=1).sum() == 1  # the q_cur row with the NaN, whole
    assert np.isnan(loss[0]) and np.isnan(float(g["loss"]))
    assert np.isnan(terms).tolist() == np.isnan(g["terms"]).tolist()
    np.testing.assert_array_equal(_td_y(rec, bool(g["double"])).cpu().numpy(), y)


def _raw_call(q_cur, g_q, rec, double):
    """agx_cqn_loss on caller-made q_cur / g_q tensors -> (y, loss, terms)."""
    from agilerl_amd import _lib

    B, A = q_cur.shape
    y = torch.full((B, 1), float("nan"), device="cuda")
    loss, terms = torch.full((1,), float("nan"), device="cuda"), torch.full((3,), float("nan"), device="cuda")
    ws = torch.empty(max(16, _lib.load().agx_cqn_workspace_bytes(B, A)), dtype=torch.uint8, device="cuda")
    qno, qnt = _dev(rec["q_next_online"]), _dev(rec["q_next_target"])
    a, r, d = _dev(rec["actions"]), _dev(rec["rewards"]), _dev(rec["dones"])
    _lib.call("agx_cqn_loss", qno.data_ptr() if double else None, qnt.data_ptr(), q_cur.data_ptr(), a.data_ptr(),
              r.data_ptr(), d.data_ptr(), B, A, float(rec["gamma"]), int(double), y.data_ptr(), g_q.data_ptr(),
              loss.data_ptr(), terms.data_ptr(), ws.data_ptr(), _lib.stream())
    return y, loss, terms


@pytest.mark.parametrize("A", [1, 2, 7, 32, 33, 65, 100])
@pytest.mark.parametrize("B", [1, 33, 64, 257])
def test_kernel_matches_twin_formula(B, A):
    """A part-filled wave, a second block holding one row, an odd row stride,
    both sides of the switch between the two forms (A = 32 / 33) and a
    part-filled column pass; every element of g_q written; the same bits from
    tensors that are not 16-byte aligned (the scalar tile loads)."""
    rec = cqn_twin.inputs(B, A)
    for double in (False, True):
        twin = cqn_twin.cqn_loss_twin(**rec, double=double)
        ref32 = cqn_twin.cqn_loss_torch32(**rec, double=double)
        err_loss = abs(ref32["loss"] - twin["loss"])
        err_terms = np.abs(ref32["terms"] - twin["terms"])
        err_grad = float(np.max(np.abs(ref32["grad"].astype(np.float64) - twin["grad"])))
        out = _call(rec, double)
        _check(f"B={B} A={A} double={double}", out, twin, err_loss, err_terms, err_grad)
        assert torch.equal(out[0], _td_y(rec, double))
        # a sentinel under every element of g_q, in tensors one float off a 16-byte boundary
        q_buf = torch.empty(B * A + 1, device="cuda")
        g_buf = torch.full((B * A + 1,), float("nan"), device="cuda")
        q_cur, g_q = q_buf[1:].view(B, A), g_buf[1:].view(B, A)
        q_cur.copy_(_dev(rec["q_cur"]))
        assert q_cur.data_ptr() % 16 == 4 and g_q.data_ptr() % 16 == 4
        y, loss, terms = _raw_call(q_cur, g_q, rec, double)
        assert not torch.isnan(g_q).any() and torch.isnan(g_buf[0])
        assert torch.equal(g_q, out[1]) and torch.equal(y, out[0])
        assert torch.equal(loss, out[2]) and torch.equal(terms, out[3])


@pytest.mark.parametrize("A", [33, 65])
def test_q_next_ties_and_nan_follow_td_target(A):
    """The row-per-wave form's argmax / max reductions: two equal maxima (the
    first index wins under double), a NaN as the maximum, the first of two
    NaNs as the argmax — y bit-equal to agx_td_target's."""
    B = 12
    rec = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in cqn_twin.inputs(B, A, seed=5).items()}
    rec["dones"][:] = 0.0
    big = np.float32(50.0)
    for q in (rec["q_next_online"], rec["q_next_target"]):
        q[0, [3, A - 1]] = big           # a tie across lanes
        q[1, [A - 1, 0]] = big           # the second maximum in the last, part-filled column pass
        q[2, [0, 64] if A > 64 else [5, 31]] = big  # one lane's two column passes / two lanes
        q[3, 7] = np.nan                 # a NaN is the maximum
        q[4, [A - 2, 2]] = np.nan        # two NaNs: the first one's index
        q[5, [0, 1]] = (np.nan, big)
        q[6, :] = 1.25                   # all equal: index 0
        q[7, A - 1] = np.inf
    # the target values at the tied online maxima differ, so a wrong index shows in y
    rec["q_next_target"][0, 3], rec["q_next_target"][0, A - 1] = 1.0, 2.0
    rec["q_next_target"][1, 0], rec["q_next_target"][1, A - 1] = 3.0, 4.0
    rec["q_next_target"][4, 2], rec["q_next_target"][4, A - 2] = 5.0, 6.0
    for double in (False, True):
        y = _call(rec, double, with_terms=False)[0].cpu().numpy()
        np.testing.assert_array_equal(y, _td_y(rec, double).cpu().numpy())
        twin = cqn_twin.cqn_loss_twin(**rec, double=double)
        np.testing.assert_array_equal(y, twin["y"])
        if double:
            g = np.float32(rec["gamma"])
            assert y[0, 0] == rec["rewards"][0] + g * np.float32(1.0) and y[1, 0] == rec["rewards"][1] + g * np.float32(3.0)
            assert y[4, 0] == rec["rewards"][4] + g * np.float32(5.0)
        else:
            assert np.isnan(y[3, 0]) and np.isnan(y[5, 0]) and np.isinf(y[7, 0])


def test_two_calls_give_the_same_bits():
    rec = cqn_twin.inputs(257, 33)
    a, b = _call(rec, True), _call(rec, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_binding_checks_shapes_and_devices():
    from agilerl_amd import kernels as K

    rec = cqn_twin.inputs(8, 4)
    q, qt, a, r, d = (_dev(rec[k]) for k in ("q_cur", "q_next_target", "actions", "rewards", "dones"))
    with pytest.raises(ValueError):
        K.cqn_loss(q, qt[:, :3].contiguous(), a, r, d, 0.99)
    with pytest.raises(TypeError):
        K.cqn_loss(q, qt, a.int(), r, d, 0.99)
    with pytest.raises(ValueError):
        K.cqn_loss(q.cpu(), qt, a, r, d, 0.99)
    with pytest.raises(TypeError):
        K.cqn_loss(q, qt, a, r, d, 0.99, double=True)  # double needs q_next_online
    # B == 0: no launch, and the means of nothing are NaN (not uninitialised memory)
    y, g_q, loss, terms = K.cqn_loss(q[:0], qt[:0], a[:0], r[:0], d[:0], 0.99, with_terms=True)
    assert y.shape == (0, 1) and g_q.shape == (0, 4) and torch.isnan(loss).all() and torch.isnan(terms).all()


# ---- learn against the twin ---------------------------------------------------------
def _spaces():
    from agilerl_amd.envs import SyntheticVecEnv

    env = SyntheticVecEnv(2)
    return env.single_observation_space, env.single_action_space


def _batches(n, B=32, obs_dim=8, A=4, seed=0):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        out.append({"obs": torch.randn(B, obs_dim, generator=gen).cuda(),
                    "action": torch.randint(0, A, (B, 1), generator=gen).cuda(),
                    "reward": torch.randn(B, 1, generator=gen).cuda(),
                    "next_obs": torch.randn(B, obs_dim, generator=gen).cuda(),
                    "done": (torch.rand(B, 1, generator=gen) < 0.2).float().cuda()})
    return out


def _graphs(agent):
    from agilerl_amd.algorithms import learn_graph
    from agilerl_amd.algorithms.flat_state import flat_state

    table = learn_graph._GRAPHS.get(flat_state(agent), {})
    return [k for k, ent in table.items() if k[0] == "cqn" and ent.graph is not None]


@pytest.mark.parametrize("double", [False, True])
def test_learn_matches_twin(double, monkeypatch):
    from agilerl_amd.algorithms import CQN

    obs, act = _spaces()
    torch.manual_seed(0)
    agent = CQN(obs, act, batch_size=32, lr=1e-3, tau=0.01, double=double)
    eager = agent.clone()
    twin = cqn_twin.Twin.of(agent)
    batches = _batches(4)
    for k, experiences in enumerate(batches):
        loss = agent.learn(experiences)
        twin_loss = twin.learn(experiences)
        print(f"update {k}: loss {loss:.7f}, twin {twin_loss:.7f}")
        assert np.isfinite(loss) and abs(loss - twin_loss) <= 1e-4 * abs(twin_loss) + 2e-5
        # the first update of a shape is eager, the second captures, later ones replay
        assert len(_graphs(agent)) == (0 if k == 0 else 1)
    for net, ref in ((agent.actor, twin.actor), (agent.actor_target, twin.actor_target)):
        for p1, p2 in zip(net.parameters(), ref.parameters()):
            torch.testing.assert_close(p1, p2, rtol=1e-4, atol=2e-5)
    steps = {float(s["step"]) for s in agent.optimizer.state_dict()["state"].values()}
    assert steps == {4.0} and len(agent.optimizer.state_dict()["state"]) == len(list(agent.actor.parameters()))
    key = _graphs(agent)[0]
    assert key[:4] == ("cqn", double, 0.99, 0.01)

    monkeypatch.setenv("AGX_LEARN_GRAPH", "0")
    for experiences in batches:
        eager.learn(tuple(experiences[k] for k in ("obs", "action", "reward", "next_obs", "done")))  # the reference's tuple
    assert _graphs(eager) == []
    for net, ref in ((agent.actor, eager.actor), (agent.actor_target, eager.actor_target)):
        for p1, p2 in zip(net.parameters(), ref.parameters()):
            torch.testing.assert_close(p1, p2, rtol=1e-4, atol=2e-5)


# ---- the drop-in trainer ---------------------------------------------------------------
def _state_equal(a, b):
    return list(a) == list(b) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)


def _adam_equal(a, b):
    sa, sb = a.state_dict()["state"], b.state_dict()["state"]
    return list(sa) == list(sb) and all(
        float(sa[k]["step"]) == float(sb[k]["step"]) and torch.equal(sa[k]["exp_avg"].cpu(), sb[k]["exp_avg"].cpu())
        and torch.equal(sa[k]["exp_avg_sq"].cpu(), sb[k]["exp_avg_sq"].cpu()) for k in sa)


def _matches_file(agent, path):
    """Every network tensor and Adam moment of ``agent`` equals the file's."""
    info = torch.load(path, map_location="cpu", weights_only=True)["network_info"]
    for n in ("actor", "actor_target"):
        assert _state_equal(getattr(agent, n).state_dict(), info["modules"][f"{n}_state_dict"]), n
    want, got = info["optimizers"]["optimizer_state_dict"]["state"], agent.optimizer.state_dict()["state"]
    assert list(want) == list(got)
    for k in want:
        assert float(want[k]["step"]) == float(got[k]["step"])
        assert torch.equal(want[k]["exp_avg"], got[k]["exp_avg"].cpu())
        assert torch.equal(want[k]["exp_avg_sq"], got[k]["exp_avg_sq"].cpu())


def _offline_dataset(rows=600):
    from agilerl_amd.envs import SyntheticVecEnv

    env = SyntheticVecEnv(1, seed=11, p_done=0.05)
    rng = np.random.default_rng(2)
    obs, _ = env.reset()
    ds = {"observations": [], "actions": [], "rewards": [], "terminals": []}
    for _ in range(rows):
        action = rng.integers(0, 4, 1)
        nxt, rew, term, trunc, _ = env.step(action)
        ds["observations"].append(np.array(obs[0], np.float32))
        ds["actions"].append(int(action[0]))
        ds["rewards"].append(float(np.asarray(rew)[0]))
        ds["terminals"].append(bool(np.asarray(term)[0]))
        obs = nxt
    return {k: np.asarray(v) for k, v in ds.items()}


def test_train_offline_checkpoint_elite_and_clone(tmp_path):
    import glob

    from agilerl_amd.components import ReplayBuffer
    from agilerl_amd.envs import SyntheticVecEnv
    from agilerl_amd.hpo.mutation import Mutations
    from agilerl_amd.hpo.registry import HyperparameterConfig, RLParameter
    from agilerl_amd.hpo.tournament import TournamentSelection
    from agilerl_amd.training import train_offline
    from agilerl_amd.utils import create_population

    env = SyntheticVecEnv(8, seed=3, p_done=0.05, max_episode_steps=60)
    dataset = _offline_dataset()
    INIT_HP = {"BATCH_SIZE": 32, "LR": 1e-3, "DOUBLE": True}
    hp_config = HyperparameterConfig(lr=RLParameter(min=1e-5, max=1e-2))
    np.random.seed(0)
    torch.manual_seed(0)
    make = lambda n: create_population("CQN", None, INIT_HP, env.single_observation_space,  # noqa: E731
                                       env.single_action_space, hp_config=hp_config, population_size=n)
    pop = make(2)
    assert all(a.algo == "CQN" and a.double for a in pop)
    memory = ReplayBuffer(1000)
    mutations = Mutations(no_mutation=0.1, architecture=0.3, new_layer_prob=0.2, parameters=0.3, activation=0,
                          rl_hp=0.3, rand_seed=1)
    ckpt, elite = str(tmp_path / "pop"), str(tmp_path / "elite")
    pop, fits = train_offline(env, "synthetic", dataset, "CQN", pop, memory, INIT_HP=INIT_HP, max_steps=16,
                              evo_steps=8, eval_steps=20, eval_loop=1, tournament=TournamentSelection(2, True, 2, 1),
                              mutation=mutations, checkpoint=8, checkpoint_path=ckpt, save_elite=True,
                              elite_path=elite, verbose=False)
    assert len(fits) == 2 and all(len(f) == 2 and np.isfinite(f).all() for f in fits)
    assert all(a.steps[-1] >= 16 for a in pop) and len(memory) == 599
    for agent in pop:
        assert all(torch.isfinite(p).all() for n in (agent.actor, agent.actor_target) for p in n.parameters())
    # a population checkpoint after each of the two generations, and the elite
    files = sorted(os.path.basename(f) for f in glob.glob(ckpt + "_*.pt"))
    assert files == ["pop_0_16.pt", "pop_0_8.pt", "pop_1_16.pt", "pop_1_8.pt"]
    assert os.path.exists(elite + ".pt")
    from agilerl_amd.algorithms import CQN

    for f in [os.path.join(str(tmp_path), x) for x in files] + [elite + ".pt"]:
        loaded = make(1)[0]
        loaded.load_checkpoint(f)
        _matches_file(loaded, f)
        assert loaded.algo == "CQN" and loaded.double and loaded.steps[-1] in (8, 16)
    for i, agent in enumerate(pop):  # the last checkpoint was written after the last mutation: the returned agents
        loaded = CQN.load(f"{ckpt}_{i}_16.pt")
        for n in ("actor", "actor_target"):
            assert _state_equal(getattr(agent, n).state_dict(), getattr(loaded, n).state_dict()), n
        assert _adam_equal(agent.optimizer, loaded.optimizer)
        assert (loaded.index, loaded.mut, loaded.lr) == (agent.index, agent.mut, agent.lr)

    agent = pop[0]
    torch.manual_seed(5)
    agent.learn(memory.sample(32))  # Adam state on the agent's current (possibly just mutated) networks
    agent.learn(memory.sample(32))
    path = str(tmp_path / "agent.pt")
    agent.save_checkpoint(path)
    other = CQN.load(path)
    for n in ("actor", "actor_target"):
        assert _state_equal(getattr(agent, n).state_dict(), getattr(other, n).state_dict()), n
    assert _adam_equal(agent.optimizer, other.optimizer)
    assert other.fitness == agent.fitness and other.steps == agent.steps

    clone = agent.clone()
    experiences = memory.sample(32)
    for a in (agent, clone):
        a.learn(experiences)
    for n in ("actor", "actor_target"):
        mine, theirs = getattr(agent, n).state_dict(), getattr(clone, n).state_dict()
        print(n, "max |agent - clone| =", max(float((mine[k] - theirs[k]).abs().max()) for k in mine))
        assert _state_equal(mine, theirs), n
