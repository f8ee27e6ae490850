"""MATD3 on the GPU: agx_matd3_critic_target against the reference's own
outputs (tests/golden/matd3_*.npz), against its numpy twin
(tests/matd3_twin.py) and against agx_maddpg_critic_target;
agx_polyak_segments against agx_polyak; MATD3.learn against a plain-PyTorch
restatement of matd3.py:700-926 on copies of the same networks, with the
launches of its tail counted; and the drop-in trainer, checkpoints, clones."""

import copy
import ctypes
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = ["matd3_0", "matd3_1", "matd3_2", "matd3_nan"]
GROUPS = ("actors", "critics_1", "critics_2", "actor_targets", "critic_targets_1", "critic_targets_2")


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1))).cuda() for x in arrays]


# ---- agx_matd3_critic_target -------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_critic_target_matches_reference_golden(golden, case):
    """The kernel against MATD3.learn_individual run by the reference: y bit
    for bit, dL/dQk and the loss to f32 rounding of the mean."""
    from agilerl_amd import kernels as K
    from tests.test_matd3_cpu import check_against_golden

    g = golden(case)
    q1, q2, qn1, qn2, r, d = _dev(*(g[k] for k in ("q1", "q2", "q_next1", "q_next2", "r", "d")))
    y, g1, g2, loss = K.matd3_critic_target(q1, q2, qn1, qn2, r, d, float(g["gamma"]))
    assert y.shape == g1.shape == g2.shape == (q1.numel(), 1) and loss.shape == (1,)
    check_against_golden(g, y.cpu().numpy(), g1.cpu().numpy(), g2.cpu().numpy(), float(loss))


def _twin_inputs(B):
    rng = np.random.default_rng(1000 + B)
    q1, q2, qn1, qn2, r = (rng.standard_normal(B).astype(np.float32) for _ in range(5))
    d = (rng.random(B) < 0.3).astype(np.float32)
    if B == 1:
        d[0] = 2.0
        return q1, q2, qn1, qn2, r, d
    r[rng.random(B) < 0.1] = np.nan
    d[rng.random(B) < 0.1] = np.nan
    last = B - 1  # 257: the one row of the second block
    r[last], d[last] = np.nan, 0.0
    d[last - 1] = np.nan
    d[last - 2], r[last - 2] = 2.0, 0.5
    d[last - 3], r[last - 3], qn1[last - 3] = 0.0, 0.25, np.nan
    return q1, q2, qn1, qn2, r, d


@pytest.mark.parametrize("B", [1, 77, 256, 257, 4096])
def test_critic_target_matches_twin(B):
    """y and both gradients bit for bit, the loss to 1e-6 relative (a NaN
    target value makes it NaN on both sides)."""
    from agilerl_amd import kernels as K
    from tests.matd3_twin import critic_target

    inputs = _twin_inputs(B)
    y, g1, g2, loss = K.matd3_critic_target(*_dev(*inputs), 0.95)
    ye, g1e, g2e, le = critic_target(*inputs, 0.95)
    for got, want in ((y, ye), (g1, g1e), (g2, g2e)):
        assert np.array_equal(got.cpu().numpy().reshape(-1), want, equal_nan=True)
    if B > 1:
        assert np.isnan(ye).sum() == 1 and np.isnan(le) and np.isnan(float(loss))
        # the loss itself: the same rows without the NaN target value
        inputs[2][B - 4] = 0.125
        _, _, _, loss = K.matd3_critic_target(*_dev(*inputs), 0.95)
        ye, _, _, le = critic_target(*inputs, 0.95)
        assert not np.isnan(ye).any()
    assert np.isfinite(le) and abs(float(loss) - float(le)) <= 1e-6 * abs(float(le))


@pytest.mark.parametrize("B", [77, 257])
def test_critic_target_consistent_with_maddpg_kernel(B):
    """With q2 = q1 and q_next2 = q_next1 the twin form is MADDPG's: y and
    dL/dQ1 bit for bit, the loss f32(l) + f32(l)."""
    from agilerl_amd import kernels as K

    q1, _, qn1, _, r, d = _twin_inputs(B)
    qn1[B - 4] = 0.125  # finite everywhere: the loss is compared
    q1, qn1, r, d = _dev(q1, qn1, r, d)
    y, g1, g2, loss = K.matd3_critic_target(q1, q1.clone(), qn1, qn1.clone(), r, d, 0.95)
    ym, gm, lm = K.maddpg_critic_target(q1, qn1, r, d, 0.95)
    assert torch.equal(y, ym) and torch.equal(g1, gm) and torch.equal(g2, gm)
    assert torch.isfinite(lm).all() and torch.equal(loss, lm + lm)


# ---- agx_polyak_segments -------------------------------------------------------------
def _carved(n, seed, sentinel):
    """An n-element f32 tensor one element into a buffer of n + 2 (so its base
    is 4-byte aligned only), the buffer's two other elements sentinels."""
    buf = torch.full((n + 2,), sentinel, dtype=torch.float32, device="cuda")
    buf[1:n + 1] = torch.randn(n, generator=torch.Generator().manual_seed(seed)).cuda()
    return buf, buf[1:n + 1]


def _check_segments(sizes, tau=0.01):
    from agilerl_amd import kernels as K

    bufs, targets, onlines, want = [], [], [], []
    for k, n in enumerate(sizes):
        tb, t = _carved(n, 2 * k, 7.5)
        ob, o = _carved(n, 2 * k + 1, -3.25)
        assert n == 0 or (t.data_ptr() % 8 == 4 and o.data_ptr() % 8 == 4)
        e = t.clone()
        K.polyak_(e, o.clone(), tau)
        bufs.append((tb, ob, o.clone()))
        targets.append(t)
        onlines.append(o)
        want.append(e)
    K.polyak_segments_(targets, onlines, tau)
    for n, t, o, e, (tb, ob, o0) in zip(sizes, targets, onlines, want, bufs):
        assert torch.equal(t, e), n
        assert torch.equal(o, o0), n
        assert tb[0] == 7.5 and tb[n + 1] == 7.5 and ob[0] == -3.25 and ob[n + 1] == -3.25, n


def test_polyak_segments_matches_polyak():
    """One call; 1 048 579 > 4096 blocks of 256, so the grid-stride loop turns."""
    _check_segments([1, 255, 256, 257, 0, 1_048_579])


def test_polyak_segments_full_table_and_split(monkeypatch):
    from agilerl_amd import _lib

    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append((name, a[1] if name == "agx_polyak_segments"
                                                                      else None)), real(name, *a))[1])
    _check_segments([7] * 64)
    assert [c for c in calls if c[0] == "agx_polyak_segments"] == [("agx_polyak_segments", 64)]
    del calls[:]
    _check_segments([7 + k % 5 for k in range(130)])
    assert [c for c in calls if c[0] == "agx_polyak_segments"] == [("agx_polyak_segments", 64)] * 2 + \
        [("agx_polyak_segments", 2)]


def test_polyak_segments_error_path_launches_nothing():
    from agilerl_amd import _lib
    from agilerl_amd.kernels import _PolyakSegment

    lib = _lib.load()
    t = torch.ones(65, 8, device="cuda")
    o = torch.zeros(65, 8, device="cuda")
    arr = (_PolyakSegment * 65)(*[_PolyakSegment(t[k].data_ptr(), o[k].data_ptr(), 8) for k in range(65)])
    ptr = ctypes.cast(arr, ctypes.c_void_p)
    assert lib.agx_polyak_segments(ptr, 65, 0.5, _lib.stream()) == -1
    assert b"agx_polyak_segments" in lib.agx_last_error()
    arr[1] = _PolyakSegment(t[1].data_ptr(), None, 8)
    assert lib.agx_polyak_segments(ptr, 4, 0.5, _lib.stream()) == -1
    arr[1] = _PolyakSegment(None, o[1].data_ptr(), 8)
    assert lib.agx_polyak_segments(ptr, 4, 0.5, _lib.stream()) == -1
    torch.cuda.synchronize()
    assert bool((t == 1).all())  # segment 0 was valid in every call: nothing ran
    with pytest.raises(ValueError):
        from agilerl_amd import kernels as K

        K.polyak_segments_([t[0]], [o[0], o[1]], 0.5)


# ---- MATD3.learn ---------------------------------------------------------------------
def _reference_learn(agent, nets, opts, counter, experiences):
    """matd3.py:700-926 in plain PyTorch (criterion nn.MSELoss) -> losses."""
    actors, critics_1, critics_2, actor_targets, critic_targets_1, critic_targets_2 = nets
    opt_a, opt_c1, opt_c2 = opts
    states, actions, rewards, next_states, dones = experiences
    ids = agent.agent_ids
    with torch.no_grad():
        next_actions = [actor_targets[a](next_states[a]) for a in ids]
    stacked = torch.cat([actions[a] for a in ids], dim=1)
    stacked_next = torch.cat(next_actions, dim=1)
    losses = {}
    for a in ids:
        q1, q2 = critics_1[a](states, stacked), critics_2[a](states, stacked)
        with torch.no_grad():
            qn1 = critic_targets_1[a](next_states, stacked_next)
            qn2 = critic_targets_2[a](next_states, stacked_next)
        qn = torch.min(qn1, qn2)
        r = torch.where(torch.isnan(rewards[a]), torch.full_like(rewards[a], 0), rewards[a]).to(torch.float32)
        d = torch.where(torch.isnan(dones[a]), torch.full_like(dones[a], 1), dones[a]).to(torch.uint8)
        y = r + (1 - d) * agent.gamma * qn
        loss = torch.nn.functional.mse_loss(q1, y) + torch.nn.functional.mse_loss(q2, y)
        opt_c1[a].zero_grad()
        opt_c2[a].zero_grad()
        loss.backward()
        opt_c1[a].step()
        opt_c2[a].step()
        actor_loss = None
        act = actors[a](states[a])
        det = {k: (act if k == a else actions[k]) for k in ids}
        counter[a] += 1
        if counter[a] % agent.policy_freq == 0:
            actor_loss = -critics_1[a](states, torch.cat([det[k] for k in ids], dim=1)).mean()
            opt_a[a].zero_grad()
            actor_loss.backward()
            opt_a[a].step()
        losses[a] = (actor_loss.item() if actor_loss is not None else None, loss.item())
    if all(c % agent.policy_freq == 0 for c in counter.values()):
        with torch.no_grad():
            for a in ids:
                for net, tgt in ((actors[a], actor_targets[a]), (critics_1[a], critic_targets_1[a]),
                                 (critics_2[a], critic_targets_2[a])):
                    for e, t in zip(net.parameters(), tgt.parameters()):
                        t.copy_(agent.tau * e + (1.0 - agent.tau) * t)
    return losses


def _snapshot(agent):
    return {g: {a: [p.detach().clone() for p in getattr(agent, g)[a].parameters()] for a in agent.agent_ids}
            for g in GROUPS}


def _learn_run(agent_dims, updates):
    """``updates`` MATD3.learn calls beside the restatement, from the same
    batches and torch seeds -> per update: the losses of both sides, the
    libagx calls made, snapshots of the agent's networks before and after."""
    from agilerl_amd import _lib
    from agilerl_amd.algorithms import MATD3
    from agilerl_amd.components import MultiAgentReplayBuffer
    from agilerl_amd.envs import SyntheticMultiAgentVecEnv

    env = SyntheticMultiAgentVecEnv(8, agent_dims=agent_dims, seed=2)
    ids = env.agents
    torch.manual_seed(0)
    agent = MATD3([env.observation_spaces[a] for a in ids], [env.action_spaces[a] for a in ids], agent_ids=ids,
                  batch_size=32, vect_noise_dim=8, policy_freq=2)
    nets = copy.deepcopy(tuple(getattr(agent, g) for g in GROUPS))
    opts = tuple({a: torch.optim.Adam(nets[k][a].parameters(), lr=lr) for a in ids}
                 for k, lr in ((0, agent.lr_actor), (1, agent.lr_critic), (2, agent.lr_critic)))
    counter = dict.fromkeys(ids, 0)
    mem = MultiAgentReplayBuffer(256, ["obs", "action", "reward", "next_obs", "done"], ids)
    obs, info = env.reset()
    for t in range(20):
        action, raw = agent.get_action(obs, infos=info)
        nxt, rew, term, trunc, info = env.step(action)
        if t == 5:
            rew[ids[-1]][0] = np.nan
        mem.save_to_memory(obs, raw, rew, nxt, term, is_vectorised=True)
        obs = nxt
    record = []
    real = _lib.call
    for it in range(updates):
        random.seed(it)
        exp = mem.sample(32)
        before, calls = _snapshot(agent), []
        _lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]  # noqa: B023
        try:
            torch.manual_seed(10 + it)  # same Gumbel draws on both sides
            losses = agent.learn(exp)
        finally:
            _lib.call = real
        torch.manual_seed(10 + it)
        ref_losses = _reference_learn(agent, nets, opts, counter, exp)
        record.append(dict(losses=losses, ref_losses=ref_losses, calls=calls, before=before, after=_snapshot(agent)))
    assert any(bool(torch.isnan(t).any()) for t in mem.sample(len(mem))[2].values())  # the NaN reward is in the buffer
    return agent, dict(zip(GROUPS, nets)), record


@pytest.fixture(scope="module")
def speaker_listener_run():
    return _learn_run(None, 4)


def _assert_same_networks(agent, nets):
    for g in GROUPS:
        for a in agent.agent_ids:
            for p1, p2 in zip(getattr(agent, g)[a].parameters(), nets[g][a].parameters()):
                torch.testing.assert_close(p1, p2, rtol=1e-4, atol=2e-5)


def test_learn_matches_torch(speaker_listener_run):
    agent, nets, record = speaker_listener_run
    ids = agent.agent_ids
    first = record[0]
    # update 1 of policy_freq = 2: critics only
    assert all(first["losses"][a][0] is None and np.isfinite(first["losses"][a][1]) for a in ids)
    for g in ("actors", "actor_targets", "critic_targets_1", "critic_targets_2"):
        for a in ids:
            assert all(torch.equal(p, q) for p, q in zip(first["before"][g][a], first["after"][g][a])), (g, a)
    for g in ("critics_1", "critics_2"):
        for a in ids:
            assert not all(torch.equal(p, q) for p, q in zip(first["before"][g][a], first["after"][g][a])), (g, a)
    for k, rec in enumerate(record):
        for a in ids:
            mine, ref = rec["losses"][a], rec["ref_losses"][a]
            assert (mine[0] is None) == (ref[0] is None) == (k % 2 == 0), (k, a)
            assert np.isfinite(mine[1]) and np.isfinite(ref[1]), (k, a)
    # update 2 moved every target
    second = record[1]
    for g in ("actor_targets", "critic_targets_1", "critic_targets_2"):
        for a in ids:
            assert not all(torch.equal(p, q) for p, q in zip(second["before"][g][a], second["after"][g][a])), (g, a)
    assert agent.learn_counter == dict.fromkeys(ids, 4)
    _assert_same_networks(agent, nets)


def test_learn_matches_torch_three_unequal_agents():
    """The cat order of observations and actions: three agents of unequal
    dimensions, two updates (the second steps the actors and the targets)."""
    agent, nets, record = _learn_run({"a_0": (3, 3), "b_0": (11, 5), "c_0": (6, 2)}, 2)
    assert all(v[0] is None for v in record[0]["losses"].values())
    assert all(v[0] is not None and np.isfinite(v).all() for v in record[1]["losses"].values())
    assert record[1]["calls"].count("agx_polyak_segments") == 1 and record[1]["calls"].count("agx_clip_adam") == 9
    _assert_same_networks(agent, nets)


def test_launch_shape_of_the_tail(speaker_listener_run):
    agent, _, record = speaker_listener_run
    N = len(agent.agent_ids)
    first, second = record[0]["calls"], record[1]["calls"]
    assert "agx_polyak" not in first and "agx_polyak_segments" not in first
    assert first.count("agx_clip_adam") == 2 * N and first.count("agx_matd3_critic_target") == N
    assert second.count("agx_polyak_segments") == 1 and "agx_polyak" not in second
    assert second.count("agx_clip_adam") == 3 * N and second.count("agx_matd3_critic_target") == N
    assert "agx_maddpg_critic_target" not in first + second and "agx_td3_critic_target" not in first + second


# ---- end to end ------------------------------------------------------------------------
def test_train_checkpoint_and_clone(tmp_path):
    from agilerl_amd.algorithms import MATD3
    from agilerl_amd.components import MultiAgentReplayBuffer
    from agilerl_amd.envs import SyntheticMultiAgentVecEnv
    from agilerl_amd.hpo.mutation import Mutations
    from agilerl_amd.hpo.tournament import TournamentSelection
    from agilerl_amd.training import train_multi_agent_off_policy
    from agilerl_amd.utils import create_population

    env = SyntheticMultiAgentVecEnv(8, seed=2)
    obs_spaces = [env.observation_spaces[a] for a in env.agents]
    act_spaces = [env.action_spaces[a] for a in env.agents]
    INIT_HP = {"AGENT_IDS": env.agents, "BATCH_SIZE": 32, "LEARN_STEP": 8}
    np.random.seed(0)
    pop = create_population("MATD3", None, INIT_HP, obs_spaces, act_spaces, population_size=2, num_envs=8)
    assert all(type(a) is MATD3 and a.policy_freq == 2 for a in pop)
    mem = MultiAgentReplayBuffer(1000, ["obs", "action", "reward", "next_obs", "done"], env.agents)
    pop, fits = train_multi_agent_off_policy(env, "synthetic_speaker_listener", "MATD3", pop, mem,
                                             INIT_HP=INIT_HP, max_steps=400, evo_steps=200, eval_loop=1,
                                             tournament=TournamentSelection(2, True, 2, 1),
                                             mutation=Mutations(1.0, 0, 0.2, 0, 0, 0, rand_seed=1), verbose=False)
    assert len(fits) == 2 and all(np.isfinite(f).all() for f in fits)
    assert all(a.steps[-1] >= 400 for a in pop) and len(mem) == 800
    assert all(c > 0 for a in pop for c in a.learn_counter.values())
    path = str(tmp_path / "matd3.pt")
    pop[0].save_checkpoint(path)
    other = create_population("MATD3", None, INIT_HP, obs_spaces, act_spaces, population_size=1, num_envs=8)[0]
    other.load_checkpoint(path)
    for g in ("actors", "critics_1", "critics_2"):
        for a in env.agents:
            for p1, p2 in zip(getattr(pop[0], g)[a].parameters(), getattr(other, g)[a].parameters()):
                assert torch.equal(p1, p2)
    assert other.fitness == pop[0].fitness and other.learn_counter == pop[0].learn_counter

    # a clone owns its flat buffers: its update leaves the parent untouched
    parent = pop[0]
    assert parent.__dict__.get("_flat")
    before = _snapshot(parent)
    clone = parent.clone(index=7)
    assert clone.index == 7 and len(clone.__dict__["_flat"]) == len(parent.__dict__["_flat"]) == 6
    mine = {p.data_ptr() for g in GROUPS for a in env.agents for p in getattr(parent, g)[a].parameters()}
    assert not mine & {p.data_ptr() for g in GROUPS for a in env.agents for p in getattr(clone, g)[a].parameters()}
    clone.learn_counter = dict.fromkeys(env.agents, 1)  # the next update steps actors and targets too
    random.seed(3)
    clone.learn(mem.sample(32))
    after, moved = _snapshot(parent), _snapshot(clone)
    for g in GROUPS:
        for a in env.agents:
            assert all(torch.equal(p, q) for p, q in zip(before[g][a], after[g][a])), (g, a)
            assert not all(torch.equal(p, q) for p, q in zip(before[g][a], moved[g][a])), (g, a)
