"""Persistent rollout and evaluation of the non-categorical PPO heads
(agx_ppo_rollout_gauss_graph_persistent / _multi_ / _bern_ and the eval twins,
PopulationRunner.head_persistent): one resident, host-paced launch per rollout
gives the bits of one policy-step launch per vector step."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

HEADS = {
    "gauss6": ("gauss", 6), "gauss17": ("gauss", 17),  # 17: the second 16-lane slot
    "multi3x3": ("multi", (3, 3)), "multi2x16": ("multi", (2,) * 16),
    "bern4": ("bern", 4), "bern32": ("bern", 32),
}


def _spec_env_kw(kind, arg, **spec_kw):
    from agilerl_amd.population import nets

    if kind == "gauss":
        return nets.GaussianActorCriticSpec(obs_dim=8, n_actions=arg, **spec_kw), dict(action_dim=arg)
    if kind == "multi":
        return (nets.MultiDiscreteActorCriticSpec(obs_dim=8, n_actions=int(sum(arg)), nvec=tuple(arg), **spec_kw),
                dict(nvec=list(arg)))
    return nets.MultiBinaryActorCriticSpec(obs_dim=8, n_actions=arg, **spec_kw), dict(n_binary=arg)


def _runner(monkeypatch, head, persistent, P=3, N=40, T=8, spec_kw=None, env_kw=None, **pop_kw):
    """(pop, runner) of `head` on the synthetic env: episodes end inside a rollout."""
    from agilerl_amd.envs import SyntheticVecEnv
    from agilerl_amd.population.ppo_pop import PPOPopulation
    from agilerl_amd.population.runner import PopulationRunner

    monkeypatch.setenv("AGX_PERSISTENT_ROLLOUT", "1" if persistent else "0")
    kind, arg = HEADS[head] if isinstance(head, str) else head
    spec, ekw = _spec_env_kw(kind, arg, **(spec_kw or {}))
    ekw.update(env_kw or {})
    kw = dict(learn_step=T * N, batch_size=64, update_epochs=2, device=DEV, seeds=list(range(P)), fused=True,
              perm_source="device")
    if kind == "multi":
        kw["multi_fused"] = True
    kw.update(pop_kw)
    pop = PPOPopulation(spec, P, N, **kw)
    run = PopulationRunner(pop, SyntheticVecEnv(P * N, seed=5, p_done=0.2, max_episode_steps=30, **ekw))
    return pop, run


def _timeout_word(run) -> int:
    return int(run.ctl_h.view(torch.int32)[1])


def _record_steps(env) -> list:
    """Every action array that env.step receives from now on, copied."""
    got = []
    step = env.step

    def recording(actions, **k):
        got.append(np.array(actions, copy=True))
        return step(actions, **k)

    env.step = recording
    return got


def _check_env_actions(pop, acts, bounds=None) -> None:
    """Shape, dtype and range of what the env was handed: float32 [P*N, A]
    (inside `bounds` when the spec has them), int64 [P*N, K] below nvec, or
    0 / 1 [P*N, n] in the MultiBinary space's dtype."""
    assert len(acts) > 0
    for a in acts:
        assert a.shape == (pop.P * pop.N, pop.spec.n_actions if pop.gaussian else pop.act_width)
        if pop.gaussian:
            assert a.dtype == np.float32 and np.isfinite(a).all()
            if bounds is not None:
                assert a.min() >= np.float32(bounds[0]) and a.max() <= np.float32(bounds[1])
        elif pop.multibinary:
            assert a.dtype == np.dtype(pop.spec.action_dtype) == np.int8
            assert ((a == 0) | (a == 1)).all()
        else:
            assert a.dtype == np.int64
            assert (a >= 0).all() and (a < np.asarray(pop.spec.nvec)[None, :]).all()


def _assert_same_steps(a: list, b: list) -> None:
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and np.array_equal(x, y), f"env step {t}"


# ---- 1. rollout parity ------------------------------------------------------------------- #
@pytest.mark.parametrize("few", ["few", "general"])
@pytest.mark.parametrize("head", list(HEADS))
def test_head_persistent_rollout_matches_per_step_launches(monkeypatch, head, few):
    """P = 3, N = 40 (row blocks of 16, 16 and a partial 8), T = 8, three
    iterations: rollout buffers, bootstrap, episode accounting, counters,
    parameters and Adam's first moment equal the per-step path's bit for bit
    (same device functions, counters counter0 + 1 + t, the bootstrap unsampled
    at counter 0, the same f32 add / f64 accumulate), in both forward forms.
    So does what the env is handed at every vector step (the host staging the
    launch writes): the per-step path's arrays, and the stored slot's values."""
    if few == "general":
        monkeypatch.setenv("AGX_GRAPH_FEW", "0")
    runs = []
    for persistent in (True, False):
        pop, run = _runner(monkeypatch, head, persistent)
        assert run.head_persistent == persistent
        assert not run.persistent and not run.graph_persistent
        assert pop._fused_learner()
        runs.append((pop, run))
    handed = [_record_steps(run.env) for _pop, run in runs]
    for _ in range(3):
        for _pop, run in runs:
            run.iteration()
    torch.cuda.synchronize()
    (a_pop, a_run), (b_pop, b_run) = runs
    for name in ("obs", "actions", "log_probs", "values", "rewards", "dones"):
        assert torch.equal(getattr(a_pop, name), getattr(b_pop, name)), name
    for name in ("last_value", "last_done", "episodes", "episode_return_sum"):
        assert torch.equal(getattr(a_run, name), getattr(b_run, name)), name
    assert int(a_run.episodes.sum()) > 0  # episodes did end inside the rollouts
    assert a_pop.act_counter == b_pop.act_counter == 3 * a_pop.T
    assert torch.equal(a_pop.params.data, b_pop.params.data)
    assert torch.equal(a_pop.opt.exp_avg, b_pop.opt.exp_avg)
    assert _timeout_word(a_run) == 0  # no workgroup timed out or was aborted
    T = a_pop.T
    assert len(handed[0]) == 3 * T
    _check_env_actions(a_pop, handed[0])
    _assert_same_steps(handed[0], handed[1])
    slot = a_pop.actions.cpu().numpy()  # [P, T, N, width]: the last rollout's
    for t in range(T):
        got = handed[0][2 * T + t].reshape(a_pop.P, a_pop.N, -1)
        assert np.array_equal(got, slot[:, t].astype(got.dtype)), t  # these specs have no bounds: nothing is clipped


# ---- 2. evaluation parity ---------------------------------------------------------------- #
BOUNDS = (-0.3, 0.3)
EVAL_HEADS = {
    # narrow bounds and a wide log_std: the env's copy is clipped on most rows
    "gauss6": dict(spec_kw=dict(action_std_init=0.5, action_low=(float(np.float32(BOUNDS[0])),) * 6,
                                action_high=(float(np.float32(BOUNDS[1])),) * 6),
                   env_kw=dict(action_low=BOUNDS[0], action_high=BOUNDS[1])),
    "multi3x3": {}, "bern4": {},
}


@pytest.mark.parametrize("max_steps", [None, 7])
@pytest.mark.parametrize("head", list(EVAL_HEADS))
def test_head_persistent_evaluation_matches_per_step_launches(monkeypatch, head, max_steps):
    """One resident launch per chunk hands the env, vector step by vector
    step, the action arrays of the per-step pass (same counters counter0 + t,
    same streams, the Box copy clipped, the MultiBinary bits in the space's
    dtype) and gives its fitness.  max_steps = None: the launch covers more
    steps than the pass needs and is ended by AGX_ROLLOUT_STOP once every
    episode has finished (checked on the driver); max_steps = 7 with chunks
    of 4 steps: two launches (4 + 3 steps), each running out by itself."""
    from agilerl_amd.population import runner as R

    if max_steps is not None:
        monkeypatch.setattr(R, "_EVAL_CHUNK", 4)
    ends = []
    real_end = R._EvalDriver.end

    def end(self):
        ends.append((self.persistent, self.step, getattr(self, "launched_to", 0)))
        real_end(self)

    monkeypatch.setattr(R._EvalDriver, "end", end)
    pop, run = _runner(monkeypatch, head, True, **EVAL_HEADS[head])
    assert run.head_persistent
    run.iteration()
    handed = _record_steps(run.env)
    rounds = getattr(pop, "eval_rounds", 0)
    fit = run.evaluate(loop=2, max_steps=max_steps)
    paced = list(handed)
    assert all(p for p, _, _ in ends) and len(ends) == 2
    if max_steps is None:
        assert all(0 < step < to for _, step, to in ends)  # stopped mid-launch
    else:
        assert all(step == to == max_steps for _, step, to in ends)
        assert len(paced) == 2 * max_steps
    del handed[:], ends[:]
    pop.eval_rounds = rounds  # the same evaluation round again
    monkeypatch.setattr(run, "head_persistent", False)
    stepped = run.evaluate(loop=2, max_steps=max_steps)
    assert not any(p for p, _, _ in ends)
    np.testing.assert_array_equal(fit, stepped)
    assert np.all(np.isfinite(fit))
    _check_env_actions(pop, paced, BOUNDS if pop.gaussian else None)
    _assert_same_steps(paced, list(handed))
    assert any(not np.array_equal(paced[0], a) for a in paced[1:])  # sampled: the steps differ
    if pop.gaussian:  # the bounds did clip
        lo, hi = np.float32(BOUNDS[0]), np.float32(BOUNDS[1])
        assert (paced[0] == lo).any() and (paced[0] == hi).any()


# ---- 3. K = 1 equals the categorical launch ------------------------------------------------ #
def test_single_component_rollout_equals_the_categorical_persistent_rollout(monkeypatch):
    """nvec = [4] under agx_ppo_rollout_multi_graph_persistent against a
    mutated-shape Discrete(4) population on the same layer list and parameters
    under agx_ppo_rollout_graph_persistent."""
    from agilerl_amd.envs import SyntheticVecEnv
    from agilerl_amd.population.nets import ActorCriticSpec
    from agilerl_amd.population.ppo_pop import PPOPopulation
    from agilerl_amd.population.runner import PopulationRunner

    shape = dict(encoder_hidden=[80], latent_dim=56, actor_hidden=[64, 64])
    P, N, T = 3, 40, 8
    md, md_run = _runner(monkeypatch, ("multi", (4,)), True, spec_kw=shape)
    assert md_run.head_persistent
    spec = ActorCriticSpec(obs_dim=8, n_actions=4, **shape)
    assert spec.n_params == md.spec.n_params
    disc = PPOPopulation(spec, P, N, learn_step=T * N, batch_size=64, update_epochs=2, device=DEV,
                         seeds=list(range(P)), fused=True, perm_source="device")
    assert disc.fused_descriptor() is None and disc.learn_descriptor() is not None
    disc.params.data.copy_(md.params.data)
    assert disc.act_seed == md.act_seed
    d_run = PopulationRunner(disc, SyntheticVecEnv(P * N, seed=5, p_done=0.2, max_episode_steps=30))
    assert d_run.graph_persistent and not d_run.head_persistent
    for _ in range(2):
        md_run.collect()
        d_run.collect()
    torch.cuda.synchronize()
    assert torch.equal(md.actions.squeeze(-1), disc.actions)
    for name in ("obs", "log_probs", "values", "rewards", "dones"):
        assert torch.equal(getattr(md, name), getattr(disc, name)), name
    for name in ("last_value", "episodes", "episode_return_sum"):
        assert torch.equal(getattr(md_run, name), getattr(d_run, name)), name


# ---- 4. the env's copy is clipped, the stored action is not ------------------------------------ #
def test_gaussian_rollout_hands_the_env_clipped_actions(monkeypatch):
    A = 6
    lo, hi = float(np.float32(-0.3)), float(np.float32(0.3))  # the bounds as the float32 the kernel clips to
    kw = dict(spec_kw=dict(action_std_init=0.5, action_low=(lo,) * A, action_high=(hi,) * A),
              env_kw=dict(action_low=lo, action_high=hi))
    # the per-step run's stored samples: the seed puts some on both sides of the bounds
    ref, ref_run = _runner(monkeypatch, ("gauss", A), False, **kw)
    assert not ref_run.head_persistent
    ref_run.collect()
    stored = ref.actions.cpu()
    assert int((stored < lo).sum()) >= 1 and int((stored > hi).sum()) >= 1

    pop, run = _runner(monkeypatch, ("gauss", A), True, **kw)
    assert run.head_persistent
    got = []
    step = run.env.step

    def recording(actions, **k):
        got.append(np.array(actions, copy=True))
        return step(actions, **k)

    run.env.step = recording
    run.collect()
    torch.cuda.synchronize()
    P, N, T = pop.P, pop.N, pop.T
    assert len(got) == T
    env_actions = torch.from_numpy(np.stack(got)).view(T, P, N, A).permute(1, 0, 2, 3)  # [P, T, N, A]
    assert float(env_actions.min()) >= lo and float(env_actions.max()) <= hi
    mine = pop.actions.cpu()
    assert torch.equal(mine, stored)  # unclipped, the per-step run's samples
    assert float(mine.min()) < lo and float(mine.max()) > hi
    assert torch.equal(env_actions, mine.clamp(lo, hi))


# ---- 5. an env that raises mid-rollout ------------------------------------------------------- #
def test_head_persistent_rollout_abort_releases_kernel(monkeypatch):
    """The runner releases the waiting workgroups with the abort word, re-arms
    the control block, and the next collect() runs normally."""
    pop, run = _runner(monkeypatch, "bern4", True)
    assert run.head_persistent
    run.collect()
    real = run._env_step
    calls = {"n": 0}

    def flaky():
        calls["n"] += 1
        if calls["n"] == 3:
            raise RuntimeError("env worker died")
        real()

    run._env_step = flaky
    with pytest.raises(RuntimeError, match="env worker died"):
        run.collect()
    run._env_step = real
    run.collect()
    torch.cuda.synchronize()
    assert run.seq_base == pop.T + 1
    assert _timeout_word(run) == 0
    assert int(pop.actions.min()) >= 0 and int(pop.actions.max()) <= 1


# ---- 6. fallbacks to the per-step path ------------------------------------------------------- #
def _check_per_step(pop, run):
    assert not run.head_persistent and not run.persistent and not run.graph_persistent
    assert not hasattr(run, "ctl_h")  # no control block: nothing is paced
    run.collect()
    torch.cuda.synchronize()
    assert pop.act_counter == pop.T and run.last_value_valid
    assert torch.isfinite(pop.log_probs).all() and torch.isfinite(run.last_value).all()


def test_action_masks_keep_the_per_step_path(monkeypatch):
    pop, run = _runner(monkeypatch, "multi3x3", True, action_masks=True)
    _check_per_step(pop, run)


def test_env_that_is_not_device_free_keeps_the_per_step_path(monkeypatch):
    from agilerl_amd.envs import SyntheticVecEnv
    from agilerl_amd.population.ppo_pop import PPOPopulation
    from agilerl_amd.population.runner import PopulationRunner

    class Env(SyntheticVecEnv):
        agx_device_free = False

    monkeypatch.setenv("AGX_PERSISTENT_ROLLOUT", "auto")
    spec, ekw = _spec_env_kw("bern", 4)
    P, N = 2, 24
    pop = PPOPopulation(spec, P, N, learn_step=4 * N, batch_size=32, device=DEV, seeds=[0, 1])
    _check_per_step(pop, PopulationRunner(pop, Env(P * N, seed=5, **ekw)))
    pop = PPOPopulation(spec, P, N, learn_step=4 * N, batch_size=32, device=DEV, seeds=[0, 1])
    assert PopulationRunner(pop, SyntheticVecEnv(P * N, seed=5, **ekw)).head_persistent  # "auto" paces this one


def test_grid_beyond_the_head_kernels_limit_keeps_the_per_step_path(monkeypatch):
    from agilerl_amd.population import runner as R

    assert R.head_max_workgroups(_runner(monkeypatch, "gauss6", False, P=1, N=8)[0]) >= 256  # one per CU at least
    monkeypatch.setattr(R, "head_max_workgroups", lambda pop: 8)  # the grid below: 3 x 3 = 9 workgroups
    pop, run = _runner(monkeypatch, "gauss6", True)
    _check_per_step(pop, run)


# ---- 7. the engine ---------------------------------------------------------------------------- #
def test_engine_trains_and_evaluates_groups_of_one_head(monkeypatch):
    """Two groups (a learn_step split) of a MultiBinary population: their
    rollouts are not paced together, train() completes, and evaluate() — one
    resident launch at a time — gives each group its own runner's fitness."""
    from agilerl_amd.envs import StackedVecEnv, SyntheticVecEnv
    from agilerl_amd.population.engine import PopulationEngine

    P, N = 4, 32
    pop, _ = _runner(monkeypatch, "bern4", True, P=P, N=N)
    envs = [SyntheticVecEnv(N, seed=10 + j, p_done=0.1, max_episode_steps=25, n_binary=4) for j in range(P)]
    views = [type("V", (), {"learn_step": pop.T * pop.N})() for _ in range(P)]
    eng = PopulationEngine(pop, views, StackedVecEnv(envs))
    states = eng.local_states()
    states[1].learn_step = states[1].learn_step // 2
    states[3].learn_step = states[3].learn_step // 2
    eng.regroup(states)
    assert len(eng.groups) == 2
    assert all(g.runner.head_persistent for g in eng.groups)
    assert not eng._paced_together()
    eng.train(2 * pop.T * pop.N)
    torch.cuda.synchronize()
    assert all(_timeout_word(g.runner) == 0 for g in eng.groups)
    handed = [_record_steps(g.runner.env) for g in eng.groups]
    fit = eng.evaluate(1, None)
    together = [list(h) for h in handed]
    for h in handed:
        del h[:]
    eng._eval_calls -= 1  # the same evaluation round, group by group
    alone = [0.0] * P
    for g in eng.groups:
        g.pop.eval_rounds = eng._eval_calls  # runner.evaluate counts this round in
        f = g.runner.evaluate(loop=1, max_steps=None)
        for r, slot in enumerate(g.slots):
            alone[slot] = float(f[r])
    assert fit == alone and all(np.isfinite(fit))
    for g, a, b in zip(eng.groups, together, handed):  # what each group's envs were handed, step by step
        _check_env_actions(g.pop, a)
        _assert_same_steps(a, b)
