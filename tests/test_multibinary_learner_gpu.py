"""agx_ppo_learn_bern_graph (graph_learner.hip, the Bernoulli instantiations):
the runtime-shape fused learner with a Bernoulli head, against the autograd
learner (PPOPopulation._learn_torch, itself pinned to an independent torch twin
by tests/test_multibinary_ppo_gpu.py::test_bern_learner_update_matches_torch_twin)
on identical inputs and permutations.  Helpers and bars are those of
tests/test_multidisc_learner_gpu.py, the masks those of
tests/multibinary_twin.py."""

import ctypes

import numpy as np
import pytest
import torch

from tests import multibinary_twin as B

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

# shapes of tests/test_graph_learner_gpu.py's SHAPES
SHAPES = {
    "latent_56": dict(encoder_hidden=[64], latent_dim=56, actor_hidden=[64], critic_hidden=[64]),
    "no_layer_norm": dict(encoder_hidden=[64, 64], latent_dim=40, actor_hidden=[48], critic_hidden=[64],
                          layer_norm=False),
    "own_critic_encoder": dict(encoder_hidden=[64], latent_dim=48, actor_hidden=[64], critic_hidden=[32],
                               share_encoders=False),
}

# how the call splits a minibatch (graph_learner.hip graph_split): the few-row
# partnered form by default, the general partnered form, one workgroup per agent
FORMS = {"default": {}, "general": {"AGX_GRAPH_FEW": "0"}, "one_workgroup": {"AGX_GRAPH_SPLIT": "1"}}

WIDTHS = [1, 5, 17, 32]  # one bit, the lanes' first logits only, one bit into the second half, full width


def _setenv(monkeypatch, form):
    for k in ("AGX_GRAPH_FEW", "AGX_GRAPH_SPLIT", "AGX_GRAPH_ROWS", "AGX_BERN_FUSED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in form.items():
        monkeypatch.setenv(k, v)


def _fill(pop, seed, masks=False):
    """A rollout for ``pop``: observations randn; the actor's output weight
    times 10 (probabilities far from a half); actions from the population's
    own policy step; with ``masks`` about a third of the bits illegal, the
    stored 1-bits legal, and for agent 0 bit 0 cleared and illegal in every
    row; log_probs = the true log-prob + 0.05 randn (both clip branches occur);
    values + 0.1 randn (both value branches)."""
    from agilerl_amd.population.nets import bernoulli_head

    spec, P, T, N, D = pop.spec, pop.P, pop.T, pop.N, pop.spec.obs_dim
    n = spec.n_actions
    W, _, _, _ = spec.views(pop.params.data, spec.actor[-1])
    W.mul_(10.0)
    g = torch.Generator(device=DEV).manual_seed(seed + 99)
    pop.obs.copy_(torch.randn(pop.obs.shape, device=DEV, generator=g))
    pop.rewards.copy_(torch.randn(pop.rewards.shape, device=DEV, generator=g))
    pop.dones.copy_((torch.rand(pop.dones.shape, device=DEV, generator=g) < 0.05).to(torch.uint8))
    for t in range(T):
        pop.act_into(t)
    mk = None
    pop.never_legal = None
    if masks:
        if n > 1:  # (with one bit, masking it everywhere would leave agent 0 no actor gradient at all)
            pop.actions[0, :, :, 0] = 0
            pop.never_legal = 0
        acts = pop.actions.reshape(-1, n).cpu().numpy()
        m = B.random_mask(np.random.default_rng(seed), P * T * N, n, keep=acts).reshape(P, T * N, n)
        if n > 1:
            m[0, :, 0] = 0
        pop.action_masks.copy_(torch.from_numpy(m).view_as(pop.action_masks))
        mk = pop.action_masks.view(P, T * N, n)
    with torch.no_grad():
        logits, _ = spec.forward(pop.params.data, pop.obs.view(P, -1, D))
        lp, _ = bernoulli_head(logits, pop.actions.view(P, T * N, n), mk)
    pop.values.add_(0.1 * torch.randn(pop.values.shape, device=DEV, generator=g))
    pop.log_probs.copy_(lp.view_as(pop.log_probs) + 0.05 * torch.randn(pop.log_probs.shape, device=DEV, generator=g))
    last_obs = torch.randn(P, N, D, device=DEV, generator=g)
    pop.finish_rollout(last_obs, torch.zeros(P, N, dtype=torch.uint8, device=DEV))


def _pop(shape, n=5, P=3, N=16, learn_step=128, batch=64, epochs=1, seed=0, masks=False, **kw):
    from agilerl_amd.population.nets import MultiBinaryActorCriticSpec
    from agilerl_amd.population.ppo_pop import PPOPopulation

    spec = MultiBinaryActorCriticSpec(obs_dim=8, n_actions=n, **SHAPES[shape])
    pop = PPOPopulation(spec, P, N, learn_step=learn_step, batch_size=batch, lr=1e-3, update_epochs=epochs,
                        seeds=[seed + i for i in range(P)], device=DEV, fused=True, action_masks=masks,
                        **kw)
    _fill(pop, seed, masks)
    return pop


def _state(pop):
    return (pop.params.data.clone(), pop.opt.exp_avg.clone(), pop.opt.exp_avg_sq.clone(),
            pop.advantages.clone(), pop.opt.steps.clone())


def _restore(pop, st):
    pop.params.data.copy_(st[0])
    pop.opt.exp_avg.copy_(st[1])
    pop.opt.exp_avg_sq.copy_(st[2])
    pop.advantages.copy_(st[3])
    pop.opt.steps.copy_(st[4])


def _fused(pop, perms):
    from agilerl_amd.population.learner import BernGraphLearner, fused_learn

    assert pop.learn_descriptor() is None and pop.bern_learn_descriptor() is not None
    loss = fused_learn(pop, perms).clone()
    torch.cuda.synchronize()
    assert isinstance(pop._fused, BernGraphLearner)
    pop.check_errors()
    return loss


def _workspace_bytes(pop):
    from agilerl_amd import _lib

    return _lib.load().agx_ppo_learn_bern_graph_workspace_bytes(
        ctypes.byref(pop.bern_learn_descriptor()), pop.P, pop.S, pop.update_epochs, pop.split_batch)


def _compare(pop, perms):
    """torch learner vs the Bernoulli graph learner from the same
    state: the drift bars of tests/test_graph_learner_gpu.py::_compare, and the
    same epochs run / Adam steps."""
    st = _state(pop)
    loss_t = pop._learn_torch(perms).clone()
    p_t, m_t, steps_t = pop.params.data.clone(), pop.opt.exp_avg.clone(), pop.opt.steps.clone()
    ran_t = pop.last_epochs_run.clone()
    _restore(pop, st)
    loss_g = _fused(pop, perms)
    m_g, m_tn = pop.opt.exp_avg.cpu().numpy(), m_t.cpu().numpy()
    scale_m = np.abs(m_tn).max()
    off = np.abs(m_g - m_tn) > 2e-3 * np.abs(m_tn) + 1e-5 * scale_m
    assert off.mean() <= 5e-3, off.mean()
    assert np.abs(m_g - m_tn).max() <= 1e-4 * scale_m
    d_t, d_g = p_t - st[0], pop.params.data - st[0]
    scale = d_t.abs().max().item()
    assert scale > 0
    bad = ((d_g - d_t).abs() > 2e-3 * scale).float().mean().item()
    assert bad <= 1e-3, bad
    assert torch.equal(pop.opt.steps, steps_t)
    assert torch.equal(pop._fused.epochs_run, ran_t)
    np.testing.assert_allclose(loss_g.cpu().numpy(), loss_t.cpu().numpy(), rtol=1e-4, atol=1e-7)


# ---- 3. single update, tight ---------------------------------------------------------- #
# S = 64: one 64-row minibatch in each of the three forms.  S = 16: the default
# form with one 16-row slice, and with AGX_GRAPH_ROWS=8 two few-row slices of 8
# (half of each 16-row tile is past the slice).
RUNS = {64: [(form, env) for form, env in FORMS.items()],
        16: [("default", {}), ("default-rows8", {"AGX_GRAPH_ROWS": "8"})]}
SINGLE = [(n, shape, S, masks) for n in WIDTHS for shape in SHAPES for S in (64, 16) for masks in (False, True)
          if (S == 64 and shape != "own_critic_encoder") or (S == 16 and shape == "latent_56" and n != 5)
          or (shape == "own_critic_encoder" and S == 64 and n == 17)]


@pytest.mark.parametrize("n,shape,S,masks", SINGLE,
                         ids=[f"n{n}-{sh}-S{s}-{'mask' if m else 'nomask'}" for n, sh, s, m in SINGLE])
def test_bern_learner_single_update_tight(n, shape, S, masks, monkeypatch):
    """One minibatch, one epoch: the clipped gradient of the single update
    (exp_avg = 0.1 g after Adam's first step) matches the autograd learner's
    in every form, the actor output layer's weight and bias asserted on their
    own; a bit that is illegal in every row of an agent gets exactly 0."""
    _setenv(monkeypatch, {})
    pop = _pop(shape, n=n, N=16, learn_step=S, batch=S, epochs=1, seed=5, masks=masks)
    st = _state(pop)
    perms = pop.permutations()
    pop._learn_torch(perms)
    gt = pop.opt.grads.cpu().numpy().copy()
    mt = pop.opt.exp_avg.cpu().numpy().copy()
    out = pop.spec.actor[-1]
    L, fin = out.fout, out.fin
    w = slice(out.w, out.w + L * fin)
    b = slice(out.b, out.b + L)
    am, ag = 1e-6 * np.abs(mt).max(), 1e-6 * np.abs(gt).max()
    assert np.abs(mt[:, w]).max() > 0 and np.abs(mt[:, b]).max() > 0
    for form, env in RUNS[S]:
        _setenv(monkeypatch, env)
        _restore(pop, st)
        pop._fused = None  # the workspace is sized by the form
        _fused(pop, perms)
        m = pop.opt.exp_avg.cpu().numpy()
        err = np.abs(m - mt) / (1e-4 * np.abs(mt) + am)
        print(f"n={n} {shape} S={S} masks={masks} {form}: worst |err| / bar: all {err.max():.3f}, "
              f"out W {err[:, w].max():.3f}, out b {err[:, b].max():.3f}")
        for sl in (w, b):
            np.testing.assert_allclose(m[:, sl], mt[:, sl], rtol=1e-4, atol=am)
            np.testing.assert_allclose(m[:, sl] / 0.1, gt[:, sl], rtol=1e-3, atol=ag)
        np.testing.assert_allclose(m, mt, rtol=1e-4, atol=am)
        np.testing.assert_allclose(m / 0.1, gt, rtol=1e-3, atol=ag)
        if masks:
            # rows of the output weight whose logit is illegal somewhere: autograd's values
            mk = pop.action_masks.view(pop.P, -1, L).cpu().numpy()
            seen = 0
            for p in range(pop.P):
                rows = np.nonzero((mk[p] == 0).any(0))[0]
                seen += rows.size
                got = m[p, w].reshape(L, fin)[rows]
                np.testing.assert_allclose(got, mt[p, w].reshape(L, fin)[rows], rtol=1e-4, atol=am)
            assert seen > 0
            j = pop.never_legal
            if j is not None:  # illegal in every row of agent 0: no gradient at all
                assert not mt[0, w].reshape(L, fin)[j].any() and mt[0, b][j] == 0
                assert not m[0, w].reshape(L, fin)[j].any() and m[0, b][j] == 0
        assert not torch.equal(pop.params.data, st[0])


# ---- 4. every form, several updates ---------------------------------------------------- #
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape,n,masks,N,learn_step,batch,epochs", [
    ("latent_56", 5, False, 16, 128, 64, 2),
    ("own_critic_encoder", 17, True, 8, 100, 32, 2),  # a short last minibatch: the second partner has no rows
    ("no_layer_norm", 32, False, 16, 128, 48, 1)])
def test_bern_learner_matches_torch_learner(shape, n, masks, N, learn_step, batch, epochs, form, monkeypatch):
    _setenv(monkeypatch, FORMS[form])
    pop = _pop(shape, n=n, N=N, learn_step=learn_step, batch=batch, epochs=epochs, masks=masks)
    np.random.seed(1234)
    _compare(pop, pop.permutations())


# ---- 10. the three forms are three runs -------------------------------------------------- #
def test_bern_learner_forms_differ_in_workspace(monkeypatch):
    """The three forms the tests here name are three different runs: the
    workspace query, which makes the call's choice, sizes each differently."""
    _setenv(monkeypatch, {})
    pop = _pop("latent_56", N=16, learn_step=128, batch=64)
    sizes = {}
    for form, env in FORMS.items():
        _setenv(monkeypatch, env)
        sizes[form] = _workspace_bytes(pop)
    assert all(v > 0 for v in sizes.values()) and len(set(sizes.values())) == 3, sizes


# ---- 5. heterogeneous hyperparameters, target_kl ------------------------------------------ #
def test_bern_learner_heterogeneous_hparams(monkeypatch):
    _setenv(monkeypatch, {})
    pop = _pop("latent_56", n=9, P=3, N=16, learn_step=128, batch=64, epochs=2)
    pop.set_agent_hparam(1, "batch_size", 32)
    pop.set_agent_hparam(2, "update_epochs", 1)
    pop.set_agent_hparam(0, "ent_coef", 0.05)
    _compare(pop, pop.permutations())
    assert pop._fused.epochs_run.tolist() == [2, 2, 1]


def test_bern_learner_target_kl_stops_like_torch(monkeypatch):
    _setenv(monkeypatch, {})
    pop = _pop("latent_56", n=9, N=16, learn_step=128, batch=32, epochs=4, target_kl=1e-4)
    _compare(pop, pop.permutations())  # equal epochs_run asserted there
    assert int(pop._fused.epochs_run.min()) < 4


# ---- 7. determinism and independence ------------------------------------------------------ #
@pytest.mark.parametrize("form", list(FORMS))
def test_bern_learner_is_deterministic_and_independent_of_the_population(form, monkeypatch):
    """Two learns from the same state give equal bits; agent 0's row after a
    P = 3 learn equals its row after a P = 1 learn from the same state and
    permutation (fixed summation order: no atomics, no dependence on the grid)."""
    _setenv(monkeypatch, FORMS[form])
    kw = dict(n=17, N=16, learn_step=128, batch=64, epochs=2, seed=11)
    pop = _pop("latent_56", P=3, **kw)
    perms = pop.permutations()
    st = _state(pop)
    _fused(pop, perms)
    first = (pop.params.data.clone(), pop.opt.exp_avg.clone(), pop.opt.exp_avg_sq.clone())
    _restore(pop, st)
    _fused(pop, perms)
    for a, b in zip(first, (pop.params.data, pop.opt.exp_avg, pop.opt.exp_avg_sq)):
        assert torch.equal(a, b)
    pop_1 = _pop("latent_56", P=1, **kw)
    pop_1.params.data.copy_(st[0][0:1])
    for name in ("obs", "actions", "log_probs", "values", "advantages", "returns", "adv_stats"):
        getattr(pop_1, name).copy_(getattr(pop, name)[0:1])
    _fused(pop_1, perms[:, 0:1].contiguous())
    assert torch.equal(pop_1.params.data[0], first[0][0])
    assert torch.equal(pop_1.opt.exp_avg[0], first[1][0]) and torch.equal(pop_1.opt.exp_avg_sq[0], first[2][0])


# ---- 8. a stored action other than 0 / 1 --------------------------------------------------- #
def test_bern_learner_counts_any_nonzero_action_as_one(monkeypatch):
    """Defined behaviour (include/agx_bernoulli.h): a stored action other than
    0 learns as 1, so the learn equals the learn of the rollout with 1 in its
    place bit for bit, and no error is flagged."""
    _setenv(monkeypatch, {})
    pop = _pop("latent_56", n=9, N=16, learn_step=16, batch=16, epochs=1, seed=13)
    perms = pop.permutations()
    st = _state(pop)
    good = pop.actions.clone()
    good[0, 0, 3, 0] = 1
    good[1, 0, 9, 8] = 1
    good[2, 0, 1, 4] = 1
    pop.actions.copy_(good)
    pop.actions[0, 0, 3, 0] = 7
    pop.actions[1, 0, 9, 8] = -3
    pop.actions[2, 0, 1, 4] = 1 << 40
    loss_a = _fused(pop, perms)
    got = (pop.params.data.clone(), pop.opt.exp_avg.clone(), pop.opt.exp_avg_sq.clone())
    _restore(pop, st)
    pop.actions.copy_(good)
    loss_b = _fused(pop, perms)
    for a, b in zip(got, (pop.params.data, pop.opt.exp_avg, pop.opt.exp_avg_sq)):
        assert torch.equal(a, b)
    assert torch.equal(loss_a, loss_b) and bool(torch.isfinite(loss_a).all())
    assert not torch.equal(pop.params.data, st[0])


# ---- 9. routing ---------------------------------------------------------------------------- #
def _dropin_population():
    from agilerl_amd.envs import Box, MultiBinary
    from agilerl_amd.utils import create_population

    INIT_HP = {"BATCH_SIZE": 32, "LR": 1e-3, "LEARN_STEP": 64, "UPDATE_EPOCHS": 2}
    agents = create_population("PPO", None, INIT_HP, Box(-np.inf, np.inf, (8,)), MultiBinary(5),
                               population_size=2, num_envs=8)
    pop = agents[0].population
    _fill(pop, 3)
    return pop


def _layer_norm_raises(monkeypatch):
    import torch.nn.functional as F

    def layer_norm(*a, **k):
        raise AssertionError("torch layer_norm during learn(): the autograd learner ran")

    monkeypatch.setattr(F, "layer_norm", layer_norm)


def test_multibinary_population_learns_through_the_fused_learner_by_default(monkeypatch):
    from agilerl_amd.population.learner import BernGraphLearner

    _setenv(monkeypatch, {})
    pop = _dropin_population()
    assert pop.multibinary and pop.fused
    assert pop.learn_descriptor() is None and pop.fused_descriptor() is None and pop.eval_descriptor() is None
    assert pop.bern_learn_descriptor() is not None and pop._fused_learner()
    before = pop.params.data.clone()
    np.random.seed(2)
    _layer_norm_raises(monkeypatch)
    loss = pop.learn()
    torch.cuda.synchronize()
    pop.check_errors()
    assert isinstance(pop._fused, BernGraphLearner)
    assert bool(torch.isfinite(loss).all()) and not torch.equal(pop.params.data, before)
    assert pop.last_kl is pop._fused.kl and pop._fused.epochs_run.tolist() == [2, 2]


@pytest.mark.parametrize("how", ["keyword", "environment"])
def test_multibinary_population_keeps_the_autograd_learner_when_switched_off(how, monkeypatch):
    _setenv(monkeypatch, {"AGX_BERN_FUSED": "0"} if how == "environment" else {})
    pop = _dropin_population()
    if how == "keyword":
        pop.fused = False
    assert pop.bern_learn_descriptor() is None and not pop._fused_learner()
    np.random.seed(2)
    _layer_norm_raises(monkeypatch)
    with pytest.raises(AssertionError, match="autograd learner ran"):
        pop.learn()
    torch.cuda.synchronize()
    pop.check_errors()


def test_mutated_multibinary_agent_still_learns_fused(monkeypatch):
    """After an architecture mutation the agent's new population routes by the
    same rule: the fused learner when the check admits the mutated layer list,
    else the autograd learner."""
    from agilerl_amd.algorithms.ppo import PPO
    from agilerl_amd.envs import Box, MultiBinary
    from agilerl_amd.population.learner import BernGraphLearner
    from agilerl_amd.population.ppo_pop import PPOPopulation

    _setenv(monkeypatch, {})
    agent = PPO(Box(-np.inf, np.inf, (8,)), MultiBinary(5), num_envs=4, learn_step=16, batch_size=8)
    old = agent.population.spec
    assert agent.architecture_mutation(0.5, np.random.default_rng(0)) is not None
    state = agent._pending_state  # the mutated networks, as the engine's regroup receives them
    assert state is not None and state.spec.shape_key() != old.shape_key()
    pop = PPOPopulation(state.spec, 1, 4, learn_step=16, batch_size=8, lr=1e-3, device=DEV, init_params=False)
    pop.params.data[0].copy_(state.params)
    assert pop.multibinary and pop.spec.n_actions == 5
    _fill(pop, 4)
    admitted = pop.spec.bern_learn_descriptor() is not None
    assert (pop.bern_learn_descriptor() is not None) == admitted and pop._fused_learner() == admitted
    before = pop.params.data.clone()
    np.random.seed(3)
    loss = pop.learn()
    torch.cuda.synchronize()
    pop.check_errors()
    assert bool(torch.isfinite(loss).all()) and not torch.equal(pop.params.data, before)
    assert admitted  # one node / layer mutation of the default network stays inside the graph learner
    assert isinstance(pop._fused, BernGraphLearner)


def test_bern_dropin_train_on_policy(monkeypatch):
    """create_population + train_on_policy, tournament and mutations on, as
    built by default: every learn() runs the fused learner; fitnesses and
    losses are finite."""
    from agilerl_amd.envs import Box, MultiBinary, SyntheticVecEnv
    from agilerl_amd.hpo.mutation import Mutations
    from agilerl_amd.hpo.tournament import TournamentSelection
    from agilerl_amd.population.ppo_pop import PPOPopulation
    from agilerl_amd.training import train_on_policy
    from agilerl_amd.utils import create_population

    _setenv(monkeypatch, {})
    losses, learners = [], []
    learn = PPOPopulation.learn

    def recorded(self, *a, **k):
        losses.append(learn(self, *a, **k))
        learners.append(type(getattr(self, "_fused", None)).__name__ if self._fused_learner() else "autograd")
        return losses[-1]

    monkeypatch.setattr(PPOPopulation, "learn", recorded)
    obs_space, act_space = Box(-np.inf, np.inf, (8,)), MultiBinary(5)
    INIT_HP = {"BATCH_SIZE": 32, "LR": 1e-3, "LEARN_STEP": 64, "UPDATE_EPOCHS": 2}
    pop = create_population("PPO", None, INIT_HP, obs_space, act_space, population_size=2, num_envs=8)
    assert pop[0].population._fused_learner()
    env = SyntheticVecEnv(8, seed=3, p_done=0.05, max_episode_steps=40, n_binary=5)
    np.random.seed(0)
    torch.manual_seed(0)
    mut = Mutations(no_mutation=0.2, architecture=0.4, new_layer_prob=0.5, parameters=0.2, activation=0, rl_hp=0.2,
                    rand_seed=1)
    pop, fits = train_on_policy(env, "Synthetic", "PPO", pop, INIT_HP=INIT_HP, max_steps=384, evo_steps=128,
                                eval_loop=1, tournament=TournamentSelection(2, True, 2, 1), mutation=mut,
                                verbose=False)
    torch.cuda.synchronize()
    assert len(fits) == 3 and all(len(f) == 2 and np.all(np.isfinite(f)) for f in fits)
    assert len(losses) >= 3 and all(bool(torch.isfinite(x).all()) for x in losses)
    assert "BernGraphLearner" in learners and set(learners) <= {"BernGraphLearner", "autograd"}, set(learners)
    for a in pop:
        a.population.check_errors()
        assert a.spec.head == "multibinary" and a.spec.n_actions == 5
