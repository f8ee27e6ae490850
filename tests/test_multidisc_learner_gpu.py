"""agx_ppo_learn_multi_graph (graph_learner.hip, the multi-categorical
instantiations): the runtime-shape fused learner with a multi-categorical head,
against the autograd learner (PPOPopulation._learn_torch, itself pinned to an
independent torch twin by
tests/test_multidisc_ppo_gpu.py::test_multi_learner_update_matches_torch_twin)
on identical inputs and permutations, and for K = 1 bit for bit against
agx_ppo_learn_graph.  Helpers and bars are those of
tests/test_gauss_learner_gpu.py, the heads and masks those of
tests/multidisc_twin.py, restated here."""

import ctypes

import numpy as np
import pytest
import torch

from tests import multidisc_twin as M

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

NVECS = M.NVECS
IDS = ["x".join(map(str, n)) if len(n) < 6 else f"{n[0]}x{len(n)}times" for n in NVECS]


def _nid(nvec):
    return IDS[NVECS.index(tuple(nvec))] if tuple(nvec) in NVECS else "x".join(map(str, nvec))


def _setenv(monkeypatch, form):
    for k in ("AGX_GRAPH_FEW", "AGX_GRAPH_SPLIT", "AGX_GRAPH_ROWS", "AGX_MULTI_FUSED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in form.items():
        monkeypatch.setenv(k, v)


def _fill(pop, seed, masks=False):
    """A rollout for ``pop``: observations randn; the actor's output weight
    times 10 (probabilities far from uniform); actions from the population's
    own policy step; with ``masks`` about a third of the logits illegal, the
    stored actions legal, and for agent 0 one logit that no stored action
    chose illegal in every row; log_probs = the true log-prob + 0.05 randn
    (both clip branches occur); values + 0.1 randn (both value branches)."""
    from agilerl_amd.population.nets import multi_categorical

    spec, P, T, N, D = pop.spec, pop.P, pop.T, pop.N, pop.spec.obs_dim
    nvec, K, L = spec.nvec, len(spec.nvec), spec.n_actions
    W, _, _, _ = spec.views(pop.params.data, spec.actor[-1])
    W.mul_(10.0)
    g = torch.Generator(device=DEV).manual_seed(seed + 99)
    pop.obs.copy_(torch.randn(pop.obs.shape, device=DEV, generator=g))
    pop.rewards.copy_(torch.randn(pop.rewards.shape, device=DEV, generator=g))
    pop.dones.copy_((torch.rand(pop.dones.shape, device=DEV, generator=g) < 0.05).to(torch.uint8))
    for t in range(T):
        pop.act_into(t)
    mk = None
    pop.never_chosen = None
    if masks:
        acts = pop.actions.reshape(-1, K).cpu().numpy()
        m = M.random_mask(np.random.default_rng(seed), P * T * N, nvec, keep=acts).reshape(P, T * N, L)
        flat0 = (acts.reshape(P, T * N, K)[0] + np.asarray(M.offsets(nvec))).ravel()
        unused = sorted(set(range(L)) - set(flat0.tolist()))
        if unused:
            pop.never_chosen = unused[0]
            m[0, :, unused[0]] = 0
        pop.action_masks.copy_(torch.from_numpy(m).view_as(pop.action_masks))
        mk = pop.action_masks.view(P, T * N, L)
    with torch.no_grad():
        logits, _ = spec.forward(pop.params.data, pop.obs.view(P, -1, D))
        lp, _ = multi_categorical(logits, nvec, pop.actions.view(P, T * N, K), mk)
    pop.values.add_(0.1 * torch.randn(pop.values.shape, device=DEV, generator=g))
    pop.log_probs.copy_(lp.view_as(pop.log_probs) + 0.05 * torch.randn(pop.log_probs.shape, device=DEV, generator=g))
    last_obs = torch.randn(P, N, D, device=DEV, generator=g)
    pop.finish_rollout(last_obs, torch.zeros(P, N, dtype=torch.uint8, device=DEV))


def _pop(shape, nvec=(3, 2), P=3, N=16, learn_step=128, batch=64, epochs=1, seed=0, masks=False, **kw):
    from agilerl_amd.population.nets import MultiDiscreteActorCriticSpec
    from agilerl_amd.population.ppo_pop import PPOPopulation

    spec = MultiDiscreteActorCriticSpec(obs_dim=8, n_actions=int(sum(nvec)), nvec=tuple(nvec), **SHAPES[shape])
    pop = PPOPopulation(spec, P, N, learn_step=learn_step, batch_size=batch, lr=1e-3, update_epochs=epochs,
                        seeds=[seed + i for i in range(P)], device=DEV, fused=True, multi_fused=True,
                        action_masks=masks, **kw)
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
    from agilerl_amd.population.learner import MultiGraphLearner, fused_learn

    assert pop.learn_descriptor() is None and pop.multi_learn_descriptor() is not None
    loss = fused_learn(pop, perms).clone()
    torch.cuda.synchronize()
    assert isinstance(pop._fused, MultiGraphLearner)
    pop.check_errors()
    return loss


def _workspace_bytes(pop):
    from agilerl_amd import _lib

    return _lib.load().agx_ppo_learn_multi_graph_workspace_bytes(
        ctypes.byref(pop.multi_learn_descriptor()), pop.multi_head(), pop.P, pop.S, pop.update_epochs,
        pop.split_batch)


def _compare(pop, perms):
    """torch learner vs the multi-categorical graph learner from the same
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
SINGLE = [(nvec, shape, S, masks) for nvec in NVECS for shape in ("latent_56", "no_layer_norm") for S in (64, 16)
          for masks in (False, True) if S == 64 or nvec in ((2,), (7, 20, 5), (2,) * 16)]


@pytest.mark.parametrize("nvec,shape,S,masks", SINGLE,
                         ids=[f"{_nid(n)}-{sh}-S{s}-{'mask' if m else 'nomask'}" for n, sh, s, m in SINGLE])
def test_multi_learner_single_update_tight(nvec, shape, S, masks, monkeypatch):
    """One minibatch, one epoch: the clipped gradient of the single update
    (exp_avg = 0.1 g after Adam's first step) matches the autograd learner's
    in every form, the actor output layer's weight and bias asserted on their
    own; a logit that is illegal in every row of an agent gets exactly 0."""
    _setenv(monkeypatch, {})
    pop = _pop(shape, nvec=nvec, N=16, learn_step=S, batch=S, epochs=1, seed=5, masks=masks)
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
        print(f"nvec={_nid(nvec)} {shape} S={S} masks={masks} {form}: worst |err| / bar: all {err.max():.3f}, "
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
            j = pop.never_chosen
            if j is not None:  # illegal in every row of agent 0: no gradient at all
                assert not mt[0, w].reshape(L, fin)[j].any() and mt[0, b][j] == 0
                assert not m[0, w].reshape(L, fin)[j].any() and m[0, b][j] == 0
        assert not torch.equal(pop.params.data, st[0])


# ---- 4. every form, several updates ---------------------------------------------------- #
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape,nvec,masks,N,learn_step,batch,epochs", [
    ("latent_56", (3, 2), False, 16, 128, 64, 2),
    ("own_critic_encoder", (5, 1, 4), True, 8, 100, 32, 2),  # a short last minibatch: the second partner has no rows
    ("no_layer_norm", (7, 20, 5), False, 16, 128, 48, 1)])
def test_multi_learner_matches_torch_learner(shape, nvec, masks, N, learn_step, batch, epochs, form, monkeypatch):
    _setenv(monkeypatch, FORMS[form])
    pop = _pop(shape, nvec=nvec, N=N, learn_step=learn_step, batch=batch, epochs=epochs, masks=masks)
    np.random.seed(1234)
    _compare(pop, pop.permutations())


# ---- 10. the three forms are three runs -------------------------------------------------- #
def test_multi_learner_forms_differ_in_workspace(monkeypatch):
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
def test_multi_learner_heterogeneous_hparams(monkeypatch):
    _setenv(monkeypatch, {})
    pop = _pop("latent_56", nvec=(3, 2, 4), P=3, N=16, learn_step=128, batch=64, epochs=2)
    pop.set_agent_hparam(1, "batch_size", 32)
    pop.set_agent_hparam(2, "update_epochs", 1)
    pop.set_agent_hparam(0, "ent_coef", 0.05)
    _compare(pop, pop.permutations())
    assert pop._fused.epochs_run.tolist() == [2, 2, 1]


def test_multi_learner_target_kl_stops_like_torch(monkeypatch):
    _setenv(monkeypatch, {})
    pop = _pop("latent_56", nvec=(3, 2, 4), N=16, learn_step=128, batch=32, epochs=4, target_kl=1e-4)
    _compare(pop, pop.permutations())  # equal epochs_run asserted there
    assert int(pop._fused.epochs_run.min()) < 4


# ---- 6. K = 1 equals the categorical learner bit for bit ------------------------------------ #
@pytest.mark.parametrize("masks", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", [2, 17, 32])
def test_single_component_equals_the_categorical_learner_bit_for_bit(n, form, masks, monkeypatch):
    """nvec = (n,): the loss row pass runs the categorical pass's float
    operations in its order, so parameters, both Adam moments, the loss and
    the approx-KL equal agx_ppo_learn_graph's at n_actions = n."""
    from agilerl_amd.population.learner import GraphLearner, fused_learn
    from agilerl_amd.population.nets import ActorCriticSpec
    from agilerl_amd.population.ppo_pop import PPOPopulation

    _setenv(monkeypatch, FORMS[form])
    kw = dict(N=16, learn_step=128, batch=64, epochs=2, seed=7)
    md = _pop("latent_56", nvec=(n,), masks=masks, **kw)
    spec = ActorCriticSpec(obs_dim=8, n_actions=n, **SHAPES["latent_56"])
    assert spec.n_params == md.spec.n_params
    disc = PPOPopulation(spec, md.P, md.N, learn_step=128, batch_size=64, lr=1e-3, update_epochs=2,
                         seeds=[7 + i for i in range(md.P)], device=DEV, fused=True, action_masks=masks)
    assert disc.fused_descriptor() is None and disc.learn_descriptor() is not None
    disc.params.data.copy_(md.params.data)
    for name in ("obs", "log_probs", "values", "advantages", "returns", "adv_stats"):
        getattr(disc, name).copy_(getattr(md, name))
    disc.actions.copy_(md.actions.squeeze(-1))
    if masks:
        disc.action_masks.copy_(md.action_masks)
    perms = md.permutations()
    loss_m = _fused(md, perms)
    loss_d = fused_learn(disc, perms).clone()
    torch.cuda.synchronize()
    disc.check_errors()
    assert type(disc._fused) is GraphLearner
    assert torch.equal(md.params.data, disc.params.data)
    assert torch.equal(md.opt.exp_avg, disc.opt.exp_avg) and torch.equal(md.opt.exp_avg_sq, disc.opt.exp_avg_sq)
    assert torch.equal(loss_m, loss_d) and torch.equal(md._fused.kl, disc._fused.kl)
    assert torch.equal(md.opt.steps, disc.opt.steps) and int(md.opt.steps.min()) == 4


# ---- 7. determinism and independence ------------------------------------------------------ #
@pytest.mark.parametrize("form", list(FORMS))
def test_multi_learner_is_deterministic_and_independent_of_the_population(form, monkeypatch):
    """Two learns from the same state give equal bits; agent 0's row after a
    P = 3 learn equals its row after a P = 1 learn from the same state and
    permutation (fixed summation order: no atomics, no dependence on the grid)."""
    _setenv(monkeypatch, FORMS[form])
    kw = dict(nvec=(5, 1, 4), N=16, learn_step=128, batch=64, epochs=2, seed=11)
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


# ---- 8. an action outside its component ----------------------------------------------------- #
def test_multi_learner_clamps_an_action_outside_its_component(monkeypatch):
    """Defined behaviour (include/agx_multi.h): a stored action outside
    [0, n_k) is clamped into its component, so the learn equals the learn of
    the rollout clamped by hand bit for bit, and no error is flagged."""
    _setenv(monkeypatch, {})
    nvec = (3, 2, 4)
    pop = _pop("latent_56", nvec=nvec, N=16, learn_step=16, batch=16, epochs=1, seed=13)
    perms = pop.permutations()
    st = _state(pop)
    good = pop.actions.clone()
    pop.actions[0, 0, 3, 0] = nvec[0] + 3
    pop.actions[1, 0, 9, 2] = -1
    loss_a = _fused(pop, perms)
    got = (pop.params.data.clone(), pop.opt.exp_avg.clone(), pop.opt.exp_avg_sq.clone())
    _restore(pop, st)
    pop.actions.copy_(good)
    pop.actions[0, 0, 3, 0] = nvec[0] - 1
    pop.actions[1, 0, 9, 2] = 0
    loss_b = _fused(pop, perms)
    for a, b in zip(got, (pop.params.data, pop.opt.exp_avg, pop.opt.exp_avg_sq)):
        assert torch.equal(a, b)
    assert torch.equal(loss_a, loss_b) and bool(torch.isfinite(loss_a).all())
    assert not torch.equal(pop.params.data, st[0])


# ---- 9. routing ---------------------------------------------------------------------------- #
def _dropin_population():
    from agilerl_amd.envs import Box, MultiDiscrete
    from agilerl_amd.utils import create_population

    INIT_HP = {"BATCH_SIZE": 32, "LR": 1e-3, "LEARN_STEP": 64, "UPDATE_EPOCHS": 2}
    agents = create_population("PPO", None, INIT_HP, Box(-np.inf, np.inf, (8,)), MultiDiscrete((3, 2)),
                               population_size=2, num_envs=8)
    pop = agents[0].population
    _fill(pop, 3)
    return pop


def _layer_norm_raises(monkeypatch):
    import torch.nn.functional as F

    def layer_norm(*a, **k):
        raise AssertionError("torch layer_norm during learn(): the autograd learner ran")

    monkeypatch.setattr(F, "layer_norm", layer_norm)


def test_multidiscrete_population_learns_through_the_fused_learner_when_switched_on(monkeypatch):
    from agilerl_amd.population.learner import MultiGraphLearner

    _setenv(monkeypatch, {"AGX_MULTI_FUSED": "1"})
    pop = _dropin_population()
    assert pop.multidiscrete and not pop.multi_fused
    assert pop.learn_descriptor() is None and pop.fused_descriptor() is None and pop.eval_descriptor() is None
    assert pop.multi_learn_descriptor() is not None and pop._fused_learner()
    before = pop.params.data.clone()
    np.random.seed(2)
    _layer_norm_raises(monkeypatch)
    loss = pop.learn()
    torch.cuda.synchronize()
    pop.check_errors()
    assert isinstance(pop._fused, MultiGraphLearner)
    assert bool(torch.isfinite(loss).all()) and not torch.equal(pop.params.data, before)
    assert pop.last_kl is pop._fused.kl and pop._fused.epochs_run.tolist() == [2, 2]


def test_multidiscrete_population_keeps_the_autograd_learner_by_default(monkeypatch):
    _setenv(monkeypatch, {})
    pop = _dropin_population()
    assert pop.multi_learn_descriptor() is None and not pop._fused_learner()
    np.random.seed(2)
    _layer_norm_raises(monkeypatch)
    with pytest.raises(AssertionError, match="autograd learner ran"):
        pop.learn()
    torch.cuda.synchronize()
    pop.check_errors()


def test_mutated_multidiscrete_agent_learns_with_the_switch_on(monkeypatch):
    """After an architecture mutation the agent's new population routes by the
    same rule: the fused learner when the check admits the mutated layer list,
    else the autograd learner."""
    from agilerl_amd.algorithms.ppo import PPO
    from agilerl_amd.envs import Box, MultiDiscrete
    from agilerl_amd.population.learner import MultiGraphLearner

    from agilerl_amd.population.ppo_pop import PPOPopulation

    _setenv(monkeypatch, {"AGX_MULTI_FUSED": "1"})
    agent = PPO(Box(-np.inf, np.inf, (8,)), MultiDiscrete((3, 2)), num_envs=4, learn_step=16, batch_size=8)
    old = agent.population.spec
    assert agent.architecture_mutation(0.5, np.random.default_rng(0)) is not None
    state = agent._pending_state  # the mutated networks, as the engine's regroup receives them
    assert state is not None and state.spec.shape_key() != old.shape_key()
    pop = PPOPopulation(state.spec, 1, 4, learn_step=16, batch_size=8, lr=1e-3, device=DEV, init_params=False)
    pop.params.data[0].copy_(state.params)
    assert pop.multidiscrete and pop.spec.nvec == (3, 2) and not pop.multi_fused
    _fill(pop, 4)
    admitted = pop.spec.multi_learn_descriptor() is not None
    assert (pop.multi_learn_descriptor() is not None) == admitted and pop._fused_learner() == admitted
    before = pop.params.data.clone()
    np.random.seed(3)
    loss = pop.learn()
    torch.cuda.synchronize()
    pop.check_errors()
    assert bool(torch.isfinite(loss).all()) and not torch.equal(pop.params.data, before)
    assert admitted  # one node / layer mutation of the default network stays inside the graph learner
    assert isinstance(pop._fused, MultiGraphLearner)


def test_multi_dropin_train_on_policy_with_the_switch_on(monkeypatch):
    """create_population + train_on_policy, tournament and mutations on, with
    AGX_MULTI_FUSED=1: every learn() runs the fused learner; fitnesses and
    losses are finite."""
    from agilerl_amd.envs import Box, MultiDiscrete, SyntheticVecEnv
    from agilerl_amd.hpo.mutation import Mutations
    from agilerl_amd.hpo.tournament import TournamentSelection
    from agilerl_amd.population.ppo_pop import PPOPopulation
    from agilerl_amd.training import train_on_policy
    from agilerl_amd.utils import create_population

    _setenv(monkeypatch, {"AGX_MULTI_FUSED": "1"})
    losses, learners = [], []
    learn = PPOPopulation.learn

    def recorded(self, *a, **k):
        losses.append(learn(self, *a, **k))
        learners.append(type(getattr(self, "_fused", None)).__name__ if self._fused_learner() else "autograd")
        return losses[-1]

    monkeypatch.setattr(PPOPopulation, "learn", recorded)
    obs_space, act_space = Box(-np.inf, np.inf, (8,)), MultiDiscrete((3, 2))
    INIT_HP = {"BATCH_SIZE": 32, "LR": 1e-3, "LEARN_STEP": 64, "UPDATE_EPOCHS": 2}
    pop = create_population("PPO", None, INIT_HP, obs_space, act_space, population_size=2, num_envs=8)
    assert pop[0].population._fused_learner()
    env = SyntheticVecEnv(8, seed=3, p_done=0.05, max_episode_steps=40, nvec=(3, 2))
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
    assert "MultiGraphLearner" in learners and set(learners) <= {"MultiGraphLearner", "autograd"}, set(learners)
    for a in pop:
        a.population.check_errors()
        assert a.spec.head == "multidiscrete" and a.spec.nvec == (3, 2)
