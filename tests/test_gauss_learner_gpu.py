"""agx_ppo_learn_gauss_graph (graph_learner.hip, GAUSS instantiations): the
runtime-shape fused learner with a Gaussian head, against the autograd learner
(PPOPopulation._learn_torch, itself pinned to an independent torch twin by
tests/test_gauss_ppo_gpu.py::test_gauss_learner_update_matches_torch_twin) on
identical inputs and permutations.  Helpers and bars are those of
tests/test_graph_learner_gpu.py, restated here for float actions."""

import ctypes

import numpy as np
import pytest
import torch

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


def _setenv(monkeypatch, form):
    for k in ("AGX_GRAPH_FEW", "AGX_GRAPH_SPLIT", "AGX_GRAPH_ROWS", "AGX_GAUSS_FUSED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in form.items():
        monkeypatch.setenv(k, v)


def _fill(pop, seed):
    """A rollout for ``pop``: observations randn; actions = mean + sigma randn
    from the population's own forward; log_probs = the true log-prob + 0.05
    randn (both clip branches occur); values + 0.1 randn."""
    from agilerl_amd.population.nets import gaussian

    spec, P, D = pop.spec, pop.P, pop.spec.obs_dim
    g = torch.Generator(device=DEV).manual_seed(seed + 99)
    pop.obs.copy_(torch.randn(pop.obs.shape, device=DEV, generator=g))
    pop.rewards.copy_(torch.randn(pop.rewards.shape, device=DEV, generator=g))
    pop.dones.copy_((torch.rand(pop.dones.shape, device=DEV, generator=g) < 0.05).to(torch.uint8))
    with torch.no_grad():
        mean, value = spec.forward(pop.params.data, pop.obs.view(P, -1, D))
        ls = spec.log_std_view(pop.params.data).unsqueeze(1)
        act = mean + torch.exp(ls) * torch.randn(mean.shape, device=DEV, generator=g)
        lp, _ = gaussian(mean, ls, act)
    pop.actions.copy_(act.view_as(pop.actions))
    pop.values.copy_(value.view_as(pop.values) + 0.1 * torch.randn(pop.values.shape, device=DEV, generator=g))
    pop.log_probs.copy_(lp.view_as(pop.log_probs) + 0.05 * torch.randn(pop.log_probs.shape, device=DEV, generator=g))
    last_obs = torch.randn(P, pop.N, D, device=DEV, generator=g)
    pop.finish_rollout(last_obs, torch.zeros(P, pop.N, dtype=torch.uint8, device=DEV))


def _pop(shape, A=6, P=3, N=16, learn_step=128, batch=64, epochs=1, seed=0, std=0.0, **kw):
    from agilerl_amd.population.nets import GaussianActorCriticSpec
    from agilerl_amd.population.ppo_pop import PPOPopulation

    spec = GaussianActorCriticSpec(obs_dim=8, n_actions=A, action_std_init=std, **SHAPES[shape])
    pop = PPOPopulation(spec, P, N, learn_step=learn_step, batch_size=batch, lr=1e-3, update_epochs=epochs,
                        seeds=[seed + i for i in range(P)], device=DEV, fused=True, **kw)
    _fill(pop, seed)
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
    from agilerl_amd.population.learner import GaussGraphLearner, fused_learn

    assert pop.learn_descriptor() is None and pop.gauss_learn_descriptor() is not None
    loss = fused_learn(pop, perms).clone()
    torch.cuda.synchronize()
    assert isinstance(pop._fused, GaussGraphLearner)
    pop.check_errors()
    return loss


def _workspace_bytes(pop):
    from agilerl_amd import _lib

    return _lib.load().agx_ppo_learn_gauss_graph_workspace_bytes(
        ctypes.byref(pop.gauss_learn_descriptor()), pop.spec.log_std, pop.P, pop.S, pop.update_epochs, pop.split_batch)


def _compare(pop, perms):
    """torch learner vs the Gaussian graph learner from the same state: the
    drift bars of tests/test_graph_learner_gpu.py::_compare, and the same
    epochs run / Adam steps."""
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
    lo, hi = pop.spec.log_std, pop.spec.log_std + pop.spec.n_actions
    assert not torch.equal(pop.params.data[:, lo:hi], st[0][:, lo:hi])
    np.testing.assert_allclose(loss_g.cpu().numpy(), loss_t.cpu().numpy(), rtol=1e-4, atol=1e-7)


# ---- 1. single update, tight ---------------------------------------------------------- #
SPLITS = [(form, 64, 64, {}) for form in FORMS] + [
    ("default", 16, 16, {}),                      # one 16-row slice: the split gives one workgroup
    ("default", 16, 16, {"AGX_GRAPH_ROWS": "8"}),  # two few-row slices of 8: half of each 16-row tile is past the slice
]
# every action width on two shapes at S = 64 in each form; the 16-row rollouts on
# the widths at the ends and across the 16-lane boundary; action_std_init = -1 on
# two widths of one shape
SINGLE = ([(A, shape, 0.0, *sp) for A in (1, 6, 16, 17, 32) for shape in ("latent_56", "no_layer_norm")
           for sp in SPLITS if sp[1] == 64 or A in (1, 17, 32)] +
          [(A, "latent_56", -1.0, *sp) for A in (6, 17) for sp in SPLITS])


@pytest.mark.parametrize("A,shape,std,form,S,batch,env", SINGLE,
                         ids=[f"A{a}-{sh}-std{st}-{f}-S{s}" + ("-rows8" if e else "") for a, sh, st, f, s, _, e in SINGLE])
def test_gauss_learner_single_update_tight(A, shape, std, form, S, batch, env, monkeypatch):
    """One minibatch, one epoch: the clipped gradient of the single update
    (exp_avg = 0.1 g after Adam's first step) matches the autograd learner's,
    the log_std entries asserted on their own, and log_std moves."""
    _setenv(monkeypatch, {**FORMS[form], **env})
    pop = _pop(shape, A=A, N=16, learn_step=S, batch=batch, epochs=1, seed=5, std=std)
    st = _state(pop)
    perms = pop.permutations()
    pop._learn_torch(perms)
    g_t = pop.opt.grads.clone()
    m_t = pop.opt.exp_avg.clone()
    _restore(pop, st)
    _fused(pop, perms)
    m, mt = pop.opt.exp_avg.cpu().numpy(), m_t.cpu().numpy()
    gt = g_t.cpu().numpy()
    lo, hi = pop.spec.log_std, pop.spec.log_std + A
    am, ag = 1e-6 * np.abs(mt).max(), 1e-6 * np.abs(gt).max()
    err = np.abs(m - mt) / (1e-4 * np.abs(mt) + am)
    print(f"A={A} {shape} std={std} {form} S={S}: worst |err| / bar: all {err.max():.3f}, "
          f"log_std {err[:, lo:hi].max():.3f}")
    np.testing.assert_allclose(m[:, lo:hi], mt[:, lo:hi], rtol=1e-4, atol=am)
    np.testing.assert_allclose(m[:, lo:hi] / 0.1, gt[:, lo:hi], rtol=1e-3, atol=ag)
    np.testing.assert_allclose(m, mt, rtol=1e-4, atol=am)
    np.testing.assert_allclose(m / 0.1, gt, rtol=1e-3, atol=ag)
    assert np.abs(mt[:, lo:hi]).min() > 0
    assert not torch.equal(pop.params.data[:, lo:hi], st[0][:, lo:hi])


# ---- 2. every form, several updates ---------------------------------------------------- #
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape,A,N,learn_step,batch,epochs", [
    ("latent_56", 6, 16, 128, 64, 2),
    ("own_critic_encoder", 6, 8, 100, 32, 2),  # a short last minibatch: the second partner has no rows
    ("no_layer_norm", 17, 16, 128, 48, 1)])
def test_gauss_learner_matches_torch_learner(shape, A, N, learn_step, batch, epochs, form, monkeypatch):
    _setenv(monkeypatch, FORMS[form])
    pop = _pop(shape, A=A, N=N, learn_step=learn_step, batch=batch, epochs=epochs)
    np.random.seed(1234)
    _compare(pop, pop.permutations())


def test_gauss_learner_forms_differ_in_workspace(monkeypatch):
    """The three forms the tests above name are three different runs: the
    workspace query, which makes the call's choice, sizes each differently."""
    pop = _pop("latent_56", N=16, learn_step=128, batch=64)
    sizes = {}
    for form, env in FORMS.items():
        _setenv(monkeypatch, env)
        sizes[form] = _workspace_bytes(pop)
    assert all(v > 0 for v in sizes.values()) and len(set(sizes.values())) == 3, sizes


# ---- 3. heterogeneous hyperparameters, target_kl ------------------------------------------ #
def test_gauss_learner_heterogeneous_hparams():
    pop = _pop("latent_56", P=3, N=16, learn_step=128, batch=64, epochs=2)
    pop.set_agent_hparam(1, "batch_size", 32)
    pop.set_agent_hparam(2, "update_epochs", 1)
    pop.set_agent_hparam(0, "ent_coef", 0.05)
    _compare(pop, pop.permutations())
    assert pop._fused.epochs_run.tolist() == [2, 2, 1]


def test_gauss_learner_target_kl_stops_like_torch():
    pop = _pop("latent_56", N=16, learn_step=128, batch=32, epochs=4, target_kl=1e-4)
    _compare(pop, pop.permutations())
    assert int(pop._fused.epochs_run.min()) < 4


# ---- 4. determinism and independence ------------------------------------------------------ #
@pytest.mark.parametrize("form", list(FORMS))
def test_gauss_learner_is_deterministic_and_independent_of_the_population(form, monkeypatch):
    """Two learns from the same state give equal bits; agent 0's row after a
    P = 3 learn equals its row after a P = 1 learn from the same state and
    permutation (fixed summation order: no atomics, no dependence on the grid)."""
    _setenv(monkeypatch, FORMS[form])
    kw = dict(A=6, N=16, learn_step=128, batch=64, epochs=2, seed=11)
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


# ---- 5. routing ---------------------------------------------------------------------------- #
def _box_population():
    from agilerl_amd.envs import Box
    from agilerl_amd.utils import create_population

    INIT_HP = {"BATCH_SIZE": 32, "LR": 1e-3, "LEARN_STEP": 64, "UPDATE_EPOCHS": 2}
    agents = create_population("PPO", None, INIT_HP, Box(-np.inf, np.inf, (8,)), Box(-1.0, 1.0, (6,)),
                               population_size=2, num_envs=8)
    pop = agents[0].population
    _fill(pop, 3)
    return pop


def _layer_norm_raises(monkeypatch):
    import torch.nn.functional as F

    def layer_norm(*a, **k):
        raise AssertionError("torch layer_norm during learn(): the autograd learner ran")

    monkeypatch.setattr(F, "layer_norm", layer_norm)


def test_box_population_learns_through_the_gaussian_graph_learner(monkeypatch):
    from agilerl_amd.population.learner import GaussGraphLearner, graph_descriptor

    _setenv(monkeypatch, {})
    pop = _box_population()
    assert pop.gaussian and pop.learn_descriptor() is None and pop.fused_descriptor() is None
    assert pop.eval_descriptor() is None and graph_descriptor(pop.spec) is None
    assert pop.gauss_learn_descriptor() is not None
    lo, hi = pop.spec.log_std, pop.spec.log_std + 6
    before = pop.params.data[:, lo:hi].clone()
    np.random.seed(2)
    _layer_norm_raises(monkeypatch)
    loss = pop.learn()
    torch.cuda.synchronize()
    pop.check_errors()
    assert isinstance(pop._fused, GaussGraphLearner)
    assert bool(torch.isfinite(loss).all()) and not torch.equal(pop.params.data[:, lo:hi], before)
    assert pop.last_kl is pop._fused.kl and pop._fused.epochs_run.tolist() == [2, 2]


def test_box_population_keeps_the_autograd_learner_when_switched_off(monkeypatch):
    _setenv(monkeypatch, {"AGX_GAUSS_FUSED": "0"})
    pop = _box_population()
    assert pop.gauss_learn_descriptor() is None and pop.learn_descriptor() is None
    np.random.seed(2)
    _layer_norm_raises(monkeypatch)
    with pytest.raises(AssertionError, match="autograd learner ran"):
        pop.learn()
    torch.cuda.synchronize()
    pop.check_errors()


def test_gauss_learner_rejects_action_masks(monkeypatch):
    from agilerl_amd import _lib
    from agilerl_amd.population.learner import fused_learn

    _setenv(monkeypatch, {})
    pop = _pop("latent_56", N=16, learn_step=64, batch=64)
    perms = pop.permutations()
    p0 = pop.params.data.clone()
    pop.action_masks = torch.ones(pop.P, pop.T, pop.N, 6, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.AgxError, match="action masks"):
        fused_learn(pop, perms)
    pop.action_masks = None
    torch.cuda.synchronize()
    assert torch.equal(pop.params.data, p0)
    pop.check_errors()
