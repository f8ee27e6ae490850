"""PPO for Box action spaces on the GPU: agx_ppo_act_gauss_graph (greedy and
sampled, against the torch forward and the numpy Philox restatement),
agx_ppo_gauss_loss_fwd_bwd against the float64 restatement (tests/gauss_twin.py,
pinned to the reference by tests/test_gauss_ppo_cpu.py), one learner update
against a pure-torch twin, and the drop-in create_population /
train_on_policy run on a Box env."""

import os

import numpy as np
import pytest
import torch

from tests import gauss_twin as G

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = {
    "default": dict(),
    "latent_56_two_layer_head": dict(latent_dim=56, actor_hidden=[48, 40]),
}


def _spec(A, shape="default", **kw):
    from agilerl_amd.population.nets import GaussianActorCriticSpec

    return GaussianActorCriticSpec(obs_dim=8, n_actions=A, **SHAPES[shape], **kw)


def _pop(A, shape="default", P=3, N=21, log_std=None, **kw):
    from agilerl_amd.population.ppo_pop import PPOPopulation

    spec = _spec(A, shape)
    pop = PPOPopulation(spec, P, N, learn_step=2 * N, batch_size=N, device=DEV, seed_base=5, **kw)
    if log_std is not None:
        spec.log_std_view(pop.params.data).copy_(torch.as_tensor(log_std, dtype=torch.float32, device=DEV))
    return pop


def _step(pop, obs, *, sample, counter=0, clip=None, flat=False):
    from agilerl_amd.population.learner import policy_step_gauss

    P, N, A = pop.P, pop.N, pop.spec.n_actions
    out = dict(actions=torch.full((P, N, A), float("nan"), device=DEV),
               log_probs=torch.empty(P, N, device=DEV), values=torch.empty(P, N, device=DEV),
               entropy=torch.empty(P, N, device=DEV))
    af = torch.full((P * N * A,), float("nan"), device=DEV) if flat else None
    policy_step_gauss(pop, pop.gauss_descriptor(), obs, N * 8, sample=sample, counter=counter, out_agent_stride=N,
                      actions_flat=af, clip=clip, **out)
    out["flat"] = None if af is None else af.view(P, N, A)
    return {k: (v.cpu() if v is not None else None) for k, v in out.items()}


def _obs(P, N, seed=1):
    return torch.randn(P, N, 8, generator=torch.Generator().manual_seed(seed)).to(DEV)


# ---- 1. the policy step, greedy --------------------------------------------------- #
@pytest.mark.parametrize("few", ["few", "general"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("A", [1, 3, 6, 16, 17, 32])
def test_gauss_policy_step_greedy_matches_torch_forward(A, shape, few, monkeypatch):
    """sample = 0: the action is the mean; mean and value against spec.forward
    at the bar of test_graph_policy_step_matches_torch_forward, the log-prob of
    the mean and the entropy against the float64 formulas.  21 envs: two row
    blocks, the second partial; A = 16 / 17: either side of the 16-lane split
    (17: the second dimension per lane), A = 32: the maximum.  Both
    forward forms (AGX_GRAPH_FEW=0: the general one)."""
    if few == "general":
        monkeypatch.setenv("AGX_GRAPH_FEW", "0")
    P, N = 3, 21
    rng = np.random.default_rng(A)
    ls = rng.uniform(-1.0, 0.5, (P, A)).astype(np.float32)
    pop = _pop(A, shape, P, N, log_std=ls)
    obs = _obs(P, N)
    out = _step(pop, obs, sample=False)
    mean, value = pop.spec.forward(pop.params.data, obs)
    torch.testing.assert_close(out["actions"], mean.cpu(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(out["values"], value.view(P, N).cpu(), rtol=1e-4, atol=1e-5)
    lp, H = G.logp_entropy(out["actions"].numpy(), ls[:, None, :], out["actions"].numpy())
    np.testing.assert_allclose(out["entropy"].numpy(), H, rtol=1e-6)
    np.testing.assert_allclose(out["log_probs"].numpy(), lp, rtol=1e-5, atol=1e-5 * A)


# ---- 2. the policy step, sampled ---------------------------------------------------- #
@pytest.mark.parametrize("P,N", [(3, 21), (2, 2048)])
@pytest.mark.parametrize("log_std", [0.0, -1.0])
def test_gauss_policy_step_samples_the_philox_stream(log_std, P, N):
    """(a - mu) / sigma against the numpy restatement of the Philox -> normal
    mapping (agx_gauss.h): |eps| <= 5.9 and a few float32 ulp of logf / cospif
    under a correctly rounded sqrtf give <= 4e-6, so atol 1e-5 max(1, |eps|),
    plus the rounding of the stored a (|a| 2^-23 / sigma).  The log-prob against
    the float64 formula on the stored (a, mu, log_std): each dimension's term
    is <= ~18 with a few ulp of error, so rtol 1e-5, atol 1e-5 A."""
    _sampled_step_follows_philox(6, log_std, P, N)


@pytest.mark.parametrize("log_std", [0.0, -1.0])
@pytest.mark.parametrize("A", [16, 32])
def test_gauss_policy_step_samples_the_philox_stream_wide(A, log_std):
    """The same at A = 16 (the last dimension of a lane's first slot) and at
    A = 32 (every lane's second slot in use: the most the kernel takes)."""
    _sampled_step_follows_philox(A, log_std, 3, 21)


def _sampled_step_follows_philox(A, log_std, P, N):
    pop = _pop(A, "default", P, N, log_std=np.full((P, A), log_std, np.float32))
    obs = _obs(P, N)
    mu = _step(pop, obs, sample=False)["actions"].numpy().astype(np.float64)
    out = _step(pop, obs, sample=True, counter=G.COUNTER)
    a = out["actions"].numpy().astype(np.float64)
    sigma = float(np.exp(np.float32(log_std)))
    eps = G.population_eps(P, N, A, pop.act_seed, G.COUNTER, env_base=pop.env_base_d.cpu().numpy())
    got = (a - mu) / sigma
    tol = 1e-5 * np.maximum(1.0, np.abs(eps)) + np.abs(a) * 2.0 ** -23 / sigma
    worst = float(np.max(np.abs(got - eps) / tol))
    print(f"eps: worst |err| / tol = {worst:.3f}, max |err| = {np.abs(got - eps).max():.3e}")
    assert worst <= 1.0
    lp, _ = G.logp_entropy(mu, np.float32(log_std), a)
    np.testing.assert_allclose(out["log_probs"].numpy(), lp, rtol=1e-5, atol=1e-5 * A)


def test_gauss_policy_step_streams_and_clipping():
    """Equal bits for an equal (seed, counter); another counter draws other
    actions; agent 2 alone (its env base set) draws what it draws among three;
    clip_low / clip_high bound only the env's copy."""
    P, N, A = 3, 21, 6
    pop = _pop(A, "default", P, N, log_std=np.zeros((P, A), np.float32))
    obs = _obs(P, N)
    one = _step(pop, obs, sample=True, counter=G.COUNTER, flat=True)
    two = _step(pop, obs, sample=True, counter=G.COUNTER)
    other = _step(pop, obs, sample=True, counter=G.COUNTER + 1)
    for k in ("actions", "log_probs", "values", "entropy"):
        assert torch.equal(one[k], two[k]), k
    assert torch.equal(one["flat"], one["actions"])  # no bounds: the env gets the stored action
    assert not torch.equal(one["actions"], other["actions"])
    assert (one["actions"] != other["actions"]).float().mean() > 0.99

    solo = _pop(A, "default", 1, N, agent_offset=2, global_pop_size=3)
    assert solo.act_seed == pop.act_seed and solo.env_base_d.tolist() == [2 * N]
    solo.params.data[0].copy_(pop.params.data[2])
    alone = _step(solo, obs[2:3].contiguous(), sample=True, counter=G.COUNTER)
    assert torch.equal(alone["actions"][0], one["actions"][2])
    assert torch.equal(alone["log_probs"][0], one["log_probs"][2])

    lo, hi = (torch.full((A,), v, device=DEV) for v in (-0.5, 0.5))
    cl = _step(pop, obs, sample=True, counter=G.COUNTER, clip=(lo, hi), flat=True)
    assert torch.equal(cl["actions"], one["actions"]) and torch.equal(cl["log_probs"], one["log_probs"])
    assert torch.equal(cl["flat"], one["actions"].clamp(-0.5, 0.5))
    assert float(cl["flat"].abs().max()) <= 0.5 and float(one["actions"].abs().max()) > 0.5


# ---- 3. the loss kernel ------------------------------------------------------------- #
def _loss_call(rec, b, clip, vf, ent):
    from agilerl_amd import kernels as K

    t = lambda k: None if rec[k] is None else torch.from_numpy(rec[k]).to(DEV)  # noqa: E731
    out = K.ppo_gauss_loss_fwd_bwd(t("mean"), t("value"), t("log_std"), t("actions"), t("old_logp"), t("adv"),
                                   t("ret"), t("old_v"), b, clip, vf, ent, index=t("index"))
    torch.cuda.synchronize()
    return [x.cpu() for x in out]


def _float32_formula_error(rec, b, clip, vf, ent, ref):
    """Worst error of the SAME formula evaluated in float32 torch on the CPU
    against the float64 restatement, for g_mean and g_log_std: what any
    float32 evaluation of these inputs loses (the kernel gets 4x this for a
    different but equally valid summation order)."""
    S, A = rec["mean"].shape
    nmb = S // b
    t = lambda k: torch.from_numpy(rec[k])  # noqa: E731
    src = torch.arange(S) if rec["index"] is None else t("index")
    mean, ls = t("mean"), t("log_std").repeat_interleave(b, 0)
    a = t("actions")[src]
    var = torch.exp(2 * ls)
    z = a - mean
    logp = (-0.5 * (z * z / var + 2 * ls + np.float32(G.LOG_2PI))).sum(-1)
    ratio = torch.exp(logp - t("old_logp")[src])
    adv = t("adv")[src]
    p1, p2 = -adv * ratio, -adv * ratio.clamp(1 - clip, 1 + clip)
    half = lambda x, y: torch.where(x > y, 1.0, torch.where(x == y, 0.5, 0.0))  # noqa: E731
    inr = ((ratio >= 1 - clip) & (ratio <= 1 + clip)).float()
    g_lp = (half(p1, p2) * -adv + half(p2, p1) * -adv * inr) / b * ratio
    g_mean = g_lp[:, None] * z / var
    g_ls = (g_lp[:, None] * (z * z / var - 1)).view(nmb, b, A).sum(1) - np.float32(ent)
    return (float(np.abs(g_mean.double().numpy() - ref["g_mean"]).max()),
            float(np.abs(g_ls.double().numpy() - ref["g_log_std"]).max()))


@pytest.mark.parametrize("gather", [False, True], ids=["direct", "gather"])
@pytest.mark.parametrize("b,nmb", [(1, 1), (5, 3), (6, 5), (128, 8)])
@pytest.mark.parametrize("A", [1, 3, 6, 16, 17, 32])
def test_gauss_loss_matches_float64_restatement(A, b, nmb, gather):
    """agx_ppo_gauss_loss_fwd_bwd against tests/gauss_twin.py loss_and_grads
    (float64), rows on the tie rules included: adv = 0 and every unclipped row
    (both surrogates equal: maximum's 1/2 : 1/2), value == old_value (both
    value losses equal), value - old_value exactly +-clip (the closed clamp
    interval; clip = 0.25 is exact in float32 and float64).  A ratio exactly
    on 1 +- clip other than through adv = 0 cannot be written down for both
    precisions at once (exp of a float32 log-prob difference), so the closed
    interval of the ratio clamp is covered by the value clamp's edge rows, which
    go through the same rule in loss_sample.  (b, nmb) = (6, 5): a batch that
    is no multiple of the four rows per pass, and one full block of four
    minibatches followed by a partial one.

    Bars: the categorical kernel's (tests/test_kernels_gpu.py): rtol 1e-5 /
    atol 1e-8 on the gradients, rtol 1e-5 / atol 1e-6 on the stats; for g_mean
    and g_log_std at least 4x the worst error of the same formula in float32
    torch on the CPU (measured figures: DESIGN.md §4)."""
    clip, vf, ent = 0.25, 0.5, 0.01
    rec = G.loss_inputs(A, b, nmb, (b * nmb + 13) if gather else None, 1000 + 31 * A + b, clip)
    ref = G.loss_and_grads(*(rec[k] for k in ("mean", "value", "log_std", "actions", "old_logp", "adv", "ret",
                                              "old_v", "index")), b, clip, vf, ent)
    g_mean, g_value, g_ls, stats = (x.double().numpy() for x in _loss_call(rec, b, clip, vf, ent))
    e_mean, e_ls = _float32_formula_error(rec, b, clip, vf, ent, ref)
    err = {k: float(np.abs(got - ref[k]).max()) for k, got in (("g_mean", g_mean), ("g_value", g_value),
                                                               ("g_log_std", g_ls), ("stats", stats))}
    print(f"A={A} b={b} nmb={nmb} gather={gather}: kernel max |err| {err}; float32 torch formula: "
          f"g_mean {e_mean:.3e} g_log_std {e_ls:.3e}")
    np.testing.assert_allclose(g_value, ref["g_value"], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(stats[:, :6], ref["stats"][:, :6], rtol=1e-5, atol=1e-6)
    assert np.all(stats[:, 6:] == 0)
    for got, want, e32 in ((g_mean, ref["g_mean"], e_mean), (g_ls, ref["g_log_std"], e_ls)):
        tol = np.maximum(1e-5 * np.abs(want) + 1e-8, 4 * e32)
        assert np.all(np.abs(got - want) <= tol), float(np.max(np.abs(got - want) / tol))
    again = _loss_call(rec, b, clip, vf, ent)
    assert torch.equal(again[2], torch.from_numpy(g_ls).float())  # g_log_std: equal bits every launch
    assert torch.equal(again[0], torch.from_numpy(g_mean).float())


# ---- 4. one learner update ---------------------------------------------------------- #
def _filled_population(ent_coef, max_grad_norm=0.5, seed=3):
    """P = 2, N = 8, T = 4 with a rollout from the policy-step kernel itself."""
    from agilerl_amd.population.ppo_pop import PPOPopulation

    P, N, T, A = 2, 8, 4, 6
    spec = _spec(A, action_std_init=0.0)
    pop = PPOPopulation(spec, P, N, learn_step=T * N, batch_size=16, update_epochs=1, lr=1e-3, ent_coef=ent_coef,
                        max_grad_norm=max_grad_norm, device=DEV, seed_base=seed)
    g = torch.Generator().manual_seed(seed)
    pop.obs.copy_(torch.randn(P, T, N, 8, generator=g))
    for t in range(T):
        pop.act_into(t)
    pop.rewards.copy_(torch.randn(P, T, N, generator=g))
    pop.dones.copy_((torch.rand(P, T, N, generator=g) < 0.1).to(torch.uint8))
    pop.finish_rollout(torch.randn(P, N, 8, generator=g).to(DEV), torch.zeros(P, N, dtype=torch.uint8, device=DEV))
    return pop


def test_gauss_learner_update_matches_torch_twin():
    """One epoch of two 16-row minibatches per agent from the same state,
    against an independent pure-torch twin: spec.forward, nets.gaussian, the
    ppo.py loss with torch ops, clip_grad_norm_ over the two groups and
    torch.optim.Adam.  The first Adam moment (log_std's included) by the
    `close` criterion of tests/test_dynamic_shapes_gpu.py; log_std moves; and
    the critic group does not see ent_coef (the entropy touches only log_std).
    That last comparison runs both updates without the gradient clip: log_std
    is in the actor clip group, so an active clip would rescale the encoder's
    step by ent_coef and the second minibatch's critic gradients with it — a
    property of the clip, not of the entropy gradient under test."""
    from agilerl_amd.population.nets import gaussian

    np.random.seed(11)
    pop = _filled_population(0.01)
    spec, P, S, A = pop.spec, pop.P, pop.S, pop.spec.n_actions
    p0 = pop.params.data.clone()
    perms = pop.permutations().clone()
    pop._learn_torch(perms)
    torch.cuda.synchronize()
    adv = pop.advantages.view(P, S)  # normalised in place by the learn
    lo, hi = spec.log_std, spec.log_std + A
    assert not torch.equal(pop.params.data[:, lo:hi], p0[:, lo:hi])

    def close(name, got, want, rtol):
        got, want = got.double().cpu().numpy().ravel(), want.double().cpu().numpy().ravel()
        bad = np.abs(got - want) > rtol * (np.abs(want) + np.sqrt(np.mean(want * want)))
        assert bad.mean() <= 1e-4, (name, int(bad.sum()), want.size)

    for p in range(P):
        w = p0[p:p + 1].clone().requires_grad_(True)
        opt = torch.optim.Adam([w], lr=1e-3, eps=1e-8)
        for s0 in range(0, S, 16):
            idx = perms[0][p, s0:s0 + 16]
            mean, value = spec.forward(w, pop.obs.view(P, S, -1)[p, idx].unsqueeze(0))
            logp, ent = gaussian(mean[0], w[:, lo:hi], pop.actions.view(P, S, A)[p, idx])
            loss, _ = G.torch_loss(logp, ent, value[0], pop.log_probs.view(P, S)[p, idx], adv[p, idx],
                                   pop.returns.view(P, S)[p, idx], pop.values.view(P, S)[p, idx], pop.clip_coef,
                                   pop.vf_coef, 0.01)
            opt.zero_grad()
            loss.backward()
            g = w.grad[0]
            for a, b in ((0, spec.actor_end), (spec.actor_end, spec.n_params)):  # clip_grad_norm_ per group, ppo.py:910-911
                g[a:b].mul_(torch.clamp(pop.max_grad_norm / (g[a:b].norm() + 1e-6), max=1.0))
            opt.step()
        st = opt.state[w]
        close(f"{p} exp_avg", pop.opt.exp_avg[p], st["exp_avg"][0], 1e-4)
        close(f"{p} exp_avg log_std", pop.opt.exp_avg[p, lo:hi], st["exp_avg"][0, lo:hi], 1e-4)
        close(f"{p} params", pop.params.data[p], w.detach()[0], 1e-4)

    ends = []
    for ent_coef in (0.01, 0.05):
        free = _filled_population(ent_coef, max_grad_norm=1e9)
        assert torch.equal(free.params.data, p0)
        free._learn_torch(perms)
        ends.append(free.params.data.clone())
    c = spec.actor_end
    assert torch.equal(ends[0][:, c:], ends[1][:, c:]) and not torch.equal(ends[0][:, c:], p0[:, c:])
    assert not torch.equal(ends[0][:, lo:hi], ends[1][:, lo:hi])


# ---- 5. drop-in ----------------------------------------------------------------------- #
def test_gauss_dropin_create_population_train_on_policy(tmp_path, monkeypatch):
    """create_population("PPO", Box actions) + train_on_policy on the
    continuous synthetic env: two generations with tournament and mutations;
    the rollouts and evaluations never reach torch's layer_norm (the policy
    step is the HIP kernel); float [16, 6] actions reach the env; checkpoints
    round-trip log_std and its Adam moments; inference actions are clipped."""
    import torch.nn.functional as F

    from agilerl_amd.algorithms.ppo import PPO
    from agilerl_amd.envs import Box, SyntheticVecEnv
    from agilerl_amd.hpo.mutation import Mutations
    from agilerl_amd.hpo.tournament import TournamentSelection
    from agilerl_amd.population.ppo_pop import PPOPopulation
    from agilerl_amd.population.runner import PopulationRunner, _EvalDriver
    from agilerl_amd.training import train_on_policy
    from agilerl_amd.utils import create_population

    seen = []

    class Env(SyntheticVecEnv):
        def step(self, actions, **kw):
            a = np.asarray(actions)
            seen.append((a.dtype, a.shape, bool(np.isfinite(a).all())))
            return super().step(actions, **kw)

    real_ln = F.layer_norm
    guard = {"on": 0}

    def layer_norm(*a, **k):
        if guard["on"]:
            raise AssertionError("torch layer_norm during a rollout / evaluation: the policy step fell back to torch")
        return real_ln(*a, **k)

    def guarded(fn):
        def run(*a, **k):
            guard["on"] += 1
            try:
                return fn(*a, **k)
            finally:
                guard["on"] -= 1
        return run

    monkeypatch.setattr(F, "layer_norm", layer_norm)
    monkeypatch.setattr(PopulationRunner, "collect", guarded(PopulationRunner.collect))
    monkeypatch.setattr(_EvalDriver, "_request_step", guarded(_EvalDriver._request_step))
    losses = []
    learn = PPOPopulation.learn
    monkeypatch.setattr(PPOPopulation, "learn", lambda self, *a, **k: losses.append(learn(self, *a, **k)) or losses[-1])

    obs_space, act_space = Box(-np.inf, np.inf, (8,)), Box(-1.0, 1.0, (6,))
    INIT_HP = {"BATCH_SIZE": 32, "LR": 1e-3, "LEARN_STEP": 64, "UPDATE_EPOCHS": 2, "ACTION_STD_INIT": 0.25}
    pop = create_population("PPO", None, INIT_HP, obs_space, act_space, population_size=2, num_envs=8)
    assert pop[0].population.gaussian and pop[0].population.actions.shape[-1] == 6
    assert pop[0].population.fused_descriptor() is None and pop[0].population.learn_descriptor() is None
    env = Env(16, seed=3, p_done=0.05, max_episode_steps=40, action_dim=6)
    np.random.seed(0)
    mut = Mutations(no_mutation=0.3, architecture=0, new_layer_prob=0.2, parameters=0.3, activation=0, rl_hp=0.4,
                    rand_seed=1)
    pop, fits = train_on_policy(env, "Synthetic", "PPO", pop, INIT_HP=INIT_HP, max_steps=256, evo_steps=128,
                                eval_loop=1, tournament=TournamentSelection(2, True, 2, 1), mutation=mut,
                                verbose=False)
    assert len(fits) == 2 and all(len(f) == 2 and np.all(np.isfinite(f)) for f in fits)
    assert all(len(a.fitness) == 2 for a in pop)
    assert seen and all(s == (np.dtype(np.float32), (16, 6), True) for s in seen), set(seen)
    assert len(losses) >= 4 and all(bool(torch.isfinite(x).all()) for x in losses)

    agent = pop[0]
    spec = agent.spec
    ck = os.path.join(tmp_path, "box.pt")
    gen = torch.Generator(device=DEV).manual_seed(2)  # moments the last mutation may have reset: any non-zero rows
    agent.population.opt.exp_avg[agent.row].normal_(generator=gen)
    agent.population.opt.exp_avg_sq[agent.row].uniform_(generator=gen)
    agent.save_checkpoint(ck)
    back = PPO.load(ck, device=DEV)
    assert back.population.gaussian and back.action_std_init == 0.25
    lo, hi = spec.log_std, spec.log_std + 6
    for a, b in ((back.population.params.data[0], agent.population.params.data[agent.row]),
                 (back.population.opt.exp_avg[0], agent.population.opt.exp_avg[agent.row]),
                 (back.population.opt.exp_avg_sq[0], agent.population.opt.exp_avg_sq[agent.row])):
        assert torch.equal(a, b) and float(b[lo:hi].abs().max()) > 0
    assert tuple(back.state_dict()["actor.head_net.log_std"].shape) == (1, 6)

    obs = np.random.default_rng(0).standard_normal((64, 8)).astype(np.float32) * 3
    with torch.no_grad():  # a policy wide enough that samples leave the bounds
        spec.log_std_view(back.population.params.data).fill_(1.0)
    a_train = back.get_action(obs)[0]
    back.training = False
    a_test, lp, ent, val = back.get_action(obs)
    assert a_train.shape == (64, 6) and a_train.dtype == np.float32 and np.abs(a_train).max() > 1.0
    assert a_test.shape == (64, 6) and np.abs(a_test).max() <= 1.0 and (np.abs(a_test) == 1.0).any()
    assert lp.shape == (64,) and ent.shape == (64,) and val.shape == (64,)


def test_gauss_standalone_agent_learn_experiences_and_rollout_buffer():
    """A standalone Box PPO: get_action's float actions through the deprecated
    learn(experiences) and through rollout_buffer.add + learn(); both move
    log_std and return finite losses."""
    from agilerl_amd.algorithms.ppo import PPO
    from agilerl_amd.envs import Box

    T, N, A = 4, 4, 3
    agent = PPO(Box(-np.inf, np.inf, (8,)), Box(-1.0, 1.0, (A,)), num_envs=N, learn_step=T * N, batch_size=8,
                update_epochs=2, lr=1e-3, action_std_init=0.2)
    rng = np.random.default_rng(0)
    np.random.seed(0)
    obs = rng.standard_normal((T, N, 8)).astype(np.float32)
    steps = [agent.get_action(obs[t]) for t in range(T)]
    actions, logp, values = (np.stack([s[i] for s in steps]) for i in (0, 1, 3))
    assert actions.shape == (T, N, A) and actions.dtype == np.float32 and logp.shape == (T, N)
    want, _ = G.logp_entropy(agent.population.evaluate(torch.from_numpy(obs[0]).to(DEV).view(1, N, 8)).cpu().numpy()[0],
                             np.float32(0.2), actions[0])
    np.testing.assert_allclose(logp[0], want, rtol=1e-5, atol=1e-5 * A)
    rewards = rng.standard_normal((T, N)).astype(np.float32)
    dones = (rng.random((T, N)) < 0.1).astype(np.float32)
    ls = lambda: agent.state_dict()["actor.head_net.log_std"].clone()  # noqa: E731
    ls0 = ls()
    assert torch.equal(ls0, torch.full((1, A), 0.2, device=DEV))
    loss = agent.learn((obs, actions, logp, rewards, dones, values, obs[-1], dones[-1]))
    ls1 = ls()
    assert np.isfinite(loss) and not torch.equal(ls1, ls0)

    buf = agent.rollout_buffer
    buf.reset()
    for t in range(T):
        buf.add(obs[t], actions[t], rewards[t], dones[t], values[t], logp[t])
    assert torch.equal(agent.population.actions[0].cpu(), torch.from_numpy(actions))
    buf.compute_returns_and_advantages(values[-1], dones[-1])
    loss = agent.learn()
    assert np.isfinite(loss) and not torch.equal(ls(), ls1)

    from agilerl_amd.envs import SyntheticVecEnv

    seen = []

    class Env(SyntheticVecEnv):
        def step(self, actions, **kw):
            seen.append(np.asarray(actions))
            return super().step(actions, **kw)

    with torch.no_grad():
        agent.spec.log_std_view(agent.population.params.data).fill_(1.0)  # samples leave the bounds
    fit = agent.test(Env(N, seed=1, p_done=0.2, max_episode_steps=10, action_dim=A), loop=1)
    assert np.isfinite(fit) and agent.fitness == [fit] and agent.training
    assert seen and all(a.shape == (N, A) and np.abs(a).max() <= 1.0 for a in seen)
    assert any((np.abs(a) == 1.0).any() for a in seen)  # test() acts with the env's copy clipped


def test_gauss_architecture_mutations_train():
    """The reference's call site (one shared N-env, cloned per agent) with
    architecture mutations on every agent: the mutated Box agents regroup by
    shape and keep training and evaluating through the Gaussian kernels, and
    an agent's log_std survives its mutation bit for bit."""
    from agilerl_amd.envs import Box, SyntheticVecEnv
    from agilerl_amd.hpo.mutation import Mutations
    from agilerl_amd.hpo.tournament import TournamentSelection
    from agilerl_amd.training import train_on_policy
    from agilerl_amd.utils import create_population

    INIT_HP = {"BATCH_SIZE": 32, "LR": 1e-3, "LEARN_STEP": 64, "UPDATE_EPOCHS": 1}
    pop = create_population("PPO", None, INIT_HP, Box(-np.inf, np.inf, (8,)), Box(-1.0, 1.0, (3,)),
                            population_size=2, num_envs=8)
    np.random.seed(1)
    torch.manual_seed(1)
    mut = Mutations(no_mutation=0, architecture=1.0, new_layer_prob=0.5, parameters=0, activation=0, rl_hp=0,
                    rand_seed=3)
    env = SyntheticVecEnv(8, seed=2, p_done=0.05, max_episode_steps=40, action_dim=3)
    pop, fits = train_on_policy(env, "Synthetic", "PPO", pop, INIT_HP=INIT_HP, max_steps=192, evo_steps=64,
                                eval_loop=1, tournament=TournamentSelection(2, True, 2, 1), mutation=mut,
                                verbose=False)
    assert len(fits) == 3 and all(np.all(np.isfinite(f)) for f in fits)
    assert any(a.mut not in (None, "None") for a in pop)
    for a in pop:
        assert a.spec.head == "gaussian" and a.population.gaussian
        ls = a.state_dict()["actor.head_net.log_std"]
        assert tuple(ls.shape) == (1, 3) and bool(torch.isfinite(ls).all())
    agent = next(a for a in pop if a.can_mutate_architecture)
    before = agent.state_dict()["actor.head_net.log_std"].clone()
    assert agent.architecture_mutation(0.5, np.random.default_rng(0)) is not None
    assert torch.equal(agent.state_dict()["actor.head_net.log_std"], before)


# ---- 6. regression guard ---------------------------------------------------------------- #
def test_discrete_population_after_box_population_keeps_the_fused_kernels():
    from agilerl_amd.envs import Box, Discrete
    from agilerl_amd.utils import create_population

    obs_space = Box(-np.inf, np.inf, (8,))
    box = create_population("PPO", None, {"LEARN_STEP": 64}, obs_space, Box(-1.0, 1.0, (6,)), population_size=2,
                            num_envs=8)
    assert box[0].population.actions.dtype == torch.float32
    net = {"encoder_config": {"hidden_size": [64]}, "head_config": {"hidden_size": [64]}, "latent_dim": 64}
    disc = create_population("PPO", net, {"LEARN_STEP": 64}, obs_space, Discrete(4), population_size=2, num_envs=8)
    population = disc[0].population
    assert not population.gaussian and population.fused_descriptor() is not None
    assert population.actions.dtype == torch.int64 and population.actions.shape == (2, 8, 8)
