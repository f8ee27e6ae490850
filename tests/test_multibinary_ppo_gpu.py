"""PPO for MultiBinary action spaces on the GPU: agx_ppo_act_bern_graph (greedy
and sampled, against the torch forward and the float64 restatement of
tests/multibinary_twin.py, pinned to the reference by
tests/test_multibinary_ppo_cpu.py), agx_ppo_bern_loss_fwd_bwd against the
restatement, one autograd-learner update against a pure-torch twin, and the
drop-in create_population / train_on_policy run on a MultiBinary env.  The
tests mirror tests/test_multidisc_ppo_gpu.py at its bars."""

import os

import numpy as np
import pytest
import torch

from tests import gauss_twin as G
from tests import multibinary_twin as B

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _spec(n):
    from agilerl_amd.population.nets import MultiBinaryActorCriticSpec

    return MultiBinaryActorCriticSpec(obs_dim=8, n_actions=n)


def _pop(n, P=3, N=21, scale=20.0, **kw):
    """A population whose actor output layer is scaled up: logits of order one
    instead of the 0.1-scaled initialisation's few hundredths."""
    from agilerl_amd.population.ppo_pop import PPOPopulation

    spec = _spec(n)
    pop = PPOPopulation(spec, P, N, learn_step=2 * N, batch_size=N, device=DEV, seed_base=5, **kw)
    W, _, _, _ = spec.views(pop.params.data, spec.actor[-1])
    W.mul_(scale)
    return pop


def _cpu_forward(pop, obs):
    """spec.forward in float32 torch on the CPU -> (logits [P, N, n] float64 numpy, value [P, N] float32 tensor)."""
    logits, value = pop.spec.forward(pop.params.data.cpu(), obs.cpu())
    return logits.double().numpy(), value


def _step(pop, obs, *, sample, counter=0, mask=None, flat=False):
    from agilerl_amd.population.learner import policy_step_bern

    P, N, n = pop.P, pop.N, pop.spec.n_actions
    out = dict(actions=torch.full((P, N, n), -7, dtype=torch.int64, device=DEV),
               log_probs=torch.empty(P, N, device=DEV), values=torch.empty(P, N, device=DEV),
               entropy=torch.empty(P, N, device=DEV))
    af = torch.full((P * N * n,), -7, dtype=torch.int64, device=DEV) if flat else None
    policy_step_bern(pop, pop.bern_descriptor(), obs, N * 8, sample=sample, counter=counter, out_agent_stride=N,
                     actions_flat=af, action_mask=mask, mask_agent_stride=N * n, **out)
    torch.cuda.synchronize()
    out["flat"] = None if af is None else af.view(P, N, n)
    return {k: (v.cpu() if v is not None else None) for k, v in out.items()}


def _obs(P, N, seed=1):
    return torch.randn(P, N, 8, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _check_logp_entropy(out, logits64, mask=None):
    """Stored log-prob and entropy against the twin on the torch-forward logits.
    The forward's bar (rtol 1e-4 / atol 1e-5 per network output) propagates to
    the log-prob through |a_j - p_j| <= 1 per bit and to the entropy through
    |dH/dl_j| < 1 per bit, so both get test_multidisc_ppo_gpu's bar with the
    bit count as its logit count: rtol 1e-5, atol 1e-5 n."""
    n = logits64.shape[-1]
    lp, H = B.logp_entropy(logits64, out["actions"].numpy(), mask)
    np.testing.assert_allclose(out["log_probs"].numpy(), lp, rtol=1e-5, atol=1e-5 * n)
    np.testing.assert_allclose(out["entropy"].numpy(), H, rtol=1e-5, atol=1e-5 * n)


def _clear_obs(pop, P, N, mask=None):
    """The first observation seed for which every (legal) |logit| of the CPU forward is above 1e-3."""
    for seed in range(1, 400):
        obs = _obs(P, N, seed)
        logits, value = _cpu_forward(pop, obs)
        live = np.abs(logits) if mask is None else np.where(mask != 0, np.abs(logits), np.inf)
        if live.min() > 1e-3:
            return obs, logits, value, seed, float(live.min())
    raise AssertionError("no observation seed with every |logit| above 1e-3")


# ---- the policy step, greedy ---------------------------------------------------------- #
@pytest.mark.parametrize("few", ["few", "general"])
@pytest.mark.parametrize("n", B.NS)
def test_bern_policy_step_greedy_matches_torch_forward(n, few, monkeypatch):
    """sample = 0: bit j is 1 iff logit j > 0; actions equal the twin's on the
    torch-forward logits, every one of which is further than 1e-3 from 0;
    log-prob, entropy and value at the multi-categorical greedy test's bars.
    21 envs: two row blocks, the second partial.  Both forward forms
    (AGX_GRAPH_FEW=0: the general one)."""
    if few == "general":
        monkeypatch.setenv("AGX_GRAPH_FEW", "0")
    P, N = 3, 21
    pop = _pop(n, P, N)
    obs, logits, value, seed, gap = _clear_obs(pop, P, N)
    print(f"n {n}: obs seed {seed}, smallest |logit| {gap:.3e}")
    out = _step(pop, obs, sample=False, flat=True)
    want = B.mode(logits)
    assert np.array_equal(out["actions"].numpy(), want)
    assert torch.equal(out["flat"], out["actions"])
    torch.testing.assert_close(out["values"], value.view(P, N), rtol=1e-4, atol=1e-5)
    _check_logp_entropy(out, logits)
    if n > 1:
        assert 0 < want.mean() < 1  # both values occur


def test_bern_policy_step_greedy_with_mask():
    """The mode runs over the masked logits: a masked bit is 0, at the same bars."""
    n, P, N = 17, 3, 21
    pop = _pop(n, P, N)
    mask = B.random_mask(np.random.default_rng(3), P * N, n).reshape(P, N, n)
    obs, logits, _, _, _ = _clear_obs(pop, P, N, mask)
    out = _step(pop, obs, sample=False, mask=torch.from_numpy(mask).to(DEV))
    got = out["actions"].numpy()
    assert np.array_equal(got, B.mode(logits, mask))
    assert (mask == 0).any() and (got[mask == 0] == 0).all() and (B.mode(logits)[mask == 0] == 1).any()
    _check_logp_entropy(out, logits, mask)


# ---- the policy step, sampled --------------------------------------------------------- #
@pytest.mark.parametrize("P,N", [(3, 21), (2, 2048)])
@pytest.mark.parametrize("n", [2, 5, 16, 17, 32])
def test_bern_policy_step_samples_the_uniform_stream(n, P, N):
    """The bits against a_j = 1[u_j < p_j] of the twin over the torch-forward
    logits; a bit whose float64 |u_j - p_j| is under 1e-4 is left out, and those
    may be at most 1 % (a condition on the twin alone, checked before the
    kernel's output is looked at).  The stored log-prob against the twin's
    log-prob of the stored bits at the greedy test's bar; the staging copy
    equals the stored actions; under a mask no masked bit is 1."""
    pop = _pop(n, P, N)
    obs = _obs(P, N)
    logits, value = _cpu_forward(pop, obs)
    u = B.uniforms(P, N, n, pop.act_seed, B.COUNTER, env_base=pop.env_base_d.cpu().numpy())
    mask = B.random_mask(np.random.default_rng(n), P * N, n).reshape(P, N, n)
    want, gap = B.choices(logits, u)
    want_m, gap_m = B.choices(logits, u, mask)
    keep, keep_m = gap >= 1e-4, gap_m >= 1e-4
    share = 1.0 - float(min(keep.mean(), keep_m.mean()))
    print(f"n {n} P {P} N {N}: excluded share {share:.5f}")
    assert share <= 0.01
    out = _step(pop, obs, sample=True, counter=B.COUNTER, flat=True)
    got = out["actions"].numpy()
    assert set(np.unique(got).tolist()) <= {0, 1}
    assert np.array_equal(got[keep], want[keep]), int((got[keep] != want[keep]).sum())
    assert torch.equal(out["flat"], out["actions"])
    torch.testing.assert_close(out["values"], value.view(P, N), rtol=1e-4, atol=1e-5)
    _check_logp_entropy(out, logits)
    assert (got != B.mode(logits)).mean() > 0.05  # not the greedy step
    outm = _step(pop, obs, sample=True, counter=B.COUNTER, mask=torch.from_numpy(mask).to(DEV), flat=True)
    gotm = outm["actions"].numpy()
    assert np.array_equal(gotm[keep_m], want_m[keep_m])
    assert (gotm[mask == 0] == 0).all() and torch.equal(outm["flat"], outm["actions"])
    _check_logp_entropy(outm, logits, mask)


@pytest.mark.parametrize("n", [5, 32])
def test_bern_policy_step_sample_frequencies(n):
    """One observation repeated over N = 2048 rows of one agent: every bit's
    empirical frequency within 5 sqrt(p q / N) of sigmoid(logit) (the rows
    differ only in their stream env)."""
    P, N = 1, 2048
    pop = _pop(n, P, N, scale=10.0)
    obs = _obs(1, 1, 7).expand(1, N, 8).contiguous()
    logits, _ = _cpu_forward(pop, obs[:, :1])
    p = B.sigmoid(logits[0, 0])
    out = _step(pop, obs, sample=True, counter=B.COUNTER)
    freq = out["actions"].numpy()[0].mean(0)
    bound = 5 * np.sqrt(p * (1 - p) / N)
    print(f"n {n}: max |freq - p| / bound = {np.max(np.abs(freq - p) / bound):.3f}")
    assert np.all(np.abs(freq - p) <= bound)


def test_bern_policy_step_streams():
    """Equal bits for an equal (seed, counter); another counter draws other
    actions; agent 2 alone (its env base set) draws what it draws among three."""
    n, P, N = 17, 3, 21
    pop = _pop(n, P, N)
    obs = _obs(P, N)
    one = _step(pop, obs, sample=True, counter=B.COUNTER)
    two = _step(pop, obs, sample=True, counter=B.COUNTER)
    other = _step(pop, obs, sample=True, counter=B.COUNTER + 1)
    for k in ("actions", "log_probs", "values", "entropy"):
        assert torch.equal(one[k], two[k]), k
    assert not torch.equal(one["actions"], other["actions"])

    solo = _pop(n, 1, N, agent_offset=2, global_pop_size=3)
    assert solo.act_seed == pop.act_seed and solo.env_base_d.tolist() == [2 * N]
    solo.params.data[0].copy_(pop.params.data[2])
    alone = _step(solo, obs[2:3].contiguous(), sample=True, counter=B.COUNTER)
    for k in ("actions", "log_probs", "values", "entropy"):
        assert torch.equal(alone[k][0], one[k][2]), k


# ---- the loss kernel ------------------------------------------------------------------ #
def _loss_call(rec, b, clip, vf, ent, n=None):
    from agilerl_amd import kernels as K

    t = lambda k: None if rec[k] is None else torch.from_numpy(rec[k]).to(DEV)  # noqa: E731
    out = K.ppo_bern_loss_fwd_bwd(t("logits"), t("value"), t("actions"), t("old_logp"), t("adv"), t("ret"),
                                  t("old_v"), b, clip, vf, ent, index=t("index"), mask=t("mask"), n=n)
    torch.cuda.synchronize()
    return [x.cpu() for x in out]


def _float32_formula_error(rec, b, clip, vf, ent, ref):
    """Worst error of the header's formula evaluated in float32 torch on the CPU
    against the float64 restatement, for g_logits: what any float32 evaluation
    of these inputs loses (the kernel gets 4x this for a different but equally
    valid order of operations)."""
    S, n = rec["logits"].shape
    t = lambda k: torch.from_numpy(rec[k])  # noqa: E731
    src = torch.arange(S) if rec["index"] is None else t("index")
    lg = t("logits")
    mk = None if rec["mask"] is None else t("mask")[src].bool()
    if mk is not None:
        lg = torch.where(mk, lg, torch.full_like(lg, -1e8))
    a = (t("actions")[src] != 0).float()
    p = torch.sigmoid(lg)
    q = 1 - p
    logp = (a * -torch.nn.functional.softplus(-lg) + (1 - a) * -torch.nn.functional.softplus(lg)).sum(-1)
    tt = lambda x: torch.log(x + 1e-8) + x / (x + 1e-8)  # noqa: E731
    dH = -p * q * (tt(p) - tt(q))
    ratio = torch.exp(logp - t("old_logp")[src])
    adv = t("adv")[src]
    p1, p2 = -adv * ratio, -adv * ratio.clamp(1 - clip, 1 + clip)
    half = lambda x, y: torch.where(x > y, 1.0, torch.where(x == y, 0.5, 0.0))  # noqa: E731
    inr = ((ratio >= 1 - clip) & (ratio <= 1 + clip)).float()
    g_lp = (half(p1, p2) * -adv + half(p2, p1) * -adv * inr) / b * ratio
    g = g_lp[:, None] * (a - p) + np.float32(-ent / b) * dH
    if mk is not None:
        g = torch.where(mk, g, torch.zeros_like(g))
    return float(np.abs(g.double().numpy() - ref["g_logits"]).max())


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("gather", [False, True], ids=["direct", "gather"])
@pytest.mark.parametrize("b,nmb", [(1, 1), (5, 3), (6, 5)])
@pytest.mark.parametrize("n", B.NS)
def test_bern_loss_matches_float64_restatement(n, b, nmb, gather, masked):
    """agx_ppo_bern_loss_fwd_bwd against tests/multibinary_twin.py
    loss_and_grads (float64), rows on the tie rules included.  (b, nmb) =
    (6, 5): a batch that is no multiple of the four rows per pass, and one full
    block of four minibatches followed by a partial one.

    Bars: those of test_multi_loss_matches_float64_restatement: rtol 1e-5 /
    atol 1e-8 on the gradients, rtol 1e-5 / atol 1e-6 on the stats; for
    g_logits at least 4x the worst error of the same formula in float32 torch
    on the CPU.  Masked entries of g_logits are exactly 0; a second launch
    gives equal bits."""
    clip, vf, ent = 0.25, 0.5, 0.01
    S = b * nmb
    rec = B.loss_inputs(n, b, nmb, (S + 13) if gather else None, 3000 + 31 * n + b, clip, masked)
    ref = B.loss_and_grads(rec["logits"], rec["value"], rec["actions"], rec["mask"], rec["old_logp"], rec["adv"],
                           rec["ret"], rec["old_v"], rec["index"], b, clip, vf, ent)
    first = _loss_call(rec, b, clip, vf, ent)
    g_logits, g_value, stats = (x.double().numpy() for x in first)
    e32 = _float32_formula_error(rec, b, clip, vf, ent, ref)
    err = {k: float(np.abs(got - ref[k]).max()) for k, got in (("g_logits", g_logits), ("g_value", g_value),
                                                               ("stats", stats))}
    print(f"n={n} b={b} nmb={nmb} gather={gather} masked={masked}: kernel max |err| {err}; float32 torch "
          f"formula: g_logits {e32:.3e}")
    np.testing.assert_allclose(g_value, ref["g_value"], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(stats[:, :6], ref["stats"][:, :6], rtol=1e-5, atol=1e-6)
    assert np.all(stats[:, 6:] == 0)
    tol = np.maximum(1e-5 * np.abs(ref["g_logits"]) + 1e-8, 4 * e32)
    assert np.all(np.abs(g_logits - ref["g_logits"]) <= tol), float(np.max(np.abs(g_logits - ref["g_logits"]) / tol))
    if masked:
        src = np.arange(S) if rec["index"] is None else rec["index"]
        off = rec["mask"][src] == 0
        assert np.all(g_logits[off] == 0)
        assert off.any() or S * n < 16
    again = _loss_call(rec, b, clip, vf, ent)
    for x, y in zip(first, again):
        assert torch.equal(x, y)


def test_bern_loss_counts_any_nonzero_action_as_one():
    """A stored 7 or -3 gives the result of a stored 1: defined behaviour, no error."""
    n, b, nmb, clip = 17, 5, 3, 0.25
    rec = B.loss_inputs(n, b, nmb, None, 77, clip, False)
    odd = dict(rec, actions=rec["actions"].copy())
    ones = np.argwhere(rec["actions"] == 1)
    assert len(ones) > 8
    for i, (r, c) in enumerate(ones[:8]):
        odd["actions"][r, c] = (7, -3, 1 << 40, -(1 << 35))[i % 4]
    assert (odd["actions"] != rec["actions"]).sum() == 8
    for x, y in zip(_loss_call(odd, b, clip, 0.5, 0.01), _loss_call(rec, b, clip, 0.5, 0.01)):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())


def test_bern_loss_extreme_and_masked_logits_stay_finite():
    """|l| = 1e8 (what a mask writes) on a legal bit: finite outputs; a masked
    bit with stored action 0 leaves the row's log-prob what it is without it."""
    n, b, clip = 2, 4, 0.25
    rec = B.loss_inputs(n, b, 1, None, 5, clip, False)
    rec["logits"][:, 1] = [1e8, -1e8, 30.0, -30.0]
    rec["actions"][:, 1] = [1, 0, 0, 1]
    out = _loss_call(rec, b, clip, 0.5, 0.01)
    assert all(bool(torch.isfinite(x).all()) for x in out)
    one = B.loss_inputs(1, b, 1, None, 5, clip, False)
    two = dict(one, logits=np.concatenate([one["logits"], np.full((b, 1), 0.7, np.float32)], 1),
               actions=np.concatenate([one["actions"], np.zeros((b, 1), np.int64)], 1),
               mask=np.tile(np.array([[1, 0]], np.uint8), (b, 1)))
    a, c = _loss_call(one, b, clip, 0.5, 0.0), _loss_call(two, b, clip, 0.5, 0.0)
    assert torch.equal(a[0][:, 0], c[0][:, 0]) and torch.equal(a[1], c[1]) and (c[0][:, 1] == 0).all()
    assert torch.equal(a[2][:, [1, 2, 4, 5]], c[2][:, [1, 2, 4, 5]])  # ent_coef 0: the entropy's 1e-8 aside


def test_bern_kernels_reject_a_bad_width():
    from agilerl_amd import _lib

    rec = B.loss_inputs(5, 5, 1, None, 5, 0.25, False)
    for n in (0, 33):
        with pytest.raises(_lib.AgxError, match="bits"):
            _loss_call(rec, 5, 0.25, 0.5, 0.01, n=n)


# ---- one learner update --------------------------------------------------------------- #
def _filled_population(ent_coef, masks, seed=3, fused=False, n=9):
    """P = 2, N = 8, T = 4 with a rollout from the policy-step kernel itself."""
    from agilerl_amd.population.ppo_pop import PPOPopulation

    P, N, T = 2, 8, 4
    pop = PPOPopulation(_spec(n), P, N, learn_step=T * N, batch_size=16, update_epochs=1, lr=1e-3,
                        ent_coef=ent_coef, device=DEV, seed_base=seed, action_masks=masks, fused=fused)
    W, _, _, _ = pop.spec.views(pop.params.data, pop.spec.actor[-1])
    W.mul_(10.0)
    g = torch.Generator().manual_seed(seed)
    pop.obs.copy_(torch.randn(P, T, N, 8, generator=g))
    if masks:
        m = B.random_mask(np.random.default_rng(seed), P * T * N, n).reshape(P, T, N, n)
        pop.action_masks.copy_(torch.from_numpy(m))
    for t in range(T):
        pop.act_into(t)
    pop.rewards.copy_(torch.randn(P, T, N, generator=g))
    pop.dones.copy_((torch.rand(P, T, N, generator=g) < 0.1).to(torch.uint8))
    pop.finish_rollout(torch.randn(P, N, 8, generator=g).to(DEV), torch.zeros(P, N, dtype=torch.uint8, device=DEV))
    return pop


@pytest.mark.parametrize("masks", [False, True], ids=["nomask", "mask"])
def test_bern_learner_update_matches_torch_twin(masks):
    """One epoch of two 16-row minibatches per agent from the same state,
    against an independent pure-torch twin: spec.forward, the Bernoulli head in
    torch ops, the ppo.py loss with torch ops, clip_grad_norm_ over the two
    groups and torch.optim.Adam; the first Adam moment and the parameters by
    the `close` criterion of test_multi_learner_update_matches_torch_twin.
    With masks the sampled bits are legal and the twin applies torch.where to
    the logits."""
    from agilerl_amd.population.nets import bernoulli_head

    np.random.seed(11)
    pop = _filled_population(0.01, masks)
    spec, P, S, n = pop.spec, pop.P, pop.S, pop.spec.n_actions
    assert pop.actions.shape == (P, 4, 8, n) and pop.actions.dtype == torch.int64
    assert set(np.unique(pop.actions.cpu().numpy()).tolist()) == {0, 1}
    assert not pop._fused_learner()
    if masks:
        assert pop.action_masks.shape == (P, 4, 8, n) and (pop.action_masks == 0).any()
        assert (pop.actions[pop.action_masks == 0] == 0).all()
    p0 = pop.params.data.clone()
    perms = pop.permutations().clone()
    pop._learn_torch(perms)
    torch.cuda.synchronize()
    adv = pop.advantages.view(P, S)  # normalised in place by the learn
    assert not torch.equal(pop.params.data, p0)

    def close(name, got, want, rtol):
        got, want = got.double().cpu().numpy().ravel(), want.double().cpu().numpy().ravel()
        bad = np.abs(got - want) > rtol * (np.abs(want) + np.sqrt(np.mean(want * want)))
        assert bad.mean() <= 1e-4, (name, int(bad.sum()), want.size)

    for p in range(P):
        w = p0[p:p + 1].clone().requires_grad_(True)
        opt = torch.optim.Adam([w], lr=1e-3, eps=1e-8)
        for s0 in range(0, S, 16):
            idx = perms[0][p, s0:s0 + 16]
            logits, value = spec.forward(w, pop.obs.view(P, S, -1)[p, idx].unsqueeze(0))
            mk = pop.action_masks.view(P, S, n)[p, idx] if masks else None
            logp, ent = bernoulli_head(logits[0], pop.actions.view(P, S, n)[p, idx], mk)
            loss, _ = G.torch_loss(logp, ent, value[0], pop.log_probs.view(P, S)[p, idx], adv[p, idx],
                                   pop.returns.view(P, S)[p, idx], pop.values.view(P, S)[p, idx], pop.clip_coef,
                                   pop.vf_coef, 0.01)
            opt.zero_grad()
            loss.backward()
            g = w.grad[0]
            for a, b in ((0, spec.actor_end), (spec.actor_end, spec.n_params)):  # clip_grad_norm_ per group
                g[a:b].mul_(torch.clamp(pop.max_grad_norm / (g[a:b].norm() + 1e-6), max=1.0))
            opt.step()
        st = opt.state[w]
        close(f"{p} exp_avg", pop.opt.exp_avg[p], st["exp_avg"][0], 1e-4)
        close(f"{p} params", pop.params.data[p], w.detach()[0], 1e-4)


# ---- drop-in -------------------------------------------------------------------------- #
def test_bern_dropin_create_population_train_on_policy(monkeypatch):
    """create_population("PPO", MultiBinary actions) + train_on_policy on the
    binary-switch synthetic env for a few generations with tournament and
    mutations on, architecture mutations included; the rollouts and evaluations
    never reach torch's layer_norm (the policy step is the HIP kernel); [8, n]
    arrays of the space's dtype holding only 0 / 1 reach every agent's env; the
    losses are finite."""
    import torch.nn.functional as F

    from agilerl_amd.envs import Box, MultiBinary, SyntheticVecEnv
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
            seen.append((a.dtype, a.shape, bool(np.isin(a, (0, 1)).all())))
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

    n = 5
    obs_space, act_space = Box(-np.inf, np.inf, (8,)), MultiBinary(n)
    INIT_HP = {"BATCH_SIZE": 32, "LR": 1e-3, "LEARN_STEP": 64, "UPDATE_EPOCHS": 2}
    pop = create_population("PPO", None, INIT_HP, obs_space, act_space, population_size=2, num_envs=8)
    population = pop[0].population
    assert population.multibinary and not population.multidiscrete and population.actions.shape == (2, 8, 8, n)
    assert population.fused_descriptor() is None and population.learn_descriptor() is None
    assert population.eval_descriptor() is None
    env = Env(8, seed=3, p_done=0.05, max_episode_steps=40, n_binary=n)  # the shared N-env, cloned per agent
    np.random.seed(0)
    torch.manual_seed(0)
    mut = Mutations(no_mutation=0.2, architecture=0.4, new_layer_prob=0.5, parameters=0.2, activation=0, rl_hp=0.2,
                    rand_seed=1)
    pop, fits = train_on_policy(env, "Synthetic", "PPO", pop, INIT_HP=INIT_HP, max_steps=384, evo_steps=128,
                                eval_loop=1, tournament=TournamentSelection(2, True, 2, 1), mutation=mut,
                                verbose=False)
    assert len(fits) == 3 and all(len(f) == 2 and np.all(np.isfinite(f)) for f in fits)
    assert seen and all(s == (np.dtype(np.int8), (8, n), True) for s in seen), set(seen)
    assert len(losses) >= 3 and all(bool(torch.isfinite(x).all()) for x in losses)
    for a in pop:
        assert a.spec.head == "multibinary" and a.spec.actor[-1].fout == n
        assert a.population.multibinary and a.population.learn_descriptor() is None


def test_bern_architecture_mutation_keeps_acting():
    from agilerl_amd.algorithms.ppo import PPO
    from agilerl_amd.envs import Box, MultiBinary

    agent = PPO(Box(-np.inf, np.inf, (8,)), MultiBinary(6), num_envs=4, learn_step=16, batch_size=8)
    assert agent.architecture_mutation(0.5, np.random.default_rng(0)) is not None
    assert agent.spec.head == "multibinary" and agent.spec.n_actions == 6 and agent.population.multibinary
    a, lp, ent, v = agent.get_action(np.zeros((4, 8), np.float32))
    assert a.shape == (4, 6) and a.dtype == np.int8 and np.isfinite(lp).all()


def test_bern_standalone_agent_and_checkpoint(tmp_path):
    """A standalone MultiBinary PPO: get_action (with an action_mask), the
    deprecated learn(experiences), rollout_buffer.add + learn(), test(); a
    checkpoint save / load reproduces the next greedy actions."""
    from agilerl_amd.algorithms.ppo import PPO
    from agilerl_amd.envs import Box, MultiBinary, SyntheticVecEnv

    T, N, n = 4, 4, 9
    agent = PPO(Box(-np.inf, np.inf, (8,)), MultiBinary(n), num_envs=N, learn_step=T * N, batch_size=8,
                update_epochs=2, lr=1e-3)
    assert agent.population.multibinary
    rng = np.random.default_rng(0)
    np.random.seed(0)
    obs = rng.standard_normal((T, N, 8)).astype(np.float32)
    steps = [agent.get_action(obs[t]) for t in range(T)]
    actions, logp, values = (np.stack([s[i] for s in steps]) for i in (0, 1, 3))
    assert actions.shape == (T, N, n) and actions.dtype == np.int8 and logp.shape == (T, N)
    assert np.isin(actions, (0, 1)).all()
    logits, _ = _cpu_forward(agent.population, torch.from_numpy(obs[0]).view(1, N, 8))
    want, _ = B.logp_entropy(logits[0], actions[0])
    np.testing.assert_allclose(logp[0], want, rtol=1e-5, atol=1e-5 * n)
    mask = np.zeros((N, n), np.uint8)
    mask[:, [1, 3, 8]] = 1
    am = agent.get_action(obs[0], action_mask=mask)[0]
    assert (am[:, [0, 2, 4, 5, 6, 7]] == 0).all()

    rewards = rng.standard_normal((T, N)).astype(np.float32)
    dones = (rng.random((T, N)) < 0.1).astype(np.float32)
    p0 = agent.population.params.data.clone()
    loss = agent.learn((obs, actions, logp, rewards, dones, values, obs[-1], dones[-1]))
    p1 = agent.population.params.data.clone()
    assert np.isfinite(loss) and not torch.equal(p0, p1)
    buf = agent.rollout_buffer
    buf.reset()
    for t in range(T):
        buf.add(obs[t], actions[t], rewards[t], dones[t], values[t], logp[t])
    assert torch.equal(agent.population.actions[0].cpu(), torch.from_numpy(actions.astype(np.int64)))
    buf.compute_returns_and_advantages(values[-1], dones[-1])
    loss = agent.learn()
    assert np.isfinite(loss) and not torch.equal(agent.population.params.data, p1)

    seen = []

    class Env(SyntheticVecEnv):
        def step(self, actions, **kw):
            seen.append(np.asarray(actions))
            return super().step(actions, **kw)

    fit = agent.test(Env(N, seed=1, p_done=0.2, max_episode_steps=10, n_binary=n), loop=1)
    assert np.isfinite(fit) and agent.fitness == [fit]
    assert seen and all(a.shape == (N, n) and a.dtype == np.int8 and np.isin(a, (0, 1)).all() for a in seen)

    ck = os.path.join(tmp_path, "bern.pt")
    agent.save_checkpoint(ck)
    back = PPO.load(ck, device=DEV)
    assert back.population.multibinary and back.spec.n_actions == n and back.action_space.n == n
    assert type(back.action_space).__name__ == "MultiBinary"
    assert torch.equal(back.population.params.data[0], agent.population.params.data[agent.row])
    o = torch.from_numpy(obs[1]).to(DEV).view(1, N, 8)
    ga, gb = agent.population.evaluate(o), back.population.evaluate(o)
    assert ga.shape == (1, N, n) and torch.equal(ga, gb)


# ---- regression guard ----------------------------------------------------------------- #
def test_discrete_population_after_multibinary_population_keeps_the_fused_kernels():
    from agilerl_amd.envs import Box, Discrete, MultiBinary
    from agilerl_amd.utils import create_population

    obs_space = Box(-np.inf, np.inf, (8,))
    mb = create_population("PPO", None, {"LEARN_STEP": 64}, obs_space, MultiBinary(4), population_size=2, num_envs=8)
    mp = mb[0].population
    assert mp.multibinary and mp.actions.shape == (2, 8, 8, 4) and mp.actions.dtype == torch.int64
    assert mp.fused_descriptor() is None and mp.learn_descriptor() is None and mp.eval_descriptor() is None
    net = {"encoder_config": {"hidden_size": [64]}, "head_config": {"hidden_size": [64]}, "latent_dim": 64}
    disc = create_population("PPO", net, {"LEARN_STEP": 64}, obs_space, Discrete(4), population_size=2, num_envs=8)
    population = disc[0].population
    assert not population.gaussian and not population.vector_int and population.fused_descriptor() is not None
    assert population.actions.dtype == torch.int64 and population.actions.shape == (2, 8, 8)
    default = create_population("PPO", None, {"LEARN_STEP": 64}, obs_space, Discrete(4), population_size=2, num_envs=8)
    assert default[0].population.learn_descriptor() is not None and not default[0].population.multibinary
