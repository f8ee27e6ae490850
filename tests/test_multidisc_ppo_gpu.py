"""PPO for MultiDiscrete action spaces on the GPU: agx_ppo_act_multi_graph
(greedy and sampled, against the torch forward and the float64 restatement of
tests/multidisc_twin.py, pinned to the reference by
tests/test_multidisc_ppo_cpu.py; K = 1 bit for bit against agx_ppo_act_graph),
agx_ppo_multi_loss_fwd_bwd against the restatement, one learner update against
a pure-torch twin, and the drop-in create_population / train_on_policy run on a
MultiDiscrete env."""

import os

import numpy as np
import pytest
import torch

from tests import gauss_twin as G
from tests import multidisc_twin as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = ["x".join(map(str, n)) if len(n) < 6 else f"{n[0]}x{len(n)}times" for n in M.NVECS]


def _spec(nvec):
    from agilerl_amd.population.nets import MultiDiscreteActorCriticSpec

    return MultiDiscreteActorCriticSpec(obs_dim=8, n_actions=int(sum(nvec)), nvec=tuple(nvec))


def _pop(nvec, P=3, N=21, scale=20.0, **kw):
    """A population whose actor output layer is scaled up: logits of order one
    instead of the 0.1-scaled initialisation's few hundredths."""
    from agilerl_amd.population.ppo_pop import PPOPopulation

    spec = _spec(nvec)
    pop = PPOPopulation(spec, P, N, learn_step=2 * N, batch_size=N, device=DEV, seed_base=5, **kw)
    W, _, _, _ = spec.views(pop.params.data, spec.actor[-1])
    W.mul_(scale)
    return pop


def _cpu_forward(pop, obs):
    """spec.forward in float32 torch on the CPU -> (logits [P, N, L] float64 numpy, value [P, N] float32 tensor)."""
    logits, value = pop.spec.forward(pop.params.data.cpu(), obs.cpu())
    return logits.double().numpy(), value


def _step(pop, obs, *, sample, counter=0, mask=None, flat=False):
    from agilerl_amd.population.learner import policy_step_multi

    P, N, K, L = pop.P, pop.N, len(pop.spec.nvec), pop.spec.n_actions
    out = dict(actions=torch.full((P, N, K), -7, dtype=torch.int64, device=DEV),
               log_probs=torch.empty(P, N, device=DEV), values=torch.empty(P, N, device=DEV),
               entropy=torch.empty(P, N, device=DEV))
    af = torch.full((P * N * K,), -7, dtype=torch.int64, device=DEV) if flat else None
    policy_step_multi(pop, pop.multi_descriptor(), obs, N * 8, sample=sample, counter=counter, out_agent_stride=N,
                      actions_flat=af, action_mask=mask, mask_agent_stride=N * L, **out)
    torch.cuda.synchronize()
    out["flat"] = None if af is None else af.view(P, N, K)
    return {k: (v.cpu() if v is not None else None) for k, v in out.items()}


def _obs(P, N, seed=1):
    return torch.randn(P, N, 8, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _check_logp_entropy(out, logits64, nvec, mask=None):
    """Stored log-prob and entropy against the twin on the torch-forward logits.
    The forward's bar (test_gauss_policy_step_greedy_matches_torch_forward:
    rtol 1e-4 / atol 1e-5 per network output) propagates to the log-prob through
    sum_j |1[j chosen] - p_j| <= 2 per component and to the entropy through
    sum_j p_j |t_j - sum p t| (of the same order), so both get that test's
    log-prob bar with the logit count in place of A: rtol 1e-5, atol 1e-5 L."""
    L = int(sum(nvec))
    lp, H = M.logp_entropy(logits64, nvec, out["actions"].numpy(), mask)
    np.testing.assert_allclose(out["log_probs"].numpy(), lp, rtol=1e-5, atol=1e-5 * L)
    np.testing.assert_allclose(out["entropy"].numpy(), H, rtol=1e-5, atol=1e-5 * L)


# ---- 4. the policy step, greedy ------------------------------------------------------- #
@pytest.mark.parametrize("few", ["few", "general"])
@pytest.mark.parametrize("nvec", M.NVECS, ids=IDS)
def test_multi_policy_step_greedy_matches_torch_forward(nvec, few, monkeypatch):
    """sample = 0: every component's first arg-max; actions equal the twin's on
    the torch-forward logits, whose top-two gap per (row, component) is above
    1e-3 (the observation seed is the first for which the CPU forward says so);
    log-prob, entropy and value at the Gaussian greedy test's bars.  21 envs:
    two row blocks, the second partial.  Both forward forms (AGX_GRAPH_FEW=0:
    the general one)."""
    if few == "general":
        monkeypatch.setenv("AGX_GRAPH_FEW", "0")
    P, N = 3, 21
    pop = _pop(nvec, P, N)
    for seed in range(1, 400):
        obs = _obs(P, N, seed)
        logits, value = _cpu_forward(pop, obs)
        want, gap = M.choices(logits, nvec)
        if gap.min() > 1e-3:
            break
    else:
        raise AssertionError("no observation seed with every top-two logit gap above 1e-3")
    print(f"nvec {nvec}: obs seed {seed}, smallest top-two gap {gap.min():.3e}")
    out = _step(pop, obs, sample=False, flat=True)
    assert np.array_equal(out["actions"].numpy(), want)
    assert torch.equal(out["flat"], out["actions"])
    torch.testing.assert_close(out["values"], value.view(P, N), rtol=1e-4, atol=1e-5)
    _check_logp_entropy(out, logits, nvec)
    for k, n in enumerate(nvec):
        assert int(out["actions"][..., k].min()) >= 0 and int(out["actions"][..., k].max()) < n


def test_multi_policy_step_greedy_with_mask():
    """The arg-max runs over the masked logits: the twin's choice under a mask
    (never an illegal index), at the same bars."""
    nvec, P, N = (7, 20, 5), 3, 21
    pop = _pop(nvec, P, N)
    rng = np.random.default_rng(3)
    mask = M.random_mask(rng, P * N, nvec).reshape(P, N, -1)
    for seed in range(1, 400):
        obs = _obs(P, N, seed)
        logits, _ = _cpu_forward(pop, obs)
        want, gap = M.choices(M.masked(logits, mask), nvec)
        if gap.min() > 1e-3:
            break
    out = _step(pop, obs, sample=False, mask=torch.from_numpy(mask).to(DEV))
    assert np.array_equal(out["actions"].numpy(), want)
    flat = out["actions"].numpy() + np.asarray(M.offsets(nvec))
    assert np.take_along_axis(mask, flat, -1).all()
    _check_logp_entropy(out, logits, nvec, mask)


# ---- 5. K = 1 equals Discrete, bit for bit ----------------------------------------------- #
@pytest.mark.parametrize("few", ["few", "general"])
@pytest.mark.parametrize("n", [2, 4, 17, 32])
def test_single_component_equals_the_categorical_step_bit_for_bit(n, few, monkeypatch):
    """nvec = [n]: agx_ppo_act_multi_graph against agx_ppo_act_graph on the same
    parameters, observations, seed, counter, agent_env_base and mask: actions,
    log-probs, entropy and values torch.equal, sampled and greedy, with a mask
    and without."""
    from agilerl_amd.population.learner import graph_descriptor, policy_step_graph
    from agilerl_amd.population.nets import ActorCriticSpec
    from agilerl_amd.population.ppo_pop import PPOPopulation

    if few == "general":
        monkeypatch.setenv("AGX_GRAPH_FEW", "0")
    P, N = 3, 21
    multi = _pop((n,), P, N)
    cat_spec = ActorCriticSpec(obs_dim=8, n_actions=n)
    cat = PPOPopulation(cat_spec, P, N, learn_step=2 * N, batch_size=N, device=DEV, seed_base=5)
    cat.params.data.copy_(multi.params.data)
    assert cat.act_seed == multi.act_seed and torch.equal(cat.env_base_d, multi.env_base_d)
    desc = graph_descriptor(cat_spec)
    assert desc is not None and multi.learn_descriptor() is None and multi.fused_descriptor() is None
    obs = _obs(P, N)
    rng = np.random.default_rng(n)
    mask = torch.from_numpy(M.random_mask(rng, P * N, (n,)).reshape(P, N, n)).to(DEV)
    differ = 0
    for sample in (True, False):
        for mk in (None, mask):
            ref = dict(actions=torch.empty(P, N, dtype=torch.int64, device=DEV),
                       log_probs=torch.empty(P, N, device=DEV), values=torch.empty(P, N, device=DEV),
                       entropy=torch.empty(P, N, device=DEV))
            policy_step_graph(cat, desc, obs, N * 8, sample=sample, counter=M.COUNTER, out_agent_stride=N,
                              action_mask=mk, mask_agent_stride=N * n, **ref)
            torch.cuda.synchronize()
            got = _step(multi, obs, sample=sample, counter=M.COUNTER, mask=mk)
            assert got["actions"].shape == (P, N, 1)
            assert torch.equal(got["actions"][..., 0], ref["actions"].cpu()), (sample, mk is not None)
            for k in ("log_probs", "entropy", "values"):
                assert torch.equal(got[k], ref[k].cpu()), (k, sample, mk is not None)
            if sample and mk is None:
                greedy = _step(multi, obs, sample=False)["actions"]
                differ = int((greedy != got["actions"]).sum())
    assert differ > 0  # the sampled step does sample


# ---- 6. the policy step, sampled, K > 1 --------------------------------------------------- #
@pytest.mark.parametrize("P,N", [(3, 21), (2, 2048)])
@pytest.mark.parametrize("nvec", [(3, 2), (5, 1, 4), (16, 16), (7, 20, 5), (2,) * 16], ids=IDS[1:6])
def test_multi_policy_step_samples_the_gumbel_stream(nvec, P, N):
    """(a) The choices against the float64 Gumbel scores of the twin over the
    torch-forward logits; a (row, component) whose float64 top-two score gap is
    under 1e-4 is left out, and those may be at most 1 % (a condition on the
    twin alone, checked before the kernel's output is looked at).  The stored
    log-prob against the twin's log-prob of the stored action at the greedy
    test's bar; the staging copy equals the stored actions."""
    pop = _pop(nvec, P, N)
    obs = _obs(P, N)
    logits, value = _cpu_forward(pop, obs)
    scores = M.gumbel_scores(logits, pop.act_seed, M.COUNTER, env_base=pop.env_base_d.cpu().numpy())
    want, gap = M.choices(scores, nvec)
    keep = gap >= 1e-4
    share = 1.0 - float(keep.mean())
    print(f"nvec {nvec} P {P} N {N}: excluded share {share:.5f}")
    assert share <= 0.01
    out = _step(pop, obs, sample=True, counter=M.COUNTER, flat=True)
    got = out["actions"].numpy()
    assert np.array_equal(got[keep], want[keep]), int((got[keep] != want[keep]).sum())
    assert torch.equal(out["flat"], out["actions"])
    torch.testing.assert_close(out["values"], value.view(P, N), rtol=1e-4, atol=1e-5)
    _check_logp_entropy(out, logits, nvec)
    assert (got != M.choices(logits, nvec)[0]).mean() > 0.05  # not the greedy step


@pytest.mark.parametrize("nvec", [(3, 2), (7, 20, 5)], ids=["3x2", "7x20x5"])
def test_multi_policy_step_sample_frequencies(nvec):
    """(b) One observation repeated over N = 2048 rows of one agent: every
    component's empirical frequencies within 5 sqrt(p (1 - p) / N) of the
    softmax probabilities (the rows differ only in their stream env)."""
    P, N = 1, 2048
    pop = _pop(nvec, P, N, scale=10.0)
    obs = _obs(1, 1, 7).expand(1, N, 8).contiguous()
    logits, _ = _cpu_forward(pop, obs[:, :1])
    p, _ = M.softmax_parts(logits[0, 0], nvec)
    out = _step(pop, obs, sample=True, counter=M.COUNTER)
    a = out["actions"].numpy()[0]
    for k, (off, n) in enumerate(zip(M.offsets(nvec), nvec)):
        freq = np.bincount(a[:, k], minlength=n) / N
        bound = 5 * np.sqrt(p[off:off + n] * (1 - p[off:off + n]) / N)
        print(f"component {k}: max |freq - p| / bound = {np.max(np.abs(freq - p[off:off + n]) / bound):.3f}")
        assert np.all(np.abs(freq - p[off:off + n]) <= bound)


def test_multi_policy_step_streams():
    """Equal bits for an equal (seed, counter); another counter draws other
    actions; agent 2 alone (its env base set) draws what it draws among three."""
    nvec, P, N = (5, 1, 4), 3, 21
    pop = _pop(nvec, P, N)
    obs = _obs(P, N)
    one = _step(pop, obs, sample=True, counter=M.COUNTER)
    two = _step(pop, obs, sample=True, counter=M.COUNTER)
    other = _step(pop, obs, sample=True, counter=M.COUNTER + 1)
    for k in ("actions", "log_probs", "values", "entropy"):
        assert torch.equal(one[k], two[k]), k
    assert not torch.equal(one["actions"], other["actions"])
    assert (one["actions"][..., 1] == 0).all()  # the one-way component

    solo = _pop(nvec, 1, N, agent_offset=2, global_pop_size=3)
    assert solo.act_seed == pop.act_seed and solo.env_base_d.tolist() == [2 * N]
    solo.params.data[0].copy_(pop.params.data[2])
    alone = _step(solo, obs[2:3].contiguous(), sample=True, counter=M.COUNTER)
    for k in ("actions", "log_probs", "values", "entropy"):
        assert torch.equal(alone[k][0], one[k][2]), k


# ---- 7. the loss kernel ------------------------------------------------------------------- #
def _loss_call(rec, nvec, b, clip, vf, ent):
    from agilerl_amd import kernels as K

    t = lambda k: None if rec[k] is None else torch.from_numpy(rec[k]).to(DEV)  # noqa: E731
    out = K.ppo_multi_loss_fwd_bwd(t("logits"), t("value"), nvec, t("actions"), t("old_logp"), t("adv"), t("ret"),
                                   t("old_v"), b, clip, vf, ent, index=t("index"), mask=t("mask"))
    torch.cuda.synchronize()
    return [x.cpu() for x in out]


def _float32_formula_error(rec, nvec, b, clip, vf, ent, ref):
    """Worst error of the SAME formula evaluated in float32 torch on the CPU
    against the float64 restatement, for g_logits: what any float32 evaluation
    of these inputs loses (the kernel gets 4x this for a different but equally
    valid summation order)."""
    S, L = rec["logits"].shape
    t = lambda k: torch.from_numpy(rec[k])  # noqa: E731
    src = torch.arange(S) if rec["index"] is None else t("index")
    lg = t("logits")
    mk = None if rec["mask"] is None else t("mask")[src].bool()
    if mk is not None:
        lg = torch.where(mk, lg, torch.full_like(lg, -1e8))
    a = t("actions")[src]
    p, onehot, dH = torch.zeros_like(lg), torch.zeros_like(lg), torch.zeros_like(lg)
    logp = torch.zeros(S)
    for k, (off, n) in enumerate(zip(M.offsets(nvec), nvec)):
        s = lg[:, off:off + n]
        lsm = torch.log_softmax(s, -1)
        pk = torch.softmax(s, -1)
        p[:, off:off + n] = pk
        logp = logp + lsm.gather(-1, a[:, k:k + 1])[:, 0]
        onehot[:, off:off + n].scatter_(-1, a[:, k:k + 1], 1.0)
        tk = torch.log(pk + 1e-8) + pk / (pk + 1e-8)
        dH[:, off:off + n] = -pk * (tk - (pk * tk).sum(-1, keepdim=True))
    ratio = torch.exp(logp - t("old_logp")[src])
    adv = t("adv")[src]
    p1, p2 = -adv * ratio, -adv * ratio.clamp(1 - clip, 1 + clip)
    half = lambda x, y: torch.where(x > y, 1.0, torch.where(x == y, 0.5, 0.0))  # noqa: E731
    inr = ((ratio >= 1 - clip) & (ratio <= 1 + clip)).float()
    g_lp = (half(p1, p2) * -adv + half(p2, p1) * -adv * inr) / b * ratio
    g = g_lp[:, None] * (onehot - p) + np.float32(-ent / b) * dH
    if mk is not None:
        g = torch.where(mk, g, torch.zeros_like(g))
    return float(np.abs(g.double().numpy() - ref["g_logits"]).max())


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("gather", [False, True], ids=["direct", "gather"])
@pytest.mark.parametrize("b,nmb", [(1, 1), (5, 3), (6, 5)])
@pytest.mark.parametrize("nvec", M.NVECS, ids=IDS)
def test_multi_loss_matches_float64_restatement(nvec, b, nmb, gather, masked):
    """agx_ppo_multi_loss_fwd_bwd against tests/multidisc_twin.py loss_and_grads
    (float64), rows on the tie rules included (gauss_twin.loss_inputs' value /
    adv rows: adv = 0, value == old_value, value - old_value exactly +-clip).
    (b, nmb) = (6, 5): a batch that is no multiple of the four rows per pass,
    and one full block of four minibatches followed by a partial one.

    Bars: those of test_gauss_loss_matches_float64_restatement: rtol 1e-5 /
    atol 1e-8 on the gradients, rtol 1e-5 / atol 1e-6 on the stats; for
    g_logits at least 4x the worst error of the same formula in float32 torch
    on the CPU.  Masked entries of g_logits are exactly 0; a second launch
    gives equal bits."""
    clip, vf, ent = 0.25, 0.5, 0.01
    S = b * nmb
    rec = M.loss_inputs(nvec, b, nmb, (S + 13) if gather else None, 2000 + 31 * sum(nvec) + b, clip, masked)
    ref = M.loss_and_grads(rec["logits"], rec["value"], nvec, rec["actions"], rec["mask"], rec["old_logp"],
                           rec["adv"], rec["ret"], rec["old_v"], rec["index"], b, clip, vf, ent)
    first = _loss_call(rec, nvec, b, clip, vf, ent)
    g_logits, g_value, stats = (x.double().numpy() for x in first)
    e32 = _float32_formula_error(rec, nvec, b, clip, vf, ent, ref)
    err = {k: float(np.abs(got - ref[k]).max()) for k, got in (("g_logits", g_logits), ("g_value", g_value),
                                                               ("stats", stats))}
    print(f"nvec={nvec} b={b} nmb={nmb} gather={gather} masked={masked}: kernel max |err| {err}; float32 torch "
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
        assert off.any() or S * sum(nvec) < 16  # (a single two-logit row may have nothing masked)
    again = _loss_call(rec, nvec, b, clip, vf, ent)
    for x, y in zip(first, again):
        assert torch.equal(x, y)


def test_multi_loss_clamps_an_action_outside_its_component():
    """An action outside [0, n_k) never indexes outside the row: it is clamped
    into the component (the result is that of the clamped action)."""
    nvec, b, nmb, clip = (5, 1, 4), 5, 3, 0.25
    rec = M.loss_inputs(nvec, b, nmb, None, 77, clip, False)
    bad = dict(rec, actions=rec["actions"].copy())
    bad["actions"][0, 0], bad["actions"][1, 2], bad["actions"][2, 1] = 99, -3, 1 << 40
    good = dict(rec, actions=np.clip(bad["actions"], 0, np.asarray(nvec) - 1))
    for x, y in zip(_loss_call(bad, nvec, b, clip, 0.5, 0.01), _loss_call(good, nvec, b, clip, 0.5, 0.01)):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())


def test_multi_kernels_reject_a_bad_head():
    from agilerl_amd import _lib
    from agilerl_amd import kernels as K

    rec = M.loss_inputs((3, 2), 5, 1, None, 5, 0.25, False)
    t = lambda k: torch.from_numpy(rec[k]).to(DEV)  # noqa: E731
    head = K.multi_head((3, 2))
    head.nvec[1] = 0
    with pytest.raises((_lib.AgxError, ValueError)):
        K.ppo_multi_loss_fwd_bwd(t("logits"), t("value"), head, t("actions"), t("old_logp"), t("adv"), t("ret"),
                                 t("old_v"), 5)
    with pytest.raises(ValueError):
        K.multi_head((20, 20))
    pop = _pop((3, 2), 1, 4)
    pop._mhead = K.multi_head((3, 3))  # sums to 6, the actor has 5 logits
    with pytest.raises(_lib.AgxError, match="nvec"):
        _step(pop, _obs(1, 4), sample=False)


# ---- 8. one learner update ---------------------------------------------------------------- #
def _filled_population(ent_coef, masks, seed=3):
    """P = 2, N = 8, T = 4 with a rollout from the policy-step kernel itself."""
    from agilerl_amd.population.ppo_pop import PPOPopulation

    P, N, T, nvec = 2, 8, 4, (3, 2, 4)
    pop = PPOPopulation(_spec(nvec), P, N, learn_step=T * N, batch_size=16, update_epochs=1, lr=1e-3,
                        ent_coef=ent_coef, device=DEV, seed_base=seed, action_masks=masks)
    W, _, _, _ = pop.spec.views(pop.params.data, pop.spec.actor[-1])
    W.mul_(10.0)
    g = torch.Generator().manual_seed(seed)
    pop.obs.copy_(torch.randn(P, T, N, 8, generator=g))
    if masks:
        m = M.random_mask(np.random.default_rng(seed), P * T * N, nvec).reshape(P, T, N, -1)
        pop.action_masks.copy_(torch.from_numpy(m))
    for t in range(T):
        pop.act_into(t)
    pop.rewards.copy_(torch.randn(P, T, N, generator=g))
    pop.dones.copy_((torch.rand(P, T, N, generator=g) < 0.1).to(torch.uint8))
    pop.finish_rollout(torch.randn(P, N, 8, generator=g).to(DEV), torch.zeros(P, N, dtype=torch.uint8, device=DEV))
    return pop


@pytest.mark.parametrize("masks", [False, True], ids=["nomask", "mask"])
def test_multi_learner_update_matches_torch_twin(masks):
    """One epoch of two 16-row minibatches per agent from the same state,
    against an independent pure-torch twin: spec.forward, per-component
    log_softmax / softmax in torch ops, the ppo.py loss with torch ops,
    clip_grad_norm_ over the two groups and torch.optim.Adam; the first Adam
    moment and the parameters by the `close` criterion of
    test_gauss_learner_update_matches_torch_twin.  With masks the sampled
    actions are legal and the twin applies torch.where to the logits."""
    from agilerl_amd.population.nets import multi_categorical

    np.random.seed(11)
    pop = _filled_population(0.01, masks)
    spec, P, S, nvec = pop.spec, pop.P, pop.S, pop.spec.nvec
    K, L = len(nvec), spec.n_actions
    assert pop.actions.shape == (P, 4, 8, K) and pop.actions.dtype == torch.int64
    assert not pop._fused_learner()
    if masks:
        assert pop.action_masks.shape == (P, 4, 8, L)
        flat = pop.actions.cpu().numpy() + np.asarray(M.offsets(nvec))
        assert np.take_along_axis(pop.action_masks.cpu().numpy(), flat, -1).all() and (pop.action_masks == 0).any()
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
            mk = pop.action_masks.view(P, S, L)[p, idx] if masks else None
            logp, ent = multi_categorical(logits[0], nvec, pop.actions.view(P, S, K)[p, idx], mk)
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


# ---- 9. drop-in ----------------------------------------------------------------------------- #
def test_multi_dropin_create_population_train_on_policy(monkeypatch):
    """create_population("PPO", MultiDiscrete actions) + train_on_policy on the
    factored synthetic env for a few generations with tournament and mutations
    on, architecture mutations included; the rollouts and evaluations never
    reach torch's layer_norm (the policy step is the HIP kernel); int64 [8, 2]
    actions within nvec reach every agent's env; the losses are finite."""
    import torch.nn.functional as F

    from agilerl_amd.envs import Box, MultiDiscrete, SyntheticVecEnv
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
            seen.append((a.dtype, a.shape, bool((a >= 0).all() and (a < np.array([3, 2])).all())))
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

    obs_space, act_space = Box(-np.inf, np.inf, (8,)), MultiDiscrete((3, 2))
    INIT_HP = {"BATCH_SIZE": 32, "LR": 1e-3, "LEARN_STEP": 64, "UPDATE_EPOCHS": 2}
    pop = create_population("PPO", None, INIT_HP, obs_space, act_space, population_size=2, num_envs=8)
    population = pop[0].population
    assert population.multidiscrete and population.actions.shape == (2, 8, 8, 2)
    assert population.fused_descriptor() is None and population.learn_descriptor() is None
    assert population.eval_descriptor() is None and not population._fused_learner()
    env = Env(8, seed=3, p_done=0.05, max_episode_steps=40, nvec=(3, 2))  # the shared N-env, cloned per agent
    np.random.seed(0)
    torch.manual_seed(0)
    mut = Mutations(no_mutation=0.2, architecture=0.4, new_layer_prob=0.5, parameters=0.2, activation=0, rl_hp=0.2,
                    rand_seed=1)
    pop, fits = train_on_policy(env, "Synthetic", "PPO", pop, INIT_HP=INIT_HP, max_steps=384, evo_steps=128,
                                eval_loop=1, tournament=TournamentSelection(2, True, 2, 1), mutation=mut,
                                verbose=False)
    assert len(fits) == 3 and all(len(f) == 2 and np.all(np.isfinite(f)) for f in fits)
    assert seen and all(s == (np.dtype(np.int64), (8, 2), True) for s in seen), set(seen)
    assert len(losses) >= 3 and all(bool(torch.isfinite(x).all()) for x in losses)
    for a in pop:
        assert a.spec.head == "multidiscrete" and a.spec.nvec == (3, 2) and a.spec.actor[-1].fout == 5
        assert a.population.multidiscrete and a.population.learn_descriptor() is None


def test_multi_architecture_mutation_keeps_acting():
    from agilerl_amd.algorithms.ppo import PPO
    from agilerl_amd.envs import Box, MultiDiscrete

    agent = PPO(Box(-np.inf, np.inf, (8,)), MultiDiscrete((3, 2)), num_envs=4, learn_step=16, batch_size=8)
    assert agent.architecture_mutation(0.5, np.random.default_rng(0)) is not None
    assert agent.spec.head == "multidiscrete" and agent.spec.nvec == (3, 2) and agent.population.multidiscrete
    a, lp, ent, v = agent.get_action(np.zeros((4, 8), np.float32))
    assert a.shape == (4, 2) and np.isfinite(lp).all()


def test_multi_standalone_agent_and_checkpoint(tmp_path):
    """A standalone MultiDiscrete PPO: get_action (with an action_mask), the
    deprecated learn(experiences), rollout_buffer.add + learn(), test(); a
    checkpoint save / load reproduces the next greedy actions."""
    from agilerl_amd.algorithms.ppo import PPO
    from agilerl_amd.envs import Box, MultiDiscrete, SyntheticVecEnv

    T, N, nvec = 4, 4, (3, 2, 4)
    agent = PPO(Box(-np.inf, np.inf, (8,)), MultiDiscrete(nvec), num_envs=N, learn_step=T * N, batch_size=8,
                update_epochs=2, lr=1e-3)
    assert agent.population.multidiscrete
    rng = np.random.default_rng(0)
    np.random.seed(0)
    obs = rng.standard_normal((T, N, 8)).astype(np.float32)
    steps = [agent.get_action(obs[t]) for t in range(T)]
    actions, logp, values = (np.stack([s[i] for s in steps]) for i in (0, 1, 3))
    assert actions.shape == (T, N, 3) and actions.dtype == np.int64 and logp.shape == (T, N)
    assert (actions >= 0).all() and (actions < np.asarray(nvec)).all()
    logits, _ = _cpu_forward(agent.population, torch.from_numpy(obs[0]).view(1, N, 8))
    want, _ = M.logp_entropy(logits[0], nvec, actions[0])
    np.testing.assert_allclose(logp[0], want, rtol=1e-5, atol=1e-5 * sum(nvec))
    mask = np.zeros((N, sum(nvec)), np.uint8)
    mask[:, [1, 3, 8]] = 1  # one legal choice per component
    am = agent.get_action(obs[0], action_mask=mask)[0]
    assert np.array_equal(am, np.tile([1, 0, 3], (N, 1)))

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
    assert torch.equal(agent.population.actions[0].cpu(), torch.from_numpy(actions))
    buf.compute_returns_and_advantages(values[-1], dones[-1])
    loss = agent.learn()
    assert np.isfinite(loss) and not torch.equal(agent.population.params.data, p1)

    seen = []

    class Env(SyntheticVecEnv):
        def step(self, actions, **kw):
            seen.append(np.asarray(actions))
            return super().step(actions, **kw)

    fit = agent.test(Env(N, seed=1, p_done=0.2, max_episode_steps=10, nvec=nvec), loop=1)
    assert np.isfinite(fit) and agent.fitness == [fit]
    assert seen and all(a.shape == (N, 3) and a.dtype == np.int64 for a in seen)

    ck = os.path.join(tmp_path, "multi.pt")
    agent.save_checkpoint(ck)
    back = PPO.load(ck, device=DEV)
    assert back.population.multidiscrete and back.spec.nvec == nvec and list(back.action_space.nvec) == list(nvec)
    assert torch.equal(back.population.params.data[0], agent.population.params.data[agent.row])
    o = torch.from_numpy(obs[1]).to(DEV).view(1, N, 8)
    ga, gb = agent.population.evaluate(o), back.population.evaluate(o)
    assert ga.shape == (1, N, 3) and torch.equal(ga, gb)


# ---- regression guard ------------------------------------------------------------------------ #
def test_discrete_population_after_multidiscrete_population_keeps_the_fused_kernels():
    from agilerl_amd.envs import Box, Discrete, MultiDiscrete
    from agilerl_amd.utils import create_population

    obs_space = Box(-np.inf, np.inf, (8,))
    md = create_population("PPO", None, {"LEARN_STEP": 64}, obs_space, MultiDiscrete((4,)), population_size=2,
                           num_envs=8)
    mp = md[0].population
    assert mp.multidiscrete and mp.actions.shape == (2, 8, 8, 1) and mp.actions.dtype == torch.int64
    assert mp.fused_descriptor() is None and mp.learn_descriptor() is None and mp.eval_descriptor() is None
    net = {"encoder_config": {"hidden_size": [64]}, "head_config": {"hidden_size": [64]}, "latent_dim": 64}
    disc = create_population("PPO", net, {"LEARN_STEP": 64}, obs_space, Discrete(4), population_size=2, num_envs=8)
    population = disc[0].population
    assert not population.gaussian and not population.multidiscrete and population.fused_descriptor() is not None
    assert population.actions.dtype == torch.int64 and population.actions.shape == (2, 8, 8)
    default = create_population("PPO", None, {"LEARN_STEP": 64}, obs_space, Discrete(4), population_size=2, num_envs=8)
    assert default[0].population.learn_descriptor() is not None and not default[0].population.multidiscrete
