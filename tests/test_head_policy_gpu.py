"""The per-step entry points agx_ppo_act_{gauss,multi,bern}_graph with every
combination of their two action outputs: ``actions`` (the rollout slot) and
``actions_flat`` (the env's staging) are optional and independent, and neither
may change what the step computes.  The three entry points share one host
launcher and one plan function per head (csrc/head_policy.h).

Every case runs P = 2 agents over N = 1 (one partial row block) and N = 17 (a
second block with one live row), at widths 1, 17 and 32 (a lane's second
slot unused, just used, full; the multi-categorical heads are (1,), (9, 8) and
(3, 14, 15), whose second component crosses lane index 16), in the few-row
form and, with AGX_GRAPH_FEW=0, in the general one:

  A. ``actions`` and ``actions_flat`` together, a legal-action mask (the int
     heads), sample = 1 at a fixed counter: the staging equals the stored
     actions (the Gaussian head's clipped to the bounds in numpy); the stored
     actions are legal under the mask, and their log-prob and entropy are the
     twins' (tests/gauss_twin.py, multidisc_twin.py, multibinary_twin.py) at the
     bars of the heads' own step tests.
  B. only ``actions_flat``, and only ``actions``: log-probs and values
     bit-equal across the three calls, and each call's one action array equal
     to case A's.
  C. sample = 0 with only ``values``: bit-equal to the sampled call's.

What the sampled actions themselves must be (the Philox streams against the
numpy restatements) is test_gauss_policy_step_samples_the_philox_stream,
test_multi_policy_step_samples_the_gumbel_stream and
test_bern_policy_step_samples_the_uniform_stream in the heads' own files;
that the persistent launch stores what the per-step launch does is
tests/test_head_persistent_gpu.py.  Neither is repeated here."""

import numpy as np
import pytest
import torch

from tests import gauss_twin as G
from tests import multibinary_twin as B
from tests import multidisc_twin as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, D = 2, 8
NS = (1, 17)
WIDTHS = {"gauss": (1, 17, 32), "bern": (1, 17, 32), "multi": ((1,), (9, 8), (3, 14, 15))}


def _pop(head, w, N):
    from agilerl_amd.population import nets
    from agilerl_amd.population.ppo_pop import PPOPopulation

    if head == "gauss":
        spec = nets.GaussianActorCriticSpec(obs_dim=D, n_actions=w, action_low=(-0.5,) * w, action_high=(0.25,) * w)
    elif head == "multi":
        spec = nets.MultiDiscreteActorCriticSpec(obs_dim=D, n_actions=int(sum(w)), nvec=tuple(w))
    else:
        spec = nets.MultiBinaryActorCriticSpec(obs_dim=D, n_actions=w)
    pop = PPOPopulation(spec, P, N, learn_step=2 * N, batch_size=N, device=DEV, seed_base=5)
    if head == "gauss":  # a log_std per agent and dimension, so a swapped lane shows
        ls = np.random.default_rng(w).uniform(-1.0, 0.5, (P, w)).astype(np.float32)
        spec.log_std_view(pop.params.data).copy_(torch.from_numpy(ls).to(DEV))
    else:  # logits of order one instead of the 0.1-scaled initialisation's few hundredths
        spec.views(pop.params.data, spec.actor[-1])[0].mul_(20.0)
    return pop


def _step(pop, obs, *, sample, counter=0, mask=None, want=("actions", "flat", "log_probs", "values", "entropy")):
    """One per-step launch writing only the arrays named in ``want``."""
    from agilerl_amd.population.learner import policy_step_head

    N, W, L = pop.N, pop.act_width, pop.spec.n_actions
    fill = float("nan") if pop.gaussian else -7
    out = {k: torch.empty(P, N, device=DEV) for k in ("log_probs", "values", "entropy") if k in want}
    if "actions" in want:
        out["actions"] = torch.full((P, N, W), fill, dtype=pop.head.dtype, device=DEV)
    flat = torch.full((P * N * W,), fill, dtype=pop.head.dtype, device=DEV) if "flat" in want else None
    policy_step_head(pop, obs, N * D, sample=sample, counter=counter, out_agent_stride=N, actions_flat=flat,
                     action_mask=None if mask is None else torch.from_numpy(mask).to(DEV), mask_agent_stride=N * L,
                     clip=pop.action_clip(), **out)
    torch.cuda.synchronize()
    if flat is not None:
        out["flat"] = flat.view(P, N, W)
    return {k: v.cpu() for k, v in out.items()}


def _check_against_twin(head, w, pop, obs, a, mask):
    """Case A's stored actions, log-prob, entropy and values against the twins."""
    N = pop.N
    act = a["actions"].numpy()
    net_out, value = pop.spec.forward(pop.params.data.cpu(), obs.cpu())  # float32 torch on the CPU
    torch.testing.assert_close(a["values"], value.view(P, N), rtol=1e-4, atol=1e-5)
    if head == "gauss":
        # the mean from the CPU forward, not from the kernel.  The forward's bar above (rtol 1e-4, atol 1e-5 per
        # output) reaches the log-prob through |a - mu| / sigma^2 = |eps| / sigma <= 5.9 e per dimension
        # (|eps| <= 5.9, log_std >= -1); that sum over the dimensions is added to the 1e-5 per dimension of
        # test_gauss_policy_step_samples_the_philox_stream
        mu = net_out.double().numpy()
        ls = pop.spec.log_std_view(pop.params.data).cpu().numpy()[:, None, :]
        lp, H = G.logp_entropy(mu, ls, act)
        np.testing.assert_allclose(a["entropy"].numpy(), H, rtol=1e-6)
        bar = 1e-5 * np.abs(lp) + 1e-5 * w + (5.9 * np.e * (1e-4 * np.abs(mu) + 1e-5)).sum(-1)
        assert (np.abs(a["log_probs"].numpy() - lp) <= bar).all(), (w, N)
        lo, hi = (np.asarray(b, np.float32) for b in (pop.spec.action_low, pop.spec.action_high))
        return np.minimum(np.maximum(act, lo), hi)  # fminf(fmaxf(a, lo), hi)
    logits = net_out.double().numpy()
    if head == "multi":
        lp, H = M.logp_entropy(logits, w, act, mask)
        chosen = act + np.asarray(M.offsets(w))  # flat indices of the chosen logits
        assert np.take_along_axis(mask, chosen, -1).all()
        for k, n in enumerate(w):
            assert act[..., k].min() >= 0 and act[..., k].max() < n
    else:
        lp, H = B.logp_entropy(logits, act, mask)
        assert set(np.unique(act)) <= {0, 1} and not (act[mask == 0] != 0).any()  # a masked bit is never 1
    L = pop.spec.n_actions  # _check_logp_entropy's bar (test_multidisc_ppo_gpu.py): rtol 1e-5, atol 1e-5 L
    np.testing.assert_allclose(a["log_probs"].numpy(), lp, rtol=1e-5, atol=1e-5 * L)
    np.testing.assert_allclose(a["entropy"].numpy(), H, rtol=1e-5, atol=1e-5 * L)
    return act


@pytest.mark.parametrize("few", ["few", "general"])
@pytest.mark.parametrize("head", ["gauss", "multi", "bern"])
def test_one_step_serves_actions_and_staging(head, few, monkeypatch):
    if few == "general":
        monkeypatch.setenv("AGX_GRAPH_FEW", "0")
    for w in WIDTHS[head]:
        for N in NS:
            pop = _pop(head, w, N)
            obs = torch.randn(P, N, D, generator=torch.Generator().manual_seed(3)).to(DEV)
            rng = np.random.default_rng(N)
            L = pop.spec.n_actions
            mask = None
            if head != "gauss":
                rows = M.random_mask(rng, P * N, w) if head == "multi" else B.random_mask(rng, P * N, w)
                mask = rows.reshape(P, N, L)
            # A: both action arrays, mask, sampled
            a = _step(pop, obs, sample=True, counter=G.COUNTER, mask=mask)
            staged = _check_against_twin(head, w, pop, obs, a, mask)
            assert np.array_equal(a["flat"].numpy(), staged), (w, N)
            # B: one action array at a time
            f = _step(pop, obs, sample=True, counter=G.COUNTER, mask=mask, want=("flat", "log_probs", "values"))
            s = _step(pop, obs, sample=True, counter=G.COUNTER, mask=mask, want=("actions", "log_probs", "values"))
            for other in (f, s):
                assert torch.equal(other["log_probs"], a["log_probs"]) and torch.equal(other["values"], a["values"])
            assert torch.equal(f["flat"], a["flat"]) and torch.equal(s["actions"], a["actions"]), (w, N)
            # C: unsampled, values only
            v = _step(pop, obs, sample=False, mask=mask, want=("values",))
            assert torch.equal(v["values"], a["values"]), (w, N)
