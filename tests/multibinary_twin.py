"""Independent restatements for the MultiBinary-PPO tests (PPO over MultiBinary
action spaces, include/agx_bernoulli.h), in float64 numpy:

  * ``uniforms`` / ``choices``: the uniforms of the flat bit indices over
    ``multidisc_twin.gumbel_uniforms`` (the multi-categorical step's stream) and
    the sampled bits a_j = 1[u_j < p_j], with the gap |u_j - p_j|;
  * ``logp_entropy`` / ``loss_and_grads``: the n Bernoullis' log-prob and
    entropy (illegal logits -> -1e8 first) and the clipped PPO loss with torch
    autograd's gradients written out by hand (a masked logit gets 0) — pinned
    to the reference's own functions by tests/golden/multibinary_*.npz
    (tests/test_multibinary_ppo_cpu.py);
  * ``loss_inputs``: seeded float32 inputs of a loss call whose value / adv
    rows sit on ``gauss_twin.loss_inputs``' tie rules.
"""

from __future__ import annotations

import numpy as np

from tests.gauss_twin import loss_inputs as _gauss_loss_inputs
from tests.multidisc_twin import COUNTER, SEED, gumbel_uniforms, masked  # noqa: F401

# the bit counts of every test: one bit, the lanes' first logits only, exactly
# the 16-lane boundary, one bit into the lanes' second logits, full width
NS = [1, 2, 5, 16, 17, 32]


# ---- sampling ------------------------------------------------------------------ #
def uniforms(P: int, N: int, n: int, seed: int, counter: int, env_base=None) -> np.ndarray:
    """float64 u [P, N, n] of a whole launch: agent p's env 0 is env_base[p], or p N."""
    base = np.arange(P) * N if env_base is None else np.asarray(env_base)
    env = (base[:, None] + np.arange(N)[None, :])[:, :, None]
    return gumbel_uniforms(env, np.arange(n)[None, None, :], seed, counter).astype(np.float64)


def sigmoid(lg) -> np.ndarray:
    lg = np.asarray(lg, np.float64)
    e = np.exp(-np.abs(lg))
    return np.where(lg >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def choices(logits, u, mask=None):
    """Sampled bits of (masked) logits [..., n] under uniforms u -> (bits int64
    [..., n], gap [..., n] = |u - p|: a bit whose gap is tiny may flip in float32)."""
    p = sigmoid(masked(logits, mask))
    return (u < p).astype(np.int64), np.abs(u - p)


def mode(logits, mask=None) -> np.ndarray:
    """The greedy bits: 1 iff the (masked) logit is > 0."""
    return (masked(logits, mask) > 0).astype(np.int64)


# ---- distribution and loss, float64 -------------------------------------------- #
def parts(logits, mask=None):
    """(p, q, log p, log q) [..., n] of the (masked) logits, each from
    exp(-|l|): finite for |l| up to 1e8."""
    lg = masked(logits, mask)
    e = np.exp(-np.abs(lg))
    s = np.log1p(e)
    p = np.where(lg >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    q = np.where(lg >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    return p, q, np.minimum(lg, 0.0) - s, np.minimum(-lg, 0.0) - s


def logp_entropy(logits, action, mask=None):
    """float64 (log_prob [...], entropy [...]) of action [..., n] (anything but
    0 counts as 1)."""
    p, q, lp, lq = parts(logits, mask)
    a = np.asarray(action) != 0
    logp = np.where(a, lp, lq).sum(-1)
    ent = -(p * np.log(p + 1e-8) + q * np.log(q + 1e-8)).sum(-1)
    return logp, ent


def loss_and_grads(logits, value, actions, mask, old_logp, adv, ret, old_v, index, b, clip, vf, ent):
    """The sum over minibatches of the ppo.py:868-902 loss and its gradients in
    float64.  logits [S, n] (raw), value [S] (minibatch m = samples [m b,
    (m + 1) b)); actions [rows, n], mask [rows, n] or None and the other
    rollout arrays are indexed by ``index`` [S] (None: sample i is row i).
    -> dict(g_logits [S, n], g_value [S], stats [nmb, 8], logp, entropy)."""
    f = lambda x: np.asarray(x, np.float64)  # noqa: E731
    logits, value = f(logits), f(value)
    S = logits.shape[0]
    nmb = S // b
    src = np.arange(S) if index is None else np.asarray(index)
    a = (np.asarray(actions)[src] != 0).astype(np.float64)
    mk = None if mask is None else np.asarray(mask)[src]
    olp, adv, ret, ov = f(old_logp)[src], f(adv)[src], f(ret)[src], f(old_v)[src]
    logp, H = logp_entropy(logits, a, mk)
    p, q, _, _ = parts(logits, mk)
    lr = logp - olp
    ratio = np.exp(lr)
    lo, hi = 1.0 - clip, 1.0 + clip
    p1, p2 = -adv * ratio, -adv * np.clip(ratio, lo, hi)
    half = lambda x, y: np.where(x > y, 1.0, np.where(x == y, 0.5, 0.0))  # noqa: E731  maximum's tie rule
    inr = ((ratio >= lo) & (ratio <= hi)).astype(np.float64)  # clamp: closed interval
    g_lp = (half(p1, p2) * -adv + half(p2, p1) * -adv * inr) / b * ratio
    dv = value - ov
    vc = ov + np.clip(dv, -clip, clip)
    eu, ec = value - ret, vc - ret
    lu, lc = eu * eu, ec * ec
    inv = ((dv >= -clip) & (dv <= clip)).astype(np.float64)
    g_v = vf * 0.5 / b * (half(lu, lc) * 2 * eu + half(lc, lu) * 2 * ec * inv)
    # d log_prob / dl_j = a_j - p_j;  dH / dl_j = -p_j q_j (t(p_j) - t(q_j))
    t = lambda x: np.log(x + 1e-8) + x / (x + 1e-8)  # noqa: E731
    dH = -p * q * (t(p) - t(q))
    g_logits = g_lp[:, None] * np.where(a != 0, q, -p) + (-ent / b) * dH
    if mk is not None:
        g_logits = np.where(mk != 0, g_logits, 0.0)  # torch.where passes nothing to a masked logit
    mb = lambda x: x.reshape(nmb, b).mean(1)  # noqa: E731
    pg, vl, el = mb(np.maximum(p1, p2)), 0.5 * mb(np.maximum(lu, lc)), -mb(H)
    stats = np.zeros((nmb, 8))
    stats[:, 0] = pg + vf * vl + ent * el
    stats[:, 1], stats[:, 2], stats[:, 3] = pg, vl, el
    stats[:, 4] = mb((ratio - 1.0) - lr)
    stats[:, 5] = mb((np.abs(ratio - 1.0) > clip).astype(np.float64))
    return dict(g_logits=g_logits, g_value=g_v, stats=stats, logp=logp, entropy=H)


def random_mask(rng, rows: int, n: int, keep=None) -> np.ndarray:
    """uint8 [rows, n], about a third illegal; the stored 1-bits of ``keep``
    [rows, n] stay legal (a masked bit is never sampled as 1)."""
    m = (rng.random((rows, n)) > 0.35).astype(np.uint8)
    if keep is not None:
        m[np.asarray(keep) != 0] = 1
    return m


def loss_inputs(n: int, b: int, nmb: int, rows: int | None, seed: int, clip: float, with_mask: bool):
    """Seeded float32 / int64 inputs of a loss call: ``nmb`` minibatches of
    ``b`` rows over a rollout of ``rows`` rows (None: no gather).  value, adv,
    ret, old_v and the gather index are gauss_twin.loss_inputs' own (rows on
    the maximum ties and on the closed clamp edges included)."""
    g = _gauss_loss_inputs(1, b, nmb, rows, seed, clip)
    rng = np.random.default_rng(seed + 2000)
    S = b * nmb
    R = S if rows is None else rows
    index = g["index"]
    src = np.arange(S) if index is None else index
    logits = (1.5 * rng.standard_normal((S, n))).astype(np.float32)
    actions = rng.integers(0, 2, (R, n)).astype(np.int64)
    mask = random_mask(rng, R, n, keep=actions) if with_mask else None
    lp, _ = logp_entropy(logits, actions[src], None if mask is None else mask[src])
    old_logp = np.zeros(R, np.float32)
    old_logp[src] = (lp + rng.normal(0, 0.15, S)).astype(np.float32)  # ratios on both sides of the clip range
    return dict(logits=logits, value=g["value"], actions=actions, mask=mask, old_logp=old_logp, adv=g["adv"],
                ret=g["ret"], old_v=g["old_v"], index=index)
