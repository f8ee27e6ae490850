"""Independent restatements for the MultiDiscrete-PPO tests (PPO over
MultiDiscrete action spaces, include/agx_multi.h), in float64 numpy:

  * ``gumbel_scores`` / ``choices``: the Gumbel-max scores of the flat logit
    indices over ``gauss_twin.philox`` (agx_ppo_act's stream, keyed by the flat
    index) and the first maximum of every component;
  * ``logp_entropy`` / ``loss_and_grads``: the K categoricals' log-prob and
    entropy (illegal logits -> -1e8 first) and the clipped PPO loss with torch
    autograd's gradients written out by hand (a masked logit gets 0) — pinned
    to the reference's own functions by tests/golden/multidisc_*.npz
    (tests/test_multidisc_ppo_cpu.py);
  * ``loss_inputs``: seeded float32 inputs of a loss call whose value / adv
    rows sit on ``gauss_twin.loss_inputs``' tie rules.
"""

from __future__ import annotations

import numpy as np

from tests.gauss_twin import loss_inputs as _gauss_loss_inputs
from tests.gauss_twin import philox

# the nvec cases of every test: smallest component, two components, a one-way
# component (log-prob 0), a boundary exactly at index 16, a component across
# index 16, K = 16 with L = 32, one full-width component
NVECS = [(2,), (3, 2), (5, 1, 4), (16, 16), (7, 20, 5), (2,) * 16, (32,)]

SEED, COUNTER = 0x5EED5EED4321, 91


def offsets(nvec) -> list[int]:
    return [int(x) for x in np.concatenate([[0], np.cumsum(nvec)[:-1]])]


def masked(logits, mask):
    """float64 logits with the illegal ones at -1e8 (mask: 1 = legal, or None)."""
    lg = np.asarray(logits, np.float64)
    return lg if mask is None else np.where(np.asarray(mask) != 0, lg, -1e8)


# ---- sampling ------------------------------------------------------------------ #
def gumbel_uniforms(env, j, seed: int, counter: int):
    """float32 u of flat logit index ``j`` of stream env ``env`` (arrays that
    broadcast): word j & 3 of the block of (env, counter ^ (j >> 2) << 56),
    u = fl32((w >> 8) + 0.5) 2^-24."""
    env = np.asarray(env, dtype=np.uint64)
    j = np.asarray(j, dtype=np.uint64)
    hi = (np.uint64(counter >> 32) ^ ((j >> np.uint64(2)) << np.uint64(24))) & np.uint64(0xFFFFFFFF)
    words = philox(env & np.uint64(0xFFFFFFFF), env >> np.uint64(32), np.uint64(counter & 0xFFFFFFFF), hi,
                   seed & 0xFFFFFFFF, seed >> 32)
    sel = (j & np.uint64(3)).astype(np.int64)
    w = np.choose(np.broadcast_to(sel, words[0].shape), words)
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def gumbel_scores(logits, seed: int, counter: int, env_base=None, mask=None) -> np.ndarray:
    """float64 scores [P, N, L] of a whole launch over (masked) logits [P, N, L]:
    lg_j - log(-log u_j); agent p's env 0 is env_base[p], or p N."""
    lg = masked(logits, mask)
    P, N, L = lg.shape
    base = np.arange(P) * N if env_base is None else np.asarray(env_base)
    env = (base[:, None] + np.arange(N)[None, :])[:, :, None]
    u = gumbel_uniforms(env, np.arange(L)[None, None, :], seed, counter).astype(np.float64)
    return lg - np.log(-np.log(u))


def choices(scores, nvec):
    """First maximum of every component of scores [..., L] -> (choice [..., K]
    int64 in [0, n_k), gap [..., K]: the top-two score gap, inf for n_k = 1)."""
    scores = np.asarray(scores, np.float64)
    ch, gap = [], []
    for off, n in zip(offsets(nvec), nvec):
        s = scores[..., off:off + n]
        ch.append(np.argmax(s, axis=-1))
        if n == 1:
            gap.append(np.full(s.shape[:-1], np.inf))
        else:
            top = np.sort(s, axis=-1)
            gap.append(top[..., -1] - top[..., -2])
    return np.stack(ch, -1).astype(np.int64), np.stack(gap, -1)


# ---- distribution and loss, float64 -------------------------------------------- #
def softmax_parts(logits, nvec, mask=None):
    """(p [..., L], lse [..., K]) of the K categoricals over (masked) logits."""
    lg = masked(logits, mask)
    p = np.zeros_like(lg)
    lse = []
    for off, n in zip(offsets(nvec), nvec):
        s = lg[..., off:off + n]
        m = s.max(-1, keepdims=True)
        l = m + np.log(np.exp(s - m).sum(-1, keepdims=True))
        p[..., off:off + n] = np.exp(s - l)
        lse.append(l[..., 0])
    return p, np.stack(lse, -1)


def logp_entropy(logits, nvec, action, mask=None):
    """float64 (log_prob [...], entropy [...]) of action [..., K], both summed
    over the components in ascending order."""
    lg = masked(logits, mask)
    p, lse = softmax_parts(lg, nvec)
    action = np.asarray(action)
    logp = np.zeros(lg.shape[:-1])
    ent = np.zeros(lg.shape[:-1])
    for k, (off, n) in enumerate(zip(offsets(nvec), nvec)):
        chosen = np.take_along_axis(lg[..., off:off + n], action[..., k:k + 1], -1)[..., 0]
        logp = logp + (chosen - lse[..., k])
        pk = p[..., off:off + n]
        ent = ent + -(pk * np.log(pk + 1e-8)).sum(-1)
    return logp, ent


def loss_and_grads(logits, value, nvec, actions, mask, old_logp, adv, ret, old_v, index, b, clip, vf, ent):
    """The sum over minibatches of the ppo.py:868-902 loss and its gradients in
    float64.  logits [S, L] (raw), value [S] (minibatch m = samples [m b,
    (m + 1) b)); actions [rows, K], mask [rows, L] or None and the other
    rollout arrays are indexed by ``index`` [S] (None: sample i is row i).
    -> dict(g_logits [S, L], g_value [S], stats [nmb, 8], logp, entropy)."""
    f = lambda x: np.asarray(x, np.float64)  # noqa: E731
    logits, value = f(logits), f(value)
    S, L = logits.shape
    nmb = S // b
    src = np.arange(S) if index is None else np.asarray(index)
    a = np.asarray(actions)[src]
    mk = None if mask is None else np.asarray(mask)[src]
    olp, adv, ret, ov = f(old_logp)[src], f(adv)[src], f(ret)[src], f(old_v)[src]
    logp, H = logp_entropy(logits, nvec, a, mk)
    p, _ = softmax_parts(logits, nvec, mk)
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
    # d log_prob / d lg_j = 1[j == off_k + a_k] - p_j;  dH_k / d lg_j = -p_j (t_j - sum_i p_i t_i)
    t = np.log(p + 1e-8) + p / (p + 1e-8)
    onehot = np.zeros_like(p)
    dH = np.zeros_like(p)
    for k, (off, n) in enumerate(zip(offsets(nvec), nvec)):
        np.put_along_axis(onehot[:, off:off + n], a[:, k:k + 1], 1.0, -1)
        pk, tk = p[:, off:off + n], t[:, off:off + n]
        dH[:, off:off + n] = -pk * (tk - (pk * tk).sum(-1, keepdims=True))
    g_logits = g_lp[:, None] * (onehot - p) + (-ent / b) * dH
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


def random_mask(rng, rows: int, nvec, keep=None) -> np.ndarray:
    """uint8 [rows, L], about a third illegal; every component keeps at least
    one legal logit, and ``keep`` [rows, K] (the stored actions) stay legal."""
    L = int(sum(nvec))
    m = (rng.random((rows, L)) > 0.35).astype(np.uint8)
    for k, (off, n) in enumerate(zip(offsets(nvec), nvec)):
        forced = rng.integers(0, n, rows) if keep is None else np.asarray(keep)[:, k]
        m[np.arange(rows), off + forced] = 1
    return m


def loss_inputs(nvec, b: int, nmb: int, rows: int | None, seed: int, clip: float, with_mask: bool):
    """Seeded float32 / int64 inputs of a loss call: ``nmb`` minibatches of
    ``b`` rows over a rollout of ``rows`` rows (None: no gather).  value, adv,
    ret, old_v and the gather index are gauss_twin.loss_inputs' own (rows on
    the maximum ties and on the closed clamp edges included)."""
    g = _gauss_loss_inputs(1, b, nmb, rows, seed, clip)
    rng = np.random.default_rng(seed + 1000)
    S, L, K = b * nmb, int(sum(nvec)), len(nvec)
    R = S if rows is None else rows
    index = g["index"]
    src = np.arange(S) if index is None else index
    logits = (1.5 * rng.standard_normal((S, L))).astype(np.float32)
    actions = np.stack([rng.integers(0, n, R) for n in nvec], -1).astype(np.int64)
    mask = random_mask(rng, R, nvec, keep=actions) if with_mask else None
    lp, _ = logp_entropy(logits, nvec, actions[src], None if mask is None else mask[src])
    old_logp = np.zeros(R, np.float32)
    old_logp[src] = (lp + rng.normal(0, 0.15, S)).astype(np.float32)  # ratios on both sides of the clip range
    assert actions.shape == (R, K)
    return dict(logits=logits, value=g["value"], actions=actions, mask=mask, old_logp=old_logp, adv=g["adv"],
                ret=g["ret"], old_v=g["old_v"], index=index)
