"""Independent restatements for the Gaussian-PPO tests (PPO over Box action
spaces, include/agx_gauss.h), in float64 numpy and in plain torch:

  * ``philox`` / ``gauss_eps``: the Philox4x32-10 block and the Box-Muller
    mapping the policy step draws its noise from (agx_gauss.h);
  * ``logp_entropy`` / ``loss_and_grads``: the diagonal Gaussian's log-prob and
    entropy and the clipped PPO loss with torch autograd's gradients written
    out by hand (maximum ties 1/2 : 1/2, clamp passing the gradient on the
    closed interval) — pinned to the reference's own functions by
    tests/golden/gauss_*.npz (tests/test_gauss_ppo_cpu.py);
  * ``torch_loss``: the same loss with torch ops, for autograd twins.
"""

from __future__ import annotations

import math

import numpy as np
import torch

LOG_2PI = math.log(2 * math.pi)

# the seed / counter of the GPU tests' sampled policy steps (tests/test_gauss_ppo_gpu.py);
# tests/test_gauss_ppo_cpu.py checks the reference noise sequence they select
SEED, COUNTER = 0x5EED5EED1234, 77


# ---- noise ------------------------------------------------------------------ #
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint32 arrays -> 4 uint32 arrays."""
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, dtype=np.uint64) & m32 for x in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(k0) & m32, np.uint64(k1) & m32
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & m32, p1 >> np.uint64(32), p1 & m32
        c = [h1 ^ c[1] ^ k0, l1, h0 ^ c[3] ^ k1, l0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return [x.astype(np.uint32) for x in c]


def gauss_uniforms(env, d, seed: int, counter: int):
    """(u1, u2) float32 of dimension ``d`` of stream env ``env`` (arrays that
    broadcast): the block of (env, counter ^ (d >> 1) << 56), words (x, y) for
    an even d and (z, w) for an odd one, u = fl32((w >> 8) + 0.5) 2^-24."""
    env = np.asarray(env, dtype=np.uint64)
    d = np.asarray(d, dtype=np.uint64)
    hi = (np.uint64(counter >> 32) ^ ((d >> np.uint64(1)) << np.uint64(24))) & np.uint64(0xFFFFFFFF)
    x, y, z, w = philox(env & np.uint64(0xFFFFFFFF), env >> np.uint64(32), np.uint64(counter & 0xFFFFFFFF), hi,
                        seed & 0xFFFFFFFF, seed >> 32)
    odd = (d & np.uint64(1)).astype(bool)
    w1, w2 = np.where(odd, z, x), np.where(odd, w, y)
    u = lambda v: ((v >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)  # noqa: E731
    return u(w1), u(w2)


def gauss_eps(env, d, seed: int, counter: int) -> np.ndarray:
    """eps = sqrt(-2 ln u1) cos(2 pi u2) in float64 from the float32 uniforms."""
    u1, u2 = gauss_uniforms(env, d, seed, counter)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))


def population_eps(P: int, N: int, A: int, seed: int, counter: int, env_base=None) -> np.ndarray:
    """[P, N, A] noise of a whole launch (agent p's env 0 is env_base[p], or p N)."""
    base = np.arange(P) * N if env_base is None else np.asarray(env_base)
    env = (base[:, None] + np.arange(N)[None, :])[:, :, None]
    return gauss_eps(env, np.arange(A)[None, None, :], seed, counter)


# ---- distribution and loss, float64 -------------------------------------------- #
def logp_entropy(mean, log_std, action):
    """float64 (log_prob [...], entropy [...]); log_std broadcasts against mean [..., A]."""
    mean, action = np.asarray(mean, np.float64), np.asarray(action, np.float64)
    ls = np.broadcast_to(np.asarray(log_std, np.float64), mean.shape)
    logp = (-0.5 * ((action - mean) ** 2 / np.exp(2 * ls) + 2 * ls + LOG_2PI)).sum(-1)
    ent = 0.5 * (1 + LOG_2PI) * mean.shape[-1] + ls.sum(-1)
    return logp, ent


def loss_and_grads(mean, value, log_std, actions, old_logp, adv, ret, old_v, index, b, clip, vf, ent):
    """The sum over minibatches of the ppo.py:868-902 loss and its gradients in
    float64.  mean [S, A], value [S], log_std [nmb, A] (minibatch m = samples
    [m b, (m + 1) b)); the rollout arrays are indexed by ``index`` [S] (None:
    sample i is row i).  -> dict(g_mean [S, A], g_value [S], g_log_std
    [nmb, A], stats [nmb, 8])."""
    f = lambda x: np.asarray(x, np.float64)  # noqa: E731
    mean, value, log_std = f(mean), f(value), f(log_std)
    S, A = mean.shape
    nmb = S // b
    src = np.arange(S) if index is None else np.asarray(index)
    a, olp, adv, ret, ov = f(actions)[src], f(old_logp)[src], f(adv)[src], f(ret)[src], f(old_v)[src]
    ls = np.repeat(log_std, b, axis=0)
    var = np.exp(2 * ls)
    z = a - mean
    logp, H = logp_entropy(mean, ls, a)
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
    g_mean = g_lp[:, None] * z / var
    g_ls = (g_lp[:, None] * (z * z / var - 1.0)).reshape(nmb, b, A).sum(1) - ent
    mb = lambda x: x.reshape(nmb, b).mean(1)  # noqa: E731
    pg, vl, el = mb(np.maximum(p1, p2)), 0.5 * mb(np.maximum(lu, lc)), -mb(H)
    stats = np.zeros((nmb, 8))
    stats[:, 0] = pg + vf * vl + ent * el
    stats[:, 1], stats[:, 2], stats[:, 3] = pg, vl, el
    stats[:, 4] = mb((ratio - 1.0) - lr)
    stats[:, 5] = mb((np.abs(ratio - 1.0) > clip).astype(np.float64))
    return dict(g_mean=g_mean, g_value=g_v, g_log_std=g_ls, stats=stats, logp=logp, entropy=H)


# ---- the same loss with torch ops (autograd twins) -------------------------------- #
def torch_loss(logp, entropy, value, old_logp, adv, ret, old_v, clip, vf, ent):
    """One minibatch's ppo.py:868-902 loss; every argument [b].  -> (loss, approx_kl)."""
    logratio = logp - old_logp
    ratio = logratio.exp()
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    v_clipped = old_v + torch.clamp(value - old_v, -clip, clip)
    v_loss = 0.5 * torch.max((value - ret) ** 2, (v_clipped - ret) ** 2).mean()
    with torch.no_grad():
        kl = ((ratio - 1) - logratio).mean()
    return pg - ent * entropy.mean() + v_loss * vf, kl


def loss_inputs(A: int, b: int, nmb: int, rows: int | None, seed: int, clip: float):
    """Seeded float32 inputs of a loss call: ``nmb`` minibatches of ``b`` rows
    over a rollout of ``rows`` rows (None: no gather).  Some rows sit on the
    tie / closed-interval rules: adv = 0, value == old_value, and value -
    old_value exactly +-clip (clip is a power of two, so float32 and float64
    agree on the edge)."""
    rng = np.random.default_rng(seed)
    S = b * nmb
    R = S if rows is None else rows
    f32 = np.float32
    log_std = rng.uniform(-1.0, 0.5, (nmb, A)).astype(f32)
    mean = rng.standard_normal((S, A)).astype(f32)
    index = None if rows is None else rng.permutation(R)[:S].astype(np.int64)  # rows >= S: no row twice
    src = np.arange(S) if index is None else index
    actions = np.zeros((R, A), f32)
    sig = np.exp(np.repeat(log_std, b, axis=0).astype(np.float64))
    actions[src] = (mean + sig * rng.standard_normal((S, A))).astype(f32)
    lp, _ = logp_entropy(mean, np.repeat(log_std, b, axis=0), actions[src])
    old_logp = np.zeros(R, f32)
    old_logp[src] = (lp + rng.normal(0, 0.15, S)).astype(f32)  # ratios on both sides of the clip range
    adv, ret = (rng.standard_normal(R).astype(f32) for _ in range(2))
    old_v = (np.round(rng.standard_normal(R) * 1024) / 1024).astype(f32)  # old_v +- clip is exact
    value = (old_v[src] + rng.normal(0, 0.3, S)).astype(f32)
    k = np.arange(S)
    adv[src[k % 7 == 0]] = 0.0
    value[k % 7 == 1] = old_v[src[k % 7 == 1]]
    value[k % 7 == 2] = old_v[src[k % 7 == 2]] + f32(clip)
    value[k % 7 == 3] = old_v[src[k % 7 == 3]] - f32(clip)
    return dict(mean=mean, value=value, log_std=log_std, actions=actions, old_logp=old_logp, adv=adv, ret=ret,
                old_v=old_v, index=index)
