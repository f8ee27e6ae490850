"""The project's own restatement of IPPO's ``_learn_individual``
(agilerl/algorithms/ippo.py:644-836) for the IPPO tests, in numpy and plain
torch on the CPU:

  * ``gae_f32``: the GAE of ippo.py:702-725 as scalar numpy-float32
    operations in the torch loop's order (bit for bit; pinned to the
    reference by tests/golden/ippo_*.npz);
  * ``normalize``: one minibatch's advantages, as torch float32 ops
    (``how="torch"``, what the reference runs) or evaluated in float64 and
    rounded once (``how="f64"``, agx_ppo_learn_args.adv_norm_minibatch);
  * ``learn``: the epochs x minibatches of ippo.py:739-836 over a flat
    parameter row of an ``ActorCriticSpec`` with separate encoders: the two
    losses, the two ``clip_grad_norm_`` calls and the two Adam steps, which
    are the row's clip groups [0, actor_end) and [actor_end, n).
"""

from __future__ import annotations

import numpy as np
import torch

from agilerl_amd.population.nets import bernoulli_head, categorical, gaussian, multi_categorical


def gae_f32(rewards, dones, values, next_value, next_done, gamma: float, gae_lambda: float):
    """rewards / dones / values float32 [T, M], next_* [M] -> (advantages,
    returns) float32 [T, M].  Every operation is one float32 operation, in the
    order of the torch ops (gamma, and the double product gamma * lambda, each
    rounded to float32 once)."""
    f = np.float32
    r, d, v = (np.asarray(x, f) for x in (rewards, dones, values))
    T = r.shape[0]
    g, gl, one = f(gamma), f(float(gamma) * float(gae_lambda)), f(1.0)
    adv = np.zeros_like(r)
    last = np.zeros(r.shape[1], f)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in reversed(range(T)):
            nd = np.asarray(next_done, f) if t == T - 1 else d[t + 1]
            nv = np.asarray(next_value, f) if t == T - 1 else v[t + 1]
            nnt = one - nd
            delta = (r[t] + (g * nv) * nnt) - v[t]
            last = delta + (gl * nnt) * last
            adv[t] = last
        ret = adv + v
    return adv, ret


def normalize(a: torch.Tensor, how: str) -> torch.Tensor:
    if how == "torch":
        return (a - a.mean()) / (a.std() + 1e-8)
    x = a.double()
    return ((x - x.mean()) / (x.std() + 1e-8)).to(a.dtype)


def normalize_f64(a: np.ndarray) -> np.ndarray:
    """float64 (a - mean) / (unbiased std + 1e-8) of float32 values (not rounded)."""
    x = np.asarray(a, np.float64)
    return (x - x.mean()) / (x.std(ddof=1) + 1e-8)


def head_logp_entropy(spec, w, out, actions):
    if spec.head == "gaussian":
        return gaussian(out, spec.log_std_view(w), actions)
    if spec.head == "multidiscrete":
        return multi_categorical(out, spec.nvec, actions)
    if spec.head == "multibinary":
        return bernoulli_head(out, actions)
    logp_all, ent = categorical(out)
    return logp_all.gather(-1, actions.unsqueeze(-1)).squeeze(-1), ent


def learn(spec, params, exp_avg, exp_avg_sq, step: int, obs, actions, old_logp, adv, ret, old_v, perms, batch: int,
          *, lr: float, clip: float, ent: float, vf: float, max_norm: float, how: str = "f64", dtype=torch.float32,
          betas=(0.9, 0.999), eps: float = 1e-8):
    """``perms`` [E, S]: epoch e visits rows perms[e] in order, in minibatches
    of ``batch`` (a one-row minibatch is skipped, ippo.py:762).  The state
    (params, exp_avg, exp_avg_sq: 1-D tensors) is not modified.  ->
    (params, exp_avg, exp_avg_sq, step, mean_loss)."""
    t = lambda x: torch.as_tensor(np.asarray(x)) if not isinstance(x, torch.Tensor) else x  # noqa: E731
    fl = lambda x: t(x).to(dtype)  # noqa: E731
    p, m, v = (fl(x).clone() for x in (params, exp_avg, exp_avg_sq))
    obs, old_logp, adv, ret, old_v = (fl(x) for x in (obs, old_logp, adv, ret, old_v))
    actions = fl(actions) if spec.head == "gaussian" else t(actions).long()
    S = adv.shape[0]
    E = len(perms)
    edges = [0, spec.actor_end, spec.n_params]
    b1, b2 = betas
    total = 0.0
    for e in range(E):
        order = np.asarray(perms[e])
        for start in range(0, S, batch):
            mb = torch.as_tensor(order[start:start + batch])
            if len(mb) <= 1:
                continue
            w = p.clone().unsqueeze(0).requires_grad_(True)
            out, value = spec.forward(w, obs[mb].unsqueeze(0))
            logp, entropy = head_logp_entropy(spec, w, out[0], actions[mb])
            logratio = logp - old_logp[mb]
            ratio = logratio.exp()
            a = normalize(adv[mb], how)
            pg = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
            val = value[0].view(-1)
            v_clipped = old_v[mb] + torch.clamp(val - old_v[mb], -clip, clip)
            v_loss = 0.5 * torch.max((val - ret[mb]) ** 2, (v_clipped - ret[mb]) ** 2).mean()
            actor_loss = pg - ent * entropy.mean()
            critic_loss = v_loss * vf
            (actor_loss + critic_loss).backward()  # the two losses' parameters are disjoint
            g = w.grad[0]
            step += 1
            with torch.no_grad():
                for lo, hi in zip(edges[:-1], edges[1:]):
                    gg = g[lo:hi]
                    coef = torch.clamp(max_norm / (torch.linalg.vector_norm(gg) + 1e-6), max=1.0)
                    gg = gg * coef
                    m[lo:hi] = b1 * m[lo:hi] + (1 - b1) * gg
                    v[lo:hi] = b2 * v[lo:hi] + (1 - b2) * gg * gg
                    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
                    p[lo:hi] -= (lr / bc1) * m[lo:hi] / (v[lo:hi].sqrt() / bc2 ** 0.5 + eps)
            total += float(actor_loss.item()) + float(critic_loss.item())
    return p, m, v, step, total / (S * E)
