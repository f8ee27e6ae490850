"""Typed torch-tensor front end of the libagx.so C ABI (include/agx.h).

Every function takes device tensors, validates shapes/dtypes/devices on the
host (so a kernel never sees a mismatched grid), launches on the current HIP
stream and returns without synchronising.  No CPU fallback exists.  (One
function here is torch ops by design: ``bandit_select_torch``, the bandit
agents' CPU arithmetic and ``bandit_select``'s stated path past the kernel's
shape range.)
"""

from __future__ import annotations

import ctypes

import torch

from . import _lib

_f32, _f64, _u8, _i64, _i32 = torch.float32, torch.float64, torch.uint8, torch.int64, torch.int32


def _need(t: torch.Tensor, name: str, dtype=None, shape=None, contiguous=True) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise ValueError(f"{name}: must live on the GPU (got {t.device})")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# --------------------------------------------------------------------------- #
# GAE                                                                         #
# --------------------------------------------------------------------------- #
def gae(rewards, dones, values, last_value, last_done, gamma=0.99, gae_lambda=0.95, use_gae=True,
        advantages=None, returns=None, with_stats=False, workspace=None, stats_out=None):
    """rewards/values f32 [P,T,N] (or [T,N]), dones u8/bool, last_* [P,N].
    Returns (advantages, returns[, stats f64 [P,2] = mean, unbiased std])."""
    squeeze = rewards.dim() == 2
    r = rewards.unsqueeze(0) if squeeze else rewards
    P, T, N = r.shape
    v = values.reshape(P, T, N)
    d = dones.reshape(P, T, N)
    if d.dtype == torch.bool:
        d = d.view(torch.uint8)
    lv = last_value.reshape(P, N)
    ld = last_done.reshape(P, N)
    if ld.dtype == torch.bool:
        ld = ld.view(torch.uint8)
    _need(r, "rewards", _f32)
    _need(v, "values", _f32)
    _need(d, "dones", _u8)
    _need(lv, "last_value", _f32)
    _need(ld, "last_done", _u8)
    adv = torch.empty_like(r) if advantages is None else advantages.reshape(P, T, N)
    ret = torch.empty_like(r) if returns is None else returns.reshape(P, T, N)
    _need(adv, "advantages", _f32)
    _need(ret, "returns", _f32)
    stats = None
    if with_stats:
        stats = torch.empty(P, 2, dtype=_f64, device=r.device) if stats_out is None else stats_out
        _need(stats, "stats_out", _f64, (P, 2))
        if workspace is None:
            workspace = _ws(_lib.load().agx_gae_workspace_bytes(P, T, N), r.device)
    _lib.call("agx_gae", r.data_ptr(), d.data_ptr(), v.data_ptr(), lv.data_ptr(), ld.data_ptr(),
              P, T, N, float(gamma), float(gae_lambda), int(bool(use_gae)), adv.data_ptr(),
              ret.data_ptr(), _lib.ptr(stats), _lib.ptr(workspace), _lib.stream())
    if squeeze:
        adv, ret = adv[0], ret[0]
    return (adv, ret, stats) if with_stats else (adv, ret)


def gae_launcher(rewards, dones, values, last_value, last_done, gamma, gae_lambda, use_gae, advantages,
                 returns, stats_out, workspace):
    """Validate once, then return ``launch(stream)``: agx_gae on these fixed
    tensors (the population's persistent rollout buffers) with no per-call
    checks — the per-iteration call costs one ctypes call, not ~10 tensor
    validations (host time that sat between the rollout and the learner)."""
    adv, ret, _ = gae(rewards, dones, values, last_value, last_done, gamma, gae_lambda, use_gae,
                      advantages=advantages, returns=returns, with_stats=True, workspace=workspace,
                      stats_out=stats_out)  # validates (and runs once)
    P, T, N = adv.shape
    d = dones.view(torch.uint8) if dones.dtype == torch.bool else dones
    ld = last_done.view(torch.uint8) if last_done.dtype == torch.bool else last_done
    fn = _lib.load().agx_gae
    args = (rewards.data_ptr(), d.data_ptr(), values.data_ptr(), last_value.data_ptr(), ld.data_ptr(), P, T, N,
            float(gamma), float(gae_lambda), int(bool(use_gae)), adv.data_ptr(), ret.data_ptr(),
            stats_out.data_ptr(), workspace.data_ptr())

    def launch(stream: int) -> None:
        rc = fn(*args, stream)
        if rc != 0:
            _lib.check(rc, "agx_gae")

    return launch


def adv_normalize_(adv: torch.Tensor, stats: torch.Tensor) -> torch.Tensor:
    P = stats.shape[0]
    _need(adv, "adv", _f32)
    _need(stats, "stats", _f64, (P, 2))
    _lib.call("agx_adv_normalize", adv.data_ptr(), stats.data_ptr(), P, adv.numel() // P, _lib.stream())
    return adv


# --------------------------------------------------------------------------- #
# PPO loss                                                                    #
# --------------------------------------------------------------------------- #
def ppo_loss_fwd_bwd(logp, old_logp, adv, ret, old_value, value, entropy, batch, clip_coef=0.2,
                     vf_coef=0.5, ent_coef=0.01, index=None, out=None, stats=None):
    """Returns (g_logp, g_value, g_entropy, stats[nmb, 8])."""
    S = logp.numel()
    if S % batch:
        raise ValueError(f"samples ({S}) must be a multiple of batch ({batch}); call per minibatch")
    nmb = S // batch
    for t, n in ((logp, "logp"), (value, "value"), (entropy, "entropy")):
        _need(t, n, _f32)
        if t.numel() != S:
            raise ValueError(f"{n}: expected {S} elements")
    src = old_logp.numel()
    for t, n in ((old_logp, "old_logp"), (adv, "adv"), (ret, "ret"), (old_value, "old_value")):
        _need(t, n, _f32)
        if t.numel() != src:
            raise ValueError(f"{n}: expected {src} elements")
    if index is not None:
        _need(index, "index", _i64)
        if index.numel() != S:
            raise ValueError("index: one entry per sample")
    elif src != S:
        raise ValueError("without an index the old_* arrays must match logp")
    if out is None:
        out = tuple(torch.empty_like(logp) for _ in range(3))
    if stats is None:
        stats = torch.empty(nmb, 8, dtype=_f32, device=logp.device)
    _lib.call("agx_ppo_loss_fwd_bwd", logp.data_ptr(), old_logp.data_ptr(), adv.data_ptr(),
              ret.data_ptr(), old_value.data_ptr(), value.data_ptr(), entropy.data_ptr(),
              _lib.ptr(index), int(batch), int(nmb), float(clip_coef), float(vf_coef),
              float(ent_coef), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
              stats.data_ptr(), _lib.stream())
    return out[0], out[1], out[2], stats


def _head_loss_rows(out, out_name, value, batch, actions, act_dtype, act_cols, old_logp, adv, ret, old_value, index,
                    mask):
    """The checks the head losses share: ``out`` (the actor output, f32
    [nmb * batch, W]) against value, the rollout arrays (actions [rows, act_cols]
    of act_dtype, old_logp / adv / ret / old_value [rows], mask uint8 [rows, W] or
    None) and ``index``.  -> nmb."""
    S, W = out.shape
    if S % batch:
        raise ValueError(f"samples ({S}) must be a multiple of batch ({batch}); call per minibatch")
    _need(value, "value", _f32)
    if value.numel() != S:
        raise ValueError(f"value: expected {S} elements")
    _need(actions, "actions", act_dtype)
    if actions.dim() != 2 or actions.shape[1] != act_cols:
        raise ValueError(f"actions: expected [rows, {act_cols}]")
    src = actions.shape[0]
    for t, name in ((old_logp, "old_logp"), (adv, "adv"), (ret, "ret"), (old_value, "old_value")):
        _need(t, name, _f32)
        if t.numel() != src:
            raise ValueError(f"{name}: expected {src} elements")
    if mask is not None:
        _need(mask, "mask", torch.uint8, (src, W))
    if index is not None:
        _need(index, "index", _i64)
        if index.numel() != S:
            raise ValueError("index: one entry per sample")
    elif src != S:
        raise ValueError(f"without an index the rollout arrays must match {out_name}")
    return S // batch


def ppo_gauss_loss_fwd_bwd(mean, value, log_std, actions, old_logp, adv, ret, old_value, batch, clip_coef=0.2,
                           vf_coef=0.5, ent_coef=0.01, index=None, out=None, stats=None):
    """The Gaussian twin of ppo_loss_fwd_bwd (agx_ppo_gauss_loss_fwd_bwd): mean
    [nmb * batch, A], value [nmb * batch], log_std [nmb, A] (one minibatch per
    row of log_std); actions [rows, A] and old_logp / adv / ret / old_value
    [rows] are the rollout, gathered through ``index`` when given.
    Returns (g_mean, g_value, g_log_std, stats[nmb, 8])."""
    _need(mean, "mean", _f32)
    if mean.dim() != 2:
        raise ValueError("mean: expected [samples, A]")
    A = mean.shape[1]
    nmb = _head_loss_rows(mean, "mean", value, batch, actions, _f32, A, old_logp, adv, ret, old_value, index,
                                 None)
    _need(log_std, "log_std", _f32, (nmb, A))
    if out is None:
        out = (torch.empty_like(mean), torch.empty_like(value), torch.empty_like(log_std))
    if stats is None:
        stats = torch.empty(nmb, 8, dtype=_f32, device=mean.device)
    _lib.call("agx_ppo_gauss_loss_fwd_bwd", mean.data_ptr(), value.data_ptr(), log_std.data_ptr(),
              actions.data_ptr(), old_logp.data_ptr(), adv.data_ptr(), ret.data_ptr(), old_value.data_ptr(),
              _lib.ptr(index), int(batch), int(nmb), int(A), float(clip_coef), float(vf_coef), float(ent_coef),
              out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stats.data_ptr(), _lib.stream())
    return out[0], out[1], out[2], stats


def multi_head(nvec) -> _lib.AgxMultiHead:
    """agx_multi_head of a MultiDiscrete space's nvec (K >= 1 sizes >= 1, at
    most 32 logits in all)."""
    nvec = [int(n) for n in nvec]
    if not nvec or min(nvec) < 1 or sum(nvec) > 32:
        raise ValueError(f"nvec {nvec}: K >= 1 components of size >= 1 with at most 32 logits in all")
    h = _lib.AgxMultiHead()
    h.K = len(nvec)
    for k, n in enumerate(nvec):
        h.nvec[k] = n
    return h


def ppo_multi_loss_fwd_bwd(logits, value, nvec, actions, old_logp, adv, ret, old_value, batch, clip_coef=0.2,
                           vf_coef=0.5, ent_coef=0.01, index=None, mask=None, out=None, stats=None):
    """The multi-categorical twin of ppo_loss_fwd_bwd (agx_ppo_multi_loss_fwd_bwd):
    logits [nmb * batch, L] (raw, L = sum(nvec)), value [nmb * batch]; actions
    int64 [rows, K], mask uint8 [rows, L] (1 = legal) or None, and old_logp /
    adv / ret / old_value [rows] are the rollout, gathered through ``index``
    when given.  ``nvec``: the sizes, or a ready ``multi_head``.
    Returns (g_logits, g_value, stats[nmb, 8])."""
    head = nvec if isinstance(nvec, _lib.AgxMultiHead) else multi_head(nvec)
    K, L = head.K, sum(head.nvec[:head.K])
    _need(logits, "logits", _f32)
    if logits.dim() != 2 or logits.shape[1] != L:
        raise ValueError(f"logits: expected [samples, {L}]")
    nmb = _head_loss_rows(logits, "logits", value, batch, actions, _i64, K, old_logp, adv, ret, old_value,
                                 index, mask)
    if out is None:
        out = (torch.empty_like(logits), torch.empty_like(value))
    if stats is None:
        stats = torch.empty(nmb, 8, dtype=_f32, device=logits.device)
    _lib.call("agx_ppo_multi_loss_fwd_bwd", logits.data_ptr(), value.data_ptr(), head, actions.data_ptr(),
              _lib.ptr(mask), old_logp.data_ptr(), adv.data_ptr(), ret.data_ptr(), old_value.data_ptr(),
              _lib.ptr(index), int(batch), int(nmb), float(clip_coef), float(vf_coef), float(ent_coef),
              out[0].data_ptr(), out[1].data_ptr(), stats.data_ptr(), _lib.stream())
    return out[0], out[1], stats


def ppo_bern_loss_fwd_bwd(logits, value, actions, old_logp, adv, ret, old_value, batch, clip_coef=0.2, vf_coef=0.5,
                          ent_coef=0.01, index=None, mask=None, out=None, stats=None, n=None):
    """The Bernoulli twin of ppo_loss_fwd_bwd (agx_ppo_bern_loss_fwd_bwd):
    logits [nmb * batch, n] (raw), value [nmb * batch]; actions int64
    [rows, n] (anything but 0 counts as 1), mask uint8 [rows, n] (1 = legal) or
    None, and old_logp / adv / ret / old_value [rows] are the rollout, gathered
    through ``index`` when given.  ``n``: the bit count handed to the kernel
    (default: the logits' width; the kernel rejects anything outside 1..32).
    Returns (g_logits, g_value, stats[nmb, 8])."""
    _need(logits, "logits", _f32)
    if logits.dim() != 2:
        raise ValueError("logits: expected [samples, n]")
    n = logits.shape[1] if n is None else int(n)
    nmb = _head_loss_rows(logits, "logits", value, batch, actions, _i64, logits.shape[1], old_logp, adv, ret,
                                 old_value, index, mask)
    if out is None:
        out = (torch.empty_like(logits), torch.empty_like(value))
    if stats is None:
        stats = torch.empty(nmb, 8, dtype=_f32, device=logits.device)
    _lib.call("agx_ppo_bern_loss_fwd_bwd", logits.data_ptr(), value.data_ptr(), n, actions.data_ptr(),
              _lib.ptr(mask), old_logp.data_ptr(), adv.data_ptr(), ret.data_ptr(), old_value.data_ptr(),
              _lib.ptr(index), int(batch), int(nmb), float(clip_coef), float(vf_coef), float(ent_coef),
              out[0].data_ptr(), out[1].data_ptr(), stats.data_ptr(), _lib.stream())
    return out[0], out[1], stats


# --------------------------------------------------------------------------- #
# PER                                                                         #
# --------------------------------------------------------------------------- #
def per_workspace(capacity: int, device) -> torch.Tensor:
    return _ws(_lib.load().agx_per_workspace_bytes(capacity, 0), device)


def per_init(sum_tree, min_tree, capacity):
    _need(sum_tree, "sum_tree", _f64, (2 * capacity,))
    _need(min_tree, "min_tree", _f64, (2 * capacity,))
    _lib.call("agx_per_init", sum_tree.data_ptr(), min_tree.data_ptr(), capacity, _lib.stream())


def per_add(sum_tree, min_tree, capacity, max_size, start, n, alpha, max_priority, workspace=None):
    _need(max_priority, "max_priority", _f64, (1,))
    _lib.call("agx_per_add", sum_tree.data_ptr(), min_tree.data_ptr(), capacity, max_size, int(start),
              int(n), float(alpha), max_priority.data_ptr(), _lib.ptr(workspace), _lib.stream())


def per_update(sum_tree, min_tree, capacity, max_size, indices, priorities, alpha, max_priority,
               floor=1e-5, workspace=None):
    idx = indices.reshape(-1)
    pri = priorities.reshape(-1)
    _need(idx, "indices", _i64)
    _need(pri, "priorities", _f32)
    if idx.numel() != pri.numel():
        raise ValueError("indices / priorities length mismatch")
    _need(max_priority, "max_priority", _f64, (1,))
    if workspace is None and idx.numel() > 1024:
        workspace = per_workspace(capacity, idx.device)
    _lib.call("agx_per_update", sum_tree.data_ptr(), min_tree.data_ptr(), capacity, max_size,
              idx.data_ptr(), pri.data_ptr(), idx.numel(), float(alpha), float(floor),
              max_priority.data_ptr(), _lib.ptr(workspace), _lib.stream())


def per_sample(sum_tree, min_tree, capacity, uniforms, size=0, beta=0.4, weights=True, err=None):
    u = uniforms.reshape(-1)
    _need(u, "uniforms", _f32)
    B = u.numel()
    idx = torch.empty(B, dtype=_i64, device=u.device)
    w = torch.empty(B, dtype=_f32, device=u.device) if weights else None
    if err is not None:
        _need(err, "err", _i32, (1,))
    _lib.call("agx_per_sample", sum_tree.data_ptr(), _lib.ptr(min_tree), capacity, u.data_ptr(), B,
              int(size), float(beta), idx.data_ptr(), _lib.ptr(w), _lib.ptr(err), _lib.stream())
    return idx, w


def per_gather(tree, nodes):
    _need(nodes, "nodes", _i64)
    out = torch.empty(nodes.numel(), dtype=_f64, device=tree.device)
    _lib.call("agx_per_gather", tree.data_ptr(), nodes.data_ptr(), nodes.numel(), out.data_ptr(),
              _lib.stream())
    return out


def debug_pow(x, y):
    _need(x, "x", _f64)
    _need(y, "y", _f64, tuple(x.shape))
    out = torch.empty_like(x)
    _lib.call("agx_debug_pow", x.data_ptr(), y.data_ptr(), out.data_ptr(), x.numel(), _lib.stream())
    return out


# --------------------------------------------------------------------------- #
# DQN / Rainbow                                                               #
# --------------------------------------------------------------------------- #
def td_target(q_next_target, rewards, dones, gamma, q_next_online=None, double=False, q_cur=None,
              actions=None, with_loss=True):
    B, A = q_next_target.shape
    _need(q_next_target, "q_next_target", _f32)
    r = rewards.reshape(-1)
    d = dones.reshape(-1)
    _need(r, "rewards", _f32, (B,))
    _need(d, "dones", _f32, (B,))
    if double:
        _need(q_next_online, "q_next_online", _f32, (B, A))
    y = torch.empty(B, 1, dtype=_f32, device=r.device)
    g_q = loss = None
    if with_loss:
        _need(q_cur, "q_cur", _f32, (B, A))
        a = actions.reshape(-1)
        _need(a, "actions", _i64, (B,))
        g_q = torch.empty(B, A, dtype=_f32, device=r.device)
        loss = torch.empty(1, dtype=_f32, device=r.device)
    else:
        a = None
    ws = _ws(_lib.load().agx_td_workspace_bytes(B), r.device) if with_loss else None
    _lib.call("agx_td_target", _lib.ptr(q_next_online), q_next_target.data_ptr(), _lib.ptr(q_cur),
              _lib.ptr(a), r.data_ptr(), d.data_ptr(), B, A, float(gamma), int(bool(double)),
              y.data_ptr(), _lib.ptr(g_q), _lib.ptr(loss), _lib.ptr(ws), _lib.stream())
    return y, g_q, loss


def cqn_loss(q_cur, q_next_target, actions, rewards, dones, gamma, q_next_online=None, double=False,
             with_terms=False):
    """-> (y (B,1), dloss/dq_cur (B,A), loss (1,)[, terms (3,)]) of CQN.learn's
    loss (cqn.py:234-252): DQN's TD target and half its MSE plus
    mean(logsumexp_a Q) - mean(Q), with the dense gradient, in one launch
    (+ the fixed-order sums).  terms = (mean lse, mean Q, MSE).  y is
    td_target's, bit for bit.  Precondition: 0 <= actions < A."""
    _need(q_cur, "q_cur", _f32)
    if q_cur.dim() != 2:
        raise ValueError(f"q_cur: expected [B, A], got {tuple(q_cur.shape)}")
    B, A = q_cur.shape
    _need(q_next_target, "q_next_target", _f32, (B, A))
    a, r, d = actions.reshape(-1), rewards.reshape(-1), dones.reshape(-1)
    _need(a, "actions", _i64, (B,))
    _need(r, "rewards", _f32, (B,))
    _need(d, "dones", _f32, (B,))
    if double:
        _need(q_next_online, "q_next_online", _f32, (B, A))
    dev = q_cur.device
    y = torch.empty(B, 1, dtype=_f32, device=dev)
    g_q = torch.empty(B, A, dtype=_f32, device=dev)
    loss = torch.empty(1, dtype=_f32, device=dev)
    terms = torch.empty(3, dtype=_f32, device=dev) if with_terms else None
    if B == 0:  # no launch: the means of nothing, as torch's mean of an empty tensor
        loss.fill_(float("nan"))
        if terms is not None:
            terms.fill_(float("nan"))
        return (y, g_q, loss, terms) if with_terms else (y, g_q, loss)
    ws = _ws(_lib.load().agx_cqn_workspace_bytes(B, A), dev)
    _lib.call("agx_cqn_loss", _lib.ptr(q_next_online) if double else None, q_next_target.data_ptr(),
              q_cur.data_ptr(), a.data_ptr(), r.data_ptr(), d.data_ptr(), B, A, float(gamma), int(bool(double)),
              y.data_ptr(), g_q.data_ptr(), loss.data_ptr(), _lib.ptr(terms), ws.data_ptr(), _lib.stream())
    return (y, g_q, loss, terms) if with_terms else (y, g_q, loss)


def _critic_target(maddpg, q1, qn1, rewards, dones, gamma, q2=None, qn2=None):
    """Shape checks, outputs and the launch of agx_maddpg_critic_target
    (``maddpg``, one critic), agx_matd3_critic_target (``maddpg``, two) or
    agx_td3_critic_target -> (y, dloss/dq1, dloss/dq2 | None, loss)."""
    B = q1.shape[0]
    f1, fn1, r, d = q1.reshape(-1), qn1.reshape(-1), rewards.reshape(-1), dones.reshape(-1)
    f2, fn2 = (q2.reshape(-1), qn2.reshape(-1)) if q2 is not None else (None, None)
    one = maddpg and q2 is None
    named = [(f1, "q" if one else "q1"), (fn1, "q_next" if one else "qn1"), (r, "rewards"), (d, "dones")]
    for t, name in named + ([(f2, "q2"), (fn2, "qn2")] if q2 is not None else []):
        _need(t, name, _f32, (B,))
    dev = r.device
    y, g1 = torch.empty(B, 1, dtype=_f32, device=dev), torch.empty(B, 1, dtype=_f32, device=dev)
    g2 = torch.empty(B, 1, dtype=_f32, device=dev) if q2 is not None else None
    loss = torch.empty(1, dtype=_f32, device=dev)
    if one:
        ws = _ws(_lib.load().agx_td_workspace_bytes(B), dev)
        _lib.call("agx_maddpg_critic_target", f1.data_ptr(), fn1.data_ptr(), r.data_ptr(), d.data_ptr(), B,
                  float(gamma), y.data_ptr(), g1.data_ptr(), loss.data_ptr(), ws.data_ptr(), _lib.stream())
    else:
        ws = _ws(_lib.load().agx_td3_workspace_bytes(B), dev)
        _lib.call("agx_matd3_critic_target" if maddpg else "agx_td3_critic_target", f1.data_ptr(), _lib.ptr(f2),
                  fn1.data_ptr(), _lib.ptr(fn2), r.data_ptr(), d.data_ptr(), B, float(gamma), y.data_ptr(),
                  g1.data_ptr(), _lib.ptr(g2), loss.data_ptr(), ws.data_ptr(), _lib.stream())
    return y, g1, g2, loss


def maddpg_critic_target(q, q_next, rewards, dones, gamma):
    """-> (y (B,1), dloss/dq (B,1), loss (1,)) of MADDPG._learn_individual's
    critic step (maddpg.py:764-790) in one launch (+ the fixed-order loss sum)."""
    y, g_q, _, loss = _critic_target(True, q, q_next, rewards, dones, gamma)
    return y, g_q, loss


def matd3_critic_target(q1, q2, qn1, qn2, rewards, dones, gamma):
    """-> (y (B,1), dloss/dq1 (B,1), dloss/dq2 (B,1), loss (1,)) of
    MATD3.learn_individual's critic step (matd3.py:861-880): MADDPG's NaN and
    uint8 rules for r and d, y from the smaller target critic, the sum of the
    two MSE losses, in one launch (+ the fixed-order loss sums)."""
    return _critic_target(True, q1, qn1, rewards, dones, gamma, q2, qn2)


def td3_smooth_actions(mu, noise, low, high, noise_clip, out=None):
    """Target-policy smoothing (td3.py:493-501, ddpg.py:448-456) in one
    launch: max(min(mu + clamp(noise, -c, c), high), low) with per-dimension
    bounds [A].  -> out [B, A] (``out`` may be ``mu`` itself)."""
    _need(mu, "mu", _f32)
    if mu.dim() != 2:
        raise ValueError(f"mu: expected [B, A], got {tuple(mu.shape)}")
    B, A = mu.shape
    _need(noise, "noise", _f32, (B, A))
    _need(low, "low", _f32, (A,))
    _need(high, "high", _f32, (A,))
    if out is None:
        out = torch.empty_like(mu)
    _need(out, "out", _f32, (B, A))
    _lib.call("agx_td3_smooth_actions", mu.data_ptr(), noise.data_ptr(), low.data_ptr(), high.data_ptr(), B, A,
              float(noise_clip), out.data_ptr(), _lib.stream())
    return out


def td3_critic_target(q1, qn1, rewards, dones, gamma, q2=None, qn2=None):
    """-> (y (B,1), dloss/dq1 (B,1), dloss/dq2 (B,1) | None, loss (1,)) of
    TD3.learn's critic step (td3.py:503-515: y from the smaller target
    critic, the sum of the two MSE losses), or DDPG's with one critic
    (ddpg.py:457-461), in one launch (+ the fixed-order loss sums)."""
    if (q2 is None) != (qn2 is None):
        raise ValueError("q2 and qn2 go together (both None: the single-critic form)")
    return _critic_target(False, q1, qn1, rewards, dones, gamma, q2, qn2)


def c51_project_loss(q_next_online, target_dist, logp_cur, actions, rewards, dones, support, v_min,
                     v_max, gamma, with_proj=False):
    B, A, Z = target_dist.shape
    _need(q_next_online, "q_next_online", _f32, (B, A))
    _need(target_dist, "target_dist", _f32)
    _need(logp_cur, "logp_cur", _f32, (B, A, Z))
    a = actions.reshape(-1)
    _need(a, "actions", _i64, (B,))
    r = rewards.reshape(-1)
    d = dones.reshape(-1)
    _need(r, "rewards", _f32, (B,))
    _need(d, "dones", _f32, (B,))
    _need(support, "support", _f32, (Z,))
    loss = torch.empty(B, dtype=_f32, device=r.device)
    proj = torch.empty(B, Z, dtype=_f32, device=r.device) if with_proj else None
    _lib.call("agx_c51_project_loss", q_next_online.data_ptr(), target_dist.data_ptr(),
              logp_cur.data_ptr(), a.data_ptr(), r.data_ptr(), d.data_ptr(), support.data_ptr(), B, A,
              Z, float(v_min), float(v_max), float(gamma), loss.data_ptr(), _lib.ptr(proj),
              _lib.stream())
    return (loss, proj) if with_proj else loss


def c51_project_loss_rows(target_rows, logp_rows, rewards, dones, support, v_min, v_max, gamma, with_proj=False):
    """agx_c51_project_loss_rows: the projection + loss on the selected rows
    ([B][Z] target distribution of a*, [B][Z] log p of the taken action)."""
    B, Z = target_rows.shape
    _need(target_rows, "target_rows", _f32, (B, Z))
    _need(logp_rows, "logp_rows", _f32, (B, Z))
    r = rewards.reshape(-1)
    d = dones.reshape(-1)
    _need(r, "rewards", _f32, (B,))
    _need(d, "dones", _f32, (B,))
    _need(support, "support", _f32, (Z,))
    loss = torch.empty(B, dtype=_f32, device=r.device)
    proj = torch.empty(B, Z, dtype=_f32, device=r.device) if with_proj else None
    _lib.call("agx_c51_project_loss_rows", target_rows.data_ptr(), logp_rows.data_ptr(), r.data_ptr(), d.data_ptr(),
              support.data_ptr(), B, Z, float(v_min), float(v_max), float(gamma), loss.data_ptr(), _lib.ptr(proj),
              _lib.stream())
    return (loss, proj) if with_proj else loss


# --------------------------------------------------------------------------- #
# optimiser                                                                   #
# --------------------------------------------------------------------------- #
class ClipAdam:
    """Fused per-agent grad-norm clip + Adam over flat [P, n] buffers, with a
    per-agent Adam step count on the device (``steps``, int64 [P])."""

    def __init__(self, params: torch.Tensor, group_offsets, lr, betas=(0.9, 0.999), eps=1e-8,
                 max_norm=0.5, grads: torch.Tensor | None = None):
        _need(params, "params", _f32)
        if params.dim() != 2:
            raise ValueError("params must be [P, n]")
        self.params = params
        P, n = params.shape
        self.grads = torch.zeros_like(params) if grads is None else grads
        _need(self.grads, "grads", _f32, tuple(params.shape))
        self.exp_avg = torch.zeros_like(params)
        self.exp_avg_sq = torch.zeros_like(params)
        self.steps = torch.zeros(P, dtype=torch.int64, device=params.device)
        self.offsets = (torch.tensor(list(group_offsets), dtype=torch.int64)).contiguous()
        if int(self.offsets[0]) != 0 or int(self.offsets[-1]) != n:
            raise ValueError("group offsets must span [0, n)")
        lr_t = torch.as_tensor(lr, dtype=_f32).reshape(-1)
        self.lr = (lr_t.expand(P) if lr_t.numel() == 1 else lr_t).to(params.device).contiguous()
        self.betas, self.eps, self.max_norm = betas, eps, max_norm
        self.workspace = _ws(_lib.load().agx_adam_workspace_bytes(P, n), params.device)

    def step(self, active: torch.Tensor | None = None):
        """One clip + Adam update of every agent (or of the agents whose
        ``active`` u8 flag is set; the others are untouched)."""
        P, n = self.params.shape
        _lib.call("agx_clip_adam", self.params.data_ptr(), self.grads.data_ptr(),
                  self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), P, n,
                  self.offsets.data_ptr(), len(self.offsets) - 1, float(self.max_norm),
                  self.lr.data_ptr(), float(self.betas[0]), float(self.betas[1]), float(self.eps),
                  self.steps.data_ptr(), _lib.ptr(active), self.workspace.data_ptr(), _lib.stream())


class _NoisyLayer(ctypes.Structure):
    _fields_ = [("eps_in", ctypes.c_void_p), ("eps_out", ctypes.c_void_p), ("weight_epsilon", ctypes.c_void_p),
                ("bias_epsilon", ctypes.c_void_p), ("in_features", ctypes.c_int64), ("out_features", ctypes.c_int64)]


def noisy_reset_(layers: list) -> None:
    """agx_noisy_reset: ``layers`` = [(eps_in, eps_out, weight_epsilon,
    bias_epsilon)] — each layer's two N(0, 1) draws and its epsilon buffers
    (NoisyLinear.reset_noise, custom_components.py:116-131), one launch."""
    arr = (_NoisyLayer * max(1, len(layers)))()
    for k, (ei, eo, we, be) in enumerate(layers):
        n_in, n_out = ei.numel(), eo.numel()
        _need(ei, "eps_in", _f32)
        _need(eo, "eps_out", _f32)
        _need(we, "weight_epsilon", _f32, (n_out, n_in))
        _need(be, "bias_epsilon", _f32, (n_out,))
        arr[k] = _NoisyLayer(ei.data_ptr(), eo.data_ptr(), we.data_ptr(), be.data_ptr(), n_in, n_out)
    _lib.call("agx_noisy_reset", ctypes.cast(arr, ctypes.c_void_p), len(layers), _lib.stream())


def polyak_(target: torch.Tensor, online: torch.Tensor, tau: float) -> None:
    _need(target, "target", _f32)
    _need(online, "online", _f32, tuple(target.shape))
    _lib.call("agx_polyak", target.data_ptr(), online.data_ptr(), target.numel(), float(tau),
              _lib.stream())


class _PolyakSegment(ctypes.Structure):
    _fields_ = [("target", ctypes.c_void_p), ("online", ctypes.c_void_p), ("n", ctypes.c_int64)]


POLYAK_MAX_SEGMENTS = 64  # AGX_POLYAK_MAX_SEGMENTS (include/agx.h)


def polyak_segments_(targets, onlines, tau: float) -> None:
    """agx_polyak_segments: target <- tau * online + (1 - tau) * target for
    every (target, online) pair of contiguous f32 tensors, one launch per 64
    pairs.  The pairs must not overlap one another."""
    if len(targets) != len(onlines):
        raise ValueError(f"polyak_segments_: {len(targets)} targets for {len(onlines)} online tensors")
    for t, o in zip(targets, onlines):
        _need(t, "target", _f32)
        _need(o, "online", _f32, tuple(t.shape))
    for k in range(0, len(targets), POLYAK_MAX_SEGMENTS):
        chunk = list(zip(targets[k:k + POLYAK_MAX_SEGMENTS], onlines[k:k + POLYAK_MAX_SEGMENTS]))
        arr = (_PolyakSegment * len(chunk))()
        for j, (t, o) in enumerate(chunk):
            arr[j] = _PolyakSegment(t.data_ptr(), o.data_ptr(), t.numel())
        _lib.call("agx_polyak_segments", ctypes.cast(arr, ctypes.c_void_p), len(chunk), float(tau), _lib.stream())


# --------------------------------------------------------------------------- #
# IPPO (include/agx_ippo.h)                                                    #
# --------------------------------------------------------------------------- #
class IppoGaeSegment(ctypes.Structure):
    """Mirror of ``agx_ippo_gae_segment`` (include/agx_ippo.h)."""

    _fields_ = [(n, ctypes.c_void_p) for n in ("rewards", "dones", "values", "next_value", "next_done",
                                                "advantages", "returns")] + [("M", ctypes.c_int64)]


IPPO_MAX_SEGMENTS = 8  # AGX_IPPO_MAX_SEGMENTS


def ippo_gae_table(segments):
    """(table, T) of ``ippo_gae``'s launch for ``segments``: tuples (rewards,
    dones, values [T, M], next_value, next_done [M], advantages, returns
    [T, M]) of contiguous f32 device tensors, one per agent group.  The table
    holds raw pointers: the caller keeps the tensors alive while it is used."""
    if not 1 <= len(segments) <= IPPO_MAX_SEGMENTS:
        raise ValueError(f"ippo_gae: 1..{IPPO_MAX_SEGMENTS} segments per launch (got {len(segments)})")
    T = int(segments[0][0].shape[0])
    arr = (IppoGaeSegment * len(segments))()
    for k, (r, d, v, nv, nd, adv, ret) in enumerate(segments):
        if r.dim() != 2 or r.shape[0] != T:
            raise ValueError(f"ippo_gae: segment {k}: rewards {tuple(r.shape)}, expected [{T}, M]")
        M = int(r.shape[1])
        for t, name in ((r, "rewards"), (d, "dones"), (v, "values"), (adv, "advantages"), (ret, "returns")):
            _need(t, name, _f32, (T, M))
        _need(nv, "next_value", _f32, (M,))
        _need(nd, "next_done", _f32, (M,))
        arr[k] = IppoGaeSegment(*(t.data_ptr() if M else None for t in (r, d, v, nv, nd, adv, ret)), M)
    return arr, T


def ippo_gae(segments, gamma: float, gae_lambda: float) -> None:
    """agx_ippo_gae: the float32 GAE of ippo.py:702-725 for every agent group
    of ``segments`` (``ippo_gae_table``) in one launch; advantages and returns
    are written in place, bit for bit the reference's torch loop."""
    arr, T = ippo_gae_table(segments)
    _lib.call("agx_ippo_gae", ctypes.cast(arr, ctypes.c_void_p), len(segments), T, float(gamma), float(gae_lambda),
              _lib.stream())


# --------------------------------------------------------------------------- #
# Neural contextual bandits (include/agx_bandit.h)                             #
# --------------------------------------------------------------------------- #
BANDIT_RESIDENT_MAX_D = 112  # AGX_BANDIT_RESIDENT_MAX_D
BANDIT_MAX_D = 1025          # AGX_BANDIT_MAX_D
BANDIT_MAX_ARMS = 1024       # AGX_BANDIT_MAX_ARMS


def bandit_normals(A: int, seed: int, counter: int):
    """float32 [A]: the Thompson draws of one agx_bandit_select call on the
    host — words (x, y) of the Philox4x32-10 block of (arm, 0, counter) under
    key ``seed``, Box-Muller (agx_bandit.h).  The device evaluates log / sqrt /
    cospi in float32; these are float64 values rounded once."""
    import numpy as np

    m32 = np.uint64(0xFFFFFFFF)
    c = [np.arange(A, dtype=np.uint64), np.zeros(A, np.uint64), np.full(A, counter & 0xFFFFFFFF, np.uint64),
         np.full(A, (counter >> 32) & 0xFFFFFFFF, np.uint64)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    u = [((w >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24) for w in c[:2]]
    return (np.sqrt(-2.0 * np.log(u[0].astype(np.float64))) * np.cos(2.0 * np.pi * u[1].astype(np.float64))
            ).astype(np.float32)


@torch.no_grad()
def bandit_select_torch(h, mu, sigma_inv, mask=None, *, bias_one=True, scale=1.0, gamma=1.0, thompson=False,
                        seed=0, counter=None):
    """agx_bandit_select's arithmetic in torch ops on the tensors' device
    (f64 sums rounded to f32 once, the rank-1 form of the update): what the
    agents run on the CPU, and what ``bandit_select`` runs for shapes past the
    kernel's range.  Same arguments and results; ``sigma_inv`` and ``counter``
    are updated in place."""
    A = h.shape[0]
    g = h.to(_f32) * scale
    if bias_one:
        g = torch.cat([g, torch.full((A, 1), float(scale), dtype=_f32, device=g.device)], dim=1)
    g64, S = g.to(_f64), sigma_inv.to(_f64)
    quad = ((g64 @ S) * g64).sum(dim=1)
    width = gamma * torch.sqrt(quad)
    if thompson:
        z = torch.from_numpy(bandit_normals(A, int(seed), int(counter.item()))).to(width.device)
        width = width * z.to(_f64)
        counter += 1
    scores, quad = (mu.to(_f64) + width).to(_f32), quad.to(_f32)
    eff = scores if mask is None else torch.where(mask.reshape(-1).to(scores.device) == 1, scores,
                                                  torch.full_like(scores, -float("inf")))
    nan = torch.isnan(eff)  # np.argmax: the first NaN wins, else the first maximum
    action = torch.where(nan.any(), nan.to(torch.int8).argmax(), torch.nan_to_num(eff, nan=-float("inf")).argmax())
    v = g64.index_select(0, action.reshape(1))[0]
    u, w = S @ v, S.t() @ v
    r = 1.0 / (1.0 + torch.dot(v, u))
    sigma_inv.copy_((S - torch.outer(u * r, w)).to(_f32))
    return action.reshape(1).to(_i64), scores, quad


def bandit_select(h, mu, sigma_inv, mask=None, *, bias_one=True, scale=1.0, gamma=1.0, thompson=False, seed=0,
                  counter=None):
    """-> (action int64 (1,), scores (A,), quad (A,)) of one NeuralUCB /
    NeuralTS step (neural_ucb_bandit.py:237-257): quad_k = g_k sigma_inv
    g_k^T with g_k = scale [h_k, 1] (``bias_one``) or scale h_k, score_k =
    mu_k + gamma sqrt(quad_k) [* z_k], numpy's masked argmax, and the
    Sherman-Morrison update of ``sigma_inv`` in place — one launch for D =
    H + bias_one <= BANDIT_RESIDENT_MAX_D, four above (agx_bandit.h).  ``h``
    [A, H] may have a row stride >= H; ``mask`` uint8 / bool [A], 1 = legal;
    ``counter`` int64 (1,) on the device, advanced by one (required when
    ``thompson``).  Nothing is read back.  Past the kernel's range (A >
    BANDIT_MAX_ARMS or D > BANDIT_MAX_D) the same arithmetic runs as torch ops."""
    _need(h, "h", _f32, contiguous=False)
    if h.dim() != 2:
        raise ValueError(f"h: expected [A, H], got {tuple(h.shape)}")
    A, H = h.shape
    D = H + int(bool(bias_one))
    if A < 1 or D < 1:
        raise ValueError(f"bandit_select: need A >= 1 and D >= 1, got A = {A}, D = {D}")
    ldh = H if A == 1 or H == 0 else h.stride(0)
    if H > 0 and (h.stride(1) != 1 or ldh < H):
        raise ValueError("h: rows must be contiguous and must not overlap")
    _need(mu, "mu", _f32, (A,))
    _need(sigma_inv, "sigma_inv", _f32, (D, D))
    if mask is not None:
        mask = mask.reshape(-1)
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        _need(mask, "mask", _u8, (A,))
    if thompson or counter is not None:
        _need(counter, "counter", _i64, (1,))
    if A > BANDIT_MAX_ARMS or D > BANDIT_MAX_D:
        return bandit_select_torch(h, mu, sigma_inv, mask, bias_one=bias_one, scale=scale, gamma=gamma,
                                   thompson=thompson, seed=seed, counter=counter)
    dev = mu.device
    action = torch.empty(1, dtype=_i64, device=dev)
    scores = torch.empty(A, dtype=_f32, device=dev)
    quad = torch.empty(A, dtype=_f32, device=dev)
    ws = _ws(_lib.load().agx_bandit_workspace_bytes(A, D), dev)
    _lib.call("agx_bandit_select", h.data_ptr() if H else None, ldh, mu.data_ptr(), sigma_inv.data_ptr(),
              _lib.ptr(mask), A, H, int(bool(bias_one)), float(scale), float(gamma), int(bool(thompson)),
              int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(counter), scores.data_ptr(), quad.data_ptr(),
              action.data_ptr(), ws.data_ptr(), _lib.stream())
    return action, scores, quad
