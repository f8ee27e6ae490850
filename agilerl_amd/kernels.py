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


# --------------------------------------------------------------------------- #
# Truncated BPTT for recurrent PPO (include/agx_bptt.h)                         #
# --------------------------------------------------------------------------- #
BPTT_TYPES = {"chunked": 0, "maximum": 1, "fifty_percent_overlap": 2}  # BPTTSequenceType values -> AGX_BPTT_*
BPTT_MAX_HIDDEN_KEYS = 4  # AGX_BPTT_MAX_HIDDEN_KEYS


def _ptr_fields(*names):
    return [(n, ctypes.c_void_p) for n in names]


class BpttGatherArgs(ctypes.Structure):
    """Mirror of ``agx_bptt_gather_args`` (include/agx_bptt.h)."""

    _fields_ = (_ptr_fields("seq", "ids", "local_off") +
                [(n, ctypes.c_int64) for n in ("S", "Bs", "L", "T", "N", "D", "A", "M", "n_valid")] +
                _ptr_fields("obs", "actions", "mask", "log_probs", "advantages", "returns", "values") +
                [("hidden", ctypes.c_void_p * BPTT_MAX_HIDDEN_KEYS), ("layers", ctypes.c_int32 * BPTT_MAX_HIDDEN_KEYS),
                 ("H", ctypes.c_int32 * BPTT_MAX_HIDDEN_KEYS), ("n_hidden", ctypes.c_int32),
                 ("pad_", ctypes.c_int32)] +
                _ptr_fields("obs_out", "act_out", "mask_out", "pad_mask") +
                [("hidden_out", ctypes.c_void_p * BPTT_MAX_HIDDEN_KEYS)] +
                _ptr_fields("old_logp", "adv", "ret", "old_value", "valid_row"))


def bptt_sequence_type(sequence_type) -> int:
    """AGX_BPTT_* of a BPTTSequenceType member, its value or its name (None: CHUNKED, the reference's default)."""
    if sequence_type is None:
        return 0
    key = getattr(sequence_type, "value", sequence_type)
    if isinstance(key, str) and key.lower() in BPTT_TYPES:
        return BPTT_TYPES[key.lower()]
    if isinstance(key, int) and not isinstance(key, bool) and key in BPTT_TYPES.values():
        return key
    raise NotImplementedError(f"Received unrecognized sequence type: {sequence_type}")


def bptt_plan(dones, max_seq_len=None, sequence_type=None):
    """agx_bptt_plan on ``dones`` uint8 / bool [T, N] -> (seq int32 [T * N, 3] = (env, first step, length),
    row_offset int32 [T * N + 1], meta int32 [4] = S, L, rows, 0); the first S table rows are written.  Nothing
    is read back."""
    if dones.dtype == torch.bool:
        dones = dones.view(torch.uint8)
    _need(dones, "dones", _u8)
    if dones.dim() != 2 or dones.numel() == 0:
        raise ValueError(f"dones: expected a non-empty [T, N], got {tuple(dones.shape)}")
    T, N = dones.shape
    dev = dones.device
    cap = _lib.load().agx_bptt_capacity(T, N)
    seq = torch.empty(cap, 3, dtype=_i32, device=dev)
    row_offset = torch.empty(cap + 1, dtype=_i32, device=dev)
    meta = torch.empty(4, dtype=_i32, device=dev)
    ws = _ws(_lib.load().agx_bptt_plan_workspace_bytes(N), dev)
    _lib.call("agx_bptt_plan", dones.data_ptr(), T, N, int(max_seq_len or 0), bptt_sequence_type(sequence_type),
              seq.data_ptr(), row_offset.data_ptr(), meta.data_ptr(), ws.data_ptr(), _lib.stream())
    return seq, row_offset, meta


def bptt_gather(seq, S, ids, local_off, n_valid, L, obs, actions, log_probs, advantages, returns, values, mask=None,
                hidden=None):
    """agx_bptt_gather: the minibatch of sequences ``ids`` (int64 [Bs], rows of the table ``seq`` with S entries)
    padded to L steps.  ``local_off`` int32 [Bs]: the exclusive prefix of the sequences' lengths, ``n_valid``
    their sum.  obs [T, N, D] / actions [T, N, A] f32, mask uint8 / bool [T, N, M] or None, log_probs /
    advantages / returns / values [T, N] f32, hidden: {key: [T, N, layers, H]} or None.  -> dict with
    observations [Bs * L, D], actions [Bs * L, A], action_masks bool [Bs * L, M] (with a mask), pad_mask bool
    [Bs * L], initial_hidden_states {key: [layers, Bs, H]}, and log_probs / advantages / returns / values
    [n_valid] with valid_row int64 [n_valid]."""
    _need(seq, "seq", _i32)
    _need(ids, "ids", _i64)
    Bs = ids.numel()
    _need(local_off, "local_off", _i32, (Bs,))
    _need(obs, "obs", _f32)
    _need(actions, "actions", _f32)
    if obs.dim() != 3 or actions.dim() != 3 or actions.shape[:2] != obs.shape[:2]:
        raise ValueError("obs [T, N, D] and actions [T, N, A] must share T and N")
    T, N, D = obs.shape
    A = actions.shape[2]
    S, L, n_valid = int(S), int(L), int(n_valid)
    if not (0 < S <= seq.shape[0] and seq.dim() == 2 and seq.shape[1] == 3):
        raise ValueError(f"seq: expected [>= {S}, 3], got {tuple(seq.shape)}")
    if not (Bs >= 1 and 1 <= L <= T and 0 <= n_valid <= Bs * L):
        raise ValueError(f"bptt_gather: Bs = {Bs}, L = {L} (T = {T}), n_valid = {n_valid}")
    for t, n in ((log_probs, "log_probs"), (advantages, "advantages"), (returns, "returns"), (values, "values")):
        _need(t, n, _f32, (T, N))
    dev = obs.device
    a = BpttGatherArgs()
    a.seq, a.ids, a.local_off = seq.data_ptr(), ids.data_ptr(), local_off.data_ptr()
    a.S, a.Bs, a.L, a.T, a.N, a.D, a.A, a.M, a.n_valid = S, Bs, L, T, N, D, A, 0, n_valid
    a.obs, a.actions = obs.data_ptr(), actions.data_ptr()
    a.log_probs, a.advantages = log_probs.data_ptr(), advantages.data_ptr()
    a.returns, a.values = returns.data_ptr(), values.data_ptr()
    out = {"observations": torch.empty(Bs * L, D, dtype=_f32, device=dev),
           "actions": torch.empty(Bs * L, A, dtype=_f32, device=dev),
           "pad_mask": torch.empty(Bs * L, dtype=torch.bool, device=dev)}
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        _need(mask, "mask", _u8)
        if mask.dim() != 3 or mask.shape[:2] != (T, N):
            raise ValueError(f"mask: expected [{T}, {N}, M], got {tuple(mask.shape)}")
        a.M, a.mask = mask.shape[2], mask.data_ptr()
        out["action_masks"] = torch.empty(Bs * L, a.M, dtype=torch.bool, device=dev)
        a.mask_out = out["action_masks"].data_ptr()
    hidden = hidden or {}
    if len(hidden) > BPTT_MAX_HIDDEN_KEYS:
        raise ValueError(f"bptt_gather: at most {BPTT_MAX_HIDDEN_KEYS} hidden-state keys (got {len(hidden)})")
    out["initial_hidden_states"] = {}
    for q, (key, h) in enumerate(hidden.items()):
        _need(h, f"hidden[{key}]", _f32)
        if h.dim() != 4 or h.shape[:2] != (T, N):
            raise ValueError(f"hidden[{key}]: expected [{T}, {N}, layers, H], got {tuple(h.shape)}")
        o = out["initial_hidden_states"][key] = torch.empty(h.shape[2], Bs, h.shape[3], dtype=_f32, device=dev)
        a.hidden[q], a.layers[q], a.H[q], a.hidden_out[q] = h.data_ptr(), h.shape[2], h.shape[3], o.data_ptr()
    a.n_hidden = len(hidden)
    for k in ("log_probs", "advantages", "returns", "values"):
        out[k] = torch.empty(n_valid, dtype=_f32, device=dev)
    out["valid_row"] = torch.empty(n_valid, dtype=_i64, device=dev)
    a.obs_out, a.act_out, a.pad_mask = out["observations"].data_ptr(), out["actions"].data_ptr(), \
        out["pad_mask"].data_ptr()
    a.old_logp, a.adv, a.ret, a.old_value = (out[k].data_ptr() for k in ("log_probs", "advantages", "returns",
                                                                           "values"))
    a.valid_row = out["valid_row"].data_ptr()
    _lib.call("agx_bptt_gather", ctypes.byref(a), _lib.stream())
    return out


def ppo_seq_loss_fwd_bwd(logp, value, entropy, valid_row, old_logp, adv, ret, old_value, clip_coef=0.2, vf_coef=0.5,
                         ent_coef=0.01):
    """agx_ppo_seq_loss_fwd_bwd: logp / value / entropy f32 [rows] over every padded row; valid_row int64
    [n_valid], strictly ascending, and old_logp / adv / ret / old_value f32 [n_valid] of those rows.
    -> (g_logp, g_value, g_entropy [rows], zero on pad rows; stats f32 [8])."""
    rows = logp.numel()
    for t, n in ((logp, "logp"), (value, "value"), (entropy, "entropy")):
        _need(t, n, _f32)
        if t.numel() != rows:
            raise ValueError(f"{n}: expected {rows} elements")
    _need(valid_row, "valid_row", _i64)
    n_valid = valid_row.numel()
    if not 1 <= n_valid <= rows:
        raise ValueError(f"valid_row: {n_valid} valid rows of {rows}")
    for t, n in ((old_logp, "old_logp"), (adv, "adv"), (ret, "ret"), (old_value, "old_value")):
        _need(t, n, _f32)
        if t.numel() != n_valid:
            raise ValueError(f"{n}: expected {n_valid} elements")
    out = tuple(torch.empty_like(logp) for _ in range(3))
    stats = torch.empty(8, dtype=_f32, device=logp.device)
    ws = _ws(_lib.load().agx_ppo_seq_loss_workspace_bytes(rows), logp.device)
    _lib.call("agx_ppo_seq_loss_fwd_bwd", logp.data_ptr(), value.data_ptr(), entropy.data_ptr(), rows,
              valid_row.data_ptr(), n_valid, old_logp.data_ptr(), adv.data_ptr(), ret.data_ptr(),
              old_value.data_ptr(), float(clip_coef), float(vf_coef), float(ent_coef), out[0].data_ptr(),
              out[1].data_ptr(), out[2].data_ptr(), stats.data_ptr(), ws.data_ptr(), _lib.stream())
    return out[0], out[1], out[2], stats


# --------------------------------------------------------------------------- #
# The fused recurrent policy step (include/agx_recurrent.h)                     #
# --------------------------------------------------------------------------- #
from .modules import lstm as _lstm  # noqa: E402  (the LSTM descriptor and its rules; imports nothing from here)

RECURRENT_MAX_HEAD, RECURRENT_MAX_WIDTH, RECURRENT_MAX_ACTIONS = 4, 512, 32  # AGX_RECURRENT_MAX_HEAD, AGX_PPO_GRAPH_MAX_*
_i32s = lambda *names: [(n, ctypes.c_int32) for n in names]  # noqa: E731


class RecurrentLinear(ctypes.Structure):
    """Mirror of ``agx_recurrent_linear``."""

    _fields_ = _ptr_fields("w", "b", "ln_w", "ln_b") + _i32s("in_", "out", "relu", "pad_")


class RecurrentNet(ctypes.Structure):
    """Mirror of ``agx_recurrent_net``."""

    _fields_ = ([("lstm", _lstm.AgxLstmDesc)] + _ptr_fields("out_w", "out_b") + _i32s("latent", "out_act") +
                [("head", RecurrentLinear * RECURRENT_MAX_HEAD)] + _i32s("n_head", "pad_") +
                _ptr_fields("h", "c", "h_next", "c_next", "h_store", "c_store"))


class RecurrentStep(ctypes.Structure):
    """Mirror of ``agx_recurrent_step`` up to ``multi``: the layout before the multi head was appended, which is
    also what the kernel takes by value."""

    _fields_ = ([("actor", RecurrentNet), ("critic", RecurrentNet)] + _ptr_fields("obs", "log_std", "reset", "mask") +
                [("N", ctypes.c_int64)] + _i32s("A", "box", "sample", "pad_") +
                [("seed", ctypes.c_uint64), ("counter", ctypes.c_uint64)] +
                _ptr_fields("actions", "log_probs", "entropy", "values", "obs_store"))


class RecurrentStepMulti(RecurrentStep):
    """Mirror of the whole ``agx_recurrent_step``: ``RecurrentStep`` and the ``agx_multi_head`` appended at its end
    (offset 1200).  This is what ``agx_ppo_act_recurrent`` is given."""

    _fields_ = [("multi", _lib.AgxMultiHead)]


HEAD_DISCRETE, HEAD_BOX, HEAD_MULTI, HEAD_BERNOULLI = range(4)  # AGX_RECURRENT_HEAD_*


def recurrent_head(space):
    """(AGX_RECURRENT_HEAD_* kind, A: the width of the actor's head, nvec or None, the columns of a row of actions)
    of an action space, or None for one the recurrent kernels have no head for.  MultiDiscrete and MultiBinary
    are 1-D."""
    nvec = getattr(space, "nvec", None)
    if nvec is not None:
        nvec = [int(n) for n in nvec] if len(getattr(space, "shape", ())) == 1 else []
        return (HEAD_MULTI, sum(nvec), nvec, len(nvec)) if nvec and min(nvec) >= 1 else None
    if type(space).__name__ == "MultiBinary":
        return (HEAD_BERNOULLI, int(space.shape[0]), None, int(space.shape[0])) if len(space.shape) == 1 else None
    if hasattr(space, "n"):
        return HEAD_DISCRETE, int(space.n), None, 1
    if hasattr(space, "low") and len(space.shape) == 1:
        return HEAD_BOX, int(space.shape[0]), None, int(space.shape[0])
    return None


def _recurrent_net(net, head, n_out: int):
    """(encoder, parameter tensors of the LSTM, output Linear, output activation code, head layers as
    (Linear, LayerNorm or None, relu)) of a recurrent network the kernel takes, or None."""
    from torch import nn

    enc = getattr(net, "encoder", None)
    if not isinstance(enc, _lstm.EvolvableLSTM) or getattr(net, "flatten_obs", False):
        return None
    found = _lstm._plan(enc.lstm)
    out = enc.model[f"{enc.name}_lstm_output"]
    act = enc.model[f"{enc.name}_output_activation"]
    code = {nn.Identity: 0, nn.ReLU: 1, nn.Tanh: 2}.get(type(act))
    if found is None or code is None or type(out) is not nn.Linear or out.bias is None or \
            not 1 <= out.out_features <= RECURRENT_MAX_WIDTH:
        return None
    layers, width = [], out.out_features
    for m in getattr(head, "model", ()):
        if type(m) is nn.Linear and m.bias is not None and m.in_features == width:
            if layers and not layers[-1][2]:  # a Linear after a layer without its ReLU
                return None
            layers.append([m, None, False])
            width = m.out_features
        elif type(m) is nn.LayerNorm and layers and m.elementwise_affine and layers[-1][1] is None \
                and not layers[-1][2] and tuple(m.normalized_shape) == (width,) and m.eps == 1e-5:
            layers[-1][1] = m
        elif type(m) is nn.ReLU and layers and not layers[-1][2]:
            layers[-1][2] = True
        elif type(m) is not nn.Identity:
            return None
    if not 2 <= len(layers) <= RECURRENT_MAX_HEAD or layers[-1][1] is not None or layers[-1][2] or \
            width != n_out or any(lay[0].out_features > RECURRENT_MAX_WIDTH for lay in layers):
        return None
    ts = [out.weight, out.bias] + [t for lin, ln, _ in layers for t in
                                   ((lin.weight, lin.bias) + ((ln.weight, ln.bias) if ln is not None else ()))]
    if any(t.dtype != _f32 or not t.is_cuda or not t.is_contiguous() for t in ts):
        return None
    return enc, found, out, code, layers


def _fill_recurrent_dense(d: RecurrentNet, plan) -> None:
    """The output Linear and the head of one network's descriptor over the live parameters."""
    _, _, out, code, layers = plan
    d.out_w, d.out_b, d.latent, d.out_act = out.weight.data_ptr(), out.bias.data_ptr(), out.out_features, code
    for j, (lin, ln, relu) in enumerate(layers):
        e = d.head[j]
        e.w, e.b, e.in_, e.out, e.relu = lin.weight.data_ptr(), lin.bias.data_ptr(), lin.in_features, \
            lin.out_features, int(relu)
        if ln is not None:
            e.ln_w, e.ln_b = ln.weight.data_ptr(), ln.bias.data_ptr()
    d.n_head = len(layers)


def _fill_recurrent_net(d: RecurrentNet, plan, hidden, N: int, nxt, store):
    """The descriptor of one network over its live parameters -> (h_next, c_next), or None on a state mismatch."""
    enc, (meta, ts), out, code, layers = plan
    (_, H, L), name = meta, enc.name
    h, c = hidden.get(f"{name}_h"), hidden.get(f"{name}_c")
    for t in (h, c):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (L, N, H) or t.dtype != _f32 or not t.is_cuda \
                or not t.is_contiguous():
            return None
    d.lstm = _lstm._desc(meta, ts)
    _fill_recurrent_dense(d, plan)
    h_next, c_next = nxt[0].view(L, N, H), nxt[1].view(L, N, H)
    d.h, d.c, d.h_next, d.c_next = h.data_ptr(), c.data_ptr(), h_next.data_ptr(), c_next.data_ptr()
    if store is not None:
        hs, cs = store[f"{name}_h"], store[f"{name}_c"]
        _need(hs, f"store[{name}_h]", _f32, (N, L, H))
        _need(cs, f"store[{name}_c]", _f32, (N, L, H))
        d.h_store, d.c_store = hs.data_ptr(), cs.data_ptr()
    return {f"{name}_h": h_next, f"{name}_c": c_next}


def ppo_act_recurrent(actor, critic, obs, hidden, *, sample=True, seed=0, counter=0, mask=None, reset=None,
                      out=None, store_hidden=None, store_obs=None):
    """agx_ppo_act_recurrent: one policy step of a ``StochasticActor`` / ``ValueNetwork`` pair on EvolvableLSTM
    encoders.  obs f32 [N, in]; hidden {``{encoder}_h`` / ``_c``: [L, N, H]} of both networks; mask uint8 / bool
    [N, A] (Discrete, 1 = legal) and reset uint8 / bool [N] (1 = start from the zero state) or None.  ``out``:
    {"actions" [N, 1] (Discrete) or [N, A] (Box), "log_probs", "values" [N]} f32 to write into (a rollout-buffer
    slot) instead of new tensors; store_hidden {key: [N, L, H]} / store_obs [N, in]: the slot's copies of the
    states the step was taken from and of obs.  -> {"actions", "log_probs" (None without ``sample``), "entropy",
    "values", "hidden": the next states}, or None where the kernel does not apply (the caller runs the torch
    modules): see include/agx_recurrent.h for the limits.  MultiDiscrete: mask [N, sum nvec], "actions" [N, K]
    (each component's index); MultiBinary: mask and "actions" [N, n] (0 / 1).

    A pair whose encoders are named alike, with one pair of states in ``hidden``, shares one encoder
    (``share_encoders``): the launch is agx_ppo_act_recurrent_shared, which runs the actor's encoder once and both
    heads on its latent; the critic's own encoder is not read."""
    from .modules._hooks import hooked

    found = recurrent_head(actor.action_space)
    if found is None:
        return None
    kind, A, nvec, cols = found
    box = kind == HEAD_BOX
    head = getattr(actor, "head_net", None)
    if not 1 <= A <= RECURRENT_MAX_ACTIONS or hooked(actor, critic) or (box and mask is not None):
        return None
    pa, pc = _recurrent_net(actor, getattr(head, "_wrapped", None), A), _recurrent_net(critic, critic.head_net, 1)
    if pa is None or pc is None or not isinstance(obs, torch.Tensor) or obs.dim() != 2 or obs.dtype != _f32 or \
            not obs.is_cuda or not obs.is_contiguous() or obs.shape[1] != pa[1][0][0] or pa[1][0][0] != pc[1][0][0] \
            or not 1 <= obs.shape[0] <= _lstm._MAX_ROWS:
        return None
    if box and (head.log_std.dtype != _f32 or not head.log_std.is_cuda or head.log_std.numel() != A):
        return None
    N, dev = obs.shape[0], obs.device
    # one encoder for both networks (share_encoders): the encoders are named alike and there is one pair of states
    shared = pa[0].name == pc[0].name and len(hidden) == 2
    sizes = [p[1][0][2] * N * p[1][0][1] for p in ((pa,) if shared else (pa, pc))]  # L N H
    nxt = torch.empty(2 * sum(sizes), dtype=_f32, device=dev)
    s = RecurrentStepMulti()
    nh_a = _fill_recurrent_net(s.actor, pa, hidden, N, (nxt[:sizes[0]], nxt[sizes[0]:2 * sizes[0]]), store_hidden)
    if shared:  # the critic gives its head; the kernel runs it on the actor's latent
        _fill_recurrent_dense(s.critic, pc)
        nh_c = {} if pc[2].out_features == pa[2].out_features else None
    else:
        nh_c = _fill_recurrent_net(s.critic, pc, hidden, N, (nxt[2 * sizes[0]:2 * sizes[0] + sizes[1]],
                                                              nxt[2 * sizes[0] + sizes[1]:]), store_hidden)
    if nh_a is None or nh_c is None:
        return None
    out = out or {}
    res = {"actions": out.get("actions"), "log_probs": out.get("log_probs"), "values": out.get("values")}
    if sample and res["actions"] is None:
        res["actions"] = torch.empty(N, cols, dtype=_f32, device=dev)
    small = torch.empty(3, N, dtype=_f32, device=dev)
    res["entropy"] = small[0]
    if res["values"] is None:
        res["values"] = small[1]
    if sample and res["log_probs"] is None:
        res["log_probs"] = small[2]
    if sample:
        _need(res["actions"], "actions", _f32, (N, cols))
        _need(res["log_probs"], "log_probs", _f32, (N,))
        s.actions, s.log_probs = res["actions"].data_ptr(), res["log_probs"].data_ptr()
    else:
        res["actions"] = res["log_probs"] = None
    _need(res["values"], "values", _f32, (N,))
    s.entropy, s.values = res["entropy"].data_ptr(), res["values"].data_ptr()
    s.obs, s.N, s.A, s.box, s.sample = obs.data_ptr(), N, A, kind, int(bool(sample))
    s.seed, s.counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    if box:
        s.log_std = head.log_std.data_ptr()
    if kind == HEAD_MULTI:
        s.multi = multi_head(nvec)
    keep = [nxt, small]
    for name, t, shape in (("mask", mask, (N, A)), ("reset", reset, (N,))):
        if t is None:
            continue
        t = torch.as_tensor(t)
        t = (t.view(_u8) if t.dtype == torch.bool else t.to(_u8)).to(dev).reshape(shape).contiguous()
        keep.append(t)
        setattr(s, name, t.data_ptr())
    if store_obs is not None:
        _need(store_obs, "store_obs", _f32, tuple(obs.shape))
        s.obs_store = store_obs.data_ptr()
    _lib.call("agx_ppo_act_recurrent_shared" if shared else "agx_ppo_act_recurrent", ctypes.byref(s), _lib.stream())
    res["hidden"] = {**nh_a, **nh_c}
    return res


# --------------------------------------------------------------------------- #
# The BPTT learner's heads (include/agx_recurrent_heads.h)                      #
# --------------------------------------------------------------------------- #
class RecurrentLinearGrad(ctypes.Structure):
    """Mirror of ``agx_recurrent_linear_grad``."""

    _fields_ = _ptr_fields("w", "b", "ln_w", "ln_b")


class RecurrentHeads(ctypes.Structure):
    """Mirror of ``agx_recurrent_heads`` up to ``multi``: the layout before the multi head was appended."""

    _fields_ = ([("net", RecurrentNet * 2), ("h_top", ctypes.c_void_p * 2), ("H", ctypes.c_int32 * 2)] +
                _ptr_fields("actions", "log_std", "mask") + [("R", ctypes.c_int64)] + _i32s("A", "box"))


class RecurrentHeadsMulti(RecurrentHeads):
    """Mirror of the whole ``agx_recurrent_heads``: ``RecurrentHeads`` and the ``agx_multi_head`` appended at its
    end (offset 1152).  This is what the head kernels' entry points are given."""

    _fields_ = [("multi", _lib.AgxMultiHead)]


class RecurrentHeadsGrads(ctypes.Structure):
    """Mirror of ``agx_recurrent_heads_grads``."""

    _fields_ = (_ptr_fields("g_log_prob", "g_entropy", "g_value") +
                [(n, ctypes.c_void_p * 2) for n in ("dh_top", "out_w", "out_b")] +
                [("head", (RecurrentLinearGrad * RECURRENT_MAX_HEAD) * 2)] + _ptr_fields("log_std"))


def _recurrent_heads_plan(actor, critic):
    """(the two networks' plans, ``recurrent_head`` of the action space, the parameter list of
    ``recurrent_heads_params``) or None."""
    from .modules._hooks import hooked

    found = recurrent_head(actor.action_space)
    if found is None:
        return None
    A, box = found[1], found[0] == HEAD_BOX
    head = getattr(actor, "head_net", None)
    if not 1 <= A <= RECURRENT_MAX_ACTIONS or hooked(actor, critic):
        return None
    pa, pc = _recurrent_net(actor, getattr(head, "_wrapped", None), A), _recurrent_net(critic, critic.head_net, 1)
    if pa is None or pc is None:
        return None
    if box and (head.log_std.dtype != _f32 or not head.log_std.is_cuda or head.log_std.numel() != A):
        return None
    shared = pa[0].name == pc[0].name  # share_encoders: one output Linear, the actor's
    if shared and pc[2].out_features != pa[2].out_features:
        return None
    ts = []
    for k, (_, _, out, _, layers) in enumerate((pa, pc)):
        ts += [] if shared and k == 1 else [out.weight, out.bias]
        for lin, ln, _ in layers:
            ts += [lin.weight, lin.bias] + ([ln.weight, ln.bias] if ln is not None else [])
    return (pa, pc), found, ts + ([head.log_std] if box else []), shared


def recurrent_heads_params(actor, critic):
    """The parameters ``recurrent_heads_forward`` reads, in the order ``recurrent_heads_backward`` returns their
    gradients: per network (actor, critic) the output Linear's weight and bias, then each head layer's weight,
    bias and LayerNorm affine; ``log_std`` last (Box).  A pair that shares one encoder (encoders named alike) has
    one output Linear, the actor's: the critic's is not in the list.  None where the kernels do not apply (the
    limits of ``ppo_act_recurrent``, include/agx_recurrent.h)."""
    found = _recurrent_heads_plan(actor, critic)
    return None if found is None else found[2]


def _recurrent_heads(actor, critic, h_top, actions, mask):
    """-> (the descriptor, the two plans, the parameter list, tensors the descriptor points into) or None."""
    found = _recurrent_heads_plan(actor, critic)
    if found is None:
        return None
    plans, (kind, A, nvec, cols), params, shared = found
    box = kind == HEAD_BOX
    R = h_top[0].shape[0] if isinstance(h_top[0], torch.Tensor) and h_top[0].dim() == 2 else 0
    if not 1 <= R <= _lstm._MAX_ROWS or (box and mask is not None) or len(h_top) != (1 if shared else 2):
        return None
    s = RecurrentHeadsMulti()
    for k, plan in enumerate(plans):
        _fill_recurrent_dense(s.net[k], plan)
        if shared and k == 1:  # the critic's head reads the actor's latent
            break
        h, H = h_top[k], plan[1][0][1]
        if not isinstance(h, torch.Tensor) or tuple(h.shape) != (R, H) or h.dtype != _f32 or not h.is_cuda or \
                not h.is_contiguous():
            return None
        s.h_top[k], s.H[k] = h.data_ptr(), H
    if not isinstance(actions, torch.Tensor) or actions.dtype != _f32 or not actions.is_cuda or \
            not actions.is_contiguous() or tuple(actions.shape) != ((R,) if kind == HEAD_DISCRETE else (R, cols)):
        return None
    keep = [actions]
    if mask is not None:
        mask = torch.as_tensor(mask)
        mask = (mask.view(_u8) if mask.dtype == torch.bool else mask.to(_u8)).to(actions.device).reshape(R, A)
        keep.append(mask := mask.contiguous())
        s.mask = mask.data_ptr()
    s.actions, s.R, s.A, s.box = actions.data_ptr(), R, A, kind
    if box:
        s.log_std = actor.head_net.log_std.data_ptr()
    if kind == HEAD_MULTI:
        s.multi = multi_head(nvec)
    return s, plans, params, keep, "_shared" if shared else ""


def recurrent_heads_forward(actor, critic, h_top, actions, mask=None, *, save=True):
    """agx_recurrent_heads_forward: everything after the LSTMs of a ``StochasticActor`` / ``ValueNetwork`` pair over
    R padded rows in one launch.  h_top: (actor's, critic's) top-layer LSTM output f32 [R, H]; actions f32 [R]
    (Discrete, the index), [R, A] (Box), [R, K] (MultiDiscrete, each component's index) or [R, n] (MultiBinary);
    mask uint8 / bool [R, A] or None, A the width of the actor's head.  -> (log_prob, entropy, value [R],
    saved: what ``recurrent_heads_backward`` reads, None without ``save``), or None where the kernels do not
    apply (the caller runs the torch modules).  A pair that shares one encoder takes h_top = (the one output,)
    and agx_recurrent_heads_forward_shared."""
    found = _recurrent_heads(actor, critic, h_top, actions, mask)
    if found is None:
        return None
    s, form = found[0], found[4]
    dev = actions.device
    out = torch.empty(3, s.R, dtype=_f32, device=dev)
    saved = None
    if save:
        nbytes = getattr(_lib.load(), "agx_recurrent_heads_saved_bytes" + form)(ctypes.byref(s))
        saved = torch.empty(nbytes // 4, dtype=_f32, device=dev)
    _lib.call("agx_recurrent_heads_forward" + form, ctypes.byref(s), out[0].data_ptr(), out[1].data_ptr(),
              out[2].data_ptr(), _lib.ptr(saved), _lib.stream())
    return out[0], out[1], out[2], saved


def recurrent_heads_backward(actor, critic, h_top, actions, mask, saved, g_log_prob, g_entropy, g_value):
    """agx_recurrent_heads_backward on the inputs and ``saved`` of ``recurrent_heads_forward`` and the upstream
    gradients f32 [R]: two launches.  -> (dh_top of the actor, of the critic [R, H], the gradients of
    ``recurrent_heads_params`` in its order), or None where the kernels do not apply.  A pair that shares one
    encoder has one dh_top, with both heads' shares; the critic's is None."""
    found = _recurrent_heads(actor, critic, h_top, actions, mask)
    if found is None:
        return None
    s, plans, params, _, form = found
    R = s.R
    for t, n in ((g_log_prob, "g_log_prob"), (g_entropy, "g_entropy"), (g_value, "g_value")):
        _need(t, n, _f32, (R,))
    g = RecurrentHeadsGrads()
    g.g_log_prob, g.g_entropy, g.g_value = g_log_prob.data_ptr(), g_entropy.data_ptr(), g_value.data_ptr()
    dh = [torch.empty_like(h) for h in h_top]
    grads = [torch.empty_like(t) for t in params]
    it = iter(grads)
    for k, (_, _, _, _, layers) in enumerate(plans):
        if k < len(dh):  # a network with an output Linear of its own
            g.dh_top[k], g.out_w[k], g.out_b[k] = dh[k].data_ptr(), next(it).data_ptr(), next(it).data_ptr()
        for j, (_, ln, _) in enumerate(layers):
            e = g.head[k][j]
            e.w, e.b = next(it).data_ptr(), next(it).data_ptr()
            if ln is not None:
                e.ln_w, e.ln_b = next(it).data_ptr(), next(it).data_ptr()
    if s.box == HEAD_BOX:
        g.log_std = next(it).data_ptr()
    nbytes = getattr(_lib.load(), "agx_recurrent_heads_workspace_bytes" + form)(ctypes.byref(s))
    ws = torch.empty(nbytes // 4, dtype=_f32, device=actions.device)
    _lib.call("agx_recurrent_heads_backward" + form, ctypes.byref(s), saved.data_ptr(), ctypes.byref(g),
              ws.data_ptr(), _lib.stream())
    return dh[0], dh[1] if len(dh) == 2 else None, grads
