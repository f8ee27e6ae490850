"""Independent restatements for the kernels on the tail of every learn():
the population optimiser (csrc/optim.hip) and DQN's TD target
(csrc/td_targets.hip), in float64 / float32 numpy and in plain torch on the
CPU, plus the seeded inputs the GPU tests (tests/test_tail_kernels_gpu.py)
feed the kernels.  tests/test_tail_twin_cpu.py pins the restatements to each
other, to torch and to tests/golden/dqn*.npz on exactly those inputs.

  * ``clip_adam_f64``: the optim.hip header in float64;
  * ``clip_adam_torch32``: clip_grad_norm_ per group + torch.optim.Adam in
    float32 — the reference project's own arithmetic;
  * ``td_target_f32``: dqn.py:296-314 in float32 numpy, one rounding per op in
    the kernel's order (libagx is built with -ffp-contract=off);
  * ``td_target_torch``: the same lines as torch ops — the authority for NaN
    rows and argmax ties.
"""

from __future__ import annotations

import functools

import numpy as np
import torch

f32 = np.float32


def _abi(x) -> float:
    """A scalar as the C ABI hands it to the kernel: rounded to float32."""
    return float(f32(x))


# ---- optimiser ------------------------------------------------------------------ #
def clip_adam_f64(params, m, v, grads, steps, offsets, max_norm, lr, betas=(0.9, 0.999), eps=1e-8, active=None):
    """One agx_clip_adam call in float64.  params / m / v / grads [P, n], steps
    [P] (each agent's count BEFORE this update), offsets [G + 1], lr a scalar or
    [P].  -> (params, m, v, grads as the call leaves them, steps) as new arrays.

    The scalars (max_norm, lr, betas, eps, the clip's 1e-6) are the float32
    values the C ABI carries, used as such in every place — so 1 - b2 is
    1 - float32(0.999), not float32(0.001) as in torch's addcmul_.  An agent
    whose ``active`` flag is 0 keeps everything, its step count included;
    max_norm <= 0 leaves the gradients alone."""
    p, m, v, g = (np.array(x, dtype=np.float64) for x in (params, m, v, grads))
    steps = np.array(steps, dtype=np.int64)
    P = p.shape[0]
    lr = np.broadcast_to(np.asarray(lr, dtype=f32).astype(np.float64).reshape(-1), (P,))
    b1, b2, eps, mn, tiny = _abi(betas[0]), _abi(betas[1]), _abi(eps), _abi(max_norm), _abi(1e-6)
    for i in range(P):
        if active is not None and not active[i]:
            continue
        if mn > 0:
            for a, b in zip(offsets[:-1], offsets[1:]):
                norm = np.sqrt(np.sum(g[i, a:b] ** 2))
                g[i, a:b] *= min(mn / (norm + tiny), 1.0)
        t = int(steps[i]) + 1
        m[i] += (1.0 - b1) * (g[i] - m[i])
        v[i] = b2 * v[i] + (1.0 - b2) * g[i] * g[i]
        denom = np.sqrt(v[i]) / np.sqrt(1.0 - b2 ** t) + eps
        p[i] -= lr[i] / (1.0 - b1 ** t) * (m[i] / denom)
        steps[i] = t
    return p, m, v, g, steps


def clip_adam_torch32(params, m, v, grads, steps, offsets, max_norm, lr, betas=(0.9, 0.999), eps=1e-8, active=None):
    """The same call as the reference runs it: per agent one torch.optim.Adam
    over one float32 Parameter per group, clip_grad_norm_ on each group, step.
    The moments and the step count go in through the optimizer's state (the
    checkpoint-restore path).  Same arguments and return as clip_adam_f64, in
    float32."""
    p, m, v, g = (torch.tensor(np.asarray(x), dtype=torch.float32).clone() for x in (params, m, v, grads))
    steps = np.array(steps, dtype=np.int64)
    P = p.shape[0]
    lr = np.broadcast_to(np.asarray(lr, dtype=np.float64).reshape(-1), (P,))
    spans = list(zip(offsets[:-1], offsets[1:]))
    for i in range(P):
        if active is not None and not active[i]:
            continue
        ws = [torch.nn.Parameter(p[i, a:b].clone()) for a, b in spans]
        opt = torch.optim.Adam(ws, lr=float(lr[i]), betas=tuple(betas), eps=eps)
        for w, (a, b) in zip(ws, spans):
            w.grad = g[i, a:b].clone()
            opt.state[w] = dict(step=torch.tensor(float(steps[i])), exp_avg=m[i, a:b].clone(),
                                exp_avg_sq=v[i, a:b].clone())
        if max_norm > 0:
            for w in ws:
                torch.nn.utils.clip_grad_norm_([w], max_norm)
        opt.step()
        for w, (a, b) in zip(ws, spans):
            p[i, a:b], g[i, a:b] = w.detach(), w.grad
            m[i, a:b], v[i, a:b] = opt.state[w]["exp_avg"], opt.state[w]["exp_avg_sq"]
            assert float(opt.state[w]["step"]) == steps[i] + 1
        steps[i] += 1
    return p.numpy(), m.numpy(), v.numpy(), g.numpy(), steps


# The optimiser cases of tests/test_tail_kernels_gpu.py.  ``norm``: the max_norm
# the gradient norms are laid out around (the case's own max_norm where that
# is positive).  ``zero``: the group whose gradient is exactly zero for agent 0.
# ``masks``: the ``active`` argument of each of the four steps.
_K = 8192  # optim.hip's sum-of-squares chunk; more than 16 chunks take the pre-reduction
ADAM_CASES = {
    # group boundaries off a multiple of 4: one inside the first chunk, one in a later chunk
    "prereduced-float4": dict(P=2, n=17 * _K + 4, offsets=[0, 3001, 70_003, 17 * _K + 4], max_norm=10.0, zero=0),
    "prereduced-scalar": dict(P=2, n=17 * _K + 5, offsets=[0, 3001, 70_003, 17 * _K + 5], max_norm=10.0, zero=0),
    "active-mask": dict(P=4, n=5000, offsets=[0, 3100, 5000], max_norm=0.5,
                        masks=[[1, 1, 1, 1], [1, 0, 1, 0], [0, 0, 1, 1], None]),
    "no-clip-float4": dict(P=2, n=5000, offsets=[0, 3100, 5000], max_norm=0.0, norm=0.5),
    "no-clip-scalar": dict(P=2, n=5001, offsets=[0, 3101, 5001], max_norm=0.0, norm=0.5),
    "one-group": dict(P=2, n=1000, offsets=[0, 1000], max_norm=0.5),
    "eight-groups": dict(P=2, n=5003, offsets=[0, 1, 600, 1203, 2000, 2900, 3001, 4100, 5003], max_norm=0.5, zero=3),
    "betas-eps-steps": dict(P=3, n=5000, offsets=[0, 3100, 5000], max_norm=0.5, betas=(0.8, 0.9), eps=1e-5,
                            steps0=[0, 7, 1000], lr=[1e-3, 5e-4, 2e-3], moments=True),
}
N_STEPS = 4


def adam_inputs(name: str) -> dict:
    """Seeded inputs of an ADAM_CASES entry: params p0, moments m0 / v0, steps0
    and one gradient array per step.  Every (agent, group) gradient is a normal
    draw rescaled to a chosen L2 norm: 4..8 x ``norm`` on the first step (clip
    active), ``norm`` / 4..8 afterwards (coef 1) — far from the clip's branch
    point, so float32 and float64 take the same branch."""
    c = dict(ADAM_CASES[name])
    P, n, offsets = c["P"], c["n"], c["offsets"]
    rng = np.random.default_rng(sorted(ADAM_CASES).index(name) + 100)
    c["p0"] = rng.standard_normal((P, n)).astype(f32)
    if c.get("moments"):  # a restored optimiser: moments that go with a non-zero step count
        c["m0"] = (0.01 * rng.standard_normal((P, n))).astype(f32)
        c["v0"] = (1e-4 * rng.random((P, n))).astype(f32)
    else:
        c["m0"], c["v0"] = np.zeros((P, n), f32), np.zeros((P, n), f32)
    c["steps0"] = np.asarray(c.get("steps0", [0] * P), dtype=np.int64)
    c["lr"] = np.asarray(c.get("lr", [1e-3, 5e-4, 2e-3, 1e-3][:P]), dtype=f32)
    c.setdefault("betas", (0.9, 0.999))
    c.setdefault("eps", 1e-8)
    c.setdefault("masks", [None] * N_STEPS)
    norm = c.get("norm", c["max_norm"])
    grads = []
    for s in range(N_STEPS):
        g = rng.standard_normal((P, n))
        for i in range(P):
            for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
                u = rng.uniform(1.0, 2.0)
                want = 4.0 * norm * u if s == 0 else norm / (4.0 * u)
                g[i, a:b] *= want / np.sqrt(np.sum(g[i, a:b] ** 2))
                if i == 0 and c.get("zero") == k:
                    g[i, a:b] = 0.0
        grads.append(g.astype(f32))
    c["grads"] = grads
    return c


def adam_norms_off_the_branch(c: dict) -> bool:
    """The condition on the inputs: every (agent, group, step) gradient norm is
    at least 2 max_norm or at most max_norm / 2 (trivially so without a clip)."""
    mn = c["max_norm"]
    for g in c["grads"]:
        for a, b in zip(c["offsets"][:-1], c["offsets"][1:]):
            norm = np.sqrt(np.sum(g[:, a:b].astype(np.float64) ** 2, axis=1))
            if mn > 0 and not np.all((norm >= 2 * mn) | (norm <= mn / 2)):
                return False
    return True


@functools.lru_cache(maxsize=None)
def adam_twins(name: str):
    """(inputs, float64 states, float32 torch states): the state (params, m, v,
    grads, steps) after each of the N_STEPS updates, each twin carrying its own
    state in its own precision.  Computed once per case; treat as read-only."""
    c = adam_inputs(name)
    out = []
    for fn in (clip_adam_f64, clip_adam_torch32):
        p, m, v, steps = c["p0"], c["m0"], c["v0"], c["steps0"]
        states = []
        for s in range(N_STEPS):
            p, m, v, g, steps = fn(p, m, v, c["grads"][s], steps, c["offsets"], c["max_norm"], c["lr"], c["betas"],
                                   c["eps"], c["masks"][s])
            states.append((p, m, v, g, steps))
        out.append(states)
    return c, out[0], out[1]


# ---- DQN's TD target ------------------------------------------------------------- #
def td_target_f32(q_next_online, q_next_target, q_cur, actions, rewards, dones, gamma, double):
    """dqn.py:296-314 in float32 numpy in the kernel's op order: q_t = max_a
    Qtgt(s') or Qtgt(s')[argmax_a Q(s')] (the first index on ties; NaN counts
    as the largest value, as in torch), y = r + (g q_t)(1 - d), dloss/dQ[a] =
    (Q[a] - y)(2 / B); the loss is the float64 mean of the squared errors
    rounded to float32.  -> (y [B, 1], g_q [B, A], loss)."""
    qnt = np.asarray(q_next_target, f32)
    B, A = qnt.shape
    r, d = np.asarray(rewards, f32).reshape(B), np.asarray(dones, f32).reshape(B)
    if double:
        qt = qnt[np.arange(B), np.argmax(np.asarray(q_next_online, f32), axis=1)]
    else:
        qt = np.max(qnt, axis=1)
    y = r + (f32(gamma) * qt) * (f32(1.0) - d)
    a = np.asarray(actions).reshape(B).astype(np.int64)
    qa = np.asarray(q_cur, f32)[np.arange(B), a]
    g_q = np.zeros((B, A), f32)
    g_q[np.arange(B), a] = (qa - y) * (f32(2.0) / f32(B))
    loss = f32(np.mean((qa.astype(np.float64) - y.astype(np.float64)) ** 2))
    return y.reshape(B, 1), g_q, loss


def td_target_torch(q_next_online, q_next_target, q_cur, actions, rewards, dones, gamma, double):
    """The reference's lines themselves on CPU tensors, autograd for
    dloss/dQ.  -> (y [B, 1], g_q [B, A], loss) as numpy."""
    t = lambda x: torch.as_tensor(np.asarray(x))  # noqa: E731
    B = np.asarray(q_next_target).shape[0]
    rewards, dones = t(rewards).reshape(B, 1), t(dones).reshape(B, 1)
    with torch.no_grad():
        if double:
            q_idx = t(q_next_online).argmax(dim=1).unsqueeze(1)
            q_target = t(q_next_target).gather(dim=1, index=q_idx)
        else:
            q_target = t(q_next_target).max(axis=1)[0].unsqueeze(1)
        y = rewards + gamma * q_target * (1 - dones)
    q = t(q_cur).clone().requires_grad_(True)
    loss = torch.nn.MSELoss()(q.gather(1, t(actions).reshape(B, 1).long()), y)
    loss.backward()
    return y.numpy(), q.grad.numpy(), loss.detach().numpy()


TD_B, TD_A = (1, 255, 256, 257, 1000), (1, 2, 6, 33)


@functools.lru_cache(maxsize=None)
def td_inputs(B: int, A: int, seed: int = 0) -> dict:
    """Seeded float32 inputs of a TD-target call: about a tenth of the rows
    done, and (from B = 255 on) rows 64..95 with all-equal online Q and rows
    80..111 with all-equal target Q, so some rows tie in one, some in both.
    Treat as read-only."""
    rng = np.random.default_rng(1000 * B + A + seed)
    rec = dict(qno=rng.standard_normal((B, A)).astype(f32), qnt=rng.standard_normal((B, A)).astype(f32),
               qc=rng.standard_normal((B, A)).astype(f32), a=rng.integers(0, A, B).astype(np.int64),
               r=rng.standard_normal(B).astype(f32), d=(rng.random(B) < 0.1).astype(f32), gamma=0.99)
    if B == 1:
        rec["qno"][:] = rec["qno"][0, 0]
    else:
        rec["qno"][64:96] = rec["qno"][64:96, :1]
        rec["qnt"][80:112] = rec["qnt"][80:112, :1]
    return rec


def td_call(fn, rec: dict, double: bool):
    return fn(rec["qno"], rec["qnt"], rec["qc"], rec["a"], rec["r"], rec["d"], rec["gamma"], double)


def td_nan_inputs(double: bool) -> dict:
    """B = 300, A = 6 with NaN rows: in q_next_target (plain max) or in
    q_next_online (double: the argmax is the first NaN's index), at the first,
    a middle and the last action, two in one row, in both blocks."""
    rec = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in td_inputs(300, 6, seed=7).items()}
    q = rec["qno"] if double else rec["qnt"]
    for row, cols in ((0, [0]), (5, [3]), (17, [5]), (70, [2, 4]), (85, [4, 1]), (255, [5]), (256, [0]), (299, [1, 5])):
        q[row, cols] = np.nan
    return rec


def ulp32(x) -> float:
    return float(np.spacing(np.abs(f32(x))))
