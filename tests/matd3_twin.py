"""The critic step of MATD3.learn_individual (matd3.py:861-880) restated in
numpy: the CPU twin ``agx_matd3_critic_target`` is held to bit for bit.
tests/test_matd3_cpu.py pins it to the reference's own outputs
(tests/golden/matd3_*.npz); tests/test_matd3_gpu.py runs the kernel beside it.

f32 throughout with one rounding per op, in the reference's op order:
  q'   = torch.min(q_next1, q_next2)              (np.minimum: a NaN wins, as in torch.min)
  r    = where(isnan(r), 0, r)
  d    = where(isnan(d), 1, d).to(uint8)          (truncation)
  y    = r + ((1 - d) * gamma) * q'               (1 - d in uint8 arithmetic: d = 2 gives 255)
  loss = f32(mean((q1 - y)^2)) + f32(mean((q2 - y)^2))   (each mean in f64, the sum in f32)
  g_qk = (qk - y) * (2 / B)
"""

from __future__ import annotations

import numpy as np


def critic_target(q1, q2, q_next1, q_next2, r, d, gamma):
    """-> (y, g_q1, g_q2, loss), flat f32 arrays and an f32 scalar."""
    q1, q2, qn1, qn2, r, d = (np.asarray(x, np.float32).reshape(-1) for x in (q1, q2, q_next1, q_next2, r, d))
    qn = np.minimum(qn1, qn2)
    r = np.where(np.isnan(r), np.float32(0), r)
    du = np.where(np.isnan(d), np.float32(1), d).astype(np.uint8)
    nd = (np.uint8(1) - du).astype(np.float32)
    with np.errstate(invalid="ignore"):
        y = (r + (nd * np.float32(gamma)) * qn).astype(np.float32)
        scale = np.float32(2.0) / np.float32(q1.shape[0])
        grads, losses = [], []
        for q in (q1, q2):
            diff = q.astype(np.float64) - y.astype(np.float64)
            losses.append(np.float32(np.sum(diff * diff) / np.float64(q.shape[0])))
            grads.append(((q - y) * scale).astype(np.float32))
    return y, grads[0], grads[1], np.float32(losses[0] + losses[1])
