"""Independent restatements for the bandit tests (NeuralUCB / NeuralTS,
include/agx_bandit.h), in float64 numpy and in plain torch:

  * ``gradients`` / ``select``: the arm gradients, the quadratic forms, the
    scores, numpy's own (masked) argmax and the Sherman-Morrison update in the
    reference's form, Sigma^-1 v v^T Sigma^-1 / (1 + v^T Sigma^-1 v)
    (neural_ucb_bandit.py:237-257) — pinned to the reference's own get_action
    by tests/golden/bandit_*.npz (tests/test_bandit_cpu.py);
  * ``normals``: the Thompson draws, from tests.gauss_twin's Philox block and
    Box-Muller mapping (dimension 0 of env k);
  * ``ref32``: the same step with float32 torch CPU ops in the reference's
    form, for the error yardstick of shapes without a golden file;
  * ``inputs``: seeded random-ReLU-feature inputs as the golden generator draws
    them, redrawn until every step's score gap clears 64 x the float32 error;
  * ``Twin``: plain-torch ``learn`` (MSE + reg ||theta - theta_0||^2, torch
    Adam) and the torch-op ``get_action`` on copies of an agent's networks.
"""

from __future__ import annotations

import numpy as np
import torch

from tests import gauss_twin


def ulp(v) -> np.ndarray:
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def bound(err_ref, value) -> np.ndarray:
    """4 x max(err_ref, 1 float32 ulp of the value) — test_cqn_gpu.py's convention."""
    return 4.0 * np.maximum(err_ref, ulp(value))


def gradients(h, bias_one: bool = True, scale: float = 1.0) -> np.ndarray:
    """float64 [A, D] of g_k = fl32(scale * [h_k, 1]) (or fl32(scale * h_k))."""
    h = np.asarray(h, np.float32)
    g = h * np.float32(scale)
    if bias_one:
        g = np.concatenate([g, np.full((h.shape[0], 1), np.float32(scale), np.float32)], axis=1)
    return g.astype(np.float64)


def normals(A: int, seed: int, counter: int) -> np.ndarray:
    return gauss_twin.gauss_eps(np.arange(A), np.zeros(A, np.int64), seed, counter)


def argmax(scores: np.ndarray, mask=None) -> int:
    if mask is None:
        return int(np.argmax(scores))
    return int(np.argmax(np.ma.array(scores, mask=1 - (np.asarray(mask) == 1).astype(np.int64))))


def select(g, mu, sigma_inv, mask=None, gamma: float = 1.0, z=None) -> dict:
    """One step in float64 -> quad, scores, action, gap (best minus second-best
    legal score; inf with one legal arm) and the updated sigma_inv."""
    g, mu, S = np.asarray(g, np.float64), np.asarray(mu, np.float64), np.asarray(sigma_inv, np.float64)
    quad = np.einsum("ki,ij,kj->k", g, S, g)
    width = gamma * np.sqrt(quad)
    scores = mu + (width if z is None else width * np.asarray(z, np.float64))
    action = argmax(scores, mask)
    legal = np.ones(len(mu), bool) if mask is None else np.asarray(mask) == 1
    top = np.sort(scores[legal])[::-1]
    gap = float(top[0] - top[1]) if len(top) > 1 else float("inf")
    v = g[action][:, None]
    new = S - (S @ v @ v.T @ S) / (1.0 + v.T @ S @ v)
    return dict(quad=quad, scores=scores, action=action, gap=gap, sigma_inv=new)


def ref32(g, mu, sigma_inv, action: int, gamma: float = 1.0) -> dict:
    """The reference's float32 torch ops on the CPU (the batched matmuls and
    the update of neural_ucb_bandit.py:238-257) with the action given."""
    g = torch.as_tensor(np.asarray(g, np.float32))
    S = torch.as_tensor(np.asarray(sigma_inv, np.float32)).clone()
    quad = torch.matmul(torch.matmul(g[:, None, :], S), g[:, :, None])[:, 0, :].squeeze(-1)
    scores = torch.as_tensor(np.asarray(mu, np.float32)) + gamma * torch.sqrt(quad)
    v = g[action].unsqueeze(-1)
    S -= (S @ v @ v.T @ S) / (1 + v.T @ S @ v)
    return dict(quad=quad.numpy(), scores=scores.numpy(), sigma_inv=S.numpy())


def inputs(A: int, H: int, T: int, seed: int = 0, masked: bool = False, lamb: float = 1.0, gamma: float = 1.0,
           bias_one: bool = True):
    """T steps of (h [A, H] random ReLU features, mu [A], mask) with, per
    step, the float32 reference's one-step error against float64 on the same
    inputs (err_scores / err_quad / err_sigma: ``ref32`` stepping its own
    float32 matrix from lamb * I, ``select`` evaluated on that matrix) and the
    float64 gap.  Redrawn with the next seed until gap >= 64 x err_scores at
    every step: a device result that picks another arm is then wrong, not
    unlucky."""
    D = H + int(bias_one)
    for s in range(seed, seed + 50):
        rng = np.random.default_rng(s)
        W = (rng.standard_normal((H, 6)) * 0.8).astype(np.float32)
        S32 = (lamb * np.eye(D)).astype(np.float32)
        steps, ok = [], True
        for _ in range(T):
            h = np.maximum(rng.standard_normal((A, 6)).astype(np.float32) @ W.T, 0).astype(np.float32)
            mu = rng.standard_normal(A).astype(np.float32)
            mask = None
            if masked:
                mask = (rng.random(A) < 0.6).astype(np.uint8)
                mask[rng.integers(0, A)] = 1
            g = gradients(h, bias_one)
            t = select(g, mu, S32, mask, gamma)
            r = ref32(g, mu, S32, t["action"], gamma)
            err_scores = float(np.max(np.abs(r["scores"].astype(np.float64) - t["scores"])))
            if not t["gap"] >= 64 * err_scores:
                ok = False
                break
            steps.append(dict(h=h, mu=mu, mask=mask, twin=t, err_scores=err_scores,
                              err_quad=float(np.max(np.abs(r["quad"].astype(np.float64) - t["quad"]))),
                              err_sigma=float(np.max(np.abs(r["sigma_inv"].astype(np.float64) - t["sigma_inv"])))))
            S32 = r["sigma_inv"]
        if ok:
            return steps
    raise AssertionError(f"no seed near {seed} keeps every gap above 64 x the float32 error (A={A}, H={H})")


class Twin:
    """Plain torch on copies of an agent's network: ``get_action`` by the
    torch-op route (kernels.bandit_select_torch, whatever the device) and
    ``learn`` as the reference writes it, with torch's Adam."""

    def __init__(self, agent):
        self.agent = agent.clone()
        self.actor = self.agent.actor
        self.opt = torch.optim.Adam(self.actor.parameters(), lr=agent.lr)
        self.theta_0 = self.agent.theta_0.clone()
        self.reg = agent.reg

    @classmethod
    def of(cls, agent) -> "Twin":
        return cls(agent)

    def learn(self, experiences) -> float:
        obs = experiences["obs"].to(torch.float32)
        rewards = experiences["reward"].to(torch.float32).reshape(obs.shape[0], 1)
        pred = self.actor(obs)
        layer = self.actor.get_output_dense()
        theta = torch.cat([w.flatten() for w in layer.parameters()])
        loss = torch.nn.functional.mse_loss(rewards, pred) + self.reg * torch.norm(theta - self.theta_0) ** 2
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return float(loss.item())

    @torch.no_grad()
    def act(self, obs, mask=None) -> tuple[int, float, float]:
        """One get_action by the torch-op route on this twin's network and
        matrix -> (action, the float64 gap of the step, the float32
        reference's score error on the same inputs)."""
        from agilerl_amd import kernels as K

        a = self.agent
        mu, h = a.arm_features(a._obs(obs))
        g = gradients(h.cpu().numpy(), True, a._scale)
        pre = a.sigma_inv.cpu().numpy()
        t = select(g, mu.cpu().numpy(), pre, mask, float(a.gamma))
        r = ref32(g, mu.cpu().numpy(), pre, t["action"], float(a.gamma))
        m = None if mask is None else torch.as_tensor(np.asarray(mask) == 1).to(torch.uint8).to(a.device)
        action, _, _ = K.bandit_select_torch(h, mu, a.sigma_inv, m, bias_one=True, scale=a._scale,
                                             gamma=float(a.gamma))
        return int(action.item()), t["gap"], float(np.max(np.abs(r["scores"].astype(np.float64) - t["scores"])))
