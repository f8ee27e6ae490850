"""CQN.learn (cqn.py:216-265) restated twice: the yardsticks agx_cqn_loss and
the shipped ``CQN.learn`` are held to.

* ``cqn_loss_twin``: the loss of cqn.py:234-252 and its gradient with respect
  to Q(s) in numpy — y in float32 in the reference's op order (it must be
  bit-equal), everything after it in float64.  tests/test_cqn_cpu.py pins it
  to the reference's own outputs (tests/golden/cqn_*.npz).
* ``cql_loss_torch``: the same loss as torch ops, written once; y bit-equal
  to the reference's.  ``cqn_loss_torch32`` runs it on float32 CPU tensors
  with autograd: its distance to the float64 twin is the error a float32
  evaluation has, the unit of the GPU tests' bounds.
* ``Twin.of(agent)``: the update as plain torch ops (``cql_loss_torch``, norm
  clip at 1, torch Adam, a per-tensor soft update) on deep copies of the
  agent's networks; tools/cqn_update_time.py times it as the baseline.
"""

from __future__ import annotations

import copy

import numpy as np
import torch

f32, f64 = np.float32, np.float64


def cqn_loss_twin(q_next_online, q_next_target, q_cur, actions, rewards, dones, gamma, double) -> dict:
    """-> dict(y [B, 1] f32, lse [B] f64, terms (mean lse, mean Q, MSE) f64,
    loss f64, grad [B, A] f64).  np.max / np.argmax treat a NaN as torch
    does: the maximum, at the first NaN's index."""
    qnt = np.asarray(q_next_target, f32)
    B, A = qnt.shape
    r, d = np.asarray(rewards, f32).reshape(B), np.asarray(dones, f32).reshape(B)
    if double:
        qt = qnt[np.arange(B), np.argmax(np.asarray(q_next_online, f32), axis=1)]
    else:
        qt = np.max(qnt, axis=1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        y = r + (f32(gamma) * qt) * (f32(1.0) - d)  # float32, one rounding per op
        q = np.asarray(q_cur, f32).astype(f64)
        a = np.asarray(actions).reshape(B).astype(np.int64)
        m = np.max(q, axis=1)  # NaN rows: NaN throughout, as torch.logsumexp
        shift = np.where(np.isinf(m), 0.0, m)
        lse = np.log(np.sum(np.exp(q - shift[:, None]), axis=1)) + shift
        qa = q[np.arange(B), a]
        td = qa - y.astype(f64)
        terms = np.array([np.mean(lse), np.mean(q), np.mean(td * td)], f64)
        loss = (terms[0] - terms[1]) + 0.5 * terms[2]
        grad = np.exp(q - lse[:, None]) / B - 1.0 / (B * A)
        grad[np.arange(B), a] += td / B
    return dict(y=y.reshape(B, 1), lse=lse, terms=terms, loss=loss, grad=grad)


def cql_loss_torch(next_online, next_target, q, actions, rewards, dones, gamma, double):
    """The update's loss as torch ops, in the tensors' own dtype and on their
    device: next_online / next_target / q are [B, A] network outputs (only q
    may carry a gradient), actions / rewards / dones [B, 1].
    -> (y [B, 1], (mean lse, mean Q, MSE), loss).  The products and sums of y
    are taken in the order that gives the reference's float32 bits:
    ((gamma * q_t) * (1 - d)) + r."""
    with torch.no_grad():
        if double:
            best_next = torch.take_along_dim(next_target, next_online.argmax(1, keepdim=True), 1)
        else:
            best_next = next_target.amax(1, keepdim=True)
        y = (best_next * gamma) * (1.0 - dones) + rewards
    taken = torch.take_along_dim(q, actions.long(), 1)
    terms = (torch.logsumexp(q, 1).mean(), q.mean(), torch.nn.functional.mse_loss(taken, y))
    return y, terms, (terms[0] - terms[1]) + 0.5 * terms[2]


def cqn_loss_torch32(q_next_online, q_next_target, q_cur, actions, rewards, dones, gamma, double) -> dict:
    """``cql_loss_torch`` on float32 CPU tensors, autograd for the gradient.
    -> dict(y, terms, loss, grad) as numpy."""
    t = lambda x: torch.as_tensor(np.asarray(x))  # noqa: E731
    B = np.asarray(q_next_target).shape[0]
    q = t(q_cur).clone().requires_grad_(True)
    y, terms, loss = cql_loss_torch(t(q_next_online), t(q_next_target), q, t(actions).reshape(B, 1),
                                    t(rewards).reshape(B, 1), t(dones).reshape(B, 1), gamma, double)
    loss.backward()
    return dict(y=y.numpy(), terms=np.array([x.item() for x in terms], f64), loss=loss.item(), grad=q.grad.numpy())


def inputs(B: int, A: int, seed: int = 0) -> dict:
    """Seeded float32 inputs: Q values 3 * randn, about a fifth of the rows done."""
    rng = np.random.default_rng(100003 * B + 31 * A + seed)
    q = lambda: (3.0 * rng.standard_normal((B, A))).astype(f32)  # noqa: E731
    return dict(q_next_online=q(), q_next_target=q(), q_cur=q(), actions=rng.integers(0, A, B).astype(np.int64),
                rewards=rng.standard_normal(B).astype(f32), dones=(rng.random(B) < 0.2).astype(f32), gamma=0.99)


class Twin:
    """The reference's update on given networks with a torch Adam optimizer."""

    def __init__(self, actor, actor_target, optimizer, gamma, tau, double):
        self.actor, self.actor_target, self.optimizer = actor, actor_target, optimizer
        self.gamma, self.tau, self.double = gamma, tau, double

    @classmethod
    def of(cls, agent):
        """On deep copies of ``agent``'s networks (a CQN of the package)."""
        actor, target = copy.deepcopy([agent.actor, agent.actor_target])
        return cls(actor, target, torch.optim.Adam(actor.parameters(), lr=agent.lr), agent.gamma, agent.tau,
                   agent.double)

    def soft_update(self):
        with torch.no_grad():
            for e, t in zip(self.actor.parameters(), self.actor_target.parameters()):
                t.copy_(self.tau * e + (1.0 - self.tau) * t)

    def learn(self, experiences) -> float:
        obs, next_obs = experiences["obs"], experiences["next_obs"]
        with torch.no_grad():
            next_online = self.actor(next_obs) if self.double else None
            next_target = self.actor_target(next_obs)
        _, _, loss = cql_loss_torch(next_online, next_target, self.actor(obs), experiences["action"],
                                    experiences["reward"], experiences["done"], self.gamma, self.double)
        self.optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.actor.parameters(), 1.0)
        self.optimizer.step()
        self.soft_update()
        return loss.item()
