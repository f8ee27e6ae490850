"""Drop-in ``CQN`` (agilerl/algorithms/cqn.py:18-325): conservative
Q-learning for offline data with Discrete actions.

The networks, ``get_action`` and ``test`` are DQN's (dqn.py).  The update's
loss — the TD target, half its MSE, mean(logsumexp_a Q(s)) - mean(Q(s)) and
the dense gradient with respect to Q(s) — is one HIP kernel (agx_cqn_loss,
include/agx_cqn.h); the tail is the flat clip_grad_norm_(1) + Adam launch and
the flat Polyak launch (flat_state.py).  Offline training calls ``learn``
back to back with no env step in between (training/train_offline.py), so the
whole update is replayed from a captured graph from the second call of a
given batch shape on (learn_graph.py); ``learn_device`` returns the loss
without reading it back, so a run of updates is enqueued without a host
round trip.
"""

from __future__ import annotations

import torch

from .. import kernels as K
from ..modules.mlp import EvolvableMLP
from . import learn_graph
from .ddpg import restore_arch, save_arch
from .dqn import _EpsilonGreedyQAgent
from .flat_state import flat_state
from .offpolicy import batch

_KEYS = ("obs", "action", "reward", "next_obs", "done")
_MAX_NORM = 1.0  # clip_grad_norm_(self.actor.parameters(), 1), cqn.py:259


class _CQLLoss(torch.autograd.Function):
    """(mean lse - mean Q) + 0.5 MSE(Q(s)[a], r + gamma * q_t * (1 - d)) with
    the HIP kernel computing y, the loss and dLoss/dQ(s) in one pass."""

    @staticmethod
    def forward(ctx, q_cur, q_next_target, q_next_online, actions, rewards, dones, gamma, double):
        _, g_q, loss = K.cqn_loss(q_cur.contiguous(), q_next_target.contiguous(), actions, rewards, dones, gamma,
                                  q_next_online=q_next_online.contiguous() if double else None, double=double)
        ctx.save_for_backward(g_q)
        return loss.view(())

    @staticmethod
    def backward(ctx, gl):
        (g_q,) = ctx.saved_tensors
        return (g_q * gl,) + (None,) * 7


class CQN(_EpsilonGreedyQAgent):
    algo = "CQN"

    def __init__(self, observation_space, action_space, index: int = 0, hp_config=None, net_config=None,
                 batch_size: int = 64, lr: float = 1e-4, learn_step: int = 5, gamma: float = 0.99,
                 tau: float = 1e-3, double: bool = False, normalize_images: bool = True, mut=None,
                 actor_network=None, device="cuda", accelerator=None, wrap: bool = True):
        assert isinstance(learn_step, int) and learn_step >= 1, "Learn step must be an integer greater than or equal to one."
        assert isinstance(tau, float) and tau > 0, "Tau must be a float greater than zero."
        assert isinstance(double, bool), "Double Q-learning flag must be boolean value True or False."
        self._setup(observation_space, action_space, index, hp_config, net_config, batch_size, lr, learn_step, gamma,
                    tau, mut, normalize_images, double, actor_network, device)

    # A checkpoint carries what architecture and activation mutations change
    # (ddpg.py save_arch / restore_arch, plus the activation, which DDPG / TD3
    # never mutate), so that a mutated agent loads into a freshly built one.
    def _ckpt_extra(self, ck: dict) -> None:
        if isinstance(getattr(self.actor, "encoder", None), EvolvableMLP):
            save_arch(self, ck)
            ck["network_activation"] = self.actor.activation

    def _ckpt_restore(self, ck: dict) -> None:
        if "network_arch" not in ck:
            return
        act = ck.get("network_activation")
        for n in ck["network_arch"]:
            if act and getattr(self, n).activation != act:
                getattr(self, n).change_activation(act, output=False)
        restore_arch(self, ck)

    def _loss(self, xs: list) -> torch.Tensor:
        """The forwards of cqn.py:234-246, the fused loss and the backward
        pass over xs = [obs, action, reward, next_obs, done]."""
        obs, actions, rewards, next_obs, dones = xs
        with torch.no_grad():
            q_next_target = self.actor_target(next_obs)
            q_next_online = self.actor(next_obs) if self.double else None
        q_cur = self.actor(obs)
        loss = _CQLLoss.apply(q_cur, q_next_target, q_next_online, actions.reshape(-1).long().contiguous(),
                              rewards.reshape(-1).float().contiguous(), dones.reshape(-1).float().contiguous(),
                              float(self.gamma), bool(self.double))
        self.optimizer.zero_grad()
        loss.backward()
        return loss.detach()

    def learn_device(self, experiences) -> torch.Tensor:
        """One update; -> the loss as a device scalar, not read back.  After a
        replayed update it is the graph's static output: read it (or add it
        to a running sum) before the next update.  ``experiences``: the
        mapping the replay buffer samples, or the reference's (states,
        actions, rewards, next_states, dones) tuple."""
        if isinstance(experiences, (tuple, list)):
            experiences = dict(zip(_KEYS, experiences))
        xs = batch(self, experiences, *_KEYS)
        fs = flat_state(self)
        nets = (self.actor, self.actor_target)
        g = self.optimizer.param_groups[0]
        key = ("cqn", bool(self.double), float(self.gamma), float(self.tau), tuple(g["betas"]), float(g["eps"]))
        loss = learn_graph.run(fs, key, xs, self._loss, nets, _MAX_NORM, self.tau)
        if loss is None:
            loss = self._loss(xs)
            flat_ok = fs is not None and fs.step(_MAX_NORM)  # clip_grad_norm_(1) + Adam: one launch (flat_state.py)
            if flat_ok:
                fs.polyak(self.tau)
            else:
                torch.nn.utils.clip_grad_norm_(self.actor.parameters(), _MAX_NORM)
                self.optimizer.step()
                self.soft_update()
            learn_graph.note_eager(fs, key, xs, nets, flat_ok)
        return loss

    def learn(self, experiences) -> float:
        """-> the loss (cqn.py:216-265).  The device work is replayed from a
        captured graph from the second update of a given shape on."""
        return float(self.learn_device(experiences).item())
