"""What the object-level off-policy agents (DQN, RainbowDQN, DDPG, TD3,
MADDPG, MATD3) share besides the network groups of evolvable.py: unpacking a
sampled batch, the fused critic loss, and the evaluation loop."""

from __future__ import annotations

import numpy as np
import torch

from .. import kernels as K


def batch(agent, experiences, *keys) -> list[torch.Tensor]:
    """``experiences[k]`` for every key on the agent's device: observations
    through ``agent._obs``, everything else as the tensor it is."""
    get = experiences.get if hasattr(experiences, "get") else experiences.__getitem__
    to = lambda x: (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).to(agent.device)  # noqa: E731
    return [agent._obs(get(k)) if k in ("obs", "next_obs") else to(get(k)) for k in keys]


class MSECriticLoss(torch.autograd.Function):
    """MSE(Q1, y) [+ MSE(Q2, y)] with y = r + (1 - d) gamma min(Q1', Q2'):
    one launch computes y, the loss and dLoss/dQk.  ``sanitize``: MADDPG's
    rules for r and d (NaN rewards -> 0, NaN dones -> 1, dones as uint8),
    with one critic (MADDPG) or two (MATD3)."""

    @staticmethod
    def forward(ctx, q1, q2, qn1, qn2, rewards, dones, gamma, sanitize):
        r, d, twin = rewards.contiguous(), dones.contiguous(), q2 is not None
        if sanitize and twin:
            _, g1, g2, loss = K.matd3_critic_target(q1.contiguous(), q2.contiguous(), qn1.contiguous(),
                                                    qn2.contiguous(), r, d, gamma)
        elif sanitize:
            _, g1, loss = K.maddpg_critic_target(q1.contiguous(), qn1.contiguous(), r, d, gamma)
        else:
            _, g1, g2, loss = K.td3_critic_target(q1.contiguous(), qn1.contiguous(), r, d, gamma,
                                                  q2=q2.contiguous() if twin else None,
                                                  qn2=qn2.contiguous() if twin else None)
        ctx.twin = twin
        ctx.save_for_backward(g1.view_as(q1), *((g2.view_as(q2),) if twin else ()))
        return loss.view(())

    @staticmethod
    def backward(ctx, gl):
        g = ctx.saved_tensors
        return (g[0] * gl, g[1] * gl if ctx.twin else None) + (None,) * 6


def _evaluate(agent, env, act, max_steps, loop) -> float:
    """Mean over ``loop`` passes of the score of every env's first finished
    episode (the reference algorithms' ``test``); appended to agent.fitness."""
    rewards = []
    num_envs = env.num_envs if hasattr(env, "num_envs") else 1
    for _ in range(loop):
        obs, _ = env.reset()
        scores = np.zeros(num_envs)
        completed = np.zeros(num_envs)
        finished = np.zeros(num_envs, dtype=bool)
        step = 0
        while not np.all(finished):
            obs, r, term, trunc, _ = env.step(act(obs))
            step += 1
            scores += np.asarray(r).reshape(num_envs)
            done = np.logical_or(term, trunc).reshape(num_envs)
            if max_steps is not None and step == max_steps:
                done[:] = True
            for i in range(num_envs):
                if done[i] and not finished[i]:
                    completed[i] = scores[i]
                    finished[i] = True
        rewards.append(float(np.mean(completed)))
    f = float(np.mean(rewards))
    agent.fitness.append(f)
    return f
