"""TD3.learn (td3.py:462-551) and DDPG.learn (ddpg.py:422-498) restated in
plain PyTorch: the yardstick the shipped update is held to.  tests/
test_td3_cpu.py pins ``smooth`` and ``critic_target`` to the reference's own
outputs (tests/golden/td3_*.npz, ddpg_*.npz); the GPU tests and
tools/td3_update_time.py run ``learn`` beside the shipped path.

One difference of form from the reference: the smoothing noise is drawn into
a fresh tensor of the actions' shape (the reference draws it in place into
the batch's actions) — same generator consumption, same values.
"""

from __future__ import annotations

import torch


def smooth(mu, noise, low, high, noise_clip):
    """td3.py:494-501: multi_dim_clamp(-c, c, noise) is torch.clamp for float
    bounds, multi_dim_clamp(low, high, x) is max(min(x, high), low) for tensors."""
    noise = torch.clamp(noise, -noise_clip, noise_clip)
    next_actions = mu + noise
    return torch.max(torch.min(next_actions, high), low)


def critic_target(q, q_next, rewards, dones, gamma):
    """td3.py:507-515 / ddpg.py:459-461: q, q_next are lists of one (DDPG) or
    two (TD3) tensors -> (y, critic loss)."""
    q_next_state = q_next[0] if len(q_next) == 1 else torch.min(q_next[0], q_next[1])
    y = rewards + ((1 - dones) * gamma * q_next_state)
    loss = torch.nn.functional.mse_loss(q[0], y)
    for qk in q[1:]:
        loss = loss + torch.nn.functional.mse_loss(qk, y)
    return y, loss


class Twin:
    """The reference's update on given networks with torch Adam optimizers.
    critics / critic_targets / critic_opts: lists of one (DDPG) or two (TD3)."""

    def __init__(self, actor, actor_target, critics, critic_targets, actor_opt, critic_opts, low, high, gamma, tau,
                 policy_freq):
        self.actor, self.actor_target, self.critics, self.critic_targets = actor, actor_target, critics, critic_targets
        self.actor_opt, self.critic_opts = actor_opt, critic_opts
        self.low, self.high, self.gamma, self.tau, self.policy_freq = low, high, gamma, tau, policy_freq
        self.learn_counter = 0

    @classmethod
    def of(cls, agent):
        """On deep copies of ``agent``'s networks (a DDPG or TD3 of the package)."""
        import copy

        nets = copy.deepcopy([[getattr(agent, n) for n in t[:2]] for t in agent._triples()])
        (actor, actor_target), pairs = nets[0], nets[1:]
        dev = next(actor.parameters()).device
        return cls(actor, actor_target, [p[0] for p in pairs], [p[1] for p in pairs],
                   torch.optim.Adam(actor.parameters(), lr=agent.lr_actor),
                   [torch.optim.Adam(p[0].parameters(), lr=agent.lr_critic) for p in pairs],
                   agent.action_low.to(dev), agent.action_high.to(dev), agent.gamma, agent.tau, agent.policy_freq)

    def networks(self):
        return [self.actor, self.actor_target, *self.critics, *self.critic_targets]

    def soft_update(self, net, target):
        with torch.no_grad():
            for e, t in zip(net.parameters(), target.parameters()):
                t.copy_(self.tau * e + (1.0 - self.tau) * t)

    def learn(self, experiences, noise_clip=0.5, policy_noise=0.2):
        obs, actions, rewards = experiences["obs"], experiences["action"], experiences["reward"]
        next_obs, dones = experiences["next_obs"], experiences["done"]
        q = [critic(obs, actions) for critic in self.critics]
        with torch.no_grad():
            mu = self.actor_target(next_obs)
            noise = torch.empty_like(actions).normal_(0, policy_noise)
            next_actions = smooth(mu, noise, self.low, self.high, noise_clip)
            q_next = [target(next_obs, next_actions) for target in self.critic_targets]
        _, critic_loss = critic_target(q, q_next, rewards, dones, self.gamma)
        for opt in self.critic_opts:
            opt.zero_grad()
        critic_loss.backward()
        for opt in self.critic_opts:
            opt.step()
        self.learn_counter += 1
        if self.learn_counter % self.policy_freq != 0:
            return None, critic_loss.item()
        actor_loss = -self.critics[0](obs, self.actor(obs)).mean()
        self.actor_opt.zero_grad()
        actor_loss.backward()
        self.actor_opt.step()
        self.soft_update(self.actor, self.actor_target)
        for critic, target in zip(self.critics, self.critic_targets):
            self.soft_update(critic, target)
        return actor_loss.item(), critic_loss.item()
