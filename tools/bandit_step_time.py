"""NeuralUCB.get_action and one train_bandits inner step on one GPU, against a
plain-torch restatement of the reference's get_action / learn on copies of
the same networks (the baseline: what the reference's step costs on this GPU).

All on SyntheticBanditEnv (10 arms, 8 features: an 80-dim context per arm) in
one process:

  * ``act``      get_action per call, default networks (D = 33: the resident
                 form of agx_bandit_select), replayed from its captured graph;
  * ``step``     one train_bandits inner step: get_action, the env step, one
                 buffer add, learn_step = 2 updates on fresh samples (B = 64),
                 the losses read once;
  * ``act501``   get_action per call with a 500-wide head (D = 501: the
                 streaming form);
  * the same three for the torch restatement: one backward pass per arm for
    the gradient matrix, the two batched matmuls, the host argmax in numpy and
    the Sigma^-1 v v^T Sigma^-1 update; learn with torch's Adam and a loss
    read per update, as the reference's loop has.

Each figure is the median and range of BLOCKS blocks of STEPS calls, the paths
alternating block by block, every block between two device events (each call
ends in the scalar read-back of its action, so a block's span includes those
round trips), after WARMUP calls of every path.

  python tools/bandit_step_time.py [--out FILE]      one JSON line (also written to FILE)
"""
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS, FEATURES, BATCH, LEARN_STEP = 10, 8, 64, 2
STEPS = int(os.environ.get("STEPS", 200))
BLOCKS = int(os.environ.get("BLOCKS", 5))
WARMUP = 30


class TorchBandit:
    """The reference's NeuralUCB step as torch ops on a copy of an agent's network."""

    def __init__(self, agent):
        import torch

        self.actor = copy.deepcopy(agent.actor)
        self.layer = self.actor.get_output_dense()
        self.opt = torch.optim.Adam(self.actor.parameters(), lr=agent.lr)
        self.sigma_inv = agent.sigma_inv.clone()
        self.theta_0 = torch.cat([w.detach().flatten() for w in self.layer.parameters()])
        self.gamma, self.reg, self.arms, self.device = agent.gamma, agent.reg, agent.action_dim, agent.device

    def _theta_grad(self):
        import numpy as np
        import torch

        return torch.cat([w.grad.detach().flatten() / np.sqrt(self.layer.weight.size(0))
                          for w in self.layer.parameters()])

    def get_action(self, obs) -> int:
        import numpy as np
        import torch

        x = torch.as_tensor(np.asarray(obs), dtype=torch.float32, device=self.device)
        mu = self.actor(x).reshape(-1)
        g = torch.zeros((self.arms, self.sigma_inv.shape[0]), device=self.device)
        for k in range(self.arms):
            self.opt.zero_grad()
            mu[k].backward(retain_graph=True)
            g[k] = self._theta_grad()
        with torch.no_grad():
            quad = torch.matmul(torch.matmul(g[:, None, :], self.sigma_inv), g[:, :, None])[:, 0, :].squeeze(-1)
            values = mu + self.gamma * torch.sqrt(quad)
        action = int(np.argmax(values.cpu().numpy()))
        v = g[action].unsqueeze(-1)
        self.sigma_inv -= (self.sigma_inv @ v @ v.T @ self.sigma_inv) / (1 + v.T @ self.sigma_inv @ v)
        return action

    def learn(self, experiences) -> float:
        import torch

        obs, rewards = experiences["obs"].float(), experiences["reward"].float()
        theta = torch.cat([w.flatten() for w in self.layer.parameters()])
        loss = torch.nn.functional.mse_loss(rewards, self.actor(obs)) + \
            self.reg * torch.norm(theta - self.theta_0) ** 2
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return loss.item()


def _blocks(paths, per_block):
    """us per call of every path: BLOCKS alternating blocks, sorted."""
    import torch

    us = {name: [] for name in paths}
    for _ in range(BLOCKS):
        for name, fn in paths.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(per_block):
                fn()
            end.record()
            end.synchronize()
            us[name].append(1e3 * start.elapsed_time(end) / per_block)
    for v in us.values():
        v.sort()
    return us


def _setup(head):
    """-> {path: one call} for the act and step measurements of one head width."""
    import numpy as np
    import torch

    from agilerl_amd.algorithms import NeuralUCB
    from agilerl_amd.components import ReplayBuffer
    from agilerl_amd.envs import SyntheticBanditEnv
    from agilerl_amd.networks.base import mlp_net_config

    torch.manual_seed(0)
    cfg = None if head is None else {"head_config": mlp_net_config([head])}
    paths = {}
    for name in ("agx", "torch"):
        env = SyntheticBanditEnv(ARMS, FEATURES, seed=1)
        torch.manual_seed(0)
        agent = NeuralUCB(env.observation_space, env.action_space, net_config=cfg, batch_size=BATCH, device="cuda")
        actor = agent if name == "agx" else TorchBandit(agent)
        memory = ReplayBuffer(10000)
        state = {"ctx": env.reset()}

        def act(actor=actor, env=env, state=state):
            action = actor.get_action(state["ctx"])
            state["ctx"], _ = env.step(action)

        def step(actor=actor, env=env, state=state, memory=memory, fused=name == "agx"):
            ctx = state["ctx"]
            action = actor.get_action(ctx)
            state["ctx"], reward = env.step(action)
            memory.add({"obs": np.asarray(ctx[action])[None], "reward": np.asarray([reward], np.float32)})
            if len(memory) < BATCH:
                return
            if fused:  # train_bandits here: the losses summed on the device, one read
                total = torch.zeros((), dtype=torch.float64, device="cuda")
                for _ in range(LEARN_STEP):
                    total += actor.learn_device(memory.sample(BATCH))
                total.item()
            else:
                for _ in range(LEARN_STEP):
                    actor.learn(memory.sample(BATCH))

        paths[name] = (act, step)
    return paths


def main():
    import torch

    out = {"steps_per_block": STEPS, "blocks": BLOCKS, "arms": ARMS, "context_dim": ARMS * FEATURES, "batch": BATCH,
           "learn_step": LEARN_STEP}
    for tag, head, kinds in (("D33", None, ("act", "step")), ("D501", 500, ("act",))):
        paths = _setup(head)
        for k, kind in enumerate(("act", "step")):
            if kind not in kinds:
                continue
            fns = {name: p[k] for name, p in paths.items()}
            for fn in fns.values():
                for _ in range(WARMUP + (BATCH if kind == "step" else 0)):
                    fn()
            torch.cuda.synchronize()
            for name, v in _blocks(fns, STEPS).items():
                out[f"{tag}_{kind}_{name}_us"] = round(v[len(v) // 2], 2)
                out[f"{tag}_{kind}_{name}_us_min_max"] = [round(v[0], 2), round(v[-1], 2)]
            out[f"{tag}_{kind}_speedup"] = round(out[f"{tag}_{kind}_torch_us"] / out[f"{tag}_{kind}_agx_us"], 2)
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
