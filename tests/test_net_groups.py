"""The one declaration of an agent's networks (EvolvableAgentMixin._groups)
and what is derived from it: the checkpoint layout of all five off-policy
classes, pinned to the literal names they have always written, and the
learning-rate / optimizer hooks on a TD3 agent."""

import numpy as np
import pytest
import torch

_COMMON = {"agilerl_version", "algo", "batch_size", "fitness", "gamma", "index", "learn_step", "mut", "net_config",
           "network_info", "scores", "steps", "tau"}
_Q = _COMMON | {"lr", "normalize_images", "spaces"}
_DPG = _COMMON | {"O_U_noise", "current_noise", "dt", "expl_noise", "learn_counter", "lr_actor", "lr_critic",
                  "mean_noise", "network_arch", "normalize_images", "policy_freq", "theta", "vect_noise_dim"}
LAYOUT = {
    "DQN": (_Q | {"double"}, ["actor", "actor_target"], ["optimizer"]),
    "RainbowDQN": (_Q | {"beta", "combined_reward", "n_step", "noise_std", "num_atoms", "prior_eps", "v_max", "v_min"},
                   ["actor", "actor_target"], ["optimizer"]),
    "DDPG": (_DPG, ["actor", "actor_target", "critic", "critic_target"], ["actor_optimizer", "critic_optimizer"]),
    "TD3": (_DPG, ["actor", "actor_target", "critic_1", "critic_target_1", "critic_2", "critic_target_2"],
            ["actor_optimizer", "critic_1_optimizer", "critic_2_optimizer"]),
    "MADDPG": (_COMMON | {"agent_ids", "lr_actor", "lr_critic"},
               ["actors", "actor_targets", "critics", "critic_targets"], ["actor_optimizers", "critic_optimizers"]),
}


def _agent(algo):
    from agilerl_amd import algorithms
    from agilerl_amd.envs import Box, Discrete

    obs, box = Box(-np.inf, np.inf, (6,)), Box(-1.0, 1.0, (3,))
    cls = getattr(algorithms, algo)
    if algo == "MADDPG":
        return cls([obs, obs], [box, box], agent_ids=["a", "b"], device="cpu")
    return cls(obs, Discrete(4) if algo in ("DQN", "RainbowDQN") else box, device="cpu")


@pytest.mark.parametrize("algo", list(LAYOUT))
def test_checkpoint_layout_is_pinned(algo, tmp_path):
    top, networks, optimizers = LAYOUT[algo]
    agent = _agent(algo)
    path = str(tmp_path / "agent.pt")
    agent.save_checkpoint(path)
    ck = torch.load(path, weights_only=True)
    assert set(ck) == top
    info = ck["network_info"]
    assert info["network_names"] == networks and info["optimizer_names"] == optimizers
    assert list(info["modules"]) == [f"{n}_state_dict" for n in networks]
    assert list(info["optimizers"]) == [f"{n}_state_dict" for n in optimizers]
    if algo == "MADDPG":  # dict-valued groups nest one level, by agent id
        assert all(list(sd) == ["a", "b"] for sd in (*info["modules"].values(), *info["optimizers"].values()))
    for n in networks:  # what was written is what the agent holds
        want = getattr(agent, n)
        for got, net in ([(info["modules"][f"{n}_state_dict"][a], want[a]) for a in want] if algo == "MADDPG"
                         else [(info["modules"][f"{n}_state_dict"], want)]):
            sd = net.state_dict()
            assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


def test_td3_hooks_derive_from_the_groups():
    agent = _agent("TD3")
    assert agent.get_lr_names() == ["lr_actor", "lr_critic"]
    assert agent._triples() == (("actor", "actor_target", "actor_optimizer"),
                                ("critic_1", "critic_target_1", "critic_1_optimizer"),
                                ("critic_2", "critic_target_2", "critic_2_optimizer"))
    actor_opt, c1, c2 = agent.actor_optimizer, agent.critic_1_optimizer, agent.critic_2_optimizer
    agent.lr_critic = 3e-3
    agent.reinit_optimizers("lr_critic")
    assert agent.actor_optimizer is actor_opt
    assert agent.critic_1_optimizer is not c1 and agent.critic_2_optimizer is not c2
    for opt, net in ((agent.critic_1_optimizer, agent.critic_1), (agent.critic_2_optimizer, agent.critic_2)):
        assert type(opt) is torch.optim.Adam and opt.param_groups[0]["lr"] == 3e-3
        assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in net.parameters()]
    agent.reinit_optimizers()
    assert agent.actor_optimizer is not actor_opt and agent.actor_optimizer.param_groups[0]["lr"] == agent.lr_actor
