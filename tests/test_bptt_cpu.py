"""Recurrent PPO's host side, where no device is needed: the binding's struct mirror, the sequence-type names,
and ``PPO(recurrent=True)`` built on the CPU (the reference's module names, hidden-state keys and 5-tuple)."""

import copy
import ctypes

import numpy as np
import pytest
import torch

from agilerl_amd import kernels as K
from agilerl_amd.algorithms.ppo import PPO
from agilerl_amd.envs import Box, Discrete, MultiDiscrete

NET = {"encoder_config": {"hidden_state_size": 16, "num_layers": 2}}


def test_gather_args_layout():
    """sizeof / offsetof of agx_bptt_gather_args (include/agx_bptt.h) as the C compiler lays it out."""
    a = K.BpttGatherArgs
    assert (ctypes.sizeof(a), a.obs.offset, a.obs_out.offset, a.valid_row.offset) == (328, 96, 224, 320)


@pytest.mark.parametrize("given,code", [(None, 0), ("chunked", 0), ("MAXIMUM", 1), ("fifty_percent_overlap", 2)])
def test_sequence_type(given, code):
    assert K.bptt_sequence_type(given) == code
    with pytest.raises(NotImplementedError):
        K.bptt_sequence_type("strided")


def test_recurrent_ppo_on_cpu():
    agent = PPO(Box(-1.0, 1.0, (4,)), Discrete(3), recurrent=True, share_encoders=False, num_envs=2, learn_step=8,
                net_config=NET, device="cpu")
    assert isinstance(agent, PPO) and agent.recurrent
    assert agent.get_hidden_state_architecture() == {f"{n}_encoder_{s}": (2, 2, 16)
                                                     for n in ("actor", "critic") for s in ("h", "c")}
    keys = set(agent.state_dict())
    assert {"actor.encoder.model.actor_encoder_lstm.weight_ih_l0",
            "actor.head_net._wrapped.model.actor_linear_layer_output.weight",
            "critic.head_net.model.value_linear_layer_output.weight"} <= keys
    hidden = agent.get_initial_hidden_state(2)
    action, log_prob, entropy, value, nxt = agent.get_action(np.zeros((2, 4), np.float32), hidden_state=hidden)
    assert action.shape == log_prob.shape == entropy.shape == value.shape == (2,)
    assert set(nxt) == set(hidden) and all(nxt[k].shape == hidden[k].shape and nxt[k].any() for k in nxt)
    assert agent.rollout_buffer.buffer["hidden_states"]["actor_encoder_h"].shape == (4, 2, 2, 16)
    # six rows under [layers, 2, H] states are two sequences of three steps; the actor still copies afterwards
    logp, _, values = agent.evaluate_actions(torch.zeros(6, 4), torch.zeros(6), hidden_state=hidden)
    assert logp.shape == values.shape == (6,) and logp.requires_grad
    assert copy.deepcopy(agent.actor).head_net.logits is None


def test_recurrent_ppo_refusals():
    obs = Box(-1.0, 1.0, (4,))
    with pytest.raises(ValueError, match="use_rollout_buffer"):
        PPO(obs, Discrete(3), recurrent=True, share_encoders=False, use_rollout_buffer=False, device="cpu")
    with pytest.raises(NotImplementedError, match="share_encoders"):
        PPO(obs, Discrete(3), recurrent=True, device="cpu")
    for kw in (dict(action_space=MultiDiscrete([2, 2])), dict(action_space=Box(-1.0, 1.0, (2,)),
                                                             net_config={**NET, "squash_output": True}),
               dict(action_space=Discrete(3), observation_space=Box(0.0, 1.0, (3, 8, 8)))):
        args = {"observation_space": obs, "net_config": NET, **kw}
        with pytest.raises(NotImplementedError):
            PPO(recurrent=True, share_encoders=False, device="cpu", **args)
    box = PPO(obs, Box(-1.0, 1.0, (2,)), recurrent=True, share_encoders=False, net_config=NET, device="cpu")
    assert tuple(box.state_dict()["actor.head_net.log_std"].shape) == (1, 2)
