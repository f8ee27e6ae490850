"""The BPTT learner's head kernels' host side where no device is needed: the binding's struct mirrors and the
switch's default."""

import ctypes

from agilerl_amd import kernels as K
from agilerl_amd.algorithms.ppo import PPO
from agilerl_amd.envs import Box, Discrete


def test_descriptor_layout():
    """sizeof / offsetof of include/agx_recurrent_heads.h's structs as the C compiler lays them out."""
    heads, grads = K.RecurrentHeads, K.RecurrentHeadsGrads
    assert ctypes.sizeof(K.RecurrentLinearGrad) == 32
    assert (ctypes.sizeof(heads), heads.h_top.offset, heads.H.offset, heads.actions.offset, heads.R.offset,
            heads.box.offset) == (1152, 1088, 1104, 1112, 1136, 1148)
    assert (ctypes.sizeof(grads), grads.dh_top.offset, grads.out_w.offset, grads.head.offset,
            grads.log_std.offset) == (336, 24, 40, 72, 328)


def test_switch_is_off_by_default(monkeypatch):
    monkeypatch.delenv("AGX_RECURRENT_LEARN", raising=False)
    kw = dict(recurrent=True, share_encoders=False, device="cpu",
              net_config={"encoder_config": {"hidden_state_size": 16}})
    assert not PPO(Box(-1.0, 1.0, (4,)), Discrete(3), **kw).fused_learn_on()
    on = PPO(Box(-1.0, 1.0, (4,)), Discrete(3), fused_learn=True, **kw)
    assert on.fused_learn_on()
    monkeypatch.setenv("AGX_RECURRENT_LEARN", "0")
    assert not on.fused_learn_on()
    monkeypatch.setenv("AGX_RECURRENT_LEARN", "1")
    assert PPO(Box(-1.0, 1.0, (4,)), Discrete(3), **kw).fused_learn_on()
