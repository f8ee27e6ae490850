"""The shared-encoder entry points' argument checks, which run on the host before anything is launched: a critic
head that does not start at the actor's latent, and a NULL actor state, are AGX_EINVAL with a message.  The
descriptors hold a made-up non-NULL address that the checks never read through."""

import ctypes

import pytest

from agilerl_amd import _lib
from agilerl_amd import kernels as K

PTR, EINVAL = 0x1000, -1


def _net(d, latent, out, head_in=None):
    """A one-layer LSTM (4 -> 16), an output Linear to ``latent`` and a head [16] -> ``out`` over made-up pointers."""
    d.lstm.in_, d.lstm.H, d.lstm.L = 4, 16, 1
    lay = d.lstm.layer[0]
    lay.w_ih = lay.w_hh = lay.b_ih = lay.b_hh = PTR
    d.out_w = d.out_b = d.h = d.c = PTR
    d.latent, d.n_head = latent, 2
    for j, (i, o) in enumerate(((head_in or latent, 16), (16, out))):
        d.head[j].w = d.head[j].b = PTR
        d.head[j].in_, d.head[j].out, d.head[j].relu = i, o, int(j == 0)


def _step(**kw):
    s = K.RecurrentStepMulti()
    _net(s.actor, 8, 3)
    _net(s.critic, 8, 1, **kw)
    s.obs, s.N, s.A, s.sample = PTR, 1, 3, 1
    return s


def _heads(**kw):
    s = K.RecurrentHeadsMulti()
    _net(s.net[0], 8, 3)
    _net(s.net[1], 8, 1, **kw)
    s.h_top[0], s.H[0], s.actions, s.R, s.A = PTR, 16, PTR, 1, 3
    return s


@pytest.mark.parametrize("what", ["latent", "state"])
def test_step_refuses(what):
    lib = _lib.load(require_gpu=False)
    s = _step(head_in=24) if what == "latent" else _step()
    if what == "state":
        s.actor.h = None
    assert lib.agx_ppo_act_recurrent_shared(ctypes.byref(s), None) == EINVAL
    msg = lib.agx_last_error().decode()
    assert "agx_ppo_act_recurrent_shared" in msg and ("critic: head layer 0: 24 -> 16 after width 8" in msg
                                                      if what == "latent" else "state is NULL" in msg)


def test_heads_refuse():
    lib = _lib.load(require_gpu=False)
    bad = _heads(head_in=24)
    assert lib.agx_recurrent_heads_saved_bytes_shared(ctypes.byref(bad)) == 0
    assert lib.agx_recurrent_heads_workspace_bytes_shared(ctypes.byref(bad)) == 0
    assert lib.agx_recurrent_heads_forward_shared(ctypes.byref(bad), PTR, PTR, PTR, None, None) == EINVAL
    assert "critic: head layer 0: 24 -> 16 after width 8" in lib.agx_last_error().decode()
    assert lib.agx_recurrent_heads_backward_shared(ctypes.byref(bad), PTR, PTR, PTR, None) == EINVAL
    ok = _heads()  # the plan of a good pair: one latent and one dZ_out, not two
    assert lib.agx_recurrent_heads_saved_bytes_shared(ctypes.byref(ok)) == 4 * (8 + 16 + 16 + 3)
    assert lib.agx_recurrent_heads_workspace_bytes_shared(ctypes.byref(ok)) == 4 * (8 + 16 + 3 + 16 + 1)
