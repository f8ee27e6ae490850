"""agx_ppo_bern_graph_check (include/agx_bernoulli.h): the check plans on the
host and makes no HIP call, so everything here runs without a GPU (as
tests/test_multidisc_learner_cpu.py).  The routing predicates of the
population are in tests/test_multibinary_ppo_cpu.py."""

import copy
import ctypes
import os

import pytest

NS = [1, 2, 5, 16, 17, 32]  # tests/multibinary_twin.py's NS, restated


@pytest.fixture(scope="module")
def lib():
    from agilerl_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load(require_gpu=False)


def _spec(n, **kw):
    from agilerl_amd.population.nets import MultiBinaryActorCriticSpec

    return MultiBinaryActorCriticSpec(obs_dim=8, n_actions=n, **kw)


def _desc(spec):
    from agilerl_amd.population.learner import layer_list

    d = layer_list(spec)
    assert d is not None
    return d


@pytest.mark.parametrize("n", NS)
def test_check_admits_the_default_layer_list_at_every_width(lib, n):
    spec = _spec(n)
    d = _desc(spec)
    assert lib.agx_ppo_bern_graph_check(ctypes.byref(d)) == 0, lib.agx_last_error()
    assert spec.bern_learn_descriptor() is not None and spec.bern_descriptor() is not None
    ws = lib.agx_ppo_learn_bern_graph_workspace_bytes(ctypes.byref(d), 2, 64, 1, 16)
    # the target and mask words are the categorical gather's: the categorical learner's workspace
    assert ws > 0 and ws == lib.agx_ppo_learn_graph_workspace_bytes(ctypes.byref(d), 2, 64, 1, 16)
    assert lib.agx_ppo_act_bern_graph_workspace_bytes(ctypes.byref(d), 2, 21) \
        == lib.agx_ppo_act_graph_workspace_bytes(ctypes.byref(d), 2, 21) > 0


def test_check_rejects_thirty_three_bits_and_none(lib):
    from agilerl_amd.population.nets import ActorCriticSpec

    for n in (33, 0):
        d = copy.deepcopy(_desc(ActorCriticSpec(obs_dim=8, n_actions=32)))
        d.n_actions = n
        d.layers[d.actor_out].fout = n
        assert lib.agx_ppo_bern_graph_check(ctypes.byref(d)) == -1
        assert lib.agx_last_error()
        assert lib.agx_ppo_learn_bern_graph_workspace_bytes(ctypes.byref(d), 2, 64, 1, 16) == 0
        assert lib.agx_ppo_act_bern_graph_workspace_bytes(ctypes.byref(d), 2, 21) == 0


def test_check_rejects_what_the_graph_check_rejects(lib):
    d = copy.deepcopy(_desc(_spec(5)))
    d.layers[d.actor_out].relu = 1  # the output layers must be plain Linear
    assert lib.agx_ppo_bern_graph_check(ctypes.byref(d)) == -1
    assert b"output layers" in lib.agx_last_error()
    assert lib.agx_ppo_graph_check(ctypes.byref(d)) == -1
    assert lib.agx_ppo_bern_graph_check(None) == -1
    assert lib.agx_ppo_learn_bern_graph_workspace_bytes(ctypes.byref(d), 2, 64, 1, 16) == 0


def test_learn_rejects_a_bad_net_before_any_gpu_work(lib):
    from agilerl_amd.population.learner import AgxPPOLearnArgs

    d = copy.deepcopy(_desc(_spec(5)))
    d.layers[d.actor_out].relu = 1
    args = AgxPPOLearnArgs()
    assert lib.agx_ppo_learn_bern_graph(ctypes.byref(d), ctypes.byref(args), 16, None) == -1
    assert b"output layers" in lib.agx_last_error()
    assert lib.agx_ppo_learn_bern_graph(None, ctypes.byref(args), 16, None) == -1


def test_rejected_layer_list_falls_back():
    """A LayerNorm layer wider than the graph learner takes: no descriptor, no error."""
    spec = _spec(5, encoder_hidden=[1024], latent_dim=32)
    assert spec.bern_learn_descriptor() is None
