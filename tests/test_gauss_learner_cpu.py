"""agx_ppo_gauss_graph_check (include/agx_gauss.h): the host-only admission
test of the fused Gaussian learner.  It plans on the host and makes no HIP
call, so everything here runs without a GPU (as test_abi.py's
test_error_path_without_gpu_work: a HIP call on a machine without a device
would fail the call, not return the verdicts asserted below)."""

import copy
import ctypes
import os

import pytest

SHAPES = {
    "default": dict(),
    "latent_56_two_layer_head": dict(latent_dim=56, actor_hidden=[48, 40]),
    "no_layer_norm": dict(encoder_hidden=[64, 64], latent_dim=40, actor_hidden=[48], critic_hidden=[64],
                          layer_norm=False),
    "own_critic_encoder": dict(encoder_hidden=[64], latent_dim=48, actor_hidden=[64], critic_hidden=[32],
                               share_encoders=False),
}


@pytest.fixture(scope="module")
def lib():
    from agilerl_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load(require_gpu=False)


def _spec(A, shape="default"):
    from agilerl_amd.population.nets import GaussianActorCriticSpec

    return GaussianActorCriticSpec(obs_dim=8, n_actions=A, **SHAPES[shape])


def _desc(spec):
    from agilerl_amd.population.learner import layer_list

    d = layer_list(spec)
    assert d is not None
    return d


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("A", [1, 6, 17, 32])
def test_check_accepts_a_gaussian_specs_descriptor(lib, A, shape):
    spec = _spec(A, shape)
    d = _desc(spec)
    assert 0 <= spec.log_std and spec.log_std + A <= spec.actor_end
    assert lib.agx_ppo_gauss_graph_check(ctypes.byref(d), spec.log_std) == 0, lib.agx_last_error()
    assert spec.gauss_learn_descriptor() is not None


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_check_rejects_a_shifted_log_std(lib, shape):
    spec = _spec(6, shape)
    d = _desc(spec)
    for off in (spec.log_std - 1, spec.log_std + 1):
        assert lib.agx_ppo_gauss_graph_check(ctypes.byref(d), off) == -1
        assert b"log_std" in lib.agx_last_error()
    assert lib.agx_ppo_gauss_graph_check(ctypes.byref(d), -1) == -1
    assert lib.agx_ppo_gauss_graph_check(ctypes.byref(d), spec.n_params) == -1


def test_check_rejects_thirty_three_dimensions(lib):
    spec = _spec(33)
    d = _desc(spec)
    assert lib.agx_ppo_gauss_graph_check(ctypes.byref(d), spec.log_std) == -1
    assert b"33 actions" in lib.agx_last_error()
    assert spec.gauss_learn_descriptor() is None


def test_check_rejects_a_row_without_a_gap(lib):
    """n_params = what the layers cover (a categorical row): no room for log_std."""
    spec = _spec(6)
    d = copy.deepcopy(_desc(spec))
    d.n_params = spec.n_params - 6
    assert lib.agx_ppo_gauss_graph_check(ctypes.byref(d), spec.log_std) == -1
    err = lib.agx_last_error()
    assert err and b"parameters" in err


def test_check_rejects_log_std_in_the_critic_group(lib):
    """A gap after critic_start: the learner clips log_std with the actor group."""
    from agilerl_amd.population.learner import graph_descriptor
    from agilerl_amd.population.nets import ActorCriticSpec

    cat = ActorCriticSpec(obs_dim=8, n_actions=6)
    d = copy.deepcopy(graph_descriptor(cat))
    d.n_params = cat.n_params + 6  # six floats no layer owns, behind the critic
    assert lib.agx_ppo_gauss_graph_check(ctypes.byref(d), cat.n_params) == -1
    assert b"actor group" in lib.agx_last_error()


def test_check_rejects_what_the_graph_check_rejects(lib):
    spec = _spec(6)
    d = copy.deepcopy(_desc(spec))
    d.layers[d.actor_out].relu = 1  # the output layers must be plain Linear
    assert lib.agx_ppo_gauss_graph_check(ctypes.byref(d), spec.log_std) == -1
    assert b"output layers" in lib.agx_last_error()
    assert lib.agx_ppo_gauss_graph_check(None, 0) == -1


def test_learn_rejects_bad_arguments_before_any_gpu_work(lib):
    """The learn call validates the net and the argument block on the host."""
    from agilerl_amd.population.learner import AgxPPOLearnArgs

    spec = _spec(6)
    d = _desc(spec)
    args = AgxPPOLearnArgs()
    assert lib.agx_ppo_learn_gauss_graph(ctypes.byref(d), spec.log_std + 1, ctypes.byref(args), 16, None) == -1
    assert b"log_std" in lib.agx_last_error()
    args.action_masks = 16
    assert lib.agx_ppo_learn_gauss_graph(ctypes.byref(d), spec.log_std, ctypes.byref(args), 16, None) == -1
    assert b"action masks" in lib.agx_last_error()
    assert lib.agx_ppo_learn_gauss_graph_workspace_bytes(ctypes.byref(d), spec.log_std + 1, 2, 64, 1, 16) == 0
