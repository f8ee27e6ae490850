"""Argument validation of the persistent rollout / evaluation entry points of
the Gaussian, multi-categorical and Bernoulli heads (include/agx_gauss.h,
agx_multi.h, agx_bernoulli.h): bad arguments return AGX_EINVAL with a reason
before any HIP call, so these run without a GPU."""

import ctypes

import pytest

EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    import os

    from agilerl_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load(require_gpu=False)


class _Args:
    """Host stand-ins for every pointer of a launch: validation never reads
    through them (it ends before the launch)."""

    def __init__(self, T=3):
        from agilerl_amd.population.runner import AgxRolloutIO

        self.buf = (ctypes.c_uint8 * 4096)()
        self.p = ctypes.addressof(self.buf)
        self.ios = (AgxRolloutIO * T)()
        for t in range(T):
            self.ios[t].stage_obs = self.p
        self.T = T


def _gauss():
    from agilerl_amd.population.nets import GaussianActorCriticSpec

    spec = GaussianActorCriticSpec(obs_dim=8, n_actions=6)
    return spec, spec.gauss_descriptor()


def _multi(nvec=(3, 3)):
    from agilerl_amd.population.nets import MultiDiscreteActorCriticSpec

    spec = MultiDiscreteActorCriticSpec(obs_dim=8, n_actions=int(sum(nvec)), nvec=tuple(nvec))
    return spec, spec.multi_descriptor()


def _bern():
    from agilerl_amd.population.nets import MultiBinaryActorCriticSpec

    spec = MultiBinaryActorCriticSpec(obs_dim=8, n_actions=4)
    return spec, spec.bern_descriptor()


def _rollout_calls(lib, a):
    """name -> call(net, ios, nsteps, clip_low) of the three rollout entry points on good arguments otherwise."""
    gs, gd = _gauss()
    ms, md = _multi()
    _, bd = _bern()
    tail = (a.p, a.p, 1.0, a.p, None)  # args_host, ctl, timeout_s, workspace, stream
    return {
        "agx_ppo_rollout_gauss_graph_persistent": lambda net=ctypes.byref(gd), ios=a.ios, n=a.T, lo=None:
            lib.agx_ppo_rollout_gauss_graph_persistent(net, gs.log_std, 2, 24, a.p, ios, n, 0, 1, 0, lo, None, *tail),
        "agx_ppo_rollout_multi_graph_persistent": lambda net=ctypes.byref(md), ios=a.ios, n=a.T, lo=None:
            lib.agx_ppo_rollout_multi_graph_persistent(net, ms.multi_head(), 2, 24, a.p, ios, n, 0, 1, 0, *tail),
        "agx_ppo_rollout_bern_graph_persistent": lambda net=ctypes.byref(bd), ios=a.ios, n=a.T, lo=None:
            lib.agx_ppo_rollout_bern_graph_persistent(net, 2, 24, a.p, ios, n, 0, 1, 0, *tail),
    }


def _eval_calls(lib, a):
    """name -> call(net, stage_obs, nsteps) of the three evaluation entry points."""
    gs, gd = _gauss()
    ms, md = _multi()
    _, bd = _bern()
    tail = (a.p, a.p, 1.0, a.p, None)
    return {
        "agx_ppo_eval_gauss_graph_persistent": lambda net=ctypes.byref(gd), obs=a.p, n=4:
            lib.agx_ppo_eval_gauss_graph_persistent(net, gs.log_std, 2, 24, a.p, obs, a.p, None, None, None, n, 0, 1,
                                                    0, *tail),
        "agx_ppo_eval_multi_graph_persistent": lambda net=ctypes.byref(md), obs=a.p, n=4:
            lib.agx_ppo_eval_multi_graph_persistent(net, ms.multi_head(), 2, 24, a.p, obs, a.p, None, n, 0, 1, 0,
                                                    *tail),
        "agx_ppo_eval_bern_graph_persistent": lambda net=ctypes.byref(bd), obs=a.p, n=4:
            lib.agx_ppo_eval_bern_graph_persistent(net, 2, 24, a.p, obs, a.p, None, n, 0, 1, 0, *tail),
    }


ROLLOUTS = ["agx_ppo_rollout_gauss_graph_persistent", "agx_ppo_rollout_multi_graph_persistent",
            "agx_ppo_rollout_bern_graph_persistent"]
EVALS = ["agx_ppo_eval_gauss_graph_persistent", "agx_ppo_eval_multi_graph_persistent",
         "agx_ppo_eval_bern_graph_persistent"]


@pytest.mark.parametrize("name", ROLLOUTS)
def test_rollout_entry_point_rejects_bad_arguments(lib, name):
    a = _Args()
    call = _rollout_calls(lib, a)[name]
    assert call(net=None) == EINVAL and name.encode() in lib.agx_last_error()
    assert call(ios=None) == EINVAL and b"bad arguments" in lib.agx_last_error()
    assert call(n=0) == EINVAL and b"bad arguments" in lib.agx_last_error()
    a.ios[1].stage_obs = None  # a step without its observation staging
    assert call() == EINVAL and b"stage_obs" in lib.agx_last_error()
    a.ios[1].stage_obs = a.p
    a.ios[1].stage_mask = a.p  # the head launches take no legal-action mask
    assert call() == EINVAL and b"mask" in lib.agx_last_error()


@pytest.mark.parametrize("name", EVALS)
def test_eval_entry_point_rejects_bad_arguments(lib, name):
    call = _eval_calls(lib, _Args())[name]
    assert call(net=None) == EINVAL and name.encode() in lib.agx_last_error()
    assert call(obs=None) == EINVAL and b"bad arguments" in lib.agx_last_error()
    assert call(n=0) == EINVAL and b"bad arguments" in lib.agx_last_error()


def test_head_rules_of_the_per_step_entry_points_hold(lib):
    """The head's own rules, as agx_ppo_act_gauss_graph / _multi_graph state them."""
    a = _Args()
    assert _rollout_calls(lib, a)["agx_ppo_rollout_gauss_graph_persistent"](lo=a.p) == EINVAL
    assert b"clip_low and clip_high" in lib.agx_last_error()
    gs, gd = _gauss()
    tail = (a.p, a.p, 1.0, a.p, None)
    rc = lib.agx_ppo_rollout_gauss_graph_persistent(ctypes.byref(gd), gs.n_params, 2, 24, a.p, a.ios, a.T, 0, 1, 0,
                                                    None, None, *tail)
    assert rc == EINVAL and b"log_std" in lib.agx_last_error()
    ms, md = _multi()
    other = _multi((2, 3))[0].multi_head()  # 5 logits against the net's 6
    rc = lib.agx_ppo_rollout_multi_graph_persistent(ctypes.byref(md), other, 2, 24, a.p, a.ios, a.T, 0, 1, 0, *tail)
    assert rc == EINVAL and b"nvec sums to 5" in lib.agx_last_error()
    rc = lib.agx_ppo_eval_multi_graph_persistent(ctypes.byref(md), other, 2, 24, a.p, a.p, a.p, None, 4, 0, 1, 0,
                                                 *tail)
    assert rc == EINVAL and b"nvec sums to 5" in lib.agx_last_error()
