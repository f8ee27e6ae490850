"""agx_ppo_multi_graph_check (include/agx_multi.h) and the routing switch of
the fused multi-categorical learner.  The check plans on the host and makes no
HIP call, and the routing predicates of PPOPopulation only read attributes, so
everything here runs without a GPU (as tests/test_gauss_learner_cpu.py)."""

import copy
import ctypes
import os

import pytest

# tests/multidisc_twin.py's NVECS, restated
NVECS = [(2,), (3, 2), (5, 1, 4), (16, 16), (7, 20, 5), (2,) * 16, (32,)]
IDS = ["x".join(map(str, n)) if len(n) < 6 else f"{n[0]}x{len(n)}times" for n in NVECS]


@pytest.fixture(scope="module")
def lib():
    from agilerl_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load(require_gpu=False)


def _spec(nvec, **kw):
    from agilerl_amd.population.nets import MultiDiscreteActorCriticSpec

    return MultiDiscreteActorCriticSpec(obs_dim=8, n_actions=int(sum(nvec)), nvec=tuple(nvec), **kw)


def _desc(spec):
    from agilerl_amd.population.learner import layer_list

    d = layer_list(spec)
    assert d is not None
    return d


def _head(nvec, K=None):
    """agx_multi_head with any K / sizes (kernels.multi_head validates; the check under test must)."""
    from agilerl_amd._lib import AgxMultiHead

    h = AgxMultiHead()
    h.K = len(nvec) if K is None else K
    for k, n in enumerate(nvec):
        h.nvec[k] = n
    return h


@pytest.mark.parametrize("nvec", NVECS, ids=IDS)
def test_check_admits_the_default_layer_list_with_every_head(lib, nvec):
    spec = _spec(nvec)
    d = _desc(spec)
    assert lib.agx_ppo_multi_graph_check(ctypes.byref(d), _head(nvec)) == 0, lib.agx_last_error()
    assert lib.agx_ppo_multi_graph_check(ctypes.byref(d), spec.multi_head()) == 0
    assert spec.multi_learn_descriptor() is not None
    assert lib.agx_ppo_learn_multi_graph_workspace_bytes(ctypes.byref(d), _head(nvec), 2, 64, 1, 16) > 0


@pytest.mark.parametrize("name,nvec,K,word", [
    ("no_components", (), 0, b"components"),
    ("an_empty_component", (3, 0, 2), None, b"choices"),
    ("sum_is_not_n_actions", (3, 3), None, b"nvec sums to 6"),
])
def test_check_rejects_a_bad_head(lib, name, nvec, K, word):
    d = _desc(_spec((3, 2)))
    h = _head(nvec, K)
    assert lib.agx_ppo_multi_graph_check(ctypes.byref(d), h) == -1
    err = lib.agx_last_error()
    assert err and word in err, err
    assert lib.agx_ppo_learn_multi_graph_workspace_bytes(ctypes.byref(d), h, 2, 64, 1, 16) == 0


def test_check_rejects_thirty_three_logits(lib):
    """sum n_k = 33: over the head's limit, whatever the layer list says."""
    from agilerl_amd.population.nets import ActorCriticSpec

    d = _desc(ActorCriticSpec(obs_dim=8, n_actions=33))
    h = _head((16, 17))
    assert lib.agx_ppo_multi_graph_check(ctypes.byref(d), h) == -1
    assert lib.agx_last_error()
    assert lib.agx_ppo_learn_multi_graph_workspace_bytes(ctypes.byref(d), h, 2, 64, 1, 16) == 0
    d32 = copy.deepcopy(_desc(_spec((16, 16))))
    assert lib.agx_ppo_multi_graph_check(ctypes.byref(d32), h) == -1  # 33 logits against a 32-logit actor
    assert b"33" in lib.agx_last_error()


def test_check_rejects_what_the_graph_check_rejects(lib):
    spec = _spec((3, 2))
    d = copy.deepcopy(_desc(spec))
    d.layers[d.actor_out].relu = 1  # the output layers must be plain Linear
    assert lib.agx_ppo_multi_graph_check(ctypes.byref(d), spec.multi_head()) == -1
    assert b"output layers" in lib.agx_last_error()
    assert lib.agx_ppo_multi_graph_check(None, spec.multi_head()) == -1


def test_learn_rejects_a_bad_head_before_any_gpu_work(lib):
    from agilerl_amd.population.learner import AgxPPOLearnArgs

    d = _desc(_spec((3, 2)))
    args = AgxPPOLearnArgs()
    assert lib.agx_ppo_learn_multi_graph(ctypes.byref(d), _head((3, 3)), ctypes.byref(args), 16, None) == -1
    assert b"nvec" in lib.agx_last_error()
    assert lib.agx_ppo_learn_multi_graph(ctypes.byref(d), _head((), 0), ctypes.byref(args), 16, None) == -1
    assert b"components" in lib.agx_last_error()


# ---- routing ----------------------------------------------------------------------------- #
def _bare_population(spec, fused=True, multi_fused=False):
    """A PPOPopulation with only what the routing predicates read: its
    constructor allocates the rollout on a device, which this machine may not
    have."""
    from agilerl_amd.population.ppo_pop import PPOPopulation

    pop = PPOPopulation.__new__(PPOPopulation)
    pop.spec = spec
    head = getattr(spec, "head", "categorical")
    pop.gaussian, pop.multidiscrete = head == "gaussian", head == "multidiscrete"
    pop.fused, pop.multi_fused = fused, multi_fused
    pop._desc = pop._gdesc = pop._edesc = pop._gauss = pop._glearn = pop._mlearn = pop._multi = pop._mhead = None
    return pop


def test_default_multidiscrete_population_keeps_the_autograd_learner(monkeypatch):
    monkeypatch.delenv("AGX_MULTI_FUSED", raising=False)
    pop = _bare_population(_spec((3, 2)))
    assert pop.multi_learn_descriptor() is None and not pop._fused_learner()
    monkeypatch.setenv("AGX_MULTI_FUSED", "0")
    assert pop.multi_learn_descriptor() is None and not pop._fused_learner()


def test_keyword_and_environment_switch_the_fused_learner_on(monkeypatch):
    monkeypatch.delenv("AGX_MULTI_FUSED", raising=False)
    pop = _bare_population(_spec((3, 2)), multi_fused=True)
    assert pop.multi_learn_descriptor() is not None and pop._fused_learner()
    assert pop.multi_learn_descriptor() is pop.multi_learn_descriptor()  # made once
    assert pop.learn_descriptor() is None and pop.fused_descriptor() is None
    pop = _bare_population(_spec((3, 2)))
    monkeypatch.setenv("AGX_MULTI_FUSED", "1")
    assert pop.multi_learn_descriptor() is not None and pop._fused_learner()


def test_fused_false_wins_over_both_switches(monkeypatch):
    monkeypatch.setenv("AGX_MULTI_FUSED", "1")
    pop = _bare_population(_spec((3, 2)), fused=False, multi_fused=True)
    assert pop.multi_learn_descriptor() is None and not pop._fused_learner()


def test_rejected_layer_list_falls_back(monkeypatch):
    """A LayerNorm layer wider than the graph learner takes: no descriptor, no error."""
    monkeypatch.setenv("AGX_MULTI_FUSED", "1")
    spec = _spec((3, 2), encoder_hidden=[1024], latent_dim=32)
    assert spec.multi_learn_descriptor() is None
    pop = _bare_population(spec, multi_fused=True)
    assert pop.multi_learn_descriptor() is None and not pop._fused_learner()


def test_other_heads_never_get_the_multi_descriptor(monkeypatch):
    from agilerl_amd.population.nets import ActorCriticSpec, GaussianActorCriticSpec

    monkeypatch.setenv("AGX_MULTI_FUSED", "1")
    for spec in (ActorCriticSpec(obs_dim=8, n_actions=5), GaussianActorCriticSpec(obs_dim=8, n_actions=5)):
        pop = _bare_population(spec, multi_fused=True)
        assert pop.multi_learn_descriptor() is None
        assert pop._fused_learner()  # their own fused learners, untouched by the switch
