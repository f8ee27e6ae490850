"""The gather prologue of the runtime-shape fused learners (ppo_gather.h), head
by head: the permutation guard, the counter reset and the per-agent epoch skip,
which only the compiled-shape categorical learner reached before
(tests/test_learner_parity_gpu.py::test_bad_permutation_index_raises).

Populations and rollouts are the neighbours' (tests/test_graph_learner_gpu.py
and the three head learner files) at their smallest: P = 3, 16 envs, S = 64,
batch 32, 2 epochs, obs_dim 8, the "latent_56" layer shape; 4 categorical
actions, A = 3, nvec = (3, 2), n = 5."""

import pytest
import torch

from tests import test_gauss_learner_gpu as TG
from tests import test_graph_learner_gpu as TC
from tests import test_multibinary_learner_gpu as TB
from tests import test_multidisc_learner_gpu as TM

pytestmark = pytest.mark.gpu

KW = dict(P=3, N=16, batch=32, epochs=2, seed=7)
# head -> (the population with a filled rollout, the learner class its learn() must run)
HEADS = {
    "categorical": (lambda S: TC._pop("latent_56", A=4, learn_step=S, **KW), "GraphLearner"),
    "gauss": (lambda S: TG._pop("latent_56", A=3, learn_step=S, **KW), "GaussGraphLearner"),
    "multi": (lambda S: TM._pop("latent_56", nvec=(3, 2), learn_step=S, **KW), "MultiGraphLearner"),
    "bern": (lambda S: TB._pop("latent_56", n=5, learn_step=S, **KW), "BernGraphLearner"),
}
# graph_learner.hip graph_split: batch 32 is two few-row partners of 16 rows by default
FORMS = {"default": {}, "general": {"AGX_GRAPH_FEW": "0"}, "one_workgroup": {"AGX_GRAPH_SPLIT": "1"}}
ERR_PERM = 2  # AGX_LEARN_ERR_PERM


def _make(head, form, monkeypatch, S=64):
    for k in ("AGX_GRAPH_FEW", "AGX_GRAPH_SPLIT", "AGX_GRAPH_ROWS", "AGX_GAUSS_FUSED", "AGX_MULTI_FUSED",
              "AGX_BERN_FUSED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    pop = HEADS[head][0](S)
    assert pop.S == S and pop.update_epochs == 2
    return pop


def _learn(pop, head, perms):
    """One fused learn -> (params, exp_avg, exp_avg_sq, loss), copies; the error word is left as the learn set it."""
    from agilerl_amd.population.learner import fused_learn

    loss = fused_learn(pop, perms).clone()
    torch.cuda.synchronize()
    assert type(pop._fused).__name__ == HEADS[head][1]
    return pop.params.data.clone(), pop.opt.exp_avg.clone(), pop.opt.exp_avg_sq.clone(), loss


def _same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("bad", ["past_S", "negative"])
@pytest.mark.parametrize("form", ["one_workgroup", "default"])
@pytest.mark.parametrize("head", list(HEADS))
def test_bad_permutation_index_is_flagged_and_gathers_row_0(head, form, bad, monkeypatch):
    """One index of one (epoch, agent) row outside [0, S): the error word gets
    the permutation bit, check_errors raises and resets it, and the learn is
    bit for bit the learn with 0 at that index (the guard gathers row 0: the
    heads' determinism tests establish run-to-run bit equality in these forms).
    The next learn with valid permutations raises nothing."""
    from agilerl_amd import _lib

    pop = _make(head, form, monkeypatch)
    st = TC._state(pop)
    perms = pop.permutations().clone()
    e, p, j = 1, 2, 17
    wrong, zero = perms.clone(), perms.clone()
    wrong[e, p, j] = pop.S + 7 if bad == "past_S" else -3
    zero[e, p, j] = 0
    got = _learn(pop, head, wrong)
    assert int(pop.err_word.item()) & ERR_PERM
    with pytest.raises(_lib.AgxError, match="permutation"):
        pop.check_errors()
    assert int(pop.err_word.item()) == 0
    TC._restore(pop, st)
    want = _learn(pop, head, zero)
    pop.check_errors()
    _same(got, want)
    assert not torch.equal(want[0], st[0])
    _learn(pop, head, perms)
    pop.check_errors()


@pytest.mark.parametrize("S", [64, 512])  # one and two gather blocks per (epoch, agent) row
def test_counters_are_reset_on_every_launch(S, monkeypatch):
    """The general partnered form counts arrivals in workspace words the gather
    zeroes: a second learn() on the same learner from the same state gives the
    first one's bits, and no partner timed out in either."""
    pop = _make("gauss", "general", monkeypatch, S=S)
    st = TC._state(pop)
    perms = pop.permutations().clone()
    first = _learn(pop, "gauss", perms)
    learner = pop._fused
    assert not learner.timed_out(pop)
    pop.check_errors()
    TC._restore(pop, st)
    second = _learn(pop, "gauss", perms)
    assert pop._fused is learner and not learner.timed_out(pop)
    pop.check_errors()
    _same(first, second)
    assert not torch.equal(first[0], st[0])


@pytest.mark.parametrize("head", list(HEADS))
def test_rows_past_an_agents_own_epochs_are_not_read(head, monkeypatch):
    """An agent with update_epochs = 1 of the population's 2: its second-epoch
    permutation row, filled with S + 7, is never read: no error bit, and the
    results are those with a valid row there."""
    pop = _make(head, "default", monkeypatch)
    pop.set_agent_hparam(2, "update_epochs", 1)
    st = TC._state(pop)
    perms = pop.permutations().clone()
    junk = perms.clone()
    junk[1, 2, :] = pop.S + 7
    got = _learn(pop, head, junk)
    assert int(pop.err_word.item()) == 0
    assert pop._fused.epochs_run.tolist() == [2, 2, 1]
    TC._restore(pop, st)
    want = _learn(pop, head, perms)
    assert int(pop.err_word.item()) == 0
    _same(got, want)
