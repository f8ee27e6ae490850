"""The fused learner's partner exchange: the tagged-word second hand-off, the
per-layer vector-gradient publish and the store-not-accumulate column partials
(DESIGN.md §5).  Same bits under load and under write-through stores, partners
without a sub-batch, the ragged tail, a workspace reused by several learn()
calls, and several sub-batches per partner."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _pop(P=3, N=16, learn_step=128, batch=64, epochs=1, seed=0, **kw):
    from agilerl_amd.population.nets import ActorCriticSpec
    from agilerl_amd.population.ppo_pop import PPOPopulation

    spec = ActorCriticSpec(obs_dim=8, n_actions=4, **kw)
    pop = PPOPopulation(spec, P, N, learn_step=learn_step, batch_size=batch, lr=1e-3, update_epochs=epochs,
                        seeds=[seed + i for i in range(P)], device=DEV, fused=True)
    g = torch.Generator(device=DEV).manual_seed(seed + 99)
    pop.obs.copy_(torch.randn(pop.obs.shape, device=DEV, generator=g))
    pop.actions.copy_(torch.randint(0, 4, pop.actions.shape, device=DEV, generator=g))
    pop.rewards.copy_(torch.randn(pop.rewards.shape, device=DEV, generator=g))
    pop.dones.copy_((torch.rand(pop.dones.shape, device=DEV, generator=g) < 0.05).to(torch.uint8))
    with torch.no_grad():
        logits, value = spec.forward(pop.params.data, pop.obs.view(P, -1, 8))
        lp = torch.log_softmax(logits, -1).gather(-1, pop.actions.view(P, -1, 1)).squeeze(-1)
    pop.values.copy_(value.view_as(pop.values) + 0.1 * torch.randn(pop.values.shape, device=DEV, generator=g))
    pop.log_probs.copy_(lp.view_as(pop.log_probs) + 0.05 * torch.randn(pop.log_probs.shape, device=DEV, generator=g))
    last_obs = torch.randn(P, N, 8, device=DEV, generator=g)
    last_done = torch.zeros(P, N, dtype=torch.uint8, device=DEV)
    pop.finish_rollout(last_obs, last_done)
    return pop


def _clone_state(pop):
    return (pop.params.data.clone(), pop.opt.exp_avg.clone(), pop.opt.exp_avg_sq.clone(),
            pop.advantages.clone(), pop.opt.steps.clone())


def _restore(pop, st):
    pop.params.data.copy_(st[0])
    pop.opt.exp_avg.copy_(st[1])
    pop.opt.exp_avg_sq.copy_(st[2])
    pop.advantages.copy_(st[3])
    pop.opt.steps.copy_(st[4])


def _bits(pop, loss):
    torch.cuda.synchronize()
    assert not pop._fused.timed_out(pop)
    return {"params": pop.params.data.cpu().numpy().copy(), "exp_avg": pop.opt.exp_avg.cpu().numpy().copy(),
            "exp_avg_sq": pop.opt.exp_avg_sq.cpu().numpy().copy(), "loss": loss.cpu().numpy().copy(),
            "approx_kl": pop._fused.kl.cpu().numpy().copy()}


def _check_against_torch(pop, st, perms, what):
    """fused_learn against the torch learner from the saved state ``st``
    (tolerances of test_fused_learner_partner_split_consistent's one-update case)."""
    from agilerl_amd.population.learner import fused_learn

    _restore(pop, st)
    loss_t = pop._learn_torch(perms).clone().cpu().numpy()
    m_t = pop.opt.exp_avg.clone().cpu().numpy()
    kl_t = pop.last_kl.clone().cpu().numpy()
    _restore(pop, st)
    loss_f = fused_learn(pop, perms).clone()
    torch.cuda.synchronize()
    assert not pop._fused.timed_out(pop)
    m_f = pop.opt.exp_avg.cpu().numpy()
    kl_f = pop._fused.kl.cpu().numpy()
    scale = np.abs(m_t).max()
    err_l = np.abs(loss_f.cpu().numpy() - loss_t).max()
    err_m = np.abs(m_f - m_t).max()
    print(f"{what}: max |loss diff| {err_l:.3e}, max |m diff| {err_m:.3e} (max |m| {scale:.3e}), "
          f"approx_kl {kl_f} vs {kl_t}")
    np.testing.assert_allclose(loss_f.cpu().numpy(), loss_t, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(m_f, m_t, rtol=1e-4, atol=1e-6 * scale)
    # the approx-KL word travels with the loss word.  Each row's term
    # (ratio - 1) - log(ratio) ~ 1e-3 cancels from f32 values near 1, so it is
    # good to ~1e-7 absolute, 1e-4 relative; 1e-2 leaves room for the two
    # learners' parameters drifting apart over the updates
    np.testing.assert_allclose(kl_f, kl_t, rtol=1e-2, atol=1e-6)


def test_same_bits_idle_loaded_and_write_through(monkeypatch):
    """16 partners x one 8-row sub-batch, 4 updates: parameters, both Adam
    moments and the loss have the same bits twice on an idle device, with a
    256 MiB copy looping on a second stream (uneven load, the consumers'
    L1 warm), and with write-through stores."""
    from agilerl_amd import _lib
    from agilerl_amd.population.learner import fused_learn

    np.random.seed(3)
    pop = _pop(P=2, N=16, learn_step=256, batch=128, epochs=2, seed=21)
    st = _clone_state(pop)
    perms = pop.permutations()

    def run():
        _restore(pop, st)
        return _bits(pop, fused_learn(pop, perms))

    runs = {"idle 1": run(), "idle 2": run()}
    src = torch.zeros(256 << 20, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    _restore(pop, st)
    for _ in range(8):  # ~0.1 ms each: in flight before and all through the learn
        _lib.call("agx_debug_stream", src.data_ptr(), dst.data_ptr(), src.numel(), 0, 256, _lib.stream(side))
    loss = fused_learn(pop, perms)
    for _ in range(4):
        _lib.call("agx_debug_stream", src.data_ptr(), dst.data_ptr(), src.numel(), 0, 256, _lib.stream(side))
    runs["loaded"] = _bits(pop, loss)
    monkeypatch.setenv("AGX_LEARN_WRITETHROUGH", "1")
    runs["write-through"] = run()
    ref = runs["idle 1"]
    for name, r in runs.items():
        for k in ref:
            assert r[k].tobytes() == ref[k].tobytes(), f"{k} differs: {name} vs idle 1"


def test_idle_partners_ragged_tail_padded_grid():
    """P = 3 (the grid is padded to 8 agents), minibatches of 72, 72 and 64 rows
    over 9 partners: ragged nine-partner updates, then one where the last
    partner has no sub-batch and publishes zeros."""
    np.random.seed(5)
    pop = _pop(P=3, N=16, learn_step=208, batch=72, epochs=1, seed=31)
    _check_against_torch(pop, _clone_state(pop), pop.permutations(), "idle partner / ragged")


def test_three_learns_on_one_workspace():
    """The tagged words are zeroed again on every launch: three learn() calls in
    a row on one workspace, each with its own minibatch order."""
    np.random.seed(7)
    pop = _pop(P=2, N=16, learn_step=256, batch=128, epochs=2, seed=41)
    st = _clone_state(pop)
    for i in range(3):
        _check_against_torch(pop, st, pop.permutations(), f"learn {i}")


def test_several_sub_batches_per_partner(monkeypatch):
    """16-row sub-batches over 4 partners, two per partner and update: the
    accumulate form of the column partials and the end-of-minibatch vector dump
    of all but the last sub-batch."""
    monkeypatch.setenv("AGX_LEARN_SB", "16")
    monkeypatch.setenv("AGX_LEARN_SPLIT", "4")
    np.random.seed(9)
    pop = _pop(P=2, N=16, learn_step=256, batch=128, epochs=2, seed=51)
    _check_against_torch(pop, _clone_state(pop), pop.permutations(), "SB=16 x 4 partners")
