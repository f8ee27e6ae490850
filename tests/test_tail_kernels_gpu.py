"""The kernels on the tail of every learn() on the paths the other tests do not
reach: agx_clip_adam (norm pre-reduction with an active clip, the ``active``
mask, no clip, 1 / 8 groups, other betas / eps / starting steps), agx_polyak's
grid-stride loop, agx_td_target over B around the 256-row block with ties,
NaN rows and no loss, and the loss sum shared with the critic-target kernels
over more than 1024 block partials.  References: tests/tail_twin.py (pinned on
the CPU by tests/test_tail_twin_cpu.py) and tests/td3_twin.py."""

import numpy as np
import pytest
import torch

from tests import tail_twin as TT
from tests import td3_twin

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def K():
    from agilerl_amd import kernels

    return kernels


def _agx_error():
    from agilerl_amd import _lib

    return _lib.AgxError


# --------------------------------------------------------------------------- #
# clip + Adam                                                                 #
# --------------------------------------------------------------------------- #
def _optimizer(c):
    opt = K().ClipAdam(T(c["p0"]), c["offsets"], torch.from_numpy(c["lr"]), betas=c["betas"], eps=c["eps"],
                       max_norm=c["max_norm"])
    opt.exp_avg.copy_(T(c["m0"]))
    opt.exp_avg_sq.copy_(T(c["v0"]))
    opt.steps.copy_(T(c["steps0"]))
    return opt


def _state(opt):
    torch.cuda.synchronize()
    return [x.cpu().clone() for x in (opt.params, opt.exp_avg, opt.exp_avg_sq, opt.grads, opt.steps)]


NAMES = ("params", "exp_avg", "exp_avg_sq", "grads")


def _run_case(name):
    """Four updates of the case through kernels.ClipAdam beside the twins.
    After every update, elementwise for params, exp_avg, exp_avg_sq and the
    grads buffer:
        |kernel - f64| <= max(1e-5 |f64| + 1e-6, 4 |torch32 - f64|)
    (the bar of test_clip_adam_matches_torch, or four times what the
    reference's own float32 arithmetic loses), and steps exactly.  On top, two
    bars from the number format alone, since 1e-6 is above most of these
    values: the clipped gradient is g * (max_norm / (norm + 1e-6)) — the norm
    from a float64 sum, so four float32 roundings, 4 * 2^-24 = 2.4e-7 relative
    — bar 1e-6 |f64|; exp_avg_sq is a sum of non-negative terms (no
    cancellation), each step adding three roundings to twice the gradient's
    error: below 4 * (2 * 2.4e-7 + 3 * 6e-8) = 2.7e-6 after four steps — bar
    4e-6 |f64|.  An agent masked out keeps the bits of all four rows and its
    step count.  -> the per-update states of the kernel."""
    c, s64, s32 = TT.adam_twins(name)
    assert TT.adam_norms_off_the_branch(c)
    opt = _optimizer(c)
    prev = _state(opt)
    worst = {k: [0.0, 0.0] for k in NAMES}
    states = []
    for s in range(TT.N_STEPS):
        mask = c["masks"][s]
        opt.grads.copy_(T(c["grads"][s]))
        g_in = opt.grads.cpu().clone()
        opt.step(None if mask is None else torch.tensor(mask, dtype=torch.uint8, device=DEV))
        got = _state(opt)
        for k, what in enumerate(NAMES):
            x, r64, r32 = got[k].double().numpy(), s64[s][k], s32[s][k].astype(np.float64)
            err, e32 = np.abs(x - r64), np.abs(r32 - r64)
            worst[what] = [max(worst[what][0], float(err.max())), max(worst[what][1], float(e32.max()))]
            tol = np.maximum(1e-5 * np.abs(r64) + 1e-6, 4 * e32)
            assert np.all(err <= tol), (name, s, what, float(np.max(err / tol)))
            if what == "grads":
                assert np.all(err <= 1e-6 * np.abs(r64)), (name, s, what, float(np.max(err / np.abs(r64).clip(1e-300))))
            if what == "exp_avg_sq":
                assert np.all(err <= 4e-6 * np.abs(r64)), (name, s, what, float(np.max(err / np.abs(r64).clip(1e-300))))
        assert np.array_equal(got[4].numpy(), s64[s][4]), (name, s, got[4], s64[s][4])
        if mask is not None:
            off = ~torch.tensor(mask, dtype=torch.bool)
            for k in range(3):
                assert torch.equal(got[k][off], prev[k][off]), (name, s, NAMES[k])
            assert torch.equal(got[3][off], g_in[off]) and torch.equal(got[4][off], prev[4][off])
        if c["max_norm"] <= 0:
            assert torch.equal(got[3], g_in)  # no clip: the gradients are not written
        prev = got
        states.append(got)
    print(f"clip_adam {name}: worst |kernel - f64| / |torch32 - f64|: " +
          ", ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in worst.items()))
    return c, states


@pytest.mark.parametrize("name", ["prereduced-float4", "prereduced-scalar"])
def test_clip_adam_prereduced_norm_with_active_clip(name):
    """n = 17 * 8192 + 4 | + 5: 18 sum-of-squares chunks per agent, so the
    clip coefficients come from clip_coef_kernel; three groups with both
    boundaries off a multiple of 4 (one in the first chunk, one later); the
    first update's coefficients are far below 1, one group's gradient is zero."""
    c, states = _run_case(name)
    assert -(-c["n"] // 8192) > 16
    g0, first = torch.from_numpy(c["grads"][0]), states[0][3]
    for a, b in zip(c["offsets"][:-1], c["offsets"][1:]):
        ratio = first[:, a:b].norm(dim=1) / g0[:, a:b].norm(dim=1).clamp(min=1e-30)
        assert bool((ratio[1:] < 0.26).all()) and bool((ratio[1:] > 0.1).all())  # 1 / 8 .. 1 / 4
    assert torch.equal(first[0, :3001], torch.zeros(3001))


def test_clip_adam_active_mask():
    c, states = _run_case("active-mask")
    assert states[-1][4].tolist() == [3, 2, 4, 3]
    # agent 1 sat out updates 2 and 3: its last update is its second, with its own bias correction
    assert not torch.equal(states[3][0][1], states[0][0][1])


@pytest.mark.parametrize("name", ["no-clip-float4", "no-clip-scalar"])
def test_clip_adam_without_clip_leaves_the_gradients(name):
    _run_case(name)


@pytest.mark.parametrize("name", ["one-group", "eight-groups"])
def test_clip_adam_group_counts(name):
    c, states = _run_case(name)
    if name == "eight-groups":
        assert c["offsets"][1] - c["offsets"][0] == 1  # a group of one element: |g| clipped to max_norm
        assert abs(abs(float(states[0][3][1, 0])) - c["max_norm"]) <= 1e-6


def test_clip_adam_rejects_bad_groups():
    n = 90
    params = torch.zeros(2, n, device=DEV)
    opt = K().ClipAdam(params, list(range(0, 100, 10)), 1e-3)  # nine groups
    with pytest.raises(_agx_error()):
        opt.step()
    with pytest.raises(ValueError):
        K().ClipAdam(params, [0, 40, n - 1], 1e-3)
    for bad in ([0, 40, n - 1], [1, 40, n]):  # past the front end's check: the C entry's own
        opt = K().ClipAdam(params, [0, 40, n], 1e-3)
        opt.offsets = torch.tensor(bad, dtype=torch.int64)
        with pytest.raises(_agx_error()):
            opt.step()
    torch.cuda.synchronize()
    assert not params.any() and int(opt.steps.sum()) == 0  # nothing ran


def test_clip_adam_betas_eps_and_starting_steps():
    """betas (0.8, 0.9), eps 1e-5, a learning rate per agent, and step counts
    [0, 7, 1000] with non-zero moments: an optimiser restored from a checkpoint."""
    c, states = _run_case("betas-eps-steps")
    assert states[-1][4].tolist() == [4, 11, 1004]


# --------------------------------------------------------------------------- #
# Polyak                                                                      #
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n", [4096 * 256 + 257, 1, 0])
def test_polyak_grid_stride_and_tiny(n):
    """The grid is capped at 4096 blocks of 256: n = 4096 * 256 + 257 takes a
    second pass of the grid-stride loop (and a partial block in it); n = 0 is
    a no-op."""
    g = torch.Generator().manual_seed(n)
    t, o = torch.randn(n, generator=g), torch.randn(n, generator=g)
    exp = 1e-3 * o + (1.0 - 1e-3) * t
    td = t.to(DEV)
    K().polyak_(td, o.to(DEV), 1e-3)
    assert torch.equal(td.cpu(), exp)


# --------------------------------------------------------------------------- #
# TD target                                                                   #
# --------------------------------------------------------------------------- #
def _td_kernel(rec, double, with_loss=True):
    out = K().td_target(T(rec["qnt"]), T(rec["r"]), T(rec["d"]), rec["gamma"], T(rec["qno"]), double,
                        T(rec["qc"]) if with_loss else None, T(rec["a"]) if with_loss else None, with_loss=with_loss)
    torch.cuda.synchronize()
    return [None if x is None else x.cpu().numpy() for x in out]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("double", [False, True], ids=["max", "double"])
@pytest.mark.parametrize("A", TT.TD_A)
@pytest.mark.parametrize("B", TT.TD_B)
def test_td_target_sweep(B, A, double):
    """y and dloss/dQ bit for bit against the float32 restatement (ties: the
    first index), the gradient within rtol 1e-5 of torch autograd's, the loss
    within one float32 ulp of the float64 mean rounded to float32 (the kernel
    sums in float64 in another order and rounds once: only a rounding tie
    moves it), and the same y without the loss outputs."""
    rec = TT.td_inputs(B, A)
    ey, eg, eloss = TT.td_call(TT.td_target_f32, rec, double)
    _, tg, _ = TT.td_call(TT.td_target_torch, rec, double)
    y, gq, loss = _td_kernel(rec, double)
    assert _same_bits(y, ey) and _same_bits(gq, eg)
    np.testing.assert_allclose(gq, tg, rtol=1e-5, atol=0)
    assert abs(float(loss[0]) - float(eloss)) <= TT.ulp32(eloss), (float(loss[0]), float(eloss))
    y2, g2, l2 = _td_kernel(rec, double, with_loss=False)
    assert _same_bits(y2, ey) and g2 is None and l2 is None


@pytest.mark.parametrize("double", [False, True], ids=["max", "double"])
def test_td_target_nan_rows_follow_torch(double):
    """A diverged target (or online) net: torch.max gives NaN, torch.argmax
    the first NaN's index; y is NaN exactly where the reference's is, torch's
    bits elsewhere, and the loss is NaN when the reference's is."""
    rec = TT.td_nan_inputs(double)
    ty, _, tloss = TT.td_call(TT.td_target_torch, rec, double)
    y, _, loss = _td_kernel(rec, double)
    assert np.array_equal(np.isnan(y), np.isnan(ty)), np.flatnonzero(np.isnan(y) != np.isnan(ty))
    ok = ~np.isnan(ty)
    assert np.array_equal(y[ok].view(np.uint32), ty[ok].view(np.uint32)), np.flatnonzero(y[ok] != ty[ok])
    assert np.isnan(float(loss[0])) == np.isnan(float(tloss))
    if not double:
        assert np.isnan(ty).sum() == 8 and np.isnan(float(loss[0]))


# --------------------------------------------------------------------------- #
# the loss sum over more than 1024 block partials                             #
# --------------------------------------------------------------------------- #
BIG = 1024 * 256 + 257  # 1026 partials: loss_finalize's 1024 threads take a second pass


def _big_critic_inputs():
    rng = np.random.default_rng(99)
    f = lambda: rng.standard_normal(BIG).astype(np.float32)  # noqa: E731
    return dict(q1=f(), q2=f(), qn1=f(), qn2=f(), r=f(), d=(rng.random(BIG) < 0.1).astype(np.float32))


def _mse64(q, y):
    return np.float32(np.mean((q.astype(np.float64).ravel() - y.astype(np.float64).ravel()) ** 2))


def test_loss_sum_over_1024_partials_td_target():
    rec = TT.td_inputs(BIG, 2)
    for double in (False, True):
        ey, eg, eloss = TT.td_call(TT.td_target_f32, rec, double)
        y, gq, loss = _td_kernel(rec, double)
        assert _same_bits(y, ey) and _same_bits(gq, eg)
        assert abs(float(loss[0]) - float(eloss)) <= TT.ulp32(eloss), (float(loss[0]), float(eloss))


@pytest.mark.parametrize("form", ["td3-twin", "td3-single", "maddpg"])
def test_loss_sum_over_1024_partials_critic_targets(form):
    """y and dloss/dQ bit for bit against tests/td3_twin.py critic_target in
    float32 torch (y) and (Q - y)(2 / B); the loss (the float32 sum of the two
    critics' for TD3) against the float64 means rounded to float32, one ulp."""
    c = _big_critic_inputs()
    two = form == "td3-twin"
    t = lambda k: torch.from_numpy(c[k]).view(BIG, 1)  # noqa: E731
    ey, _ = td3_twin.critic_target([t("q1")] + ([t("q2")] if two else []), [t("qn1")] + ([t("qn2")] if two else []),
                                   t("r"), t("d"), 0.99)
    ey = ey.numpy()
    scale = np.float32(2.0) / np.float32(BIG)
    g = lambda k: T(c[k]).view(BIG, 1)  # noqa: E731
    if form == "maddpg":
        y, g1, loss = K().maddpg_critic_target(g("q1"), g("qn1"), g("r"), g("d"), 0.99)
        g2 = None
    else:
        y, g1, g2, loss = K().td3_critic_target(g("q1"), g("qn1"), g("r"), g("d"), 0.99, g("q2") if two else None,
                                                g("qn2") if two else None)
    torch.cuda.synchronize()
    assert _same_bits(y.cpu().numpy(), ey)
    assert _same_bits(g1.cpu().numpy(), (c["q1"].reshape(BIG, 1) - ey) * scale)
    want = _mse64(c["q1"], ey)
    if two:
        assert _same_bits(g2.cpu().numpy(), (c["q2"].reshape(BIG, 1) - ey) * scale)
        want = want + _mse64(c["q2"], ey)
    else:
        assert g2 is None
    assert abs(float(loss.item()) - float(want)) <= TT.ulp32(want), (float(loss.item()), float(want))
