"""The restatements of tests/tail_twin.py against each other, against torch and
against the reference's golden vectors, on the inputs the GPU tests
(tests/test_tail_kernels_gpu.py) feed the kernels.  No GPU."""

import numpy as np
import pytest
import torch

from tests import tail_twin as TT


# ---- optimiser -------------------------------------------------------------------- #
@pytest.mark.parametrize("name", list(TT.ADAM_CASES))
def test_adam_inputs_keep_off_the_clip_branch(name):
    c = TT.adam_inputs(name)
    assert TT.adam_norms_off_the_branch(c)
    norms = [np.sqrt(np.sum(g[:, a:b].astype(np.float64) ** 2, axis=1)) for g in c["grads"]
             for a, b in zip(c["offsets"][:-1], c["offsets"][1:])]
    ref = c.get("norm", c["max_norm"])
    assert max(n.max() for n in norms[:len(c["offsets"]) - 1]) >= 2 * ref  # the first step clips
    if "zero" in c:
        assert any(n[0] == 0.0 for n in norms) and all(n[1] > 0 for n in norms)


@pytest.mark.parametrize("name", list(TT.ADAM_CASES))
def test_adam_float64_and_torch_float32_twins_agree(name):
    """Both after every step, at the bar the kernel is held to against torch
    (tests/test_kernels_gpu.py test_clip_adam_matches_torch: rtol 1e-5, atol
    1e-6); the step counts exactly; the first step's clip coefficient below 1
    and the later ones' 1 show in the returned gradients."""
    c, s64, s32 = TT.adam_twins(name)
    for s in range(TT.N_STEPS):
        for k, what in enumerate(("params", "exp_avg", "exp_avg_sq", "grads")):
            np.testing.assert_allclose(s32[s][k], s64[s][k], rtol=1e-5, atol=1e-6, err_msg=f"step {s} {what}")
        assert np.array_equal(s32[s][4], s64[s][4])
        on = np.ones(c["P"], bool) if c["masks"][s] is None else np.asarray(c["masks"][s], bool)
        same = np.all(s64[s][3] == c["grads"][s].astype(np.float64), axis=1)
        if c["max_norm"] > 0 and s == 0:
            assert not same[on].any()  # clipped
        else:
            assert same.all()
    first = np.asarray(c["steps0"])
    moved = sum((np.ones(c["P"], np.int64) if mk is None else np.asarray(mk, np.int64)) for mk in c["masks"])
    assert np.array_equal(s64[-1][4], first + moved)


def test_adam_twins_hold_inactive_agents():
    c, s64, s32 = TT.adam_twins("active-mask")
    for states in (s64, s32):
        for s in (1, 2):
            off = ~np.asarray(c["masks"][s], bool)
            for k in range(3):
                assert np.array_equal(states[s][k][off], states[s - 1][k][off])
                assert not np.array_equal(states[s][k][~off], states[s - 1][k][~off])
            assert np.array_equal(states[s][4][off], states[s - 1][4][off])
            assert np.array_equal(states[s][3][off], np.asarray(c["grads"][s], states[s][3].dtype)[off])


def test_adam_float64_twin_without_clip_is_plain_adam():
    """max_norm = 0: the gradients come back untouched and the update is
    torch.optim.Adam's in float64 on the unclipped gradient."""
    c, s64, _ = TT.adam_twins("no-clip-scalar")
    w = torch.nn.Parameter(torch.tensor(c["p0"][0], dtype=torch.float64))
    opt = torch.optim.Adam([w], lr=float(c["lr"][0]), betas=tuple(float(np.float32(b)) for b in c["betas"]),
                           eps=float(np.float32(c["eps"])))
    for s in range(TT.N_STEPS):
        w.grad = torch.tensor(c["grads"][s][0], dtype=torch.float64)
        opt.step()
        assert np.array_equal(s64[s][3][0], c["grads"][s][0].astype(np.float64))
        # addcdiv_ may round in another order than p - step (m / denom): a few float64 ulp
        np.testing.assert_allclose(s64[s][0][0], w.detach().numpy(), rtol=1e-12, atol=1e-12)


# ---- DQN's TD target ---------------------------------------------------------------- #
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("A", TT.TD_A)
@pytest.mark.parametrize("B", TT.TD_B)
def test_td_target_float32_twin_equals_torch(B, A, double):
    """y bit for bit (ties: the first index), the gradient and the loss at
    float32 rounding."""
    rec = TT.td_inputs(B, A)
    y, gq, loss = TT.td_call(TT.td_target_f32, rec, double)
    ty, tgq, tloss = TT.td_call(TT.td_target_torch, rec, double)
    assert y.shape == ty.shape and np.array_equal(y.view(np.uint32), ty.view(np.uint32))
    np.testing.assert_allclose(gq, tgq, rtol=1e-5, atol=0)
    assert (gq != 0).sum(1).max() <= 1
    assert abs(float(loss) - float(tloss)) <= 1e-5 * abs(float(tloss))
    if B > 1:  # the tie rows take the first action's target value
        want = rec["qnt"][64:96, 0] if double else rec["qnt"][80:112, 0]
        rows = slice(64, 96) if double else slice(80, 112)
        exp = rec["r"][rows] + (np.float32(rec["gamma"]) * want) * (np.float32(1) - rec["d"][rows])
        assert np.array_equal(y[rows, 0], exp)


@pytest.mark.parametrize("case", ["dqn0", "dqn1", "dqn2"])
def test_td_target_float32_twin_matches_the_golden_vectors(golden, case):
    g = golden(case)
    y, gq, loss = TT.td_target_f32(g["q_next_online"], g["q_next_target"], g["q_cur"], g["a"], g["r"], g["d"],
                                   float(g["gamma"]), bool(g["double"]))
    assert np.array_equal(y.reshape(g["y"].shape), g["y"])
    np.testing.assert_allclose(gq, g["g_q"], rtol=1e-5, atol=1e-9)
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))


@pytest.mark.parametrize("double", [False, True])
def test_td_target_twins_propagate_nan_as_torch(double):
    """A NaN among the values the max / argmax runs over: torch.max returns
    NaN, torch.argmax the first NaN's index; numpy's do the same, so the
    float32 twin's y has torch's bits on every finite row and NaN where
    torch's is NaN, and the loss is NaN."""
    rec = TT.td_nan_inputs(double)
    y, _, loss = TT.td_call(TT.td_target_f32, rec, double)
    ty, _, tloss = TT.td_call(TT.td_target_torch, rec, double)
    assert np.array_equal(np.isnan(y), np.isnan(ty))
    assert np.array_equal(y[~np.isnan(y)].view(np.uint32), ty[~np.isnan(ty)].view(np.uint32))
    if double:  # the selected target value is finite: y is the first NaN column's target
        first = np.array([np.flatnonzero(np.isnan(row))[0] if np.isnan(row).any() else -1 for row in rec["qno"]])
        rows = np.flatnonzero(first >= 0)
        assert rows.size == 8 and first[70] == 2 and first[85] == 1 and first[299] == 1
        exp = rec["r"][rows] + (np.float32(rec["gamma"]) * rec["qnt"][rows, first[rows]]) * (1 - rec["d"][rows])
        assert np.array_equal(y[rows, 0], exp.astype(np.float32)) and np.isfinite(float(loss))
    else:
        assert np.isnan(y).sum() == 8 and np.isnan(float(loss)) and np.isnan(float(tloss))
