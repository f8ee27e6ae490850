"""The split LSTM form (csrc/lstm_split.hip): equal bits with the whole-sequence kernels, and parity with nn.LSTM
in float64 on the CPU.

Error measure and bound as in tests/test_lstm_gpu.py: max |a - ref| / max |ref| per tensor, at most 4 x the
float32 CPU nn.LSTM's own error + 8 * 2^-23."""

import pytest
import torch
from torch import nn

from agilerl_amd.modules.lstm import EvolvableLSTM, lstm_sequence

pytestmark = pytest.mark.gpu

# (B, T, in, H, L): one row, one step, unaligned input (forward reads h0 only, backward is the first step and the
# tail); a one-row second tile, input not a multiple of 4, a layer below the top; more rows than a workgroup's row
# group and nine unit tiles; three layers (the projection in `saved` and in the workspace); the widest slice
CASES = [(1, 1, 3, 16, 1), (17, 5, 5, 48, 2), (130, 3, 8, 144, 1), (33, 4, 20, 272, 3), (4, 2, 4, 512, 1)]
FLOOR = 8 * 2.0 ** -23
NAMES = ["y", "h_n", "c_n", "dx", "dh0", "dc0"]


def _build(B, T, n_in, H, L):
    torch.manual_seed(0)
    m = EvolvableLSTM(n_in, H, 4, num_layers=L, max_layers=L + 1, device="cuda")
    data = [torch.randn(B, T, n_in), 0.5 * torch.randn(L, B, H), 0.5 * torch.randn(L, B, H)]
    cots = [torch.randn(B, T, H), torch.randn(L, B, H), torch.randn(L, B, H)]
    return m, data, cots


def _run(lstm, data, cots, fused=None, plan=None, state_cots=True):
    """(y, h_n, c_n, dx, dh0, dc0, parameter gradients...); without ``state_cots`` only y is differentiated and x
    needs no gradient (gh_n / gc_n None, no gx)."""
    p = next(lstm.parameters())
    x, h0, c0 = (t.to(p.device, p.dtype) for t in data)
    wrt = [h0.requires_grad_(), c0.requires_grad_(), *lstm.parameters()]
    if state_cots:
        wrt.insert(0, x.requires_grad_())
    if fused is not None:
        outs = lstm_sequence(fused, x, h0, c0, plan=plan)
    else:
        y, (h_n, c_n) = lstm(x, (h0, c0))
        outs = (y, h_n, c_n)
    cots = [c.to(p.device, p.dtype) for c in cots]
    grads = torch.autograd.grad(outs if state_cots else outs[:1], wrt, cots if state_cots else cots[:1])
    return [t.detach().double().cpu() for t in (*outs, *grads)]


def _err(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("state_cots", [True, False], ids=["all", "y-only"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_equal_bits(case, state_cots):
    m, data, cots = _build(*case)
    split = _run(m.lstm, data, cots, fused=m, plan="split", state_cots=state_cots)
    whole = _run(m.lstm, data, cots, fused=m, plan="whole", state_cots=state_cots)
    names = (NAMES if state_cots else NAMES[:3] + NAMES[4:]) + [n for n, _ in m.lstm.named_parameters()]
    assert len(names) == len(split)
    assert [n for n, a, b in zip(names, split, whole) if not torch.equal(a, b)] == []
    with torch.no_grad():  # the no-grad forward: the projection in the workspace, lower layers through y
        x, h0, c0 = (t.cuda() for t in data)
        for a, b in zip(lstm_sequence(m, x, h0, c0, plan="split"), whole[:3]):
            assert torch.equal(a.double().cpu(), b)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_parity(case):
    m, data, cots = _build(*case)
    cpu32 = nn.LSTM(case[2], case[3], case[4], batch_first=True)
    cpu32.load_state_dict(m.lstm.state_dict())
    cpu64 = nn.LSTM(case[2], case[3], case[4], batch_first=True).double()
    cpu64.load_state_dict(m.lstm.state_dict())
    ref, base = _run(cpu64, data, cots), _run(cpu32, data, cots)
    got = _run(m.lstm, data, cots, fused=m, plan="split")
    worst = []
    for n, g, b, r in zip(NAMES + [n for n, _ in m.lstm.named_parameters()], got, base, ref):
        e, e32 = _err(g, r), _err(b, r)
        print(f"{case} {n}: split {e:.3e} cpu32 {e32:.3e} ratio {e / max(e32, 2.0 ** -24):.2f}")
        if e > 4 * e32 + FLOOR:
            worst.append((n, e, e32))
    assert not worst, worst


def test_chunked_equals_whole_and_deterministic():
    m, (x, h0, c0), _ = _build(17, 6, 8, 144, 2)
    x, h0, c0 = x.cuda(), h0.cuda(), c0.cuda()
    with torch.no_grad():
        want = lstm_sequence(m, x, h0, c0, plan="whole")
        got = lstm_sequence(m, x, h0, c0, plan="split")
        again = lstm_sequence(m, x, h0, c0, plan="split")
        ys, h, c = [], h0, c0
        for t in range(0, 6, 2):
            yc, h, c = lstm_sequence(m, x[:, t:t + 2].contiguous(), h, c, plan="split")
            ys.append(yc)
    for w, g, a, ch in zip(want, got, again, (torch.cat(ys, 1), h, c)):
        assert torch.equal(g, w) and torch.equal(a, g) and torch.equal(ch, g)
