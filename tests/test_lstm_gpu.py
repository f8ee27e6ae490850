"""The fused LSTM sequence kernels (csrc/lstm.hip) against nn.LSTM in float64 on the CPU.

Error measure: max |a - ref| / max |ref| per tensor.  Bound: 4 x the float32 CPU nn.LSTM's own error against
float64 on the same inputs, + 8 * 2^-23 (eight float32 roundings of the largest element)."""

import copy

import pytest
import torch
from torch import nn

from agilerl_amd.modules.lstm import EvolvableLSTM, lstm_sequence

pytestmark = pytest.mark.gpu

# (B, T, in, H, L): one row / one step / smallest H; a full and a one-row tile; H not a power of two, input not
# a multiple of 4, two layers; one unit tile per wave on all eight waves, three layers; the first H above the
# register-resident threshold (64); the largest H
CASES = [(1, 1, 3, 16, 1), (17, 5, 8, 32, 1), (16, 7, 5, 48, 2), (33, 4, 20, 128, 3), (8, 3, 9, 80, 1),
         (4, 2, 4, 512, 1)]
FLOOR = 8 * 2.0 ** -23


def _build(B, T, n_in, H, L, seed=0):
    torch.manual_seed(seed)
    m = EvolvableLSTM(n_in, H, 4, num_layers=L, max_layers=max(L, 1) + 1, device="cuda")
    data = [torch.randn(B, T, n_in), 0.5 * torch.randn(L, B, H), 0.5 * torch.randn(L, B, H)]
    cots = [torch.randn(B, T, H), torch.randn(L, B, H), torch.randn(L, B, H)]
    return m, data, cots


def _run(lstm, data, cots, fused=None):
    """(y, h_n, c_n, dx, dh0, dc0, parameter gradients...) of ``lstm`` on its own device / dtype; ``fused``:
    the EvolvableLSTM whose kernels run instead of the nn.LSTM."""
    p = next(lstm.parameters())
    x, h0, c0 = (t.to(p.device, p.dtype).requires_grad_() for t in data)
    if fused is not None:
        y, h_n, c_n = lstm_sequence(fused, x, h0, c0)
    else:
        y, (h_n, c_n) = lstm(x, (h0, c0))
    outs = (y, h_n, c_n)
    grads = torch.autograd.grad(outs, [x, h0, c0, *lstm.parameters()], [c.to(p.device, p.dtype) for c in cots])
    return [t.detach().double().cpu() for t in (*outs, *grads)]


def _err(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("case", CASES, ids=str)
def test_parity(case):
    m, data, cots = _build(*case)
    cpu32 = nn.LSTM(case[2], case[3], case[4], batch_first=True)
    cpu32.load_state_dict(m.lstm.state_dict())
    cpu64 = nn.LSTM(case[2], case[3], case[4], batch_first=True).double()
    cpu64.load_state_dict(m.lstm.state_dict())
    ref, base, got = _run(cpu64, data, cots), _run(cpu32, data, cots), _run(m.lstm, data, cots, fused=m)
    names = ["y", "h_n", "c_n", "dx", "dh0", "dc0"] + [n for n, _ in m.lstm.named_parameters()]
    worst = []
    for n, g, b, r in zip(names, got, base, ref):
        e, e32 = _err(g, r), _err(b, r)
        print(f"{case} {n}: fused {e:.3e} cpu32 {e32:.3e} ratio {e / max(e32, 2.0 ** -24):.2f}")
        if e > 4 * e32 + FLOOR:
            worst.append((n, e, e32))
    assert not worst, worst


def test_chunked_equals_whole():
    m, (x, h0, c0), _ = _build(17, 6, 8, 32, 2)
    x, h0, c0 = x.cuda(), h0.cuda(), c0.cuda()
    with torch.no_grad():
        y, h_n, c_n = lstm_sequence(m, x, h0, c0)
        ys, h, c = [], h0, c0
        for t in range(0, 6, 2):
            yc, h, c = lstm_sequence(m, x[:, t:t + 2].contiguous(), h, c)
            ys.append(yc)
    assert torch.equal(torch.cat(ys, 1), y) and torch.equal(h, h_n) and torch.equal(c, c_n)
    x.requires_grad_()  # the saving forward has the no-grad forward's bits
    assert torch.equal(lstm_sequence(m, x, h0, c0)[0], y)


def test_deterministic():
    m, data, cots = _build(*CASES[3])
    a, b = _run(m.lstm, data, cots, fused=m), _run(m.lstm, data, cots, fused=m)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_fallbacks(monkeypatch):
    def args(m, B=3, T=2, dtype=torch.float32):
        L, H = m.num_layers, m.hidden_state_size
        return (torch.randn(B, T, m.input_size, device="cuda", dtype=dtype),
                torch.zeros(L, B, H, device="cuda", dtype=dtype), torch.zeros(L, B, H, device="cuda", dtype=dtype))

    ok = EvolvableLSTM(6, 32, 4, device="cuda")
    assert lstm_sequence(ok, *args(ok)) is not None
    assert lstm_sequence(EvolvableLSTM(6, 40, 4, device="cuda"), *args(EvolvableLSTM(6, 40, 4))) is None
    assert lstm_sequence(ok, *args(ok, dtype=torch.float64)) is None
    drop = EvolvableLSTM(6, 32, 4, num_layers=2, dropout=0.5, device="cuda")
    assert lstm_sequence(drop, *args(drop)) is None and lstm_sequence(drop.eval(), *args(drop)) is not None
    hooked = EvolvableLSTM(6, 32, 4, device="cuda")
    hooked.lstm.register_forward_hook(lambda *_: None)
    assert lstm_sequence(hooked, *args(hooked)) is None
    x, h0, c0 = args(ok)
    want = ok.model["lstm_lstm_output"](ok.lstm(x, (h0, c0))[0]).flatten(0, 1)
    monkeypatch.setenv("AGX_LSTM", "0")
    assert lstm_sequence(ok, x, h0, c0) is None
    out, nxt = ok(x.flatten(0, 1), {"lstm_h": h0, "lstm_c": c0})
    assert torch.equal(out, want) and nxt["lstm_h"].shape == h0.shape


def test_network_step_and_sequence(monkeypatch):
    from agilerl_amd.envs import Box

    from agilerl_amd.networks.actors import DeterministicActor

    monkeypatch.setenv("AGX_LSTM", "1")
    torch.manual_seed(1)
    obs_space, act_space = Box(-1.0, 1.0, (6,)), Box(-1.0, 1.0, (2,))
    net = DeterministicActor(obs_space, act_space, recurrent=True, device="cuda",
                             encoder_config={"hidden_state_size": 32, "num_layers": 2})
    ref32 = DeterministicActor(obs_space, act_space, recurrent=True,
                               encoder_config={"hidden_state_size": 32, "num_layers": 2})
    ref32.load_state_dict(net.state_dict())
    ref = copy.deepcopy(ref32).double()
    step, seq = torch.randn(5, 6), torch.randn(5 * 4, 6)

    def run(n, dev, dtype):
        hid = {k: v.to(dtype) for k, v in n.initialize_hidden_state(5).items()}
        a1, hid = n(step.to(dev, dtype), hid)
        a2, hid = n(seq.to(dev, dtype), hid)
        return [t.detach().double().cpu() for t in (a1, a2, hid["encoder_h"], hid["encoder_c"])], a1.sum() + a2.sum()

    (want, _), (base, _), (got, loss) = run(ref, "cpu", torch.float64), run(ref32, "cpu", torch.float32), \
        run(net, "cuda", torch.float32)
    for g, b, r in zip(got, base, want):
        assert g.shape == r.shape and _err(g, r) <= 4 * _err(b, r) + FLOOR
    loss.backward()
    assert all(p.grad is not None and p.grad.abs().sum() > 0 for p in net.encoder.parameters())
