"""agx_replay_gather (csrc/replay_gather.hip): the sampled batch of every
stored field in one launch, bit-exact against torch's index_select of the
same rows — uint8 frames (16-byte units), int64 / f32 scalars (4-byte units)
and an odd-width uint8 field (1-byte units); uniform and prioritized
sampling (replay_buffer.py:97-137, 361-409).  Then the C entry called
directly: the stride loop over rows of more than 64 x 256 units, the width
fallback for unaligned bases, eight fields, the err flag and the host-side
rejections."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _fill(buf, n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf.add({"obs": torch.randint(0, 256, (n, 4, 84, 84), dtype=torch.uint8, device=DEV, generator=g),
             "action": torch.randint(0, 6, (n,), device=DEV, generator=g),
             "reward": torch.randn(n, device=DEV, generator=g),
             "next_obs": torch.randint(0, 256, (n, 4, 84, 84), dtype=torch.uint8, device=DEV, generator=g),
             "done": (torch.rand(n, device=DEV, generator=g) < 0.1).float(),
             "tag": torch.randint(0, 256, (n, 3), dtype=torch.uint8, device=DEV, generator=g)})


def _same(samples, storage, idx):
    for k, v in storage.items():
        ref = v.index_select(0, idx.reshape(-1).to(torch.int64))
        assert samples[k].dtype == ref.dtype and samples[k].shape == ref.shape, k
        assert torch.equal(samples[k], ref), k


def test_prioritized_sample_gathers_every_field():
    from agilerl_amd.components import PrioritizedReplayBuffer

    torch.manual_seed(0)
    buf = PrioritizedReplayBuffer(5000, alpha=0.6)
    _fill(buf, 3000, 1)
    for B in (1, 64, 257):
        s = buf.sample(B, beta=0.4)
        _same(s, buf.storage, s["idxs"])


def test_uniform_sample_gathers_every_field():
    from agilerl_amd.components import ReplayBuffer

    torch.manual_seed(1)
    buf = ReplayBuffer(4000)
    _fill(buf, 2500, 2)
    s = buf.sample(128, return_idx=True)
    _same(s, buf.storage, s["idxs"])


# ---- the C entry itself, on the paths the buffers' shapes do not reach ------------ #
BIG_ROW = 16 * (64 * 256 + 5)  # bytes: 16 389 sixteen-byte units, past one pass of the 64 x 256 grid
SENTINEL = 0xAB


def _rand(shape, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, dtype=dtype, device=DEV, generator=g)
    if dtype == torch.int64:
        return torch.randint(-2 ** 40, 2 ** 40, shape, dtype=dtype, device=DEV, generator=g)
    return torch.randn(shape, dtype=dtype, device=DEV, generator=g)


def _offset_rows(rows, row_bytes, off, seed=None):
    """A [rows, row_bytes] uint8 view starting ``off`` bytes into a larger
    allocation (random bytes with a seed, else the sentinel)."""
    n = rows * row_bytes
    big = (_rand((n + 64,), torch.uint8, seed) if seed is not None
           else torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device=DEV))
    view = big[off:off + n].view(rows, row_bytes)
    assert view.data_ptr() == big.data_ptr() + off and big.data_ptr() % 16 == 0
    return big, view


def _call(srcs, dsts, idx, rows, err=None, B=None):
    """agx_replay_gather as ReplayBuffer._gather_sampled calls it."""
    import ctypes

    from agilerl_amd import _lib

    n = len(srcs)
    for s, d in zip(srcs, dsts):
        assert s.is_contiguous() and d.is_contiguous() and s.shape[0] == rows and s.shape[1:] == d.shape[1:]
    ps = (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs])
    pd = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dsts])
    rb = (ctypes.c_int64 * n)(*[s[0].numel() * s.element_size() for s in srcs])
    _lib.call("agx_replay_gather", ctypes.cast(ps, ctypes.c_void_p), ctypes.cast(pd, ctypes.c_void_p),
              ctypes.cast(rb, ctypes.c_void_p), n, idx.data_ptr(), idx.numel() if B is None else B, rows,
              _lib.ptr(err), _lib.stream())
    torch.cuda.synchronize()


def _check(srcs, idx, rows, dsts=None, guards=()):
    dsts = [torch.empty((idx.numel(), *s.shape[1:]), dtype=s.dtype, device=DEV) for s in srcs] if dsts is None else dsts
    _call(srcs, dsts, idx, rows)
    for k, (s, d) in enumerate(zip(srcs, dsts)):
        assert torch.equal(d, s.index_select(0, idx)), k
    for big, view in guards:  # the bytes around an offset destination keep the sentinel
        n = view.numel()
        off = view.data_ptr() - big.data_ptr()
        assert bool((big[:off] == SENTINEL).all()) and bool((big[off + n:] == SENTINEL).all())


def test_gather_stride_loop_with_small_fields_behind():
    """One uint8 field of 16 389 sixteen-byte units per row (the lanes of the
    64 x 256 grid take a second pass), a float32 field of 3 words and a uint8
    field of 3 bytes after it in the same launch; rows = 3, B = 2."""
    rows = 3
    srcs = [_rand((rows, BIG_ROW), torch.uint8, 1), _rand((rows, 3), torch.float32, 2),
            _rand((rows, 3), torch.uint8, 3)]
    for idx in ([2, 0], [1, 1]):  # the last and the first row; a repeat
        _check(srcs, torch.tensor(idx, device=DEV), rows)


@pytest.mark.parametrize("side", ["src", "dst"])
@pytest.mark.parametrize("off", [4, 1])
def test_gather_width_fallback_for_unaligned_bases(off, side):
    """The same row size from (or into) a view ``off`` bytes into a larger
    allocation: 4-byte units for off = 4, single bytes for off = 1 (65 556 and
    262 224 units per row: the stride loop again)."""
    rows = 3
    idx = torch.tensor([2, 0, 2, 1], device=DEV)
    if side == "src":
        _, src = _offset_rows(rows, BIG_ROW, off, seed=4)
        _check([src], idx, rows)
    else:
        src = _rand((rows, BIG_ROW), torch.uint8, 5)
        big, dst = _offset_rows(idx.numel(), BIG_ROW, off)
        _check([src], idx, rows, dsts=[dst], guards=[(big, dst)])


def _eight_fields(rows):
    kinds = [((32,), torch.uint8), ((4,), torch.float32), ((3,), torch.float32), ((1,), torch.int64),
             ((3,), torch.uint8), ((5,), torch.uint8), ((1,), torch.float32), ((2, 24), torch.uint8)]
    return [_rand((rows, *shape), dtype, 10 + k) for k, (shape, dtype) in enumerate(kinds)]


def test_gather_eight_fields_and_no_more():
    """Eight fields of 16-, 4- and 1-byte units in one launch; a ninth is rejected."""
    from agilerl_amd import _lib

    rows = 7
    idx = torch.tensor([0, 6, 3, 3, 0], device=DEV)
    srcs = _eight_fields(rows)
    _check(srcs, idx, rows)
    nine = srcs + [_rand((rows, 2), torch.float32, 30)]
    dsts = [torch.full((idx.numel(), *s.shape[1:]), 7, dtype=s.dtype, device=DEV) for s in nine]
    with pytest.raises(_lib.AgxError):
        _call(nine, dsts, idx, rows)
    assert all(bool((d == 7).all()) for d in dsts)


def test_gather_out_of_range_index_sets_err_and_skips_the_row():
    """-1 and ``rows`` are outside [0, rows): the kernel's own guard leaves
    those batch rows alone and raises the flag; every other row is gathered."""
    rows = 7
    idx = torch.tensor([0, -1, 2, rows, 6, 2], device=DEV)
    good = torch.tensor([0, 2, 4, 5], device=DEV)
    srcs = _eight_fields(rows)[:3] + [_rand((rows, 1040), torch.uint8, 40)]
    dsts = [torch.full((idx.numel(), *s.shape[1:]), SENTINEL if s.dtype == torch.uint8 else -7.5, dtype=s.dtype,
                       device=DEV) for s in srcs]
    before = [d.clone() for d in dsts]
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    _call(srcs, dsts, idx, rows, err=err)
    assert int(err.item()) == 1
    for s, d, b in zip(srcs, dsts, before):
        assert torch.equal(d[good], s.index_select(0, idx[good]))
        assert torch.equal(d[[1, 3]], b[[1, 3]])
    err.zero_()
    _call(srcs, dsts, idx[good].contiguous(), rows, err=err)
    assert int(err.item()) == 0  # in-range indices leave the flag alone


def test_gather_batch_limit_is_a_host_error():
    """B = 65536 (one grid row per sample: the grid's y limit) is refused
    before any launch."""
    from agilerl_amd import _lib

    rows = 4
    src = _rand((rows, 1), torch.float32, 50)
    idx = torch.zeros(65536, dtype=torch.int64, device=DEV)
    dst = torch.full((65536, 1), -7.5, device=DEV)
    with pytest.raises(_lib.AgxError):
        _call([src], [dst], idx, rows)
    assert bool((dst == -7.5).all())
    _call([src], [dst], idx, rows, B=65535)
    assert bool((dst[:65535] == src[0]).all()) and float(dst[65535]) == -7.5


def test_uniform_sample_of_65536_rows():
    """ReplayBuffer.sample(65536), as the reference returns it: past the gather
    kernel's batch limit the buffer gathers with index_select."""
    from agilerl_amd.components import ReplayBuffer

    torch.manual_seed(2)
    buf = ReplayBuffer(70_000)
    buf.add({"x": _rand((70_000,), torch.float32, 60)})
    s = buf.sample(65536, return_idx=True)
    assert s["x"].shape == (65536, 1) and s["idxs"].unique().numel() == 65536
    _same({"x": s["x"]}, buf.storage, s["idxs"])
