"""tests/per_twin.py against both restatements of the reference's
prioritized-replay loops — oracle.cref.PERTree on every case,
oracle.per.PER where the case is small enough for Python loops — on the
cases tests/test_per_paths_gpu.py feeds the kernels: every node of both trees,
max_priority, the sampled indices and the out-of-range count bit for bit, the
weights at one float32 ulp.  Also the conditions the cases' inputs must meet,
and the host path each of them is listed under.  No GPU."""

import numpy as np
import pytest

from tests import per_twin as PT

f32 = np.float32
ALL = list(PT.CASES)


def _records_equal(got, want, ops, what):
    recs = [op for op in ops if op[0] != "set_max"]
    assert len(got) == len(want) == len(recs)
    for j, (g, w, op) in enumerate(zip(got, want, recs)):
        tag = f"{what}: op {j} ({op[0]})"
        if op[0] == "sample":
            assert np.array_equal(g[0], w[0]), tag
            np.testing.assert_allclose(g[1], w[1], rtol=2e-7, err_msg=tag)
            assert g[2] == w[2], tag
        else:
            assert np.array_equal(PT.bits(g[0])[1:], PT.bits(w[0])[1:]), tag + " sum tree"
            assert np.array_equal(PT.bits(g[1])[1:], PT.bits(w[1])[1:]), tag + " min tree"
            assert PT.bits([g[2]])[0] == PT.bits([w[2]])[0], tag + " max_priority"


@pytest.mark.parametrize("name", ALL)
def test_twin_equals_c_oracle(name):
    ms, alpha, ops = PT.case(name)
    _records_equal(PT.run(PT.Twin(ms, alpha), ops), PT.expected(name), ops, name)


@pytest.mark.parametrize("name", [n for n in ALL if PT.python_oracle_fits(n)])
def test_twin_equals_python_oracle(name):
    ms, alpha, ops = PT.case(name)
    _records_equal(PT.run(PT.Twin(ms, alpha), ops), PT.run(PT.PyOracle(ms, alpha), ops), ops, name)


def test_python_oracle_covers_the_small_cases():
    fits = {n for n in ALL if PT.python_oracle_fits(n)}
    assert "two-bands" not in fits
    assert {"top-only-cap2048", "top-only-cap256", "tiny-1", "tiny-2", "one-level-band", "long-ring-cap2048",
            "sparse-update-1025", "sparse-add-wrap", "contended-1-leaf", "staged-shallow-cap256",
            "staged-shallow-cap4096", "error-counter-staged"} <= fits


# ---- the path every op is listed under --------------------------------------------- #
@pytest.mark.parametrize("name", ALL)
def test_every_op_takes_the_path_it_is_listed_under(name):
    ms, _, ops = PT.case(name)
    for op in ops:
        takes, listed = PT.op_route(ms, op)
        assert takes == listed, (name, op[0])


def test_route_names_on_the_thresholds():
    r, v = PT.route, PT.sample_variant
    assert [r(1 << 16, n) for n in (1, 1024, 1025, 2047, 2048)] == ["small", "small", "sparse-levels",
                                                                    "sparse-levels", "bands(5)"]
    assert [r(c, 1025) for c in (1, 2, 256, 2048, 4096, 1 << 15, 1 << 16)] == [
        "top-only", "top-only", "top-only", "top-only", "bands(1)", "bands(4)", "sparse-levels"]
    assert r(1 << 17, 20_000) == "bands(6)" and r(1 << 20, 1 << 16) == "bands(9)"
    assert r(1 << 21, 1 << 16) == "bands(9,1)" and r(1 << 21, (1 << 16) - 1) == "sparse-levels"
    assert r(1 << 30, 1 << 26) == "bands(9,9,1)"
    assert r(1024, 1500, max_size=1000) == "small" and r(2048, 4000, max_size=1500) == "top-only"
    assert [v(1 << 16, B) for B in (1, 8191, 8192)] == ["walk", "walk", "staged-top(5)"]
    assert [v(c, 8192) for c in (1, 256, 2048, 4096)] == ["staged-all", "staged-all", "staged-all", "staged-top(1)"]


def test_every_route_and_variant_is_taken_by_some_case():
    taken = set()
    for name in ALL:
        ms, _, ops = PT.case(name)
        taken |= {(op[0], PT.op_route(ms, op)[0]) for op in ops if op[0] != "set_max"}
    for kind in ("add", "update"):
        assert {(kind, r) for r in ("small", "top-only", "sparse-levels", "bands(1)", "bands(5)", "bands(9,1)")} <= taken
    assert {("sample", s) for s in ("walk", "staged-all", "staged-top(1)", "staged-top(5)")} <= taken


# ---- conditions on the inputs -------------------------------------------------------- #
@pytest.mark.parametrize("name", ALL)
def test_sample_inputs_in_range_or_counted(name):
    """In-range cases: the oracle counts no bound out of range and the total is
    finite and positive.  Error-counter cases: at most 8 bounds out of range,
    and the oracle counts exactly the number the case lists."""
    ms, _, ops = PT.case(name)
    recs = [op for op in ops if op[0] != "set_max"]
    for op, rec in zip(recs, PT.expected(name)):
        if op[0] != "sample":
            total = rec[0][1]
            assert np.isfinite(total) and total > 0
            continue
        assert rec[2] == op[4] <= 8
        assert (op[4] > 0) == name.startswith("error-counter")
        assert not np.isnan(op[1]).any() and np.isfinite(op[1]).all()
    if name.startswith("error-counter"):
        u = [op for op in ops if op[0] == "sample"][0][1]
        assert u[0] < 0 and u[-1] > 1  # a negative bound in the first stratum, one beyond the total in the last


@pytest.mark.parametrize("name", [n for n in ALL if n.startswith(("staged-shallow", "sample-deep"))])
def test_sample_streams_hold_the_edge_uniforms(name):
    ms, _, ops = PT.case(name)
    samples = [op for op in ops if op[0] == "sample"]
    want = PT.SHALLOW_B if name.startswith("staged-shallow") else PT.DEEP_B
    assert tuple(op[1].size for op in samples) == want
    longest = max(samples, key=lambda op: op[1].size)[1]
    for op in samples:
        u = op[1]
        assert u.dtype == f32 and (u == 0.0).any() and (u == f32(PT.U_TOP)).any() and u.max() < 1.0 and u.min() >= 0.0
        assert np.array_equal(u[:-1], longest[:u.size - 1])  # one stream's prefix (its last draw set to the edge)
    assert f32(PT.U_TOP) < 1 and np.nextafter(f32(PT.U_TOP), f32(2)) == f32(1)


def test_a_sampled_ring_is_partly_filled():
    ms, alpha, ops = PT.case("staged-shallow-cap2048-partly-filled")
    t = PT.Twin(ms, alpha)
    PT.run(t, ops)
    assert 0 < t.size < ms


def test_sparse_update_stream_edges():
    ms = 60_000
    cases = [PT.case(n)[2][1] for n in ("sparse-update-1025", "sparse-update-2047", "dense-update-2048")]
    full = cases[2]
    for op, n in zip(cases, (1025, 2047, 2048)):
        idx, pri = op[1], op[2]
        assert idx.size == n and np.array_equal(idx, full[1][:n]) and np.array_equal(pri, full[2][:n])
        assert idx.min() == 0 and idx.max() == ms - 1
        assert np.unique(idx).size < n  # duplicates
        s = set(idx.tolist())
        assert any(i % 2 == 0 and i + 1 in s for i in s)  # a pair of sibling leaves
        assert (pri < PT.FLOOR).any()


@pytest.mark.parametrize("name", [n for n in ALL if n.startswith(("max-last", "max-inner-wave"))])
def test_running_max_is_unique_and_where_the_case_says(name):
    ms, _, ops = PT.case(name)
    recs = [op for op in ops if op[0] != "set_max"]
    before, waves = 1.0, []
    for op, rec in zip(recs, PT.expected(name)):
        if op[0] != "update":
            continue
        pri = op[2].astype(np.float64)
        top = int(np.argmax(pri))
        assert np.count_nonzero(pri == pri[top]) == 1  # unique ...
        assert np.sort(pri)[-2] < before < pri[top]  # ... and the only element above the value so far
        if name.startswith("max-last"):
            assert top == pri.size - 1
        else:
            assert top // 256 > 0 and top % 256 >= 64
            waves.append(top % 256 // 64)
        assert rec[2] == pri[top]
        before = pri[top]
    assert waves == ([] if name.startswith("max-last") else [1, 2, 3])


@pytest.mark.parametrize("name", [n for n in ALL if n.startswith("max-below")])
def test_running_max_below_cases(name):
    ms, _, ops = PT.case(name)
    start = [op for op in ops if op[0] == "set_max"][-1][1]
    pri = ops[-1][2].astype(np.float64)
    got = PT.expected(name)[-1][2]
    if "below-current" in name:
        assert pri.max() < start and PT.bits([got])[0] == PT.bits([start])[0]
    else:
        assert pri.max() < PT.FLOOR
        assert got == (start if "from-above" in name else PT.FLOOR)
        assert (start > PT.FLOOR) == ("from-above" in name)


@pytest.mark.parametrize("name,distinct", [("contended-3-leaves", 3), ("contended-1-leaf", 1)])
def test_contended_priorities_are_distinct_per_leaf(name, distinct):
    ms, alpha, ops = PT.case(name)
    idx, pri = ops[-1][1], ops[-1][2]
    assert np.unique(idx).size == distinct and idx.size >= 1500
    floored = np.maximum(pri.astype(np.float64), PT.FLOOR)
    for leaf in np.unique(idx):
        p = floored[idx == leaf]
        assert np.unique(p).size == p.size
    # the surviving leaf is the one written at the highest position
    s = PT.expected(name)[-1][0]
    for leaf in np.unique(idx):
        last = int(np.flatnonzero(idx == leaf)[-1])
        assert s[PT.capacity(ms) + leaf] == PT.cref.libm_pow(floored[last:last + 1], alpha)[0]


def test_leaf_is_pow_of_the_widened_float32_priority():
    """max(p, floor) acts on the float32 priority widened to float64 — not on
    a float64 priority, and not in float32 (1e-5 itself is not a float32)."""
    pri = np.array([1e-5, 0.3, 1e-9], dtype=f32)
    leaf = PT.leaves(PT.empty_leaves(4), 0.6, indices=[0, 1, 2], priorities=pri)
    want = [max(float(p), 1e-5) ** 0.6 for p in pri]
    assert leaf[:3].tolist() == want and np.isnan(leaf[3])
    assert float(f32(1e-5)) != 1e-5
    s, m = PT.rebuild(leaf)
    assert s[4 + 3] == 0.0 and m[4 + 3] == np.inf and s[1] == (want[0] + want[1]) + (want[2] + 0.0)
    assert m[1] == min(want)
