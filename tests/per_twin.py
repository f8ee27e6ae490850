"""A plain restatement of what the prioritized-replay trees (csrc/per.hip) must
hold, in float64 numpy, plus the seeded cases the GPU tests
(tests/test_per_paths_gpu.py) feed the kernels.  tests/test_per_twin_cpu.py
pins the restatement to oracle.per.PER and oracle.cref.PERTree bit for bit on
exactly those cases.

The twin knows nothing of how the kernels split the work: a batch becomes a
leaf array (``leaves``), the trees are a function of the leaves alone
(``rebuild``), a sample is one walk per stratum (``sample``).  Only ``route``
and ``sample_variant`` restate the host's dispatch thresholds, so that every
test can assert the path it was written for.

  * ``leaves``          one add or update batch applied to a leaf array;
  * ``rebuild``         (sum tree, min tree) from the leaves;
  * ``max_priority``    the running maximum after an update batch;
  * ``sample``          stratified indices and the count of bounds outside
                        [0, total + 1e-5];
  * ``weights``         importance weights (replay_buffer.py:383-409);
  * ``route`` / ``sample_variant``  which host path a batch takes.
"""

from __future__ import annotations

import copy
import functools

import numpy as np

from oracle import cref
from oracle import per as oper

f32 = np.float32
FLOOR = 1e-5


def capacity(max_size: int) -> int:
    cap = 1
    while cap < max_size:
        cap *= 2
    return cap


def empty_leaves(cap: int) -> np.ndarray:
    """A leaf array nobody has written: NaN marks a leaf that still holds each
    tree's own neutral element (0 in the sum tree, inf in the min tree)."""
    return np.full(cap, np.nan)


def leaves(leaf, alpha, *, indices=None, priorities=None, start=None, n=None, max_size=None, max_priority=None,
           floor=FLOOR):
    """One batch on a copy of ``leaf``.  Update (``indices`` given): leaf =
    max(p, floor) ** alpha on the float32 priority widened to float64, the last
    duplicate wins.  Add: ``max_priority ** alpha`` at (start + i) % max_size
    for i < n.  The power is libm's pow."""
    out = np.array(leaf, dtype=np.float64)
    if indices is not None:
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        p = np.maximum(np.asarray(priorities, dtype=f32).reshape(-1).astype(np.float64), floor)
        val = cref.libm_pow(p, alpha)
        # the position of the last write to each distinct index
        _, first_from_end = np.unique(idx[::-1], return_index=True)
        last = idx.size - 1 - first_from_end
        out[idx[last]] = val[last]
    else:
        pos = (start + np.arange(n, dtype=np.int64)) % max_size
        out[pos] = cref.libm_pow(np.array([max_priority], dtype=np.float64), alpha)[0]
    return out


def rebuild(leaf):
    """(sum tree, min tree), each 2 * cap float64 with node k's children at 2k
    and 2k + 1 and the leaves at cap + i: every internal node is left + right,
    and right if right < left else left (Python's min(left, right)).  Node 0
    is never written (0 and inf)."""
    leaf = np.asarray(leaf, dtype=np.float64)
    cap = leaf.size
    s, m = np.zeros(2 * cap), np.full(2 * cap, np.inf)
    s[cap:] = np.where(np.isnan(leaf), 0.0, leaf)
    m[cap:] = np.where(np.isnan(leaf), np.inf, leaf)
    width = cap
    while width > 1:
        half = width // 2
        ls, rs = s[width:2 * width:2], s[width + 1:2 * width:2]
        s[half:width] = ls + rs
        lm, rm = m[width:2 * width:2], m[width + 1:2 * width:2]
        m[half:width] = np.where(rm < lm, rm, lm)
        width = half
    return s, m


def max_priority(current: float, priorities, floor=FLOOR) -> float:
    p = np.maximum(np.asarray(priorities, dtype=f32).reshape(-1).astype(np.float64), floor)
    return float(max(float(current), float(p.max()))) if p.size else float(current)


def sample(sum_tree, u, B: int):
    """-> (indices [B], number of upper bounds outside [0, total + 1e-5]).
    Stratum i draws ub = u * (b - a) + a with a = segment * i, b = segment *
    (i + 1); from the root, go left iff left > ub, else subtract left and go
    right."""
    sum_tree = np.asarray(sum_tree, dtype=np.float64)
    cap = sum_tree.size // 2
    total = sum_tree[1]
    segment = total / B
    i = np.arange(B, dtype=np.float64)
    a = segment * i
    b = segment * (i + 1.0)
    ub = np.asarray(u, dtype=f32).reshape(-1)[:B].astype(np.float64) * (b - a) + a
    bad = int(np.count_nonzero(~((ub >= 0.0) & (ub <= total + 1e-5))))
    k = np.ones(B, dtype=np.int64)
    while k[0] < cap:  # every walk is log2(cap) steps long
        left = sum_tree[2 * k]
        go_left = left > ub
        ub = np.where(go_left, ub, ub - left)
        k = np.where(go_left, 2 * k, 2 * k + 1)
    return k - cap, bad


def weights(sum_tree, min_tree, indices, size: int, beta: float) -> np.ndarray:
    sum_tree = np.asarray(sum_tree, dtype=np.float64)
    cap = sum_tree.size // 2
    total = sum_tree[1]
    p_min = np.asarray(min_tree, dtype=np.float64)[1] / total
    max_weight = cref.libm_pow(np.array([p_min * size]), -beta)[0]
    p_sample = sum_tree[cap + np.asarray(indices, dtype=np.int64).reshape(-1)] / total
    with np.errstate(divide="ignore"):
        return (cref.libm_pow(p_sample * size, -beta) / max_weight).astype(f32)


# ---- the host's dispatch, restated ------------------------------------------------ #
SMALL_BATCH, TOP_LEVELS, BAND_LEVELS, DENSE_FACTOR, STAGE_BATCH, SAMPLES_PER_BLOCK = 1024, 11, 9, 32, 8192, 1024


def _levels(cap: int) -> int:
    return int(cap).bit_length() - 1


def route(cap: int, n: int, max_size: int | None = None) -> str:
    """The rebuild an add / update of ``n`` writes takes.  For an add pass
    ``max_size``: a ring longer than the buffer is cut to its last max_size
    writes before the dispatch.  "small" | "top-only" | "sparse-levels" |
    "bands(k1,k2,..)" with the band sizes bottom-up."""
    if max_size is not None:
        n = min(n, max_size)
    if n <= SMALL_BATCH:
        return "small"
    levels = _levels(cap)
    if levels <= TOP_LEVELS:
        return "top-only"
    if n * DENSE_FACTOR < cap:
        return "sparse-levels"
    bands, lo = [], levels
    while lo > TOP_LEVELS:
        k = min(lo - TOP_LEVELS, BAND_LEVELS)
        bands.append(k)
        lo -= k
    return "bands(" + ",".join(map(str, bands)) + ")"


def sample_variant(cap: int, B: int) -> str:
    """"walk": every level from HBM.  "staged-all": the whole sum tree above
    the leaves in LDS.  "staged-top(j)": the top 11 levels in LDS, j internal
    levels and the leaves from HBM."""
    if B < STAGE_BATCH:
        return "walk"
    levels = _levels(cap)
    return "staged-all" if levels <= TOP_LEVELS else f"staged-top({levels - TOP_LEVELS})"


# ---- one interface over the twin and both oracles --------------------------------- #
class Twin:
    """The functions above behind the interface the cases are run through."""

    def __init__(self, max_size: int, alpha: float) -> None:
        self.max_size, self.alpha, self.cap = max_size, alpha, capacity(max_size)
        self.leaf = empty_leaves(self.cap)
        self.maxp, self.size = 1.0, 0

    def set_max(self, v: float) -> None:
        self.maxp = float(v)

    def add(self, start: int, n: int) -> None:
        self.leaf = leaves(self.leaf, self.alpha, start=start, n=n, max_size=self.max_size, max_priority=self.maxp)
        self.size = min(self.size + n, self.max_size)

    def update(self, idx, pri) -> None:
        self.leaf = leaves(self.leaf, self.alpha, indices=idx, priorities=pri)
        self.maxp = max_priority(self.maxp, pri)

    def state(self):
        s, m = rebuild(self.leaf)
        return s, m, self.maxp

    def sample(self, u, beta: float):
        s, m = rebuild(self.leaf)
        idx, bad = sample(s, u, np.asarray(u).size)
        return idx, weights(s, m, idx, self.size, beta), bad


class COracle:
    """oracle.cref.PERTree: the C restatement of the reference's loops."""

    def __init__(self, max_size: int, alpha: float) -> None:
        self.t = cref.PERTree(max_size, alpha)

    def set_max(self, v: float) -> None:
        self.t.max_priority = float(v)

    def add(self, start: int, n: int) -> None:
        self.t.tree_ptr[0] = start
        self.t.add(n)

    def update(self, idx, pri) -> None:
        self.t.update(idx, pri)

    def state(self):
        return self.t.sum.copy(), self.t.min.copy(), float(self.t.max_priority)

    def sample(self, u, beta: float):
        idx, bad = self.t.sample(u)
        with np.errstate(divide="ignore"):
            return idx, self.t.weights(idx, beta), bad


@functools.lru_cache(maxsize=None)
def _py_full_ring(max_size: int, alpha: float):
    """oracle.per.PER after add(max_size) from its initial state: the one long
    Python loop several cases share.  Copied, never changed."""
    p = oper.PER(max_size, alpha)
    p.add(max_size)
    return p


class PyOracle:
    """oracle.per.PER: the Python restatement of the reference."""

    def __init__(self, max_size: int, alpha: float) -> None:
        self.p = oper.PER(max_size, alpha)
        self.fresh = True

    def set_max(self, v: float) -> None:
        self.p.max_priority = float(v)

    def add(self, start: int, n: int) -> None:
        if self.fresh and start == 0 and n == self.p.max_size and self.p.max_priority == 1.0:
            self.p = copy.deepcopy(_py_full_ring(self.p.max_size, self.p.alpha))
        else:
            self.p.tree_ptr = start
            self.p.add(n)
        self.fresh = False

    def update(self, idx, pri) -> None:
        self.fresh = False
        self.p.update_priorities(idx, pri)

    def state(self):
        return np.asarray(self.p.sum_tree.tree), np.asarray(self.p.min_tree.tree), float(self.p.max_priority)

    def sample(self, u, beta: float):
        """The reference asserts on a bound out of range; here the failed
        asserts are counted and the walk goes on, as in the C oracle."""
        u = np.asarray(u, dtype=f32).reshape(-1)
        B, tree = u.size, self.p.sum_tree
        total = tree.sum()
        segment = total / B
        out, bad = np.zeros(B, dtype=np.int64), 0
        for i in range(B):
            a = segment * i
            b = segment * (i + 1)
            ub = float(u[i]) * (b - a) + a
            try:
                out[i] = tree.retrieve(ub)
            except AssertionError:
                bad += 1
                k = 1
                while k < tree.capacity:
                    if tree.tree[2 * k] > ub:
                        k = 2 * k
                    else:
                        ub -= tree.tree[2 * k]
                        k = 2 * k + 1
                out[i] = k - tree.capacity
        return out, self._weights(out, beta), bad

    def _weights(self, idx, beta: float) -> np.ndarray:
        """PER.weights with ``x ** -beta`` of a zero leaf giving inf (libm's
        pow) where Python's float power raises."""
        p = self.p
        total = p.sum_tree.sum()
        max_weight = (p.min_tree.min() / total * p.size) ** -beta
        w = np.zeros(len(idx), dtype=f32)
        for i, j in enumerate(idx):
            base = p.sum_tree.tree[p.sum_tree.capacity + int(j)] / total * p.size
            w[i] = f32(np.inf) if base == 0.0 and beta > 0 else f32(base ** -beta / max_weight)
        return w


# ---- the cases --------------------------------------------------------------------- #
# A case is (max_size, alpha, ops).  An op is one of
#   ("set_max", value)
#   ("add", start, n, route)            route: the name route() must give
#   ("update", indices, priorities, route)
#   ("sample", u, beta, variant, bad)   variant: the name sample_variant() must
#                                       give; bad: how many bounds the inputs
#                                       push out of range
# After every add / update all nodes of both trees and max_priority are
# compared; after every sample the indices, the weights and the bad count.
U_TOP = float(np.nextafter(f32(1.0), f32(0.0)))  # the largest float32 below 1


def _seeded(name: str) -> np.random.Generator:
    return np.random.default_rng([ord(c) for c in name])


def _priorities(rng, n: int, scale: float = 1.0) -> np.ndarray:
    return (np.abs(rng.standard_normal(n)) * scale).astype(f32)


def _uniforms(rng, B: int) -> np.ndarray:
    """float32 uniforms in [0, 1) with exactly 0.0 and the largest float32
    below 1 at positions every prefix of 1023 or more keeps."""
    u = rng.random(B, dtype=f32)
    u[0], u[7] = 0.0, 0.0
    u[5], u[1000] = U_TOP, U_TOP
    u[B - 1] = U_TOP
    return u


def _stream_65536(ms: int):
    """The shared index / priority stream of the sparse-update cases: index 0,
    index ms - 1, a pair of sibling leaves and duplicates inside every prefix
    the cases use."""
    rng = _seeded("sparse-update")
    idx = rng.integers(0, ms, 2048).astype(np.int64)
    idx[0], idx[1], idx[2], idx[3] = 0, ms - 1, 1234, 1235
    idx[500:520] = idx[20:40]  # duplicates with different priorities
    idx[1024] = idx[0]  # index 0 again, from another block
    idx[2047] = idx[1]
    pri = _priorities(rng, 2048, 2.0)
    pri[40:50] = 1e-9  # below the floor
    return idx, pri


def _case_sparse_update(n: int):
    ms = 60_000
    idx, pri = _stream_65536(ms)
    return ms, 0.6, [("add", 0, ms, "bands(5)"),
                     ("update", idx[:n], pri[:n], "bands(5)" if n >= 2048 else "sparse-levels")]


def _case_sparse_add(start: int, n: int):
    ms = 60_000
    rng = _seeded("sparse-add")
    return ms, 0.6, [("add", 0, ms, "bands(5)"),
                     ("update", rng.integers(0, ms, 2048), _priorities(rng, 2048), "bands(5)"),
                     ("set_max", 2.5),
                     ("add", start, n, "sparse-levels")]


def _case_top_only(ms: int):
    rng = _seeded(f"top-only-{ms}")
    if ms == 2000:
        return ms, 0.6, [("set_max", 1.75), ("add", 1200, 1500, "top-only"),
                         ("update", rng.integers(0, ms, 3000), _priorities(rng, 3000, 2.0), "top-only")]
    return ms, 0.6, [("add", 0, ms, "small"),
                     ("update", rng.integers(0, ms, 1500), _priorities(rng, 1500, 2.0), "top-only")]


def _case_tiny(ms: int):
    """Trees of one and two leaves: levels 0 and 1."""
    rng = _seeded(f"tiny-{ms}")
    u = rng.random(8, dtype=f32)
    u[0], u[7] = 0.0, U_TOP
    return ms, 0.6, [("add", 0, ms, "small"),
                     ("update", np.arange(ms)[::-1].copy(), _priorities(rng, ms) + f32(0.5), "small"),
                     ("sample", u, 0.4, "walk", 0),
                     ("update", rng.integers(0, ms, 1500), _priorities(rng, 1500), "top-only"),
                     ("sample", u, 0.4, "walk", 0)]


def _case_one_level_band():
    ms = 4096
    rng = _seeded("one-level-band")
    idx = rng.integers(0, ms, 1025)
    idx[0], idx[1], idx[1024] = 0, ms - 1, 0
    return ms, 0.6, [("add", 0, ms, "bands(1)"), ("update", idx, _priorities(rng, 1025), "bands(1)")]


def _case_two_bands():
    ms = 2_000_000
    rng = _seeded("two-bands")
    idx = rng.integers(0, ms, 65_536)
    idx[0], idx[1], idx[65_535] = 0, ms - 1, 0
    idx[30_000:31_000] = idx[:1000]
    idx2 = rng.integers(0, ms, 4000)
    idx2[0], idx2[1], idx2[2], idx2[3], idx2[3999] = 0, ms - 1, 777_776, 777_777, ms - 1
    return ms, 0.6, [("add", 0, ms, "bands(9,1)"),
                     ("update", idx, _priorities(rng, 65_536, 2.0), "bands(9,1)"),
                     ("update", idx2, _priorities(rng, 4000, 3.0), "sparse-levels")]


def _case_long_ring(ms: int, start: int, n: int, want: str):
    rng = _seeded(f"long-ring-{ms}")
    return ms, 0.6, [("add", 0, 1000, "small"),
                     ("update", rng.integers(0, 1000, 100), _priorities(rng, 100, 3.0), "small"),
                     ("add", start, n, want)]


def _case_contended(n: int, distinct: int, want: str):
    ms = 60_000
    rng = _seeded(f"contended-{n}")
    targets = np.array([59_999, 0, 31_337])[:distinct]
    idx = targets[rng.integers(0, distinct, n)]
    pri = rng.permutation((1.0 + np.arange(n)) * 1e-3).astype(f32)  # pairwise distinct, above the floor
    return ms, 0.6, [("add", 0, ms, "bands(5)"), ("update", idx, pri, want)]


def _case_running_max(kind: str, n: int, start_max: float = 1.0):
    ms = 60_000
    rng = _seeded(f"running-max-{kind}-{n}")
    idx = rng.integers(0, ms, n)
    pri = rng.random(n, dtype=f32)  # all below 1
    ops = [("add", 0, ms, "bands(5)")]
    if kind == "last":  # the unique maximum at position n - 1
        pri[n - 1] = 7.5
    elif kind == "inner-wave":  # ... in the second, third and fourth 64 of a later block, one batch each
        want = "sparse-levels" if n * 32 < 65_536 else "bands(5)"
        for j, lane in enumerate((70, 130, 200)):
            pos = 256 * ((n // 256 - 1) // (j + 1)) + lane
            assert pos < n and pos // 256 > 0
            p = rng.random(n, dtype=f32)
            p[pos] = 7.5 + j  # above everything before it
            ops.append(("update", rng.integers(0, ms, n), p, want))
        return ms, 0.6, ops
    elif kind == "below-current":
        ops.append(("set_max", 50.123))
    elif kind == "below-floor":
        pri = (rng.random(n, dtype=f32) * f32(9e-6) + f32(1e-7)).astype(f32)
        ops.append(("set_max", start_max))
    ops.append(("update", idx, pri, "sparse-levels" if n * 32 < 65_536 else "bands(5)"))
    return ms, 0.6, ops


SHALLOW_B = (8191, 8192, 8193, 9216)


def _case_staged_shallow(ms: int, fill: int):
    """A shallow tree filled (``fill`` < ms: partly), updated with random
    priorities, then sampled at every B from one stream's prefixes."""
    cap = capacity(ms)
    rng = _seeded(f"staged-shallow-{ms}")
    n = min(fill, 1000)
    ops = [("add", 0, fill, route(cap, fill, ms)),
           ("update", rng.permutation(fill)[:n], _priorities(rng, n, 2.0) + f32(1e-3), "small")]
    u = _uniforms(rng, max(SHALLOW_B))
    for B in SHALLOW_B:
        ub = u[:B].copy()
        ub[B - 1] = U_TOP
        staged = "staged-all" if cap <= 2048 else "staged-top(1)"
        ops.append(("sample", ub, 0.4, "walk" if B == 8191 else staged, 0))
    return ms, 0.6, ops


DEEP_B = (1023, 1024, 1025, 8192)


def _case_sample_deep():
    ms = 60_000
    rng = _seeded("sample-deep")
    ops = [("add", 0, ms, "bands(5)"),
           ("update", rng.integers(0, ms, 2048), _priorities(rng, 2048, 2.0), "bands(5)")]
    u = _uniforms(rng, max(DEEP_B))
    for B in DEEP_B:
        ub = u[:B].copy()
        ub[B - 1] = U_TOP
        ops.append(("sample", ub, 0.4, "walk" if B < 8192 else "staged-top(5)", 0))
    return ms, 0.6, ops


def _case_error_counter(staged: bool):
    """Bounds pushed out of range: negative in the first two strata, beyond
    the total in the last three, each by a quarter of a stratum or more (a
    stratum is 0.1 wide or wider here, the slack only 1e-5)."""
    ms, B = (2000, 8192) if staged else (60_000, 1000)
    cap = capacity(ms)
    rng = _seeded(f"error-counter-{staged}")
    n = 1000
    u = rng.random(B, dtype=f32)
    u[0], u[1] = -0.5, -1.5
    u[B - 1], u[B - 2], u[B - 3] = 1.5, 2.25, 3.5
    return ms, 0.6, [("add", 0, ms, route(cap, ms, ms)),
                     ("update", rng.permutation(ms)[:n], _priorities(rng, n, 2.0) + f32(1e-3), "small"),
                     ("sample", u, 0.4, "staged-all" if staged else "walk", 5)]


def _case_exponents(alpha: float):
    ms = 60_000
    rng = _seeded(f"exponents-{alpha}")
    u = _uniforms(rng, 1025)
    pri = _priorities(rng, 2048, 2.0)
    pri[:4] = [1e-5, 1.0, 1e-9, 2.0]
    return ms, alpha, [("set_max", 2.5), ("add", 0, ms, "bands(5)"),
                       ("update", rng.integers(0, ms, 2048), pri, "bands(5)"),
                       ("sample", u, 0.0, "walk", 0), ("sample", u, 1.0, "walk", 0)]


CASES = {
    "sparse-update-1025": lambda: _case_sparse_update(1025),
    "sparse-update-2047": lambda: _case_sparse_update(2047),
    "dense-update-2048": lambda: _case_sparse_update(2048),
    "sparse-add-wrap": lambda: _case_sparse_add(59_500, 1500),
    "sparse-add-from-0": lambda: _case_sparse_add(0, 1100),
    "top-only-cap2048": lambda: _case_top_only(2000),
    "top-only-cap256": lambda: _case_top_only(200),
    "tiny-1": lambda: _case_tiny(1),
    "tiny-2": lambda: _case_tiny(2),
    "one-level-band": _case_one_level_band,
    "two-bands": _case_two_bands,
    "long-ring-cap2048": lambda: _case_long_ring(1500, 700, 4000, "top-only"),
    "long-ring-cap65536": lambda: _case_long_ring(40_000, 39_000, 100_000, "bands(5)"),
    "contended-3-leaves": lambda: _case_contended(3000, 3, "bands(5)"),
    "contended-1-leaf": lambda: _case_contended(1500, 1, "sparse-levels"),
    "max-last-1500": lambda: _case_running_max("last", 1500),
    "max-last-5000": lambda: _case_running_max("last", 5000),
    "max-inner-wave-1500": lambda: _case_running_max("inner-wave", 1500),
    "max-inner-wave-5000": lambda: _case_running_max("inner-wave", 5000),
    "max-below-current-1500": lambda: _case_running_max("below-current", 1500),
    "max-below-current-5000": lambda: _case_running_max("below-current", 5000),
    "max-below-floor-from-above-1500": lambda: _case_running_max("below-floor", 1500, 1.0),
    "max-below-floor-from-above-5000": lambda: _case_running_max("below-floor", 5000, 1.0),
    "max-below-floor-from-below-1500": lambda: _case_running_max("below-floor", 1500, 1e-6),
    "max-below-floor-from-below-5000": lambda: _case_running_max("below-floor", 5000, 1e-6),
    "staged-shallow-cap256": lambda: _case_staged_shallow(200, 200),
    "staged-shallow-cap2048-partly-filled": lambda: _case_staged_shallow(2000, 1500),
    "staged-shallow-cap4096": lambda: _case_staged_shallow(4096, 4096),
    "sample-deep-cap65536": _case_sample_deep,
    "error-counter-walk": lambda: _case_error_counter(False),
    "error-counter-staged": lambda: _case_error_counter(True),
    "exponents-alpha0.0": lambda: _case_exponents(0.0),
    "exponents-alpha0.4": lambda: _case_exponents(0.4),
    "exponents-alpha1.0": lambda: _case_exponents(1.0),
}


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(max_size, alpha, ops) of a CASES entry.  Treat as read-only."""
    ms, alpha, ops = CASES[name]()
    fixed = []
    for op in ops:
        if op[0] == "update":
            op = ("update", np.ascontiguousarray(op[1], dtype=np.int64), np.ascontiguousarray(op[2], dtype=f32), op[3])
        elif op[0] == "sample":
            op = ("sample", np.ascontiguousarray(op[1], dtype=f32), *op[2:])
        fixed.append(op)
    return ms, alpha, tuple(fixed)


def op_route(ms: int, op) -> tuple[str, str]:
    """(the path the host takes for this op, the path the case lists it under)."""
    cap = capacity(ms)
    if op[0] == "add":
        return route(cap, op[2], ms), op[3]
    if op[0] == "update":
        return route(cap, op[1].size), op[3]
    if op[0] == "sample":
        return sample_variant(cap, op[1].size), op[3]
    return "", ""


def run(backend, ops) -> list:
    """Feed a case's ops to a backend (Twin, COracle, PyOracle or the GPU
    driver of the GPU tests).  -> one record per add / update, (sum tree, min
    tree, max_priority), and per sample, (indices, weights, bad)."""
    out = []
    for op in ops:
        if op[0] == "set_max":
            backend.set_max(op[1])
        elif op[0] == "add":
            backend.add(op[1], op[2])
            out.append(backend.state())
        elif op[0] == "update":
            backend.update(op[1], op[2])
            out.append(backend.state())
        else:
            out.append(backend.sample(op[1], op[2]))
    return out


@functools.lru_cache(maxsize=None)
def expected(name: str) -> list:
    """The C oracle's records of a case: what the kernels are held to.
    Computed once; treat as read-only."""
    ms, alpha, ops = case(name)
    return run(COracle(ms, alpha), ops)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def python_oracle_fits(name: str) -> bool:
    """Small enough for oracle.per.PER's Python loops: cap <= 2^16, and at most
    about a second of writes beyond the full-ring add the cases share."""
    ms, _, ops = case(name)
    if capacity(ms) > 1 << 16:
        return False
    writes = 0
    for j, op in enumerate(ops):
        if op[0] == "add" and not (j == 0 and op[1] == 0 and op[2] == ms):
            writes += op[2]
        elif op[0] == "update":
            writes += op[1].size
    return writes <= 110_000
