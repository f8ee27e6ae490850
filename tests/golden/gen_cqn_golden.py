"""Generate the CQN golden vectors from the reference's OWN ``CQN.learn``.

Test infrastructure only, in the manner of gen_matd3_golden.py (the import
stubs and path loader are gen_golden.py's): the reference source file is
executed in place, nothing of it is copied, and only seeded inputs and the
outputs the reference produced are written — ``cqn_0..5.npz``, ``cqn_nan.npz``
and ``META_cqn.json`` beside this script.  Skips cleanly when the reference
checkout is absent.

Reference function exercised (path relative to the reference checkout):
  * agilerl/algorithms/cqn.py:216-265   CQN.learn (max / argmax + gather over Q(s'), y, logsumexp,
                                        the two means, MSE, the combined loss and its backward pass)

``learn`` runs unbound on an ``object.__new__`` stand-in whose ``actor`` /
``actor_target`` return fixed seeded tensors; ``criterion`` records y and the
optimizer stub's ``step`` records dLoss/dQ(s).

META_cqn.json also records, per case, the error of that float32 evaluation
against a float64 evaluation of the same formula (torch ops on float64
tensors, y taken as the reference produced it): ``err_ref_loss``,
``err_ref_grad`` (max abs over elements) and ``err_ref_terms`` (mean lse,
mean Q, MSE; the float32 terms from the torch ops the reference's lines call).  The
tests' bounds are multiples of these.

Usage:  python tests/golden/gen_cqn_golden.py --ref <reference checkout>
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import _install_stubs, _load  # noqa: E402

# (B, A, double, gamma, seed): one row; a part-filled wave; one wave; a second block of one row;
# more columns than a wave's half (the kernel's row-per-wave form); four blocks
CASES = [(1, 1, False, 0.99, 401), (33, 2, True, 0.95, 402), (64, 4, False, 0.99, 403), (257, 6, True, 0.9, 404),
         (64, 33, False, 0.99, 405), (1024, 6, True, 0.99, 406)]
NAN_CASE = (33, 6, False, 0.95, 407)  # a NaN in q_next_target on a live row, a NaN in one row of q_cur


def _inputs(B: int, A: int, seed: int, nan: bool) -> dict:
    rng = np.random.default_rng(seed)
    q = lambda: (3.0 * rng.standard_normal((B, A))).astype(np.float32)  # noqa: E731
    rec = dict(q_next_online=q(), q_next_target=q(), q_cur=q(),
               a=rng.integers(0, A, (B, 1)).astype(np.int64), r=rng.standard_normal((B, 1)).astype(np.float32),
               d=(rng.random((B, 1)) < 0.2).astype(np.float32))
    if nan:
        rec["d"][2, 0] = 0.0
        rec["q_next_target"][2, 3] = np.nan  # a live row: y is NaN there
        rec["q_cur"][5, 1] = np.nan
    return rec


def _terms(q: torch.Tensor, actions: np.ndarray, y: torch.Tensor) -> list:
    """(mean lse, mean Q, MSE of the taken action's value against y) in q's dtype."""
    taken = torch.take_along_dim(q, torch.as_tensor(actions), 1)
    return [torch.logsumexp(q, 1).mean(), q.mean(), torch.nn.functional.mse_loss(taken, y.to(q.dtype))]


def _f64(rec: dict, y: np.ndarray):
    """The same formula on float64 tensors, y as given -> (terms, loss, grad)."""
    q = torch.tensor(rec["q_cur"], dtype=torch.float64, requires_grad=True)
    terms = _terms(q, rec["a"], torch.tensor(y))
    loss = (terms[0] - terms[1]) + 0.5 * terms[2]
    loss.backward()
    return np.array([t.item() for t in terms]), loss.item(), q.grad.numpy()


def _run(CQN, B: int, A: int, double: bool, gamma: float, seed: int, nan: bool = False):
    rec = _inputs(B, A, seed, nan)
    Q = torch.tensor(rec["q_cur"], requires_grad=True)
    states, next_states = torch.zeros(B, 1), torch.ones(B, 1)
    got: dict = {}

    class _Net:
        def __init__(self, on_next, on_cur=None):
            self.on_next, self.on_cur = on_next, on_cur

        def __call__(self, x):
            return self.on_next if x is next_states else self.on_cur

        def parameters(self):
            return []

    class _Opt:
        def zero_grad(self):
            Q.grad = None

        def step(self):
            got["g_q"] = Q.grad.clone()

    class _Crit:
        def __call__(self, value, target):
            got["y"] = target.detach().clone()
            return torch.nn.functional.mse_loss(value, target)

    fake = object.__new__(CQN)
    fake.gamma, fake.double, fake.accelerator = gamma, double, None
    fake.preprocess_observation = lambda x: x
    fake.actor = _Net(torch.tensor(rec["q_next_online"]), Q)
    fake.actor_target = _Net(torch.tensor(rec["q_next_target"]))
    fake.optimizer, fake.criterion = _Opt(), _Crit()
    fake.soft_update = lambda: None
    loss = CQN.learn(fake, (states, torch.tensor(rec["a"]), torch.tensor(rec["r"]), next_states,
                            torch.tensor(rec["d"])))
    y, g_q = got["y"].numpy(), got["g_q"].numpy()
    # the three terms in float32, from the same torch ops the reference's lines call
    with torch.no_grad():
        terms32 = np.array([t.item() for t in _terms(torch.tensor(rec["q_cur"]), rec["a"], got["y"])])
    rec.update(gamma=np.float64(gamma), double=np.bool_(double), y=y, g_q=g_q, loss=np.float32(loss),
               terms=terms32.astype(np.float32))
    if nan:
        assert np.isnan(y[2, 0]) and np.isnan(y).sum() == 1 and np.isnan(loss)
        assert np.isnan(g_q[5]).all() and np.isnan(g_q[2, int(rec["a"][2, 0])])
        return rec, None
    assert np.isfinite(y).all() and np.isfinite(g_q).all() and np.isfinite(loss)
    assert (rec["d"] == 1).any() or B == 1
    terms64, loss64, grad64 = _f64(rec, y)
    err = dict(err_ref_loss=abs(float(np.float32(loss)) - loss64),
               err_ref_grad=float(np.max(np.abs(g_q.astype(np.float64) - grad64))),
               err_ref_terms=[abs(float(a) - float(b)) for a, b in zip(terms32.astype(np.float32), terms64)])
    return rec, err


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=None, help="the reference checkout (the directory that holds agilerl/)")
    args = ap.parse_args()
    ref = args.ref
    if ref is None or not os.path.isdir(os.path.join(ref, "agilerl")):
        print("reference checkout not present; nothing generated")
        return
    torch.set_num_threads(1)
    _install_stubs()
    cqn = _load(ref, "agilerl.algorithms.cqn", "agilerl/algorithms/cqn.py")

    groups: dict[str, dict] = {}
    errors: dict[str, dict] = {}
    for k, case in enumerate(CASES):
        groups[f"cqn_{k}"], errors[f"cqn_{k}"] = _run(cqn.CQN, *case)
    groups["cqn_nan"], _ = _run(cqn.CQN, *NAN_CASE, nan=True)
    for name, rec in groups.items():
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **rec)
    meta = {"generator": "tests/golden/gen_cqn_golden.py", "torch": torch.__version__, "numpy": np.__version__,
            "python": sys.version.split()[0], "groups": sorted(groups),
            "shapes": {n: [int(r["q_cur"].shape[0]), int(r["q_cur"].shape[1]), bool(r["double"])]
                       for n, r in groups.items()},
            "errors": errors,
            "errors_yardstick": "the reference's float32 outputs against the same formula in torch float64 ops "
                                "(y as the reference produced it); another float64 evaluation, such as the numpy "
                                "twin's, differs from that one by float64 rounding",
            "reference_lines": {"agilerl/algorithms/cqn.py": "216-265 (CQN.learn)"}}
    with open(os.path.join(HERE, "META_cqn.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", len(groups), "fixtures")


if __name__ == "__main__":
    main()
