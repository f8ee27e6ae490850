"""Generate the MultiBinary-PPO golden vectors (PPO over MultiBinary action
spaces) from the reference's OWN distribution functions.

Test infrastructure only, in the manner of gen_multidisc_golden.py (it borrows
gen_golden.py's import stubs and path loader): the reference's
``utils/torch_utils.py`` and ``networks/distributions.py`` are executed in
place, nothing of them is copied, and only seeded inputs and the outputs the
reference produced are written — ``multibinary_0..4.npz`` and
``META_multibinary.json`` beside this script.  Exits cleanly when the reference
checkout is absent.

Reference functions exercised (paths relative to the reference checkout):
  * agilerl/utils/torch_utils.py:348-364     log_prob_multi_binary
  * agilerl/utils/torch_utils.py:367-376     entropy_multi_binary
  * agilerl/networks/distributions.py:16-28  apply_action_mask_discrete
and torch autograd (float64) of the agilerl/algorithms/ppo.py:868-902 loss
over them — the loss as tests/gauss_twin.py ``torch_loss`` writes it with
torch ops — for the gradients of the raw logits and the value.  Inputs are
float32 values (tests/multibinary_twin.py ``loss_inputs``: value / adv rows on
the maximum ties and on the closed clamp edges, taken from
gauss_twin.loss_inputs) evaluated in float64, so the expected outputs carry no
float32 rounding of their own.

Usage:  python tests/golden/gen_multibinary_golden.py --ref <reference checkout>
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
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from gen_golden import _install_stubs, _load  # noqa: E402

# (n, b, nmb, rollout rows or None, seed, clip, vf, ent, masked)
CASES = [(1, 1, 1, None, 501, 0.25, 0.5, 0.01, False),
         (5, 5, 3, None, 502, 0.25, 0.5, 0.01, False),
         (16, 16, 2, 40, 503, 0.125, 0.7, 0.02, True),    # the 16-lane boundary, a gather index and masks
         (17, 8, 2, None, 504, 0.25, 0.5, 0.02, True),    # one bit into the lanes' second logits, masked
         (32, 7, 2, 20, 505, 0.25, 0.5, 0.0, False)]      # full width, a gather index


def _case(tu, dist, n, b, nmb, rows, seed, clip, vf, ent, with_mask) -> dict:
    from tests.gauss_twin import torch_loss
    from tests.multibinary_twin import loss_inputs

    rec = loss_inputs(n, b, nmb, rows, seed, clip, with_mask)
    t64 = lambda k: torch.tensor(rec[k], dtype=torch.float64)  # noqa: E731
    logits, value = (t64(k).requires_grad_(True) for k in ("logits", "value"))
    S = b * nmb
    src = torch.arange(S) if rec["index"] is None else torch.tensor(rec["index"])
    olp, adv, ret, ov = (t64(k)[src] for k in ("old_logp", "adv", "ret", "old_v"))
    act = torch.tensor(rec["actions"])[src]
    lg = logits
    if with_mask:
        lg = dist.apply_action_mask_discrete(logits, torch.tensor(rec["mask"])[src].bool())
    logp = tu.log_prob_multi_binary(lg, act)
    entropy = tu.entropy_multi_binary(lg)
    losses, kls = [], []
    for m in range(nmb):
        s = slice(m * b, (m + 1) * b)
        loss, kl = torch_loss(logp[s], entropy[s], value[s], olp[s], adv[s], ret[s], ov[s], clip, vf, ent)
        losses.append(loss)
        kls.append(kl)
    torch.stack(losses).sum().backward()
    out = {k: v for k, v in rec.items() if v is not None}
    out.update(n=n, b=b, clip=clip, vf=vf, ent=ent, logp=logp.detach().numpy(),
               entropy=entropy.detach().numpy(), loss=torch.stack(losses).detach().numpy(),
               approx_kl=torch.stack(kls).numpy(), g_logits=logits.grad.numpy(), g_value=value.grad.numpy())
    if with_mask:
        out["masked_logits"] = lg.detach().numpy()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("AGX_REFERENCE", ""))
    args = ap.parse_args()
    if not args.ref or not os.path.isdir(os.path.join(args.ref, "agilerl")):
        print("reference checkout not present; nothing generated")
        return
    torch.set_num_threads(1)
    _install_stubs()
    tu = _load(args.ref, "agilerl.utils.torch_utils", "agilerl/utils/torch_utils.py")
    dist = _load(args.ref, "agilerl.networks.distributions", "agilerl/networks/distributions.py")
    for i, case in enumerate(CASES):
        np.savez_compressed(os.path.join(HERE, f"multibinary_{i}.npz"), **_case(tu, dist, *case))
    with open(os.path.join(HERE, "META_multibinary.json"), "w") as f:
        json.dump({"generator": "tests/golden/gen_multibinary_golden.py", "torch": torch.__version__,
                   "numpy": np.__version__,
                   "cases": [list(c) for c in CASES],
                   "case_fields": ["n", "b", "nmb", "rows", "seed", "clip", "vf", "ent", "masked"]}, f, indent=1)
    print("wrote", len(CASES), "fixtures")


if __name__ == "__main__":
    main()
