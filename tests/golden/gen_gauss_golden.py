"""Generate the Gaussian-PPO golden vectors (PPO over Box action spaces) from
the reference's OWN distribution functions.

Test infrastructure only, in the manner of gen_golden.py (whose import stubs
and path loader it borrows): the reference's ``utils/torch_utils.py`` is
executed in place, nothing of it is copied, and only seeded inputs and the
outputs the reference produced are written — ``gauss_0..3.npz`` and
``META_gauss.json`` beside this script.  Exits cleanly when the reference
checkout is absent.

Reference functions exercised (paths relative to the reference checkout):
  * agilerl/utils/torch_utils.py:225-244  log_prob_continuous
  * agilerl/utils/torch_utils.py:247-257  entropy_continuous
and torch autograd (float64) of the agilerl/algorithms/ppo.py:868-902 loss
over them — the loss as tests/gauss_twin.py ``torch_loss`` writes it with
torch ops — for the gradients of mean, value and log_std.  Inputs are float32
values (tests/gauss_twin.py ``loss_inputs``: rows on the maximum ties and on
the closed clamp edges included) evaluated in float64, so the expected
outputs carry no float32 rounding of their own.

Parameter order of a reference ``StochasticActor`` over a Box space: the
networks package cannot be imported under the stubs (EvolvableNetwork needs
the real agilerl.modules / tensordict / gymnasium), so the order is pinned by
reading networks/distributions.py:152-156: ``log_std`` is a parameter of the
EvolvableDistribution wrapper itself and the wrapped MLP is its submodule
``_wrapped``, so ``nn.Module.named_parameters`` yields ``head_net.log_std``
before every ``head_net._wrapped.*`` (and after ``encoder.*``, registered
first).  META_gauss.json records that order for a default actor head.

Usage:  python tests/golden/gen_gauss_golden.py --ref <reference checkout>
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

# (A, b, nmb, rollout rows or None, seed, clip, vf, ent)
CASES = [(1, 1, 1, None, 301, 0.25, 0.5, 0.01), (3, 5, 3, None, 302, 0.25, 0.5, 0.01),
         (6, 16, 2, 40, 303, 0.125, 0.7, 0.02), (17, 8, 2, None, 304, 0.25, 0.5, 0.0)]

ACTOR_PARAMETER_ORDER = [
    "encoder.*", "head_net.log_std", "head_net._wrapped.model.actor_linear_layer_1.weight",
    "head_net._wrapped.model.actor_linear_layer_1.bias", "head_net._wrapped.model.actor_layer_norm_1.weight",
    "head_net._wrapped.model.actor_layer_norm_1.bias", "head_net._wrapped.model.actor_linear_layer_output.weight",
    "head_net._wrapped.model.actor_linear_layer_output.bias"]


def _case(tu, A, b, nmb, rows, seed, clip, vf, ent) -> dict:
    from tests.gauss_twin import loss_inputs, torch_loss

    rec = loss_inputs(A, b, nmb, rows, seed, clip)
    t64 = lambda k: torch.tensor(rec[k], dtype=torch.float64)  # noqa: E731
    mean, value, log_std = (t64(k).requires_grad_(True) for k in ("mean", "value", "log_std"))
    S = b * nmb
    src = torch.arange(S) if rec["index"] is None else torch.tensor(rec["index"])
    act, olp, adv, ret, ov = (t64(k)[src] for k in ("actions", "old_logp", "adv", "ret", "old_v"))
    ls = log_std.repeat_interleave(b, 0)
    logp = tu.log_prob_continuous(mean, ls, act)
    entropy = tu.entropy_continuous(mean, ls)
    losses, kls = [], []
    for m in range(nmb):
        s = slice(m * b, (m + 1) * b)
        loss, kl = torch_loss(logp[s], entropy[s], value[s], olp[s], adv[s], ret[s], ov[s], clip, vf, ent)
        losses.append(loss)
        kls.append(kl)
    torch.stack(losses).sum().backward()
    out = {k: v for k, v in rec.items() if v is not None}
    out.update(b=b, clip=clip, vf=vf, ent=ent, logp=logp.detach().numpy(), entropy=entropy.detach().numpy(),
               loss=torch.stack(losses).detach().numpy(), approx_kl=torch.stack(kls).numpy(),
               g_mean=mean.grad.numpy(), g_value=value.grad.numpy(), g_log_std=log_std.grad.numpy())
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(args.ref, "agilerl")):
        print("reference checkout not present; nothing generated")
        return
    torch.set_num_threads(1)
    _install_stubs()
    tu = _load(args.ref, "agilerl.utils.torch_utils", "agilerl/utils/torch_utils.py")
    for i, case in enumerate(CASES):
        np.savez_compressed(os.path.join(HERE, f"gauss_{i}.npz"), **_case(tu, *case))
    with open(os.path.join(HERE, "META_gauss.json"), "w") as f:
        json.dump({"generator": "tests/golden/gen_gauss_golden.py", "torch": torch.__version__,
                   "numpy": np.__version__, "cases": [list(c) for c in CASES],
                   "actor_parameter_order": ACTOR_PARAMETER_ORDER,
                   "actor_parameter_order_source": "read from networks/distributions.py:152-156 (the networks "
                                                   "package does not import under the generator's stubs)"}, f, indent=1)
    print("wrote", len(CASES), "fixtures")


if __name__ == "__main__":
    main()
