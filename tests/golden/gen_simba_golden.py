"""Golden vectors for SimBa encoders, from the reference's OWN code.

Test infrastructure only, under the rules of gen_arch_golden.py, whose
path-loader and stand-ins this reuses: the reference's files are executed in
place, and only seeded inputs and the outputs the reference produced are
written (tests/golden/simba_ref.npz).  On top of gen_arch_golden's set-up it
path-loads agilerl/modules/simba.py and hands its EvolvableSimBa to
agilerl/networks/base.py.

Written: the seeded state dict of EvolvableSimBa(6, 8, hidden 16, 2 blocks),
an input and the output, the parameter shapes and values after add_node(16),
add_block() and remove_block() at the minimum, and the mutation table of a
QNetwork(simba=True) under PYTHONHASHSEED=0.

Usage:  python tests/golden/gen_simba_golden.py [--ref /root/reference]
"""

from __future__ import annotations

import os
import subprocess
import sys

HASH_SEED = "0"
if __name__ == "__main__" and os.environ.get("PYTHONHASHSEED") != HASH_SEED:
    sys.exit(subprocess.call([sys.executable, *sys.argv], env={**os.environ, "PYTHONHASHSEED": HASH_SEED}))

import argparse  # noqa: E402

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_arch_golden as G  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ref = ap.parse_args().ref
    if not os.path.isdir(ref):
        sys.exit(f"{ref}: reference checkout not found")
    m = G._setup(ref)
    sb = G._load(ref, "agilerl.modules.simba", "agilerl/modules/simba.py")
    sys.modules["agilerl.modules"].EvolvableSimBa = sb.EvolvableSimBa
    m["nb"].EvolvableSimBa = sb.EvolvableSimBa
    out: dict[str, np.ndarray] = {}

    def put(tag: str, net) -> None:
        sd = net.state_dict()
        out[f"{tag}_keys"] = np.array(list(sd))
        for k, v in sd.items():
            out[f"{tag}/{k}"] = v.numpy().copy()

    torch.manual_seed(0)
    net = sb.EvolvableSimBa(num_inputs=6, num_outputs=8, hidden_size=16, num_blocks=2, random_seed=0)
    put("init", net)
    x = torch.randn(5, 6, generator=torch.Generator().manual_seed(1))
    out["x"] = x.numpy()
    with torch.no_grad():
        out["y"] = net(x).numpy()
    torch.manual_seed(2)
    net.add_node(numb_new_nodes=16)
    put("add_node", net)
    net.add_block()
    put("add_block", net)
    one = sb.EvolvableSimBa(num_inputs=6, num_outputs=8, hidden_size=16, num_blocks=1, random_seed=0)
    one.remove_block()  # at the minimum: falls back to add_node
    out["remove_block_min"] = np.array([one.num_blocks, one.hidden_size, int(one.last_mutation_attr == "add_node")])
    q = m["qnets"].QNetwork(G.Box(-1.0, 1.0, (8,)), G.Discrete(4), simba=True)
    out["qnetwork_methods"] = np.array(list(q.mutation_methods))
    out["qnetwork_encoder"] = np.array([q.encoder.hidden_size, q.encoder.num_blocks])
    np.savez_compressed(os.path.join(HERE, "simba_ref.npz"), **out)
    print("wrote simba_ref.npz:", len(out), "arrays; table", list(out["qnetwork_methods"]))


if __name__ == "__main__":
    main()
