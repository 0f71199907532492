"""Golden vectors of the reference's own ``pairwise_cosine_similarity`` (manner/models/components/utils.py:4-31, plain torch) ->
tests/golden/miner_step.npz.

Run in the build container only, like its siblings, with the reference checkout given on the command line (or in MANNER_REFERENCE):

    python tests/golden/make_golden_miner_step.py <reference checkout>

The function is loaded from its file (it needs torch only), run in float32 at (B, K, D) = (3, 5, 64) with one all-zero row, with and
without ``zero_diagonal``; the inputs, both matrices, the ``.mean()`` MINERModule.model_step takes (baselines/miner_module.py:237-241) and
the autograd gradient of that mean are stored.  Only data goes into the fixture; no test reads the reference.

There is no golden of the category bias: ``MINERModule`` itself cannot be imported in the build container (lightning, torchmetrics and
torch_geometric are absent), and the bias is computed by torchmetrics' ``pairwise_cosine_similarity``, not by this function.
tests/miner_step_ref.py restates those lines instead and says so.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
B, K, D, ZERO_ROW, SEED = 3, 5, 64, (1, 3), 67


def reference_function(root):
    path = os.path.join(root, "manner", "models", "components", "utils.py")
    spec = importlib.util.spec_from_file_location("reference_components_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.pairwise_cosine_similarity


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MANNER_REFERENCE")
    if not root:
        raise SystemExit("usage: make_golden_miner_step.py <reference checkout>")
    sys.dont_write_bytecode = True
    fn = reference_function(root)
    x = torch.from_numpy(np.random.default_rng(SEED).standard_normal((B, K, D)).astype(np.float32))
    x[ZERO_ROW] = 0.0
    leaf = x.clone().requires_grad_(True)
    zeroed = fn(leaf, leaf, zero_diagonal=True)
    loss = zeroed.mean()
    loss.backward()
    with torch.no_grad():
        full = fn(x.clone(), x.clone())
    np.savez(os.path.join(HERE, "miner_step.npz"), user=x.numpy(), distance=full.numpy(), distance_zero_diagonal=zeroed.detach().numpy(),
             loss=loss.detach().numpy(), d_user=leaf.grad.numpy(),
             meta=json.dumps({"source": "reference pairwise_cosine_similarity (components/utils.py:4-31), float32, torch " + torch.__version__,
                              "shape": [B, K, D], "zero_row": list(ZERO_ROW), "seed": SEED}))


if __name__ == "__main__":
    main()
