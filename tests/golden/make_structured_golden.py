#!/usr/bin/env python3
"""Record tests/golden/structured_compose.npz from the reference's OWN LatentGaussianModel (scene/latent_gaussian_model.py), run on
the CPU of the authoring container only: the reference does not exist where the tests run, and no test runs this script.

The reference's model imports on a machine without its CUDA extensions once `simple_knn`, `simple_knn._C` and `plyfile` are
stubbed in sys.modules (the model's forward touches none of them).  For two small configurations with fixed seeds it stores
  state/<name>   the model's state_dict
  out/<name>     the six composed tensors (_xyz, _opacity, _scaling, _rotation, _features_dc, _features_rest) and `returned`,
                 the [P, D] array forward() returns
  w/<name>       the weights of one fixed linear functional  L = sum_name <w[name], out[name]>  of the six composed tensors
  grad/<name>    dL/d(parameter) for every parameter
Only data is stored, no source.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_structured_golden.py PATH_TO_THE_REFERENCE_CHECKOUT
"""
import os
import sys
import types

import numpy as np
import torch

if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "scene", "latent_gaussian_model.py")):
    sys.exit(__doc__)
REF = os.path.abspath(sys.argv[1])
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
for name in ("simple_knn", "simple_knn._C", "plyfile"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["simple_knn._C"].distCUDA2 = None
sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = None

from scene.latent_gaussian_model import LatentGaussianModel  # noqa: E402

CASES = (dict(name="b5_k8_deg0", B=5, K=8, deg=0, pos=False, seed=11), dict(name="b4_k3_deg1_pos", B=4, K=3, deg=1, pos=True, seed=12))
LATENT, HIDDEN = 16, 8       # (the defaults are 32: smaller layers keep the file at a few tens of KB)
COMPOSED = ("_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest")


def record(case, out):
    torch.manual_seed(case["seed"])
    model = LatentGaussianModel(case["deg"], torch.randn(case["B"], 3), latent_size=LATENT, hidden_size=HIDDEN,
                                gaussians_per_structure=case["K"], use_positional_embedding=case["pos"])
    with torch.no_grad():                       # away from the constructor's constants: every rule gets a generic input
        model.structure_opacities.add_(torch.randn(case["B"], 1) * 0.5)
        model.structure_scales.add_(torch.randn(case["B"], 3) * 0.5)
    pre = case["name"] + "/"
    for k, v in model.state_dict().items():
        out[pre + "state/" + k] = v.detach().numpy().copy()
    returned = model.forward()
    out[pre + "out/returned"] = returned.detach().numpy().copy()
    g = torch.Generator().manual_seed(case["seed"] + 100)
    loss = 0.0
    for k in COMPOSED:
        t = getattr(model, k)
        w = torch.randn(t.shape, generator=g)
        out[pre + "out/" + k] = t.detach().numpy().copy()
        out[pre + "w/" + k] = w.numpy().copy()
        loss = loss + (t * w).sum()
    loss.backward()
    for k, p in model.named_parameters():
        out[pre + "grad/" + k] = p.grad.numpy().copy()
    out[pre + "meta"] = np.array([case["B"], case["K"], case["deg"], int(case["pos"]), LATENT, HIDDEN], dtype=np.int64)


if __name__ == "__main__":
    arrays = {}
    for case in CASES:
        record(case, arrays)
    path = os.path.join(OUT, "structured_compose.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")
