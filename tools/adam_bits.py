"""The bits of one Adam step, to compare two builds of libgsrast.so (GSR_LIB_PATH selects the library; one fresh process per library):

  python tools/adam_bits.py dump OUT.npz    on the GPU: p', m', v' of one step from the seeded states of tests/training_ref.py through
                                            adam_step_multi and adam_step_sparse_multi (bool and int32 masks, some rows hidden)
  python tools/adam_bits.py cmp A.npz B.npz on the host: per case, the elements whose bits differ, split into those a float4 covers
                                            (index < n - n % 4) and the trailing n % 4

Cases: every training_ref.adam_cases() entry, the eight-tensor launch, [rows, w] for the widths the sparse kernel specialises (1, 3, 4,
12, 27, 48) and a generic one (5) at 257 and 4099 rows.  cmp fails unless every difference is a trailing element's v' or p' with m' equal."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "structured-gaussian-splatting_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import training_ref as R  # noqa: E402


def cases():
    """name -> [(n, row_len, split, step, lr, lr_tail, seed)] of one launch, and the common row count of its tensors (None: dense only)."""
    out = {}
    for c in R.adam_cases():
        out["case n=%d row_len=%d split=%d step=%d" % c[:4]] = ([c], c[0] // c[1] if c[1] else c[0])
    out["eight tensors"] = (R.ADAM_EIGHT, None)
    for rows in (257, 4099):
        for w in (1, 3, 4, 5, 12, 27, 48):
            row_len, split = (w, 3) if w >= 5 else (0, 0)
            out[f"rows={rows} w={w}"] = ([(rows * w, row_len, split, 7, 0.0025, 0.000125, 10 * rows + w)], rows)
    return out


def dump(path):
    from diff_gaussian_rasterization import _native as N
    dev, (b1, b2), eps = "cuda:0", R.ADAM_BETAS, R.ADAM_EPS
    result = {}
    for name, (launch, rows) in cases().items():
        masks = {"dense": None}
        if rows is not None:
            seen = torch.rand(rows, generator=torch.Generator().manual_seed(rows)) < 0.7
            i = torch.arange(rows)
            masks.update(bool=seen, int32=torch.where(seen, 1 + i % 9, -(i % 2) * 7).to(torch.int32))
        for kind, mask in masks.items():
            state = [[t.to(dev) for t in R.adam_state(c[0], c[6])] for c in launch]
            items = [(p, g, m, v, c[4], c[5], c[3], c[1], c[2]) for (p, g, m, v), c in zip(state, launch)]
            if mask is None:
                N.adam_step_multi(items, b1, b2, eps)
            else:
                N.adam_step_sparse_multi(items, mask.to(dev), b1, b2, eps)
            torch.cuda.synchronize()
            for k, (p, g, m, v) in enumerate(state):
                for what, t in (("p", p), ("m", m), ("v", v)):
                    result[f"{name} | {kind} | tensor {k} | {what}"] = t.cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **result)
    print(f"adam_bits: {len(result)} arrays from {N.lib_path()} -> {path}")


def cmp(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different cases"
    total = {"float4": 0, "trailing": 0, "elements": 0}
    bad = []
    for key in a.files:
        x, y = a[key].view(np.int32), b[key].view(np.int32)
        assert x.shape == y.shape, key
        diff = np.nonzero(x != y)[0]
        body = int((diff < x.size // 4 * 4).sum())
        total["float4"] += body
        total["trailing"] += diff.size - body
        total["elements"] += x.size
        if diff.size:
            print(f"{key}: n = {x.size} (n % 4 = {x.size % 4}), {body} differ inside a float4, {diff.size - body} trailing")
        if body or (diff.size and key.endswith("| m")):
            bad.append(key)
    print(f"adam_bits: {total['elements']} elements in {len(a.files)} arrays: {total['float4']} differ inside a float4, {total['trailing']} trailing")
    if bad:
        raise SystemExit(f"adam_bits: differences that are no trailing element's v' or p': {bad}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "cmp":
        cmp(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
