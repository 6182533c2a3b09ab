"""Generator of cmmd_tiny.npz by RUNNING the reference's own CMMD functions, loaded by file path as make_golden.py does
(nothing of them is copied into this repository; the .npz holds inputs and recorded outputs only):

    python tests/golden/make_cmmd_golden.py        (where the reference tree is; not on the GPU machine)

  * cmmd-pytorch/distance.py ``mmd`` on the seeded unit-norm embeddings of tests/clip_vision_oracle.py (``cmmd_embeddings``) for
    every (n, m, D) of ``MMD_CASES`` and every shift of ``MMD_SHIFTS``: once on the fp32 arrays, which is the reference as it
    is used (``mmd_f32``), and once on the same values widened to fp64 (``mmd_f64``).  The embeddings themselves are not
    stored (the largest pair is 12 MB): the tests draw them again from numpy's frozen RandomState stream, and ``mmd_xsum`` /
    ``mmd_ysum`` (fp64 sums of the draws) tell a changed draw from a changed result.  The smallest case is stored whole.
  * cmmd-pytorch/embedding.py ``_resize_bicubic`` on small seeded images: up, down, identity and a non-square source.
    ``ClipEmbeddingModel`` is never constructed (its constructor fetches weights)."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = "/root/reference"

RESIZES = {"up": ((2, 24, 24, 3), 56), "down": ((2, 80, 80, 3), 56), "identity": ((1, 56, 56, 3), 56), "nonsquare": ((2, 30, 50, 3), 28)}


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    from tests.clip_vision_oracle import MMD_CASES, MMD_SHIFTS, cmmd_embeddings
    distance = _load("ref_cmmd_distance", "cmmd-pytorch/distance.py")
    embedding = _load("ref_cmmd_embedding", "cmmd-pytorch/embedding.py")
    out = {}
    rows = []
    for n, m, D in MMD_CASES:
        for shift in MMD_SHIFTS:
            x, y = cmmd_embeddings(n, m, D, shift)
            f32 = float(distance.mmd(x, y))
            f64 = float(distance.mmd(x.astype(np.float64), y.astype(np.float64)))
            rows.append((n, m, D, shift, f32, f64, x.astype(np.float64).sum(), y.astype(np.float64).sum()))
            print(n, m, D, shift, f32, f64)
    a = np.array(rows, dtype=np.float64)
    out["mmd_cases"], out["mmd_f32"], out["mmd_f64"], out["mmd_xsum"], out["mmd_ysum"] = a[:, :4], a[:, 4], a[:, 5], a[:, 6], a[:, 7]
    out["small_x"], out["small_y"] = cmmd_embeddings(*MMD_CASES[-1], MMD_SHIFTS[0])
    rs = np.random.RandomState(99)
    for name, (shape, size) in RESIZES.items():
        img = rs.uniform(0.0, 1.0, shape).astype(np.float32)
        out[f"resize_{name}_in"] = img
        out[f"resize_{name}_size"] = np.int64(size)
        out[f"resize_{name}_out"] = embedding._resize_bicubic(img, size)
    path = os.path.join(HERE, "cmmd_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
