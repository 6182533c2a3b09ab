"""Text features of the CLIP score, on the HIP kernels (the reference's scripts/metrics/clip_features.py,
pdm/utils/clip_utils.py:224-263): every caption through the text tower of a CLIP model, L2-normalised, one ``.npy`` per caption.

    python tools/clip_features.py IDS.npy OUT_DIR --model CLIP_FOLDER [--names NAMES.txt] [--batch_size 64] [--precision bf16]

IDS.npy is an integer [n, L] array of token ids (L <= 77; tokenizing is not part of this package: ``clip.tokenize`` or
transformers' CLIPTokenizer writes such an array).  OUT_DIR receives ``{name}.npy`` (fp32 [projection_dim]) per row; --names is a
text file with one name per row, by default the rows are numbered ``000000``, ``000001``, ... so that the sorted listing keeps their
order.  --model is a transformers CLIPModel folder (config.json + model.safetensors)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def feature_names(n, names_file=None):
    if names_file is None:
        return [f"{i:06d}" for i in range(n)]
    with open(names_file) as f:
        names = [ln.strip() for ln in f if ln.strip()]
    if len(names) != n or len(set(names)) != n:
        raise SystemExit(f"clip_features: {names_file} must hold {n} distinct names, one per caption")
    return [os.path.splitext(nm)[0] for nm in names]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("ids")
    ap.add_argument("out_dir")
    ap.add_argument("--model", required=True, help="transformers CLIPModel folder (config.json and model.safetensors)")
    ap.add_argument("--names", default=None)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--precision", default="bf16", choices=("bf16", "fp32"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("clip_features: no GPU (the HIP kernels are the only compute path)")
    ids = np.load(a.ids)
    if ids.ndim != 2 or not np.issubdtype(ids.dtype, np.integer):
        raise SystemExit(f"clip_features: {a.ids} must be an integer [n, L] array, got {ids.dtype} {ids.shape}")
    names = feature_names(ids.shape[0], a.names)
    from diffusion_pruning_amd import metrics
    from diffusion_pruning_amd.clip_model import CLIPModel
    sm = metrics.ClipScoreModel(CLIPModel.from_pretrained(a.model).to("cuda:0"), precision=a.precision)
    feats = sm.text_features(ids.astype(np.int64), a.batch_size).cpu().numpy()
    os.makedirs(a.out_dir, exist_ok=True)
    for nm, row in zip(names, feats):
        np.save(os.path.join(a.out_dir, nm + ".npy"), row)
    print(f"CLIP features of {len(names)} captions saved to {a.out_dir}")


if __name__ == "__main__":
    main()
