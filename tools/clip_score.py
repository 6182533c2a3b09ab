"""CLIP score of a folder of generated images against a folder of text features, on the HIP kernels (the reference's
scripts/metrics/clip_score.py, pdm/utils/clip_utils.py:197-221).

    python tools/clip_score.py IMAGES_DIR TEXT_FEATURES_DIR --model CLIP_FOLDER [--batch_size 64] [--precision bf16]

IMAGES_DIR holds one uint8 [H, W, 3] ``.npy`` per generated image (what generate_fid_images.py saves), TEXT_FEATURES_DIR one
``.npy`` feature row per caption (what tools/clip_features.py, or the reference's clip_features, writes).  As in the reference, the
two folders are listed without dot files, sorted by name and paired by position; unlike the reference, folders of different
lengths are refused rather than read past the shorter one.  --model is a transformers CLIPModel folder (config.json +
model.safetensors) of openai/clip-vit-base-patch32.  Images of one size are batched together; each is preprocessed exactly as
OpenAI CLIP's ``preprocess`` would (ops.image_patches_pil)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def list_folder(path):
    """the reference's ``_combine_without_prefix``: every entry that does not start with a dot, sorted"""
    return sorted(os.path.join(path, n) for n in os.listdir(path) if not n.startswith("."))


def pair_folders(images_dir, text_dir):
    """[(image file, feature file)] paired by position in the two sorted listings"""
    imgs, txts = list_folder(images_dir), list_folder(text_dir)
    if not imgs:
        raise SystemExit(f"clip_score: no files in {images_dir}")
    if len(imgs) != len(txts):
        raise SystemExit(f"clip_score: {len(imgs)} images in {images_dir} but {len(txts)} text features in {text_dir}")
    return list(zip(imgs, txts))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("images_dir")
    ap.add_argument("text_features_dir")
    ap.add_argument("--model", required=True, help="transformers CLIPModel folder (config.json and model.safetensors)")
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--precision", default="bf16", choices=("bf16", "fp32"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("clip_score: no GPU (the HIP kernels are the only compute path)")
    from diffusion_pruning_amd import metrics, ops
    from diffusion_pruning_amd.clip_model import CLIPModel
    sm = metrics.ClipScoreModel(CLIPModel.from_pretrained(a.model).to("cuda:0"), precision=a.precision)
    pairs = pair_folders(a.images_dir, a.text_features_dir)
    total = torch.zeros((), dtype=torch.float64, device="cuda:0")
    for i in range(0, len(pairs), a.batch_size):
        chunk = pairs[i:i + a.batch_size]
        imgs = [np.load(f) for f, _ in chunk]
        txt = torch.from_numpy(np.stack([np.load(f).astype(np.float32).reshape(-1) for _, f in chunk])).to("cuda:0")
        by_shape = {}
        for j, im in enumerate(imgs):
            by_shape.setdefault(im.shape, []).append(j)
        for idx in by_shape.values():                     # (the sum over pairs does not depend on how they are grouped)
            feats = sm.image_features(np.stack([imgs[j] for j in idx]), a.batch_size)
            ops.paired_cosine(feats, txt[idx].contiguous(), total=total)
    score = sm.logit_scale * float(total) / len(pairs)
    print(f"CLIP Score: {score:.4f}")


if __name__ == "__main__":
    main()
