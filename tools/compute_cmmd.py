"""CMMD between two folders of images on the HIP kernels: the reference CLI's arguments (cmmd-pytorch/compute_cmmd.py).

    python tools/compute_cmmd.py REF_DIR EVAL_DIR --model CLIP_FOLDER [--ref_embed_file F.npy] [--batch_size 32] [--max_count -1]

REF_DIR / EVAL_DIR hold png / jpg / jpeg files (read with PIL, center-cropped to a square and resized to the encoder's input size
with PIL's bicubic filter, as the reference's CMMDDataset does).  --ref_embed_file replaces REF_DIR by precomputed reference
embeddings (pass "" or "-" for REF_DIR then).  --model is a transformers folder of openai/clip-vit-large-patch14-336
(config.json + model.safetensors; a full CLIPModel file is fine).  Unlike the reference, a last incomplete batch is embedded too."""
import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def list_images(path, max_count=-1):
    files = []
    for ext in ("png", "jpg", "jpeg"):
        files += glob.glob(os.path.join(path, f"*.{ext}")) + glob.glob(os.path.join(path, f"*.{ext.upper()}"))
    files = sorted(set(files))
    return files[:max_count] if max_count > 0 else files


def read_image(path, size):
    """[size, size, 3] fp32 in [0, 1]"""
    from PIL import Image
    im = Image.open(path).convert("RGB")
    w, h = im.size
    s = min(w, h)
    left, top = (w - s) // 2, (h - s) // 2
    im = im.crop((left, top, left + s, top + s)).resize((size, size), resample=Image.BICUBIC)
    return np.asarray(im).astype(np.float32) / 255.0


def embed_dir(path, em, batch_size, max_count=-1):
    files = list_images(path, max_count)
    if not files:
        raise SystemExit(f"compute_cmmd: no png / jpg / jpeg images in {path}")
    print(f"Calculating embeddings for {len(files)} images from {path}.")
    out = []
    for i in range(0, len(files), batch_size):
        batch = np.stack([read_image(f, em.input_image_size) for f in files[i:i + batch_size]])
        out.append(em.embed(batch, batch_size))
    return torch.cat(out, 0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("ref_dir")
    ap.add_argument("eval_dir")
    ap.add_argument("--model", required=True, help="folder with config.json and model.safetensors of the CLIP checkpoint")
    ap.add_argument("--ref_embed_file", default=None)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--max_count", type=int, default=-1)
    ap.add_argument("--precision", default="bf16", choices=("bf16", "fp32"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compute_cmmd: no GPU (the HIP kernels are the only compute path)")
    if a.ref_embed_file and a.ref_dir not in ("", "-"):
        raise SystemExit("compute_cmmd: give REF_DIR or --ref_embed_file, not both (pass - for REF_DIR with --ref_embed_file)")
    from diffusion_pruning_amd import metrics
    from diffusion_pruning_amd.image_encoder import CLIPVisionModelWithProjection
    model = CLIPVisionModelWithProjection.from_pretrained(a.model).to("cuda:0")
    em = metrics.ClipEmbeddingModel(model, precision=a.precision)
    if a.ref_embed_file:
        ref = torch.from_numpy(np.load(a.ref_embed_file).astype(np.float32)).to("cuda:0")
    else:
        ref = embed_dir(a.ref_dir, em, a.batch_size, a.max_count)
    ev = embed_dir(a.eval_dir, em, a.batch_size, a.max_count)
    print(f"The CMMD value is:  {float(metrics.mmd(ref, ev)):.3f}")


if __name__ == "__main__":
    main()
