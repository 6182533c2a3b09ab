"""CLIP score throughput on one GPU: ViT-B/32 (diffusion_pruning_amd.clip_model, init_synthetic weights, bf16) at B = 64 pairs of
256 x 256 uint8 images and 77-token captions, each stage replayed from a HIP graph -- the text tower (ids -> unit-norm features),
the image front end (ops.image_patches_pil), the image tower (uint8 images -> unit-norm features, front end included) and the whole
score (both towers and ops.paired_cosine) -- median of --iters replays.  For scale only, the front end's time stands next to
F.interpolate(mode="bicubic", antialias=True) of the same batch on the same GPU (not bit-compatible with PIL, no crop, no unfold).
Prints ONE JSON line.  usage: python tools/bench_clip_score.py [--iters 10] [--batch 64]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from diffusion_pruning_amd import _lib, ops
from diffusion_pruning_amd.clip_model import CLIPModel, CLIPTextModelWithProjection, CLIPTextProjectionConfig
from diffusion_pruning_amd.image_encoder import CLIPVisionConfig, CLIPVisionModelWithProjection
from tools.bench_image_encoder import capture, time_events


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_score: no GPU")
    dev = torch.device("cuda:0")
    _lib.load()
    B, S = a.batch, a.size
    tcfg, vcfg = CLIPTextProjectionConfig(), CLIPVisionConfig.vit_b_32()
    model = CLIPModel(CLIPTextModelWithProjection(tcfg).init_synthetic(0), CLIPVisionModelWithProjection(vcfg).init_synthetic(1)).to(dev)
    tm, vm = model.text_model, model.vision_model
    gen = torch.Generator().manual_seed(2)
    ids = torch.randint(3, tcfg.vocab_size, (B, 77), generator=gen).to(dev)
    img = torch.randint(0, 256, (B, S, S, 3), generator=gen, dtype=torch.uint8).to(dev)
    imgf = img.permute(0, 3, 1, 2).float()

    def text():
        return ops.l2_normalize(tm.embed_ids(ids))

    def front():
        return ops.image_patches_pil(img, vcfg.image_size, vcfg.patch_size)

    def image():
        return ops.l2_normalize(vm.encode_patches(front(), B)[0])

    def score():
        return ops.paired_cosine(vm.encode_patches(front(), B)[0], tm.embed_ids(ids))

    def torch_front():
        return F.interpolate(imgf, size=(vcfg.image_size, vcfg.image_size), mode="bicubic", antialias=True)

    res = {"metric": "clip_score", "box": "1 x AMD Instinct MI355X (gfx950)", "device_name": torch.cuda.get_device_name(0),
           "model": "CLIP ViT-B/32 (text 12 x 512, 8 heads, 77 tokens; vision 12 x 768, 12 heads, 50 tokens), bf16, init_synthetic",
           "batch": B, "image_input": f"{S}x{S} uint8", "tokens": 77, "timing": f"median of {a.iters} graph replays"}
    with torch.no_grad():
        for name, fn, unit in (("text", text, "text_encodes_per_s"), ("front_end", front, "images_per_s"), ("image", image, "images_per_s"),
                               ("score", score, "pairs_per_s")):
            g = capture(fn)
            ms = time_events(g.replay, a.iters)
            res[name] = {"graph_ms": round(ms, 4), unit: round(B / (ms * 1e-3), 1)}
            del g
        tms = time_events(torch_front, a.iters)
        res["torch_interpolate_bicubic_antialias_ms"] = round(tms, 4)
        res["front_end"]["over_torch_interpolate"] = round(res["front_end"]["graph_ms"] / tms, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
