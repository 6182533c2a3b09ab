"""Generator of clip_vision_tiny.npz: a tiny CLIP image encoder run by the installed transformers.CLIPVisionModelWithProjection
(fp64), the fixture that pins tests/clip_vision_oracle.py on machines without transformers.

    python tests/golden/make_clip_vision_golden.py

Configuration: hidden 128, intermediate 128, 2 heads of 64, 2 layers, patch 14, image 56 (17 tokens), projection 64,
hidden_act "quick_gelu"; a second forward of the same weights runs with hidden_act "gelu".  Every parameter is drawn from a
seeded normal distribution and rounded to fp16 so that it is stored exactly (the model runs on the fp16 values widened to fp64).
Stored: the parameters (transformers names), ``pixel_values`` (fp32, two images), and per activation ``last_hidden_state_{act}``
and ``image_embeds_{act}`` (fp64).

Attention runs through transformers' "sdpa" implementation: the "eager" one of current transformers rounds the softmax to fp32
whatever the model's dtype (``softmax(..., dtype=torch.float32)``), which would leave 3e-8 of fp32 rounding in an fp64 fixture;
F.scaled_dot_product_attention on fp64 CPU tensors computes in fp64 throughout."""
import os

import numpy as np
import torch

CFG = dict(hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_channels=3, patch_size=14,
           image_size=56, projection_dim=64, layer_norm_eps=1e-5)
ACTS = ("quick_gelu", "gelu")


def _model(act):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    cfg = CLIPVisionConfig(**CFG, hidden_act=act)
    cfg._attn_implementation = "sdpa"
    return CLIPVisionModelWithProjection(cfg).double().eval()


def main():
    g = torch.Generator().manual_seed(4321)
    out, values = {}, {}
    m = _model(ACTS[0])
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "patch_embedding" in name:
                v = p[0].numel() ** -0.5 * torch.randn(p.shape, generator=g)
            elif "embedding" in name:
                v = 0.5 * torch.randn(p.shape, generator=g)
            elif name.endswith("bias"):
                v = 0.05 * torch.randn(p.shape, generator=g)
            elif p.dim() == 1:
                v = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
            else:
                v = p.shape[1] ** -0.5 * torch.randn(p.shape, generator=g)
            values[name] = v.to(torch.float16)
            out[name] = values[name].numpy()
        px = torch.randn(2, 3, CFG["image_size"], CFG["image_size"], generator=g).float()
        out["pixel_values"] = px.numpy()
        for act in ACTS:
            m = _model(act)
            for name, p in m.named_parameters():
                p.copy_(values[name].double())
            r = m(pixel_values=px.double())
            out[f"last_hidden_state_{act}"] = r.last_hidden_state.numpy()
            out[f"image_embeds_{act}"] = r.image_embeds.numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_vision_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
