"""Generator of clip_model_tiny.npz: a tiny transformers ``CLIPModel`` run in fp64, the fixture that pins the text tower of
tests/clip_score_oracle.py (and, again, tests/clip_vision_oracle.py) on machines without transformers.

    python tests/golden/make_clip_model_golden.py

Text tower: vocab 256, hidden 128, intermediate 128, 2 heads of 64, 2 layers, 77 positions, hidden_act "quick_gelu", projection
64.  Vision tower: clip_vision_tiny's configuration AND its weights and ``pixel_values``, read from clip_vision_tiny.npz and not
stored again (random fp16 values do not compress; both towers in one file would pass the size limit of a committed file).  Every
text parameter is drawn from a seeded normal distribution and rounded to fp16 so that it is stored exactly (the model runs on
the fp16 values widened to fp64); ``logit_scale`` is ln 100.  Attention runs through "sdpa", which computes in fp64 throughout (the
"eager" path rounds its softmax to fp32: tests/golden/make_clip_vision_golden.py).

Ids, for L in 1, 9, 77 (``ids_L{L}``, int64 [3, L], values below 200 unless said): row 0 has the largest id, 255, once in the middle;
row 1 has 255 twice (the first one counts) and 200 twice; row 2 is plain.  Two poolings are recorded: ``text_embeds_L{L}`` with
``eos_token_id`` 2 (the largest id) and ``text_embeds_eos200_L{L}`` with ``eos_token_id`` 200 (the first 200: present in row 1
only, rows 0 and 2 fall back to position 0).  Embeddings are the projected pooled outputs, NOT normalised.  Also stored:
``last_hidden_state_L1`` and ``_L9`` whole, ``last_hidden_state_L77_last`` (the last position of each row: it attends to all 77
tokens) and ``image_embeds`` of clip_vision_tiny's ``pixel_values`` through this model's vision tower and projection."""
import math
import os

import numpy as np
import torch

TEXT = dict(vocab_size=256, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
            max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, bos_token_id=0, pad_token_id=1, projection_dim=64)
VISION = dict(hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_channels=3, patch_size=14,
              image_size=56, projection_dim=64, layer_norm_eps=1e-5, hidden_act="quick_gelu")
LENGTHS = (1, 9, 77)
EOS_ALT = 200


def _model(eos):
    from transformers import CLIPConfig, CLIPModel
    cfg = CLIPConfig(text_config={**TEXT, "eos_token_id": eos}, vision_config=VISION, projection_dim=64)
    for c in (cfg, cfg.text_config, cfg.vision_config):
        c._attn_implementation = "sdpa"
    return CLIPModel(cfg).double().eval()


def make_ids(L, g):
    ids = torch.randint(3, EOS_ALT, (3, L), generator=g)
    if L >= 9:
        ids[0, L // 2] = 255
        ids[1, L // 3], ids[1, 2 * L // 3] = 255, 255
        ids[1, 2], ids[1, L - 2] = EOS_ALT, EOS_ALT
    return ids


def main():
    g = torch.Generator().manual_seed(9876)
    out, values = {}, {}
    m = _model(2)
    vz = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_vision_tiny.npz"))
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith(("vision_model.", "visual_projection.")):
                values[name] = torch.from_numpy(vz[name])
                continue
            if name == "logit_scale":
                v = torch.tensor(math.log(100.0))
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
        ids = {L: make_ids(L, g) for L in LENGTHS}
        px = torch.from_numpy(vz["pixel_values"])
        for eos, tag in ((2, ""), (EOS_ALT, f"_eos{EOS_ALT}")):
            m = _model(eos)
            for name, p in m.named_parameters():
                p.copy_(values[name].double())
            for L in LENGTHS:
                r = m.text_model(input_ids=ids[L])
                out[f"text_embeds{tag}_L{L}"] = m.text_projection(r.pooler_output).numpy()
                if not tag:
                    out[f"ids_L{L}"] = ids[L].numpy()
                    if L < 77:
                        out[f"last_hidden_state_L{L}"] = r.last_hidden_state.numpy()
                    else:
                        out[f"last_hidden_state_L{L}_last"] = r.last_hidden_state[:, -1].numpy()
            if not tag:
                out["image_embeds"] = m.visual_projection(m.vision_model(pixel_values=px.double()).pooler_output).numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_model_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
