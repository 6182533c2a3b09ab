"""Generator of mpnet_tiny.npz: a tiny MPNet encoder run by the installed transformers.MPNetModel (fp64, no pooler), the
fixture that pins tests/mpnet_oracle.py and the host bias table on machines without transformers.

    python tests/golden/make_mpnet_golden.py

Configuration: vocab 96, hidden 128, intermediate 128, 2 heads of 64, 2 layers, 204 positions (L up to 200 + pad + 1),
hidden_act "gelu", 32 relative-position buckets, pad id 1.  Every parameter is drawn from a seeded normal distribution and
rounded to fp16 so that it is stored exactly (the model runs on the fp16 values widened to fp64); the relative-position
table has std 1.  Batches (ids with pad tokens where the mask is 0, as the tokenizer pads):
  a  [4, 24]   prefix masks of lengths 24 / 10 / 1 / 17
  b  [2, 200]  prefix masks of lengths 200 / 37: relative distances past 128, the saturated buckets
  c  [2, 16]   a NON-prefix mask: sample 0 masks tokens 3..5 and 9 (their ids stay real tokens), sample 1 an interior pad
               TOKEN at 4 that the mask also drops (position ids skip it)
Stored: the parameters (transformers names), ``ids_{n}``, ``mask_{n}``, ``last_hidden_state_{n}`` and ``pooled_{n}`` (the
reference's masked mean) as fp32, and ``bucket_L{L}`` = MPNetEncoder.relative_position_bucket(j - i) for j - i =
-(L-1) .. L-1 at L = 1, 7, 128, 129, 512."""
import os

import numpy as np
import torch

CFG = dict(vocab_size=96, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
           max_position_embeddings=204, hidden_act="gelu", layer_norm_eps=1e-5, relative_attention_num_buckets=32,
           pad_token_id=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
BUCKET_LENGTHS = (1, 7, 128, 129, 512)


def batches(g):
    out = {}
    for name, B, L, lengths in (("a", 4, 24, (24, 10, 1, 17)), ("b", 2, 200, (200, 37))):
        ids = torch.randint(3, CFG["vocab_size"], (B, L), generator=g)
        mask = torch.zeros(B, L, dtype=torch.long)
        for i, n in enumerate(lengths):
            mask[i, :n] = 1
            ids[i, n:] = 1
        out[name] = (ids, mask)
    ids = torch.randint(3, CFG["vocab_size"], (2, 16), generator=g)
    mask = torch.ones(2, 16, dtype=torch.long)
    mask[0, 3:6] = 0
    mask[0, 9] = 0
    ids[1, 4] = 1
    mask[1, 4] = 0
    ids[1, 13:] = 1
    mask[1, 13:] = 0
    out["c"] = (ids, mask)
    return out


def main():
    from transformers import MPNetConfig, MPNetModel
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder
    m = MPNetModel(MPNetConfig(**CFG), add_pooling_layer=False).double().eval()
    g = torch.Generator().manual_seed(4321)
    out = {}
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "relative_attention_bias" in name:
                v = torch.randn(p.shape, generator=g)
            elif name.endswith("bias"):
                v = 0.05 * torch.randn(p.shape, generator=g)
            elif p.dim() == 1:
                v = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
            elif "embeddings" in name:
                v = 0.5 * torch.randn(p.shape, generator=g)
            else:
                v = p.shape[1] ** -0.5 * torch.randn(p.shape, generator=g)
            v16 = v.to(torch.float16)
            p.copy_(v16.double())
            out[name] = v16.numpy()
        for n, (ids, mask) in batches(g).items():
            h = m(input_ids=ids, attention_mask=mask)[0]
            me = mask.unsqueeze(-1).expand(h.size()).double()
            pooled = torch.sum(h * me, 1) / torch.clamp(me.sum(1), min=1e-9)
            out[f"ids_{n}"], out[f"mask_{n}"] = ids.numpy(), mask.numpy().astype(np.int8)
            out[f"last_hidden_state_{n}"] = h.float().numpy()
            out[f"pooled_{n}"] = pooled.float().numpy()
    for L in BUCKET_LENGTHS:
        rel = torch.arange(-(L - 1), L, dtype=torch.long)
        out[f"bucket_L{L}"] = MPNetEncoder.relative_position_bucket(rel, num_buckets=32).numpy().astype(np.int8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mpnet_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
