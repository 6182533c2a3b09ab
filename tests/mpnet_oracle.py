"""Plain torch restatement of transformers ``MPNetModel`` (no pooler) and of the reference's masked mean
(pdm/utils/data_utils.py:130-155), in fp32 or fp64, on the CPU:

  pos_id = cumsum(ids != pad) * (ids != pad) + pad                                        (create_position_ids_from_input_ids)
  x      = LayerNorm(word[ids] + position[pos_id])                                        (MPNetEmbeddings)
  bias[h, i, j] = relative_attention_bias[bucket(j - i), h]                               (MPNetEncoder.compute_position_bias)
  per layer:  s = q k^T / sqrt(64) + bias + (1 - mask[b, j]) * finfo.min ; a = softmax(s) v
              x = LayerNorm(o(a) + x) ; x = LayerNorm(dense_out(gelu_erf(dense_in(x))) + x)  (post-LayerNorm, BERT order)
  pooled = sum(x * mask) / clamp(sum(mask), 1e-9)                                         (NOT L2-normalised)
"""
import math

import torch
import torch.nn.functional as F


def relative_position_bucket(relative_position: torch.Tensor, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """MPNetEncoder.relative_position_bucket: half the buckets per sign, distances below num_buckets / 4 exact, then
    log-spaced (the fp32 log of transformers), saturating from max_distance on"""
    n = -relative_position
    num_buckets //= 2
    ret = (n < 0).to(torch.long) * num_buckets
    n = torch.abs(n)
    max_exact = num_buckets // 2
    is_small = n < max_exact
    val_if_large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact)
                                * (num_buckets - max_exact)).to(torch.long)
    val_if_large = torch.min(val_if_large, torch.full_like(val_if_large, num_buckets - 1))
    return ret + torch.where(is_small, n, val_if_large)


def position_ids(ids: torch.Tensor, pad: int = 1) -> torch.Tensor:
    m = ids.ne(pad).int()
    return (torch.cumsum(m, dim=1).type_as(m) * m).long() + pad


def position_bias(weight: torch.Tensor, L: int) -> torch.Tensor:
    """[heads, L, L] from relative_attention_bias.weight [buckets, heads]"""
    ar = torch.arange(L, dtype=torch.long)
    bucket = relative_position_bucket(ar[None, :] - ar[:, None], num_buckets=weight.shape[0])
    return weight[bucket].permute(2, 0, 1)


def mpnet_forward(p, ids, mask=None, heads=12, layers=12, eps=1e-5, pad=1, dtype=torch.float32):
    """(last_hidden_state [B, L, H], pooled [B, H]) from a transformers-named state dict ``p``"""
    p = {k: v.to(dtype) for k, v in p.items()}
    B, L = ids.shape
    mask = torch.ones(B, L, dtype=dtype) if mask is None else mask.to(dtype)
    H = p["embeddings.word_embeddings.weight"].shape[1]
    x = p["embeddings.word_embeddings.weight"][ids] + p["embeddings.position_embeddings.weight"][position_ids(ids, pad)]
    x = F.layer_norm(x, (H,), p["embeddings.LayerNorm.weight"], p["embeddings.LayerNorm.bias"], eps)
    bias = position_bias(p["encoder.relative_attention_bias.weight"], L)[None]
    ext = (1.0 - mask)[:, None, None, :] * torch.finfo(dtype).min
    d = H // heads
    for i in range(layers):
        pre = f"encoder.layer.{i}."
        lin = lambda t, n: F.linear(t, p[pre + n + ".weight"], p[pre + n + ".bias"])      # noqa: E731
        sh = lambda t: t.view(B, L, heads, d).transpose(1, 2)                               # noqa: E731
        q, k, v = sh(lin(x, "attention.attn.q")), sh(lin(x, "attention.attn.k")), sh(lin(x, "attention.attn.v"))
        s = q @ k.transpose(-1, -2) / math.sqrt(d) + bias + ext
        c = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, L, H)
        x = F.layer_norm(lin(c, "attention.attn.o") + x, (H,), p[pre + "attention.LayerNorm.weight"],
                         p[pre + "attention.LayerNorm.bias"], eps)
        f = lin(F.gelu(lin(x, "intermediate.dense")), "output.dense")
        x = F.layer_norm(f + x, (H,), p[pre + "output.LayerNorm.weight"], p[pre + "output.LayerNorm.bias"], eps)
    pooled = (x * mask[..., None]).sum(1) / mask.sum(1, keepdim=True).clamp(min=1e-9)
    return x, pooled
