"""CPU oracle of the CLIP image encoder, CMMD and the CLIP score -- TEST INFRASTRUCTURE ONLY.

A from-scratch restatement in plain torch (run in fp32 or fp64) of

  * transformers' ``CLIPVisionModelWithProjection`` forward:
      x      = [class_embedding | conv(pixel_values, patch_embedding, stride = patch)] + position_embedding   (CLIPVisionEmbeddings)
      x      = pre_layrnorm(x)
      layer  = x + out_proj(SDPA(q_proj(n1), k_proj(n1), v_proj(n1))),  n1 = layer_norm1(x)                     (CLIPEncoderLayer)
               x + fc2(act(fc1(layer_norm2(x)))),  act = v * sigmoid(1.702 v) ("quick_gelu") or the erf GELU ("gelu")
      SDPA   = per head of 64: softmax(q k^T / 8) v, no mask
      out    = last_hidden_state = x;  image_embeds = visual_projection(post_layernorm(x[:, 0]))
  * CMMD's preprocessing (cmmd-pytorch/embedding.py): F.interpolate(mode="bicubic") to the input size, then (v - mean) / std
    with OpenAI CLIP's constants, and the unfold into patch rows the HIP front end emits;
  * CMMD's statistic (cmmd-pytorch/distance.py): scale * (mean k_xx + mean k_yy - 2 mean k_xy) with the Gaussian kernel of
    bandwidth sigma, on squared distances formed from the Gram matrix and its diagonal as there;
  * the CLIP score of pdm/utils/clip_utils.py:159-170.

``tests/golden/clip_vision_tiny.npz`` pins the encoder against the installed transformers at a tiny configuration and
``tests/golden/cmmd_tiny.npz`` pins the resize and the statistic against the reference's own functions, so that machines with
neither still check this file.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _ln(x, p, name, eps):
    return F.layer_norm(x, (x.shape[-1],), p[name + ".weight"], p[name + ".bias"], eps)


def _lin(x, p, name):
    return x @ p[name + ".weight"].t() + p[name + ".bias"]


def _act(x, hidden_act):
    if hidden_act == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    assert hidden_act == "gelu", hidden_act
    return F.gelu(x)


def encoder_layer(x, p: Dict[str, torch.Tensor], i: int, heads: int, eps: float, hidden_act: str):
    pre = f"vision_model.encoder.layers.{i}."
    B, L, C = x.shape
    d = C // heads
    n = _ln(x, p, pre + "layer_norm1", eps)
    q, k, v = (_lin(n, p, pre + f"self_attn.{t}_proj").reshape(B, L, heads, d).transpose(1, 2) for t in "qkv")
    s = (q @ k.transpose(-1, -2)) * d ** -0.5
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, L, C)
    x = x + _lin(o, p, pre + "self_attn.out_proj")
    n = _ln(x, p, pre + "layer_norm2", eps)
    return x + _lin(_act(_lin(n, p, pre + "mlp.fc1"), hidden_act), p, pre + "mlp.fc2")


def clip_vision_forward(params: Dict[str, torch.Tensor], pixel_values: torch.Tensor, heads: int, layers: int, patch: int,
                        hidden_act: str = "quick_gelu", eps: float = 1e-5, dtype=torch.float64, streams: Optional[List] = None):
    """(image_embeds, last_hidden_state) in ``dtype``; ``streams`` (a list) receives the residual stream before layer 0 and
    after every layer"""
    p = {k: v.detach().to("cpu", dtype) for k, v in params.items() if not k.endswith("position_ids")}
    px = pixel_values.detach().to("cpu", dtype)
    B = px.shape[0]
    e = "vision_model.embeddings."
    pe = F.conv2d(px, p[e + "patch_embedding.weight"], stride=patch).flatten(2).transpose(1, 2)
    x = torch.cat([p[e + "class_embedding"].expand(B, 1, -1), pe], 1) + p[e + "position_embedding.weight"]
    x = _ln(x, p, "vision_model.pre_layrnorm", eps)
    if streams is not None:
        streams.append(x)
    for i in range(layers):
        x = encoder_layer(x, p, i, heads, eps, hidden_act)
        if streams is not None:
            streams.append(x)
    pooled = _ln(x[:, 0], p, "vision_model.post_layernorm", eps)
    return pooled @ p["visual_projection.weight"].t(), x


def resize_bicubic(images: torch.Tensor, size: int) -> torch.Tensor:
    """[B, H, W, 3] -> [B, size, size, 3] as cmmd-pytorch/embedding.py:26-30 does it"""
    return F.interpolate(images.permute(0, 3, 1, 2), size=(size, size), mode="bicubic").permute(0, 2, 3, 1)


def preprocess(images: torch.Tensor, size: int, dtype=torch.float64) -> torch.Tensor:
    """images [B, H, W, 3] in [0, 1] -> pixel_values [B, 3, size, size]: bicubic resize, then CLIP's mean / std"""
    x = resize_bicubic(images.detach().to("cpu", dtype), size).permute(0, 3, 1, 2)
    mean, std = (torch.tensor(v, dtype=dtype).view(1, 3, 1, 1) for v in (CLIP_MEAN, CLIP_STD))
    return (x - mean) / std


def patch_rows(pixel_values: torch.Tensor, patch: int) -> torch.Tensor:
    """[B, 3, S, S] -> [B * (S / patch)^2, 3 patch^2], rows in (b, gy, gx) order, elements in (c, py, px) order: F.unfold"""
    return F.unfold(pixel_values, kernel_size=patch, stride=patch).transpose(1, 2).reshape(-1, 3 * patch * patch)


def mmd(x, y, sigma: float = 10.0, scale: float = 1000.0) -> float:
    """cmmd-pytorch/distance.py:28-64 in fp64"""
    x, y = (torch.as_tensor(t).detach().to("cpu", torch.float64) for t in (x, y))
    gamma = 1.0 / (2.0 * sigma ** 2)
    xs, ys = (x * x).sum(1), (y * y).sum(1)

    def kmean(a, b, sa, sb):
        return torch.exp(-gamma * (-2.0 * (a @ b.t()) + sa[:, None] + sb[None, :])).mean()
    return float(scale * (kmean(x, x, xs, xs) + kmean(y, y, ys, ys) - 2.0 * kmean(x, y, xs, ys)))


def clip_score(image_embeds, text_features, logit_scale: float = 100.0) -> float:
    """pdm/utils/clip_utils.py:159-170 for one batch, in fp64"""
    a, b = (torch.as_tensor(t).detach().to("cpu", torch.float64) for t in (image_embeds, text_features))
    a, b = a / a.norm(dim=1, keepdim=True), b / b.norm(dim=1, keepdim=True)
    return float(logit_scale * (a * b).sum() / a.shape[0])


# the embedding draws of the MMD tests: unit-norm rows of N(0, I) + 2 base, the second set moved by shift * dir (base and dir
# are unit-variance Gaussian vectors).  numpy's RandomState stream is frozen, so every machine draws the same values.
MMD_CASES = [(512, 512, 768), (2048, 2048, 768), (1000, 3000, 768), (37, 129, 64)]
MMD_SHIFTS = (0.3, 0.05)


def cmmd_embeddings(n: int, m: int, D: int, shift: float, seed: int = 0):
    rs = np.random.RandomState(seed + 7919 * n + 104729 * m + D)
    base, direction = rs.standard_normal(D), rs.standard_normal(D)
    x = rs.standard_normal((n, D)) + 2.0 * base
    y = rs.standard_normal((m, D)) + 2.0 * base + shift * direction
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    return x.astype(np.float32), y.astype(np.float32)
