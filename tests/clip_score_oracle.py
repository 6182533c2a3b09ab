"""CPU oracle of the CLIP score's device path -- TEST INFRASTRUCTURE ONLY.

Three from-scratch restatements, none of which calls the package under test:

  * ``pil_resize`` / ``clip_preprocess_u8``: PIL's 8-bit bicubic resampler (Resample.c: ``precompute_coeffs``,
    ``normalize_coeffs_8bpc``, ``ImagingResampleHorizontal_8bpc`` / ``Vertical_8bpc``) in numpy integers, and torchvision's
    ``Resize(size)`` + ``CenterCrop(size)`` around it.  ``tests/golden/clip_preprocess_tiny.npz`` pins it against the PIL that
    generated the fixture on every pixel, so machines without PIL still check it.
  * ``clip_text_embeds``: transformers' ``CLIPTextModelWithProjection`` forward in plain torch (fp64 by default): embeddings,
    pre-LayerNorm layers under the causal mask with QuickGELU or exact GELU, ``final_layer_norm``, the pooled row (the first
    largest id when ``eos_token_id == 2``, else the first ``eos_token_id`` or row 0), ``text_projection``.
    ``tests/golden/clip_model_tiny.npz`` pins it against the installed transformers.
  * ``clip_score``: pdm/utils/clip_utils.py:141-170 in fp64 -- preprocess, both towers, unit vectors, ``logit_scale * mean cos``.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from tests import clip_vision_oracle as V

CLIP_MEAN, CLIP_STD = V.CLIP_MEAN, V.CLIP_STD
PRECISION_BITS = 32 - 8 - 2


# ---------------------------------------------------------------------------------------------------------------------
# PIL's bicubic resampler for 8-bit images
# ---------------------------------------------------------------------------------------------------------------------
def _bicubic(x: np.ndarray) -> np.ndarray:
    """Keys' kernel with a = -0.5 on |x| (PIL's bicubic_filter)"""
    a = -0.5
    x = np.abs(x)
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    outer = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


def coeff_table(in_size: int, out_size: int):
    """(bounds int32 [out, 2] = (xmin, count), weights int32 [out, ksize]): double-precision weights over the window
    [xmin, xmax) = [max(int(c - s + 0.5), 0), min(int(c + s + 0.5), in)), c = (i + 0.5) scale, s = 2 max(scale, 1), normalised to
    sum 1 and rounded to PRECISION_BITS fractional bits, away from zero by one half"""
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    weights = np.zeros((out_size, ksize), np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = _bicubic((np.arange(xmin, xmax).astype(np.float64) - center + 0.5) * (1.0 / fscale))
        ww = 0.0
        for v in w:                                  # the C loop's summation order
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        fixed = w * float(1 << PRECISION_BITS)
        weights[i, :xmax - xmin] = np.where(w < 0, np.trunc(fixed - 0.5), np.trunc(fixed + 0.5)).astype(np.int32)
        bounds[i] = (xmin, xmax - xmin)
    return bounds, weights


def _resample_axis0(img: np.ndarray, out_size: int) -> np.ndarray:
    """one pass along axis 0 of a uint8 array: int32 accumulators starting at one half, arithmetic shift, clamp, uint8"""
    bounds, weights = coeff_table(img.shape[0], out_size)
    src = img.astype(np.int64)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    tail = (1,) * (img.ndim - 1)
    for i, (x0, n) in enumerate(bounds):
        acc = (src[x0:x0 + n] * weights[i, :n].astype(np.int64).reshape((n,) + tail)).sum(0) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31                # PIL accumulates in int32: nothing here may need more
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def pil_resize(img: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """``PIL.Image.fromarray(img).resize((out_w, out_h), BICUBIC)`` of a uint8 [H, W, C] array: the horizontal pass, then the
    vertical one, each skipped when its size does not change"""
    assert img.dtype == np.uint8 and img.ndim == 3
    if out_w != img.shape[1]:
        img = np.swapaxes(_resample_axis0(np.swapaxes(img, 0, 1), out_w), 0, 1)
    if out_h != img.shape[0]:
        img = _resample_axis0(img, out_h)
    return np.ascontiguousarray(img)


def resized_size(h: int, w: int, size: int):
    """torchvision's Resize(size) on an (h, w) image: the shorter side to size, the longer to int(size * long / short)"""
    return (size, int(size * w / h)) if h <= w else (int(size * h / w), size)


def crop_offset(extent: int, size: int) -> int:
    """torchvision's CenterCrop: int(round((extent - size) / 2.0)), Python's round (halves to even)"""
    return int(round((extent - size) / 2.0))


def clip_preprocess_u8(img: np.ndarray, size: int) -> np.ndarray:
    """uint8 [H, W, 3] -> uint8 [size, size, 3]: Resize(size, BICUBIC) and CenterCrop(size) of OpenAI CLIP's preprocess"""
    h1, w1 = resized_size(img.shape[0], img.shape[1], size)
    r = pil_resize(img, h1, w1)
    top, left = crop_offset(h1, size), crop_offset(w1, size)
    return np.ascontiguousarray(r[top:top + size, left:left + size])


def pixel_values(images_u8: np.ndarray, size: int, dtype=torch.float32) -> torch.Tensor:
    """uint8 [B, H, W, 3] -> [B, 3, size, size]: preprocess, ToTensor (/ 255) and Normalize, in ``dtype`` (torchvision: fp32)"""
    u8 = np.stack([clip_preprocess_u8(im, size) for im in images_u8])
    x = torch.from_numpy(u8).permute(0, 3, 1, 2).to(dtype) / 255
    mean, std = (torch.tensor(v, dtype=torch.float32).to(dtype).view(1, 3, 1, 1) for v in (CLIP_MEAN, CLIP_STD))
    return (x - mean) / std


# ---------------------------------------------------------------------------------------------------------------------
# the text tower
# ---------------------------------------------------------------------------------------------------------------------
def pool_index(ids: torch.Tensor, eos_token_id: int = 2) -> torch.Tensor:
    """first index of the largest id when eos_token_id == 2, else the first index equal to eos_token_id (0 without one)"""
    ids = ids.cpu().long()
    out = []
    for row in ids.tolist():
        if eos_token_id == 2:
            out.append(row.index(max(row)))
        else:
            out.append(row.index(eos_token_id) if eos_token_id in row else 0)
    return torch.tensor(out, dtype=torch.long)


def text_stream(params: Dict[str, torch.Tensor], input_ids: torch.Tensor, heads: int, layers: int, hidden_act: str = "quick_gelu",
                eps: float = 1e-5, dtype=torch.float64) -> torch.Tensor:
    """the residual stream after the last layer, BEFORE final_layer_norm, [B, L, hidden] in ``dtype``"""
    p = {k: v.detach().to("cpu", dtype) for k, v in params.items() if v.is_floating_point()}
    ids = input_ids.cpu().long()
    B, L = ids.shape
    x = p["text_model.embeddings.token_embedding.weight"][ids] + p["text_model.embeddings.position_embedding.weight"][:L]
    mask = torch.triu(torch.ones(L, L, dtype=torch.bool), diagonal=1)
    for i in range(layers):
        pre = f"text_model.encoder.layers.{i}."
        C = x.shape[-1]
        d = C // heads
        n = V._ln(x, p, pre + "layer_norm1", eps)
        q, k, v = (V._lin(n, p, pre + f"self_attn.{t}_proj").reshape(B, L, heads, d).transpose(1, 2) for t in "qkv")
        s = ((q @ k.transpose(-1, -2)) * d ** -0.5).masked_fill(mask, float("-inf"))
        o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, L, C)
        x = x + V._lin(o, p, pre + "self_attn.out_proj")
        n = V._ln(x, p, pre + "layer_norm2", eps)
        x = x + V._lin(V._act(V._lin(n, p, pre + "mlp.fc1"), hidden_act), p, pre + "mlp.fc2")
    return x


def clip_text_embeds(params: Dict[str, torch.Tensor], input_ids: torch.Tensor, heads: int, layers: int,
                     hidden_act: str = "quick_gelu", eos_token_id: int = 2, eps: float = 1e-5, dtype=torch.float64):
    """(text_embeds [B, proj], last_hidden_state [B, L, hidden]) in ``dtype``, text_embeds not normalised"""
    x = text_stream(params, input_ids, heads, layers, hidden_act, eps, dtype)
    p = {k: params[k].detach().to("cpu", dtype) for k in ("text_model.final_layer_norm.weight", "text_model.final_layer_norm.bias",
                                                           "text_projection.weight")}
    h = V._ln(x, p, "text_model.final_layer_norm", eps)
    pooled = h[torch.arange(h.shape[0]), pool_index(input_ids, eos_token_id)]
    return pooled @ p["text_projection.weight"].t(), h


def pooled_ln(x: torch.Tensor, ids: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, eos_token_id: int = 2):
    """fp64 LayerNorm of the pooled row of each sample of a stream x [B, L, C]: (rows [B, C], indices [B])"""
    at = pool_index(ids, eos_token_id)
    rows = x.detach().cpu().double()[torch.arange(x.shape[0]), at]
    return F.layer_norm(rows, (rows.shape[-1],), gamma.detach().cpu().double(), beta.detach().cpu().double(), eps), at


# ---------------------------------------------------------------------------------------------------------------------
# the score
# ---------------------------------------------------------------------------------------------------------------------
def cosines(a, b) -> torch.Tensor:
    a, b = (torch.as_tensor(t).detach().to("cpu", torch.float64) for t in (a, b))
    return ((a / a.norm(dim=1, keepdim=True)) * (b / b.norm(dim=1, keepdim=True))).sum(1)


def clip_score(params: Dict[str, torch.Tensor], images_u8: np.ndarray, input_ids: torch.Tensor, *, text: dict, vision: dict,
               logit_scale: float, text_features: Optional[torch.Tensor] = None):
    """(score, cosines [n]) in fp64: calculate_clip_score over one batch.  text: heads, layers, hidden_act, eos_token_id;
    vision: heads, layers, patch, image_size, hidden_act"""
    if text_features is None:
        text_features, _ = clip_text_embeds(params, input_ids, text["heads"], text["layers"], text["hidden_act"], text["eos_token_id"])
    px = pixel_values(images_u8, vision["image_size"], torch.float64)
    vp = {k: v for k, v in params.items() if k.startswith(("vision_model.", "visual_projection."))}
    emb, _ = V.clip_vision_forward(vp, px, heads=vision["heads"], layers=vision["layers"], patch=vision["patch"],
                                   hidden_act=vision["hidden_act"])
    cos = cosines(emb, text_features)
    return float(logit_scale * cos.sum() / cos.shape[0]), cos
