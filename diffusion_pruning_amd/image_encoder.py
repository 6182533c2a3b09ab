"""CLIP's image encoder (transformers ``CLIPVisionModelWithProjection`` semantics) on the HIP kernels of this package.

The reference scores generated images with CLIP embeddings: CMMD embeds with ``openai/clip-vit-large-patch14-336``
(cmmd-pytorch/embedding.py:22, :38-40, :67-71) and the CLIP score with a ViT-B/32 (scripts/metrics/clip_score.py,
pdm/utils/clip_utils.py:141-170).  This module keeps transformers' parameter names (``vision_model.embeddings.{class_embedding,
patch_embedding.weight, position_embedding.weight}``, ``vision_model.pre_layrnorm`` -- transformers' own spelling --,
``vision_model.encoder.layers.i.{self_attn.{q,k,v,out}_proj, layer_norm1, mlp.fc1, mlp.fc2, layer_norm2}``,
``vision_model.post_layernorm``, ``visual_projection.weight``) and runs every layer on the kernels:

  * front end: ``ops.image_patches`` writes each patch as one GEMM operand row (from ``pixel_values``, or from raw images with
    the bicubic resize and the normalisation of CMMD's preprocessing in the same launch), so the patch convolution is one
    ``ops.linear`` without bias (fp32 output); ``ops.vit_embed_ln`` adds the class row and the position embedding and applies
    ``pre_layrnorm`` in fp32, with one rounding to the residual stream;
  * each pre-LayerNorm layer: LN1 -> one fused q|k|v linear -> ``ops.attention`` (heads of 64, scale 1/8, no mask, 577 or 50
    tokens) -> out_proj with the residual in its epilogue -> LN2 -> fc1 with QuickGELU (``ACT_QUICK_GELU``) or exact-erf GELU in
    its epilogue -> fc2 with the residual in its epilogue;
  * ``post_layernorm`` on the class row only, then ``visual_projection`` (fp32 output): ``image_embeds``.

The layer loop and its packing are the text tower's (``modules.run_clip_layers`` / ``pack_clip_layers``) with ``ops.attention``
and stand-alone ``ops.layernorm`` launches.  The folded form of the text encoder (text_encoder.py, ``FOLD_LN_MAX_ROWS``) paid off
only under ~512 rows; one image is already 577 rows, and the A/B at this encoder's shapes has not been measured, so the form that
was faster at every comparable size is the one that ships.

With ``ops.ACT_DTYPE = torch.float32`` the same code runs the fp32 parity instantiations of every kernel.  Every launch goes to
torch's current stream and ``forward`` makes no host sync, so an encode can be captured with ``torch.cuda.graph`` after one eager
warm-up call of the same shape.
"""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from .loading import load_strict, read_pretrained
from .modules import (ACTS, LinearP, ModelOutput, PlannedModule, _LayerNorm, _PlanCache, _versions, clip_init_rule, init_synthetic_,
                      pack_clip_layers, run_clip_layers)
from .text_encoder import _Encoder


@dataclass(frozen=True)
class CLIPVisionConfig:
    """transformers ``CLIPVisionConfig`` fields the encoder uses (``projection_dim`` included); defaults are
    ``openai/clip-vit-large-patch14-336``, CMMD's embedding model."""
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    num_channels: int = 3
    patch_size: int = 14
    image_size: int = 336
    projection_dim: int = 768
    hidden_act: str = "quick_gelu"
    layer_norm_eps: float = 1e-5

    @classmethod
    def from_dict(cls, d: dict) -> "CLIPVisionConfig":
        """a CLIPVisionConfig dict, or a full CLIPModel config (its ``vision_config`` and top-level ``projection_dim``)"""
        if "vision_config" in d:
            top, d = d, dict(d["vision_config"])
            if "projection_dim" in top:
                d["projection_dim"] = top["projection_dim"]
        return cls(**{f.name: d[f.name] for f in fields(cls) if f.name in d})

    @classmethod
    def vit_b_32(cls) -> "CLIPVisionConfig":
        """``openai/clip-vit-base-patch32``, the model of the reference's CLIP score"""
        return cls(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, patch_size=32,
                   image_size=224, projection_dim=512)

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def num_tokens(self) -> int:
        return 1 + self.grid * self.grid


def image_encoder_flops(cfg: CLIPVisionConfig) -> float:
    """algorithmic FLOPs of one encode of ONE image: the patch GEMM, per layer the linears (q|k|v, out_proj, fc1, fc2) over all
    tokens and the attention's two contractions over all (query, key) pairs, and the projection of the class row"""
    H, I, T = cfg.hidden_size, cfg.intermediate_size, cfg.num_tokens
    patch = 2.0 * (T - 1) * cfg.num_channels * cfg.patch_size ** 2 * H
    lin = 2.0 * T * (4 * H * H + 2 * H * I)
    attn = 2.0 * 2.0 * H * T * T
    return patch + cfg.num_hidden_layers * (lin + attn) + 2.0 * H * cfg.projection_dim


class _PatchEmbedding(nn.Module):
    def __init__(self, cin: int, c: int, p: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(c, cin, p, p))


class _PositionEmbedding(nn.Module):
    def __init__(self, n: int, c: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n, c))


class _VisionEmbeddings(nn.Module):
    def __init__(self, cfg: CLIPVisionConfig):
        super().__init__()
        self.class_embedding = nn.Parameter(torch.empty(cfg.hidden_size))
        self.patch_embedding = _PatchEmbedding(cfg.num_channels, cfg.hidden_size, cfg.patch_size)
        self.position_embedding = _PositionEmbedding(cfg.num_tokens, cfg.hidden_size)


class _VisionTransformer(nn.Module):
    def __init__(self, cfg: CLIPVisionConfig):
        super().__init__()
        self.embeddings = _VisionEmbeddings(cfg)
        self.pre_layrnorm = _LayerNorm(cfg.hidden_size, cfg.layer_norm_eps)
        self.encoder = _Encoder(cfg)
        self.post_layernorm = _LayerNorm(cfg.hidden_size, cfg.layer_norm_eps)


@dataclass
class CLIPVisionModelOutput(ModelOutput):
    """transformers' ``CLIPVisionModelOutput`` as CMMD uses it: ``.image_embeds`` / ``out[0]``, then ``last_hidden_state``."""
    image_embeds: torch.Tensor
    last_hidden_state: torch.Tensor


def _is_foreign(name: str) -> bool:
    """keys of a full CLIPModel checkpoint that are not the vision tower's, and the position_ids buffers"""
    return (name.startswith("text_model.") or name.startswith("text_projection.") or name == "logit_scale"
            or name.endswith("embeddings.position_ids"))


class CLIPVisionModelWithProjection(PlannedModule):
    """``CLIPVisionModelWithProjection`` of transformers for 64-wide heads, 3-channel images and ``hidden_act`` "quick_gelu" or
    "gelu", forward only."""

    def __init__(self, config: Optional[CLIPVisionConfig] = None, **kw):
        super().__init__()
        cfg = config or CLIPVisionConfig(**kw)
        if cfg.hidden_act not in ACTS:
            raise NotImplementedError(f"CLIPVisionModelWithProjection: hidden_act {cfg.hidden_act!r} (only 'quick_gelu' and 'gelu')")
        if cfg.hidden_size % cfg.num_attention_heads != 0 or cfg.head_dim != 64:
            raise NotImplementedError(f"CLIPVisionModelWithProjection: head dim {cfg.hidden_size / cfg.num_attention_heads:g} (only 64)")
        if cfg.num_channels != 3:
            raise NotImplementedError(f"CLIPVisionModelWithProjection: {cfg.num_channels} image channels (only 3)")
        if cfg.patch_size < 1 or cfg.image_size < cfg.patch_size or cfg.image_size % cfg.patch_size != 0:
            raise ValueError(f"CLIPVisionModelWithProjection: image size {cfg.image_size} is not a multiple of patch size {cfg.patch_size}")
        if cfg.hidden_size > 2048 or cfg.projection_dim % 8 != 0:
            raise NotImplementedError("CLIPVisionModelWithProjection: hidden_size <= 2048 and projection_dim a multiple of 8")
        self.config = cfg
        self.vision_model = _VisionTransformer(cfg)
        self.visual_projection = LinearP(cfg.hidden_size, cfg.projection_dim, bias=False)
        self._plans = _PlanCache(cap=2)          # one plan per activation dtype

    # ---- weights ----------------------------------------------------------------------------------------------------
    def init_synthetic(self, seed: int = 0) -> "CLIPVisionModelWithProjection":
        """Deterministic weights under which every layer changes the residual stream measurably (the text encoder's recipe):
        linear weights with std fan_in^-1/2 (out_proj and fc2 scaled by 0.5), the patch convolution likewise over its 3 P^2
        inputs, LayerNorm affine near identity, small biases, class and position embeddings with std 0.5."""
        return init_synthetic_(self, seed, clip_init_rule)

    def load_vision_state_dict(self, sd: Dict[str, torch.Tensor]) -> "CLIPVisionModelWithProjection":
        """Strict load of a transformers CLIPVisionModelWithProjection state dict.  ``position_ids`` buffers are ignored, and so
        are the ``text_model.*`` / ``text_projection.*`` / ``logit_scale`` keys of a full CLIPModel file; any other missing,
        unexpected or mis-shaped key raises."""
        return load_strict(self, sd, ignore=_is_foreign)

    @classmethod
    def from_pretrained(cls, root: str, subfolder: Optional[str] = None) -> "CLIPVisionModelWithProjection":
        """Read ``config.json`` and ``model.safetensors`` of a transformers CLIPVisionModelWithProjection or CLIPModel folder."""
        cfg, sd = read_pretrained(CLIPVisionConfig, root, subfolder, "model.safetensors", skip=_is_foreign)
        return cls(cfg).load_vision_state_dict(sd)

    # ---- packed weights ---------------------------------------------------------------------------------------------
    def plan(self, device) -> dict:
        """packed weights per (device, ACT_DTYPE) in the _PlanCache: a plan seen during a capture outlives the graph; a weight
        update (parameter versions) replaces the entry"""
        key, version = (str(device), ops.ACT_DTYPE), _versions(self)
        pl = self._plans.get(key, version)
        if pl is not None:
            return pl
        f32 = lambda t: t.detach().float().to(device).contiguous()      # noqa: E731
        ln = lambda m: (f32(m.weight), f32(m.bias))                     # noqa: E731
        vm = self.vision_model
        emb = vm.embeddings
        pl = {"patch": ops.pack_weight(emb.patch_embedding.weight.detach().flatten(1), None, device=device),   # rows in (c, py, px) order
              "cls": f32(emb.class_embedding), "pos": f32(emb.position_embedding.weight),
              "pre": ln(vm.pre_layrnorm), "post": ln(vm.post_layernorm),
              "proj": ops.pack_weight(self.visual_projection.weight.detach(), None, device=device),
              "layers": pack_clip_layers(vm.encoder.layers, device, fold=False)}
        return self._plans.put(key, version, pl)

    # ---- forward ----------------------------------------------------------------------------------------------------
    def _device(self):
        dev = self.vision_model.embeddings.class_embedding.device
        if dev.type != "cuda":
            raise RuntimeError("CLIPVisionModelWithProjection runs on the HIP kernels only: move it to a GPU first (model.to('cuda'))")
        return dev

    def encode_patches(self, patches: torch.Tensor, B: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """``ops.image_patches`` rows of B images, in ops.ACT_DTYPE -> (image_embeds fp32 [B, proj], the encoder's output in
        ops.ACT_DTYPE [B, tokens, hidden])"""
        cfg = self.config
        pl = self.plan(patches.device)
        C, eps = cfg.hidden_size, cfg.layer_norm_eps
        G2 = cfg.grid * cfg.grid
        pe = ops.linear(patches.view(B, G2, patches.shape[1])[..., :pl["patch"].Cin], pl["patch"], out_f32=True)
        x = ops.vit_embed_ln(pe.view(B * G2, C), B, pl["cls"], pl["pos"], *pl["pre"], eps=eps, out_f32=ops.ACT_DTYPE == torch.float32)
        x = run_clip_layers(x, pl["layers"], attn=ops.attention, heads=cfg.num_attention_heads, act=ACTS[cfg.hidden_act], eps=eps,
                            who="CLIPVisionModelWithProjection")
        pooled = ops.layernorm(x[:, 0, :].unsqueeze(0), *pl["post"], eps)          # the class rows as one [1, B, C] strided view
        emb = ops.linear(pooled, pl["proj"], out_f32=True)
        return emb[0], x

    @torch.no_grad()
    def embed_images(self, images: torch.Tensor) -> torch.Tensor:
        """fp32 images in [0, 1] on the device, [B, H, W, 3] or [B, 3, H, W] of any size -> image_embeds fp32 [B, proj]: CMMD's
        preprocessing (bicubic resize to image_size, CLIP mean / std) inside the front-end kernel, then the encoder"""
        dev = self._device()
        if images.dim() != 4 or images.dtype != torch.float32 or images.device != dev:
            raise ValueError(f"CLIPVisionModelWithProjection: images must be an fp32 4-D tensor on {dev}, got {images.dtype} "
                             f"{tuple(images.shape)} on {images.device}")
        cfg = self.config
        patches = ops.image_patches(images.contiguous(), cfg.image_size, cfg.patch_size, out_f32=ops.ACT_DTYPE == torch.float32)
        return self.encode_patches(patches, images.shape[0])[0]

    @torch.no_grad()
    def forward(self, pixel_values: torch.Tensor, output_attentions: bool = False, output_hidden_states: bool = False,
                interpolate_pos_encoding: bool = False, return_dict: bool = True, **kw):
        """pixel_values fp32 [B, 3, image_size, image_size] (already normalised) -> image_embeds fp32 [B, projection_dim], not
        normalised, and last_hidden_state fp32 [B, tokens, hidden] (the encoder's output, before post_layernorm)."""
        if output_attentions or output_hidden_states or interpolate_pos_encoding or kw:
            raise NotImplementedError("CLIPVisionModelWithProjection: output_attentions, output_hidden_states, "
                                      "interpolate_pos_encoding and other arguments are not supported")
        cfg = self.config
        dev = self._device()
        S = cfg.image_size
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, S, S) or pixel_values.shape[0] < 1 \
                or not pixel_values.is_floating_point():
            raise ValueError(f"CLIPVisionModelWithProjection: pixel_values must be a floating [B, 3, {S}, {S}] tensor, got "
                             f"{pixel_values.dtype} {tuple(pixel_values.shape)}")
        px = pixel_values.to(device=dev, dtype=torch.float32).contiguous()
        patches = ops.image_patches(px, S, cfg.patch_size, resize=False, out_f32=ops.ACT_DTYPE == torch.float32)
        emb, h = self.encode_patches(patches, px.shape[0])
        out = CLIPVisionModelOutput(image_embeds=emb, last_hidden_state=h.float())
        return out if return_dict else out.to_tuple()
