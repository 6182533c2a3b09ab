"""The text side of the CLIP score: ``CLIPTextModelWithProjection`` and ``CLIPModel`` (transformers semantics) on the HIP kernels.

The reference turns captions into the unit-norm text features of its CLIP score with OpenAI ViT-B/32's ``encode_text``
(pdm/utils/clip_utils.py:174-194, :224-263, scripts/metrics/clip_features.py): token and position embeddings, 12 pre-LayerNorm
layers with QuickGELU under the causal mask, ``ln_final``, the row at ``text.argmax(-1)``, ``text_projection``.  transformers
stores the same model as ``CLIPModel`` (``text_model.*``, ``text_projection.weight``, ``vision_model.*``,
``visual_projection.weight``, ``logit_scale``); this module keeps those names.

  * ``CLIPTextModelWithProjection`` runs the layer stack of text_encoder.py (its ``_TextTower``: the same plans, the same folded
    LayerNorms, ``hidden_act`` "quick_gelu" or "gelu") and then pools BEFORE normalising: ``ops.eos_pool_ln`` finds each
    prompt's pooling position from the ids and applies ``final_layer_norm`` to that one row, and a bias-free ``ops.linear`` with
    fp32 output is the projection.  ``last_hidden_state`` (the final LayerNorm of all B x L rows, cast to fp32) is computed only
    by ``forward``; ``embed_ids`` -- what the score uses -- never touches the other rows.
  * ``CLIPModel`` holds that tower, ``image_encoder.CLIPVisionModelWithProjection`` and ``logit_scale``.

Token ids in, as everywhere in this package; there is no tokenizer here.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, fields
from typing import Dict, Optional

import torch

from . import ops
from .image_encoder import CLIPVisionConfig, CLIPVisionModelWithProjection
from .loading import load_strict, read_pretrained, read_safetensors
from .modules import LinearP, ModelOutput
from .text_encoder import CLIPTextConfig, _TextTower


@dataclass(frozen=True)
class CLIPTextProjectionConfig(CLIPTextConfig):
    """``CLIPTextConfig`` plus ``projection_dim``; the defaults of the added and changed fields are
    ``openai/clip-vit-base-patch32``'s text tower as transformers stores it (eos_token_id 2: pooling at the largest id)."""
    hidden_size: int = 512
    intermediate_size: int = 2048
    num_hidden_layers: int = 12
    num_attention_heads: int = 8
    hidden_act: str = "quick_gelu"
    projection_dim: int = 512

    @classmethod
    def from_dict(cls, d: dict) -> "CLIPTextProjectionConfig":
        """a CLIPTextConfig dict, or a full CLIPModel config (its ``text_config`` and top-level ``projection_dim``)"""
        if "text_config" in d:
            top, d = d, dict(d["text_config"])
            if "projection_dim" in top:
                d["projection_dim"] = top["projection_dim"]
        return cls(**{f.name: d[f.name] for f in fields(cls) if f.name in d})


@dataclass
class CLIPTextModelOutput(ModelOutput):
    """transformers' ``CLIPTextModelOutput``: ``.text_embeds`` / ``out[0]``, then ``last_hidden_state``."""
    text_embeds: torch.Tensor
    last_hidden_state: torch.Tensor


def _is_foreign(name: str) -> bool:
    """keys of a full CLIPModel checkpoint that are not the text tower's, and the position_ids buffers"""
    return (name.startswith("vision_model.") or name.startswith("visual_projection.") or name == "logit_scale"
            or name.endswith("embeddings.position_ids"))


class CLIPTextModelWithProjection(_TextTower):
    """``CLIPTextModelWithProjection`` of transformers for 64-wide heads and ``hidden_act`` "quick_gelu" or "gelu", forward only."""

    _ACTS_ACCEPTED = ("quick_gelu", "gelu")
    _ACTS_NOTE = "only 'quick_gelu' and 'gelu'"

    def __init__(self, config: Optional[CLIPTextProjectionConfig] = None, **kw):
        cfg = config or CLIPTextProjectionConfig(**kw)
        if not hasattr(cfg, "projection_dim"):
            raise TypeError("CLIPTextModelWithProjection: the config needs projection_dim (CLIPTextProjectionConfig)")
        super().__init__(cfg)
        if cfg.hidden_size > 2048 or cfg.projection_dim < 8 or cfg.projection_dim % 8 != 0:
            raise NotImplementedError("CLIPTextModelWithProjection: hidden_size <= 2048 and projection_dim a multiple of 8")
        self.text_projection = LinearP(cfg.hidden_size, cfg.projection_dim, bias=False)

    # ---- weights ----------------------------------------------------------------------------------------------------
    def load_text_state_dict(self, sd: Dict[str, torch.Tensor]) -> "CLIPTextModelWithProjection":
        """Strict load of a transformers CLIPTextModelWithProjection state dict.  ``position_ids`` buffers are ignored, and so
        are the ``vision_model.*`` / ``visual_projection.*`` / ``logit_scale`` keys of a full CLIPModel file; any other missing,
        unexpected or mis-shaped key raises."""
        return load_strict(self, sd, ignore=_is_foreign)

    @classmethod
    def from_pretrained(cls, root: str, subfolder: Optional[str] = None) -> "CLIPTextModelWithProjection":
        """Read ``config.json`` and ``model.safetensors`` of a transformers CLIPTextModelWithProjection or CLIPModel folder."""
        cfg, sd = read_pretrained(CLIPTextProjectionConfig, root, subfolder, "model.safetensors", skip=_is_foreign)
        return cls(cfg).load_text_state_dict(sd)

    def _plan_extra(self, pl: dict, device):
        pl["proj"] = ops.pack_weight(self.text_projection.weight.detach(), None, device=device)

    # ---- forward ----------------------------------------------------------------------------------------------------
    @property
    def eos_mode(self) -> str:
        """transformers' rule: the largest id when eos_token_id == 2 (every checkpoint converted from OpenAI's, whose
        encode_text does the same), the first eos_token_id otherwise"""
        return "argmax" if self.config.eos_token_id == 2 else "first_eos"

    def _pool_project(self, ids: torch.Tensor, x: torch.Tensor, pl: dict) -> torch.Tensor:
        cfg = self.config
        _, pooled = ops.eos_pool_ln(ids, x, *pl["final"], cfg.layer_norm_eps, eos_mode=self.eos_mode, eos_token_id=cfg.eos_token_id)
        return ops.linear(pooled.unsqueeze(0), pl["proj"], out_f32=True)[0]

    @torch.no_grad()
    def embed_ids(self, input_ids: torch.Tensor) -> torch.Tensor:
        """input_ids int64 [B, L] -> text_embeds fp32 [B, projection_dim], not normalised (``get_text_features``): the layer
        stack, final_layer_norm of the pooled rows only, the projection"""
        ids = self._device_ids(input_ids)
        x, pl = self.encode_stream(ids)
        return self._pool_project(ids, x, pl)

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask=None, position_ids=None, output_hidden_states: bool = False,
                return_dict: bool = True, **kw):
        """input_ids int64 [B, L], 1 <= L <= max_position_embeddings -> text_embeds fp32 [B, projection_dim], not normalised,
        and last_hidden_state fp32 [B, L, hidden]."""
        if attention_mask is not None or position_ids is not None or output_hidden_states or kw:
            raise NotImplementedError("CLIPTextModelWithProjection: attention_mask, position_ids, output_hidden_states and other "
                                      "arguments are not supported (the tower runs with the causal mask only)")
        ids = self._device_ids(input_ids)
        x, pl = self.encode_stream(ids)
        emb = self._pool_project(ids, x, pl)
        h = ops.layernorm(x, *pl["final"], self.config.layer_norm_eps).float()
        out = CLIPTextModelOutput(text_embeds=emb, last_hidden_state=h)
        return out if return_dict else out.to_tuple()


class CLIPModel:
    """transformers' ``CLIPModel`` as the CLIP score uses it: the two towers with their projections and ``logit_scale`` (the
    stored parameter, a logarithm: the score multiplies by ``logit_scale_exp``)."""

    def __init__(self, text_model: CLIPTextModelWithProjection, vision_model: CLIPVisionModelWithProjection, logit_scale: float = 4.6052):
        if text_model.config.projection_dim != vision_model.config.projection_dim:
            raise ValueError(f"CLIPModel: the towers project to {text_model.config.projection_dim} and "
                             f"{vision_model.config.projection_dim} dimensions")
        self.text_model = text_model
        self.vision_model = vision_model
        self.logit_scale = float(logit_scale)
        self.projection_dim = text_model.config.projection_dim

    @property
    def logit_scale_exp(self) -> float:
        import math
        return math.exp(self.logit_scale)

    @classmethod
    def from_pretrained(cls, root: str, subfolder: Optional[str] = None) -> "CLIPModel":
        """Read ``config.json`` (``text_config``, ``vision_config``, ``projection_dim``) and ``model.safetensors`` (both towers and
        ``logit_scale``) of a transformers CLIPModel folder; every key must belong to one of the three."""
        d = os.path.join(root, subfolder) if subfolder else root
        with open(os.path.join(d, "config.json")) as f:
            cfg = json.load(f)
        if "text_config" not in cfg or "vision_config" not in cfg:
            raise ValueError(f"CLIPModel: {d}/config.json has no text_config / vision_config (not a CLIPModel folder)")
        sd = read_safetensors(os.path.join(d, "model.safetensors"), skip=lambda n: n.endswith("embeddings.position_ids"))
        if "logit_scale" not in sd:
            raise KeyError("CLIPModel: missing key logit_scale")
        text = CLIPTextModelWithProjection(CLIPTextProjectionConfig.from_dict(cfg)).load_text_state_dict(sd)
        vision = CLIPVisionModelWithProjection(CLIPVisionConfig.from_dict(cfg)).load_vision_state_dict(sd)
        return cls(text, vision, float(sd["logit_scale"].reshape(-1)[0]))

    def to(self, device) -> "CLIPModel":
        self.text_model.to(device)
        self.vision_model.to(device)
        return self

    def get_text_features(self, input_ids: torch.Tensor) -> torch.Tensor:
        """fp32 [B, projection_dim], not normalised"""
        return self.text_model.embed_ids(input_ids)

    def get_image_features(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """pixel_values [B, 3, image_size, image_size], already preprocessed -> fp32 [B, projection_dim], not normalised"""
        return self.vision_model(pixel_values).image_embeds
