"""SD-2.1's CLIP text encoder (transformers 4.34 ``CLIPTextModel`` semantics) on the HIP kernels of this package.

The reference encodes token ids with ``text_encoder(input_ids)[0]`` (pdm/training/trainer.py:1126, :1443 with the one-token
``torch.tensor([[100]])``, :1713) and in ``encode_prompt`` (pdm/pipelines/pruning_pipelines.py:735-744).  This module keeps
transformers' parameter names (``text_model.embeddings.{token,position}_embedding``, ``text_model.encoder.layers.i.{self_attn.
{q,k,v,out}_proj, layer_norm1, mlp.fc1, mlp.fc2, layer_norm2}``, ``text_model.final_layer_norm``) and runs every layer on
the kernels:

  * embeddings: ``ops.token_embed`` (token row + position row, fp32 sum, one rounding to the bf16 residual stream);
  * each pre-LayerNorm layer: LN1 -> one fused q|k|v linear with bias -> ``ops.attention_causal`` (16 heads of 64, scale
    1/8, causal mask only: SD-2.1's config has no padding mask) -> out_proj with the residual in its epilogue -> LN2 ->
    fc1 with exact-erf GELU in its epilogue (``ACT_GELU``) -> fc2 with the residual in its epilogue;
  * ``final_layer_norm``: ``ops.layernorm`` on the bf16 stream, followed by one cast to fp32 (``last_hidden_state`` is fp32).

LayerNorm folding (encodes of at most ``FOLD_LN_MAX_ROWS`` tokens): out_proj and fc2 emit per-row (sum, sumsq) partials of the
values they store;
the next q|k|v and fc1 launches read the un-normalised stream with gamma folded into their packed weights and beta into
their bias, and finish the normalisation in their epilogue (include/aptp_hip.h, ln_stats) -- no LayerNorm launch inside
the stack.  Layer 0's LN1 (its input comes from the embedding) and any launch whose producer could not emit statistics
take the stand-alone ``ops.layernorm``.  Larger encodes use stand-alone LayerNorms everywhere: measured on MI355X, the folded
form is 3.4 % faster at 2 x 77 tokens and 4.9 % / 1.8 % slower at 16 x 77 / 64 x 77 (profiles/r8_text_encoder_bench_line.json).
The layer loop and its packing are ``modules.run_clip_layers`` / ``pack_clip_layers``, which image_encoder.py runs too.

With ``ops.ACT_DTYPE = torch.float32`` the same code runs the fp32 parity instantiations of every kernel.
Every launch goes to torch's current stream; ``forward`` makes no host sync while a graph is being captured (the id range
check below is skipped then), so an encode can be captured with ``torch.cuda.graph`` after one eager warm-up call.
"""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from .loading import load_strict, read_pretrained
from .modules import (ACTS, LinearP, ModelOutput, PlannedModule, _Embedding, _LayerNorm, _PlanCache, _versions, check_token_ids,
                      clip_init_rule, init_synthetic_, pack_clip_layers, run_clip_layers)

# encodes of at most this many tokens (B * L) fold LN1 / LN2 into the q|k|v and fc1 GEMMs, larger ones launch stand-alone
# LayerNorms.  Measured (tools/bench_text_encoder.py, graph replays, both forms alternately): folded 1.455 vs 1.503 ms at
# 154 tokens, 2.631 vs 2.502 ms at 1,232, 6.974 vs 6.851 ms at 4,928.  The cut-off lies between the first two; 512 is not
# itself measured.  0 / a huge value force one form (A/B timing, tests).
FOLD_LN_MAX_ROWS = 512


@dataclass(frozen=True)
class CLIPTextConfig:
    """transformers ``CLIPTextConfig`` fields the encoder uses; defaults are SD-2.1's ``text_encoder/config.json``."""
    vocab_size: int = 49408
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_hidden_layers: int = 23
    num_attention_heads: int = 16
    max_position_embeddings: int = 77
    hidden_act: str = "gelu"
    layer_norm_eps: float = 1e-5
    bos_token_id: int = 0
    eos_token_id: int = 2
    pad_token_id: int = 1

    @classmethod
    def from_dict(cls, d: dict) -> "CLIPTextConfig":
        return cls(**{f.name: d[f.name] for f in fields(cls) if f.name in d})

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads


def text_encoder_flops(cfg: CLIPTextConfig, L: int) -> float:
    """algorithmic FLOPs of one encode of ONE sequence of L tokens: the linears (q|k|v, out_proj, fc1, fc2) and the causal
    attention's two contractions over the L (L + 1) / 2 (query, key) pairs that are not masked"""
    H, I = cfg.hidden_size, cfg.intermediate_size
    lin = 2.0 * L * (4 * H * H + 2 * H * I)
    attn = 2.0 * 2.0 * H * L * (L + 1) / 2
    return cfg.num_hidden_layers * (lin + attn)


class _Attention(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (LinearP(c, c) for _ in range(4))


class _MLP(nn.Module):
    def __init__(self, c: int, i: int):
        super().__init__()
        self.fc1, self.fc2 = LinearP(c, i), LinearP(i, c)


class _Layer(nn.Module):
    def __init__(self, cfg: CLIPTextConfig):
        super().__init__()
        self.self_attn = _Attention(cfg.hidden_size)
        self.layer_norm1 = _LayerNorm(cfg.hidden_size, cfg.layer_norm_eps)
        self.mlp = _MLP(cfg.hidden_size, cfg.intermediate_size)
        self.layer_norm2 = _LayerNorm(cfg.hidden_size, cfg.layer_norm_eps)


class _Embeddings(nn.Module):
    def __init__(self, cfg: CLIPTextConfig):
        super().__init__()
        self.token_embedding = _Embedding(cfg.vocab_size, cfg.hidden_size)
        self.position_embedding = _Embedding(cfg.max_position_embeddings, cfg.hidden_size)


class _Encoder(nn.Module):
    def __init__(self, cfg: CLIPTextConfig):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(cfg) for _ in range(cfg.num_hidden_layers)])


class _TextTransformer(nn.Module):
    def __init__(self, cfg: CLIPTextConfig):
        super().__init__()
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)
        self.final_layer_norm = _LayerNorm(cfg.hidden_size, cfg.layer_norm_eps)


@dataclass
class CLIPTextModelOutput(ModelOutput):
    """transformers' ``BaseModelOutputWithPooling`` as the reference uses it: ``out[0]`` / ``.last_hidden_state``."""
    last_hidden_state: torch.Tensor
    pooler_output: torch.Tensor


class _TextTower(PlannedModule):
    """What ``CLIPTextModel`` and ``clip_model.CLIPTextModelWithProjection`` share: the ``text_model`` parameters, the packed
    plans and the layer stack up to (not including) ``final_layer_norm``.  A subclass names the activations it accepts and adds
    its own loading and outputs."""

    _ACTS_ACCEPTED = ("gelu",)
    _ACTS_NOTE = "only the exact-erf 'gelu' of SD-2.x"

    def __init__(self, cfg: CLIPTextConfig):
        super().__init__()
        who = type(self).__name__
        if cfg.hidden_act not in self._ACTS_ACCEPTED:
            raise NotImplementedError(f"{who}: hidden_act {cfg.hidden_act!r} ({self._ACTS_NOTE})")
        if cfg.hidden_size % cfg.num_attention_heads != 0 or cfg.head_dim != 64:
            raise NotImplementedError(f"{who}: head dim {cfg.hidden_size / cfg.num_attention_heads:g} (only 64)")
        if cfg.max_position_embeddings > ops.CAUSAL_MAX_L:
            raise NotImplementedError(f"{who}: max_position_embeddings {cfg.max_position_embeddings} > {ops.CAUSAL_MAX_L}")
        self.config = cfg
        self.text_model = _TextTransformer(cfg)
        # 2 dtypes x 2 LayerNorm forms fit unpinned: an encode of one form never evicts the other form's packs
        self._plans = _PlanCache(cap=4)

    # ---- weights ----------------------------------------------------------------------------------------------------
    def init_synthetic(self, seed: int = 0):
        """Deterministic weights under which every layer changes the residual stream measurably: linear weights with std
        fan_in^-1/2 (out_proj and fc2 scaled by 0.5, so the stream grows slowly over the 23 residual additions), LayerNorm
        affine near identity, small biases, embeddings with std 0.5."""
        return init_synthetic_(self, seed, clip_init_rule)

    # ---- packed weights ---------------------------------------------------------------------------------------------
    def plan(self, device, fold: bool = True) -> dict:
        """packed weights per (device, ACT_DTYPE, LayerNorm form) in the _PlanCache: a plan seen during a capture outlives
        the graph, whichever form or dtype is encoded afterwards; a weight update (parameter versions) replaces the entry"""
        key, version = (str(device), ops.ACT_DTYPE, fold), _versions(self)
        pl = self._plans.get(key, version)
        if pl is not None:
            return pl
        f32 = lambda t: t.detach().float().to(device).contiguous()      # noqa: E731
        tm = self.text_model
        pl = {"tok": f32(tm.embeddings.token_embedding.weight), "pos": f32(tm.embeddings.position_embedding.weight),
              "final": (f32(tm.final_layer_norm.weight), f32(tm.final_layer_norm.bias)),
              "layers": pack_clip_layers(tm.encoder.layers, device, fold)}
        self._plan_extra(pl, device)
        return self._plans.put(key, version, pl)

    def _plan_extra(self, pl: dict, device):
        """packed weights a subclass needs beyond the tower's (the text projection)"""

    # ---- forward ----------------------------------------------------------------------------------------------------
    def encode_stream(self, input_ids: torch.Tensor) -> Tuple[torch.Tensor, dict]:
        """int64 [B, L] ids on the device -> (the residual stream after the last layer, before final_layer_norm, in
        ops.ACT_DTYPE [B, L, hidden]; the plan that encoded it)"""
        cfg = self.config
        fold = input_ids.numel() <= FOLD_LN_MAX_ROWS
        pl = self.plan(input_ids.device, fold)
        x = ops.token_embed(input_ids, pl["tok"], pl["pos"], out_f32=ops.ACT_DTYPE == torch.float32)
        x = run_clip_layers(x, pl["layers"], attn=ops.attention_causal, heads=cfg.num_attention_heads, act=ACTS[cfg.hidden_act],
                            eps=cfg.layer_norm_eps, who=type(self).__name__, fold=fold)
        return x, pl

    def encode_nhwc(self, input_ids: torch.Tensor) -> torch.Tensor:
        """int64 [B, L] ids on the device -> the final LayerNorm's output in ops.ACT_DTYPE [B, L, hidden]"""
        x, pl = self.encode_stream(input_ids)
        g, b = pl["final"]
        return ops.layernorm(x, g, b, self.config.layer_norm_eps)

    def _device_ids(self, input_ids: torch.Tensor) -> torch.Tensor:
        """the argument checks of a forward: int64 [B, L] ids on the model's device"""
        cfg = self.config
        return check_token_ids(type(self).__name__, input_ids, self.text_model.embeddings.token_embedding.weight.device,
                               cfg.max_position_embeddings, cfg.vocab_size)


class CLIPTextModel(_TextTower):
    """``CLIPTextModel`` of transformers 4.34 for ``hidden_act == "gelu"`` and 64-wide heads, forward only (the reference freezes
    the text encoder, trainer.py:725)."""

    def __init__(self, config: Optional[CLIPTextConfig] = None, **kw):
        super().__init__(config or CLIPTextConfig(**kw))

    def load_text_state_dict(self, sd: Dict[str, torch.Tensor]) -> "CLIPTextModel":
        """Strict load of a transformers CLIPTextModel state dict, with or without the ``text_model.`` prefix (transformers
        4.34 writes it); ``embeddings.position_ids`` (a buffer some checkpoints carry) is ignored.  A missing, unexpected
        or mis-shaped key raises."""
        return load_strict(self, sd, lambda n: n if n.startswith("text_model.") else "text_model." + n,
                           lambda n: n == "text_model.embeddings.position_ids")

    @classmethod
    def from_pretrained(cls, root: str, subfolder: Optional[str] = "text_encoder") -> "CLIPTextModel":
        """Read ``config.json`` and ``model.safetensors`` of a transformers CLIPTextModel folder."""
        cfg, sd = read_pretrained(CLIPTextConfig, root, subfolder, "model.safetensors",
                                  skip=lambda n: n.endswith("embeddings.position_ids"))
        return cls(cfg).load_text_state_dict(sd)

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask=None, position_ids=None, output_hidden_states: bool = False,
                return_dict: bool = True, **kw):
        """input_ids int64 [B, L], 1 <= L <= max_position_embeddings -> last_hidden_state fp32 [B, L, hidden] and
        pooler_output fp32 [B, hidden] (transformers 4.34: the row at input_ids.argmax(-1) when eos_token_id == 2, else at
        the first eos_token_id)."""
        if attention_mask is not None or position_ids is not None or output_hidden_states or kw:
            raise NotImplementedError("CLIPTextModel: attention_mask, position_ids, output_hidden_states and other arguments "
                                      "are not supported (SD-2.1's encoder runs with the causal mask only)")
        cfg = self.config
        ids = self._device_ids(input_ids)
        B, dev = ids.shape[0], ids.device
        h = self.encode_nhwc(ids).float()
        if cfg.eos_token_id == 2:
            eos_at = ids.argmax(dim=-1)
        else:
            eos_at = (ids == cfg.eos_token_id).int().argmax(dim=-1)
        pooled = h[torch.arange(B, device=dev), eos_at]
        out = CLIPTextModelOutput(last_hidden_state=h, pooler_output=pooled)
        return out if return_dict else out.to_tuple()
