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
from .unet import LinearP, _PlanCache, _versions

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


class _Embedding(nn.Module):
    def __init__(self, n: int, c: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n, c))


class _LayerNorm(nn.Module):
    def __init__(self, c: int, eps: float):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.empty(c))
        self.bias = nn.Parameter(torch.empty(c))


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
class CLIPTextModelOutput:
    """transformers' ``BaseModelOutputWithPooling`` as the reference uses it: ``out[0]`` / ``.last_hidden_state``."""
    last_hidden_state: torch.Tensor
    pooler_output: torch.Tensor

    def to_tuple(self) -> Tuple[torch.Tensor, torch.Tensor]:
        return (self.last_hidden_state, self.pooler_output)

    def __getitem__(self, i):
        if isinstance(i, str):
            return getattr(self, i)
        return self.to_tuple()[i]


_ACTS = {"gelu": ops.ACT_GELU, "quick_gelu": ops.ACT_QUICK_GELU}


class _TextTower(nn.Module):
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
    @torch.no_grad()
    def init_synthetic(self, seed: int = 0):
        """Deterministic weights under which every layer changes the residual stream measurably: linear weights with std
        fan_in^-1/2 (out_proj and fc2 scaled by 0.5, so the stream grows slowly over the 23 residual additions), LayerNorm
        affine near identity, small biases, embeddings with std 0.5."""
        g = torch.Generator().manual_seed(seed)
        for name, p in self.named_parameters():
            if "embedding" in name:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            elif name.endswith("bias"):
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:                                   # LayerNorm gamma
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                scale = 0.5 if (".out_proj." in name or ".fc2." in name) else 1.0
                p.copy_(scale * p.shape[1] ** -0.5 * torch.randn(p.shape, generator=g))
        self.invalidate()
        return self

    def invalidate(self):
        self._plans.clear()
        self.__dict__.pop("_vparams", None)

    def _apply(self, fn, *a, **k):
        self.invalidate()
        return super()._apply(fn, *a, **k)

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
        layers = []
        for i, ly in enumerate(tm.encoder.layers):
            a = ly.self_attn
            wqkv = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0).detach()
            bqkv = torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0).detach()
            e = {"ln1": (f32(ly.layer_norm1.weight), f32(ly.layer_norm1.bias)),
                 "ln2": (f32(ly.layer_norm2.weight), f32(ly.layer_norm2.bias)),
                 "out": ops.pack_weight(a.out_proj.weight.detach(), a.out_proj.bias.detach(), device=device),
                 "fc2": ops.pack_weight(ly.mlp.fc2.weight.detach(), ly.mlp.fc2.bias.detach(), device=device)}
            for nm, idx, w, b in (("qkv", 1, wqkv, bqkv), ("fc1", 2, ly.mlp.fc1.weight.detach(), ly.mlp.fc1.bias.detach())):
                g_, b_ = e[f"ln{idx}"]
                # folded form wherever the producer emits statistics (every launch but layer 0's q|k|v); the plain form for
                # layer 0 and for the stand-alone LayerNorm path
                if fold and not (i == 0 and nm == "qkv"):
                    e[nm + "_ln"] = ops.pack_weight(w, b, device=device, ln_gamma=g_, ln_beta=b_)
                    e[nm + "_make"] = (lambda w=w, b=b: ops.pack_weight(w, b, device=device))
                else:
                    e[nm] = ops.pack_weight(w, b, device=device)
            layers.append(e)
        pl = {"tok": f32(tm.embeddings.token_embedding.weight), "pos": f32(tm.embeddings.position_embedding.weight),
              "final": (f32(tm.final_layer_norm.weight), f32(tm.final_layer_norm.bias)), "layers": layers}
        self._plan_extra(pl, device)
        return self._plans.put(key, version, pl)

    def _plan_extra(self, pl: dict, device):
        """packed weights a subclass needs beyond the tower's (the text projection)"""

    # ---- forward ----------------------------------------------------------------------------------------------------
    def _ln_linear(self, x, st, e, idx, name, **kw):
        """linear(LayerNorm_idx(x)): one launch when the producer of x emitted row statistics, otherwise the stand-alone
        LayerNorm kernel followed by the plain GEMM"""
        eps = self.config.layer_norm_eps
        if st is not None:
            return ops.linear(x, e[name + "_ln"], ln=(st, eps), **kw)
        pw = e.get(name)
        if pw is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{type(self).__name__}: run one eager encode of this shape before capturing it")
            pw = e[name] = e[name + "_make"]()
        g, b = e[f"ln{idx}"]
        return ops.linear(ops.layernorm(x, g, b, eps), pw, **kw)

    def encode_stream(self, input_ids: torch.Tensor) -> Tuple[torch.Tensor, dict]:
        """int64 [B, L] ids on the device -> (the residual stream after the last layer, before final_layer_norm, in
        ops.ACT_DTYPE [B, L, hidden]; the plan that encoded it)"""
        cfg = self.config
        act = _ACTS[cfg.hidden_act]
        fold = input_ids.numel() <= FOLD_LN_MAX_ROWS
        pl = self.plan(input_ids.device, fold)
        C, nh = cfg.hidden_size, cfg.num_attention_heads
        f32 = ops.ACT_DTYPE == torch.float32
        x = ops.token_embed(input_ids, pl["tok"], pl["pos"], out_f32=f32)
        st = None
        for e in pl["layers"]:
            qkv = self._ln_linear(x, st, e, 1, "qkv")
            o = ops.attention_causal(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], nh)
            x, st = ops.linear(o, e["out"], residual=x, rowstats=fold)
            f = self._ln_linear(x, st, e, 2, "fc1", act=act)
            x, st = ops.linear(f, e["fc2"], residual=x, rowstats=fold)
        return x, pl

    def encode_nhwc(self, input_ids: torch.Tensor) -> torch.Tensor:
        """int64 [B, L] ids on the device -> the final LayerNorm's output in ops.ACT_DTYPE [B, L, hidden]"""
        x, pl = self.encode_stream(input_ids)
        g, b = pl["final"]
        return ops.layernorm(x, g, b, self.config.layer_norm_eps)

    def _device_ids(self, input_ids: torch.Tensor) -> torch.Tensor:
        """the argument checks of a forward: int64 [B, L] ids on the model's device"""
        who = type(self).__name__
        cfg = self.config
        dev = self.text_model.embeddings.token_embedding.weight.device
        if dev.type != "cuda":
            raise RuntimeError(f"{who} runs on the HIP kernels only: move it to a GPU first (model.to('cuda'))")
        if input_ids.dim() != 2 or input_ids.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"{who}: input_ids must be an integer [B, L] tensor, got {input_ids.dtype} {tuple(input_ids.shape)}")
        B, L = input_ids.shape
        if B < 1 or not 1 <= L <= cfg.max_position_embeddings:
            raise ValueError(f"{who}: sequence length {L} outside [1, {cfg.max_position_embeddings}] (batch {B})")
        ids = input_ids.to(device=dev, dtype=torch.int64).contiguous()
        if not torch.cuda.is_current_stream_capturing() and bool(((ids < 0) | (ids >= cfg.vocab_size)).any()):
            raise ValueError(f"{who}: token ids outside [0, {cfg.vocab_size})")
        return ids


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
