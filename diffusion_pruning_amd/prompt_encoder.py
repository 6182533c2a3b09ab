"""The router's prompt encoder: sentence-transformers/all-mpnet-base-v2 (transformers ``MPNetModel`` without the pooler,
followed by the masked mean) on the HIP kernels of this package.

APTP chooses the expert from ``hyper_net(mpnet_embedding)``.  The reference computes that embedding in
pdm/utils/data_utils.py:130-155 (``get_mpnet_embeddings``: tokenizer -> ``mpnet_model(**tok)[0]`` -> masked mean, NOT
L2-normalised) for the training batches (:158-172), the pipeline's ``hyper_net_input`` and ``filter_dataset`` (:195-223).
This module keeps transformers' parameter names (``embeddings.{word_embeddings, position_embeddings, LayerNorm}``,
``encoder.layer.i.attention.attn.{q,k,v,o}``, ``encoder.layer.i.attention.LayerNorm``, ``encoder.layer.i.intermediate.dense``,
``encoder.layer.i.output.{dense, LayerNorm}``, ``encoder.relative_attention_bias``) and runs every step on the kernels:

  * embeddings: ``ops.embed_ln`` (position ids from the ids, word row + position row, LayerNorm, one rounding);
  * each post-LayerNorm layer, 7 launches: one fused q|k|v linear -> ``ops.attention_bias`` (bidirectional, relative-position
    bias table [heads, 2L-1], key padding mask) -> o with the residual in its epilogue -> ``ops.layernorm`` -> intermediate
    dense with exact-erf GELU in its epilogue -> output dense with the residual in its epilogue -> ``ops.layernorm``;
  * ``encode``: ``ops.masked_mean`` on the stream.

The layers normalise AFTER the residual sum, so the LayerNorm output is itself the next residual and cannot be folded into
the next GEMM the way CLIP's pre-LayerNorms are.  The bias table is built on the host with the fp32 ``log`` expression of
``MPNetEncoder.relative_position_bucket`` (bucket boundaries cannot differ) and cached per L in the plan.

With ``ops.ACT_DTYPE = torch.float32`` the same code runs the fp32 parity instantiations of every kernel.  Every launch goes
to torch's current stream; ``forward`` makes no host sync while a graph is being captured (the id range check is skipped
then), so an encode can be captured with ``torch.cuda.graph`` after one eager call of the same shape.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import ops
from .launch_policy import _lean_tile
from .loading import load_strict, read_pretrained
from .modules import (LinearP, ModelOutput, PlannedModule, _Embedding, _LayerNorm, _PlanCache, _versions, cat_qkv, check_token_ids,
                      init_synthetic_)

# True: every linear of the bf16 path is launched on the lean tile of its row count with no K split, so every output element is one
# K-ordered accumulation whatever else shares the batch, and a prompt's embedding does not depend on the other prompts or on the
# padding (tests/test_prompt_encoder_gpu.py::test_padding_invariance).  False: launch_policy.choose_launch decides; it hands
# the output dense (K = 3072) of encodes of at most 512 tokens to the library's K-split heuristic, whose partial sums depend on
# the row count: measured on MI355X, the pooled embedding of 8 x 24 tokens then differs by 4.9e-3 from the same prompts padded
# to 8 x 64.  The fp32 parity path always takes its own tiles.
BATCH_INVARIANT = True


@dataclass(frozen=True)
class MPNetConfig:
    """transformers ``MPNetConfig`` fields the encoder uses; defaults are all-mpnet-base-v2's ``config.json``."""
    vocab_size: int = 30527
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    hidden_act: str = "gelu"
    max_position_embeddings: int = 514
    layer_norm_eps: float = 1e-5
    relative_attention_num_buckets: int = 32
    pad_token_id: int = 1

    @classmethod
    def from_dict(cls, d: dict) -> "MPNetConfig":
        return cls(**{f.name: d[f.name] for f in fields(cls) if f.name in d})

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads

    @property
    def max_length(self) -> int:
        """longest sequence: position ids run from pad + 1 to pad + L"""
        return self.max_position_embeddings - self.pad_token_id - 1


def prompt_encoder_flops(cfg: MPNetConfig, L: int) -> float:
    """algorithmic FLOPs of one encode of ONE sequence of L tokens: the linears (q, k, v, o, intermediate, output) and the
    attention's two contractions over all L x L (query, key) pairs (4 H L^2 per layer)"""
    H, I = cfg.hidden_size, cfg.intermediate_size
    lin = 2.0 * L * (4 * H * H + 2 * H * I)
    attn = 4.0 * H * L * L
    return cfg.num_hidden_layers * (lin + attn)


def relative_position_bucket(relative_position: torch.Tensor, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """``MPNetEncoder.relative_position_bucket``, expression for expression (the log is taken in fp32 as there)"""
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


def relative_bias_table(weight: torch.Tensor, L: int) -> torch.Tensor:
    """fp32 [heads, 2L - 1] on the CPU: entry [h, j - i + L - 1] = weight[bucket(j - i), h] (the bias depends on j - i only)"""
    rel = torch.arange(-(L - 1), L, dtype=torch.long)
    bucket = relative_position_bucket(rel, num_buckets=weight.shape[0])
    return weight.detach().float().cpu()[bucket].t().contiguous()


class _Embeddings(nn.Module):
    def __init__(self, cfg: MPNetConfig):
        super().__init__()
        self.word_embeddings = _Embedding(cfg.vocab_size, cfg.hidden_size)
        self.position_embeddings = _Embedding(cfg.max_position_embeddings, cfg.hidden_size)
        self.LayerNorm = _LayerNorm(cfg.hidden_size, cfg.layer_norm_eps)


class _SelfAttention(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.q, self.k, self.v, self.o = (LinearP(c, c) for _ in range(4))


class _Attention(nn.Module):
    def __init__(self, cfg: MPNetConfig):
        super().__init__()
        self.attn = _SelfAttention(cfg.hidden_size)
        self.LayerNorm = _LayerNorm(cfg.hidden_size, cfg.layer_norm_eps)


class _Intermediate(nn.Module):
    def __init__(self, cfg: MPNetConfig):
        super().__init__()
        self.dense = LinearP(cfg.hidden_size, cfg.intermediate_size)


class _Output(nn.Module):
    def __init__(self, cfg: MPNetConfig):
        super().__init__()
        self.dense = LinearP(cfg.intermediate_size, cfg.hidden_size)
        self.LayerNorm = _LayerNorm(cfg.hidden_size, cfg.layer_norm_eps)


class _Layer(nn.Module):
    def __init__(self, cfg: MPNetConfig):
        super().__init__()
        self.attention = _Attention(cfg)
        self.intermediate = _Intermediate(cfg)
        self.output = _Output(cfg)


class _Encoder(nn.Module):
    def __init__(self, cfg: MPNetConfig):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(cfg) for _ in range(cfg.num_hidden_layers)])
        self.relative_attention_bias = _Embedding(cfg.relative_attention_num_buckets, cfg.num_attention_heads)


@dataclass
class MPNetModelOutput(ModelOutput):
    """transformers' ``BaseModelOutput`` as the reference uses it: ``out[0]`` / ``.last_hidden_state``."""
    last_hidden_state: torch.Tensor


def _init_rule(name: str, p: torch.Tensor) -> Optional[float]:
    """init_synthetic_'s rule: a relative-position table with std 1 (O(1) score terms), embeddings with std 0.5, o and the output
    dense scaled by 0.5"""
    if name == "encoder.relative_attention_bias.weight":
        return 1.0
    if "embeddings.weight" in name:
        return 0.5
    if p.dim() == 2 and (".attn.o." in name or ".output.dense." in name):
        return 0.5 * p.shape[1] ** -0.5
    return None


def _ignored_key(n: str) -> bool:
    # the published checkpoint carries a pooler and a position_ids buffer the reference never uses
    return n.startswith("pooler.") or n == "embeddings.position_ids"


class MPNetModel(PlannedModule):
    """``MPNetModel`` of transformers without the pooler, for ``hidden_act == "gelu"`` and 64-wide heads, forward only (the
    reference runs the router's encoder under no_grad)."""

    def __init__(self, config: Optional[MPNetConfig] = None, **kw):
        super().__init__()
        cfg = config or MPNetConfig(**kw)
        if cfg.hidden_act != "gelu":
            raise NotImplementedError(f"MPNetModel: hidden_act {cfg.hidden_act!r} (only the exact-erf 'gelu')")
        if cfg.hidden_size % cfg.num_attention_heads != 0 or cfg.head_dim != 64:
            raise NotImplementedError(f"MPNetModel: head dim {cfg.hidden_size / cfg.num_attention_heads:g} (only 64)")
        if cfg.max_length > ops.BIAS_MAX_L:
            raise NotImplementedError(f"MPNetModel: max_position_embeddings {cfg.max_position_embeddings} allows sequences "
                                      f"longer than {ops.BIAS_MAX_L}")
        if cfg.relative_attention_num_buckets % 4 != 0:
            raise NotImplementedError("MPNetModel: relative_attention_num_buckets must be a multiple of 4")
        self.config = cfg
        self.embeddings = _Embeddings(cfg)
        self.encoder = _Encoder(cfg)
        self._plans = _PlanCache(cap=2)          # one per activation dtype

    # ---- weights ----------------------------------------------------------------------------------------------------
    def init_synthetic(self, seed: int = 0) -> "MPNetModel":
        """Deterministic weights under which every layer moves the residual stream measurably: linear weights with std
        fan_in^-1/2 (o and the output dense scaled by 0.5; the stream is re-normalised after every sum), LayerNorm affine
        near identity, small biases, embeddings with std 0.5, and a relative-position table with std 1 (O(1) score terms)."""
        return init_synthetic_(self, seed, _init_rule)

    def load_mpnet_state_dict(self, sd: Dict[str, torch.Tensor]) -> "MPNetModel":
        """Strict load of a transformers MPNetModel state dict (with or without an ``mpnet.`` prefix); ``pooler.*`` and
        ``embeddings.position_ids`` are ignored.  A missing, unexpected or mis-shaped key raises."""
        return load_strict(self, sd, lambda n: n[len("mpnet."):] if n.startswith("mpnet.") else n, _ignored_key)

    @classmethod
    def from_pretrained(cls, root: str, subfolder: Optional[str] = None) -> "MPNetModel":
        """Read ``config.json`` and ``model.safetensors`` of a transformers MPNetModel folder."""
        cfg, sd = read_pretrained(MPNetConfig, root, subfolder, "model.safetensors",
                                  skip=lambda n: n.endswith("embeddings.position_ids"))
        return cls(cfg).load_mpnet_state_dict(sd)

    # ---- packed weights ---------------------------------------------------------------------------------------------
    def plan(self, device) -> dict:
        """packed weights per (device, ACT_DTYPE) in the _PlanCache, with the relative-bias tables per L"""
        key, version = (str(device), ops.ACT_DTYPE), _versions(self)
        pl = self._plans.get(key, version)
        if pl is not None:
            return pl
        f32 = lambda t: t.detach().float().to(device).contiguous()      # noqa: E731
        pack = lambda m: ops.pack_weight(m.weight.detach(), m.bias.detach(), device=device)      # noqa: E731
        layers = []
        for ly in self.encoder.layer:
            a = ly.attention.attn
            layers.append({"qkv": ops.pack_weight(*cat_qkv(a.q, a.k, a.v), device=device), "o": pack(a.o),
                           "ln1": (f32(ly.attention.LayerNorm.weight), f32(ly.attention.LayerNorm.bias)),
                           "in": pack(ly.intermediate.dense), "out": pack(ly.output.dense),
                           "ln2": (f32(ly.output.LayerNorm.weight), f32(ly.output.LayerNorm.bias))})
        e = self.embeddings
        pl = {"word": f32(e.word_embeddings.weight), "pos": f32(e.position_embeddings.weight),
              "eln": (f32(e.LayerNorm.weight), f32(e.LayerNorm.bias)), "layers": layers, "bias": {}}
        return self._plans.put(key, version, pl)

    def _bias_table(self, pl: dict, L: int, device) -> torch.Tensor:
        t = pl["bias"].get(L)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("MPNetModel: run one eager encode of this shape before capturing it")
            t = pl["bias"][L] = relative_bias_table(self.encoder.relative_attention_bias.weight, L).to(device)
        return t

    # ---- forward ----------------------------------------------------------------------------------------------------
    def encode_stream(self, input_ids: torch.Tensor, key_mask: Optional[torch.Tensor]) -> torch.Tensor:
        """int64 [B, L] ids and an fp32 [B, L] mask (or None) on the device -> the last layer's output in ops.ACT_DTYPE
        [B, L, hidden]: 1 + 7 * layers launches"""
        cfg = self.config
        pl = self.plan(input_ids.device)
        C, nh, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
        rb = self._bias_table(pl, input_ids.shape[1], input_ids.device)
        x = ops.embed_ln(input_ids, pl["word"], pl["pos"], *pl["eln"], eps=eps, pad_id=cfg.pad_token_id,
                         out_f32=ops.ACT_DTYPE == torch.float32)
        kw = {}
        if BATCH_INVARIANT and ops.ACT_DTYPE != torch.float32:
            kw = {"tile": _lean_tile(input_ids.numel()), "split_k": 1}
        for e in pl["layers"]:
            qkv = ops.linear(x, e["qkv"], **kw)
            c = ops.attention_bias(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], nh, rb, key_mask)
            x = ops.layernorm(ops.linear(c, e["o"], residual=x, **kw), *e["ln1"], eps)
            f = ops.linear(x, e["in"], act=ops.ACT_GELU, **kw)
            x = ops.layernorm(ops.linear(f, e["out"], residual=x, **kw), *e["ln2"], eps)
        return x

    def _check_inputs(self, input_ids, attention_mask):
        cfg = self.config
        dev = self.embeddings.word_embeddings.weight.device
        ids = check_token_ids("MPNetModel", input_ids, dev, cfg.max_length, cfg.vocab_size)
        B, L = ids.shape
        mask = None
        if attention_mask is not None:
            if tuple(attention_mask.shape) != (B, L):
                raise ValueError(f"MPNetModel: attention_mask {tuple(attention_mask.shape)} does not match input_ids {(B, L)}")
            mask = attention_mask.to(device=dev, dtype=torch.float32).contiguous()
        return ids, mask

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, return_dict: bool = True, **kw):
        """input_ids int64 [B, L], 1 <= L <= max_position_embeddings - 2, attention_mask [B, L] of 0 / 1 (None: all ones)
        -> last_hidden_state fp32 [B, L, hidden].  Position ids come from input_ids (pad tokens), not from the mask."""
        if any(v is not None and v is not False for v in kw.values()):
            raise NotImplementedError(f"MPNetModel: arguments {sorted(kw)} are not supported (the reference passes input_ids "
                                      "and attention_mask only)")
        ids, mask = self._check_inputs(input_ids, attention_mask)
        out = MPNetModelOutput(last_hidden_state=self.encode_stream(ids, mask).float())
        return out if return_dict else out.to_tuple()

    @torch.no_grad()
    def encode(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``get_mpnet_embeddings``: fp32 [B, hidden] = the masked mean of the last hidden state, not L2-normalised"""
        ids, mask = self._check_inputs(input_ids, attention_mask)
        return ops.masked_mean(self.encode_stream(ids, mask), mask)


@torch.no_grad()
def assign_experts(prompt_encoder: MPNetModel, hyper_net, quantizer, input_ids: torch.Tensor,
                   attention_mask: Optional[torch.Tensor] = None, batch_size: int = 2048) -> torch.Tensor:
    """The device-side core of ``filter_dataset`` (pdm/utils/data_utils.py:195-223): int64 [N] expert indices of N tokenised
    captions -- encode -> hyper_net -> quantizer.get_cosine_sim_min_encoding_indices, in chunks of ``batch_size``, with
    hyper_net and quantizer in eval mode (their training flags are restored)."""
    if input_ids.dim() != 2 or input_ids.shape[0] < 1:
        raise ValueError(f"assign_experts: input_ids must be a non-empty [N, L] tensor, got {tuple(input_ids.shape)}")
    if batch_size < 1:
        raise ValueError("assign_experts: batch_size must be positive")
    was = [(m, m.training) for m in (hyper_net, quantizer)]
    for m, _ in was:
        m.eval()
    try:
        out = []
        for i in range(0, input_ids.shape[0], batch_size):
            am = None if attention_mask is None else attention_mask[i:i + batch_size]
            z = prompt_encoder.encode(input_ids[i:i + batch_size], am)
            out.append(quantizer.get_cosine_sim_min_encoding_indices(hyper_net(z)).to(torch.int64))
        return torch.cat(out)
    finally:
        for m, t in was:
            m.train(t)
