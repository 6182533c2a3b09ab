"""What the models of this package share besides the kernels: the plumbing of every module that packs weights, and the CLIP layer
stack of the two CLIP towers.

  * plumbing: the parameter containers ``_Params`` / ``LinearP``, ``_versions`` and the ``_PlanCache`` (unet.py imports them back:
    ``unet._PlanCache`` is this class), and ``PlannedModule``, the base of a module that keeps a ``_PlanCache`` in ``self._plans``:
    ``invalidate()`` and the ``_apply`` override that calls it, so ``.to()`` can never leave packs of replaced parameters behind;
  * what the forward-only encoders (text_encoder.py, clip_model.py, image_encoder.py, prompt_encoder.py) had each spelled out:
    ``ModelOutput`` (transformers' ``to_tuple`` / ``out[0]`` / ``out["name"]``), ``_Embedding``, ``_LayerNorm``, ``ACTS``,
    ``cat_qkv``, ``init_synthetic_`` (one loop, a per-model rule for the deviations) and ``check_token_ids``;
  * the pre-LayerNorm CLIP layer: ``pack_clip_layers`` and ``run_clip_layers`` -- LN1 -> fused q|k|v -> attention -> out_proj with
    the residual -> LN2 -> fc1 with the activation -> fc2 with the residual.  The towers choose the attention kernel and whether the
    LayerNorms are folded into the q|k|v and fc1 GEMMs (text_encoder.py describes the folded form and where it pays).

Nothing here launches a kernel of its own: every launch goes through ``ops``.
"""
from __future__ import annotations

from dataclasses import fields
from typing import Callable, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops

# ---- parameter containers (diffusers / transformers names and shapes at the state-dict boundary; never called) -----


class _Params(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container; the owning block launches the HIP kernels")


class LinearP(_Params):
    def __init__(self, cin, cout, bias=True):
        super().__init__()
        self.in_features, self.out_features = cin, cout
        self.weight = nn.Parameter(torch.empty(cout, cin))
        self.bias = nn.Parameter(torch.empty(cout)) if bias else None


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


# ---- packed-weight plans -------------------------------------------------------------------------------------------
def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _versions(mod: nn.Module) -> tuple:
    """in-place update counters of a module's parameters: optimizer steps, ``param.data.copy_`` and ``load_state_dict``
    all bump them, so packs made from older values can be recognised as stale without any hook on the training loop"""
    if mod.__dict__.get("_pk") is not None:
        return ()      # under a PackedTrainer the diffusers-layout masters are not what is trained: the packs ARE the state
    ps = mod.__dict__.get("_vparams")
    if ps is None:
        ps = mod.__dict__["_vparams"] = list(mod.parameters())      # (dropped by invalidate(): .to() may replace parameters)
    return tuple(p._version for p in ps)


class _PlanCache:
    """Packed-weight plans of one module, keyed by whatever the packs depend on besides the parameters (mask, semantics,
    device, activation dtype, ...).  Every module of the package that packs weights keeps them here.

    * At most ``cap`` UNPINNED entries; the oldest is evicted.  A plan that is created or looked up while a stream is
      capturing is PINNED: a HIP graph bakes raw pointers to its packs, so it must outlive the graph and is only released
      by ``clear()`` (``invalidate_plans``), however many other masks pass through the module in between.
    * Every entry remembers the parameter versions it was packed from.  A lookup with newer versions is a miss and drops
      the stale entry (a pinned one is parked, never returned again, so the memory a graph points to stays allocated):
      fine-tuning forwards always compute with the current weights, whatever loop drives the optimizer."""

    def __init__(self, cap: int = 4):
        self.cap, self.entries, self.parked = cap, {}, []

    def get(self, key, version):
        e = self.entries.get(key)
        if e is None:
            return None
        if e[0] != version:
            del self.entries[key]
            if e[2]:
                self.parked.append(e[1])
            return None
        if not e[2] and _capturing():
            e[2] = True
        return e[1]

    def put(self, key, version, plan):
        unpinned = [k for k, e in self.entries.items() if not e[2]]
        if len(unpinned) >= self.cap:
            del self.entries[unpinned[0]]
        self.entries[key] = [version, plan, _capturing()]
        return plan

    def lookup(self, key, version, make):
        """the current plan under ``key``, made by ``make()`` on a miss"""
        plan = self.get(key, version)
        return plan if plan is not None else self.put(key, version, make())

    def clear(self):
        self.entries.clear()
        self.parked.clear()

    def __len__(self):
        return len(self.entries)


class PlannedModule(nn.Module):
    """A module that keeps its packed weights in ``self._plans`` (a _PlanCache; each class sets its own, the caps differ).
    ``invalidate()`` releases the plans and the parameter list ``_versions`` remembers; anything that may replace the parameters
    (``.to()``, ``.float()``: they all go through ``_apply``) invalidates first."""

    def invalidate(self):
        self._plans.clear()
        self.__dict__.pop("_vparams", None)

    def _apply(self, fn, *a, **k):
        self.invalidate()
        return super()._apply(fn, *a, **k)


# ---- what the forward-only encoders share --------------------------------------------------------------------------
class ModelOutput:
    """Base of the transformers-style output dataclasses: ``out.to_tuple()`` is the fields in declaration order, ``out[0]``
    indexes that tuple and ``out["name"]`` is the attribute."""

    def to_tuple(self) -> tuple:
        return tuple(getattr(self, f.name) for f in fields(self))

    def __getitem__(self, i):
        if isinstance(i, str):
            return getattr(self, i)
        return self.to_tuple()[i]


ACTS = {"gelu": ops.ACT_GELU, "quick_gelu": ops.ACT_QUICK_GELU}      # transformers' hidden_act -> the GEMM epilogue's activation


def cat_qkv(q: LinearP, k: LinearP, v: LinearP) -> Tuple[torch.Tensor, torch.Tensor]:
    """(weight [3C, C], bias [3C]) of the one GEMM that computes q | k | v"""
    return torch.cat([q.weight, k.weight, v.weight], 0).detach(), torch.cat([q.bias, k.bias, v.bias], 0).detach()


@torch.no_grad()
def init_synthetic_(module: PlannedModule, seed: int, rule: Callable[[str, torch.Tensor], Optional[float]]):
    """Deterministic weights under which every layer changes the residual stream measurably, drawn from one generator in
    ``named_parameters()`` order: ``rule(name, p)`` may name the std of a parameter's normal draw (embeddings, the linears that
    feed a residual sum); where it returns None a bias gets std 0.02, a LayerNorm gamma 1 + 0.1 N(0, 1) and a weight std
    fan_in^-1/2.  Invalidates the plans and returns the module."""
    g = torch.Generator().manual_seed(seed)
    for name, p in module.named_parameters():
        std = rule(name, p)
        if std is not None:
            p.copy_(std * torch.randn(p.shape, generator=g))
        elif name.endswith("bias"):
            p.copy_(0.02 * torch.randn(p.shape, generator=g))
        elif p.dim() == 1:                                   # LayerNorm gamma
            p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
        else:
            p.copy_(p.shape[1] ** -0.5 * torch.randn(p.shape, generator=g))
    module.invalidate()
    return module


def clip_init_rule(name: str, p: torch.Tensor) -> Optional[float]:
    """init_synthetic_'s rule of both CLIP towers: the patch convolution over its 3 P^2 inputs, the other embeddings with std
    0.5, out_proj and fc2 scaled by 0.5 so that the stream grows slowly over the residual additions"""
    if "patch_embedding" in name:
        return p[0].numel() ** -0.5
    if "embedding" in name:
        return 0.5
    if p.dim() == 2 and (".out_proj." in name or ".fc2." in name):
        return 0.5 * p.shape[1] ** -0.5
    return None


def check_token_ids(who: str, input_ids: torch.Tensor, device: torch.device, max_len: int, vocab_size: int) -> torch.Tensor:
    """the argument checks of an encoder's forward: integer [B, L] ids, 1 <= L <= max_len -> int64 ids on ``device`` (the
    model's, which must be a GPU).  The range check costs a host sync and is skipped while a graph is being captured."""
    if device.type != "cuda":
        raise RuntimeError(f"{who} runs on the HIP kernels only: move it to a GPU first (model.to('cuda'))")
    if input_ids.dim() != 2 or input_ids.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"{who}: input_ids must be an integer [B, L] tensor, got {input_ids.dtype} {tuple(input_ids.shape)}")
    B, L = input_ids.shape
    if B < 1 or not 1 <= L <= max_len:
        raise ValueError(f"{who}: sequence length {L} outside [1, {max_len}] (batch {B})")
    ids = input_ids.to(device=device, dtype=torch.int64).contiguous()
    if not torch.cuda.is_current_stream_capturing() and bool(((ids < 0) | (ids >= vocab_size)).any()):
        raise ValueError(f"{who}: token ids outside [0, {vocab_size})")
    return ids


# ---- the CLIP layer stack ------------------------------------------------------------------------------------------
def pack_clip_layers(layers, device, fold: bool) -> List[dict]:
    """One dict of packed weights per transformers ``CLIPEncoderLayer``: ``ln1`` / ``ln2`` (fp32 gamma, beta) and the packs
    ``qkv``, ``out``, ``fc1``, ``fc2``.  fold: the q|k|v and fc1 packs carry their LayerNorm (``qkv_ln``, ``fc1_ln``) wherever
    the producer emits statistics -- every launch but layer 0's q|k|v --, and their plain forms are made on demand
    (``qkv_make``, ``fc1_make``: run_clip_layers, a producer without statistics)."""
    f32 = lambda t: t.detach().float().to(device).contiguous()      # noqa: E731
    out = []
    for i, ly in enumerate(layers):
        a = ly.self_attn
        e = {"ln1": (f32(ly.layer_norm1.weight), f32(ly.layer_norm1.bias)),
             "ln2": (f32(ly.layer_norm2.weight), f32(ly.layer_norm2.bias)),
             "out": ops.pack_weight(a.out_proj.weight.detach(), a.out_proj.bias.detach(), device=device),
             "fc2": ops.pack_weight(ly.mlp.fc2.weight.detach(), ly.mlp.fc2.bias.detach(), device=device)}
        for nm, idx, (w, b) in (("qkv", 1, cat_qkv(a.q_proj, a.k_proj, a.v_proj)),
                                ("fc1", 2, (ly.mlp.fc1.weight.detach(), ly.mlp.fc1.bias.detach()))):
            g_, b_ = e[f"ln{idx}"]
            if fold and not (i == 0 and nm == "qkv"):
                e[nm + "_ln"] = ops.pack_weight(w, b, device=device, ln_gamma=g_, ln_beta=b_)
                e[nm + "_make"] = (lambda w=w, b=b: ops.pack_weight(w, b, device=device))
            else:
                e[nm] = ops.pack_weight(w, b, device=device)
        out.append(e)
    return out


def _ln_linear(x, st, e, idx, name, eps, who, **kw):
    """linear(LayerNorm_idx(x)): one launch when the producer of x emitted row statistics, otherwise the stand-alone
    LayerNorm kernel followed by the plain GEMM"""
    if st is not None:
        return ops.linear(x, e[name + "_ln"], ln=(st, eps), **kw)
    pw = e.get(name)
    if pw is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who}: run one eager encode of this shape before capturing it")
        pw = e[name] = e[name + "_make"]()
    g, b = e[f"ln{idx}"]
    return ops.linear(ops.layernorm(x, g, b, eps), pw, **kw)


def _with_stats(y):
    """ops.linear returns (y, statistics or None) when it was given the rowstats keyword, y alone otherwise"""
    return y if isinstance(y, tuple) else (y, None)


def run_clip_layers(x: torch.Tensor, layers: List[dict], *, attn, heads: int, act: int, eps: float, who: str,
                    fold: Optional[bool] = None) -> torch.Tensor:
    """The residual stream x [B, L, C] through pack_clip_layers' entries; ``attn(q, k, v, heads)`` is the attention kernel.
    fold of a tower that has both LayerNorm forms: out_proj and fc2 are launched with ``rowstats=fold``, and with the statistics
    the next q|k|v / fc1 finishes the LayerNorm in its epilogue.  None (a tower that only has stand-alone LayerNorms): the
    producers are launched without the keyword -- the same launches as ``fold=False``."""
    C = x.shape[-1]
    rs = {} if fold is None else {"rowstats": fold}
    st = None
    for e in layers:
        qkv = _ln_linear(x, st, e, 1, "qkv", eps, who)
        o = attn(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads)
        x, st = _with_stats(ops.linear(o, e["out"], residual=x, **rs))
        f = _ln_linear(x, st, e, 2, "fc1", eps, who, act=act)
        x, st = _with_stats(ops.linear(f, e["fc2"], residual=x, **rs))
    return x
