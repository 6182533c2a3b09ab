"""Tensor-level wrappers over the C ABI (include/aptp_hip.h).

Activations are bf16 channels-last tensors ``[B, H, W, C]`` whose last dim is contiguous; the pixel stride
``x.stride(2)`` may exceed C (a channel slice of a wider buffer), which is how skip-concats are consumed without
copies.  Token tensors ``[B, L, C]`` are passed as ``[B, L, 1, C]``.  All launches go to torch's current stream,
so the whole forward can be captured into a HIP graph with ``torch.cuda.graph``.
"""
from __future__ import annotations

import ctypes
import os
import threading
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib, scratch
from ._lib import ImageInParams, LatentDistParams, UnetEpilogueParams, UnetPrologueParams
from ._lib import ACT_GELU, AttentionCausalParams, TokenEmbedParams  # noqa: F401
from ._lib import AttentionBiasParams, EmbedLnParams, MaskedMeanParams
from ._lib import ACT_QUICK_GELU, ImagePatchesParams, L2NormalizeParams, MmdRbfParams, VitEmbedLnParams  # noqa: F401
from ._lib import EOS_ARGMAX, EOS_FIRST, EosPoolLnParams, ImagePatchesPilParams, PairedCosineParams
from ._lib import GuidedStepParams, LossStageParams, LossTermsParams, PhiloxNormalParams, TrainNoiseParams
from ._lib import GumbelRelaxParams, PhiloxGumbelParams, RouterStageParams, SinkhornParams
from ._lib import (ACT_GEGLU, ACT_NONE, ACT_SILU, AttentionBwdParams, AttentionParams, ConvGemmParams, DepthLerpParams, GateBwdParams, WgradParams, FfTailParams, FoldRowsParams, PackDgradParams, MseParams,
                   GegluParams, GroupNormBwdParams, GroupNormParams, LayerNormBwdParams, LayerNormParams,
                   ColsumParams, LayerNormPgradParams, AttentionWideParams, ImageOutParams)
# The tuning table and the rules that pick a launch's tile / split-K depth / order live in launch_policy.py (pure host logic).
# The names are re-exported for readers (tests, bench.py, tools); TUNING is the very dict the lookup reads.  Change the table
# through set_tuning / set_entry, and the policy's switches on the launch_policy module itself.
from .launch_policy import (BK, SK_AUTO, SK_TILE_FIRST, TUNING, _HALO_TILES, choose_launch, key_of, parse_key,  # noqa: F401
                            set_entry, set_tuning, splitk_in_kernel, tuning_key, tuning_lookup)

# Storage type of activations and packed weights.  The HIP kernels exist for bf16 only (MFMA operands); the test-only CPU
# emulator (tests/hip_emulator.py) can switch both to fp32 to run the SAME host logic -- compaction, GroupNorm-beta
# correction, gate plumbing, batched time / text projections, in-place skip-concats, depth lerp -- without any rounding and
# compare it with the fp32 oracle at 1e-5 (tests/test_host_logic.py); the kernels themselves refuse anything but bf16.
ACT_DTYPE = torch.bfloat16


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _check_act(x: torch.Tensor, name: str):
    # bf16 is the product's activation format; fp32 tensors take the fp32 PARITY instantiations of the kernels (io_f32 of the
    # parameter blocks: same code paths on exact-fp32 arithmetic, tests/test_fp32_parity_gpu.py; never benchmarked)
    if x.dtype not in (torch.bfloat16, torch.float32) or x.dim() != 4 or x.stride(3) != 1 or not x.is_cuda:
        raise ValueError(f"{name}: expected a CUDA bf16 (or, parity path, fp32) [B,H,W,C] tensor with contiguous channels, got "
                         f"{x.dtype} {tuple(x.shape)} strides {x.stride()}")
    B, H, W, C = x.shape
    ld = _ld(x)
    if (W > 1 and x.stride(2) != ld) or (H > 1 and x.stride(1) != W * ld) or (B > 1 and x.stride(0) != H * W * ld):
        raise ValueError(f"{name}: rows must be uniformly strided (ld={ld}), got strides {x.stride()}")
    if ld % 8 != 0 or x.data_ptr() % 16 != 0:
        raise ValueError(f"{name}: pixel stride {ld} must be a multiple of 8 elements and the base 16-byte aligned")
    return ld


def _ld(x: torch.Tensor) -> int:
    # pixel stride of a [B,H,W,C] view (robust to size-1 dims)
    B, H, W, C = x.shape
    if W > 1:
        return x.stride(2)
    if H > 1:
        return x.stride(1)
    if B > 1:
        return x.stride(0)
    return max(x.stride(2), C)


def _set_views(p, **views):
    """fill the pointer / batch stride / row stride fields ``<name>``, ``<name>_stride_b``, ``<name>_stride_l`` of a params
    struct from [B, L, C] views"""
    for name, t in views.items():
        setattr(p, name, t.data_ptr())
        setattr(p, name + "_stride_b", t.stride(0))
        setattr(p, name + "_stride_l", t.stride(1))


@dataclass
class PackedWeight:
    """bf16 weights in the kernel's [N][taps][cin_pad] layout + fp32 bias (both already gathered/compacted)."""
    w: torch.Tensor            # bf16 [N, KH*KW, cin_pad]
    bias: Optional[torch.Tensor]  # fp32 [N] or None
    N: int
    Cin: int
    KH: int
    KW: int
    geglu: bool = False
    ln_colsum: Optional[torch.Tensor] = None   # fp32 [N]: row sums of the bf16 weights when a LayerNorm is folded in
    Cin2: int = 0                              # second-operand K-segment (pack_weight_cat): channels, padded channels
    cin2_pad: int = 0
    cin_pad_: int = 0                          # cin_pad of the main segment when w is the flat [N, 1, Ktot] of a cat pack

    @property
    def cin_pad(self) -> int:
        return self.cin_pad_ or self.w.shape[2]


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def pack_weight(w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, out_idx: Optional[torch.Tensor] = None,
                in_idx: Optional[torch.Tensor] = None, n_pad_to: int = 8, cin_pad_to: int = 8,
                geglu: bool = False, device=None, ln_gamma: Optional[torch.Tensor] = None,
                ln_beta: Optional[torch.Tensor] = None) -> PackedWeight:
    """Pack an OIHW conv weight (or [out,in] linear weight) for aptp_conv_gemm.

    out_idx / in_idx: live output / input channel indices (architecture-code compaction; the reference's
    prune() slicing, blocks.py:436-463, 159-177, 55-64, 126).  Output rows and input columns are zero-padded to
    multiples of n_pad_to / cin_pad_to (pad rows produce exact zeros), then Cin to a multiple of 64.
    geglu: interleave the two halves of a GEGLU projection in [16 value | 16 gate] row blocks so the epilogue finds
    h and g of one hidden unit in the same lane.
    ln_gamma / ln_beta: fold the LayerNorm that precedes this linear layer into it (include/aptp_hip.h, ln_stats):
    w' = w * gamma, bias' = bias + w @ beta; PackedWeight.ln_colsum = row sums of the bf16-rounded w'."""
    if w.dim() == 2:
        w = w[:, :, None, None]
    device = device or w.device
    w = w.to(device=device, dtype=torch.float32)
    if bias is not None:
        bias = bias.to(device=device, dtype=torch.float32)
    if ln_gamma is not None:
        assert w.shape[2] == 1 and w.shape[3] == 1 and in_idx is None, "a LayerNorm folds into a linear layer over all its channels"
        ga = ln_gamma.to(device=device, dtype=torch.float32)
        be = ln_beta.to(device=device, dtype=torch.float32)
        shift = w[:, :, 0, 0] @ be
        bias = shift if bias is None else bias + shift
        w = w * ga[None, :, None, None]
    if geglu:
        inner = w.shape[0] // 2
        wh, wg = w[:inner], w[inner:]
        bh, bg = (bias[:inner], bias[inner:]) if bias is not None else (None, None)
        if out_idx is not None:
            out_idx = out_idx.to(device)
            wh, wg = wh[out_idx], wg[out_idx]
            if bias is not None:
                bh, bg = bh[out_idx], bg[out_idx]
        if in_idx is not None:
            in_idx = in_idx.to(device)
            wh, wg = wh[:, in_idx], wg[:, in_idx]
        n_live = wh.shape[0]
        n_p = round_up(n_live, 16)

        def padrows(t):
            if t.shape[0] == n_p:
                return t
            return torch.cat([t, t.new_zeros((n_p - t.shape[0],) + tuple(t.shape[1:]))], 0)
        wh, wg = padrows(wh), padrows(wg)
        # [n_p/16, 16, ...] blocks interleaved
        w = torch.stack([wh.reshape(n_p // 16, 16, *wh.shape[1:]), wg.reshape(n_p // 16, 16, *wg.shape[1:])], 1)
        w = w.reshape(2 * n_p, *wh.shape[1:])
        if bias is not None:
            bh, bg = padrows(bh), padrows(bg)
            bias = torch.stack([bh.reshape(n_p // 16, 16), bg.reshape(n_p // 16, 16)], 1).reshape(2 * n_p)
    else:
        if out_idx is not None:
            out_idx = out_idx.to(device)
            w = w[out_idx]
            if bias is not None:
                bias = bias[out_idx]
        if in_idx is not None:
            w = w[:, in_idx.to(device)]
        n_live = w.shape[0]
        n_p = round_up(n_live, n_pad_to)
        if n_p != n_live:
            w = torch.cat([w, w.new_zeros((n_p - n_live,) + tuple(w.shape[1:]))], 0)
            if bias is not None:
                bias = torch.cat([bias, bias.new_zeros(n_p - n_live)], 0)
    N, Cin, KH, KW = w.shape
    cin_live = round_up(Cin, cin_pad_to)
    cin_pad = round_up(cin_live, BK)
    packed = torch.zeros(N, KH * KW, cin_pad, dtype=ACT_DTYPE, device=device)
    packed[:, :, :Cin] = w.permute(0, 2, 3, 1).reshape(N, KH * KW, Cin).to(ACT_DTYPE)
    colsum = packed.float().sum(dim=(1, 2)).contiguous() if ln_gamma is not None else None
    return PackedWeight(packed.contiguous(), None if bias is None else bias.contiguous(), N, cin_live, KH, KW, geglu, colsum)


def pack_weight_cat(pw: PackedWeight, w2: torch.Tensor, bias2: Optional[torch.Tensor] = None, *,
                    in_idx: Optional[torch.Tensor] = None) -> PackedWeight:
    """Append a second-operand K-segment (include/aptp_hip.h, x2) to packed conv weights: w2 [N_logical, Cin2] is the 1x1
    convolution applied to x2 at the output pixel (the resnet's conv_shortcut fused into conv2), bias2 is added to the
    bias.  Rows follow pw's rows (w2 is zero-padded to pw.N rows)."""
    assert not pw.geglu and pw.ln_colsum is None and pw.Cin2 == 0
    dev = pw.w.device
    w2 = w2.to(device=dev, dtype=torch.float32).reshape(w2.shape[0], -1)
    if in_idx is not None:
        w2 = w2[:, in_idx.to(dev)]
    n_live, c2 = w2.shape
    assert n_live <= pw.N
    c2_live = round_up(c2, 8)
    c2_pad = round_up(c2_live, BK)
    ext = torch.zeros(pw.N, c2_pad, dtype=ACT_DTYPE, device=dev)
    ext[:n_live, :c2] = w2.to(ACT_DTYPE)
    flat = torch.cat([pw.w.reshape(pw.N, -1), ext], 1).reshape(pw.N, 1, -1).contiguous()
    bias = pw.bias
    if bias2 is not None:
        b2 = torch.zeros(pw.N, dtype=torch.float32, device=dev)
        b2[:n_live] = bias2.to(device=dev, dtype=torch.float32)
        bias = b2 if bias is None else bias + b2
    return PackedWeight(flat, bias, pw.N, pw.Cin, pw.KH, pw.KW, False, None, c2_live, c2_pad, pw.cin_pad)


# Optional launch recorder used by bench.py's roofline leg: when a list, every aptp_conv_gemm launch appends
# {"params": ConvGemmParams, "flops": algorithmic FLOPs, "keep": tensors referenced by the params}.
LAUNCH_LOG = None
# Same for aptp_groupnorm calls (bench.py's HBM roofline leg): {"params", "bytes": x read once + y written once, "keep"}
GN_LAUNCH_LOG = None
ATTN_LAUNCH_LOG = None      # bench.py: the attention launches of ONE forward (re-timed for roofline_attention)

# Split-K launches combine their K-slices inside the kernel (AptpConvGemmParams.tile_counters) instead of launching
# splitk_reduce_kernel; False restores the two-launch form (A/B timing, tests of both forms)
SPLITK_IN_KERNEL = True

# Launch scratch -- the split-K arrival counters, the grow-only workspaces, the unit-statistics arena of a forward and the
# domain that keeps concurrently replaying graphs apart -- lives in scratch.py; these are the same objects under the names the
# models, tools and tests use.
scratch_domain, _domain = scratch.scratch_domain, scratch.domain
_tile_counters, _N_COUNTERS = scratch.counters, scratch.N_COUNTERS
_workspace, _ws_capture_keep = scratch.workspace, scratch.capture_keep
ustat_begin, ustat_end, _ustat_alloc = scratch.ustat_begin, scratch.ustat_end, scratch.ustat_alloc
USTAT, USTAT_NREP = scratch.USTAT, scratch.USTAT_NREP

# AptpGroupNormParams.variant used when the caller asks for "auto" (0).  0 = the library's own choice (small maps in one
# launch, large maps in three).  3 (large maps in two launches: <= 16 coarse statistics chunks folded by the apply
# workgroups) measured much SLOWER on MI355X (149.5 vs 167.4 steps/s: 64 statistics workgroups cannot stream a level-64
# map fast enough), so it stays opt-in.
GN_DEFAULT_VARIANT = 0
GN_STATS_ONE_LAUNCH = True     # keep_stats on the small maps through the one-launch kernel (False: always three launches; A/B, tests)

# AptpAttentionParams.variant for every launch (1 = staggered wave groups: A/B timing, tests of both forms)
ATTN_VARIANT = int(os.environ.get("APTP_ATTN_VARIANT", "0"))      # AptpAttentionParams.variant: 0 = the library chooses (A/B timing, tests)

# GroupNorm on the large maps: True lets the last statistics workgroup of a sample finalise mean / rstd (two launches
# instead of three).  Measured SLOWER on MI355X (162.5 vs 164.7 steps/s: 128 tickets on one counter + the acquire cost
# more than the 5.5 us launch they replace), so it is off; kept for tests and as a measured negative result.
GN_FUSED_FINALIZE = False

# AptpConvGemmParams.epilogue for every launch: 0 = auto (coalesced epilogue where alignment allows), 1 = force the
# accumulator-layout epilogue (A/B timing, tests of both forms)
EPILOGUE = 0


# GroupNorm statistics emitted by the GEMM that produces a tensor (AptpConvGemmParams.colstat_out) travel with the
# tensor: they are recorded on its root storage owner (the tensor itself, or the concat buffer it is a channel slice of)
# under the view's storage offset, so the consumer finds them through any permute / reshape view, and the two halves of
# a skip-concat buffer keep separate records.  COLSTATS_MIN_HW: only maps large enough for GroupNorm's multi-launch form.
COLSTATS = True
COLSTATS_MIN_HW = 1024


def _root(t: torch.Tensor) -> torch.Tensor:
    return t._base if t._base is not None else t


def _colstats_drop(out: torch.Tensor):
    d = getattr(_root(out), "_aptp_colstats", None)
    if d:
        d.pop(out.storage_offset(), None)


def _colstats_put(out: torch.Tensor, stats: torch.Tensor, rows_per_block: int, ustat=None):
    root = _root(out)
    d = getattr(root, "_aptp_colstats", None)
    if d is None:
        d = {}
        root._aptp_colstats = d
    d[out.storage_offset()] = (stats, rows_per_block, out.shape[3], (out.shape[0], out.shape[1] * out.shape[2]), _ld(out), ustat)


def _colstats_get(x: torch.Tensor, C: int):
    """producer statistics covering the NHWC view x (C real channels, the rest zero padding): one record, or two adjacent
    ones (skip-concat); returns [(stats, rows_per_block, channels used), ...] or None"""
    d = getattr(_root(x), "_aptp_colstats", None)
    if not d:
        return None
    segs, off, left, pad = [], x.storage_offset(), x.shape[3], x.shape[3] - C
    while left > 0 and len(segs) < 2:
        rec = d.get(off)
        if rec is None or rec[3] != (x.shape[0], x.shape[1] * x.shape[2]) or rec[4] != _ld(x) or rec[2] > left:
            return None
        segs.append([rec[0], rec[1], rec[2], rec[5] if len(rec) > 5 else None])
        off += rec[2]
        left -= rec[2]
    if left != 0 or segs[-1][2] <= pad:
        return None
    segs[-1][2] -= pad
    return segs


class _PrefetchPlan:
    """Order in which one forward reads its packed weights.  The first forward records it; later forwards hand launch i
    the weights of launch i+1 as AptpConvGemmParams.prefetch.  A forward whose order differs from the recorded one
    (another batch of expert masks, other packs) re-records from the point of divergence.
    (Tried and dropped: the same hook in the GroupNorm launch that sits between two convolutions, as eight extra
    prefetch-only workgroups per sample -- 183.7-184.5 vs 184.8 steps/s without it.)"""

    def __init__(self):
        self.seq = []
        self.i = 0

    def begin(self):
        self.i = 0

    def step(self, w):
        i, self.i = self.i, self.i + 1
        if i < len(self.seq) and self.seq[i] is w:
            nxt = self.seq[i + 1] if i + 1 < len(self.seq) else None
        else:
            del self.seq[i:]
            self.seq.append(w)
            nxt = None
        if nxt is not None and not (PREFETCH_MIN_BYTES <= nxt.numel() * nxt.element_size() <= PREFETCH_MAX_BYTES):
            return None
        return nxt


# The plan of the forward in progress is per THREAD (a model installs its own at the top of forward(), see unet.py):
# forwards issued from different host threads -- e.g. one per stream -- never see each other's launch order.
_tls = threading.local()


def set_prefetch_plan(plan: Optional[_PrefetchPlan]):
    _tls.prefetch_plan = plan
    if plan is not None:
        plan.begin()


def _current_prefetch_plan() -> Optional[_PrefetchPlan]:
    return getattr(_tls, "prefetch_plan", None)


# Next-launch weight prefetch (AptpConvGemmParams.prefetch): on for weights that fit the XCD L2s next to the running
# launch's own traffic (<= 12 MB: +1.5 % on the headline forward; all sizes +0.5 %; off: APTP_PREFETCH=0)
PREFETCH_WEIGHTS = os.environ.get("APTP_PREFETCH", "1") == "1"
PREFETCH_MIN_BYTES = int(os.environ.get("APTP_PREFETCH_MIN", "0"))
PREFETCH_MAX_BYTES = int(os.environ.get("APTP_PREFETCH_MAX", str(12 << 20)))


def conv_gemm(x: torch.Tensor, pw: PackedWeight, *, stride: int = 1, pad: Optional[int] = None, ups: int = 0,
              out: Optional[torch.Tensor] = None, rowbias: Optional[torch.Tensor] = None,
              colgate: Optional[torch.Tensor] = None, gate_group: int = 0, act: int = ACT_NONE,
              corr: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
              depth: Optional[torch.Tensor] = None, depth_in: Optional[torch.Tensor] = None,
              out_f32: bool = False, split_k: Optional[int] = None, tile: int = 0, order: int = 0,
              rowstats: bool = False, ln=None, colstats: bool = False, x2: Optional[torch.Tensor] = None,
              prefetch=None, gn=None, pad_end: int = 0):
    """y = epilogue(conv(x, w)); see include/aptp_hip.h for the epilogue order and the reference call sites.
    pad_end: extra zero rows / columns after the input's last ones (diffusers Downsample2D with padding 0:
    F.pad(x, (0, 1, 0, 1)) then a stride-2, pad-0 convolution is stride=2, pad=0, pad_end=1).
    gn = (gamma, beta, groups, eps, silu, C): return GroupNorm(+SiLU) of the convolution output over its first C channels
    instead of the output itself.  On the small maps, where the launch is split along K anyway, the reduce launch of the
    split applies the normalisation (AptpConvGemmParams.gn_gamma: one launch and one round trip less); otherwise this is
    conv_gemm followed by ops.groupnorm.
    rowstats: also emit the per-row (sum, sumsq) partials of y a following folded LayerNorm needs; returns (y, stats)
    with stats fp32 [slots / 2, M, 4] (two (sum, sumsq) slots per element), or (y, None) when this launch is split along K (the caller then normalises with
    ops.layernorm).  ln = (stats, eps): x is the un-normalised input of a LayerNorm folded into pw (pack_weight ln_gamma)."""
    if pad_end < 0 or (pad_end and (ups or corr is not None or x2 is not None)):
        raise ValueError("conv_gemm: pad_end must be >= 0 and does not go with ups, corr or x2")
    lib = _lib.load()
    if gn is not None and (colgate is not None or act != ACT_NONE or pw.geglu or corr is not None or residual is not None
                           or depth is not None or out_f32 or rowstats or ln is not None or out is not None):
        raise ValueError("conv_gemm: gn= goes with a plain bf16 convolution (bias / rowbias only)")
    _check_act(x, "conv_gemm x")
    B, Hin, Win, Cx = x.shape
    if Cx != pw.Cin:
        raise ValueError(f"conv_gemm: x has {Cx} channels, packed weight expects {pw.Cin}")
    if pad is None:
        pad = pw.KH // 2
    sh = 1 if ups else 0            # ups 1 = nearest x2, ups 2 = zero-insertion x2 (dgrad of a stride-2 conv)
    HinE, WinE = Hin << sh, Win << sh
    Hout = (HinE + 2 * pad + pad_end - pw.KH) // stride + 1
    Wout = (WinE + 2 * pad + pad_end - pw.KW) // stride + 1
    if pw.geglu:
        act = ACT_GEGLU
    nout = pw.N // 2 if act == ACT_GEGLU else pw.N
    f32 = x.dtype == torch.float32                # fp32 parity instantiation: every tensor operand fp32, tiles 1..6, no tables
    gn_f32 = None
    if f32:
        if pw.w.dtype != torch.float32:
            raise ValueError("conv_gemm: fp32 activations need weights packed under ops.ACT_DTYPE = torch.float32")
        out_f32, colstats, prefetch, gn_f32, gn = True, False, False, gn, None
        if tile not in (0, 1, 2, 3, 4, 5, 6):
            raise ValueError("conv_gemm: the fp32 parity path runs on the register-staged tiles 1..6")
    if out is None:
        out = torch.empty(B, Hout, Wout, nout, dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    else:
        _colstats_drop(out)          # whatever statistics were recorded for this memory describe its old contents
        if tuple(out.shape) != (B, Hout, Wout, nout) or out.stride(3) != 1:
            raise ValueError(f"conv_gemm: out shape {tuple(out.shape)} != {(B, Hout, Wout, nout)}")
        if out.dtype != (torch.float32 if out_f32 else torch.bfloat16):
            raise ValueError("conv_gemm: out dtype mismatch")
    p = ConvGemmParams()
    p.x, p.ldx = x.data_ptr(), _ld(x)
    p.B, p.Hin, p.Win, p.Cin, p.Hout, p.Wout = B, Hin, Win, Cx, Hout, Wout
    p.KH, p.KW, p.stride, p.pad, p.ups = pw.KH, pw.KW, stride, pad, ups
    p.pad_end = pad_end
    p.w, p.N, p.cin_pad = pw.w.data_ptr(), pw.N, pw.cin_pad
    if (x2 is not None) != (pw.Cin2 > 0):
        raise ValueError("conv_gemm: x2 goes with weights packed by pack_weight_cat (and only with them)")
    if x2 is not None:
        _check_act(x2, "conv_gemm x2")
        if tuple(x2.shape) != (B, Hout, Wout, pw.Cin2):
            raise ValueError(f"conv_gemm: x2 shape {tuple(x2.shape)} != {(B, Hout, Wout, pw.Cin2)}")
        p.x2, p.ldx2, p.Cin2, p.cin2_pad = x2.data_ptr(), _ld(x2), pw.Cin2, pw.cin2_pad
    p.bias = None if pw.bias is None else pw.bias.data_ptr()
    if rowbias is not None:
        assert rowbias.dtype == torch.float32 and rowbias.dim() == 2 and rowbias.shape[0] == B and rowbias.stride(1) == 1
        assert rowbias.shape[1] >= pw.N
        p.rowbias, p.ld_rowbias = rowbias.data_ptr(), rowbias.stride(0)
    if colgate is not None:
        assert colgate.dtype == torch.float32 and colgate.dim() == 2 and colgate.is_contiguous()
        assert gate_group > 0 and colgate.shape[1] * gate_group == nout and B % colgate.shape[0] == 0
        p.colgate, p.gate_group, p.gate_B = colgate.data_ptr(), gate_group, colgate.shape[0]
    p.act = act
    if corr is not None:
        assert corr.dtype == torch.float32 and corr.is_contiguous() and corr.shape[1:] == (9, nout)
        assert B % corr.shape[0] == 0
        p.corr, p.corr_B = corr.data_ptr(), corr.shape[0]
    if residual is not None:
        _check_act(residual, "conv_gemm residual")
        assert tuple(residual.shape) == (B, Hout, Wout, nout)
        p.residual, p.ldres = residual.data_ptr(), _ld(residual)
    if depth is not None:
        assert depth.dtype == torch.float32 and depth.dim() == 1 and B % depth.shape[0] == 0 and depth_in is not None
        _check_act(depth_in, "conv_gemm depth_in")
        assert tuple(depth_in.shape) == (B, Hout, Wout, nout)
        p.depth, p.depth_B = depth.data_ptr(), depth.shape[0]
        p.depth_in, p.lddin = depth_in.data_ptr(), _ld(depth_in)
    p.y, p.ldy, p.out_f32 = out.data_ptr(), _ld(out), int(out_f32)
    p.epilogue = EPILOGUE
    p.io_f32 = int(f32)
    if f32:
        for t_, nm in ((x2, "x2"), (residual, "residual"), (depth_in, "depth_in")):
            if t_ is not None and t_.dtype != torch.float32:
                raise ValueError(f"conv_gemm: fp32 parity path: {nm} must be fp32 too")
    if prefetch is False:             # the "weights" of this launch are a temporary (conv_wgrad): not part of any plan
        prefetch = None
    elif PREFETCH_WEIGHTS and prefetch is None:
        plan = _current_prefetch_plan()
        if plan is not None:
            prefetch = plan.step(pw.w)
    if prefetch is not None:
        p.prefetch, p.prefetch_bytes = prefetch.data_ptr(), prefetch.numel() * prefetch.element_size()
    # a plain linear layer the lean kernel can take (csrc/lin_gemm.hip, aptp_lin_eligible)
    plain_linear = pw.KH == 1 and pw.KW == 1 and stride == 1 and not ups and x2 is None and colgate is None and corr is None \
        and rowbias is None and depth is None and not out_f32 and gn is None and (act != ACT_GEGLU or (residual is None and not rowstats))
    p.split_k = 1
    p.tile, sk, in_kernel, p.order = choose_launch(B * Hout * Wout, pw.N, Cx, pw.cin_pad, pw.KH, pw.KW, stride, ups, act, pw.Cin2, pw.cin2_pad,
                                                   plain_linear=plain_linear, f32=f32, tile=tile, split_k=split_k, order=order)
    p.split_k = max(1, int(lib.aptp_conv_gemm_suggest_split_k(ctypes.byref(p)) if sk is None else sk))
    ws = cnt = None
    gn_fused = False
    if gn is not None and FUSE_GN_REDUCE and p.split_k > 1 and Hout * Wout <= GN_REDUCE_MAX_HW:
        gamma, beta, groups, eps_, silu_, Cn = gn
        cgn = Cn // groups
        gn_fused = Cn % 8 == 0 and Cn % groups == 0 and cgn % 4 == 0 and Hout * Wout * cgn <= 4 * 24 * 256 and Cn <= nout
    if gn_fused:                           # the K-slices are combined by the reduce launch, which also normalises
        colstats = False
        p.gn_gamma, p.gn_beta, p.gn_groups, p.gn_C, p.gn_silu, p.gn_eps = gamma.data_ptr(), beta.data_ptr(), groups, Cn, int(silu_), eps_
    # column statistics this launch would want to emit (whether it can is decided below, once the split-K form is known)
    want_cols = colstats and COLSTATS and Hout * Wout >= COLSTATS_MIN_HW and act != ACT_GEGLU and not out_f32
    if p.split_k > 1:
        in_kernel = splitk_in_kernel(p.split_k, in_kernel, explicit=split_k is not None, reduce_launch=gn_fused, rowstats=rowstats, colstats=want_cols)
        sk_tile = p.tile >= SK_TILE_FIRST     # persistent stream-K tiles: partial tiles are always combined in-kernel
        if (SPLITK_IN_KERNEL or sk_tile) and (in_kernel or sk_tile) and lib.aptp_conv_gemm_tiles(ctypes.byref(p)) <= _N_COUNTERS:
            cnt = _tile_counters(x.device)
            if cnt is not None:
                p.tile_counters = cnt.data_ptr()
        if sk_tile and cnt is None:
            p.split_k = 1                     # no counters at hand (a new key under capture and no free slab): whole tiles only
        else:
            ws = _workspace(lib.aptp_conv_gemm_workspace_bytes(ctypes.byref(p)), x.device)
            p.workspace = ws.data_ptr()
    stats = None
    if rowstats and (p.split_k == 1 or cnt is not None):
        slots = lib.aptp_conv_gemm_rowstat_slots(ctypes.byref(p))
        assert slots % 2 == 0
        stats = torch.empty(slots // 2, B * Hout * Wout, 4, dtype=torch.float32, device=x.device)
        p.rowstat_out, p.rowstat_slots = stats.data_ptr(), slots
    cstats = ustat = None
    if want_cols and (p.split_k == 1 or cnt is not None) and _ld(out) % 8 == 0 and out.data_ptr() % 16 == 0 and nout % 8 == 0 \
            and (residual is None or (_ld(residual) % 8 == 0 and residual.data_ptr() % 16 == 0)) \
            and (depth_in is None or (_ld(depth_in) % 8 == 0 and depth_in.data_ptr() % 16 == 0)) and p.epilogue == 0:
        rpb = lib.aptp_conv_gemm_colstat_rows(ctypes.byref(p))
        if rpb > 0 and (Hout * Wout) % rpb == 0:
            M = B * Hout * Wout
            nblk = (M + rpb - 1) // rpb + 16          # (+ the padding blocks of the last, partial tile)
            cstats = torch.empty(nblk, nout, 2, dtype=torch.float32, device=x.device)
            p.colstat_out, p.colstat_ld = cstats.data_ptr(), nout
            ustat = _ustat_alloc(B, nout)
            if ustat is not None:
                p.ustat_out, p.ustat_unit, p.ustat_units, p.ustat_nrep = ustat[0].data_ptr(), ustat[1], ustat[2], ustat[3]
    if ln is not None:
        ln_stats, ln_eps = ln
        if pw.ln_colsum is None:
            raise ValueError("conv_gemm: ln= needs weights packed with ln_gamma / ln_beta")
        assert ln_stats.dtype == torch.float32 and ln_stats.is_contiguous() and ln_stats.shape[1] == B * Hout * Wout \
            and ln_stats.shape[2] == 4
        p.ln_stats, p.ln_slots, p.ln_colsum = ln_stats.data_ptr(), 2 * ln_stats.shape[0], pw.ln_colsum.data_ptr()
        p.ln_eps, p.ln_C = ln_eps, Cx
    elif pw.ln_colsum is not None:
        raise ValueError("conv_gemm: weights with a folded LayerNorm need ln=(stats, eps)")
    _lib.check(lib.aptp_conv_gemm(ctypes.byref(p), _stream()), "aptp_conv_gemm")
    if cstats is not None:
        _colstats_put(out, cstats, rpb, ustat)
    if LAUNCH_LOG is not None:
        LAUNCH_LOG.append({"params": p, "flops": 2.0 * B * Hout * Wout * pw.N * (pw.KH * pw.KW * pw.Cin + pw.Cin2),
                           "keep": (x, pw, out, rowbias, colgate, corr, residual, depth, depth_in, ws, stats, ln, cnt, cstats, x2, gn, ustat)})
    if f32 and gn_f32 is not None:
        gn = gn_f32
    if gn is not None and not gn_fused:
        gamma, beta, groups, eps_, silu_, Cn = gn
        return groupnorm(out, gamma, beta, groups, eps_, silu_, C=Cn)
    return (out, stats) if rowstats else out


def linear(x: torch.Tensor, pw: PackedWeight, **kw) -> torch.Tensor:
    """x [B, L, C] -> [B, L, N] through the 1x1 path (tokens = H, W = 1)."""
    B, L, C = x.shape
    out = kw.pop("out", None)
    for k in ("residual", "depth_in"):
        if kw.get(k) is not None:
            kw[k] = kw[k].unsqueeze(2)
    y = conv_gemm(x.unsqueeze(2), pw, pad=0, out=None if out is None else out.unsqueeze(2), **kw)
    if "rowstats" in kw:
        return (y[0].squeeze(2), y[1]) if kw["rowstats"] else (y.squeeze(2), None)
    return y.squeeze(2)


def groupnorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, silu: bool,
              C: Optional[int] = None, out: Optional[torch.Tensor] = None, keep_stats: bool = False, variant: int = 0):
    """GroupNorm(+SiLU) of a [B,H,W,Cp] tensor over its first C real channels (Cp = roundup8(C)).
    keep_stats: also return the fp32 [B, nchunk, groups, 2] statistics partials (needed by groupnorm_bwd; variant 4: one
    launch on the small maps, three elsewhere).  variant: see AptpGroupNormParams in include/aptp_hip.h."""
    lib = _lib.load()
    _check_act(x, "groupnorm x")
    B, H, W, Cp = x.shape
    C = Cp if C is None else C
    assert Cp == round_up(C, 8), f"groupnorm: tensor width {Cp} != roundup8({C})"
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == C and beta.numel() == C
    if out is None:
        out = torch.empty(B, H, W, Cp, dtype=x.dtype, device=x.device)
    p = GroupNormParams()
    p.x, p.ldx, p.y, p.ldy = x.data_ptr(), _ld(x), out.data_ptr(), _ld(out)
    p.B, p.HW, p.C, p.groups = B, H * W, C, groups
    p.gamma, p.beta, p.eps, p.silu = gamma.data_ptr(), beta.data_ptr(), eps, int(silu)
    if x.dtype == torch.float32:          # fp32 parity path (csrc/parity_f32.hip): three plain launches, no producer statistics
        assert out.dtype == torch.float32 and not keep_stats
        p.io_f32, p.variant = 1, 1
        ws = _workspace(lib.aptp_groupnorm_workspace_bytes(ctypes.byref(p)), x.device)
        p.workspace = ws.data_ptr()
        _lib.check(lib.aptp_groupnorm(ctypes.byref(p), _stream()), "aptp_groupnorm(io_f32)")
        return out
    if keep_stats:
        # [B, nchunk + 1, G, 2]: the partials the backward needs, plus the finalised (mean, rstd) slot the kernels append
        nch = lib.aptp_groupnorm_nchunk(H * W)
        ws_full = torch.empty(B * (nch + 1) * groups * 2, dtype=torch.float32, device=x.device)
        ws = ws_full[:B * nch * groups * 2].view(B, nch, groups, 2)
        p.workspace = ws_full.data_ptr()
        p.variant = 4 if GN_STATS_ONE_LAUNCH else 1
        _lib.check(lib.aptp_groupnorm(ctypes.byref(p), _stream()), "aptp_groupnorm")
        return out, ws
    else:
        ws = _workspace(lib.aptp_groupnorm_workspace_bytes(ctypes.byref(p)), x.device)
    p.variant = variant if variant else GN_DEFAULT_VARIANT
    p.workspace = ws.data_ptr()
    segs = _colstats_get(x, C) if (COLSTATS and variant == 0 and H * W >= COLSTATS_MIN_HW) else None
    if segs is not None:
        for i, (st, rpb, cseg, us) in enumerate(segs):
            p.colstats[i].stats, p.colstats[i].ld, p.colstats[i].rows_per_block, p.colstats[i].C = st.data_ptr(), st.shape[1], rpb, cseg
            if us is not None and us[0].shape[0] == us[3] * B * us[2] * 2:
                p.colstats[i].ustats, p.colstats[i].unit, p.colstats[i].units, p.colstats[i].nrep = us[0].data_ptr(), us[1], us[2], us[3]
        p.variant = 1                       # the multi-launch skeleton (statistics pass replaced by the finalise)
    cnt = _tile_counters(x.device) if (GN_FUSED_FINALIZE and B <= _N_COUNTERS) else None
    if cnt is not None:
        p.counters = cnt.data_ptr()
    _lib.check(lib.aptp_groupnorm(ctypes.byref(p), _stream()), "aptp_groupnorm")
    if GN_LAUNCH_LOG is not None:
        GN_LAUNCH_LOG.append({"params": p, "bytes": 2.0 * B * H * W * (C + Cp), "keep": (x, out, gamma, beta, ws, segs, cnt)})
    return (out, ws) if keep_stats else out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm over the last dim of a bf16 [B, L, C] tensor."""
    lib = _lib.load()
    B, L, C = x.shape
    assert x.dtype in (torch.bfloat16, torch.float32) and x.stride(2) == 1 and x.is_cuda
    ld = x.stride(1) if L > 1 else max(x.stride(1), C)
    assert B == 1 or L == 1 or x.stride(0) == L * ld
    if out is None:
        out = torch.empty(B, L, C, dtype=x.dtype, device=x.device)
    p = LayerNormParams()
    p.io_f32 = int(x.dtype == torch.float32)      # fp32 parity path (csrc/parity_f32.hip)
    p.x, p.ldx, p.y, p.ldy = x.data_ptr(), ld, out.data_ptr(), out.stride(1) if L > 1 else C
    p.rows, p.C = B * L, C
    p.gamma, p.beta, p.eps = gamma.data_ptr(), beta.data_ptr(), eps
    _lib.check(lib.aptp_layernorm(ctypes.byref(p), _stream()), "aptp_layernorm")
    return out


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: Optional[float] = None,
              out: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(q k^T * scale) v with head_dim 64.  q [B, Lq, >=heads*64], k/v [B, Lk, >=heads*64] are bf16 views
    (e.g. column slices of a fused QKV buffer); heads are laid out as consecutive 64-wide column blocks."""
    lib = _lib.load()
    B, Lq = q.shape[0], q.shape[1]
    Lk = k.shape[1]
    for t in (q, k, v):
        assert t.dtype == q.dtype and t.dtype in (torch.bfloat16, torch.float32) and t.stride(2) == 1 and t.shape[2] == heads * 64 and t.is_cuda
    if out is None:
        out = torch.empty(B, Lq, heads * 64, dtype=q.dtype, device=q.device)
    p = AttentionParams()
    p.io_f32 = int(q.dtype == torch.float32)      # fp32 parity path (csrc/parity_f32.hip)
    _set_views(p, q=q, k=k, v=v, o=out)
    p.B, p.heads, p.Lq, p.Lk = B, heads, Lq, Lk
    p.scale = (1.0 / 8.0) if scale is None else scale
    p.variant = ATTN_VARIANT
    if lse is not None:
        assert lse.dtype == torch.float32 and lse.is_contiguous() and tuple(lse.shape) == (B, heads, Lq)
        p.lse = lse.data_ptr()
    if ATTN_LAUNCH_LOG is not None and not p.io_f32:
        ATTN_LAUNCH_LOG.append({"params": p, "flops": 4.0 * B * heads * Lq * Lk * 64, "keep": (q, k, v, out, lse), "Lk": Lk})
    _lib.check(lib.aptp_attention(ctypes.byref(p), _stream()), "aptp_attention")
    return out


# GroupNorm applied by the reduce launch of a split-K convolution (conv_gemm(gn=...)) on maps of at most this many pixels
# (SD-2.1 levels 16 and 8: norm2 + SiLU of the 12 resnets there).  Measured on MI355X: it TIES the separate launches
# (187.3-187.7 vs 187.6 steps/s; 327 instead of 339 kernels per step): only groups x B = 64 workgroups exist, and their
# 16 waves each stream the K-slices about as slowly as splitk_reduce_kernel on 256 CUs plus the single-launch GroupNorm take
# together (a 256-thread version lost 3.8 %).  Off by default; APTP_FUSE_GN_REDUCE=1 turns it on (A/B timing, tests).
FUSE_GN_REDUCE = os.environ.get("APTP_FUSE_GN_REDUCE", "0") != "0"
GN_REDUCE_MAX_HW = 256


# Fused transformer tail (aptp_ff_tail): LN3 -> GEGLU projection -> ff.net[2] + residual -> proj_out + residual as one kernel
# per 64-token tile.  Worth it only where a row tile per CU fills the chip and the activations, not the weights, are the
# bytes that matter: M >= FUSE_TAIL_MIN_ROWS (SD-2.1 level 64 at bs >= 4).  APTP_FUSE_TAIL=0 disables; APTP_FUSE_TAIL_MIN_ROWS
# moves the threshold (tests exercise the kernel on small maps).
# Round 4: OFF by default.  With the lean linear kernel (csrc/lin_gemm.hip) the three separate launches are faster than the
# fused tile (same-box A/B on the headline forward: 202.8 steps/s without, 201.6 with; round 2, against the general kernel, the
# fused tile won by 0.3-0.6 %): one workgroup per CU walks 40 dependent K-steps while the launches keep 3-5 workgroups per CU
# in different phases.  APTP_FUSE_TAIL=1 turns it back on (tests of the kernel, A/B timing); it still saves 0.8 GB of HBM
# traffic per step.
FUSE_TAIL = os.environ.get("APTP_FUSE_TAIL", "0") != "0"
FUSE_TAIL_MIN_ROWS = int(os.environ.get("APTP_FUSE_TAIL_MIN_ROWS", "16384"))


def ff_tail_supported(h: torch.Tensor, pw1: PackedWeight, pw2: PackedWeight, pw3: PackedWeight) -> bool:
    if not (FUSE_TAIL and h.is_cuda and h.dtype == torch.bfloat16 and pw1.geglu and pw1.ln_colsum is not None):
        return False
    B, L, C = h.shape
    if B * L < FUSE_TAIL_MIN_ROWS or pw2.N != C or pw3.N != C or pw2.bias is None or pw3.bias is None or pw1.bias is None:
        return False
    return bool(_lib.load().aptp_ff_tail_supported(B * L, C, pw1.N, pw1.cin_pad, pw2.cin_pad, pw3.cin_pad))


def ff_tail(h: torch.Tensor, x: torch.Tensor, pw1: PackedWeight, pw2: PackedWeight, pw3: PackedWeight, eps: float = 1e-5,
            out: Optional[torch.Tensor] = None, colstats: bool = False) -> torch.Tensor:
    """y = proj_out(h + ff2(GEGLU(LN(h) W1'))) + x on token tensors [B, L, C] (bf16, contiguous channels, uniform row stride);
    pw1 = GEGLU projection packed with geglu=True and the LayerNorm folded in, pw2 = ff.net[2], pw3 = proj_out."""
    lib = _lib.load()
    B, L, C = h.shape
    for t, nm in ((h, "h"), (x, "x")):
        assert t.dtype == torch.bfloat16 and t.is_cuda and tuple(t.shape) == (B, L, C) and t.stride(2) == 1, nm
    if out is None:
        out = torch.empty(B, L, C, dtype=torch.bfloat16, device=h.device)
    else:
        _colstats_drop(out.unsqueeze(2))
    assert tuple(out.shape) == (B, L, C) and out.dtype == torch.bfloat16 and out.stride(2) == 1
    p = FfTailParams()
    for name, t in (("h", h), ("x", x), ("y", out)):
        _, _, _, ld = _rows(t)
        assert B == 1 or t.stride(0) == L * ld, "rows must be uniformly strided"
        setattr(p, name, t.data_ptr())
        setattr(p, "ld" + name, ld)
    p.w1, p.b1, p.cs1, p.n1, p.ld1 = pw1.w.data_ptr(), pw1.bias.data_ptr(), pw1.ln_colsum.data_ptr(), pw1.N, pw1.cin_pad
    p.w2, p.b2, p.ld2 = pw2.w.data_ptr(), pw2.bias.data_ptr(), pw2.cin_pad
    p.w3, p.b3, p.ld3 = pw3.w.data_ptr(), pw3.bias.data_ptr(), pw3.cin_pad
    p.M, p.C, p.eps = B * L, C, eps
    cstats = None
    if colstats and COLSTATS and L >= COLSTATS_MIN_HW and L % 64 == 0:
        cstats = torch.empty(B * L // 64, C, 2, dtype=torch.float32, device=h.device)
        p.colstat, p.colstat_ld = cstats.data_ptr(), C
    _lib.check(lib.aptp_ff_tail(ctypes.byref(p), _stream()), "aptp_ff_tail")
    if cstats is not None:
        _colstats_put(out.unsqueeze(2), cstats, 64)
    if LAUNCH_LOG is not None:       # same contraction work as the three aptp_conv_gemm launches it replaces: part of the family
        LAUNCH_LOG.append({"params": p, "fn": "aptp_ff_tail", "flops": 2.0 * B * L * (C * pw1.N + pw2.Cin * C + C * C),
                           "keep": (h, x, out, pw1, pw2, pw3, cstats)})
    return out


def unet_prologue(sample: torch.Tensor, timesteps: torch.Tensor, freqs: torch.Tensor, cin_pad: int):
    """sample [B,C,H,W] (fp32 / bf16, NCHW contiguous) -> (x bf16 [B,H,W,cin_pad] with zero padding channels,
    t_emb bf16 [B, 2*len(freqs)] = [cos | sin] of timesteps * freqs) in one launch (include/aptp_hip.h)."""
    lib = _lib.load()
    assert sample.is_cuda and sample.dim() == 4 and sample.dtype in (torch.float32, torch.bfloat16)
    sample = sample.contiguous()
    B, C, H, W = sample.shape
    t = timesteps.to(device=sample.device, dtype=torch.float32).contiguous()
    assert t.numel() == B and freqs.dtype == torch.float32 and freqs.is_contiguous()
    x = torch.empty(B, H, W, cin_pad, dtype=torch.bfloat16, device=sample.device)
    temb = torch.empty(B, 2 * freqs.numel(), dtype=torch.bfloat16, device=sample.device)
    p = UnetPrologueParams()
    p.sample, p.sample_bf16, p.x = sample.data_ptr(), int(sample.dtype == torch.bfloat16), x.data_ptr()
    p.B, p.C, p.H, p.W, p.cin_pad = B, C, H, W, cin_pad
    p.timesteps, p.freqs, p.half, p.t_emb = t.data_ptr(), freqs.data_ptr(), freqs.numel(), temb.data_ptr()
    _lib.check(lib.aptp_unet_prologue(ctypes.byref(p), _stream()), "aptp_unet_prologue")
    return x, temb


def unet_epilogue(y: torch.Tensor, channels: int, out_dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv_out's fp32 [B,H,W,ld] -> [B,channels,H,W] (fp32 or bf16) in one launch (into `out` when given: a contiguous
    tensor of that shape and dtype)."""
    lib = _lib.load()
    assert y.is_cuda and y.dtype == torch.float32 and y.dim() == 4 and y.is_contiguous() and out_dtype in (torch.float32, torch.bfloat16)
    B, H, W, ld = y.shape
    if out is None:
        out = torch.empty(B, channels, H, W, dtype=out_dtype, device=y.device)
    assert tuple(out.shape) == (B, channels, H, W) and out.dtype == out_dtype and out.is_contiguous() and out.is_cuda
    p = UnetEpilogueParams()
    p.y, p.ldy, p.out, p.out_bf16 = y.data_ptr(), ld, out.data_ptr(), int(out_dtype == torch.bfloat16)
    p.B, p.C, p.H, p.W = B, channels, H, W
    _lib.check(lib.aptp_unet_epilogue(ctypes.byref(p), _stream()), "aptp_unet_epilogue")
    return out


# ------------------------------------------------------------------------------------------------------------------
# model-I/O wrappers of the VAE and the text encoder
# ------------------------------------------------------------------------------------------------------------------
WIDE_HEAD = 512
ATTN_WIDE_LAUNCH_LOG = None     # tools/bench_vae.py: the wide-head attention launches of one decode (re-timed on their own)


def attention_wide(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: Optional[float] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(q k^T * scale) v with ONE head of width 512 (the VAE decoder's mid-block attention; default scale 512^-0.5).
    q [B, Lq, 512], k/v [B, Lk, 512] are bf16 (or, parity path, fp32) views with contiguous channels -- e.g. column slices
    of a fused q|k|v buffer; out [B, Lq, 512] is allocated unless given."""
    lib = _lib.load()
    B, Lq = q.shape[0], q.shape[1]
    Lk = k.shape[1]
    for t, nm in ((q, "q"), (k, "k"), (v, "v")):
        if t.dim() != 3 or t.dtype != q.dtype or t.dtype not in (torch.bfloat16, torch.float32) or t.stride(2) != 1 \
                or t.shape[2] != WIDE_HEAD or t.shape[0] != B or not t.is_cuda:
            raise ValueError(f"attention_wide: {nm} must be a CUDA bf16 (or fp32) [B, L, 512] view with contiguous channels, "
                             f"got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    if v.shape[1] != Lk:
        raise ValueError("attention_wide: k and v must have the same length")
    if out is None:
        out = torch.empty(B, Lq, WIDE_HEAD, dtype=q.dtype, device=q.device)
    if tuple(out.shape) != (B, Lq, WIDE_HEAD) or out.dtype != q.dtype or out.stride(2) != 1:
        raise ValueError("attention_wide: out must be [B, Lq, 512] of q's dtype with contiguous channels")
    p = AttentionWideParams()
    p.io_f32 = int(q.dtype == torch.float32)
    _set_views(p, q=q, k=k, v=v, o=out)
    p.B, p.Lq, p.Lk = B, Lq, Lk
    p.scale = WIDE_HEAD ** -0.5 if scale is None else float(scale)
    if ATTN_WIDE_LAUNCH_LOG is not None and not p.io_f32:
        ATTN_WIDE_LAUNCH_LOG.append({"params": p, "flops": 4.0 * B * Lq * Lk * WIDE_HEAD, "keep": (q, k, v, out)})
    _lib.check(lib.aptp_attention_wide(ctypes.byref(p), _stream()), "aptp_attention_wide")
    return out


def image_out(y: torch.Tensor, out_dtype: torch.dtype = torch.float32, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The VAE decoder's image epilogue (diffusers postprocess, do_denormalize): conv_out's fp32 [B, H, W, ld] (3 real
    channels) -> clamp(y / 2 + 0.5, 0, 1) as fp32 [B, 3, H, W], or as uint8 [B, H, W, 3] = round_half_even(255 v)
    (out_dtype=torch.uint8, numpy_to_pil's rounding)."""
    lib = _lib.load()
    if not (y.is_cuda and y.dtype == torch.float32 and y.dim() == 4 and y.shape[3] >= 3 and y.stride(3) == 1
            and y.is_contiguous()):
        raise ValueError(f"image_out: expected a contiguous CUDA fp32 [B, H, W, >=3] tensor, got {y.dtype} {tuple(y.shape)}")
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError("image_out: out_dtype is torch.float32 or torch.uint8")
    B, H, W, ld = y.shape
    shape = (B, H, W, 3) if out_dtype == torch.uint8 else (B, 3, H, W)
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=y.device)
    if tuple(out.shape) != shape or out.dtype != out_dtype or not out.is_contiguous():
        raise ValueError(f"image_out: out must be a contiguous {out_dtype} {shape} tensor")
    p = ImageOutParams()
    p.y, p.ldy, p.out, p.out_u8 = y.data_ptr(), ld, out.data_ptr(), int(out_dtype == torch.uint8)
    p.B, p.H, p.W = B, H, W
    _lib.check(lib.aptp_image_out(ctypes.byref(p), _stream()), "aptp_image_out")
    return out


def image_in(x: torch.Tensor, out_f32: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The VAE encoder's image prologue: pixel_values NCHW [B, 3, H, W] (fp32 or bf16) -> the 3x3 / pad-1 im2col of every
    pixel, [B, H, W, 32] tap-major ((ky, kx, c): 27 values, then 5 zeros), bf16 (fp32 with out_f32: the parity path).
    encoder.conv_in then runs as a 1x1 contraction over 32 channels (pack_conv_in_im2col)."""
    lib = _lib.load()
    if not (x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16) and x.is_contiguous()):
        raise ValueError(f"image_in: expected a contiguous CUDA fp32 / bf16 NCHW tensor, got {x.dtype} {tuple(x.shape)}")
    B, C, H, W = x.shape
    dt = torch.float32 if out_f32 else torch.bfloat16
    if out is None:
        out = torch.empty(B, H, W, 32, dtype=dt, device=x.device)
    if tuple(out.shape) != (B, H, W, 32) or out.dtype != dt or not out.is_contiguous():
        raise ValueError(f"image_in: out must be a contiguous {dt} {(B, H, W, 32)} tensor")
    p = ImageInParams()
    p.x, p.x_bf16, p.out, p.out_f32 = x.data_ptr(), int(x.dtype == torch.bfloat16), out.data_ptr(), int(out_f32)
    p.B, p.C, p.H, p.W = B, C, H, W
    _lib.check(lib.aptp_image_in(ctypes.byref(p), _stream()), "aptp_image_in")
    return out


def pack_conv_in_im2col(w: torch.Tensor, bias: Optional[torch.Tensor], device=None) -> PackedWeight:
    """conv_in's OIHW [O, 3, 3, 3] weight as the [O, 32] weight of the 1x1 contraction over image_in's columns:
    w'[o, (ky * 3 + kx) * 3 + c] = w[o, c, ky, kx], columns 27..31 zero"""
    O, C, KH, KW = w.shape
    if (C, KH, KW) != (3, 3, 3):
        raise ValueError(f"pack_conv_in_im2col: expected a [O, 3, 3, 3] weight, got {tuple(w.shape)}")
    w2 = torch.zeros(O, 32, dtype=torch.float32, device=w.device)
    w2[:, :27] = w.detach().float().permute(0, 2, 3, 1).reshape(O, 27)
    return pack_weight(w2, None if bias is None else bias.detach(), device=device)


def latent_dist(y: torch.Tensor, wq: torch.Tensor, bq: torch.Tensor, eps: Optional[torch.Tensor] = None,
                scale: float = 1.0, moments: bool = True, latents_dtype: torch.dtype = torch.float32,
                moments_out: Optional[torch.Tensor] = None, latents_out: Optional[torch.Tensor] = None):
    """The VAE encoder's tail: quant_conv (wq fp32 [8, 8], bq fp32 [8]) on conv_out's fp32 [B, h, w, ld] -> (moments fp32
    [B, 8, h, w] NCHW or None, latents [B, 4, h, w] or None), latents = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps)
    for the given fp32 NCHW eps [B, 4, h, w]."""
    lib = _lib.load()
    if not (y.is_cuda and y.dtype == torch.float32 and y.dim() == 4 and y.shape[3] >= 8 and y.is_contiguous()):
        raise ValueError(f"latent_dist: expected a contiguous CUDA fp32 [B, h, w, >=8] tensor, got {y.dtype} {tuple(y.shape)}")
    B, H, W, ld = y.shape
    wq = wq.to(device=y.device, dtype=torch.float32).reshape(8, 8).contiguous()
    bq = bq.to(device=y.device, dtype=torch.float32).reshape(8).contiguous()
    p = LatentDistParams()
    p.y, p.ldy, p.wq, p.bq = y.data_ptr(), ld, wq.data_ptr(), bq.data_ptr()
    p.B, p.H, p.W, p.scale = B, H, W, float(scale)
    mom = lat = None
    if moments:
        mom = moments_out if moments_out is not None else torch.empty(B, 8, H, W, dtype=torch.float32, device=y.device)
        if tuple(mom.shape) != (B, 8, H, W) or mom.dtype != torch.float32 or not mom.is_contiguous():
            raise ValueError(f"latent_dist: moments must be a contiguous fp32 {(B, 8, H, W)} tensor")
        p.moments = mom.data_ptr()
    if eps is not None:
        if tuple(eps.shape) != (B, 4, H, W) or eps.dtype != torch.float32 or not eps.is_contiguous() or eps.device != y.device:
            raise ValueError(f"latent_dist: eps must be a contiguous fp32 {(B, 4, H, W)} tensor on {y.device}")
        if latents_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("latent_dist: latents_dtype is torch.float32 or torch.bfloat16")
        lat = latents_out if latents_out is not None else torch.empty(B, 4, H, W, dtype=latents_dtype, device=y.device)
        if tuple(lat.shape) != (B, 4, H, W) or lat.dtype != latents_dtype or not lat.is_contiguous():
            raise ValueError(f"latent_dist: latents must be a contiguous {latents_dtype} {(B, 4, H, W)} tensor")
        p.eps, p.latents, p.latents_bf16 = eps.data_ptr(), lat.data_ptr(), int(latents_dtype == torch.bfloat16)
    _lib.check(lib.aptp_latent_dist(ctypes.byref(p), _stream()), "aptp_latent_dist")
    return mom, lat


CAUSAL_MAX_L = 128


def attention_causal(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: Optional[float] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(q k^T * scale + causal mask) v with head_dim 64 and 1 <= L <= 128 (CLIP's text self-attention): key j > query i
    gets weight 0.  q, k, v and out [B, L, heads*64] are views with a contiguous last dim on one device (e.g. column slices of
    a fused q|k|v buffer); bf16, or fp32 for the parity path.  Default scale 64^-0.5."""
    lib = _lib.load()
    B, L = q.shape[0], q.shape[1]
    if out is None:
        out = torch.empty(B, L, heads * 64, dtype=q.dtype, device=q.device)
    _check_heads64_views(q, k, v, out, B, L, heads, "attention_causal")
    p = AttentionCausalParams()
    p.io_f32 = int(q.dtype == torch.float32)
    _set_views(p, q=q, k=k, v=v, o=out)
    p.B, p.heads, p.L = B, heads, L
    p.scale = 0.125 if scale is None else scale
    _lib.check(lib.aptp_attention_causal(ctypes.byref(p), _stream()), "aptp_attention_causal")
    return out


def token_embed(ids: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor, out_f32: bool = False,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, L] int64 ids -> bf16 (fp32 when out_f32) [B, L, C] = tok[ids] + pos[:L] (CLIPTextEmbeddings), one rounding.
    tok fp32 [vocab, C], pos fp32 [>= L, C].  An id outside [0, vocab) is not read: its row comes out NaN (the caller
    checks ids where it can afford a host sync)."""
    lib = _lib.load()
    if ids.dtype != torch.int64 or ids.dim() != 2 or not ids.is_contiguous() or not ids.is_cuda:
        raise ValueError(f"token_embed: ids must be a contiguous CUDA int64 [B, L] tensor, got {ids.dtype} {tuple(ids.shape)}")
    B, L = ids.shape
    V, C = tok.shape
    for t, nm in ((tok, "tok"), (pos, "pos")):
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.shape[1] != C or t.device != ids.device:
            raise ValueError(f"token_embed: {nm} must be a contiguous fp32 [rows, {C}] tensor on the ids' device")
    if pos.shape[0] < L:
        raise ValueError(f"token_embed: {L} tokens but only {pos.shape[0]} positions")
    odt = torch.float32 if out_f32 else torch.bfloat16
    if out is None:
        out = torch.empty(B, L, C, dtype=odt, device=ids.device)
    elif tuple(out.shape) != (B, L, C) or out.dtype != odt or not out.is_contiguous():
        raise ValueError(f"token_embed: out must be a contiguous {odt} [{B}, {L}, {C}] tensor")
    p = TokenEmbedParams()
    p.ids, p.tok, p.pos, p.out, p.ldo = ids.data_ptr(), tok.data_ptr(), pos.data_ptr(), out.data_ptr(), C
    p.B, p.L, p.C, p.vocab, p.out_f32, p.pos_rows = B, L, C, V, int(out_f32), pos.shape[0]
    _lib.check(lib.aptp_token_embed(ctypes.byref(p), _stream()), "aptp_token_embed")
    return out


BIAS_MAX_L = 512


def _check_heads64_views(q, k, v, out, B: int, L: int, heads: int, name: str):
    for t in (q, k, v, out):
        if t.dtype != q.dtype or t.dtype not in (torch.bfloat16, torch.float32) or t.dim() != 3 or t.stride(2) != 1 \
                or tuple(t.shape) != (B, L, heads * 64) or not t.is_cuda or t.device != q.device:
            raise ValueError(f"{name}: q, k, v and out must be {q.dtype} [B, L, {heads * 64}] views with contiguous "
                             f"channels on {q.device}, got {t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")


def _check_mask(mask: Optional[torch.Tensor], B: int, L: int, device, name: str):
    if mask is not None and (mask.dtype != torch.float32 or tuple(mask.shape) != (B, L) or not mask.is_contiguous()
                             or mask.device != device):
        raise ValueError(f"{name}: the mask must be a contiguous fp32 [{B}, {L}] tensor on {device}, got {mask.dtype} "
                         f"{tuple(mask.shape)} on {mask.device}")


def attention_bias(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, relbias: torch.Tensor,
                   key_mask: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(q k^T * scale + relbias[h, j - i + L - 1] + key mask) v with head_dim 64 and 1 <= L <= 512 (MPNet's
    self-attention).  q, k, v and out [B, L, heads*64] are views with a contiguous last dim on one device (e.g. column slices
    of a fused q|k|v buffer); bf16, or fp32 for the parity path.  relbias fp32 [heads, 2L-1]; key_mask fp32 [B, L] (0 = masked,
    any pattern) or None for all valid: a masked key gets weight exactly 0.  Default scale 64^-0.5.

    Every row of out below L is written.  With kend = 1 + the last valid key of a sample (0 when it has none), the bf16 kernel
    writes exact zeros into every 16-row strip that starts at or past kend (so into every row of a sample without a valid key)
    and ordinary attention values into the rows past kend inside the strip that straddles it; the fp32 path computes every row
    (zeros only for a sample without a valid key).  Rows at or past kend are padding either way."""
    lib = _lib.load()
    B, L = q.shape[0], q.shape[1]
    if out is None:
        out = torch.empty(B, L, heads * 64, dtype=q.dtype, device=q.device)
    _check_heads64_views(q, k, v, out, B, L, heads, "attention_bias")
    if relbias.dtype != torch.float32 or tuple(relbias.shape) != (heads, 2 * L - 1) or not relbias.is_contiguous() \
            or relbias.device != q.device:
        raise ValueError(f"attention_bias: relbias must be a contiguous fp32 [{heads}, {2 * L - 1}] tensor on {q.device}, got "
                         f"{relbias.dtype} {tuple(relbias.shape)} on {relbias.device}")
    _check_mask(key_mask, B, L, q.device, "attention_bias")
    p = AttentionBiasParams()
    p.io_f32 = int(q.dtype == torch.float32)
    _set_views(p, q=q, k=k, v=v, o=out)
    p.relbias, p.key_mask = relbias.data_ptr(), (None if key_mask is None else key_mask.data_ptr())
    p.B, p.heads, p.L = B, heads, L
    p.scale = 0.125 if scale is None else scale
    _lib.check(lib.aptp_attention_bias(ctypes.byref(p), _stream()), "aptp_attention_bias")
    return out


def embed_ln(ids: torch.Tensor, word: torch.Tensor, pos: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
             eps: float = 1e-5, pad_id: int = 1, out_f32: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, L] int64 ids -> bf16 (fp32 when out_f32) [B, L, C] = LayerNorm(word[ids] + pos[pos_id]) (MPNetEmbeddings), where
    pos_id counts the non-pad ids up to and including the token, plus pad_id (a pad token: pad_id).  word fp32 [vocab, C], pos
    fp32 [> L + pad_id, C], gamma / beta fp32 [C].  An id outside [0, vocab) is not read: its row comes out NaN."""
    lib = _lib.load()
    if ids.dtype != torch.int64 or ids.dim() != 2 or not ids.is_contiguous() or not ids.is_cuda:
        raise ValueError(f"embed_ln: ids must be a contiguous CUDA int64 [B, L] tensor, got {ids.dtype} {tuple(ids.shape)}")
    B, L = ids.shape
    V, C = word.shape
    for t, nm, shp in ((word, "word", (V, C)), (pos, "pos", (pos.shape[0], C)), (gamma, "gamma", (C,)), (beta, "beta", (C,))):
        if t.dtype != torch.float32 or tuple(t.shape) != shp or not t.is_contiguous() or t.device != ids.device:
            raise ValueError(f"embed_ln: {nm} must be a contiguous fp32 {shp} tensor on the ids' device")
    if pos.shape[0] <= L + pad_id:
        raise ValueError(f"embed_ln: {L} tokens with pad id {pad_id} need {L + pad_id + 1} positions, have {pos.shape[0]}")
    odt = torch.float32 if out_f32 else torch.bfloat16
    if out is None:
        out = torch.empty(B, L, C, dtype=odt, device=ids.device)
    elif tuple(out.shape) != (B, L, C) or out.dtype != odt or not out.is_contiguous():
        raise ValueError(f"embed_ln: out must be a contiguous {odt} [{B}, {L}, {C}] tensor")
    p = EmbedLnParams()
    p.ids, p.word, p.pos, p.gamma, p.beta = ids.data_ptr(), word.data_ptr(), pos.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    p.out, p.ldo = out.data_ptr(), C
    p.B, p.L, p.C, p.vocab, p.pos_rows, p.pad_id, p.out_f32, p.eps = B, L, C, V, pos.shape[0], pad_id, int(out_f32), eps
    _lib.check(lib.aptp_embed_ln(ctypes.byref(p), _stream()), "aptp_embed_ln")
    return out


def masked_mean(x: torch.Tensor, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 or fp32 [B, L, C] -> fp32 [B, C] = sum_l x * mask / max(sum_l mask, 1e-9); mask fp32 [B, L] or None (all ones).
    fp32 sums in a fixed order: bit-identical from run to run."""
    lib = _lib.load()
    if x.dtype not in (torch.bfloat16, torch.float32) or x.dim() != 3 or x.stride(2) != 1 or not x.is_cuda:
        raise ValueError(f"masked_mean: x must be a CUDA bf16 or fp32 [B, L, C] tensor with contiguous channels, got {x.dtype} "
                         f"{tuple(x.shape)}")
    B, L, C = x.shape
    _check_mask(mask, B, L, x.device, "masked_mean")
    if out is None:
        out = torch.empty(B, C, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (B, C) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"masked_mean: out must be a contiguous fp32 [{B}, {C}] tensor on {x.device}")
    p = MaskedMeanParams()
    p.x, p.x_stride_b, p.x_stride_l = x.data_ptr(), x.stride(0), (x.stride(1) if L > 1 else max(x.stride(1), C))
    p.mask, p.out = (None if mask is None else mask.data_ptr()), out.data_ptr()
    p.B, p.L, p.C, p.x_f32 = B, L, C, int(x.dtype == torch.float32)
    _lib.check(lib.aptp_masked_mean(ctypes.byref(p), _stream()), "aptp_masked_mean")
    return out


# OpenAI CLIP's image normalisation (transformers OPENAI_CLIP_MEAN / OPENAI_CLIP_STD, the CLIPImageProcessor defaults)
CLIP_IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)


def image_patches(x: torch.Tensor, size: int, patch: int, *, resize: bool = True, mean=CLIP_IMAGE_MEAN, std=CLIP_IMAGE_STD,
                  out_f32: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Image front end of the CLIP image encoder.  resize=True: fp32 images in [0, 1], [B, H, W, 3] or [B, 3, H, W] (told apart
    by which of the two dims is 3; [B, 3, H, 3] is refused) -> bicubic resize to size x size (F.interpolate semantics),
    (v - mean) / std, patchify.  resize=False: x is pixel_values [B, 3, size, size], only patchified.  Returns bf16 (fp32 when
    out_f32) [B * (size / patch)^2, Kpad], Kpad = roundup64(3 patch^2), row element order (c, py, px), zero tail."""
    lib = _lib.load()
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError(f"image_patches: x must be a contiguous CUDA fp32 4-D tensor, got {x.dtype} {tuple(x.shape)}")
    if size < 1 or patch < 1 or size % patch != 0:
        raise ValueError(f"image_patches: size {size} must be a positive multiple of patch {patch}")
    first, last = x.shape[1] == 3, x.shape[3] == 3
    if first == last:
        raise ValueError(f"image_patches: cannot tell [B, H, W, 3] from [B, 3, H, W] in shape {tuple(x.shape)}")
    nchw = first
    B = x.shape[0]
    H, W = (x.shape[2], x.shape[3]) if nchw else (x.shape[1], x.shape[2])
    if not resize and not (nchw and H == size and W == size):
        raise ValueError(f"image_patches: resize=False takes pixel_values [B, 3, {size}, {size}], got {tuple(x.shape)}")
    if B < 1 or H < 1 or W < 1:
        raise ValueError("image_patches: empty input")
    G = size // patch
    kpad = round_up(3 * patch * patch, 64)
    odt = torch.float32 if out_f32 else torch.bfloat16
    if out is None:
        out = torch.empty(B * G * G, kpad, dtype=odt, device=x.device)
    elif tuple(out.shape) != (B * G * G, kpad) or out.dtype != odt or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"image_patches: out must be a contiguous {odt} [{B * G * G}, {kpad}] tensor on {x.device}")
    p = ImagePatchesParams()
    p.x, p.nchw, p.B, p.H, p.W, p.S, p.P, p.resize = x.data_ptr(), int(nchw), B, H, W, size, patch, int(resize)
    for c in range(3):
        p.mean[c], p.std[c] = float(mean[c]), float(std[c])
    p.out, p.ldo, p.out_f32 = out.data_ptr(), kpad, int(out_f32)
    _lib.check(lib.aptp_image_patches(ctypes.byref(p), _stream()), "aptp_image_patches")
    return out


def vit_embed_ln(patches: torch.Tensor, B: int, cls: torch.Tensor, pos: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                 eps: float = 1e-5, out_f32: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 patch GEMM output [B * (T - 1), C] -> bf16 (fp32 when out_f32) [B, T, C] = LayerNorm([cls | patches] + pos)
    (transformers CLIPVisionEmbeddings + pre_layrnorm): fp32 sum and statistics, one rounding.  cls fp32 [C], pos fp32 [T, C]."""
    lib = _lib.load()
    if patches.dtype != torch.float32 or patches.dim() != 2 or patches.stride(1) != 1 or not patches.is_cuda:
        raise ValueError(f"vit_embed_ln: patches must be a CUDA fp32 [rows, C] tensor, got {patches.dtype} {tuple(patches.shape)}")
    rows, C = patches.shape
    T = pos.shape[0]
    if B < 1 or T < 2 or rows != B * (T - 1):
        raise ValueError(f"vit_embed_ln: {rows} patch rows do not make {B} samples of {T} - 1 tokens")
    for t, nm, shp in ((cls, "cls", (C,)), (pos, "pos", (T, C)), (gamma, "gamma", (C,)), (beta, "beta", (C,))):
        if t.dtype != torch.float32 or tuple(t.shape) != shp or not t.is_contiguous() or t.device != patches.device:
            raise ValueError(f"vit_embed_ln: {nm} must be a contiguous fp32 {shp} tensor on the patches' device")
    odt = torch.float32 if out_f32 else torch.bfloat16
    if out is None:
        out = torch.empty(B, T, C, dtype=odt, device=patches.device)
    elif tuple(out.shape) != (B, T, C) or out.dtype != odt or not out.is_contiguous():
        raise ValueError(f"vit_embed_ln: out must be a contiguous {odt} [{B}, {T}, {C}] tensor")
    p = VitEmbedLnParams()
    p.patches, p.ldp = patches.data_ptr(), patches.stride(0) if rows > 1 else max(patches.stride(0), C)
    p.cls, p.pos, p.gamma, p.beta = cls.data_ptr(), pos.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    p.out, p.ldo, p.B, p.T, p.C, p.out_f32, p.eps = out.data_ptr(), C, B, T, C, int(out_f32), eps
    _lib.check(lib.aptp_vit_embed_ln(ctypes.byref(p), _stream()), "aptp_vit_embed_ln")
    return out


def l2_normalize(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [n, D] -> rows divided by their Euclidean norm (no epsilon, as the reference); out may be x itself"""
    lib = _lib.load()
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous() or not x.is_cuda or x.shape[0] < 1:
        raise ValueError(f"l2_normalize: x must be a contiguous CUDA fp32 [n, D] tensor, got {x.dtype} {tuple(x.shape)}")
    n, D = x.shape
    if out is None:
        out = torch.empty_like(x)
    elif tuple(out.shape) != (n, D) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"l2_normalize: out must be a contiguous fp32 [{n}, {D}] tensor on {x.device}")
    p = L2NormalizeParams()
    p.x, p.ldx, p.out, p.ldo, p.n, p.D = x.data_ptr(), D, out.data_ptr(), D, n, D
    _lib.check(lib.aptp_l2_normalize(ctypes.byref(p), _stream()), "aptp_l2_normalize")
    return out


MMD_SIGMA = 10.0          # bandwidth of CMMD's Gaussian kernel and its readability scale (cmmd-pytorch/distance.py:20-25)
MMD_SCALE = 1000.0


def mmd_rbf(x: torch.Tensor, y: torch.Tensor, sigma: float = MMD_SIGMA, scale: float = MMD_SCALE, parts: bool = False) -> torch.Tensor:
    """scale * (mean k(x, x) + mean k(y, y) - 2 mean k(x, y)), k(a, b) = exp(-|a - b|^2 / (2 sigma^2)), for fp32 x [n, D] and
    y [m, D] on the device: an fp64 scalar tensor (parts: the fp64 [4] the kernel writes, include/aptp_hip.h).  The kernel
    matrices are never stored; the only allocation is the workspace of 4 (n + m) bytes and 4 bytes per 128 x 128 tile."""
    lib = _lib.load()
    for t, nm in ((x, "x"), (y, "y")):
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or not t.is_cuda or t.shape[0] < 1:
            raise ValueError(f"mmd_rbf: {nm} must be a contiguous CUDA fp32 [rows, D] tensor, got {t.dtype} {tuple(t.shape)}")
    if x.shape[1] != y.shape[1] or x.shape[1] % 4 != 0 or x.shape[1] < 4 or x.device != y.device:
        raise ValueError(f"mmd_rbf: x and y need the same width, a multiple of 4, on one device; got {tuple(x.shape)} and {tuple(y.shape)}")
    if not sigma > 0:
        raise ValueError("mmd_rbf: sigma must be positive")
    n, m, D = x.shape[0], y.shape[0], x.shape[1]
    ws = torch.empty(lib.aptp_mmd_rbf_workspace_bytes(n, m) // 4, dtype=torch.float32, device=x.device)
    out = torch.empty(4, dtype=torch.float64, device=x.device)
    p = MmdRbfParams()
    p.x, p.ldx, p.y, p.ldy, p.n, p.m, p.D = x.data_ptr(), D, y.data_ptr(), D, n, m, D
    p.sigma, p.scale, p.workspace, p.out = sigma, scale, ws.data_ptr(), out.data_ptr()
    _lib.check(lib.aptp_mmd_rbf(ctypes.byref(p), _stream()), "aptp_mmd_rbf")
    return out if parts else out[0]


# ------------------------------------------------------------------------------------------------------------------
# the CLIP score's device path (csrc/clip_score_ops.hip)
# ------------------------------------------------------------------------------------------------------------------
PIL_PRECISION_BITS = 22           # PIL's fixed point for 8-bit images: 32 - 8 - 2 (Resample.c)


def _pil_bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _pil_filter_table(in_size: int, out_size: int, filt, filt_support: float, what: str):
    """PIL's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for one axis and one filter, statement for statement in Python
    floats (IEEE doubles, as PIL's C doubles)"""
    import math

    import numpy as np
    if in_size < 1 or out_size < 1:
        raise ValueError(f"{what}: sizes must be positive, got {in_size} -> {out_size}")
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = filt_support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    weights = np.zeros((out_size, ksize), np.int32)
    one = float(1 << PIL_PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)                  # int() truncates like C's cast
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        bounds[xx] = (xmin, xmax)
        for x, w in enumerate(k):
            weights[xx, x] = int(-0.5 + w * one) if w < 0 else int(0.5 + w * one)
    return bounds, weights


def pil_bicubic_table(in_size: int, out_size: int):
    """PIL's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for a bicubic resize of one axis, statement for statement in
    Python floats (IEEE doubles, as PIL's C doubles): (bounds int32 [out, 2] = (xmin, count), weights int32 [out, ksize]) as numpy
    arrays; weights past ``count`` are 0.  ksize = 2 ceil(2 max(in / out, 1)) + 1."""
    return _pil_filter_table(in_size, out_size, _pil_bicubic, 2.0, "pil_bicubic_table")


def _pil_bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def pil_bilinear_table(in_size: int, out_size: int):
    """The same for PIL's BILINEAR (the triangle filter: support 1, 1 - |x| inside it), the training transform's resize:
    ksize = 2 ceil(max(in / out, 1)) + 1."""
    return _pil_filter_table(in_size, out_size, _pil_bilinear, 1.0, "pil_bilinear_table")


def pil_resized_size(H: int, W: int, size: int):
    """(H1, W1, top, left): torchvision's Resize(size) of an H x W image -- the shorter side to size, the longer one to
    int(size * long / short) -- and CenterCrop(size)'s offsets round((H1 - size) / 2), round((W1 - size) / 2) (Python's round)"""
    if H < 1 or W < 1 or size < 1:
        raise ValueError(f"pil_resized_size: sizes must be positive, got {H} x {W} -> {size}")
    H1, W1 = (size, int(size * W / H)) if H <= W else (int(size * H / W), size)
    return H1, W1, int(round((H1 - size) / 2.0)), int(round((W1 - size) / 2.0))


_PIL_TABLES = {}
_PIL_TABLES_CAP = 16


def _pil_tables(H: int, W: int, size: int, device):
    """device copies of the two coefficient tables of an (H, W) -> size preprocess, cached per (H, W, size, device); the entry of
    an axis whose size does not change is None"""
    key = (H, W, size, str(device))
    t = _PIL_TABLES.get(key)
    if t is None:
        H1, W1, _, _ = pil_resized_size(H, W, size)
        t = []
        for n_in, n_out in ((W, W1), (H, H1)):
            if n_in == n_out:
                t.append(None)
            else:
                b, w = pil_bicubic_table(n_in, n_out)
                t.append((torch.from_numpy(b).to(device), torch.from_numpy(w).to(device)))
        if len(_PIL_TABLES) >= _PIL_TABLES_CAP:
            _PIL_TABLES.pop(next(iter(_PIL_TABLES)))
        _PIL_TABLES[key] = t
    return t


def image_patches_pil(x: torch.Tensor, size: int, patch: int, *, mean=CLIP_IMAGE_MEAN, std=CLIP_IMAGE_STD, out_f32: bool = False,
                      out: Optional[torch.Tensor] = None, tables=None) -> torch.Tensor:
    """Image front end of the CLIP score: uint8 images [B, H, W, 3] -> OpenAI CLIP's ``preprocess`` (PIL bicubic resize of the
    shorter side to size, bit-exact; centre crop; / 255; (v - mean) / std) -> the rows of ``image_patches``: bf16 (fp32 when
    out_f32) [B * (size / patch)^2, Kpad].  The coefficient tables of a new (H, W, size) are built on the host and uploaded, so
    call once eagerly before capturing a graph of that shape.  tables: ((xbounds, xweights) | None, (ybounds, yweights) | None)
    instead of the cached ones (tests)."""
    lib = _lib.load()
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError(f"image_patches_pil: x must be a contiguous CUDA uint8 [B, H, W, 3] tensor, got {x.dtype} {tuple(x.shape)}")
    if size < 1 or patch < 1 or size % patch != 0:
        raise ValueError(f"image_patches_pil: size {size} must be a positive multiple of patch {patch}")
    B, H, W, _ = x.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"image_patches_pil: empty input {tuple(x.shape)}")
    H1, W1, _, _ = pil_resized_size(H, W, size)
    if tables is None:
        if torch.cuda.is_current_stream_capturing() and (H, W, size, str(x.device)) not in _PIL_TABLES:
            raise RuntimeError("image_patches_pil: run one eager call of this shape before capturing it")
        tables = _pil_tables(H, W, size, x.device)
    G = size // patch
    kpad = round_up(3 * patch * patch, 64)
    odt = torch.float32 if out_f32 else torch.bfloat16
    if out is None:
        out = torch.empty(B * G * G, kpad, dtype=odt, device=x.device)
    elif tuple(out.shape) != (B * G * G, kpad) or out.dtype != odt or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"image_patches_pil: out must be a contiguous {odt} [{B * G * G}, {kpad}] tensor on {x.device}")
    p = ImagePatchesPilParams()
    p.x, p.B, p.H, p.W, p.S, p.P = x.data_ptr(), B, H, W, size, patch
    for axis, n_out, tb in (("x", W1, tables[0]), ("y", H1, tables[1])):
        if tb is None:
            continue
        bnd, wts = tb
        if bnd.dtype != torch.int32 or wts.dtype != torch.int32 or tuple(bnd.shape) != (n_out, 2) or wts.dim() != 2 \
                or wts.shape[0] != n_out or not bnd.is_contiguous() or not wts.is_contiguous() or bnd.device != x.device \
                or wts.device != x.device:
            raise ValueError(f"image_patches_pil: the {axis} table must be int32 [{n_out}, 2] bounds and int32 [{n_out}, k] weights on "
                             f"{x.device}")
        setattr(p, axis + "bounds", bnd.data_ptr())
        setattr(p, axis + "weights", wts.data_ptr())
        setattr(p, axis + "k", wts.shape[1])
    scratch = torch.empty(B, H, W1, 3, dtype=torch.uint8, device=x.device) if W1 != W else None
    p.scratch = None if scratch is None else scratch.data_ptr()
    for c in range(3):
        p.mean[c], p.std[c] = float(mean[c]), float(std[c])
    p.out, p.ldo, p.out_f32 = out.data_ptr(), kpad, int(out_f32)
    _lib.check(lib.aptp_image_patches_pil(ctypes.byref(p), _stream()), "aptp_image_patches_pil")
    return out


# ------------------------------------------------------------------------------------------------------------------
# the training dataloader's transform (csrc/train_image_ops.hip)
# ------------------------------------------------------------------------------------------------------------------
_BILINEAR_TABLES = {}             # (in, out, device) -> (flat int32 device tensor [out * (2 + k)], host bounds [out, 2], k)
_BILINEAR_TABLES_CAP = 256        # a few KB each: one per distinct (source extent, resized extent) of a dataset


def _bilinear_table_on(n_in: int, n_out: int, device):
    """the bilinear table of one axis on the device in aptp_train_images' layout (bounds, then weights), cached per
    (in, out, device); the least recently used entry leaves a full cache"""
    key = (n_in, n_out, str(device))
    t = _BILINEAR_TABLES.pop(key, None)
    if t is None:
        import numpy as np
        b, w = pil_bilinear_table(n_in, n_out)
        flat = torch.from_numpy(np.concatenate([b.reshape(-1), w.reshape(-1)])).to(device)
        t = (flat, b, w.shape[1])
        if len(_BILINEAR_TABLES) >= _BILINEAR_TABLES_CAP:
            _BILINEAR_TABLES.pop(next(iter(_BILINEAR_TABLES)))
    _BILINEAR_TABLES[key] = t         # (re)inserted last: the dict's order is the order of use
    return t


def _check_train_images(images, R, tops, lefts, flips, resized_sizes):
    """argument checks of train_images, none of which touches a device: the resized sizes [(H1, W1)]"""
    if not isinstance(images, (list, tuple)) or len(images) == 0:
        raise ValueError("train_images: images must be a non-empty list of uint8 [H, W, 3] tensors")
    if not isinstance(R, int) or R < 1:
        raise ValueError(f"train_images: R must be a positive int, got {R!r}")
    B = len(images)
    for nm, v in (("tops", tops), ("lefts", lefts), ("flips", flips)):
        if len(v) != B:
            raise ValueError(f"train_images: {nm} has {len(v)} entries for {B} images")
    if resized_sizes is not None and len(resized_sizes) != B:
        raise ValueError(f"train_images: resized_sizes has {len(resized_sizes)} entries for {B} images")
    sizes = []
    for i, im in enumerate(images):
        if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.shape[0] < 1 \
                or im.shape[1] < 1:
            got = f"{im.dtype} {tuple(im.shape)}" if isinstance(im, torch.Tensor) else type(im).__name__
            raise ValueError(f"train_images: image {i} must be a uint8 [H, W, 3] tensor, got {got}")
        H, W = int(im.shape[0]), int(im.shape[1])
        H1, W1 = pil_resized_size(H, W, R)[:2] if resized_sizes is None else (int(resized_sizes[i][0]), int(resized_sizes[i][1]))
        if H1 < R or W1 < R:
            raise ValueError(f"train_images: image {i} ({H} x {W}) is resized to {H1} x {W1}, smaller than the crop {R}")
        top, left, flip = int(tops[i]), int(lefts[i]), int(flips[i])
        if top < 0 or left < 0 or top + R > H1 or left + R > W1:
            raise ValueError(f"train_images: image {i}: the crop window (top {top}, left {left}, size {R}) leaves the resized image "
                             f"{H1} x {W1}")
        if flip not in (0, 1):
            raise ValueError(f"train_images: image {i}: flip must be 0 or 1, got {flips[i]!r}")
        sizes.append((H1, W1))
    return sizes


def _train_images_plan(shapes, sizes, R, tops, lefts, flips, device):
    """(descriptor rows, the concatenated table buffer on ``device`` or None, scratch bytes) of one batch: images of equal
    (in, out) share a table; an image's scratch region holds only the rows its vertical windows reach"""
    B = len(shapes)
    desc = (_lib.TrainImageDesc * B)()
    pieces, offsets, tab_len = [], {}, 0

    def table(n_in, n_out):
        nonlocal tab_len
        t = _bilinear_table_on(n_in, n_out, device)
        if (n_in, n_out) not in offsets:
            offsets[(n_in, n_out)] = tab_len
            pieces.append(t[0])
            tab_len += t[0].numel()
        return offsets[(n_in, n_out)], t[1], t[2]

    src_off = scratch_len = 0
    for i, (H, W) in enumerate(shapes):
        d = desc[i]
        H1, W1 = sizes[i]
        d.src_off, d.H, d.W, d.H1, d.W1 = src_off, H, W, H1, W1
        d.top, d.left, d.flip = int(tops[i]), int(lefts[i]), int(flips[i])
        src_off += H * W * 3
        d.xtab_off = d.ytab_off = _lib.TRAIN_NO_TABLE
        row0, nrows = d.top, R                          # without a vertical pass the window's own rows
        if H1 != H:
            d.ytab_off, yb, d.yk = table(H, H1)
            win = yb[d.top:d.top + R]
            row0 = int(win[:, 0].min())
            nrows = int((win[:, 0] + win[:, 1]).max()) - row0
        if W1 != W:
            d.xtab_off, _, d.xk = table(W, W1)
            d.row0, d.nrows, d.scratch_off = row0, nrows, scratch_len
            scratch_len += nrows * R * 3
    tables = torch.cat(pieces) if len(pieces) > 1 else (pieces[0] if pieces else None)
    return desc, tables, scratch_len


def train_images(images, R: int, tops, lefts, flips, out_f32: bool = True, out: Optional[torch.Tensor] = None, *,
                 resized_sizes=None, device=None) -> torch.Tensor:
    """The training dataloader's transform on a ragged batch: a list of uint8 [H, W, 3] images (CPU or GPU tensors, any mix
    of sizes) -> pixel_values NCHW [B, 3, R, R], fp32 (bf16 when not out_f32): PIL's bilinear Resize(R) bit for bit, the crop
    window at (tops[i], lefts[i]) of the resized image, a horizontal flip where flips[i], ToTensor and Normalize(0.5, 0.5).
    The draws are the caller's (data.draw_crop_flip).  resized_sizes: [(H1, W1)] per image, default pil_resized_size (the
    shorter side to R).  Two launches for the whole batch; one host-to-device copy for the images (when they are on the CPU),
    one for the descriptor table, and one per coefficient table not yet on the device (cached per (in, out, device), so none
    in steady state) -- host copies: not for graph capture.  device: where to run when every image is on the CPU (default: the
    current CUDA device)."""
    sizes = _check_train_images(images, R, tops, lefts, flips, resized_sizes)
    B = len(images)
    odt = torch.float32 if out_f32 else torch.bfloat16
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, 3, R, R) or out.dtype != odt
                            or not out.is_contiguous() or not out.is_cuda):
        raise ValueError(f"train_images: out must be a contiguous CUDA {odt} [{B}, 3, {R}, {R}] tensor")
    lib = _lib.load()
    if device is None:
        device = out.device if out is not None else next((im.device for im in images if im.is_cuda), None)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"train_images: the transform runs on HIP kernels only, got device {device}")
    for i, im in enumerate(images):
        if im.is_cuda and im.device != device:
            raise ValueError(f"train_images: image {i} is on {im.device}, the batch on {device}")
    if out is not None and out.device != device:
        raise ValueError(f"train_images: out is on {out.device}, the batch on {device}")
    with torch.cuda.device(device):
        if all(not im.is_cuda for im in images):
            flat = torch.cat([im.reshape(-1) for im in images]).to(device)              # one copy
        else:
            flat = torch.cat([im.to(device).reshape(-1) for im in images])
        desc, tables, scratch_len = _train_images_plan([(int(im.shape[0]), int(im.shape[1])) for im in images], sizes, R, tops, lefts,
                                                       flips, device)
        desc_dev = torch.frombuffer(desc, dtype=torch.uint8).to(device)                  # one copy
        scratch = torch.empty(scratch_len, dtype=torch.uint8, device=device) if scratch_len else None
        if out is None:
            out = torch.empty(B, 3, R, R, dtype=odt, device=device)
        p = _lib.TrainImagesParams()
        p.images, p.images_bytes = flat.data_ptr(), flat.numel()
        p.desc, p.desc_dev = ctypes.addressof(desc), desc_dev.data_ptr()
        p.tables, p.tables_count = (None, 0) if tables is None else (tables.data_ptr(), tables.numel())
        p.scratch, p.scratch_bytes = (None, 0) if scratch is None else (scratch.data_ptr(), scratch_len)
        p.out, p.B, p.R, p.out_f32 = out.data_ptr(), B, R, int(out_f32)
        _lib.check(lib.aptp_train_images(ctypes.byref(p), _stream()), "aptp_train_images")
    return out


def eos_pool_ln(ids: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5, *,
                eos_mode: str = "argmax", eos_token_id: int = 2, return_index: bool = False):
    """Pooled output of a CLIP text tower: per prompt, LayerNorm of the ONE row of the residual stream x [B, L, C] (bf16 or
    fp32, before final_layer_norm) at the pooling position -- eos_mode "argmax": the first index of the largest id (OpenAI
    encode_text; transformers with eos_token_id == 2); "first_eos": the first index equal to eos_token_id, 0 without one.
    ids int64 [B, L]; gamma / beta fp32 [C].  Returns (fp32 [B, C], the same rows in x's dtype [B, C] for the projection GEMM)
    and, with return_index, the int32 [B] positions."""
    lib = _lib.load()
    if ids.dtype != torch.int64 or ids.dim() != 2 or not ids.is_contiguous() or not ids.is_cuda:
        raise ValueError(f"eos_pool_ln: ids must be a contiguous CUDA int64 [B, L] tensor, got {ids.dtype} {tuple(ids.shape)}")
    B, L = ids.shape
    if x.dtype not in (torch.bfloat16, torch.float32) or x.dim() != 3 or tuple(x.shape[:2]) != (B, L) or x.stride(2) != 1 \
            or x.device != ids.device or B < 1 or L < 1:
        raise ValueError(f"eos_pool_ln: x must be a bf16 or fp32 [{B}, {L}, C] tensor with contiguous channels on {ids.device}, got "
                         f"{x.dtype} {tuple(x.shape)} on {x.device}")
    C = x.shape[2]
    for t, nm in ((gamma, "gamma"), (beta, "beta")):
        if t.dtype != torch.float32 or tuple(t.shape) != (C,) or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"eos_pool_ln: {nm} must be a contiguous fp32 [{C}] tensor on the stream's device")
    modes = {"argmax": EOS_ARGMAX, "first_eos": EOS_FIRST}
    if eos_mode not in modes:
        raise ValueError(f"eos_pool_ln: eos_mode must be one of {sorted(modes)}, got {eos_mode!r}")
    out = torch.empty(B, C, dtype=torch.float32, device=x.device)
    act = torch.empty(B, C, dtype=x.dtype, device=x.device)
    idx = torch.empty(B, dtype=torch.int32, device=x.device) if return_index else None
    p = EosPoolLnParams()
    p.ids, p.x = ids.data_ptr(), x.data_ptr()
    p.x_stride_l = x.stride(1) if L > 1 else max(x.stride(1), C)
    p.x_stride_b = x.stride(0) if B > 1 else L * p.x_stride_l
    p.gamma, p.beta, p.out, p.out_act, p.ldo_act = gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), act.data_ptr(), C
    p.index_out = None if idx is None else idx.data_ptr()
    p.B, p.L, p.C, p.eos_mode, p.eos_token_id = B, L, C, modes[eos_mode], int(eos_token_id)
    p.x_f32 = p.act_f32 = int(x.dtype == torch.float32)
    p.eps = eps
    _lib.check(lib.aptp_eos_pool_ln(ctypes.byref(p), _stream()), "aptp_eos_pool_ln")
    return (out, act, idx) if return_index else (out, act)


def paired_cosine(a: torch.Tensor, b: torch.Tensor, total: Optional[torch.Tensor] = None):
    """fp32 a, b [n, D] -> (cos fp32 [n] with cos[i] = a_i . b_i / (|a_i| |b_i|), their sum as an fp64 scalar tensor).  The sum is
    added in a fixed order: bit-identical from run to run.  total: an fp64 scalar tensor the sum is ADDED to (and which is
    returned), for scores accumulated over chunks."""
    lib = _lib.load()
    for t, nm in ((a, "a"), (b, "b")):
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or not t.is_cuda or t.shape[0] < 1:
            raise ValueError(f"paired_cosine: {nm} must be a contiguous CUDA fp32 [n, D] tensor, got {t.dtype} {tuple(t.shape)}")
    if tuple(a.shape) != tuple(b.shape) or a.shape[1] % 4 != 0 or a.shape[1] < 4 or a.device != b.device:
        raise ValueError(f"paired_cosine: a and b must be equal [n, D] with D a multiple of 4 on one device, got {tuple(a.shape)} and "
                         f"{tuple(b.shape)}")
    if total is not None and (total.dtype != torch.float64 or total.numel() != 1 or total.device != a.device):
        raise ValueError(f"paired_cosine: total must be an fp64 scalar tensor on {a.device}")
    n, D = a.shape
    cos = torch.empty(n, dtype=torch.float32, device=a.device)
    s = torch.empty((), dtype=torch.float64, device=a.device) if total is None else total
    p = PairedCosineParams()
    p.a, p.lda, p.b, p.ldb, p.cos_out, p.sum_out, p.n, p.D = a.data_ptr(), D, b.data_ptr(), D, cos.data_ptr(), s.data_ptr(), n, D
    p.accumulate = int(total is not None)
    _lib.check(lib.aptp_paired_cosine(ctypes.byref(p), _stream()), "aptp_paired_cosine")
    return cos, s


def guided_step(noise: torch.Tensor, sample: torch.Tensor, state: dict, *, scheduler: str, prediction_type: str,
                guidance_scale: float = 1.0, guidance_rescale: float = 0.0, do_cfg: bool = False,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Everything a denoise step does after the U-Net call, in one launch (csrc/sched_step.hip): classifier-free guidance
    ``u + s (t - u)`` on noise [2b, ...] = [uncond; text] (do_cfg; otherwise noise is [b, ...]), the guidance rescale
    (guidance_rescale > 0: the guided output takes the text branch's per-sample standard deviation, blended by that factor)
    and the scheduler update.  noise: bf16 or fp32, contiguous; sample: fp32 [b, ...]; state: the scheduler's per-step
    device tensors (``make_state`` / ``load_step`` of pipeline.DDIMSchedulerLite -- "coef" [4] -- or PNDMSchedulerLite --
    "slot", "w", "coef", "flags", "E", "saved"; E and saved are updated in place -- or DPMSolverMultistepSchedulerLite -- "coef"
    [6], "prev"; prev is updated in place).  scheduler: "ddim", "pndm" or "dpmpp".  Returns the fp32 next sample (``out`` if
    given).  No host synchronisation: safe to capture."""
    lib = _lib.load()
    kinds = {"ddim": _lib.STEP_DDIM, "pndm": _lib.STEP_PNDM, "dpmpp": _lib.STEP_DPMPP}
    preds = {"epsilon": _lib.STEP_EPSILON, "v_prediction": _lib.STEP_V_PREDICTION}
    if scheduler not in kinds:
        raise ValueError(f"guided_step: scheduler must be one of {sorted(kinds)}, got {scheduler!r}")
    if prediction_type not in preds:
        raise ValueError(f"guided_step: prediction_type must be one of {sorted(preds)}, got {prediction_type!r}")
    if sample.dtype != torch.float32 or not sample.is_contiguous() or not sample.is_cuda or sample.dim() < 1 or sample.numel() == 0:
        raise ValueError(f"guided_step: sample must be a contiguous CUDA fp32 [b, ...] tensor, got {sample.dtype} {tuple(sample.shape)}")
    if not noise.is_contiguous() or noise.device != sample.device or noise.dim() != sample.dim() \
            or tuple(noise.shape[1:]) != tuple(sample.shape[1:]):
        raise ValueError(f"guided_step: noise must be contiguous [b or 2b, ...] like sample {tuple(sample.shape)} on {sample.device}, got "
                         f"{tuple(noise.shape)} on {noise.device}")
    b = sample.shape[0]
    n = sample.numel() // b
    if out is None:
        out = torch.empty_like(sample)
    elif out.dtype != torch.float32 or tuple(out.shape) != tuple(sample.shape) or not out.is_contiguous() or out.device != sample.device:
        raise ValueError(f"guided_step: out must be a contiguous fp32 {tuple(sample.shape)} tensor on {sample.device}")
    names = {"ddim": ("coef",), "pndm": ("slot", "w", "coef", "flags", "E", "saved"), "dpmpp": ("coef", "prev")}[scheduler]
    want = {"coef": (torch.float32, {"ddim": 4, "pndm": 2, "dpmpp": 6}[scheduler]), "slot": (torch.int64, 1), "w": (torch.float32, 5),
            "flags": (torch.float32, 2), "E": (torch.float32, 5 * b * n), "saved": (torch.float32, b * n),
            "prev": (torch.float32, b * n)}
    for nm in names:
        t = state.get(nm)
        dt, cnt = want[nm]
        if t is None or t.dtype != dt or t.numel() != cnt or not t.is_contiguous() or t.device != sample.device:
            raise ValueError(f"guided_step: state[{nm!r}] must be a contiguous {dt} tensor of {cnt} elements on {sample.device}")
    p = GuidedStepParams()
    p.noise, p.sample, p.out, p.coef = noise.data_ptr(), sample.data_ptr(), out.data_ptr(), state["coef"].data_ptr()
    if scheduler == "pndm":
        p.slot, p.w, p.flags = state["slot"].data_ptr(), state["w"].data_ptr(), state["flags"].data_ptr()
        p.E, p.saved = state["E"].data_ptr(), state["saved"].data_ptr()
    elif scheduler == "dpmpp":
        p.saved = state["prev"].data_ptr()                   # the previous data prediction travels in ``saved``
    p.n, p.b, p.noise_rows = n, b, noise.shape[0]
    # (a dtype the kernel does not know goes through as such and is refused there)
    p.noise_dtype = {torch.bfloat16: _lib.STEP_NOISE_BF16, torch.float32: _lib.STEP_NOISE_F32}.get(noise.dtype, -1)
    p.scheduler, p.prediction, p.do_cfg = kinds[scheduler], preds[prediction_type], int(bool(do_cfg))
    p.guidance_scale, p.guidance_rescale = float(guidance_scale), float(guidance_rescale)
    _lib.check(lib.aptp_guided_step(ctypes.byref(p), _stream()), "aptp_guided_step")
    return out


def _seed_tensor(seeds, b: int, device, what: str) -> torch.Tensor:
    """seeds of b samples as a device int64 [b] tensor: an int (shared by all samples), b ints, or such a tensor already"""
    if isinstance(seeds, torch.Tensor):
        if seeds.dtype != torch.int64 or seeds.dim() != 1 or not seeds.is_contiguous() or seeds.device != device:
            raise ValueError(f"{what}: seeds must be a contiguous int64 [b] tensor on {device}, got {seeds.dtype} "
                             f"{tuple(seeds.shape)} on {seeds.device}")
        if seeds.shape[0] != b:
            raise ValueError(f"{what}: {seeds.shape[0]} seeds for {b} samples")
        return seeds
    vals = [seeds] * b if isinstance(seeds, int) and not isinstance(seeds, bool) else list(seeds)
    if len(vals) != b:
        raise ValueError(f"{what}: {len(vals)} seeds for {b} samples")
    for v in vals:
        if not isinstance(v, int) or isinstance(v, bool) or not -(1 << 63) <= v < (1 << 64):
            raise ValueError(f"{what}: a seed must be an int in [-2^63, 2^64), got {v!r}")
    # the kernel reads the int64 as uint64: seeds from 2^63 up travel as their two's complement
    return torch.tensor([v - (1 << 64) if v >= (1 << 63) else v for v in vals], dtype=torch.int64, device=device)


def _philox(what, kind, out, base, seeds, draw, draw_dev, offset, scale, scale_dev):
    """the checks every form shares, then the launch; out [b, ...] is fully described by the caller"""
    dev = out.device
    b = out.shape[0]
    n = out.numel() // b
    for name, t, dt in (("draw_dev", draw_dev, torch.int64), ("scale_dev", scale_dev, torch.float32)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or t.numel() != 1 or t.device != dev):
            raise ValueError(f"{what}: {name} must be a {dt} tensor of one element on {dev}")
    if not isinstance(draw, int) or draw < 0 or draw >= (1 << 63):
        raise ValueError(f"{what}: draw must be an int in [0, 2^63), got {draw!r}")
    if not isinstance(offset, int) or offset < 0 or offset > (1 << 62):
        raise ValueError(f"{what}: offset must be an int in [0, 2^62], got {offset!r}")
    if b > 65535 or b * n > (1 << 40):
        raise ValueError(f"{what}: at most 65535 samples and 2^40 elements, got {b} x {n}")
    lib = _lib.load()
    p = PhiloxNormalParams()
    p.out, p.base, p.seeds_dev = out.data_ptr(), None if base is None else base.data_ptr(), seeds.data_ptr()
    p.draw_dev = None if draw_dev is None else draw_dev.data_ptr()
    p.scale_dev = None if scale_dev is None else scale_dev.data_ptr()
    p.n, p.offset, p.draw, p.b, p.out_kind, p.scale = n, offset, draw, b, kind, float(scale)
    _lib.check(lib.aptp_philox_normal(ctypes.byref(p), _stream()), "aptp_philox_normal")
    return out


def _philox_out(what, shape, dtype, out, device, seeds):
    shape = tuple(int(v) for v in shape)
    if len(shape) < 1 or any(v < 1 for v in shape):
        raise ValueError(f"{what}: shape must be [b, ...] with no empty dimension, got {shape}")
    if out is None:
        if device is None:
            device = seeds.device if isinstance(seeds, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"{what}: the generator runs on the GPU, got device {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return shape, None, device
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous() \
            or (device is not None and torch.device(device).type != "cuda"):
        raise ValueError(f"{what}: out must be a contiguous CUDA {dtype} tensor of shape {shape}")
    return shape, out, out.device


def randn(shape, seeds, draw: int = 0, *, offset: int = 0, dtype=torch.float32, scale: float = 1.0,
          out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """Seeded standard normals on the device (csrc/philox_normal.hip): ``scale * z`` of shape [b, ...], where row r's values are
    a pure function of (seeds[r], draw, offset + element index) -- Philox4x32-10 and Box-Muller in fp32, the project's own
    stream (not torch's generator): a row is the same whichever batch it is drawn in.  seeds: an int shared by all samples, b
    ints, or a device int64 [b] tensor.  dtype fp32 or bf16 (the fp32 value rounded).  ``offset`` starts each row's stream that
    many elements in: ``randn((b, n), s)[:, k:] == randn((b, n - k), s, offset=k)``."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"randn: dtype must be torch.float32 or torch.bfloat16, got {dtype}")
    shape, out, dev = _philox_out("randn", shape, dtype, out, device, seeds)
    sd = _seed_tensor(seeds, shape[0], dev, "randn")
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    kind = _lib.PHILOX_F32 if dtype == torch.float32 else _lib.PHILOX_BF16
    return _philox("randn", kind, out, None, sd, draw, None, offset, scale, None)


def philox_bits(shape, seeds, draw: int = 0, *, offset: int = 0, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """The raw form of ``randn``: the uint32 word behind every element, as an int32 tensor holding its bits (view it as
    uint32 on the host)."""
    shape, out, dev = _philox_out("philox_bits", shape, torch.int32, out, device, seeds)
    sd = _seed_tensor(seeds, shape[0], dev, "philox_bits")
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=dev)
    return _philox("philox_bits", _lib.PHILOX_RAW, out, None, sd, draw, None, offset, 1.0, None)


def add_noise(base: torch.Tensor, seeds_dev: torch.Tensor, draw_dev: torch.Tensor, scale_dev: torch.Tensor,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``base + scale_dev * z`` with z = ``randn(base.shape, seeds_dev, draw_dev)``: the capturable form, every scalar in device
    memory (seeds_dev int64 [b], draw_dev int64 [1], scale_dev fp32 [1]), so one captured launch serves every step of a loop.
    base fp32 [b, ...]; a multiply, then an add, as the tensor expression rounds.  Returns ``out`` (a new tensor by default;
    ``out=base`` works in place).  No host synchronisation."""
    if not isinstance(base, torch.Tensor) or base.dtype != torch.float32 or not base.is_cuda or not base.is_contiguous() \
            or base.dim() < 1 or base.numel() == 0:
        raise ValueError("add_noise: base must be a non-empty contiguous CUDA fp32 [b, ...] tensor")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != tuple(base.shape)
                            or not out.is_contiguous() or out.device != base.device):
        raise ValueError(f"add_noise: out must be a contiguous fp32 {tuple(base.shape)} tensor on {base.device}")
    if not isinstance(seeds_dev, torch.Tensor) or draw_dev is None or scale_dev is None:
        raise ValueError("add_noise: seeds_dev, draw_dev and scale_dev must be device tensors")
    sd = _seed_tensor(seeds_dev, base.shape[0], base.device, "add_noise")
    if out is None:
        out = torch.empty_like(base)
    return _philox("add_noise", _lib.PHILOX_F32, out, base, sd, 0, draw_dev, 0, 1.0, scale_dev)


def train_noise(moments: Optional[torch.Tensor] = None, *, latents: Optional[torch.Tensor] = None, sqrt_table: torch.Tensor, seeds,
                draw: int = 0, draw_dev: Optional[torch.Tensor] = None, scale: float = 1.0, noise_offset: float = 0.0,
                input_perturbation: float = 0.0, prediction_type: str = "v_prediction", want_latents: bool = False,
                want_noise: bool = False, out: Optional[dict] = None) -> dict:
    """A seeded training batch in one launch (csrc/train_noise.hip; the draw map and the arithmetic in csrc/train_noise.h, DESIGN
    6m): ``moments`` fp32 [B, 8, h, w] (``vae.encode(x).latent_dist.parameters``; the posterior is sampled here, times ``scale``)
    or ``latents`` fp32 [B, 4, h, w], exactly one of the two; ``sqrt_table`` fp32 [T, 2] (``NoiseSchedule.sqrt_table``; a
    timestep is drawn from its T rows); ``seeds`` as ``randn`` takes them.  Sample r's timestep, noise, offset noise and input
    perturbation are a pure function of (seeds[r], draw + draw_dev[0], element), whatever batch it sits in.  Returns
    {"noisy_latents", "target", "timesteps"} and, when asked for, "latents" (x0) and "noise" (with its offset, without the
    perturbation).  ``out`` is a dict of such tensors to write into; with it, and ``seeds`` / ``draw_dev`` device tensors, the
    call is capturable.  No host synchronisation."""
    what = "train_noise"
    if (moments is None) == (latents is None):
        raise ValueError(f"{what}: give exactly one of moments and latents")
    src, ch = (moments, 8) if moments is not None else (latents, 4)
    if not isinstance(src, torch.Tensor) or src.dtype != torch.float32 or not src.is_cuda or not src.is_contiguous() or src.dim() != 4 \
            or src.shape[1] != ch or src.numel() == 0:
        got = f"{src.dtype} {tuple(src.shape)}" if isinstance(src, torch.Tensor) else type(src).__name__
        raise ValueError(f"{what}: {'moments' if ch == 8 else 'latents'} must be a non-empty contiguous CUDA fp32 [B, {ch}, h, w] "
                         f"tensor, got {got}")
    dev = src.device
    B, _, h, w = (int(v) for v in src.shape)
    if B > 65535:
        raise ValueError(f"{what}: at most 65535 samples, got {B}")
    if not isinstance(sqrt_table, torch.Tensor) or sqrt_table.dtype != torch.float32 or sqrt_table.dim() != 2 or sqrt_table.shape[1] != 2 \
            or sqrt_table.shape[0] < 1 or not sqrt_table.is_contiguous() or sqrt_table.device != dev:
        raise ValueError(f"{what}: sqrt_table must be a contiguous fp32 [T, 2] tensor on {dev}")
    if draw_dev is not None and (not isinstance(draw_dev, torch.Tensor) or draw_dev.dtype != torch.int64 or draw_dev.numel() != 1
                                 or draw_dev.device != dev):
        raise ValueError(f"{what}: draw_dev must be a {torch.int64} tensor of one element on {dev}")
    if not isinstance(draw, int) or isinstance(draw, bool) or draw < 0 or draw >= (1 << 59):
        raise ValueError(f"{what}: draw must be an int in [0, 2^59), got {draw!r}")
    preds = {"epsilon": _lib.TRAIN_NOISE_EPSILON, "v_prediction": _lib.TRAIN_NOISE_V_PREDICTION}
    if prediction_type not in preds:
        raise ValueError(f"{what}: unknown prediction_type {prediction_type!r}")
    for name, v in (("scale", scale), ("noise_offset", noise_offset), ("input_perturbation", input_perturbation)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or abs(v) == float("inf"):
            raise ValueError(f"{what}: {name} must be a finite number, got {v!r}")
    sd = _seed_tensor(seeds, B, dev, what)
    names = ["noisy_latents", "target", "timesteps"] + (["latents"] if want_latents else []) + (["noise"] if want_noise else [])
    if out is not None and (not isinstance(out, dict) or any(nm not in out for nm in names)):
        raise ValueError(f"{what}: out must be a dict with {names}")
    res = {}
    for nm in names:
        shape, dt = ((B,), torch.int64) if nm == "timesteps" else ((B, 4, h, w), torch.float32)
        if out is None:
            res[nm] = torch.empty(shape, dtype=dt, device=dev)
            continue
        t = out[nm]
        if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{what}: out[{nm!r}] must be a contiguous {dt} {shape} tensor on {dev}")
        res[nm] = t
    lib = _lib.load()
    p = TrainNoiseParams()
    p.moments = None if moments is None else moments.data_ptr()
    p.latents_in = None if latents is None else latents.data_ptr()
    p.sqrt_table, p.seeds_dev = sqrt_table.data_ptr(), sd.data_ptr()
    p.draw_dev = None if draw_dev is None else draw_dev.data_ptr()
    p.noisy, p.target, p.timesteps = res["noisy_latents"].data_ptr(), res["target"].data_ptr(), res["timesteps"].data_ptr()
    p.latents_out = res["latents"].data_ptr() if want_latents else None
    p.noise_out = res["noise"].data_ptr() if want_noise else None
    p.draw, p.B, p.h, p.w, p.T, p.prediction = draw, B, h, w, int(sqrt_table.shape[0]), preds[prediction_type]
    p.scale, p.noise_offset, p.input_perturbation = float(scale), float(noise_offset), float(input_perturbation)
    _lib.check(lib.aptp_train_noise(ctypes.byref(p), _stream()), "aptp_train_noise")
    return res


# ------------------------------------------------------------------------------------------------------------------
# backward-path wrappers
# ------------------------------------------------------------------------------------------------------------------
def pack_weight_dgrad(w: torch.Tensor, device=None) -> PackedWeight:
    """Packed weights of the data-gradient contraction: OIHW -> IOHW with the filter rotated by 180 degrees
    (a linear weight [out,in] -> its transpose)."""
    if w.dim() == 2:
        return pack_weight(w.detach().t().contiguous(), None, device=device)
    return pack_weight(w.detach().flip(2, 3).transpose(0, 1).contiguous(), None, device=device)


def _rows(t: torch.Tensor):
    """[B, H, W, C] or [B, L, C] -> (B, rows per sample, C, ld)"""
    if t.dim() == 4:
        return t.shape[0], t.shape[1] * t.shape[2], t.shape[3], _ld(t)
    B, L, C = t.shape
    return B, L, C, (t.stride(1) if L > 1 else max(t.stride(1), C))


def _mse_order(t: torch.Tensor):
    """dimension order that sorts t's strides descending (ties by position): the permutation under which a permuted view --
    the NCHW face of a channels-last activation -- becomes row-major again"""
    return tuple(sorted(range(t.dim()), key=lambda d: (-t.stride(d), d)))


def _mse_view(t: torch.Tensor, order=None):
    """(tensor to keep alive, rows, C, ld) of an operand of aptp_mse: any tensor whose elements, taken in dimension order
    `order`, form rows of C contiguous values at a constant row stride (contiguous tensors, NCHW faces of NHWC activations,
    channel slices of NHWC buffers); anything else is copied once."""
    if order is not None and order != tuple(range(t.dim())):
        t = t.permute(order)
    v = _mse_view_in_place(t)
    return v if v is not None else _mse_view_in_place(t.contiguous())


def _mse_view_in_place(t: torch.Tensor):
    """_mse_view of a tensor already in its memory order, without the copy: None where t has no such view"""
    if t.is_contiguous():
        n = t.numel()
        C = t.shape[-1] if (t.dim() > 1 and t.shape[-1] % 8 == 0) else n
        return t, n // C, C, C
    if t.dim() >= 2 and t.stride(-1) == 1 and t.shape[-1] % 8 == 0:
        ld = t.stride(-2)
        ok = ld % 8 == 0 and ld >= t.shape[-1]
        for d in range(t.dim() - 2, 0, -1):               # outer dimensions must collapse onto the row stride
            ok = ok and t.stride(d - 1) == t.stride(d) * t.shape[d]
        if ok:
            return t, t.numel() // t.shape[-1], t.shape[-1], ld
    return None


def _mse_operands(a: torch.Tensor, b: torch.Tensor):
    order = _mse_order(a)
    a2, rows, C, lda = _mse_view(a, order)
    b2, rows_b, C_b, ldb = _mse_view(b, order)
    if (rows_b, C_b) != (rows, C):                         # different row shapes for the same elements: flatten both
        a2, rows, C, lda = _mse_view(a2.contiguous().reshape(-1))
        b2, _, _, ldb = _mse_view(b2.contiguous().reshape(-1))
    assert C % 8 == 0, "aptp_mse needs a multiple of 8 elements per row"
    return order, a2, b2, rows, C, lda, ldb


def mse(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """mean((a - b)^2) as an fp32 device scalar: two launches, no copies, fixed summation order (csrc/loss_ops.hip)"""
    lib = _lib.load()
    assert a.shape == b.shape and a.dtype == b.dtype and a.dtype in (torch.bfloat16, torch.float32) and a.is_cuda
    _, a, b, rows, C, lda, ldb = _mse_operands(a, b)
    nblk = lib.aptp_mse_nblocks(rows, C)
    partial = torch.empty(nblk, dtype=torch.float32, device=a.device)
    out = torch.empty((), dtype=torch.float32, device=a.device)
    p = MseParams()
    p.a, p.lda, p.b, p.ldb, p.rows, p.C, p.f32 = a.data_ptr(), lda, b.data_ptr(), ldb, rows, C, int(a.dtype == torch.float32)
    p.partial, p.out, p.backward = partial.data_ptr(), out.data_ptr(), 0
    _lib.check(lib.aptp_mse(ctypes.byref(p), _stream()), "aptp_mse")
    return out


def mse_bwd(a: torch.Tensor, b: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """d mean((a - b)^2) / da * g = (a - b) * 2 g / n, in a's dtype, shape AND memory order (the gradient of the NCHW face of
    a channels-last activation is channels-last again, so the next backward kernel takes it without a copy)"""
    lib = _lib.load()
    order, a2, b2, rows, C, lda, ldb = _mse_operands(a, b)
    g = g.detach().to(torch.float32).reshape(1)
    pshape = [a.shape[d] for d in order]
    da = torch.empty(pshape, dtype=a.dtype, device=a.device)
    p = MseParams()
    p.a, p.lda, p.b, p.ldb, p.rows, p.C, p.f32 = a2.data_ptr(), lda, b2.data_ptr(), ldb, rows, C, int(a.dtype == torch.float32)
    p.g, p.da, p.ldda, p.backward = g.data_ptr(), da.data_ptr(), C, 1
    _lib.check(lib.aptp_mse(ctypes.byref(p), _stream()), "aptp_mse(bwd)")
    inv = [0] * len(order)
    for i, d in enumerate(order):
        inv[d] = i
    return da.permute(inv)


@dataclass
class LossTerm:
    """one term of ops.LossTerms: mean((a - b)^2), times `scale`, added to group `group`; per_sample=True makes it the weighted
    term: (1/B) sum_b weights[b] * mean((a[b] - b[b])^2)"""
    a: torch.Tensor
    b: torch.Tensor
    group: int = 0
    scale: float = 1.0
    per_sample: bool = False


class LossTerms:
    """All loss terms of a validation step in three launches (csrc/loss_terms.hip).

    terms: LossTerm objects or (a, b, group[, scale[, per_sample]]) tuples, at most 16.  The operands' views are the ones
    ops.mse(a, b) -- for the per-sample term ops.mse(a[i], b[i]) -- chooses, so every unweighted term and every per-sample mean
    has ops.mse's bits.  An operand ops.mse reads in place is read in place here; one it can only reach through a copy (the
    4-channel NCHW face of a prediction sliced out of 8-wide rows, and the target walked in that order) gets a staging tensor,
    allocated once and refreshed by one `copy_` per run() -- shared by the terms that read the same tensor in the same order.
    No dtype casts are made: a bf16 operand against an fp32 one is read as it is.
    out[g] = sum of value * scale over the terms of group g (divided by group_div[g] where given: the training step's block
    loss is a sum divided by 9), out[G] = sum_g group_coef[g] * out[g].  `weights`: fp32 [B] device vector of the per-sample
    term.  `running`: fp32 [G + 2] totals, running[g] += out[g] and running[G + 1] += 1 on every run(); the caller zeroes it.
    The parameter block is built once: run() is the staging copies and three launches, safe to capture and replay as long as
    the operands, `weights` and `running` stay where they are."""

    def __init__(self, terms, group_coef, weights: Optional[torch.Tensor] = None, running: Optional[torch.Tensor] = None,
                 group_div=None):
        lib = _lib.load()
        terms = [t if isinstance(t, LossTerm) else LossTerm(*t) for t in terms]
        assert 1 <= len(terms) <= _lib.LOSS_TERMS_MAX, f"LossTerms takes 1..{_lib.LOSS_TERMS_MAX} terms"
        G = len(group_coef)
        assert 1 <= G <= _lib.LOSS_TERMS_MAX
        p = LossTermsParams()
        p.n_terms, p.n_groups = len(terms), G
        for g in range(G):
            p.group_coef[g] = float(group_coef[g])
            p.group_div[g] = float(group_div[g]) if group_div is not None else 0.0
        self._keep, self.n_samples = [weights, running], 0
        self._staged, self.copies = {}, []                 # staging tensor by source view; (staging, source) in run() order
        dev = terms[0].a.device
        for i, t in enumerate(terms):
            a, b = t.a, t.b
            assert a.shape == b.shape and a.is_cuda and b.device == a.device
            assert a.dtype in (torch.bfloat16, torch.float32) and b.dtype in (torch.bfloat16, torch.float32)
            q = p.terms[i]
            if t.per_sample:
                B = a.shape[0]
                _, ap, bp, (a2, b2, rows, C, lda, ldb) = self._per_sample_pair(a, b)
                assert weights is not None and weights.dtype == torch.float32 and weights.is_contiguous() \
                    and weights.numel() >= B and weights.device == a.device, "LossTerms: weights = fp32 [B] on the operands' device"
                q.rows, q.rows_per_sample, self.n_samples = rows * B, rows, B
                self._keep += [ap, bp]
            else:
                order = _mse_order(a)
                a2, b2, rows, C, lda, ldb = self._pair(a.permute(order), b.permute(order), stage=True)
                q.rows, q.rows_per_sample = rows, 0
            q.a, q.lda, q.b, q.ldb, q.C = a2.data_ptr(), lda, b2.data_ptr(), ldb, C
            q.a_f32, q.b_f32 = int(a.dtype == torch.float32), int(b.dtype == torch.float32)
            q.group, q.scale = int(t.group), float(t.scale)
            self._keep += [a, b, a2, b2]
        if running is not None:
            assert running.dtype == torch.float32 and running.is_contiguous() and running.numel() >= G + 2 and running.device == dev
        p.w = _ptr(weights)
        p.running = _ptr(running)
        n_scratch = lib.aptp_loss_terms_scratch_floats(ctypes.byref(p))
        if n_scratch <= 0:
            _lib.check(lib.aptp_loss_terms(ctypes.byref(p), None), "aptp_loss_terms")      # (refuses the table with its reason)
        self.n_groups, self.nblocks = G, lib.aptp_loss_terms_nblocks(ctypes.byref(p))
        self.partial = self._alloc(n_scratch, dev)
        self.out = self._alloc(G + 1, dev)
        self.sample_out = self._alloc(self.n_samples, dev) if self.n_samples else None
        p.partial, p.out, p.sample_out = self.partial.data_ptr(), self.out.data_ptr(), _ptr(self.sample_out)
        self.running, self._p, self._lib = running, p, lib

    @staticmethod
    def _alloc(n: int, device) -> torch.Tensor:
        return torch.empty(n, dtype=torch.float32, device=device)

    def _stage(self, src: torch.Tensor) -> torch.Tensor:
        """contiguous staging tensor of the view `src`, refreshed by every run(); one per distinct view"""
        key = (src.data_ptr(), tuple(src.shape), tuple(src.stride()), src.dtype)
        if key not in self._staged:
            self._staged[key] = torch.empty(src.shape, dtype=src.dtype, device=src.device)
            self.copies.append((self._staged[key], src))
        return self._staged[key]

    def _per_sample_pair(self, a: torch.Tensor, b: torch.Tensor):
        """the view of a per-sample term: (order, a permuted, b permuted, _pair of sample 0), every sample in the order
        ops.mse(a[i], b[i]) walks and sample s lying s * rows rows behind sample 0 -- in place where the operands allow it, else
        both whole batches are staged"""
        B = a.shape[0]
        order = (0,) + tuple(d + 1 for d in _mse_order(a[0]))
        ap, bp = a.permute(order), b.permute(order)
        v = self._pair(ap[0], bp[0], stage=False)
        ok = v is not None
        for s in range(1, B if ok else 0):         # sample s lies rows * ld elements behind sample s - 1, in the same view?
            vs = self._pair(ap[s], bp[s], stage=False)
            ok = ok and vs is not None and vs[2:] == v[2:] \
                and vs[0].data_ptr() == v[0].data_ptr() + s * v[2] * v[4] * a.element_size() \
                and vs[1].data_ptr() == v[1].data_ptr() + s * v[2] * v[5] * b.element_size()
        if not ok:                                  # stage both whole batches: sample s = rows s * rows .. of the staging
            ap, bp = self._stage(ap), self._stage(bp)
            v = self._pair(ap[0], bp[0], stage=False)
        return order, ap, bp, v

    def _pair(self, a: torch.Tensor, b: torch.Tensor, stage: bool):
        """_mse_operands for a pair already permuted into the first operand's memory order: (a2, b2, rows, C, lda, ldb) with the
        same row shapes.  Where _mse_operands would copy an operand, `stage` puts a staging tensor in its place; without
        `stage` the answer is None."""
        views = []
        for t in (a, b):
            v = _mse_view_in_place(t)
            if v is None:
                if not stage:
                    return None
                v = _mse_view_in_place(self._stage(t))
            views.append(v)
        (a2, rows, C, lda), (b2, rows_b, C_b, ldb) = views
        if (rows_b, C_b) != (rows, C):                     # different row shapes for the same elements: flatten both
            if not stage and not (a2.is_contiguous() and b2.is_contiguous()):
                return None
            a2, rows, C, lda = _mse_view_in_place((a2 if a2.is_contiguous() else self._stage(a2)).reshape(-1))
            b2, _, _, ldb = _mse_view_in_place((b2 if b2.is_contiguous() else self._stage(b2)).reshape(-1))
        assert C % 8 == 0, "aptp_loss_terms needs a multiple of 8 elements per row"
        return a2, b2, rows, C, lda, ldb

    def run(self) -> torch.Tensor:
        """the staging copies (none for operands ops.mse reads in place) and three launches on the current stream; returns `out`
        ([G + 1]: the groups, then their weighted sum), which the next run() overwrites"""
        for dst, src in self.copies:
            dst.copy_(src)
        _lib.check(self._lib.aptp_loss_terms(ctypes.byref(self._p), _stream()), "aptp_loss_terms")
        return self.out


def loss_terms(terms, group_coef, weights: Optional[torch.Tensor] = None, running: Optional[torch.Tensor] = None, group_div=None):
    """one-off LossTerms(...).run(): (out [G + 1], per-sample means of the weighted term or None)"""
    lt = LossTerms(terms, group_coef, weights, running, group_div)
    return lt.run(), lt.sample_out


class LossStage(LossTerms):
    """The loss stage of a TRAINING step whose batch may be short (csrc/loss_stage.hip): every term per sample, a 0 / 1 mask over
    the samples, the mean over the samples present, and every gradient from one launch.

    terms: LossTerm objects or (a, b, group[, scale[, per_sample]]) tuples, at most 16, all [B, ...] with the same B <= 1024.
    Every term is taken per sample here; `per_sample=True` marks the terms that use `weights` (the min-SNR term), the others
    have weight 1.  The views are the ones ops.mse(a[i], b[i]) chooses (LossTerms' rules, its staging included), so every unit
    has ops.mse's bits.  valid: fp32 [B] of 0 and 1 in any pattern (None: all ones); weights: fp32 [B].
      term_t = (1/n) sum_b valid[b] * w_or_1[b] * mse(a_t[b], b_t[b]),  n = sum_b valid[b];  groups and total as in LossTerms
      out = [G + 2]: the groups, the total, n.  n = 0: zeros.  Samples that are not valid are skipped, whatever their rows hold.
    run() is the staging copies and three launches; backward(g) ONE launch that writes the gradient of `g * total` w.r.t. every
    distinct first operand (a tensor that is the first operand of two terms -- the prediction of the diffusion and of the
    distillation term -- gets one gradient, not two to be summed); rows of samples that are not valid are written as zeros.
    Everything either reads at launch time -- valid, weights, n, g -- is device memory: both are safe to capture and replay while
    the operands stay where they are.  `grad_inputs` are the first operands in the order of `backward`'s list."""

    def __init__(self, terms, group_coef, weights: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None,
                 group_div=None, dense_grads: bool = True):
        lib = _lib.load()
        terms = [t if isinstance(t, LossTerm) else LossTerm(*t) for t in terms]
        assert 1 <= len(terms) <= _lib.LOSS_TERMS_MAX, f"LossStage takes 1..{_lib.LOSS_TERMS_MAX} terms"
        G = len(group_coef)
        assert 1 <= G <= _lib.LOSS_TERMS_MAX
        p = LossStageParams()
        p.n_terms, p.n_groups = len(terms), G
        for g in range(G):
            p.group_coef[g] = float(group_coef[g])
            p.group_div[g] = float(group_div[g]) if group_div is not None else 0.0
        dev, B = terms[0].a.device, int(terms[0].a.shape[0])
        assert 1 <= B <= _lib.LOSS_STAGE_MAX_B, f"LossStage: 1..{_lib.LOSS_STAGE_MAX_B} samples (got {B})"
        if valid is None:
            valid = torch.ones(B, dtype=torch.float32, device=dev)
        for name, v in (("valid", valid), ("weights", weights)):
            assert v is None or (v.dtype == torch.float32 and v.is_contiguous() and v.numel() == B and v.device == dev), \
                f"LossStage: {name} = fp32 [B] on the operands' device"
        self._keep, self.n_samples = [weights, valid], B
        self._staged, self.copies = {}, []
        self.items, by_a = [], {}                          # gradient items: one per distinct first-operand view
        for i, t in enumerate(terms):
            a, b = t.a.detach(), t.b.detach()
            assert a.shape == b.shape and a.is_cuda and b.device == a.device and a.dim() >= 2 and a.shape[0] == B, \
                "LossStage: operands are [B, ...] pairs of one shape"
            assert a.dtype in (torch.bfloat16, torch.float32) and b.dtype in (torch.bfloat16, torch.float32)
            assert not t.per_sample or weights is not None, "LossStage: a per_sample term needs weights"
            order, ap, bp, (a2, b2, rows, C, lda, ldb) = self._per_sample_pair(a, b)
            q = p.terms[i]
            q.a, q.lda, q.b, q.ldb, q.C = a2.data_ptr(), lda, b2.data_ptr(), ldb, C
            q.rows, q.rows_per_sample = rows * B, rows
            q.a_f32, q.b_f32 = int(a.dtype == torch.float32), int(b.dtype == torch.float32)
            q.group, q.scale, q.weighted = int(t.group), float(t.scale), int(bool(t.per_sample))
            self._keep += [a, b, ap, bp, a2, b2]
            key = (a2.data_ptr(), lda, rows, C, a.dtype)
            item = by_a.get(key)
            if item is None:
                assert all(it["src"] is not t.a for it in self.items), \
                    "LossStage: one tensor is read through two different views as a first operand"
                item = by_a[key] = dict(src=t.a, order=order, shape=tuple(ap.shape), dtype=a.dtype, rows=rows * B, C=C, lda=lda, terms=[])
                self.items.append(item)
            assert len(item["terms"]) < 2, "LossStage: a first operand appears in at most two terms"
            item["terms"].append(i)
        p.valid, p.w = valid.data_ptr(), _ptr(weights)
        n_scratch = lib.aptp_loss_stage_scratch_floats(ctypes.byref(p))
        if n_scratch <= 0:
            _lib.check(lib.aptp_loss_stage(ctypes.byref(p), None), "aptp_loss_stage")      # (refuses the table with its reason)
        self.n_groups, self.nblocks = G, lib.aptp_loss_stage_nblocks(ctypes.byref(p))
        self.partial = self._alloc(n_scratch, dev)
        self.out = self._alloc(G + 2, dev)
        self.sample_out = self._alloc(B, dev)
        p.partial, p.out, p.sample_out = self.partial.data_ptr(), self.out.data_ptr(), self.sample_out.data_ptr()
        self.valid, self.weights, self.running = valid, weights, None
        self.dense_grads, self.grads, self._grad_bufs, self._g = bool(dense_grads), None, [], None
        self._p, self._lib = p, lib

    @staticmethod
    def _alloc(n: int, device) -> torch.Tensor:
        return scratch._alloc(n, torch.float32, device, zero=False)

    @staticmethod
    def _alloc_grad(n: int, dtype, device) -> torch.Tensor:
        return scratch._alloc(n, dtype, device, zero=False)

    @property
    def grad_inputs(self):
        return [it["src"] for it in self.items]

    @property
    def total(self) -> torch.Tensor:
        return self.out[self.n_groups]

    @property
    def n_valid(self) -> torch.Tensor:
        """fp32 device scalar: the number of samples the last run() counted"""
        return self.out[self.n_groups + 1]

    def run(self) -> torch.Tensor:
        """the staging copies (none for operands ops.mse reads in place) and three launches on the current stream; returns `out`
        ([G + 2]: the groups, their weighted sum, n), which the next run() overwrites"""
        for dst, src in self.copies:
            dst.copy_(src)
        _lib.check(self._lib.aptp_loss_stage(ctypes.byref(self._p), _stream()), "aptp_loss_stage")
        return self.out

    @property
    def units(self) -> torch.Tensor:
        """fp32 [n_terms, B] view of the scratch: mean((a_t[b] - b_t[b])^2) as the last run() left it, samples that are not valid
        included (whatever their rows gave)"""
        return self.partial[self.nblocks:self.nblocks + self._p.n_terms * self.n_samples].view(self._p.n_terms, self.n_samples)

    def _build_grads(self):
        """the gradient buffers, allocated once: rows of C elements at pitch C (dense_grads) or at the operand's pitch, handed
        out in the first operand's shape and memory order"""
        p, self.grads = self._p, []
        p.n_grads = len(self.items)
        for i, it in enumerate(self.items):
            ld = it["C"] if self.dense_grads else it["lda"]
            buf = self._alloc_grad(it["rows"] * ld, it["dtype"], self.out.device)
            self._grad_bufs.append(buf)
            q = p.grads[i]
            q.grad_out, q.ldg = buf.data_ptr(), ld
            q.term0, q.term1 = it["terms"][0], (it["terms"][1] if len(it["terms"]) > 1 else -1)
            inv = [0] * len(it["order"])
            for j, d in enumerate(it["order"]):
                inv[d] = j
            self.grads.append(buf.view(it["rows"], ld)[:, :it["C"]].view(it["shape"]).permute(inv))

    def backward(self, g: torch.Tensor):
        """ONE launch after run(): the gradients of g * total w.r.t. `grad_inputs`, in that order, each in its operand's dtype, shape
        and memory order; the same tensors on every call.  g: fp32 device scalar."""
        assert g.is_cuda and g.dtype == torch.float32 and g.numel() == 1, "LossStage.backward: g is an fp32 device scalar"
        if self.grads is None:
            self._build_grads()
        self._g = g.detach().reshape(1)
        self._p.g = self._g.data_ptr()
        _lib.check(self._lib.aptp_loss_stage_bwd(ctypes.byref(self._p), _stream()), "aptp_loss_stage_bwd")
        return self.grads


def _check_valid(valid: torch.Tensor, B: int, device, what: str):
    assert valid.dtype == torch.float32 and valid.is_contiguous() and valid.numel() == B and valid.device == device, \
        f"{what}: valid = fp32 [B] on the operands' device"


def sinkhorn_assign(scores: torch.Tensor, valid: torch.Tensor, eps: float, iters: int, out: Optional[torch.Tensor] = None,
                    q: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The quantiser's Sinkhorn assignment over the valid samples of a batch in ONE launch (csrc/router_stage.hip):
    scores fp32 [B, K] (rows at any pitch), valid fp32 [B] of 0 and 1 -> idx int64 [B] (`out` when given).  A sample that is not
    valid gets the argmax of its own raw scores.  q: fp32 [B, K] contiguous, the kernel's workspace and, afterwards, the
    transport plan (zeros on the rows that are not valid); allocated when not given.  Everything is read at launch time: safe to
    capture and replay while scores, valid, out and q stay where they are."""
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and scores.stride(1) == 1, \
        "sinkhorn_assign: scores = fp32 [B, K] with contiguous rows on the GPU"
    B, K = scores.shape
    _check_valid(valid, B, scores.device, "sinkhorn_assign")
    if out is None:
        out = torch.empty(B, dtype=torch.int64, device=scores.device)
    if q is None:
        q = torch.empty((B, K), dtype=torch.float32, device=scores.device)
    assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() == B and out.device == scores.device
    assert q.dtype == torch.float32 and q.is_contiguous() and q.shape == (B, K) and q.device == scores.device
    p = SinkhornParams()
    p.scores, p.ld, p.valid, p.idx, p.q = scores.data_ptr(), (scores.stride(0) if B > 1 else K), valid.data_ptr(), out.data_ptr(), q.data_ptr()
    p.B, p.K, p.iters, p.eps = B, K, int(iters), float(eps)
    _lib.check(_lib.load().aptp_sinkhorn_assign(ctypes.byref(p), _stream()), "aptp_sinkhorn_assign")
    return out


class RouterStage:
    """The router's batch-coupled losses of a pruning step whose batch may be short (csrc/router_stage.hip): the contrastive loss
    and the three MAC losses over the samples present, and their gradients.

    text fp32 [B, D] (no gradient), arch fp32 [B, E] (the width_depth_normalize'd architecture vectors), ratios fp32 [B] (the
    per-sample prunable-MAC ratios), valid fp32 [B] of 0 and 1 in any pattern (None: all ones); B <= 1024, E and D <= 4096.
    The constants are baked in at construction: the two temperatures, the resource target `p` and type ("log" | "mae" | "mse"),
    the four weights.  run() is three launches and returns `out` (fp32 [8]: contrastive, resource, max_loss, std_loss,
    router_loss, mean ratio, n, the number of samples at the maximum); backward(g) two launches that write the gradient of
    g * router_loss as (d_arch [B, E], d_ratios [B]) -- the same tensors on every call, rows of samples that are not valid as
    zeros.  Everything either reads at launch time -- the operands, valid, n, g -- is device memory, and all buffers are allocated
    here, once per object (a captured router builds one per phase; an eager router one per step, on that step's tensors): both are
    safe to capture and replay while the operands stay where they are."""

    def __init__(self, text: torch.Tensor, arch: torch.Tensor, ratios: torch.Tensor, valid: Optional[torch.Tensor] = None, *,
                 arch_temperature: float = 1.0, text_temperature: float = 1.0, p: float = 0.9, resource_type: str = "log",
                 resource_weight: float = 1.0, contrastive_weight: float = 1.0, std_weight: float = 0.0, max_weight: float = 0.0):
        lib = _lib.load()
        self.grad_inputs = [arch, ratios]                  # with their autograd history: what autograd.router_stage applies to
        self.text_requires_grad = bool(text.requires_grad)
        text, arch, ratios = text.detach(), arch.detach(), ratios.detach()
        for name, t in (("text", text), ("arch", arch)):
            assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1, \
                f"RouterStage: {name} = fp32 [B, features] with contiguous rows on the GPU"
        B, E = arch.shape
        D = text.shape[1]
        dev = arch.device
        assert text.shape[0] == B and text.device == dev, "RouterStage: text and arch have one row per sample"
        assert ratios.dtype == torch.float32 and ratios.is_contiguous() and ratios.numel() == B and ratios.device == dev, \
            "RouterStage: ratios = fp32 [B] on the operands' device"
        assert resource_type in _lib.RESOURCE_TYPES, f"RouterStage: unknown resource type {resource_type!r}"
        if valid is None:
            valid = torch.ones(B, dtype=torch.float32, device=dev)
        _check_valid(valid, B, dev, "RouterStage")
        q = RouterStageParams()
        q.text, q.ld_text = text.data_ptr(), (text.stride(0) if B > 1 else D)
        q.arch, q.ld_arch = arch.data_ptr(), (arch.stride(0) if B > 1 else E)
        q.ratios, q.valid = ratios.data_ptr(), valid.data_ptr()
        q.B, q.E, q.D, q.resource_type = B, E, D, _lib.RESOURCE_TYPES[resource_type]
        q.tau_arch, q.tau_text, q.p = float(arch_temperature), float(text_temperature), float(p)
        q.w_resource, q.w_contrastive, q.w_std, q.w_max = float(resource_weight), float(contrastive_weight), float(std_weight), float(max_weight)
        n_work = lib.aptp_router_stage_work_floats(B, E, D)
        self.work = scratch._alloc(max(int(n_work), 1), torch.float32, dev, zero=False)
        self.out = scratch._alloc(8, torch.float32, dev, zero=False)
        self.d_arch = scratch._alloc(B * E, torch.float32, dev, zero=False).view(B, E)
        self.d_ratios = scratch._alloc(B, torch.float32, dev, zero=False).view(ratios.shape)
        q.work, q.out, q.d_arch, q.ld_darch, q.d_ratios = self.work.data_ptr(), self.out.data_ptr(), self.d_arch.data_ptr(), E, self.d_ratios.data_ptr()
        self.text, self.arch, self.ratios, self.valid = text, arch, ratios, valid
        self.B, self.E, self.D = B, E, D
        self._g, self._p, self._lib = None, q, lib

    contrastive = property(lambda self: self.out[0])
    resource = property(lambda self: self.out[1])
    max_loss = property(lambda self: self.out[2])
    std_loss = property(lambda self: self.out[3])
    router_loss = property(lambda self: self.out[4])
    mean_ratio = property(lambda self: self.out[5])
    n_valid = property(lambda self: self.out[6])

    def run(self) -> torch.Tensor:
        """three launches on the current stream; returns `out`, which the next run() overwrites"""
        _lib.check(self._lib.aptp_router_stage(ctypes.byref(self._p), _stream()), "aptp_router_stage")
        return self.out

    def backward(self, g: torch.Tensor):
        """two launches after run(): (d_arch, d_ratios) of g * router_loss.  g: fp32 device scalar."""
        assert g.is_cuda and g.dtype == torch.float32 and g.numel() == 1, "RouterStage.backward: g is an fp32 device scalar"
        self._g = g.detach().reshape(1)
        self._p.g = self._g.data_ptr()
        _lib.check(self._lib.aptp_router_stage_bwd(ctypes.byref(self._p), _stream()), "aptp_router_stage_bwd")
        return self.d_arch, self.d_ratios


def _check_noise_source(what: str, R: int, seeds_dev, draw_dev, sub, device):
    if not isinstance(seeds_dev, torch.Tensor) or not isinstance(draw_dev, torch.Tensor):
        raise ValueError(f"{what}: seeds_dev and draw_dev must be device tensors")
    _seed_tensor(seeds_dev, R, device, what)
    if draw_dev.dtype != torch.int64 or draw_dev.numel() != 1 or draw_dev.device != device:
        raise ValueError(f"{what}: draw_dev must be an int64 tensor of one element on {device}")
    if sub not in (_lib.ROUTER_ASSIGN_SUBDRAW, _lib.ROUTER_RELAX_SUBDRAW):
        raise ValueError(f"{what}: sub must be {_lib.ROUTER_ASSIGN_SUBDRAW} (assignment) or {_lib.ROUTER_RELAX_SUBDRAW} (relaxation), got {sub!r}")


def philox_gumbel(shape, seeds, draw, sub: int, offset: int = 0, *, codebook: bool = False, words: bool = False,
                  out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """The router's seeded Gumbel noise on its own (csrc/gumbel_relax.hip, the stream in csrc/gumbel_relax.h): fp32 [R, n] with
    ``G[r, i] = -log(1e-20 - log(u))``, u the (0, 1] uniform of word ``offset + i`` of (seeds[r], Philox draw), where the Philox
    draw is ``8 * draw + sub`` (sub 6: the assignment's noise, 7: the relaxation's) or, with ``codebook=True``, ``2^63 | draw``.
    seeds as ``randn`` takes them; draw an int in [0, 2^59) or a device int64 [1] tensor (the capturable form).  ``words=True``
    returns the uint32 words behind the values instead, as an int32 tensor holding their bits."""
    shape, out, dev = _philox_out("philox_gumbel", shape, torch.int32 if words else torch.float32, out, device, seeds)
    if len(shape) != 2:
        raise ValueError(f"philox_gumbel: shape must be [R, n], got {shape}")
    R, n = shape
    sd = _seed_tensor(seeds, R, dev, "philox_gumbel")
    if not isinstance(draw, torch.Tensor):
        if not isinstance(draw, int) or isinstance(draw, bool) or not 0 <= draw < (1 << 59):
            raise ValueError(f"philox_gumbel: draw must be an int in [0, 2^59) or a device int64 [1] tensor, got {draw!r}")
        draw = torch.tensor([draw], dtype=torch.int64, device=dev)
    _check_noise_source("philox_gumbel", R, sd, draw, sub, dev)
    if not isinstance(offset, int) or offset < 0 or offset > (1 << 62):
        raise ValueError(f"philox_gumbel: offset must be an int in [0, 2^62], got {offset!r}")
    if out is None:
        out = torch.empty(shape, dtype=torch.int32 if words else torch.float32, device=dev)
    p = PhiloxGumbelParams()
    p.out, p.words = (None, out.data_ptr()) if words else (out.data_ptr(), None)
    p.seeds, p.draw, p.n, p.offset = sd.data_ptr(), draw.data_ptr(), n, offset
    p.R, p.sub, p.codebook = R, int(sub), int(bool(codebook))
    _lib.check(_lib.load().aptp_philox_gumbel(ctypes.byref(p), _stream()), "aptp_philox_gumbel")
    return out


class GumbelRelax:
    """The router's training-mode Gumbel-sigmoid relaxation on seeded device noise, one launch forward and one backward
    (csrc/gumbel_relax.hip; formulas and draw map in csrc/gumbel_relax.h).

    widths: the width segments (their sum nw); depth_order: a permutation of range(nd) (entries are taken mod nd, as the quantiser
    normalises them); rows: R.  The tables, `out` and `dz` (fp32 [R, nw + nd]) are allocated here, once.  run(z, seeds_dev,
    draw_dev, sub, codebook=False) returns `out` = [w | d] of ``gumbel_sigmoid_trick(z)`` with row r's noise a function of
    (seeds_dev[r], draw_dev[0], sub / codebook) alone; backward(dout) returns `dz` for the operands of the last run().  Both read
    z, the seeds and the draw at launch time: safe to capture and replay while those tensors stay where they are."""

    def __init__(self, widths, depth_order, temperature: float, base: float, non_zero_width: bool, rows: int, device):
        self._lib = _lib.load()
        widths = [int(w) for w in widths]
        nd = len(list(depth_order))
        order = [int(o) % nd for o in depth_order]
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"GumbelRelax: the stage runs on the GPU, got device {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        starts = [0]
        for w in widths:
            starts.append(starts[-1] + w)
        self.nw, self.nd, self.R, self.E, self.device = starts[-1], nd, int(rows), starts[-1] + nd, device
        self._seg_host = (ctypes.c_int32 * len(starts))(*starts)
        self._order_host = (ctypes.c_int32 * max(nd, 1))(*(order or [0]))
        p = GumbelRelaxParams()
        p.R, p.nw, p.nd, p.n_seg = self.R, self.nw, nd, len(widths)
        p.non_zero_width, p.T, p.base = int(bool(non_zero_width)), float(temperature), float(base)
        p.sub = _lib.ROUTER_RELAX_SUBDRAW
        p.seg_start_host = ctypes.cast(self._seg_host, ctypes.c_void_p)
        p.depth_order_host = ctypes.cast(self._order_host, ctypes.c_void_p)
        # refuse a bad geometry before anything is allocated for it: the limits are the library's
        if not (1 <= self.R <= _lib.GUMBEL_RELAX_MAX_R and 1 <= self.E <= _lib.GUMBEL_RELAX_MAX_E and nd <= _lib.GUMBEL_RELAX_MAX_ND
                and len(widths) <= _lib.GUMBEL_RELAX_MAX_SEG and all(w >= 1 for w in widths) and sorted(order) == list(range(nd))
                and float(temperature) > 0):
            raise ValueError(f"GumbelRelax: R in 1..{_lib.GUMBEL_RELAX_MAX_R}, nw + nd in 1..{_lib.GUMBEL_RELAX_MAX_E}, at most "
                             f"{_lib.GUMBEL_RELAX_MAX_SEG} non-empty segments, depth_order a permutation of at most "
                             f"{_lib.GUMBEL_RELAX_MAX_ND} entries and a positive temperature; got R = {self.R}, nw = {self.nw}, "
                             f"nd = {nd}, {len(widths)} segments, depth_order = {order}, temperature = {temperature}")
        self.seg_start = torch.tensor(starts, dtype=torch.int32, device=device)
        self.depth_order = torch.tensor(order or [0], dtype=torch.int32, device=device)
        self.out = scratch._alloc(self.R * self.E, torch.float32, device, zero=False).view(self.R, self.E)
        self.dz = scratch._alloc(self.R * self.E, torch.float32, device, zero=False).view(self.R, self.E)
        p.seg_start, p.depth_order = self.seg_start.data_ptr(), self.depth_order.data_ptr()
        p.out, p.dz = self.out.data_ptr(), self.dz.data_ptr()
        self._p, self._keep = p, None

    def _check_rows(self, t, what):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (self.R, self.E) \
                or t.device != self.device:
            raise ValueError(f"GumbelRelax: {what} must be a contiguous fp32 [{self.R}, {self.E}] tensor on {self.device}")

    def run(self, z: torch.Tensor, seeds_dev: torch.Tensor, draw_dev: torch.Tensor, sub: int, codebook: bool = False) -> torch.Tensor:
        """one launch on the current stream; returns `out`, which the next run() overwrites"""
        self.bind(z, seeds_dev, draw_dev, sub, codebook)
        _lib.check(self._lib.aptp_gumbel_relax(ctypes.byref(self._p), _stream()), "aptp_gumbel_relax")
        return self.out

    def bind(self, z, seeds_dev, draw_dev, sub, codebook=False):
        """the operands run() and backward() launch on (run() binds its own; autograd.GumbelRelaxFn re-binds a node's before its
        backward, so two nodes may share a stage as long as each one's `out` is consumed before the next run())"""
        z = z.detach()
        self._check_rows(z, "z")
        _check_noise_source("GumbelRelax", self.R, seeds_dev, draw_dev, sub, self.device)
        p = self._p
        p.z, p.seeds, p.draw, p.sub, p.codebook = z.data_ptr(), seeds_dev.data_ptr(), draw_dev.data_ptr(), int(sub), int(bool(codebook))
        self._keep = (z, seeds_dev, draw_dev, int(sub), bool(codebook))

    def backward(self, dout: torch.Tensor) -> torch.Tensor:
        """one launch after run(): d out / d z applied to dout, for the z, seeds and draw of that run; returns `dz`"""
        if self._keep is None:
            raise RuntimeError("GumbelRelax.backward: call run() first")
        dout = dout.detach()
        self._check_rows(dout, "dout")
        self._p.dout = dout.data_ptr()
        _lib.check(self._lib.aptp_gumbel_relax_bwd(ctypes.byref(self._p), _stream()), "aptp_gumbel_relax_bwd")
        return self.dz


def fold_rows(partials: torch.Tensor, n_rows: int, C: int, out: Optional[torch.Tensor] = None,
              tail_out: Optional[torch.Tensor] = None, deferrable: bool = False, pair_split: bool = False,
              tail_n: int = 0, pair_out=None) -> torch.Tensor:
    """out[row, c] = sum_r partials[r, row, c] (fp32, fixed order); partials is [R, n_rows (+ tail rows), C] contiguous; `out` may
    be a [n_rows, ld >= C] buffer whose extra columns are left alone (the padded packed layout of a weight gradient).
    tail_out (fp32, contiguous, a multiple of C elements): the rows after the first n_rows are summed into it instead -- the
    bias-gradient slabs that ride behind a weight gradient's slabs, folded by the same launch."""
    lib = _lib.load()
    if pair_split and pair_out is not None:
        # (a, b) pairs straight into two existing gradient tensors (direct-gradient mode): a -> pair_out[0], b -> pair_out[1]
        a_t, b_t = pair_out
        assert n_rows == 1 and C % 2 == 0 and a_t.dtype == b_t.dtype == torch.float32 and a_t.is_contiguous() and b_t.is_contiguous() \
            and a_t.numel() >= C // 2 and b_t.numel() >= C // 2
        assert partials.dtype == torch.float32 and partials.is_contiguous() and partials.numel() % C == 0
        p = FoldRowsParams()
        p.partials, p.out, p.R, p.n_rows, p.C, p.ld_out = partials.data_ptr(), a_t.data_ptr(), partials.numel() // C, 1, C, C
        p.tail_out, p.tail_rows, p.pair_split = b_t.data_ptr(), 0, 1
        if FOLD_DEFER is not None and deferrable:
            FOLD_DEFER.append({"params": p, "keep": (partials, a_t, b_t)})
        else:
            _lib.check(lib.aptp_fold_rows(ctypes.byref(p), _stream()), "aptp_fold_rows")
        return None
    if tail_n:
        # the tail destination holds tail_n values (a bias gradient written in place); the slabs carry whole rows of C
        tail_rows = (tail_n + C - 1) // C
        assert tail_out is not None and tail_out.dtype == torch.float32 and tail_out.is_contiguous() and tail_out.numel() >= tail_n
    else:
        tail_rows = 0 if tail_out is None else tail_out.numel() // C
    total_rows = n_rows + tail_rows
    assert partials.dtype == torch.float32 and partials.is_contiguous() and partials.numel() % (total_rows * C) == 0
    R = partials.numel() // (total_rows * C)
    if pair_split:
        # one row of (a, b) pairs -> out [2, half]: a in row 0, b in row 1 (half = C/2 rounded up to 4: both rows 16-byte aligned)
        assert n_rows == 1 and tail_out is None and out is None and C % 2 == 0
        half = round_up(C // 2, 4)
        out = torch.empty(2, half, dtype=torch.float32, device=partials.device)
        o2 = out
    else:
        if out is None:
            out = torch.empty(n_rows, C, dtype=torch.float32, device=partials.device)
        o2 = out.reshape(n_rows, -1)
        assert o2.dtype == torch.float32 and o2.stride(1) == 1 and o2.shape[1] >= C and (n_rows == 1 or o2.stride(0) == o2.shape[1])
    p = FoldRowsParams()
    p.partials, p.out, p.R, p.n_rows, p.C, p.ld_out = partials.data_ptr(), o2.data_ptr(), R, total_rows, C, o2.shape[1]
    if tail_out is not None:
        assert tail_out.dtype == torch.float32 and tail_out.is_contiguous() and (tail_n or tail_out.numel() == tail_rows * C)
        p.tail_out, p.tail_rows, p.tail_n = tail_out.data_ptr(), tail_rows, int(tail_n)
    p.pair_split = int(pair_split)          # (n_rows == 1: out = [C/2 first-of-pair sums | C/2 second-of-pair sums])
    if FOLD_DEFER is not None and deferrable:
        # deferred: the caller of the backward folds everything at once (FoldBatch); `out` is returned UNWRITTEN and must not be
        # read before that (weight / bias gradients: nothing reads them before the optimizer)
        FOLD_DEFER.append({"params": p, "keep": (partials, out, tail_out)})
        return out
    _lib.check(lib.aptp_fold_rows(ctypes.byref(p), _stream()), "aptp_fold_rows")
    return out


# Deferred slab folds.  The weight-gradient kernel splits the pixel range over workgroups and leaves fp32 slabs; summing them is
# one fold launch per weight -- 357 launches of 7.8 us in the expert fine-tune step, 2.8 ms of 39.  Nothing reads a weight (or
# bias) gradient before the optimizer, so with FOLD_DEFER set to a list the folds of a backward pass are only RECORDED (slabs and
# destinations stay referenced, so a capturing allocator cannot hand their memory to a later kernel), and FoldBatch runs them as
# ONE launch over a descriptor table in device memory -- after the replayed graph, next to the one-launch AdamW
# (train_step.GraphedFineTunerStep).  Bitwise the same sums as the single folds (same kernel body, same order).
FOLD_DEFER = None

# Direct parameter gradients (train_step.GraphedFineTunerStep sets it around its warm-up and capture).  The packed trainable
# tensors own PERSISTENT, zero-initialised .grad buffers, and the weight-gradient kernel, the slab folds and the norm-affine
# folds write their results straight into them; the autograd Functions return None for those inputs.  Autograd's
# AccumulateGrad is out of the loop: it clones any incoming gradient another object still references (a recorded, not yet
# executed fold) -- i.e. it would read the buffer BEFORE the fold wrote it -- and each fresh gradient tensor with pad
# columns cost a zero fill per step (80 launches).  Every parameter is used once per step, so "write" equals "accumulate".
GRAD_DIRECT = False

GRAD_ACCUM_MODES = {"store": _lib.GRAD_ACCUM_STORE, "add": _lib.GRAD_ACCUM_ADD, "final": _lib.GRAD_ACCUM_FINAL}


def grad_accumulate(acc: torch.Tensor, g: torch.Tensor, mode) -> None:
    """One launch of the gradient window of train_step.GraphedFineTunerStep(accumulation_steps=N) over two contiguous fp32
    ranges of equal length (csrc/optim.hip): "store" acc <- g (first micro-step: acc is not read), "add" acc <- acc + g,
    "final" g <- acc + g (last micro-step: the sum lands where the exchange and the optimizer read).  Plain fp32 addition:
    torch's ``acc + g`` bit for bit, non-finite values included.  `mode` may also be the integer of the C interface."""
    assert acc.is_cuda and g.is_cuda and acc.device == g.device, "grad_accumulate: device tensors"
    assert acc.dtype == torch.float32 and g.dtype == torch.float32 and acc.is_contiguous() and g.is_contiguous()
    assert acc.numel() == g.numel(), "grad_accumulate: acc and g differ in length"
    q = _lib.GradAccumParams()
    q.acc, q.g, q.n = acc.data_ptr(), g.data_ptr(), acc.numel()
    q.mode = GRAD_ACCUM_MODES[mode] if isinstance(mode, str) else int(mode)
    _lib.check(_lib.load().aptp_grad_accumulate(ctypes.byref(q), _stream()), "aptp_grad_accumulate")


class GradNorm:
    """The global L2 norm of a fixed list of gradient tensors and the clip coefficient of torch.nn.utils.clip_grad_norm_, computed
    and kept on the device (csrc/grad_norm.hip: two launches, fp64 accumulation in a fixed order, the same bits at every replay).
    grads: contiguous, 16-byte aligned fp32 tensors whose addresses stay put (they go into a device table, built here once).
    ``run`` is one call and is capturable; ``out`` = {total_norm, clip_coef, verdict, clipped_count}, with views
      norm     the norm of grad_scale * gradients
      coef     min(1, max_norm / (norm + 1e-6)), exactly 1 without a threshold: what grad_scale_dev of the AdamW passes reads
      verdict  the norm when it and the gate are finite, else NaN: the gate of the optimizer and the EMA
      clipped  calls so far with a finite verdict and coef < 1
    share: another GradNorm whose ``out`` and threshold this one uses (tables over subsets of one optimizer's gradients)."""

    def __init__(self, grads, device=None, max_norm: Optional[float] = None, share: Optional["GradNorm"] = None):
        lib = _lib.load()
        grads = list(grads)
        assert grads, "GradNorm: no gradient tensors"
        device = torch.device(device) if device is not None else grads[0].device
        items = (_lib.GradNormItem * len(grads))()
        for it, g in zip(items, grads):
            assert g.device == device and g.dtype == torch.float32 and g.is_contiguous() and g.numel() >= 1 and g.data_ptr() % 16 == 0, \
                "GradNorm: contiguous, 16-byte aligned fp32 tensors on one device"
            it.g, it.n = g.data_ptr(), g.numel()
        self.grads = grads                        # keeps the addresses in the table alive
        self.table = _lib.BlockTable(items, [lib.aptp_grad_norm_blocks(g.numel()) for g in grads], device)
        self.partials = torch.zeros(self.table.total, dtype=torch.float64, device=device)
        self.out = torch.zeros(4, dtype=torch.float32, device=device) if share is None else share.out
        self.norm, self.coef, self.verdict, self.clipped = self.out[0:1], self.out[1:2], self.out[2:3], self.out[3:4]
        if share is None:
            self.max_norm_dev = torch.full((1,), float("inf"), dtype=torch.float32, device=device)
            self.set_max_norm(max_norm)
        else:
            self.max_norm_dev, self.max_norm = share.max_norm_dev, share.max_norm

    def set_max_norm(self, value: Optional[float]):
        """the threshold, written into device memory: replays of a captured run read it (no recapture).  None: measure only."""
        assert value is None or float(value) > 0.0, "GradNorm: max_norm must be > 0 (None: measure only)"
        self.max_norm = None if value is None else float(value)
        self.max_norm_dev.fill_(float("inf") if value is None else float(value))
        return self

    def run(self, grad_scale: float = 1.0, gate: Optional[torch.Tensor] = None):
        """grad_scale: the scale the optimizer will apply to the gradients (the norm is that of the scaled gradients); gate:
        optional fp32 device scalar (the step's loss).  Returns ``out``."""
        q = _lib.GradNormParams()
        q.items_dev, q.starts_dev, q.n_items, q.total_blocks = self.table.args()
        q.partials_dev, q.grad_scale, q.out_dev = self.partials.data_ptr(), float(grad_scale), self.out.data_ptr()
        q.max_norm_dev = self.max_norm_dev.data_ptr()
        if gate is not None:
            assert gate.dtype == torch.float32 and gate.device == self.out.device and gate.numel() == 1
            q.gate_dev = gate.data_ptr()
        _lib.check(_lib.load().aptp_grad_norm(ctypes.byref(q), _stream()), "aptp_grad_norm")
        return self.out


class FoldBatch:
    def __init__(self, records):
        lib = _lib.load()
        records = list(records)
        assert records
        dev = records[0]["keep"][0].device
        items = (FoldRowsParams * len(records))()
        blocks = []
        for i, rec in enumerate(records):
            ctypes.memmove(ctypes.byref(items[i]), ctypes.byref(rec["params"]), ctypes.sizeof(FoldRowsParams))
            blocks.append(lib.aptp_fold_rows_blocks(ctypes.byref(items[i])))
            assert blocks[-1] > 0
        assert sum(blocks) < 2 ** 31
        self.table = _lib.BlockTable(items, blocks, dev)
        self.keep = [r["keep"] for r in records]

    def run(self):
        _lib.check(_lib.load().aptp_fold_rows_many(*self.table.args(), _stream()), "aptp_fold_rows_many")


# Batched weight gradients (round 3).  Issued layer by layer, each aptp_conv_wgrad launch has to fill the chip on its own: a
# 176 x 176 projection at 16,384 pixels becomes 9 tiles x 57 pixel slices and 57 fp32 slabs to fold.  With WGRAD_DEFER set to a list
# (the graphed fine-tune step, direct-gradient mode) the stride-1 launches of a backward are only recorded -- operands are kept
# alive by the record -- and WgradBatch runs them as one launch per filter size afterwards, slices of ~WGRAD_BATCH_SLICE pixels:
# most weights need no slabs at all and their gradients go straight into the optimizer's buffer.  Run it BEFORE the FoldBatch of
# the same backward (the remaining slabs are folded there).
WGRAD_DEFER = None
WGRAD_SPLIT_RULE = "launch"        # "batch": per-layer launches use the batch's pixel split too (bitwise comparisons with a batched step)
WGRAD_BATCH_SLICE = int(os.environ.get("APTP_WGRAD_BATCH_SLICE", "2048"))


class WgradBatch:
    def __init__(self, records):
        lib = _lib.load()
        records = list(records)
        assert records
        dev = records[0]["keep"][0].device
        nbytes = int(lib.aptp_conv_wgrad_many_item_bytes())
        self.groups = []
        self.keep = [r["keep"] for r in records]
        for taps in (1, 9):
            recs = [r for r in records if r["taps"] == taps]
            if not recs:
                continue
            # long slices first: the short ones (small maps) fill the tail of the grid
            recs.sort(key=lambda r: -((r["params"].B * r["params"].H * r["params"].W) // r["params"].split_m))
            table = (ctypes.c_uint8 * (nbytes * len(recs)))()
            block_item, first = [], 0
            for i, r in enumerate(recs):
                nb = lib.aptp_conv_wgrad_many_blocks(ctypes.byref(r["params"]))
                assert nb > 0
                _lib.check(lib.aptp_conv_wgrad_many_fill(ctypes.byref(r["params"]), ctypes.addressof(table) + i * nbytes, first),
                           "aptp_conv_wgrad_many_fill")
                block_item.append(torch.full((nb,), i, dtype=torch.int32))
                first += nb
            assert first < 2 ** 31
            items = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
            assert items.data_ptr() % 16 == 0
            self.groups.append((taps, items, torch.cat(block_item).to(dev), len(recs), first))

    def run(self):
        lib = _lib.load()
        for taps, items, block_item, n, total in self.groups:
            _lib.check(lib.aptp_conv_wgrad_many(items.data_ptr(), block_item.data_ptr(), n, total, taps, _stream()),
                       "aptp_conv_wgrad_many")

    def launches(self):
        return len(self.groups)


def pack_dgrad_from_packed(pw: PackedWeight, pwb: PackedWeight) -> PackedWeight:
    """refresh the data-gradient operand `pwb` (ops.pack_weight_dgrad layout) from the forward operand `pw` of the same
    weights, bf16 -> bf16, one launch"""
    lib = _lib.load()
    taps = pw.KH * pw.KW
    p = PackDgradParams()
    p.src, p.dst, p.N, p.C, p.taps = pw.w.data_ptr(), pwb.w.data_ptr(), pw.N, pw.Cin, taps
    p.src_ld, p.dst_ld, p.dst_rows = pw.cin_pad, pwb.cin_pad, pwb.N
    assert pwb.KH == pw.KH and pwb.N >= pw.Cin and pwb.cin_pad >= pw.N and pw.Cin2 == 0
    _lib.check(lib.aptp_pack_dgrad(ctypes.byref(p), _stream()), "aptp_pack_dgrad")
    return pwb


class PackDgradBatch:
    """pack_dgrad_from_packed for a fixed list of (forward operand, data-gradient operand) pairs as ONE launch: the
    descriptors live in device memory (built once; the operands' storage must not move afterwards)."""

    def __init__(self, pairs):
        lib = _lib.load()
        pairs = list(pairs)
        assert pairs
        dev = pairs[0][0].w.device
        items = (PackDgradParams * len(pairs))()
        for i, (pw, pwb) in enumerate(pairs):
            assert pwb.KH == pw.KH and pwb.N >= pw.Cin and pwb.cin_pad >= pw.N and pw.Cin2 == 0
            assert pw.cin_pad % 8 == 0 and pwb.cin_pad % 8 == 0 and pw.w.data_ptr() % 16 == 0 and pwb.w.data_ptr() % 16 == 0
            p = items[i]
            p.src, p.dst, p.N, p.C, p.taps = pw.w.data_ptr(), pwb.w.data_ptr(), pw.N, pw.Cin, pw.KH * pw.KW
            p.src_ld, p.dst_ld, p.dst_rows = pw.cin_pad, pwb.cin_pad, pwb.N
        self.table = _lib.BlockTable(items, [lib.aptp_pack_dgrad_blocks(ctypes.byref(p)) for p in items], dev)
        self.keep = pairs
        self.key = tuple((pw.w.data_ptr(), pwb.w.data_ptr()) for pw, pwb in pairs)

    def run(self):
        _lib.check(_lib.load().aptp_pack_dgrad_many(*self.table.args(), _stream()), "aptp_pack_dgrad_many")


def gate_bwd(dy: torch.Tensor, y0: torch.Tensor, gate: torch.Tensor, want_dgate: bool = True):
    """dx = dy * gate (expanded over channel groups, batch tiled), dgate [Bg, G] = sum dy*y0 (fp32).
    want_dgate=False: the forward gate multiply (dy := y0) -- the partials are not folded, dgate is None."""
    lib = _lib.load()
    B, HW, C, lddy = _rows(dy)
    _, _, _, ldy0 = _rows(y0)
    assert dy.dtype == torch.bfloat16 and y0.dtype == torch.bfloat16 and dy.shape == y0.shape
    gate = gate.detach().to(dtype=torch.float32).contiguous()
    Bg, G = gate.shape
    dx = torch.empty_like(dy, memory_format=torch.contiguous_format)
    nchunk = lib.aptp_groupnorm_nchunk(HW)
    part = torch.empty(B, nchunk, G, dtype=torch.float32, device=dy.device)
    dgate = torch.empty(Bg, G, dtype=torch.float32, device=dy.device) if want_dgate else None
    p = GateBwdParams()
    p.dy, p.lddy, p.y0, p.ldy0, p.dx, p.lddx = dy.data_ptr(), lddy, y0.data_ptr(), ldy0, dx.data_ptr(), C
    p.B, p.HW, p.C, p.groups = B, HW, C, G
    p.gate, p.gate_B, p.dgate_partial, p.dgate = gate.data_ptr(), Bg, part.data_ptr(), (dgate.data_ptr() if want_dgate else None)
    _lib.check(lib.aptp_gate_bwd(ctypes.byref(p), _stream()), "aptp_gate_bwd")   # (the partials are folded by the same call)
    return dx, dgate


def geglu_fwd(hg: torch.Tensor, gate: Optional[torch.Tensor]) -> torch.Tensor:
    lib = _lib.load()
    B, HW, C2, ld = _rows(hg)
    C = C2 // 2
    out = torch.empty(*hg.shape[:-1], C, dtype=torch.bfloat16, device=hg.device)
    p = GegluParams()
    p.hg, p.ldhg, p.out, p.ldout = hg.data_ptr(), ld, out.data_ptr(), C
    p.B, p.HW, p.C = B, HW, C
    if gate is not None:
        gate = gate.detach().to(dtype=torch.float32).contiguous()
        p.gate, p.gate_B, p.groups = gate.data_ptr(), gate.shape[0], gate.shape[1]
    else:
        p.groups = 32 if C % 32 == 0 else 1
    p.backward = 0
    _lib.check(lib.aptp_geglu(ctypes.byref(p), _stream()), "aptp_geglu")
    return out


def geglu_bwd(hg: torch.Tensor, dout: torch.Tensor, gate: Optional[torch.Tensor]):
    lib = _lib.load()
    B, HW, C2, ld = _rows(hg)
    C = C2 // 2
    _, _, _, lddout = _rows(dout)
    dhg = torch.empty(*hg.shape, dtype=torch.bfloat16, device=hg.device)
    p = GegluParams()
    p.hg, p.ldhg, p.dout, p.lddout, p.dhg, p.lddhg = hg.data_ptr(), ld, dout.data_ptr(), lddout, dhg.data_ptr(), C2
    p.B, p.HW, p.C = B, HW, C
    Bg, G = (gate.shape if gate is not None else (1, 32 if C % 32 == 0 else 1))
    if gate is not None:
        gate = gate.detach().to(dtype=torch.float32).contiguous()
        p.gate, p.gate_B = gate.data_ptr(), Bg
    p.groups = G
    part = torch.empty(B, lib.aptp_groupnorm_nchunk(HW), G, dtype=torch.float32, device=hg.device)
    p.dgate_partial = part.data_ptr()
    dgate = None
    if gate is not None:
        dgate = torch.empty(Bg, G, dtype=torch.float32, device=hg.device)
        p.dgate = dgate.data_ptr()
    p.backward = 1
    _lib.check(lib.aptp_geglu(ctypes.byref(p), _stream()), "aptp_geglu(bwd)")
    return dhg, dgate


def depth_lerp(x_in: torch.Tensor, x_out: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """DepthGate.forward in one launch: (1 - d[b % dB]) * x_in + d[b % dB] * x_out; x_in may be a channel slice of a wider
    buffer (the un-sliced skip-concat of an up-block resnet, blocks.py:485-495)."""
    lib = _lib.load()
    B, HW, C, ldin = _rows(x_in)
    _, _, _, ldout = _rows(x_out)
    assert x_in.dtype == torch.bfloat16 and x_out.dtype == torch.bfloat16 and x_in.shape == x_out.shape and x_in.is_cuda
    d = d.detach().to(dtype=torch.float32).reshape(-1).contiguous()
    y = torch.empty(x_out.shape, dtype=torch.bfloat16, device=x_out.device)
    p = DepthLerpParams()
    p.x_in, p.ld_in, p.x_out, p.ld_out, p.y, p.ld_y = x_in.data_ptr(), ldin, x_out.data_ptr(), ldout, y.data_ptr(), C
    p.B, p.HW, p.C, p.d, p.d_B, p.backward = B, HW, C, d.data_ptr(), d.numel(), 0
    _lib.check(lib.aptp_depth_lerp(ctypes.byref(p), _stream()), "aptp_depth_lerp")
    return y


def depth_lerp_bwd(dy: torch.Tensor, x_in: torch.Tensor, x_out: torch.Tensor, d: torch.Tensor):
    """(d_in, d_out, dd [dB] fp32) of depth_lerp"""
    lib = _lib.load()
    B, HW, C, ldin = _rows(x_in)
    _, _, _, ldout = _rows(x_out)
    _, _, _, lddy = _rows(dy)
    d = d.detach().to(dtype=torch.float32).reshape(-1).contiguous()
    d_in = torch.empty(x_out.shape, dtype=torch.bfloat16, device=dy.device)
    d_out = torch.empty(x_out.shape, dtype=torch.bfloat16, device=dy.device)
    part = torch.empty(B, lib.aptp_groupnorm_nchunk(HW), dtype=torch.float32, device=dy.device)
    dd = torch.empty(d.numel(), dtype=torch.float32, device=dy.device)
    p = DepthLerpParams()
    p.x_in, p.ld_in, p.x_out, p.ld_out = x_in.data_ptr(), ldin, x_out.data_ptr(), ldout
    p.dy, p.ld_dy, p.d_in, p.ld_d_in, p.d_out, p.ld_d_out = dy.data_ptr(), lddy, d_in.data_ptr(), C, d_out.data_ptr(), C
    p.B, p.HW, p.C, p.d, p.d_B = B, HW, C, d.data_ptr(), d.numel()
    p.dd_partial, p.dd, p.backward = part.data_ptr(), dd.data_ptr(), 1
    _lib.check(lib.aptp_depth_lerp(ctypes.byref(p), _stream()), "aptp_depth_lerp(bwd)")
    return d_in, d_out, dd


def groupnorm_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float,
                  silu: bool, stats: torch.Tensor, C: Optional[int] = None, want_pgrad: bool = False, pgrad_out=None,
                  add: Optional[torch.Tensor] = None):
    """dx (and, with want_pgrad, (dgamma, dbeta) fp32 [C]) of GroupNorm(+SiLU); C = real channel count when the
    tensor is padded to a multiple of 8.  add (bf16, x's shape): the gradient arriving over the residual path that forked
    at x -- summed into dx in fp32 inside the kernel instead of by a separate elementwise launch."""
    lib = _lib.load()
    B, HW, Cp, ldx = _rows(x)
    C = Cp if C is None else C
    _, _, _, lddy = _rows(dy)
    dx = torch.zeros(*x.shape, dtype=torch.bfloat16, device=x.device) if C != Cp else \
        torch.empty(*x.shape, dtype=torch.bfloat16, device=x.device)
    p = GroupNormBwdParams()
    p.x, p.ldx, p.dy, p.lddy, p.dx, p.lddx = x.data_ptr(), ldx, dy.data_ptr(), lddy, dx.data_ptr(), Cp
    p.B, p.HW, p.C, p.groups = B, HW, C, groups
    p.gamma, p.beta, p.eps, p.silu = gamma.data_ptr(), beta.data_ptr(), eps, int(silu)
    p.fwd_stats = stats.data_ptr()
    ws = torch.empty_like(stats)
    p.workspace = ws.data_ptr()
    if add is not None:
        assert add.dtype == torch.bfloat16 and add.shape == x.shape
        p.add, p.ldadd = add.data_ptr(), _rows(add)[3]
    part = None
    if want_pgrad:
        part = torch.empty(B, stats.shape[1], C, 2, dtype=torch.float32, device=x.device)
        p.pgrad_partial = part.data_ptr()
    _lib.check(lib.aptp_groupnorm_bwd(ctypes.byref(p), _stream()), "aptp_groupnorm_bwd")
    if want_pgrad:
        # (dbeta, dgamma) pairs -> two contiguous [C] gradients straight from the fold (was: one [C, 2] tensor + two strided copies)
        if pgrad_out is not None:          # (dgamma, dbeta) destinations: the parameters' own gradient buffers
            fold_rows(part.view(-1, 1, C * 2), 1, C * 2, deferrable=True, pair_split=True, pair_out=(pgrad_out[1], pgrad_out[0]))
            return dx, None, None
        pg = fold_rows(part.view(-1, 1, C * 2), 1, C * 2, deferrable=True, pair_split=True)
        return dx, pg[1, :C], pg[0, :C]
    return dx


def layernorm_pgrad(x: torch.Tensor, dy: torch.Tensor, eps: float = 1e-5, pgrad_out=None):
    """(dgamma, dbeta) fp32 [C] of LayerNorm over the last dim."""
    lib = _lib.load()
    B, L, C, ldx = _rows(x)
    _, _, _, lddy = _rows(dy)
    nchunk = lib.aptp_rows_nchunk(B * L)
    part = torch.empty(nchunk, C, 2, dtype=torch.float32, device=x.device)
    p = LayerNormPgradParams()
    p.x, p.ldx, p.dy, p.lddy, p.rows, p.C, p.eps, p.partial = x.data_ptr(), ldx, dy.data_ptr(), lddy, B * L, C, eps, part.data_ptr()
    _lib.check(lib.aptp_layernorm_pgrad(ctypes.byref(p), _stream()), "aptp_layernorm_pgrad")
    if pgrad_out is not None:
        fold_rows(part.view(-1, 1, C * 2), 1, C * 2, deferrable=True, pair_split=True, pair_out=(pgrad_out[1], pgrad_out[0]))
        return None, None
    pg = fold_rows(part.view(-1, 1, C * 2), 1, C * 2, deferrable=True, pair_split=True)
    return pg[1, :C], pg[0, :C]


def colsum(x: torch.Tensor, per_sample: bool = False) -> torch.Tensor:
    """fp32 column sums of a bf16 [..., C] tensor with contiguous last dim and uniform row stride (bias gradients): [C];
    per_sample: one sum per leading index, [B, C] (the gradient of a per-sample output bias), still two launches."""
    lib = _lib.load()
    C = x.shape[-1]
    B = x.shape[0] if per_sample else 1
    x2 = x.reshape(-1, C)
    rows = x2.shape[0] // B
    nchunk = lib.aptp_groupnorm_nchunk(rows) if B > 1 else lib.aptp_rows_nchunk(rows)
    part = torch.empty(nchunk, B, C, dtype=torch.float32, device=x.device)
    p = ColsumParams()
    p.x, p.ldx, p.rows, p.C, p.partial, p.batch = x2.data_ptr(), (x2.stride(0) if x2.shape[0] > 1 else C), rows, C, part.data_ptr(), B
    _lib.check(lib.aptp_colsum(ctypes.byref(p), _stream()), "aptp_colsum")
    out = fold_rows(part, B, C)
    return out if per_sample else out.view(C)


def layernorm_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, eps: float = 1e-5,
                  add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """add: as in groupnorm_bwd (the residual-path gradient of the fork at x, summed inside the kernel)"""
    lib = _lib.load()
    B, L, C, ldx = _rows(x)
    _, _, _, lddy = _rows(dy)
    dx = torch.empty(*x.shape, dtype=torch.bfloat16, device=x.device)
    p = LayerNormBwdParams()
    p.x, p.ldx, p.dy, p.lddy, p.dx, p.lddx = x.data_ptr(), ldx, dy.data_ptr(), lddy, dx.data_ptr(), C
    p.rows, p.C, p.gamma, p.eps = B * L, C, gamma.data_ptr(), eps
    if add is not None:
        assert add.dtype == torch.bfloat16 and add.shape == x.shape
        p.add, p.ldadd = add.data_ptr(), _rows(add)[3]
    _lib.check(lib.aptp_layernorm_bwd(ctypes.byref(p), _stream()), "aptp_layernorm_bwd")
    return dx


ATTN_BWD_Q_SPLIT = True      # False: never split the dK/dV kernel's query range (A/B timing, tests of both forms)


def attention_bwd(q, k, v, o, dout, lse, heads: int, dq, dk, dv, scale: Optional[float] = None, q_split: Optional[int] = None):
    """dq/dk/dv are preallocated bf16 views (e.g. column slices of one fused gradient buffer), written in place.
    q_split: slices of the query range in the dK/dV kernel (None: the library's rule -- only where few keys leave the chip idle)"""
    lib = _lib.load()
    B, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    delta = torch.empty(B, heads, Lq, dtype=torch.float32, device=q.device)
    p = AttentionBwdParams()
    views = dict(q=q, k=k, v=v, o=o, dout=dout, dq=dq, dk=dk, dv=dv)
    for name, t in views.items():
        assert t.dtype == torch.bfloat16 and t.stride(2) == 1 and t.shape[2] == heads * 64, name
    _set_views(p, **views)
    p.lse, p.delta = lse.data_ptr(), delta.data_ptr()
    p.B, p.heads, p.Lq, p.Lk = B, heads, Lq, Lk
    p.scale = (1.0 / 8.0) if scale is None else scale
    if q_split is None:
        q_split = lib.aptp_attention_bwd_q_split(ctypes.byref(p)) if ATTN_BWD_Q_SPLIT else 1
    ws = None
    if q_split > 1:
        ws = torch.empty(lib.aptp_attention_bwd_workspace_bytes(ctypes.byref(p), q_split), dtype=torch.uint8, device=q.device)
        p.q_split, p.workspace = q_split, ws.data_ptr()
    _lib.check(lib.aptp_attention_bwd(ctypes.byref(p), _stream()), "aptp_attention_bwd")
    return dq, dk, dv


# ------------------------------------------------------------------------------------------------------------------
# weight gradients (expert fine-tuning): dW[n, tap, c] = sum_m dy[m, n] * x[pix(m, tap), c]
# Stride-1 3x3 / 1x1 / linear layers (all but the six down/up-sampler convolutions of SD-2.1) run aptp_conv_wgrad: the
# operands stay in their forward layout and the kernel reads its LDS tiles K-major (transposed LDS reads), one input halo
# per 32-pixel step serving all nine taps.  The remaining geometries fall back to the implicit-GEMM kernel on transposed
# copies ("activations" = dy^T, "weights" = im2col(x)^T; the copies are torch strided copies).
# WGRAD_KERNEL=False forces the fallback everywhere (A/B timing, tests of both forms).
# ------------------------------------------------------------------------------------------------------------------
WGRAD_KERNEL = os.environ.get("APTP_WGRAD_KERNEL", "1") != "0"
WGRAD_SPLIT_TARGET = int(os.environ.get("APTP_WGRAD_SPLIT_TARGET", "0"))
WGRAD_PARITY = True       # _wgrad_parity where its rule selects it (False: copies + GEMM for every resampling convolution)
WGRAD_RESAMPLE = os.environ.get("APTP_WGRAD_RESAMPLE", "1") != "0"    # stride-2 / nearest-x2 3x3 layers through aptp_conv_wgrad itself


def _wgrad_direct(x: torch.Tensor, dy: torch.Tensor, KH: int, KW: int, split_m: Optional[int] = None,
                  out: Optional[torch.Tensor] = None, want_db: bool = False, stride: int = 1, ups: int = 0,
                  db_out: Optional[torch.Tensor] = None):
    """x [B,H,W,C], dy [B,H,W,N] (bf16, channels contiguous, uniform pixel stride) -> fp32 [N, KH*KW, C] or None when
    the geometry is not handled by aptp_conv_wgrad.  out: an fp32 [N, KH*KW, ld >= C] buffer (a packed-layout gradient) that
    receives the result in its first C columns (the rest is left alone); returned instead of a fresh tensor."""
    lib = _lib.load()
    B, C = x.shape[0], x.shape[3]
    H, W, N = dy.shape[1], dy.shape[2], dy.shape[3]           # (the OUTPUT map: the pixels the contraction runs over)
    p = WgradParams()
    p.x, p.ldx, p.dy, p.lddy = x.data_ptr(), _ld(x), dy.data_ptr(), _ld(dy)
    p.B, p.H, p.W, p.C, p.N, p.KH, p.KW = B, H, W, C, N, KH, KW
    p.stride, p.ups = stride, ups
    if x.data_ptr() % 16 or dy.data_ptr() % 16 or not lib.aptp_conv_wgrad_supported(ctypes.byref(p)):
        return None
    _check_act(x, "conv_wgrad x")
    _check_act(dy, "conv_wgrad dy")
    # batched mode (WGRAD_DEFER): the launch is only RECORDED -- every stride-1 weight gradient of the backward runs as one launch
    # per filter size when the backward is complete (WgradBatch), so a pixel slice only has to be worth a workgroup
    defer = WGRAD_DEFER is not None and out is not None and stride == 1 and (not want_db or db_out is not None)
    p.split_m = int(split_m) if split_m else lib.aptp_conv_wgrad_suggest_split(ctypes.byref(p))
    if not split_m and stride == 1 and (defer or WGRAD_SPLIT_RULE == "batch"):
        p.split_m = max(1, min(64, (B * H * W + WGRAD_BATCH_SLICE // 2) // WGRAD_BATCH_SLICE))

    def launch():
        if defer:
            WGRAD_DEFER.append({"params": p, "taps": KH * KW, "keep": (x, dy, out, db_out)})
        else:
            _lib.check(lib.aptp_conv_wgrad(ctypes.byref(p), _stream()), "aptp_conv_wgrad")
    if not split_m and WGRAD_SPLIT_TARGET and not defer and WGRAD_SPLIT_RULE != "batch":
        # (A/B of the pixel-range split: workgroups wanted per launch; the library's own rule is 512)
        tiles = ((N + 63) // 64) * ((C + 63) // 64)
        nsteps = (B * H * W + 31) // 32
        p.split_m = max(1, min(-(-WGRAD_SPLIT_TARGET // tiles), max(1, nsteps // 4), 64))
    if out is not None:
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape[:2]) == (N, KH * KW) and out.shape[2] >= C
    if db_out is not None:
        assert want_db and db_out.dtype == torch.float32 and db_out.is_contiguous() and db_out.numel() >= N
    if p.split_m == 1:
        db = (db_out if db_out is not None else torch.empty(N, dtype=torch.float32, device=x.device)) if want_db else None
        if want_db:
            p.db = db.data_ptr()
        res = out if out is not None else torch.empty(N, KH * KW, C, dtype=torch.float32, device=x.device)
        p.dw, p.ld_dw = res.data_ptr(), res.shape[2]
        launch()
        return (res, db) if want_db else res
    # slabs: [split][N*taps rows of C | ceil(N / C) more rows holding the slice's N bias-gradient sums]; ONE fold for both
    rows, dbrows = N * KH * KW, ((N + C - 1) // C if want_db else 0)
    slabs = torch.empty(p.split_m, rows + dbrows, C, dtype=torch.float32, device=x.device)
    p.dw = slabs.data_ptr()
    tail = None
    if want_db:
        p.slab_stride = (rows + dbrows) * C
        p.db, p.db_stride = slabs.data_ptr() + rows * C * 4, (rows + dbrows) * C
        tail = torch.empty(dbrows * C, dtype=torch.float32, device=x.device) if db_out is None else db_out
    launch()
    if defer:
        WGRAD_DEFER[-1]["keep"] += (slabs,)
    # (tail entries past N are sums of unwritten slab floats: unused, and never written when the destination is db_out)
    res = fold_rows(slabs, rows, C, out=out, tail_out=tail, deferrable=True, tail_n=(N if db_out is not None else 0))
    res = res if out is not None else res.view(N, KH * KW, C)
    return (res, tail[:N]) if want_db else res


def _im2col_T(x: torch.Tensor, KH: int, KW: int, stride: int, pad: int, ups: int) -> torch.Tensor:
    """x [B,H,W,C] bf16 -> [KH*KW*C, M] (M = B*Hout*Wout), taps-major then channels, matching the packed weight order."""
    B, H, W, C = x.shape
    if ups == 1:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        H, W = 2 * H, 2 * W
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    if KH == 1 and KW == 1 and stride == 1 and pad == 0:
        return x.reshape(B * H * W, C).t().contiguous()
    xp = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))
    cols = torch.empty(KH * KW, C, B, Ho, Wo, dtype=x.dtype, device=x.device)
    for ky in range(KH):
        for kx in range(KW):
            v = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride, :]
            cols[ky * KW + kx].copy_(v.permute(3, 0, 1, 2))
    return cols.reshape(KH * KW * C, B * Ho * Wo)


_PARITY_IDX = {}


def _wgrad_parity(x: torch.Tensor, dy: torch.Tensor, stride: int, ups: int, out: Optional[torch.Tensor], want_db: bool):
    """Weight gradient of the six resampling convolutions of the U-Net (3x3 / stride 2 / pad 1 downsamplers; 3x3 on the
    nearest-x2 upsampled input) through the stride-1 kernel.  Splitting the FINE grid by pixel parity turns either one into
    four stride-1 correlations on the coarse grid:
      stride 2:   x[2*oy + ky - 1] = x_p[oy + s],  (p, s) = (1, -1), (0, 0), (1, 0) for ky = 0, 1, 2   (x_p = rows of parity p)
      upsample:   xu[2*i + a + ky - 1] = x[i + s], s = floor((a + ky - 1) / 2): (-1, 0, 0) for a = 0, (0, 0, 1) for a = 1
    and the same along x, so dW[ky][kx] is a gather (stride 2) or a four-term sum (upsample) of taps of the four 3x3 results.
    One parity-split copy of the fine operand replaces nine im2col copies, a transposed dy and a GEMM on them.  Returns None
    when the coarse geometry is not handled by aptp_conv_wgrad."""
    B, H, W, C = x.shape
    N = dy.shape[-1]
    dev = x.device
    if stride == 2:
        if H % 2 or W % 2 or tuple(dy.shape[1:3]) != (H // 2, W // 2):
            return None
        fine, coarse_other = x, dy
    else:
        if tuple(dy.shape[1:3]) != (2 * H, 2 * W):
            return None
        fine, coarse_other = dy, x
    # the four parity planes of the fine operand, contiguous: [2, 2, B, h, w, ch]
    Bf, Hf, Wf, Cf = fine.shape
    planes = fine.reshape(Bf, Hf // 2, 2, Wf // 2, 2, Cf).permute(2, 4, 0, 1, 3, 5).contiguous()
    key = (stride, ups, str(dev))
    idx = _PARITY_IDX.get(key)
    if idx is None:
        if stride == 2:
            par, sh = (1, 0, 1), (0, 1, 1)               # ky -> (parity of the source row, tap row of the stride-1 result)
            dst = {(p_, q_): [] for p_ in (0, 1) for q_ in (0, 1)}
            src = {(p_, q_): [] for p_ in (0, 1) for q_ in (0, 1)}
            for ky in range(3):
                for kx in range(3):
                    dst[(par[ky], par[kx])].append(ky * 3 + kx)
                    src[(par[ky], par[kx])].append(sh[ky] * 3 + sh[kx])
            idx = {k: (torch.tensor(dst[k], device=dev), torch.tensor(src[k], device=dev)) for k in dst}
        else:
            ty = ((0, 1, 1), (1, 1, 2))                  # output-row parity a, ky -> tap row of the stride-1 result
            idx = {(a, b): torch.tensor([ty[a][ky] * 3 + ty[b][kx] for ky in range(3) for kx in range(3)], device=dev)
                   for a in (0, 1) for b in (0, 1)}
        _PARITY_IDX[key] = idx
    dW = torch.zeros(N, 9, C, dtype=torch.float32, device=dev) if stride != 2 else torch.empty(N, 9, C, dtype=torch.float32, device=dev)
    db = None
    for a in (0, 1):
        for b in (0, 1):
            xs, dys = (planes[a, b], coarse_other) if stride == 2 else (coarse_other, planes[a, b])
            first = (a, b) == (0, 0)
            r = _wgrad_direct(xs, dys, 3, 3, want_db=want_db and (first or stride != 2))
            if r is None:
                return None
            if want_db and (first or stride != 2):
                r, dbp = r
                db = dbp if db is None else db + dbp      # upsample: the four parity planes of dy together are dy
            if stride == 2:
                d_i, s_i = idx[(a, b)]
                dW[:, d_i] = r[:, s_i]
            else:
                dW += r[:, idx[(a, b)]]
    if out is not None:
        out[:, :, :C] = dW
        dW = out
    return (dW, db) if want_db else dW


def conv_wgrad(x: torch.Tensor, dy: torch.Tensor, KH: int, KW: int, stride: int = 1, pad: int = 0, ups: int = 0,
               out: Optional[torch.Tensor] = None, want_db: bool = False, db_out: Optional[torch.Tensor] = None):
    """Weight gradient of y = conv(x, w): returns fp32 [N, KH*KW, C] (the packed-weight order, unpadded), or `out` (fp32
    [N, KH*KW, ld >= C], e.g. a zero-initialised packed-layout gradient) with the result in its first C columns.
    x [B,H,W,C] (or tokens [B,L,C] with KH=KW=1), dy [B,Ho,Wo,N] (or [B,L,N]); both bf16.
    want_db: also return the bias gradient (fp32 [N] column sums of dy) -- a by-product of the weight-gradient kernel, which
    stages every dy tile anyway; a separate column-sum pass only on the fallback geometries."""
    if x.dim() == 3:
        # tokens: one image of B*L x 1 "pixels" (a linear layer has no spatial structure)
        x, dy = x.reshape(1, -1, 1, x.shape[-1]), dy.reshape(1, -1, 1, dy.shape[-1])
    C, N = x.shape[-1], dy.shape[-1]
    if WGRAD_KERNEL and stride == 1 and ups == 0 and KH == KW and pad == KH // 2 and x.shape[:3] == dy.shape[:3]:
        g = _wgrad_direct(x, dy, KH, KW, out=out, want_db=want_db, db_out=db_out)
        if g is not None:
            return g
    # the six resampling convolutions of the U-Net (3x3: stride-2 down-samplers, nearest-x2 up-samplers): the same kernel with
    # a strided / up-sampled halo (csrc/wgrad.hip)
    if (WGRAD_KERNEL and WGRAD_RESAMPLE and KH == 3 and KW == 3 and pad == 1 and x.dim() == 4 and x.shape[0] == dy.shape[0]
            and ((stride == 2 and ups == 0 and x.shape[1] == 2 * dy.shape[1] and x.shape[2] == 2 * dy.shape[2])
                 or (stride == 1 and ups == 1 and dy.shape[1] == 2 * x.shape[1] and dy.shape[2] == 2 * x.shape[2]))):
        g = _wgrad_direct(x, dy, KH, KW, out=out, want_db=want_db, stride=stride, ups=ups, db_out=db_out)
        if g is not None:
            return g
    # resampling convolutions: the parity split only pays where the fine grid is large and the weight small -- it runs the
    # nine-tap kernel four times and uses 9 of the 36 tap results (tools/bench_wgrad_resample.py, us, parity vs copies+GEMM:
    # upsample to 64x64 at 640 / 352 channels 449 vs 810 / 259 vs 396; every other resampling layer of SD-2.1 is 1.2-3.5x
    # SLOWER that way, e.g. 704 vs 199 at 8x8 / 1280 channels), so the rule is narrow
    if (WGRAD_KERNEL and WGRAD_PARITY and KH == 3 and KW == 3 and pad == 1 and x.dim() == 4 and stride == 1 and ups == 1
            and dy.shape[0] * dy.shape[1] * dy.shape[2] >= 16384 and x.shape[-1] * dy.shape[-1] <= 640 * 640 and db_out is None):
        g = _wgrad_parity(x, dy, stride, ups, out, want_db)
        if g is not None:
            return g
    xt = _im2col_T(x, KH, KW, stride, pad, ups)                   # [K, M]
    K, M = xt.shape
    dyt = dy.reshape(M, N).t().contiguous()                         # [N, M]
    Mp = round_up(M, BK)
    if Mp != M:                                                     # ragged reduction length (e.g. 4*77 text tokens)
        xt = torch.nn.functional.pad(xt, (0, Mp - M))
        dyt = torch.nn.functional.pad(dyt, (0, Mp - M))
    Kp = round_up(K, 8)
    if Kp != K:
        xt = torch.nn.functional.pad(xt, (0, 0, 0, Kp - K))
    pw = PackedWeight(xt.view(Kp, 1, Mp), None, Kp, Mp, 1, 1)
    Np = round_up(N, 8)
    if Np != N:
        dyt = torch.nn.functional.pad(dyt, (0, 0, 0, Np - N))
    res = conv_gemm(dyt.view(1, Np, 1, Mp), pw, pad=0, out_f32=True, prefetch=False)            # [1, Np, 1, Kp] fp32
    res = res.view(Np, Kp)[:N, :K].reshape(N, KH * KW, C)
    if out is not None:
        out[:, :, :C] = res
        res = out
    if want_db and db_out is not None:
        db_out[:N].copy_(colsum(dy))
        return res, db_out[:N]
    return (res, colsum(dy)) if want_db else res
