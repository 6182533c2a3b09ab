"""fp64 reference, elementwise error bound and a format model of the MFMA contraction kernels behind ops.conv_gemm / ops.linear
(csrc/conv_gemm_core.h, conv_gemm.hip, conv_gemm_sk.hip, lin_gemm.hip, conv_lean.hip) and of the weight-gradient kernel
(csrc/wgrad.hip).  Plain torch, device-agnostic: the host test (tests/test_gemm_model_host.py) runs it on the CPU and proves
that the reference, the bound and the metrics are sound and see seeded defects; the GPU test (tests/test_gemm_parity_gpu.py)
evaluates the SAME functions in fp64 on the device and applies them to the kernels.

Tensors are channels-last, [B, H, W, C], fp64 holding bf16 values (epilogue vectors: fp32 values).  Weights are logical OIHW
[N, Cin, k, k]; a GEGLU projection is [2 * inner, Cin, 1, 1] with the value rows first and the gate rows second, and its output
has ``inner`` columns (the kernels' interleaved packing and padding are a matter of ops.pack_weight, not of the mathematics).

Where the kernels round, and therefore where ``model`` rounds:
  products      bf16 x bf16 is exact in fp32; every K-step is accumulated in fp32 MFMA registers
                (conv_gemm.hip, conv_lean.hip, lin_gemm.hip, conv_gemm_sk.hip: f32x4 acc[MF][NF])
  split-K       slices are stored as fp32 and re-summed in slice order, also in fp32: the row slabs of the reduce launch
                (conv_gemm.hip:240-250, :645-655, :866-876, conv_lean.hip:285-295, summed by splitk_reduce_kernel,
                conv_gemm.hip:897-913), the accumulator-order slabs of the in-kernel form (conv_gemm_core.h:787-830) and the
                stream-K partial tiles (conv_gemm_sk.hip:81, float4 workspace).  No bf16 rounding of a slice anywhere.
  epilogue      bias, rowbias, gate, activation, corr (epilogue_pre, conv_gemm_core.h:127-176), residual and depth lerp
                (epilogue_quad :186-211; coalesced form :560-574; lean 3x3 form :726-758) all in fp32 on the unrounded
                accumulator; the residual is added BEFORE any rounding.  The coalesced forms pass the fp32 value through LDS
                unrounded (:527, :541, :703).
  store         ONE round-to-nearest-even conversion to bf16 (pack_bf16x2, aptp_common.h:41-46, called at
                conv_gemm_core.h:221, :575, :759), or the fp32 value itself when out_f32 (:213-214)
  activations   silu_f = x * rcp(1 + __expf(-x)) (aptp_common.h:65): v_rcp_f32 and v_exp_f32 are 1 ulp each, the argument scaling
                of __expf costs |x| log2(e) ulps more.  gelu_erf_f = x * Phi(x) with Phi by Abramowitz & Stegun 7.1.26
                (aptp_common.h:66-83): |Phi error| <= ~6e-7 ABSOLUTE in fp32, far more than an fp32 rounding -- the one place
                where the kernels are deliberately less exact than fp32, and a term of its own in ``bound``.
  wgrad         fp32 accumulators, fp32 slabs per pixel slice (wgrad.hip:209-221), folded in slice order in fp32 by
                aptp_fold_rows; fp32 output.  The bias gradient is the fp32 column sum of dy (wgrad.hip:204).

Elementwise bound (first order), with u = 2^-24, U_out = 2^-8 for bf16 outputs (half an ulp of a value just above a power of
two is 2^-8 of it) and 2^-24 for fp32 outputs:
    |got - ref| <= U_out |v| + n u S + E
  S  the expression of ``ref64`` evaluated on the absolute values of every term that enters the fp32 accumulator and the
     epilogue (|x| * |w| summed over K, |bias|, |rowbias|, times |gate|, ..., |residual|, |1 - d| |depth_in| + |d| S); through an
     activation S follows its Lipschitz constant (max |silu'| < 1.1, max |gelu'| < 1.13; GEGLU: S_h |gelu(g)| + 1.13 |h| S_g)
  n  the number of such terms: K = taps * Cin + Cin2 products plus 8 epilogue operations (any summation order of n fp32
     additions errs by at most (n - 1) u times the sum of absolute values)
  E  what is not an fp32 rounding: 2^-20 |h g| for the A&S normal CDF (GEGLU / GELU), (3 + 1.5 |h|) u |v| for SiLU's
     exp / rcp, both carried through the later gate / lerp factors.
"""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
CDF_ABS_ERR = 2.0 ** -20            # aptp_common.h:66-67: "~6e-7 in fp32" absolute error of norm_cdf_f
BK = 64                             # K-step of every kernel: channels are zero-padded to it
ACT_NONE, ACT_SILU, ACT_GEGLU = 0, 1, 2

HARD_LIMIT = 1.0
RATIO_LIMIT = 1.25


class Problem:
    """one ops.conv_gemm call; see the module docstring for the conventions"""

    def __init__(self, x, w, bias=None, *, stride=1, pad=None, pad_end=0, ups=0, x2=None, w2=None, rowbias=None, colgate=None,
                 gate_group=0, act=ACT_NONE, corr=None, residual=None, depth=None, depth_in=None, out_f32=False):
        self.x, self.w, self.bias = x, w, bias
        self.k = w.shape[2]
        self.stride, self.pad, self.pad_end, self.ups = stride, (self.k // 2 if pad is None else pad), pad_end, ups
        self.x2, self.w2 = x2, w2
        self.rowbias, self.colgate, self.gate_group, self.act = rowbias, colgate, gate_group, act
        self.corr, self.residual, self.depth, self.depth_in, self.out_f32 = corr, residual, depth, depth_in, out_f32

    @property
    def geometry(self):
        """(B, Hin, Win, HinE, WinE, Hout, Wout): HinE / WinE are the extents the gather walks (doubled by ups)"""
        B, Hin, Win, _ = self.x.shape
        sh = 1 if self.ups else 0
        HinE, WinE = Hin << sh, Win << sh
        Hout = (HinE + 2 * self.pad + self.pad_end - self.k) // self.stride + 1
        Wout = (WinE + 2 * self.pad + self.pad_end - self.k) // self.stride + 1
        return B, Hin, Win, HinE, WinE, Hout, Wout

    @property
    def K(self):
        return self.k * self.k * self.x.shape[3] + (0 if self.x2 is None else self.x2.shape[3])

    @property
    def n_out(self):
        return self.w.shape[0] // 2 if self.act == ACT_GEGLU else self.w.shape[0]

    def to(self, device):
        p = Problem.__new__(Problem)
        for k, v in vars(self).items():
            setattr(p, k, v.to(device) if torch.is_tensor(v) else v)
        return p


# ---------------------------------------------------------------------------------------------------------------------
# the contraction: im2col + matmul
# ---------------------------------------------------------------------------------------------------------------------
def gather_index(prob, _defect=None):
    """[Hout * Wout, taps] indices into the flattened input pixels of one sample, Hin * Win meaning "reads zero"
    (include/aptp_hip.h: pix = (o * stride - pad + k) >> u, zero outside the (up-sampled) extent; ups 2: odd coordinates zero)"""
    B, Hin, Win, HinE, WinE, Hout, Wout = prob.geometry
    k, dev = prob.k, prob.x.device
    oy = torch.arange(Hout, device=dev)[:, None, None, None]
    ox = torch.arange(Wout, device=dev)[None, :, None, None]
    ky = torch.arange(k, device=dev)[None, None, :, None]
    kx = torch.arange(k, device=dev)[None, None, None, :]
    iy = (oy * prob.stride - prob.pad + ky).expand(Hout, Wout, k, k)
    ix = (ox * prob.stride - prob.pad + kx).expand(Hout, Wout, k, k)
    ok = (iy >= 0) & (iy < HinE) & (ix >= 0) & (ix < WinE)
    if prob.ups == 2:
        ok = ok & (iy % 2 == 0) & (ix % 2 == 0)
    sh = 1 if prob.ups else 0
    sy, sx = iy >> sh, ix >> sh
    if _defect == "ups_source_rounds_up" and prob.ups == 1:
        sy, sx = ((iy + 1) >> 1).clamp(max=Hin - 1), ((ix + 1) >> 1).clamp(max=Win - 1)
    idx = torch.where(ok, sy * Win + sx, torch.full_like(sy, Hin * Win))
    if _defect == "right_edge_tap_wraps_to_next_row":
        # the tap one past the right edge, in the last output row, reads the flat successor pixel = first pixel of the next row
        wrap = (~ok) & (ix == WinE) & (iy >= 0) & (iy + 1 < HinE) & (oy == Hout - 1)
        idx = torch.where(wrap, ((iy + 1) >> sh) * Win, idx)
    return idx.reshape(Hout * Wout, k * k)


def im2col(x, prob, _defect=None):
    """x [B, Hin, Win, C] -> [B * Hout * Wout, taps, C] in the kernels' row order (b, oy, ox) and tap order (ky, kx)"""
    B, Hin, Win, C = x.shape
    flat = torch.cat([x.reshape(B, Hin * Win, C), x.new_zeros(B, 1, C)], 1)
    idx = gather_index(prob, _defect)
    return flat[:, idx].reshape(B * idx.shape[0], idx.shape[1], C)


def _operands(prob, _defect=None):
    """A [M, Kp], W [N, Kp] with every tap's channels zero-padded to whole 64-channel K-steps (the packed-weight layout
    [N][taps][cin_pad] + [cin2_pad], ops.pack_weight / pack_weight_cat), and the list of K-step column ranges"""
    x, w = prob.x, prob.w
    N, C, k, _ = w.shape
    cp = -(-C // BK) * BK
    cols = F.pad(im2col(x, prob, _defect), (0, cp - C))                            # [M, taps, cp]
    wm = F.pad(w.permute(0, 2, 3, 1).reshape(N, k * k, C), (0, cp - C))             # [N, taps, cp]
    A, W = cols.reshape(cols.shape[0], -1), wm.reshape(N, -1)
    if prob.x2 is not None:
        C2 = prob.x2.shape[3]
        c2p = -(-C2 // BK) * BK
        a2 = prob.x2.reshape(-1, C2)
        if _defect == "x2_ragged_last_chunk_dropped" and C2 % BK:
            a2 = a2.clone()
            a2[:, C2 // BK * BK:] = 0
        A = torch.cat([A, F.pad(a2, (0, c2p - C2))], 1)
        W = torch.cat([W, F.pad(prob.w2.reshape(N, C2), (0, c2p - C2))], 1)
    return A, W


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _bf_trunc(t):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero): what a store without the rounding add would do"""
    bits = t.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(t.dtype)


def _contract(prob, dtype, split_k=1, _defect=None):
    """sum over K in ``dtype``: one pass, or split_k contiguous ranges of 64-channel K-steps summed in slice order"""
    A, W = _operands(prob, _defect)
    A, W = A.to(dtype), W.to(dtype)
    nK = A.shape[1] // BK
    split_k = max(1, min(split_k, nK))
    if split_k == 1:
        acc = A @ W.t()
    else:
        acc = None
        for z in range(split_k):
            k0, k1 = z * nK // split_k * BK, (z + 1) * nK // split_k * BK
            part = A[:, k0:k1] @ W[:, k0:k1].t()
            if _defect == "splitk_slices_rounded_to_bf16":
                part = _bf(part)
            acc = part if acc is None else acc + part
    if _defect in ("one_chunk_of_one_tap_dropped_in_one_tile", "one_chunk_of_corner_tap_dropped_in_one_fragment"):
        C = prob.x.shape[3]
        cp = -(-C // BK) * BK
        if _defect == "one_chunk_of_one_tap_dropped_in_one_tile":
            # rows 32..63 x columns 32..63 of the output lose one K-step: the centre tap's 4th channel chunk
            tap, r = prob.k * prob.k // 2, slice(32, min(64, acc.shape[0]))
        else:
            # the mildest form of the same loss: one 16-row MFMA fragment (rows 0..15 x columns 32..63) loses the 4th channel chunk
            # of the FIRST tap, which reads padding on the first image row and column -- on an 8 x 8 map 7 of the 16 rows are hit
            tap, r = 0, slice(0, min(16, acc.shape[0]))
        k0 = tap * cp + min(3, cp // BK - 1) * BK
        c = slice(32, min(64, acc.shape[1]))
        acc = acc.clone()
        acc[r, c] -= A[r, k0:k0 + BK] @ W[c, k0:k0 + BK].t()
    return acc


# ---------------------------------------------------------------------------------------------------------------------
# the epilogue, in the order of include/aptp_hip.h (AptpConvGemmParams): bias, rowbias, colgate, act, corr, residual, depth
# ---------------------------------------------------------------------------------------------------------------------
def _gelu(t):
    return t * 0.5 * (1.0 + torch.erf(t * 0.7071067811865476))


def _silu(t):
    return t * torch.sigmoid(t)


def _epilogue(prob, acc, dtype, S=None, _defect=None):
    """acc [M, N] -> (v [M, n_out], S, E).  With ``S`` (the contraction on absolute values) given, S and E of the module
    docstring are carried along; otherwise they come back as None."""
    B, _, _, _, _, Hout, Wout = prob.geometry
    HW, M, N = Hout * Wout, acc.shape[0], acc.shape[1]
    dev = acc.device
    b = torch.arange(M, device=dev) // HW
    track = S is not None
    E = torch.zeros_like(acc) if track else None
    v = acc
    if prob.bias is not None:
        bias = prob.bias.to(dtype)
        if _defect == "bias_missing_on_ragged_last_column_block" and N % 32:
            bias = bias.clone()
            bias[N // 32 * 32:] = 0
        v = v + bias
        if track:
            S = S + prob.bias.abs()
    if prob.rowbias is not None:
        br = b
        if _defect == "rowbias_of_previous_sample_for_the_last" and B > 1:
            br = torch.where(b == B - 1, b - 1, b)
        v = v + prob.rowbias.to(dtype)[br]
        if track:
            S = S + prob.rowbias.abs()[b]
    geglu = prob.act == ACT_GEGLU
    if geglu:
        inner = N // 2
        h, g = v[:, :inner], v[:, inner:]
        if track:
            Sh, Sg = S[:, :inner], S[:, inner:]
            E = E[:, :inner]
    if prob.colgate is not None:
        Bg = prob.colgate.shape[0]
        bg = b % Bg
        if _defect == "colgate_batch_not_tiled":
            bg = b.clamp(max=Bg - 1)
        gm = prob.colgate.to(dtype)[bg].repeat_interleave(prob.gate_group, dim=1)
        if geglu:
            h, g = h * gm, g * gm
        else:
            v = v * gm
        if track:
            ga = prob.colgate.abs()[b % Bg].repeat_interleave(prob.gate_group, dim=1)
            if geglu:
                Sh, Sg = Sh * ga, Sg * ga
            else:
                S = S * ga
    if geglu:
        ge = _gelu(g)
        v = h * ge
        if track:
            S = Sh * ge.abs() + 1.13 * h.abs() * Sg + v.abs()
            E = E + CDF_ABS_ERR * (h * g).abs()
    elif prob.act == ACT_SILU:
        h = v
        v = _silu(h)
        if track:
            S = 1.1 * S + v.abs()
            E = E + (3.0 + 1.5 * h.abs()) * U32 * v.abs()
    if prob.corr is not None:
        rem = torch.arange(M, device=dev) % HW
        oy, ox = rem // Wout, rem % Wout
        rc = torch.where(oy == 0, 0, torch.where(oy == Hout - 1, 2, 1))
        cc = torch.where(ox == 0, 0, torch.where(ox == Wout - 1, 2, 1))
        cls = rc * 3 + cc
        if _defect == "corr_corner_taken_as_bottom_edge":
            cls = torch.where(cls == 8, torch.full_like(cls, 7), cls)
        Bc = prob.corr.shape[0]
        v = v + prob.corr.to(dtype)[b % Bc, cls]
        if track:
            S = S + prob.corr.abs()[b % Bc, cls]
    if prob.residual is not None:
        if _defect == "rounded_to_bf16_before_the_residual":
            v = _bf(v)
        v = v + prob.residual.reshape(M, -1).to(dtype)
        if track:
            S = S + prob.residual.reshape(M, -1).abs()
    if prob.depth is not None:
        d = prob.depth.to(dtype)[b % prob.depth.shape[0]][:, None]
        din = prob.depth_in.reshape(M, -1)
        v = (1.0 - d) * din.to(dtype) + d * v
        if track:
            da = prob.depth[b % prob.depth.shape[0]][:, None]
            S = (1.0 - da).abs() * din.abs() + da.abs() * S
            E = da.abs() * E
    if _defect == "pad_end_ignored" and prob.pad_end:
        # the output extent computed without pad_end: the last output row and column are never written
        rem = torch.arange(M, device=dev) % HW
        last = (rem // Wout == Hout - 1) | (rem % Wout == Wout - 1)
        v = torch.where(last[:, None], torch.zeros_like(v), v)
    return v, S, E


def _shape_out(prob, v):
    B, _, _, _, _, Hout, Wout = prob.geometry
    return v.reshape(B, Hout, Wout, -1)


def ref64(prob):
    """the exact result of ops.conv_gemm on these operands, fp64 [B, Hout, Wout, n_out]"""
    assert prob.x.dtype == torch.float64 and prob.w.dtype == torch.float64
    v, _, _ = _epilogue(prob, _contract(prob, torch.float64), torch.float64)
    return _shape_out(prob, v)


def abs_problem(prob):
    """the same problem with every contraction operand replaced by its absolute value"""
    p = Problem.__new__(Problem)
    for k, val in vars(prob).items():
        setattr(p, k, val)
    p.x, p.w = prob.x.abs(), prob.w.abs()
    if prob.x2 is not None:
        p.x2, p.w2 = prob.x2.abs(), prob.w2.abs()
    return p


def ref_and_bound(prob):
    """(ref64, bound): the reference and the elementwise hard bound of the module docstring, both [B, Hout, Wout, n_out]"""
    acc = _contract(prob, torch.float64)
    S0 = _contract(abs_problem(prob), torch.float64)
    v, S, E = _epilogue(prob, acc, torch.float64, S=S0)
    u_out = U32 if prob.out_f32 else U_BF16
    n = prob.K + 8
    return _shape_out(prob, v), _shape_out(prob, u_out * v.abs() + n * U32 * S + E)


def bound(prob):
    return ref_and_bound(prob)[1]


def model(prob, dtype=torch.float32, split_k=1, _defect=None):
    """The format model: accumulate and run the epilogue in ``dtype`` (fp32 = the kernels; fp64 = the harmless, more exact
    variant), one round-to-nearest-even store.  ``_defect`` seeds one defect of a kind a kernel could have."""
    acc = _contract(prob, dtype, split_k, _defect)
    v, _, _ = _epilogue(prob, acc, dtype, _defect=_defect)
    if prob.out_f32:
        v = v.float()
    elif _defect == "truncating_bf16_store":
        v = _bf_trunc(v)
    else:
        v = _bf(v.float())
    return _shape_out(prob, v.double())


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------
def wgrad_ref64(x, dy, k, stride=1, ups=0, absval=False):
    """dw [N, taps, C] (the packed-weight order) and db [N] of y = conv(x, w) with pad = k // 2, given dy [B, Hout, Wout, N];
    ``absval``: on absolute values (the S of the bound).  The contraction length is B * Hout * Wout."""
    if absval:
        x, dy = x.abs(), dy.abs()
    N = dy.shape[3]
    prob = Problem(x, x.new_zeros(N, x.shape[3], k, k), stride=stride, ups=ups)
    cols = im2col(x, prob)                                   # [M, taps, C]
    dyf = dy.reshape(-1, N)
    assert cols.shape[0] == dyf.shape[0], "dy does not live on this convolution's output map"
    dw = (dyf.t() @ cols.reshape(cols.shape[0], -1)).reshape(N, k * k, -1)
    return dw, dyf.sum(0)


def wgrad_bound(x, dy, k, stride=1, ups=0, split_m=1):
    """fp32 outputs: u |v| for the store of the folded value + (M + split_m) u S for M fp32 accumulations and the slab fold"""
    dw, db = wgrad_ref64(x, dy, k, stride, ups)
    Sw, Sb = wgrad_ref64(x, dy, k, stride, ups, absval=True)
    n = dy.shape[0] * dy.shape[1] * dy.shape[2] + split_m
    return U32 * dw.abs() + n * U32 * Sw, U32 * db.abs() + n * U32 * Sb


# ---------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------
def hard_use(got, ref, bound):
    """max over elements of |got - ref| / bound; <= 1 passes.  Non-finite values, or any error where the bound is zero (an
    output that is exactly representable, such as a column gated to zero), give inf."""
    got = got.to(ref.device, torch.float64)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    diff = (got - ref).abs()
    use = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
    return float(use.max())


def _tile_sums(t, M, N):
    """sum of t over 32 x 32 tiles of its [M, N] view -> [ceil(M/32), ceil(N/32)]"""
    t = t.reshape(M, N)
    t = F.pad(t, (0, -N % 32, 0, -M % 32))
    return t.reshape(t.shape[0] // 32, 32, t.shape[1] // 32, 32).sum(dim=(1, 3))


def tile_ratios(got, model_out, ref, bound):
    """Per 32 x 32 tile of the [B * Hout * Wout, N] view (the kernels' row order): rms(got - ref) / max(rms(model - ref),
    2^-12 rms(bound)).  Ragged last rows / columns form tiles of their own; while a tail strip holds a tile of fewer than 64
    elements it is merged into the strip before it.  The floor covers outputs that are exactly representable (zero format
    error), where only fp32 summation order separates got, model and ref."""
    got = got.to(ref.device, torch.float64)
    N = ref.shape[-1]
    M = ref.numel() // N
    num = _tile_sums((got - ref) ** 2, M, N)
    den = _tile_sums((model_out - ref) ** 2, M, N)
    bnd = _tile_sums(bound ** 2, M, N)
    cnt = _tile_sums(torch.ones_like(ref), M, N)
    while cnt.shape[0] > 1 and float(cnt[-1].min()) < 64:
        num, den, bnd, cnt = (torch.cat([t[:-2], t[-2:].sum(0, keepdim=True)], 0) for t in (num, den, bnd, cnt))
    while cnt.shape[1] > 1 and float(cnt[:, -1].min()) < 64:
        num, den, bnd, cnt = (torch.cat([t[:, :-2], t[:, -2:].sum(1, keepdim=True)], 1) for t in (num, den, bnd, cnt))
    floor = 2.0 ** -12 * (bnd / cnt).sqrt()
    d = torch.maximum((den / cnt).sqrt(), floor)
    r = (num / cnt).sqrt() / d
    return torch.where(num == 0, torch.zeros_like(r), r)


def tile_ratio(got, model_out, ref, bound):
    got = got.to(ref.device, torch.float64)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(tile_ratios(got, model_out, ref, bound).max())


def rel_l2(got, ref):
    """the criterion of tests/test_ops_gpu.py (asserted there at <= 4e-3), for the record of what it would have let through"""
    got = got.to(ref.device, torch.float64)
    return float((got - ref).norm() / (ref.norm() + 1e-30))


# ---------------------------------------------------------------------------------------------------------------------
# cases: the smallest at which each mechanism of the kernels is exercised
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, shape, *, stride=1, pad=None, pad_end=0, ups=0, split_k=None, Cin2=0, dgrad=False, geglu=None,
                 epilogue=None, only_tiles=None, why=""):
        self.name, self.shape = name, tuple(shape)          # shape = (B, H, W, Cin, Cout, k)
        self.stride, self.pad, self.pad_end, self.ups, self.split_k, self.Cin2 = stride, pad, pad_end, ups, split_k, Cin2
        self.dgrad, self.geglu, self.epilogue, self.only_tiles, self.why = dgrad, geglu, epilogue, only_tiles, why

    @property
    def linear(self):
        return self.shape[2] == 1 and self.shape[5] == 1


CASES = [
    Case("ragged-3x7x5x72x40", (3, 7, 5, 72, 40, 3), why="ragged M, N and Cin"),
    Case("padchunk-2x32x32x160x320", (2, 32, 32, 160, 320, 3), why="zero-padded K chunk"),
    Case("stride2-2x16x16x128x128", (2, 16, 16, 128, 128, 3), stride=2, why="downsample"),
    Case("ups1-2x8x8x128x128", (2, 8, 8, 128, 128, 3), ups=1, why="folded nearest x2"),
    Case("dgrad-2x16x16x128x128", (2, 16, 16, 128, 128, 3), stride=2, dgrad=True, why="zero insertion: dgrad of stride 2"),
    Case("1x1-2x16x16x192x128", (2, 16, 16, 192, 128, 1), why="three K-tiles"),
    Case("1x1-2x16x16x64x64", (2, 16, 16, 64, 64, 1), why="one K-tile"),
    Case("splitk4-1x8x8x1280x1280", (1, 8, 8, 1280, 1280, 3), split_k=4, why="explicit split-K"),
    Case("splitk5-1x8x8x1280x1280", (1, 8, 8, 1280, 1280, 3), split_k=5, why="explicit split-K, uneven slices"),
    Case("largestK-1x8x8x2560x1280", (1, 8, 8, 2560, 1280, 3), why="largest K, the library's own split"),
    Case("raggedN-1x24x24x64x200", (1, 24, 24, 64, 200, 3), split_k=3, why="ragged N with split-K"),
    Case("x2-64-2x16x16x320x136", (2, 16, 16, 320, 136, 3), Cin2=64, why="second K segment, one chunk"),
    Case("x2-200-2x16x16x320x136", (2, 16, 16, 320, 136, 3), Cin2=200, why="second K segment, ragged last chunk"),
    Case("zeropage-1x32x32x4160x200", (1, 32, 32, 4160, 200, 1), only_tiles=(0, 2, 6, 64), why="Cin past the zero page"),
    Case("padend-2x16x16x64x64", (2, 16, 16, 64, 64, 3), stride=2, pad=0, pad_end=1, why="pad_end downsampler"),
    Case("lin-7x64x64", (1, 7, 1, 64, 64, 1), why="plain linear, seven rows"),
    Case("lin-130x640x320", (1, 130, 1, 640, 320, 1), why="plain linear, ragged M"),
    Case("lin-308x1024x136", (1, 308, 1, 1024, 136, 1), why="plain linear, ragged M and N"),
    Case("lin-4x320x1280", (1, 4, 1, 320, 1280, 1), why="plain linear, four rows"),
    Case("lin-1000x160x200", (1, 1000, 1, 160, 200, 1), why="plain linear, channel padding in the last K-tile"),
    Case("geglu-2x96x64x256", (2, 96, 1, 64, 512, 1), geglu="gated", why="interleaved GEGLU projection with a width gate"),
    Case("geglu-compact-50x128x512", (1, 50, 1, 128, 1024, 1), geglu="compact", why="compacted GEGLU projection"),
    Case("epi-gate-4x8x8x64x64", (4, 8, 8, 64, 64, 3), epilogue="gate", why="bias + rowbias + colgate, gate batch 2 over B = 4"),
    Case("epi-lerp-4x8x8x64x64", (4, 8, 8, 64, 64, 3), epilogue="lerp", why="corr + residual + depth lerp, depth batch 2"),
    Case("epi-gate-3x7x5x72x40", (3, 7, 5, 72, 40, 3), epilogue="gate1", why="the same on ragged tiles (gate batch 1)"),
    Case("epi-lerp-2x16x16x320x136", (2, 16, 16, 320, 136, 3), epilogue="lerp", why="the same with ragged N"),
    Case("x2-lerp-2x16x16x72x136", (2, 16, 16, 72, 136, 3), Cin2=200, epilogue="lerp", why="second K segment with the lerp epilogue (views)"),
    Case("silu-f32-50x128x96", (1, 50, 1, 128, 96, 1), epilogue="silu_f32", why="SiLU with fp32 output"),
]
CASE_IDS = [c.name for c in CASES]


def case_index(name):
    return CASE_IDS.index(name)


def _randn(shape, g, scale=1.0):
    return torch.randn(shape, generator=g) * scale


def make_problem(index, seed=0):
    """CASES[index] as a Problem on the CPU (fp64 holding bf16 / fp32 values) plus ``extra``: what the GPU test needs besides to
    call ops with the same operands (the un-flipped weight of a dgrad, the live units of a compact GEGLU).  The generator is
    seeded from the case's position, never from hash()."""
    case = CASES[index]
    B, H, W, Cin, Cout, k = case.shape
    g = torch.Generator().manual_seed(7919 * index + 104729 * seed + 1)
    bf = lambda t: t.bfloat16().double()
    f32 = lambda t: t.float().double()
    extra = {}
    if case.dgrad:
        # forward: [B, H, W, Cin] -> stride 2 -> [B, H/2, W/2, Cout]; the problem is its data gradient
        w = bf(_randn((Cout, Cin, k, k), g, 1.0 / math.sqrt(Cin * k * k)))
        dy = bf(_randn((B, H // 2, W // 2, Cout), g))
        extra["w_forward"] = w
        return Problem(dy, w.flip(2, 3).transpose(0, 1).contiguous(), None, stride=1, pad=k - 1 - k // 2, ups=2), extra
    x = bf(_randn((B, H, W, Cin), g))
    w = bf(_randn((Cout, Cin, k, k), g, 1.0 / math.sqrt(Cin * k * k + case.Cin2)))
    bias = f32(_randn((Cout,), g, 0.1))
    kw = dict(stride=case.stride, pad=case.pad, pad_end=case.pad_end, ups=case.ups)
    if case.Cin2:
        kw["x2"] = bf(_randn((B, H, W, case.Cin2), g))
        kw["w2"] = bf(_randn((Cout, case.Cin2), g, 1.0 / math.sqrt(Cin * k * k + case.Cin2)))
        extra["bias2"] = f32(_randn((Cout,), g, 0.1))
        extra["bias1"] = bias
        bias = f32(bias.float() + extra["bias2"].float())            # pack_weight_cat adds the two in fp32
    if case.geglu == "gated":
        inner = Cout // 2
        kw.update(act=ACT_GEGLU, colgate=(torch.rand((B, 32), generator=g) > 0.3).double(), gate_group=inner // 32)
    elif case.geglu == "compact":
        inner = Cout // 2
        keep = torch.arange(inner)[(torch.arange(inner) // 16) % 3 != 1]
        extra.update(keep=keep, w_full=w, bias_full=bias)
        rows = torch.cat([keep, keep + inner])
        w, bias = w[rows], bias[rows]
        kw.update(act=ACT_GEGLU)
    prob = Problem(x, w, bias, **kw)
    _, _, _, _, _, Hout, Wout = prob.geometry
    n_out = prob.n_out
    if case.epilogue in ("gate", "gate1"):
        G = 8 if Cout % 32 else 32
        prob.rowbias = f32(_randn((B, Cout), g, 0.5))
        prob.colgate = f32(torch.rand((2 if case.epilogue == "gate" else 1, G), generator=g))
        prob.gate_group = Cout // G
    elif case.epilogue == "lerp":
        prob.corr = f32(_randn((1, 9, n_out), g, 0.3))
        prob.residual = bf(_randn((B, Hout, Wout, n_out), g))
        prob.depth = f32(torch.rand((2,), generator=g))
        prob.depth_in = bf(_randn((B, Hout, Wout, n_out), g))
    elif case.epilogue == "silu_f32":
        prob.bias, prob.act, prob.out_f32 = None, ACT_SILU, True
    return prob, extra


# seeded defects: name -> (the case it must be caught on, whether the rel-L2 <= 4e-3 criterion is expected to let it through)
DEFECTS = {
    "truncating_bf16_store": "padchunk-2x32x32x160x320",
    "one_chunk_of_one_tap_dropped_in_one_tile": "largestK-1x8x8x2560x1280",
    "one_chunk_of_corner_tap_dropped_in_one_fragment": "largestK-1x8x8x2560x1280",
    "splitk_slices_rounded_to_bf16": "splitk4-1x8x8x1280x1280",
    "rounded_to_bf16_before_the_residual": "epi-lerp-2x16x16x320x136",
    "bias_missing_on_ragged_last_column_block": "ragged-3x7x5x72x40",
    "rowbias_of_previous_sample_for_the_last": "epi-gate-4x8x8x64x64",
    "colgate_batch_not_tiled": "epi-gate-4x8x8x64x64",
    "right_edge_tap_wraps_to_next_row": "ragged-3x7x5x72x40",
    "pad_end_ignored": "padend-2x16x16x64x64",
    "ups_source_rounds_up": "ups1-2x8x8x128x128",
    "corr_corner_taken_as_bottom_edge": "epi-lerp-4x8x8x64x64",
    "x2_ragged_last_chunk_dropped": "x2-200-2x16x16x320x136",
}
# the bias defect on the other two ragged widths the kernels meet (N = 200, 136)
DEFECT_ALSO = {"bias_missing_on_ragged_last_column_block": ("raggedN-1x24x24x64x200", "x2-64-2x16x16x320x136"),
               "truncating_bf16_store": ("largestK-1x8x8x2560x1280", "ragged-3x7x5x72x40")}
OLD_CRITERION_MUST_PASS = ("truncating_bf16_store", "one_chunk_of_corner_tap_dropped_in_one_fragment")
OLD_REL_L2_TOL = 4e-3
