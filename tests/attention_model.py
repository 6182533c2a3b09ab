"""fp64 reference, elementwise error bounds and a bf16 format model of the U-Net attention kernels (csrc/attention.hip forward
with log-sum-exp, csrc/attention_bwd.hip backward).  Plain torch on the CPU; shared by tests/test_attention_model_host.py
(which proves that the reference, the bounds and the metrics are sound and see seeded defects) and
tests/test_attention_grad_gpu.py (which applies them to the kernels).

Tensors are [B, heads, L, 64] here; ``to_heads`` / ``from_heads`` convert from / to the kernels' [B, L, heads*64].

Where the kernels round (head_dim 64, bf16 operands, fp32 accumulation), and therefore where ``model`` rounds:
  forward   S = Q K^T in fp32; p = exp2(S*c - m), c = scale*log2(e)          attention.hip:219-225 (:470, :715-716)
            row sum l over the UNROUNDED fp32 p                              attention.hip:226-230 (:472-475, :717, :769)
            p -> bf16 as the operand of P.V                                  attention.hip:246 (:493, :718)
            o = (P.V) / l -> bf16                                            attention.hip:296-306 (:540-550, :836-846)
            lse = m + log2(l) in fp32                                        attention.hip:295 (:539, :835)
  backward  delta = sum_d dO*O over the bf16 forward output, fp32            attention_bwd.hip:47-54
            P = exp2(fma(S, c, -lse)) from the forward's lse                 attention_bwd.hip:162, :272
            dS = P*(dP - delta) with the unrounded fp32 P, then dS -> bf16   attention_bwd.hip:163,169, :274,281
            P -> bf16 as the operand of P^T dO                               attention_bwd.hip:281
            dq = scale*(dS K) -> bf16; dk = scale*(dS^T Q), dv -> bf16       attention_bwd.hip:184, :311-315 (split: :298-300, :336-338)

Elementwise bounds with u = 2^-8, the unit roundoff of bf16 (first order in u; P, o, dS, dq, dk, dv are the exact fp64 values):
  b_o   = u (P |V| + |o|)                      each p is off by <= u p before P.V; the output is rounded once
  A_q   = sum_d |dO_qd| (P |V| + |o|)_qd       |delta_q - exact| <= u A_q, because delta is taken from the bf16 o
  b_dv  = u (P^T |dO| + |dv|)
  b_dS  = u (P o A + |dS|)                     the delta error times P, then the bf16 rounding of dS itself
  b_dq  = scale b_dS |K| + u |dq|
  b_dk  = scale b_dS^T |Q| + u |dk|
  b_lse = 2^-18 (c max_j sum_d |q_d||k_jd| + |lse| + 1) + 2^-23 Lk
          64 fp32 products per score (64 * 2^-24 = 2^-18 of the absolute sum), the fp32 roundings of m, log2 l and their sum, and
          Lk fp32 additions plus one hardware exp2 (1 ulp) per term of the row sum (log2(e) * Lk * 2^-24 < 2^-23 Lk)
The hard check is |got - ref| <= (1 + 2^-6) b + 2^-20 rms(ref) for EVERY element: 2^-6 = 4u covers the second-order terms (the
backward runs on the forward's rounded lse and o; u^2 cross terms), 2^-20 rms(ref) the fp32 accumulation of up to a few thousand
terms.
"""
import math

import torch

U = 2.0 ** -8
LOG2E = 1.4426950408889634
KEYS = ("o", "lse", "dq", "dk", "dv")
RATIO_KEYS = ("o", "dq", "dk", "dv")          # per-block ratio against the format model; lse has no bf16 rounding to model


def to_heads(t, heads):
    """[B, L, heads*64] -> [B, heads, L, 64]"""
    B, L, _ = t.shape
    return t.reshape(B, L, heads, 64).transpose(1, 2)


def from_heads(t):
    """[B, heads, L, 64] -> [B, L, heads*64] contiguous"""
    B, h, L, _ = t.shape
    return t.transpose(1, 2).reshape(B, L, h * 64).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# cases: (B, heads, Lq, Lk), all head_dim 64 -- the smallest shapes that reach each code path of the kernels
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, shape, scale=None, spike=0.0, amp=1.0, why=""):
        self.shape, self.scale, self.spike, self.amp, self.why = tuple(shape), scale, spike, amp, why
        self.smooth = scale is None and spike == 0.0          # the per-block ratio is asserted on smooth cases only

    @property
    def id(self):
        s = "x".join(str(n) for n in self.shape)
        if self.scale is not None:
            s += f"-scale{self.scale:g}"
        if self.spike:
            s += f"-spike{self.spike:g}"
        return s

    @property
    def eff_scale(self):
        return 0.125 if self.scale is None else self.scale


# amp: q and k are scaled by 2 in half of the cases (scores of standard deviation 4 instead of 1: a peaked softmax).  Which half
# was decided by the reference alone (test_attention_model_host.py): at amplitude 2 the error of a block with few rows, or of a
# dK block under 2048 keys, is dominated by a handful of roundings and the ratio between two sound forms of the model reaches
# 3-5 there (1x77, row 128 of 129, 100x2048/2077, 200x77: 1.85); those cases run at amplitude 1, where it stays below 1.35.
CASES = [
    Case((1, 1, 1, 1), amp=2.0, why="degenerate lengths"),
    Case((2, 2, 1, 77), why="degenerate query length, cross-attention keys"),
    Case((2, 2, 16, 16), amp=2.0, why="mid-block attention at 32x32 latents: below one tile on both sides"),
    Case((1, 2, 129, 65), why="one past each tile edge"),
    Case((2, 3, 200, 77), why="cross-attention, ragged on both sides"),
    Case((1, 2, 384, 320), amp=2.0, why="five key tiles over two wave groups (3 + 2)"),
    Case((1, 2, 256, 256), amp=2.0, why="smallest shape of the software-pipelined kernel"),
    Case((1, 1, 100, 2048), why="double-buffered kernel as auto selects it, ragged queries"),
    Case((1, 1, 100, 2077), why="double-buffered kernel as auto selects it, ragged queries and keys"),
    Case((1, 2, 1024, 77), amp=2.0, why="the library's own q_split (8)"),
    Case((1, 2, 256, 256), spike=6.0, why="one key x6: peaked softmax"),
    Case((1, 2, 256, 256), spike=30.0, amp=2.0, why="one key x30: one-hot softmax"),
    Case((2, 2, 192, 77), scale=0.3, amp=2.0, why="explicit scale, peaked"),
    Case((2, 2, 192, 77), scale=0.05, why="explicit scale, flat"),
]


def make_inputs(index, seed=0):
    """q, k, v, do as fp64 [B, heads, L, 64] holding bf16 values.  The generator is seeded from the case's position in CASES (not
    from hash(), which differs between interpreter runs for some types); q and k are scaled by the case's amp."""
    case = CASES[index]
    B, h, Lq, Lk = case.shape
    g = torch.Generator().manual_seed(7919 * index + 104729 * seed + 1)
    amp = case.amp
    q = torch.randn(B, h, Lq, 64, generator=g) * amp
    k = torch.randn(B, h, Lk, 64, generator=g) * amp
    v = torch.randn(B, h, Lk, 64, generator=g)
    do = torch.randn(B, h, Lq, 64, generator=g)
    if case.spike:
        k[:, :, (Lk * 2) // 3] *= case.spike
    return tuple(t.bfloat16().double() for t in (q, k, v, do))


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def ref64(q, k, v, do, scale):
    """All fp64, closed forms of the header of csrc/attention_bwd.hip.  Returns (out, bound): dicts over KEYS; lse is in the log2
    domain of the scaled scores, as the kernels define it."""
    assert all(t.dtype == torch.float64 for t in (q, k, v, do))
    Lk = k.shape[2]
    c = scale * LOG2E
    x = (q @ k.transpose(-1, -2)) * scale
    lse_nat = torch.logsumexp(x, dim=-1)
    P = torch.exp(x - lse_nat[..., None])
    o = P @ v
    delta = (do * o).sum(-1)
    dv = P.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    dS = P * (dP - delta[..., None])
    dq = scale * (dS @ k)
    dk = scale * (dS.transpose(-1, -2) @ q)
    lse = lse_nat * LOG2E
    out = {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}

    po = P @ v.abs() + o.abs()
    A = (do.abs() * po).sum(-1)
    b_dS = U * (P * A[..., None] + dS.abs())
    bound = {
        "o": U * po,
        "dv": U * (P.transpose(-1, -2) @ do.abs() + dv.abs()),
        "dq": scale * (b_dS @ k.abs()) + U * dq.abs(),
        "dk": scale * (b_dS.transpose(-1, -2) @ q.abs()) + U * dk.abs(),
        "lse": 2.0 ** -18 * (c * (q.abs() @ k.abs().transpose(-1, -2)).amax(-1) + lse.abs() + 1.0) + 2.0 ** -23 * Lk,
    }
    return out, bound


# ---------------------------------------------------------------------------------------------------------------------
# format model
# ---------------------------------------------------------------------------------------------------------------------
def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def model(q, k, v, do, scale, dtype, shift=0.0, _defect=None):
    """The same computation with bf16 roundings exactly where the kernels round (see the module docstring); ``dtype`` is the
    accumulation type.  ``shift`` moves the softmax reference maximum by a constant, so p = exp2(x - m - shift) meets other bf16
    rounding boundaries -- what a lagging running maximum (online softmax over key tiles, the software-pipelined kernel) does
    to the p of earlier tiles.  The backward runs on the model's own o and lse, as the kernels' backward runs on theirs."""
    q, k, v, do = (t.to(dtype) for t in (q, k, v, do))
    Lq, Lk = q.shape[2], k.shape[2]
    c = scale * LOG2E
    x = (q @ k.transpose(-1, -2)) * c                                  # log2 domain
    if _defect == "last_key_of_ragged_tile_dropped" and Lk % 64 and Lk > 1:
        x[..., -1] = -math.inf
    # forward
    m = x.amax(-1, keepdim=True) + shift
    p = torch.exp2(x - m)
    l = p.sum(-1, keepdim=True)                                        # over the unrounded p
    pv = p if _defect == "p_not_rounded_before_pv" else _bf(p)
    o = _bf((pv @ v) / l)
    lse = (m + torch.log2(l)).squeeze(-1)
    if _defect == "lse_plus_0.01":
        lse = lse + 0.01
    # backward
    nd = 56 if _defect == "delta_over_56_channels" else 64
    delta = (do[..., :nd] * o[..., :nd]).sum(-1)                       # from the bf16 o
    lse_b = lse
    if _defect == "last_row_of_ragged_query_tile_reuses_lse" and Lq % 64 and Lq > 1:
        lse_b = lse.clone()
        lse_b[..., -1] = lse[..., -2]
    P = torch.exp2(x - lse_b[..., None])
    dP = do @ v.transpose(-1, -2)
    dS = P * (dP - delta[..., None])                                   # unrounded P
    Pr, dSr = _bf(P), _bf(dS)
    dv = _bf(Pr.transpose(-1, -2) @ do)
    dq = _bf(scale * (dSr @ k))
    dSk = dSr
    nt = (Lq + 63) // 64
    if _defect == "dk_misses_one_query_tile" and nt >= 2:
        dSk = dSr.clone()
        dSk[..., 64 * (nt - 1):, :] = 0
    dk = _bf(scale * (dSk.transpose(-1, -2) @ q))
    return {"o": o.double(), "lse": lse.double(), "dq": dq.double(), "dk": dk.double(), "dv": dv.double()}


def _broken(name):
    def f(q, k, v, do, scale, dtype, shift=0.0):
        return model(q, k, v, do, scale, dtype, shift, _defect=name)
    f.__name__ = name
    return f


# one seeded defect each, of a kind a kernel could have
HARMLESS = "p_not_rounded_before_pv"          # more precise than the kernels: must PASS (the metrics are not simply tight)
broken_models = {name: _broken(name) for name in (
    "last_key_of_ragged_tile_dropped", "last_row_of_ragged_query_tile_reuses_lse", "lse_plus_0.01", "delta_over_56_channels",
    "dk_misses_one_query_tile", HARMLESS)}


# ---------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------
def _rms(t):
    return float(t.double().pow(2).mean().sqrt()) if t.numel() else 0.0


def hard_use(got, ref, bound):
    """largest |got - ref| / allowed over all elements, allowed = (1 + 2^-6) bound + 2^-20 rms(ref); <= 1 passes.  Non-finite
    values of ``got`` give inf."""
    got = got.double().cpu()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    diff = (got - ref).abs()
    allowed = (1.0 + 2.0 ** -6) * bound + 2.0 ** -20 * _rms(ref)
    use = torch.where(diff == 0, torch.zeros_like(diff), diff / allowed)
    return float(use.max())


def block_ratio(got, model_out, ref, bound=None):
    """Per (batch, head, 64-row block): rms(got - ref) / max(rms(model - ref), 2^-20 rms(ref)), as a [B, heads, blocks] tensor.
    A kernel differs from the model only by fp32 summation order and the hardware exp2, so its error per block is the model's
    up to the spread between two such forms (measured in test_attention_model_host.py).

    The floor keeps the ratio meaningful where the format error vanishes.  Where the true result is exactly zero -- dQ and dK
    at Lk = 1, where dP = delta -- rms(ref) is zero as well and only fp32 summation order separates got, model and ref; with
    ``bound`` given the floor is therefore max(2^-20 rms(ref), 2^-12 rms(bound)) = 2^-20 of the magnitude of the summed terms
    (bound / u >= |ref| elementwise), which never exceeds a few 2^-20 rms(ref) unless the sum cancels."""
    got = got.double().cpu()
    B, h, L = got.shape[:3]
    nb = (L + 63) // 64
    out = torch.zeros(B, h, nb, dtype=torch.float64)
    for i in range(nb):
        sl = slice(64 * i, min(64 * i + 64, L))
        for b in range(B):
            for hh in range(h):
                r = ref[b, hh, sl]
                num = _rms(got[b, hh, sl] - r)
                floor = 2.0 ** -20 * _rms(r)
                if bound is not None:
                    floor = max(floor, 2.0 ** -12 * _rms(bound[b, hh, sl]))
                den = max(_rms(model_out[b, hh, sl] - r), floor)
                out[b, hh, i] = 0.0 if num == 0.0 else (num / den if den > 0 else math.inf)
    return out


_CACHE = {}


def case_reference(index, seed=0):
    """(inputs, ref, bound, sound model in fp64) of CASES[index], computed once per process and never modified"""
    key = (index, seed)
    if key not in _CACHE:
        ins = make_inputs(index, seed)
        ref, bound = ref64(*ins, CASES[index].eff_scale)
        mdl = model(*ins, CASES[index].eff_scale, torch.float64)
        _CACHE[key] = (ins, ref, bound, mdl)
    return _CACHE[key]


def measure(got, ref, bound, mdl, keys=KEYS):
    """{key: (hard_use, worst block ratio or None)} of the outputs in ``got`` ([B, heads, L, 64]; lse [B, heads, L])"""
    res = {}
    for key in keys:
        hu = hard_use(got[key], ref[key], bound[key])
        br = None
        if key in RATIO_KEYS:
            br = float(block_ratio(got[key], mdl[key], ref[key], bound[key]).max()) if math.isfinite(hu) else math.inf
        res[key] = (hu, br)
    return res


HARD_LIMIT = 1.0
RATIO_LIMIT = 2.0        # measured spread between two forms of the model <= 1.5 (host test asserts <= 1.6): a third of margin
