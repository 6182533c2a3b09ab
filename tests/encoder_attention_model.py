"""fp64 reference, elementwise error bounds and bf16 format models of the three attention kernels outside the U-Net:
  causal   csrc/attention_causal.hip  head 64, L <= 128, one-shot softmax            (CLIP text encoder)
  bias     csrc/attention_bias.hip    head 64, L <= 512, relative bias + key mask,   (MPNet prompt encoder)
                                      online softmax over 128-key chunks
  wide     csrc/attention_wide.hip    one head of width 512, online softmax over     (VAE mid-block)
                                      32-key tiles
Plain torch on the CPU, in the style of tests/attention_model.py (whose hard check, rounding helper and rms are imported, not
copied); shared by tests/test_encoder_attention_model_host.py (which proves that the reference, the bounds and the metrics are
sound and see seeded defects) and tests/test_encoder_attention_parity_gpu.py (which applies them to the kernels).

Tensors are [B, heads, L, D] here (wide: heads = 1, D = 512); ``to_heads`` / ``from_heads`` convert from / to the kernels'
[B, L, heads * D].  The additive term ``add`` is [B or 1, heads or 1, Lq, Lk] in natural-log units, -inf at a masked key.

Where the kernels round, and therefore where ``model`` rounds (c = scale * log2(e); all statistics fp32):
  score     S = Q K^T on mfma_f32_16x16x32_bf16, fp32 accumulator chained over D / 32
            instructions: 2 at D = 64, 16 at D = 512                             attention_short.h:90-91, attention_wide.hip:99-102
            t = S * c (+ Bs[j - i + L - 1], the table times log2(e) in fp32)     attention_causal.hip:64, attention_bias.hip:77, :134,
                                                                                 attention_wide.hip:126
  softmax   p = exp2(t - m): m the row maximum (causal), the running maximum
            after this 128-key chunk (bias; 0 while every key so far is masked)
            or after this 32-key tile (wide)                                     attention_short.h:121, attention_bias.hip:143-146,
                                                                                 attention_wide.hip:132-137
            row sum over the UNROUNDED fp32 p                                    attention_short.h:122, :131, attention_wide.hip:138-143
            p -> bf16 as the operand of P V                                      attention_short.h:123, attention_wide.hip:146-148
            l = l * alpha + rs, O = O * alpha + P V, alpha = exp2(m_old - m)
            in fp32                                                              attention_bias.hip:152-156, attention_wide.hip:143, :159, :165
  store     o = O * (1 / l) -> bf16, once (1 / l replaced by 0 where l = 0)     attention_short.h:160, attention_bias.hip:167,
                                                                                 attention_wide.hip:176-183

Elementwise bound of the bf16 kernels (first order; P, o the exact fp64 values; u = 2^-8, u32 = 2^-24):
  b_o = (u + e_s + e_a) (P |V| + |o|)
  u (P|V| + |o|)   each p is off by <= u p when it is rounded for P V (whatever maximum it was taken against: a relative error),
                   and the output is rounded once -- attention_model's b_o.
  e_s              the relative error of a weight p_ij before it is rounded = the absolute error of its exponent in natural-log
                   units, maximised over the valid keys j of the row.  A relative error e_j of the weights moves the weighted mean
                   o = sum p_j v_j / sum p_j by at most max_j |e_j| (P|V| + |o|).  Per (i, j), with x = scale * q.k, b the bias:
                     D u32 scale sum_d |q_d||k_jd|   D fp32 products summed in one accumulator chain (the products of two bf16 are
                                                     exact in fp32; every one of the D additions, inside an MFMA or between two,
                                                     is charged one rounding of the absolute sum)
                     u32 (2|x| + |b| + |x + b|)      c itself rounded to fp32 and the product S * c; the table entry times log2(e);
                                                     their sum
                     u32 |x + b - m|                 the subtraction of the maximum (its largest value over the row is used)
                     2^-23                           one hardware exp2 (1 ulp)
                   At D = 64 (|q.k| of a few tens) this is ~3e-6 against u = 3.9e-3.  At D = 512 the first term alone is
                   512 * 2^-24 * 512^-1/2 * sum|q||k| = 1.35e-6 * 327 amp^2 = 4.4e-4 amp^2 for N(0, amp^2) operands: 11 % of u at
                   amplitude 1, 45 % at amplitude 2 -- as a worst case; the measured use (profiles/encoder_attention_host_table.txt)
                   shows how little of it a random-sign sum needs.
  e_a = 2 Lk u32   ADDED to attention_model's form: the fp32 accumulation of P V over the keys (an MFMA chain of Lk / 32 steps of
                   32 products, plus one multiply by alpha per chunk or tile) and of the row sum (Lk terms), each charged Lk
                   roundings of the absolute sum: the first is <= Lk u32 P|V|, the second <= Lk u32 |o|.  6e-5 at Lk = 512 (1.6 %
                   of u).  alpha multiplies l and O as the same fp32 number and cancels in O / l.
The hard check is attention_model.hard_use unchanged: |got - ref| <= (1 + 2^-6) b + 2^-20 rms(ref) for EVERY element.

Bound of the fp32 parity instantiations (row_f32, attention_short.h:168-209: one thread per row, key by key; attn_wide_f32_kernel,
attention_wide.hip:198-268: 32-key tiles, everything sequential in fp32; operands are fp32 tensors holding bf16 values):
  b_32 = (e_s32 + (4 n + 8) u32) (P |V| + |o|),   n = the valid keys of the row
  e_s32            as e_s with the chain lengths of these kernels: the dot product is D sequential fp32 additions in channel
                   order (attention_short.h:183-188, attention_wide.hip:224) and the exponent takes two more roundings,
                   (sdot * scale + rb) * log2(e) (attention_bias.hip:188), so u32 (D scale sum|q||k| + 3|x| + 2|x + b| + |b|
                   + |x + b - m|) + 2^-23;
  2 n u32          the accumulator chain: per key one rounding of acc * alpha and one of the fused pr * v + (.) on O, the same two
                   on l (attention_short.h:193, :201; the wide kernel :240, :249, :253 has fewer per key);
  2 n u32          the weight a key ends with is pr_j times every later alpha; alpha is the same number for l and O, but each
                   change of the maximum costs one exp2 (2^-23); the roundings of the exponents m_old - m_new telescope to
                   u32 (max - min of the row's exponents), which the |x + b - m| term above already holds once more;
  8 u32            1 / l, the two final products, the fp32 store, and the roundings of c.
A dropped key of weight P_ij moves o by P_ij |v_j - o| ~ 1 / n of |v|, five orders above this bound (host test).

Blocks of the per-block ratio rms(got - ref) / rms(model - ref) -- the units of work of the kernels:
  causal, bias   (sample, head, 16-row strip); a ragged last strip (< 16 rows) is merged into its predecessor (<= 31 rows)
  wide           (sample, 32-row query tile, 128-channel wave slice); a last tile of < 16 rows cannot be merged into a 32-row
                 predecessor (no block may exceed 32 rows), so the predecessor is split at its 16-row accumulator half
                 (oacc[rb], attention_wide.hip:155) and the tail joins the second half (<= 31 rows)
Every element belongs to exactly one block; the hard bound leaves out nothing.

The padding contract of the bf16 bias kernel (kend = 1 + the last valid key of the sample): every row below L is written; the rows
of a 16-row strip that starts at or past kend (so also every strip of a 128-row query block with qbase >= kend) are exactly zero;
the rows past kend inside the strip that straddles kend hold ordinary attention values, as the fp32 kernel computes them for every
row.  ``kernel_zero_rows`` gives the zero rows; ``reference`` takes them, so the contract is part of the reference and those
elements are held to |got| <= 2^-20 rms(ref) -- and to exactly zero by the GPU test.
"""
import math

import torch

from tests.attention_model import LOG2E, U, _bf, _rms, hard_use  # noqa: F401  (hard_use is this module's hard check too)

U32 = 2.0 ** -24
HEAD = {"causal": 64, "bias": 64, "wide": 512}
CHUNK = {"causal": None, "bias": 128, "wide": 32}        # keys per step of the online softmax (None: one shot)
OTHER_CHUNK = {"causal": 32, "bias": 64, "wide": 16}     # the second sound form: another chunking (and the keys reversed)
OLD_LIMIT = {"causal": 4e-3, "bias": 6e-3, "wide": 4e-3}  # whole-tensor rel-L2 of the tests that were there before


def to_heads(t, heads):
    """[B, L, heads*D] -> [B, heads, L, D]"""
    B, L, C = t.shape
    return t.reshape(B, L, heads, C // heads).transpose(1, 2)


def from_heads(t):
    """[B, heads, L, D] -> [B, L, heads*D] contiguous"""
    B, h, L, D = t.shape
    return t.transpose(1, 2).reshape(B, L, h * D).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """kind, (B, heads, Lq, Lk) and the data: amp scales q and k; sink / spike scale one key; mask and table are the bias
    kernel's key mask and bias table.  ``ratio`` is False where the per-block ratio is recorded but not asserted (``why``)."""

    def __init__(self, kind, B, heads, Lq, Lk=None, amp=1.0, scale=None, sink=0.0, spike=0.0, mask="none", table="randn",
                 ratio=True, why="", f32=False, old=False):
        self.kind, self.B, self.heads, self.Lq, self.Lk = kind, B, heads, Lq, Lq if Lk is None else Lk
        self.amp, self.scale, self.sink, self.spike, self.mask, self.table = amp, scale, sink, spike, mask, table
        self.ratio, self.why, self.f32, self.old = ratio, why, f32, old
        self.D = HEAD[kind]

    @property
    def id(self):
        s = f"{self.kind}-B{self.B}-h{self.heads}-L{self.Lq}" + (f"x{self.Lk}" if self.Lk != self.Lq else "")
        if self.kind == "bias":
            m = self.mask if isinstance(self.mask, str) else self.mask[0] + "_".join(str(n) for n in self.mask[1:])
            s += f"-mask_{m}-table_{self.table}"
        s += f"-amp{self.amp:g}"
        for name, val in (("scale", self.scale), ("sink", self.sink), ("spike", self.spike)):
            if val:
                s += f"-{name}{val:g}"
        return s

    @property
    def eff_scale(self):
        return self.D ** -0.5 if self.scale is None else self.scale


# amp: which cases run at amplitude 2 (scores of standard deviation 4: a peaked softmax) was decided by the reference alone
# (test_encoder_attention_model_host.py measures the spread of the block ratio between two sound forms of the model per case; the
# notes beside the cases say where a case was moved to amplitude 1 or left without the ratio, and why).
_CAUSAL_AMP = {1: 2.0, 15: 1.0, 16: 2.0, 17: 1.0, 31: 2.0, 32: 1.0, 33: 2.0, 77: 1.0, 112: 2.0, 127: 1.0, 128: 2.0}
_BIAS_AMP = {1: 2.0, 16: 1.0, 17: 2.0, 127: 1.0, 128: 2.0, 129: 1.0, 200: 2.0, 257: 1.0, 384: 2.0, 512: 1.0}


def _cases():
    out = []
    for heads in (1, 3):
        for L, amp in _CAUSAL_AMP.items():
            out.append(Case("causal", 2, heads, L, amp=amp, f32=heads == 3 and L in (1, 17, 33, 112, 128)))
    out.append(Case("causal", 2, 3, 77, amp=1.0, sink=6.0, f32=True))      # key 0 x6: CLIP's attention sink
    out.append(Case("causal", 64, 16, 77, amp=1.0))                        # the training batch: where a lost row hides
    for heads in (1, 3):
        for L, amp in _BIAS_AMP.items():
            out.append(Case("bias", 2, heads, L, amp=amp, f32=heads == 3 and L in (1, 17, 129, 512)))
    # prefix masks: kend per sample (B = 3)
    out.append(Case("bias", 3, 3, 200, mask=("prefix", 1, 16, 17), f32=True))
    out.append(Case("bias", 3, 1, 200, mask=("prefix", 128, 129, 200), amp=2.0))
    out.append(Case("bias", 3, 3, 384, mask=("prefix", 17, 129, 128), table="rising"))
    out.append(Case("bias", 2, 3, 129, mask="holes"))
    out.append(Case("bias", 2, 1, 200, mask="holes", amp=2.0, f32=True))
    out.append(Case("bias", 2, 3, 512, mask="holes", table="falling"))
    # a fully masked FIRST chunk (keys 0..k, k >= 128): the muse = 0 path of attn_bias_kernel, then the first real maximum
    for table in ("randn", "rising", "falling"):
        out.append(Case("bias", 2, 3, 200, mask=("late", 139), table=table, f32=table == "rising"))
    out.append(Case("bias", 2, 1, 300, mask=("late", 130), table="randn", amp=2.0))
    out.append(Case("bias", 2, 3, 300, mask=("late", 260), table="rising"))      # two fully masked chunks
    # a fully masked MIDDLE chunk: keys 128..255 at L = 300
    for table in ("randn", "rising", "falling"):
        out.append(Case("bias", 2, 3, 300, mask=("middle", 128, 255), table=table, f32=table == "falling"))
    out.append(Case("bias", 3, 3, 200, mask="allmasked", f32=True))              # sample 1 has no valid key
    # the steep tables without a mask: the running maximum moves at every chunk change (rising) or never (falling)
    for L in (257, 384, 512):
        for table in ("rising", "falling"):
            out.append(Case("bias", 2, 3 if L != 384 else 1, L, table=table, f32=L == 257))
    wide_amp = {(1, 1): 2.0, (1, 33): 1.0, (31, 16): 2.0, (31, 17): 1.0, (33, 31): 2.0, (33, 32): 1.0, (64, 65): 2.0, (70, 333): 1.0}
    for (Lq, Lk), amp in wide_amp.items():
        out.append(Case("wide", 2, 1, Lq, Lk, amp=amp, f32=(Lq, Lk) in ((1, 33), (31, 17), (33, 31), (70, 333))))
    out.append(Case("wide", 2, 1, 33, 31, spike=6.0))
    out.append(Case("wide", 2, 1, 70, 333, spike=6.0, f32=True))
    out.append(Case("wide", 2, 1, 64, 65, scale=0.02))
    out.append(Case("wide", 2, 1, 31, 17, scale=0.1, amp=1.0))
    return out


CASES = _cases()

# the shapes and data of the tests that were there before (randn * 1.5, bias randn): where the old criterion is evaluated
OLD_CASES = [
    Case("causal", 64, 16, 77, amp=1.5, old=True),
    Case("bias", 2, 12, 512, amp=1.5, old=True),
    Case("bias", 2, 12, 200, amp=1.5, mask="holes", old=True),
    Case("wide", 4, 1, 200, amp=1.5, old=True),
    Case("wide", 2, 1, 70, 333, amp=1.5, scale=0.02, old=True),
]


def steep_table(heads, L, rising, total=40.0):
    """linear in j - i over the 2L - 1 entries, ``total`` logits from end to end (a few tens), a little steeper per head"""
    ramp = torch.linspace(-0.5, 0.5, 2 * L - 1, dtype=torch.float64) if L > 1 else torch.zeros(1, dtype=torch.float64)
    sign = 1.0 if rising else -1.0
    return torch.stack([sign * total * (1.0 + 0.25 * h) * ramp for h in range(heads)]).float().double()


def key_mask(case, g):
    """fp64 [B, L] of 0 / 1, or None"""
    B, L, m = case.B, case.Lk, case.mask
    if m == "none":
        return None
    km = torch.zeros(B, L, dtype=torch.float64)
    if m == "holes":                                   # as tests/test_prompt_encoder_gpu.py: keep 0.6, the last key, not key 0 of sample 0
        km = (torch.rand(B, L, generator=g) < 0.6).double()
        km[:, L - 1] = 1
        if L > 1:
            km[0, 0] = 0
    elif m == "allmasked":
        km[0, :max(L // 2, 1)] = 1
        km[2:] = 1
    elif m[0] == "prefix":
        for b in range(B):
            km[b, :m[1 + b % (len(m) - 1)]] = 1
    elif m[0] == "late":                               # keys 0..k masked; sample 1 also loses a few later keys
        km[:, m[1] + 1:] = 1
        km[1:, m[1] + 3:m[1] + 6] = 0
    elif m[0] == "middle":
        km[:] = 1
        km[:, m[1]:m[2] + 1] = 0
    return km


def make_inputs(case, seed=0):
    """dict: q, k, v fp64 [B, heads, L, D] holding bf16 values; relbias fp64 [heads, 2L - 1] holding fp32 values, or None; mask
    fp64 [B, L] or None.  Seeded from the case's own fields (not from hash())."""
    B, h, Lq, Lk, D = case.B, case.heads, case.Lq, case.Lk, case.D
    kinds = {"causal": 1, "bias": 2, "wide": 3}
    g = torch.Generator().manual_seed(1 + 7919 * (Lq * 1000 + Lk) + 31 * h + 977 * B + 104729 * seed + 13 * kinds[case.kind]
                                      + int(100 * case.amp))
    q = torch.randn(B, h, Lq, D, generator=g) * case.amp
    k = torch.randn(B, h, Lk, D, generator=g) * case.amp
    v = torch.randn(B, h, Lk, D, generator=g) * (case.amp if case.old else 1.0)
    if case.sink:
        k[:, :, 0] *= case.sink
    if case.spike:
        k[:, :, (Lk * 2) // 3] *= case.spike
    out = {n: t.bfloat16().double() for n, t in (("q", q), ("k", k), ("v", v))}
    out["relbias"] = out["mask"] = None
    if case.kind == "bias":
        if case.table == "randn":
            out["relbias"] = torch.randn(h, 2 * Lq - 1, generator=g).double()
        else:
            out["relbias"] = steep_table(h, Lq, case.table == "rising")
        out["mask"] = key_mask(case, g)
    return out


def additive(case, ins):
    """the additive term [B or 1, heads or 1, Lq, Lk] in natural-log units (-inf at a masked key), or None"""
    L = case.Lq
    ar = torch.arange(L)
    if case.kind == "causal":
        add = torch.zeros(L, L, dtype=torch.float64)
        add[ar[None, :] > ar[:, None]] = -math.inf
        return add[None, None]
    if case.kind == "bias":
        add = ins["relbias"][:, (ar[None, :] - ar[:, None]) + L - 1][None]              # [1, heads, L, L]
        if ins["mask"] is not None:
            add = add + torch.where(ins["mask"] == 0, -math.inf, 0.0)[:, None, None, :]
        return add
    return None


def kernel_zero_rows(mask, L):
    """bool [B, L]: the rows the bf16 bias kernel leaves exactly zero -- whole 16-row strips at or past kend -- or None"""
    if mask is None:
        return None
    idx = torch.arange(1, L + 1, dtype=torch.float64)
    kend = ((mask != 0).double() * idx).amax(-1)                                        # [B]; 0 when nothing is valid
    first = (torch.ceil(kend / 16.0) * 16.0)[:, None]
    return torch.arange(L, dtype=torch.float64)[None, :] >= first


# ---------------------------------------------------------------------------------------------------------------------
# reference and bounds
# ---------------------------------------------------------------------------------------------------------------------
def _softmax_parts(x):
    """(m, e, l) of a row-wise softmax over scores with -inf entries; a row of -inf only has m = 0, e = 0, l = 0"""
    m = x.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(x - m)
    return m, e, e.sum(-1, keepdim=True)


def reference(q, k, v, scale, add=None, relbias_abs=None, zero_rows=None):
    """All fp64.  Returns dict: o; b16, b32 (the elementwise bounds of the bf16 kernels and of the fp32 parity kernels); es16, es32
    (the score terms per row, for the tables).  ``relbias_abs`` is |b| broadcastable to the scores (the table's own rounding);
    ``zero_rows`` bool [B, L]: rows that are zero by contract (o and both bounds are zero there)."""
    assert all(t.dtype == torch.float64 for t in (q, k, v))
    D, Lk = q.shape[-1], k.shape[-2]
    xs = (q @ k.transpose(-1, -2)) * scale
    x = xs if add is None else xs + add
    m, e, l = _softmax_parts(x)
    P = torch.where(l > 0, e / l, torch.zeros_like(e))
    o = P @ v
    po = P @ v.abs() + o.abs()
    valid = torch.isfinite(x)
    n = valid.sum(-1, keepdim=True).double()
    b = torch.zeros_like(xs) if relbias_abs is None else relbias_abs.expand_as(xs)
    t = torch.where(valid, x, torch.zeros_like(x))                                     # x + b with the -inf taken out
    qk = scale * (q.abs() @ k.abs().transpose(-1, -2))
    dist = torch.where(valid, (t - m).abs(), torch.zeros_like(t))
    e16 = U32 * (D * qk + 2 * xs.abs() + b + t.abs() + dist) + 2.0 ** -23
    e32 = U32 * (D * qk + 3 * xs.abs() + b + 2 * t.abs() + dist) + 2.0 ** -23
    es16 = torch.where(valid, e16, torch.zeros_like(e16)).amax(-1, keepdim=True)
    es32 = torch.where(valid, e32, torch.zeros_like(e32)).amax(-1, keepdim=True)
    b16 = (U + es16 + 2 * Lk * U32) * po
    b32 = (es32 + (4 * n + 8) * U32) * po
    if zero_rows is not None:
        keep = (~zero_rows)[:, None, :, None].double()
        o, b16, b32 = o * keep, b16 * keep, b32 * keep
    return {"o": o, "b16": b16, "b32": b32, "es16": es16.squeeze(-1), "es32": es32.squeeze(-1)}


# ---------------------------------------------------------------------------------------------------------------------
# format model
# ---------------------------------------------------------------------------------------------------------------------
def _bf_trunc(t):
    """bf16 by truncation (the low 16 bits of the fp32 dropped) instead of round-to-nearest-even"""
    bits = t.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(t.dtype)


DEFECTS = {                      # name: the kernels it can occur in
    "truncating_bf16_store": ("causal", "bias", "wide"),
    "p_truncated_not_rounded": ("causal", "bias", "wide"),
    "one_row_lost_zero": ("causal", "bias", "wide"),
    "one_row_lost_stale": ("causal", "bias", "wide"),
    "diagonal_key_dropped_last_row_of_strip": ("causal",),
    "zero_tile_after_odd_tile_count_not_written": ("causal",),
    "last_key_of_ragged_chunk_dropped": ("causal", "bias", "wide"),
    "bias_one_entry_off_in_second_query_block": ("bias",),
    "alpha_not_applied_to_row_sum_once": ("bias", "wide"),
    "masked_first_chunk_poisons_maximum": ("bias",),
    "odd_partner_key_taken_as_valid": ("wide",),
    "neighbour_heads_v_on_last_strip": ("causal", "bias"),
}
HARMLESS = "p_not_rounded_before_pv"      # more precise than the kernels: must PASS (the metrics are not simply tight)


def model(case, ins, dtype, chunk="kernel", reverse=False, fmt=True, defect=None):
    """The same computation with bf16 roundings exactly where ``case.kind``'s kernel rounds (module docstring); ``dtype`` is the
    accumulation type.  chunk: keys per step of the online softmax ("kernel": the kernel's own; None: one shot); reverse: the
    keys in reverse order (another summation order, other chunk contents); fmt=False: no bf16 rounding at all (a model of the fp32
    parity kernels).  Returns o as fp64 [B, heads, Lq, D]; the bias kernel's zero rows are NOT applied here."""
    kind = case.kind
    if defect is not None:
        assert kind in DEFECTS.get(defect, (kind,)) and not reverse
    if chunk == "kernel":
        chunk = CHUNK[kind]
    q, k, v = (ins[n].to(dtype) for n in ("q", "k", "v"))
    B, h, Lq, D = q.shape
    Lk = k.shape[2]
    c = case.eff_scale * LOG2E
    add = additive(case, ins)
    if defect == "bias_one_entry_off_in_second_query_block" and Lq > 128:
        rb = ins["relbias"]
        off = additive(case, dict(ins, relbias=torch.cat([rb[:, 1:], rb[:, -1:]], 1)))
        add = add.expand(-1, h, -1, -1).clone()
        add[:, :, 128:256] = off.expand_as(add)[:, :, 128:256]
    x = (q @ k.transpose(-1, -2)) * c                                                    # log2 domain
    if add is not None:
        x = x + (add * LOG2E).to(dtype)
    x = x.expand(B, h, Lq, Lk).clone()
    if defect == "diagonal_key_dropped_last_row_of_strip":
        for i in range(15, Lq, 16):
            if i > 0:
                x[:, :, i, i] = -math.inf
    if defect == "last_key_of_ragged_chunk_dropped":
        unit = 32 if kind == "wide" else 16
        if kind == "bias" and ins["mask"] is not None:
            for b in range(B):
                nz = torch.nonzero(ins["mask"][b])
                if len(nz) and (int(nz[-1]) + 1) % unit and len(nz) > 1:
                    x[b, :, :, int(nz[-1])] = -math.inf
        elif Lk % unit and Lk > 1:
            if kind == "causal":
                x[:, :, Lk - 1, Lk - 1] = -math.inf                                      # (only the last row sees the last key)
            else:
                x[..., Lk - 1] = -math.inf
    if defect == "one_key_dropped":                                                      # (the fp32 bound's own seeded defect)
        cnt = torch.isfinite(x).sum(-1, keepdim=True)                                    # the row's heaviest key, if it has another
        top = torch.zeros_like(x, dtype=torch.bool).scatter_(-1, x.argmax(-1, keepdim=True), True)
        x = torch.where(top & (cnt > 1), torch.full_like(x, -math.inf), x)
    if defect == "odd_partner_key_taken_as_valid" and Lk % 2:                            # the clamped partner row counts again
        x = torch.cat([x, x[..., -1:]], -1)
        v = torch.cat([v, v[..., -1:, :]], -2)
        Lk += 1
    if reverse:
        x, v = x.flip(-1), v.flip(-2)
    round_p = (lambda t: t) if (not fmt or defect == HARMLESS) else (_bf_trunc if defect == "p_truncated_not_rounded" else _bf)
    vv = v
    if defect == "neighbour_heads_v_on_last_strip" and h > 1:
        vv = v.roll(-1, dims=1)
    step = Lk if chunk is None else chunk
    m = torch.full((B, h, Lq), -math.inf, dtype=dtype)
    l = torch.zeros(B, h, Lq, dtype=dtype)
    acc = torch.zeros(B, h, Lq, D, dtype=dtype)
    last0 = 16 * ((Lq - 1) // 16)
    for ci, k0 in enumerate(range(0, Lk, step)):
        xc = x[..., k0:k0 + step]
        mnew = torch.maximum(m, xc.amax(-1))
        muse = mnew if defect == "masked_first_chunk_poisons_maximum" else torch.where(torch.isinf(mnew), torch.zeros_like(mnew), mnew)
        alpha = torch.exp2(m - muse)
        p = torch.exp2(xc - muse[..., None])
        rs = p.sum(-1)
        pr = round_p(p)
        l = l + rs if (defect == "alpha_not_applied_to_row_sum_once" and ci == 1) else l * alpha + rs
        pv = pr @ v[..., k0:k0 + step, :]
        if vv is not v:
            pv[:, :, last0:] = pr[:, :, last0:] @ vv[:, :, k0:k0 + step, :]
        acc = acc * alpha[..., None] + pv
        m = mnew
    if defect == "zero_tile_after_odd_tile_count_not_written":
        # strip s has s + 1 tiles; when that is odd, the last 32-key step of P V reads tile s + 1 of the wave's P strip, which holds
        # what an earlier workgroup's strip s + 4 of the same wave left there: modelled by this pair's own strip s + 4
        pfull = _bf(torch.exp2(x - m[..., None]))
        nstrips = (Lq + 15) // 16
        for s in range(0, nstrips, 2):
            if s + 4 >= nstrips:
                continue
            rows = torch.arange(16 * s, min(16 * s + 16, Lq))
            src = torch.clamp(rows + 64, max=Lq - 1)
            keys = slice(16 * (s + 1), min(16 * (s + 2), Lk))
            acc[:, :, rows] += pfull[:, :, src][..., keys] @ v[:, :, keys]
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    o = acc * inv[..., None]
    if fmt:
        o = _bf_trunc(o) if defect == "truncating_bf16_store" else _bf(o)
    o = o.double()
    if defect in ("one_row_lost_zero", "one_row_lost_stale"):
        row = Lq - 1                                                                     # the last row of the last pair
        o[B - 1, h - 1, row] = 0.0 if defect.endswith("zero") or row == 0 else o[B - 1, h - 1, row - 1]
    return o


# ---------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------
def row_blocks(kind, L):
    """the row ranges [(a, b)] of the per-block ratio (module docstring); none exceeds 32 rows"""
    unit = 32 if kind == "wide" else 16
    edges = list(range(0, L, unit)) + [L]
    blocks = [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]
    if len(blocks) > 1 and blocks[-1][1] - blocks[-1][0] < 16:
        tail = blocks.pop()
        a, b = blocks.pop()
        blocks += [(a, tail[1])] if kind != "wide" else [(a, a + 16), (a + 16, tail[1])]
    assert all(0 < b - a <= 32 for a, b in blocks) and blocks[0][0] == 0 and blocks[-1][1] == L
    assert all(blocks[i][1] == blocks[i + 1][0] for i in range(len(blocks) - 1))
    return blocks


def block_ratio(kind, got, model_out, ref, bound):
    """rms(got - ref) / max(rms(model - ref), floor) per block as a [B, heads, row blocks, channel slices] tensor; the floor is
    attention_model.block_ratio's: max(2^-20 rms(ref), 2^-12 rms(bound)) over the block."""
    got = got.double().cpu()
    B, h, L, D = got.shape
    cs = 128 if kind == "wide" else D
    blocks = row_blocks(kind, L)
    out = torch.zeros(B, h, len(blocks), D // cs, dtype=torch.float64)

    def rms(t):
        return t.reshape(B, h, -1, D // cs, cs).pow(2).mean(dim=(2, 4)).sqrt()

    for i, (a, b) in enumerate(blocks):
        r = ref[:, :, a:b]
        num = rms(got[:, :, a:b] - r)
        den = torch.maximum(rms(model_out[:, :, a:b] - r), torch.maximum(2.0 ** -20 * rms(r), 2.0 ** -12 * rms(bound[:, :, a:b])))
        ratio = torch.where(den > 0, num / den, torch.full_like(num, math.inf))
        out[:, :, i] = torch.where(num == 0, torch.zeros_like(num), ratio)
    return out


def rel_l2(got, ref):
    """the old criterion: whole-tensor relative L2"""
    return float((got.double() - ref).norm() / (ref.norm() + 1e-30))


_CACHE = {}


def case_reference(case, seed=0, f32=False):
    """(inputs, reference dict, sound fp64 model) of a case, computed once per process and never modified.  With f32 the
    reference is the fp32 kernels' (every row computed); otherwise the bf16 kernel's zero rows are part of it."""
    key = (case.id, seed, f32)
    if key not in _CACHE:
        ins = make_inputs(case, seed)
        add = additive(case, ins)
        zr = None if f32 or case.kind != "bias" else kernel_zero_rows(ins["mask"], case.Lq)
        rb_abs = None
        if case.kind == "bias":
            ar = torch.arange(case.Lq)
            rb_abs = ins["relbias"].abs()[:, (ar[None, :] - ar[:, None]) + case.Lq - 1][None]
        ref = reference(ins["q"], ins["k"], ins["v"], case.eff_scale, add, rb_abs, zr)
        ref["zero_rows"] = zr
        mdl = None
        if not f32:
            mdl = model(case, ins, torch.float64)
            if zr is not None:
                mdl = mdl * (~zr)[:, None, :, None].double()
        _CACHE[key] = (ins, ref, mdl)
    return _CACHE[key]


def apply_zero_rows(o, zero_rows):
    return o if zero_rows is None else o * (~zero_rows)[:, None, :, None].to(o.dtype)


def measure(case, got, ref, mdl):
    """(hard_use over every element, worst block ratio) of a bf16 result [B, heads, Lq, D]"""
    hu = hard_use(got, ref["o"], ref["b16"])
    br = float(block_ratio(case.kind, got, mdl, ref["o"], ref["b16"]).max()) if math.isfinite(hu) else math.inf
    return hu, br


HARD_LIMIT = 1.0
SPREAD_MEASURED = 1.2     # the largest block ratio between two sound forms of the model, every case, 4 seeds: 1.18 (host test:
                          # asserted <= this)
RATIO_LIMIT = 1.6         # that plus a third, as attention_model.RATIO_LIMIT (1.5 measured, 2.0 used)
