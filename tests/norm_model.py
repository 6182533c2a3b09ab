"""fp64 reference, elementwise error bound and a format model of the normalisation kernels behind ops.groupnorm / ops.layernorm
(csrc/norm.hip), of the GroupNorm applied by the split-K reduce launch (csrc/conv_gemm.hip, splitk_reduce_gn_kernel), of the
LayerNorm folded into a linear layer (ln_finish, csrc/conv_gemm_core.h) and of the statistics the GEMM epilogues emit for them
(emit_col_stats / emit_unit_stats / the row statistics, csrc/conv_gemm_core.h, csrc/lin_gemm.hip).  Plain torch, device-agnostic:
tests/test_norm_model_host.py runs it on the CPU and proves that the reference, the bound and the metrics are sound and see seeded
defects; tests/test_norm_parity_gpu.py evaluates the SAME functions in fp64 on the device and applies them to the kernels.

Tensors are channels-last [B, H, W, roundup8(C)], fp64 holding bf16 values, C real channels, pad columns exact zero (and expected
back as exact zero: their bound is 0).  gamma / beta are fp64 holding fp32 values.  LayerNorm rows are [rows, C].

Where the kernels round, and therefore what ``bound`` charges for:
  statistics    GroupNorm: ONE pass, fp32 sums of x and x * x (bf16 x bf16 is exact in fp32), then mean = a / n and
    (GroupNorm)   var = a2 / n - mean * mean, clamped at zero, rstd = rsqrtf(var + eps) -- gn_finalize_sample (norm.hip:58-63),
                  gn_finalize_cols_kernel (:115-120), the fold_in_apply branch (:316-321), gn_group_kernel (:483-488),
                  splitk_reduce_gn_kernel (conv_gemm.hip:803-807).  The unit-statistics branch (norm.hip:296-301) takes 64-bit
                  fixed-point totals and finishes in double; its producers round every contribution once to 2^-20 (sums) and
                  2^-12 (sums of squares) (conv_gemm_core.h:416-417).
  statistics    LayerNorm: two passes in registers, mean = sum / C, var = sum((x - mean)^2) / C (norm.hip:574-587): no mean^2
    (LayerNorm)   is subtracted.  The FOLDED LayerNorm is one pass again (ln_finish, conv_gemm_core.h:244-250) and then forms
                  rstd * (acc - mean * colsum) (conv_gemm_core.h:132-133, lin_gemm.hip:294): a second cancellation.
  affine        k = rstd * gamma, shift = beta - mean * k, v = x * k + shift in fp32 (norm.hip:341-343, :370; :506-508, :526);
                LayerNorm (x - mean) * rstd * gamma + beta (:600); SiLU by silu_f (aptp_common.h:65) as in tests/gemm_model.py
  store         ONE round-to-nearest-even conversion to bf16 (pack_bf16x8, norm.hip:375, :530, :601; pack_bf16x2,
                conv_gemm.hip:825)

Elementwise bound (first order in u = 2^-24, exact in the statistics' errors), U_out = 2^-8:
    |got - ref| <= U_out |y| + L stat + 8 u S + E
  stat  |gamma| (r dmu + (|x - mu| + dmu) dr): what an error dmu of the mean and dr of rstd do to gamma r (x - mu) + beta
  dmu   d u mean|x| + 2 u |mu|            (any order of fp32 additions whose longest chain is d errs by at most d u sum|a|)
  dvar  one pass:  (d + 2) u mean(x^2) + 2 |mu| dmu + dmu^2 + 2 u mu^2
        two passes (LayerNorm): (d + 4) u (var + dmu^2) + dmu^2                                          -- no mu^2 anywhere
        unit statistics add cnt 2^-21 / n to dmu and cnt 2^-13 / n to dvar: half a fixed-point step for each of the cnt
        contributions to a group (``unit_contributions``)
  dr    max(r(max(var - dvar, 0)) - r(var), r(var) - r(var + dvar)) + 4 u r, r(v) = (v + eps)^-1/2: the exact interval, which
        is never below the first-order dr / r = dvar / (2 (var + eps)) on the side where the kernels' clamp at zero is not met
        (1 / sqrt is convex) and stays finite when dvar exceeds var + eps (a constant group with a large value)
  L     1 without SiLU, 1.1 = max |silu'| with it;  S the affine expression on absolute values (|x| |k| + |mu| |k| + |beta|,
        through SiLU 1.1 S + |y|);  E = (3 + 1.5 |v|) u |y| for SiLU's exp / rcp -- S, E and the 8 as tests/gemm_model.py words
        them
  folded LayerNorm:  y = r (A - mu c) + b', A = x W'^T, c = colsum(W'), b' = the packed bias.  The reference is LayerNorm-then-
        linear on the kernel's operands (x, the bf16 W', b') in fp64, and ``acc - mean * colsum`` is bounded on absolute values:
        T = sum|x| |W'| + |mu| |c|;  |got - ref| <= U_out |y| + (K + 8) u (r T + |b'|) + dr T + (r + dr) |c| dmu
        + r |mu| |c - c64|, the last term being the measured fp32 error of the packed colsum itself.

d, the longest addition chain, is ``depth``: a function of (path, HW, C, G, nchunk) read from the kernels, never below the real
chain of additions that can round (adding to a zero-initialised accumulator, or adding the exact zero of a row slot that holds
no row, cannot; the first is nevertheless counted, the second is not).  tests/test_norm_model_host.py checks it against the
chain that ``chunked_group_sums`` -- the three-launch form's summation order -- really has.

Format model: fp64 statistics, fp64 affine, one RNE bf16 store (the ``model`` method of GroupNormRef / LayerNormRef /
FoldedLayerNormRef with dtype=torch.float64).  With dtype=torch.float32 and an ``order`` the same methods evaluate the kernels'
arithmetic (one-pass fp32 statistics in sequential, pairwise or kernel-chunk order): the host test's "sound forms".

Metrics: ``hard_use`` = max |got - ref| / bound (limit HARD_LIMIT = 1) and, per TILE -- one (sample, group) of a GroupNorm, one
row of a LayerNorm -- ``tile_ratios`` = rms(got - ref) / max(rms(model - ref), 2^-12 rms(bound)) (limit RATIO_LIMIT = 1.25), both
limits those of tests/gemm_model.py.  The ratio measures the kernel against the bf16 store alone, so it is asserted only on tiles
where the store dominates: the rms over the tile of the statistic term L stat is at most 1/8 of the rms of the store term
U_out |y| (``ratio_tiles``) -- the ratio compares energies, and so does its precondition.  An element-by-element form of it holds
on no tile at all: where y crosses zero an element's store term vanishes while the mean's term does not.  The hard bound is
asserted everywhere.
"""
import math

import numpy as np
import torch

from tests.gemm_model import HARD_LIMIT, RATIO_LIMIT, U32, U_BF16, _bf, _bf_trunc, hard_use, rel_l2      # noqa: F401

USTAT_SUM_SCALE = 2.0 ** 20          # conv_gemm_core.h:389-390
USTAT_SQ_SCALE = 2.0 ** 12
OLD_REL_L2_TOL = 4e-3
RATIO_STORE_SHARE = 1.0 / 8.0
KINDS = ("plain", "offset4", "offset16", "offset32", "offset64", "tiny", "mixed", "outlier")
STRESS_KINDS = ("offset32", "offset64")          # hard bound asserted, ratio and rstd error recorded only


def roundup8(c):
    return (c + 7) // 8 * 8


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch of aptp_groupnorm (norm.hip:637-751) and the longest addition chain of every path
# ---------------------------------------------------------------------------------------------------------------------
def nchunk_of(HW):
    """aptp_groupnorm_nchunk (norm.hip:612-620)"""
    return max(1, min(128, HW // 4 if HW <= 256 else HW // 16))


def gn_dispatch(variant, HW, C, G, producer=None):
    """(path, info) aptp_groupnorm takes: 'group' (gn_group_kernel<U, NT>), 'stats' (gn_stats_kernel<NP> + finalise + apply),
    'stats3' (variant 3: coarse chunks folded by every apply workgroup), 'cols' / 'units' (producer statistics), or 'refused'
    (variant 2 where the slab does not fit).  ``producer``: None, 'cols' or 'units'."""
    cg, CO = C // G, roundup8(C) // 8
    NP = 1 if CO <= 256 else 2
    gpb = 1
    while (gpb * cg) % 8:
        gpb *= 2
    tpr = gpb * cg // 8
    if variant != 1 and tpr <= 32 and producer is None and (variant == 2 or HW <= 256):
        for NT, rows_max in ((256, 24), (1024, 16)):
            rpar = NT // tpr
            rows = _cdiv(HW, rpar)
            if rows <= rows_max:
                U = next(u for u in (4, 8, 16, 24) if rows <= u)
                return "group", dict(NT=NT, U=U, RPAR=rpar, tpr=tpr, gpb=gpb, rows=rows)
    if variant == 2:
        return "refused", {}
    if producer is not None:
        return producer, dict(NP=NP)
    if variant == 3:
        return "stats3", dict(NP=NP, nchunk=max(1, min(16, HW // 256)))
    return "stats", dict(NP=NP, nchunk=nchunk_of(HW))


def depth(path, HW, C, G, nchunk=None, rpb=(), unit=0, slots=0):
    """Longest chain of fp32 additions behind one statistic of the path (an upper bound, see the module docstring):
      stats    rows a thread walks (ceil(rows of a chunk / RPAR), norm.hip:140) + the LDS fold of the min(RPAR, rows) row slots that
               hold a row x ceil(cg / 8) channels (:183-188) + 3 shuffles (:191-194) + the chunk fold of gn_finalize_sample: ceil(nchunk / 8) + 3 (:40-56)
      stats3   the same partials, folded in chunk order by every apply workgroup: + nchunk (:313-315)
      group    rows per thread (:434-443) + LDS rounds - 1 (:448-458) + row slots that hold a row (:463) + ceil(cg / 32) (:472-475) + 5 shuffles
      cols     the producer's rows of one wave block, rpb (conv_gemm_core.h:583, :452) + ceil(row blocks x cg / 256) partials
               per thread and segment (norm.hip:91-102) + the 8 levels of the LDS tree (:110-113)
      units    rpb + the channels of a unit (conv_gemm_core.h:412); the totals are integers
      reduce   splitk_reduce_gn_kernel: 24 values per thread + 16 strided sums + 6 shuffles (conv_gemm.hip:765-801)
      ln       ln_kernel: 8 NO values per lane + 6 shuffles (norm.hip:561-574), NO = ceil(C / 512)
      lnfold   row statistics: <= 20 columns per lane + 4 shuffles in the producer (conv_gemm_core.h:218-226, :374-375;
               lin_gemm.hip:341-344), two additions per slot pair in the consumer (:311-312; conv_gemm.hip:741) + 2 shuffles"""
    cg, CO = (C // G if G else C), roundup8(C) // 8
    if path in ("stats", "stats3"):
        TPR = min(CO, 256)
        RPAR = 256 // TPR
        if nchunk is None:
            nchunk = nchunk_of(HW) if path == "stats" else max(1, min(16, HW // 256))
        rows = _cdiv(HW, nchunk)
        d = _cdiv(rows, RPAR) + min(RPAR, rows) * _cdiv(cg, 8) + 3
        return d + (_cdiv(nchunk, 8) + 3 if path == "stats" else nchunk)
    if path == "group":
        info = gn_dispatch(2, HW, C, G)[1]
        R256 = 256 // info["tpr"]
        return info["rows"] + (_cdiv(min(info["RPAR"], HW), R256) - 1) + min(info["RPAR"], R256, HW) + _cdiv(cg, 32) + 5
    if path == "cols":
        return max(rpb) + sum(_cdiv((HW // r) * cg, 256) for r in rpb) + 8
    if path == "units":
        return max(rpb) + unit
    if path == "reduce":
        return 24 + 16 + 6
    if path == "ln":
        return 8 * _cdiv(C, 512) + 6
    if path == "lnfold":
        return 24 + slots + 2
    raise ValueError(path)


def unit_contributions(HW, cg, unit, rpb, wl=None):
    """upper count of fixed-point contributions to one group's totals: every wave block of ``rpb`` rows adds once per unit and
    per wave-column block of ``wl`` columns the unit touches (conv_gemm_core.h:403-417) -- at most two for unit <= wl"""
    per_unit = 2 if wl is None else (_cdiv(unit, wl) + 1)
    return (HW // rpb) * (cg // unit) * per_unit


# ---------------------------------------------------------------------------------------------------------------------
# fp32 summation in a chosen order (the host test's sound forms)
# ---------------------------------------------------------------------------------------------------------------------
def _seq(v):
    """strictly sequential fp32 sum over the last axis"""
    a = np.ascontiguousarray(v.detach().cpu().to(torch.float32).numpy())
    return torch.from_numpy(np.add.accumulate(a, axis=-1, dtype=np.float32)[..., -1].copy())


def _tree(v):
    """fp32 sum over the last axis by halving (lane j + lane j ^ half: the shuffle trees of the kernels)"""
    v = v.to(torch.float32)
    n = 1 << max(0, (v.shape[-1] - 1).bit_length())
    v = torch.nn.functional.pad(v, (0, n - v.shape[-1]))
    while n > 1:
        n //= 2
        v = v[..., :n] + v[..., n:]
    return v[..., 0]


def sum_f32(v, order):
    return _seq(v) if order == "sequential" else _tree(v)


def chunked_group_sums(xg, nchunk, fold="lanes"):
    """xg [B, HW, G, cg] -> (fp32 sums [B, G], the longest addition chain): the order of gn_stats_kernel + gn_finalize_sample
    (norm.hip:125-195, :33-65).  Rows r0 + rl, r0 + rl + RPAR, ... of a chunk go through one thread per channel; 8 threads per
    group fold row slots x every 8th channel; a 3-level shuffle tree; the chunk partials fold as c = sub, sub + 8, ... and a tree."""
    B, HW, G, cg = xg.shape
    C = G * cg
    TPR = min(roundup8(C) // 8, 256)
    RPAR = 256 // TPR
    xg = xg.to(torch.float32)
    parts, chain_rows, chain_slots = [], 0, 0
    for c in range(nchunk):
        r0, r1 = HW * c // nchunk, HW * (c + 1) // nchunk
        slots = []
        for rl in range(RPAR):
            rows = xg[:, r0 + rl:r1:RPAR]                                        # [B, n, G, cg]
            chain_rows = max(chain_rows, rows.shape[1])
            chain_slots = max(chain_slots, rl + 1 if rows.shape[1] else 0)
            slots.append(_seq(rows.permute(0, 2, 3, 1)) if rows.shape[1] else xg.new_zeros(B, G, cg))
        st = torch.stack(slots, 2)                                               # [B, G, RPAR, cg]
        lanes = [_seq(st[..., sub::8].reshape(B, G, -1)) if sub < cg else xg.new_zeros(B, G) for sub in range(8)]
        parts.append(_tree(torch.stack(lanes, -1)))
    pt = torch.stack(parts, -1)                                                  # [B, G, nchunk]
    chain = chain_rows + chain_slots * _cdiv(cg, 8) + 3
    if fold == "sequential":                                                     # variant 3: every apply workgroup, in chunk order
        return _seq(pt), chain + nchunk
    lanes = [_seq(pt[..., sub::8]) if sub < nchunk else xg.new_zeros(B, G) for sub in range(8)]
    return _tree(torch.stack(lanes, -1)), chain + _cdiv(nchunk, 8) + 3


def chunked_row_sums(x):
    """x [rows, C] -> fp32 row sums in ln_kernel's order: lane l owns octets l, l + 64, ...; 6-level shuffle tree"""
    rows, C = x.shape
    NO = _cdiv(C, 512)
    v = torch.nn.functional.pad(x.to(torch.float32), (0, NO * 512 - C)).reshape(rows, NO, 64, 8).permute(0, 2, 1, 3)
    return _tree(_seq(v.reshape(rows, 64, NO * 8)))


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------------
def _silu(t):
    return t * torch.sigmoid(t)


def _rstd_interval(var, dvar, eps):
    r = (var + eps) ** -0.5
    hi = ((var - dvar).clamp_min(0.0) + eps) ** -0.5
    lo = (var + dvar + eps) ** -0.5
    return r, torch.maximum(hi - r, r - lo) + 4.0 * U32 * hi


class GroupNormRef:
    """fp64 GroupNorm(+SiLU) of x [B, H, W, roundup8(C)] and everything the bound needs; computed once, never modified"""

    def __init__(self, x, gamma, beta, C, G, eps, silu):
        assert x.dtype == torch.float64 and x.shape[-1] == roundup8(C) and C % G == 0
        self.x, self.gamma, self.beta, self.C, self.G, self.eps, self.silu = x, gamma, beta, C, G, eps, silu
        B, H, W, Cp = x.shape
        self.B, self.HW, self.Cp, self.cg = B, H * W, Cp, C // G
        self.n = self.cg * self.HW
        xg = self.groups(x)
        self.mean = xg.mean((1, 3))
        self.var = ((xg - self.mean[:, None, :, None]) ** 2).mean((1, 3))
        self.ex2 = (xg * xg).mean((1, 3))
        self.a1 = xg.abs().mean((1, 3))
        self.rstd = (self.var + eps) ** -0.5
        self.v, self.y = self._apply(self.mean, self.rstd)
        self.store = U_BF16 * self.y.abs()
        mu, r = self._pc(self.mean), self._pc(self.rstd)
        k = (gamma * r).abs()
        xs = x[..., :C]
        S = xs.abs() * k + mu.abs() * k + beta.abs()
        if silu:
            S = 1.1 * S + self.y[..., :C].abs()
            E = (3.0 + 1.5 * self.v[..., :C].abs()) * U32 * self.y[..., :C].abs()
        else:
            E = torch.zeros_like(S)
        self.base = self._pad(U_BF16 * self.y[..., :C].abs() + 8.0 * U32 * S + E)

    def groups(self, t):
        """[B, H, W, >= C] -> [B, HW, G, cg] over the real channels"""
        return t[..., :self.C].reshape(self.B, self.HW, self.G, self.cg)

    def _pc(self, s):
        """per-(sample, group) [B, G] -> broadcastable against [B, H, W, C]"""
        return s.repeat_interleave(self.cg, dim=1)[:, None, None, :]

    def _pad(self, t):
        return torch.nn.functional.pad(t, (0, self.Cp - self.C))

    def _apply(self, mean, rstd, dtype=torch.float64, gamma=None, beta=None, silu_mask=None):
        gamma = self.gamma if gamma is None else gamma
        beta = self.beta if beta is None else beta
        k = self._pc(rstd.to(dtype)) * gamma.to(dtype)
        sh = beta.to(dtype) - self._pc(mean.to(dtype)) * k
        v = self.x[..., :self.C].to(dtype) * k + sh
        y = v
        if self.silu:
            y = _silu(v)
            if silu_mask is not None:
                y = torch.where(silu_mask, y, v)
        return self._pad(v), self._pad(y)

    def stat_errors(self, d, cnt=0):
        """(dmu, dr) [B, G] of a path whose longest chain is d (an int or a [B, G] tensor); cnt: fixed-point contributions"""
        mu = self.mean.abs()
        dmu = d * U32 * self.a1 + 2.0 * U32 * mu + cnt * 0.5 / USTAT_SUM_SCALE / self.n
        dvar = (d + 2.0) * U32 * self.ex2 + 2.0 * mu * dmu + dmu * dmu + 2.0 * U32 * mu * mu + cnt * 0.5 / USTAT_SQ_SCALE / self.n
        _, dr = _rstd_interval(self.var, dvar, self.eps)
        return dmu, dr

    def bound(self, d, cnt=0):
        """(bound, stat): the elementwise hard bound of the module docstring and its statistic term L stat, [B, H, W, Cp]"""
        dmu, dr = self.stat_errors(d, cnt)
        xs = self.x[..., :self.C]
        stat = self.gamma.abs() * (self._pc(self.rstd * dmu) + ((xs - self._pc(self.mean)).abs() + self._pc(dmu)) * self._pc(dr))
        stat = self._pad((1.1 if self.silu else 1.0) * stat)
        return self.base + stat, stat

    def ratio_tiles(self, stat):
        """[B, G] bool: tiles where the statistic term's rms is at most 1/8 of the store term's rms"""
        stat_rms = (self.groups(stat) ** 2).mean((1, 3)).sqrt()
        store_rms = (self.groups(self.store) ** 2).mean((1, 3)).sqrt()
        return stat_rms <= RATIO_STORE_SHARE * store_rms

    def tile_ratios(self, got, model_out, bound):
        """[B, G]: rms(got - ref) / max(rms(model - ref), 2^-12 rms(bound)) per (sample, group)"""
        got = got.to(self.y.device, torch.float64)
        num = (self.groups(got - self.y) ** 2).mean((1, 3)).sqrt()
        den = (self.groups(model_out - self.y) ** 2).mean((1, 3)).sqrt()
        floor = 2.0 ** -12 * (self.groups(bound) ** 2).mean((1, 3)).sqrt()
        r = num / torch.maximum(den, floor)
        return torch.where(num == 0, torch.zeros_like(r), r)

    def model(self, dtype=torch.float64, order=None, nchunk=None, _defect=None, seg0=None):
        """The format model (dtype fp64) or the kernels' arithmetic (dtype fp32: one-pass statistics summed in ``order`` =
        'sequential' | 'pairwise' | 'chunked', fp32 affine), one RNE store.  ``_defect`` seeds one defect a kernel could have;
        ``seg0``: channels of the first of two producer segments (only the straddle defect reads it)."""
        B, HW, G, cg, C, n = self.B, self.HW, self.G, self.cg, self.C, self.n
        xg = self.groups(self.x)
        sel = torch.ones_like(xg)
        if _defect == "one_row_of_ragged_chunk_not_summed":
            sel[B - 1, HW - 1] = 0                                     # the last row of the last sample's last chunk
        if _defect == "straddling_group_reads_first_segment":
            ch = torch.arange(C, device=xg.device).reshape(G, cg)
            straddles = (ch[:, 0] < seg0) & (ch[:, -1] >= seg0)
            sel = sel * (~(straddles[:, None] & (ch >= seg0))).to(sel.dtype)
        xs = xg * sel
        div = torch.full((G,), float(n), dtype=torch.float64, device=xg.device)
        if _defect == "divisor_minus_one":
            div -= 1.0
        if _defect == "pad_channels_counted":
            div[G - 1] = (cg + self.Cp - C) * HW
        if dtype == torch.float64:
            a, a2 = xs.sum((1, 3)), (xs * xs).sum((1, 3))
            mean = a / div
            var = ((xs - mean[:, None, :, None]) ** 2 * sel).sum((1, 3)) / div if _defect is None else a2 / div - mean * mean
        else:
            x32 = xs.to(torch.float32)
            if order == "chunked":
                a, _ = chunked_group_sums(x32, nchunk or nchunk_of(HW))
                a2, _ = chunked_group_sums(x32 * x32, nchunk or nchunk_of(HW))
            else:
                flat = x32.permute(0, 2, 1, 3).reshape(B, G, n)
                a, a2 = sum_f32(flat, order), sum_f32(flat * flat, order)
            a, a2 = a.to(xg.device), a2.to(xg.device)
            inv = (1.0 / div).to(torch.float32)
            mean = a * inv
            var = a2 * inv - mean * mean
        var = var.clamp_min(0.0)
        eps = 0.0 if _defect == "eps_omitted" else self.eps
        rstd = (var + torch.tensor(eps, dtype=var.dtype)) ** -0.5
        if _defect == "ragged_last_group_takes_previous_statistics":
            mean, rstd = mean.clone(), rstd.clone()
            mean[:, G - 1], rstd[:, G - 1] = mean[:, G - 2], rstd[:, G - 2]
        gamma, beta, mask = self.gamma, self.beta, None
        if _defect == "affine_shifted_in_ragged_tail_octet" and C % 8:
            gamma, beta = gamma.clone(), beta.clone()
            t0 = C // 8 * 8
            gamma[t0:], beta[t0:] = self.gamma[t0 - 1:C - 1], self.beta[t0 - 1:C - 1]
        if _defect == "silu_skipped_on_second_octet_page":
            mask = (torch.arange(C, device=xg.device) < 2048).expand(B, 1, 1, C)
        _, y = self._apply(mean, rstd, dtype, gamma, beta, mask)
        y = _bf_trunc(y.float()) if _defect == "truncating_bf16_store" else _bf(y.float())
        return y.double()


def measure_gn(ref, got, d, cnt=0, model_out=None):
    """dict(hard_use, tile_ratio over the ratio tiles (0.0 if there is none), asserted share of tiles, worst ratio over all
    tiles) of ``got`` against ``ref`` at chain d"""
    bnd, stat = ref.bound(d, cnt)
    got = got.to(ref.y.device, torch.float64)
    if not bool(torch.isfinite(got).all()):
        return dict(hard_use=math.inf, tile_ratio=math.inf, share=0.0, ratio_all=math.inf)
    mdl = ref.model() if model_out is None else model_out
    ok = ref.ratio_tiles(stat)
    tr = ref.tile_ratios(got, mdl, bnd)
    return dict(hard_use=hard_use(got, ref.y, bnd), tile_ratio=float(tr[ok].max()) if bool(ok.any()) else 0.0,
                share=float(ok.double().mean()), ratio_all=float(tr.max()))


def rstd_error(ref, got):
    """[B, G] relative error of the rstd the kernel used, read back from its output: the least-squares slope of
    (got - beta) / gamma on x - mu per (sample, group) over the reference's rstd, minus 1 (GroupNorm without SiLU; the bf16 store
    averages out over the n elements of a group)"""
    assert not ref.silu
    z = ref.groups((got.to(ref.y.device, torch.float64)[..., :ref.C] - ref.beta) / ref.gamma)
    xc = ref.groups(ref.x) - ref.mean[:, None, :, None]
    slope = (z * xc).sum((1, 3)) / (xc * xc).sum((1, 3)).clamp_min(1e-300)
    return slope / ref.rstd - 1.0


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm (ln_kernel) and the LayerNorm folded into a linear layer
# ---------------------------------------------------------------------------------------------------------------------
class LayerNormRef:
    """fp64 LayerNorm of x [rows, C]; a tile is one row"""

    def __init__(self, x, gamma, beta, eps):
        assert x.dtype == torch.float64
        self.x, self.gamma, self.beta, self.eps = x, gamma, beta, eps
        self.rows, self.C = x.shape
        self.mean = x.mean(1, keepdim=True)
        self.var = ((x - self.mean) ** 2).mean(1, keepdim=True)
        self.a1 = x.abs().mean(1, keepdim=True)
        self.rstd = (self.var + eps) ** -0.5
        self.y = (x - self.mean) * self.rstd * gamma + beta
        self.store = U_BF16 * self.y.abs()
        self.base = self.store + 6.0 * U32 * ((x - self.mean).abs() * self.rstd * gamma.abs() + beta.abs())

    def bound(self, d=None):
        d = depth("ln", 0, self.C, 0) if d is None else d
        dmu = d * U32 * self.a1 + 2.0 * U32 * self.mean.abs()
        dvar = (d + 4.0) * U32 * (self.var + dmu * dmu) + dmu * dmu
        _, dr = _rstd_interval(self.var, dvar, self.eps)
        stat = self.gamma.abs() * (self.rstd * dmu + ((self.x - self.mean).abs() + dmu) * dr)
        return self.base + stat, stat

    def ratio_tiles(self, stat):
        return (stat ** 2).mean(1).sqrt() <= RATIO_STORE_SHARE * (self.store ** 2).mean(1).sqrt()

    def tile_ratios(self, got, model_out, bound):
        got = got.to(self.y.device, torch.float64)
        num, den = ((got - self.y) ** 2).mean(1).sqrt(), ((model_out - self.y) ** 2).mean(1).sqrt()
        r = num / torch.maximum(den, 2.0 ** -12 * (bound ** 2).mean(1).sqrt())
        return torch.where(num == 0, torch.zeros_like(r), r)

    def model(self, dtype=torch.float64, order=None, _defect=None):
        x = self.x.to(dtype)
        if dtype == torch.float64:
            mean, var = self.mean, self.var
        else:
            s = (lambda t: chunked_row_sums(t)) if order == "chunked" else (lambda t: sum_f32(t, order))
            mean = (s(x) / torch.tensor(float(self.C), dtype=dtype))[:, None].to(x.device)
            dlt = x - mean
            var = (s(dlt * dlt) / torch.tensor(float(self.C), dtype=dtype))[:, None].to(x.device)
        rstd = (var + torch.tensor(self.eps, dtype=dtype)) ** -0.5
        y = (x - mean) * rstd * self.gamma.to(dtype) + self.beta.to(dtype)
        y = _bf_trunc(y.float()) if _defect == "truncating_bf16_store" else _bf(y.float())
        y = y.double()
        if _defect == "ln_last_partial_workgroup_not_written" and self.rows % 4:
            y[self.rows // 4 * 4:] = 0.0                                # (the output buffer's previous contents: zeros)
        return y


def measure_ln(ref, got, d=None, model_out=None):
    bnd, stat = ref.bound(d)
    got = got.to(ref.y.device, torch.float64)
    if not bool(torch.isfinite(got).all()):
        return dict(hard_use=math.inf, tile_ratio=math.inf, share=0.0, ratio_all=math.inf)
    mdl = ref.model() if model_out is None else model_out
    ok = ref.ratio_tiles(stat)
    tr = ref.tile_ratios(got, mdl, bnd)
    return dict(hard_use=hard_use(got, ref.y, bnd), tile_ratio=float(tr[ok].max()) if bool(ok.any()) else 0.0,
                share=float(ok.double().mean()), ratio_all=float(tr.max()))


class FoldedLayerNormRef(LayerNormRef):
    """y = LayerNorm(x) W'^T + b' with gamma folded into the bf16 W' [N, C] and beta into the fp32 b' (ops.pack_weight
    ln_gamma / ln_beta); ``colsum`` is the packed fp32 row sum of W'.  The kernels' statistics are ONE pass over the producer's
    row partials (ln_finish); a tile is one row of the output."""

    def __init__(self, x, w, bias, colsum, eps):
        one, zero = torch.ones(x.shape[1], dtype=torch.float64, device=x.device), torch.zeros(x.shape[1], dtype=torch.float64, device=x.device)
        super().__init__(x, one, zero, eps)
        self.w, self.bias, self.colsum = w, bias, colsum
        self.ex2 = (x * x).mean(1, keepdim=True)
        self.yn = ((x - self.mean) * self.rstd) @ w.t() + bias
        self.T = x.abs() @ w.abs().t() + self.mean.abs() * colsum.abs()
        self.c_err = (colsum - w.sum(1)).abs()
        self.y = self.yn
        self.store = U_BF16 * self.y.abs()

    def bound(self, d):
        mu = self.mean.abs()
        dmu = d * U32 * self.a1 + 2.0 * U32 * mu
        dvar = (d + 2.0) * U32 * self.ex2 + 2.0 * mu * dmu + dmu * dmu + 2.0 * U32 * mu * mu
        r, dr = _rstd_interval(self.var, dvar, self.eps)
        stat = dr * self.T + (r + dr) * self.colsum.abs() * dmu
        K = self.x.shape[1]
        return self.store + (K + 8.0) * U32 * (r * self.T + self.bias.abs()) + stat + r * mu * self.c_err, stat

    def model(self, dtype=torch.float64, order=None, _defect=None):
        assert dtype == torch.float64
        y = self.yn
        return (_bf_trunc(y.float()) if _defect == "truncating_bf16_store" else _bf(y.float())).double()


# ---------------------------------------------------------------------------------------------------------------------
# the statistics the GEMM epilogues leave with a tensor: references are fp64 sums of the STORED bf16 values
# ---------------------------------------------------------------------------------------------------------------------
def col_stats_ref(y, rpb):
    """y [B, HW, C] fp64 -> (ref [B * HW / rpb, C, 2], bound): (sum, sumsq) per (row block, channel); rpb u sum|a|"""
    B, HW, C = y.shape
    blk = y.reshape(B * HW // rpb, rpb, C)
    ref = torch.stack([blk.sum(1), (blk * blk).sum(1)], -1)
    bnd = rpb * U32 * torch.stack([blk.abs().sum(1), (blk * blk).sum(1)], -1)
    return ref, bnd


def row_stats_ref(y, d=24):
    """y [M, N] fp64 -> (ref [M, 2], bound): per-row (sum, sumsq); the slots are added up in fp64 by the caller, so d is the
    chain inside one slot"""
    ref = torch.stack([y.sum(1), (y * y).sum(1)], -1)
    return ref, d * U32 * torch.stack([y.abs().sum(1), (y * y).sum(1)], -1)


def _unit_keys(C, unit, wl):
    """per channel: (unit, id of the (wave-column block, unit) pair the channel's contribution goes through)"""
    c = torch.arange(C)
    u = c // unit
    blk = torch.zeros_like(c) if wl is None else c // wl
    pair = blk * (C // unit + 2) + u
    _, key = torch.unique(pair, return_inverse=True)
    return u, key


def unit_stats_ref(y, unit, rpb, wl=None):
    """y [B, HW, C] fp64 -> (ref [B, units, 2] in real units, bound, its fp32 share, its fixed-point share): per-(sample, unit)
    (sum, sumsq) over the whole units of C; (rpb + unit) u sum|a| for the fp32 partials + half a fixed-point step per
    contribution (counted exactly when the wave-column width ``wl`` is known, else two per unit and row block)"""
    B, HW, C = y.shape
    nu = C // unit
    yu = y[..., :nu * unit].reshape(B, HW, nu, unit)
    ref = torch.stack([yu.sum((1, 3)), (yu * yu).sum((1, 3))], -1)
    cnt = unit_contributions(HW, unit, unit, rpb, wl)
    if wl is not None:                                   # exact: the wave-column blocks each unit really touches
        lo = torch.arange(nu, device=y.device) * unit
        cnt = (HW // rpb) * ((lo + unit - 1) // wl - lo // wl + 1).to(torch.float64)[None, :]
    fix = torch.stack([torch.as_tensor(cnt * 0.5 / USTAT_SUM_SCALE, dtype=torch.float64, device=y.device).expand(B, nu),
                       torch.as_tensor(cnt * 0.5 / USTAT_SQ_SCALE, dtype=torch.float64, device=y.device).expand(B, nu)], -1)
    flt = (rpb + unit) * U32 * torch.stack([yu.abs().sum((1, 3)), (yu * yu).sum((1, 3))], -1)
    return ref, flt + fix, flt, fix


def unit_stats_model(y, unit, rpb, wl, dtype=torch.float64, _defect=None):
    """[B, units, 2] in real units: every (row block, wave-column block, unit) partial rounded once to the fixed-point grid
    (round to nearest even; the seeded defect truncates the sum of squares), integer totals"""
    B, HW, C = y.shape
    nu = C // unit
    u, key = _unit_keys(nu * unit, unit, wl)
    u, key = u.to(y.device), key.to(y.device)
    nk = int(key.max()) + 1
    blk = y[..., :nu * unit].reshape(B, HW // rpb, rpb, nu * unit).to(dtype)
    s = torch.zeros(B, HW // rpb, nk, dtype=dtype, device=y.device).index_add_(2, key, blk.sum(2))
    s2 = torch.zeros(B, HW // rpb, nk, dtype=dtype, device=y.device).index_add_(2, key, (blk * blk).sum(2))
    q1 = torch.round(s.double() * USTAT_SUM_SCALE)
    q2 = s2.double() * USTAT_SQ_SCALE
    q2 = torch.floor(q2) if _defect == "unit_sumsq_truncated" else torch.round(q2)
    ku = torch.zeros(nk, dtype=torch.long, device=y.device).index_copy_(0, key, u)
    out = torch.zeros(B, nu, 2, dtype=torch.float64, device=y.device)
    out[..., 0].index_add_(1, ku, q1.sum(1))
    out[..., 1].index_add_(1, ku, q2.sum(1))
    out[..., 0] /= USTAT_SUM_SCALE
    out[..., 1] /= USTAT_SQ_SCALE
    return out


def stat_ratio(got, model_out, ref, fix, flt):
    """error energy of emitted unit statistics over the fixed-point model's, per statistic (sum, sumsq), over the entries where
    the fp32 partial's share of the bound is at most 1/8 of the fixed-point share (elsewhere the rounding to the grid does not
    dominate and the model says nothing); (ratio, share of entries compared)"""
    ok = flt <= RATIO_STORE_SHARE * fix
    out = []
    for k in range(2):
        m = ok[..., k]
        if not bool(m.any()):
            out.append(0.0)
            continue
        num = ((got[..., k] - ref[..., k])[m] ** 2).mean().sqrt()
        den = ((model_out[..., k] - ref[..., k])[m] ** 2).mean().sqrt().clamp_min(2.0 ** -12 * float(fix[..., k][m].mean()))
        out.append(float(num / den))
    return max(out), float(ok.double().mean())


def group_sums_from_units(tot, C, G, unit):
    """[B, units, 2] -> [B, G, 2]: the units of every group added up (a group is a whole number of units)"""
    B = tot.shape[0]
    upg = C // G // unit
    return tot[:, :G * upg].reshape(B, G, upg, 2).sum(2)


# ---------------------------------------------------------------------------------------------------------------------
# cases and seeded data
# ---------------------------------------------------------------------------------------------------------------------
class Shape:
    def __init__(self, B, H, W, C, G, silu=True, eps=1e-5, why="", seg0=None, gpu=True):
        self.B, self.H, self.W, self.C, self.G, self.silu, self.eps, self.why, self.seg0, self.gpu = B, H, W, C, G, silu, eps, why, seg0, gpu
        self.kinds = KINDS if gpu else ("plain",)          # the host-only shapes carry one seeded defect each, on plain data
        self.name = f"{B}x{H}x{W}x{C}g{G}"

    @property
    def HW(self):
        return self.H * self.W


# the smallest shapes at which every template and edge of aptp_groupnorm's dispatch is reached (the table of
# tests/test_norm_parity_gpu.py says which), plus three the seeded defects need (host only)
GN_SHAPES = [
    Shape(2, 4, 4, 64, 32, why="small map"),
    Shape(3, 4, 4, 170, 17, why="ragged, padded to 176 columns"),
    Shape(2, 16, 16, 85, 17, why="8 groups per workgroup"),
    Shape(2, 16, 16, 340, 17, silu=False, why="ragged group layout"),
    Shape(1, 12, 16, 2048, 8, why="U = 24"),
    Shape(1, 16, 16, 2048, 8, silu=False, why="NT = 1024"),
    Shape(1, 8, 8, 2560, 32, why="two octet pages"),
    Shape(1, 8, 8, 4096, 32, silu=False, why="C limit"),
    Shape(1, 8, 8, 2112, 8, why="cg = 264, the group kernel refuses"),
    Shape(2, 5, 7, 320, 32, why="ragged chunks"),
    Shape(1, 32, 32, 320, 32, silu=False, eps=1e-6, why="larger map (HW 1024)"),
    Shape(1, 64, 64, 320, 32, silu=False, why="nchunk caps (HW 4096)"),
    Shape(1, 8, 8, 960, 32, seg0=640, gpu=False, why="640 + 320 skip-concat: group 21 straddles the segments"),
    Shape(2, 13, 19, 320, 32, gpu=False, why="ragged chunks on a map large enough that one lost row hides from rel-L2"),
    Shape(1, 128, 128, 170, 17, gpu=False, why="ragged last group on a map large enough that all groups' statistics agree to 1 %"),
]
GN_SHAPE_IDS = [s.name for s in GN_SHAPES]


def shape_index(name):
    return GN_SHAPE_IDS.index(name)


def _gen(*key):
    seed = 1
    for k in key:
        seed = (seed * 1000003 + int(k) + 7919) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def group_data(B, HW, G, cg, kind, g):
    """[B, HW, G, cg] fp32 before the bf16 rounding.  plain: 2 N(0,1) + 0.7 (tests/test_ops_gpu.py); offsetK: N(0,1) with
    per-group means of +-K, the sign alternating by group; tiny: sigma 2^-9, var < eps; mixed: sigma per group from 2^-9 to
    2^3, group 1 constant 1.5, group 2 all zero; outlier: one element of 2^7 in group G // 2 of every sample"""
    z = torch.randn(B, HW, G, cg, generator=g)
    sign = (1.0 - 2.0 * (torch.arange(G) % 2)).reshape(1, 1, G, 1)
    if kind == "plain":
        return 2.0 * z + 0.7
    if kind.startswith("offset"):
        return z + float(kind[6:]) * sign
    if kind == "tiny":
        return 2.0 ** -9 * (z + 0.35)
    if kind == "mixed":
        sig = 2.0 ** (-9.0 + 12.0 * torch.arange(G) / max(G - 1, 1)).reshape(1, 1, G, 1)
        x = sig * (z + 0.35 * sign)
        x[:, :, 1 % G] = 1.5
        if G > 2:
            x[:, :, 2] = 0.0
        return x
    if kind == "outlier":
        x = z.clone()
        pos = torch.randint(0, HW * cg, (B,), generator=g)
        for b in range(B):
            x[b, int(pos[b]) // cg, G // 2, int(pos[b]) % cg] = 2.0 ** 7
        return x
    raise ValueError(kind)


def make_gn(index, kind, seed=0):
    """(x [B, H, W, roundup8(C)] fp64 holding bf16, gamma, beta fp64 holding fp32) of GN_SHAPES[index]; seeded from the shape's
    position and the kind's, never from hash()"""
    s = GN_SHAPES[index]
    g = _gen(index, KINDS.index(kind), seed)
    xg = group_data(s.B, s.HW, s.G, s.C // s.G, kind, g).bfloat16().double()
    x = torch.zeros(s.B, s.H, s.W, roundup8(s.C), dtype=torch.float64)
    x[..., :s.C] = xg.reshape(s.B, s.H, s.W, s.C)
    gamma = (1.0 + 0.2 * torch.randn(s.C, generator=g)).float().double()
    beta = (0.3 * torch.randn(s.C, generator=g)).float().double()
    return x, gamma, beta


def gn_reference(index, kind, device="cpu"):
    s = GN_SHAPES[index]
    x, gamma, beta = make_gn(index, kind)
    return GroupNormRef(x.to(device), gamma.to(device), beta.to(device), s.C, s.G, s.eps, s.silu)


LN_KINDS = ("plain", "offset16", "tiny")
LN_CASES = [(rows, C) for C in (64, 512, 1024, 1536, 2048) for rows in (1, 5, 130)]


def make_ln(rows, C, kind, seed=0):
    g = _gen(rows, C, LN_KINDS.index(kind) if kind in LN_KINDS else 9, seed)
    z = torch.randn(rows, C, generator=g)
    sign = (1.0 - 2.0 * (torch.arange(rows) % 2)).reshape(rows, 1)
    if kind == "plain":
        x = 1.5 * z + 0.4
    elif kind.startswith("offset"):
        x = z + float(kind[6:]) * sign
    else:
        x = 2.0 ** -9 * (z + 0.35)
    gamma = (1.0 + 0.2 * torch.randn(C, generator=g)).float().double()
    beta = (0.3 * torch.randn(C, generator=g)).float().double()
    return x.bfloat16().double(), gamma, beta


# seeded defects: name -> (shape or LayerNorm case it must be caught on, data kind)
DEFECTS = {
    "truncating_bf16_store": ("3x4x4x170g17", "plain"),
    "ragged_last_group_takes_previous_statistics": ("1x128x128x170g17", "plain"),
    "one_row_of_ragged_chunk_not_summed": ("2x13x19x320g32", "plain"),
    "eps_omitted": ("2x4x4x64g32", "tiny"),
    "divisor_minus_one": ("2x4x4x64g32", "plain"),
    "pad_channels_counted": ("3x4x4x170g17", "plain"),
    "straddling_group_reads_first_segment": ("1x8x8x960g32", "plain"),
    "silu_skipped_on_second_octet_page": ("1x8x8x2560g32", "plain"),
    "affine_shifted_in_ragged_tail_octet": ("3x4x4x170g17", "plain"),
}
DEFECT_ALSO = {
    "truncating_bf16_store": (("1x64x64x320g32", "plain"), ("2x16x16x340g17", "offset4")),
    "ragged_last_group_takes_previous_statistics": (("3x4x4x170g17", "plain"), ("3x4x4x170g17", "mixed")),
    "one_row_of_ragged_chunk_not_summed": (("2x5x7x320g32", "plain"),),
    "eps_omitted": (("2x16x16x85g17", "mixed"),),
}
LN_DEFECTS = {
    "truncating_bf16_store": (130, 512, "plain"),
    "ln_last_partial_workgroup_not_written": (130, 64, "plain"),
}
UNIT_DEFECT_CASE = ("1x32x32x320g32", "tiny", 10, 32, 80)        # shape, kind, unit, rows per wave block, wave columns
OLD_CRITERION_MUST_PASS = ("truncating_bf16_store", "ragged_last_group_takes_previous_statistics", "one_row_of_ragged_chunk_not_summed")
