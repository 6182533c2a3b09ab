"""Elementwise and per-(sample, group) / per-row accuracy of the normalisation kernels (ops.groupnorm through every template of
csrc/norm.hip, ops.layernorm, the GroupNorm of the split-K reduce launch, the LayerNorm folded into a linear layer) and of the
statistics the GEMM epilogues emit for them, against the fp64 references, the hard bound and the bf16 format model of
tests/norm_model.py, all evaluated in fp64 on the device from the same bf16 operands.  tests/test_norm_model_host.py proves on
the CPU that these metrics pass the sound forms of the model and fail each seeded defect -- among them a truncating bf16 store, a
ragged last group that takes its neighbour's statistics and a row lost from a statistics chunk, which the whole-tensor
rel-L2 <= 4e-3 of tests/test_ops_gpu.py lets through.

Which kernel each GroupNorm shape reaches (aptp_groupnorm, norm.hip:658-748; tpr = 16-byte chunks per slab row, RPAR = rows in
parallel; variant 1 always takes gn_stats_kernel<NP> + gn_finalize_kernel (or the last-arriver finalise with counters) +
gn_apply_kernel<NP>; variant 3 and 4 take the group kernel wherever variant 0 does):

  (B,H,W,C,G)        variant 0 / 2                              variant 1                  variant 3
  (2,4,4,64,32)      group<4,256>   gpb 4 tpr 1: small map      stats<1> 4 chunks          = variant 0
  (3,4,4,170,17)     group<4,256>   gpb 4 tpr 5, ragged last    stats<1>, 176 columns      = variant 0
  (2,16,16,85,17)    group<8,256>   gpb 8 tpr 5, ragged last    stats<1> 64 chunks         = variant 0
  (2,16,16,340,17)   group<8,256>   gpb 2 tpr 5, ragged last    stats<1> 64 chunks         = variant 0
  (1,12,16,2048,8)   group<24,256>  tpr 32, 24 rows per thread  stats<1> TPR 256           = variant 0
  (1,16,16,2048,8)   group<8,1024>  tpr 32, NT = 1024           stats<1> TPR 256           = variant 0
  (1,8,8,2560,32)    group<4,256>   tpr 10                      stats<2>: two octet pages  = variant 0
  (1,8,8,4096,32)    group<4,256>   tpr 16                      stats<2>: CO = 512, limit  = variant 0
  (1,8,8,2112,8)     stats<2> (tpr 33: refused) / not generated stats<2>                   fold_in_apply, 1 chunk
  (2,5,7,320,32)     group<4,256>   gpb 4 tpr 5                 stats<1>: 8 ragged chunks  = variant 0
  (1,32,32,320,32)   stats<1> 64 chunks / group<24,256>         stats<1> 64 chunks         fold_in_apply, 4 chunks
  (1,64,64,320,32)   stats<1> 128 chunks (cap) / not generated  stats<1> 128 chunks        fold_in_apply, 16 chunks (cap)

Every assertion goes through margins.check; no test repeats a launch.  The committed record is profiles/norm_parity_margins.json."""
import math

import pytest
import torch

from tests import margins
from tests import norm_model as NM
from tests import tiles

pytestmark = pytest.mark.gpu

GPU_SHAPES = [i for i, s in enumerate(NM.GN_SHAPES) if s.gpu]
FEW_KINDS = ("plain", "offset16", "offset32", "offset64", "tiny", "mixed")      # variants 2, 3, 4 (1 and 0 take every kind)
WAVE_COLUMNS = {t: tiles.BY_ID[t].bn // tiles.BY_ID[t].wn for t in (9, 18, 34, 64)}    # bn / wn of the tiles asked for by id
SENTINEL = 0x5A5B


@pytest.fixture(scope="module")
def ops(cuda):
    from diffusion_pruning_amd import ops as o
    o._lib.load()
    return o


_REF = {}


def reference(index, kind, cuda):
    """(GroupNormRef on the device, bf16 x, fp32 gamma, beta, the fp64 format model) of (GN_SHAPES[index], kind): once, unchanged"""
    if (index, kind) not in _REF:
        ref = NM.gn_reference(index, kind, cuda)
        _REF[(index, kind)] = (ref, ref.x.bfloat16().contiguous(), ref.gamma.float().contiguous(), ref.beta.float().contiguous(), ref.model())
    return _REF[(index, kind)]


def _rstd_text(ref, got, mdl):
    """the worst relative rstd error read back from the output, next to what the same estimator reads from the fp64 format model
    (its own noise: the bf16 store averaged over the n elements of a group)"""
    return (f" rstd error {float(NM.rstd_error(ref, got).abs().max()):.2e} (n = {ref.n}, estimator floor "
            f"{float(NM.rstd_error(ref, mdl).abs().max()):.1e})")


def _assert_gn(ref, got, mdl, d, what, kind, cnt=0):
    m = NM.measure_gn(ref, got, d, cnt, model_out=mdl)
    print(f"{what}: d {d} hard_use {m['hard_use']:.4f} tile_ratio {m['tile_ratio']:.4f} (share {m['share']:.2f}, all tiles {m['ratio_all']:.3f})")
    margins.check(m["hard_use"], NM.HARD_LIMIT, what + " hard_use")
    if kind in NM.STRESS_KINDS:
        err = "" if ref.silu else _rstd_text(ref, got, mdl)
        margins.check(m["hard_use"], NM.HARD_LIMIT, what + f" hard_use again, stress offset: tile_ratio {m['ratio_all']:.3f}{err} recorded only")
    else:
        margins.check(m["tile_ratio"], NM.RATIO_LIMIT, what + f" tile_ratio over {m['share']:.2f} of the tiles (all tiles: {m['ratio_all']:.3f}, recorded)")
    return m


def _gn_params():
    out = []
    for index in GPU_SHAPES:
        s = NM.GN_SHAPES[index]
        for variant in (1, 2, 3, 0, 4):
            path = NM.gn_dispatch(variant, s.HW, s.C, s.G)[0]
            if path == "refused":
                continue                              # (variant 2 where the slab does not fit: aptp_groupnorm's documented refusal)
            for kind in (NM.KINDS if variant in (0, 1) else FEW_KINDS):
                for fused in ((False, True) if path == "stats" and variant != 4 else (False,)):
                    out.append(pytest.param(index, kind, variant, fused, id=f"{s.name}-{kind}-v{variant}-{path}" + ("-fused-finalize" if fused else "")))
    return out


@pytest.mark.parametrize("index,kind,variant,fused", _gn_params())
def test_groupnorm_elementwise_and_per_group(ops, cuda, index, kind, variant, fused):
    s = NM.GN_SHAPES[index]
    ref, x, gamma, beta, mdl = reference(index, kind, cuda)
    path, _ = NM.gn_dispatch(variant, s.HW, s.C, s.G)
    d = NM.depth(path, s.HW, s.C, s.G)
    ops.GN_FUSED_FINALIZE = fused
    try:
        if variant == 4:
            y, ws = ops.groupnorm(x, gamma, beta, s.G, s.eps, s.silu, C=s.C, keep_stats=True)
        else:
            y = ops.groupnorm(x, gamma, beta, s.G, s.eps, s.silu, C=s.C, variant=variant)
    finally:
        ops.GN_FUSED_FINALIZE = False
    torch.cuda.synchronize()
    what = f"groupnorm {s.name} {kind} variant {variant} [{path}{', fused finalise' if fused else ''}]"
    _assert_gn(ref, y, mdl, d, what, kind)
    if variant == 4:
        # the partials the backward consumes, summed over the chunks in fp64, against the fp64 sums of the same bf16 values
        tot = ws.double().sum(1)
        want = torch.stack([ref.mean * ref.n, ref.ex2 * ref.n], -1)
        bnd = (d + 1) * NM.U32 * torch.stack([ref.a1 * ref.n, ref.ex2 * ref.n], -1)
        margins.check(NM.hard_use(tot, want, bnd), NM.HARD_LIMIT, what + " keep_stats partials hard_use")


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_groupnorm_strided_views_per_group(ops, cuda, variant):
    """the input a channel slice of a wider NaN-filled buffer, the output a slice of a buffer holding a sentinel bit pattern"""
    index = NM.shape_index("2x16x16x340g17")
    s = NM.GN_SHAPES[index]
    ref, x, gamma, beta, mdl = reference(index, "offset4", cuda)
    Cp = x.shape[-1]
    wide = torch.full((s.B, s.H, s.W, Cp + 56), float("nan"), dtype=torch.bfloat16, device=cuda)
    wide[..., 8:8 + Cp] = x
    outw = torch.empty(s.B, s.H, s.W, Cp + 40, dtype=torch.bfloat16, device=cuda)
    outw.view(torch.int16).fill_(SENTINEL)
    y = ops.groupnorm(wide[..., 8:8 + Cp], gamma, beta, s.G, s.eps, s.silu, C=s.C, out=outw[..., 16:16 + Cp], variant=variant)
    torch.cuda.synchronize()
    bits = outw.view(torch.int16)
    assert bool((bits[..., :16] == SENTINEL).all()) and bool((bits[..., 16 + Cp:] == SENTINEL).all())
    path = NM.gn_dispatch(variant, s.HW, s.C, s.G)[0]
    _assert_gn(ref, y, mdl, NM.depth(path, s.HW, s.C, s.G), f"groupnorm views {s.name} variant {variant} [{path}]", "offset4")


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def _assert_ln(ref, got, mdl, what, d=None):
    m = NM.measure_ln(ref, got, d, model_out=mdl)
    print(f"{what}: hard_use {m['hard_use']:.4f} tile_ratio {m['tile_ratio']:.4f} (share {m['share']:.2f}, all rows {m['ratio_all']:.3f})")
    margins.check(m["hard_use"], NM.HARD_LIMIT, what + " hard_use")
    margins.check(m["tile_ratio"], NM.RATIO_LIMIT, what + f" tile_ratio over {m['share']:.2f} of the rows (all rows: {m['ratio_all']:.3f}, recorded)")
    return m


@pytest.mark.parametrize("kind", NM.LN_KINDS)
@pytest.mark.parametrize("rows,C,wide", [(r, c, 0) for r, c in NM.LN_CASES] + [(130, 512, 64)])
def test_layernorm_elementwise_and_per_row(ops, cuda, rows, C, wide, kind):
    x, gamma, beta = (t.to(cuda) for t in NM.make_ln(rows, C, kind))
    ref = NM.LayerNormRef(x, gamma, beta, 1e-5)
    xb = x.bfloat16()[None]
    if wide:                                        # ld > C: a column slice of a wider NaN-filled buffer
        buf = torch.full((1, rows, C + wide), float("nan"), dtype=torch.bfloat16, device=cuda)
        buf[..., 8:8 + C] = xb
        xb = buf[..., 8:8 + C]
    y = ops.layernorm(xb, gamma.float().contiguous(), beta.float().contiguous(), 1e-5)
    torch.cuda.synchronize()
    _assert_ln(ref, y[0], ref.model(), f"layernorm {rows}x{C} {kind}" + (f" ld {C + wide}" if wide else ""))


# ---------------------------------------------------------------------------------------------------------------------
# producer statistics and the GroupNorm that consumes them
# ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = {  # name -> (channels of the segments, groups, unit)
    "one-320": ((320,), 32, 10),
    "straddle-640+320": ((640, 320), 32, 10),          # SD-2.1 skip-concat: groups of 30, group 21 spans both producers
    "straddle-200+312": ((200, 312), 32, 8),           # groups of 16, group 12 spans both
}


def _producer_bias(Cs, G, kind, g):
    """per-channel producer bias: a small one, or +-K (in units of the convolution's unit output spread) alternating by group"""
    C = sum(Cs)
    b = 0.3 * torch.randn(C, generator=g)
    if kind.startswith("offset"):
        b = b + float(kind[6:]) * (1.0 - 2.0 * ((torch.arange(C) // (C // G)) % 2))
    return b


@pytest.mark.parametrize("kind", ["plain", "offset16", "offset32", "offset64", "tiny"])
@pytest.mark.parametrize("units", [False, True], ids=["column-statistics", "unit-statistics"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("tile", [0, 9, 18, 34, 64])
def test_producer_statistics_and_their_groupnorm(ops, cuda, tile, k, layout, units, kind):
    """conv_gemm(colstats=True) at 32 x 32 leaves (sum, sumsq) per (row block, channel) and, inside an ops.ustat_begin bracket,
    fixed-point sums per (sample, unit): each entry against the fp64 sums of the STORED tensor; then the GroupNorm that is fed by
    them (gn_finalize_cols_kernel, or the unit branch of gn_apply_kernel) per group"""
    Cs, G, unit = LAYOUTS[layout]
    B, H = 2, 32
    HW, C = H * H, sum(Cs)
    g = NM._gen(tile, k, list(LAYOUTS).index(layout), int(units), len(kind))
    Cin = 128 if k == 1 else 64
    scale = (2.0 ** -9 if kind == "tiny" else 1.0) / math.sqrt(Cin * k * k)
    bias = _producer_bias(Cs, G, kind, g) * (2.0 ** -9 if kind == "tiny" else 1.0)
    cat = torch.zeros(B, H, H, C, dtype=torch.bfloat16, device=cuda)
    gamma = (1.0 + 0.2 * torch.randn(C, generator=g)).to(cuda)
    beta = (0.3 * torch.randn(C, generator=g)).to(cuda)
    if units:
        ops.ustat_begin(cuda, unit)
    try:
        off = 0
        for Cn in Cs:
            x = torch.randn(B, H, H, Cin, generator=g).bfloat16().to(cuda)
            pw = ops.pack_weight(torch.randn(Cn, Cin, k, k, generator=g) * scale, bias[off:off + Cn], device=cuda)
            try:
                ops.conv_gemm(x, pw, out=cat[..., off:off + Cn], colstats=True, tile=tile, split_k=1)
            except ops._lib.AptpError as e:
                if "rc=-1" in str(e):
                    pytest.skip(f"refused by aptp_conv_gemm: {e}")
                raise
            off += Cn
    finally:
        ops.ustat_end()
    rec = ops._colstats_get(cat, C)
    assert rec is not None and len(rec) == len(Cs), "every producer must have left column statistics"
    assert all((r[3] is not None) == units for r in rec)
    y64 = cat.double().reshape(B, HW, C)
    what = f"tile {tile} {k}x{k} {layout} {kind}"
    wl = WAVE_COLUMNS.get(tile)
    off, rpbs = 0, []
    for (st, rpb, Cn, us) in rec:
        rpbs.append(rpb)
        seg = y64[..., off:off + Cn]
        want, bnd = NM.col_stats_ref(seg, rpb)
        margins.check(NM.hard_use(st[:B * HW // rpb].double(), want, bnd), NM.HARD_LIMIT, what + f" column statistics of {Cn} channels hard_use")
        if units:
            buf, u_unit, nunits, nrep = us
            assert u_unit == unit
            nu = Cn // unit
            tot = buf.view(nrep, B, nunits, 2).sum(0)[:, :nu].double()
            tot = torch.stack([tot[..., 0] / NM.USTAT_SUM_SCALE, tot[..., 1] / NM.USTAT_SQ_SCALE], -1)
            want, bnd, flt, fix = NM.unit_stats_ref(seg, unit, rpb, wl)
            margins.check(NM.hard_use(tot, want, bnd), NM.HARD_LIMIT, what + f" unit statistics of {Cn} channels hard_use")
            if wl is not None:
                ratio, share = NM.stat_ratio(tot, NM.unit_stats_model(seg, unit, rpb, wl), want, fix, flt)
                margins.check(ratio, NM.RATIO_LIMIT, what + f" unit statistics of {Cn} channels: error over the fixed-point model's, {share:.2f} of the entries")
        off += Cn
    # the consumer, per group; no SiLU, so the rstd it used can be read back from its output
    ref = NM.GroupNormRef(cat.double(), gamma.double(), beta.double(), C, G, 1e-5, False)
    ops.GN_LAUNCH_LOG = []
    try:
        out = ops.groupnorm(cat, gamma, beta, G, 1e-5, False, C=C)
        p = ops.GN_LAUNCH_LOG[-1]["params"]
        assert p.colstats[0].stats and bool(p.colstats[0].ustats) == units, "the GroupNorm must have taken the producer's statistics"
    finally:
        ops.GN_LAUNCH_LOG = None
    torch.cuda.synchronize()
    if units:
        d, cnt = NM.depth("units", HW, C, G, rpb=rpbs, unit=unit), NM.unit_contributions(HW, C // G, unit, min(rpbs), wl)
    else:
        d, cnt = NM.depth("cols", HW, C, G, rpb=rpbs), 0
    mdl = ref.model()
    m = _assert_gn(ref, out, mdl, d, f"groupnorm from {'unit' if units else 'column'} statistics, {what}", kind, cnt)
    if kind not in NM.STRESS_KINDS:
        margins.check(m["hard_use"], NM.HARD_LIMIT, f"groupnorm from {'unit' if units else 'column'} statistics, {what}: hard_use again,"
                      f"{_rstd_text(ref, out, mdl)} recorded")


@pytest.mark.parametrize("rows,C,N,tile", [(96, 64, 64, 0), (200, 192, 320, 0), (130, 640, 1280, 38), (300, 640, 640, 58), (300, 640, 640, 64)])
def test_linear_row_statistics_per_row(ops, cuda, rows, C, N, tile):
    g = NM._gen(rows, C, N, tile)
    x = torch.randn(1, rows, C, generator=g).bfloat16().to(cuda)
    pw = ops.pack_weight(torch.randn(N, C, generator=g) * 0.1, torch.randn(N, generator=g) * 0.5 + 2.0, device=cuda)
    res = (torch.randn(1, rows, N, generator=g) + 0.7).bfloat16().to(cuda)
    y, st = ops.linear(x, pw, residual=res, rowstats=True, tile=tile, split_k=1)
    torch.cuda.synchronize()
    tot = st.double().sum(0)
    want, bnd = NM.row_stats_ref(y[0].double())
    got = torch.stack([tot[:, 0] + tot[:, 2], tot[:, 1] + tot[:, 3]], -1)
    margins.check(NM.hard_use(got, want, bnd), NM.HARD_LIMIT, f"row statistics {rows}x{C}->{N} tile {tile} hard_use")


# ---------------------------------------------------------------------------------------------------------------------
# the GroupNorm of the split-K reduce launch and the LayerNorm folded into a linear layer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "offset16", "offset32", "offset64"])
@pytest.mark.parametrize("B,H,Cin,N,G,silu", [(2, 8, 320, 88, 11, True), (2, 16, 128, 64, 16, False)])
def test_groupnorm_in_the_splitk_reduce_per_group(ops, cuda, B, H, Cin, N, G, silu, kind):
    """conv_gemm(gn=...) with the reduce launch normalising (splitk_reduce_gn_kernel) against GroupNorm of the bf16 tensor the
    plain reduce launch stores for the same slices (conv_gemm.hip:771, :788: bit-identical sums, the same rounding)"""
    g = NM._gen(B, H, Cin, N, len(kind))
    x = torch.randn(B, H, H, Cin, generator=g).bfloat16().to(cuda)
    bias = _producer_bias((N,), G, kind, g)
    pw = ops.pack_weight(torch.randn(N, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin), bias, device=cuda)
    rb = (torch.randn(B, pw.N, generator=g) * 0.2).to(cuda).contiguous()
    gamma, beta = (1.0 + 0.2 * torch.randn(N, generator=g)).to(cuda), (0.3 * torch.randn(N, generator=g)).to(cuda)
    old = (ops.FUSE_GN_REDUCE, ops.SPLITK_IN_KERNEL)
    try:
        ops.FUSE_GN_REDUCE, ops.SPLITK_IN_KERNEL, ops.LAUNCH_LOG = True, False, []
        fused = ops.conv_gemm(x, pw, rowbias=rb, gn=(gamma, beta, G, 1e-5, silu, N), split_k=4)
        assert ops.LAUNCH_LOG[-1]["params"].gn_gamma, "the reduce launch must have carried the normalisation"
        conv = ops.conv_gemm(x, pw, rowbias=rb, split_k=4)
        assert ops.LAUNCH_LOG[-1]["params"].split_k == 4 and not ops.LAUNCH_LOG[-1]["params"].tile_counters
    finally:
        ops.FUSE_GN_REDUCE, ops.SPLITK_IN_KERNEL = old
        ops.LAUNCH_LOG = None
    torch.cuda.synchronize()
    ref = NM.GroupNormRef(conv.double(), gamma.double(), beta.double(), N, G, 1e-5, silu)
    _assert_gn(ref, fused, ref.model(), NM.depth("reduce", H * H, N, G), f"groupnorm in the split-K reduce {B}x{H}x{H}x{N}g{G} {kind}", kind)


@pytest.mark.parametrize("kind", ["plain", "offset4", "offset16"])
@pytest.mark.parametrize("rows,C,N,split_k", [(200, 320, 384, 1), (130, 640, 1280, 2)])
def test_linear_with_folded_layernorm_per_row(ops, cuda, rows, C, N, split_k, kind):
    """linear(LayerNorm(x)) in one launch: mean / rstd from the producer's row statistics in ONE pass (ln_finish), then
    rstd * (acc - mean * colsum).  split_k 2 goes through the reduce launch, which folds the row statistics itself
    (conv_gemm.hip:738-742).  Rows with a mean of 4 and 16 spreads come from the producer's bias."""
    g = NM._gen(rows, C, N, split_k, len(kind))
    gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    src = torch.randn(1, rows, 64, generator=g).bfloat16().to(cuda)
    shift = {"plain": 0.4, "offset4": 4.0, "offset16": 16.0}[kind]
    x, st = ops.linear(src, ops.pack_weight(torch.randn(C, 64, generator=g) * 0.125, torch.full((C,), shift), device=cuda), rowstats=True, split_k=1)
    pw = ops.pack_weight(torch.randn(N, C, generator=g) * 0.06, torch.randn(N, generator=g) * 0.2, device=cuda, ln_gamma=gamma, ln_beta=beta)
    old = ops.SPLITK_IN_KERNEL
    try:
        ops.SPLITK_IN_KERNEL = split_k == 1
        y = ops.linear(x, pw, ln=(st, 1e-5), split_k=split_k)
    finally:
        ops.SPLITK_IN_KERNEL = old
    torch.cuda.synchronize()
    w = pw.w.double().reshape(pw.N, -1)[:, :C]
    ref = NM.FoldedLayerNormRef(x[0].double(), w, pw.bias.double(), pw.ln_colsum.double(), 1e-5)
    d = NM.depth("lnfold", 0, C, 0, slots=2 * st.shape[0])
    _assert_ln(ref, y[0], ref.model(), f"linear with folded layernorm {rows}x{C}->{N} split_k {split_k} {kind}", d)
