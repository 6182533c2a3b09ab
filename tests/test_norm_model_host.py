"""CPU checks behind tests/test_norm_parity_gpu.py: tests/norm_model.py's fp64 references equal fp64 F.group_norm / F.layer_norm;
the kernels' arithmetic evaluated in fp32 -- one-pass statistics summed sequentially, pairwise and in the chunk order of the
three-launch kernels -- stays inside the hard bound on every data kind and at a tile ratio of ~1 on every non-stress kind; each
seeded defect of a kind a kernel could have fails one of the two metrics on the case named for it, with a record of whether the
whole-tensor rel-L2 <= 4e-3 of tests/test_ops_gpu.py would have let it through; at least 90 % of the (case, tile) pairs of the
non-stress kinds qualify for the ratio; and depth() is never below the chain the chunked order really has.  The figures are
printed as one table by the last test of the module; with NORM_MODEL_TABLE=<path> in the environment it is also written there
(the committed copy is profiles/norm_model_host_table.txt)."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import norm_model as NM

ROWS = []            # (case, form / defect, hard_use, tile_ratio, share, old rel-L2, verdict)
COVER = {}           # (case, kind) -> (ratio tiles, tiles) of the non-stress kinds
_REF, _LNREF = {}, {}
ORDERS = ("sequential", "pairwise", "chunked")
NONSTRESS = [k for k in NM.KINDS if k not in NM.STRESS_KINDS]


def reference(index, kind):
    """GroupNormRef of (GN_SHAPES[index], kind) and the chain of its three-launch path: computed once, never modified"""
    if (index, kind) not in _REF:
        s = NM.GN_SHAPES[index]
        _REF[(index, kind)] = (NM.gn_reference(index, kind), NM.depth("stats", s.HW, s.C, s.G))
    return _REF[(index, kind)]


def ln_reference(rows, C, kind):
    if (rows, C, kind) not in _LNREF:
        x, gamma, beta = NM.make_ln(rows, C, kind)
        _LNREF[(rows, C, kind)] = NM.LayerNormRef(x, gamma, beta, 1e-5)
    return _LNREF[(rows, C, kind)]


def _row(case, what, m, l2, verdict):
    ROWS.append((case, what, m["hard_use"], m["tile_ratio"], m["share"], l2, verdict))


def _fails(m):
    return m["hard_use"] > NM.HARD_LIMIT or m["tile_ratio"] > NM.RATIO_LIMIT


# ---------------------------------------------------------------------------------------------------------------------
# the references and the dispatch table are right
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("3x4x4x170g17", "plain"), ("2x16x16x340g17", "offset16"), ("2x4x4x64g32", "mixed"),
                                       ("1x8x8x2560g32", "outlier")])
def test_groupnorm_reference_equals_fp64_group_norm(name, kind):
    index = NM.shape_index(name)
    s = NM.GN_SHAPES[index]
    ref, _ = reference(index, kind)
    want = F.group_norm(ref.x[..., :s.C].permute(0, 3, 1, 2), s.G, ref.gamma, ref.beta, s.eps)
    want = (F.silu(want) if s.silu else want).permute(0, 2, 3, 1)
    assert float((ref.y[..., :s.C] - want).abs().max()) <= 1e-10 * float(want.abs().max())
    assert float(ref.y[..., s.C:].abs().sum()) == 0.0 and float(ref.bound(10)[0][..., s.C:].abs().sum()) == 0.0


@pytest.mark.parametrize("rows,C,kind", [(5, 64, "plain"), (130, 1536, "offset16"), (1, 2048, "tiny")])
def test_layernorm_reference_equals_fp64_layer_norm(rows, C, kind):
    ref = ln_reference(rows, C, kind)
    want = F.layer_norm(ref.x, (C,), ref.gamma, ref.beta, 1e-5)
    assert float((ref.y - want).abs().max()) <= 1e-10 * float(want.abs().max())


def test_folded_layernorm_reference_is_layernorm_then_linear():
    g = torch.Generator().manual_seed(5)
    x, gamma, beta = NM.make_ln(37, 192, "offset4")
    w = (torch.randn(40, 192, generator=g) * 0.07).double()
    b = torch.randn(40, generator=g).double()
    wf = (w * gamma).bfloat16().double()
    bf = (b + w @ beta).float().double()
    ref = NM.FoldedLayerNormRef(x, wf, bf, wf.sum(1).float().double(), 1e-5)
    want = F.linear(F.layer_norm(x, (192,), None, None, 1e-5), wf, bf)
    assert float((ref.y - want).abs().max()) <= 1e-10 * float(want.abs().max())
    # the kernels' formula in fp32, statistics in one pass: inside the bound
    x32, w32 = x.float(), wf.float()
    a, a2 = NM.sum_f32(x32, "sequential"), NM.sum_f32(x32 * x32, "sequential")
    mean = a * torch.tensor(1.0 / 192).float()
    var = (a2 * torch.tensor(1.0 / 192).float() - mean * mean).clamp_min(0)
    rstd = (var + 1e-5) ** -0.5
    got = (rstd[:, None] * (x32 @ w32.t() - mean[:, None] * ref.colsum.float()) + bf.float()).bfloat16().double()
    bnd, stat = ref.bound(NM.depth("lnfold", 0, 192, 0, slots=4))
    assert NM.hard_use(got, ref.y, bnd) <= NM.HARD_LIMIT
    bad = (rstd[:, None] * (x32 @ w32.t()) + bf.float()).bfloat16().double()          # the mean * colsum term forgotten
    assert NM.hard_use(bad, ref.y, bnd) > NM.HARD_LIMIT


DISPATCH = [  # shape -> (path of variant 0, of variant 2), read from aptp_groupnorm (norm.hip:658-748)
    ("2x4x4x64g32", ("group", dict(NT=256, U=4, gpb=4)), "group"),
    ("3x4x4x170g17", ("group", dict(NT=256, U=4, gpb=4)), "group"),
    ("2x16x16x85g17", ("group", dict(NT=256, U=8, gpb=8)), "group"),
    ("2x16x16x340g17", ("group", dict(NT=256, U=8, gpb=2)), "group"),
    ("1x12x16x2048g8", ("group", dict(NT=256, U=24, gpb=1)), "group"),
    ("1x16x16x2048g8", ("group", dict(NT=1024, U=8, gpb=1)), "group"),
    ("1x8x8x2560g32", ("group", dict(NT=256, U=4, gpb=1)), "group"),
    ("1x8x8x4096g32", ("group", dict(NT=256, U=4, gpb=1)), "group"),
    ("1x8x8x2112g8", ("stats", dict(NP=2, nchunk=16)), "refused"),
    ("2x5x7x320g32", ("group", dict(NT=256, U=4, gpb=4)), "group"),
    ("1x32x32x320g32", ("stats", dict(NP=1, nchunk=64)), "group"),
    ("1x64x64x320g32", ("stats", dict(NP=1, nchunk=128)), "refused"),
]


@pytest.mark.parametrize("name,auto,forced", DISPATCH)
def test_dispatch_table_reaches_the_paths_it_names(name, auto, forced):
    s = NM.GN_SHAPES[NM.shape_index(name)]
    path, info = NM.gn_dispatch(0, s.HW, s.C, s.G)
    assert path == auto[0] and all(info[k] == v for k, v in auto[1].items()), (path, info)
    assert NM.gn_dispatch(2, s.HW, s.C, s.G)[0] == forced
    assert NM.gn_dispatch(1, s.HW, s.C, s.G)[0] == "stats" and NM.gn_dispatch(3, s.HW, s.C, s.G)[0] in ("group", "stats3")
    assert NM.gn_dispatch(1, s.HW, s.C, s.G)[1]["NP"] == (2 if s.C > 2048 else 1)


@pytest.mark.parametrize("index", range(len(NM.GN_SHAPES)), ids=NM.GN_SHAPE_IDS)
def test_depth_is_at_least_the_chain_of_the_chunked_order(index):
    s = NM.GN_SHAPES[index]
    x = torch.ones(1, s.HW, s.G, s.C // s.G)
    for path, nchunk, fold in (("stats", NM.nchunk_of(s.HW), "lanes"), ("stats3", max(1, min(16, s.HW // 256)), "sequential")):
        total, chain = NM.chunked_group_sums(x, nchunk, fold)
        assert float(total[0, 0]) == s.HW * (s.C // s.G)
        assert NM.depth(path, s.HW, s.C, s.G) >= chain, (path, chain)
    # every chain is far below the element count (the point of the chunking) and at least the depth of a perfect tree
    n = s.HW * (s.C // s.G)
    for path in ("stats", "stats3") + (("group",) if NM.gn_dispatch(2, s.HW, s.C, s.G)[0] == "group" else ()):
        assert (n - 1).bit_length() <= NM.depth(path, s.HW, s.C, s.G) <= max(64, n // 8)


# ---------------------------------------------------------------------------------------------------------------------
# sound forms pass, seeded defects fail
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,kind", [(i, k) for i, s in enumerate(NM.GN_SHAPES) for k in s.kinds],
                         ids=[f"{s.name}-{k}" for s in NM.GN_SHAPES for k in s.kinds])
def test_groupnorm_sound_orders_stay_inside_the_bound_and_at_ratio_one(index, kind):
    s = NM.GN_SHAPES[index]
    ref, d = reference(index, kind)
    m64 = ref.model()
    stress = kind in NM.STRESS_KINDS
    # every order is held to the bound of ITS OWN longest chain: all n values, a perfect tree, the kernels' chunks
    chains = {"sequential": ref.n - 1, "pairwise": (ref.n - 1).bit_length(), "chunked": d}
    for order in ORDERS:
        got = ref.model(torch.float32, order)
        m = NM.measure_gn(ref, got, chains[order], model_out=m64)
        _row(f"{s.name} {kind}", f"fp32 one pass, {order} (d = {chains[order]})", m, NM.rel_l2(got, ref.y),
             "sound" + (" (stress: ratio recorded)" if stress else ""))
        assert m["hard_use"] <= NM.HARD_LIMIT, (s.name, kind, order, m)
        if not stress:
            assert m["tile_ratio"] <= NM.RATIO_LIMIT, (s.name, kind, order, m)
    m = NM.measure_gn(ref, m64, d, model_out=m64)              # the harmless, more exact variant
    assert m["hard_use"] <= NM.HARD_LIMIT and m["tile_ratio"] <= 1.0 + 1e-12
    if not stress:
        ok = ref.ratio_tiles(ref.bound(d)[1])
        COVER[(s.name, kind)] = (int(ok.sum()), ok.numel())


@pytest.mark.parametrize("kind", NM.LN_KINDS)
@pytest.mark.parametrize("rows,C", NM.LN_CASES)
def test_layernorm_sound_orders_stay_inside_the_bound_and_at_ratio_one(rows, C, kind):
    ref = ln_reference(rows, C, kind)
    m64 = ref.model()
    for order in ORDERS:
        got = ref.model(torch.float32, order)
        m = NM.measure_ln(ref, got, model_out=m64)
        _row(f"ln {rows}x{C} {kind}", f"fp32 two passes, {order}", m, NM.rel_l2(got, ref.y), "sound")
        assert m["hard_use"] <= NM.HARD_LIMIT and m["tile_ratio"] <= NM.RATIO_LIMIT, (rows, C, kind, order, m)
    ok = ref.ratio_tiles(ref.bound()[1])
    COVER[(f"ln {rows}x{C}", kind)] = (int(ok.sum()), ok.numel())


def test_at_least_nine_tenths_of_the_tiles_are_ratio_asserted():
    """on the reference alone (no kernel, no model output enters ratio_tiles)"""
    for index in range(len(NM.GN_SHAPES)):
        for kind in NONSTRESS:
            s = NM.GN_SHAPES[index]
            if kind in s.kinds and (s.name, kind) not in COVER:
                ref, d = reference(index, kind)
                ok = ref.ratio_tiles(ref.bound(d)[1])
                COVER[(s.name, kind)] = (int(ok.sum()), ok.numel())
    for rows, C in NM.LN_CASES:
        for kind in NM.LN_KINDS:
            if (f"ln {rows}x{C}", kind) not in COVER:
                ref = ln_reference(rows, C, kind)
                ok = ref.ratio_tiles(ref.bound()[1])
                COVER[(f"ln {rows}x{C}", kind)] = (int(ok.sum()), ok.numel())
    asserted, tiles = sum(a for a, _ in COVER.values()), sum(t for _, t in COVER.values())
    by_kind = {}
    for (_, kind), (a, t) in COVER.items():
        by_kind[kind] = (by_kind.get(kind, (0, 0))[0] + a, by_kind.get(kind, (0, 0))[1] + t)
    print({k: f"{a}/{t}" for k, (a, t) in by_kind.items()}, asserted, tiles)
    ROWS.append(("coverage", "ratio-asserted (case, tile) pairs: " + ", ".join(f"{k} {a}/{t}" for k, (a, t) in sorted(by_kind.items())),
                 0.0, 0.0, asserted / tiles, 0.0, f"{asserted}/{tiles}"))
    assert asserted >= 0.9 * tiles, (asserted, tiles, by_kind)


@pytest.mark.parametrize("name", list(NM.DEFECTS))
def test_metrics_see_the_seeded_groupnorm_defects(name):
    for sname, kind in (NM.DEFECTS[name],) + NM.DEFECT_ALSO.get(name, ()):
        index = NM.shape_index(sname)
        s = NM.GN_SHAPES[index]
        ref, d = reference(index, kind)
        got = ref.model(torch.float32, "chunked", _defect=name, seg0=s.seg0)
        assert not torch.equal(got, ref.model(torch.float32, "chunked")), "the defect does not touch this case"
        m = NM.measure_gn(ref, got, d)
        l2 = NM.rel_l2(got, ref.y)
        old = "old criterion passes" if l2 <= NM.OLD_REL_L2_TOL else "old criterion fails too"
        _row(f"{sname} {kind}", "DEFECT " + name, m, l2, ("caught; " if _fails(m) else "NOT CAUGHT; ") + old)
        assert _fails(m), (name, sname, kind, m)
        if name in NM.OLD_CRITERION_MUST_PASS and (sname, kind) == NM.DEFECTS[name]:
            assert l2 <= NM.OLD_REL_L2_TOL, (name, sname, l2)


@pytest.mark.parametrize("name", list(NM.LN_DEFECTS))
def test_metrics_see_the_seeded_layernorm_defects(name):
    rows, C, kind = NM.LN_DEFECTS[name]
    ref = ln_reference(rows, C, kind)
    got = ref.model(torch.float32, "chunked", _defect=name)
    m = NM.measure_ln(ref, got)
    l2 = NM.rel_l2(got, ref.y)
    old = "old criterion passes" if l2 <= NM.OLD_REL_L2_TOL else "old criterion fails too"
    _row(f"ln {rows}x{C} {kind}", "DEFECT " + name, m, l2, ("caught; " if _fails(m) else "NOT CAUGHT; ") + old)
    assert _fails(m), (name, m)


def test_unit_statistics_model_and_the_truncated_sum_of_squares():
    sname, kind, unit, rpb, wl = NM.UNIT_DEFECT_CASE
    ref, _ = reference(NM.shape_index(sname), kind)
    y = ref.x.reshape(ref.B, ref.HW, ref.Cp)[..., :ref.C]
    want, bnd, flt, fix = NM.unit_stats_ref(y, unit, rpb, wl)
    mdl = NM.unit_stats_model(y, unit, rpb, wl)
    for what, defect in (("fp32 partials, rounded", None), ("DEFECT unit_sumsq_truncated", "unit_sumsq_truncated")):
        got = NM.unit_stats_model(y, unit, rpb, wl, torch.float32, _defect=defect)
        hu = NM.hard_use(got, want, bnd)
        ratio, share = NM.stat_ratio(got, mdl, want, fix, flt)
        m = dict(hard_use=hu, tile_ratio=ratio, share=share)
        _row(f"units {sname} {kind}", what, m, 0.0, "sound" if defect is None else ("caught" if _fails(m) else "NOT CAUGHT"))
        assert _fails(m) == (defect is not None), (what, m)
    assert share >= 0.45                     # the sums of squares: on tiny data the grid, not fp32, is what rounds
    # the group totals of the model reproduce the reference's mean and variance to the fixed-point step
    tot = NM.group_sums_from_units(mdl, ref.C, ref.G, unit)
    assert float((tot[..., 0] / ref.n - ref.mean).abs().max()) <= NM.unit_contributions(ref.HW, ref.cg, unit, rpb, wl) * 2.0 ** -21 / ref.n
    # one entry per statistic and unit, also where a unit straddles two wave-column blocks (unit 8 on 200 + 312 columns)
    yy = torch.randn(1, 64, 512, generator=torch.Generator().manual_seed(3)).bfloat16().double()
    w2, b2, _, _ = NM.unit_stats_ref(yy, 8, 32, 80)
    assert NM.hard_use(NM.unit_stats_model(yy, 8, 32, 80, torch.float32), w2, b2) <= NM.HARD_LIMIT


def test_measure_flags_non_finite_and_pad_columns():
    ref, d = reference(NM.shape_index("3x4x4x170g17"), "plain")
    got = ref.model().clone()
    got[0, 0, 0, 172] = 2.0 ** -20                                 # a pad column that is not exact zero
    assert NM.measure_gn(ref, got, d)["hard_use"] == float("inf")
    got[0, 0, 0, 172] = float("nan")
    assert NM.measure_gn(ref, got, d)["tile_ratio"] == float("inf")
    clean = NM.GroupNormRef(*NM.make_gn(NM.shape_index("3x4x4x170g17"), "plain"), 170, 17, 1e-5, False)
    assert float(NM.rstd_error(clean, clean.y).abs().max()) <= 1e-12


def _table_lines():
    out = [f"Normalisation format model on the CPU: hard_use = max |got - ref| / bound (limit 1), tile_ratio = worst (sample, group) "
           f"or row rms error over the bf16 format error among the tiles where the store dominates (limit {NM.RATIO_LIMIT}), share = "
           f"those tiles' share, old = whole-tensor rel-L2 (tests/test_ops_gpu.py asserts <= {NM.OLD_REL_L2_TOL:g})",
           f"{'case':32s} {'form / defect':52s} {'hard_use':>9s} {'tile_ratio':>10s} {'share':>6s} {'old rel-L2':>10s}  verdict"]
    for case, what, hu, tr, share, l2, verdict in ROWS:
        out.append(f"{case:32s} {what:52s} {hu:9.3f} {tr:10.3f} {share:6.2f} {l2:10.2e}  {verdict}")
    return out


def test_print_the_measured_table(capsys):
    """last in the module: the figures the tests above measured, shown even when output is captured"""
    lines = _table_lines()
    with capsys.disabled():
        print()
        for line in lines:
            if "DEFECT" in line or "coverage" in line or line is lines[0] or line is lines[1] or os.environ.get("NORM_MODEL_TABLE"):
                print(line)
    path = os.environ.get("NORM_MODEL_TABLE")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
