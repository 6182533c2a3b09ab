"""CPU checks behind tests/test_gemm_parity_gpu.py: tests/gemm_model.py's fp64 reference equals fp64 F.conv2d / autograd with a
plain-torch epilogue for every option it covers; two sound forms of the format model (K in one pass; split-K slices of
64-channel chunks combined in slice order) stay inside the hard bound and at a tile ratio of ~1 on every case of the GPU list;
each seeded defect of a kind a kernel could have fails one of the two metrics on the case named for it -- with a record of
whether the whole-tensor rel-L2 <= 4e-3 of tests/test_ops_gpu.py would have let it through -- and the more exact variant (fp64
accumulation) passes.  The figures are printed as one table by the last test of the module; with GEMM_MODEL_TABLE=<path> in the
environment it is also written there (the committed copy is profiles/gemm_model_host_table.txt)."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_model as GM

SOUND_RATIO_LIMIT = 1.1
ROWS = []            # (case, form / defect, hard_use, tile_ratio, old rel-L2, verdict)
_REF = {}


def reference(index):
    """(problem, ref, bound, fp64 model) of CASES[index]: computed once per process, never modified"""
    if index not in _REF:
        prob, _ = GM.make_problem(index)
        ref, bnd = GM.ref_and_bound(prob)
        _REF[index] = (prob, ref, bnd, GM.model(prob, torch.float64))
    return _REF[index]


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _r(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).bfloat16().double()


# ---------------------------------------------------------------------------------------------------------------------
# the reference is right
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride,pad,pad_end,ups", [
    (3, 7, 5, 72, 40, 3, 1, 1, 0, 0), (2, 6, 6, 16, 24, 3, 2, 1, 0, 0), (2, 4, 5, 16, 8, 3, 1, 1, 0, 1),
    (2, 6, 6, 8, 8, 3, 2, 0, 1, 0), (2, 5, 3, 72, 16, 1, 1, 0, 0, 0), (1, 7, 6, 8, 8, 3, 2, 0, 1, 0),
    (1, 6, 6, 8, 16, 3, 2, 1, 1, 0)])
def test_ref64_convolution_equals_fp64_conv2d(B, H, W, Cin, Cout, k, stride, pad, pad_end, ups):
    g = _g(H * 100 + W * 10 + k + stride)
    x, w = _r((B, H, W, Cin), g), _r((Cout, Cin, k, k), g, 0.1)
    b = torch.randn(Cout, generator=g).double()
    got = GM.ref64(GM.Problem(x, w, b, stride=stride, pad=pad, pad_end=pad_end, ups=ups))
    xr = nchw(x)
    if ups:
        xr = F.interpolate(xr, scale_factor=2.0, mode="nearest")
    if pad_end:
        xr = F.pad(xr, (0, pad_end, 0, pad_end))
    want = nhwc(F.conv2d(xr, w, b, stride=stride, padding=pad))
    assert got.shape == want.shape
    assert _rel(got, want) <= 1e-12


@pytest.mark.parametrize("B,H,W,Cin,Cout,k", [(2, 8, 8, 16, 24, 3), (1, 6, 10, 8, 8, 3), (2, 16, 16, 128, 128, 3)])
def test_ref64_zero_insertion_is_the_data_gradient_of_stride_2(B, H, W, Cin, Cout, k):
    g = _g(H + W + Cin)
    x = _r((B, H, W, Cin), g).requires_grad_()
    w = _r((Cout, Cin, k, k), g, 0.1)
    y = F.conv2d(nchw(x), w, None, stride=2, padding=k // 2)
    dy = _r(tuple(y.shape), g)
    y.backward(dy)
    prob = GM.Problem(nhwc(dy).contiguous(), w.flip(2, 3).transpose(0, 1).contiguous(), None, stride=1, pad=k - 1 - k // 2, ups=2)
    got = GM.ref64(prob)
    assert got.shape == x.grad.shape
    assert _rel(got, x.grad) <= 1e-12


def test_ref64_epilogues_equal_plain_torch():
    """the two epilogues of test_conv_full_epilogue, the second operand, SiLU and both GEGLU forms, written out in plain torch"""
    g = _g(11)
    B, H, W, Cin, Cout, G = 4, 8, 8, 64, 64, 32
    x, w, b = _r((B, H, W, Cin), g), _r((Cout, Cin, 3, 3), g, 0.05), torch.randn(Cout, generator=g).double() * 0.1
    conv = F.conv2d(nchw(x), w, b, padding=1)
    temb = torch.randn(B, Cout, generator=g).double() * 0.5
    gate = torch.rand(2, G, generator=g).double()
    got = GM.ref64(GM.Problem(x, w, b, rowbias=temb, colgate=gate, gate_group=Cout // G))
    want = (conv + temb[:, :, None, None]) * gate.repeat_interleave(Cout // G, dim=1).repeat(2, 1)[:, :, None, None]
    assert _rel(got, nhwc(want)) <= 1e-12
    res, din = _r((B, H, W, Cout), g), _r((B, H, W, Cout), g)
    d = torch.rand(2, generator=g).double()
    corr = torch.randn(1, 9, Cout, generator=g).double() * 0.3
    got = GM.ref64(GM.Problem(x, w, b, corr=corr, residual=res, depth=d, depth_in=din))
    cls = torch.ones(H, dtype=torch.long); cls[0] = 0; cls[-1] = 2
    cmap = cls[:, None] * 3 + cls[None, :]
    want = nhwc(conv) + corr[0][cmap][None] + res
    dm = d.repeat(2)[:, None, None, None]
    want = (1 - dm) * din + dm * want
    assert _rel(got, want) <= 1e-12
    # every one of the nine border classes is met, each with its own vector
    Hn, Wn = 5, 4
    xs, ws = _r((1, Hn, Wn, 8), g), _r((8, 8, 3, 3), g, 0.1)
    corr9 = torch.arange(9).double()[None, :, None].expand(1, 9, 8).contiguous()
    got = GM.ref64(GM.Problem(xs, ws, None, corr=corr9)) - GM.ref64(GM.Problem(xs, ws, None))
    rows = torch.tensor([0] + [1] * (Hn - 2) + [2])
    cols = torch.tensor([0] + [1] * (Wn - 2) + [2])
    assert torch.allclose(got[0, :, :, 0], (rows[:, None] * 3 + cols[None, :]).double(), atol=1e-12)
    # second K segment
    x2, w2 = _r((B, H, W, 200), g), _r((Cout, 200), g, 0.05)
    got = GM.ref64(GM.Problem(x, w, b, x2=x2, w2=w2))
    want = conv + F.conv2d(nchw(x2), w2[:, :, None, None])
    assert _rel(got, nhwc(want)) <= 1e-12
    # SiLU; GEGLU with a width gate (test_linear_geglu); compact GEGLU = the live units of the full one
    got = GM.ref64(GM.Problem(x, w, b, act=GM.ACT_SILU))
    assert _rel(got, nhwc(F.silu(conv))) <= 1e-12
    L, C, inner = 96, 64, 256
    xl, wl, bl = _r((2, L, 1, C), g), _r((2 * inner, C, 1, 1), g, 0.125), torch.randn(2 * inner, generator=g).double() * 0.1
    gt = (torch.rand(2, 32, generator=g) > 0.3).double()
    got = GM.ref64(GM.Problem(xl, wl, bl, act=GM.ACT_GEGLU, colgate=gt, gate_group=inner // 32))
    h, gg = F.linear(xl[:, :, 0], wl[:, :, 0, 0], bl).chunk(2, dim=-1)
    m = gt.repeat_interleave(inner // 32, dim=1)[:, None, :]
    assert _rel(got[:, :, 0], (h * m) * F.gelu(gg * m)) <= 1e-12
    index = GM.case_index("geglu-compact-50x128x512")
    prob, extra = GM.make_problem(index)
    full = GM.ref64(GM.Problem(prob.x, extra["w_full"], extra["bias_full"], act=GM.ACT_GEGLU))
    assert torch.equal(GM.ref64(prob), full[..., extra["keep"]])


@pytest.mark.parametrize("B,H,W,C,N,k,stride,ups", [(2, 8, 8, 16, 24, 3, 1, 0), (1, 12, 1, 40, 16, 1, 1, 0), (2, 8, 8, 16, 8, 3, 2, 0),
                                                    (2, 4, 4, 8, 16, 3, 1, 1)])
def test_wgrad_ref64_equals_fp64_autograd(B, H, W, C, N, k, stride, ups):
    g = _g(B + H + C + N + k + stride + ups)
    x = _r((B, H, W, C), g)
    w = torch.zeros(N, C, k, k, dtype=torch.float64, requires_grad=True)
    xr = nchw(x)
    if ups:
        xr = F.interpolate(xr, scale_factor=2.0, mode="nearest")
    y = F.conv2d(xr, w, None, stride=stride, padding=k // 2)
    dy = _r(tuple(y.shape), g)
    y.backward(dy)
    dw, db = GM.wgrad_ref64(x, nhwc(dy).contiguous(), k, stride, ups)
    assert _rel(dw, w.grad.permute(0, 2, 3, 1).reshape(N, k * k, C)) <= 1e-12
    assert _rel(db, dy.sum(dim=(0, 2, 3))) <= 1e-12
    bw, bb = GM.wgrad_bound(x, nhwc(dy).contiguous(), k, stride, ups)
    dw32, db32 = GM.wgrad_ref64(x.float(), nhwc(dy).contiguous().float(), k, stride, ups)
    assert GM.hard_use(dw32, dw, bw) <= 1.0 and GM.hard_use(db32, db, bb) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the metrics: sound forms pass, seeded defects fail
# ---------------------------------------------------------------------------------------------------------------------
def _measure(got, index):
    prob, ref, bnd, m64 = reference(index)
    hu = GM.hard_use(got, ref, bnd)
    tr = None if prob.out_f32 else GM.tile_ratio(got, m64, ref, bnd)
    return hu, tr, GM.rel_l2(got, ref)


def _fails(hu, tr):
    return hu > GM.HARD_LIMIT or (tr is not None and tr > GM.RATIO_LIMIT)


def _row(case, what, hu, tr, l2, verdict):
    ROWS.append((case, what, hu, tr, l2, verdict))


@pytest.mark.parametrize("index", range(len(GM.CASES)), ids=GM.CASE_IDS)
def test_sound_models_stay_inside_the_bound_and_at_ratio_one(index):
    case = GM.CASES[index]
    prob = reference(index)[0]
    forms = [("fp32 one pass", dict(split_k=1)), ("fp32 split-K 5", dict(split_k=5))]
    for name, kw in forms:
        hu, tr, l2 = _measure(GM.model(prob, torch.float32, **kw), index)
        _row(case.name, name, hu, tr, l2, "sound")
        assert hu <= GM.HARD_LIMIT, (case.name, name, hu)
        assert tr is None or tr <= SOUND_RATIO_LIMIT, (case.name, name, tr)
    # the harmless variant -- more exact than the kernels -- passes too: the metrics are not merely tight
    hu, tr, l2 = _measure(GM.model(prob, torch.float64), index)
    _row(case.name, "fp64 accumulate (harmless)", hu, tr, l2, "sound")
    assert hu <= GM.HARD_LIMIT and (tr is None or tr <= SOUND_RATIO_LIMIT), (case.name, hu, tr)


@pytest.mark.parametrize("name", list(GM.DEFECTS))
def test_metrics_see_the_seeded_defects(name):
    for cname in (GM.DEFECTS[name],) + GM.DEFECT_ALSO.get(name, ()):
        index = GM.case_index(cname)
        prob = reference(index)[0]
        split_k = 4 if name == "splitk_slices_rounded_to_bf16" else 1
        got = GM.model(prob, torch.float32, split_k=split_k, _defect=name)
        assert not torch.equal(got, GM.model(prob, torch.float32, split_k=split_k)), "the defect does not touch this case"
        hu, tr, l2 = _measure(got, index)
        old = "old criterion passes" if l2 <= GM.OLD_REL_L2_TOL else "old criterion fails too"
        _row(cname, "DEFECT " + name, hu, tr, l2, ("caught; " if _fails(hu, tr) else "NOT CAUGHT; ") + old)
        assert _fails(hu, tr), (name, cname, hu, tr)
        if name in GM.OLD_CRITERION_MUST_PASS and cname == GM.DEFECTS[name]:
            assert l2 <= GM.OLD_REL_L2_TOL, (name, cname, l2)


def test_tile_ratio_keeps_the_ragged_tails_and_merges_slivers():
    ref = torch.zeros(65, 40, dtype=torch.float64)
    mdl = ref + 1.0
    bnd = torch.ones_like(ref)
    got = mdl.clone()
    r = GM.tile_ratios(got, mdl, ref, bnd)
    assert tuple(r.shape) == (2, 2)                     # 65 rows = 32 + 33 (the one-row sliver merged), 40 columns = 32 + 8
    got[64, 39] = 30.0                                  # one bad element in the merged corner tile of 33 x 8
    r = GM.tile_ratios(got, mdl, ref, bnd)
    assert float(r[1, 1]) > 1.25 and float(r[0, 0]) == 1.0 and float(r[0, 1]) == 1.0 and float(r[1, 0]) == 1.0
    # exactly representable outputs: the floor takes over, a tiny difference passes and a real one does not
    zero = torch.zeros(32, 32, dtype=torch.float64)
    one = torch.ones_like(zero)
    assert GM.tile_ratio(zero + 2.0 ** -14, zero, zero, one) <= 1.0
    assert GM.tile_ratio(zero + 2.0 ** -10, zero, zero, one) > 1.25
    assert GM.hard_use(zero + 1e-30, zero, zero) == math.inf and GM.hard_use(zero, zero, zero) == 0.0
    assert GM.hard_use(zero + float("nan"), zero, one) == math.inf


def _table_lines():
    out = ["GEMM format model on the CPU: hard_use = max |got - ref| / bound (limit 1), tile_ratio = worst 32x32-tile rms error over "
           f"the bf16 format error (limit {GM.RATIO_LIMIT}; sound forms asserted <= {SOUND_RATIO_LIMIT}), old = whole-tensor rel-L2 "
           f"(tests/test_ops_gpu.py asserts <= {GM.OLD_REL_L2_TOL:g})",
           f"{'case':28s} {'form / defect':58s} {'hard_use':>9s} {'tile_ratio':>10s} {'old rel-L2':>10s}  verdict"]
    for case, what, hu, tr, l2, verdict in ROWS:
        trs = "   (fp32)" if tr is None else f"{tr:10.3f}"
        out.append(f"{case:28s} {what:58s} {hu:9.3f} {trs:>10s} {l2:10.2e}  {verdict}")
    return out


def test_print_the_measured_table(capsys):
    """last in the module: the figures the tests above measured, shown even when output is captured"""
    lines = _table_lines()
    with capsys.disabled():
        print()
        for line in lines:
            print(line)
    path = os.environ.get("GEMM_MODEL_TABLE")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
