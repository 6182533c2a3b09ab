"""Elementwise and per-tile accuracy of the MFMA contraction kernels (ops.conv_gemm / ops.linear through every kernel family,
ops._wgrad_direct / ops.conv_wgrad) against the fp64 reference, the hard bound and the bf16 format model of tests/gemm_model.py,
all evaluated in fp64 on the device from the same bf16 operands.  tests/test_gemm_model_host.py proves on the CPU that these
metrics pass the sound forms of the model and fail each seeded defect -- among them a truncating bf16 store and a lost K-step,
which the whole-tensor rel-L2 <= 4e-3 of tests/test_ops_gpu.py lets through.

Every assertion goes through margins.check; the text names the tile id and split-K depth that ops.LAUNCH_LOG recorded for the
launch, so the committed record (profiles/gemm_parity_margins.json) shows which kernel families really ran.  No test here
repeats a launch to look for nondeterminism."""
import pytest
import torch

from tests import gemm_model as GM
from tests import margins
from tests import tiles

pytestmark = pytest.mark.gpu

HALO_TILES = tiles.HALO
WIDE160_TILES = tiles.WIDE160                          # GEGLU refuses them
SK_TILES = tiles.SK
# (family, tile id of include/aptp_hip.h, split_k or None = the case's own, ops.EPILOGUE)
FAMILIES = [
    ("staged", 2, None, 0), ("staged", 6, None, 0),
    ("lds-dma", 9, None, 0),
    ("lds-dma3/lean3x3", 18, None, 0),                 # a 3x3 convolution takes csrc/conv_lean.hip on this tile
    ("pingpong/lean3x3", 34, None, 0),                 # the same for the ping-pong tile ...
    ("pingpong", 34, None, 1),                         # ... and EPILOGUE 1 keeps it on the general kernel
    ("halo", 43, None, 0),
    ("ring8", 46, None, 0),
    ("ku2", 50, None, 0),
    ("ks2", 59, None, 0),
    ("streamk", 64, 1, 0), ("streamk", 64, 2, 0), ("streamk", 65, 1, 0), ("streamk", 65, 2, 0), ("streamk", 66, 1, 0), ("streamk", 66, 2, 0),
    ("streamk-l", 68, 1, 0), ("streamk-l", 68, 2, 0),
    ("streamk-128", 72, 1, 0), ("streamk-128", 72, 2, 0),
    ("auto", 0, None, 0),
]
# plain linear layers: the tiles csrc/lin_gemm.hip instantiates (LIN_TILES of tests/test_ops_gpu.py), one per tile shape and ring
LIN_FAMILIES = [("lean-linear 64x64", 12, None, 0), ("lean-linear 64x64 ku2", 49, None, 0), ("lean-linear 64x128", 15, None, 0),
                ("lean-linear 128x64", 26, None, 0)]
# (both are hand-picked: one id per kernel family; what must hold is that the table knows them)
assert {t for _, t, _, _ in FAMILIES} <= {0, *tiles.ALL} and {t for _, t, _, _ in LIN_FAMILIES} <= set(tiles.LIN)
assert {t for f, t, _, _ in FAMILIES if f.startswith("streamk")} <= set(SK_TILES)
assert {t for f, t, _, _ in FAMILIES if "lean3x3" in f} <= set(tiles.C3)


def _statically_refused(case, tile):
    """combinations aptp_conv_gemm refuses by its documented rules (include/aptp_hip.h): not generated at all"""
    B, H, W, Cin, Cout, k = case.shape
    if case.only_tiles is not None and tile not in case.only_tiles:
        return True
    if tile in HALO_TILES:
        prob_w = W << (1 if case.ups or case.dgrad else 0)
        plain3x3 = k == 3 and case.stride == 1 and not case.ups and not case.dgrad and not case.pad_end and not case.Cin2
        return not (plain3x3 and prob_w in (16, 32, 64) and (H * prob_w) % 128 == 0)
    if case.geglu and tile in WIDE160_TILES:
        return True
    return False


def _params():
    out = []
    for index, case in enumerate(GM.CASES):
        fams = FAMILIES + (LIN_FAMILIES if case.linear else [])
        epis = (0, 1) if case.epilogue else (None,)
        for fam, tile, fsplit, fepi in fams:
            if _statically_refused(case, tile):
                continue
            split = fsplit if tile in SK_TILES else case.split_k
            both = tile not in SK_TILES and split != 1 and (split is not None or case.name.startswith("largestK"))
            for epi in epis:
                if epi is not None and fepi == 1:
                    continue                      # (the epilogue cases sweep EPILOGUE themselves)
                e = fepi if epi is None else epi
                for in_kernel in ((True, False) if both else (True,)):
                    pid = f"{case.name}-{fam}-t{tile}-sk{split if split is not None else 'auto'}-epi{e}" + ("" if in_kernel else "-reduce")
                    out.append(pytest.param(index, fam, tile, split, e, in_kernel, id=pid))
    return out


@pytest.fixture(scope="module")
def ops(cuda):
    from diffusion_pruning_amd import ops as o
    o._lib.load()
    return o


_REF = {}
ATTEMPTED, RAN = {}, {}          # tile id asked for -> launches attempted / launches the library accepted


def reference(index, cuda):
    """(problem on the device, extra, ref, bound, format model) of GM.CASES[index]; computed once, never modified.  The model is
    evaluated with fp64 accumulation: its distance from the reference is then the bf16 store alone, which is what the tile
    ratio divides by (the host test shows fp32 accumulation in any order changes that distance by < 0.1 %)."""
    if index not in _REF:
        prob, extra = GM.make_problem(index)
        prob = prob.to(cuda)
        ref, bnd = GM.ref_and_bound(prob)
        _REF[index] = (prob, extra, ref, bnd, GM.model(prob, torch.float64))
    return _REF[index]


def _dev(t, cuda, dtype):
    return None if t is None else t.to(device=cuda, dtype=dtype).contiguous()


def launch(ops, cuda, index, tile, split_k, views=None, act_dtype=torch.bfloat16):
    """ops.conv_gemm of GM.CASES[index] -> (y [B, Hout, Wout, n_out] without the packing's pad columns, pad columns or None,
    'tile / split_k' as ops.LAUNCH_LOG recorded them).  ``views``: a function (name, tensor) -> tensor that places an operand
    inside a wider buffer."""
    case = GM.CASES[index]
    prob, extra = reference(index, cuda)[:2]
    f32 = torch.float32
    if case.dgrad:
        pw = ops.pack_weight_dgrad(extra["w_forward"].float(), device=cuda)
    elif case.geglu == "compact":
        pw = ops.pack_weight(extra["w_full"].float(), extra["bias_full"].float(), geglu=True, out_idx=extra["keep"], device=cuda)
    else:
        bias = extra.get("bias1", prob.bias)
        pw = ops.pack_weight(prob.w.float(), None if bias is None else bias.float(), geglu=prob.act == GM.ACT_GEGLU, device=cuda)
        if prob.x2 is not None:
            pw = ops.pack_weight_cat(pw, prob.w2.float(), extra["bias2"].float())
    place = views or (lambda name, t: t)
    kw = dict(stride=prob.stride, pad=prob.pad, pad_end=prob.pad_end, ups=prob.ups, tile=tile, split_k=split_k, out_f32=prob.out_f32)
    if prob.act == GM.ACT_SILU:
        kw["act"] = ops.ACT_SILU
    if prob.x2 is not None:
        kw["x2"] = place("x2", _dev(prob.x2, cuda, act_dtype))
    if prob.rowbias is not None:
        kw["rowbias"] = _dev(prob.rowbias, cuda, f32)
    if prob.colgate is not None:
        kw.update(colgate=_dev(prob.colgate, cuda, f32), gate_group=prob.gate_group)
    if prob.corr is not None:
        kw["corr"] = _dev(prob.corr, cuda, f32)
    if prob.residual is not None:
        kw["residual"] = place("residual", _dev(prob.residual, cuda, act_dtype))
    if prob.depth is not None:
        kw.update(depth=_dev(prob.depth, cuda, f32), depth_in=place("depth_in", _dev(prob.depth_in, cuda, act_dtype)))
    B, _, _, _, _, Hout, Wout = prob.geometry
    n_pack = pw.N // 2 if pw.geglu else pw.N
    if views is not None:
        kw["out"] = place("out", torch.empty(B, Hout, Wout, n_pack, dtype=f32 if prob.out_f32 else torch.bfloat16, device=cuda))
    ATTEMPTED[tile] = ATTEMPTED.get(tile, 0) + 1
    ops.LAUNCH_LOG = []
    try:
        y = ops.conv_gemm(place("x", _dev(prob.x, cuda, act_dtype)), pw, **kw)
        p = ops.LAUNCH_LOG[-1]["params"]
        ran = f"tile {p.tile} split_k {p.split_k}" + (" in-kernel" if p.split_k > 1 and p.tile_counters else "")
    finally:
        ops.LAUNCH_LOG = None
    torch.cuda.synchronize()
    RAN[tile] = RAN.get(tile, 0) + 1
    n = prob.n_out
    return y[..., :n], (y[..., n:] if y.shape[-1] > n else None), ran


def _refused(ops, fn):
    """run fn(); a launch the library refuses with APTP_EINVAL (nothing was launched) skips the combination"""
    try:
        return fn()
    except ops._lib.AptpError as e:
        if "rc=-1" in str(e):
            pytest.skip(f"refused by aptp_conv_gemm: {e}")
        raise


@pytest.mark.parametrize("index,family,tile,split_k,epilogue,in_kernel", _params())
def test_conv_gemm_elementwise_and_per_tile(ops, cuda, index, family, tile, split_k, epilogue, in_kernel):
    prob, _, ref, bnd, mdl = reference(index, cuda)
    ops.EPILOGUE, ops.SPLITK_IN_KERNEL = epilogue, in_kernel
    try:
        y, pad_cols, ran = _refused(ops, lambda: launch(ops, cuda, index, tile, split_k))
    finally:
        ops.EPILOGUE, ops.SPLITK_IN_KERNEL = 0, True
    assert tuple(y.shape) == tuple(ref.shape)
    if pad_cols is not None:
        assert float(pad_cols.float().abs().max()) == 0.0, "padding columns of the packed weight must come out as exact zeros"
    what = f"{GM.CASES[index].name} [{family}: {ran}]"
    hu = GM.hard_use(y, ref, bnd)
    tr = GM.tile_ratio(y, mdl, ref, bnd)
    print(f"{what}: hard_use {hu:.4f} tile_ratio {tr:.4f} rel_l2 {GM.rel_l2(y, ref):.3e}")
    margins.check(hu, GM.HARD_LIMIT, what + " hard_use")
    if prob.out_f32:
        # no bf16 store to model: the ratio (against an fp32 store of the fp64 value) is reported, not asserted
        margins.check(hu, GM.HARD_LIMIT, what + f" hard_use again, fp32 output: tile_ratio {tr:.3f} reported only")
    else:
        margins.check(tr, GM.RATIO_LIMIT, what + " tile_ratio")


def test_every_kernel_family_asked_for_has_run(ops, cuda):
    """after the sweep above (same module, same process): no tile id was refused for every case it was tried on, and a full
    run has been through every family of FAMILIES and LIN_FAMILIES"""
    if not ATTEMPTED:
        return                   # selected on its own: there is no sweep to account for
    never = sorted(t for t in ATTEMPTED if not RAN.get(t))
    assert not never, f"tiles refused on every case: {never}"
    if sum(ATTEMPTED.values()) >= len(_params()):
        assert set(RAN) >= {t for _, t, _, _ in FAMILIES + LIN_FAMILIES}


# one case per kernel family: every tensor operand a channel slice of a wider NaN-filled buffer, the output a slice of a buffer
# that holds a sentinel bit pattern
VIEW_FAMILIES = [(2, None), (6, 2), (9, None), (18, None), (34, None), (34, 3), (43, None), (46, None), (50, 2), (59, None),
                 (64, 2), (66, 1), (68, 2), (72, 1), (0, None)]
SENTINEL = 0x5A5B


@pytest.mark.parametrize("epilogue", [0, 1], ids=["epi-auto", "epi-acc-layout"])
@pytest.mark.parametrize("tile,split_k", VIEW_FAMILIES)
def test_strided_views_are_bit_equal_and_write_nothing_outside(ops, cuda, tile, split_k, epilogue):
    # corr + residual + depth lerp, with the second operand wherever the tile takes one (the halo tiles do not)
    index = GM.case_index("epi-lerp-2x16x16x320x136" if tile in HALO_TILES else "x2-lerp-2x16x16x72x136")
    wide = {}

    def place(name, t):
        lo = {"x": 8, "x2": 16, "residual": 24, "depth_in": 8, "out": 40}[name]
        C = t.shape[-1]
        if name == "out":
            buf = torch.empty(*t.shape[:-1], C + 96, dtype=t.dtype, device=t.device)
            buf.view(torch.int16).fill_(SENTINEL)
        else:
            buf = torch.full((*t.shape[:-1], C + 64), float("nan"), dtype=t.dtype, device=t.device)
            buf[..., lo:lo + C] = t
        wide[name] = (buf, lo, C)
        return buf[..., lo:lo + C]

    ops.EPILOGUE = epilogue
    try:
        want, _, ran0 = _refused(ops, lambda: launch(ops, cuda, index, tile, split_k))
        got, _, ran = _refused(ops, lambda: launch(ops, cuda, index, tile, split_k, views=place))
    finally:
        ops.EPILOGUE = 0
    assert ran == ran0
    assert torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)), ran
    buf, lo, C = wide["out"]
    bits = buf.view(torch.int16)
    assert bool((bits[..., :lo] == SENTINEL).all()) and bool((bits[..., lo + C:] == SENTINEL).all()), ran
    prob, _, ref, bnd, mdl = reference(index, cuda)
    margins.check(GM.hard_use(got, ref, bnd), GM.HARD_LIMIT, f"views [{ran}] hard_use")
    margins.check(GM.tile_ratio(got, mdl, ref, bnd), GM.RATIO_LIMIT, f"views [{ran}] tile_ratio")


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("name,split_k", [("ragged-3x7x5x72x40", 1), ("ups1-2x8x8x128x128", 2), ("epi-lerp-2x16x16x320x136", 1)])
def test_fp32_parity_instantiation_elementwise(ops, cuda, monkeypatch, name, split_k, tile):
    """io_f32 (exact-fp32 MFMAs through the same gather / tap walk / split-K / epilogue code as the register-staged tiles), fed
    the same bf16-valued operands.  Only the hard bound, with U_out = 2^-24: there is no bf16 store to model.  The bound is
    n * 2^-24 * S with n = K + 8 <= 3088 here, i.e. at most 2^-12.4 of the sum of absolute products, while ONE dropped or
    misplaced product changes the result by a typical |x w| = S / K: K^2 * 2^-24 <= 0.5 at these K (0.03, 0.08 and 0.5), so a
    single wrong term already exceeds the bound."""
    index = GM.case_index(name)
    prob = reference(index, cuda)[0]
    monkeypatch.setattr(ops, "ACT_DTYPE", torch.float32)
    y, _, ran = launch(ops, cuda, index, tile, split_k, act_dtype=torch.float32)
    assert y.dtype == torch.float32
    p32 = prob.to(cuda)
    p32.out_f32 = True
    ref, bnd = GM.ref_and_bound(p32)
    assert prob.K ** 2 * GM.U32 < 0.6
    margins.check(GM.hard_use(y, ref, bnd), GM.HARD_LIMIT, f"{name} io_f32 [{ran}] hard_use")


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------
WGRAD_CASES = [  # (B, H, W, C, N, k) of tests/test_bwd_ops_gpu.py
    (2, 64, 64, 64, 64, 3), (1, 32, 32, 320, 160, 3), (2, 16, 16, 128, 200, 3), (4, 8, 8, 72, 64, 3), (2, 32, 32, 320, 320, 1),
    (1, 308, 1, 1024, 136, 1), (1, 4, 1, 320, 1280, 1)]
_WREF = {}


def _wgrad_reference(key, cuda):
    """(x, dy as bf16 device tensors, dw, db, their bounds at split_m 64 -- the largest split the library chooses)"""
    if key not in _WREF:
        B, H, W, C, N, k, stride, ups = key
        g = torch.Generator().manual_seed(B * 7919 + H * 131 + C + N + k + 17 * stride + 29 * ups)
        Hx, Wx = (2 * H, 2 * W) if stride == 2 else ((H // 2, W // 2) if ups else (H, W))
        x = torch.randn(B, Hx, Wx, C, generator=g).bfloat16().to(cuda)
        dy = torch.randn(B, H, W, N, generator=g).bfloat16().to(cuda)
        dw, db = GM.wgrad_ref64(x.double(), dy.double(), k, stride, ups)
        bw, bb = GM.wgrad_bound(x.double(), dy.double(), k, stride, ups, split_m=64)
        _WREF[key] = (x, dy, dw, db, bw, bb)
    return _WREF[key]


# (split_m 3 of the four-row case would be more slices than 32-pixel K-steps: not generated)
@pytest.mark.parametrize("case,split", [(c, s) for c in WGRAD_CASES for s in (None, 1, 3)
                                        if s is None or s <= (c[0] * c[1] * c[2] + 31) // 32])
def test_wgrad_kernel_elementwise(ops, cuda, case, split):
    """aptp_conv_wgrad writes fp32 (fp32 slabs folded in fp32): hard bound with U_out = 2^-24 over a contraction of B*H*W"""
    B, H, W, C, N, k = case
    x, dy, dw, db, bw, bb = _wgrad_reference(case + (1, 0), cuda)
    got, gdb = ops._wgrad_direct(x, dy, k, k, split_m=split, want_db=True)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, k * k, C)
    margins.check(GM.hard_use(got, dw, bw), GM.HARD_LIMIT, f"wgrad {case} split_m {split} dw hard_use")
    margins.check(GM.hard_use(gdb, db, bb), GM.HARD_LIMIT, f"wgrad {case} split_m {split} db hard_use")


@pytest.mark.parametrize("kind,B,H,W,C,N", [("stride2", 2, 8, 8, 72, 136), ("ups", 2, 32, 32, 72, 136)])
def test_wgrad_resampling_elementwise(ops, cuda, kind, B, H, W, C, N):
    """H, W: the output map dy lives on; stride 2 reads x of twice, ups of half that extent"""
    stride, ups = (2, 0) if kind == "stride2" else (1, 1)
    x, dy, dw, db, bw, bb = _wgrad_reference((B, H, W, C, N, 3, stride, ups), cuda)
    assert ops._wgrad_direct(x, dy, 3, 3, stride=stride, ups=ups) is not None, "must take the kernel path"
    got, gdb = ops.conv_wgrad(x, dy, 3, 3, stride=stride, pad=1, ups=ups, want_db=True)
    torch.cuda.synchronize()
    margins.check(GM.hard_use(got, dw, bw), GM.HARD_LIMIT, f"wgrad {kind} dw hard_use")
    margins.check(GM.hard_use(gdb, db, bb), GM.HARD_LIMIT, f"wgrad {kind} db hard_use")
