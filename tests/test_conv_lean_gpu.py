"""The lean 3x3 kernel (csrc/conv_lean.hip) against conv_gemm_dma_kernel on the same tile and split: the two share the K order,
MFMA mapping, split-K slab layout and epilogue order, so y and the unit statistics (integer atomics) must be bit-identical and
the column statistics equal up to summation order.  AptpConvGemmParams.epilogue = 2 keeps a launch on the general kernel.
Reference call sites of the convolutions: blocks.py:331,362 (ResnetBlock2D), unet.py:375-475."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from oracle import unet_oracle as O
from tests.tiles import C3 as LEAN_TILES               # the tiles csrc/conv_lean.hip instantiates

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clone(p):
    return type(p).from_buffer_copy(p)


def _run_both(lib, p, cuda, what):
    """Launch p on the lean kernel (epilogue 0) and on the general kernel (epilogue 2), each into fresh outputs / statistics /
    split-K workspace / counters.  Returns {side: (y, colstats, unitstats)}."""
    from diffusion_pruning_amd import _lib
    M = p.B * p.Hout * p.Wout
    nout = p.N // 2 if p.act == 2 else p.N
    outs = {}
    for side, epi in (("lean", 0), ("general", 2)):
        q = _clone(p)
        q.epilogue = epi
        q.prefetch, q.prefetch_bytes = None, 0
        y = torch.full((M, nout), float("nan"), dtype=torch.bfloat16, device=cuda)
        q.y, q.ldy, q.out_f32 = y.data_ptr(), nout, 0
        keep = [y]
        cs = us = None
        if p.colstat_out:
            rows = lib.aptp_conv_gemm_colstat_rows(ctypes.byref(q))
            cs = torch.zeros(M // rows, q.colstat_ld, 2, dtype=torch.float32, device=cuda)
            q.colstat_out = cs.data_ptr()
        if p.ustat_out:
            us = torch.zeros(q.ustat_nrep * q.B * q.ustat_units * 2, dtype=torch.int64, device=cuda)
            q.ustat_out = us.data_ptr()
        if p.split_k > 1:
            ws = torch.empty(lib.aptp_conv_gemm_workspace_bytes(ctypes.byref(q)) // 4 + 64, dtype=torch.float32, device=cuda)
            q.workspace = ws.data_ptr()
            keep.append(ws)
            if p.tile_counters:
                ctr = torch.zeros(lib.aptp_conv_gemm_tiles(ctypes.byref(q)) + 64, dtype=torch.int32, device=cuda)
                q.tile_counters = ctr.data_ptr()
                keep.append(ctr)
        _lib.check(lib.aptp_conv_gemm(ctypes.byref(q), torch.cuda.current_stream().cuda_stream), what + f" [{side}]")
        torch.cuda.synchronize()
        outs[side] = (y, cs, us, keep)
    return outs


def _assert_same(outs, what):
    (y0, c0, u0, _), (y1, c1, u1, _) = outs["lean"], outs["general"]
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16)), (what, int((y0 != y1).sum()))
    if c0 is not None:
        assert torch.allclose(c0, c1, rtol=1e-5, atol=1e-4), (what, float((c0 - c1).abs().max()))
    if u0 is not None:
        assert torch.equal(u0, u1), what


@pytest.fixture(scope="module")
def headline_log(cuda):
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    model = UNet2DConditionModelGated().init_synthetic(seed=0).to(cuda)
    model.set_structure({k: [v.to(cuda) for v in vs] for k, vs in O.fixed_half_mask(O.SD21).items()})
    sample, t, ehs = O.synthetic_inputs(O.SD21, 4, 64, seed=5)
    with torch.no_grad():
        model(sample.to(cuda), t.to(cuda), ehs.to(cuda))
        ops.LAUNCH_LOG = []
        try:
            model(sample.to(cuda), t.to(cuda), ehs.to(cuda))
            torch.cuda.synchronize()
            log = ops.LAUNCH_LOG
        finally:
            ops.LAUNCH_LOG = None
    return model, log


def test_every_headline_3x3_launch_lean_equals_general(headline_log, cuda):
    from diffusion_pruning_amd import _lib
    lib = _lib.load()
    _, log = headline_log
    seen, tiles, forms = set(), set(), set()
    for r in log:
        if "fn" in r:
            continue
        p = r["params"]
        if p.KH != 3 or p.tile < 7:
            continue
        key = (p.B * p.Hout * p.Wout, p.N, p.Cin, p.stride, p.ups, p.act, p.Cin2, p.tile, p.split_k, bool(p.residual),
               bool(p.rowbias), bool(p.corr), bool(p.colgate), bool(p.depth), bool(p.tile_counters), bool(p.gn_gamma), bool(p.colstat_out))
        if key in seen:
            continue
        seen.add(key)
        tiles.add(p.tile)
        forms.add("in-kernel" if p.tile_counters else ("gn" if p.gn_gamma else "reduce") if p.split_k > 1 else "one")
        what = f"M{key[0]} N{p.N} Cin{p.Cin} s{p.stride} u{p.ups} x2 {p.Cin2} tile {p.tile} split {p.split_k}"
        _assert_same(_run_both(lib, p, cuda, what), what)
    assert len(seen) >= 20, len(seen)
    assert tiles & set(LEAN_TILES), tiles


def _pw(cuda, cin, cout, cin2=0, seed=0):
    from diffusion_pruning_amd import ops
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(cuda)
    b = (torch.randn(cout, generator=g) * 0.1).to(cuda)
    pw = ops.pack_weight(w, b)
    if cin2:
        pw = ops.pack_weight_cat(pw, (torch.randn(cout, cin2, generator=g) / cin2 ** 0.5).to(cuda))
    return pw


def _act(cuda, *shape, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(cuda).to(torch.bfloat16)


# (B, H, W, Cin, N, stride, ups, tile, split_k, extras)
MATRIX = [
    (4, 64, 64, 320, 320, 1, 0, 34, 1, ""),            # level 64
    (4, 32, 32, 640, 640, 1, 0, 28, 1, "rowbias gate"),
    (4, 32, 32, 640, 640, 1, 0, 19, 1, "rowbias gate"),        # tile 19: stays on the general kernel
    (4, 16, 16, 1280, 1280, 1, 0, 28, 2, ""),           # level 16, split along K
    (4, 64, 64, 320, 320, 2, 0, 40, 1, ""),             # stride 2
    (4, 16, 16, 640, 640, 1, 1, 30, 1, "silu"),         # nearest x2
    (4, 16, 16, 320, 256, 1, 2, 18, 1, ""),             # zero insertion
    (4, 32, 32, 640, 640, 1, 0, 56, 1, "x2 corr residual"),
    (4, 32, 32, 640, 640, 1, 0, 28, 1, "x2 corr depth"),         # depth lerp: stays on the general kernel
    (2, 16, 16, 8, 72, 1, 0, 34, 1, ""),                # ragged Cin, N
    (3, 9, 7, 72, 200, 1, 0, 28, 1, "corr rowbias gate silu"),   # ragged Cin, N, M
    (4, 16, 16, 1280, 1280, 1, 0, 30, 4, ""),
    (4, 32, 32, 320, 320, 1, 0, 63, 1, ""),             # a tile the lean kernel does not take (falls back)
]


@pytest.mark.parametrize("case", MATRIX, ids=lambda c: f"t{c[7]}-{c[1]}x{c[2]}x{c[3]}-n{c[4]}-s{c[5]}u{c[6]}k{c[8]}-{c[9].replace(' ', '+')}")
def test_lean_matrix_bit_identical(case, cuda):
    from diffusion_pruning_amd import ops
    B, H, W, cin, n, stride, ups, tile, split, extras = case
    cin2 = 2 * cin if "x2" in extras else 0
    pw = _pw(cuda, cin, n, cin2)
    x = _act(cuda, B, H, W, cin)
    Ho = ((H << (1 if ups else 0)) + 2 - 3) // stride + 1
    Wo = ((W << (1 if ups else 0)) + 2 - 3) // stride + 1
    kw = {}
    g = torch.Generator().manual_seed(7)
    if cin2:
        kw["x2"] = _act(cuda, B, Ho, Wo, cin2, seed=3)
    if "rowbias" in extras:
        kw["rowbias"] = (torch.randn(B, n, generator=g) * 0.2).to(cuda)
    if "gate" in extras:
        kw["colgate"], kw["gate_group"] = (torch.rand(B, n // 8, generator=g)).to(cuda), 8
    if "silu" in extras:
        kw["act"] = ops.ACT_SILU
    if "corr" in extras:
        kw["corr"] = (torch.randn(B, 9, n, generator=g) * 0.1).to(cuda)
    if "residual" in extras:
        kw["residual"] = _act(cuda, B, Ho, Wo, n, seed=4)
    if "depth" in extras:
        kw["depth"], kw["depth_in"] = torch.rand(B, generator=g).to(cuda), _act(cuda, B, Ho, Wo, n, seed=5)
    ys = {}
    old = ops.EPILOGUE
    try:
        for side, epi in (("lean", 0), ("general", 2)):
            ops.EPILOGUE = epi
            ys[side] = ops.conv_gemm(x, pw, stride=stride, pad=1, ups=ups, tile=tile, split_k=split, prefetch=False, **kw)
            torch.cuda.synchronize()
    finally:
        ops.EPILOGUE = old
    a, b = ys["lean"], ys["general"]
    assert torch.isfinite(b.float()).all()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), int((a != b).sum())


def test_lean_repeat_under_concurrent_load(headline_log, cuda):
    """The three most frequent headline 3x3 launches, 20 times each while a second stream keeps the GPU busy: bit-equal."""
    from diffusion_pruning_amd import _lib
    lib = _lib.load()
    _, log = headline_log
    count = {}
    for r in log:
        if "fn" in r or r["params"].KH != 3:
            continue
        p = r["params"]
        key = (p.B * p.Hout * p.Wout, p.N, p.Cin, p.stride, p.ups, p.Cin2, p.tile, p.split_k)
        count.setdefault(key, [0, p])[0] += 1
    top = sorted(count.values(), key=lambda v: -v[0])[:3]
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device=cuda, dtype=torch.bfloat16)
    for _, p in top:
        ref = _run_both(lib, p, cuda, "repeat")["lean"][0]
        with torch.cuda.stream(side):
            for _ in range(8):
                a = (a @ a).clamp_(-1, 1)
        for i in range(20):
            y = _run_both(lib, p, cuda, "repeat")["lean"][0]
            assert torch.equal(y.view(torch.int16), ref.view(torch.int16)), i
    torch.cuda.synchronize()


def test_headline_forward_graph_lean_equals_general(tmp_path):
    """The whole headline forward, graph-replayed (bench.py --dump-outputs), in fresh child processes with APTP_CONV_LEAN=0 / 1."""
    outs = {}
    for v in ("0", "1"):
        d = tmp_path / f"lean{v}"
        env = dict(os.environ, APTP_CONV_LEAN=v)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                            "--no-extras", "--no-extra-configs", "--no-vendor-baseline", "--no-cpu-baseline", "--sustain-seconds", "0",
                            "--dump-outputs", str(d)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        files = sorted(os.listdir(d))
        assert files, r.stdout[-2000:]
        outs[v] = {f: open(d / f, "rb").read() for f in files}
    assert outs["0"].keys() == outs["1"].keys()
    for f in outs["0"]:
        assert outs["0"][f] == outs["1"][f], f
