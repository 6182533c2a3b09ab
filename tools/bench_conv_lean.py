"""Lean 3x3 kernel (csrc/conv_lean.hip) against the general implicit-GEMM kernel on every distinct 3x3 launch of the headline
forward (bs=4, fixed 50 % mask, SD-2.1 size, recorded through ops.LAUNCH_LOG), launch by launch from replayed HIP graphs, on the
table's tile and split (AptpConvGemmParams.epilogue = 2 keeps a launch on the general kernel; the split-K reduce launch, when
there is one, is part of both timings).
Usage: python3 tools/bench_conv_lean.py [out.txt]"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusion_pruning_amd import _lib, ops  # noqa: E402
from diffusion_pruning_amd.unet import UNet2DConditionModelGated  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

dev = torch.device("cuda:0")
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def emit(s):
    print(s, flush=True)
    if out:
        out.write(s + "\n")


def timed(fn, reps=20):
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    fn()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            for _ in range(reps):
                fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(5):
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / reps)
    return best


lib = _lib.load()
model = UNet2DConditionModelGated().init_synthetic(seed=0).to(dev)
model.set_structure({k: [v.to(dev) for v in vs] for k, vs in O.fixed_half_mask(O.SD21).items()})
sample, t, ehs = O.synthetic_inputs(O.SD21, 4, 64, seed=5)
with torch.no_grad():
    model(sample.to(dev), t.to(dev), ehs.to(dev))
    ops.LAUNCH_LOG = []
    model(sample.to(dev), t.to(dev), ehs.to(dev))
    torch.cuda.synchronize()
    log, ops.LAUNCH_LOG = ops.LAUNCH_LOG, None

shapes = {}
for r in log:
    if "fn" in r or r["params"].KH != 3:
        continue
    p = r["params"]
    key = (p.B * p.Hout * p.Wout, p.N, p.Cin, p.stride, p.ups, p.Cin2, p.tile, p.split_k, bool(p.tile_counters), bool(p.gn_gamma))
    shapes.setdefault(key, [0, p])[0] += 1

tot_old = tot_new = 0.0
for key, (cnt, p) in sorted(shapes.items(), key=lambda kv: -kv[1][0]):
    def run(epi):
        q = type(p).from_buffer_copy(p)
        q.epilogue = epi

        def fn():
            _lib.check(lib.aptp_conv_gemm(ctypes.byref(q), torch.cuda.current_stream().cuda_stream), "bench_conv_lean")
        return fn
    t_old, t_new = timed(run(2)), timed(run(0))
    M, N, C, s, u, c2, tile, sk, ik, gn = key
    form = "in-kernel" if ik else ("gn-reduce" if gn else "reduce") if sk > 1 else "-"
    emit(f"M{M:6d} N{N:5d} Cin{C:5d} s{s} u{u} x2 {c2:4d} tile {tile:2d} split {sk} {form:9s} x{cnt:2d}: general {t_old:7.2f} us | "
         f"lean {t_new:7.2f} us ({t_old / t_new:4.2f}x)")
    tot_old += cnt * t_old
    tot_new += cnt * t_new
emit(f"sum over the step's 3x3 launches: general {tot_old:.0f} us, lean {tot_new:.0f} us ({tot_old / tot_new:4.3f}x)")
