"""CLIP image encoder and CMMD throughput on one GPU: the HIP ViT-L/14-336 encode (diffusion_pruning_amd.image_encoder,
init_synthetic weights, bf16) at B in {1, 8, 32} replayed from a HIP graph -- ms per encode, images/s, algorithmic TFLOP/s
(image_encoder_flops) and share of the bf16 MFMA peak --; the image front end (ops.image_patches) for 512 x 512 -> 336 x 336 at
B = 32; and aptp_mmd_rbf at n = m in {2048, 8192, 30000}, D = 768, next to a torch evaluation of the same formula on the same GPU
where its three kernel matrices fit in memory (the reference's distance.py, fp32).
Prints ONE JSON line.  usage: python tools/bench_image_encoder.py [--iters 10]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from diffusion_pruning_amd import _lib, ops
from diffusion_pruning_amd import image_encoder as V

PEAK_BF16_TFLOPS = 2500.0
BATCHES = (1, 8, 32)
MMD_SIZES = (2048, 8192, 30000)
TORCH_MMD_MAX_N = 8192          # three fp32 n x n matrices and their temporaries: 30000 would need > 20 GiB


def time_events(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def torch_mmd(x, y, sigma=10.0, scale=1000.0):
    """the reference's formula with torch on the device (fp32): the three kernel matrices are materialised"""
    gamma = 1.0 / (2.0 * sigma ** 2)
    xs, ys = torch.diag(x @ x.t()), torch.diag(y @ y.t())
    k_xx = torch.exp(-gamma * (-2 * (x @ x.t()) + xs[:, None] + xs[None, :])).mean()
    k_xy = torch.exp(-gamma * (-2 * (x @ y.t()) + xs[:, None] + ys[None, :])).mean()
    k_yy = torch.exp(-gamma * (-2 * (y @ y.t()) + ys[:, None] + ys[None, :])).mean()
    return scale * (k_xx + k_yy - 2 * k_xy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_encoder: no GPU")
    dev = torch.device("cuda:0")
    _lib.load()
    cfg = V.CLIPVisionConfig()
    m = V.CLIPVisionModelWithProjection(cfg).init_synthetic(seed=0).to(dev)
    gen = torch.Generator().manual_seed(1)
    res = {"metric": "clip_image_encode", "model": "CLIP ViT-L/14-336 vision tower (24 layers, 1024 wide, 16 heads, 577 tokens), bf16",
           "gemm_shapes_tuned": False, "layernorm_form": "stand-alone (folded form not measured)", "encode": {}, "mmd_rbf": {}}
    with torch.no_grad():
        for B in BATCHES:
            px = torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=gen).to(dev)
            g = capture(lambda: m(px))
            ms = time_events(g.replay, a.iters)
            flop = V.image_encoder_flops(cfg) * B
            tf = flop / (ms * 1e-3) / 1e12
            res["encode"][f"B{B}"] = {"graph_ms": round(ms, 4), "images_per_s": round(B / (ms * 1e-3), 1), "algorithmic_tflop": round(flop / 1e12, 4),
                                      "tflops": round(tf, 1), "frac_of_bf16_peak": round(tf / PEAK_BF16_TFLOPS, 4)}
            del g
        img = torch.rand(32, 512, 512, 3, generator=gen).to(dev)
        ms = time_events(lambda: ops.image_patches(img, cfg.image_size, cfg.patch_size), a.iters)
        res["front_end_512_to_336_B32"] = {"ms": round(ms, 4), "images_per_s": round(32 / (ms * 1e-3), 1)}
        del img
        for n in MMD_SIZES:
            x = F.normalize(torch.randn(n, 768, generator=gen) + 1.0).to(dev)
            y = F.normalize(torch.randn(n, 768, generator=gen) + 1.05).to(dev)
            it = max(2, a.iters // (1 if n <= 8192 else 5))
            ms = time_events(lambda: ops.mmd_rbf(x, y), it, warmup=1)
            r = {"ms": round(ms, 3), "value": float(ops.mmd_rbf(x, y)), "fp32_tflops": round(3 * 2.0 * n * n * 768 / (ms * 1e-3) / 1e12, 1)}
            if n <= TORCH_MMD_MAX_N:
                tms = time_events(lambda: torch_mmd(x, y), it, warmup=1)
                r.update({"torch_ms": round(tms, 3), "torch_value": float(torch_mmd(x, y)), "torch_over_hip": round(tms / ms, 3)})
            else:
                r["torch_ms"] = None
            res["mmd_rbf"][f"n{n}"] = r
            del x, y
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
