"""VAE decoder throughput on one GPU: the HIP decode (diffusion_pruning_amd.vae) at (latent 32, batch 8) and (latent 64, batch 4),
its algorithmic TFLOP/s (layer table) and share of the bf16 MFMA peak, the wide-head attention's share of decode time, a vendor
baseline (the same decoder as plain torch modules in bf16, channels-last: MIOpen convolutions, hipBLASLt linears,
F.scaled_dot_product_attention), and, at the reference generation point (256 px, batch 8, 25 PNDM steps, CFG, dense SD-2.1
U-Net), the denoise loop against the decode.  Prints ONE JSON line.  usage: python tools/bench_vae.py [--iters 10]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from diffusion_pruning_amd import _lib, ops
from diffusion_pruning_amd.vae import AutoencoderKL, VAEConfig, vae_decoder_macs

PEAK_BF16_TFLOPS = 2500.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-pipeline", action="store_true", help="skip the reference-point U-Net loop")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.load()
    cfg = VAEConfig()
    vae = AutoencoderKL(cfg).init_synthetic(seed=0).to(dev)
    g = torch.Generator().manual_seed(1)
    res = {"metric": "vae_decode", "shapes": {}}
    lat_in = {}
    for lat, B in ((32, 8), (64, 4)):
        z = torch.randn(B, 4, lat, lat, generator=g).to(dev)
        lat_in[(lat, B)] = z
        ms = time_events(lambda: vae.decode(z), a.iters)
        macs, attn_macs = vae_decoder_macs(cfg, lat, lat)
        tf = 2.0 * macs * B / (ms * 1e-3) / 1e12
        # attention's share: the decode's wide-head launches re-timed on their own
        ops.ATTN_WIDE_LAUNCH_LOG = []
        vae.decode(z)
        recs, ops.ATTN_WIDE_LAUNCH_LOG = ops.ATTN_WIDE_LAUNCH_LOG, None
        lib = _lib.load()

        def attn_only():
            for r in recs:
                _lib.check(lib.aptp_attention_wide(ctypes.byref(r["params"]), ops._stream()), "aptp_attention_wide")
        attn_ms = time_events(attn_only, a.iters)
        res["shapes"][f"latent{lat}_b{B}"] = {
            "decode_ms": round(ms, 3), "images_per_s": round(B / (ms * 1e-3), 2),
            "algorithmic_tflop": round(2.0 * macs * B / 1e12, 3), "tflops": round(tf, 1),
            "frac_of_bf16_peak": round(tf / PEAK_BF16_TFLOPS, 4),
            "attention_ms": round(attn_ms, 3), "attention_share": round(attn_ms / ms, 4),
            "attention_tflops": round(2.0 * attn_macs * B / (attn_ms * 1e-3) / 1e12, 1),
        }
    # ---- reference generation point: 25 PNDM steps, CFG, batch 8 at latent 32, dense U-Net -------------------------------
    if not a.no_pipeline:
        from diffusion_pruning_amd.pipeline import PNDMSchedulerLite, PruningDenoiseLoop
        from diffusion_pruning_amd.unet import UNet2DConditionModelGated
        unet = UNet2DConditionModelGated().init_synthetic(seed=0).to(dev)
        loop = PruningDenoiseLoop(unet, scheduler=PNDMSchedulerLite(), vae=vae)
        cond = torch.randn(8, 77, 1024, generator=g).to(dev)
        unc = torch.randn(8, 77, 1024, generator=g).to(dev)
        lat = torch.randn(8, 4, 32, 32, generator=g).to(dev)
        loop(cond, lat, 25, 7.5, negative_prompt_embeds=unc)                     # capture
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = loop(cond, lat, 25, 7.5, negative_prompt_embeds=unc).latents
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        assert torch.isfinite(out).all()
        loop_ms = sorted(ts)[1]
        dec_ms = res["shapes"]["latent32_b8"]["decode_ms"]
        res["reference_point"] = {"unet_loop_ms": round(loop_ms, 2), "unet_calls": loop.scheduler.n_model_calls(),
                                  "decode_ms": dec_ms, "decode_share_of_generation": round(dec_ms / (loop_ms + dec_ms), 4)}
        del unet, loop
        torch.cuda.empty_cache()
    # ---- vendor baseline (after the timed HIP region) --------------------------------------------------------------------
    from tests import vae_oracle as V

    class _VendorSDPA(torch.nn.Module):
        def forward(self, q, k, v):
            return F.scaled_dot_product_attention(q, k, v)
    ref = V.DecoderOracle()
    ref.load_state_dict(vae.state_dict())
    ref.decoder.mid_block.attentions[0].sdpa = _VendorSDPA()
    ref = ref.to(device=dev, dtype=torch.bfloat16, memory_format=torch.channels_last).eval()
    for (lat, B), z in lat_in.items():
        zb = z.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            ms = time_events(lambda: ref(zb), a.iters)
        key = f"latent{lat}_b{B}"
        res["shapes"][key]["vendor_ms"] = round(ms, 3)
        res["shapes"][key]["vendor_images_per_s"] = round(B / (ms * 1e-3), 2)
        res["shapes"][key]["speedup_vs_vendor"] = round(ms / res["shapes"][key]["decode_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
