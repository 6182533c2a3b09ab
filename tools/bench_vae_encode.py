"""VAE encoder throughput on one GPU: the HIP encode (diffusion_pruning_amd.vae, AutoencoderKL(with_encoder=True)) at
(256 px, batch 64) -- the reference's training point -- and (512 px, batch 4): encode images/s, the trainer's
encode_latents, algorithmic TFLOP/s (layer table vae_encoder_macs) and share of the bf16 MFMA peak; an A/B of the two
conv_in forms in the same run (ops.image_in im2col + a 1x1 contraction over 32 channels, against a 3x3 convolution over the
image zero padded to 8 channels), timed alternately; and a vendor baseline (the same encoder as plain torch modules in bf16,
channels-last: MIOpen convolutions, hipBLASLt linears, F.scaled_dot_product_attention) timed after the HIP region.
Prints ONE JSON line.  usage: python tools/bench_vae_encode.py [--iters 10]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from diffusion_pruning_amd import _lib
from diffusion_pruning_amd.vae import AutoencoderKL, VAEConfig, vae_encoder_macs

PEAK_BF16_TFLOPS = 2500.0
SHAPES = ((256, 64), (512, 4))


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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vae_encode: no GPU")
    dev = torch.device("cuda:0")
    _lib.load()
    cfg = VAEConfig()
    vae = AutoencoderKL(cfg, with_encoder=True).init_synthetic(seed=0).to(dev)
    g = torch.Generator().manual_seed(1)
    res = {"metric": "vae_encode", "shapes": {}}
    px_in = {}
    for S, B in SHAPES:
        x = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)
        px_in[(S, B)] = x
        vae.conv_in_im2col = True
        ms = time_events(lambda: vae.encode(x), a.iters)
        gen = torch.Generator().manual_seed(0)
        lat_ms = time_events(lambda: vae.encode_latents(x, generator=gen), a.iters)
        macs, attn_macs = vae_encoder_macs(cfg, S, S)
        tf = 2.0 * macs * B / (ms * 1e-3) / 1e12
        # conv_in A/B: the two forms alternately, same inputs, same run
        ab = {"im2col": [], "plain": []}
        for rep in range(2):
            for form in (("im2col", "plain") if rep == 0 else ("plain", "im2col")):
                vae.conv_in_im2col = form == "im2col"
                ab[form].append(time_events(lambda: vae.encode(x), a.iters))
        vae.conv_in_im2col = False
        plain_mom = vae.encode(x).latent_dist.parameters
        vae.conv_in_im2col = True
        im_mom = vae.encode(x).latent_dist.parameters
        diff = float((plain_mom.double() - im_mom.double()).norm() / im_mom.double().norm())
        res["shapes"][f"{S}px_b{B}"] = {
            "encode_ms": round(ms, 3), "images_per_s": round(B / (ms * 1e-3), 2),
            "encode_latents_ms": round(lat_ms, 3),
            "algorithmic_tflop": round(2.0 * macs * B / 1e12, 3), "tflops": round(tf, 1),
            "frac_of_bf16_peak": round(tf / PEAK_BF16_TFLOPS, 4),
            "attention_gmac_per_image": round(attn_macs / 1e9, 3),
            "conv_in_ab": {"im2col_ms": [round(t, 3) for t in ab["im2col"]], "plain_ms": [round(t, 3) for t in ab["plain"]],
                           "plain_over_im2col": round(min(ab["plain"]) / min(ab["im2col"]), 4),
                           "moments_rel_l2_between_forms": diff},
        }
    # ---- vendor baseline (after the timed HIP region) --------------------------------------------------------------------
    from tests import vae_encoder_oracle as E

    class _VendorSDPA(torch.nn.Module):
        def forward(self, q, k, v):
            return F.scaled_dot_product_attention(q, k, v)
    ref = E.EncoderOracle()
    ref.load_state_dict({k: v for k, v in vae.state_dict().items() if k.startswith(("encoder.", "quant_conv."))})
    ref.encoder.mid_block.attentions[0].sdpa = _VendorSDPA()
    ref = ref.to(device=dev, dtype=torch.bfloat16, memory_format=torch.channels_last).eval()
    for (S, B), x in px_in.items():
        xb = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            ms = time_events(lambda: ref(xb), a.iters)
        key = f"{S}px_b{B}"
        res["shapes"][key]["vendor_ms"] = round(ms, 3)
        res["shapes"][key]["vendor_images_per_s"] = round(B / (ms * 1e-3), 2)
        res["shapes"][key]["speedup_vs_vendor"] = round(ms / res["shapes"][key]["encode_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
