"""The training step's input path on one GPU: a ragged batch of 64 decoded uint8 images, sizes drawn from a fixed list of CC3M-like
shapes, through the dataloader's transform at R = 256 (data.TrainTransform: two launches, ops.train_images) and then through
vae.encode_latents -- so the transform's time stands next to the time of the encoder that consumes its output.  Reported: the
transform with the images already on the device and with the images in host memory (one host-to-device copy of the packed
batch inside the timed call), encode_latents on the result, and, where PIL imports, the wall time a single-thread PIL + numpy
loop takes for the same batch and the same draws on this host (Image.resize BILINEAR, crop, flip, / 255, Normalize).  Device
times are medians of HIP-event timings after warm-up.  Prints ONE JSON line; --out also writes it to a file.
usage: python tools/bench_train_input.py [--iters 20] [--out profiles/train_input_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from diffusion_pruning_amd import _lib, ops
from diffusion_pruning_amd.data import TrainTransform
from diffusion_pruning_amd.vae import AutoencoderKL, VAEConfig

R, BATCH = 256, 64
# (H, W) of typical CC3M files: 500 px on the longer side in the common aspect ratios, some larger and smaller ones
SHAPES = ((333, 500), (375, 500), (500, 500), (500, 333), (281, 500), (400, 600), (600, 400), (256, 256), (450, 800), (512, 384),
          (768, 1024), (256, 341))


def time_events(fn, iters, warmup=3):
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


def pil_loop(images, tops, lefts, flips):
    from PIL import Image
    out = np.empty((len(images), 3, R, R), np.float32)
    for i, a in enumerate(images):
        h1, w1 = ops.pil_resized_size(a.shape[0], a.shape[1], R)[:2]
        r = np.asarray(Image.fromarray(a).resize((w1, h1), Image.BILINEAR))
        win = r[tops[i]:tops[i] + R, lefts[i]:lefts[i] + R]
        if flips[i]:
            win = win[:, ::-1]
        out[i] = (win.transpose(2, 0, 1).astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_input: no GPU")
    dev = torch.device("cuda:0")
    _lib.load()
    rs = np.random.RandomState(0)
    shapes = [SHAPES[i] for i in rs.randint(0, len(SHAPES), BATCH)]
    images = [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in shapes]
    host = [torch.from_numpy(x) for x in images]
    on_dev = [t.to(dev) for t in host]
    tf = TrainTransform(R)
    tops, lefts, flips = tf.draw(host, torch.Generator().manual_seed(0))
    px = ops.train_images(on_dev, R, tops, lefts, flips)
    res = {"metric": "train_input", "batch": BATCH, "resolution": R, "distinct_shapes": len(set(shapes)),
           "input_megabytes": round(sum(x.size for x in images) / 1e6, 2)}
    res["transform_ms_images_on_device"] = round(time_events(lambda: ops.train_images(on_dev, R, tops, lefts, flips), a.iters), 3)
    res["transform_ms_images_on_host"] = round(time_events(lambda: ops.train_images(host, R, tops, lefts, flips, device=dev), a.iters), 3)
    gen = torch.Generator().manual_seed(1)
    res["transform_with_draws_ms_images_on_device"] = round(time_events(lambda: tf(on_dev, generator=gen), a.iters), 3)
    vae = AutoencoderKL(VAEConfig(), with_encoder=True).init_synthetic(seed=0).to(dev)
    g2 = torch.Generator().manual_seed(0)
    res["encode_latents_ms"] = round(time_events(lambda: vae.encode_latents(px, generator=g2), max(3, a.iters // 2), warmup=2), 3)
    res["transform_share_of_transform_plus_encode"] = round(
        res["transform_ms_images_on_device"] / (res["transform_ms_images_on_device"] + res["encode_latents_ms"]), 4)
    res["images_per_s_transform"] = round(BATCH / (res["transform_ms_images_on_device"] * 1e-3), 1)
    try:
        import PIL
    except ImportError:
        res["pil_single_thread_ms"] = None
    else:
        ref = pil_loop(images, tops, lefts, flips)
        res["equal_to_pil"] = bool(np.array_equal(px.cpu().numpy(), ref))
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            pil_loop(images, tops, lefts, flips)
            ts.append((time.perf_counter() - t0) * 1e3)
        res["pil_single_thread_ms"] = round(sorted(ts)[1], 2)
        res["pil_version"] = PIL.__version__
        res["pil_over_transform"] = round(res["pil_single_thread_ms"] / res["transform_ms_images_on_device"], 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
