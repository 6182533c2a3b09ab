"""The training step's input path on one GPU: a ragged batch of 64 decoded uint8 images, sizes drawn from a fixed list of CC3M-like
shapes, through the dataloader's transform at R = 256 (data.TrainTransform: two launches, ops.train_images) and then through
vae.encode_latents -- so the transform's time stands next to the time of the encoder that consumes its output.  Reported: the
transform with the images already on the device and with the images in host memory (one host-to-device copy of the packed
batch inside the timed call), encode_latents on the result, and, where PIL imports, the wall time a single-thread PIL + numpy
loop takes for the same batch and the same draws on this host (Image.resize BILINEAR, crop, flip, / 255, Normalize).  Device
times are medians of HIP-event timings after warm-up.  Prints ONE JSON line; --out also writes it to a file.
--seeds adds the seeded path to the same line: the same batch through batch_from_uint8 with a generator and with
seeds=, and the noise stage on its own -- everything after the encoder: the posterior eps, the noise, the timesteps, add_noise
and the target, about a dozen torch launches from a generator against ONE ops.train_noise launch from seeds.  The variants run
interleaved, round by round, in this one process; reported are the median and the minimum of the rounds.
usage: python tools/bench_train_input.py [--iters 20] [--seeds] [--out profiles/train_input_bench.json]"""
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


def time_interleaved(variants, rounds, warmup=3):
    """{name: fn} -> {name: (median ms, min ms)}: one HIP-event timing of every variant per round, round after round"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in ts.items()}


def seeded_figures(res, vae, on_dev, px, dev, iters):
    """the generator path and the seeded path side by side: the noise stage alone, then the whole batch_from_uint8"""
    from diffusion_pruning_amd.train_step import NoiseSchedule, batch_from_uint8, noisy_latents_and_target
    from diffusion_pruning_amd.vae import randn_tensor
    sch = NoiseSchedule()
    seeds = list(range(1000, 1000 + BATCH))
    seeds_dev = torch.tensor(seeds, dtype=torch.int64, device=dev)
    mom = vae.encode(px).latent_dist.parameters
    lat = vae.encode_latents(px)
    tab = sch.sqrt_table(dev)
    scale = vae.config.scaling_factor
    shape = tuple(lat.shape)

    def from_generator(g):
        def fn():
            randn_tensor(shape, generator=g, device=dev, dtype=torch.float32)                 # the posterior's eps
            noise = randn_tensor(shape, generator=g, device=dev, dtype=torch.float32)
            t = torch.randint(0, 1000, (BATCH,), generator=g, device=g.device if g is not None else dev).to(dev)
            return noisy_latents_and_target(lat, noise, t, sch.alphas_cumprod)
        return fn

    step = [0]

    def seeded(sd):
        def fn():
            step[0] += 1
            return ops.train_noise(mom, sqrt_table=tab, seeds=sd, draw=step[0], scale=scale)
        return fn

    stage = time_interleaved({"generator_device": from_generator(None), "generator_cpu": from_generator(torch.Generator().manual_seed(2)),
                              "seeded_host_seeds": seeded(seeds), "seeded_device_seeds": seeded(seeds_dev)}, iters)
    for k, (med, lo) in stage.items():
        res[f"noise_stage_ms_{k}"] = round(med, 4)
        res[f"noise_stage_min_ms_{k}"] = round(lo, 4)
    res["noise_stage_generator_device_over_seeded"] = round(stage["generator_device"][0] / stage["seeded_device_seeds"][0], 2)
    ehs = torch.zeros(BATCH, 77, 8, device=dev)
    mp = torch.zeros(BATCH, 768, device=dev)
    kw = dict(resolution=R, encoder_hidden_states=ehs, mpnet_embeddings=mp, schedule=sch)
    gt = torch.Generator().manual_seed(3)
    whole = time_interleaved({"generator": lambda: batch_from_uint8(vae, on_dev, transform_generator=gt, **kw),
                              "seeded": lambda: batch_from_uint8(vae, on_dev, seeds=seeds, draw=step[0], **kw)},
                             max(3, iters // 4), warmup=2)
    for k, (med, lo) in whole.items():
        res[f"batch_from_uint8_ms_{k}"] = round(med, 3)
        res[f"batch_from_uint8_min_ms_{k}"] = round(lo, 3)


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
    ap.add_argument("--seeds", action="store_true", help="add the seeded path and the noise stage, beside the generator path")
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
    if a.seeds:
        seeded_figures(res, vae, on_dev, px, dev, a.iters)
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
