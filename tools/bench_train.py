"""BASELINE configs[2]: APTP pruning train step (teacher fwd + student fwd/bwd + router) at SD-2.1 size on one MI355X,
synthetic CC3M-shape batch.  Prints one JSON line (secondary metric; bench.py stays on the headline inference config)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusion_pruning_amd.hypernet import HyperStructure  # noqa: E402
from diffusion_pruning_amd.quantizer import StructureVectorQuantizer  # noqa: E402
from diffusion_pruning_amd.train_step import GraphedPrunerStep, PrunerStep, synthetic_batch  # noqa: E402
from diffusion_pruning_amd.unet import UNet2DConditionModelGated  # noqa: E402


def _ab(args, unet, hn, qz, batch, specs, res, out_name):
    """two captured steps, each with its own copy of the router under a RouterAdamW with the router captured, in ONE process and in
    alternating rounds (the clocks of two processes differ by more than these steps do).  specs: (name, constructor keywords, the
    batch it runs) per side; res: the head of the JSON line, which is also written to profiles/<out_name>"""
    import copy
    from diffusion_pruning_amd import graph_utils
    from diffusion_pruning_amd.router_optim import RouterAdamW
    graph_utils.KEEP_GRAPHS = True
    sides = {}
    for name, kw, b in specs:
        h, q = copy.deepcopy(hn), copy.deepcopy(qz)
        step = GraphedPrunerStep(unet, h, q, **kw)
        step.count_macs(args.latent)                          # (the shared U-Net's MAC constants: the same values for every side)
        opt = RouterAdamW([{"params": [p for p in h.parameters() if p.requires_grad], "lr": 2e-4, "weight_decay": 0.0},
                           {"params": [p for p in q.parameters() if p.requires_grad], "lr": 2e-4, "weight_decay": 0.0}])
        step.capture(batch, optimizer=opt)
        sides[name] = dict(step=step, opt=opt, batch=b, ms=[])
    rounds = 4
    for r in range(rounds + 1):                               # round 0 warms both up
        for name, sd in sides.items():
            for _ in range(args.warmup if r == 0 else 0):
                sd["step"].train_step(sd["opt"], sd["batch"])
            sd["step"].finish()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out = sd["step"].train_step(sd["opt"], sd["batch"])
            sd["step"].finish()
            torch.cuda.synchronize()
            if r:
                sd["ms"].append((time.perf_counter() - t0) / args.steps * 1e3)
            sd["loss"] = float(out["loss"])
    res = dict(res, steps_per_round=args.steps, rounds=rounds)
    for name, sd in sides.items():
        best = min(sd["ms"])
        res[name] = {"steps_per_s": round(1e3 / best, 3), "ms_per_step_best": round(best, 3), "ms_per_step_rounds": [round(m, 3) for m in sd["ms"]],
                     "graph_nodes": sd["step"].graph_nodes(), "loss": sd["loss"], "applied_steps": sd["opt"].applied_steps(),
                     "skipped_steps": sd["opt"].skipped_steps()}
    line = json.dumps(res)
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, out_name), "w") as f:
        f.write(line + "\n")
    print(line)


def _short_batch(args, batch):
    n_valid = args.batch - 1 if args.valid is None else args.valid
    assert 1 <= n_valid <= args.batch, "--valid: 1..batch"
    return n_valid, {k: v[:n_valid] for k, v in batch.items()}


def short_batches_ab(args, dev, unet, hn, qz):
    """--short-batches: the default captured step against GraphedPrunerStep(short_batches=True).  The switched step runs
    `--valid` samples of the batch (default: all but one)."""
    batch = synthetic_batch(args.batch, args.latent, dev)
    n_valid, short = _short_batch(args, batch)
    _ab(args, unet, hn, qz, batch, (("default", {}, batch), ("short_batches", {"short_batches": True}, short)),
        {"metric": "pruning-train-steps/s, default captured step vs short_batches=True (same process, alternating rounds)",
         "batch": args.batch, "latent": args.latent, "valid": n_valid}, "bench_train_short_batches.json")


def router_noise_ab(args, dev, unet, hn, qz):
    """--router-seed S: the captured step with its Gumbel noise from the host generator (the default) against
    GraphedPrunerStep(router_seed=S), whose router draws it on the device from the batch's seeds.  With
    --short-batches both sides run `--valid` samples through short_batches=True.  The seeds are device memory, as a loader
    that builds its batches on the device (train_step.batch_from_images(seeds=)) hands them over."""
    batch = synthetic_batch(args.batch, args.latent, dev)
    kw, n_valid, run = {}, args.batch, batch
    if args.short_batches:
        kw = {"short_batches": True}
        n_valid, run = _short_batch(args, batch)
    seeded = dict(run, seeds=torch.arange(1000, 1000 + n_valid, dtype=torch.int64, device=dev), draw=3)
    _ab(args, unet, hn, qz, batch, (("default", kw, run), ("seeded", dict(kw, router_seed=args.router_seed), seeded)),
        {"metric": "pruning-train-steps/s, host-generator router noise vs router_seed (same process, alternating rounds)",
         "batch": args.batch, "latent": args.latent, "valid": n_valid, "short_batches": bool(args.short_batches),
         "router_seed": args.router_seed}, "bench_train_router_noise.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--eager", action="store_true", help="no HIP graphs (the host-bound reference point)")
    ap.add_argument("--router-optimizer", choices=("torch", "hip"), default="torch",
                    help="torch: torch.optim.AdamW, router eager between the U-Net graphs; hip: router_optim.RouterAdamW, the router "
                         "captured for both phases with its schedule in device memory (DESIGN 6p)")
    ap.add_argument("--lr-warmup", type=int, default=0, help="hip: constant_with_warmup over this many applied steps")
    ap.add_argument("--pretrain-steps", type=int, default=0, help="hip: the first P steps run the hyper-net pre-training phase")
    ap.add_argument("--max-grad-norm", type=float, default=None,
                    help="hip: clip the global gradient norm of the router at this value on the device (RouterAdamW(max_grad_norm=))")
    ap.add_argument("--lr-scheduler", default=None,
                    help="hip: the curve of both groups' rates over the applied steps (RouterAdamW(lr_schedule=), DESIGN 6y), with "
                         "--lr-warmup as its warm-up: constant, constant_with_warmup, linear, cosine, cosine_with_restarts, polynomial")
    ap.add_argument("--max-train-steps", type=int, default=None, help="with --lr-scheduler: num_training_steps, in optimizer steps")
    ap.add_argument("--short-batches", action="store_true",
                    help="A/B of the default captured step and GraphedPrunerStep(short_batches=True) in one process; writes "
                         "profiles/bench_train_short_batches.json")
    ap.add_argument("--valid", type=int, default=None, help="with --short-batches: samples per step of the switched side (default batch - 1)")
    ap.add_argument("--router-seed", type=int, default=None,
                    help="with --router-optimizer hip: A/B of the default captured step and GraphedPrunerStep(router_seed=S) in one "
                         "process (with --short-batches: both under short_batches=True); writes profiles/bench_train_router_noise.json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    unet = UNet2DConditionModelGated().init_synthetic(seed=0).to(dev)
    unet.freeze()
    st = unet.get_structure()
    torch.manual_seed(0)
    hn = HyperStructure(structure=st, input_dim=768, wn_flag=False, linear_bias=True).to(dev)
    qz = StructureVectorQuantizer(n_e=8, structure=st, temperature=0.4, base=3,
                                  depth_order=[-1, -2, 0, 1, -3, -4, 2, 3, -5, -6, 4, 5, -7, 6],
                                  resource_aware_normalization=False, optimal_transport=True).to(dev)
    hn.train(); qz.train()
    if args.router_seed is not None:
        if args.router_optimizer != "hip" or args.eager:
            ap.error("--router-seed compares two captured routers: it needs --router-optimizer hip and no --eager")
        return router_noise_ab(args, dev, unet, hn, qz)
    if args.short_batches:
        return short_batches_ab(args, dev, unet, hn, qz)
    step = (PrunerStep if args.eager else GraphedPrunerStep)(unet, hn, qz)
    step.count_macs(args.latent)
    hip = args.router_optimizer == "hip"
    if not hip and (args.lr_warmup or args.pretrain_steps or args.max_grad_norm is not None or args.lr_scheduler is not None):
        ap.error("--lr-warmup, --pretrain-steps, --max-grad-norm and --lr-scheduler need --router-optimizer hip")
    batch = synthetic_batch(args.batch, args.latent, dev)
    done = 0
    if hip:
        from diffusion_pruning_amd import graph_utils
        from diffusion_pruning_amd.router_optim import RouterAdamW
        sched = None
        if args.lr_scheduler is not None:
            from diffusion_pruning_amd.packed_train import LrSchedule
            sched = LrSchedule(args.lr_scheduler, warmup_steps=args.lr_warmup, training_steps=args.max_train_steps)
        graph_utils.KEEP_GRAPHS = True                      # (graph_nodes() below)
        opt = RouterAdamW([{"params": [p for p in hn.parameters() if p.requires_grad], "lr": 2e-4, "weight_decay": 0.0},
                           {"params": [p for p in qz.parameters() if p.requires_grad], "lr": 2e-4, "weight_decay": 0.0}],
                          warmup_steps=0 if sched is not None else args.lr_warmup, max_grad_norm=args.max_grad_norm, lr_schedule=sched)
        if not args.eager:
            step.capture(batch, optimizer=opt, pretrain=args.pretrain_steps > 0)
            if args.pretrain_steps > 0:
                step.capture_router(batch, pretrain=False)

        def one():
            nonlocal done
            o = step.train_step(opt, batch, pretrain=done < args.pretrain_steps)
            done += 1
            return o
    else:
        opt = torch.optim.AdamW(step.trainable_parameters(), lr=2e-4)
        if not args.eager:
            step.capture(batch)

        def one():
            return step.train_step(opt, batch)
    for _ in range(args.warmup):
        out = one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = one()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    extra = {}
    if hip:
        if not args.eager:
            step.finish()
            extra["graph_nodes"] = step.graph_nodes()
        extra.update(router_optimizer="hip", applied_steps=opt.applied_steps(), skipped_steps=opt.skipped_steps(), last_lr=opt.last_lr())
        if args.lr_scheduler is not None:
            extra.update(lr_scheduler=args.lr_scheduler, max_train_steps=args.max_train_steps)
        if args.max_grad_norm is not None:
            extra.update(max_grad_norm=args.max_grad_norm, grad_norm_last=opt.last_grad_norm(), clipped_steps=opt.clipped_steps())
    print(json.dumps({"metric": "pruning-train-steps/s (SD-2.1, 64x64 latents, teacher fwd + student fwd/bwd + router)",
                      "value": round(1.0 / dt, 3), "unit": "steps/s", "ms_per_step": round(dt * 1e3, 2),
                      "batch": args.batch, "loss": float(out["loss"].detach()),
                      "resource_ratio": float(out["resource_ratio"]),
                      "max_mem_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), "mode": "eager (no HIP graph)" if args.eager else ("U-Net passes and router replayed from HIP graphs" if hip else "U-Net passes replayed from HIP graphs, router eager"), **extra}))


if __name__ == "__main__":
    main()
