"""BASELINE configs[4]: expert fine-tune step (teacher dense fwd + pruned student fwd/bwd incl. weight gradients + AdamW) at
SD-2.1 size, one expert per GPU (rank r fine-tunes expert r: keep ratio 0.4..0.75, 0-4 depth gates off).
Experts never communicate (scripts/aptp/finetune.py:27-28), so N GPUs = N independent processes; this tool runs ONE expert
(--expert k) on cuda:0 and prints one JSON line; under `python -m torch.distributed.run --nproc-per-node 8` every rank takes
expert = RANK on cuda:LOCAL_RANK and prints its own line.

--validate K (graphed mode) runs K validation batches of --val-batch samples through GraphedFineTunerStep.validate after the
timed steps and adds their rate to the line; --validate-baseline times the same batches through torch.no_grad() +
FineTunerStep.step under the attached trainer as well (what validation cost before the graphs existed), alternating the two.

--ema (graphed mode) keeps an EMA of the trained weights (packed_train.PackedEMA) and adds `adamw_ms` / `ema_update_ms` (HIP
events around the two launches, median over the timed steps), `ema_bytes` = 12 x trainable elements and the two rates; with
--validate also `validate_losses_ema`, the means of the averaged weights from the same graphs.

--adam8bit (graphed mode) keeps both AdamW moments as block-wise 8-bit codes (GraphedFineTunerStep(use_8bit_adam=True),
csrc/optim8.hip) and adds `optimizer_state_bytes`, `adamw_ms` (the fp32 launch over the small tensors) and `adamw8_ms` (the 8-bit
launch), HIP events around each, median over the timed steps, with `optimizer_pass_ms` their sum; --optimizer-times adds the same
fields for the fp32 state (no `adamw8_ms`), for the comparison.

--short-batches (graphed mode) runs the step with GraphedFineTunerStep(short_batches=True) -- the fused masked loss stage, batches of
up to --batch samples -- and, in the same process, the default step on a second copy of the expert: `short_batches` in the line holds
both rates (alternating rounds of --steps steps, the faster round of each) and the nodes of both loss-and-backward graphs.
--valid N hands the switched step batches of N samples (default: the full batch).

--lr-scheduler NAME --max-train-steps T [--lr-num-cycles C] [--lr-power P] (graphed mode) runs the step under
GraphedFineTunerStep(lr_scheduler=NAME, max_train_steps=T, ...) with --lr-warmup as its warm-up -- one more small launch per optimizer
step (csrc/lr_schedule.hip) -- and adds `lr_scheduler`, `max_train_steps` and `last_lr`, the rate of the next step."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusion_pruning_amd.train_step import FineTunerStep, synthetic_batch  # noqa: E402
from diffusion_pruning_amd.unet import UNet2DConditionModelGated, UNet2DConditionModelPruned  # noqa: E402


from bench import expert_mask  # noqa: E402,F401  (the eight benchmark experts live with the benchmark)


def time_validation(step, batches, baseline: bool, rounds: int = 2):
    """validate() over `batches`, `rounds` times after one untimed pass (capture + warm-up); with `baseline` every round also runs
    the batches through no_grad + FineTunerStep.step (one host sync at the end of the pass, like validate), right after the
    graphed pass, so both see the same machine state"""
    def graphed():
        return step.validate(batches)

    def eager():
        tot = None
        with torch.no_grad():
            for b in batches:
                out = FineTunerStep.step(step, b["noisy_latents"], b["timesteps"], b["encoder_hidden_states"], b["target"])
                v = torch.stack([out[k].detach() for k in ("loss", "diff_loss", "distillation_loss", "block_loss")])
                tot = v if tot is None else tot + v
        return dict(zip(("loss", "diff_loss", "distillation_loss", "block_loss"), (tot / len(batches)).tolist()))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(batches), res

    graphed()
    if baseline:
        eager()
    tg, te, res, res_e = [], [], None, None
    for _ in range(rounds):
        t, res = timed(graphed)
        tg.append(t)
        if baseline:
            t, res_e = timed(eager)
            te.append(t)
    out = {"validate_batches": len(batches), "validate_batch": int(batches[0]["noisy_latents"].shape[0]),
           "validate_ms_per_batch": round(min(tg) * 1e3, 2), "validate_batches_per_s": round(1.0 / min(tg), 3),
           "validate_ms_per_batch_rounds": [round(t * 1e3, 2) for t in tg], "validate_losses": res,
           "peak_gib_with_validation": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    # launches of one validation batch: the graphs again, captured with their hipGraph_t kept so that the runtime can count nodes
    from diffusion_pruning_amd import graph_utils
    graph_utils.KEEP_GRAPHS = True
    step.capture_validation(batches[0])
    out["validate_graph_nodes"] = step.validation_graph_nodes()[out["validate_batch"]]
    graph_utils.KEEP_GRAPHS = False
    if baseline:
        out.update({"validate_baseline_ms_per_batch": round(min(te) * 1e3, 2),
                    "validate_baseline_ms_per_batch_rounds": [round(t * 1e3, 2) for t in te], "validate_baseline_losses": res_e})
    return out


class LaunchTimer:
    """HIP events around every call of obj._launch while `on` (the one-launch AdamW / EMA passes of the optimizer tail): the
    events go onto the stream the launch goes to, so a pair brackets that kernel alone"""

    def __init__(self, obj, name="_launch"):
        self.pairs, self.on, inner = [], False, getattr(obj, name)

        def timed(*a, **k):
            if not self.on:
                return inner(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = inner(*a, **k)
            e1.record()
            self.pairs.append((e0, e1))
            return r
        setattr(obj, name, timed)

    def ms(self):
        """median over the recorded launches (call after a synchronize)"""
        t = sorted(e0.elapsed_time(e1) for e0, e1 in self.pairs)
        return t[len(t) // 2] if t else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--expert", type=int, default=0)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", choices=("graphed", "packed-eager", "eager"), default="graphed",
                    help="graphed: packed masters + HIP graphs (GraphedFineTunerStep); packed-eager: packed masters, eager; "
                         "eager: diffusers-layout masters, eager (the round-1 path)")
    ap.add_argument("--accum", type=int, default=1,
                    help="gradient accumulation (graphed mode): --batch is the micro-batch, every step a micro-step, and the "
                         "exchange + AdamW run once per window of this many; --steps / --warmup are rounded up to whole windows")
    ap.add_argument("--lr-warmup", type=int, default=0, help="constant_with_warmup over this many optimizer steps (graphed mode)")
    ap.add_argument("--validate", type=int, default=0, help="validation batches to run through the forward-only graphs (graphed mode)")
    ap.add_argument("--val-batch", type=int, default=32, help="validation batch size (validation_batch_size of the fine-tune config)")
    ap.add_argument("--validate-baseline", action="store_true",
                    help="also time the same batches through torch.no_grad() + FineTunerStep.step, alternating with the graphs")
    ap.add_argument("--ema", action="store_true",
                    help="keep an EMA of the trained weights (graphed mode, PackedEMA defaults); adds the EMA and AdamW launch times "
                         "(HIP events over the timed steps) and, with --validate, the validation means of the averaged weights")
    ap.add_argument("--max-grad-norm", type=float, default=None,
                    help="clip the global gradient norm at this value on the device (graphed mode, GraphedFineTunerStep(max_grad_norm=)); "
                         "adds max_grad_norm, grad_norm_last, clipped_steps and the norm pass's time (HIP events) to the JSON line")
    ap.add_argument("--adam8bit", action="store_true",
                    help="block-wise 8-bit AdamW moments (graphed mode, GraphedFineTunerStep(use_8bit_adam=True)); adds "
                         "optimizer_state_bytes and the optimizer launches' times (HIP events) to the JSON line")
    ap.add_argument("--optimizer-times", action="store_true",
                    help="the same fields without the 8-bit state (graphed mode): what --adam8bit is compared with")
    ap.add_argument("--short-batches", action="store_true",
                    help="GraphedFineTunerStep(short_batches=True) (graphed mode), timed against the default step in the same run; adds "
                         "both rates and the node counts of both loss-and-backward graphs to the JSON line")
    ap.add_argument("--valid", type=int, default=None, help="with --short-batches: samples per timed batch, 1..--batch (default: all)")
    ap.add_argument("--lr-scheduler", default=None,
                    help="the curve of the rate over the applied optimizer steps (graphed mode, GraphedFineTunerStep(lr_scheduler=)): "
                         "constant, constant_with_warmup, linear, cosine, cosine_with_restarts, polynomial")
    ap.add_argument("--max-train-steps", type=int, default=None, help="with --lr-scheduler: num_training_steps, in optimizer steps")
    ap.add_argument("--lr-num-cycles", type=float, default=None, help="with --lr-scheduler cosine / cosine_with_restarts")
    ap.add_argument("--lr-power", type=float, default=1.0, help="with --lr-scheduler polynomial")
    args = ap.parse_args()
    assert args.lr_scheduler is None or args.mode == "graphed", "--lr-scheduler belongs to the graphed step"
    assert not args.short_batches or args.mode == "graphed", "--short-batches belongs to the graphed step"
    assert args.valid is None or (args.short_batches and 1 <= args.valid <= args.batch), "--valid N needs --short-batches and 1 <= N <= --batch"
    args.optimizer_times = args.optimizer_times or args.adam8bit
    assert not args.optimizer_times or args.mode == "graphed", "--adam8bit / --optimizer-times belong to the graphed step"
    assert args.validate == 0 or args.mode == "graphed", "--validate belongs to the graphed step"
    assert args.max_grad_norm is None or args.mode == "graphed", "--max-grad-norm belongs to the graphed step"
    assert not args.ema or args.mode == "graphed", "--ema belongs to the graphed step"
    assert args.accum >= 1 and (args.mode == "graphed" or (args.accum == 1 and args.lr_warmup == 0)), \
        "--accum / --lr-warmup belong to the graphed step"
    args.steps = -(-args.steps // args.accum) * args.accum
    args.warmup = -(-args.warmup // args.accum) * args.accum
    # under torchrun: one expert per GPU (rank r -> expert r on cuda:LOCAL_RANK); the processes never communicate
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if "RANK" in os.environ:
        args.expert = int(os.environ["RANK"])
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    teacher = UNet2DConditionModelGated().init_synthetic(seed=0)
    student = UNet2DConditionModelPruned()
    student.load_state_dict(teacher.state_dict())
    teacher.to(dev).freeze()
    st = teacher.get_structure()
    teacher.set_structure({"width": [torch.ones(1, w, device=dev) for sub in st["width"] for w in sub],
                           "depth": [torch.ones(1, device=dev) for sub in st["depth"] for d in sub if d == 1]})
    student.to(dev)
    student.prune(expert_mask(st, args.expert, dev))
    batch = synthetic_batch(args.batch, 64, dev)
    n_train, timers, base = None, {}, None
    timed_batch = batch if args.valid is None else {k: v[:args.valid].clone() for k, v in batch.items()}
    if args.mode == "graphed":
        from diffusion_pruning_amd import graph_utils
        from diffusion_pruning_amd.train_step import GraphedFineTunerStep
        kw = dict(lr=1e-5, accumulation_steps=args.accum, lr_warmup_steps=args.lr_warmup,
                  **({"ema": True} if args.ema else {}), **({"use_8bit_adam": True} if args.adam8bit else {}),
                  **({"max_grad_norm": args.max_grad_norm} if args.max_grad_norm is not None else {}),
                  **({"lr_scheduler": args.lr_scheduler, "max_train_steps": args.max_train_steps, "lr_num_cycles": args.lr_num_cycles,
                      "lr_power": args.lr_power} if args.lr_scheduler is not None else {}))
        if args.short_batches:
            # the default step on a second copy of the same expert, for the comparison; graphs kept so that their nodes can be counted
            graph_utils.KEEP_GRAPHS = True
            student2 = UNet2DConditionModelPruned()
            student2.load_state_dict(teacher.state_dict())
            student2.to(dev)
            student2.prune(expert_mask(st, args.expert, dev))
            base = GraphedFineTunerStep(student2, teacher, **kw)
            base.capture(batch, offload_masters=True)
            kw["short_batches"] = True
        step = GraphedFineTunerStep(student, teacher, **kw)
        step.capture(batch, offload_masters=True)
        graph_utils.KEEP_GRAPHS = False
        opt, n_train = None, step.trainer.n_trainable()
        if args.max_grad_norm is not None:
            timers = {"grad_norm_ms": LaunchTimer(step.optimizer.grad_norm, "run")}
        if args.ema:
            timers.update({"adamw_ms": LaunchTimer(step.optimizer), "ema_update_ms": LaunchTimer(step.ema)})
        if args.optimizer_times:
            if "adamw_ms" not in timers:
                timers["adamw_ms"] = LaunchTimer(step.optimizer)
            if args.adam8bit:
                timers["adamw8_ms"] = LaunchTimer(step.optimizer, "_launch8")
    elif args.mode == "packed-eager":
        from diffusion_pruning_amd.packed_train import PackedTrainer
        step = FineTunerStep(student, teacher)
        pk = PackedTrainer(student).attach().materialize(batch["noisy_latents"], batch["timesteps"], batch["encoder_hidden_states"])
        opt, n_train = torch.optim.AdamW(pk.parameters(), lr=1e-5, fused=True), pk.n_trainable()
    else:
        step = FineTunerStep(student, teacher)
        opt = torch.optim.AdamW([p for p in student.parameters() if p.requires_grad], lr=1e-5, fused=True)
    for _ in range(args.warmup):
        out = step.train_step(opt, timed_batch)
    torch.cuda.synchronize()
    for t in timers.values():
        t.on = True
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step.train_step(opt, timed_batch)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    peak_train, val = torch.cuda.max_memory_allocated(), {}
    if base is not None:
        for t in timers.values():
            t.on = False

        def per_step(s, b):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                s.train_step(None, b)
            torch.cuda.synchronize()
            return (time.perf_counter() - t1) / args.steps
        for _ in range(args.warmup):
            base.train_step(None, batch)
        rounds = [(per_step(base, batch), per_step(step, timed_batch)) for _ in range(2)]
        dt_off, dt_on = min(r[0] for r in rounds), min(r[1] for r in rounds)
        val["short_batches"] = {"valid": args.batch if args.valid is None else args.valid, "steps_per_s": round(1.0 / dt_on, 3),
                                "default_steps_per_s": round(1.0 / dt_off, 3), "ratio_to_default": round(dt_off / dt_on, 4),
                                "loss_bwd_graph_nodes": step.graph_nodes()["student_bwd"],
                                "default_loss_bwd_graph_nodes": base.graph_nodes()["student_bwd"],
                                "n_valid_last": float(out["n_valid"])}
    if args.ema:
        # both passes stream the same tensors in the same geometry: 30 B per element (AdamW: p, g, m, v read; p, m, v and the
        # bf16 operand of a weight written) against 12 B (EMA: p, ema read; ema written)
        for t in timers.values():
            t.on = False
        val = {k: round(t.ms(), 4) for k, t in timers.items()}
        n_el = step.ema.n_elements()
        val.update({"ema_bytes": 12 * n_el, "ema_steps": step.ema.steps(), "ema_cur_decay": step.ema.cur_decay(),
                    "ema_gb_per_s": round(12 * n_el / val["ema_update_ms"] * 1e-6, 1),
                    "adamw_gb_per_s": round(30 * n_el / val["adamw_ms"] * 1e-6, 1)})
    if args.optimizer_times:
        # bytes of the pass by the model of csrc/optim.hip / optim8.hip: 30 B per element with fp32 moments (26 without an
        # operand); 18 B + 16 B per 256 elements with 8-bit ones
        for t in timers.values():
            t.on = False
        o = step.optimizer
        ms = {k: timers[k].ms() for k in ("adamw_ms", "adamw8_ms") if k in timers and timers[k].ms() is not None}
        n8 = sum(p.numel() for p, q in zip(o.params, o.is8) if q)
        val.update({k: round(v, 4) for k, v in ms.items()})
        val.update({"optimizer_state_bytes": o.state_bytes(), "optim_bits": o.optim_bits, "elements_8bit": n8,
                    "elements_fp32": n_train - n8, "optimizer_pass_ms": round(sum(ms.values()), 4)})
        if "adamw8_ms" in ms:
            val["adamw8_gb_per_s"] = round((18 + 16 / 256) * n8 / ms["adamw8_ms"] * 1e-6, 1)
        elif "adamw_ms" in ms:
            val["adamw_gb_per_s"] = round(30 * n_train / ms["adamw_ms"] * 1e-6, 1)
    if args.max_grad_norm is not None:
        # the pass reads every gradient element once: 4 B per trainable element
        for t in timers.values():
            t.on = False
        gn_ms = timers["grad_norm_ms"].ms()
        val.update({"max_grad_norm": args.max_grad_norm, "grad_norm_last": step.optimizer.last_grad_norm(),
                    "clipped_steps": step.optimizer.clipped_steps(), "grad_norm_ms": round(gn_ms, 4),
                    "grad_norm_gb_per_s": round(4 * n_train / gn_ms * 1e-6, 1)})
    if args.lr_scheduler is not None:
        val.update({"lr_scheduler": args.lr_scheduler, "max_train_steps": args.max_train_steps, "last_lr": step.optimizer.last_lr()})
    if args.validate:
        batches = [synthetic_batch(args.val_batch, 64, dev, seed=100 + i) for i in range(args.validate)]
        val.update(time_validation(step, batches, args.validate_baseline))
        if args.ema:
            val["validate_losses_ema"] = step.validate(batches, use_ema=True)
    print(json.dumps({"metric": "expert-finetune-steps/s (SD-2.1 pruned expert, 64x64 latents, teacher fwd + student fwd/bwd/wgrad + AdamW)",
                      "value": round(1.0 / dt, 3), "unit": "steps/s", "ms_per_step": round(dt * 1e3, 1), "expert": args.expert,
                      "batch": args.batch, "loss": float(out["loss"].detach()),
                      "max_mem_GiB": round(peak_train / 2 ** 30, 1), "mode": args.mode,
                      "trainable_parameters": n_train, "accumulation_steps": args.accum, "lr_warmup_steps": args.lr_warmup,
                      "micro_steps_per_s": round(1.0 / dt, 3), "optimizer_steps_per_s": round(1.0 / (dt * args.accum), 3),
                      "peak_gib": round(peak_train / 2 ** 30, 2), **val}))


if __name__ == "__main__":
    main()
