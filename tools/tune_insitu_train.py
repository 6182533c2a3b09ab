"""In-situ autotune of the conv_gemm table entries the TRAINING steps use (the companion of tools/tune_insitu.py, whose objective
is the inference forward).  Objective = wall time of the captured graphs of one step, replayed the way the step replays them:

  --step train      GraphedPrunerStep at SD-2.1 size, bs=4: teacher graph on the side stream next to the student's forward graph,
                    then the loss + backward graph (router, host RNG and the chain rule into the hyper-net are not GEMM work)
  --step finetune   GraphedFineTunerStep.train_step (teacher + student forward/backward graphs, batched weight gradients, folds,
                    AdamW) of benchmark expert --expert

A table entry is baked into a graph when it is captured, so every candidate costs one capture (~3 s).  Greedy over the shapes by
share of the step's GEMM time; candidates as in tune_insitu.py (what the table uses for the class + the incumbent's neighbours);
a candidate must beat the incumbent by --margin twice.  Entries of shapes the inference forward also uses are left alone (they
were tuned on that objective).  Writes gpurun_out/tuning_gfx950.json (merged) and gpurun_out/tune_insitu_<step>.txt.

Usage: python tools/tune_insitu_train.py --step train|finetune [--expert 3] [--top 20] [--replays 12] [--budget-s 900]"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import expert_mask  # noqa: E402
from diffusion_pruning_amd import ops  # noqa: E402

dev = torch.device("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["train", "finetune"], default="train")
    ap.add_argument("--expert", type=int, default=3)
    ap.add_argument("--top", type=int, default=20)
    ap.add_argument("--skip", type=int, default=0, help="shapes (in order of share) already visited by an earlier pass")
    ap.add_argument("--replays", type=int, default=12)
    ap.add_argument("--margin", type=float, default=0.003)
    ap.add_argument("--budget-s", type=float, default=900.0)
    ap.add_argument("--apply", action="store_true")
    args = ap.parse_args()
    t_start = time.time()
    lib = ops._lib.load()
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep, GraphedPrunerStep, synthetic_batch
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated, UNet2DConditionModelPruned
    batch = synthetic_batch(4, 64, dev, seed=1234)

    if args.step == "train":
        from diffusion_pruning_amd.hypernet import HyperStructure
        from diffusion_pruning_amd.quantizer import StructureVectorQuantizer
        unet = UNet2DConditionModelGated().init_synthetic(seed=0).to(dev)
        unet.freeze()
        st = unet.get_structure()
        torch.manual_seed(0)
        hn = HyperStructure(structure=st, input_dim=768, wn_flag=False, linear_bias=True).to(dev)
        qz = StructureVectorQuantizer(n_e=8, structure=st, temperature=0.4, base=3, resource_aware_normalization=False,
                                      optimal_transport=True).to(dev)
        hn.train(); qz.train()
        code = (torch.rand(4, qz.vq_embed_dim, generator=torch.Generator().manual_seed(9)) * 0.6 + 0.4).to(dev)

        def build(log):
            step = GraphedPrunerStep(unet, hn, qz)
            step.count_macs(64)
            ops.LAUNCH_LOG = [] if log else None
            try:
                step.capture(batch)
            finally:
                ops.LAUNCH_LOG = None
            step._cap["install_code"](code)
            return step

        def replay(step):
            cap = step._cap
            step._stage_batch_and_launch_teacher(batch["noisy_latents"], batch["timesteps"], batch["encoder_hidden_states"], batch["target"])
            cap["g_student"].replay()
            torch.cuda.current_stream().wait_stream(cap["side"])
            cap["g_student_bwd"].replay()
    else:
        teacher = unet = UNet2DConditionModelGated().init_synthetic(seed=0).to(dev)
        teacher.freeze()

        def build(log):
            student = UNet2DConditionModelPruned().init_synthetic(seed=0).to(dev)
            student.prune(expert_mask(student.get_structure(), args.expert, dev))
            step = GraphedFineTunerStep(student, teacher, lr=1e-5)
            ops.LAUNCH_LOG = [] if log else None
            try:
                step.capture(batch, offload_masters=True)
            finally:
                ops.LAUNCH_LOG = None
            return step

        def replay(step):
            step.train_step(None, batch)

    # the shapes of the headline forward keep their entries (they were tuned on that objective)
    from bench import fixed_half_mask, ones_mask
    st0 = unet.get_structure()
    g0 = torch.Generator().manual_seed(1234)
    smp, ehs0 = torch.randn(4, 4, 64, 64, generator=g0).to(dev), torch.randn(4, 77, 1024, generator=g0).to(dev)
    t0 = torch.full((4,), 500, dtype=torch.int64, device=dev)
    unet.set_structure(fixed_half_mask(st0, dev))
    with torch.no_grad():
        unet(smp, t0, ehs0)
        ops.LAUNCH_LOG = []
        unet(smp, t0, ehs0)
        torch.cuda.synchronize()
    hl_log, ops.LAUNCH_LOG = ops.LAUNCH_LOG, None
    headline_keys = set()
    for rec in hl_log:
        if "fn" not in rec:
            p = rec["params"]
            headline_keys.add(ops.key_of(p))
    unet.set_structure(ones_mask(st0, dev))
    del hl_log

    def measure(step=None):
        own = step is None
        if own:
            step = build(False)
        for _ in range(3):
            replay(step)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.replays):
            replay(step)
        e1.record()
        torch.cuda.synchronize()
        v = args.replays / (e0.elapsed_time(e1) * 1e-3)
        if own:
            del step
        return v

    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    base_step = build(True)
    log = base_step._cap["launch_log"]
    shapes = {}
    for rec in log:
        if "fn" in rec:
            continue
        p = rec["params"]
        key = ops.key_of(p)
        s = shapes.setdefault(key, {"count": 0, "flops": rec["flops"], "params": p})
        s["count"] += 1
    order = sorted(shapes, key=lambda k: -shapes[k]["flops"] * shapes[k]["count"])[args.skip:args.skip + args.top]

    def cls(key):
        M, N, C, T, s_, u, g_, x2 = ops.parse_key(key)
        return (T, s_, u, int(g_), x2 > 0), M, N, T * C + x2

    by_class = {}
    for k, v in ops.TUNING.items():
        if ops.parse_key(k):
            by_class.setdefault(cls(k)[0], set()).add((v["tile"], v["split_k"], v.get("order", 1), int(v.get("in_kernel", 0))))

    from tools.tune_convs import clone_params
    ws = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    counters = ops._tile_counters(dev)

    def runnable(key, cd):
        q = clone_params(shapes[key]["params"])
        q.tile, q.split_k, q.order = cd[0], cd[1], cd[2]
        q.workspace = ws.data_ptr() if cd[1] > 1 else None
        q.tile_counters = counters.data_ptr() if (cd[1] > 1 and (cd[3] or cd[0] >= ops.SK_TILE_FIRST)) else None
        q.prefetch, q.prefetch_bytes = None, 0
        q.y = ws.data_ptr() + (512 << 20)           # (never write through the recorded output pointer: scratch output instead)
        q.rowstat_out = q.colstat_out = q.ustat_out = None
        q.residual = q.depth_in = None
        if cd[1] > 1 and lib.aptp_conv_gemm_workspace_bytes(ctypes.byref(q)) > (512 << 20):
            return False
        if q.B * q.Hout * q.Wout * max(q.ldy, q.N) * 4 > (512 << 20):
            return False
        rc = lib.aptp_conv_gemm(ctypes.byref(q), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc == 0

    # (the baseline comes from a fresh capture like every candidate's: the step captured with the launch log on replays ~7 %
    #  slower, which made the first candidate of the first shape "win" in the first version of this tool)
    base = max(measure(), measure())
    out(f"{args.step}: baseline {base:.3f} steps/s (graph replays), {len(shapes)} distinct shapes, visiting {len(order)}")
    changed = {}
    for key in order:
        if time.time() - t_start > args.budget_s:
            out("time budget reached")
            break
        if key in headline_keys:
            out(f"{key:42s} x{shapes[key]['count']:3d}  a shape of the headline forward: kept")
            continue
        c, M, N, K = cls(key)
        nK = (K + 63) // 64
        cur = ops.tuning_lookup(*ops.parse_key(key))
        if cur is None:
            continue
        inc = (cur["tile"], cur["split_k"], cur.get("order", 1), int(cur.get("in_kernel", 0)))
        cands = set(by_class.get(c, ()))
        for dk in (-2, -1, 1, 2):
            sk = inc[1] + dk
            if 1 <= sk <= max(1, nK // 3):
                cands.add((inc[0], sk, inc[2], 1 if sk > 1 else 0))
        for o in (2, 3):
            cands.add((inc[0], inc[1], o, inc[3]))
        cands.discard(inc)
        cands = [cd for cd in sorted(cands) if not (cd[1] > 1 and nK // cd[1] < 3)][:10]
        best, best_v = inc, base
        saved = ops.TUNING.get(key)
        for cd in cands:
            if time.time() - t_start > args.budget_s:
                break
            if not runnable(key, cd):
                continue
            ops.set_entry(key, {"tile": cd[0], "split_k": cd[1], "order": cd[2], "in_kernel": cd[3]})
            try:
                v = measure()
            except Exception:  # noqa: BLE001    (a tile that cannot run this shape under the step's epilogue)
                torch.cuda.synchronize()
                continue
            if v > best_v * (1 + args.margin):
                v2 = measure()
                if min(v, v2) > best_v * (1 + args.margin):
                    best, best_v = cd, min(v, v2)
        if best != inc:
            changed[key] = {"tile": best[0], "split_k": best[1], "order": best[2], "in_kernel": best[3], "insitu_" + args.step: round(best_v, 3)}
            ops.set_entry(key, changed[key])
            out(f"{key:42s} x{shapes[key]['count']:3d}  {inc} -> {best}   {base:.3f} -> {best_v:.3f} steps/s")
            base = best_v
        else:
            ops.set_entry(key, saved)
            out(f"{key:42s} x{shapes[key]['count']:3d}  keeps {inc}")
    del base_step
    final = max(measure(), measure())
    out(f"final {final:.3f} steps/s with {len(changed)} entries changed")
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    src = os.path.join(ROOT, "diffusion_pruning_amd", "tuning_gfx950.json")
    table = json.load(open(src)) if os.path.exists(src) else {}
    table.update(changed)
    json.dump(table, open(os.path.join(ROOT, "gpurun_out", "tuning_gfx950.json"), "w"), indent=0, sort_keys=True)
    if args.apply:
        json.dump(table, open(src, "w"), indent=0, sort_keys=True)
    with open(os.path.join(ROOT, "gpurun_out", "tune_insitu_%s.txt" % args.step), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
