"""Mixed prompt batches at SD-2.1 size: 8 prompts, CFG on, 25 PNDM steps (26 U-Net calls; --scheduler ddim / dpmpp: DDIM or
DPM-Solver++ (2M), --steps calls), routed to k in {1, 2, 4, 8} distinct
benchmark experts (bench.expert_mask), through
  (a) PruningDenoiseLoop: the per-prompt codes installed as one structure -- dense compute, per-sample gates in the epilogues;
  (b) ExpertDispatchLoop cold: a fresh loop, captures included;
  (c) ExpertDispatchLoop warm: new prompts through the captured steps;
in ms per image, plus the graph-node count and the steady-state ms of one step with the fused step off and on (one expert, the
whole batch).  Prints one JSON line.
usage: python tools/bench_dispatch.py [--scheduler pndm|ddim|dpmpp] [--steps 25] [--prompts 8] [--ks 1,2,4,8]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench
from diffusion_pruning_amd import graph_utils
from diffusion_pruning_amd.hypernet import HyperStructure
from diffusion_pruning_amd.pipeline import (DDIMSchedulerLite, DPMSolverMultistepSchedulerLite, ExpertDispatchLoop, PNDMSchedulerLite,
                                            PruningDenoiseLoop)
from diffusion_pruning_amd.quantizer import StructureVectorQuantizer
from diffusion_pruning_amd.unet import UNet2DConditionModelGated

ap = argparse.ArgumentParser()
ap.add_argument("--scheduler", choices=["pndm", "ddim", "dpmpp"], default="pndm")
ap.add_argument("--steps", type=int, default=25)
ap.add_argument("--prompts", type=int, default=8)
ap.add_argument("--ks", default="1,2,4,8")
ap.add_argument("--guidance", type=float, default=7.5)
a = ap.parse_args()
dev = torch.device("cuda:0")
graph_utils.KEEP_GRAPHS = True                     # so that a captured step can be asked for its node count
model = UNet2DConditionModelGated().init_synthetic(seed=0).to(dev)
st = model.get_structure()


class TableRouter(HyperStructure):
    """the router's input IS the architecture logits: the benchmark chooses each prompt's expert"""

    def forward(self, x):
        return x


def flat(mask):
    return torch.cat([w.reshape(1, -1) for w in mask["width"]] + [d.reshape(1, 1) for d in mask["depth"]], dim=1)


BASE = 3
codes = torch.cat([flat(bench.expert_mask(st, e, dev)) for e in range(8)])            # [8, D], 0.9 / 0
hn = TableRouter(structure=st, input_dim=8, single_arch_param=True).to(dev)
qz = StructureVectorQuantizer(n_e=8, structure=st, temperature=0.4, base=BASE, resource_aware_normalization=False).to(dev)
qz.embedding_gs.data = codes.clone()
logits = 20.0 * (2.0 * (codes >= 0.5).float() - 1.0) - BASE                            # the relaxation saturates to the hard code
g = torch.Generator().manual_seed(3)
Scheduler = {"pndm": PNDMSchedulerLite, "ddim": DDIMSchedulerLite, "dpmpp": DPMSolverMultistepSchedulerLite}[a.scheduler]
n_calls = a.steps + (1 if a.scheduler == "pndm" else 0)


def batch(assign):
    n = len(assign)
    return dict(prompt_embeds=torch.randn(n, 77, 1024, generator=g).to(dev), latents=torch.randn(n, 4, 64, 64, generator=g).to(dev),
                negative_prompt_embeds=torch.randn(n, 77, 1024, generator=g).to(dev), hyper_net_input=logits[assign],
                num_inference_steps=a.steps, guidance_scale=a.guidance)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


res = {"tool": "bench_dispatch", "prompts": a.prompts, "steps": a.steps, "unet_calls": n_calls,
       "scheduler": {"pndm": "PNDM", "ddim": "DDIM", "dpmpp": "DPM-Solver++ (2M)"}[a.scheduler], "cfg": True,
       "guidance_scale": a.guidance, "by_k": {}}
for k in [int(v) for v in a.ks.split(",")]:
    assign = [i % k for i in range(a.prompts)]
    parent = PruningDenoiseLoop(model, hn, qz, scheduler=Scheduler())
    out = parent(**batch(assign))
    assert out.arch_indices.tolist() == assign, (out.arch_indices.tolist(), assign)
    ta = sorted(timed(lambda: parent(**batch(assign)))[0] for _ in range(3))[1]
    model.invalidate_plans()
    loop = ExpertDispatchLoop(model, hn, qz, scheduler=Scheduler())
    tb, out = timed(lambda: loop(**batch(assign)))
    assert out.arch_indices.tolist() == assign and torch.isfinite(out.latents).all()
    warm = [timed(lambda: loop(**batch(assign))) for _ in range(3)]
    assert all(r for _, o in warm for *_, r in o.groups)
    tc = sorted(t for t, _ in warm)[1]
    res["by_k"][str(k)] = {"per_sample_gates_ms_per_image": round(ta / a.prompts, 2), "dispatch_cold_ms_per_image": round(tb / a.prompts, 2),
                           "dispatch_warm_ms_per_image": round(tc / a.prompts, 2), "groups": [(e, len(r), b) for e, r, b, _ in out.groups],
                           "graphs": len(loop._graphs)}
    del parent, loop
# one step, fused off / on: one expert, the whole batch
model.set_structure(bench.expert_mask(st, 2, dev))
step = {}
for fused in (False, True):
    loop = PruningDenoiseLoop(model, scheduler=Scheduler())
    kw = batch([2] * a.prompts)
    kw.pop("hyper_net_input")
    loop(**kw, fused_step=fused)
    t = sorted(timed(lambda: loop(**kw, fused_step=fused))[0] for _ in range(3))[1]
    step["fused" if fused else "torch"] = {"graph_nodes": graph_utils.node_count(loop._graph["graph"]), "ms_per_step": round(t / n_calls, 3)}
res["step"] = step
print(json.dumps(res))
