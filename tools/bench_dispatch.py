"""Mixed prompt batches at SD-2.1 size: 8 prompts, CFG on, 25 PNDM steps (26 U-Net calls; --scheduler ddim / dpmpp: DDIM or
DPM-Solver++ (2M), --steps calls), routed to k in {1, 2, 4, 8} distinct
benchmark experts (bench.expert_mask), through
  (a) PruningDenoiseLoop: the per-prompt codes installed as one structure -- dense compute, per-sample gates in the epilogues;
  (b) ExpertDispatchLoop cold: a fresh loop, captures included;
  (c) ExpertDispatchLoop warm: new prompts through the captured steps;
in ms per image, plus the graph-node count and the steady-state ms of one step with the fused step off and on (one expert, the
whole batch).  --seeds: the latents are drawn in the loop from one seed per prompt (ops.randn) instead of handed in.
--eta X (DDIM) / --sde (SDE-DPM-Solver++): the stochastic samplers, seeded; the JSON line then also carries "noise_node": the
fused step of the same scheduler class without and with the noise launch, measured in this same run.
--lanes N (1..4): ExpertDispatchLoop(lanes=N), the expert groups side by side on stream lanes; the JSON line carries "lanes", the
effective number of lanes and what the side-stream probe measured.  Prints one JSON line.
usage: python tools/bench_dispatch.py [--scheduler pndm|ddim|dpmpp] [--steps 25] [--prompts 8] [--ks 1,2,4,8] [--seeds]
       [--eta X | --sde] [--lanes N]"""
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
ap.add_argument("--seeds", action="store_true", help="draw the latents in the loop from one seed per prompt")
ap.add_argument("--eta", type=float, default=0.0, help="stochastic DDIM (implies --scheduler ddim and --seeds)")
ap.add_argument("--sde", action="store_true", help="SDE-DPM-Solver++ (implies --scheduler dpmpp and --seeds)")
ap.add_argument("--lanes", type=int, default=1, help="stream lanes of ExpertDispatchLoop (1 = groups one after another)")
a = ap.parse_args()
if a.eta > 0.0 and a.sde:
    ap.error("--eta and --sde exclude each other")
if a.eta > 0.0:
    a.scheduler = "ddim"
if a.sde:
    a.scheduler = "dpmpp"
stochastic = a.eta > 0.0 or a.sde
a.seeds = a.seeds or stochastic
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


def Scheduler(noise=True):
    """the scheduler of this run; noise=False: the deterministic one of the same class"""
    if a.scheduler == "ddim":
        return DDIMSchedulerLite(eta=a.eta if noise else 0.0)
    if a.scheduler == "dpmpp":
        return DPMSolverMultistepSchedulerLite(algorithm_type="sde-dpmsolver++" if noise and a.sde else "dpmsolver++")
    return PNDMSchedulerLite()


n_calls = a.steps + (1 if a.scheduler == "pndm" else 0)


def batch(assign):
    n = len(assign)
    kw = dict(prompt_embeds=torch.randn(n, 77, 1024, generator=g).to(dev), latents=torch.randn(n, 4, 64, 64, generator=g).to(dev),
              negative_prompt_embeds=torch.randn(n, 77, 1024, generator=g).to(dev), hyper_net_input=logits[assign],
              num_inference_steps=a.steps, guidance_scale=a.guidance)
    if a.seeds:
        kw.update(latents=None, seeds=torch.randint(0, 2 ** 62, (n,), generator=g).tolist(), latent_shape=(4, 64, 64))
    return kw


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


res = {"tool": "bench_dispatch", "prompts": a.prompts, "steps": a.steps, "unet_calls": n_calls,
       "scheduler": {"pndm": "PNDM", "ddim": "DDIM", "dpmpp": "DPM-Solver++ (2M)"}[a.scheduler] + (" SDE" if a.sde else ""), "cfg": True,
       "eta": a.eta, "seeded_latents": a.seeds, "guidance_scale": a.guidance, "lanes": a.lanes, "lanes_effective": 1, "stream_probe": None, "by_k": {}}
for k in [int(v) for v in a.ks.split(",")]:
    assign = [i % k for i in range(a.prompts)]
    parent = PruningDenoiseLoop(model, hn, qz, scheduler=Scheduler())
    out = parent(**batch(assign))
    assert out.arch_indices.tolist() == assign, (out.arch_indices.tolist(), assign)
    ta = sorted(timed(lambda: parent(**batch(assign)))[0] for _ in range(3))[1]
    model.invalidate_plans()
    loop = ExpertDispatchLoop(model, hn, qz, scheduler=Scheduler(), lanes=a.lanes)
    tb, out = timed(lambda: loop(**batch(assign)))
    assert out.arch_indices.tolist() == assign and torch.isfinite(out.latents).all()
    warm = [timed(lambda: loop(**batch(assign))) for _ in range(3)]
    assert all(r for _, o in warm for *_, r in o.groups)
    tc = sorted(t for t, _ in warm)[1]
    res["by_k"][str(k)] = {"per_sample_gates_ms_per_image": round(ta / a.prompts, 2), "dispatch_cold_ms_per_image": round(tb / a.prompts, 2),
                           "dispatch_warm_ms_per_image": round(tc / a.prompts, 2), "groups": [(e, len(r), b) for e, r, b, _ in out.groups],
                           "graphs": len(loop._graphs)}
    if a.lanes > 1:
        res["by_k"][str(k)]["group_lanes"] = out.lanes
        res["lanes_effective"], res["stream_probe"] = len(loop.lane_streams), loop.stream_probe
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
if stochastic:
    # the cost of the noise node: the fused step of the same class without and with it, interleaved in this run
    loops = {nm: PruningDenoiseLoop(model, scheduler=Scheduler(noise=nm == "stochastic")) for nm in ("deterministic", "stochastic")}
    kw = batch([2] * a.prompts)
    kw.pop("hyper_net_input")
    times = {nm: [] for nm in loops}
    for rnd in range(6):
        for nm, loop in loops.items():
            t = timed(lambda: loop(**kw, fused_step=True))[0]
            if rnd:                                     # (round 0 captures)
                times[nm].append(t / n_calls)
    res["noise_node"] = {nm: {"graph_nodes": graph_utils.node_count(loops[nm]._graph["graph"]),
                              "ms_per_step": round(sorted(times[nm])[len(times[nm]) // 2], 4)} for nm in loops}
    res["noise_node"]["delta_us_per_step"] = round(1e3 * (res["noise_node"]["stochastic"]["ms_per_step"]
                                                          - res["noise_node"]["deterministic"]["ms_per_step"]), 1)
print(json.dumps(res))
