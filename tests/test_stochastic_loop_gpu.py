"""Seeded latents and the stochastic samplers (DDIM with eta > 0, SDE-DPM-Solver++) in PruningDenoiseLoop and
ExpertDispatchLoop on the GPU: ``seeds=`` is ``latents=ops.randn(...)``, the captured step with its extra noise node equals the
eager one and replays bit for bit, and each loop matches a host loop made of the oracle U-Net, the fp64 restatement of the step
(the scheduler's fp64 table, which tests/test_stochastic_sched_host.py pins against explicit history lists) and the numpy oracle
of the noise stream.

Budget: ``LOOP_BUDGET`` of tests/test_dispatch_gpu.py, as the deterministic loops are held to (same steps, same guidance)."""
import numpy as np
import pytest
import torch

from oracle import unet_oracle as O
from tests import philox_oracle as PO
from tests.margins import check
from tests.test_dispatch_gpu import LOOP_BUDGET, S, SPLIT, STEPS, inputs, rel_l2, router, tiny  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SHAPE = (4, 16, 16)
N = 4 * 16 * 16
SEEDS = [1234, 7, -3, 2 ** 63 - 1, 0, 99]            # one per prompt of SPLIT


def scheduler(name):
    from diffusion_pruning_amd import pipeline as P
    return {"ddim": lambda: P.DDIMSchedulerLite(), "ddim-eta": lambda: P.DDIMSchedulerLite(eta=0.5),
            "sde": lambda: P.DPMSolverMultistepSchedulerLite(algorithm_type="sde-dpmsolver++")}[name]()


def oracle_z(seeds, draw):
    return torch.from_numpy(PO.normals_rows(seeds, draw, 0, N)).reshape(len(seeds), *SHAPE)


def host_loop(cfg, params, mask, name, seeds, cond, uncond):
    """oracle U-Net (fp32 weights, as every loop test runs it), everything after it in fp64: guidance, the step from the fp64
    table, the oracle's normals; draw 0 is the initial latents, call i adds draw i + 1"""
    sch = scheduler(name)
    ts = sch.set_timesteps(STEPS)
    gates = O.assign_gates(cfg, mask)
    B = len(seeds)
    x, ehs = oracle_z(seeds, 0), torch.cat([uncond, cond])
    prev = torch.zeros_like(x)
    for i in range(STEPS):
        out = O.unet_forward(params, cfg, torch.cat([x, x]).float(), ts[i].expand(2 * B), ehs, gates, "gated").double()
        u, c = out.chunk(2)
        g = u + S * (c - u)
        row, ns = sch.table[i].tolist(), float(sch.noise_table[i])
        x0 = row[0] * x - row[1] * g                                         # v-prediction
        if name == "sde":
            x, prev = (row[2] * x + row[3] * x0) + row[4] * prev, x0
        else:
            x = row[2] * x0 + row[3] * (row[0] * g + row[1] * x)
        x = x + ns * oracle_z(seeds, i + 1)
    return x


@pytest.fixture(scope="module")
def plain(tiny, cuda):
    """two prompts through one batch-shared structure: the inputs of the PruningDenoiseLoop tests"""
    cfg, model, params = tiny
    _, cond, uncond = inputs(cfg, 2, seed=21)
    return {"cond": cond.to(cuda), "uncond": uncond.to(cuda), "seeds": SEEDS[:2], "cond_cpu": cond, "uncond_cpu": uncond}


def install(tiny, cuda):
    cfg, model, _ = tiny
    model.set_structure({k: [v.to(cuda) for v in vs] for k, vs in O.fixed_half_mask(cfg).items()})
    return model


def run(loop, case, **kw):
    return loop(case["cond"], kw.pop("latents", None), STEPS, S, negative_prompt_embeds=case["uncond"], **kw)


def test_seeds_are_latents_from_randn(tiny, plain, cuda):
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd.pipeline import PruningDenoiseLoop
    loop = PruningDenoiseLoop(install(tiny, cuda), scheduler=scheduler("ddim"))
    lat = ops.randn((2,) + SHAPE, plain["seeds"], device=cuda)
    assert float((lat.cpu().double() - oracle_z(plain["seeds"], 0)).abs().max()) <= 4e-6
    a = run(loop, plain, seeds=plain["seeds"], latent_shape=SHAPE).latents
    b = run(loop, plain, latents=lat).latents
    assert a.dtype == torch.float32 and torch.equal(a, b)
    # one int: every prompt the same seed, so with the same prompt the same sample
    same = {"cond": plain["cond"][:1].expand(2, -1, -1).contiguous(), "uncond": plain["uncond"][:1].expand(2, -1, -1).contiguous()}
    c = run(loop, same, seeds=5, latent_shape=SHAPE).latents
    assert torch.equal(c[0], c[1])


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", ["ddim-eta", "sde"])
def test_captured_step_equals_eager_and_replays(tiny, plain, cuda, name, fused):
    from diffusion_pruning_amd.pipeline import PruningDenoiseLoop
    loop = PruningDenoiseLoop(install(tiny, cuda), scheduler=scheduler(name))
    kw = {"seeds": plain["seeds"], "latent_shape": SHAPE, "fused_step": fused}
    first = run(loop, plain, **kw).latents
    graph = loop._graph["graph"]
    assert sorted(loop._graph["state"]) == sorted(["coef", "draw", "noise_scale", "seeds"] + (["prev"] if name == "sde" else []))
    eager = run(loop, plain, use_graph=False, **kw).latents
    assert torch.equal(first, eager)
    # other seeds through the same captured step, then the first ones again: the replay refreshes the seeds
    other = run(loop, plain, **dict(kw, seeds=[5, 6])).latents
    assert loop._graph["graph"] is graph and not torch.equal(other, first)
    assert torch.equal(other, run(loop, plain, use_graph=False, **dict(kw, seeds=[5, 6])).latents)
    again = run(loop, plain, **kw).latents
    assert loop._graph["graph"] is graph and torch.equal(again, first)
    # the deterministic scheduler of the same class is another step: it has one node less
    det = PruningDenoiseLoop(loop.unet, scheduler=scheduler("ddim"))
    det._graph, det._graph_key = loop._graph, loop._graph_key
    run(det, plain, seeds=plain["seeds"], latent_shape=SHAPE, fused_step=fused)
    assert det._graph["graph"] is not graph


@pytest.mark.parametrize("name", ["ddim-eta", "sde"])
def test_loop_matches_the_host_loop(tiny, plain, cuda, name):
    from diffusion_pruning_amd.pipeline import PruningDenoiseLoop
    cfg, model, params = tiny
    loop = PruningDenoiseLoop(install(tiny, cuda), scheduler=scheduler(name))
    got = run(loop, plain, seeds=plain["seeds"], latent_shape=SHAPE, fused_step=True).latents
    ref = host_loop(cfg, params, O.fixed_half_mask(cfg), name, plain["seeds"], plain["cond_cpu"], plain["uncond_cpu"])
    e = check(rel_l2(got.cpu(), ref), LOOP_BUDGET, f"{name} seeded loop vs host fp64 loop")
    # the noise is a real part of the sample: without it the deterministic sampler ends somewhere else
    det = run(PruningDenoiseLoop(model, scheduler=scheduler("ddim")), plain, seeds=plain["seeds"], latent_shape=SHAPE).latents
    print(f"{name}: {e:.3e}; deterministic DDIM from the same latents is {rel_l2(det.cpu(), ref):.3e} away")
    assert rel_l2(det.cpu(), ref) > 4 * LOOP_BUDGET


@pytest.fixture(scope="module")
def mixed(tiny, router):
    cfg, _, _ = tiny
    _, cond, uncond = inputs(cfg, len(SPLIT), seed=31)
    return {"x": router.take(SPLIT), "cond": cond, "uncond": uncond}


def call(loop, case, cuda, rows=None, **kw):
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    return loop(sel(case["cond"]).to(cuda), kw.pop("latents", None), STEPS, S, hyper_net_input=sel(case["x"]).to(cuda),
                negative_prompt_embeds=sel(case["uncond"]).to(cuda), **kw)


@pytest.mark.parametrize("name", ["ddim-eta", "sde"])
def test_mixed_batch_with_a_seed_per_prompt(tiny, router, mixed, cuda, name):
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd.pipeline import ExpertDispatchLoop
    cfg, model, params = tiny
    loop = ExpertDispatchLoop(model, router.hn, router.qz, scheduler=scheduler(name))
    first = call(loop, mixed, cuda, seeds=SEEDS, latent_shape=SHAPE)
    assert first.arch_indices.tolist() == SPLIT
    assert [(e, rows, b, r) for e, rows, b, r in first.groups] == [(0, [0, 2, 5], 4, False), (1, [1, 4], 2, False), (2, [3], 1, False)]
    # the caller's order: every prompt against the host loop of its own seed, prompt and expert
    ref = host_loop(cfg, params, router.mask(SPLIT), name, SEEDS, mixed["cond"], mixed["uncond"])
    check(rel_l2(first.latents.cpu(), ref), LOOP_BUDGET, f"{name} seeded dispatch vs host fp64 loop")
    per_row = [rel_l2(first.latents[i].cpu(), ref[i]) for i in range(len(SPLIT))]
    assert max(per_row) <= 2 * LOOP_BUDGET, per_row
    second = call(loop, mixed, cuda, seeds=SEEDS, latent_shape=SHAPE)
    assert all(r for *_, r in second.groups) and len(loop._graphs) == 3
    assert torch.equal(second.latents, first.latents)
    eager = call(loop, mixed, cuda, seeds=SEEDS, latent_shape=SHAPE, use_graph=False)
    assert torch.equal(eager.latents, first.latents)
    # seeds= is latents=ops.randn(...) here too (a stochastic scheduler takes the seeds next to the latents)
    lat = ops.randn((len(SPLIT),) + SHAPE, SEEDS, device=cuda)
    assert torch.equal(call(loop, mixed, cuda, latents=lat, seeds=SEEDS).latents, first.latents)
    # a prompt's initial latents depend on its seed alone, whatever batch, bucket or group it lands in
    for i, s in enumerate(SEEDS):
        assert torch.equal(lat[i:i + 1], ops.randn((1,) + SHAPE, [s], device=cuda))
    assert np.array_equal(ops.philox_bits((len(SPLIT), N), SEEDS, device=cuda).cpu().numpy().view(np.uint32), PO.bits_rows(SEEDS, 0, 0, N))
