"""pipeline.ExpertDispatchLoop on the GPU: a routed batch whose prompts go to several experts runs group by group through each
expert's compacted weights, one captured step per (expert, bucket), and comes back in the caller's prompt order.

Budgets are taken from tests/test_unet_gpu.py, not restated: the loop against the fp32 oracle loop under the 6e-2 that
``test_denoise_loop_hip_graph_matches_eager_and_oracle`` applies to its loop (guidance 3.0; here 5 steps against its 4, the same
number), pruned-expert runs under the 2e-2 (``TOL``) of ``test_pruned_model_semantics``."""
import copy

import pytest
import torch

from oracle import unet_oracle as O
from tests.margins import check

pytestmark = pytest.mark.gpu

LOOP_BUDGET = 6e-2       # test_unet_gpu.test_denoise_loop_hip_graph_matches_eager_and_oracle
PRUNED_TOL = 2e-2        # test_unet_gpu.TOL, as test_pruned_model_semantics applies it
STEPS, S = 5, 3.0


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def tiny(cuda):
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    cfg = O.TINY
    model = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                      cross_attention_dim=cfg.cross_attention_dim).init_synthetic(seed=0)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.to(cuda)
    return cfg, model, params


class Router:
    """a seeded hyper_net and a quantizer whose four hard codes are seeded 50 % masks, plus a pool of router inputs whose
    expert is known (evaluated on the host, kept only where the cosine assignment has a clear margin)"""

    def __init__(self, cfg, cuda):
        from diffusion_pruning_amd.hypernet import HyperStructure
        from diffusion_pruning_amd.quantizer import StructureVectorQuantizer
        st = O.get_structure(cfg)
        torch.manual_seed(0)
        hn = HyperStructure(structure=st, input_dim=16, wn_flag=False, linear_bias=True)
        qz = StructureVectorQuantizer(n_e=4, structure=st, temperature=0.4, base=3, resource_aware_normalization=False)
        codes = []
        for e in range(4):
            m = O.random_mask(cfg, 0.5, 20 + e, n_depth_off=e % 2)
            codes.append(torch.cat([w.reshape(1, -1) for w in m["width"]] + [d.reshape(1, 1) for d in m["depth"]], dim=1))
        self.codes = torch.cat(codes)                                     # [4, D] hard codes
        qz.embedding_gs.data = self.codes.clone()
        hn.eval()
        qz.eval()
        # the eval quantizer adds fixed-seed Gumbel noise PER BATCH ROW, so a weak assignment depends on where a prompt sits in
        # its batch: inputs large enough that the noise does not matter, kept only where the assignment has a clear cosine margin
        # and is the same alone, in the pool and in two shuffles of it
        gen = torch.Generator().manual_seed(1)
        pool = torch.randn(192, 16, generator=gen) * 400.0
        with torch.no_grad():
            z = hn(pool)
            sims = qz._unit(qz.gumbel_sigmoid_trick(z)) @ qz._unit(qz.embedding_gs).t()
            idx = qz(z)[1][2]
            stable = torch.cat([qz(hn(pool[i:i + 1]))[1][2] for i in range(len(pool))]) == idx
            for _ in range(2):
                perm = torch.randperm(len(pool), generator=gen)
                stable[perm] &= qz(hn(pool[perm]))[1][2] == idx[perm]
        top2 = sims.topk(2, dim=1).values
        stable &= (top2[:, 0] - top2[:, 1]) > 5e-3
        self.pool, self.idx, self.cpu = pool, idx, (hn, qz)
        self.free = {e: [i for i in range(len(pool)) if stable[i] and int(idx[i]) == e] for e in range(4)}
        assert all(len(v) >= 12 for v in self.free.values()), {e: len(v) for e, v in self.free.items()}
        self.hn, self.qz = copy.deepcopy(hn).to(cuda), copy.deepcopy(qz).to(cuda)

    def take(self, experts):
        """router inputs [len(experts), 16] whose prompts go to the given experts, in that order, checked on the host for this
        very batch; never handed out twice"""
        hn, qz = self.cpu
        rows = [self.free[e].pop(0) for e in experts]
        for _ in range(8):
            with torch.no_grad():
                got = qz(hn(self.pool[rows]))[1][2].tolist()
            wrong = [i for i, e in enumerate(experts) if got[i] != e]
            if not wrong:
                return self.pool[rows]
            for i in wrong:
                rows[i] = self.free[experts[i]].pop(0)
        raise AssertionError(f"no router inputs found for the split {experts}")

    def mask(self, experts):
        """the per-sample structure of these experts for the oracle"""
        return O.split_arch_vector(O.TINY, self.codes[list(experts)].clone())


@pytest.fixture(scope="module")
def router(cuda):
    return Router(O.TINY, cuda)


def inputs(cfg, n, seed):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(n, 4, 16, 16, generator=g)
    cond = torch.randn(n, 77, cfg.cross_attention_dim, generator=g)
    uncond = torch.randn(n, 77, cfg.cross_attention_dim, generator=g)
    return lat, cond, uncond


def scheduler(name):
    from diffusion_pruning_amd.pipeline import DDIMSchedulerLite, PNDMSchedulerLite
    return DDIMSchedulerLite() if name == "ddim" else PNDMSchedulerLite()


def oracle_loop(cfg, params, mask, name, lat, cond, uncond):
    sch = scheduler(name)
    ts = sch.set_timesteps(STEPS)
    gates = O.assign_gates(cfg, mask)
    B = lat.shape[0]
    x, ehs, state = lat.clone(), torch.cat([uncond, cond]), sch.make_state(lat)
    for i in range(sch.n_model_calls()):
        sch.load_step(state, i)
        noise = O.unet_forward(params, cfg, torch.cat([x, x]), ts[i].expand(2 * B), ehs, gates, "gated")
        u, c = noise.chunk(2)
        x = sch.step(u + S * (c - u), x, state)
    return x


SPLIT = [0, 1, 0, 2, 1, 0]                         # six prompts, three experts, 3 + 2 + 1, interleaved


@pytest.fixture(scope="module")
def mixed(tiny, router):
    """the 3 + 2 + 1 batch every test shares, and its oracle results (computed once per scheduler)"""
    cfg, _, params = tiny
    lat, cond, uncond = inputs(cfg, len(SPLIT), seed=11)
    case = {"x": router.take(SPLIT), "lat": lat, "cond": cond, "uncond": uncond, "oracle": {}}

    def oracle(name):
        if name not in case["oracle"]:
            case["oracle"][name] = oracle_loop(cfg, params, router.mask(SPLIT), name, lat, cond, uncond)
        return case["oracle"][name]
    case["oracle_fn"] = oracle
    return case


def call(loop, case, cuda, rows=None, **kw):
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    return loop(sel(case["cond"]).to(cuda), sel(case["lat"]).to(cuda), STEPS, S, hyper_net_input=sel(case["x"]).to(cuda),
                negative_prompt_embeds=sel(case["uncond"]).to(cuda), **kw)


@pytest.mark.parametrize("name", ["ddim", "pndm"])
def test_mixed_batch_matches_the_oracle_loop(tiny, router, mixed, cuda, name):
    from diffusion_pruning_amd.pipeline import ExpertDispatchLoop, PruningDenoiseLoop
    cfg, model, params = tiny
    loop = ExpertDispatchLoop(model, router.hn, router.qz, scheduler=scheduler(name))
    res = call(loop, mixed, cuda)
    torch.cuda.synchronize()
    assert res.arch_indices.tolist() == SPLIT                             # three experts, 3 + 2 + 1: nothing degenerated
    assert [(e, rows, b) for e, rows, b, _ in res.groups] == [(0, [0, 2, 5], 4), (1, [1, 4], 2), (2, [3], 1)]
    assert res.latents.shape == mixed["lat"].shape
    assert torch.equal(res.arch_vectors_quantized.cpu(), router.codes[SPLIT])
    ref = mixed["oracle_fn"](name)
    e = check(rel_l2(res.latents.float().cpu(), ref), LOOP_BUDGET, f"{name} dispatch vs oracle loop")
    # recorded, not bounded: this error relative to the parent's per-sample-gate call on the same inputs
    parent = call(PruningDenoiseLoop(model, router.hn, router.qz, scheduler=scheduler(name)), mixed, cuda, use_graph=False)
    e_parent = rel_l2(parent.latents.float().cpu(), ref)
    assert parent.arch_indices.tolist() == SPLIT
    print(f"{name}: dispatch {e:.3e}, per-sample gates {e_parent:.3e}")
    check(e / e_parent, float("inf"), f"{name} dispatch error / per-sample-gate error (recorded only)")


def test_results_come_back_in_caller_order(tiny, router, mixed, cuda):
    from diffusion_pruning_amd.pipeline import ExpertDispatchLoop, PruningDenoiseLoop
    cfg, model, params = tiny
    res = call(ExpertDispatchLoop(model, router.hn, router.qz), mixed, cuda)
    parent = PruningDenoiseLoop(model, router.hn, router.qz)
    singles = torch.cat([call(parent, mixed, cuda, rows=slice(i, i + 1), use_graph=False).latents for i in range(len(SPLIT))])
    _, idx = parent.route(mixed["x"].to(cuda))
    assert torch.equal(res.arch_indices, idx)
    d = torch.cdist(res.latents.flatten(1).double(), singles.flatten(1).double())
    assert d.argmin(dim=1).tolist() == list(range(len(SPLIT))), d
    assert float(d.diag().max()) < float(d[~torch.eye(len(SPLIT), dtype=torch.bool, device=d.device)].min())


def test_graphs_are_reused_across_calls(tiny, router, mixed, cuda):
    from diffusion_pruning_amd.pipeline import ExpertDispatchLoop
    cfg, model, params = tiny
    loop = ExpertDispatchLoop(model, router.hn, router.qz, scheduler=scheduler("pndm"))
    first = call(loop, mixed, cuda)
    assert not any(r for *_, r in first.groups) and len(loop._graphs) == 3
    graphs = [g["graph"] for g in loop._graphs.values()]
    # other prompts, the same split (another order): every captured step is reused
    order = [2, 0, 0, 1, 0, 1]
    lat, cond, uncond = inputs(cfg, 6, seed=12)
    other = {"x": router.take(order), "lat": lat, "cond": cond, "uncond": uncond}
    second = call(loop, other, cuda)
    assert second.arch_indices.tolist() == order
    assert all(r for *_, r in second.groups) and len(loop._graphs) == 3
    assert all(a is b for a, b in zip(graphs, [g["graph"] for g in loop._graphs.values()]))
    third = call(loop, other, cuda)
    assert torch.equal(second.latents, third.latents)
    assert not torch.equal(second.latents[:, 0], first.latents[:, 0])
    # a fourth expert: exactly one more capture
    order4 = [0, 3, 1, 0, 2, 1, 0]
    lat, cond, uncond = inputs(cfg, 7, seed=13)
    four = call(loop, {"x": router.take(order4), "lat": lat, "cond": cond, "uncond": uncond}, cuda)
    assert four.arch_indices.tolist() == order4
    assert [r for *_, r in four.groups] == [True, True, True, False] and len(loop._graphs) == 4


def test_padded_rows_are_computed_and_dropped(tiny, router, mixed, cuda):
    from diffusion_pruning_amd.pipeline import ExpertDispatchLoop
    cfg, model, params = tiny
    loop = ExpertDispatchLoop(model, router.hn, router.qz, group_sizes=(4,))
    res = call(loop, mixed, cuda)
    assert [(e, rows, b) for e, rows, b, _ in res.groups] == [(0, [0, 2, 5], 4), (1, [1, 4], 4), (2, [3], 4)]
    assert res.latents.shape == mixed["lat"].shape                         # [B, ...]: no padded row
    check(rel_l2(res.latents.float().cpu(), mixed["oracle_fn"]("ddim")), LOOP_BUDGET, "buckets (4,) vs oracle loop")


def test_experts_with_weights_of_their_own(tiny, router, mixed, cuda):
    from diffusion_pruning_amd.pipeline import ExpertDispatchLoop
    from diffusion_pruning_amd.unet import UNet2DConditionModelPruned
    cfg, model, params = tiny
    experts = {}
    for e in (0, 1):
        pm = UNet2DConditionModelPruned(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                        cross_attention_dim=cfg.cross_attention_dim)
        pm.load_state_dict(params)
        pm.to(cuda)
        experts[e] = pm.prune({k: [v.to(cuda) for v in vs] for k, vs in router.mask([e]).items()})
    rows = [0, 1, 2, 4]                                                     # experts 0, 1, 0, 1 of the shared batch
    own = call(ExpertDispatchLoop(model, router.hn, router.qz, experts=experts), mixed, cuda, rows=rows)
    assert own.arch_indices.tolist() == [0, 1, 0, 1] and [(e, r) for e, r, _, _ in own.groups] == [(0, [0, 2]), (1, [1, 3])]
    model.semantics = "pruned"                                              # the shared weights in pruned semantics
    try:
        shared = call(ExpertDispatchLoop(model, router.hn, router.qz), mixed, cuda, rows=rows)
    finally:
        model.semantics = "gated"
    check(rel_l2(own.latents, shared.latents), PRUNED_TOL, "experts= vs shared weights, pruned semantics")
    with pytest.raises(KeyError, match="2"):
        call(ExpertDispatchLoop(model, router.hn, router.qz, experts=experts), mixed, cuda)         # expert 2 is routed to


def test_lru_holds_at_most_max_graphs(tiny, router, mixed, cuda):
    from diffusion_pruning_amd.pipeline import ExpertDispatchLoop
    cfg, model, params = tiny
    loop = ExpertDispatchLoop(model, router.hn, router.qz, max_graphs=2)
    seen = []
    orig = loop._capture

    def counting(*a, **k):
        seen.append(len(loop._graphs))
        return orig(*a, **k)
    loop._capture = counting
    for _ in range(2):
        res = call(loop, mixed, cuda)
        assert len(loop._graphs) == 2
        check(rel_l2(res.latents.float().cpu(), mixed["oracle_fn"]("ddim")), LOOP_BUDGET, "max_graphs=2 vs oracle loop")
    assert seen and max(seen) <= 1                                          # room is made BEFORE a capture: never more than two


def test_images_in_caller_order(tiny, router, mixed, cuda):
    from diffusion_pruning_amd import vae as V
    from diffusion_pruning_amd.pipeline import ExpertDispatchLoop
    cfg, model, params = tiny
    m = V.AutoencoderKL().init_synthetic(seed=0).to(cuda)
    loop = ExpertDispatchLoop(model, router.hn, router.qz, vae=m)
    res = call(loop, mixed, cuda, output_type="pt")
    assert res.images.shape == (len(SPLIT), 3, 128, 128) and res.images.dtype == torch.float32
    assert torch.equal(res.images, loop.decode_latents(res.latents, "pt"))
    assert torch.equal(res.latents, call(loop, mixed, cuda).latents)       # the same latents as without decoding
