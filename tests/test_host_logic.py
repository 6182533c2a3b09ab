"""CPU tests of the product's host logic (no GPU): the model code runs unchanged, with the HIP ops replaced by the
test-only PyTorch emulator (tests/hip_emulator.py), and must agree with the oracle."""
import pytest
import torch

from oracle import unet_oracle as O
from tests import hip_emulator
from tests import tiles

TOL = 2e-2


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def clone_mask(m):
    return {k: [v.clone() for v in vs] for k, vs in m.items()}


@pytest.fixture()
def tiny(monkeypatch):
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    hip_emulator.install(monkeypatch)
    cfg = O.TINY
    model = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                      cross_attention_dim=cfg.cross_attention_dim).init_synthetic(seed=0)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return cfg, model, params


def run(model, mask, sample, t, ehs):
    model.set_structure(clone_mask(mask))
    with torch.no_grad():
        return model(sample, t, ehs).sample.float()


def test_state_dict_matches_diffusers_names_and_sd21_param_count():
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    m = UNet2DConditionModelGated()
    sd = m.state_dict()
    shapes = O.param_shapes(O.SD21)
    assert set(sd) == set(shapes)
    assert all(tuple(sd[k].shape) == shapes[k] for k in shapes)
    assert sum(p.numel() for p in m.parameters()) == 865_910_724
    st = m.get_structure()
    assert st == O.get_structure(O.SD21)
    assert sum(len(s) for s in st["width"]) == 70 and sum(d for s in st["depth"] for d in s) == 14
    mask = O.fixed_half_mask(O.SD21)
    m.set_structure(mask)
    assert mask["width"] == [] and mask["depth"] == []      # set_structure consumes the caller's lists


def test_dense(tiny):
    cfg, model, params = tiny
    sample, t, ehs = O.synthetic_inputs(cfg, 2, 16)
    ref = O.unet_forward(params, cfg, sample, t, ehs)
    assert rel_l2(run(model, O.ones_mask(cfg), sample, t, ehs), ref) <= TOL


def test_skip_concats_are_views_without_autograd(tiny):
    """the 12 torch.cat([hidden, skip]) of the up path (diffusers CrossAttnUpBlock2D.forward) are written in place by
    their producers; a hard depth gate of 0 makes the skipped block's consumer fall back to the copying concat"""
    from diffusion_pruning_amd import unet as U
    cfg, model, params = tiny
    sample, t, ehs = O.synthetic_inputs(cfg, 2, 16)
    n_cat = sum(len(b.resnets) for b in model.up_blocks)
    U.CAT_STATS.update(views=0, copies=0)
    ref = O.unet_forward(params, cfg, sample, t, ehs)
    assert rel_l2(run(model, O.ones_mask(cfg), sample, t, ehs), ref) <= TOL
    assert U.CAT_STATS == {"views": n_cat, "copies": 0}
    mask = O.ones_mask(cfg)
    for d in mask["depth"]:
        d.zero_()
    U.CAT_STATS.update(views=0, copies=0)
    ref = O.unet_forward(params, cfg, sample, t, ehs, O.assign_gates(cfg, clone_mask(mask)), "gated")
    assert rel_l2(run(model, mask, sample, t, ehs), ref) <= TOL
    assert U.CAT_STATS["views"] + U.CAT_STATS["copies"] == n_cat and U.CAT_STATS["copies"] > 0


def test_half_mask_matches_gated_not_pruned(tiny):
    cfg, model, params = tiny
    sample, t, ehs = O.synthetic_inputs(cfg, 2, 16)
    mask = O.fixed_half_mask(cfg)
    ref = O.unet_forward(params, cfg, sample, t, ehs, O.assign_gates(cfg, clone_mask(mask)), "gated")
    refp = O.unet_forward(params, cfg, sample, t, ehs, O.assign_gates(cfg, clone_mask(mask)), "pruned")
    out = run(model, mask, sample, t, ehs)
    e, ep = rel_l2(out, ref), rel_l2(out, refp)
    assert e <= TOL and ep > 2 * e, (e, ep)


@pytest.mark.parametrize("seed,keep,ndoff", [(1, 0.4, 2), (2, 0.75, 4)])
def test_random_masks_with_depth(tiny, seed, keep, ndoff):
    cfg, model, params = tiny
    sample, t, ehs = O.synthetic_inputs(cfg, 2, 16, seed=seed)
    mask = O.random_mask(cfg, keep, seed, n_depth_off=ndoff)
    ref = O.unet_forward(params, cfg, sample, t, ehs, O.assign_gates(cfg, clone_mask(mask)), "gated")
    assert rel_l2(run(model, mask, sample, t, ehs), ref) <= TOL


def test_soft_per_sample_cfg(tiny):
    cfg, model, params = tiny
    sample, t, ehs = O.synthetic_inputs(cfg, 4, 16, seed=9)
    g = torch.Generator().manual_seed(4)
    st = O.get_structure(cfg)
    mask = {"width": [torch.rand(2, w, generator=g) * 0.9 + 0.1 for sub in st["width"] for w in sub],
            "depth": [torch.rand(2, generator=g) for sub in st["depth"] for d in sub if d == 1]}
    ref = O.unet_forward(params, cfg, sample, t, ehs, O.assign_gates(cfg, clone_mask(mask)), "gated")
    assert rel_l2(run(model, mask, sample, t, ehs), ref) <= TOL


def test_hard_per_sample(tiny):
    cfg, model, params = tiny
    sample, t, ehs = O.synthetic_inputs(cfg, 2, 16, seed=5)
    mask = O.random_mask(cfg, 0.5, 7, n_depth_off=1, batch=2)
    mask["depth"][0] = torch.tensor([1.0, 0.0])
    ref = O.unet_forward(params, cfg, sample, t, ehs, O.assign_gates(cfg, clone_mask(mask)), "gated")
    assert rel_l2(run(model, mask, sample, t, ehs), ref) <= TOL


def test_pruned_semantics(tiny, monkeypatch):
    from diffusion_pruning_amd.unet import UNet2DConditionModelPruned
    cfg, model, params = tiny
    pm = UNet2DConditionModelPruned(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                    cross_attention_dim=cfg.cross_attention_dim)
    pm.load_state_dict(params)
    mask = O.random_mask(cfg, 0.5, 11, n_depth_off=2)
    soft = {"width": [w * 0.9 for w in mask["width"]], "depth": [d * 0.9 for d in mask["depth"]]}
    pm.prune(clone_mask(soft))
    sample, t, ehs = O.synthetic_inputs(cfg, 2, 16, seed=6)
    ref = O.unet_forward(params, cfg, sample, t, ehs, O.assign_gates(cfg, clone_mask(soft)), "pruned")
    with torch.no_grad():
        out = pm(sample, t, ehs, return_dict=False)[0]
    assert rel_l2(out.float(), ref) <= TOL


def test_product_rejects_cpu_tensors_without_the_emulator():
    """no CPU fallback: with the real ops, a CPU forward must fail loudly"""
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    cfg = O.TINY
    model = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                      cross_attention_dim=cfg.cross_attention_dim).init_synthetic(seed=0)
    sample, t, ehs = O.synthetic_inputs(cfg, 1, 16)
    with pytest.raises(Exception):
        model(sample, t, ehs)


def test_vectorised_relaxation_equals_the_per_segment_loop():
    """quantizer.gumbel_sigmoid_trick / width_depth_normalize are evaluated as whole-vector passes; the reference loops
    over the 70 width segments / 14 depth-gated blocks (quantizer.py:196-261).  Same host-RNG stream, same values, same
    gradients, including the non-zero-width rule on segments whose relaxation is dead."""
    import torch
    from diffusion_pruning_amd.estimation_utils import (gumbel_softmax_sample, hard_concrete,
                                                        importance_gumbel_softmax_sample)
    from diffusion_pruning_amd.quantizer import StructureVectorQuantizer
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    from oracle import unet_oracle as O
    cfg = O.TINY
    st = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                   cross_attention_dim=cfg.cross_attention_dim).get_structure()
    q = StructureVectorQuantizer(n_e=4, structure=st, temperature=0.4, base=3, resource_aware_normalization=False)
    q.train()
    nw = sum(q.width_list)
    torch.manual_seed(0)
    z = torch.randn(3, q.vq_embed_dim)
    s0 = 0
    for j, w in enumerate(q.width_list):          # kill a few segments (row 1) so the +0.5 rule fires
        if j % 9 == 0:
            z[1, s0:s0 + w] = -40.0
        s0 += w
    z1 = z.clone().requires_grad_(True)
    z2 = z.clone().requires_grad_(True)

    torch.manual_seed(77)
    got = q.gumbel_sigmoid_trick(z1)

    torch.manual_seed(77)                         # the reference's loop, verbatim order of host draws
    zw, zd = z2[:, :nw], z2[:, nw:]
    d_sorted = importance_gumbel_softmax_sample(zd, temperature=q.temperature, offset=q.base, fixed_seed=False)
    d = torch.zeros_like(d_sorted)
    d[:, q.depth_order] = d_sorted
    parts, s0 = [], 0
    for w in q.width_list:
        parts.append(gumbel_softmax_sample(zw[:, s0:s0 + w], temperature=q.temperature, offset=q.base,
                                           force_width_non_zero=True, fixed_seed=False))
        s0 += w
    ref = torch.cat([torch.cat(parts, dim=1), d], dim=1)
    assert torch.equal(got, ref)
    assert float((hard_concrete(got)[1, :nw].reshape(1, -1) @ q._seg_maps(got.device)[0]).min()) >= 1.0   # no dead segment left
    wgt = torch.randn_like(got)
    (got * wgt).sum().backward()
    (ref * wgt).sum().backward()
    assert torch.allclose(z1.grad, z2.grad, rtol=0, atol=0)

    # width_depth_normalize against the slice-assign loop
    a = got.detach().clone().requires_grad_(True)
    b = got.detach().clone().requires_grad_(True)
    out = q.width_depth_normalize(a)
    tmp = hard_concrete(b.clone())
    for i, has_depth in enumerate(q.depth_list):
        if has_depth != 0:
            lo, hi = q.width_intervals[i]
            di = q.depth_indices[i]
            tmp[:, lo:hi] = b[:, lo:hi] * b[:, di:di + 1]
    ref2 = tmp * torch.sqrt(q.template).detach()
    assert torch.equal(out, ref2)
    (out * wgt).sum().backward()
    (ref2 * wgt).sum().backward()
    assert torch.allclose(a.grad, b.grad, rtol=1e-5, atol=1e-6)    # the depth columns sum many products: order of summation only


def test_plan_cache_pins_plans_seen_during_capture_and_drops_stale_ones(monkeypatch):
    """a captured HIP graph bakes pointers to a plan's packs, so a plan created or used during capture must
    survive any number of other masks; and packs made from older parameter values must never be served again."""
    from diffusion_pruning_amd import modules as U
    c = U._PlanCache(cap=4)
    capturing = {"on": False}
    monkeypatch.setattr(U, "_capturing", lambda: capturing["on"])
    c.put("m0", (0,), "plan0")
    capturing["on"] = True
    assert c.get("m0", (0,)) == "plan0"             # used while capturing -> pinned
    c.put("mcap", (0,), "plancap")                  # created while capturing -> pinned
    capturing["on"] = False
    for i in range(1, 9):                           # eight more masks pass through a cache of four
        c.put(f"m{i}", (0,), f"plan{i}")
    assert c.get("m0", (0,)) == "plan0" and c.get("mcap", (0,)) == "plancap"
    assert c.get("m1", (0,)) is None and c.get("m8", (0,)) == "plan8"
    assert sum(1 for e in c.entries.values() if not e[2]) <= 4
    # an in-place parameter update bumps the version: stale entries are misses; a pinned one stays allocated (parked)
    assert c.get("m8", (1,)) is None and "m8" not in c.entries
    assert c.get("m0", (1,)) is None and "plan0" in c.parked
    c.clear()
    assert len(c) == 0 and not c.parked


def _captured_plan_outlives_updates(monkeypatch, mod, lookup, param):
    """a plan looked up "during capture" stays referenced by ``mod._plans`` (served or parked) through a lookup under the
    other ops.ACT_DTYPE and through an in-place weight update: a captured graph holds raw pointers to its packs.  Before
    these caches were _PlanCaches, AutoencoderKL's single slot per half and CLIPTextModel's dict released such a plan."""
    from diffusion_pruning_amd import modules as U, ops
    capturing = {"on": True}
    monkeypatch.setattr(U, "_capturing", lambda: capturing["on"])
    held = lambda: [id(e[1]) for e in mod._plans.entries.values()] + [id(q) for q in mod._plans.parked]      # noqa: E731
    pl = lookup()
    capturing["on"] = False
    with monkeypatch.context() as mp:
        mp.setattr(ops, "ACT_DTYPE", torch.float32)
        lookup()
        assert id(pl) in held()
    assert lookup() is pl                           # still the plan of its own key
    with torch.no_grad():
        param.mul_(1.0)                             # bumps the version counter
    assert lookup() is not pl and id(pl) in held()  # stale: never served again, but not released
    mod.invalidate()
    assert id(pl) not in held() and len(mod._plans) == 0


@pytest.mark.parametrize("half", ["decoder", "encoder"])
def test_vae_plan_seen_during_capture_outlives_dtype_switch_and_weight_update(monkeypatch, half):
    from diffusion_pruning_amd.vae import AutoencoderKL, VAEConfig
    vae = AutoencoderKL(VAEConfig(block_out_channels=(32, 64), layers_per_block=1), with_encoder=True).init_synthetic(0)
    cpu = torch.device("cpu")
    if half == "decoder":
        _captured_plan_outlives_updates(monkeypatch, vae, lambda: vae.plan(cpu), vae.decoder.conv_in.weight)
    else:
        _captured_plan_outlives_updates(monkeypatch, vae, lambda: vae.encoder_plan(cpu), vae.encoder.conv_in.weight)


@pytest.mark.parametrize("fold", [True, False])
def test_text_encoder_plan_seen_during_capture_outlives_dtype_switch_and_weight_update(monkeypatch, fold):
    from diffusion_pruning_amd.text_encoder import CLIPTextModel
    te = CLIPTextModel(vocab_size=256, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                       max_position_embeddings=77).init_synthetic(0)
    _captured_plan_outlives_updates(monkeypatch, te, lambda: te.plan(torch.device("cpu"), fold),
                                    te.text_model.final_layer_norm.weight)
    # and a plan of the other form does not displace it: 2 dtypes x 2 forms fit unpinned
    pl = te.plan(torch.device("cpu"), fold)
    te.plan(torch.device("cpu"), not fold)
    assert te.plan(torch.device("cpu"), fold) is pl


@pytest.mark.parametrize("cls", ["Downsample2D", "Upsample2D"])
def test_resample_plan_seen_during_capture_outlives_dtype_switch_and_weight_update(monkeypatch, cls):
    from diffusion_pruning_amd import unet as U
    m = getattr(U, cls)(32)
    with torch.no_grad():
        m.conv.weight.normal_()
        m.conv.bias.zero_()
    _captured_plan_outlives_updates(monkeypatch, m, lambda: m.plan(torch.device("cpu")), m.conv.weight)


def test_resnet_plan_follows_in_place_parameter_updates(tiny):
    """a fine-tuning loop that never calls invalidate_plans() must still compute with the current weights"""
    cfg, model, params = tiny
    model.set_structure(clone_mask(O.fixed_half_mask(cfg)))
    r = model.down_blocks[0].resnets[0]
    p0 = r.plan(torch.device("cpu"))
    assert r.plan(torch.device("cpu")) is p0
    with torch.no_grad():
        r.conv1.weight.mul_(2.0)                    # what optimizer.step() does: an in-place update
    p1 = r.plan(torch.device("cpu"))
    assert p1 is not p0
    assert torch.allclose(p1["w1"].w.float(), (p0["w1"].w.float() * 2), rtol=1e-2)
    assert len(r._plans) == 1                       # the stale plan is gone, not merely shadowed
    t = model.down_blocks[0].attentions[0]
    q0 = t.plan(torch.device("cpu"))
    with torch.no_grad():
        t.proj_in.bias.add_(1.0)
    assert t.plan(torch.device("cpu")) is not q0


def test_prefetch_plan_is_per_thread_and_scoped_to_the_forward(tiny):
    import threading
    from diffusion_pruning_amd import ops
    cfg, model, params = tiny
    seen = {}

    def probe(x, pw, **kw):
        seen.setdefault(threading.get_ident(), []).append(ops._current_prefetch_plan())
        return hip_emulator.conv_gemm(x, pw, **kw)
    ops.conv_gemm = probe                           # (restored by the fixture's monkeypatch teardown)
    sample, t, ehs = O.synthetic_inputs(cfg, 1, 16)
    run(model, O.ones_mask(cfg), sample, t, ehs)
    main_plans = set(id(p) for p in seen[threading.get_ident()])
    assert len(main_plans) == 1 and None not in seen[threading.get_ident()]
    assert ops._current_prefetch_plan() is None     # cleared when the forward returns
    other = {}
    th = threading.Thread(target=lambda: other.setdefault("plan", ops._current_prefetch_plan()))
    th.start(); th.join()
    assert other["plan"] is None                    # another thread never sees this thread's plan


def test_tuning_lookup_falls_back_to_the_nearest_tuned_shape_of_the_same_class():
    """shapes of architecture codes that were never tuned (config 5's experts) take the tile of the closest tuned shape"""
    from diffusion_pruning_amd import ops
    exact = ops.tuning_lookup(16384, 320, 320, 1, 1, 0, False)
    assert exact is ops.TUNING[ops.tuning_key(16384, 320, 320, 1, 1, 0, False)]
    near = ops.tuning_lookup(16384, 328, 320, 1, 1, 0, False)               # a 41-group expert width: not in the table
    assert near is not None and near["tile"] == exact["tile"]
    assert ops.tuning_lookup(16384, 328, 320, 1, 1, 0, False) is near       # cached
    assert ops.tuning_lookup(24, 40, 72, 1, 1, 0, False) is None            # nothing within reach: the library heuristic decides
    far3x3 = ops.tuning_lookup(16384, 176, 352, 9, 1, 0, False)
    assert far3x3 is not None and far3x3["tile"] not in ops._HALO_TILES
    # a neighbour's split-K never leaves a slice with fewer than four K-steps
    deep = ops.tuning_lookup(256, 1280, 1200, 9, 1, 0, False)
    assert deep is not None and deep["split_k"] <= max(1, (9 * 1200 // 64) // 4)
    # the LDS-DMA tiles (every id past the six register-staged ones) take channel steps up to 4032: a shape with more channels per tap
    # never inherits one from a neighbour (round 4: the batch-64 training shapes put 128x160 DMA tiles next to K = 5120 linears)
    for M in (16384, 12288, 4096 * 3):
        wide = ops.tuning_lookup(M, 1280, 5100, 1, 1, 0, False)
        assert wide is None or wide["tile"] <= 6, wide


# ---- ops.conv_gemm's launch choice (diffusion_pruning_amd/launch_policy.py), rule by rule; shapes from the committed table -------
LIBRARY = (0, None, None)          # tile 0 = the library's pick_tile, split_k None = aptp_conv_gemm_suggest_split_k


@pytest.fixture()
def policy(monkeypatch):
    """the policy module; table and switches are put back afterwards (the entries keep their identity)"""
    from diffusion_pruning_amd import launch_policy as lp
    saved = dict(lp.TUNING)
    for sw in ("TUNING_NEAREST", "LEAN_REMAP", "SK_AUTO"):
        monkeypatch.setattr(lp, sw, True)
    yield lp
    lp.set_tuning(saved)


def choose(lp, M, N, Cin, taps=1, *, geglu=False, Cin2=0, plain=False, f32=False, tile=0, split_k=None, order=0, stride=1, ups=0):
    k = {1: 1, 9: 3}[taps]
    pad = lambda c: (c + 63) // 64 * 64
    return lp.choose_launch(M, N, Cin, pad(Cin), k, k, stride, ups, 2 if geglu else 0, Cin2, pad(Cin2),      # (2 = ACT_GEGLU)
                            plain_linear=plain, f32=f32, tile=tile, split_k=split_k, order=order)


def test_launch_policy_imports_without_torch_or_the_library():
    import os
    import subprocess
    import sys
    code = ("import sys; import diffusion_pruning_amd.launch_policy as lp; assert 'torch' not in sys.modules; "
            "assert lp.choose_launch(24, 40, 72, 128, 1, 1, 1, 0, 0, 0, 0, plain_linear=False, f32=False, tile=0, split_k=None, order=0) == (0, None, None, 0)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


def test_rule1_caller_given_tile_split_k_and_the_fp32_path_bypass_table_and_heuristics(policy):
    assert policy.tuning_lookup(16384, 320, 320, 1, 1, 0, False) is not None           # an exact entry that would otherwise decide
    assert choose(policy, 16384, 320, 320, plain=True, tile=3, order=2) == (3, None, None, 2)
    assert choose(policy, 16384, 320, 320, plain=True, split_k=2) == (0, 2, None, 0)
    assert choose(policy, 16384, 320, 320, plain=True, f32=True) == LIBRARY + (0,)
    assert choose(policy, 65536, 1280, 1280, 9, f32=True) == LIBRARY + (0,)             # (stream-K sized: still the library's tiles 1..6)


def test_rule2_the_table_entry_gives_tile_split_k_form_and_order(policy):
    e = policy.TUNING["M16384_N320_C320_T1_s1u0g0"]                                    # a lean tile, tuned in situ, order 3
    assert (e["tile"], e["split_k"], e["in_kernel"], e["order"]) == (11, 1, 0, 3)
    assert choose(policy, 16384, 320, 320, plain=True) == (11, 1, False, 3)
    assert choose(policy, 16384, 320, 320, plain=True, order=2) == (11, 1, False, 2)   # a caller-given order survives
    e = policy.TUNING["M256_N640_C1280_T1_s1u0g0"]                                     # split along K, combined in-kernel
    assert choose(policy, 256, 640, 1280, plain=True) == (e["tile"], 4, True, e["order"])
    e = policy.TUNING["M16384_N320_C960_T1_s1u0g0"]                                    # no "in_kernel" in the entry: false
    assert "in_kernel" not in e and choose(policy, 16384, 320, 960) == (e["tile"], e["split_k"], False, e["order"])
    assert policy.TUNING["M1024_N10240_C1280_T1_s1u0g0"]["order"] == 0                 # the entry's own 0 is passed on as it is
    assert choose(policy, 1024, 10240, 1280, plain=True)[3] == 0
    policy.set_entry("M24_N40_C72_T1_s1u0g0", {"tile": 12, "split_k": 1})              # an entry without "order": the legacy order
    assert choose(policy, 24, 40, 72) == (12, 1, False, 1)
    assert choose(policy, 24, 40, 72, order=3) == (12, 1, False, 3)
    # the nearest tuned shape of the same class stands in (a 41-group expert width)
    assert "M16384_N328_C320_T1_s1u0g0" not in policy.TUNING
    assert choose(policy, 16384, 328, 320, plain=True) == (11, 1, False, 3)
    policy.TUNING_NEAREST = False
    assert choose(policy, 16384, 328, 320) == LIBRARY + (0,)
    assert choose(policy, 16384, 320, 320, plain=True) == (11, 1, False, 3)            # (exact entries are not affected)


def test_rule3_entries_that_do_not_apply_are_dropped(policy):
    # only a neighbour's entry, and the shape is in the stream-K range of rule 6: stream-K wins
    near = policy.tuning_lookup(65536, 328, 1280, 1, 1, 0, False)
    assert "M65536_N328_C1280_T1_s1u0g0" not in policy.TUNING and near is not None and near["tile"] == 19
    assert 65536 * 328 >= policy.SK_AUTO_MIN_OUTPUTS and 1280 // 64 >= 16
    assert choose(policy, 65536, 328, 1280) == (64, 2, True, 3)
    assert choose(policy, 65536, 320, 1280) == (19, 1, False, 0)                       # the exact entry of the same range is kept
    assert choose(policy, 65536, 328, 640)[0] == policy.tuning_lookup(65536, 328, 640, 1, 1, 0, False)["tile"]     # 10 K-steps: kept
    policy.SK_AUTO = False
    assert choose(policy, 65536, 328, 1280) == (19, 1, False, 0)
    # an LDS-DMA tile (id >= 7) addresses 4032 channels per tap, a stream-K tile 32704
    policy.set_tuning({"M64_N64_C4096_T1_s1u0g0": {"tile": 9, "split_k": 1, "order": 1},
                       "M64_N64_C4032_T1_s1u0g0": {"tile": 9, "split_k": 1, "order": 1},
                       "M128_N64_C4096_T1_s1u0g0": {"tile": 6, "split_k": 2, "order": 1},
                       "M64_N64_C64_T9_s1u0g0x4096": {"tile": 13, "split_k": 1, "order": 1},
                       "M256_N64_C4096_T1_s1u0g0": {"tile": 64, "split_k": 2, "in_kernel": 1, "order": 3},
                       "M256_N64_C32768_T1_s1u0g0": {"tile": 64, "split_k": 2, "in_kernel": 1, "order": 3}})
    assert choose(policy, 64, 64, 4096) == LIBRARY + (0,)
    assert choose(policy, 64, 64, 4032) == (9, 1, False, 1)
    assert choose(policy, 128, 64, 4096) == (6, 2, False, 1)                           # register-staged: no limit
    assert choose(policy, 64, 64, 64, 9, Cin2=4096) == LIBRARY + (0,)                  # the second operand's channels count too
    assert choose(policy, 256, 64, 4096) == (64, 2, True, 3)
    assert choose(policy, 256, 64, 32768) == LIBRARY + (0,)


def test_rule4_a_tuned_plain_linear_layer_on_a_tile_without_lean_instantiation_is_remapped(policy):
    for M, N, C, was, now in ((16384, 640, 320, 19, 11), (4096, 5120, 640, 19, 18), (256, 1280, 640, 59, 49)):
        e = policy.TUNING[policy.tuning_key(M, N, C, 1, 1, 0, False)]
        assert e["tile"] == was and was not in policy._LEAN_TILES and e["split_k"] == 1 and "insitu" not in e
        assert choose(policy, M, N, C, plain=True) == (now, 1, False, e["order"])
        assert choose(policy, M, N, C, plain=False) == (was, 1, False, e["order"])     # some epilogue the lean kernel does not have
    e = policy.TUNING["M1024_N7680_C1280_T1_s1u0g1"]                                   # chosen in situ with the lean kernel present: kept
    assert e["tile"] == 21 and "insitu" in e
    assert choose(policy, 1024, 7680, 1280, geglu=True, plain=True)[0] == 21
    e = policy.TUNING["M256_N1280_C3840_T1_s1u0g0"]                                    # split along K: not the lean kernel's
    assert e["tile"] == 40 and e["split_k"] == 6
    assert choose(policy, 256, 1280, 3840, plain=True)[:2] == (40, 6)
    assert choose(policy, 16384, 320, 320, plain=True)[0] == 11                        # already a lean tile: as tuned
    assert policy.TUNING["M4096_N1280_C1280_T1_s1u0g0"]["tile"] == 9 and choose(policy, 4096, 1280, 1280, plain=True)[0] == 9
    # only a key named exactly "insitu" exempts an entry
    policy.set_entry("M24_N40_C72_T1_s1u0g0", {"tile": 19, "split_k": 1, "order": 1, "insitu_train": 1.0})
    assert choose(policy, 24, 40, 72, plain=True) == (49, 1, False, 1)
    policy.set_entry("M24_N40_C72_T1_s1u0g0", {"tile": 19, "split_k": 1, "order": 1, "insitu": 1.0})
    assert choose(policy, 24, 40, 72, plain=True) == (19, 1, False, 1)
    policy.LEAN_REMAP = False
    assert choose(policy, 16384, 640, 320, plain=True)[0] == 19


def test_rule5_an_untuned_plain_linear_layer_takes_a_lean_tile_by_row_count(policy):
    assert policy.tuning_lookup(24, 40, 72, 1, 1, 0, False) is None                    # nothing within reach in the committed table
    assert choose(policy, 24, 40, 72, plain=True, order=2) == (49, 1, None, 2)
    policy.set_tuning({})                                                              # no neighbour interferes below
    assert choose(policy, 8192, 320, 320, plain=True) == (11, 1, None, 0)
    assert choose(policy, 8191, 320, 320, plain=True) == (18, 1, None, 0)
    assert choose(policy, 2048, 320, 320, plain=True) == (18, 1, None, 0)
    assert choose(policy, 2047, 320, 320, plain=True) == (49, 1, None, 0)
    assert choose(policy, 4096, 5120, 640, geglu=True, plain=True) == (18, 1, None, 0)
    # tiny M with a long K wants a K split: back to the library
    assert choose(policy, 512, 1280, 1280, plain=True) == LIBRARY + (0,)
    assert choose(policy, 513, 1280, 1280, plain=True) == (49, 1, None, 0)
    assert choose(policy, 512, 1280, 1216, plain=True) == (49, 1, None, 0)
    assert choose(policy, 4096, 1280, 4032, plain=True) == (18, 1, None, 0)
    assert choose(policy, 4096, 1280, 4040, plain=True) == LIBRARY + (0,)              # past the LDS-DMA tiles' channel range
    assert choose(policy, 4096, 320, 320, plain=False) == LIBRARY + (0,)
    assert choose(policy, 65536, 1280, 1280, plain=True) == (11, 1, None, 0)           # (before the stream-K take-over)
    policy.LEAN_REMAP = False
    assert choose(policy, 4096, 320, 320, plain=True) == LIBRARY + (0,)


def test_rule6_large_untuned_contractions_take_the_stream_k_tiles(policy):
    policy.set_tuning({})
    assert policy.SK_AUTO_MIN_OUTPUTS == 256 * 256 * 160 == 8192 * 1280
    assert choose(policy, 8192, 1280, 1280, 9) == (64, 2, True, 3)
    assert choose(policy, 8192, 1280, 1280, 9, order=2) == (64, 2, True, 2)            # a caller-given order survives
    assert choose(policy, 8192, 2560, 1280, geglu=True) == (65, 2, True, 3)            # 256 x 128 for GEGLU's column pairs
    assert choose(policy, 8192, 1272, 1280, 9) == LIBRARY + (0,)                       # too few outputs
    assert choose(policy, 8192, 1280, 1024) == (64, 2, True, 3)                        # 16 K-steps
    assert choose(policy, 8192, 1280, 960) == LIBRARY + (0,)                           # 15
    assert choose(policy, 8192, 1280, 64, 9, Cin2=448) == (64, 2, True, 3)             # 9 + 7 K-steps with the second operand's
    assert choose(policy, 8192, 1280, 32704) == (64, 2, True, 3)
    assert choose(policy, 8192, 1280, 32768) == LIBRARY + (0,)                         # past the stream-K tiles' channel range
    policy.SK_AUTO = False
    assert choose(policy, 8192, 1280, 1280, 9) == LIBRARY + (0,)


def test_rule7_otherwise_the_library_decides(policy):
    assert choose(policy, 24, 40, 72) == LIBRARY + (0,)
    assert choose(policy, 24, 40, 72, 9, order=3) == LIBRARY + (3,)


def test_split_k_form(policy):
    f = policy.splitk_in_kernel
    kw = dict(explicit=False, reduce_launch=False, rowstats=False, colstats=False)
    assert [f(s, None, **kw) for s in (2, 4, 5, 8)] == [True, True, False, False]      # untuned: in-kernel up to 4 slices
    assert f(8, None, **dict(kw, explicit=True))                                       # ... or when the caller chose the depth
    assert not f(2, False, **kw) and f(8, True, **kw)                                  # tuned per shape
    assert f(8, False, **dict(kw, rowstats=True))                                      # only the combining workgroup can emit statistics
    assert policy.COLS_SPLIT_MAX == 2
    assert f(2, False, **dict(kw, colstats=True)) and not f(3, False, **dict(kw, colstats=True))
    assert not f(2, True, **dict(kw, reduce_launch=True))                              # the reduce launch applies the fused GroupNorm


def test_editing_the_table_drops_the_cached_nearest_shape_answers(policy):
    from diffusion_pruning_amd import ops
    assert ops.TUNING is policy.TUNING
    key = "M16384_N320_C320_T1_s1u0g0"
    near = ops.tuning_lookup(16384, 328, 320, 1, 1, 0, False)
    assert near["tile"] == policy.TUNING[key]["tile"] == 11
    tuned = policy.TUNING[key]
    ops.set_entry(key, dict(tuned, tile=12))                                           # (no other entry of the class within reach has tile 12)
    assert ops.tuning_lookup(16384, 328, 320, 1, 1, 0, False)["tile"] == 12
    ops.set_entry(key, None)                                                           # removed: some other neighbour, or none
    assert key not in ops.TUNING and (ops.tuning_lookup(16384, 328, 320, 1, 1, 0, False) or {"tile": 0})["tile"] != 12
    ops.set_entry(key, tuned)
    assert ops.tuning_lookup(16384, 320, 320, 1, 1, 0, False) is tuned and ops.tuning_lookup(16384, 328, 320, 1, 1, 0, False) == near
    ops.set_tuning({})
    assert ops.TUNING is policy.TUNING and not ops.TUNING
    assert ops.tuning_lookup(16384, 328, 320, 1, 1, 0, False) is None and ops.tuning_lookup(16384, 320, 320, 1, 1, 0, False) is None
    ops.set_tuning({key: {"tile": 25, "split_k": 1, "order": 1}})
    assert ops.tuning_lookup(16384, 328, 320, 1, 1, 0, False)["tile"] == 25


def test_tuning_keys_round_trip():
    from types import SimpleNamespace
    from diffusion_pruning_amd import _lib, launch_policy as lp
    for k in lp.TUNING:
        assert lp.tuning_key(*lp.parse_key(k)) == k
    assert lp.parse_key("M4096_N640_C320_T9_s1u0g0x640") == (4096, 640, 320, 9, 1, 0, False, 640)
    assert lp.parse_key("M4_N8_C8_T1_s1u0g1") == (4, 8, 8, 1, 1, 0, True, 0) and lp.parse_key("us") is None
    p = SimpleNamespace(B=4, Hout=32, Wout=32, N=640, Cin=320, KH=3, KW=3, stride=1, ups=0, act=_lib.ACT_GEGLU, Cin2=640, x2=None)
    assert lp.key_of(p) == "M4096_N640_C320_T9_s1u0g1"                                 # Cin2 counts only with an x2 operand
    p.x2, p.act = 1234, 0
    assert lp.key_of(p) == "M4096_N640_C320_T9_s1u0g0x640"


def test_the_tile_ids_of_the_policy_are_the_library_s():
    import os
    import re
    from diffusion_pruning_amd import _lib, launch_policy as lp
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "aptp_hip.h")).read()
    enum = {n: int(v) for n, v in re.findall(r"APTP_TILE_(\w+)\s*=\s*(\d+)", header)}
    assert enum["AUTO"] == 0 and len(set(enum.values())) == len(enum)
    n_tiles = len(tiles.TILES) + 1                                                     # (kNumTiles: the rows and id 0 = auto)
    assert sorted(enum.values()) == list(range(n_tiles))
    assert {t.name: t.id for t in tiles.TILES} == {n: v for n, v in enum.items() if n != "AUTO"}   # (csrc static_asserts the same)
    named = {n[5:]: v for n, v in vars(_lib).items() if n.startswith("TILE_")}
    assert named and all(enum[n] == v for n, v in named.items())                       # no second numbering
    assert set(tiles.LIN) == set(lp._LEAN_TILES) == {9, 11, 12, 15, 17, 18, 24, 25, 26} | set(range(45, 54))
    assert set(lp._HALO_TILES) == set(tiles.HALO) == {enum["HALO_128x160"], enum["HALO_128x128"]}
    assert lp.DMA_TILE_FIRST == max(tiles.REG) + 1 == len(tiles.REG) + 1 and lp.SK_TILE_FIRST == min(tiles.SK)
    assert tiles.SK == tuple(range(min(tiles.SK), n_tiles))                            # (ops and the policy test `tile >= SK_TILE_FIRST`)
    assert lp.DMA_TILE_FIRST == enum["DMA_128x128"] == enum["64x64"] + 1 and lp.SK_TILE_FIRST == enum["SK_256x160"]
    policy_tiles = set(lp._LEAN_TILES) | set(lp._HALO_TILES) | {lp.DMA_TILE_FIRST, lp.SK_TILE_FIRST, _lib.TILE_SK_256x160, _lib.TILE_SK_256x128}
    policy_tiles |= {lp._lean_tile(M) for M in (1, 2048, 8192)}
    assert {lp._lean_tile(M) for M in (1, 2048, 8192)} <= set(lp._LEAN_TILES)
    assert all(0 < t < n_tiles for t in policy_tiles)
    assert all(0 < e["tile"] < n_tiles for e in lp.TUNING.values())


def test_the_compiled_tile_geometry_is_the_table_s():
    """The host helpers that size a launch's workspace, arrival counters and statistics buffers index the compiled tile table by id:
    a wrong extent there is a slab that is too small, not a failing number.  For every id the library's answers equal the ones
    recorded from the last library with a hand-written table (tests/golden/conv_gemm_tile_helpers.json) AND what the id's row of
    csrc/conv_gemm_tiles.h predicts.  The problem's extents (M = 407, N = 328) are multiples of no tile size and tell every
    (bm, bn, wn, waves) combination apart.  The stream-K workspace scales with the CU count the runtime reports: a positive
    multiple of two fp32 tiles, whatever the machine."""
    import ctypes
    import json
    import os
    from diffusion_pruning_amd import _lib
    lib = _lib.load()
    rec = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_gemm_tile_helpers.json")))
    prob = rec["problem"]
    M, N, split_k = prob["B"] * prob["Hout"] * prob["Wout"], prob["N"], prob["split_k"]
    assert (M, N, split_k) == (407, 328, 3) and rec["columns"] == ["tiles", "colstat_rows", "rowstat_slots", "workspace_bytes"]
    assert sorted(map(int, rec["rows"])) == list(tiles.ALL) + [len(tiles.ALL) + 1]
    assert [rec["rows"][i] for i in ("1", "6")] == [[12, 64, 6, 2359296], [42, 32, 12, 2064384]]
    assert rec["rows"]["66"][:3] == [8, 64, 8] and rec["rows"]["72"][:3] == [12, 32, 6]

    def ask(tile):
        p = _lib.ConvGemmParams(tile=tile, **prob)
        r = ctypes.byref(p)
        return [lib.aptp_conv_gemm_tiles(r), lib.aptp_conv_gemm_colstat_rows(r), lib.aptp_conv_gemm_rowstat_slots(r),
                lib.aptp_conv_gemm_workspace_bytes(r)]

    for t in tiles.TILES:
        got, want = ask(t.id), rec["rows"][str(t.id)]
        tm, tn = -(-M // t.bm), -(-N // t.bn)
        row = [tm * tn, t.bm // t.wm, tn * t.wn, split_k * tm * t.bm * tn * t.bn * 4]
        if t.id in tiles.SK:
            assert got[3] > 0 and got[3] % (2 * t.bm * t.bn * 4) == 0 and want[3] % (2 * t.bm * t.bn * 4) == 0, (t, got, want)
            got, want, row = got[:3], want[:3], row[:3]
        assert got == want == row, (t, got, want, row)
    past = len(tiles.TILES) + 1                                                        # no such tile: no tiles, no statistics rows
    assert ask(past)[:3] == rec["rows"][str(past)][:3] == [0, 0, 0] and ask(past)[3] == rec["rows"][str(past)][3] == split_k * M * N * 4


# ---- the same host logic without any rounding: fp32 storage end to end (emulator exact mode) vs the fp32 oracle -------------
EXACT_TOL = 1e-5


@pytest.fixture()
def tiny_exact(monkeypatch):
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    hip_emulator.install(monkeypatch, exact=True)
    cfg = O.TINY
    model = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                      cross_attention_dim=cfg.cross_attention_dim).init_synthetic(seed=0)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return cfg, model, params


@pytest.mark.parametrize("case", ["dense", "half_gated", "random_depth", "soft_cfg", "hard_per_sample"])
def test_host_logic_is_exact_in_fp32(tiny_exact, case):
    """SURVEY §8 preamble asks for an fp32 path at <= 1e-5 per op / <= 1e-4 whole U-Net.  The MFMA kernels are bf16 by
    construction, so what an fp32 run can pin is everything AROUND them: weight compaction by architecture code, the
    GroupNorm-beta border-class correction that separates gated from pruned semantics, gate / depth-lerp epilogue
    semantics, LayerNorm folding into packed weights, the fused shortcut K-segment, batched time-embedding and text K/V
    projections, in-place skip-concats.  Here that logic runs with fp32 storage end to end (no rounding point left) and
    must reproduce the fp32 oracle to 1e-5 -- two orders below the 1e-2 level at which bf16 storage would mask a defect."""
    cfg, model, params = tiny_exact
    if case == "dense":
        B, mask, sem, seed = 2, O.ones_mask(cfg), "gated", 1
    elif case == "half_gated":
        B, mask, sem, seed = 2, O.fixed_half_mask(cfg), "gated", 2
    elif case == "random_depth":
        B, mask, sem, seed = 2, O.random_mask(cfg, 0.4, 1, n_depth_off=2), "gated", 3
    elif case == "soft_cfg":
        g = torch.Generator().manual_seed(4)
        st = O.get_structure(cfg)
        B, sem, seed = 4, "gated", 9
        mask = {"width": [torch.rand(2, w, generator=g) * 0.9 + 0.1 for sub in st["width"] for w in sub],
                "depth": [torch.rand(2, generator=g) for sub in st["depth"] for d in sub if d == 1]}
    else:
        B, sem, seed = 2, "gated", 5
        mask = O.random_mask(cfg, 0.5, 7, n_depth_off=1, batch=2)
        mask["depth"][0] = torch.tensor([1.0, 0.0])
    sample, t, ehs = O.synthetic_inputs(cfg, B, 16, seed=seed)
    ref, blocks = O.unet_forward(params, cfg, sample, t, ehs, O.assign_gates(cfg, clone_mask(mask)), sem, return_blocks=True)
    seen = {}
    hooks = [model.mid_block.register_forward_hook(lambda m, i, o: seen.__setitem__("mid", o)),
             model.down_blocks[0].register_forward_hook(lambda m, i, o: seen.__setitem__("down0", o[0]))]
    out = run(model, mask, sample, t, ehs)
    for h in hooks:
        h.remove()
    assert out.dtype == torch.float32
    assert rel_l2(seen["down0"].float(), blocks[0]) <= EXACT_TOL
    assert rel_l2(seen["mid"].float(), blocks[4]) <= EXACT_TOL
    e = rel_l2(out, ref)
    assert e <= EXACT_TOL, e


def test_pruned_semantics_is_exact_in_fp32(tiny_exact):
    from diffusion_pruning_amd.unet import UNet2DConditionModelPruned
    cfg, _, params = tiny_exact
    pm = UNet2DConditionModelPruned(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                    cross_attention_dim=cfg.cross_attention_dim)
    pm.load_state_dict(params)
    mask = O.random_mask(cfg, 0.5, 3, n_depth_off=2)
    sample, t, ehs = O.synthetic_inputs(cfg, 2, 16, seed=8)
    ref = O.unet_forward(params, cfg, sample, t, ehs, O.assign_gates(cfg, clone_mask(mask)), "pruned")
    pm.prune(clone_mask(mask))
    with torch.no_grad():
        out = pm(sample, t, ehs).sample.float()
    assert rel_l2(out, ref) <= EXACT_TOL
    gated = O.unet_forward(params, cfg, sample, t, ehs, O.assign_gates(cfg, clone_mask(mask)), "gated")
    assert rel_l2(out, gated) > 100 * EXACT_TOL        # ... and the two semantics really differ (the beta term)


@pytest.mark.parametrize("wn,bias", [(True, False), (False, True), (True, True), (False, False)])
def test_hypernet_heads_as_one_gemm_equal_the_per_head_loop(wn, bias):
    """HyperStructure._forward_fused (parameters re-homed into flat storage, one weight-normalised GEMM) vs the reference's
    per-head loop (hypernet.py:62-72): same outputs, same per-parameter gradients, same state_dict keys; the aliasing
    survives optimizer steps, load_state_dict and deepcopy."""
    import copy
    from diffusion_pruning_amd.hypernet import HyperStructure
    st = {"width": [[32, 32], [5, 5, 20]], "depth": [[1, 1], [1]]}
    torch.manual_seed(0)
    h = HyperStructure(st, wn_flag=wn, linear_bias=bias)
    if bias:
        with torch.no_grad():
            for hd in h.mh_fc:
                hd.bias.normal_()
    loop = copy.deepcopy(h)
    loop.fuse_heads = False
    x = torch.randn(4, 768)

    def close(a, b):
        # 1e-6 relative to the outputs' scale (they reach ~5): the fused GEMM and the per-head GEMMs may take different
        # BLAS kernels, whose summation order -- and so the last bits -- depend on the CPU they run on
        return float((a - b).abs().max()) <= 1e-6 * max(1.0, float(b.abs().max()))
    a, b = h(x), loop(x)
    assert close(a, b)
    a.square().sum().backward()
    b.square().sum().backward()
    for (n, p), (n2, p2) in zip(h.named_parameters(), loop.named_parameters()):
        assert n == n2 and p.grad is not None
        assert float((p.grad - p2.grad).abs().max()) <= 1e-5 * float(p2.grad.abs().max()) + 1e-12, n
    assert list(h.state_dict().keys()) == list(loop.state_dict().keys())
    o1, o2 = torch.optim.AdamW(h.parameters(), 1e-2), torch.optim.AdamW(loop.parameters(), 1e-2)
    o1.step(); o2.step()
    assert float((h(x) - loop(x)).abs().max()) < 1e-5
    assert h._flat["v"].data_ptr() == h._head_params()["v"][0].data_ptr()
    loop2 = HyperStructure(st, wn_flag=wn, linear_bias=bias)
    h.load_state_dict(loop2.state_dict())
    loop2.fuse_heads = False
    assert close(h(x), loop2(x))
    assert close(copy.deepcopy(h)(x), loop2(x))
    h.double()                                       # re-allocates the parameters: the flat buffers are rebuilt
    assert h(x.double()).dtype == torch.float64 and h._flat["v"].dtype == torch.float64


@pytest.mark.parametrize("fixed", [False, True])
def test_one_host_draw_equals_the_per_block_gumbel_draws(fixed):
    """estimation_utils.sample_gumbel_blocks vs the reference's order of draws (quantizer.py:196-213: depth block, then one
    torch.rand per width segment on the host generator): identical values AND the generator ends in the same state."""
    from diffusion_pruning_amd.estimation_utils import sample_gumbel, sample_gumbel_blocks
    widths = [14, 320, 320, 5, 1280, 17, 1]
    for B in (1, 4):
        torch.manual_seed(77)
        ref = torch.cat([sample_gumbel((B, w), fixed_seed=fixed) for w in widths], dim=1)
        after_ref = torch.rand(3)
        torch.manual_seed(77)
        got = sample_gumbel_blocks(B, widths, fixed_seed=fixed)
        after_got = torch.rand(3)
        assert torch.equal(ref, got)
        assert torch.equal(after_ref, after_got)


def test_scratch_domain_is_thread_local_and_restores():
    """ops.scratch_domain: the key under which split-K counters / scratch are looked up (graphs that replay concurrently are
    captured under different domains); nesting restores the outer name, other threads are not affected"""
    import threading
    from diffusion_pruning_amd import ops
    assert ops._domain() is None
    seen = {}
    with ops.scratch_domain("teacher"):
        assert ops._domain() == "teacher"
        t = threading.Thread(target=lambda: seen.setdefault("other", ops._domain()))
        t.start(); t.join()
        with ops.scratch_domain("inner"):
            assert ops._domain() == "inner"
        assert ops._domain() == "teacher"
    assert ops._domain() is None and seen["other"] is None


def test_single_arch_param_baseline_repeats_one_code_over_the_batch():
    """trainer.py:1134-1136: with ``HyperStructure(single_arch_param=True)`` the one learned architecture vector is repeated over
    the batch AFTER the Gumbel-sigmoid relaxation (every sample sees the same noise draw), kept as ``hyper_net.arch_gs``, and
    its gradient reaches the single parameter"""
    from diffusion_pruning_amd.hypernet import HyperStructure
    from diffusion_pruning_amd.quantizer import StructureVectorQuantizer
    from diffusion_pruning_amd.train_step import PrunerStep, synthetic_batch
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    from tests.test_distributed_cpu import DEPTH_ORDER, StubUNet
    cfg = O.TINY
    real = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                     cross_attention_dim=cfg.cross_attention_dim)
    torch.manual_seed(1)
    hn = HyperStructure(structure=real.get_structure(), input_dim=16, single_arch_param=True)
    qz = StructureVectorQuantizer(n_e=4, structure=real.get_structure(), temperature=0.4, base=3, depth_order=DEPTH_ORDER,
                                  resource_aware_normalization=False, optimal_transport=False)
    step = PrunerStep(StubUNet(real), hn, qz)
    hn.train(); qz.train()
    step.count_macs(8)
    batch = synthetic_batch(3, 8, "cpu", seed=5, cross_dim=cfg.cross_attention_dim, text_dim=16)
    torch.manual_seed(3)
    out = step.step(batch["noisy_latents"], batch["timesteps"], batch["encoder_hidden_states"], batch["mpnet_embeddings"],
                    batch["target"], pretrain=True)
    E = sum(hn.width_list) + sum(hn.depth_list)
    assert hn.arch_gs.shape == (3, E) and torch.equal(hn.arch_gs[0], hn.arch_gs[1]) and torch.equal(hn.arch_gs[0], hn.arch_gs[2])
    out["loss"].backward()
    assert hn.arch.grad is not None and float(hn.arch.grad.abs().sum()) > 0 and torch.isfinite(out["loss"])
