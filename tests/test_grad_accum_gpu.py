"""GPU checks of gradient accumulation and learning-rate warm-up in the graphed expert fine-tune step
(train_step.GraphedFineTunerStep(accumulation_steps=N, lr_warmup_steps=W); csrc/optim.hip: aptp_grad_accumulate and the
warm-up inside the one-launch AdamW).  Tiny expert (O.TINY), 16x16 latents, micro-batches of 2."""
from types import SimpleNamespace

import pytest
import torch

from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
from tests.margins import check  # noqa: E402

KW = dict(lr=1e-3, weight_decay=1e-2)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def build(cuda, mask):
    from diffusion_pruning_amd.unet import UNet2DConditionModelPruned
    cfg = O.TINY
    pm = UNet2DConditionModelPruned(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                    cross_attention_dim=cfg.cross_attention_dim).init_synthetic(seed=0)
    params = {k: v.detach().clone().requires_grad_() for k, v in pm.state_dict().items()}
    pm.to(cuda)
    pm.prune({k: [v.clone().to(cuda) for v in vs] for k, vs in mask.items()})
    return cfg, pm, params


def _two_students(cuda, mask):
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    cfg, a, params = build(cuda, mask)
    _, b, _ = build(cuda, mask)
    teacher = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                        cross_attention_dim=cfg.cross_attention_dim)
    teacher.load_state_dict({k: v.detach() for k, v in params.items()})
    teacher.to(cuda).freeze()
    teacher.set_structure({k: [v.to(cuda) for v in vs] for k, vs in O.ones_mask(cfg).items()})
    return cfg, a, b, teacher


def _setup(cuda, seeds=(4, 5, 6, 7, 8, 9)):
    from diffusion_pruning_amd.train_step import synthetic_batch
    mask = O.random_mask(O.TINY, 0.6, 9, n_depth_off=1)
    cfg, sa, sb, teacher = _two_students(cuda, mask)
    batches = [synthetic_batch(2, 16, cuda, seed=s, cross_dim=cfg.cross_attention_dim) for s in seeds]
    return sa, sb, teacher, batches


def _state(step):
    return ([p.detach().clone() for p in step.trainer.parameters()], [m.clone() for m in step.optimizer.m],
            [v.clone() for v in step.optimizer.v], float(step.optimizer.step_t))


def _state_equal(step, snap):
    ps, ms, vs, t = snap
    return (all(torch.equal(p.detach(), s) for p, s in zip(step.trainer.parameters(), ps))
            and all(torch.equal(m, s) for m, s in zip(step.optimizer.m, ms))
            and all(torch.equal(v, s) for v, s in zip(step.optimizer.v, vs)) and float(step.optimizer.step_t) == t)


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
GUARD = 8            # elements on either side of a carved range: a multiple of 4, so the range stays 16-byte aligned


def _carve(n, seed, cuda):
    buf = torch.randn(n + 2 * GUARD, generator=torch.Generator().manual_seed(seed)).to(cuda)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD:GUARD + n]


def _same(a, b):
    """equal element by element, a NaN matching a NaN"""
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


@pytest.mark.parametrize("n", [1, 3, 64, 4095, 4096, 4097, 2 * 4096 + 5])
def test_grad_accumulate_kernel(cuda, n):
    from diffusion_pruning_amd import ops
    for special in (False, True):
        for mode in ("store", "add", "final"):
            abuf, acc = _carve(n, 1, cuda)
            gbuf, g = _carve(n, 2, cuda)
            if special:                                  # non-finite values come through in place
                g[0] = float("nan")
                g[n // 2] = float("inf") if n > 1 else float("nan")
                if n > 2:
                    g[n - 1] = float("-inf")
            a0, g0 = abuf.clone(), gbuf.clone()
            want = g0[GUARD:GUARD + n] if mode == "store" else a0[GUARD:GUARD + n] + g0[GUARD:GUARD + n]
            ops.grad_accumulate(acc, g, mode)
            torch.cuda.synchronize()
            dst, dst0, src, src0 = (gbuf, g0, abuf, a0) if mode == "final" else (abuf, a0, gbuf, g0)
            if special:
                assert _same(dst[GUARD:GUARD + n], want), (n, mode)
                assert bool(dst[GUARD:GUARD + n].isnan()[0]) and (n <= 2 or float(dst[GUARD + n - 1]) == float("-inf"))
                assert _same(src, src0)
            else:
                assert torch.equal(dst[GUARD:GUARD + n], want), (n, mode)
                assert torch.equal(src, src0), (n, mode)                                    # the source, its guards included
            assert torch.equal(dst[:GUARD], dst0[:GUARD]) and torch.equal(dst[GUARD + n:], dst0[GUARD + n:]), (n, mode)


def test_grad_accumulate_rejects_bad_arguments(cuda):
    from diffusion_pruning_amd import _lib, ops
    n = 64
    abuf, acc = _carve(n + 4, 1, cuda)
    gbuf, g = _carve(n + 4, 2, cuda)
    a0, g0 = abuf.clone(), gbuf.clone()
    with pytest.raises(_lib.AptpError, match="aligned"):
        ops.grad_accumulate(acc[1:n + 1], g[:n], "add")
    with pytest.raises(_lib.AptpError, match="aligned"):
        ops.grad_accumulate(acc[:n], g[2:n + 2], "final")
    for bad in (3, -1):
        with pytest.raises(_lib.AptpError, match="mode"):
            ops.grad_accumulate(acc[:n], g[:n], bad)
    torch.cuda.synchronize()
    assert torch.equal(abuf, a0) and torch.equal(gbuf, g0)                # nothing was launched


# ---- 2. a window equals the sum of its parts, bit for bit ----------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 3])
def test_window_is_the_sum_of_its_micro_batches(cuda, N):
    from diffusion_pruning_amd.packed_train import PackedAdamW
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    sa, sb, teacher, batches = _setup(cuda)
    A = GraphedFineTunerStep(sa, teacher, accumulation_steps=N, **KW)
    A.capture(batches[0])
    B = GraphedFineTunerStep(sb, teacher, lr=0.0, weight_decay=0.0)          # B's parameters never move
    B.capture(batches[0])
    arena, offs = A.trainer.grad_arena, A.trainer.grad_offsets
    assert A._accum is not None and A._accum.shape == arena.shape and getattr(B.trainer, "grad_arena", None) is None

    def gather(step, loss):             # B's per-parameter gradients in A's arena order, the loss in slot 0
        flat = torch.zeros_like(arena)
        flat[0] = loss
        for p, o in zip(step.trainer.parameters(), offs):
            flat[o:o + p.numel()] = p.grad.reshape(-1)
        return flat
    init_b = [p.detach().clone() for p in B.trainer.parameters()]
    gs = []
    for b in batches[:N]:
        out = B.train_step(None, b)
        torch.cuda.synchronize()
        assert out["applied"] is True and out["accum_index"] == 0
        gs.append(gather(B, out["loss"]))
    assert all(torch.equal(p.detach(), s) for p, s in zip(B.trainer.parameters(), init_b))
    init = _state(A)
    assert init[3] == 0.0
    losses = []
    for i, b in enumerate(batches[:N]):
        out = A.train_step(None, b)
        torch.cuda.synchronize()
        losses.append(out["loss"])
        assert out["accum_index"] == i and out["applied"] is (i == N - 1)
        if i < N - 1:
            assert _state_equal(A, init)                                   # parameters, moments, step count: untouched
    total = gs[0]
    for g in gs[1:]:
        total = total + g
    assert torch.equal(arena[64:], total[64:])
    lsum = losses[0]
    for x in losses[1:]:
        lsum = lsum + x
    assert torch.equal(arena[0], lsum) and torch.equal(arena[0], total[0]) and float(arena[1:64].abs().max()) == 0.0
    assert float(A.optimizer.step_t) == 1.0 and A.accum_index == 0
    # the optimizer's view: B (still at the initial values) takes one step on the summed gradients with grad_scale = 1 / N
    for p, o in zip(B.trainer.parameters(), offs):
        p.grad.copy_(total[o:o + p.numel()].view_as(p))
    fresh = PackedAdamW(B.trainer, **KW)
    fresh.step(grad_scale=1.0 / N)
    torch.cuda.synchronize()
    moved = 0
    for pa, pb, s in zip(A.trainer.parameters(), B.trainer.parameters(), init[0]):
        assert torch.equal(pa.detach(), pb.detach())
        moved += float((pa.detach() - s).abs().max()) > 0
    assert moved >= len(init[0]) // 2


# ---- 3. a window against one large batch ---------------------------------------------------------------------------------------
def test_window_against_one_large_batch(cuda):
    """two micro-batches of 2 against one captured step on their concatenation (B = 4): arena / 2 vs the large batch's
    gradient, per packed tensor and over all of them.  Cap 0.12 = the triangle bound of two bf16-pipeline gradients the
    project budgets at 6e-2 each against the fp32 oracle (test_parameter_gradients_match_oracle); the measured values are
    kept by tests.margins."""
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    sa, sb, teacher, batches = _setup(cuda, seeds=(4, 5))
    A = GraphedFineTunerStep(sa, teacher, accumulation_steps=2, **KW)
    A.capture(batches[0])
    big = {k: torch.cat([batches[0][k], batches[1][k]], 0) for k in batches[0]}
    C = GraphedFineTunerStep(sb, teacher, lr=0.0, weight_decay=0.0)
    C.capture(big)
    C.train_step(None, big)
    for b in batches:
        A.train_step(None, b)
    torch.cuda.synchronize()
    names = [n for n, _ in A.trainer.named_parameters()]
    errs, got_all, ref_all = {}, [], []
    for name, pa, pc in zip(names, A.trainer.parameters(), C.trainer.parameters()):
        got, ref = pa.grad.detach().flatten() / 2, pc.grad.detach().flatten()
        assert torch.isfinite(got).all() and got.shape == ref.shape, name
        errs[name] = rel_l2(got, ref)
        got_all.append(got)
        ref_all.append(ref)
    e_all = rel_l2(torch.cat(got_all), torch.cat(ref_all))
    worst = sorted(errs.items(), key=lambda kv: -kv[1])
    print("window vs large batch: all tensors %.3e; worst %s" % (e_all, [(n, "%.3e" % e) for n, e in worst[:5]]))
    check(e_all, 0.12, "window of 2 x 2 vs one batch of 4: all packed gradients")
    check(worst[0][1], 0.12, "window of 2 x 2 vs one batch of 4: worst packed tensor " + worst[0][0])


# ---- 4. a NaN in any micro-batch skips the window ------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [0, 1])
def test_nan_in_a_micro_batch_skips_the_window(cuda, where):
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    sa, sb, teacher, batches = _setup(cuda)
    A = GraphedFineTunerStep(sa, teacher, accumulation_steps=2, **KW)
    A.capture(batches[0])
    for b in batches[0:2]:
        A.train_step(None, b)
    torch.cuda.synchronize()
    snap = _state(A)
    assert snap[3] == 1.0
    window = [{k: v.clone() for k, v in b.items()} for b in batches[2:4]]
    window[where]["target"][0, 0, 0, 0] = float("nan")
    outs = [A.train_step(None, b) for b in window]
    torch.cuda.synchronize()
    assert outs[1]["applied"] is True and not torch.isfinite(outs[where]["loss"]) and torch.isfinite(outs[1 - where]["loss"])
    assert _state_equal(A, snap)
    for b in batches[4:6]:
        out = A.train_step(None, b)
    torch.cuda.synchronize()
    assert torch.isfinite(out["loss"]) and float(A.optimizer.step_t) == 2.0
    assert all(torch.isfinite(p).all() for p in A.trainer.parameters())
    moved = sum(float((p.detach() - s).abs().max()) > 0 for p, s in zip(A.trainer.parameters(), snap[0]))
    assert moved >= len(snap[0]) // 2


# ---- 5. warm-up ----------------------------------------------------------------------------------------------------------------
SHAPES = [(64, 9, 72), (8, 1, 8), (1283,), (5,), (4096 * 3 + 7,)]


def _toy_trainer(cuda):
    ps = [torch.nn.Parameter(torch.randn(*s, generator=torch.Generator().manual_seed(11 + i)).to(cuda)) for i, s in enumerate(SHAPES)]
    sh = [torch.zeros(s, dtype=torch.bfloat16, device=cuda) for s in SHAPES[:2]]
    gemms = {0: SimpleNamespace(P=ps[0], Pb=ps[2], pw=SimpleNamespace(w=sh[0])), 1: SimpleNamespace(P=ps[1], Pb=None, pw=SimpleNamespace(w=sh[1]))}
    tr = SimpleNamespace(gemms=gemms, affines={0: SimpleNamespace(Pg=ps[3], Pb=ps[4])}, refresh_=lambda shadows_done=False: None)
    for p in ps:
        p.grad = torch.zeros_like(p)
    return ps, sh, tr


def test_warmup_matches_torch_lambda_lr(cuda):
    from diffusion_pruning_amd.packed_train import PackedAdamW
    W = 4
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    grads = [torch.randn(*s, generator=torch.Generator().manual_seed(40 + i)).to(cuda) for i, s in enumerate(SHAPES)]
    ps, sh, tr = _toy_trainer(cuda)
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for p, r, g in zip(ps, ref, grads):
        p.grad.copy_(g)
        r.grad = g.clone()
    opt = PackedAdamW(tr, warmup_steps=W, **kw)
    topt = torch.optim.AdamW(ref, **kw)
    sched = torch.optim.lr_scheduler.LambdaLR(topt, lambda k: float(k) / float(max(1.0, W)) if k < W else 1.0)
    before = [p.detach().clone() for p in ps]
    for it in range(6):
        opt.step()
        topt.step()
        sched.step()
        if it == 0:                      # rate 0: the decay factor is 1 and the update 0 (the moments do start)
            assert all(torch.equal(p.detach(), b) for p, b in zip(ps, before))
            assert any(float(m.abs().max()) > 0 for m in opt.m)
        for p, r in zip(ps, ref):
            assert float((p.detach() - r.detach()).abs().max()) <= 1e-6 * float(r.detach().abs().max()) + 1e-7, it
    assert float(opt.step_t) == 6.0 and any(float((p.detach() - b).abs().max()) > 0 for p, b in zip(ps, before))
    assert torch.equal(sh[0], ps[0].detach().to(torch.bfloat16))
    # a skipped (gated) step does not advance the ramp
    t0 = float(opt.step_t)
    opt.step(gate=torch.tensor(float("nan"), device=cuda))
    assert float(opt.step_t) == t0


def test_warmup_zero_is_the_optimizer_without_it(cuda):
    from diffusion_pruning_amd.packed_train import PackedAdamW
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    grads = [torch.randn(*s, generator=torch.Generator().manual_seed(40 + i)).to(cuda) for i, s in enumerate(SHAPES)]
    ps0, sh0, tr0 = _toy_trainer(cuda)
    ps1, sh1, tr1 = _toy_trainer(cuda)
    o0, o1 = PackedAdamW(tr0, **kw), PackedAdamW(tr1, warmup_steps=0, **kw)
    for it in range(3):
        for ps in (ps0, ps1):
            for p, g in zip(ps, grads):
                p.grad.copy_(g * (it + 1))
        o0.step()
        o1.step()
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(ps0, ps1))
    assert all(torch.equal(a, b) for a, b in zip(o0.m + o0.v + sh0, o1.m + o1.v + sh1))


# ---- 6. the data-parallel schedule on one rank ---------------------------------------------------------------------------------
def test_accumulating_data_parallel_schedule_on_one_rank(cuda):
    import os
    import socket
    import torch.distributed as dist
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    sa, sb, teacher, batches = _setup(cuda, seeds=(4, 5, 6, 7))
    plain = GraphedFineTunerStep(sa, teacher, accumulation_steps=2, **KW)
    plain.capture(batches[0])
    la = [float(plain.train_step(None, b)["loss"]) for b in batches]
    torch.cuda.synchronize()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(port)
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=cuda)
    try:
        dp = GraphedFineTunerStep(sb, teacher, data_parallel=True, bucket_bytes=1 << 20, accumulation_steps=2, **KW)
        dp.capture(batches[0])
        outs = [dp.train_step(None, b) for b in batches]
        lb = [float(o["loss"]) for o in outs]
        torch.cuda.synchronize()
        red = dp.reducer
        assert [o["applied"] for o in outs] == [False, True, False, True]
        assert len(red.buckets) >= 2 and red.stats["steps"] == 2
        assert red.stats["collectives"] == 2 * len(red.buckets) * 2 and red.stats["tensor_ops"] == 0
    finally:
        if created:
            dist.destroy_process_group()
    assert la == lb, (la, lb)
    assert float(dp.optimizer.step_t) == 2.0 and float(plain.optimizer.step_t) == 2.0
    for pa, pb in zip(plain.trainer.parameters(), dp.trainer.parameters()):
        assert torch.equal(pa.detach(), pb.detach())


# ---- 7. the defaults take none of the new paths --------------------------------------------------------------------------------
def test_defaults_are_untouched(cuda):
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    sa, sb, teacher, batches = _setup(cuda, seeds=(4, 5))
    step = GraphedFineTunerStep(sa, teacher, **KW)
    assert step.accumulation_steps == 1 and step.lr_warmup_steps == 0
    step.capture(batches[0])
    assert step._accum is None and step.optimizer.warmup_steps == 0
    assert getattr(step.trainer, "grad_arena", None) is None              # per-parameter gradient buffers, no arena
    ptrs = sorted((p.grad.data_ptr(), p.numel()) for p in step.trainer.parameters())
    for b in batches:
        out = step.train_step(None, b)
        assert out["applied"] is True and out["accum_index"] == 0
        assert set(out) == {"loss", "diff_loss", "distillation_loss", "block_loss", "applied", "accum_index"}
    torch.cuda.synchronize()
    assert float(step.optimizer.step_t) == 2.0 and step._accum is None
    assert ptrs == sorted((p.grad.data_ptr(), p.numel()) for p in step.trainer.parameters())
