"""GPU checks of gradient-norm clipping on the device (csrc/grad_norm.hip, ops.GradNorm, PackedAdamW / RouterAdamW /
GraphedFineTunerStep(max_grad_norm=...)): the kernel against its numpy model bit for bit, its range and its refusals, and the
three users against torch and against themselves without the clip."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import grad_norm_model as M

pytestmark = pytest.mark.gpu
from tests.test_grad_accum_gpu import KW, SHAPES, _setup, _toy_trainer  # noqa: E402
from tests.test_router_optim_gpu import batch_of, router_bits, toy, world  # noqa: E402,F401  (world: a fixture)


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32).tolist()


def on_device(items, cuda):
    return [torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).to(cuda) for g in items]


def run_kernel(items, cuda, grad_scale=1.0, max_norm=None, gate=None, clipped_before=0.0):
    from diffusion_pruning_amd import ops
    gn = ops.GradNorm(on_device(items, cuda), cuda, max_norm=max_norm)
    gn.clipped.fill_(clipped_before)
    g = None if gate is None else torch.tensor([gate], dtype=torch.float32, device=cuda)
    out = gn.run(grad_scale, g)
    torch.cuda.synchronize()
    return out.cpu().numpy(), gn


# ---- 1. the kernel against the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.tables()))
def test_kernel_against_the_model(cuda, name):
    sizes = M.tables()[name]
    items = M.items_of(sizes, seed=len(sizes) + sizes[0])
    ref = M.reference_norm(items)
    # measure only; a threshold below the norm with a scale; a threshold above it
    for kw in (dict(), dict(grad_scale=0.25, max_norm=float(ref) * 0.25 / 3.0, clipped_before=4.0), dict(max_norm=float(ref) * 2.0)):
        got, gn = run_kernel(items, cuda, **kw)
        want = M.grad_norm(items, **kw)
        print(name, kw, got.tolist(), want.tolist())
        assert gn.table.total == sum(M.blocks_of(n) for n in sizes)
        assert bits(got) == bits(want), (name, kw, got, want)
    got, _ = run_kernel(items, cuda)
    assert M.ulps(got[0], ref) <= 1, (got[0], ref)      # fp64 accumulation: < 1e-9 relative over <= 2e6 terms, then one rounding
    assert got[1] == 1.0 and got[2] == got[0] and got[3] == 0.0
    got, _ = run_kernel(items, cuda, grad_scale=0.25, max_norm=float(ref) * 0.25 / 3.0, clipped_before=4.0)
    assert abs(float(got[1]) - 1.0 / 3.0) <= 1e-5 and got[3] == 5.0


def test_replays_give_the_same_bits(cuda):
    from diffusion_pruning_amd import ops
    items = M.items_of(M.tables()["all"] + M.tables()["300_tiny"], seed=9)
    gn = ops.GradNorm(on_device(items, cuda), cuda, max_norm=1.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gn.run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gn.run()
    seen = set()
    for _ in range(5):
        graph.replay()
        torch.cuda.synchronize()
        seen.add(tuple(bits(gn.out[:3].cpu().numpy())))
    assert len(seen) == 1 and list(seen)[0] == tuple(bits(M.grad_norm(items, max_norm=1.0)[:3]))
    assert float(gn.clipped) == 6.0


# ---- 2. range ----------------------------------------------------------------------------------------------------------------------
def test_range(cuda):
    big = [np.full(5000, 1e30, dtype=np.float32), np.full(7, 1e-30, dtype=np.float32)]      # an fp32 accumulator: inf
    got, _ = run_kernel(big, cuda)
    assert np.isfinite(got[0]) and got[0] > 0 and M.ulps(got[0], M.reference_norm(big)) <= 1 and bits(got) == bits(M.grad_norm(big))
    small = [np.full(3, 1e-30, dtype=np.float32), np.full(4097, -1e-30, dtype=np.float32)]    # an fp32 accumulator: 0
    got, _ = run_kernel(small, cuda)
    assert np.isfinite(got[0]) and got[0] > 0 and M.ulps(got[0], M.reference_norm(small)) <= 1 and bits(got) == bits(M.grad_norm(small))
    got, _ = run_kernel([np.zeros(4097, dtype=np.float32), np.zeros(3, dtype=np.float32)], cuda, max_norm=1.0)
    assert got.tolist() == [0.0, 1.0, 0.0, 0.0]


# ---- 3. non-finite -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["grad_nan", "grad_inf", "gate_nan", "gate_inf"])
def test_non_finite(cuda, how):
    items = M.items_of([5, 4097, 2 * 4096 + 5], seed=3)
    gate = 0.5
    if how == "grad_nan":
        items[2][4096 + 77] = np.nan
    elif how == "grad_inf":
        items[0][4] = np.inf
    else:
        gate = float("nan") if how == "gate_nan" else float("inf")
    got, _ = run_kernel(items, cuda, max_norm=0.1, gate=gate, clipped_before=2.0)
    want = M.grad_norm(items, max_norm=0.1, gate=gate, clipped_before=2.0)
    assert not np.isfinite(got[2]) and got[1] == 1.0 and got[3] == 2.0, got
    assert bits(got[1:]) == bits(want[1:])
    if how.startswith("gate"):
        assert bits(got) == bits(want) and np.isfinite(got[0])
    else:
        assert not np.isfinite(got[0])
    # and the same table is fine again with a finite gate and gradients
    got, _ = run_kernel(M.items_of([5, 4097, 2 * 4096 + 5], seed=3), cuda, max_norm=0.1, gate=0.5, clipped_before=2.0)
    assert np.isfinite(got[2]) and got[1] < 1.0 and got[3] == 3.0


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(cuda):
    from diffusion_pruning_amd import _lib, ops
    lib = _lib.load()
    gn = ops.GradNorm(on_device(M.items_of([5, 4097], seed=1), cuda), cuda)
    gn.out.copy_(torch.tensor([7.0, 8.0, 9.0, 10.0]))
    gn.partials.fill_(-3.0)
    wide = torch.zeros(8, dtype=torch.float32, device=cuda)
    before = (gn.out.clone(), gn.partials.clone())

    def params():
        q = _lib.GradNormParams()
        q.items_dev, q.starts_dev, q.n_items, q.total_blocks = gn.table.args()
        q.partials_dev, q.grad_scale, q.out_dev, q.max_norm_dev = gn.partials.data_ptr(), 1.0, gn.out.data_ptr(), gn.max_norm_dev.data_ptr()
        return q

    def refused(**kw):
        q = params()
        for k, v in kw.items():
            setattr(q, k, v)
        assert lib.aptp_grad_norm(ctypes.byref(q), ops._stream()) == -1, kw
        assert b"grad_norm" in lib.aptp_last_error()
    for name in ("items_dev", "starts_dev", "partials_dev", "out_dev"):
        refused(**{name: None})
    assert lib.aptp_grad_norm(None, None) == -1
    refused(n_items=0)
    refused(total_blocks=0)
    refused(grad_scale=-1.0)
    refused(out_dev=gn.out.data_ptr() + 4)
    refused(out_dev=wide.data_ptr() + 8)
    refused(partials_dev=gn.partials.data_ptr() + 4)
    torch.cuda.synchronize()
    assert torch.equal(gn.out, before[0]) and torch.equal(gn.partials, before[1]) and not wide.any()
    q = params()
    assert lib.aptp_grad_norm(ctypes.byref(q), ops._stream()) == 0            # and the untouched arguments are fine
    torch.cuda.synchronize()
    assert float(gn.out[0]) > 0 and float(gn.out[3]) == 10.0 and float(gn.partials.min()) >= 0.0


# ---- 5. PackedAdamW ----------------------------------------------------------------------------------------------------------------
OPT = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


def _grads(cuda, k):
    return [torch.randn(*s, generator=torch.Generator().manual_seed(40 + 7 * k + i)).to(cuda) for i, s in enumerate(SHAPES)]


def _set(ps, grads):
    for p, g in zip(ps, grads):
        p.grad.copy_(g)


def _opt_bits(ps, opt, sh):
    return [p.detach() for p in ps] + list(opt.m) + list(opt.v) + list(sh)


def test_packed_adamw_clips_as_torch_does(cuda):
    from diffusion_pruning_amd.packed_train import PackedAdamW
    scale = 0.5
    g0 = _grads(cuda, 0)
    norm0 = float(M.reference_norm([g.cpu().numpy() for g in g0], scale))
    max_norm = norm0 / 3.0
    ps, sh, tr = _toy_trainer(cuda)
    qs, sh2, tr2 = _toy_trainer(cuda)
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt, twin = PackedAdamW(tr, max_grad_norm=max_norm, **OPT), PackedAdamW(tr2, **OPT)
    topt = torch.optim.AdamW(ref, **OPT)
    for k in range(2):
        gs = _grads(cuda, k)
        _set(ps, gs)
        _set(qs, gs)
        for r, g in zip(ref, gs):
            r.grad = g * scale
        gate = opt.step(grad_scale=scale)
        coef = np.float32(float(opt.grad_norm.coef))
        assert gate is opt.grad_norm.verdict and coef < 1.0
        want = M.grad_norm([g.cpu().numpy() for g in opt.grads], grad_scale=scale, max_norm=max_norm, clipped_before=float(k))
        assert bits(opt.grad_norm.out.cpu().numpy()) == bits(want)
        twin.step(grad_scale=float(np.float32(scale) * coef))
        assert all(torch.equal(a, b) for a, b in zip(_opt_bits(ps, opt, sh), _opt_bits(qs, twin, sh2))), k
        torch.nn.utils.clip_grad_norm_(ref, max_norm)
        topt.step()
        for p, r in zip(ps, ref):
            err, size = float((p.detach() - r.detach()).abs().max()), float(r.detach().abs().max())
            print("step", k, "max |p - torch| / max |torch|", err / size)
            assert err <= 1e-6 * size, (k, err, size)
    assert float(opt.step_t) == 2.0 and opt.clipped_steps() == 2
    assert M.ulps(opt.last_grad_norm(), M.reference_norm([g.cpu().numpy() for g in _grads(cuda, 1)], scale)) <= 1
    assert torch.equal(sh[0], ps[0].detach().to(torch.bfloat16))
    opt.set_max_grad_norm(None)                   # measure only: the unclipped step from here on
    _set(ps, g0)
    _set(qs, g0)
    opt.step(grad_scale=scale)
    twin.step(grad_scale=scale)
    assert all(torch.equal(a, b) for a, b in zip(_opt_bits(ps, opt, sh), _opt_bits(qs, twin, sh2))) and opt.clipped_steps() == 2


def test_packed_adamw_above_the_norm_is_the_unclipped_optimizer(cuda):
    from diffusion_pruning_amd.packed_train import PackedAdamW
    ps, sh, tr = _toy_trainer(cuda)
    qs, sh2, tr2 = _toy_trainer(cuda)
    norm0 = float(M.reference_norm([g.cpu().numpy() for g in _grads(cuda, 0)]))
    opt, plain = PackedAdamW(tr, max_grad_norm=4.0 * norm0, warmup_steps=2, **OPT), PackedAdamW(tr2, warmup_steps=2, **OPT)
    assert plain.grad_norm is None
    loss = torch.tensor([0.25], device=cuda)
    for k in range(3):
        gs = _grads(cuda, k)
        _set(ps, gs)
        _set(qs, gs)
        opt.step(gate=loss, grad_scale=0.5)
        plain.step(gate=loss, grad_scale=0.5)
    assert all(torch.equal(a, b) for a, b in zip(_opt_bits(ps, opt, sh), _opt_bits(qs, plain, sh2)))
    assert float(opt.step_t) == float(plain.step_t) == 3.0 and opt.clipped_steps() == 0 and float(opt.grad_norm.coef) == 1.0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_packed_adamw_skips_a_non_finite_gradient(cuda, bad):
    from diffusion_pruning_amd.packed_train import PackedAdamW, PackedEMA
    ps, sh, tr = _toy_trainer(cuda)
    tr.named_parameters = lambda: [(f"t{i}", p) for i, p in enumerate(ps)]
    opt = PackedAdamW(tr, max_grad_norm=1.0, **OPT)
    ema = PackedEMA(tr, opt, decay=0.5)
    loss = torch.tensor([0.25], device=cuda)
    _set(ps, _grads(cuda, 0))
    ema.step(opt.step(gate=loss))
    assert float(opt.step_t) == 1.0 and ema.steps() == 1 and opt.clipped_steps() == 1
    before = [t.clone() for t in _opt_bits(ps, opt, sh) + ema.ema]
    gs = _grads(cuda, 1)
    gs[4][4096 + 3] = bad                         # one element, a finite loss
    _set(ps, gs)
    gate = opt.step(gate=loss)
    ema.step(gate)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(gate)) and float(opt.grad_norm.coef) == 1.0
    assert all(torch.equal(a, b) for a, b in zip(_opt_bits(ps, opt, sh) + ema.ema, before))
    assert float(opt.step_t) == 1.0 and ema.steps() == 1 and opt.clipped_steps() == 1
    _set(ps, _grads(cuda, 1))
    ema.step(opt.step(gate=loss))
    assert float(opt.step_t) == 2.0 and ema.steps() == 2 and not torch.equal(ps[0].detach(), before[0])
    # a non-finite loss with finite gradients skips as it always did
    ema.step(opt.step(gate=torch.tensor([bad], device=cuda)))
    assert float(opt.step_t) == 2.0 and ema.steps() == 2


# ---- 6. RouterAdamW ----------------------------------------------------------------------------------------------------------------
def _router_toy(cuda, **kw):
    """the tensors of test_router_optim_gpu.toy as ranges of ONE buffer, 64 elements apart at least: the optimizer orders its items by
    address, and the order of the items is the order of the norm's sum"""
    from diffusion_pruning_amd.router_optim import RouterAdamW
    shapes, g, loose = toy(cuda)
    offs, total = [], 0
    for sh in shapes:
        offs.append(total)
        total += (int(np.prod(sh)) + 64 + 63) // 64 * 64
    buf = torch.zeros(total, device=cuda)
    ps = []
    for sh, o, p0 in zip(shapes, offs, loose):
        view = buf[o:o + p0.numel()].view(sh)
        view.copy_(p0.detach())
        ps.append(torch.nn.Parameter(view))
    opt = RouterAdamW([{"params": ps[:2], "lr": 1e-3, "weight_decay": 1e-2}, {"params": ps[2:], "lr": 3e-3, "weight_decay": 0.1}], **kw)
    src = [torch.randn(*s, generator=g).to(cuda) for s in shapes]
    return ps, opt, src


def test_router_adamw_captured_equals_eager_with_the_clip(cuda):
    ps, opt, src = _router_toy(cuda, max_grad_norm=1.0, warmup_steps=2)
    qs, eager, _ = _router_toy(cuda, max_grad_norm=1.0, warmup_steps=2)
    plain_ps, plain, _ = _router_toy(cuda, warmup_steps=2)
    n0 = float(M.reference_norm([s.cpu().numpy() for s in src], 0.5))
    loss = torch.tensor([0.25], device=cuda)

    def body(o, params):
        for p, s0 in zip(params, src):
            p.grad.add_(s0)
        o.step(gate=loss, grad_scale=0.5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        snap = opt._snapshot()
        body(opt, ps)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    opt._restore(snap)
    assert opt.clipped_steps() == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body(opt, ps)
    coefs = []
    for thr in (n0 / 2.0, n0 / 2.0, 4.0 * n0, n0 / 8.0):       # (the threshold changes between replays: no recapture)
        opt.set_max_grad_norm(thr)
        eager.set_max_grad_norm(thr)
        graph.replay()
        body(eager, qs)
        body(plain, plain_ps)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(router_bits(opt), router_bits(eager)))
        assert torch.equal(opt.grad_norm.out, eager.grad_norm.out)
        assert M.ulps(opt.last_grad_norm(), n0) <= 1
        coefs.append(float(opt.grad_norm.coef))
    assert abs(coefs[0] - 0.5) < 1e-5 and coefs[1] == coefs[0] and coefs[2] == 1.0 and abs(coefs[3] - 0.125) < 1e-5
    assert opt.clipped_steps() == 3 and opt.applied_steps() == 4 and all(not p.grad.any() for p in ps)
    assert not torch.equal(ps[3].detach(), plain_ps[3].detach())          # the clip took effect
    assert set(opt.state_dict()) == set(plain.state_dict())               # no state beyond the counter


def make_clip(world, **kw):
    from diffusion_pruning_amd.router_optim import RouterAdamW
    from diffusion_pruning_amd.train_step import GraphedPrunerStep
    cfg, unet, hn0, qz0 = world
    hn, qz = copy.deepcopy(hn0), copy.deepcopy(qz0)
    step = GraphedPrunerStep(unet, hn, qz)
    step.count_macs(16)
    opt = RouterAdamW([{"params": [p for p in hn.parameters() if p.requires_grad], "lr": 1e-3, "weight_decay": 0.0},
                       {"params": [p for p in qz.parameters() if p.requires_grad], "lr": 1e-3, "weight_decay": 0.1}], **kw)
    return step, opt, hn, qz


def test_pruning_step_pretraining_reports_the_hyper_net_norm(cuda, world):  # noqa: F811
    cfg = world[0]
    step, opt, hn, qz = make_clip(world, max_grad_norm=1e9)
    torch.manual_seed(5)
    step.capture(batch_of(cfg, cuda, 3))                                   # the U-Net graphs; the router runs eagerly
    seen = []
    real = opt.step

    def recording_step(table=None, gate=None, grad_scale=1.0):
        seen.append(([opt.grads[i].detach().clone() for i in opt.table_keys[table]], [g.clone() for g in opt.grads]))
        return real(table=table, gate=gate, grad_scale=grad_scale)
    opt.step = recording_step
    code = qz.embedding.weight
    ci = [i for i, p in enumerate(opt.params) if p is code][0]
    hi = [i for i, p in enumerate(opt.params) if any(p is h for h in hn.parameters())]
    for s in (3, 4):
        out = step.train_step(opt, batch_of(cfg, cuda, s), pretrain=True)
        torch.cuda.synchronize()
        in_table, every = seen[-1]
        assert not every[ci].any()                                         # the codebook got no gradient
        want = np.float32(np.sqrt(sum(float(every[i].double().pow(2).sum()) for i in hi)))
        assert want > 0 and M.ulps(float(out["grad_norm"]), want) <= 1, (float(out["grad_norm"]), want)
        assert M.ulps(float(out["grad_norm"]), np.float32(np.sqrt(sum(float(g.double().pow(2).sum()) for g in in_table)))) <= 1
    assert opt.clipped_steps() == 0 and opt.applied_steps() == 2
    step.remove_hooks()


def test_pruning_step_captured_with_the_clip(cuda, world):  # noqa: F811
    cfg = world[0]
    batches = [batch_of(cfg, cuda, s) for s in (3, 4, 5, 6)]
    step, opt, hn, qz = make_clip(world, max_grad_norm=1e9, warmup_steps=2)
    torch.manual_seed(77)
    step.capture(batches[0], optimizer=opt, pretrain=True)
    step.capture_router(batches[0], pretrain=False)
    assert opt.clipped_steps() == 0 and opt.applied_steps() == 0          # the capture's warm-up steps left no trace
    norms, coefs = [], []
    for i, b in enumerate(batches):
        if i == 1 or i == 3:
            opt.set_max_grad_norm(norms[-1] / 4.0)                         # between replays, no recapture
        if i == 2:
            opt.set_max_grad_norm(1e9)
        o = step.train_step(opt, b, pretrain=i < 2)
        step.finish()
        torch.cuda.synchronize()
        assert float(o["applied"]) == 1.0
        norms.append(float(o["grad_norm"]))
        coefs.append(float(opt.grad_norm.coef))
    print("norms", norms, "coefs", coefs)
    assert all(np.isfinite(n) and n > 0 for n in norms)
    assert coefs[0] == 1.0 and coefs[1] < 1.0 and coefs[2] == 1.0 and coefs[3] < 1.0 and opt.clipped_steps() == 2
    # the same replay from the same state: the same bits
    snap, seen = opt._snapshot(), set()
    for _ in range(3):
        opt._restore(snap)
        torch.manual_seed(123)
        o = step.train_step(opt, batches[1], pretrain=False)
        step.finish()
        torch.cuda.synchronize()
        seen.add((tuple(bits(o["grad_norm"].cpu().numpy())), tuple(bits(opt.grad_norm.out.cpu().numpy())),
                  hash(torch.cat([p.detach().flatten() for p in opt.params]).cpu().numpy().tobytes())))
    assert len(seen) == 1 and opt.clipped_steps() == 3
    # a NaN batch is skipped under the clip as without it, and counts as no clip
    bad = batch_of(cfg, cuda, 4)
    bad["target"][1, 2, 3, 4] = float("nan")
    before = router_bits(opt)[:-1]
    o = step.train_step(opt, bad)
    step.finish()
    torch.cuda.synchronize()
    assert float(o["applied"]) == 0.0 and opt.clipped_steps() == 3 and float(opt.grad_norm.coef) == 1.0
    assert all(torch.equal(a, b) for a, b in zip(router_bits(opt)[:-1], before))
    step.remove_hooks()


# ---- 7. GraphedFineTunerStep --------------------------------------------------------------------------------------------------------
def _arena_norm(step, scale):
    """the norm of the gradients AdamW read, computed by torch in fp64 from the arena's views, times scale, rounded once"""
    total = sum(float(g.double().pow(2).sum()) for g in step.optimizer.grads)
    return np.float32(np.sqrt(total) * scale)


def test_finetune_step_reports_and_repeats_the_norm(cuda):
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    sa, sb, teacher, batches = _setup(cuda, seeds=(4, 5, 6, 7))
    acc = GraphedFineTunerStep(sa, teacher, accumulation_steps=2, max_grad_norm=1e-4, **KW)
    acc.capture(batches[0])
    for w in range(2):
        o0 = acc.train_step(None, batches[2 * w])
        o1 = acc.train_step(None, batches[2 * w + 1])
        torch.cuda.synchronize()
        assert o0["grad_norm"] is None and o0["applied"] is False and o1["applied"] is True
        want = _arena_norm(acc, 0.5)
        print("window", w, "grad_norm", float(o1["grad_norm"]), "torch", float(want))
        assert want > 0 and M.ulps(float(o1["grad_norm"]), want) <= 1, (float(o1["grad_norm"]), want)
    assert float(acc.optimizer.step_t) == 2.0 and acc.optimizer.clipped_steps() == 2 and acc.optimizer.last_grad_norm() == float(o1["grad_norm"])

    one = GraphedFineTunerStep(sb, teacher, max_grad_norm=1e-4, **KW)
    one.capture(batches[0])
    one.train_step(None, batches[1])                                      # (a seasoned state: non-zero moments)
    torch.cuda.synchronize()
    opt = one.optimizer
    state = [t.detach().clone() for t in one.trainer.parameters() + opt.m + opt.v] + [opt.step_t.clone()]
    seen = set()
    for _ in range(5):
        with torch.no_grad():
            for dst, src in zip(one.trainer.parameters() + opt.m + opt.v + [opt.step_t], state):
                dst.copy_(src)
            one.trainer.refresh_()
        o = one.train_step(None, batches[2])
        one.finish()
        torch.cuda.synchronize()
        seen.add((tuple(bits(o["grad_norm"].cpu().numpy())), tuple(bits(opt.grad_norm.out[:3].cpu().numpy())),
                  hash(torch.cat([p.detach().flatten() for p in one.trainer.parameters()]).cpu().numpy().tobytes())))
    assert len(seen) == 1
    assert M.ulps(float(o["grad_norm"]), _arena_norm(one, 1.0)) <= 1


def test_finetune_step_without_the_argument_is_unchanged(cuda, monkeypatch):
    from diffusion_pruning_amd import _lib
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    sa, sb, teacher, batches = _setup(cuda, seeds=(4, 5))
    lib = _lib.load()
    calls = {}
    for name, _, _ in _lib.EXPORTS:
        fn = getattr(lib, name)

        def counting(*a, _fn=fn, _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counting)
    results = []
    for student, kw in ((sa, {}), (sb, dict(max_grad_norm=None, log_grad_norm=False))):
        step = GraphedFineTunerStep(student, teacher, **KW, **kw)
        step.capture(batches[0])
        assert step.optimizer.grad_norm is None
        calls.clear()
        outs = [step.train_step(None, b) for b in batches]
        torch.cuda.synchronize()
        assert all(set(o) == {"loss", "diff_loss", "distillation_loss", "block_loss", "applied", "accum_index"} for o in outs)
        results.append((dict(calls), [[float(o[k]) for k in ("loss", "diff_loss", "distillation_loss", "block_loss")] for o in outs],
                        [p.detach().clone() for p in step.trainer.parameters()]))
    (ca, la, pa), (cb, lb, pb) = results
    assert ca == cb and "aptp_grad_norm" not in ca and ca.get("aptp_adamw_many") == 2
    assert la == lb and all(torch.equal(a, b) for a, b in zip(pa, pb))


def test_finetune_data_parallel_schedule_with_the_clip_on_one_rank(cuda):
    """with a norm the data-parallel step exchanges every bucket first, then takes the norm over the summed arena and applies
    ONE AdamW launch: on one rank, the numbers of the step without data_parallel"""
    import os
    import socket
    import torch.distributed as dist
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    sa, sb, teacher, batches = _setup(cuda, seeds=(4, 5, 6, 7))
    plain = GraphedFineTunerStep(sa, teacher, accumulation_steps=2, max_grad_norm=1e-4, **KW)
    plain.capture(batches[0])
    oa = [plain.train_step(None, b) for b in batches]
    torch.cuda.synchronize()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(port)
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=cuda)
    try:
        dp = GraphedFineTunerStep(sb, teacher, data_parallel=True, bucket_bytes=1 << 20, accumulation_steps=2, max_grad_norm=1e-4, **KW)
        dp.capture(batches[0])
        ob = [dp.train_step(None, b) for b in batches]
        torch.cuda.synchronize()
        assert len(dp.reducer.buckets) >= 2 and dp.reducer.stats["steps"] == 2
    finally:
        if created:
            dist.destroy_process_group()
    assert [o["grad_norm"] is None for o in ob] == [True, False, True, False]
    assert [float(o["grad_norm"]) for o in oa[1::2]] == [float(o["grad_norm"]) for o in ob[1::2]]
    assert float(dp.optimizer.step_t) == 2.0 and dp.optimizer.clipped_steps() == plain.optimizer.clipped_steps() == 2
    for pa, pb in zip(plain.trainer.parameters(), dp.trainer.parameters()):
        assert torch.equal(pa.detach(), pb.detach())
