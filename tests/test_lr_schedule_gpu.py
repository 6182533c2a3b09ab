"""GPU checks of the device-side learning-rate schedules: aptp_lr_schedule against tests/lr_schedule_model.py, the AdamW
entry points that read the rate from device memory against the ones that take it as a number, and the three users --
PackedAdamW(lr_schedule=), RouterAdamW(lr_schedule=) eager and inside a captured pruning step, GraphedFineTunerStep(lr_scheduler=)
-- against the same code without a schedule and a host-side rate taken from the model before every step."""
import ctypes

import numpy as np
import pytest
import torch

from tests import lr_schedule_model as M
from tests.margins import check

pytestmark = pytest.mark.gpu

BASE = (2e-4, 3e-3)        # two base rates (the recipe's 2e-4 and a larger one)
EXACT_KINDS = ("constant", "constant_with_warmup", "linear")


def f32(x):
    return float(np.float32(x))


def _sched(kind, W, T, kw):
    from diffusion_pruning_amd.packed_train import LrSchedule
    return LrSchedule(kind, warmup_steps=W, training_steps=T, **kw)


def _ulps(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """distance in fp32 units in the last place, element by element (all values here are >= 0)"""
    return (got.cpu().view(torch.int32).long() - want.cpu().view(torch.int32).long()).abs()


# ---- 1. the rate kernel ----------------------------------------------------------------------------------------------------------
def test_rate_kernel_against_the_model(cuda):
    """every (kind, W, T, k) of the CPU grid, with n = 1 (+ mult_dev) and with n = 2, out_stride = 3 into a [2, 3] table.  Bit-equal
    for constant, constant_with_warmup, every warm-up ramp and linear (only correctly rounded fp64 operations before one rounding
    to fp32); at most 1 ulp of fp32 for the cosines and polynomial past the ramp (the device's fp64 cos / pow differ from the
    host's by a few fp64 ulps, which can move one fp32 rounding by at most one)."""
    cases = [(kind, W, T, kw, k) for kind, W, T, kw in M.grid() for k in M.GRID_STEPS]
    n = len(cases)
    ks = torch.tensor([float(k) for k in M.GRID_STEPS], dtype=torch.float32).to(cuda)
    base1 = torch.tensor([f32(BASE[0])], dtype=torch.float32).to(cuda)
    base2 = torch.tensor([f32(b) for b in BASE], dtype=torch.float32).to(cuda)
    out1, mult = torch.full((n,), -1.0, device=cuda), torch.full((n,), -1.0, device=cuda)
    fill = torch.arange(n * 6, dtype=torch.float32).reshape(n, 2, 3).to(cuda) + 0.5
    tables = fill.clone()
    for i, (kind, W, T, kw, k) in enumerate(cases):
        s = _sched(kind, W, T, kw)
        s.launch(ks[k:k + 1], base1, out1[i:i + 1], mult=mult[i:i + 1])
        s.launch(ks[k:k + 1], base2, tables[i].reshape(-1), out_stride=3)
    torch.cuda.synchronize()
    want1 = torch.tensor(np.array([M.rate(kind, BASE[0], k, W, T, **kw) for kind, W, T, kw, k in cases], dtype=np.float32))
    want2 = torch.tensor(np.array([[M.rate(kind, b, k, W, T, **kw) for b in BASE] for kind, W, T, kw, k in cases], dtype=np.float32))
    wantm = torch.tensor(np.array([np.float32(M.multiplier(kind, k, W, T, **kw)) for kind, W, T, kw, k in cases], dtype=np.float32))
    exact = torch.tensor([kind in EXACT_KINDS or k < W for kind, W, T, kw, k in cases])
    assert torch.equal(tables[:, :, 1:], fill[:, :, 1:]), "the other columns of the group table keep their bits"
    d1, d2, dm = _ulps(out1, want1), _ulps(tables[:, :, 0], want2).amax(1), _ulps(mult, wantm)
    for what, d in (("rate, n = 1", d1), ("rate, n = 2 stride 3", d2), ("multiplier", dm)):
        off = [(cases[i], int(d[i])) for i in torch.nonzero(d * exact).flatten().tolist()[:3]]
        print(f"{what}: largest distance {int(d.max())} ulp; cases that must be bit-equal and are not: {off}")
        assert not off, (what, off)
        check(float(d[~exact].max()), 1.0, f"aptp_lr_schedule vs host model, cosines and polynomial past the ramp, fp32 ulps: {what}")
    assert bool(torch.isfinite(out1).all()) and float(out1.min()) >= 0.0


def test_rate_kernel_refuses_bad_arguments(cuda):
    from diffusion_pruning_amd import _lib, ops
    lib = _lib.load()
    count, base = torch.zeros(1, device=cuda), torch.full((16,), 1e-3, device=cuda)
    out, mult = torch.full((64,), -7.0, device=cuda), torch.full((1,), -7.0, device=cuda)

    def params(**over):
        q = _lib.LrScheduleParams()
        q.kind, q.warmup_steps, q.training_steps, q.n = _lib.LR_KINDS["cosine"], 2, 6, 1
        q.num_cycles, q.power, q.lr_end, q.lr_init = 0.5, 1.0, 1e-7, 1e-3
        q.count_dev, q.base_dev, q.out_dev, q.out_stride, q.mult_dev = count.data_ptr(), base.data_ptr(), out.data_ptr(), 1, mult.data_ptr()
        for k, v in over.items():
            setattr(q, k, v)
        return q
    P = _lib.LR_KINDS["polynomial"]
    bad = [dict(count_dev=None), dict(base_dev=None), dict(out_dev=None), dict(count_dev=count.data_ptr() + 2),
           dict(base_dev=base.data_ptr() + 1), dict(out_dev=out.data_ptr() + 2), dict(mult_dev=mult.data_ptr() + 2),
           dict(kind=6), dict(kind=-1), dict(warmup_steps=-1), dict(training_steps=-1), dict(warmup_steps=7),
           dict(kind=_lib.LR_KINDS["linear"], warmup_steps=7), dict(kind=_lib.LR_KINDS["cosine_with_restarts"], warmup_steps=7),
           dict(kind=P, warmup_steps=7), dict(kind=P, warmup_steps=6), dict(training_steps=1 << 24), dict(n=0), dict(n=17),
           dict(out_stride=0), dict(kind=P, lr_init=1e-7), dict(kind=P, lr_init=1e-8), dict(num_cycles=0.0), dict(num_cycles=-1.0),
           dict(kind=_lib.LR_KINDS["cosine_with_restarts"], num_cycles=0.0), dict(kind=P, power=0.0), dict(kind=P, power=-1.0)]
    for over in bad:
        assert lib.aptp_lr_schedule(ctypes.byref(params(**over)), ops._stream()) == -1, over
        assert b"lr_schedule" in lib.aptp_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and float(mult) == -7.0                # nothing was launched
    assert lib.aptp_lr_schedule(ctypes.byref(params(n=16, out_stride=4)), ops._stream()) == 0      # and the untouched arguments are fine
    torch.cuda.synchronize()
    assert bool((out[0::4] == 0.0).all()) and bool((out.reshape(16, 4)[:, 1:] == -7.0).all()) and float(mult) == 0.0


# ---- 2. AdamW with the rate in device memory -------------------------------------------------------------------------------------
def _toy(cuda, grads_seed=40, scale=1.0):
    from tests.test_grad_accum_gpu import SHAPES, _toy_trainer
    ps, sh, tr = _toy_trainer(cuda)
    for i, (p, s) in enumerate(zip(ps, SHAPES)):
        p.grad.copy_(torch.randn(*s, generator=torch.Generator().manual_seed(grads_seed + i)).to(cuda) * scale)
    return ps, sh, tr


def _new_grads(ps, seed, cuda, nan=False):
    for i, p in enumerate(ps):
        p.grad.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(seed + i)).to(cuda))
    if nan:
        ps[1].grad.view(-1)[3] = float("nan")


def _bits(ps, sh, opt):
    extra = [a for a in opt.absmax1 + opt.absmax2 if a is not None]
    return [p.detach().clone() for p in ps] + [t.clone() for t in opt.m + opt.v + sh + extra] + [opt.step_t.clone()]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


OPT_KW = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


@pytest.mark.parametrize("bits", [32, 8])
@pytest.mark.parametrize("how", ["plain", "grad_scale_dev", "gated"])
def test_adamw_with_lr_dev_equals_adamw_with_lr(cuda, bits, how):
    """one step of aptp_adamw_many_lr / aptp_adamw8_many_lr with lr_dev[0] = r against aptp_adamw_many / aptp_adamw8_many with lr = r,
    warmup_steps = 0, over the toy trainer's shapes (5 elements, 1283, 3 * 4096 + 7: scalar tails and a block boundary; with 8-bit
    state two tensors of 4096 elements or more and three below min_8bit_size): parameters, both moments and the bf16 operands."""
    from diffusion_pruning_amd.packed_train import PackedAdamW
    r = f32(3.7e-3)
    kw = dict(optim_bits=bits, **OPT_KW, **({"max_grad_norm": 0.5} if how == "grad_scale_dev" else {}))
    (pa, sa, ta), (pb, sb, tb) = _toy(cuda), _toy(cuda)
    A = PackedAdamW(ta, lr=r, **kw)
    B = PackedAdamW(tb, lr=123.0, **kw)                 # (p->lr is ignored with lr_dev)
    B.lr_t = torch.tensor([r], dtype=torch.float32).to(cuda)      # no schedule: nothing rewrites it; _launch hands it to the *_lr entry point
    assert (bits == 8) == (A.table8 is not None) and A.table is not None and sum(A.is8) == (2 if bits == 8 else 0)
    for step in range(2):                               # the second step starts from moments that are not zero
        gate = torch.tensor([float("nan") if (how == "gated" and step == 1) else 1.0], device=cuda)
        before = _bits(pb, sb, B)
        _new_grads(pa, 70 + 10 * step, cuda)
        _new_grads(pb, 70 + 10 * step, cuda)
        A.step(gate=gate)
        B.step(gate=gate)
        torch.cuda.synchronize()
        assert _same(_bits(pa, sa, A), _bits(pb, sb, B)), (bits, how, step)
        if how == "gated" and step == 1:
            assert _same(_bits(pb, sb, B), before)      # nothing moves under a non-finite gate
        else:
            assert not torch.equal(before[0], pb[0].detach())
    if how == "grad_scale_dev":
        assert float(B.grad_norm.coef) < 1.0            # the clip coefficient was a factor on both sides


@pytest.mark.parametrize("bits", [32, 8])
def test_lr_dev_with_warmup_is_refused(cuda, bits):
    from diffusion_pruning_amd import _lib
    from diffusion_pruning_amd.packed_train import PackedAdamW
    ps, sh, tr = _toy(cuda)
    opt = PackedAdamW(tr, lr=1e-3, warmup_steps=2, optim_bits=bits, min_8bit_size=1, **OPT_KW)
    opt.lr_t = torch.tensor([1e-3], dtype=torch.float32).to(cuda)
    before = _bits(ps, sh, opt)
    with pytest.raises(_lib.AptpError, match="warmup_steps"):
        opt.step()
    torch.cuda.synchronize()
    assert _same(_bits(ps, sh, opt), before)
    with pytest.raises(AssertionError, match="lr_schedule and warmup_steps"):
        PackedAdamW(tr, lr=1e-3, warmup_steps=2, lr_schedule=_sched("cosine", 2, 6, {}), **OPT_KW)


# ---- 3. PackedAdamW(lr_schedule=) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bits", [("cosine", 32), ("linear", 32), ("cosine", 8)])
def test_packed_adamw_follows_the_schedule(cuda, kind, bits):
    """8 steps with W = 2, T = 6 against a second PackedAdamW without a schedule whose rate the test sets from LrSchedule.rate(lr, k)
    before each step; the fourth call is NaN-gated: step count, rate and every tensor keep their bits and the curve resumes at the
    same k.  A state_dict() taken after four calls, loaded into a fresh optimizer, continues bit-equal to the uninterrupted run."""
    from diffusion_pruning_amd.packed_train import PackedAdamW
    lr, sched = 1e-2, _sched(kind, 2, 6, {})
    (pa, sa, ta), (pb, sb, tb), (pc, sc, tc) = _toy(cuda), _toy(cuda), _toy(cuda)
    A = PackedAdamW(ta, lr=lr, lr_schedule=sched, optim_bits=bits, **OPT_KW)
    B = PackedAdamW(tb, lr=lr, optim_bits=bits, **OPT_KW)
    assert A.lr_t is not None and A.lr_base_t is not None and B.lr_t is None and B.lr_base_t is None and B.lr_schedule is None
    assert A.state_dict()["lr_schedule"] == sched.as_dict() and B.state_dict()["lr_schedule"] is None
    C, k, rates = None, 0, []
    for call in range(9):
        gated = call == 3
        gate = torch.tensor([float("inf") if gated else 0.5], device=cuda)
        for ps in (pa, pb) + ((pc,) if C is not None else ()):
            _new_grads(ps, 100 + 7 * call, cuda)
        assert A.last_lr() == sched.rate(lr, k) == f32(M.rate(kind, lr, k, 2, 6))
        B.set_lr(sched.rate(lr, k))
        before = _bits(pa, sa, A)
        A.step(gate=gate)
        B.step(gate=gate)
        if C is not None:
            C.step(gate=gate)
        torch.cuda.synchronize()
        assert float(A.lr_t) == sched.rate(lr, k), (call, k)          # the rate this call ran at (or would have)
        rates.append(float(A.lr_t))
        assert _same(_bits(pa, sa, A), _bits(pb, sb, B)), (kind, bits, call)
        if C is not None:
            assert _same(_bits(pa, sa, A), _bits(pc, sc, C)), (kind, bits, call)
        if gated:
            assert _same(_bits(pa, sa, A), before) and float(A.step_t) == k
        else:
            k += 1
            assert float(A.step_t) == k
        if call == 4:         # four applied steps: a fresh optimizer over a copy of the state takes over next to the original
            for dst, src in zip(pc + sc, pa + sa):
                dst.data.copy_(src.data)
            C = PackedAdamW(tc, lr=lr, lr_schedule=sched.as_dict(), optim_bits=bits, **OPT_KW)
            C.load_state_dict(A.state_dict())
            assert float(C.step_t) == 4.0 and C.last_lr() == A.last_lr() and C.lr_schedule == sched
    # (the gated fourth call found k = 3 and left it: the fifth ran at the same rate)
    assert k == 8 and rates[3] == rates[4] != rates[2] and rates[0] == 0.0 and rates[2] == f32(lr) and len(set(rates[2:])) >= 5
    A.set_lr(2 * lr)
    assert A.last_lr() == sched.rate(2 * lr, 8) and float(A.lr_base_t) == f32(2 * lr)


def test_constant_with_warmup_schedule_is_warmup_steps(cuda):
    from diffusion_pruning_amd.packed_train import PackedAdamW
    W, lr = 3, 1e-2
    (pa, sa, ta), (pb, sb, tb) = _toy(cuda), _toy(cuda)
    A = PackedAdamW(ta, lr=lr, lr_schedule=_sched("constant_with_warmup", W, None, {}), **OPT_KW)
    B = PackedAdamW(tb, lr=lr, warmup_steps=W, **OPT_KW)
    for call in range(5):
        _new_grads(pa, 200 + call, cuda)
        _new_grads(pb, 200 + call, cuda)
        assert A.last_lr() == B.last_lr()
        A.step()
        B.step()
        torch.cuda.synchronize()
        assert _same(_bits(pa, sa, A), _bits(pb, sb, B)), call


def test_step_group_reads_the_same_rate(cuda):
    """the bucketed path: every group launch of a step runs at the rate of the step count before finish_step"""
    from diffusion_pruning_amd.packed_train import PackedAdamW
    lr, sched = 1e-2, _sched("cosine", 2, 6, {})
    (pa, sa, ta), (pb, sb, tb) = _toy(cuda), _toy(cuda)
    ids = {id(p): i % 2 for i, p in enumerate(pa)}
    A = PackedAdamW(ta, lr=lr, lr_schedule=sched, group_of=lambda p: ids[id(p)], **OPT_KW)
    B = PackedAdamW(tb, lr=lr, lr_schedule=sched, **OPT_KW)
    for call in range(4):
        _new_grads(pa, 300 + call, cuda)
        _new_grads(pb, 300 + call, cuda)
        for gi in sorted(A.groups):
            A.step_group(gi)
        A.finish_step()
        B.step()
        torch.cuda.synchronize()
        assert _same(_bits(pa, sa, A), _bits(pb, sb, B)), call


# ---- 4. RouterAdamW(lr_schedule=), eager -----------------------------------------------------------------------------------------
def _router_pair(cuda, sched, seed=3):
    from diffusion_pruning_amd.router_optim import RouterAdamW
    from tests.test_router_optim_gpu import toy
    shapes, g, ps = toy(cuda, seed)
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    groups = lambda ts: [{"params": ts[:2], "lr": BASE[0], "weight_decay": 1e-2}, {"params": ts[2:], "lr": BASE[1], "weight_decay": 0.1}]   # noqa: E731
    return shapes, g, ps, qs, RouterAdamW(groups(ps), lr_schedule=sched), RouterAdamW(groups(qs))


def _router_bits(opt):
    return [p.detach().clone() for p in opt.params] + [t.clone() for t in opt.m + opt.v] + [opt.steps.clone(), opt.counters.clone()]


@pytest.mark.parametrize("kind", ["cosine", "polynomial"])
def test_router_adamw_follows_the_schedule(cuda, kind):
    sched = _sched(kind, 2, 6, {})
    shapes, g, ps, qs, A, B = _router_pair(cuda, sched)
    assert A.base_lr_dev is not None and B.base_lr_dev is None and B.lr_schedule is None
    assert A.base_lr_dev.tolist() == [f32(b) for b in BASE] and A.groups_dev[:, 2].tolist() == [0.0, 0.0]
    k = 0
    for call in range(8):
        skip = call == 3
        want = [sched.rate(b, k) for b in BASE]
        assert A.last_lr() == want == [f32(M.rate(kind, b, k, 2, 6)) for b in BASE]
        for gi, r in enumerate(want):
            B.set_lr(gi, r)
        for i, (p, q) in enumerate(zip(ps, qs)):
            gr = torch.randn(*shapes[i], generator=g).to(cuda)
            if skip and i == 1:
                gr[2] = float("nan")
            p.grad.copy_(gr)
            q.grad.copy_(gr)
        before = _router_bits(A)
        A.step()
        B.step()
        torch.cuda.synchronize()
        assert A.groups_dev[:, 0].tolist() == want and A.groups_dev[:, 1:].tolist() == [[f32(1e-2), 0.0], [f32(0.1), 0.0]]
        a, b = _router_bits(A), _router_bits(B)
        assert _same(a, b), (kind, call)
        if skip:
            assert _same(a[:-1], before[:-1]) and A.skipped_steps() == 1 and A.applied_steps() == k
        else:
            k += 1
    assert A.applied_steps() == 7
    sd = A.state_dict()
    assert sd["router_adamw"]["lr_schedule"] == sched.as_dict() and [pg["lr"] for pg in sd["param_groups"]] == list(BASE)
    assert "lr_schedule" not in B.state_dict()["router_adamw"]
    A.set_lr(1, 1e-3)
    assert A.last_lr() == [sched.rate(BASE[0], 7), sched.rate(1e-3, 7)] and A.base_lr_dev.tolist() == [f32(BASE[0]), f32(1e-3)]


# ---- 5. captured steps -----------------------------------------------------------------------------------------------------------
def test_captured_pruning_step_follows_the_schedule(cuda):
    """a tiny GraphedPrunerStep as in tests/test_router_optim_gpu.py with the schedule installed, against the same captured step
    under a RouterAdamW without a schedule whose rates the host sets from the model before every step (the eager sequence of the
    test above): bit for bit over both phases and a recapture of the main phase; last_lr() follows the model throughout."""
    import copy
    from diffusion_pruning_amd.router_optim import RouterAdamW
    from diffusion_pruning_amd.train_step import GraphedPrunerStep
    from tests.test_router_optim_gpu import batch_of
    from tests.test_train_step_gpu import build
    cfg, unet, params, hn0, qz0 = build(cuda)
    unet.to(cuda).freeze()
    hn0.to(cuda).train()
    qz0.to(cuda).train()
    sched = _sched("cosine", 2, 6, {})
    batches = [batch_of(cfg, cuda, s) for s in (3, 4, 5, 6, 7)]

    def run(with_schedule):
        hn, qz = copy.deepcopy(hn0), copy.deepcopy(qz0)
        step = GraphedPrunerStep(unet, hn, qz)
        step.count_macs(16)
        opt = RouterAdamW([{"params": [p for p in hn.parameters() if p.requires_grad], "lr": BASE[0], "weight_decay": 0.0},
                           {"params": [p for p in qz.parameters() if p.requires_grad], "lr": BASE[1], "weight_decay": 0.1}],
                          lr_schedule=sched if with_schedule else None)
        torch.manual_seed(77)
        step.capture(batches[0], optimizer=opt, pretrain=True)
        step.capture_router(batches[0], pretrain=False)
        assert opt.applied_steps() == 0                 # the capture's warm-up steps were undone
        trace = []
        for i, b in enumerate(batches):
            if i == 4:
                step.capture_router(batches[0], pretrain=False)        # a recapture in the middle of the run
            k = opt.applied_steps()
            want = [sched.rate(r, k) for r in BASE]
            if with_schedule:
                assert opt.last_lr() == want, (i, k)
            else:
                for gi, r in enumerate(want):
                    opt.set_lr(gi, r)
            o = step.train_step(opt, b, pretrain=i < 2)
            step.finish()
            torch.cuda.synchronize()
            assert float(o["applied"]) == 1.0 and opt.applied_steps() == i + 1
            if with_schedule:
                assert opt.groups_dev[:, 0].tolist() == want, (i, want)
            trace.append([float(o["loss"])] + _router_bits(opt)[:-2] + [opt.steps.clone()])
        step.remove_hooks()
        return trace

    ta, tb = run(True), run(False)
    for i, (a, b) in enumerate(zip(ta, tb)):
        assert a[0] == b[0] and _same(a[1:], b[1:]), i
    assert not _same(ta[0][1:], ta[-1][1:])


def test_graphed_finetune_step_follows_the_schedule(cuda):
    """GraphedFineTunerStep(lr_scheduler="cosine", lr_warmup_steps=2, max_train_steps=6, accumulation_steps=2): the rate advances
    once per window, not per micro-batch; a non-finite micro-batch skips the window and the rate stays; log_lr returns the model's
    value.  Next to it the step without a scheduler: no rate tensors, no "lr" entry."""
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    from tests.test_grad_accum_gpu import KW, _setup
    sa, sb, teacher, batches = _setup(cuda, seeds=(4, 5, 6, 7))
    lr = KW["lr"]
    A = GraphedFineTunerStep(sa, teacher, lr_scheduler="cosine", lr_warmup_steps=2, max_train_steps=6, accumulation_steps=2,
                             log_lr=True, **KW)
    A.capture(batches[0])
    opt = A.optimizer
    assert opt.lr_schedule == _sched("cosine", 2, 6, {}) and opt.warmup_steps == 0 and opt.lr_t is not None
    k = 0
    for w in range(6):                                  # six windows of two micro-batches; the third holds a NaN
        window = [{n: v.clone() for n, v in batches[(2 * w + j) % 4].items()} for j in range(2)]
        if w == 2:
            window[1]["target"][0, 0, 0, 0] = float("nan")
        o0 = A.train_step(None, window[0])
        torch.cuda.synchronize()
        assert o0["applied"] is False and o0["lr"] is None and float(opt.step_t) == k
        o1 = A.train_step(None, window[1])
        torch.cuda.synchronize()
        assert o1["applied"] is True and torch.is_tensor(o1["lr"]) and o1["lr"].device.type == "cuda"
        assert float(o1["lr"]) == f32(M.rate("cosine", lr, k, 2, 6)), (w, k)
        if w != 2:
            k += 1
        assert float(opt.step_t) == k and opt.last_lr() == f32(M.rate("cosine", lr, k, 2, 6))
    assert k == 5
    B = GraphedFineTunerStep(sb, teacher, **KW)
    B.capture(batches[0])
    assert B.lr_schedule is None and B.optimizer.lr_schedule is None and B.optimizer.lr_t is None and B.optimizer.lr_base_t is None
    out = B.train_step(None, batches[0])
    torch.cuda.synchronize()
    assert "lr" not in out and set(out) == {"loss", "diff_loss", "distillation_loss", "block_loss", "applied", "accum_index"}
    with pytest.raises(AssertionError, match="log_lr"):
        GraphedFineTunerStep(sb, teacher, log_lr=True, **KW)
    with pytest.raises(ValueError, match="piecewise_constant"):
        GraphedFineTunerStep(sb, teacher, lr_scheduler="piecewise_constant", **KW)


# ---- 6. the defaults take none of the new paths ----------------------------------------------------------------------------------
def test_defaults_are_the_unchanged_entry_points(cuda):
    """without a schedule PackedAdamW and RouterAdamW hold no rate tensors, and a step is, bit for bit, a direct call of the unchanged
    symbols aptp_adamw_many and aptp_group_adamw"""
    from diffusion_pruning_amd import _lib, ops
    from diffusion_pruning_amd.packed_train import PackedAdamW
    lib = _lib.load()
    (pa, sa, ta), (pb, sb, tb) = _toy(cuda), _toy(cuda)
    A, B = PackedAdamW(ta, lr=1e-2, warmup_steps=2, **OPT_KW), PackedAdamW(tb, lr=1e-2, warmup_steps=2, **OPT_KW)
    assert A.lr_t is None and A.lr_base_t is None and A.lr_schedule is None
    for call in range(3):
        _new_grads(pa, 400 + call, cuda)
        _new_grads(pb, 400 + call, cuda)
        A.step()
        q = _lib.AdamWParams()
        q.items_dev, q.starts_dev, q.n_items, q.total_blocks = B.table.args()
        q.lr, q.beta1, q.beta2, q.eps, q.weight_decay = 1e-2, 0.9, 0.999, 1e-8, 1e-2
        q.step_dev, q.grad_scale, q.warmup_steps = B.step_t.data_ptr(), 1.0, 2.0
        assert lib.aptp_adamw_many(ctypes.byref(q), ops._stream()) == 0
        B.step_t += 1.0
        torch.cuda.synchronize()
        assert _same(_bits(pa, sa, A), _bits(pb, sb, B)), call
    from diffusion_pruning_amd.router_optim import RouterAdamW
    from tests.test_router_optim_gpu import toy
    shapes, g, ps = toy(cuda)
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    S, R = (RouterAdamW([{"params": ts[:2], "lr": BASE[0], "weight_decay": 1e-2}, {"params": ts[2:], "lr": BASE[1], "weight_decay": 0.1}],
                        warmup_steps=2) for ts in (ps, qs))
    assert S.base_lr_dev is None and S.lr_schedule is None and "lr_schedule" not in S.state_dict()["router_adamw"]
    for call in range(3):
        for i, (p, q_) in enumerate(zip(ps, qs)):
            gr = torch.randn(*shapes[i], generator=g).to(cuda)
            p.grad.copy_(gr)
            q_.grad.copy_(gr)
        S.step()
        tb_ = R.tables[None]
        q = _lib.GroupAdamWParams()
        q.items_dev, q.starts_dev, q.n_items, q.total_blocks = tb_.args()
        q.groups_dev, q.n_groups, q.counters_dev = R.groups_dev.data_ptr(), 2, R.counters.data_ptr()
        q.beta1, q.beta2, q.eps, q.grad_scale, q.zero_grad = 0.9, 0.999, 1e-8, 1.0, 1
        assert lib.aptp_group_adamw(ctypes.byref(q), ops._stream()) == 0
        torch.cuda.synchronize()
        assert _same(_router_bits(S), _router_bits(R)), call
