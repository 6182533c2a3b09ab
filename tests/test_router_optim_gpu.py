"""GPU tests of the router's optimizer and of the captured pruning step that runs the whole recipe from one capture:
csrc/router_optim.hip against the fp64 model of tests/router_adamw_model.py, router_optim.RouterAdamW against torch.optim.AdamW,
and GraphedPrunerStep with both phases, the rate in device memory, the NaN skip and a resume.  TINY U-Net, 4 x 16 x 16 batches."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import router_adamw_model as M
from tests.test_train_step_gpu import build, rel_l2

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 4096, 4097, 3 * 4096 + 7]     # scalar tail only, float4 + tail, whole blocks, more than one block


def f32(x):
    return float(np.float32(x))


# rates between the recipe's base rate (2e-4, configs/pruning/sd-2-1_cc3m.yaml:115-116) and its scaled one; fp32-representable, so the
# fp64 model sees the numbers the kernel sees
BETAS, EPS = (f32(0.9), f32(0.999)), f32(1e-8)
GROUPS = [(f32(1e-3), f32(1e-2), 4.0), (f32(3e-3), f32(0.1), 0.0)]


class Bench:
    """a table of toy tensors in device memory and one call of aptp_group_adamw over it"""

    def __init__(self, dev, sizes, group_of, groups, seed=0):
        from diffusion_pruning_amd import _lib
        self.lib, self._lib, self.dev = _lib.load(), _lib, dev
        g = torch.Generator().manual_seed(seed)
        self.gen = g
        self.p = [torch.randn(n, generator=g).to(dev) for n in sizes]
        self.g = [torch.zeros(n, device=dev) for n in sizes]
        self.m = [torch.zeros(n, device=dev) for n in sizes]
        self.v = [torch.zeros(n, device=dev) for n in sizes]
        self.steps = torch.zeros(len(sizes), device=dev)
        self.counters = torch.zeros(4, device=dev)
        self.group_of = list(group_of)
        self.groups = torch.tensor(groups, dtype=torch.float32).to(dev)
        self.n_groups = len(groups)
        self.host = (_lib.GroupAdamWItem * len(sizes))()
        starts = [0]
        for i, it in enumerate(self.host):
            it.p, it.g, it.m, it.v = (t[i].data_ptr() for t in (self.p, self.g, self.m, self.v))
            it.step, it.n, it.group = self.steps.data_ptr() + 4 * i, sizes[i], self.group_of[i]
            starts.append(starts[-1] + self.lib.aptp_group_adamw_blocks(sizes[i]))
        self.total = starts[-1]
        self.starts = torch.tensor(starts, dtype=torch.int32).to(dev)
        self.upload()

    def upload(self):
        self.items = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(self.dev)

    def params(self, gate=None, grad_scale=1.0, zero_grad=1):
        q = self._lib.GroupAdamWParams()
        q.items_dev, q.starts_dev, q.n_items, q.total_blocks = self.items.data_ptr(), self.starts.data_ptr(), len(self.p), self.total
        q.groups_dev, q.n_groups, q.counters_dev = self.groups.data_ptr(), self.n_groups, self.counters.data_ptr()
        q.beta1, q.beta2, q.eps, q.grad_scale, q.zero_grad = BETAS[0], BETAS[1], EPS, grad_scale, zero_grad
        q.gate_dev = None if gate is None else gate.data_ptr()
        q.items_host = ctypes.cast(self.host, ctypes.c_void_p)
        return q

    def call(self, q):
        from diffusion_pruning_amd import ops
        return self.lib.aptp_group_adamw(ctypes.byref(q), ops._stream())

    def model_items(self):
        st = self.steps.tolist()
        return [{"p": self.p[i].cpu(), "g": self.g[i].cpu(), "m": self.m[i].cpu(), "v": self.v[i].cpu(), "step": st[i],
                 "group": self.group_of[i]} for i in range(len(self.p))]

    def new_grads(self):
        for gr in self.g:
            gr.copy_(torch.randn(gr.shape, generator=self.gen).to(self.dev))

    def bits(self):
        return [t.clone() for t in self.p + self.m + self.v + [self.steps]]


def close(got, ref):
    """the project's margin for aptp_adamw_many against torch (tests/test_finetune_gpu.py:268), per tensor"""
    return float((got.double().cpu() - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) + 1e-7


def seasoned_bench(cuda, lag=2):
    """every item but `lag` has three steps behind it (moments of three unit-variance gradients, step_i = 3); `lag` starts fresh"""
    b = Bench(cuda, SIZES, [i % 2 for i in range(len(SIZES))], GROUPS)
    items = b.model_items()
    for _ in range(3):
        for it in items:
            it["g"] = torch.randn(it["p"].shape, generator=b.gen)
        items, _ = M.step(items, [(0.0, 0.0, 0.0)] * 2, [0.0] * 4, BETAS, EPS)       # rate 0: only the moments and counts move
    for i, it in enumerate(items):
        if i != lag:
            b.m[i].copy_(it["m"].float())
            b.v[i].copy_(it["v"].float())
            b.steps[i] = 3.0
    return b


def test_kernel_against_the_model(cuda):
    b = seasoned_bench(cuda)
    W_group_items = [i for i in range(len(SIZES)) if b.group_of[i] == 0]
    for k in range(6):
        b.new_grads()
        items = b.model_items()
        before = b.bits()
        ref, ref_c = M.step(items, GROUPS, b.counters.tolist(), BETAS, EPS, zero_grad=True)
        assert b.call(b.params()) == 0
        torch.cuda.synchronize()
        for i, r in enumerate(ref):
            assert close(b.p[i], r["p"]) and close(b.m[i], r["m"]) and close(b.v[i], r["v"]), (k, i)
            assert not b.g[i].any()
        assert b.steps.tolist() == [r["step"] for r in ref] and b.counters.tolist() == ref_c, k
        if k == 0:          # applied = 0 in the warm-up group: rate 0 -- p keeps its bits while m moves
            for i in W_group_items:
                assert torch.equal(b.p[i], before[i]) and not torch.equal(b.m[i], before[len(SIZES) + i])
            assert not torch.equal(b.p[1], before[1])
    assert b.steps.tolist() == [9.0, 9.0, 6.0, 9.0, 9.0, 9.0, 9.0, 9.0] and b.counters.tolist() == [6.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("how", ["gate_nan", "gate_inf", "gate_minus_inf", "grad_nan"])
def test_skips(cuda, how):
    b = seasoned_bench(cuda)
    b.new_grads()
    assert b.call(b.params()) == 0                                   # one clean step first: applied = 1
    b.new_grads()
    gate = torch.tensor([{"gate_nan": float("nan"), "gate_inf": float("inf"), "gate_minus_inf": -float("inf")}.get(how, 0.5)], device=cuda)
    if how == "grad_nan":
        b.g[-1][4096 + 5] = float("nan")                             # one element of the largest item, second block
    before = b.bits()
    assert b.call(b.params(gate=gate)) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(b.bits(), before))
    assert b.counters.tolist() == [1.0, 1.0, 0.0, 0.0]
    assert all(not gr.any() for gr in b.g)
    # the next clean step matches the model
    b.new_grads()
    ref, ref_c = M.step(b.model_items(), GROUPS, b.counters.tolist(), BETAS, EPS, gate=0.5, zero_grad=True)
    gate.fill_(0.5)
    assert b.call(b.params(gate=gate)) == 0
    torch.cuda.synchronize()
    for i, r in enumerate(ref):
        assert close(b.p[i], r["p"]) and close(b.m[i], r["m"]) and close(b.v[i], r["v"]), i
    assert b.steps.tolist() == [r["step"] for r in ref] and b.counters.tolist() == ref_c == [2.0, 1.0, 0.0, 0.0]


def test_refusals(cuda):
    b = Bench(cuda, [5, 4097], [0, 1], GROUPS)
    b.new_grads()
    before = b.bits() + [gr.clone() for gr in b.g] + [b.counters.clone()]

    def refused(**kw):
        q = b.params()
        for k, v in kw.items():
            setattr(q, k, v)
        assert b.call(q) == -1, kw
    for name in ("items_dev", "starts_dev", "groups_dev", "counters_dev"):
        refused(**{name: None})
    assert b.lib.aptp_group_adamw(None, None) == -1
    refused(n_items=0)
    refused(n_groups=0)
    refused(total_blocks=0)
    refused(total_blocks=b.total + 1)                                # more blocks than the items need
    for name in ("beta1", "beta2"):
        refused(**{name: 1.0})
        refused(**{name: -0.1})
    refused(eps=0.0)
    refused(eps=-1e-8)
    refused(grad_scale=-1.0)
    refused(counters_dev=b.counters.data_ptr() + 4)                  # misaligned table
    for field, bad in (("p", b.p[1].data_ptr() + 4), ("g", b.g[1].data_ptr() + 8), ("m", 0), ("step", 0), ("n", 0), ("group", 2), ("group", -1)):
        keep = getattr(b.host[1], field)
        setattr(b.host[1], field, bad)
        refused()
        setattr(b.host[1], field, keep)
    torch.cuda.synchronize()
    after = b.bits() + [gr.clone() for gr in b.g] + [b.counters.clone()]
    assert all(torch.equal(a, c) for a, c in zip(after, before))
    assert b.call(b.params()) == 0                                   # and the untouched arguments are fine
    torch.cuda.synchronize()
    assert b.counters.tolist() == [1.0, 0.0, 0.0, 0.0]


# ---- RouterAdamW ------------------------------------------------------------------------------------------------------------------
def toy(cuda, seed=3):
    g = torch.Generator().manual_seed(seed)
    shapes = [(17, 5), (9,), (4, 4), (4097,)]
    return shapes, g, [torch.nn.Parameter(torch.randn(*s, generator=g).to(cuda)) for s in shapes]


def test_interop_with_torch_adamw(cuda):
    from diffusion_pruning_amd.router_optim import RouterAdamW
    shapes, g, ps = toy(cuda)
    kw = dict(betas=(0.9, 0.999), eps=1e-8)
    topt = torch.optim.AdamW([{"params": ps[:2], "lr": 1e-3, "weight_decay": 1e-2}, {"params": ps[2:], "lr": 3e-3, "weight_decay": 0.1}], **kw)
    for k in range(2):
        for i, p in enumerate(ps):
            p.grad = None if (i == 3 and k == 0) else torch.randn(*shapes[i], generator=g).to(cuda)   # one tensor lags by a step
        topt.step()
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = RouterAdamW([{"params": qs[:2], "lr": 5e-2, "weight_decay": 0.0}, {"params": qs[2:], "lr": 5e-2, "weight_decay": 0.0}], **kw)
    opt.load_state_dict(topt.state_dict())
    assert opt.steps.tolist() == [2.0, 2.0, 2.0, 1.0] and opt.applied_steps() == 2
    assert [pg["lr"] for pg in opt.param_groups] == [1e-3, 3e-3] and [pg["weight_decay"] for pg in opt.param_groups] == [1e-2, 0.1]
    for i, (p, q) in enumerate(zip(ps, qs)):
        gr = torch.randn(*shapes[i], generator=g).to(cuda)
        p.grad = gr.clone()
        q.grad.copy_(gr)
    topt.step()
    opt.step()
    for p, q in zip(ps, qs):
        assert close(q.detach(), p.detach().double().cpu())
    assert opt.steps.tolist() == [3.0, 3.0, 3.0, 2.0] and all(not q.grad.any() for q in qs)
    # the reverse direction: a fresh torch optimizer takes our state and the same fourth step
    rs = [torch.nn.Parameter(q.detach().clone()) for q in qs]
    topt2 = torch.optim.AdamW([{"params": rs[:2], "lr": 1.0}, {"params": rs[2:], "lr": 1.0}], **kw)
    topt2.load_state_dict(opt.state_dict())
    assert [pg["lr"] for pg in topt2.param_groups] == [1e-3, 3e-3]
    for i, (q, r) in enumerate(zip(qs, rs)):
        gr = torch.randn(*shapes[i], generator=g).to(cuda)
        q.grad.copy_(gr)
        r.grad = gr.clone()
    opt.step()
    topt2.step()
    for q, r in zip(qs, rs):
        assert close(q.detach(), r.detach().double().cpu())
    # a different tensor list is refused
    other = RouterAdamW([{"params": [torch.nn.Parameter(torch.zeros(3, device=cuda))], "lr": 1e-3, "weight_decay": 0.0}])
    with pytest.raises(ValueError):
        other.load_state_dict(opt.state_dict())


def test_rate_without_recapture(cuda):
    from diffusion_pruning_amd.router_optim import RouterAdamW
    shapes, g, ps = toy(cuda)
    opt = RouterAdamW([{"params": ps[:2], "lr": 1e-3, "weight_decay": 1e-2}, {"params": ps[2:], "lr": 3e-3, "weight_decay": 0.1}])
    src = [torch.randn(*s, generator=g).to(cuda) for s in shapes]

    def body():
        for p, s0 in zip(ps, src):
            p.grad.add_(s0)
        opt.step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        snap = opt._snapshot()
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    opt._restore(snap)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    assert opt.applied_steps() == 0
    opt.set_lr(0, 0.0)
    opt.set_lr(1, 0.0)
    p0, m0 = [p.detach().clone() for p in ps], [m.clone() for m in opt.m]
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p.detach(), a) for p, a in zip(ps, p0)) and all(not torch.equal(m, a) for m, a in zip(opt.m, m0))
    assert opt.applied_steps() == 1 and opt.last_lr() == [0.0, 0.0]
    opt.set_lr(0, 1e-3)
    opt.set_lr(1, 3e-3)
    graph.replay()
    torch.cuda.synchronize()
    assert all(not torch.equal(p.detach(), a) for p, a in zip(ps, p0)) and opt.applied_steps() == 2


# ---- the captured pruning step ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(cuda):
    cfg, unet, params, hn, qz = build(cuda)
    unet.to(cuda).freeze()
    hn.to(cuda).train()
    qz.to(cuda).train()
    return cfg, unet, hn, qz


def batch_of(cfg, cuda, seed):
    from diffusion_pruning_amd.train_step import synthetic_batch
    return synthetic_batch(4, 16, cuda, seed=seed, cross_dim=cfg.cross_attention_dim, text_dim=32)


def make(world, lr=1e-3, wd_q=0.0, warmup=0, overlap=True):
    from diffusion_pruning_amd.router_optim import RouterAdamW
    from diffusion_pruning_amd.train_step import GraphedPrunerStep
    cfg, unet, hn0, qz0 = world
    hn, qz = copy.deepcopy(hn0), copy.deepcopy(qz0)
    step = GraphedPrunerStep(unet, hn, qz)
    step.overlap_router = overlap
    step.count_macs(16)
    opt = RouterAdamW([{"params": [p for p in hn.parameters() if p.requires_grad], "lr": lr, "weight_decay": 0.0},
                       {"params": [p for p in qz.parameters() if p.requires_grad], "lr": lr, "weight_decay": wd_q}], warmup_steps=warmup)
    return step, opt, hn, qz


def router_bits(opt):
    return [p.detach().clone() for p in opt.params] + [m.clone() for m in opt.m] + [v.clone() for v in opt.v] + [opt.steps.clone(), opt.counters.clone()]


def test_capture_is_free_in_any_state(cuda, world):
    cfg = world[0]
    step, opt, hn, qz = make(world, wd_q=0.1, warmup=4)
    torch.manual_seed(5)
    for s in (3, 4):
        step.train_step(opt, batch_of(cfg, cuda, s), pretrain=True)              # eager: nothing is captured yet
    torch.cuda.synchronize()
    assert opt.applied_steps() == 2 and float(opt.steps.max()) == 2.0
    before, rng = router_bits(opt), torch.get_rng_state()
    step.capture(batch_of(cfg, cuda, 3), optimizer=opt, pretrain=True)
    step.capture_router(batch_of(cfg, cuda, 3), pretrain=False)
    torch.cuda.synchronize()
    assert set(step._cap["router"]) >= {True, False}
    assert all(torch.equal(a, b) for a, b in zip(router_bits(opt), before)) and torch.equal(torch.get_rng_state(), rng)
    assert all(not p.grad.any() for p in opt.params)
    step.remove_hooks()


def test_phases_from_one_capture(cuda, world):
    cfg = world[0]
    step, opt, hn, qz = make(world, wd_q=0.1)
    torch.manual_seed(5)
    step.capture(batch_of(cfg, cuda, 3), optimizer=opt, pretrain=True)
    step.capture_router(batch_of(cfg, cuda, 3), pretrain=False)
    code = qz.embedding.weight
    ci = [i for i, p in enumerate(opt.params) if p is code][0]
    hi = [i for i, p in enumerate(opt.params) if any(p is h for h in hn.parameters())]
    code0 = code.detach().clone()
    for s in (3, 4):
        step.train_step(opt, batch_of(cfg, cuda, s), pretrain=True)
    step.finish()
    torch.cuda.synchronize()
    st = opt.steps.tolist()
    assert torch.equal(code.detach(), code0) and st[ci] == 0.0 and all(st[i] == 2.0 for i in hi)
    assert not opt.m[ci].any() and opt.applied_steps() == 2
    for s in (5, 6):
        step.train_step(opt, batch_of(cfg, cuda, s), pretrain=False)
    step.finish()
    torch.cuda.synchronize()
    assert not torch.equal(code.detach(), code0) and opt.steps.tolist()[ci] == 2.0 and opt.applied_steps() == 4
    assert all(opt.steps.tolist()[i] == 4.0 for i in hi) and opt.skipped_steps() == 0
    step.remove_hooks()


def test_captured_equals_eager_under_the_same_optimizer(cuda, world):
    cfg = world[0]
    batches = [batch_of(cfg, cuda, s) for s in (3, 4, 5, 6)]
    keys = ("loss", "diff_loss", "distillation_loss", "block_loss", "resource_loss", "contrastive_loss")

    def run(captured, overlap=True):
        step, opt, hn, qz = make(world, wd_q=0.1, warmup=2, overlap=overlap)
        p0 = torch.cat([p.detach().flatten().clone() for p in opt.params])
        torch.manual_seed(77)
        if captured:
            step.capture(batches[0], optimizer=opt, pretrain=True)
            step.capture_router(batches[0], pretrain=False)
        else:
            step.capture(batches[0])
        losses = []
        for i, b in enumerate(batches):
            o = step.train_step(opt, b, pretrain=i < 2)
            step.finish()
            losses.append({k: float(o[k]) for k in keys})
            assert float(o["applied"]) == 1.0
        step.finish()
        torch.cuda.synchronize()
        step.remove_hooks()
        return losses, torch.cat([p.detach().flatten().clone() for p in opt.params]), p0, opt.steps.clone()

    la, pa, p0, sa = run(False)
    lb, pb, _, sb = run(True)
    for a, b in zip(la, lb):
        for k in a:
            assert abs(a[k] - b[k]) <= 2e-3 * abs(a[k]) + 1e-5, (k, a, b)
    assert float((pa - p0).abs().max()) > 0 and torch.equal(sa, sb)
    assert rel_l2(pb - p0, pa - p0) <= 2e-2, rel_l2(pb - p0, pa - p0)
    lc, pc, _, _ = run(True, overlap=False)
    assert lc == lb and torch.equal(pc, pb)


def test_nan_batch_is_skipped(cuda, world):
    cfg = world[0]
    step, opt, hn, qz = make(world, wd_q=0.1)
    torch.manual_seed(5)
    step.capture(batch_of(cfg, cuda, 3), optimizer=opt, pretrain=False)
    step.train_step(opt, batch_of(cfg, cuda, 3))
    step.finish()
    torch.cuda.synchronize()
    before = router_bits(opt)[:-1]
    bad = batch_of(cfg, cuda, 4)
    bad["target"][1, 2, 3, 4] = float("nan")
    o = step.train_step(opt, bad)
    step.finish()
    torch.cuda.synchronize()
    assert float(o["applied"]) == 0.0 and opt.skipped_steps() == 1 and opt.applied_steps() == 1
    assert all(torch.equal(a, b) for a, b in zip(router_bits(opt)[:-1], before))
    assert all(not p.grad.any() for p in opt.params)
    o = step.train_step(opt, batch_of(cfg, cuda, 5))
    step.finish()
    torch.cuda.synchronize()
    assert float(o["applied"]) == 1.0 and opt.applied_steps() == 2 and opt.skipped_steps() == 1
    assert not torch.equal(router_bits(opt)[0], before[0])
    step.remove_hooks()


def test_resume(cuda, world):
    cfg = world[0]
    batches = [batch_of(cfg, cuda, s) for s in (3, 4, 5, 6)]

    def fourth(step, opt):
        torch.manual_seed(123)
        o = step.train_step(opt, batches[3])
        step.finish()
        torch.cuda.synchronize()
        return [float(o[k]) for k in ("loss", "diff_loss", "contrastive_loss", "resource_loss")], [p.detach().clone() for p in opt.params]

    step, opt, hn, qz = make(world, wd_q=0.1, warmup=8)
    torch.manual_seed(5)
    step.capture(batches[0], optimizer=opt, pretrain=False)
    for b in batches[:3]:
        step.train_step(opt, b)
    step.finish()
    torch.cuda.synchronize()
    saved = copy.deepcopy({"hn": hn.state_dict(), "qz": qz.state_dict(), "opt": opt.state_dict()})
    la, pa = fourth(step, opt)
    step.remove_hooks()

    step2, opt2, hn2, qz2 = make(world, wd_q=0.1, warmup=8)
    hn2.load_state_dict(saved["hn"])
    qz2.load_state_dict(saved["qz"])
    opt2.load_state_dict(saved["opt"])
    assert opt2.applied_steps() == 3 and abs(opt2.last_lr()[0] - 1e-3 * 3 / 8) < 1e-12
    torch.manual_seed(999)                                              # the capture leaves the generator where it finds it
    step2.capture(batches[0], optimizer=opt2, pretrain=False)
    lb, pb = fourth(step2, opt2)
    step2.remove_hooks()
    assert la == lb and all(torch.equal(a, b) for a, b in zip(pa, pb))
