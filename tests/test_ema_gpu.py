"""GPU checks of the EMA of the expert fine-tune: csrc/ema.hip (aptp_ema_many: UPDATE and SWAP) against the fp64 model of
tests/ema_model.py, packed_train.PackedEMA, and its place in train_step.GraphedFineTunerStep(ema=...): trajectory, gating,
accumulation, swap, validation of the averaged weights, export and resume.  Tiny expert (O.TINY), 16x16 latents,
micro-batches of 2, lr = 1e-3 -- the setting of tests/test_grad_accum_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import unet_oracle as O
from tests import ema_model as M

pytestmark = pytest.mark.gpu

KW = dict(lr=1e-3, weight_decay=1e-2)
GUARD = 8            # elements on either side of a carved range: 32 B of fp32, 16 B of bf16 -- the range keeps its alignment
# one update: three roundings in ema - (1 - d) * (ema - p), at most four in the fp32 evaluation of 1 - d, |ema - p| <= 2 max:
# <= 13 * 2^-24 * max(|ema|, |p|), rounded up
EPS_UPDATE = 2.0 ** -20
EPS_DECAY = 2.0 ** -22
FORMS = [dict(), dict(use_ema_warmup=True, inv_gamma=1.0, power=2.0 / 3.0)]
COUNTS = [0, 1, 2, 7, 29999]
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 5]
TABLES = [(n,) for n in SIZES] + [(5, 4097, 1)]


# ---- helpers of the kernel tests ---------------------------------------------------------------------------------------------------
def _carve(n, seed, cuda, dtype=torch.float32):
    buf = torch.randn(n + 2 * GUARD, generator=torch.Generator().manual_seed(seed)).to(device=cuda, dtype=dtype)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD:GUARD + n]


def _same(a, b):
    """equal element by element, a NaN matching a NaN"""
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


class _Table:
    """items of sizes `ns`, each tensor carved from a guarded buffer of its own; shadows[i]: item i has a bf16 operand"""

    def __init__(self, ns, cuda, shadows=None, seed=0):
        from diffusion_pruning_amd import _lib
        lib = _lib.load()
        shadows = shadows if shadows is not None else [True] * len(ns)
        self.ns, self.bufs, self.p, self.ema, self.sh = ns, [], [], [], []
        items = (_lib.EmaItem * len(ns))()
        starts = [0]
        for i, n in enumerate(ns):
            pb, p = _carve(n, seed + 10 * i + 1, cuda)
            eb, e = _carve(n, seed + 10 * i + 2, cuda)
            self.bufs += [pb, eb]
            self.p.append(p)
            self.ema.append(e)
            items[i].p, items[i].ema, items[i].n = p.data_ptr(), e.data_ptr(), n
            if shadows[i]:
                sb, s = _carve(n, seed + 10 * i + 3, cuda, torch.bfloat16)
                assert s.data_ptr() % 8 == 0
                self.bufs.append(sb)
                self.sh.append(s)
                items[i].shadow = s.data_ptr()
            else:
                self.sh.append(None)
            starts.append(starts[-1] + lib.aptp_adamw_blocks(n))
        self.items = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(cuda)
        self.starts = torch.tensor(starts, dtype=torch.int32).to(cuda)
        self.total = starts[-1]
        self.count = torch.zeros((), dtype=torch.float32, device=cuda)
        self.cur = torch.full((), -1.0, dtype=torch.float32, device=cuda)

    def params(self, mode, gate=None, **kw):
        from diffusion_pruning_amd import _lib
        h = dict(M.DEFAULTS)
        h.update(kw)
        q = _lib.EmaParams()
        q.items_dev, q.starts_dev, q.n_items, q.total_blocks = self.items.data_ptr(), self.starts.data_ptr(), len(self.ns), self.total
        q.mode, q.count_dev, q.cur_decay_dev = mode, self.count.data_ptr(), self.cur.data_ptr()
        q.gate_dev = None if gate is None else gate.data_ptr()
        q.decay, q.min_decay, q.update_after_step = h["decay"], h["min_decay"], h["update_after_step"]
        q.use_warmup, q.inv_gamma, q.power = int(h["use_ema_warmup"]), h["inv_gamma"], h["power"]
        return q

    def run(self, mode, gate=None, **kw):
        from diffusion_pruning_amd import _lib, ops
        q = self.params(mode, gate, **kw)
        _lib.check(_lib.load().aptp_ema_many(ctypes.byref(q), ops._stream()), "aptp_ema_many")
        torch.cuda.synchronize()

    def snapshot(self):
        return [b.clone() for b in self.bufs] + [self.cur.clone(), self.count.clone()]

    def unchanged(self, snap):
        return all(_same(a, b) for a, b in zip(self.bufs + [self.cur, self.count], snap))


def _guards_intact(buf, buf0, n):
    return torch.equal(buf[:GUARD], buf0[:GUARD]) and torch.equal(buf[GUARD + n:], buf0[GUARD + n:])


# ---- 1. the kernel: UPDATE -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", TABLES, ids=lambda ns: "x".join(map(str, ns)))
def test_update_kernel_against_fp64_model(cuda, ns):
    from diffusion_pruning_amd import _lib
    for fi, form in enumerate(FORMS):
        for count in COUNTS:
            t = _Table(ns, cuda, seed=100 * fi + count % 97)
            t.count.fill_(float(count))
            snap = t.snapshot()
            p0 = [p.clone() for p in t.p]
            e0 = [e.double().cpu().numpy() for e in t.ema]
            s0 = [s.clone() for s in t.sh]
            t.run(_lib.EMA_UPDATE, **form)
            d_ref = M.ema_decay(count, **form)
            assert abs(float(t.cur) - d_ref) <= EPS_DECAY, (count, form, float(t.cur), d_ref)
            assert float(t.count) == float(count)                      # the caller counts
            for i, n in enumerate(ns):
                ref, _ = M.ema_update(e0[i], p0[i].double().cpu().numpy(), count, **form)
                got = t.ema[i].double().cpu().numpy()
                bound = EPS_UPDATE * np.maximum(np.abs(e0[i]), np.abs(p0[i].double().cpu().numpy()))
                worst = float(np.max(np.abs(got - ref) - bound))
                assert worst <= 0.0, (ns, i, count, form, worst)
                assert torch.equal(t.p[i], p0[i]) and torch.equal(t.sh[i], s0[i])          # p is read only, the shadow ignored
                if count == 0:
                    assert torch.equal(t.ema[i], p0[i])                # d = 0: the parameters, bit for bit
                else:
                    assert not torch.equal(t.ema[i], p0[i]) or n < 3
            k = 0
            for i, n in enumerate(ns):                                 # buffers: p, ema, shadow per item
                for _ in range(3):
                    assert _guards_intact(t.bufs[k], snap[k], n), (ns, i, count)
                    k += 1


@pytest.mark.parametrize("gate,applied", [(0.25, True), (-3.0e38, True), (3.2e38, True), (-3.2e38, True), (float("nan"), False),
                                          (float("inf"), False), (float("-inf"), False)])
def test_update_kernel_gate(cuda, gate, applied):
    from diffusion_pruning_amd import _lib
    t = _Table((5, 4097, 1), cuda, seed=7)
    t.count.fill_(2.0)
    g = torch.tensor(gate, dtype=torch.float32, device=cuda)
    snap = t.snapshot()
    e0 = [e.clone() for e in t.ema]
    t.run(_lib.EMA_UPDATE, gate=g)
    if applied:
        assert abs(float(t.cur) - 0.25) <= EPS_DECAY
        for i in range(3):
            ref, _ = M.ema_update(e0[i].double().cpu().numpy(), t.p[i].double().cpu().numpy(), 2)
            bound = EPS_UPDATE * np.maximum(np.abs(e0[i].double().cpu().numpy()), np.abs(t.p[i].double().cpu().numpy()))
            assert float(np.max(np.abs(t.ema[i].double().cpu().numpy() - ref) - bound)) <= 0.0
            assert not torch.equal(t.ema[i], e0[i])
    else:
        assert t.unchanged(snap) and float(t.cur) == -1.0              # averages, guards and the reported decay: untouched


# ---- 2. the kernel: SWAP -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,shadows", [((n,), [True]) for n in SIZES] + [((n,), [False]) for n in SIZES]
                         + [((5, 4097, 1), [True, False, True]), ((5, 4097, 1), [False, True, False])],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "".join("s" if s else "n" for s in v))
def test_swap_kernel(cuda, ns, shadows):
    from diffusion_pruning_amd import _lib
    t = _Table(ns, cuda, shadows=shadows, seed=3)
    for i, n in enumerate(ns):                            # non-finite values travel as they are
        t.p[i][0] = float("nan")
        t.ema[i][n // 2] = float("inf") if n > 1 else float("nan")
        if n > 2:
            t.ema[i][n - 1] = float("-inf")
            t.p[i][1] = float("-inf")
        if t.sh[i] is not None:
            t.sh[i].copy_(t.p[i])                         # the state a trainer is in: shadow = bf16(master)
    snap = t.snapshot()
    p0, e0 = [p.clone() for p in t.p], [e.clone() for e in t.ema]
    t.count.fill_(3.0)
    snap[-1].fill_(3.0)
    t.run(_lib.EMA_SWAP, gate=torch.tensor(float("nan"), device=cuda))          # ungated
    for i, n in enumerate(ns):
        assert _same(t.p[i], e0[i]) and _same(t.ema[i], p0[i]), (ns, i)
        if t.sh[i] is not None:
            assert _same(t.sh[i].float(), t.p[i].to(torch.bfloat16).float()), (ns, i)
    assert float(t.cur) == -1.0 and float(t.count) == 3.0               # no decay reported, no count
    k = 0
    for i, n in enumerate(ns):
        for _ in range(3 if shadows[i] else 2):
            assert _guards_intact(t.bufs[k], snap[k], n), (ns, i)
            k += 1
    t.run(_lib.EMA_SWAP)
    assert t.unchanged(snap)                              # two swaps: p, ema, shadow and every guard as at the start


# ---- 3. bad arguments ----------------------------------------------------------------------------------------------------------------
BAD = [("items_dev", None), ("starts_dev", None), ("n_items", 0), ("n_items", -1), ("mode", 2), ("mode", -1),
       ("decay", -0.1), ("decay", 1.5), ("decay", float("nan")), ("min_decay", -0.1), ("min_decay", 0.99995),
       ("update_after_step", -1), ("inv_gamma", 0.0), ("inv_gamma", -1.0), ("power", 0.0), ("power", -2.0)]


@pytest.mark.parametrize("mode", [0, 1])
def test_bad_arguments_launch_nothing(cuda, mode):
    from diffusion_pruning_amd import _lib, ops
    lib = _lib.load()
    t = _Table((5, 4097, 1), cuda, seed=5)
    t.count.fill_(2.0)
    snap = t.snapshot()
    for field, value in BAD:
        q = t.params(mode)
        setattr(q, field, value)
        with pytest.raises(_lib.AptpError):
            _lib.check(lib.aptp_ema_many(ctypes.byref(q), ops._stream()), "aptp_ema_many")
    with pytest.raises(_lib.AptpError):
        _lib.check(lib.aptp_ema_many(None, ops._stream()), "aptp_ema_many")
    torch.cuda.synchronize()
    assert t.unchanged(snap)
    t.run(mode)                                           # the unmodified parameters are accepted
    assert not t.unchanged(snap)


# ---- the tiny expert -------------------------------------------------------------------------------------------------------------------
def _build(cuda, mask):
    from diffusion_pruning_amd.unet import UNet2DConditionModelPruned
    cfg = O.TINY
    pm = UNet2DConditionModelPruned(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                    cross_attention_dim=cfg.cross_attention_dim).init_synthetic(seed=0)
    params = {k: v.detach().clone() for k, v in pm.state_dict().items()}
    pm.to(cuda)
    pm.prune({k: [v.clone().to(cuda) for v in vs] for k, vs in mask.items()})
    return cfg, pm, params


def _setup(cuda, seeds=(4, 5, 6, 7, 8), n_students=1):
    from diffusion_pruning_amd.train_step import synthetic_batch
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    mask = O.random_mask(O.TINY, 0.6, 9, n_depth_off=1)
    students = []
    for _ in range(n_students):
        cfg, s, params = _build(cuda, mask)
        students.append(s)
    teacher = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                        cross_attention_dim=cfg.cross_attention_dim)
    teacher.load_state_dict(params)
    teacher.to(cuda).freeze()
    teacher.set_structure({k: [v.to(cuda) for v in vs] for k, vs in O.ones_mask(cfg).items()})
    batches = [synthetic_batch(2, 16, cuda, seed=s, cross_dim=cfg.cross_attention_dim) for s in seeds]
    return students, teacher, batches


def _masters(step):
    """the packed masters by name, after the pending optimizer tail"""
    step.finish()
    return {n: p.detach().clone() for n, p in step.trainer.named_parameters()}


def _emas(step):
    step.finish()
    return [a.clone() for a in step.ema.ema]


def _operands(step):
    step.finish()
    return [e.pw.w.clone() for e in step.trainer.gemms.values()]


def _within_trajectory_bound(got, p0, masters, steps, what, **kw):
    """|got - fp64 EMA of `masters`| <= steps * 2^-20 * max|.| of the tensor: one update's bound per update, earlier error being
    scaled by d <= 1"""
    ref = M.ema_trajectory(p0.double().cpu().numpy(), [m.double().cpu().numpy() for m in masters], **kw)[-1]
    scale = max(float(np.abs(ref).max()), max(float(m.abs().max()) for m in masters), float(p0.abs().max()))
    err = float(np.abs(got.double().cpu().numpy() - ref).max())
    assert err <= steps * EPS_UPDATE * scale, (what, err, steps * EPS_UPDATE * scale)
    return err / max(scale, 1e-30)


# ---- 4. trajectory -------------------------------------------------------------------------------------------------------------------
def test_trajectory_against_fp64_model(cuda):
    from diffusion_pruning_amd.packed_train import PackedEMA
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    (sa,), teacher, batches = _setup(cuda)
    A = GraphedFineTunerStep(sa, teacher, ema=True, **KW)
    assert A.ema is None
    A.capture(batches[0])
    assert isinstance(A.ema, PackedEMA) and A.ema.steps() == 0 and not A.ema.swapped
    names = [n for n, _ in A.trainer.named_parameters()]
    assert sorted(A.ema.names) == sorted(names) and A.ema.n_elements() == A.trainer.n_trainable()
    start = _masters(A)
    assert all(torch.equal(a, start[n]) for n, a in zip(A.ema.names, A.ema.ema))       # clones of the masters
    assert all(a.data_ptr() != p.data_ptr() for a, p in zip(A.ema.ema, A.ema.params))
    seq = []
    for b in batches[:5]:
        out = A.train_step(None, b)
        assert torch.isfinite(out["loss"])
        seq.append(_masters(A))
    assert A.ema.steps() == 5 and float(A.optimizer.step_t) == 5.0
    assert abs(A.ema.cur_decay() - 5.0 / 14.0) <= EPS_DECAY
    worst, lagging = 0.0, 0
    for n, a in zip(A.ema.names, _emas(A)):
        worst = max(worst, _within_trajectory_bound(a, start[n], [s[n] for s in seq], 5, n))
        lagging += not torch.equal(a, seq[-1][n])
    assert lagging >= len(names) // 2                                                   # averages, not the last masters
    print("EMA trajectory, 5 steps: worst error / max|.| = %.3e (bound %.3e)" % (worst, 5 * EPS_UPDATE))


# ---- 5. the EMA does not disturb training --------------------------------------------------------------------------------------------
def test_ema_does_not_disturb_training(cuda):
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    (sa, sb), teacher, batches = _setup(cuda, n_students=2)
    A = GraphedFineTunerStep(sa, teacher, ema=True, **KW).capture(batches[0])
    B = GraphedFineTunerStep(sb, teacher, **KW).capture(batches[0])
    for b in batches[:4]:
        la, lb = A.train_step(None, b), B.train_step(None, b)
        assert torch.equal(la["loss"], lb["loss"])
    torch.cuda.synchronize()
    assert A.ema.steps() == 4 and B.ema is None
    assert float(A.optimizer.step_t) == float(B.optimizer.step_t) == 4.0
    for pa, pb in zip(A.trainer.parameters(), B.trainer.parameters()):
        assert torch.equal(pa.detach(), pb.detach())
    for x, y in zip(A.optimizer.m + A.optimizer.v + _operands(A), B.optimizer.m + B.optimizer.v + _operands(B)):
        assert torch.equal(x, y)
    for ea, eb in zip(A.trainer.gemms.values(), B.trainer.gemms.values()):
        assert (ea.pwb is None) == (eb.pwb is None) and (ea.pwb is None or torch.equal(ea.pwb.w, eb.pwb.w))


# ---- 6. accumulation and NaN ---------------------------------------------------------------------------------------------------------
def test_accumulation_and_nan_window(cuda):
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    form = dict(use_ema_warmup=True, inv_gamma=2.0, power=0.75, decay=0.999)
    (sa,), teacher, batches = _setup(cuda, seeds=(4, 5, 6, 7, 8, 9, 10, 11))
    A = GraphedFineTunerStep(sa, teacher, accumulation_steps=2, ema=form, **KW).capture(batches[0])
    assert A.ema.use_ema_warmup and A.ema.inv_gamma == 2.0 and A.ema.power == 0.75 and A.ema.decay == 0.999
    prev, changed = _emas(A), []
    for b in batches[:4]:
        out = A.train_step(None, b)
        cur = _emas(A)
        changed.append(not all(torch.equal(x, y) for x, y in zip(cur, prev)))
        assert changed[-1] is out["applied"]
        prev = cur
    assert changed == [False, True, False, True] and A.ema.steps() == 2
    assert abs(A.ema.cur_decay() - M.ema_decay(1, **form)) <= EPS_DECAY
    # a NaN in the first micro-batch of a window: averages, decay and count keep their bits across it
    window = [{k: v.clone() for k, v in b.items()} for b in batches[4:6]]
    window[0]["target"][0, 0, 0, 0] = float("nan")
    d0 = A.ema.cur_decay()
    outs = [A.train_step(None, b) for b in window]
    assert outs[1]["applied"] is True and not torch.isfinite(outs[0]["loss"])
    assert all(torch.equal(x, y) for x, y in zip(_emas(A), prev))
    assert A.ema.steps() == 2 and A.ema.cur_decay() == d0 and float(A.optimizer.step_t) == 2.0
    for b in batches[6:8]:
        A.train_step(None, b)
    cur = _emas(A)
    assert A.ema.steps() == 3 and float(A.optimizer.step_t) == 3.0
    assert abs(A.ema.cur_decay() - M.ema_decay(2, **form)) <= EPS_DECAY
    assert sum(not torch.equal(x, y) for x, y in zip(cur, prev)) >= len(cur) // 2
    assert all(torch.isfinite(x).all() for x in cur)


# ---- 7. swap on the real state -------------------------------------------------------------------------------------------------------
def test_swap_on_the_trained_state(cuda):
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    (sa,), teacher, batches = _setup(cuda)
    A = GraphedFineTunerStep(sa, teacher, ema=True, **KW).capture(batches[0])
    for b in batches[:3]:
        A.train_step(None, b)
    masters, emas, ops0 = _masters(A), _emas(A), _operands(A)
    dgrad0 = [e.pwb.w.clone() for e in A.trainer.gemms.values() if e.pwb is not None]
    assert sum(not torch.equal(a, masters[n]) for n, a in zip(A.ema.names, emas)) >= len(emas) // 2
    A.ema.swap_()
    assert A.ema.swapped
    torch.cuda.synchronize()
    now = {n: p.detach() for n, p in A.trainer.named_parameters()}
    for n, a0, a in zip(A.ema.names, emas, A.ema.ema):
        assert torch.equal(now[n], a0) and torch.equal(a, masters[n]), n          # weights, biases and affines alike
    for e in A.trainer.gemms.values():
        assert torch.equal(e.pw.w, e.P.detach().to(torch.bfloat16))
        assert e.Pb is None or e.pw.bias.data_ptr() == e.Pb.data_ptr()             # (the kernels read the swapped bias in place)
    with pytest.raises(RuntimeError, match="EMA"):
        A.train_step(None, batches[3])
    with pytest.raises(AssertionError):
        A.ema.state_dict()
    with pytest.raises(AssertionError):
        A.ema.load_state_dict({})
    A.ema.swap_()
    assert not A.ema.swapped
    torch.cuda.synchronize()
    back = _masters(A)
    assert all(torch.equal(back[n], masters[n]) for n in masters)
    assert all(torch.equal(x, y) for x, y in zip(_emas(A) + _operands(A), emas + ops0))
    assert all(torch.equal(x, y) for x, y in zip([e.pwb.w for e in A.trainer.gemms.values() if e.pwb is not None], dgrad0))
    with A.ema.applied() as e:
        assert e is A.ema and A.ema.swapped
    assert not A.ema.swapped
    out = A.train_step(None, batches[3])                                          # training goes on
    assert torch.isfinite(out["loss"]) and A.ema.steps() == 4


# ---- 8. validation of the averaged weights -------------------------------------------------------------------------------------------
def test_validation_with_the_average(cuda):
    from diffusion_pruning_amd import graph_utils
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep, synthetic_batch
    (sa,), teacher, batches = _setup(cuda)
    A = GraphedFineTunerStep(sa, teacher, ema=True, **KW).capture(batches[0])
    for b in batches[:3]:
        A.train_step(None, b)
    val = [synthetic_batch(2, 16, cuda, seed=s, cross_dim=O.TINY.cross_attention_dim) for s in (31, 32)]
    graph_utils.KEEP_GRAPHS = True
    try:
        A.capture_validation(val[0])
    finally:
        graph_utils.KEEP_GRAPHS = False
    nodes, graphs = A.validation_graph_nodes(), {B: id(c["g_student"]) for B, c in A._val.items()}
    before = (_masters(A), _emas(A), _operands(A), [m.clone() for m in A.optimizer.m + A.optimizer.v], float(A.optimizer.step_t))
    plain = A.validate(val)
    got = A.validate(val, use_ema=True)
    assert not A.ema.swapped
    A.ema.swap_()
    want = A.validate(val)
    one_want = A.eval_step_graphed(val[1])
    A.ema.swap_()
    one = A.eval_step_graphed(val[1], use_ema=True)
    assert got == want and got != plain and all(np.isfinite(v) for v in got.values())
    assert all(torch.equal(one[k], one_want[k]) for k in one)
    assert A.validate(val) == plain                                     # and the trained weights score as before
    after = (_masters(A), _emas(A), _operands(A), [m.clone() for m in A.optimizer.m + A.optimizer.v], float(A.optimizer.step_t))
    assert all(torch.equal(before[0][n], after[0][n]) for n in before[0])
    assert all(torch.equal(x, y) for i in (1, 2, 3) for x, y in zip(before[i], after[i])) and before[4] == after[4]
    assert A.validation_graph_nodes() == nodes and {B: id(c["g_student"]) for B, c in A._val.items()} == graphs
    assert A.ema.steps() == 3
    # a failure inside the pass still swaps back
    with pytest.raises(KeyError):
        A.validate([{"noisy_latents": val[0]["noisy_latents"]}], use_ema=True)
    assert not A.ema.swapped and all(torch.equal(before[0][n], p) for n, p in _masters(A).items())


# ---- 9. checkpoint -------------------------------------------------------------------------------------------------------------------
def _exported(step):
    model = step.trainer.export_()
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_export_and_resume(cuda, tmp_path):
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    (sa, sb), teacher, batches = _setup(cuda, n_students=2)
    A = GraphedFineTunerStep(sa, teacher, ema=True, **KW).capture(batches[0])
    start = _exported(A)
    seq = []
    for b in batches[:3]:
        A.train_step(None, b)
        seq.append(_exported(A))
    model = A.export_ema_()
    assert model is sa and not A.ema.swapped
    # (named_parameters: under the attached trainer model.state_dict() would export the packed state -- the trained weights -- first)
    ema_sd = {k: v.detach().clone() for k, v in model.named_parameters()}
    assert set(ema_sd) == set(start)
    moved = 0
    for k, v in ema_sd.items():
        _within_trajectory_bound(v, start[k], [s[k] for s in seq], 3, k)
        moved += not torch.equal(v, seq[-1][k])
    assert moved >= len(ema_sd) // 4                                     # (a dropped block's tensors never train)
    again = _exported(A)                                                 # a plain export_: the trained weights, as before the call
    assert all(torch.equal(again[k], seq[-1][k]) for k in again)
    # the same through the checkpoint writer: <root>/unet_ema holds the average, <root>/unet the trained weights
    from safetensors.torch import load_file
    from diffusion_pruning_amd import checkpoint
    d_ema = A.save_ema_pretrained(str(tmp_path))
    d_unet = checkpoint.save_pretrained(sa, str(tmp_path))
    assert d_ema.endswith("unet_ema") and d_unet.endswith("unet") and (tmp_path / checkpoint.ARCH_VECTOR_NAME).exists()
    assert not A.ema.swapped and all(torch.equal(v, seq[-1][k]) for k, v in sa.named_parameters())
    f_ema, f_unet = load_file(d_ema + "/" + checkpoint.WEIGHTS_NAME), load_file(d_unet + "/" + checkpoint.WEIGHTS_NAME)
    assert set(f_ema) == set(f_unet) and sum(not torch.equal(f_ema[k], f_unet[k]) for k in f_ema) >= len(f_ema) // 4
    whole = [k for k in f_ema if k in ema_sd and f_ema[k].shape == ema_sd[k].shape]      # tensors the pruning does not slice
    assert len(whole) >= 4 and all(torch.equal(f_ema[k], ema_sd[k].cpu()) and torch.equal(f_unet[k], seq[-1][k].cpu()) for k in whole)
    # resume: a fresh step takes the masters, the optimizer state and the EMA state; one more step on each
    B = GraphedFineTunerStep(sb, teacher, ema=True, **KW).capture(batches[0])
    A.finish()
    for pa, pb in zip(A.trainer.parameters(), B.trainer.parameters()):
        pb.data.copy_(pa.detach())
    B.trainer.refresh_()
    B.optimizer.load_state_dict(A.optimizer.state_dict())
    sd = A.ema.state_dict()
    assert sorted(sd["names"]) == sorted(n for n, _ in A.trainer.named_parameters()) and float(sd["count"]) == 3.0
    ptrs = [a.data_ptr() for a in B.ema.ema]
    B.ema.load_state_dict({**sd, "names": sd["names"][::-1], "ema": sd["ema"][::-1]})      # matched by name, whatever the order
    assert ptrs == [a.data_ptr() for a in B.ema.ema] and B.ema.steps() == 3
    with pytest.raises(AssertionError, match="another expert"):
        B.ema.load_state_dict({**sd, "names": sd["names"][:-1] + ["nope"]})
    with pytest.raises(AssertionError, match="saved average"):
        B.ema.load_state_dict({**sd, "ema": [sd["ema"][0].reshape(-1)[:1]] + sd["ema"][1:]})
    ea0 = _emas(A)
    A.train_step(None, batches[3])
    B.train_step(None, batches[3])
    ea, eb = _emas(A), _emas(B)
    assert A.ema.steps() == B.ema.steps() == 4 and A.ema.cur_decay() == B.ema.cur_decay()
    assert all(torch.equal(x, y) for x, y in zip(ea, eb))
    assert sum(not torch.equal(x, y) for x, y in zip(ea, ea0)) >= len(ea) // 2


# ---- 10. the defaults take none of the new paths -------------------------------------------------------------------------------------
def test_defaults_are_untouched(cuda):
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    (sa, sb), teacher, batches = _setup(cuda, n_students=2)
    X = GraphedFineTunerStep(sa, teacher, ema=None, **KW).capture(batches[0])
    Y = GraphedFineTunerStep(sb, teacher, **KW).capture(batches[0])
    assert X.ema is None and Y.ema is None
    logs = []
    for step in (X, Y):
        ops.LAUNCH_LOG = []
        try:
            outs = [step.train_step(None, b) for b in batches[:3]]
            torch.cuda.synchronize()
            logs.append((len(ops.LAUNCH_LOG), outs))
        finally:
            ops.LAUNCH_LOG = None
    assert logs[0][0] == logs[1][0]
    for ox, oy in zip(logs[0][1], logs[1][1]):
        assert set(ox) == set(oy) == {"loss", "diff_loss", "distillation_loss", "block_loss", "applied", "accum_index"}
        assert all(torch.equal(ox[k], oy[k]) if torch.is_tensor(ox[k]) else ox[k] == oy[k] for k in ox)
    for px, py in zip(X.trainer.parameters(), Y.trainer.parameters()):
        assert torch.equal(px.detach(), py.detach())
    with pytest.raises(AssertionError, match="ema"):
        X.validate(batches[:1], use_ema=True)
    with pytest.raises(AssertionError, match="ema"):
        X.export_ema_()
