"""GPU checks of the block-wise 8-bit AdamW state: csrc/optim8.hip (aptp_adamw8_many) against the fp64 model of
tests/adamw8_model.py run on the SAME old codes, packed_train.PackedAdamW(optim_bits=8), and its place in
train_step.GraphedFineTunerStep(use_8bit_adam=True).  Tiny expert (O.TINY), 16x16 latents, micro-batches of 2, lr = 1e-3 -- the
setting of tests/test_ema_gpu.py.

Starting states of the kernel tests are random codes with positive random scales, so the old moments are known exactly; they
are states an optimizer can have produced: per block absmax_v = absmax_m^2 and every second-moment code stands for at least
the square of the first moment's value, so m^2 <= v before the step and |m| / sqrt(v) <= 10 after it (the update stays a small
fraction of |p|, as in training, and the margin on p -- relative to max |p| -- keeps its meaning).

(The file is named after csrc/optim8.hip.  The name once mattered: it sorts after the other captured-step tests because every
GraphedFineTunerStep takes split-K counter slabs for its streams, the pool was fixed at 16, and tests/test_clip_score_gpu.py
compares an eager run with a replay bit for bit, which needs a slab for both.  The pool grows now, scratch.py, and the order of
the files no longer decides a launch's form.)"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import unet_oracle as O
from tests import adamw8_model as M
from tests import ema_model as EM
from tests import margins

pytestmark = pytest.mark.gpu

KW = dict(lr=1e-3, weight_decay=1e-2)
GUARD = 16           # elements on either side of a carved range: the range keeps a 16-byte alignment in every element type
# fp32 roundings behind a stored moment, each <= 2^-24 relative to a term no larger than the block's absmax in these tests:
# first moment -- g * gscale (two when gscale is itself a product), 1 - beta1, two products, the sum: <= 6; second moment -- the
# error of g * gscale counts twice, 1 - beta2, three products, the sum: <= 8; then the reciprocal of absmax and the product by
# it: + 2.  <= 10 * 2^-24, rounded up to a power of two
EPS = 2.0 ** -20
HYPER = dict(lr=float(np.float32(1e-3)), beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)), eps=float(np.float32(1e-8)),
             weight_decay=float(np.float32(1e-2)))
STEPS = [0, 1, 7, 29999]
SIZES = [4096, 4097, 4099, 4096 + 255, 4096 + 256, 4096 + 257, 2 * 4096 + 5]
TABLE = (4097, 8192, 4100)
CASES = [((n,), (True,)) for n in SIZES] + [(TABLE, (True, True, True)), (TABLE, (False, False, False))]


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v[0], int) and not isinstance(v[0], bool) else "".join("s" if s else "n" for s in v)


# ---- the checker: assertions 1-4 of one step ------------------------------------------------------------------------------------------
def check_step(old, new, g, step, what, hyper=None, grad_scale=1.0, warmup_steps=0):
    """old, new: dicts of numpy arrays p (fp32), m8, v8 (uint8), absmax_m, absmax_v (fp32), shadow (bf16 bits as fp32, or None)
    before and after one step on gradient g: the fp64 model on the old codes against what the kernel left"""
    ref = M.step(old["p"].astype(np.float64), g.astype(np.float64), old["m8"], old["v8"], old["absmax_m"].astype(np.float64),
                 old["absmax_v"].astype(np.float64), step, grad_scale=grad_scale, warmup_steps=warmup_steps, **(hyper or HYPER))
    n = old["p"].size
    ok = np.isfinite(ref["p"])
    # 1. parameters
    assert np.array_equal(np.isnan(new["p"]), ~ok), what
    tol = 1e-6 * float(np.abs(ref["p"][ok]).max()) + 1e-7
    err = float(np.abs(new["p"].astype(np.float64)[ok] - ref["p"][ok]).max())
    print("%s: p error %.3e (margin %.3e)" % (what, err, tol))
    assert err <= tol, (what, err, tol)
    for name, qmap, c8, mom, zero in (("m", M.MAP_SIGNED, "m8", "m", M.ZERO_SIGNED), ("v", M.MAP_UNSIGNED, "v8", "v", M.ZERO_UNSIGNED)):
        a_ref, a = ref["absmax_" + name], new["absmax_" + name].astype(np.float64)
        bad = np.isnan(a_ref)                                      # poisoned blocks: a NaN scale, codes mean nothing
        assert np.array_equal(np.isnan(a), bad), (what, name)
        # 3. scales
        assert np.all(np.abs(a - a_ref)[~bad] <= EPS * a_ref[~bad]), (what, name, float(np.max((np.abs(a - a_ref) / np.maximum(a_ref, 1e-300))[~bad])))
        assert np.all(a[a_ref == 0.0] == 0.0), (what, name)
        # 4. codes: nearest-code rounding plus fp32 slack, either side of a tie
        live = np.repeat(~bad & (a_ref > 0), M.BLOCK)[:n]
        a_e, ar_e = np.repeat(a, M.BLOCK)[:n][live], np.repeat(a_ref, M.BLOCK)[:n][live]
        x_ref = ref[mom][live] / ar_e
        got = qmap.astype(np.float64)[new[c8][live]] * a_e
        bound = ar_e * (M.nearest_distance(qmap, x_ref) + 2 * EPS) + np.abs(a_e - ar_e)
        worst = float(np.max(np.abs(got - ref[mom][live]) - bound)) if live.any() else 0.0
        assert worst <= 0.0, (what, name, worst)
        dead = np.repeat(a_ref == 0.0, M.BLOCK)[:n]
        assert np.all(new[c8][dead] == zero), (what, name)
    return ref


# ---- helpers of the kernel tests ---------------------------------------------------------------------------------------------------
def _carve(values, cuda, dtype):
    """`values` (numpy) inside a buffer with GUARD elements of a pattern on either side"""
    n = values.size
    if dtype == torch.uint8:
        buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=dtype)
    else:
        buf = torch.full((n + 2 * GUARD,), -7.25, dtype=dtype)
    buf[GUARD:GUARD + n] = torch.from_numpy(values).to(dtype)
    buf = buf.to(cuda)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD:GUARD + n]


def _same(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all()) if a.is_floating_point() else torch.equal(a, b)


def random_state(n, rng):
    """(m8, v8, absmax_m, absmax_v) as the module docstring describes; block 1 is the untouched state (zero codes, zero scales)"""
    nb = M.n_blocks(n)
    am = rng.uniform(0.5e-2, 1.5e-2, nb).astype(np.float32)
    av = (am.astype(np.float64) ** 2).astype(np.float32)
    m8 = rng.integers(0, 256, n).astype(np.uint8)
    x2 = M.MAP_SIGNED.astype(np.float64)[m8] ** 2 * np.repeat(am.astype(np.float64) ** 2 / av.astype(np.float64), M.BLOCK)[:n]
    floor = np.minimum(np.searchsorted(M.MAP_UNSIGNED.astype(np.float64), x2), 255)
    v8 = np.maximum(rng.integers(0, 256, n), floor).astype(np.uint8)
    sl = slice(M.BLOCK, 2 * M.BLOCK)
    m8[sl], v8[sl], am[1], av[1] = M.ZERO_SIGNED, M.ZERO_UNSIGNED, 0.0, 0.0
    return m8, v8, am, av


def classed_gradient(n, rng):
    """block 0: ordinary; block 1: zero (over zero state); block 2: dwarfs the state; block 3: dwarfed by it; the rest ordinary"""
    g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    g[M.BLOCK:2 * M.BLOCK] = 0.0
    g[2 * M.BLOCK:3 * M.BLOCK] *= 1e4
    g[3 * M.BLOCK:4 * M.BLOCK] *= 1e-6
    return g


class _Table:
    """items of sizes `ns`, every array carved from a guarded buffer of its own; shadows[i]: item i has a bf16 operand"""
    KEYS = ("p", "g", "m8", "v8", "absmax_m", "absmax_v", "shadow")

    def __init__(self, ns, cuda, shadows=None, seed=0):
        from diffusion_pruning_amd import _lib
        lib = _lib.load()
        rng = np.random.default_rng(seed)
        shadows = shadows if shadows is not None else [True] * len(ns)
        self.ns, self.bufs, self.t = ns, [], []
        self.host = (_lib.AdamW8Item * len(ns))()
        starts = [0]
        for i, n in enumerate(ns):
            m8, v8, am, av = random_state(n, rng)
            arrays = dict(p=(rng.standard_normal(n).astype(np.float32), torch.float32), g=(classed_gradient(n, rng), torch.float32),
                          m8=(m8, torch.uint8), v8=(v8, torch.uint8), absmax_m=(am, torch.float32), absmax_v=(av, torch.float32))
            if shadows[i]:
                arrays["shadow"] = (rng.standard_normal(n).astype(np.float32), torch.bfloat16)
            t = {}
            for k, (vals, dt) in arrays.items():
                buf, t[k] = _carve(vals, cuda, dt)
                self.bufs.append((buf, vals.size))
            t.setdefault("shadow", None)
            self.t.append(t)
            it = self.host[i]
            it.p, it.g, it.m8, it.v8, it.n = t["p"].data_ptr(), t["g"].data_ptr(), t["m8"].data_ptr(), t["v8"].data_ptr(), n
            it.absmax_m, it.absmax_v = t["absmax_m"].data_ptr(), t["absmax_v"].data_ptr()
            it.shadow = None if t["shadow"] is None else t["shadow"].data_ptr()
            starts.append(starts[-1] + lib.aptp_adamw8_blocks(n))
        self.items = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(cuda)
        self.starts = torch.tensor(starts, dtype=torch.int32).to(cuda)
        self.total = starts[-1]
        self.step = torch.zeros((), dtype=torch.float32, device=cuda)
        self.qs, self.qu = torch.from_numpy(M.MAP_SIGNED).to(cuda), torch.from_numpy(M.MAP_UNSIGNED).to(cuda)

    def params(self, gate=None, grad_scale=1.0, warmup_steps=0.0):
        from diffusion_pruning_amd import _lib
        q = _lib.AdamW8Params()
        q.items_dev, q.starts_dev, q.n_items, q.total_blocks = self.items.data_ptr(), self.starts.data_ptr(), len(self.ns), self.total
        q.lr, q.beta1, q.beta2, q.eps, q.weight_decay = HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["weight_decay"]
        q.step_dev = self.step.data_ptr()
        q.gate_dev = None if gate is None else gate.data_ptr()
        q.grad_scale, q.warmup_steps = grad_scale, warmup_steps
        q.qmap_signed_dev, q.qmap_unsigned_dev = self.qs.data_ptr(), self.qu.data_ptr()
        q.items_host = ctypes.cast(self.host, ctypes.c_void_p)
        return q

    def run(self, gate=None, grad_scale=1.0, grad_scale_dev=None, warmup_steps=0.0):
        from diffusion_pruning_amd import _lib, ops
        q = self.params(gate, grad_scale, warmup_steps)
        _lib.check(_lib.load().aptp_adamw8_many(ctypes.byref(q), None if grad_scale_dev is None else grad_scale_dev.data_ptr(),
                                                ops._stream()), "aptp_adamw8_many")
        torch.cuda.synchronize()

    def host_state(self, i):
        t = self.t[i]
        return {k: (None if t[k] is None else t[k].float().cpu().numpy() if k == "shadow" else t[k].cpu().numpy()) for k in self.KEYS}

    def snapshot(self):
        return [b.clone() for b, _ in self.bufs] + [self.step.clone()]

    def unchanged(self, snap):
        return all(_same(a, b) for a, b in zip([b for b, _ in self.bufs] + [self.step], snap))

    def guards_intact(self, snap):
        return all(torch.equal(b[:GUARD], s[:GUARD]) and torch.equal(b[GUARD + n:], s[GUARD + n:]) for (b, n), s in zip(self.bufs, snap))

    def check(self, olds, step, what, **kw):
        for i in range(len(self.ns)):
            new = self.host_state(i)
            check_step(olds[i], new, olds[i]["g"], step, "%s item %d" % (what, i), **kw)
            assert np.array_equal(new["g"], olds[i]["g"], equal_nan=True)                      # the gradient is read only
            if new["shadow"] is not None:                                                       # 2. operand = bf16 of the kernel's own p
                assert _same(self.t[i]["shadow"], self.t[i]["p"].to(torch.bfloat16)), (what, i)


# ---- 1-4. one step against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,shadows", CASES, ids=_ids)
def test_kernel_step_against_fp64_model(cuda, ns, shadows):
    for step in STEPS:
        t = _Table(ns, cuda, shadows=shadows, seed=step % 97 + len(ns))
        t.step.fill_(float(step))
        snap = t.snapshot()
        olds = [t.host_state(i) for i in range(len(ns))]
        t.run()
        assert float(t.step) == float(step)                            # the caller counts
        t.check(olds, step, "%s step %d" % (ns, step))
        assert t.guards_intact(snap), (ns, step)
        assert not t.unchanged(snap)


def test_kernel_warmup_rate(cuda):
    t = _Table(TABLE, cuda, seed=11)
    t.step.fill_(3.0)
    olds = [t.host_state(i) for i in range(3)]
    t.run(warmup_steps=8.0)
    t.check(olds, 3, "warm-up 3/8", warmup_steps=8)


# ---- 5. gates and factors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate,applied", [(float("nan"), False), (float("inf"), False), (3.4e38, True)])
def test_kernel_gate(cuda, gate, applied):
    t = _Table(TABLE, cuda, seed=5)
    t.step.fill_(2.0)
    snap = t.snapshot()
    olds = [t.host_state(i) for i in range(3)]
    t.run(gate=torch.tensor(gate, dtype=torch.float32, device=cuda))
    if applied:
        t.check(olds, 2, "gate %g" % gate)
        assert t.guards_intact(snap)
    else:
        assert t.unchanged(snap)


def test_kernel_grad_scale_factors_multiply(cuda):
    t = _Table(TABLE, cuda, seed=6)
    t.step.fill_(7.0)
    snap = t.snapshot()
    olds = [t.host_state(i) for i in range(3)]
    s, c = 0.3, 0.7
    t.run(grad_scale=s, grad_scale_dev=torch.tensor(c, dtype=torch.float32, device=cuda))
    t.check(olds, 7, "grad_scale", grad_scale=float(np.float32(s) * np.float32(c)))
    assert t.guards_intact(snap)


# ---- 6. determinism --------------------------------------------------------------------------------------------------------------------
def test_kernel_is_deterministic(cuda):
    outs = []
    for _ in range(2):
        t = _Table(TABLE, cuda, shadows=[True, False, True], seed=8)
        t.step.fill_(4.0)
        t.run()
        outs.append(t.snapshot())
    assert all(_same(a, b) for a, b in zip(*outs))


# ---- 7. a NaN gradient ---------------------------------------------------------------------------------------------------------------
def test_kernel_nan_gradient_poisons_its_block_only(cuda):
    t = _Table(TABLE, cuda, seed=9)
    t.step.fill_(1.0)
    where = [4096, 4096 + 3, 5 * M.BLOCK + 17]                         # the scalar tail, the second workgroup, a whole quad
    for i, x in enumerate(where):
        t.t[i]["g"][x] = float("nan")
    snap = t.snapshot()
    olds = [t.host_state(i) for i in range(3)]
    t.run(gate=torch.tensor(1.0, dtype=torch.float32, device=cuda))
    t.check(olds, 1, "NaN gradient")                                   # every other block within bounds, the poisoned ones NaN
    for i, x in enumerate(where):
        new = t.host_state(i)
        assert np.isnan(new["p"][x]) and int(np.isnan(new["p"]).sum()) == 1
        for k in ("absmax_m", "absmax_v"):
            assert np.isnan(new[k][x // M.BLOCK]) and int(np.isnan(new[k]).sum()) == 1
    assert t.guards_intact(snap)


# ---- 8. PackedAdamW(optim_bits=8) over a fake trainer --------------------------------------------------------------------------------
SHAPES = [(64, 9, 72), (8, 1, 8), (1283,), (5,), (4096 * 3 + 7,)]
OPT = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
OPT_HYPER = dict(lr=float(np.float32(1e-2)), beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)), eps=float(np.float32(1e-8)),
                 weight_decay=float(np.float32(1e-2)))


def _fake_trainer(cuda, seed=21):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g).to(cuda)) for s in SHAPES]
    shadows = [torch.zeros(s, dtype=torch.bfloat16, device=cuda) for s in SHAPES[:2]]
    gemms = {0: SimpleNamespace(P=ps[0], Pb=ps[2], pw=SimpleNamespace(w=shadows[0])),
             1: SimpleNamespace(P=ps[1], Pb=None, pw=SimpleNamespace(w=shadows[1]))}
    affines = {0: SimpleNamespace(Pg=ps[3], Pb=ps[4])}
    trainer = SimpleNamespace(gemms=gemms, affines=affines, refresh_=lambda shadows_done=False: None)
    for p in ps:
        p.grad = torch.zeros_like(p)
    return trainer, ps, shadows


def _feed(ps_list, seed, cuda):
    g = torch.Generator().manual_seed(seed)
    for k in range(len(ps_list[0])):
        gr = (torch.randn(ps_list[0][k].shape, generator=g) * 1e-2).to(cuda)
        for ps in ps_list:
            ps[k].grad.copy_(gr)                          # in place: the addresses are part of the kernels' tables


def _opt_state(opt):
    torch.cuda.synchronize()
    return [p.detach().clone() for p in opt.params] + [t.clone() for t in opt.m + opt.v] + \
        [a.clone() for a in opt.absmax1 + opt.absmax2 if a is not None] + [opt.step_t.clone()]


def _equal_states(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and _same(x, y) for x, y in zip(a, b))


def _host8(opt, i, shadow=None):
    return dict(p=opt.params[i].detach().reshape(-1).cpu().numpy(), m8=opt.m[i].cpu().numpy(), v8=opt.v[i].cpu().numpy(),
                absmax_m=opt.absmax1[i].cpu().numpy(), absmax_v=opt.absmax2[i].cpu().numpy(), shadow=shadow)


def test_packed_adamw_8bit(cuda):
    from diffusion_pruning_amd.packed_train import PackedAdamW, adam_state_bytes
    (tr8, ps8, sh8), (tr32, ps32, sh32), (trg, psg, shg) = _fake_trainer(cuda), _fake_trainer(cuda), _fake_trainer(cuda)
    opt = PackedAdamW(tr8, optim_bits=8, **OPT)
    ref32 = PackedAdamW(tr32, optim_bits=32, **OPT)
    grouped = PackedAdamW(trg, optim_bits=8, group_of=lambda p: 0 if p.numel() in (64 * 9 * 72, 1283) else 1, **OPT)
    # partition: two 8-bit tensors, three fp32 ones
    assert opt.is8 == [True, False, False, False, True] and opt.params[0] is ps8[0] and opt.params[4] is ps8[4]
    assert opt.table8.n == 2 and opt.table.n == 3 and ref32.table8 is None and ref32.table.n == 5 and ref32.qmap1 is None
    assert all((m.dtype == torch.uint8) == q for m, q in zip(opt.m, opt.is8)) and all(bool((m == 127).all()) for m, q in zip(opt.m, opt.is8) if q)
    sizes = [p.numel() for p in opt.params]
    assert opt.state_bytes() == adam_state_bytes(sizes, 8) and ref32.state_bytes() == adam_state_bytes(sizes, 32) == 8 * sum(sizes)
    i8 = [i for i, q in enumerate(opt.is8) if q]
    i32 = [i for i, q in enumerate(opt.is8) if not q]
    for it in range(4):
        _feed([ps8, ps32, psg], 100 + it, cuda)
        olds = {i: _host8(opt, i) for i in i8}
        opt.step()
        ref32.step()
        for gi in (1, 0):
            grouped.step_group(gi)
        grouped.finish_step()
        torch.cuda.synchronize()
        for i in i8:                                      # the model, restarted from the GPU's codes
            check_step(olds[i], _host8(opt, i), opt.params[i].grad.reshape(-1).cpu().numpy(), it, "PackedAdamW step %d tensor %d" % (it, i),
                       hyper=OPT_HYPER)
        for i in i32:                                     # the same kernel, the same bits
            assert torch.equal(opt.params[i].detach(), ref32.params[i].detach()), (it, i)
            assert torch.equal(opt.m[i], ref32.m[i]) and torch.equal(opt.v[i], ref32.v[i]), (it, i)
        assert _equal_states(_opt_state(opt), _opt_state(grouped)), it
    assert float(opt.step_t) == 4.0
    assert torch.equal(sh8[0], ps8[0].detach().to(torch.bfloat16)) and torch.equal(sh8[1], ps8[1].detach().to(torch.bfloat16))
    assert torch.equal(shg[0], sh8[0]) and torch.equal(shg[1], sh8[1])
    # a non-finite gate: nothing moves, the count included; a finite one just below FLT_MAX applies the step
    _feed([ps8], 300, cuda)
    before = _opt_state(opt) + [s.clone() for s in sh8]
    for bad in (float("nan"), float("inf")):
        opt.step(gate=torch.tensor(bad, dtype=torch.float32, device=cuda))
        assert _equal_states(_opt_state(opt) + list(sh8), before)
    # dequantized_state: map[codes] * scale, computed on the CPU
    dq = opt.dequantized_state()
    assert dq["names"] == opt.names and sorted(dq["state"]) == list(range(5))
    for i in range(5):
        st = dq["state"][i]
        assert st["exp_avg"].shape == opt.params[i].shape and st["exp_avg"].dtype == torch.float32 and float(st["step"]) == 4.0
        if opt.is8[i]:
            n = opt.params[i].numel()
            m = M.MAP_SIGNED[opt.m[i].cpu().numpy()] * np.repeat(opt.absmax1[i].cpu().numpy(), M.BLOCK)[:n]
            v = M.MAP_UNSIGNED[opt.v[i].cpu().numpy()] * np.repeat(opt.absmax2[i].cpu().numpy(), M.BLOCK)[:n]
            assert np.array_equal(st["exp_avg"].reshape(-1).cpu().numpy(), m) and np.array_equal(st["exp_avg_sq"].reshape(-1).cpu().numpy(), v)
            assert float(st["exp_avg"].abs().max()) > 0 and float(st["exp_avg_sq"].max()) > 0
        else:
            assert torch.equal(st["exp_avg"], opt.m[i]) and torch.equal(st["exp_avg_sq"], opt.v[i])
    # save, build a fresh optimizer, load, step: the uninterrupted step, bit for bit
    sd = opt.state_dict()
    assert sd["optim_bits"] == 8 and [a is not None for a in sd["absmax1"]] == opt.is8 == [a is not None for a in sd["absmax2"]]
    assert sd["exp_avg"][i8[0]].dtype == torch.uint8 and torch.equal(sd["qmap1"].cpu(), torch.from_numpy(M.MAP_SIGNED))
    assert torch.equal(sd["qmap2"].cpu(), torch.from_numpy(M.MAP_UNSIGNED))
    snap = [p.detach().clone() for p in ps8]
    opt.step(gate=torch.tensor(3.4e38, dtype=torch.float32, device=cuda))
    after = _opt_state(opt)
    assert float(opt.step_t) == 5.0 and not _equal_states(after, before[:len(after)])
    with torch.no_grad():
        for p, s0 in zip(ps8, snap):
            p.copy_(s0)
    opt2 = PackedAdamW(tr8, optim_bits=8, **OPT)
    ptrs = [t.data_ptr() for t in opt2.m + opt2.v]
    perm = [4, 2, 0, 3, 1]                                 # matched by name, whatever the order
    opt2.load_state_dict({k: ([v[j] for j in perm] if isinstance(v, list) else v) for k, v in sd.items()})
    assert ptrs == [t.data_ptr() for t in opt2.m + opt2.v]
    opt2.step()
    assert _equal_states(_opt_state(opt2), after)
    # refusals: the other width, another partition, other maps
    with pytest.raises(AssertionError, match="32-bit"):
        opt2.load_state_dict(ref32.state_dict())
    with pytest.raises(AssertionError, match="8-bit"):
        ref32.load_state_dict(sd)
    with pytest.raises(AssertionError, match="partition"):
        PackedAdamW(tr8, optim_bits=8, min_8bit_size=20000, **OPT).load_state_dict(sd)
    with pytest.raises(AssertionError, match="code map"):
        opt2.load_state_dict({**sd, "qmap1": sd["qmap1"] * 0.5})
    assert _equal_states(_opt_state(opt2), after)          # a refused state leaves everything as it was


# ---- 9. in the captured step -----------------------------------------------------------------------------------------------------------
def _setup(cuda, seeds=(4, 5, 6, 7, 8), n_students=1):
    from tests.test_ema_gpu import _setup as setup
    return setup(cuda, seeds=seeds, n_students=n_students)


CHECK_BUDGET = 1 << 20      # elements per step that go through the fp64 model on the host (about a second of numpy)


def _checked(opt):
    """the 8-bit tensors a captured step is checked on: those with a short last block first, then by size from both ends, while
    their elements fit CHECK_BUDGET (the model runs on the host; every size class and both ends of the table are in)"""
    idx = sorted((i for i, q in enumerate(opt.is8) if q), key=lambda i: (opt.params[i].numel() % M.BLOCK == 0, opt.params[i].numel()))
    order, lo, hi = [], 0, len(idx) - 1
    while lo <= hi:
        order.append(idx[lo])
        if hi > lo:
            order.append(idx[hi])
        lo, hi = lo + 1, hi - 1
    out, total = [], 0
    for i in order:
        if not out or total + opt.params[i].numel() <= CHECK_BUDGET:
            out.append(i)
            total += opt.params[i].numel()
    return sorted(out)


def _snap8(step):
    """the checked 8-bit tensors' state by index, after the pending optimizer tail"""
    step.finish()
    torch.cuda.synchronize()
    opt = step.optimizer
    return {i: _host8(opt, i) for i in _checked(opt)}


def _check_captured(step, olds, count, what, grad_scale=1.0):
    opt = step.optimizer
    news = _snap8(step)
    hyper = dict(HYPER)
    for i, old in olds.items():
        g = opt.grads[i].reshape(-1).cpu().numpy()        # the persistent gradient the captured backward left: what the table points at
        check_step(old, news[i], g, count, "%s %s" % (what, opt.names[i]), hyper=hyper, grad_scale=grad_scale)
        sh = opt.entries[i][1]
        if sh is not None:
            assert torch.equal(sh.reshape(-1), opt.params[i].detach().reshape(-1).to(torch.bfloat16))
    return news


def _bits(step):
    step.finish()
    torch.cuda.synchronize()
    return _opt_state(step.optimizer)


def test_captured_step_follows_the_model(cuda):
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    (sa,), teacher, batches = _setup(cuda)
    A = GraphedFineTunerStep(sa, teacher, use_8bit_adam=True, **KW).capture(batches[0])
    opt = A.optimizer
    assert opt.optim_bits == 8 and sum(opt.is8) >= 1 and sum(not q for q in opt.is8) >= 1
    assert opt.state_bytes() < 8 * A.trainer.n_trainable()
    print("8-bit tensors: %d of %d (%d checked against the model); moment state %d B against %d B in fp32"
          % (sum(opt.is8), len(opt.is8), len(_checked(opt)), opt.state_bytes(), 8 * A.trainer.n_trainable()))
    assert len(_checked(opt)) >= min(3, sum(opt.is8))
    olds = _snap8(A)
    for k, b in enumerate(batches[:3]):
        out = A.train_step(None, b)
        assert out["applied"] is True and torch.isfinite(out["loss"])
        olds = _check_captured(A, olds, k, "captured step %d" % k)
    assert float(opt.step_t) == 3.0
    # a poisoned batch: reported as not applied, nothing moves
    before = _bits(A)
    bad = {k: v.clone() for k, v in batches[3].items()}
    bad["target"][0, 0, 0, 0] = float("nan")
    out = A.train_step(None, bad)
    after = _bits(A)
    assert not torch.isfinite(out["loss"]) and _equal_states(after, before) and float(opt.step_t) == 3.0
    out = A.train_step(None, batches[4])                  # training goes on
    _check_captured(A, olds, 3, "after the poisoned batch")


def test_captured_accumulation_and_clip(cuda):
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    (sa, sb), teacher, batches = _setup(cuda, n_students=2)
    A = GraphedFineTunerStep(sa, teacher, use_8bit_adam=True, accumulation_steps=2, **KW).capture(batches[0])
    olds = _snap8(A)
    start = _bits(A)
    out0 = A.train_step(None, batches[0])
    assert out0["applied"] is False and _equal_states(_bits(A), start)          # the optimizer runs on the closing call only
    out1 = A.train_step(None, batches[1])
    assert out1["applied"] is True and float(A.optimizer.step_t) == 1.0
    _check_captured(A, olds, 0, "window of two", grad_scale=0.5)                 # (the arena holds the window's sum)
    # a threshold small enough to clip: the model under the coefficient ops.GradNorm reports
    B = GraphedFineTunerStep(sb, teacher, use_8bit_adam=True, max_grad_norm=1e-4, **KW).capture(batches[0])
    olds = _snap8(B)
    for k, b in enumerate(batches[:2]):
        out = B.train_step(None, b)
        B.finish()
        torch.cuda.synchronize()
        coef = float(B.optimizer.grad_norm.coef)
        assert 0.0 < coef < 1.0 and float(out["grad_norm"]) > 1e-4
        olds = _check_captured(B, olds, k, "clipped step %d" % k, grad_scale=coef)
    assert B.optimizer.clipped_steps() == 2


def test_captured_ema_follows_the_8bit_masters(cuda):
    from tests.test_ema_gpu import _emas, _masters, _within_trajectory_bound
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    (sa,), teacher, batches = _setup(cuda)
    A = GraphedFineTunerStep(sa, teacher, use_8bit_adam=True, ema=True, **KW).capture(batches[0])
    start, seq = _masters(A), []
    for b in batches[:3]:
        A.train_step(None, b)
        seq.append(_masters(A))
    assert A.ema.steps() == 3 and abs(A.ema.cur_decay() - EM.ema_decay(2)) <= 2.0 ** -22
    for n, a in zip(A.ema.names, _emas(A)):
        _within_trajectory_bound(a, start[n], [s[n] for s in seq], 3, n)


def test_captured_resume_is_bit_exact(cuda):
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    (sa, sb), teacher, batches = _setup(cuda, n_students=2)
    A = GraphedFineTunerStep(sa, teacher, use_8bit_adam=True, **KW).capture(batches[0])
    B = GraphedFineTunerStep(sb, teacher, use_8bit_adam=True, **KW).capture(batches[0])
    for b in batches[:2]:
        A.train_step(None, b)
    A.finish()
    for pa, pb in zip(A.trainer.parameters(), B.trainer.parameters()):
        pb.data.copy_(pa.detach())
    B.trainer.refresh_()
    B.optimizer.load_state_dict(A.optimizer.state_dict())
    for b in batches[2:4]:
        A.train_step(None, b)
        B.train_step(None, b)
    a, b_ = _bits(A), _bits(B)
    assert float(A.optimizer.step_t) == float(B.optimizer.step_t) == 4.0 and _equal_states(a, b_)
    assert any(bool((m != 127).any()) for m, q in zip(A.optimizer.m, A.optimizer.is8) if q)


def test_default_takes_none_of_the_new_paths(cuda, monkeypatch):
    from diffusion_pruning_amd import _lib, ops
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    (sa, sb, sc), teacher, batches = _setup(cuda, seeds=(4, 5, 6), n_students=3)
    lib = _lib.load()
    calls = {}
    for name, _, _ in _lib.EXPORTS:
        fn = getattr(lib, name)

        def counting(*a, _fn=fn, _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counting)
    results = []
    for student, kw in ((sa, {}), (sb, dict(use_8bit_adam=False)), (sc, dict(use_8bit_adam=True))):
        step = GraphedFineTunerStep(student, teacher, **KW, **kw).capture(batches[0])
        calls.clear()
        ops.LAUNCH_LOG = []
        try:
            outs = [step.train_step(None, b) for b in batches]
            torch.cuda.synchronize()
            n_log = len(ops.LAUNCH_LOG)
        finally:
            ops.LAUNCH_LOG = None
        results.append((dict(calls), n_log, [float(o["loss"]) for o in outs], [p.detach().clone() for p in step.trainer.parameters()], step))
    (ca, na, la, pa, A), (cb, nb, lb, pb, B), (cc, nc, lc, pc, C) = results
    assert ca == cb and na == nb and "aptp_adamw8_many" not in ca and ca.get("aptp_adamw_many") == 3
    assert la == lb and all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert B.optimizer.table8 is None and B.optimizer.qmap1 is None and all(m.dtype == torch.float32 for m in B.optimizer.m)
    assert B.optimizer.state_bytes() == 8 * B.trainer.n_trainable()
    # with it: one more launch per optimizer step, nothing else
    assert cc.get("aptp_adamw8_many") == 3 and cc.get("aptp_adamw_many") == 3
    assert {k: v for k, v in cc.items() if k != "aptp_adamw8_many"} == ca and nc == na          # (the log holds the contractions)


# ---- 10. sanity of the whole: measured, not pinned -------------------------------------------------------------------------------------
def test_eight_steps_against_the_fp32_state(cuda):
    """The same fixed batch for eight steps under fp32 and 8-bit moments.  Recorded (tests.margins): both loss curves and the
    relative L2 distance of the total parameter updates.  Asserted: the 8-bit run's loss falls by at least half of what the
    fp32 run's (the parent's code) falls."""
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    (sa, sb), teacher, batches = _setup(cuda, n_students=2)
    runs = []
    for student, kw in ((sa, {}), (sb, dict(use_8bit_adam=True))):
        step = GraphedFineTunerStep(student, teacher, **KW, **kw).capture(batches[0])
        step.finish()
        p0 = torch.cat([p.detach().flatten() for p in step.trainer.parameters()]).double()
        losses = [float(step.train_step(None, batches[0])["loss"]) for _ in range(9)]      # (the ninth call reports the loss after eight steps)
        step.finish()
        torch.cuda.synchronize()
        runs.append((losses, torch.cat([p.detach().flatten() for p in step.trainer.parameters()]).double() - p0))
    (l32, d32), (l8, d8) = runs
    print("loss, fp32 state :", " ".join("%.6f" % x for x in l32))
    print("loss, 8-bit state:", " ".join("%.6f" % x for x in l8))
    rel = float((d8 - d32).norm() / d32.norm())
    print("relative L2 distance of the total updates: %.4e" % rel)
    for k, (x, y) in enumerate(zip(l32, l8)):
        margins.check(abs(x - y), float("inf"), "loss after %d steps: |fp32 state - 8-bit state| (%.6f vs %.6f)" % (k, x, y))
    margins.check(rel, float("inf"), "relative L2 distance of the total update after 9 steps, 8-bit vs fp32 state")
    fall32, fall8 = l32[0] - l32[8], l8[0] - l8[8]
    assert fall32 > 0, ("the fp32 run's loss does not fall in this setting", l32)
    assert fall8 >= 0.5 * fall32, (fall8, fall32)
