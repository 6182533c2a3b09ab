"""U-Net attention forward (output and log-sum-exp, every forward kernel) and backward against the fp64 reference of
tests/attention_model.py: an elementwise bound with no exceptions, and a per-(batch, head, 64-row block) error ratio against the
bf16 format model, which a single wrong tile cannot hide in.  tests/test_attention_model_host.py proves on the CPU that these
metrics pass two sound forms of the model and catch each of five seeded kernel defects.  Then the call forms the training path
uses -- column slices of fused buffers, rows of longer buffers, batched heads, the autograd Functions -- bit for bit against
the contiguous call."""
import math

import pytest
import torch

from tests import attention_model as AM
from tests import margins

pytestmark = pytest.mark.gpu

VARIANTS = (0, 1, 2, 3, 4, 5, 6)       # AptpAttentionParams.variant: 0 = the library's choice; the launcher accepts every variant on
#                                        every shape (where a kernel does not apply it takes the next form), so every one must be right
CASE_IDS = [c.id for c in AM.CASES]


@pytest.fixture(scope="module")
def ops(cuda):
    from diffusion_pruning_amd import ops as o
    o._lib.load()
    return o


@pytest.fixture
def force_variant(ops):
    """sets ops.ATTN_VARIANT for the following forward launches; back to 0 (the library chooses) after the test"""
    def force(v):
        ops.ATTN_VARIANT = v
    yield force
    ops.ATTN_VARIANT = 0


def _dev(t, cuda):
    """fp64 [B, heads, L, 64] of bf16 values -> the kernels' bf16 [B, L, heads*64] on the GPU"""
    return AM.from_heads(t).bfloat16().to(cuda)


def _host(t, heads):
    return AM.to_heads(t.double().cpu(), heads)


def _forward(ops, cuda, q, k, v, heads, scale=None):
    lse = torch.full((q.shape[0], heads, q.shape[1]), float("nan"), dtype=torch.float32, device=cuda)
    o = ops.attention(q, k, v, heads, scale=scale, lse=lse)
    return o, lse


def _backward(ops, q, k, v, o, do, lse, heads, scale=None, q_split=None):
    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
    ops.attention_bwd(q, k, v, o, do, lse, heads, dq, dk, dv, scale=scale, q_split=q_split)
    return dq, dk, dv


def _check(results, case, what):
    """results: {label: measure() dict}.  Every label must pass; the worst value per output goes to the parity-margins record."""
    for key in next(iter(results.values())):
        label, hu = max(((lb, r[key][0]) for lb, r in results.items()), key=lambda t: t[1])
        margins.check(hu, AM.HARD_LIMIT, f"{what} {case.id} hard_use {key} (worst: {label})")
        if key in AM.RATIO_KEYS:
            label, br = max(((lb, r[key][1]) for lb, r in results.items()), key=lambda t: t[1])
            if case.smooth:
                margins.check(br, AM.RATIO_LIMIT, f"{what} {case.id} block_ratio {key} (worst: {label})")
            else:
                print(f"{what} {case.id} block_ratio {key} = {br:.3f} (worst: {label}; spiked case, not asserted)")


# ---------------------------------------------------------------------------------------------------------------------
# a. forward: o and lse of every forward kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(AM.CASES)), ids=CASE_IDS)
def test_forward_output_and_lse_of_every_variant(ops, cuda, force_variant, index):
    case = AM.CASES[index]
    h = case.shape[1]
    ins, ref, bound, mdl = AM.case_reference(index)
    q, k, v, _ = (_dev(t, cuda) for t in ins)
    results = {}
    for variant in VARIANTS:
        force_variant(variant)
        o, lse = _forward(ops, cuda, q, k, v, h, case.scale)
        got = {"o": _host(o, h), "lse": lse.double().cpu()}
        results[f"variant {variant}"] = AM.measure(got, ref, bound, mdl, keys=("o", "lse"))
    for label, r in results.items():
        print(case.id, label, {key: tuple(None if x is None else round(x, 3) for x in val) for key, val in r.items()})
    _check(results, case, "fwd")


# ---------------------------------------------------------------------------------------------------------------------
# b. backward on the GPU forward's own o and lse: the library's q_split, none, and three slices
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(AM.CASES)), ids=CASE_IDS)
def test_backward_of_every_q_split(ops, cuda, index):
    case = AM.CASES[index]
    B, h, Lq, Lk = case.shape
    ins, ref, bound, mdl = AM.case_reference(index)
    q, k, v, do = (_dev(t, cuda) for t in ins)
    o, lse = _forward(ops, cuda, q, k, v, h, case.scale)
    splits = {"library": None, "1": 1}
    if (Lq + 63) // 64 >= 3:
        splits["3"] = 3
    results = {}
    for label, s in splits.items():
        dq, dk, dv = _backward(ops, q, k, v, o, do, lse, h, case.scale, q_split=s)
        got = {"dq": _host(dq, h), "dk": _host(dk, h), "dv": _host(dv, h)}
        results[f"q_split {label}"] = AM.measure(got, ref, bound, mdl, keys=("dq", "dk", "dv"))
    for label, r in results.items():
        print(case.id, label, {key: tuple(round(x, 3) for x in val) for key, val in r.items()})
    _check(results, case, "bwd")


def test_library_q_split_is_exercised(ops, cuda):
    """the case list reaches the split dK/dV kernel and its fold through the library's own rule"""
    import ctypes
    from diffusion_pruning_amd import _lib
    p = _lib.AttentionBwdParams()
    p.B, p.heads, p.Lq, p.Lk = 1, 2, 1024, 77
    assert (1, 2, 1024, 77) in [c.shape for c in AM.CASES]
    assert _lib.load().aptp_attention_bwd_q_split(ctypes.byref(p)) == 8 and ops.ATTN_BWD_Q_SPLIT


# ---------------------------------------------------------------------------------------------------------------------
# c. real call forms, bit for bit against the contiguous call (same kernels on both sides: only the addressing differs)
# ---------------------------------------------------------------------------------------------------------------------
def _rand(shape, g, cuda):
    return torch.randn(shape, generator=g).bfloat16().to(cuda)


@pytest.mark.parametrize("kind,q_split", [("self", 1), ("self", 3), ("cross", 1), ("cross", 3)])
def test_fused_buffer_slices_equal_the_contiguous_call_and_stay_inside(ops, cuda, kind, q_split):
    """q/k/v as column slices of one fused projection output, dq/dk/dv as column slices of one gradient buffer (what
    autograd.SelfAttnFn / CrossAttnFn pass), here with 64 sentinel columns and 2 sentinel rows per batch around the gradients"""
    B, h, Lq = 2, 2, 200
    w = h * 64
    g = torch.Generator().manual_seed(11 + q_split + (kind == "self"))
    if kind == "self":
        Lk = Lq
        buf = _rand((B, Lq, 3 * w), g, cuda)
        q, k, v = buf[..., :w], buf[..., w:2 * w], buf[..., 2 * w:]
        gbuf = _rand((B, Lq + 2, 3 * w + 64), g, cuda)
        before = gbuf.clone()
        dq, dk, dv = gbuf[:, :Lq, :w], gbuf[:, :Lk, w:2 * w], gbuf[:, :Lk, 2 * w:3 * w]
        ncol = 3 * w
    else:
        Lk = 77
        q = _rand((B, Lq, w), g, cuda)
        buf = _rand((B, Lk, 2 * w), g, cuda)
        k, v = buf[..., :w], buf[..., w:]
        gbuf = _rand((B, Lk + 2, 2 * w + 64), g, cuda)
        before = gbuf.clone()
        dq = torch.empty_like(q)
        dk, dv = gbuf[:, :Lk, :w], gbuf[:, :Lk, w:2 * w]
        ncol = 2 * w
    do = _rand((B, Lq, w), g, cuda)
    obuf = _rand((B, Lq + 2, w + 64), g, cuda)
    obefore = obuf.clone()
    lse = torch.empty(B, h, Lq, dtype=torch.float32, device=cuda)
    o = ops.attention(q, k, v, h, out=obuf[:, :Lq, :w], lse=lse)
    ops.attention_bwd(q, k, v, o, do, lse, h, dq, dk, dv, q_split=q_split)

    qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
    oc, lsec = _forward(ops, cuda, qc, kc, vc, h)
    dqc, dkc, dvc = _backward(ops, qc, kc, vc, oc, do, lsec, h, q_split=q_split)
    assert torch.equal(o, oc) and torch.equal(lse, lsec)
    assert torch.equal(dq, dqc) and torch.equal(dk, dkc) and torch.equal(dv, dvc)
    assert bool(torch.isfinite(dqc.float()).all() and torch.isfinite(dkc.float()).all() and torch.isfinite(dvc.float()).all())
    # sentinels: the extra columns and rows hold what they held (compared as bit patterns)
    assert torch.equal(gbuf[:, :, ncol:].view(torch.int16), before[:, :, ncol:].view(torch.int16))
    assert torch.equal(gbuf[:, -2:].view(torch.int16), before[:, -2:].view(torch.int16))
    assert torch.equal(obuf[:, :, w:].view(torch.int16), obefore[:, :, w:].view(torch.int16))
    assert torch.equal(obuf[:, -2:].view(torch.int16), obefore[:, -2:].view(torch.int16))


@pytest.mark.parametrize("shape", [(2, 2, 129, 65), (1, 2, 256, 256), (1, 1, 100, 2077)], ids=lambda s: "x".join(map(str, s)))
def test_rows_past_the_length_are_never_read(ops, cuda, shape):
    """k/v are the first Lk rows, q/o/do the first Lq rows of longer buffers whose other rows are NaN: the kernels clamp row
    indices to L - 1, so nothing past L may reach a result (the single-group, software-pipelined and double-buffered forwards)"""
    B, h, Lq, Lk = shape
    w = h * 64
    g = torch.Generator().manual_seed(Lq * 7 + Lk)
    q, do = (_rand((B, Lq, w), g, cuda) for _ in range(2))
    k, v = (_rand((B, Lk, w), g, cuda) for _ in range(2))

    def longer(t, extra):
        buf = torch.full((B, t.shape[1] + extra, w), float("nan"), dtype=torch.bfloat16, device=cuda)
        buf[:, :t.shape[1]] = t
        return buf[:, :t.shape[1]]
    o, lse = _forward(ops, cuda, q, k, v, h)
    ql, kl, vl, dol = longer(q, 3), longer(k, 130), longer(v, 67), longer(do, 5)
    obuf = torch.full((B, Lq + 3, w), float("nan"), dtype=torch.bfloat16, device=cuda)
    lse2 = torch.empty_like(lse)
    o2 = ops.attention(ql, kl, vl, h, out=obuf[:, :Lq], lse=lse2)
    assert bool(torch.isfinite(o2.float()).all() and torch.isfinite(lse2).all())
    assert torch.equal(o2, o) and torch.equal(lse2, lse)
    assert bool(torch.isnan(obuf[:, Lq:].float()).all())
    splits = (1, 3) if (Lq + 63) // 64 >= 3 else (1,)
    for s in splits:
        dq, dk, dv = _backward(ops, q, k, v, o, do, lse, h, q_split=s)
        gq, gk, gv = longer(torch.zeros_like(q), 3), longer(torch.zeros_like(k), 2), longer(torch.zeros_like(v), 2)
        ops.attention_bwd(ql, kl, vl, o2, dol, lse2, h, gq, gk, gv, q_split=s)
        for name, a, b in (("dq", gq, dq), ("dk", gk, dk), ("dv", gv, dv)):
            assert bool(torch.isfinite(a.float()).all()), (name, s)
            assert torch.equal(a, b), (name, s)


@pytest.mark.parametrize("variant,q_split", [(3, 1), (3, 3), (5, 1), (1, 3)])
def test_batches_and_heads_are_independent(ops, cuda, force_variant, variant, q_split):
    """the (b, h) slice of a B = 2, heads = 3 launch equals a B = 1, heads = 1 launch on that slice: o, lse, dq, dk, dv"""
    B, h, Lq, Lk = 2, 3, 200, 77
    g = torch.Generator().manual_seed(variant * 10 + q_split)
    q, do = (_rand((B, Lq, h * 64), g, cuda) for _ in range(2))
    k, v = (_rand((B, Lk, h * 64), g, cuda) for _ in range(2))
    force_variant(variant)                 # an explicit variant: the occupancy rule, which sees the grid size, is out of the way
    o, lse = _forward(ops, cuda, q, k, v, h)
    dq, dk, dv = _backward(ops, q, k, v, o, do, lse, h, q_split=q_split)
    for b in range(B):
        for hh in range(h):
            def one(t):
                return t[b:b + 1, :, 64 * hh:64 * hh + 64].contiguous()
            q1, k1, v1, do1 = one(q), one(k), one(v), one(do)
            o1, lse1 = _forward(ops, cuda, q1, k1, v1, 1)
            dq1, dk1, dv1 = _backward(ops, q1, k1, v1, o1, do1, lse1, 1, q_split=q_split)
            assert torch.equal(o1, one(o)) and torch.equal(lse1[0, 0], lse[b, hh]), (b, hh)
            assert torch.equal(dq1, one(dq)) and torch.equal(dk1, one(dk)) and torch.equal(dv1, one(dv)), (b, hh)


# ---------------------------------------------------------------------------------------------------------------------
# d. the autograd Functions, as the gated U-Net calls them
# ---------------------------------------------------------------------------------------------------------------------
def _check_function(name, got, ins, heads):
    ref, bound = AM.ref64(*ins, 0.125)
    mdl = AM.model(*ins, 0.125, torch.float64)
    res = AM.measure(got, ref, bound, mdl, keys=("o", "dq", "dk", "dv"))
    for key, (hu, br) in res.items():
        print(name, key, f"hard_use {hu:.3f} block_ratio {br:.3f}")
        margins.check(hu, AM.HARD_LIMIT, f"{name} hard_use {key}")
        margins.check(br, AM.RATIO_LIMIT, f"{name} block_ratio {key}")


def test_self_attn_function(ops, cuda):
    from diffusion_pruning_amd import autograd as AG
    B, L, h = 2, 200, 2
    w = h * 64
    g = torch.Generator().manual_seed(2024)
    qkv = _rand((B, L, 3 * w), g, cuda).requires_grad_()
    gt = _rand((B, w, L), g, cuda)                     # the upstream gradient arrives as a transposed view of this
    o = AG.SelfAttnFn.apply(qkv, h)
    y = o.transpose(1, 2)
    assert not gt.transpose(1, 2).is_contiguous()
    y.backward(gt)
    torch.cuda.synchronize()
    dqkv = qkv.grad
    assert dqkv.shape == qkv.shape and bool(torch.isfinite(dqkv.float()).all())
    ins = tuple(_host(t, h) for t in (qkv.detach()[..., :w], qkv.detach()[..., w:2 * w], qkv.detach()[..., 2 * w:], gt.transpose(1, 2)))
    # the three column blocks together are every element of dqkv: none can be left unwritten and still meet the bound
    got = {"o": _host(o.detach(), h), "dq": _host(dqkv[..., :w], h), "dk": _host(dqkv[..., w:2 * w], h), "dv": _host(dqkv[..., 2 * w:], h)}
    _check_function("SelfAttnFn", got, ins, h)
    # a second backward through a fresh graph writes the same bits (nothing depends on what the empty gradient buffer held)
    qkv2 = qkv.detach().clone().requires_grad_()
    AG.SelfAttnFn.apply(qkv2, h).transpose(1, 2).backward(gt)
    assert torch.equal(qkv2.grad, dqkv)


def test_cross_attn_function(ops, cuda):
    from diffusion_pruning_amd import autograd as AG
    B, L, Lk, h = 2, 200, 77, 2
    w = h * 64
    g = torch.Generator().manual_seed(2025)
    q = _rand((B, L, w), g, cuda).requires_grad_()
    kv = _rand((B, Lk, 2 * w), g, cuda).requires_grad_()
    gt = _rand((B, w, L), g, cuda)
    o = AG.CrossAttnFn.apply(q, kv, h)
    o.transpose(1, 2).backward(gt)
    torch.cuda.synchronize()
    assert q.grad.shape == q.shape and kv.grad.shape == kv.shape
    assert bool(torch.isfinite(q.grad.float()).all() and torch.isfinite(kv.grad.float()).all())
    ins = tuple(_host(t, h) for t in (q.detach(), kv.detach()[..., :w], kv.detach()[..., w:], gt.transpose(1, 2)))
    got = {"o": _host(o.detach(), h), "dq": _host(q.grad, h), "dk": _host(kv.grad[..., :w], h), "dv": _host(kv.grad[..., w:], h)}
    _check_function("CrossAttnFn", got, ins, h)
    q2, kv2 = q.detach().clone().requires_grad_(), kv.detach().clone().requires_grad_()
    AG.CrossAttnFn.apply(q2, kv2, h).transpose(1, 2).backward(gt)
    assert torch.equal(q2.grad, q.grad) and torch.equal(kv2.grad, kv.grad)
