"""GPU checks of the masked loss stage (csrc/loss_stage.hip, ops.LossStage, autograd.LossStageFn): every valid unit has the bits
ops.mse gives that sample's view; groups, total and every gradient element stay inside bounds derived from the number of fp32
roundings on their path, against the fp64 model of tests/loss_stage_model.py; samples that are not valid reach no output, whatever
their rows hold, and get gradient rows of exact zeros; nothing outside the outputs is written; a captured call replays to the
eager bits next to a busy stream.  Nothing here provokes a fault: bad tables are refused by the host validation."""
import ctypes

import numpy as np
import pytest
import torch

from tests import loss_stage_model as M

pytestmark = pytest.mark.gpu
from tests.margins import check  # noqa: E402

EPS = M.EPS
BF, F32 = torch.bfloat16, torch.float32
COEF, DIV = (0.01, 0.5), (0.0, 2.0)
ITEMS = [(0, 2), (1, None)]                 # x is the first operand of terms 0 and 2, y of term 1
R_SMALL = 3                                 # aptp_mse_nblocks = 1, an odd number of rows


def r_big(C):
    """rows per sample that give a unit two workgroups, and no multiple of the 256-thread stride"""
    return 520 if C == 8 else 70


def _rand(shape, dtype, cuda, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(cuda, dtype)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _case(cuda, B, C, kind, strided=False, big_x=False):
    """three terms in two groups: (x, t0) weighted in group 0; (y, u) * 0.5 and (x, t2) in group 1, divided by 2"""
    from diffusion_pruning_amd import ops
    dx, dt0, dt2, dy, du = {"bf16": (BF, BF, BF, BF, BF), "f32": (F32, F32, F32, F32, F32), "mixed": (BF, F32, BF, F32, BF)}[kind]
    rx, ry = (r_big(C), R_SMALL) if big_x else (R_SMALL, r_big(C))
    assert M.mse_nblocks(R_SMALL, C) == 1 and M.mse_nblocks(r_big(C), C) >= 2
    if strided:
        wide = _rand((B, rx, C + 32), dx, cuda, 1)
        x = wide[..., :C]                    # a channel slice of a wider tensor: pitch C + 32
        assert not x.is_contiguous()
    else:
        wide = x = _rand((B, rx, C), dx, cuda, 1)
    t0, t2 = _rand((B, rx, C), dt0, cuda, 2), _rand((B, rx, C), dt2, cuda, 3)
    y, u = _rand((B, ry, C), dy, cuda, 4), _rand((B, ry, C), du, cuda, 5)
    w = (torch.rand(B, generator=torch.Generator().manual_seed(6)) + 0.1).to(cuda)
    terms = [ops.LossTerm(x, t0, 0, 1.0, True), ops.LossTerm(y, u, 1, 0.5, False), ops.LossTerm(x, t2, 1, 1.0, False)]
    return dict(terms=terms, w=w, B=B, C=C, rows=(rx, ry, rx), wide=wide, tensors=[wide, t0, t2, y, u])


def _model_terms(case):
    return [dict(a=_np(t.a), b=_np(t.b), group=t.group, scale=t.scale, weighted=t.per_sample) for t in case["terms"]]


def _patterns(B):
    pats = [[1.0] * B]
    if B > 1:
        pats.append([1.0, 0.0, 1.0, 1.0, 0.0][:B])
    return pats


def _ops_mse(ops, a, b):
    if a.dtype != b.dtype:
        return ops.mse(a.float().contiguous(), b.float().contiguous())
    return ops.mse(a, b)


def _ulp_bf16(x):
    """one unit in the last place of bf16 (8 significant bits) at |x|"""
    ax = np.maximum(np.abs(x), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(ax)) - 7)


def _value_bounds(case):
    """roundings on the path of each group and of the total, from the table sizes"""
    B, C = case["B"], case["C"]
    path = [M.unit_ops(r, C) + M.term_ops(B, t.per_sample) for r, t in zip(case["rows"], case["terms"])]
    g0 = path[0] + M.group_ops(1, False)
    g1 = max(path[1], path[2]) + M.group_ops(2, True)
    return [g0, g1], max(g0, g1) + M.total_ops(2)


def _check_against_model(case, stage, valid, g, what):
    """forward and backward of `stage` as it stands against the fp64 model on the tensors as they stand"""
    from diffusion_pruning_amd import ops
    terms, w, B = case["terms"], case["w"], case["B"]
    out = stage.run().clone()
    grads = [x.clone() for x in stage.backward(g)]
    torch.cuda.synchronize()
    units = stage.units.clone()
    for t, T in enumerate(terms):
        for b in range(B):
            if valid[b]:
                assert torch.equal(units[t][b], _ops_mse(ops, T.a[b], T.b[b])), (what, t, b)
    mt = _model_terms(case)
    fw = M.forward(mt, valid, _np(w), COEF, DIV)
    gb, tb = _value_bounds(case)
    for i in range(2):
        err = abs(float(out[i]) - fw["groups"][i]) / fw["groups"][i]
        print("%s: group %d rel err %.3e of %.3e" % (what, i, err, gb[i] * EPS))
        check(err, gb[i] * EPS, "%s: group %d vs fp64" % (what, i))
    err = abs(float(out[2]) - fw["total"]) / fw["total"]
    print("%s: total rel err %.3e of %.3e" % (what, err, tb * EPS))
    check(err, tb * EPS, "%s: total vs fp64" % what)
    assert float(out[3]) == sum(valid) == fw["n"]
    assert torch.equal(stage.sample_out, torch.where(torch.tensor(valid, device=units.device) != 0, units[0], torch.zeros_like(units[0])))
    want = M.backward(mt, ITEMS, valid, _np(w), COEF, DIV, g=float(g))
    for i, (got, (ref, bound)) in enumerate(zip(grads, want)):
        src = stage.grad_inputs[i]
        assert got.shape == src.shape and got.dtype == src.dtype
        e = np.abs(_np(got) - ref)
        if got.dtype == F32:
            worst = float((e / np.maximum(bound, 1e-300)).max())
            print("%s: gradient %d worst error %.3f of 8 roundings" % (what, i, worst / EPS))
            assert (e <= 8 * EPS * bound).all(), (what, i, worst / EPS)
        else:
            worst = float((e / _ulp_bf16(ref)).max())
            print("%s: gradient %d worst error %.3f bf16 ulp" % (what, i, worst))
            assert (e <= _ulp_bf16(ref)).all(), (what, i, worst)
        for b in range(B):
            if not valid[b]:
                assert float(got[b].float().abs().max()) == 0.0, (what, i, b)
            else:
                assert float(got[b].float().abs().max()) > 0.0
    return out, grads


@pytest.mark.parametrize("kind", ["bf16", "f32", "mixed"])
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_stage_against_ops_mse_and_the_fp64_model(cuda, B, C, kind):
    from diffusion_pruning_amd import ops
    case = _case(cuda, B, C, kind)
    valid = torch.ones(B, device=cuda)
    stage = ops.LossStage(case["terms"], COEF, weights=case["w"], valid=valid, group_div=DIV)
    assert len(stage.items) == 2 and stage.items[0]["terms"] == [0, 2] and stage.copies == []
    assert stage.nblocks == B * sum(M.mse_nblocks(r, C) for r in case["rows"])
    g = torch.tensor(0.75, device=cuda)
    keep = [t.clone() for t in case["tensors"]]
    for pat in _patterns(B):
        valid.copy_(torch.tensor(pat))
        what = "B%d C%d %s valid %s" % (B, C, kind, "".join(str(int(v)) for v in pat))
        out, grads = _check_against_model(case, stage, pat, g, what)
        if 0.0 in pat:
            # the rows of the samples that are not there hold NaN: no output bit changes, their gradient rows stay zero
            for t in case["tensors"]:
                for b, v in enumerate(pat):
                    if not v:
                        t[b] = float("nan")
            out2 = stage.run().clone()
            grads2 = [x.clone() for x in stage.backward(g)]
            assert torch.equal(out2, out) and bool(torch.isfinite(stage.sample_out).all())
            for a, b in zip(grads, grads2):
                assert torch.equal(a, b)
            for t, k in zip(case["tensors"], keep):
                t.copy_(k)
    # nobody there: every output and every gradient is zero, also with NaN in every row
    valid.zero_()
    for t in case["tensors"]:
        t[0] = float("nan")
    out = stage.run()
    grads = stage.backward(g)
    assert float(out.abs().max()) == 0.0 and float(stage.sample_out.abs().max()) == 0.0
    assert all(float(x.float().abs().max()) == 0.0 for x in grads)


class _Guarded:
    """buffers between guard words"""
    PAD, WORD = 8, 12345.0

    def __init__(self):
        self.bufs = []

    def alloc(self, n, device, dtype=F32):
        buf = torch.full((n + 2 * self.PAD,), self.WORD, dtype=dtype, device=device)
        self.bufs.append((buf, n))
        return buf[self.PAD:self.PAD + n]

    def alloc_grad(self, n, dtype, device):
        return self.alloc(n, device, dtype)

    def intact(self):
        word = torch.tensor(self.WORD)
        return all(bool((b[:self.PAD] == word.to(b.dtype)).all()) and bool((b[self.PAD + n:] == word.to(b.dtype)).all())
                   for b, n in self.bufs)


@pytest.mark.parametrize("kind,dense", [("bf16", False), ("f32", False), ("mixed", True)])
def test_strided_first_operand_guards_and_untouched_operands(cuda, kind, dense):
    """x is a channel slice of a wider tensor, read in place, and here the operand with two workgroups per unit.  Without
    dense_grads its gradient has x's pitch: the columns between C and the pitch, and the guard words on either side of every
    output, stay as they were"""
    from diffusion_pruning_amd import ops
    B, C = 3, 64
    case = _case(cuda, B, C, kind, strided=True, big_x=True)
    guard = _Guarded()

    class LS(ops.LossStage):
        _alloc = staticmethod(guard.alloc)
        _alloc_grad = staticmethod(guard.alloc_grad)

    valid = torch.tensor([1.0, 0.0, 1.0], device=cuda)
    stage = LS(case["terms"], COEF, weights=case["w"], valid=valid, group_div=DIV, dense_grads=dense)
    assert stage.copies == [] and stage._p.terms[0].lda == C + 32
    keep = [t.clone() for t in case["tensors"]]
    g = torch.tensor(-1.5, device=cuda)
    _check_against_model(case, stage, [1.0, 0.0, 1.0], g, "strided %s" % kind)
    assert len(guard.bufs) == 5                             # partial, out, sample_out, two gradients
    assert guard.intact()
    assert all(torch.equal(t, k) for t, k in zip(case["tensors"], keep))
    ld = C if dense else C + 32
    assert stage._p.grads[0].ldg == ld and stage._p.grads[1].ldg == C
    gx = stage._grad_bufs[0].view(B * r_big(C), ld)
    if not dense:
        assert bool((gx[:, C:] == torch.tensor(guard.WORD).to(gx.dtype)).all())
    assert stage.grads[0].shape == case["terms"][0].a.shape


def test_one_autograd_node_returns_every_gradient(cuda):
    """LossStageFn: total.backward() leaves the stage's gradients in the leaves, targets get none, and the prediction's gradient
    is written once although it is the first operand of two terms"""
    from diffusion_pruning_amd import autograd as AG, ops
    case = _case(cuda, 3, 8, "f32")
    x, y = case["terms"][0].a.requires_grad_(), case["terms"][1].a.requires_grad_()
    valid = torch.tensor([1.0, 1.0, 0.0], device=cuda)
    stage = ops.LossStage(case["terms"], COEF, weights=case["w"], valid=valid, group_div=DIV)
    total = AG.loss_stage(stage)
    assert total.grad_fn is not None and torch.equal(total.detach(), stage.out[2])
    (total * 2.0).backward()
    direct = [t.clone() for t in stage.backward(torch.tensor(2.0, device=cuda))]
    assert torch.equal(x.grad, direct[0]) and torch.equal(y.grad, direct[1])
    assert all(t.b.grad is None for t in case["terms"]) and case["w"].grad is None and valid.grad is None
    assert float(x.grad[2].abs().max()) == 0.0 and float(x.grad[:2].abs().min()) > 0.0


def test_captured_call_replays_to_the_eager_bits_next_to_a_busy_stream(cuda):
    from diffusion_pruning_amd import ops
    case = _case(cuda, 5, 64, "mixed", big_x=True)
    valid = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0], device=cuda)
    g = torch.tensor(0.75, device=cuda)
    noise = torch.randn(1 << 22, device=cuda)

    def busy():
        y = noise
        for _ in range(50):
            y = y * 1.0001 + 1.0
        return y
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        stage = ops.LossStage(case["terms"], COEF, weights=case["w"], valid=valid, group_div=DIV)
        stage.run(); stage.backward(g); busy()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    stage.run()
    eager = [stage.out.clone(), stage.sample_out.clone()] + [x.clone() for x in stage.backward(g)]
    g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1):
        stage.run()
        stage.backward(g)
    with torch.cuda.graph(g2):
        keep = busy()                                         # noqa: F841
    vals = []
    for _ in range(5):
        for x in stage.grads:
            x.fill_(7.0)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            g2.replay()
        g1.replay()
        vals.append([stage.out.clone(), stage.sample_out.clone()] + [x.clone() for x in stage.grads])
        torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(all(torch.equal(a, b) for a, b in zip(v, eager)) for v in vals)
    # the mask is device memory: the same graph follows a new one
    valid.copy_(torch.tensor([0.0, 1.0, 1.0, 0.0, 1.0]))
    g1.replay()
    torch.cuda.synchronize()
    assert float(stage.out[3]) == 3.0 and float(stage.grads[0][0].float().abs().max()) == 0.0 \
        and float(stage.grads[0][1].float().abs().max()) > 0.0


def test_sixteen_terms_of_1024_samples(cuda):
    """the largest table: the combine launch reads 16 * 1024 unit values from global memory"""
    from diffusion_pruning_amd import ops
    B = 1024
    pairs = [(_rand((B, 1, 8), BF, cuda, 100 + i), _rand((B, 1, 8), BF, cuda, 200 + i)) for i in range(16)]
    w = (torch.rand(B, generator=torch.Generator().manual_seed(7)) + 0.1).to(cuda)
    valid = (torch.rand(B, generator=torch.Generator().manual_seed(8)) < 0.7).float().to(cuda)
    terms = [ops.LossTerm(a, b, i % 4, 1.0, i == 0) for i, (a, b) in enumerate(pairs)]
    coef = (1.0, 2.0, 0.5, 0.25)
    stage = ops.LossStage(terms, coef, weights=w, valid=valid)
    out = stage.run().cpu()
    mt = [dict(a=_np(t.a), b=_np(t.b), group=t.group, scale=1.0, weighted=t.per_sample) for t in terms]
    fw = M.forward(mt, valid.cpu().tolist(), _np(w), coef)
    path = M.unit_ops(1, 8) + M.term_ops(B, True) + M.group_ops(4, False)
    for i in range(4):
        check(abs(float(out[i]) - fw["groups"][i]) / fw["groups"][i], path * EPS, "16 x 1024: group %d vs fp64" % i)
    check(abs(float(out[4]) - fw["total"]) / fw["total"], (path + M.total_ops(4)) * EPS, "16 x 1024: total vs fp64")
    assert float(out[5]) == float(valid.sum())
    with pytest.raises(AssertionError):
        ops.LossStage(terms + [terms[0]], coef, weights=w, valid=valid)


def test_bad_tables_return_einval(cuda):
    from diffusion_pruning_amd import _lib, ops
    from tests.test_loss_stage_host import bad_tables
    lib = _lib.load()
    for what, p, word, bwd_only in bad_tables():
        if not bwd_only:
            assert lib.aptp_loss_stage(ctypes.byref(p), None) == -1 and word in lib.aptp_last_error(), what
        assert lib.aptp_loss_stage_bwd(ctypes.byref(p), None) == -1 and word in lib.aptp_last_error(), what
    a, b = _rand((3, 4, 8), BF, cuda, 1), _rand((3, 4, 8), BF, cuda, 2)
    with pytest.raises(AssertionError, match="needs weights"):
        ops.LossStage([ops.LossTerm(a, b, 0, 1.0, True)], (1.0,))
    with pytest.raises(AssertionError, match="one shape"):
        ops.LossStage([ops.LossTerm(a, b, 0), ops.LossTerm(a[:2], b[:2], 0)], (1.0,))
    with pytest.raises(AssertionError, match="valid"):
        ops.LossStage([ops.LossTerm(a, b, 0)], (1.0,), valid=torch.ones(4, device=cuda))
    with pytest.raises(_lib.AptpError, match="group"):
        ops.LossStage([ops.LossTerm(a, b, 1)], (1.0,))
    torch.cuda.synchronize()
