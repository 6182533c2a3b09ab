"""GPU checks of aptp_loss_terms (csrc/loss_terms.hip, ops.LossTerms): every unweighted term and every per-sample mean has the
bits ops.mse gives the same views, the weighted sum / the groups / the total stay inside bounds derived from their operation
counts, the running totals are plain fp32 sums, nothing outside the outputs is written, and a captured call replays to the
eager bits next to a busy graph.  Nothing here provokes a fault: bad arguments are refused by the host validation
(tests/test_loss_terms_host.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
from tests.margins import check  # noqa: E402

EPS = 2.0 ** -24                  # unit roundoff of fp32
BF, F32 = torch.bfloat16, torch.float32
# vectors of 8 elements: one; the workgroup edge; aptp_mse_nblocks 1 -> 2; past the 1024-workgroup cap (grid stride)
VECTOR_COUNTS = [1, 255, 256, 257, 512, 513, 512 * 1024 + 8]


def _rand(shape, dtype, cuda, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(cuda, dtype)


def mse64(a, b):
    return float(((a.double() - b.double()) ** 2).mean())


def _ops_mse(ops, a, b):
    """ops.mse takes one dtype: a mixed pair goes through its fp32 casts (bf16 -> fp32 is exact)"""
    if a.dtype != b.dtype:
        return ops.mse(a.float(), b.float())
    return ops.mse(a, b)


@pytest.mark.parametrize("da,db", [(BF, BF), (F32, F32), (BF, F32)], ids=["bf16", "f32", "bf16_vs_f32"])
def test_single_term_has_the_bits_of_ops_mse(cuda, da, db):
    from diffusion_pruning_amd import ops
    for nv in VECTOR_COUNTS:
        a, b = _rand((nv, 8), da, cuda, nv), _rand((nv, 8), db, cuda, nv + 1)
        lt = ops.LossTerms([(a, b, 0)], (1.0,))
        assert lt.nblocks == ops._lib.load().aptp_mse_nblocks(nv, 8)
        out = lt.run()
        want = _ops_mse(ops, a, b)
        assert torch.equal(out[0], want), (nv, float(out[0]), float(want))
        assert torch.equal(out[1], want)                      # one group, coefficient 1
        assert abs(float(out[0]) - mse64(a, b)) <= 2e-6 * mse64(a, b)


def _strided_pairs(cuda):
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).to(cuda, BF)          # noqa: E731
    return {
        "slice": (r(2, 8, 8, 640), r(2, 8, 8, 960)[..., :640]),
        "nchw_face": (r(2, 8, 8, 640).permute(0, 3, 1, 2), r(2, 8, 8, 960)[..., :640].permute(0, 3, 1, 2)),
        "odd_rows": (r(3, 5, 7, 24), r(3, 5, 7, 24)),
    }


@pytest.mark.parametrize("case", ["slice", "nchw_face", "odd_rows"])
def test_strided_operands_are_read_in_place_like_ops_mse(cuda, case):
    from diffusion_pruning_amd import ops
    a, b = _strided_pairs(cuda)[case]
    if case != "odd_rows":
        assert not b.is_contiguous()
    a0, b0 = a.clone(), b.clone()
    out, _ = ops.loss_terms([(a, b, 0)], (1.0,))
    assert torch.equal(out[0], ops.mse(a, b))
    # the same strided bf16 operand against an fp32 one of the same shape, and the other way round
    bf = b.float().contiguous() if case != "nchw_face" else b.permute(0, 2, 3, 1).float().contiguous().permute(0, 3, 1, 2)
    out, _ = ops.loss_terms([(a, bf, 0)], (1.0,))
    assert torch.equal(out[0], ops.mse(a.float(), bf))
    out, _ = ops.loss_terms([(bf, a, 0)], (1.0,))
    assert torch.equal(out[0], ops.mse(bf, a.float()))
    assert torch.equal(a, a0) and torch.equal(b, b0)


@pytest.mark.parametrize("shape,dtype", [((3, 4, 8, 8), F32), ((3, 5, 7, 24), BF)], ids=["f32_nchw", "bf16_odd_rows"])
def test_weighted_term(cuda, shape, dtype):
    """B = 3 samples.  Per-sample means: ops.mse's bits.  Term: (1/B) sum_b w_b m_b in fp32, sequentially: B products, B - 1
    additions and one scale of positive numbers, each within 2^-24 relative -> (B + 2) 2^-24 of the exact value."""
    from diffusion_pruning_amd import ops
    B = shape[0]
    a, b = _rand(shape, dtype, cuda, 11), _rand(shape, dtype, cuda, 12)
    w = torch.tensor([0.3, 1.0, 0.017], device=cuda)
    lt = ops.LossTerms([ops.LossTerm(a, b, 0, 1.0, per_sample=True)], (1.0,), weights=w)
    out = lt.run()
    means = torch.stack([ops.mse(a[i], b[i]) for i in range(B)])
    assert torch.equal(lt.sample_out, means)
    exact = float((w.double() * means.double()).sum() / B)
    check(abs(float(out[0]) - exact) / exact, (B + 2) * EPS, "weighted term vs fp64 of the fp32 means and weights")


def _full_table(cuda, scale_blocks=1.0 / 9.0):
    """1 weighted + 9 block + 1 distillation term, the layout of a fine-tune validation step, with operands of different shapes,
    dtypes and strides"""
    from diffusion_pruning_amd import ops
    pred, target, full = _rand((3, 4, 8, 8), F32, cuda, 1), _rand((3, 4, 8, 8), F32, cuda, 2), _rand((3, 4, 8, 8), F32, cuda, 3)
    sp = _strided_pairs(cuda)
    blocks = [sp["slice"], sp["nchw_face"], sp["odd_rows"],
              (_rand((3, 4, 4, 32), BF, cuda, 4), _rand((3, 4, 4, 32), BF, cuda, 5)),
              (_rand((3, 2, 2, 64), BF, cuda, 6), _rand((3, 2, 2, 64), F32, cuda, 7)),
              (_rand((3, 16, 16, 320), BF, cuda, 8), _rand((3, 16, 16, 320), BF, cuda, 9)),          # 60 workgroups
              (_rand((513, 8), F32, cuda, 10), _rand((513, 8), BF, cuda, 11)),
              (_rand((3, 1, 1, 8), BF, cuda, 12), _rand((3, 1, 1, 8), BF, cuda, 13)),
              (_rand((3, 8, 8, 48), F32, cuda, 14), _rand((3, 8, 8, 48), F32, cuda, 15))]
    terms = [ops.LossTerm(pred, target, 0, 1.0, per_sample=True)]
    terms += [ops.LossTerm(x, y, 1, scale_blocks) for x, y in blocks]
    terms.append(ops.LossTerm(pred, full, 2))
    w = torch.tensor([0.3, 1.0, 0.017], device=cuda)
    return terms, w, (0.01, 0.5, 0.5)


def _exact_groups(terms, w):
    g = [0.0, 0.0, 0.0]
    for t in terms:
        if t.per_sample:
            v = sum(float(w[i]) * mse64(t.a[i], t.b[i]) for i in range(t.a.shape[0])) / t.a.shape[0]
        else:
            v = mse64(t.a, t.b)
        g[t.group] += v * float(torch.tensor(t.scale, dtype=F32))          # (the scale the kernel holds is fp32)
    return g


def test_full_table_against_fp64(cuda):
    from diffusion_pruning_amd import ops
    terms, w, coef = _full_table(cuda)
    lt = ops.LossTerms(terms, coef, weights=w)
    out = lt.run().cpu()
    exact = _exact_groups(terms, w)
    for g in range(3):
        # 2e-6: the tolerance of aptp_mse against fp64 (tests/test_bwd_ops_gpu.py); positive summands keep it for their sum
        check(abs(float(out[g]) - exact[g]) / exact[g], 2e-6, "group %d vs fp64" % g)
    total = sum(c * float(out[g]) for g, c in enumerate(coef))
    # three fp32 multiply-adds of positive numbers and the rounding of 0.01 to fp32
    check(abs(float(out[3]) - total) / total, 4 * EPS, "out[G] vs the fp64 combination of the fp32 groups")
    # every block term alone is ops.mse of the same views
    for t in terms[1:-1]:
        one, _ = ops.loss_terms([(t.a, t.b, 0)], (1.0,))
        want = ops.mse(t.a.float(), t.b.float()) if t.a.dtype != t.b.dtype else ops.mse(t.a, t.b)
        assert torch.equal(one[0], want)
    # scale 1 and group_div 9: the bits of the training step's (m_1 + .. + m_9) / 9
    terms1, _, _ = _full_table(cuda, scale_blocks=1.0)
    out1 = ops.LossTerms(terms1, coef, weights=w, group_div=(0, 9, 0)).run()
    blk = torch.zeros((), device=cuda)
    for t in terms1[1:-1]:
        blk = blk + (ops.mse(t.a.float(), t.b.float()) if t.a.dtype != t.b.dtype else ops.mse(t.a, t.b))
    assert torch.equal(out1[1], blk / 9)
    assert torch.equal(out1[2], ops.mse(terms1[-1].a, terms1[-1].b)) and torch.equal(out1[0], out.to(cuda)[0])


def test_sixteen_terms_and_one_term(cuda):
    from diffusion_pruning_amd import ops
    pairs = [(_rand((5 + i, 8 * (1 + i % 3)), BF if i % 2 else F32, cuda, 40 + i),
              _rand((5 + i, 8 * (1 + i % 3)), BF if i % 3 else F32, cuda, 80 + i)) for i in range(16)]
    terms = [ops.LossTerm(a, b, i % 4, 1.0) for i, (a, b) in enumerate(pairs)]
    coef = (1.0, 2.0, 0.5, 0.25)
    out = ops.LossTerms(terms, coef).run()
    for g in range(4):
        want = torch.zeros((), device=cuda)
        for i in range(g, 16, 4):                             # index order; scale 1: plain fp32 additions
            want = want + _ops_mse(ops, *pairs[i])
        assert torch.equal(out[g], want), g
    exact = sum(c * float(out[g]) for g, c in enumerate(coef))
    check(abs(float(out[4]) - exact) / exact, 4 * EPS, "16 terms: out[G] vs fp64 of the fp32 groups")
    with pytest.raises(AssertionError):
        ops.LossTerms(terms + [terms[0]], coef)
    a, b = pairs[3]
    out = ops.LossTerms([ops.LossTerm(a, b, 0, 1.0)], (0.5,)).run()
    assert torch.equal(out[0], _ops_mse(ops, a, b)) and torch.equal(out[1], out[0] * 0.5)


class _Guarded:
    """LossTerms whose buffers sit between guard words"""
    PAD, WORD = 8, 12345.0

    def __init__(self):
        self.bufs = []

    def alloc(self, n, device):
        buf = torch.full((n + 2 * self.PAD,), self.WORD, dtype=F32, device=device)
        self.bufs.append((buf, n))
        return buf[self.PAD:self.PAD + n]

    def intact(self):
        return all(bool((b[:self.PAD] == self.WORD).all()) and bool((b[self.PAD + n:] == self.WORD).all()) for b, n in self.bufs)


def test_running_totals_guards_and_operands(cuda):
    from diffusion_pruning_amd import ops
    terms, w, coef = _full_table(cuda)
    guard = _Guarded()

    class LT(ops.LossTerms):
        _alloc = staticmethod(guard.alloc)

    running = guard.alloc(5, cuda)
    running.zero_()
    lt = LT(terms, coef, weights=w, running=running)
    assert len(guard.bufs) == 4                               # running, partial, out, sample_out
    outs = []
    for k in range(3):
        for t in terms:                                       # different inputs on every call, same addresses
            if k:
                t.a.mul_(1.25)
        before = [(t.a.clone(), t.b.clone()) for t in terms]
        outs.append(lt.run().clone())
        assert all(torch.equal(t.a, x) and torch.equal(t.b, y) for t, (x, y) in zip(terms, before))
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    assert torch.equal(running[:4], (outs[0] + outs[1]) + outs[2])
    assert float(running[4]) == 3.0
    assert guard.intact()
    # a NaN in the distillation operand: its group and the total go NaN, the other slots and the count do not
    running.zero_()
    full = terms[-1].b
    for k in range(3):
        if k == 1:
            keep = full[0, 0, 0, 0].clone()
            full[0, 0, 0, 0] = float("nan")
        lt.run()
        if k == 1:
            full[0, 0, 0, 0] = keep
    r = running.cpu()
    assert torch.isnan(r[2]) and torch.isnan(r[3]) and torch.isfinite(r[:2]).all() and float(r[4]) == 3.0
    assert guard.intact()


def test_captured_call_replays_to_the_eager_bits_next_to_a_busy_graph(cuda):
    """the pattern of test_mse_inside_replayed_graphs_matches_eager (tests/test_bwd_ops_gpu.py)"""
    from diffusion_pruning_amd import ops
    terms, w, coef = _full_table(cuda)
    terms[6] = ops.LossTerm(_rand((2, 64, 64, 320), BF, cuda, 20), _rand((2, 64, 64, 320), BF, cuda, 21), 1, 1.0 / 9.0)
    running = torch.zeros(5, device=cuda)
    noise = torch.randn(1 << 22, device=cuda)

    def busy():
        y = noise
        for _ in range(50):
            y = y * 1.0001 + 1.0
        return y
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lt = ops.LossTerms(terms, coef, weights=w, running=running)
        lt.run(); busy()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager, eager_samples = lt.run().clone(), lt.sample_out.clone()
    running.zero_()
    g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1):
        lt.run()
    with torch.cuda.graph(g2):
        keep = busy()                                         # noqa: F841
    vals = []
    for _ in range(8):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            g2.replay()
        g1.replay()
        vals.append((lt.out.clone(), lt.sample_out.clone()))
        torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(o, eager) and torch.equal(s, eager_samples) for o, s in vals)
    want = torch.zeros(4, device=cuda)
    for _ in range(8):
        want = want + eager
    assert float(running[4]) == 8.0 and torch.equal(running[:4], want)


def test_operands_ops_mse_can_only_copy_are_staged_once_and_follow_their_source(cuda):
    """what the fine-tuning forward hands over: the 4-channel NCHW face of an fp32 [B, H, W, 8] conv output, against NCHW
    targets.  ops.mse walks the pair in the prediction's memory order through copies; LossTerms keeps one staging tensor per
    distinct view (the prediction's is shared by both terms) and refreshes it on every run"""
    from diffusion_pruning_amd import ops
    y = _rand((3, 16, 16, 8), F32, cuda, 30)
    pred = y[..., :4].permute(0, 3, 1, 2)
    target, full = _rand((3, 4, 16, 16), F32, cuda, 31), _rand((3, 4, 16, 16), F32, cuda, 32)
    w = torch.tensor([0.3, 1.0, 0.017], device=cuda)
    lt = ops.LossTerms([ops.LossTerm(pred, target, 0, 1.0, per_sample=True), ops.LossTerm(pred, full, 1)], (1.0, 1.0), weights=w)
    assert len(lt.copies) == 3
    for k in range(2):
        if k:
            y.mul_(0.5); target.add_(1.0); full.sub_(0.25)
        keep = (y.clone(), target.clone(), full.clone())
        out = lt.run()
        assert torch.equal(lt.sample_out, torch.stack([ops.mse(pred[i], target[i]) for i in range(3)])), k
        assert torch.equal(out[1], ops.mse(pred, full)), k
        assert torch.equal(y, keep[0]) and torch.equal(target, keep[1]) and torch.equal(full, keep[2])
    # operands ops.mse reads in place get no staging
    a, b = _strided_pairs(cuda)["nchw_face"]
    assert ops.LossTerms([(a, b, 0)], (1.0,)).copies == []
