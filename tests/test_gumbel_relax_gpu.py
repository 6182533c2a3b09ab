"""GPU checks of the router's seeded Gumbel relaxation (csrc/gumbel_relax.hip, ops.GumbelRelax, ops.philox_gumbel,
autograd.gumbel_relax) against the fp64 model (tests/gumbel_relax_model.py).

Noise words are bit-equal to the oracle.  Values are compared with fp64 under the project's rule: twice what the
existing fp32 relaxation (quantizer.gumbel_sigmoid_trick, run on the GPU on the same noise) needs, plus
64 * 2^-24 * max(1, |value|); gradients the same way on rel-L2.  The non-zero-width decision must be the model's on every (row,
segment) whose entries all have |z + G + base| >= 1e-4, and at most 1 % of the pairs may be left out."""
import numpy as np
import pytest
import torch

from oracle import unet_oracle as O
from tests import gumbel_relax_model as M
from tests.test_train_step_gpu import DEPTH_ORDER

pytestmark = pytest.mark.gpu
from tests.margins import check  # noqa: E402

FLOOR = 64 * 2.0 ** -24
T, BASE = 0.4, 3.0
MARGIN = 1e-4
D, SUB = 3, 7                     # the batch's draw and the sub-draw: Philox draw 8 * 3 + 7


def _sd21_widths():
    st = O.get_structure(O.SD21)
    widths = [w for sub in st["width"] for w in sub]
    assert sum(d for sub in st["depth"] for d in sub) == len(DEPTH_ORDER)
    return tuple(widths)


SHAPES = {"1x3x1": (1, (3,), [0]), "5x49x3": (5, (4, 1, 7, 32, 5), [-1, 0, 1]), "8xsd21": (8, None, DEPTH_ORDER),
          "64xsd21": (64, None, DEPTH_ORDER)}
_REF = {}


def _np(t):
    return t.detach().double().cpu().numpy()


def _rel_l2(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def reference(shape, variant):
    """inputs, the fp64 model's outputs and gradient: computed once per case, shared, left unchanged"""
    key = (shape, variant)
    if key in _REF:
        return _REF[key]
    R, widths, order = SHAPES[shape]
    widths = list(_sd21_widths() if widths is None else widths)
    if variant == "odd" and sum(widths) % 2 == 0:
        widths[-1] -= 1                                               # an odd width sum: the depth block starts at an odd column
    nw, nd = sum(widths), len(order)
    g = torch.Generator().manual_seed(5)
    z = 2 * torch.randn(R, nw + nd, generator=g)
    dout = torch.randn(R, nw + nd, generator=g)
    starts = M.seg_starts(widths)
    forced = []
    if variant == "dead3":
        forced = sorted({0, len(widths) // 2, len(widths) - 1})
        for s in forced:
            z[:, starts[s]:starts[s + 1]] = -60.0
    seeds = [1000 + 7 * i for i in range(R)]
    nzw = variant != "off"
    words = M.words(seeds, M.philox_draw(D, SUB), nw + nd)
    G64 = torch.from_numpy(M.gumbel(words))
    z64 = z.double().requires_grad_(True)
    out, dead, margin = M.forward(z64, G64, widths, order, T, BASE, nzw)
    out.backward(dout.double())
    ref = dict(R=R, widths=widths, order=order, nw=nw, nd=nd, z=z, dout=dout, seeds=seeds, nzw=nzw, words=words, G64=G64,
               out=out.detach().numpy(), dead=dead.numpy(), close=(margin < MARGIN).numpy(), dz=z64.grad.numpy(), starts=starts,
               forced=forced)
    _REF[key] = ref
    return ref


def _elementwise(err, scale, e_torch, what):
    """err <= 2 e_torch + FLOOR max(1, |value|) on every element, recorded as the largest share of its bound any element uses"""
    return check(float((err / (2 * e_torch + FLOOR * np.maximum(1.0, np.abs(scale)))).max()), 1.0, what)


@pytest.mark.parametrize("variant", ["on", "off", "dead3", "odd"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forward_and_backward_against_fp64(cuda, shape, variant):
    from diffusion_pruning_amd import ops
    c = reference(shape, variant)
    R, nw, nd, widths, order, starts = c["R"], c["nw"], c["nd"], c["widths"], c["order"], c["starts"]
    what = "%s %s" % (shape, variant)
    z, dout = c["z"].to(cuda), c["dout"].to(cuda)
    seeds_dev = torch.tensor(c["seeds"], dtype=torch.int64, device=cuda)
    draw_dev = torch.tensor([D], dtype=torch.int64, device=cuda)
    # the noise: words bit for bit, values under the rule
    w = ops.philox_gumbel((R, nw + nd), seeds_dev, draw_dev, SUB, words=True).cpu().numpy().view(np.uint32)
    assert np.array_equal(w, c["words"]), what
    G = ops.philox_gumbel((R, nw + nd), seeds_dev, draw_dev, SUB)
    G32 = M.torch_noise(c["words"], device=cuda)
    G64 = c["G64"].numpy()
    eG_torch = float(np.abs(_np(G32) - G64).max())
    print("%s: G max error kernel %.3e torch %.3e" % (what, np.abs(_np(G) - G64).max(), eG_torch))
    _elementwise(np.abs(_np(G) - G64), G64, eG_torch, "%s: G vs fp64" % what)
    # the existing fp32 relaxation on the GPU on the same noise
    qz = M.make_quantizer(widths, order, T, BASE, c["nzw"]).to(cuda)
    z32 = z.clone().requires_grad_(True)
    ref = M.torch_relax(qz, z32, G32)
    ref.backward(dout)
    stage = ops.GumbelRelax(widths, order, T, BASE, c["nzw"], R, cuda)
    out = _np(stage.run(z, seeds_dev, draw_dev, SUB))
    dz = _np(stage.backward(dout))
    # the decision: the model's wherever it was not taken within the margin; at most 1 % of the pairs left out
    close, dead = c["close"], c["dead"]
    print("%s: %d of %d (row, segment) pairs within the margin" % (what, close.sum(), close.size))
    assert close.mean() <= 0.01, what
    firsts = starts[:-1]
    excess = out[:, firsts] - c["out"][:, firsts]                      # ~0 where the decisions agree, +-0.5 where they differ
    assert (np.abs(excess)[~close] < 0.25).all(), what
    if c["nzw"]:
        unbumped = c["out"][:, firsts] - 0.5 * dead
        got_dead = (out[:, firsts] - unbumped) > 0.25
        assert np.array_equal(got_dead[~close], dead[~close]), what
        assert dead[:, c["forced"]].all()
    else:
        assert (out[:, :nw] < 1.0 + 1e-6).all() and not (np.abs(excess) > 0.25).any()
    keep = np.ones(out.shape, dtype=bool)
    for r, s in zip(*np.nonzero(close)):
        keep[r, starts[s]] = False
    for name, sl in (("w", slice(0, nw)), ("d", slice(nw, nw + nd))):
        e_torch = float((np.abs(_np(ref) - c["out"])[:, sl] * keep[:, sl]).max())
        err = np.abs(out - c["out"])[:, sl] * keep[:, sl]
        print("%s: %s max error kernel %.3e torch %.3e" % (what, name, err.max(), e_torch))
        _elementwise(err, c["out"][:, sl], e_torch, "%s: %s vs fp64" % (what, name))
    e_kernel, e_torch = _rel_l2(dz, c["dz"]), _rel_l2(_np(z32.grad), c["dz"])
    print("%s: dz rel-L2 kernel %.3e torch %.3e" % (what, e_kernel, e_torch))
    check(e_kernel, 2 * e_torch + FLOOR, "%s: dz rel-L2 vs fp64 autograd" % what)
    # dead segments: exactly + 0.5f on the first entry against the rule switched off, and only there
    if variant == "dead3":
        out32 = stage.out.cpu().numpy()
        off = ops.GumbelRelax(widths, order, T, BASE, False, R, cuda).run(z, seeds_dev, draw_dev, SUB).cpu().numpy()
        off_dead = np.stack([(off[:, a:b] < 0.5).all(axis=1) for a, b in zip(starts[:-1], starts[1:])], axis=1)
        want = off.copy()
        want[:, firsts] = np.where(off_dead, off[:, firsts] + np.float32(0.5), off[:, firsts])
        assert np.array_equal(out32, want), what
        assert off_dead[:, c["forced"]].all()


def test_draws_seeds_and_offsets(cuda):
    """sub 6, the codebook draw (top bit set), seeds above 2^32 and from 2^63 up, offsets that are no multiples of 4"""
    from diffusion_pruning_amd import ops
    seeds = [7, (1 << 40) + 12345, (1 << 63) + 99, -5]
    n = 37
    for d, sub, codebook, offset in ((3, 6, False, 0), (3, 7, False, 5), ((1 << 58) + 1, 6, False, 3), (11, 7, True, 0), (0, 7, True, 6)):
        w = ops.philox_gumbel((4, n), seeds, d, sub, offset, codebook=codebook, words=True, device=cuda).cpu().numpy().view(np.uint32)
        want = M.words([s & ((1 << 64) - 1) for s in seeds], M.philox_draw(d, sub, codebook), n, offset)
        assert np.array_equal(w, want), (d, sub, codebook, offset)
    a = ops.philox_gumbel((4, n), seeds, 3, 6, device=cuda)
    b = ops.philox_gumbel((4, n), seeds, 3, 7, device=cuda)
    c = ops.philox_gumbel((4, n), seeds, 3, 7, codebook=True, device=cuda)
    assert not torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(b, c)
    assert torch.equal(ops.philox_gumbel((4, n - 5), seeds, 3, 7, 5, device=cuda), b[:, 5:])
    for bad in (dict(sub=5), dict(draw=-1), dict(draw=1 << 59), dict(offset=-1)):
        kw = dict(draw=3, sub=7, offset=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.philox_gumbel((4, n), seeds, kw["draw"], kw["sub"], kw["offset"], device=cuda)


def test_rows_do_not_depend_on_their_batch(cuda):
    from diffusion_pruning_amd import ops
    c = reference("5x49x3", "on")
    z = c["z"].to(cuda)
    draw_dev = torch.tensor([D], dtype=torch.int64, device=cuda)
    seeds = torch.tensor(c["seeds"], dtype=torch.int64, device=cuda)
    full = ops.GumbelRelax(c["widths"], c["order"], T, BASE, True, 5, cuda).run(z, seeds, draw_dev, SUB).clone()
    one = ops.GumbelRelax(c["widths"], c["order"], T, BASE, True, 1, cuda)
    for r in range(5):
        assert torch.equal(one.run(z[r:r + 1].contiguous(), seeds[r:r + 1].contiguous(), draw_dev, SUB)[0], full[r])
    perm = torch.tensor([3, 0, 4, 1, 2], device=cuda)
    again = ops.GumbelRelax(c["widths"], c["order"], T, BASE, True, 5, cuda).run(z[perm].contiguous(), seeds[perm].contiguous(), draw_dev, SUB)
    assert torch.equal(again, full[perm])


def test_capture_and_replay(cuda):
    from diffusion_pruning_amd import ops
    c = reference("8xsd21", "on")
    R = c["R"]
    z, dout = c["z"].to(cuda), c["dout"].to(cuda)
    seeds_dev = torch.tensor(c["seeds"], dtype=torch.int64, device=cuda)
    draw_dev = torch.tensor([D], dtype=torch.int64, device=cuda)
    stage = ops.GumbelRelax(c["widths"], c["order"], T, BASE, True, R, cuda)
    eager = (stage.run(z, seeds_dev, draw_dev, SUB).clone(), stage.backward(dout).clone())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        stage.run(z, seeds_dev, draw_dev, SUB)
        stage.backward(dout)
    seen = []
    for _ in range(2):
        stage.out.zero_()
        stage.dz.zero_()
        g.replay()
        seen.append((stage.out.clone(), stage.dz.clone()))
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])
    assert torch.equal(seen[0][0], eager[0]) and torch.equal(seen[0][1], eager[1])
    # the seeds and the draw are read at launch time
    draw_dev.fill_(9)
    seeds_dev.copy_(torch.tensor([5 * i + 1 for i in range(R)], dtype=torch.int64, device=cuda))
    g.replay()
    replayed = (stage.out.clone(), stage.dz.clone())
    other = ops.GumbelRelax(c["widths"], c["order"], T, BASE, True, R, cuda)
    want = (other.run(z, seeds_dev.clone(), torch.tensor([9], dtype=torch.int64, device=cuda), SUB), other.backward(dout))
    assert torch.equal(replayed[0], want[0]) and torch.equal(replayed[1], want[1])
    assert not torch.equal(replayed[0], eager[0])


def test_the_quantiser_takes_a_noise_source(cuda):
    """gumbel_sigmoid_trick(z, noise) is the one stage as one autograd node; forward(noise=) sends its two calls through the
    codebook draw and sub-draw 6 -- with as many samples as codes, so the calls of a step share a row count"""
    from diffusion_pruning_amd.quantizer import RouterNoise, StructureVectorQuantizer
    widths, order = (4, 1, 7, 32, 5), [-1, 0, 1]
    structure = {"width": [[w] for w in widths], "depth": [[1], [1], [1], [0], [0]]}
    torch.manual_seed(3)
    qz = StructureVectorQuantizer(n_e=4, structure=structure, temperature=T, base=BASE, depth_order=order,
                                  resource_aware_normalization=False).to(cuda).train()
    noise = RouterNoise.of([11, 12, 13, 14], 3, 500, 2, 4, cuda)
    assert noise.code_seeds_dev.tolist() == [500, 501, 502, 503] and noise.step_dev.tolist() == [2]
    z = (2 * torch.randn(4, 52, device=cuda)).requires_grad_(True)
    out = qz.gumbel_sigmoid_trick(z, noise.samples(7))
    want, _, _, G = M.relax(z, [11, 12, 13, 14], 3, 7, widths, order, T, BASE)
    assert float((out.detach().double().cpu() - want).abs().max()) < 1e-5
    dout = torch.randn(4, 52, device=cuda)
    out.backward(dout)
    z64 = z.detach().double().cpu().requires_grad_(True)
    M.forward(z64, G, widths, order, T, BASE)[0].backward(dout.double().cpu())
    assert _rel_l2(_np(z.grad), z64.grad.numpy()) < 1e-5
    # the whole forward: codes from the codebook draw with the gradient reaching the codebook, indices from sub-draw 6
    z_q, (_, _, idx) = qz(z.detach(), noise=noise)
    codes, _, _, _ = M.relax(qz.embedding.weight, [500, 501, 502, 503], 2, 7, widths, order, T, BASE, codebook=True)
    assert float((z_q.detach().double().cpu() - codes[idx.cpu()]).abs().max()) < 1e-5
    assert float((qz.embedding_gs.double().cpu() - codes).abs().max()) < 1e-5
    z_q.sum().backward()
    assert qz.embedding.weight.grad is not None and float(qz.embedding.weight.grad.abs().max()) > 0
    again, (_, _, idx2) = qz(z.detach(), noise=noise)
    assert torch.equal(again, z_q) and torch.equal(idx, idx2)                         # no hidden state: the same bits
    qz.eval()
    with pytest.raises(ValueError, match="eval mode"):
        qz(z.detach(), noise=noise)
    with pytest.raises(ValueError, match="eval mode"):
        qz.gumbel_sigmoid_trick(z.detach(), noise.samples(7))


def test_stage_refuses_bad_geometry(cuda):
    from diffusion_pruning_amd import ops
    for kw in (dict(widths=(4, 0, 3)), dict(order=[0, 0]), dict(rows=0), dict(rows=65536), dict(widths=(4096,)), dict(T=0.0),
               dict(order=list(range(65)))):
        a = dict(widths=(4, 3), order=[1, 0], rows=2, T=T)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.GumbelRelax(a["widths"], a["order"], a["T"], BASE, True, a["rows"], cuda)
    with pytest.raises(ValueError):
        ops.GumbelRelax((4, 3), [1, 0], T, BASE, True, 2, "cpu")
    stage = ops.GumbelRelax((4, 3), [1, 0], T, BASE, True, 2, cuda)
    z = torch.zeros(2, 9, device=cuda)
    seeds, draw = torch.zeros(2, dtype=torch.int64, device=cuda), torch.zeros(1, dtype=torch.int64, device=cuda)
    for bad in ((z[:, :8], seeds, draw, 7), (z.double(), seeds, draw, 7), (z, seeds[:1], draw, 7), (z, seeds, draw.int(), 7),
                (z, seeds, draw, 5), (z.cpu(), seeds, draw, 7)):
        with pytest.raises(ValueError):
            stage.run(*bad)
    with pytest.raises(RuntimeError):
        stage.backward(z)
