"""aptp_philox_normal (csrc/philox_normal.hip) on the GPU against the numpy oracle (tests/philox_oracle.py): the words bit for
bit, the normals against Box-Muller in fp64, the output forms, independence of the batch, capture and refusals.

Bound of the normals (derived, not measured): the uniforms are exact in fp32; u1 >= 2^-24 gives |z| <= sqrt(48 ln 2) = 5.77;
logf, sinpif and cospif are accurate to 1-2 ulp and sqrtf to 1 ulp (ROCm's documented device accuracies), so a few ulp of the
factors of a value below 5.77 stays under about 2e-6.  NORMAL_TOL is twice that, about 1e-6 of a unit normal.  A measured value
above it means that an approximate intrinsic or a contraction has crept into the kernel."""
import itertools

import numpy as np
import pytest
import torch

from tests import philox_oracle as PO
from tests.margins import check

pytestmark = pytest.mark.gpu

NORMAL_TOL = 4e-6
SEEDS = [0, 1234, 2 ** 63 - 1, -1]
DRAWS = [0, 1, 2 ** 32, 2 ** 40 + 3]
OFFSETS = [0, 1, 2, 3, 2 ** 34 - 4]      # the last: the block counter carries into its high word inside an 8-element row
NS = [1, 3, 4, 5, 7, 64, 1027]
BS = [1, 3]
N_LATENT = 4 * 64 * 64


def wrap(v):
    v &= 2 ** 64 - 1
    return v - 2 ** 64 if v >= 2 ** 63 else v


def row_seeds(seed, b):
    """b distinct seeds derived from one"""
    return [wrap(seed + r * 0x9E3779B97F4A7C15) for r in range(b)]


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def cases():
    return itertools.product(SEEDS, DRAWS, OFFSETS, NS, BS)


def test_bits_equal_the_oracle(cuda):
    from diffusion_pruning_amd import ops
    bad = []
    for seed, draw, off, n, b in cases():
        sd = row_seeds(seed, b)
        got = u32(ops.philox_bits((b, n), sd, draw, offset=off, device=cuda))
        if not np.array_equal(got, PO.bits_rows(sd, draw, off, n)):
            bad.append((seed, draw, off, n, b))
    assert not bad, bad[:10]
    # out as a view one element into a buffer: 4-byte aligned only, every element on the single-element path
    for off, n, b in itertools.product(OFFSETS, NS, BS):
        sd = row_seeds(1234, b)
        buf = torch.full((b * n + 2,), 7, dtype=torch.int32, device=cuda)
        out = buf[1:1 + b * n].view(b, n)
        assert ops.philox_bits((b, n), sd, 1, offset=off, out=out) is out
        assert np.array_equal(u32(out), PO.bits_rows(sd, 1, off, n)), (off, n, b)
        assert int(buf[0]) == 7 and int(buf[-1]) == 7                     # nothing written outside
    # a device tensor of seeds and an int shared by all rows
    t = torch.tensor(row_seeds(5, 3), dtype=torch.int64, device=cuda)
    assert np.array_equal(u32(ops.philox_bits((3, 9), t, 2)), PO.bits_rows(row_seeds(5, 3), 2, 0, 9))
    assert np.array_equal(u32(ops.philox_bits((3, 9), 5, 2, device=cuda)), PO.bits_rows([5, 5, 5], 2, 0, 9))
    # seeds from 2^63 up are their two's complement
    assert torch.equal(ops.philox_bits((1, 8), [2 ** 64 - 1], device=cuda), ops.philox_bits((1, 8), [-1], device=cuda))


def test_normals_against_the_fp64_oracle(cuda):
    from diffusion_pruning_amd import ops
    worst, where = 0.0, None
    big = [(s, d, o, N_LATENT, b) for s, d, o, b in [(0, 0, 0, 1), (1234, 1, 0, 3), (2 ** 63 - 1, 2 ** 40 + 3, 2 ** 34 - 4, 1), (-1, 2 ** 32, 3, 3)]]
    for seed, draw, off, n, b in itertools.chain(cases(), big):
        sd = row_seeds(seed, b)
        got = ops.randn((b, n), sd, draw, offset=off, device=cuda)
        assert got.dtype == torch.float32 and got.shape == (b, n)
        e = float(np.abs(got.cpu().numpy().astype(np.float64) - PO.normals_rows(sd, draw, off, n)).max())
        if e > worst:
            worst, where = e, (seed, draw, off, n, b)
    print(f"normals vs fp64 oracle: max abs error {worst:.3e} at {where}")
    check(worst, NORMAL_TOL, "philox normals vs fp64 oracle, max abs error")


def test_a_latent_shaped_draw_is_standard_normal(cuda):
    from diffusion_pruning_amd import ops
    z = ops.randn((8, 4, 64, 64), list(range(8)), device=cuda)
    assert z.shape == (8, 4, 64, 64) and torch.isfinite(z).all()
    N = z.numel()
    assert abs(float(z.mean())) * N ** 0.5 <= 4.0 and abs(float(z.var()) - 1.0) * (N / 2) ** 0.5 <= 4.0


def test_output_forms(cuda):
    from diffusion_pruning_amd import ops
    for (b, n), off in itertools.product([(1, 5), (3, 64), (2, 1027), (2, N_LATENT)], [0, 3]):
        sd = row_seeds(99, b)
        z = ops.randn((b, n), sd, 4, offset=off, device=cuda)
        assert torch.equal(ops.randn((b, n), sd, 4, offset=off, dtype=torch.bfloat16, device=cuda), z.bfloat16())
        assert torch.equal(ops.randn((b, n), sd, 4, offset=off, scale=0.37, device=cuda), torch.tensor(0.37, device=cuda) * z)
        out = torch.empty(b, n, device=cuda)
        assert ops.randn((b, n), sd, 4, offset=off, out=out) is out and torch.equal(out, z)
        if off == 0:
            base = torch.randn(b, n, device=cuda)
            sdt = torch.tensor(sd, dtype=torch.int64, device=cuda)
            draw, scale = torch.tensor([4], device=cuda), torch.tensor([0.6180339], device=cuda)
            want = base + scale * z
            keep = base.clone()
            apart = ops.add_noise(base, sdt, draw, scale)
            assert torch.equal(apart, want) and torch.equal(base, keep) and apart.data_ptr() != base.data_ptr()
            assert ops.add_noise(base, sdt, draw, scale, out=base) is base and torch.equal(base, want)
    # a 4-d base, as the loops pass it
    base = torch.randn(2, 4, 16, 16, device=cuda)
    sdt = torch.tensor([3, 4], dtype=torch.int64, device=cuda)
    got = ops.add_noise(base, sdt, torch.tensor([2], device=cuda), torch.tensor([0.25], device=cuda))
    assert torch.equal(got, base + torch.tensor(0.25, device=cuda) * ops.randn((2, 4, 16, 16), sdt, 2))


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_an_offset_split_equals_the_whole(cuda, k):
    from diffusion_pruning_amd import ops
    for n in (7, 64, 1027):
        whole = ops.randn((1, n), 1234, 1, device=cuda)
        assert torch.equal(whole[:, k:], ops.randn((1, n - k), 1234, 1, offset=k, device=cuda)), n
        wb = ops.philox_bits((1, n), 1234, 1, device=cuda)
        assert torch.equal(wb[:, k:], ops.philox_bits((1, n - k), 1234, 1, offset=k, device=cuda)), n


def test_rows_do_not_depend_on_the_batch(cuda):
    from diffusion_pruning_amd import ops
    sd = [11, -5, 2 ** 63 - 1, 0, 11]
    for n in (5, 64, 1027):                                               # n % 4 != 0: rows off the block grid; == 0: on it
        together = ops.randn((5, n), sd, 3, device=cuda)
        for r, s in enumerate(sd):
            assert torch.equal(together[r:r + 1], ops.randn((1, n), [s], 3, device=cuda)), (n, r)
        assert torch.equal(together[0], together[4])
        perm = [3, 0, 4, 2, 1]
        assert torch.equal(ops.randn((5, n), [sd[i] for i in perm], 3, device=cuda), together[perm])


def test_one_captured_launch_follows_draw_and_seeds(cuda):
    from diffusion_pruning_amd import ops
    base = torch.randn(3, 4, 16, 16, device=cuda)
    seeds = torch.tensor([1, 2, 3], dtype=torch.int64, device=cuda)
    draw, scale = torch.tensor([1], device=cuda), torch.tensor([0.5], device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.add_noise(base, seeds, draw, scale)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.add_noise(base, seeds, draw, scale)
    for sd, sc in (([1, 2, 3], 0.5), ([9, 2 ** 63 - 1, -4], 1.25)):
        seeds.copy_(torch.tensor(sd, dtype=torch.int64))
        scale.fill_(sc)
        for d in (1, 2, 3):
            draw.fill_(d)
            graph.replay()
            first = out.clone()
            assert torch.equal(first, ops.add_noise(base, seeds, draw, scale)), (sd, d)
            assert torch.equal(first, base + scale * ops.randn(base.shape, sd, d, device=cuda))
            graph.replay()
            assert torch.equal(out, first)
    torch.cuda.synchronize()


def test_refusals_leave_out_untouched(cuda):
    from diffusion_pruning_amd import ops
    out = torch.full((2, 8), 3.0, device=cuda)
    keep = out.clone()
    sd = torch.tensor([1, 2], dtype=torch.int64, device=cuda)
    one = torch.tensor([1], device=cuda)
    sc = torch.tensor([1.0], device=cuda)
    bad = [
        lambda: ops.randn((2, 8), [1, 2, 3], out=out),                              # seed count
        lambda: ops.randn((2, 8), torch.tensor([1, 2, 3], device=cuda), out=out),
        lambda: ops.randn((2, 8), sd.int(), out=out),                               # seed dtype
        lambda: ops.randn((2, 8), sd.cpu(), out=out),                               # seed device
        lambda: ops.randn((2, 8), [1.5, 2], out=out),
        lambda: ops.randn((2, 8), sd, -1, out=out),                                 # negative draw
        lambda: ops.randn((2, 8), sd, offset=-1, out=out),                          # negative offset
        lambda: ops.randn((2, 4), sd, out=out),                                     # shape
        lambda: ops.randn((2, 8), sd, dtype=torch.bfloat16, out=out),               # dtype of out
        lambda: ops.randn((2, 8), sd, dtype=torch.float16),
        lambda: ops.randn((2, 0), sd),                                              # n = 0
        lambda: ops.randn((2, 8), sd, device="cpu"),
        lambda: ops.randn((2, 4), sd, out=out.t()[:4].t()),                         # non-contiguous
        lambda: ops.philox_bits((2, 8), sd, out=out),                               # the raw words are int32
        lambda: ops.add_noise(out, sd[:1], one, sc, out=out),
        lambda: ops.add_noise(out, sd, one.int(), sc, out=out),
        lambda: ops.add_noise(out, sd, one, sc.double(), out=out),
        lambda: ops.add_noise(out, sd, one.cpu(), sc, out=out),
        lambda: ops.add_noise(out, sd, one, None, out=out),
        lambda: ops.add_noise(out.t(), sd, one, sc),
        lambda: ops.add_noise(out.bfloat16(), sd, one, sc),
        lambda: ops.add_noise(out, sd, one, sc, out=out[:1]),
        lambda: ops.add_noise(out.cpu(), sd, one, sc),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"refusal {i} ran")
        assert torch.equal(out, keep), i
