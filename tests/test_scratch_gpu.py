"""The split-K counter pool grows (diffusion_pruning_amd/scratch.py): the form and the bits of a launch do not depend on how many
(stream, domain) keys the process used before it.  The launch is the smallest split-K case of tests/test_ops_gpu.py
(test_splitk_in_kernel_matches_reduce_launch_bitwise_and_is_stable); the reference bits are its reduce-launch form."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

N_KEYS = 40           # the pool used to hold 16 slabs per device and never grew
B, H, CIN, COUT, K, TILE, SPLIT_K = 1, 24, 64, 200, 3, 12, 3


def nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def ops(cuda):
    from diffusion_pruning_amd import ops as o
    o._lib.load()
    return o


@pytest.fixture(scope="module")
def many_keys(ops, cuda):
    """the launch under N_KEYS scratch domains in turn on the current stream: operands, the reduce-launch reference, and per
    domain (output, tile_counters of the launch, its counter slab)"""
    g = torch.Generator().manual_seed(B * H + CIN + COUT)

    def rand(shape, scale=1.0):
        return torch.randn(shape, generator=g) * scale
    x = nhwc(rand((B, CIN, H, H))).bfloat16().to(cuda)
    res = nhwc(rand((B, COUT, H, H))).bfloat16().to(cuda)
    pw = ops.pack_weight(rand((COUT, CIN, K, K), 1.0 / math.sqrt(CIN * K * K)), rand((COUT,), 0.1), device=cuda)

    def launch(out=None):
        return ops.conv_gemm(x, pw, residual=res, tile=TILE, split_k=SPLIT_K, out=out)
    ops.SPLITK_IN_KERNEL = False
    try:
        ref = launch().clone()
    finally:
        ops.SPLITK_IN_KERNEL = True
    runs = []
    ops.LAUNCH_LOG = []
    try:
        for i in range(N_KEYS):
            with ops.scratch_domain(f"k{i}"):
                y = launch()
                runs.append((y, ops.LAUNCH_LOG[-1]["params"].tile_counters, ops._tile_counters(cuda)))
    finally:
        ops.LAUNCH_LOG = None
    torch.cuda.synchronize()
    return launch, ref, runs


def test_every_key_gets_counters_and_the_same_bits(ops, cuda, many_keys):
    from diffusion_pruning_amd import scratch
    _, ref, runs = many_keys
    no_counters = [i for i, (_, cnt, _) in enumerate(runs) if not cnt]
    assert no_counters == [], f"keys {no_counters} fell back to the reduce launch"
    assert [i for i, (y, _, _) in enumerate(runs) if not torch.equal(y, ref)] == []
    assert all(cnt == slab.data_ptr() for _, cnt, slab in runs) and len({cnt for _, cnt, _ in runs}) == N_KEYS
    assert int(torch.stack([slab for _, _, slab in runs]).abs().sum()) == 0      # every launch left its counters at zero
    assert scratch.counter_keys(cuda) >= N_KEYS


def test_eager_equals_replay_after_many_keys(ops, cuda, many_keys):
    launch, ref, _ = many_keys
    with ops.scratch_domain("after-many-keys"):
        eager = launch().clone()
        out = torch.empty_like(eager)
        graph = torch.cuda.CUDAGraph()
        ops.LAUNCH_LOG = []
        try:
            with torch.cuda.graph(graph):
                launch(out)
            captured = ops.LAUNCH_LOG[-1]["params"]
        finally:
            ops.LAUNCH_LOG = None
    assert captured.tile_counters and captured.split_k == SPLIT_K
    assert torch.equal(eager, ref)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
