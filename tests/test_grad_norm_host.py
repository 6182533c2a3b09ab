"""CPU checks of the gradient-norm pass (csrc/grad_norm.hip) through its numpy model (tests/grad_norm_model.py): the model's
summation order against numpy's fp64 norm, its clip coefficient against torch.nn.utils.clip_grad_norm_, and the block geometry of
the library against the AdamW pass it shares a table layout with."""
import os

import numpy as np
import pytest
import torch

from tests import grad_norm_model as M


@pytest.mark.parametrize("name", list(M.tables()))
def test_model_against_numpy_norm(name):
    items = M.items_of(M.tables()[name], seed=1)
    out = M.grad_norm(items)
    ref = M.reference_norm(items)
    # fp64 accumulation over <= 2e6 terms errs by < 1e-9 relative: what remains is the one rounding to fp32
    assert M.ulps(out[0], ref) <= 1, (out[0], ref)
    assert out[1] == 1.0 and out[2] == out[0] and out[3] == 0.0
    assert M.partials(items).size == sum(M.blocks_of(n) for n in M.tables()[name])


def test_model_order_is_the_documented_one():
    # one block, hand-rolled: thread t sees elements (i * 256 + t) * 4 + j in the order i, j
    g = M.items_of([4096], seed=2)[0]
    s = np.zeros(256, dtype=np.float64)
    for t in range(256):
        for i in range(4):
            for j in range(4):
                x = np.float64(g[(i * 256 + t) * 4 + j])
                s[t] = s[t] + x * x
    waves = []
    for w in range(4):
        v = s[w * 64:(w + 1) * 64].copy()
        for off in (32, 16, 8, 4, 2, 1):
            v = np.array([v[l] + v[l ^ off] for l in range(64)])
        waves.append(v[0])
    want = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    assert M.partials([g])[0] == want


def test_model_range_and_zero():
    big = [np.full(5000, 1e30, dtype=np.float32), np.full(7, 1e-30, dtype=np.float32)]
    out = M.grad_norm(big)
    assert np.isfinite(out[0]) and M.ulps(out[0], M.reference_norm(big)) <= 1
    small = [np.full(3, 1e-30, dtype=np.float32)]
    out = M.grad_norm(small)
    assert out[0] > 0 and M.ulps(out[0], M.reference_norm(small)) <= 1
    out = M.grad_norm([np.zeros(4097, dtype=np.float32)], max_norm=1.0)
    assert out[0] == 0.0 and out[1] == 1.0 and out[2] == 0.0 and out[3] == 0.0


def test_model_non_finite():
    for bad in (np.nan, np.inf):
        g = M.items_of([5, 4097], seed=3)
        g[1][77] = bad
        out = M.grad_norm(g, max_norm=0.1, clipped_before=2.0)
        assert not np.isfinite(out[2]) and out[1] == 1.0 and out[3] == 2.0
    out = M.grad_norm(M.items_of([5, 4097], seed=3), max_norm=0.1, gate=np.inf, clipped_before=2.0)
    assert np.isfinite(out[0]) and np.isnan(out[2]) and out[1] == 1.0 and out[3] == 2.0


@pytest.mark.parametrize("max_norm_rel", [1.0 / 3.0, 0.999, 1.0, 1.5])
@pytest.mark.parametrize("scale", [1.0, 0.25])
def test_coefficient_against_torch_clip_grad_norm(max_norm_rel, scale):
    sizes = [5, 4097, 1283]
    items = M.items_of(sizes, seed=4)
    norm = float(M.reference_norm(items, scale))
    max_norm = max_norm_rel * norm
    out = M.grad_norm(items, grad_scale=scale, max_norm=max_norm)
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in sizes]
    for p, g in zip(ps, items):
        p.grad = torch.from_numpy(g.copy()) * scale
    before = [p.grad.clone() for p in ps]
    tn = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    assert abs(float(tn) - float(out[0])) <= 1e-6 * float(out[0])
    for p, b in zip(ps, before):
        want = b * float(out[1])
        assert float((p.grad - want).abs().max()) <= 1e-6 * float(b.abs().max())
    if max_norm_rel >= 1.0 + 1e-3:
        assert out[1] == 1.0 and out[3] == 0.0 and all(torch.equal(p.grad, b) for p, b in zip(ps, before))
    if max_norm_rel < 0.99:
        assert out[1] < 1.0 and out[3] == 1.0


def test_blocks_agree_with_the_adamw_pass():
    from diffusion_pruning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    for n in [-1, 0, 1, 3, 4095, 4096, 4097, 2 * 4096 + 5, 2 * 10 ** 6 + 3, (1 << 31) + 5]:
        assert lib.aptp_grad_norm_blocks(n) == lib.aptp_adamw_blocks(n) == M.blocks_of(n), n
