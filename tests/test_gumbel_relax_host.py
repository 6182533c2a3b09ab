"""CPU checks of the router's seeded Gumbel relaxation: csrc/gumbel_relax.h compiled for the host against the fp64
model (tests/gumbel_relax_model.py), the model against quantizer.gumbel_sigmoid_trick on injected noise (the function the
reference's golden vectors pin), the stream's moments, row independence, the non-zero-width rule on dead segments, and the
refusals that need no GPU.

Bounds against fp64: what torch's own fp32 formulas need on this host for the SAME noise (measured here), times two, plus
64 * 2^-24 * max(1, |value|) -- the project's rule."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import gumbel_relax_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 64 * 2.0 ** -24
T, BASE = 0.4, 3.0
MARGIN = 1e-4

HOST_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "gumbel_relax.h"
static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }
static float flt(unsigned u) { float v; std::memcpy(&v, &u, 4); return v; }
// one row, composed as the kernel composes it: width pass, depth chain, rule, scatter; then the backward
int main() {
  int R, nw, nd, n_seg, sub, codebook, nzw; float T, base; unsigned long long d;
  if (std::scanf("%d %d %d %d %d %d %d %f %f %llu", &R, &nw, &nd, &n_seg, &sub, &codebook, &nzw, &T, &base, &d) != 10) return 1;
  const int E = nw + nd;
  std::vector<int> seg(n_seg + 1), order(nd > 0 ? nd : 1);
  for (auto& v : seg) if (std::scanf("%d", &v) != 1) return 1;
  for (int j = 0; j < nd; ++j) if (std::scanf("%d", &order[j]) != 1) return 1;
  const uint64_t draw = aptp_gr_draw((uint64_t)d, sub, codebook != 0);
  std::printf("draw %016llx\n", (unsigned long long)draw);
  std::vector<float> z(E), dout(E), row(E), dz(E), sm(nd + 1), p(nd + 1), ds(nd + 1), g(nd + 1), dzd(nd + 1);
  for (int r = 0; r < R; ++r) {
    long long seed_in; unsigned u;
    if (std::scanf("%lld", &seed_in) != 1) return 1;
    const uint64_t seed = (uint64_t)seed_in;
    for (int e = 0; e < E; ++e) { if (std::scanf("%x", &u) != 1) return 1; z[e] = flt(u); }
    for (int e = 0; e < E; ++e) { if (std::scanf("%x", &u) != 1) return 1; dout[e] = flt(u); }
    for (int e = 0; e < E; ++e) std::printf("%08x ", aptp_gr_word(seed, draw, (uint64_t)e));
    std::printf("\n");
    for (int e = 0; e < E; ++e) std::printf("%08x ", bits(aptp_gr_gumbel(seed, draw, (uint64_t)e)));
    std::printf("\n");
    for (int c = 0; c < nw; ++c) row[c] = aptp_gr_relax(z[c], aptp_gr_gumbel(seed, draw, (uint64_t)c), base, T);
    if (nd > 0) {
      aptp_gr_depth_forward(z.data() + nw, nd, seed, draw, nw, T, base, sm.data(), p.data(), ds.data());
      for (int j = 0; j < nd; ++j) row[nw + order[j]] = ds[j];
    }
    if (nzw)
      for (int s = 0; s < n_seg; ++s)
        if (aptp_gr_segment_dead(row.data(), seg[s], seg[s + 1])) row[seg[s]] += 0.5f;
    for (int e = 0; e < E; ++e) std::printf("%08x ", bits(row[e]));
    std::printf("\n");
    for (int c = 0; c < nw; ++c)
      dz[c] = dout[c] * aptp_gr_relax_grad(aptp_gr_relax(z[c], aptp_gr_gumbel(seed, draw, (uint64_t)c), base, T), T);
    if (nd > 0) {
      for (int j = 0; j < nd; ++j) g[j] = dout[nw + order[j]];
      aptp_gr_depth_backward(g.data(), sm.data(), p.data(), ds.data(), nd, T, dzd.data());
      for (int k = 0; k < nd; ++k) dz[nw + k] = dzd[k];
    }
    for (int e = 0; e < E; ++e) std::printf("%08x ", bits(dz[e]));
    std::printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("gumbel_relax_host")
    src, exe = str(d / "m.cpp"), str(d / "m")
    open(src, "w").write(HOST_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "diffusion_pruning_amd", "csrc"),
                    "-o", exe, src], check=True)
    return exe


def _f32_hex(a):
    return " ".join("%08x" % v for v in np.asarray(a, dtype=np.float32).view(np.uint32).ravel())


def run_header(exe, z, dout, seeds, d, sub, codebook, widths, depth_order, nzw):
    """(philox draw, words uint32 [R, E], G, out, dz fp32 [R, E]) from the header on the host"""
    R, E = z.shape
    nd = len(depth_order)
    order = [int(o) % nd for o in depth_order]
    starts = M.seg_starts(widths)
    lines = ["%d %d %d %d %d %d %d %r %r %d" % (R, sum(widths), nd, len(widths), sub, int(codebook), int(nzw), T, BASE, d),
             " ".join(map(str, starts)), " ".join(map(str, order))]
    for r in range(R):
        s = int(seeds[r])
        lines += [str(s - (1 << 64) if s >= (1 << 63) else s), _f32_hex(z[r]), _f32_hex(dout[r])]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split("\n")
    draw = int(out[0].split()[1], 16)
    rows = [np.array([int(v, 16) for v in line.split()], dtype=np.uint32) for line in out[1:1 + 4 * R]]
    pick = lambda k: np.stack(rows[k::4])      # noqa: E731
    return draw, pick(0), pick(1).view(np.float32), pick(2).view(np.float32), pick(3).view(np.float32)


def _case(R, widths, nd, seed=5):
    g = torch.Generator().manual_seed(seed)
    E = sum(widths) + nd
    return 2 * torch.randn(R, E, generator=g), torch.randn(R, E, generator=g)


def test_words_and_uniforms_are_the_oracles(host_exe):
    """element offsets that are no multiples of 4 (every e of a row of 11), seeds above 2^32, a draw with the top bit set"""
    widths, order = (4, 1, 3), [-1, 0, 1]
    z, dout = _case(3, widths, 3)
    seeds = [7, (1 << 40) + 12345, (1 << 63) + 99]
    for d, sub, codebook in ((3, 7, False), (3, 6, False), ((1 << 58) + 5, 7, False), (11, 7, True)):
        draw, w, G, _, _ = run_header(host_exe, z.numpy(), dout.numpy(), seeds, d, sub, codebook, widths, order, True)
        assert draw == M.philox_draw(d, sub, codebook) and (draw >> 63) == int(codebook)
        want = M.words(seeds, draw, z.shape[1])
        assert np.array_equal(w, want), (d, sub, codebook)
        # u is exact in fp32: the header's G is the fp32 formula on the oracle's u
        u = M.uniforms(want)
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u) and u.min() > 0 and u.max() <= 1
        # offset k of the stream is element k: a row read from element 5 on equals the tail of the row
        assert np.array_equal(M.words(seeds, draw, 6, offset=5), want[:, 5:])


@pytest.mark.parametrize("R,widths,order", [(1, (3,), [0]), (5, (4, 1, 7, 32, 5), [-1, 0, 1]), (8, tuple([20, 7, 13, 1] * 5), [2, -1, 0, 1])])
def test_header_values_against_fp64(host_exe, R, widths, order):
    nd, nw = len(order), sum(widths)
    z, dout = _case(R, widths, nd)
    seeds = [1000 + 7 * i for i in range(R)]
    d, sub = 3, 7
    draw, w, G, out, dz = run_header(host_exe, z.numpy(), dout.numpy(), seeds, d, sub, False, widths, order, True)
    z64 = z.double().requires_grad_(True)
    G64 = torch.from_numpy(M.gumbel(w))
    want, dead, margin = M.forward(z64, G64, widths, order, T, BASE, True)
    want.backward(dout.double())
    # torch's own fp32 formulas on the same noise, on this host
    G32 = M.torch_noise(w)
    qz = M.make_quantizer(widths, order, T, BASE, True)
    z32 = z.clone().requires_grad_(True)
    ref = M.torch_relax(qz, z32, G32)
    ref.backward(dout)
    scale = lambda v: np.maximum(1.0, np.abs(v))      # noqa: E731
    eG_torch = np.abs(G32.double().numpy() - G64.numpy()).max()
    errG = np.abs(G.astype(np.float64) - G64.numpy())
    print("G: header %.3e torch %.3e" % (errG.max(), eG_torch))
    assert (errG <= 2 * eG_torch + FLOOR * scale(G64.numpy())).all()
    # entries whose rule was decided within the margin are left out of the value comparison (at most 1 % of the pairs)
    starts = M.seg_starts(widths)
    close = (margin < MARGIN).numpy()
    assert close.mean() <= 0.01
    keep = np.ones(out.shape, dtype=bool)
    for r, s in zip(*np.nonzero(close)):
        keep[r, starts[s]] = False
    wn = want.detach().numpy()
    for name, sl in (("w", slice(0, nw)), ("d", slice(nw, nw + nd))):
        e_torch = (np.abs(ref.detach().double().numpy() - wn)[:, sl] * keep[:, sl]).max()
        e = np.abs(out.astype(np.float64) - wn)[:, sl] * keep[:, sl]
        print("%s: header %.3e torch %.3e" % (name, e.max(), e_torch))
        assert (e <= 2 * e_torch + FLOOR * scale(wn[:, sl])).all(), name
    # the decision itself, where it was not taken within the margin: the rule switched off changes exactly the bumped entries
    off = run_header(host_exe, z.numpy(), dout.numpy(), seeds, d, sub, False, widths, order, False)[3]
    firsts = starts[:-1]
    got_dead = (out - off)[:, firsts] > 0.25
    assert np.array_equal(got_dead[~close], dead.numpy()[~close])
    want_on = off.copy()
    want_on[:, firsts] = np.where(got_dead, off[:, firsts] + np.float32(0.5), off[:, firsts])
    assert np.array_equal(out, want_on)                       # exactly + 0.5f on the first entry of a dead segment, only there
    # backward: rel-L2 against fp64 autograd
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))      # noqa: E731
    g64 = z64.grad.numpy()
    e_torch, e = rel(z32.grad.double().numpy(), g64), rel(dz.astype(np.float64), g64)
    print("dz rel-L2: header %.3e torch %.3e" % (e, e_torch))
    assert e <= 2 * e_torch + FLOOR


def test_model_is_the_quantisers_relaxation():
    """the fp64 model on injected noise equals quantizer.gumbel_sigmoid_trick (patched sample_gumbel_blocks) to 1e-6"""
    for widths, order, nzw in (((4, 1, 7, 32, 5), [-1, 0, 1], True), ((3,), [0], True), ((6, 2, 9), [1, 0], False)):
        z, _ = _case(6, widths, len(order), seed=9)
        if nzw:
            z[:, :widths[0]] = -60.0                                     # a dead first segment in every row
        w = M.words(range(6), M.philox_draw(2, 7), z.shape[1])
        G32 = M.torch_noise(w)
        qz = M.make_quantizer(widths, order, T, BASE, nzw)
        got = M.torch_relax(qz, z, G32)
        want, dead, _ = M.forward(z.double(), G32.double(), widths, order, T, BASE, nzw)
        assert float((got.double() - want).abs().max()) <= 1e-6
        assert not nzw or bool(dead[:, 0].all())


def test_moments_of_the_stream():
    """2^20 values: mean within 0.01 of Euler's constant, variance within 0.02 of pi^2 / 6"""
    G = M.gumbel(M.words([3, 1 << 35], M.philox_draw(5, 7), 1 << 19))
    print("mean %.4f variance %.4f" % (G.mean(), G.var()))
    assert abs(G.mean() - 0.5772) <= 0.01 and abs(G.var() - 1.6449) <= 0.02


def test_rows_are_independent_of_their_batch():
    widths, order = (4, 1, 7, 32, 5), [-1, 0, 1]
    z, _ = _case(5, widths, 3)
    seeds = [11, 1 << 33, 5, 77, 1234567]
    out, _, _, G = M.relax(z, seeds, 4, 7, widths, order, T, BASE)
    for r in range(5):
        one, _, _, _ = M.relax(z[r:r + 1], seeds[r:r + 1], 4, 7, widths, order, T, BASE)
        assert torch.equal(one[0], out[r])
    perm = [3, 0, 4, 1, 2]
    outp, _, _, Gp = M.relax(z[perm], [seeds[i] for i in perm], 4, 7, widths, order, T, BASE)
    assert torch.equal(outp, out[perm]) and torch.equal(Gp, G[perm])
    G6 = M.relax(z, seeds, 4, 6, widths, order, T, BASE)[3]
    Gc = M.relax(z, seeds, 4, 7, widths, order, T, BASE, codebook=True)[3]
    assert not torch.equal(G6, G) and not torch.equal(Gc, G) and not torch.equal(Gc, G6)
    assert all(not torch.equal(a, b) for a, b in zip(G6, G)) and all(not torch.equal(a, b) for a, b in zip(Gc, G))


def test_dead_segments_get_the_bump_on_their_first_entry_only(host_exe):
    widths, order = (4, 1, 7, 32, 5), [-1, 0, 1]
    nw = sum(widths)
    z, dout = _case(5, widths, 3)
    starts = M.seg_starts(widths)
    for s in (0, 2, 4):
        z[:, starts[s]:starts[s + 1]] = -60.0
    seeds = [1000 + 7 * i for i in range(5)]
    on, dead, _, _ = M.relax(z, seeds, 3, 7, widths, order, T, BASE, True)
    off = M.relax(z, seeds, 3, 7, widths, order, T, BASE, False)[0]
    assert bool(dead[:, [0, 2, 4]].all())
    diff = on - off
    want = torch.zeros_like(diff)
    want[:, [starts[s] for s in range(len(widths))]] = 0.5 * dead.double()
    assert torch.equal(diff, want)
    # and the header does the same: exactly + 0.5f on those entries, bit-equal elsewhere
    h_on = run_header(host_exe, z.numpy(), dout.numpy(), seeds, 3, 7, False, widths, order, True)[3]
    h_off = run_header(host_exe, z.numpy(), dout.numpy(), seeds, 3, 7, False, widths, order, False)[3]
    hd = h_on - h_off
    for s in (0, 2, 4):
        assert (hd[:, starts[s]] == 0.5).all() and (h_off[:, starts[s]] < 0.5).all()
    mask = np.ones(nw + 3, dtype=bool)
    mask[[starts[s] for s in (0, 2, 4)]] = False
    lively = ~dead.numpy()[:, [1, 3]].any()
    assert lively and np.array_equal(h_on[:, mask], h_off[:, mask])


def test_the_seeded_path_refuses_the_cpu_and_eval_mode():
    qz = M.make_quantizer((4, 1, 7), [0, 1], T, BASE)
    z = torch.randn(2, 14)
    noise = (torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), 7, False)
    with pytest.raises(NotImplementedError, match="GPU"):
        qz.gumbel_sigmoid_trick(z, noise)
    qz.eval()
    with pytest.raises(ValueError, match="eval mode"):
        qz.gumbel_sigmoid_trick(z, noise)
    # without a noise source nothing changed: eval mode's fixed seed-0 host stream, twice the same
    assert torch.equal(qz.gumbel_sigmoid_trick(z), qz.gumbel_sigmoid_trick(z))


def test_validation_errors_do_not_launch():
    """APTP_EINVAL before any HIP call for every limit of include/aptp_hip.h (no GPU is needed: nothing is launched)"""
    import ctypes
    from diffusion_pruning_amd import _lib
    lib = _lib.load()
    seg = (ctypes.c_int32 * 3)(0, 4, 6)
    order = (ctypes.c_int32 * 2)(1, 0)
    addr = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731

    def good():
        p = _lib.GumbelRelaxParams()
        # (the device pointers only have to be non-null: a refused call reads none of them)
        p.z = p.out = p.dout = p.dz = p.seeds = p.draw = p.seg_start = p.depth_order = 64
        p.seg_start_host, p.depth_order_host = addr(seg), addr(order)
        p.R, p.nw, p.nd, p.n_seg, p.sub, p.T, p.base = 2, 6, 2, 2, 7, 0.4, 3.0
        return p
    bad = []
    for field, value in (("R", 0), ("R", 65536), ("nw", 4096), ("nd", 65), ("n_seg", 1025), ("n_seg", 0), ("sub", 5), ("sub", 8),
                         ("T", 0.0), ("z", None), ("seeds", None), ("draw", None), ("seg_start", None), ("depth_order", None),
                         ("seg_start_host", None), ("depth_order_host", None), ("nw", 5)):
        p = good()
        setattr(p, field, value)
        bad.append((field, value, p))
    for name, table in (("seg from 1", (1, 4, 6)), ("seg not to nw", (0, 4, 5)), ("seg decreasing", (0, 7, 6))):
        p = good()
        t = (ctypes.c_int32 * 3)(*table)
        p.seg_start_host = addr(t)
        bad.append((name, t, p))
    for name, table in (("order above", (0, 2)), ("order below", (-1, 0)), ("order twice", (1, 1))):
        p = good()
        t = (ctypes.c_int32 * 2)(*table)
        p.depth_order_host = addr(t)
        bad.append((name, t, p))
    for field, value, p in bad:
        for fn in (lib.aptp_gumbel_relax, lib.aptp_gumbel_relax_bwd):
            assert fn(ctypes.byref(p), None) == -1 and lib.aptp_last_error().startswith(b"gumbel_relax"), (field, value)
    for field in ("out",):
        p = good()
        p.out = None
        assert lib.aptp_gumbel_relax(ctypes.byref(p), None) == -1
    for field in ("dout", "dz"):
        p = good()
        setattr(p, field, None)
        assert lib.aptp_gumbel_relax_bwd(ctypes.byref(p), None) == -1
    assert lib.aptp_gumbel_relax(None, None) == -1

    def good_pg():
        q = _lib.PhiloxGumbelParams()
        q.out = q.seeds = q.draw = 64
        q.n, q.offset, q.R, q.sub = 8, 0, 2, 6
        return q
    for field, value in (("R", 0), ("R", 65536), ("n", 0), ("n", (1 << 31) + 1), ("offset", -1), ("sub", 0), ("out", None),
                         ("seeds", None), ("draw", None)):
        q = good_pg()
        setattr(q, field, value)
        assert lib.aptp_philox_gumbel(ctypes.byref(q), None) == -1 and lib.aptp_last_error().startswith(b"philox_gumbel"), (field, value)
