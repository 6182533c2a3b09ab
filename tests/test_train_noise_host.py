"""The seeded training batch on the host: the host half of the draw map (data.philox_words, draw_crop_flip_seeded)
against the numpy oracle, the kernel's arithmetic header (csrc/train_noise.h) compiled for the CPU against
tests/train_noise_oracle.py, the statistics of the timestep and flip draws, batch_from_images' generator path with and without
the reference's three knobs, the refusals, and the C ABI of aptp_train_noise.

Tolerances are the per-element bounds the oracle module states (derived from u = 2^-24 and the 4e-6 bound of a normal); the
host-compiled header takes its sin / cos from fp64 and is held to the same bounds."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import philox_oracle as PO
from tests import train_noise_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "diffusion_pruning_amd", "csrc", "train_noise.h")
SHAPES = [(1, 1), (2, 2), (3, 3), (8, 8), (5, 7)]
SEEDS3 = [1234, -1, 0x1234567890abcdef]


# ---- the host half of the map -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, -1, 2 ** 63 - 1, 0x1234567890abcdef])
def test_philox_words_equal_the_oracle(seed):
    from diffusion_pruning_amd import data
    for draw in (0, 5, 2 ** 32, 2 ** 59 - 1):
        assert data.philox_words(seed, draw) == [int(v) for v in PO.bits(seed, draw, 0, 4)], (seed, draw)
    assert data.philox_words(seed, 7, block=2 ** 33 + 1) == [int(v) for v in PO.bits(seed, 7, 4 * (2 ** 33 + 1), 4)]
    assert np.array_equal(TO.words_of_seeds([seed], 5)[0], PO.bits(seed, 5, 0, 4))


def test_crop_and_flip_follow_the_map():
    from diffusion_pruning_amd.data import draw_crop_flip_seeded
    R = 256
    sizes = [(256, 256), (256, 341), (300, 256), (384, 512), (256, 455), (1024, 257)]
    seeds = [0, 1, -1, 2 ** 63 - 1, 0x1234567890abcdef, 77]
    for draw in (0, 3, 2 ** 59 - 1):
        tops, lefts, flips = draw_crop_flip_seeded(sizes, R, seeds, draw)
        want = [TO.crop_flip(s, draw, h, w, R) for s, (h, w) in zip(seeds, sizes)]
        assert list(zip(tops, lefts, flips)) == want
        for (h, w), t, l, f in zip(sizes, tops, lefts, flips):
            assert 0 <= t <= h - R and 0 <= l <= w - R and f in (0, 1)
        assert (tops[0], lefts[0]) == (0, 0)                                      # H1 = W1 = R: nothing to choose
        # center_crop ignores x0 and x1, random_flip=False ignores x2, and neither shifts the other
        ct, cl, cf = draw_crop_flip_seeded(sizes, R, seeds, draw, center_crop=True)
        assert ct == [int(round((h - R) / 2.0)) for h, _ in sizes] and cl == [int(round((w - R) / 2.0)) for _, w in sizes]
        assert cf == flips
        nt, nl, nf = draw_crop_flip_seeded(sizes, R, seeds, draw, random_flip=False)
        assert (nt, nl) == (tops, lefts) and nf == [0] * len(sizes)
        # a sample's draws are its own: permuting or dropping samples permutes or drops the results
        perm = [4, 0, 5, 2, 1, 3]
        pt, pl, pf = draw_crop_flip_seeded([sizes[i] for i in perm], R, [seeds[i] for i in perm], draw)
        assert (pt, pl, pf) == ([tops[i] for i in perm], [lefts[i] for i in perm], [flips[i] for i in perm])
        keep = [0, 1, 3, 4, 5]
        dt, dl, df = draw_crop_flip_seeded([sizes[i] for i in keep], R, [seeds[i] for i in keep], draw)
        assert (dt, dl, df) == ([tops[i] for i in keep], [lefts[i] for i in keep], [flips[i] for i in keep])
    assert draw_crop_flip_seeded(sizes, R, seeds, 0) != draw_crop_flip_seeded(sizes, R, seeds, 1)
    assert draw_crop_flip_seeded(sizes, R, torch.tensor([s if s < 2 ** 63 else s - 2 ** 64 for s in seeds]), 3) == \
        draw_crop_flip_seeded(sizes, R, seeds, 3)


def test_transform_takes_seeds_or_a_generator():
    from diffusion_pruning_amd.data import TrainTransform, draw_crop_flip_seeded
    tf = TrainTransform(16)
    images = [torch.zeros(20, 31, 3, dtype=torch.uint8), torch.zeros(40, 16, 3, dtype=torch.uint8)]
    assert tf.draw(images, seeds=[5, 6], draw=2) == draw_crop_flip_seeded(tf.resized_sizes(images), 16, [5, 6], 2)
    with pytest.raises(ValueError, match="not both"):
        tf.draw(images, torch.Generator().manual_seed(0), seeds=[5, 6])
    with pytest.raises(ValueError, match="not both"):
        tf(images, torch.Generator().manual_seed(0), seeds=[5, 6])
    with pytest.raises(ValueError, match="draw"):
        tf.draw(images, seeds=[5, 6], draw=-1)
    with pytest.raises(ValueError, match="draw"):
        tf.draw(images, seeds=[5, 6], draw=2 ** 59)
    with pytest.raises(ValueError, match="seeds for 2"):
        tf.draw(images, seeds=[5], draw=0)


# ---- train_noise.h compiled for the CPU ---------------------------------------------------------------------------------------
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "%s"
// in:  int64 B, h, w, T, draw, v_prediction, from_moments, H1span, W1span; float scale, noise_offset, input_perturbation;
//      int64 seeds[B]; float table[2 T]; float input[B (8 | 4) hw]
// out: int64 t[B]; int64 top, left, flip [B][3]; float noisy, target, x0, n [4][B 4 hw]; int64 mismatches of the 4-wide form
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t hd[9];
  AptpTnKnobs k;
  float kn[3];
  if (fread(hd, 8, 9, f) != 9 || fread(kn, 4, 3, f) != 3) return 4;
  const int64_t B = hd[0], hw = hd[1] * hd[2], T = hd[3], n4 = 4 * hw, ch = hd[6] ? 8 : 4;
  const uint64_t draw = (uint64_t)hd[4];
  k.scale = kn[0]; k.noise_offset = kn[1]; k.input_perturbation = kn[2]; k.v_prediction = (int)hd[5];
  std::vector<int64_t> seeds(B), t(B), tf(3 * B);
  std::vector<float> table(2 * T), in(B * ch * hw), out(4 * B * n4);
  if (fread(seeds.data(), 8, B, f) != (size_t)B || fread(table.data(), 4, 2 * T, f) != (size_t)(2 * T) ||
      fread(in.data(), 4, in.size(), f) != in.size()) return 5;
  fclose(f);
  float *noisy = out.data(), *target = noisy + B * n4, *x0 = target + B * n4, *n = x0 + B * n4;
  int64_t mismatches = 0;
  for (int64_t r = 0; r < B; ++r) {
    const uint64_t seed = (uint64_t)seeds[r];
    AptpTnSample s;
    aptp_tn_sample(seed, draw, T, table.data(), k.noise_offset != 0.f, &s);
    t[r] = s.t;
    uint32_t x[4];
    aptp_philox_block(seed, aptp_tn_subdraw(draw, APTP_TN_TRANSFORM), 0, x);
    tf[3 * r] = aptp_tn_choice(x[0], hd[7]); tf[3 * r + 1] = aptp_tn_choice(x[1], hd[8]); tf[3 * r + 2] = x[2] >> 31;
    for (int64_t e = 0; e < n4; ++e) {
      const int64_t i = r * n4 + e, im = r * 2 * n4 + e;
      aptp_tn_element_of(k, s, seed, draw, e, hw, hd[6] != 0, hd[6] ? in[im] : 0.f, hd[6] ? in[im + n4] : 0.f, hd[6] ? 0.f : in[i],
                         &x0[i], &noisy[i], &target[i], &n[i]);
    }
    if (hw %% 4) continue;
    for (int64_t e = 0; e < n4; e += 4) {                      // the form a lane with four elements uses: the same bits
      const int64_t i = r * n4 + e, im = r * 2 * n4 + e;
      float z1[4], z2[4], z4[4] = {0.f, 0.f, 0.f, 0.f}, a0[4], an[4], at[4], ann[4];
      if (hd[6]) {
        aptp_philox_block(seed, aptp_tn_subdraw(draw, APTP_TN_EPS), (uint64_t)e >> 2, x);
        aptp_philox_normals4(x, z1);
        for (int j = 0; j < 4; ++j) a0[j] = aptp_tn_x0(in[im + j], in[im + n4 + j], z1[j], k.scale);
      } else {
        for (int j = 0; j < 4; ++j) a0[j] = in[i + j];
      }
      aptp_philox_block(seed, aptp_tn_subdraw(draw, APTP_TN_NOISE), (uint64_t)e >> 2, x);
      aptp_philox_normals4(x, z2);
      if (k.input_perturbation != 0.f) {
        aptp_philox_block(seed, aptp_tn_subdraw(draw, APTP_TN_PERTURB), (uint64_t)e >> 2, x);
        aptp_philox_normals4(x, z4);
      }
      aptp_tn_element4(k, s, a0, z2, s.z3[e / hw], z4, an, at, ann);
      mismatches += memcmp(an, noisy + i, 16) != 0 || memcmp(at, target + i, 16) != 0 || memcmp(a0, x0 + i, 16) != 0 ||
                    memcmp(ann, n + i, 16) != 0;
    }
  }
  f = fopen(argv[2], "wb");
  if (!f) return 6;
  fwrite(t.data(), 8, B, f); fwrite(tf.data(), 8, 3 * B, f); fwrite(out.data(), 4, out.size(), f); fwrite(&mismatches, 8, 1, f);
  fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("train_noise_host")
    src, exe = d / "t.cpp", d / "t"
    src.write_text(DRIVER % HEADER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"], check=True)
    count = [0]

    def run(seeds, draw, table, inp, from_moments, scale, noise_offset, input_perturbation, prediction, spans=(1, 1)):
        B, _, h, w = inp.shape
        count[0] += 1
        fin, fout = d / f"in{count[0]}.bin", d / f"out{count[0]}.bin"
        with open(fin, "wb") as f:
            np.array([B, h, w, table.shape[0], draw, int(prediction == "v_prediction"), int(from_moments), spans[0], spans[1]],
                     dtype=np.int64).tofile(f)
            np.array([scale, noise_offset, input_perturbation], dtype=np.float32).tofile(f)
            np.array([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], dtype=np.int64).tofile(f)
            table.astype(np.float32).tofile(f)
            inp.astype(np.float32).tofile(f)
        subprocess.run([str(exe), str(fin), str(fout)], check=True)
        raw = open(fout, "rb").read()
        n = B * 4 * h * w
        t = np.frombuffer(raw, np.int64, B, 0)
        tf = np.frombuffer(raw, np.int64, 3 * B, 8 * B).reshape(B, 3)
        vals = np.frombuffer(raw, np.float32, 4 * n, 32 * B).reshape(4, B, 4, h, w)
        mism = int(np.frombuffer(raw, np.int64, 1, 32 * B + 16 * n)[0])
        return {"t": t, "transform": tf, "noisy": vals[0], "target": vals[1], "latents": vals[2], "noise": vals[3], "mismatches": mism}
    return run


def sqrt_table(T=1000):
    from diffusion_pruning_amd.train_step import NoiseSchedule
    return NoiseSchedule(T).sqrt_table().numpy()


def test_sqrt_table_is_the_two_square_roots():
    from diffusion_pruning_amd.train_step import NoiseSchedule
    sch = NoiseSchedule()
    tab = sch.sqrt_table()
    ac = sch.alphas_cumprod
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (1000, 2) and tab.is_contiguous()
    assert torch.equal(tab, torch.stack([ac ** 0.5, (1 - ac) ** 0.5], 1))
    # torch's CPU square root is within an ulp of the correctly rounded one (not always equal to it: the table is data)
    for col, operand in ((0, ac.numpy()), (1, np.float32(1) - ac.numpy())):
        exact = np.sqrt(operand.astype(np.float64))
        assert np.abs(tab.numpy()[:, col].astype(np.float64) - exact).max() <= np.spacing(exact.astype(np.float32)).max()
    assert sch.sqrt_table() is tab                                                # cached


@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("from_moments", [True, False], ids=["moments", "latents"])
def test_header_compiled_for_the_cpu_matches_the_oracle(driver, h, w, from_moments):
    table = sqrt_table()
    inp = TO.make_inputs(3, h, w, from_moments=from_moments)
    worst = {}
    for prediction in ("epsilon", "v_prediction"):
        for no, ip in ((0.0, 0.0), (0.1, 0.0), (0.0, 0.1), (0.05, 0.2)):
            kw = dict(scale=0.18215 if from_moments else 1.0, noise_offset=no, input_perturbation=ip, prediction=prediction)
            got = driver(SEEDS3, 3, table, inp, from_moments, kw["scale"], no, ip, prediction, spans=(45, 246))
            ref = TO.batch(SEEDS3, 3, table, **{"moments" if from_moments else "latents": inp}, **kw)
            assert np.array_equal(got["t"], ref["t"])
            assert [tuple(r) for r in got["transform"]] == [TO.crop_flip(s, 3, 256 + 44, 256 + 245, 256) for s in SEEDS3]
            assert got["mismatches"] == 0
            for name in ("noisy", "target", "latents", "noise"):
                worst[name] = max(worst.get(name, 0.0), TO.worst_used(got[name], ref, name))
    print(f"host header vs oracle at {h}x{w}: worst fraction of the bound used {worst}")
    for name, used in worst.items():
        assert used <= 1.0, (name, used)


def test_header_follows_draw_and_ignores_the_batch(driver):
    table = sqrt_table()
    inp = TO.make_inputs(3, 3, 3)
    a = driver(SEEDS3, 2 ** 59 - 1, table, inp, True, 0.18215, 0.1, 0.1, "v_prediction")
    ref = TO.batch(SEEDS3, 2 ** 59 - 1, table, moments=inp, scale=0.18215, noise_offset=0.1, input_perturbation=0.1)
    assert np.array_equal(a["t"], ref["t"]) and TO.worst_used(a["noisy"], ref, "noisy") <= 1.0
    b = driver(SEEDS3[1:2], 2 ** 59 - 1, table, inp[1:2], True, 0.18215, 0.1, 0.1, "v_prediction")
    for name in ("noisy", "target", "latents", "noise", "t"):
        assert np.array_equal(a[name][1:2], b[name])


# ---- statistics of the integer draws: conditions on fixed inputs, nothing is left to chance -----------------------------------
N_STAT = 20000


def chi2(t, T, bins):
    cnt = np.bincount((t * bins // T).astype(np.int64), minlength=bins).astype(np.float64)
    exp = np.bincount((np.arange(T) * bins // T), minlength=bins) * (len(t) / T)
    return float(((cnt - exp) ** 2 / exp).sum())


def test_timestep_and_flip_statistics(driver):
    from diffusion_pruning_amd.data import draw_crop_flip_seeded
    seeds = list(range(N_STAT))
    lat = np.zeros((N_STAT, 4, 1, 1), np.float32)
    t1000 = driver(seeds, 3, sqrt_table(1000), lat, False, 1.0, 0.0, 0.0, "epsilon")["t"]
    t7 = driver(seeds, 3, sqrt_table(7), lat, False, 1.0, 0.0, 0.0, "epsilon")["t"]
    assert np.array_equal(t1000, TO.timesteps_of_seeds(seeds, 3, 1000).astype(np.int64))
    assert np.array_equal(t7, TO.timesteps_of_seeds(seeds, 3, 7).astype(np.int64))
    assert [int(v) for v in t1000[:50]] == [TO.timestep(s, 3, 1000) for s in seeds[:50]]
    c1000, c7 = chi2(t1000, 1000, 100), chi2(t7, 7, 7)
    _, _, flips = draw_crop_flip_seeded([(300, 300)] * N_STAT, 256, seeds, 3)
    flip_se = abs(np.mean(flips) - 0.5) / (0.5 / np.sqrt(N_STAT))
    print(f"chi2 T=1000 in 100 bins {c1000:.1f}, T=7 {c7:.1f}, range {t1000.min()}..{t1000.max()}, flip rate off by {flip_se:.2f} se")
    assert c1000 <= 99 + 4 * np.sqrt(198)
    assert c7 <= 6 + 4 * np.sqrt(12)
    assert t1000.min() == 0 and t1000.max() == 999 and t7.min() == 0 and t7.max() == 6
    assert flip_se <= 4.0


# ---- batch_from_images on the generator path ----------------------------------------------------------------------------------
class StubVae:
    """encode_latents returns fixed latents and draws nothing: what follows is the batch builder's own use of the generator"""

    class config:
        scaling_factor = 0.18215

    def __init__(self, latents):
        self.latents = latents

    def encode_latents(self, pixel_values, generator=None):
        return self.latents


def stub_batch(B=3, h=5, w=7):
    g = torch.Generator().manual_seed(5)
    return (torch.randn(B, 4, h, w, generator=g), torch.zeros(B, 3, 8 * h, 8 * w), torch.randn(B, 77, 8, generator=g),
            torch.randn(B, 768, generator=g))


@pytest.mark.parametrize("prediction", ["epsilon", "v_prediction"])
def test_defaults_consume_the_generator_as_before(prediction):
    from diffusion_pruning_amd import train_step as TS
    lat, px, ehs, mp = stub_batch()
    sch = TS.NoiseSchedule()
    g, g0 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    got = TS.batch_from_images(StubVae(lat), px, ehs, mp, sch, prediction, g)
    # the parent's statements
    noise = torch.randn(lat.shape, generator=g0, dtype=lat.dtype)
    timesteps = torch.randint(0, 1000, (lat.shape[0],), generator=g0)
    noisy, target = TS.noisy_latents_and_target(lat, noise, timesteps, sch.alphas_cumprod, prediction)
    assert torch.equal(g.get_state(), g0.get_state())
    assert torch.equal(got["timesteps"], timesteps) and torch.equal(got["noisy_latents"], noisy) and torch.equal(got["target"], target)
    assert got["encoder_hidden_states"] is ehs and got["mpnet_embeddings"] is mp


@pytest.mark.parametrize("prediction", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("no,ip,steps", [(0.1, 0.0, None), (0.0, 0.1, None), (0.0, 0.0, 300), (0.05, 0.2, 500)])
def test_the_three_knobs_follow_the_reference_order(prediction, no, ip, steps):
    from diffusion_pruning_amd import train_step as TS
    lat, px, ehs, mp = stub_batch()
    sch = TS.NoiseSchedule()
    g, g0 = torch.Generator().manual_seed(12), torch.Generator().manual_seed(12)
    got = TS.batch_from_images(StubVae(lat), px, ehs, mp, sch, prediction, g, noise_offset=no, input_perturbation=ip,
                               max_scheduler_steps=steps)
    # trainer.py:1100-1123 on the same generator
    noise = torch.randn(lat.shape, generator=g0)
    if no:
        noise = noise + no * torch.randn((lat.shape[0], lat.shape[1], 1, 1), generator=g0)
    if ip:
        new_noise = noise + ip * torch.randn(lat.shape, generator=g0)
    timesteps = torch.randint(0, 1000 if steps is None else steps, (lat.shape[0],), generator=g0)
    ac = sch.alphas_cumprod
    sa, so = (ac[timesteps] ** 0.5).reshape(-1, 1, 1, 1), ((1 - ac[timesteps]) ** 0.5).reshape(-1, 1, 1, 1)
    noisy = sa * lat + so * (new_noise if ip else noise)
    target = noise if prediction == "epsilon" else sa * noise - so * lat
    assert torch.equal(g.get_state(), g0.get_state())
    assert torch.equal(got["timesteps"], timesteps) and torch.equal(got["noisy_latents"], noisy) and torch.equal(got["target"], target)
    if steps is not None:
        assert int(got["timesteps"].max()) < steps


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_python_refusals():
    from diffusion_pruning_amd import ops, train_step as TS
    lat, px, ehs, mp = stub_batch()
    vae = StubVae(lat)
    with pytest.raises(ValueError, match="not both"):
        TS.batch_from_images(vae, px, ehs, mp, generator=torch.Generator().manual_seed(0), seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="draw"):
        TS.batch_from_images(vae, px, ehs, mp, seeds=[1, 2, 3], draw=-1)
    with pytest.raises(ValueError, match="draw"):
        TS.batch_from_images(vae, px, ehs, mp, seeds=[1, 2, 3], draw=2 ** 59)
    with pytest.raises(ValueError, match="max_scheduler_steps"):
        TS.batch_from_images(vae, px, ehs, mp, max_scheduler_steps=1001)
    with pytest.raises(ValueError, match="max_scheduler_steps"):
        TS.batch_from_images(vae, px, ehs, mp, seeds=[1, 2, 3], max_scheduler_steps=0)
    with pytest.raises(ValueError, match="noise_offset"):
        TS.batch_from_images(vae, px, ehs, mp, noise_offset=float("nan"))
    images = [torch.zeros(20, 31, 3, dtype=torch.uint8)] * 3
    with pytest.raises(ValueError, match="not both"):
        TS.batch_from_uint8(vae, images, resolution=16, encoder_hidden_states=ehs, mpnet_embeddings=mp, seeds=[1, 2, 3],
                            transform_generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="not both"):
        TS.batch_from_uint8(vae, images, resolution=16, encoder_hidden_states=ehs, mpnet_embeddings=mp, seeds=[1, 2, 3],
                            generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match="seeds for 3"):
        TS.batch_from_uint8(vae, images, resolution=16, encoder_hidden_states=ehs, mpnet_embeddings=mp, seeds=[1, 2])
    table = TS.NoiseSchedule().sqrt_table()
    with pytest.raises(ValueError, match="exactly one"):
        ops.train_noise(torch.zeros(1, 8, 2, 2), latents=torch.zeros(1, 4, 2, 2), sqrt_table=table, seeds=[1])
    with pytest.raises(ValueError, match="exactly one"):
        ops.train_noise(sqrt_table=table, seeds=[1])
    with pytest.raises(ValueError, match="CUDA"):
        ops.train_noise(torch.zeros(1, 8, 2, 2), sqrt_table=table, seeds=[1])
    with pytest.raises(ValueError, match="max_scheduler_steps"):
        TS.SeededBatchBuilder(None, 2, (4, 8, 8), "cpu", max_scheduler_steps=1001)
    with pytest.raises(ValueError, match="latent_shape"):
        TS.SeededBatchBuilder(None, 2, (3, 8, 8), "cpu")


def test_train_noise_refuses_before_launching():
    """made-up addresses: every refusal returns APTP_EINVAL (-1) with its reason before anything is launched"""
    from diffusion_pruning_amd import _lib
    lib = _lib.load()

    def params(**kw):
        p = _lib.TrainNoiseParams()
        p.moments, p.sqrt_table, p.seeds_dev, p.noisy, p.target, p.timesteps = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
        p.B, p.h, p.w, p.T, p.prediction, p.scale = 2, 8, 8, 1000, _lib.TRAIN_NOISE_V_PREDICTION, 1.0
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def refused(needle, **kw):
        assert lib.aptp_train_noise(ctypes.byref(params(**kw)), None) == -1
        assert needle in lib.aptp_last_error(), lib.aptp_last_error()

    assert lib.aptp_train_noise(None, None) == -1 and b"null pointer" in lib.aptp_last_error()
    for name in ("sqrt_table", "seeds_dev", "noisy", "target", "timesteps"):
        refused(b"null pointer", **{name: None})
    refused(b"exactly one", latents_in=0x70000)
    refused(b"exactly one", moments=None)
    refused(b"outside 1..65535", B=0)
    refused(b"outside 1..65535", B=65536)
    refused(b"bad extents", h=0)
    refused(b"bad extents", w=-1)
    refused(b"bad extents", h=2 ** 20, w=2 ** 20)
    refused(b"below 1", T=0)
    refused(b"draw", draw=-1)
    refused(b"draw", draw=2 ** 59)
    refused(b"unknown prediction", prediction=2)
    for name in ("moments", "sqrt_table", "noisy", "target", "latents_out", "noise_out"):
        refused(b"alignment", **{name: 0x80002})
    refused(b"alignment", moments=None, latents_in=0x80002)
    for name in ("seeds_dev", "draw_dev", "timesteps"):
        refused(b"alignment", **{name: 0x80004})


def test_train_noise_ctypes_layout_matches_the_c_header(tmp_path):
    from diffusion_pruning_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    header = os.path.join(ROOT, "include", "aptp_hip.h")
    cls = _lib.TrainNoiseParams
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){",
            'printf("%zu\\n", sizeof(AptpTrainNoiseParams));']
    for fname, _ in cls._fields_:
        body.append(f'printf("%zu\\n", offsetof(AptpTrainNoiseParams, {fname}));')
    body.append('printf("%d %d\\n", (int)APTP_TRAIN_NOISE_EPSILON, (int)APTP_TRAIN_NOISE_V_PREDICTION);')
    body.append("return 0;}")
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(body))
    subprocess.run([cc, "-std=c99", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(cls)
    assert [int(v) for v in out[1:1 + len(cls._fields_)]] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert [int(v) for v in out[-2:]] == [_lib.TRAIN_NOISE_EPSILON, _lib.TRAIN_NOISE_V_PREDICTION]
