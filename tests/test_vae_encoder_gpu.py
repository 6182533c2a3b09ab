"""The HIP VAE encoder on the GPU: conv_gemm with bottom / right padding (pad_end) on every tile family it can take, the
im2col image prologue and the latent-distribution tail against torch math, the whole encoder against the CPU oracle
(tests/vae_encoder_oracle.py) in bf16 and on the fp32 parity path, sampling, graph capture, determinism, and a training
batch built from images.  Margins go through tests.margins.check, which keeps the measured values."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vae_encoder_oracle as E
from tests.helpers import rel_l2
from tests.margins import check

pytestmark = pytest.mark.gpu

CONV_BF16_TOL = 4e-3
CONV_F32_TOL = 1e-5
ENC_BF16_TOL = 2e-2
ENC_F32_TOL = 1e-4


def max_ulps(a, b, mag=None):
    """largest |a - b| in units of the fp32 spacing at mag (default |b|).  For a sum mean + std * eps, mag is the larger
    addend: an ulp of exp() in std is an ulp of that term, whatever cancellation leaves of the sum"""
    a, b = a.float().cpu().numpy().astype(np.float64), b.float().cpu().numpy().astype(np.float64)
    m = np.abs(b) if mag is None else mag.float().cpu().numpy()
    return float(np.max(np.abs(a - b) / np.spacing(np.abs(m).astype(np.float32)).astype(np.float64)))


def _addend_mag(mean, std, eps):
    return torch.maximum(mean.abs(), (std * eps).abs())


def _down_ref(x, w, b):
    return F.conv2d(F.pad(x.double(), (0, 1, 0, 1)), w.double(), b.double(), stride=2)


# ---------------------------------------------------------------------------------------------------------------------
# conv_gemm(stride=2, pad=0, pad_end=1)
# ---------------------------------------------------------------------------------------------------------------------
# 0 = automatic; 1 / 5 = register-staged (general); 7 / 13 = LDS-DMA; 33 = ping-pong; 64 / 72 = persistent stream-K
@pytest.mark.parametrize("tile", [0, 1, 5, 7, 13, 33, 64, 72])
@pytest.mark.parametrize("C,B,H,W", [(128, 2, 32, 32), (256, 1, 24, 40), (512, 1, 16, 16)])
def test_downsample_conv_bf16(cuda, tile, C, B, H, W):
    from diffusion_pruning_amd import ops
    g = torch.Generator().manual_seed(C + H + tile)
    x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(C, C, 3, 3, generator=g) * C ** -0.5 / 3).to(torch.bfloat16).float()
    b = torch.randn(C, generator=g) * 0.1
    pw = ops.pack_weight(w, b, device=cuda)
    y = ops.conv_gemm(x.to(cuda), pw, stride=2, pad=0, pad_end=1, tile=tile)
    torch.cuda.synchronize()
    ref = _down_ref(x.float().permute(0, 3, 1, 2), w, b).permute(0, 2, 3, 1)
    assert y.shape == ref.shape == (B, H // 2, W // 2, C)
    check(rel_l2(y, ref), CONV_BF16_TOL, f"conv pad_end=1 bf16 tile {tile} C={C} {B}x{H}x{W}")


def test_downsample_conv_bf16_with_column_statistics(cuda):
    """the encoder's form: colstats=True, then the GroupNorm that consumes the statistics"""
    from diffusion_pruning_amd import ops
    g = torch.Generator().manual_seed(3)
    C, B, H, W = 256, 2, 64, 48
    x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(C, C, 3, 3, generator=g) * C ** -0.5 / 3).to(torch.bfloat16).float()
    b = torch.randn(C, generator=g) * 0.1
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(cuda), (0.1 * torch.randn(C, generator=g)).to(cuda)
    y = ops.conv_gemm(x.to(cuda), ops.pack_weight(w, b, device=cuda), stride=2, pad=0, pad_end=1, colstats=True)
    a = ops.groupnorm(y, gamma, beta, 32, 1e-6, True)
    torch.cuda.synchronize()
    ref = _down_ref(x.float().permute(0, 3, 1, 2), w, b)
    check(rel_l2(y, ref.permute(0, 2, 3, 1)), CONV_BF16_TOL, "conv pad_end=1 bf16 with colstats")
    refa = F.silu(F.group_norm(y.permute(0, 3, 1, 2).double().cpu(), 32, gamma.double().cpu(), beta.double().cpu(), 1e-6))
    check(rel_l2(a.permute(0, 3, 1, 2), refa), CONV_BF16_TOL, "groupnorm after the pad_end=1 conv (producer statistics)")


@pytest.mark.parametrize("tile", [0, 1, 3, 6])
@pytest.mark.parametrize("C,B,H,W", [(128, 1, 32, 32), (256, 1, 24, 40), (512, 2, 16, 16)])
def test_downsample_conv_fp32_parity(cuda, monkeypatch, tile, C, B, H, W):
    from diffusion_pruning_amd import ops
    monkeypatch.setattr(ops, "ACT_DTYPE", torch.float32)
    g = torch.Generator().manual_seed(C * 7 + W + tile)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) * C ** -0.5 / 3
    b = torch.randn(C, generator=g) * 0.1
    y = ops.conv_gemm(x.to(cuda), ops.pack_weight(w, b, device=cuda), stride=2, pad=0, pad_end=1, tile=tile)
    torch.cuda.synchronize()
    ref = _down_ref(x.permute(0, 3, 1, 2), w, b).permute(0, 2, 3, 1)
    check(rel_l2(y, ref), CONV_F32_TOL, f"conv pad_end=1 fp32 tile {tile} C={C} {B}x{H}x{W}")


# ---------------------------------------------------------------------------------------------------------------------
# image_in and conv_in
# ---------------------------------------------------------------------------------------------------------------------
def _im2col_ref(x):
    B, C, H, W = x.shape
    cols = F.unfold(x.float(), 3, padding=1)                                   # [B, (c, ky, kx), HW]
    cols = cols.reshape(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B, H, W, 27)   # tap-major (ky, kx, c)
    return torch.cat([cols, cols.new_zeros(B, H, W, 5)], -1)


@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 64, 64), (1, 37, 53), (3, 8, 16)])
def test_image_in_is_bit_exact(cuda, in_dtype, shape):
    from diffusion_pruning_amd import ops
    B, H, W = shape
    x = (torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(H)) * 2 - 1).to(in_dtype).to(cuda)
    ref = _im2col_ref(x.cpu())
    out = ops.image_in(x)
    out32 = ops.image_in(x, out_f32=True)
    torch.cuda.synchronize()
    assert out.shape == (B, H, W, 32) and out.dtype == torch.bfloat16
    assert torch.equal(out.cpu(), ref.to(torch.bfloat16))
    assert torch.equal(out32.cpu(), ref)


def test_conv_in_through_im2col(cuda):
    from diffusion_pruning_amd import ops
    g = torch.Generator().manual_seed(8)
    x = (torch.rand(2, 3, 96, 80, generator=g) * 2 - 1).to(torch.bfloat16)
    w = (torch.randn(128, 3, 3, 3, generator=g) / 27 ** 0.5).to(torch.bfloat16).float()
    b = torch.randn(128, generator=g) * 0.02
    y = ops.conv_gemm(ops.image_in(x.to(cuda)), ops.pack_conv_in_im2col(w, b, device=cuda), pad=0)
    torch.cuda.synchronize()
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    check(rel_l2(y, ref), CONV_BF16_TOL, "encoder conv_in via image_in + 1x1 (bf16)")


# ---------------------------------------------------------------------------------------------------------------------
# latent_dist
# ---------------------------------------------------------------------------------------------------------------------
def test_latent_dist_against_torch(cuda):
    from diffusion_pruning_amd import ops
    g = torch.Generator().manual_seed(12)
    B, h, w = 3, 16, 24
    y = torch.randn(B, h, w, 8, generator=g) * 3
    y[0, 0, :4, 4] = torch.tensor([60.0, 25.0, -45.0, -31.0])                 # logvar past both clamp bounds
    y[1, 2, :4, 7] = torch.tensor([-80.0, 21.0, 19.5, -29.5])
    wq = torch.eye(8) + 0.01 * torch.randn(8, 8, generator=g)
    bq = 0.05 * torch.randn(8, generator=g)
    eps = torch.randn(B, 4, h, w, generator=g)
    yc, ec = y.to(cuda), eps.to(cuda)
    mom, lat = ops.latent_dist(yc, wq, bq, eps=ec, scale=1.0)
    _, lat_s = ops.latent_dist(yc, wq, bq, eps=ec, scale=0.18215, moments=False)
    _, lat_b = ops.latent_dist(yc, wq, bq, eps=ec, scale=1.0, moments=False, latents_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    ref = (y.double() @ wq.double().t() + bq.double()).permute(0, 3, 1, 2)
    check(rel_l2(mom, ref), 1e-6, "latent_dist moments vs quant_conv in fp64")
    lv = mom[:, 4:]
    assert float(lv.max()) > 20 and float(lv.min()) < -30
    d = E.DiagonalGaussianDistribution(mom)                                     # torch formula on the same moments (GPU)
    z = d.sample(ec)
    mag = _addend_mag(d.mean, d.std, ec)
    check(max_ulps(lat, z, mag), 2.0, "latent_dist sample vs torch (ulps of the larger addend)")
    # the scaled sample is the unscaled one times scale, rounded once: the scale multiply is the last operation
    assert torch.equal(lat_s, lat * 0.18215)
    assert torch.equal(lat_b, lat.to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------------------------------
# the whole encoder
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vae_pair():
    from diffusion_pruning_amd.vae import AutoencoderKL
    m = AutoencoderKL(with_encoder=True).init_synthetic(seed=0)
    oracle = E.EncoderOracle()
    oracle.load_state_dict({k: v for k, v in m.state_dict().items() if k.startswith(("encoder.", "quant_conv."))})
    oracle.eval()
    return m, oracle


def _pixels(B, H, W, seed):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed)) * 2 - 1


@pytest.mark.parametrize("B,H,W", [(2, 256, 256), (1, 512, 512), (1, 192, 320)])
def test_encoder_bf16_against_oracle(cuda, vae_pair, B, H, W):
    m, oracle = vae_pair
    m.to(cuda)
    x = _pixels(B, H, W, seed=H + W)
    dist = m.encode(x.to(cuda)).latent_dist
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = oracle.float()(x)
    assert dist.parameters.shape == ref.shape == (B, 8, H // 8, W // 8)
    assert 0.1 <= float(ref.std()) <= 10.0
    check(rel_l2(dist.parameters, ref), ENC_BF16_TOL, f"vae encode bf16 B={B} {H}x{W}")


def test_encoder_fp32_parity_path(cuda, vae_pair, monkeypatch):
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd.vae import AutoencoderKL
    monkeypatch.setattr(ops, "ACT_DTYPE", torch.float32)
    m0, oracle = vae_pair
    m = AutoencoderKL(with_encoder=True)
    m.load_state_dict(m0.state_dict())
    m.to(cuda)
    x = _pixels(1, 128, 96, seed=5)
    mom = m.encode(x.to(cuda)).latent_dist.parameters
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = oracle.double()(x.double())
    oracle.float()
    check(rel_l2(mom, ref), ENC_F32_TOL, "vae encode fp32 parity B=1 128x96")


def test_encode_rejects_sizes_not_multiple_of_8(cuda, vae_pair):
    m, _ = vae_pair
    m.to(cuda)
    with pytest.raises(ValueError):
        m.encode(torch.zeros(1, 3, 64, 60, device=cuda))


def test_sample_and_encode_latents(cuda, vae_pair):
    m, _ = vae_pair
    m.to(cuda)
    x = _pixels(2, 128, 160, seed=21).to(cuda)
    dist = m.encode(x).latent_dist
    s = dist.sample(torch.Generator().manual_seed(77))
    eps = torch.randn(dist.mean.shape, generator=torch.Generator().manual_seed(77)).to(cuda)
    torch.cuda.synchronize()
    check(max_ulps(s, dist.mean + dist.std * eps, _addend_mag(dist.mean, dist.std, eps)), 2.0,
          "sample(g) vs mean + std * randn(g) (ulps of the larger addend)")
    lat = m.encode_latents(x, generator=torch.Generator().manual_seed(77))
    two_step = m.encode(x).latent_dist.sample(torch.Generator().manual_seed(77)) * m.config.scaling_factor
    torch.cuda.synchronize()
    assert lat.dtype == torch.float32 and torch.equal(lat, two_step)
    assert torch.equal(dist.mode(), dist.mean)


def test_encode_graph_replay_equals_eager(cuda, vae_pair):
    m, _ = vae_pair
    m.to(cuda)
    x = _pixels(2, 128, 192, seed=7).to(cuda)
    eager = m.encode(x).latent_dist.parameters.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.encode(x)                       # warm-up on the capture stream (packs, workspaces)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.encode(x).latent_dist.parameters
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_encode_is_bit_stable_at_512(cuda, vae_pair):
    m, _ = vae_pair
    m.to(cuda)
    x = _pixels(1, 512, 512, seed=9).to(cuda)
    first = m.encode(x).latent_dist.parameters.clone()
    for _ in range(20):
        again = m.encode(x).latent_dist.parameters
        torch.cuda.synchronize()
        assert torch.equal(again, first)


def test_batch_from_images_feeds_a_training_step(cuda, vae_pair):
    from diffusion_pruning_amd.train_step import NoiseSchedule, PrunerStep, batch_from_images, noisy_latents_and_target
    from tests.test_train_step_gpu import build
    m, _ = vae_pair
    m.to(cuda)
    cfg, unet, params, hn, qz = build(cuda)
    unet.to(cuda).freeze()
    hn.to(cuda); qz.to(cuda)
    g = torch.Generator().manual_seed(31)
    px = _pixels(4, 128, 128, seed=31).to(cuda)
    ehs = torch.randn(4, 77, cfg.cross_attention_dim, generator=g).to(cuda)
    mp = (0.05 * torch.randn(4, 32, generator=g)).to(cuda)
    batch = batch_from_images(m, px, ehs, mp, generator=torch.Generator().manual_seed(5))
    assert set(batch) == {"noisy_latents", "target", "encoder_hidden_states", "mpnet_embeddings", "timesteps"}
    assert batch["noisy_latents"].shape == batch["target"].shape == (4, 4, 16, 16)
    # the same draws by hand: latents, then noise, then timesteps from one generator
    g2 = torch.Generator().manual_seed(5)
    lat = m.encode_latents(px, generator=g2)
    noise = torch.randn(lat.shape, generator=g2).to(cuda)
    t = torch.randint(0, 1000, (4,), generator=g2).to(cuda)
    noisy, target = noisy_latents_and_target(lat, noise, t, NoiseSchedule().alphas_cumprod)
    assert torch.equal(batch["timesteps"], t)
    assert torch.equal(batch["noisy_latents"], noisy) and torch.equal(batch["target"], target)
    step = PrunerStep(unet, hn, qz)
    hn.train(); qz.train()
    step.count_macs(16)
    opt = torch.optim.AdamW(step.trainable_parameters(), lr=1e-3)
    out = step.train_step(opt, batch, pretrain=True)
    assert torch.isfinite(out["loss"])
