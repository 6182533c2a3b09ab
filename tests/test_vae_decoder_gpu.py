"""The HIP VAE decoder on the GPU: the wide-head attention kernel and the image epilogue against torch math, the whole
decoder against the CPU oracle (tests/vae_oracle.py) in bf16 and on the fp32 parity path, graph capture, and the pipeline's
image outputs.  Margins go through tests.margins.check, which keeps the measured values."""
import numpy as np
import pytest
import torch

from tests import vae_oracle as V
from tests.helpers import rel_l2
from tests.margins import check

pytestmark = pytest.mark.gpu

ATTN_BF16_TOL = 4e-3
ATTN_F32_TOL = 1e-5
DEC_BF16_TOL = 2e-2
DEC_F32_TOL = 1e-4


def _qkv(B, L, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, L, 3 * 512, generator=g) * 1.5      # fused q|k|v buffer, read through strided views
    qkv = qkv.to(device=dev, dtype=dtype)
    return qkv[..., :512], qkv[..., 512:1024], qkv[..., 1024:]


def _ref_attention(q, k, v):
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.transpose(1, 2) * 512 ** -0.5
    return torch.softmax(s, dim=-1) @ v


@pytest.mark.parametrize("L", [1, 81, 200, 1024, 4096])
@pytest.mark.parametrize("B", [1, 4, 8])
def test_attention_wide_bf16(cuda, B, L):
    from diffusion_pruning_amd import ops
    q, k, v = _qkv(B, L, torch.bfloat16, cuda, seed=B * 10007 + L)
    out = ops.attention_wide(q, k, v)
    torch.cuda.synchronize()
    ref = _ref_attention(q.float(), k.float(), v.float())
    assert torch.isfinite(out.float()).all()
    check(rel_l2(out, ref), ATTN_BF16_TOL, f"attention_wide bf16 B={B} L={L}")


@pytest.mark.parametrize("L", [1, 81, 200, 1024])
@pytest.mark.parametrize("B", [1, 4])
def test_attention_wide_fp32(cuda, B, L):
    from diffusion_pruning_amd import ops
    q, k, v = _qkv(B, L, torch.float32, cuda, seed=B * 7919 + L)
    out = ops.attention_wide(q, k, v)
    torch.cuda.synchronize()
    check(rel_l2(out, _ref_attention(q, k, v)), ATTN_F32_TOL, f"attention_wide fp32 B={B} L={L}")


def test_attention_wide_lq_ne_lk_and_explicit_scale(cuda):
    from diffusion_pruning_amd import ops
    g = torch.Generator().manual_seed(5)
    q = torch.randn(2, 70, 512, generator=g).to(cuda, torch.bfloat16)
    k = torch.randn(2, 333, 512, generator=g).to(cuda, torch.bfloat16)
    v = torch.randn(2, 333, 512, generator=g).to(cuda, torch.bfloat16)
    out = ops.attention_wide(q, k, v, scale=0.02)
    s = q.double() @ k.double().transpose(1, 2) * 0.02
    ref = torch.softmax(s, -1) @ v.double()
    check(rel_l2(out, ref), ATTN_BF16_TOL, "attention_wide bf16 Lq=70 Lk=333 scale=0.02")


def test_attention_wide_is_bit_stable(cuda):
    from diffusion_pruning_amd import ops
    q, k, v = _qkv(4, 4096, torch.bfloat16, cuda, seed=11)
    first = ops.attention_wide(q, k, v).clone()
    for _ in range(20):
        again = ops.attention_wide(q, k, v)
        torch.cuda.synchronize()
        assert torch.equal(again, first)


@pytest.mark.parametrize("shape", [(2, 64, 64), (1, 37, 53)])
def test_image_out_is_bit_exact(cuda, shape):
    from diffusion_pruning_amd import ops
    B, H, W = shape
    g = torch.Generator().manual_seed(3)
    y = (torch.randn(B, H, W, 8, generator=g) * 1.5).to(cuda)
    y[0, 0, 0, :3] = torch.tensor([-1.0, 1.0, 0.0])                       # the clamp ends and 0.5
    y[0, 0, 1, :3] = torch.tensor([2 * (0.5 / 255) - 1, 2 * (1.5 / 255) - 1, 3.0])   # (near) rounding ties
    pt = ops.image_out(y, torch.float32)
    u8 = ops.image_out(y, torch.uint8)
    torch.cuda.synchronize()
    ref = V.postprocess(y[..., :3].permute(0, 3, 1, 2))
    assert pt.shape == (B, 3, H, W) and torch.equal(pt, ref.contiguous())
    ref8 = torch.from_numpy((ref.permute(0, 2, 3, 1).cpu().numpy() * 255).round().astype("uint8"))
    assert u8.shape == (B, H, W, 3) and u8.dtype == torch.uint8 and torch.equal(u8.cpu(), ref8)


@pytest.fixture(scope="module")
def vae_pair():
    from diffusion_pruning_amd.vae import AutoencoderKL
    m = AutoencoderKL().init_synthetic(seed=0)
    oracle = V.DecoderOracle()
    oracle.load_state_dict(m.state_dict())
    oracle.eval()
    return m, oracle


def _latents(B, h, w, seed):
    return torch.randn(B, 4, h, w, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("B,h,w", [(2, 32, 32), (1, 64, 64), (1, 24, 40)])
def test_decoder_bf16_against_oracle(cuda, vae_pair, B, h, w):
    m, oracle = vae_pair
    m.to(cuda)
    z = _latents(B, h, w, seed=h * 100 + w)
    out = m.decode(z.to(cuda)).sample
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = oracle.float()(z)
    assert out.shape == ref.shape == (B, 3, 8 * h, 8 * w)
    assert 0.1 <= float(ref.std()) <= 10.0
    check(rel_l2(out, ref), DEC_BF16_TOL, f"vae decode bf16 B={B} latent {h}x{w}")


def test_decoder_fp32_parity_path(cuda, vae_pair, monkeypatch):
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd.vae import AutoencoderKL
    monkeypatch.setattr(ops, "ACT_DTYPE", torch.float32)
    m0, oracle = vae_pair
    m = AutoencoderKL()
    m.load_state_dict(m0.state_dict())
    m.to(cuda)
    z = _latents(1, 16, 16, seed=16)
    out = m.decode(z.to(cuda)).sample
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = oracle.double()(z.double())
    oracle.float()
    check(rel_l2(out, ref), DEC_F32_TOL, "vae decode fp32 parity B=1 latent 16")


def test_decode_graph_replay_equals_eager(cuda, vae_pair):
    m, _ = vae_pair
    m.to(cuda)
    z = _latents(2, 16, 24, seed=7).to(cuda)
    eager = m.decode(z).sample.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.decode(z)                       # warm-up on the capture stream (packs, workspaces)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.decode(z).sample
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_pipeline_decodes_images(cuda, vae_pair):
    from diffusion_pruning_amd.pipeline import PruningDenoiseLoop
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    from oracle import unet_oracle as O
    m, _ = vae_pair
    m.to(cuda)
    cfg = O.TINY
    unet = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                     cross_attention_dim=cfg.cross_attention_dim).init_synthetic(seed=0).to(cuda)
    loop = PruningDenoiseLoop(unet, vae=m)
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(2, 4, 16, 16, generator=g).to(cuda)
    ehs = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).to(cuda)
    base = loop(ehs, lat, num_inference_steps=3, use_graph=False)
    assert base.images is None
    res = loop(ehs, lat, num_inference_steps=3, use_graph=False, output_type="pt")
    assert torch.equal(res.latents, base.latents)
    ref = V.postprocess(m.decode(res.latents / 0.18215).sample)
    assert res.images.shape == (2, 3, 128, 128) and res.images.dtype == torch.float32
    assert torch.equal(res.images, ref)
    npi = loop(ehs, lat, num_inference_steps=3, use_graph=False, output_type="np").images
    assert isinstance(npi, np.ndarray) and npi.shape == (2, 128, 128, 3) and npi.dtype == np.float32
    assert np.array_equal(npi, ref.permute(0, 2, 3, 1).cpu().numpy())
    pil = loop(ehs, lat, num_inference_steps=3, use_graph=False, output_type="pil").images
    assert len(pil) == 2 and pil[0].size == (128, 128) and pil[0].mode == "RGB"
    want = (ref.permute(0, 2, 3, 1).cpu().numpy() * 255).round().astype("uint8")
    assert np.array_equal(np.asarray(pil[1]), want[1])
