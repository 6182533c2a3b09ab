"""CPU checks of the VAE encoder's host side: module structure against diffusers' SD-2.1 VAE, the whole-model loader, the
synthetic weights, the MAC table, the slicing plan, the new ABI structs and argument checks, the distribution's semantics and
the training batch's add-noise / velocity helper."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import vae_encoder_oracle as E
from tests import vae_oracle as V
from tests.helpers import write_safetensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aptp_hip.h")


def _enc_keys(sd):
    return {k: v for k, v in sd.items() if k.startswith("encoder.") or k.startswith("quant_conv.")}


def test_parameter_count_and_names_follow_diffusers():
    from diffusion_pruning_amd.vae import AutoencoderKL
    m = AutoencoderKL(with_encoder=True)
    assert sum(p.numel() for p in m.parameters()) == 83_653_863
    assert sum(p.numel() for n, p in m.named_parameters() if n.startswith(("encoder.", "quant_conv."))) == 34_163_664
    sd = m.state_dict()
    ref = {**V.DecoderOracle().state_dict(), **E.EncoderOracle().state_dict()}
    assert set(sd) == set(ref)
    for k in sd:
        assert tuple(sd[k].shape) == tuple(ref[k].shape), k
    for k, shape in {"encoder.conv_in.weight": (128, 3, 3, 3), "encoder.conv_out.weight": (8, 512, 3, 3),
                     "quant_conv.weight": (8, 8, 1, 1), "encoder.down_blocks.0.downsamplers.0.conv.weight": (128, 128, 3, 3),
                     "encoder.down_blocks.1.resnets.0.conv_shortcut.weight": (256, 128, 1, 1),
                     "encoder.mid_block.attentions.0.to_k.weight": (512, 512),
                     "encoder.conv_norm_out.weight": (512,)}.items():
        assert tuple(sd[k].shape) == shape, k
    assert not any(k.startswith("encoder.down_blocks.3.downsamplers") for k in sd)
    # the default instance is the decoder alone, as before
    d = AutoencoderKL()
    assert not any(k.startswith(("encoder.", "quant_conv.")) for k in d.state_dict())
    assert list(d.state_dict()) == [k for k in sd if not k.startswith(("encoder.", "quant_conv."))]


def _vae_dir(tmp_path, disk):
    d = tmp_path / "vae"
    d.mkdir()
    (d / "config.json").write_text(json.dumps({"_class_name": "AutoencoderKL", "block_out_channels": [128, 256, 512, 512],
                                               "latent_channels": 4, "layers_per_block": 2, "norm_num_groups": 32,
                                               "scaling_factor": 0.18215, "sample_size": 768}))
    write_safetensors(str(d / "diffusion_pytorch_model.safetensors"), disk)
    return str(tmp_path)


def _full_sd(seed=0):
    g = torch.Generator().manual_seed(seed)
    ref = {**V.DecoderOracle().state_dict(), **E.EncoderOracle().state_dict()}
    return {k: torch.randn(v.shape, generator=g) * 0.01 for k, v in ref.items()}


@pytest.mark.parametrize("naming", ["to_qkv", "deprecated"])
def test_loader_reads_encoder_with_both_attention_namings(naming, tmp_path):
    from diffusion_pruning_amd.vae import AutoencoderKL
    sd = _full_sd()
    disk = dict(sd)
    if naming == "deprecated":
        for pre in ("encoder.mid_block.attentions.0.", "decoder.mid_block.attentions.0."):
            for new, old in (("to_q", "query"), ("to_k", "key"), ("to_v", "value"), ("to_out.0", "proj_attn")):
                disk[pre + old + ".weight"] = disk.pop(pre + new + ".weight")[:, :, None, None]
                disk[pre + old + ".bias"] = disk.pop(pre + new + ".bias")
    root = _vae_dir(tmp_path, disk)
    m = AutoencoderKL.from_pretrained(root, subfolder="vae", with_encoder=True)
    assert m.with_encoder
    got = m.state_dict()
    assert set(got) == set(sd)
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    # the decoder-only load of the same folder still ignores the encoder
    d = AutoencoderKL.from_pretrained(root, subfolder="vae")
    assert not d.with_encoder and set(d.state_dict()) == {k for k in sd if not k.startswith(("encoder.", "quant_conv."))}


def test_loader_rejects_missing_and_misshaped_encoder_keys():
    from diffusion_pruning_amd.vae import AutoencoderKL
    sd = _full_sd()
    bad = dict(sd)
    bad.pop("encoder.down_blocks.2.resnets.1.conv2.weight")
    with pytest.raises(KeyError):
        AutoencoderKL(with_encoder=True).load_vae_state_dict(bad)
    bad = dict(sd)
    bad.pop("quant_conv.bias")
    with pytest.raises(KeyError):
        AutoencoderKL(with_encoder=True).load_vae_state_dict(bad)
    bad = dict(sd)
    bad["encoder.conv_out.weight"] = torch.zeros(4, 512, 3, 3)
    with pytest.raises(ValueError):
        AutoencoderKL(with_encoder=True).load_vae_state_dict(bad)
    bad = dict(sd)
    bad["encoder.extra.weight"] = torch.zeros(1)
    with pytest.raises(KeyError):
        AutoencoderKL(with_encoder=True).load_vae_state_dict(bad)


def test_init_synthetic_keeps_the_decoder_weights_and_encoder_moments_are_order_one():
    from diffusion_pruning_amd.vae import AutoencoderKL
    dec = AutoencoderKL().init_synthetic(3).state_dict()
    full = AutoencoderKL(with_encoder=True).init_synthetic(3).state_dict()
    for k, v in dec.items():
        assert torch.equal(full[k], v), k
    o = E.EncoderOracle()
    o.load_state_dict(_enc_keys(full))
    x = torch.rand(1, 3, 64, 96, generator=torch.Generator().manual_seed(1)) * 2 - 1
    with torch.no_grad():
        y32 = o(x)
        y64 = o.double()(x.double())
    assert float((y32.double() - y64).norm() / y64.norm()) < 1e-5
    assert y64.shape == (1, 8, 8, 12)
    assert 0.1 <= float(y64.std()) <= 10.0


@pytest.mark.parametrize("H,W", [(256, 256), (512, 512), (192, 320)])
def test_mac_table_equals_hook_count_of_the_oracle(H, W):
    from diffusion_pruning_amd.vae import VAEConfig, vae_encoder_macs
    hooked = V.count_macs(E.EncoderOracle().to("meta"), torch.empty(1, 3, H, W, device="meta"))
    macs, attn = vae_encoder_macs(VAEConfig(), H, W)
    assert macs == hooked
    assert attn == 2 * (H * W // 64) ** 2 * 512
    if (H, W) == (256, 256):
        assert macs == 136_361_082_880


def test_encoder_slicing_plan_stays_below_the_verified_size():
    from diffusion_pruning_amd.vae import (MAX_TENSOR_BYTES, VAEConfig, encoder_largest_activation_elements,
                                           encoder_slice_plan)
    cfg = VAEConfig()
    assert encoder_largest_activation_elements(cfg, 512, 512) == 512 * 512 * 128
    for H, W, B, esz in ((256, 256, 64, 2), (512, 512, 64, 2), (512, 512, 64, 4), (768, 768, 16, 2), (192, 320, 8, 4)):
        plan = encoder_slice_plan(cfg, B, H, W, esz)
        assert sum(plan) == B
        assert max(plan) * encoder_largest_activation_elements(cfg, H, W) * esz < MAX_TENSOR_BYTES
    assert encoder_slice_plan(cfg, 64, 256, 256) == [64]        # the reference's training point runs in one slice
    assert len(encoder_slice_plan(cfg, 64, 512, 512)) > 1


def test_new_ctypes_structs_match_the_c_layout():
    from diffusion_pruning_amd import _lib
    structs = {"AptpImageInParams": _lib.ImageInParams, "AptpLatentDistParams": _lib.LatentDistParams,
               "AptpConvGemmParams": _lib.ConvGemmParams}
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        body.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            body.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    body.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(body))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.strip().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert _lib.ConvGemmParams._fields_[-1][0] == "pad_end"
    names = {n for n, _, _ in _lib.EXPORTS}
    assert {"aptp_image_in", "aptp_latent_dist"} <= names


def _lib_loaded():
    from diffusion_pruning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.load()


def _conv_params(_lib):
    # a stride-2, pad-0 3x3 problem on an 8 x 8 map.  The pointers are not real: every call below must fail its argument
    # checks, and tile 9999 (no such tile) stops even a call that passes them before any launch
    p = _lib.ConvGemmParams()
    p.x = p.w = p.y = 1 << 20
    p.B, p.Hin, p.Win, p.Cin, p.ldx = 1, 8, 8, 64, 64
    p.KH, p.KW, p.stride, p.pad = 3, 3, 2, 0
    p.N, p.cin_pad, p.ldy, p.split_k, p.tile = 64, 64, 64, 1, 9999
    return p


def test_new_entry_points_reject_bad_arguments_without_launching():
    _lib, lib = _lib_loaded()
    p = _conv_params(_lib)
    p.Hout = p.Wout = 4                          # (8 + 0 + 1 - 3) / 2 + 1: consistent with pad_end = 1 only
    p.pad_end = 0
    assert lib.aptp_conv_gemm(ctypes.byref(p), None) == -1
    assert b"inconsistent" in lib.aptp_last_error()
    p.pad_end = 1                                # geometry accepted: stops at the (deliberately unknown) tile
    assert lib.aptp_conv_gemm(ctypes.byref(p), None) == -1
    assert b"unknown tile" in lib.aptp_last_error()
    p.pad_end = -1
    assert lib.aptp_conv_gemm(ctypes.byref(p), None) == -1
    assert b"pad_end" in lib.aptp_last_error()
    p.pad_end = 1
    p.corr, p.corr_B = 1 << 20, 1
    assert lib.aptp_conv_gemm(ctypes.byref(p), None) == -1
    assert b"pad_end" in lib.aptp_last_error()
    p.corr, p.corr_B = None, 0
    p.ups = 1
    assert lib.aptp_conv_gemm(ctypes.byref(p), None) == -1
    assert b"pad_end" in lib.aptp_last_error()
    p.ups = 0
    p.x2, p.ldx2, p.Cin2, p.cin2_pad = 1 << 20, 64, 64, 64
    assert lib.aptp_conv_gemm(ctypes.byref(p), None) == -1
    assert b"pad_end" in lib.aptp_last_error()

    a = _lib.ImageInParams()
    assert lib.aptp_image_in(ctypes.byref(a), None) == -1
    assert b"null pointer" in lib.aptp_last_error()
    a.x = a.out = 1 << 20
    a.B, a.C, a.H, a.W = 1, 4, 8, 8
    assert lib.aptp_image_in(ctypes.byref(a), None) == -1          # 3 channels only
    assert b"3 channels" in lib.aptp_last_error()
    a.C, a.H = 3, 0
    assert lib.aptp_image_in(ctypes.byref(a), None) == -1

    d = _lib.LatentDistParams()
    assert lib.aptp_latent_dist(ctypes.byref(d), None) == -1
    d.y = d.wq = d.bq = 1 << 20
    d.B, d.H, d.W, d.ldy, d.scale = 1, 4, 4, 8, 1.0
    assert lib.aptp_latent_dist(ctypes.byref(d), None) == -1       # nothing to write
    d.eps = 1 << 20
    assert lib.aptp_latent_dist(ctypes.byref(d), None) == -1       # eps without latents
    d.latents, d.moments, d.ldy = 1 << 20, 1 << 20, 4
    assert lib.aptp_latent_dist(ctypes.byref(d), None) == -1       # ldy < 8
    d.ldy, d.H = 8, 0
    assert lib.aptp_latent_dist(ctypes.byref(d), None) == -1


def test_ops_conv_gemm_rejects_pad_end_with_ups_corr_or_x2():
    from diffusion_pruning_amd import ops
    pw = ops.pack_weight(torch.zeros(64, 64, 3, 3), torch.zeros(64), device="cpu")
    x = torch.zeros(1, 8, 8, 64, dtype=ops.ACT_DTYPE)
    for kw in ({"pad_end": -1}, {"pad_end": 1, "ups": 1}, {"pad_end": 1, "corr": torch.zeros(1, 9, 64)}):
        with pytest.raises(ValueError):
            ops.conv_gemm(x, pw, stride=2, pad=0, **kw)


def test_decoder_only_instance_still_refuses_encode():
    from diffusion_pruning_amd.vae import AutoencoderKL
    with pytest.raises(NotImplementedError):
        AutoencoderKL().encode(torch.zeros(1, 3, 64, 64))
    with pytest.raises(NotImplementedError):
        AutoencoderKL().encode_latents(torch.zeros(1, 3, 64, 64))


def test_distribution_follows_diffusers_on_the_cpu():
    from diffusion_pruning_amd.vae import DiagonalGaussianDistribution, randn_tensor
    g = torch.Generator().manual_seed(0)
    par = torch.randn(2, 8, 5, 6, generator=g) * 3
    par[0, 4, 0, 0], par[0, 5, 0, 0] = -50.0, 40.0                  # past both clamp bounds
    other = torch.randn(2, 8, 5, 6, generator=g)
    d, r = DiagonalGaussianDistribution(par), E.DiagonalGaussianDistribution(par)
    for f in ("mean", "logvar", "std", "var"):
        assert torch.equal(getattr(d, f), getattr(r, f)), f
    assert float(d.logvar.min()) == -30.0 and float(d.logvar.max()) == 20.0
    assert torch.equal(d.mode(), r.mode())
    assert torch.equal(d.kl(), r.kl())
    assert torch.equal(d.kl(DiagonalGaussianDistribution(other)), r.kl(E.DiagonalGaussianDistribution(other)))
    s = torch.randn(2, 4, 5, 6, generator=g)
    assert torch.equal(d.nll(s), r.nll(s))
    eps = torch.randn(2, 4, 5, 6, generator=torch.Generator().manual_seed(9))
    assert torch.equal(d.sample(torch.Generator().manual_seed(9)), r.sample(eps))
    assert torch.equal(randn_tensor((2, 4, 5, 6), torch.Generator().manual_seed(9)), eps)
    det = DiagonalGaussianDistribution(par, deterministic=True)
    assert float(det.std.abs().sum()) == 0.0 and float(det.kl()[0]) == 0.0


@pytest.mark.parametrize("prediction_type", ["v_prediction", "epsilon"])
def test_add_noise_and_target_helper(prediction_type):
    from diffusion_pruning_amd.train_step import NoiseSchedule, noisy_latents_and_target
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(6, 4, 8, 8, generator=g)
    noise = torch.randn(6, 4, 8, 8, generator=g)
    t = torch.tensor([0, 1, 250, 500, 998, 999])
    ac = NoiseSchedule().alphas_cumprod
    noisy, target = noisy_latents_and_target(x0, noise, t, ac, prediction_type)
    for i in range(6):
        a = float(ac[t[i]])
        sa, so = np.sqrt(a), np.sqrt(1 - a)
        assert torch.allclose(noisy[i].double(), sa * x0[i].double() + so * noise[i].double(), rtol=1e-6, atol=1e-6)
        want = noise[i].double() if prediction_type == "epsilon" else sa * noise[i].double() - so * x0[i].double()
        assert torch.allclose(target[i].double(), want, rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError):
        noisy_latents_and_target(x0, noise, t, ac, "sample")
