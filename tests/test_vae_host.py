"""CPU checks of the VAE decoder's host side: module structure against diffusers' SD-2.1 VAE, the FLOP table, the weight
loader, the oracle, the slicing plan, the new ABI structs and the pipeline's default output."""
import ctypes
import json
import os
import subprocess
import tempfile

import pytest
import torch

from tests import vae_oracle as V
from tests.helpers import write_safetensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aptp_hip.h")


def test_parameter_count_and_names_follow_diffusers():
    from diffusion_pruning_amd.vae import AutoencoderKL, VAEConfig
    m = AutoencoderKL(VAEConfig())
    assert sum(p.numel() for p in m.parameters()) == 49_490_199
    sd = m.state_dict()
    ref = V.DecoderOracle().state_dict()
    assert set(sd) == set(ref)
    for k in sd:
        assert tuple(sd[k].shape) == tuple(ref[k].shape), k
    for k, shape in {"post_quant_conv.weight": (4, 4, 1, 1), "decoder.conv_in.weight": (512, 4, 3, 3),
                     "decoder.mid_block.attentions.0.to_q.weight": (512, 512),
                     "decoder.mid_block.attentions.0.to_out.0.bias": (512,),
                     "decoder.mid_block.attentions.0.group_norm.weight": (512,),
                     "decoder.up_blocks.2.resnets.0.conv_shortcut.weight": (256, 512, 1, 1),
                     "decoder.up_blocks.0.upsamplers.0.conv.weight": (512, 512, 3, 3),
                     "decoder.conv_norm_out.weight": (128,), "decoder.conv_out.weight": (3, 128, 3, 3)}.items():
        assert tuple(sd[k].shape) == shape, k
    assert not any(k.startswith("decoder.up_blocks.3.upsamplers") for k in sd)
    assert m.config.scaling_factor == 0.18215


@pytest.mark.parametrize("h,w", [(32, 32), (64, 64), (24, 40)])
def test_flop_table_equals_hook_count_of_the_oracle(h, w):
    from diffusion_pruning_amd.vae import VAEConfig, vae_decoder_macs
    model = V.DecoderOracle().to("meta")
    hooked = V.count_macs(model, torch.empty(1, 4, h, w, device="meta"))
    macs, attn = vae_decoder_macs(VAEConfig(), h, w)
    assert macs == hooked
    assert attn == 2 * (h * w) ** 2 * 512
    if (h, w) == (32, 32):
        assert macs == 311_093_641_216
    if (h, w) == (64, 64):
        assert macs == 1_257_259_466_752


def _small_sd(seed=0):
    g = torch.Generator().manual_seed(seed)
    ref = V.DecoderOracle().state_dict()
    return {k: torch.randn(v.shape, generator=g) * 0.01 for k, v in ref.items()}


@pytest.mark.parametrize("naming", ["to_qkv", "deprecated"])
def test_loader_reads_both_attention_namings_and_ignores_the_encoder(naming, tmp_path):
    from diffusion_pruning_amd.vae import AutoencoderKL
    sd = _small_sd()
    disk = dict(sd)
    disk["encoder.conv_in.weight"] = torch.zeros(128, 3, 3, 3)
    disk["quant_conv.weight"] = torch.zeros(8, 8, 1, 1)
    if naming == "deprecated":
        pre = "decoder.mid_block.attentions.0."
        for new, old in (("to_q", "query"), ("to_k", "key"), ("to_v", "value"), ("to_out.0", "proj_attn")):
            disk[pre + old + ".weight"] = disk.pop(pre + new + ".weight")[:, :, None, None]      # 1x1-conv shaped
            disk[pre + old + ".bias"] = disk.pop(pre + new + ".bias")
    d = tmp_path / "vae"
    d.mkdir()
    (d / "config.json").write_text(json.dumps({"_class_name": "AutoencoderKL", "block_out_channels": [128, 256, 512, 512],
                                               "latent_channels": 4, "layers_per_block": 2, "norm_num_groups": 32,
                                               "scaling_factor": 0.18215, "sample_size": 768}))
    write_safetensors(str(d / "diffusion_pytorch_model.safetensors"), disk)
    m = AutoencoderKL.from_pretrained(str(tmp_path), subfolder="vae")
    got = m.state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k], v), k


def test_loader_rejects_missing_and_misshaped_keys(tmp_path):
    from diffusion_pruning_amd.vae import AutoencoderKL
    sd = _small_sd()
    bad = dict(sd)
    bad.pop("decoder.up_blocks.1.resnets.2.conv1.weight")
    with pytest.raises(KeyError):
        AutoencoderKL().load_decoder_state_dict(bad)
    bad = dict(sd)
    bad["decoder.conv_out.weight"] = torch.zeros(3, 128, 1, 1)
    with pytest.raises(ValueError):
        AutoencoderKL().load_decoder_state_dict(bad)


def test_encode_is_not_implemented():
    from diffusion_pruning_amd.vae import AutoencoderKL
    with pytest.raises(NotImplementedError):
        AutoencoderKL().encode(torch.zeros(1, 3, 64, 64))


def test_oracle_fp32_agrees_with_fp64_and_synthetic_output_is_order_one():
    from diffusion_pruning_amd.vae import AutoencoderKL
    sd = AutoencoderKL().init_synthetic(0).state_dict()
    o = V.DecoderOracle()
    o.load_state_dict(sd)
    z = torch.randn(1, 4, 8, 12, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        y32 = o(z)
        y64 = o.double()(z.double())
    err = float((y32.double() - y64).norm() / y64.norm())
    assert err < 1e-5, err
    assert 0.1 <= float(y64.std()) <= 10.0


def test_slicing_plan_stays_below_the_verified_size():
    from diffusion_pruning_amd.vae import MAX_TENSOR_BYTES, VAEConfig, largest_activation_elements, slice_plan
    cfg = VAEConfig()
    assert largest_activation_elements(cfg, 64, 64) == 512 * 512 * 256
    for h, w, B, esz in ((96, 96, 64, 2), (96, 96, 64, 4), (64, 64, 16, 2), (32, 32, 8, 2), (24, 40, 8, 2)):
        plan = slice_plan(cfg, B, h, w, esz)
        assert sum(plan) == B
        assert max(plan) * largest_activation_elements(cfg, h, w) * esz < MAX_TENSOR_BYTES
    assert slice_plan(cfg, 8, 32, 32) == [8]           # the reference point runs in one slice
    assert len(slice_plan(cfg, 64, 96, 96)) > 1


def test_new_ctypes_structs_match_the_c_layout():
    from diffusion_pruning_amd import _lib
    structs = {"AptpAttentionWideParams": _lib.AttentionWideParams, "AptpImageOutParams": _lib.ImageOutParams}
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
    names = {n for n, _, _ in _lib.EXPORTS}
    assert {"aptp_attention_wide", "aptp_image_out"} <= names


def test_new_entry_points_reject_bad_arguments_without_launching():
    from diffusion_pruning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    a = _lib.AttentionWideParams()
    assert lib.aptp_attention_wide(ctypes.byref(a), None) == -1
    assert b"null pointer" in lib.aptp_last_error()
    a.q = a.k = a.v = a.o = 4096
    a.B, a.Lq, a.Lk, a.scale = 1, 10, 10, 0.0
    for st in ("q_stride_l", "k_stride_l", "v_stride_l", "o_stride_l"):
        setattr(a, st, 512)
    assert lib.aptp_attention_wide(ctypes.byref(a), None) == -1          # scale must be positive
    a.scale, a.k_stride_l = 0.04, 500
    assert lib.aptp_attention_wide(ctypes.byref(a), None) == -1          # row stride below the head width
    a.k_stride_l, a.Lk = 512, 0
    assert lib.aptp_attention_wide(ctypes.byref(a), None) == -1
    o = _lib.ImageOutParams()
    assert lib.aptp_image_out(ctypes.byref(o), None) == -1
    o.y, o.out, o.ldy, o.B, o.H, o.W = 4096, 4096, 2, 1, 4, 4
    assert lib.aptp_image_out(ctypes.byref(o), None) == -1              # ldy < 3


def test_pipeline_default_output_is_unchanged():
    import dataclasses
    from diffusion_pruning_amd.pipeline import PipelineOutput, PruningDenoiseLoop
    names = [f.name for f in dataclasses.fields(PipelineOutput)]
    assert names == ["latents", "arch_indices", "arch_vectors_quantized", "resource_ratios", "images"]
    out = PipelineOutput(latents=torch.zeros(1), arch_indices=None, arch_vectors_quantized=None)
    assert out.resource_ratios is None and out.images is None
    loop = PruningDenoiseLoop(unet=None)
    assert loop.vae is None
    with pytest.raises(ValueError):
        loop(torch.zeros(1, 77, 8), torch.zeros(1, 4, 8, 8), output_type="pt")       # no vae
    with pytest.raises(ValueError):
        loop(torch.zeros(1, 77, 8), torch.zeros(1, 4, 8, 8), output_type="png")
