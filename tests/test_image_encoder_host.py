"""Host tests of the CLIP image encoder and the image metrics: the oracle against the two golden fixtures (and against
transformers where it imports), the configuration, the FLOP count, strict loading, rejected configurations and arguments, the
ctypes layouts and the argument checks of the new C entry points and of metrics.py."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from diffusion_pruning_amd import metrics
from diffusion_pruning_amd.image_encoder import (CLIPVisionConfig, CLIPVisionModelOutput, CLIPVisionModelWithProjection,
                                                 image_encoder_flops)
from tests import clip_vision_oracle as O
from tests.helpers import rel_l2, write_safetensors

HERE = os.path.dirname(os.path.abspath(__file__))
VISION_GOLDEN = os.path.join(HERE, "golden", "clip_vision_tiny.npz")
CMMD_GOLDEN = os.path.join(HERE, "golden", "cmmd_tiny.npz")
TINY = dict(hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, patch_size=14, image_size=56,
            projection_dim=64)
MMD_BOUND = 1000 * 4 * 2.0 ** -23          # granularity of the reference's own fp32 result (three means just under 1, x 1000)
# config.json of openai/clip-vit-large-patch14-336 (a CLIPModel file: the vision tower is its vision_config)
L14_336_CONFIG = {"architectures": ["CLIPModel"], "model_type": "clip", "projection_dim": 768, "logit_scale_init_value": 2.6592,
                  "text_config": {"hidden_size": 768, "intermediate_size": 3072, "num_hidden_layers": 12, "projection_dim": 768},
                  "vision_config": {"hidden_size": 1024, "intermediate_size": 4096, "num_hidden_layers": 24, "num_attention_heads": 16,
                                    "patch_size": 14, "image_size": 336, "projection_dim": 768, "hidden_act": "quick_gelu",
                                    "layer_norm_eps": 1e-05, "model_type": "clip_vision_model", "num_channels": 3}}


def _vision_golden():
    z = np.load(VISION_GOLDEN)
    params = {k: torch.from_numpy(z[k].astype(np.float64)) for k in z.files
              if not k.startswith(("pixel_values", "last_hidden_state_", "image_embeds_"))}
    return z, params


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_oracle_reproduces_the_vision_fixture(act):
    z, params = _vision_golden()
    px = torch.from_numpy(z["pixel_values"])
    for dtype, tol in ((torch.float64, 1e-9), (torch.float32, 1e-5)):
        emb, h = O.clip_vision_forward(params, px, heads=2, layers=2, patch=14, hidden_act=act, dtype=dtype)
        assert rel_l2(h, torch.from_numpy(z[f"last_hidden_state_{act}"])) <= tol, (act, dtype)
        assert rel_l2(emb, torch.from_numpy(z[f"image_embeds_{act}"])) <= tol, (act, dtype)
    assert z["last_hidden_state_quick_gelu"].shape == (2, 17, 128) and z["image_embeds_gelu"].shape == (2, 64)
    assert rel_l2(torch.from_numpy(z["image_embeds_gelu"]), torch.from_numpy(z["image_embeds_quick_gelu"])) > 1e-3


def test_oracle_reproduces_the_cmmd_fixture():
    z = np.load(CMMD_GOLDEN)
    assert [tuple(int(v) for v in r[:3]) for r in z["mmd_cases"][::2]] == O.MMD_CASES
    for (n, m, D, shift), f32, f64, xs, ys in zip(z["mmd_cases"], z["mmd_f32"], z["mmd_f64"], z["mmd_xsum"], z["mmd_ysum"]):
        x, y = O.cmmd_embeddings(int(n), int(m), int(D), float(shift))
        assert x.astype(np.float64).sum() == xs and y.astype(np.float64).sum() == ys, "the seeded draws changed"
        got = O.mmd(x, y)
        assert abs(got - f64) <= 1e-9 * max(1.0, abs(f64)), (n, m, D, shift, got, f64)
        assert abs(f32 - got) <= MMD_BOUND, (n, m, D, shift, f32, got)          # the reference's fp32 result is inside the bound
    x, y = O.cmmd_embeddings(*O.MMD_CASES[-1], O.MMD_SHIFTS[0])
    assert np.array_equal(x, z["small_x"]) and np.array_equal(y, z["small_y"])
    assert abs(O.mmd(x, x)) <= 1e-9
    for name in ("up", "down", "identity", "nonsquare"):
        img, size = torch.from_numpy(z[f"resize_{name}_in"]), int(z[f"resize_{name}_size"])
        ref = torch.from_numpy(z[f"resize_{name}_out"])
        assert tuple(ref.shape) == (img.shape[0], size, size, 3)
        assert rel_l2(O.resize_bicubic(img, size), ref) <= 1e-5, name
        assert rel_l2(O.resize_bicubic(img.double(), size), ref) <= 1e-5, name
    assert torch.equal(O.resize_bicubic(torch.from_numpy(z["resize_identity_in"]), 56), torch.from_numpy(z["resize_identity_in"]))


def test_oracle_preprocess_and_patch_rows_are_the_patch_convolution():
    g = torch.Generator().manual_seed(2)
    img = torch.rand(2, 40, 24, 3, generator=g)
    px = O.preprocess(img, 28)
    assert tuple(px.shape) == (2, 3, 28, 28) and px.dtype == torch.float64
    back = px * torch.tensor(O.CLIP_STD, dtype=torch.float64).view(1, 3, 1, 1) + torch.tensor(O.CLIP_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    assert rel_l2(back.permute(0, 2, 3, 1), O.resize_bicubic(img.double(), 28)) <= 1e-12
    w = torch.randn(8, 3, 14, 14, generator=g).double()
    conv = torch.nn.functional.conv2d(px, w, stride=14).flatten(2).transpose(1, 2).reshape(-1, 8)
    assert rel_l2(O.patch_rows(px, 14) @ w.flatten(1).t(), conv) <= 1e-12


def test_clip_score_oracle():
    a = torch.tensor([[3.0, 0.0, 4.0, 0.0], [0.0, 2.0, 0.0, 0.0]])
    b = torch.tensor([[3.0, 0.0, 4.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
    assert abs(O.clip_score(a, b) - 50.0) <= 1e-12 and abs(O.clip_score(a, b, logit_scale=2.0) - 1.0) <= 1e-12


def test_golden_parameters_load_into_the_module():
    _, params = _vision_golden()
    m = CLIPVisionModelWithProjection(CLIPVisionConfig(**TINY))
    m.load_vision_state_dict({k: v.float() for k, v in params.items()})
    assert set(m.state_dict()) == set(params)


def test_oracle_matches_transformers_at_the_vit_b_32_config():
    tr = pytest.importorskip("transformers")
    c = CLIPVisionConfig.vit_b_32()
    cfg = tr.CLIPVisionConfig(hidden_size=c.hidden_size, intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers,
                              num_attention_heads=c.num_attention_heads, patch_size=c.patch_size, image_size=c.image_size,
                              projection_dim=c.projection_dim, hidden_act=c.hidden_act)
    cfg._attn_implementation = "eager"
    ref = tr.CLIPVisionModelWithProjection(cfg).eval()
    sd = CLIPVisionModelWithProjection(c).init_synthetic(0).state_dict()
    missing, unexpected = ref.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    px = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        r = ref(pixel_values=px)
    emb, h = O.clip_vision_forward(sd, px, heads=12, layers=12, patch=32)
    assert rel_l2(h, r.last_hidden_state) <= 1e-5 and rel_l2(emb, r.image_embeds) <= 1e-5


def test_default_config_parameter_count_and_flops():
    cfg = CLIPVisionConfig.from_dict(L14_336_CONFIG)
    assert cfg == CLIPVisionConfig()
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.head_dim) == (1024, 4096, 24, 16, 64)
    assert (cfg.patch_size, cfg.image_size, cfg.projection_dim, cfg.hidden_act, cfg.layer_norm_eps) == (14, 336, 768, "quick_gelu", 1e-5)
    assert (cfg.grid, cfg.num_tokens) == (24, 577)
    H, I, T, P = 1024, 4096, 577, 14
    layer = 4 * (H * H + H) + (H * I + I) + (I * H + H) + 2 * 2 * H                # q, k, v, out; fc1; fc2; two LayerNorms
    count = H + H * 3 * P * P + T * H + 2 * H + 24 * layer + 2 * H + H * 768      # class, patch, position, pre-LN, layers, post-LN, projection
    m = CLIPVisionModelWithProjection(cfg)
    assert sum(p.numel() for p in m.parameters()) == count
    flops = 2 * 576 * 3 * P * P * H + 24 * (2 * T * (4 * H * H + 2 * H * I) + 4 * H * T * T) + 2 * H * 768
    assert image_encoder_flops(cfg) == float(flops)
    assert 3.4e11 < image_encoder_flops(cfg) < 3.9e11                              # ~0.37 TFLOP per image
    b32 = CLIPVisionConfig.vit_b_32()
    assert (b32.hidden_size, b32.intermediate_size, b32.num_hidden_layers, b32.num_attention_heads, b32.patch_size, b32.image_size,
            b32.projection_dim, b32.num_tokens) == (768, 3072, 12, 12, 32, 224, 512, 50)
    assert CLIPVisionModelWithProjection(b32).config.head_dim == 64
    assert CLIPVisionConfig.from_dict({**L14_336_CONFIG["vision_config"], "hidden_act": "gelu"}).hidden_act == "gelu"


@pytest.mark.parametrize("bad", [dict(hidden_act="gelu_new"), dict(hidden_act="relu"), dict(hidden_size=1280, num_attention_heads=16),
                                 dict(hidden_size=128, num_attention_heads=4), dict(num_channels=1)])
def test_unsupported_configs_raise(bad):
    with pytest.raises(NotImplementedError):
        CLIPVisionModelWithProjection(CLIPVisionConfig(**{**TINY, **bad}))


def test_a_patch_size_that_does_not_divide_the_image_raises():
    with pytest.raises(ValueError):
        CLIPVisionModelWithProjection(CLIPVisionConfig(**{**TINY, "image_size": 60}))


@pytest.mark.parametrize("kw", [dict(output_attentions=True), dict(output_hidden_states=True), dict(interpolate_pos_encoding=True),
                                dict(attention_mask=torch.ones(1, 17))])
def test_unsupported_forward_arguments_raise(kw):
    m = CLIPVisionModelWithProjection(CLIPVisionConfig(**TINY))
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 3, 56, 56), **kw)


def test_forward_refuses_the_cpu_and_bad_shapes():
    m = CLIPVisionModelWithProjection(CLIPVisionConfig(**TINY)).init_synthetic(0)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        m(torch.zeros(1, 3, 56, 56))
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        m.embed_images(torch.zeros(1, 56, 56, 3))


def test_output_indexing_follows_transformers():
    e, h = torch.zeros(1, 3), torch.ones(1, 2, 3)
    o = CLIPVisionModelOutput(image_embeds=e, last_hidden_state=h)
    assert o[0] is e and o[1] is h and o["last_hidden_state"] is h and o.image_embeds is e and o.to_tuple() == (e, h)


def _folder(tmp_path, sd, config=None):
    d = tmp_path / "clip"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(config or {**TINY, "hidden_act": "quick_gelu", "model_type": "clip_vision_model"}))
    write_safetensors(str(d / "model.safetensors"), sd)
    return str(d)


def test_from_pretrained_with_a_stray_position_ids(tmp_path):
    src = CLIPVisionModelWithProjection(CLIPVisionConfig(**TINY)).init_synthetic(3)
    sd = dict(src.state_dict())
    sd["vision_model.embeddings.position_ids"] = torch.arange(17)[None].float()
    m = CLIPVisionModelWithProjection.from_pretrained(_folder(tmp_path, sd))
    assert m.config == CLIPVisionConfig(**TINY)
    for k, v in src.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k


def test_from_pretrained_skips_the_text_tower_of_a_full_clip_model(tmp_path):
    src = CLIPVisionModelWithProjection(CLIPVisionConfig(**TINY)).init_synthetic(4)
    sd = dict(src.state_dict())
    sd.update({"text_model.embeddings.token_embedding.weight": torch.zeros(10, 8), "text_model.embeddings.position_ids": torch.zeros(1, 7),
               "text_model.encoder.layers.0.mlp.fc1.bias": torch.zeros(8), "text_model.final_layer_norm.weight": torch.zeros(8),
               "text_projection.weight": torch.zeros(64, 8), "logit_scale": torch.tensor(4.6)})
    config = {"model_type": "clip", "projection_dim": 64, "text_config": {"hidden_size": 8},
              "vision_config": {k: v for k, v in TINY.items() if k != "projection_dim"}}
    m = CLIPVisionModelWithProjection.from_pretrained(_folder(tmp_path, sd, config))
    assert m.config == CLIPVisionConfig(**TINY)
    for k, v in src.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    assert not any(k.startswith("text_") or k == "logit_scale" for k in m.state_dict())


@pytest.mark.parametrize("change", ["missing", "extra", "shape", "misnamed_pre_layernorm"])
def test_from_pretrained_is_strict(tmp_path, change):
    sd = dict(CLIPVisionModelWithProjection(CLIPVisionConfig(**TINY)).init_synthetic(3).state_dict())
    if change == "missing":
        sd.pop("vision_model.encoder.layers.1.mlp.fc2.bias")
    elif change == "extra":
        sd["vision_model.encoder.layers.1.mlp.fc3.bias"] = torch.zeros(128)
    elif change == "shape":
        sd["vision_model.post_layernorm.weight"] = torch.zeros(64)
    else:
        sd["vision_model.pre_layernorm.weight"] = sd.pop("vision_model.pre_layrnorm.weight")
    with pytest.raises((KeyError, ValueError)):
        CLIPVisionModelWithProjection.from_pretrained(_folder(tmp_path, sd))


def test_every_layer_changes_the_stream_under_init_synthetic():
    c = CLIPVisionConfig.vit_b_32()
    m = CLIPVisionModelWithProjection(c).init_synthetic(0)
    img = torch.rand(1, 64, 64, 3, generator=torch.Generator().manual_seed(1))
    streams = []
    O.clip_vision_forward(m.state_dict(), O.preprocess(img, 224), heads=12, layers=12, patch=32, dtype=torch.float32, streams=streams)
    assert len(streams) == 13
    for i in range(1, 13):
        rel = float((streams[i] - streams[i - 1]).norm() / streams[i - 1].norm())
        assert rel >= 0.05, (i, rel)


def test_new_ctypes_layouts_match_the_c_header(tmp_path):
    import subprocess
    from diffusion_pruning_amd import _lib
    root = os.path.dirname(HERE)
    structs = {"AptpImagePatchesParams": _lib.ImagePatchesParams, "AptpVitEmbedLnParams": _lib.VitEmbedLnParams,
               "AptpL2NormalizeParams": _lib.L2NormalizeParams, "AptpMmdRbfParams": _lib.MmdRbfParams}
    body = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(root, "include", "aptp_hip.h")}"', "int main(void){"]
    want = []
    for cname, cls in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            body.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            want.append(getattr(cls, fname).offset)
    body.append('printf("%d\\n", (int)APTP_ACT_QUICK_GELU);')
    want.append(_lib.ACT_QUICK_GELU)
    body.append("return 0;}")
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(body))
    subprocess.run(["cc", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert _lib.ACT_QUICK_GELU == 5 and _lib.ACT_GELU == 3


def test_c_entry_points_refuse_bad_extents_before_launching():
    """never dereferenced pointers: each launch is refused by the argument checks"""
    from diffusion_pruning_amd import _lib
    lib = _lib.load()
    err = lambda: lib.aptp_last_error()                                          # noqa: E731
    ip = _lib.ImagePatchesParams()
    assert lib.aptp_image_patches(ctypes.byref(ip), None) == -1 and b"null pointer" in err()
    ip.x, ip.out = 1 << 20, 2 << 20
    ip.B, ip.H, ip.W, ip.S, ip.P, ip.resize, ip.ldo = 1, 64, 64, 60, 14, 1, 640
    assert lib.aptp_image_patches(ctypes.byref(ip), None) == -1 and b"multiple of P" in err()
    ip.S, ip.ldo = 56, 588
    assert lib.aptp_image_patches(ctypes.byref(ip), None) == -1 and b"ldo" in err()
    ip.ldo = 640
    assert lib.aptp_image_patches(ctypes.byref(ip), None) == -1 and b"std must be positive" in err()
    ip.resize = 0
    assert lib.aptp_image_patches(ctypes.byref(ip), None) == -1 and b"pixel_values" in err()
    ip.resize, ip.B = 1, 0
    assert lib.aptp_image_patches(ctypes.byref(ip), None) == -1 and b"bad extents" in err()
    ip.B, ip.out = 1, (2 << 20) + 4
    for c in range(3):
        ip.std[c] = 1.0
    assert lib.aptp_image_patches(ctypes.byref(ip), None) == -1 and b"alignment" in err()

    ve = _lib.VitEmbedLnParams()
    assert lib.aptp_vit_embed_ln(ctypes.byref(ve), None) == -1 and b"null pointer" in err()
    ve.patches, ve.cls, ve.pos, ve.gamma, ve.beta, ve.out = (i << 20 for i in range(1, 7))
    ve.ldp, ve.ldo, ve.B, ve.T, ve.C, ve.eps = 128, 128, 1, 17, 2056, 1e-5
    assert lib.aptp_vit_embed_ln(ctypes.byref(ve), None) == -1 and b"bad extents" in err()
    ve.C, ve.T = 128, 1
    assert lib.aptp_vit_embed_ln(ctypes.byref(ve), None) == -1 and b"bad extents" in err()
    ve.T, ve.ldo = 17, 132
    assert lib.aptp_vit_embed_ln(ctypes.byref(ve), None) == -1 and b"ldo" in err()
    ve.ldo, ve.eps = 128, 0.0
    assert lib.aptp_vit_embed_ln(ctypes.byref(ve), None) == -1 and b"eps" in err()
    ve.eps, ve.pos = 1e-5, (3 << 20) + 4
    assert lib.aptp_vit_embed_ln(ctypes.byref(ve), None) == -1 and b"alignment" in err()

    l2 = _lib.L2NormalizeParams()
    assert lib.aptp_l2_normalize(ctypes.byref(l2), None) == -1 and b"null pointer" in err()
    l2.x, l2.out, l2.n, l2.D, l2.ldx, l2.ldo = 1 << 20, 2 << 20, 4, 6, 6, 6
    assert lib.aptp_l2_normalize(ctypes.byref(l2), None) == -1 and b"multiple of 4" in err()
    l2.D, l2.ldx, l2.ldo = 8, 4, 8
    assert lib.aptp_l2_normalize(ctypes.byref(l2), None) == -1 and b"row strides" in err()

    mm = _lib.MmdRbfParams()
    assert lib.aptp_mmd_rbf(ctypes.byref(mm), None) == -1 and b"null pointer" in err()
    mm.x, mm.y, mm.workspace, mm.out = (i << 20 for i in range(1, 5))
    mm.n, mm.m, mm.D, mm.ldx, mm.ldy, mm.sigma, mm.scale = 0, 4, 64, 64, 64, 10.0, 1000.0
    assert lib.aptp_mmd_rbf(ctypes.byref(mm), None) == -1 and b"bad extents" in err()
    mm.n, mm.D = 4, 66
    assert lib.aptp_mmd_rbf(ctypes.byref(mm), None) == -1 and b"bad extents" in err()
    mm.D, mm.ldy = 64, 60
    assert lib.aptp_mmd_rbf(ctypes.byref(mm), None) == -1 and b"row strides" in err()
    mm.ldy, mm.sigma = 64, 0.0
    assert lib.aptp_mmd_rbf(ctypes.byref(mm), None) == -1 and b"sigma" in err()
    mm.sigma, mm.workspace = 10.0, (3 << 20) + 8
    assert lib.aptp_mmd_rbf(ctypes.byref(mm), None) == -1 and b"alignment" in err()
    # the workspace: squared norms of every row and one partial per 128 x 128 tile of the three kernel matrices
    assert lib.aptp_mmd_rbf_workspace_bytes(0, 5) == 0
    assert lib.aptp_mmd_rbf_workspace_bytes(128, 129) == 4 * (260 + 1 + 4 + 2)
    assert lib.aptp_mmd_rbf_workspace_bytes(16384, 16384) == 4 * (32768 + 3 * 128 * 128) < (1 << 20)


def test_metrics_argument_checks():
    m = CLIPVisionModelWithProjection(CLIPVisionConfig(**TINY))
    with pytest.raises(ValueError, match="precision"):
        metrics.ClipEmbeddingModel(m, precision="fp16")
    with pytest.raises(TypeError):
        metrics.ClipEmbeddingModel(torch.nn.Linear(2, 2))
    em = metrics.ClipEmbeddingModel(m)
    assert em.input_image_size == 56 and em.precision in ("bf16", "fp32")
    with pytest.raises(ValueError, match="batch_size"):
        em.embed(np.zeros((2, 8, 8, 3), np.float32), batch_size=0)
    for bad in (np.zeros((2, 3, 8, 8), np.float32), np.zeros((8, 8, 3), np.float32), np.zeros((0, 8, 8, 3), np.float32)):
        with pytest.raises(ValueError, match=r"\[B, H, W, 3\]"):
            em.embed(bad)
    with pytest.raises(RuntimeError, match="HIP kernels only"):                    # the model is on the CPU
        em.embed(np.zeros((2, 8, 8, 3), np.float32))
    with pytest.raises(ValueError, match="no CPU path"):
        metrics.mmd(torch.zeros(4, 8), torch.zeros(4, 8))
    with pytest.raises(ValueError, match="no CPU path"):
        metrics.clip_score(torch.zeros(4, 8), torch.zeros(4, 8))
    with pytest.raises(ValueError, match="reference set"):
        metrics.compute_cmmd(np.zeros((4, 8, 3), np.float32), np.zeros((2, 8, 8, 3), np.float32), m)
    with pytest.raises(TypeError):
        metrics.compute_cmmd(np.zeros((4, 64), np.float32), np.zeros((2, 8, 8, 3), np.float32), torch.nn.Linear(2, 2))
