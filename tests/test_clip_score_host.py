"""Host tests of the CLIP score path: the oracle (tests/clip_score_oracle.py) against its two golden fixtures, the coefficient
tables and crop offsets the kernels are given, the configurations and checkpoints the new classes accept and refuse, folder
pairing in the tools, and the C ABI of the three new entry points."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from diffusion_pruning_amd import _lib, metrics, ops
from diffusion_pruning_amd.clip_model import (CLIPModel, CLIPTextModelOutput, CLIPTextModelWithProjection, CLIPTextProjectionConfig)
from diffusion_pruning_amd.image_encoder import CLIPVisionConfig, CLIPVisionModelWithProjection
from diffusion_pruning_amd.text_encoder import CLIPTextConfig, CLIPTextModel
from tests import clip_score_oracle as O
from tests import clip_vision_oracle as V
from tests.helpers import rel_l2, write_safetensors

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PRE_GOLDEN = os.path.join(HERE, "golden", "clip_preprocess_tiny.npz")
MODEL_GOLDEN = os.path.join(HERE, "golden", "clip_model_tiny.npz")
VISION_GOLDEN = os.path.join(HERE, "golden", "clip_vision_tiny.npz")
TEXT_TINY = dict(vocab_size=256, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                 max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=64)
VISION_TINY = dict(hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, patch_size=14, image_size=56,
                   projection_dim=64)
PRE_CASES = ("37x53", "53x37", "64x64", "40x96", "24x24", "32x32")


def model_golden():
    """(the npz, every parameter of the tiny CLIPModel in fp64: the text tower's from clip_model_tiny, the vision tower's from
    clip_vision_tiny)"""
    z, vz = np.load(MODEL_GOLDEN), np.load(VISION_GOLDEN)
    params = {k: torch.from_numpy(z[k].astype(np.float64)) for k in z.files if k.startswith(("text_model.", "text_projection."))}
    params.update({k: torch.from_numpy(vz[k].astype(np.float64)) for k in vz.files if k.startswith(("vision_model.", "visual_projection."))})
    return z, vz, params


# ---------------------------------------------------------------------------------------------------------------------
# the oracle against its fixtures
# ---------------------------------------------------------------------------------------------------------------------
def test_integer_resampler_reproduces_pil_on_every_pixel():
    z = np.load(PRE_GOLDEN)
    assert sorted(k[3:] for k in z.files if k.startswith("in_")) == sorted(PRE_CASES)
    total = 0
    for name in PRE_CASES:
        img, size, ref = z[f"in_{name}"], int(z[f"size_{name}"]), z[f"out_{name}"]
        got = O.clip_preprocess_u8(img, size)
        assert got.dtype == np.uint8 and got.shape == ref.shape == (size, size, 3)
        assert int((got != ref).sum()) == 0, name
        total += ref.size
        assert ref.min() == 0 and ref.max() == 255, name                 # both clamps are met
    assert total == 4 * 32 * 32 * 3 + 48 * 48 * 3 + 32 * 32 * 3
    assert np.array_equal(z["in_32x32"], z["out_32x32"])                 # nothing to resize, nothing to crop


def test_text_tower_oracle_reproduces_the_model_fixture():
    z, _, params = model_golden()
    for L in (1, 9, 77):
        ids = torch.from_numpy(z[f"ids_L{L}"])
        assert tuple(ids.shape) == (3, L)
        emb, h = O.clip_text_embeds(params, ids, heads=2, layers=2, hidden_act="quick_gelu", eos_token_id=2)
        assert rel_l2(emb, torch.from_numpy(z[f"text_embeds_L{L}"])) <= 1e-9, L
        emb200, _ = O.clip_text_embeds(params, ids, heads=2, layers=2, hidden_act="quick_gelu", eos_token_id=200)
        assert rel_l2(emb200, torch.from_numpy(z[f"text_embeds_eos200_L{L}"])) <= 1e-9, L
        if L < 77:
            assert rel_l2(h, torch.from_numpy(z[f"last_hidden_state_L{L}"])) <= 1e-9, L
        else:
            assert rel_l2(h[:, -1], torch.from_numpy(z["last_hidden_state_L77_last"])) <= 1e-9
    gelu, _ = O.clip_text_embeds(params, ids, heads=2, layers=2, hidden_act="gelu")
    assert rel_l2(gelu, torch.from_numpy(z["text_embeds_L77"])) > 1e-3            # the activation is visible in the fixture


def test_the_fixture_ids_cover_the_three_pooling_cases():
    z, _, _ = model_golden()
    for L in (9, 77):
        ids = torch.from_numpy(z[f"ids_L{L}"])
        at = O.pool_index(ids, 2).tolist()
        assert at[0] == L // 2 and 0 < at[0] < L - 1                      # the largest id in the middle
        assert (ids[1] == ids[1].max()).sum() == 2 and at[1] == L // 3    # the largest id twice: the first one
        assert torch.equal(O.pool_index(ids, 2), ids.argmax(-1))
        assert O.pool_index(ids, 200).tolist() == [0, 2, 0]               # eos 200: absent, present twice, absent
        assert (ids[0] == 200).sum() == 0 and (ids[1] == 200).sum() == 2
        assert not np.allclose(z[f"text_embeds_L{L}"], z[f"text_embeds_eos200_L{L}"])
    assert O.pool_index(torch.from_numpy(z["ids_L1"]), 2).tolist() == [0, 0, 0]


def test_the_vision_tower_of_the_model_fixture_is_the_vision_fixture():
    z, vz, params = model_golden()
    vp = {k: v for k, v in params.items() if k.startswith(("vision_model.", "visual_projection."))}
    emb, _ = V.clip_vision_forward(vp, torch.from_numpy(vz["pixel_values"]), heads=2, layers=2, patch=14)
    assert rel_l2(emb, torch.from_numpy(z["image_embeds"])) <= 1e-9
    assert abs(float(z["logit_scale"]) - np.log(100.0)) < 1e-2


def test_score_oracle_on_known_vectors():
    a = torch.tensor([[3.0, 0.0, 4.0, 0.0], [0.0, 2.0, 0.0, 0.0]])
    b = torch.tensor([[3.0, 0.0, 4.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
    assert torch.allclose(O.cosines(a, b), torch.tensor([1.0, 0.0], dtype=torch.float64))
    px = O.pixel_values(np.full((1, 8, 8, 3), 255, np.uint8), 8)
    want = (1.0 - torch.tensor(O.CLIP_MEAN)) / torch.tensor(O.CLIP_STD)
    assert px.dtype == torch.float32 and torch.allclose(px[0, :, 0, 0], want, rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# coefficient tables and crop offsets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(256, 224), (512, 224), (400, 298), (160, 358), (24, 32), (53, 45), (96, 76), (1, 7), (7, 1)])
def test_table_builder_equals_the_oracle(n_in, n_out):
    b, w = ops.pil_bicubic_table(n_in, n_out)
    ob, ow = O.coeff_table(n_in, n_out)
    assert b.dtype == np.int32 and w.dtype == np.int32
    assert np.array_equal(b, ob) and np.array_equal(w, ow)
    ksize = 2 * int(np.ceil(2.0 * max(n_in / n_out, 1.0))) + 1
    assert w.shape == (n_out, ksize) and b[:, 1].max() <= ksize and b[:, 1].min() >= 1
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all()
    assert np.abs(w.sum(1) - (1 << 22)).max() <= ksize                   # rows sum to one up to the rounding of each weight
    for i in range(n_out):
        assert not w[i, b[i, 1]:].any()


def test_window_widths_of_the_two_reference_sizes():
    assert ops.pil_bicubic_table(256, 224)[1].shape[1] == 7              # support 2 * 256 / 224 = 2.29
    assert ops.pil_bicubic_table(512, 224)[1].shape[1] == 11             # support 4.57
    assert ops.pil_bicubic_table(24, 32)[1].shape[1] == 5                # an upscale: support 2


@pytest.mark.parametrize("H,W,S,want", [(37, 53, 32, (32, 45, 0, 6)),        # margin 13: 6.5 -> 6
                                         (53, 37, 32, (45, 32, 6, 0)),
                                         (40, 96, 32, (32, 76, 0, 22)),       # even margin 44
                                         (300, 400, 224, (224, 298, 0, 37)),
                                         (100, 160, 224, (224, 358, 0, 67)),
                                         (32, 35, 32, (32, 35, 0, 2)),        # margin 3: 1.5 -> 2
                                         (32, 33, 32, (32, 33, 0, 0)),        # margin 1: 0.5 -> 0
                                         (32, 37, 32, (32, 37, 0, 2)),        # margin 5: 2.5 -> 2
                                         (256, 256, 224, (224, 224, 0, 0))])
def test_resized_size_and_crop_offsets(H, W, S, want):
    assert ops.pil_resized_size(H, W, S) == want
    assert O.resized_size(H, W, S) == want[:2]
    assert (O.crop_offset(want[0], S), O.crop_offset(want[1], S)) == want[2:]
    lib = _lib.load()
    out = [ctypes.c_int32() for _ in range(4)]
    assert lib.aptp_image_patches_pil_size(H, W, S, *[ctypes.byref(v) for v in out]) == 0
    assert tuple(v.value for v in out) == want
    assert lib.aptp_image_patches_pil_size(H, W, S, None, None, None, None) == 0


# ---------------------------------------------------------------------------------------------------------------------
# configurations, checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def test_quick_gelu_is_accepted_here_and_still_refused_by_clip_text_model():
    for act in ("quick_gelu", "gelu"):
        assert CLIPTextModelWithProjection(CLIPTextProjectionConfig(**{**TEXT_TINY, "hidden_act": act})).config.hidden_act == act
    with pytest.raises(NotImplementedError, match="quick_gelu"):
        CLIPTextModel(CLIPTextConfig(**{k: v for k, v in TEXT_TINY.items() if k != "projection_dim"}))
    assert CLIPTextModel(CLIPTextConfig(**{**{k: v for k, v in TEXT_TINY.items() if k != "projection_dim"}, "hidden_act": "gelu"}))


@pytest.mark.parametrize("bad", [dict(hidden_act="gelu_new"), dict(hidden_act="relu"), dict(hidden_size=192, num_attention_heads=2),
                                 dict(hidden_size=128, num_attention_heads=4), dict(max_position_embeddings=129),
                                 dict(projection_dim=60)])
def test_unsupported_text_configs_raise(bad):
    with pytest.raises(NotImplementedError):
        CLIPTextModelWithProjection(CLIPTextProjectionConfig(**{**TEXT_TINY, **bad}))


def test_default_config_is_vit_b_32s_text_tower():
    cfg = CLIPTextProjectionConfig()
    assert (cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.head_dim,
            cfg.max_position_embeddings, cfg.hidden_act, cfg.projection_dim) == (49408, 512, 2048, 12, 8, 64, 77, "quick_gelu", 512)
    m = CLIPTextModelWithProjection(cfg)
    H, I = 512, 2048
    layer = 4 * (H * H + H) + (H * I + I) + (I * H + H) + 2 * 2 * H
    assert sum(p.numel() for p in m.parameters()) == 49408 * H + 77 * H + 12 * layer + 2 * H + H * 512
    assert m.eos_mode == "argmax"
    assert CLIPTextModelWithProjection(CLIPTextProjectionConfig(**{**TEXT_TINY, "eos_token_id": 49407})).eos_mode == "first_eos"
    full = {"projection_dim": 64, "text_config": {k: v for k, v in TEXT_TINY.items() if k != "projection_dim"}, "vision_config": {}}
    assert CLIPTextProjectionConfig.from_dict(full) == CLIPTextProjectionConfig(**TEXT_TINY)


def test_forward_refuses_the_cpu_and_unsupported_arguments():
    m = CLIPTextModelWithProjection(CLIPTextProjectionConfig(**TEXT_TINY)).init_synthetic(0)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        m(torch.zeros(1, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        m.embed_ids(torch.zeros(1, 4, dtype=torch.long))
    for kw in (dict(attention_mask=torch.ones(1, 4)), dict(position_ids=torch.arange(4)[None]), dict(output_hidden_states=True)):
        with pytest.raises(NotImplementedError):
            m(torch.zeros(1, 4, dtype=torch.long), **kw)
    e, h = torch.zeros(1, 3), torch.ones(1, 2, 3)
    o = CLIPTextModelOutput(text_embeds=e, last_hidden_state=h)
    assert o[0] is e and o[1] is h and o["text_embeds"] is e and o.to_tuple() == (e, h)


def test_golden_parameters_load_into_the_modules():
    _, _, params = model_golden()
    tp = {k: v.float() for k, v in params.items() if k.startswith("text_")}
    m = CLIPTextModelWithProjection(CLIPTextProjectionConfig(**TEXT_TINY)).load_text_state_dict({k: v.float() for k, v in params.items()})
    assert set(m.state_dict()) == set(tp)
    for k, v in tp.items():
        assert torch.equal(m.state_dict()[k], v), k


def _clip_folder(tmp_path, sd, config=None):
    d = tmp_path / "clip"
    d.mkdir()
    cfg = {"model_type": "clip", "projection_dim": 64, "logit_scale_init_value": 2.6592,
           "text_config": {k: v for k, v in TEXT_TINY.items() if k != "projection_dim"},
           "vision_config": {k: v for k, v in VISION_TINY.items() if k != "projection_dim"}}
    (d / "config.json").write_text(json.dumps(config or cfg))
    write_safetensors(str(d / "model.safetensors"), sd)
    return str(d)


def _clip_state_dict():
    t = CLIPTextModelWithProjection(CLIPTextProjectionConfig(**TEXT_TINY)).init_synthetic(3)
    v = CLIPVisionModelWithProjection(CLIPVisionConfig(**VISION_TINY)).init_synthetic(4)
    sd = {**t.state_dict(), **v.state_dict(), "logit_scale": torch.tensor(4.25)}
    sd["text_model.embeddings.position_ids"] = torch.arange(77)[None]
    sd["vision_model.embeddings.position_ids"] = torch.arange(17)[None]
    return t, v, sd


def test_clip_model_from_pretrained(tmp_path):
    t, v, sd = _clip_state_dict()
    folder = _clip_folder(tmp_path, sd)
    m = CLIPModel.from_pretrained(folder)
    assert m.text_model.config == CLIPTextProjectionConfig(**TEXT_TINY) and m.vision_model.config == CLIPVisionConfig(**VISION_TINY)
    assert m.projection_dim == 64 and m.logit_scale == 4.25 and abs(m.logit_scale_exp - np.exp(4.25)) < 1e-9
    for src, got in ((t, m.text_model), (v, m.vision_model)):
        for k, val in src.state_dict().items():
            assert torch.equal(got.state_dict()[k], val), k
    only_text = CLIPTextModelWithProjection.from_pretrained(folder)
    assert torch.equal(only_text.text_projection.weight, t.text_projection.weight)
    assert not any(k.startswith("vision") or k == "logit_scale" for k in only_text.state_dict())
    sm = metrics.ClipScoreModel(m)
    assert sm.input_image_size == 56 and abs(sm.logit_scale - np.exp(4.25)) < 1e-9


@pytest.mark.parametrize("change", ["missing", "extra", "shape", "no_logit_scale", "missing_vision"])
def test_from_pretrained_is_strict(tmp_path, change):
    _, _, sd = _clip_state_dict()
    if change == "missing":
        sd.pop("text_projection.weight")
    elif change == "extra":
        sd["text_model.encoder.layers.1.mlp.fc3.bias"] = torch.zeros(128)
    elif change == "shape":
        sd["text_projection.weight"] = torch.zeros(128, 64)
    elif change == "no_logit_scale":
        sd.pop("logit_scale")
    else:
        sd.pop("vision_model.post_layernorm.bias")
    folder = _clip_folder(tmp_path, sd)
    with pytest.raises((KeyError, ValueError)):
        CLIPModel.from_pretrained(folder)
    if change in ("missing", "extra", "shape"):
        with pytest.raises((KeyError, ValueError)):
            CLIPTextModelWithProjection.from_pretrained(folder)


def test_clip_model_needs_a_clip_model_config_and_matching_projections(tmp_path):
    _, _, sd = _clip_state_dict()
    with pytest.raises(ValueError, match="text_config"):
        CLIPModel.from_pretrained(_clip_folder(tmp_path, sd, {**TEXT_TINY, "model_type": "clip_text_model"}))
    with pytest.raises(ValueError, match="project"):
        CLIPModel(CLIPTextModelWithProjection(CLIPTextProjectionConfig(**TEXT_TINY)),
                  CLIPVisionModelWithProjection(CLIPVisionConfig(**{**VISION_TINY, "projection_dim": 32})))


def test_every_layer_changes_the_stream_under_init_synthetic():
    cfg = CLIPTextProjectionConfig()
    m = CLIPTextModelWithProjection(cfg).init_synthetic(0)
    ids = torch.randint(3, cfg.vocab_size, (1, 77), generator=torch.Generator().manual_seed(1))
    sd = m.state_dict()
    prev = None
    for n in range(0, 13, 4):
        x = O.text_stream(sd, ids, heads=8, layers=n, dtype=torch.float32)
        if prev is not None:
            assert float((x - prev).norm() / prev.norm()) >= 0.05, n
        prev = x


# ---------------------------------------------------------------------------------------------------------------------
# metrics, tools
# ---------------------------------------------------------------------------------------------------------------------
def test_clip_score_model_argument_checks():
    m = CLIPModel(CLIPTextModelWithProjection(CLIPTextProjectionConfig(**TEXT_TINY)), CLIPVisionModelWithProjection(CLIPVisionConfig(**VISION_TINY)))
    with pytest.raises(ValueError, match="precision"):
        metrics.ClipScoreModel(m, precision="fp16")
    with pytest.raises(TypeError):
        metrics.ClipScoreModel(m.vision_model)
    sm = metrics.ClipScoreModel(m)
    assert sm.precision == "bf16" and abs(sm.logit_scale - 100.0) < 0.01
    img = np.zeros((2, 8, 8, 3), np.uint8)
    ids = np.zeros((2, 5), np.int64)
    with pytest.raises(ValueError, match="uint8"):
        sm.image_features(img.astype(np.float32))
    with pytest.raises(ValueError, match=r"\[n, H, W, 3\]"):
        sm.image_features(np.zeros((2, 3, 8, 8), np.uint8))
    with pytest.raises(ValueError, match="batch_size"):
        sm.image_features(img, batch_size=0)
    with pytest.raises(ValueError, match="integer"):
        sm.text_features(ids.astype(np.float32))
    with pytest.raises(ValueError, match="not both"):
        sm.score(img, ids, text_features=np.zeros((2, 64), np.float32))
    with pytest.raises(ValueError, match="not both"):
        sm.score(img)
    with pytest.raises(RuntimeError, match="HIP kernels only"):                  # the model is on the CPU
        sm.image_features(img)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        sm.text_features(ids)


def test_ops_wrappers_refuse_cpu_and_mistyped_tensors():
    with pytest.raises(ValueError, match="uint8"):
        ops.image_patches_pil(torch.zeros(1, 8, 8, 3), 8, 4)
    with pytest.raises(ValueError, match="uint8"):
        ops.image_patches_pil(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 8, 4)              # not on a GPU
    with pytest.raises(ValueError, match="int64"):
        ops.eos_pool_ln(torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, 4, 64), torch.ones(64), torch.zeros(64))
    with pytest.raises(ValueError, match="fp32"):
        ops.paired_cosine(torch.zeros(2, 8), torch.zeros(2, 8))
    with pytest.raises(ValueError):
        ops.pil_bicubic_table(0, 4)
    with pytest.raises(ValueError):
        ops.pil_resized_size(0, 4, 4)


def test_tools_pair_folders_by_sorted_name(tmp_path):
    sys.path.insert(0, ROOT)
    from tools import clip_features, clip_score
    a, b = tmp_path / "images", tmp_path / "features"
    a.mkdir()
    b.mkdir()
    for n in ("000010.npy", "000002.npy", "000001.npy", ".hidden"):
        (a / n).write_bytes(b"")
    for n in ("cap_b.npy", "cap_a.npy", "cap_c.npy", ".DS_Store"):
        (b / n).write_bytes(b"")
    pairs = clip_score.pair_folders(str(a), str(b))
    assert [(os.path.basename(x), os.path.basename(y)) for x, y in pairs] == [("000001.npy", "cap_a.npy"), ("000002.npy", "cap_b.npy"),
                                                                              ("000010.npy", "cap_c.npy")]
    (b / "cap_d.npy").write_bytes(b"")
    with pytest.raises(SystemExit, match="3 images"):
        clip_score.pair_folders(str(a), str(b))
    assert clip_features.feature_names(3) == ["000000", "000001", "000002"]
    names = tmp_path / "names.txt"
    names.write_text("b.txt\na.txt\nc.txt\n")
    assert clip_features.feature_names(3, str(names)) == ["b", "a", "c"]
    with pytest.raises(SystemExit):
        clip_features.feature_names(4, str(names))


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_and_bound():
    import re
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aptp_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(aptp_[a-z_0-9]+)\s*\(", src))
    bound = {n for n, _, _ in _lib.EXPORTS}
    new = {"aptp_image_patches_pil", "aptp_image_patches_pil_size", "aptp_eos_pool_ln", "aptp_paired_cosine"}
    assert new <= declared and new <= bound and declared == bound
    lib = _lib.load()
    for n in new:
        assert getattr(lib, n) is not None


def test_new_ctypes_layouts_match_the_c_header(tmp_path):
    structs = {"AptpImagePatchesPilParams": _lib.ImagePatchesPilParams, "AptpEosPoolLnParams": _lib.EosPoolLnParams,
               "AptpPairedCosineParams": _lib.PairedCosineParams}
    body = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "aptp_hip.h")}"', "int main(void){"]
    want = []
    for cname, cls in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            body.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            want.append(getattr(cls, fname).offset)
    body.append('printf("%d\\n%d\\n", (int)APTP_EOS_ARGMAX, (int)APTP_EOS_FIRST);')
    want += [_lib.EOS_ARGMAX, _lib.EOS_FIRST]
    body.append("return 0;}")
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(body))
    subprocess.run(["cc", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want


def test_c_entry_points_refuse_bad_arguments_before_launching():
    """never dereferenced pointers: each launch is refused by the argument checks"""
    lib = _lib.load()
    err = lambda: lib.aptp_last_error()                                          # noqa: E731
    ip = _lib.ImagePatchesPilParams()
    assert lib.aptp_image_patches_pil(ctypes.byref(ip), None) == -1 and b"null pointer" in err()
    ip.x, ip.out, ip.scratch = 1 << 20, 2 << 20, 3 << 20
    ip.xbounds, ip.xweights, ip.ybounds, ip.yweights = (i << 20 for i in range(4, 8))
    ip.B, ip.H, ip.W, ip.S, ip.P, ip.ldo, ip.xk, ip.yk = 1, 0, 64, 56, 14, 640, 7, 7
    for c in range(3):
        ip.std[c] = 1.0
    assert lib.aptp_image_patches_pil(ctypes.byref(ip), None) == -1 and b"shorter side" in err()      # an image whose shorter side is 0
    ip.H, ip.W = 64, 0
    assert lib.aptp_image_patches_pil(ctypes.byref(ip), None) == -1 and b"shorter side" in err()
    ip.W, ip.S = 64, 60
    assert lib.aptp_image_patches_pil(ctypes.byref(ip), None) == -1 and b"multiple of P" in err()
    ip.S, ip.ldo = 56, 588
    assert lib.aptp_image_patches_pil(ctypes.byref(ip), None) == -1 and b"ldo" in err()
    ip.ldo, ip.xk = 640, 5                                                       # 64 -> 56 needs ceil(2 * 64 / 56) * 2 + 1 = 7 taps
    assert lib.aptp_image_patches_pil(ctypes.byref(ip), None) == -1 and b"wider than the horizontal table" in err()
    ip.xk, ip.yk = 7, 6
    assert lib.aptp_image_patches_pil(ctypes.byref(ip), None) == -1 and b"wider than the vertical table" in err()
    ip.yk, ip.xweights = 7, None
    assert lib.aptp_image_patches_pil(ctypes.byref(ip), None) == -1 and b"the width changes" in err()
    ip.xweights, ip.std[1] = 5 << 20, 0.0
    assert lib.aptp_image_patches_pil(ctypes.byref(ip), None) == -1 and b"std must be positive" in err()
    ip.std[1], ip.out = 1.0, (2 << 20) + 4
    assert lib.aptp_image_patches_pil(ctypes.byref(ip), None) == -1 and b"alignment" in err()
    assert lib.aptp_image_patches_pil_size(0, 4, 4, None, None, None, None) == -1 and b"shorter side" in err()
    assert lib.aptp_image_patches_pil_size(1, 16384, 224, None, None, None, None) == -1 and b"aspect ratio" in err()

    ep = _lib.EosPoolLnParams()
    assert lib.aptp_eos_pool_ln(ctypes.byref(ep), None) == -1 and b"null pointer" in err()
    ep.ids, ep.x, ep.gamma, ep.beta, ep.out, ep.out_act = (i << 20 for i in range(1, 7))
    ep.B, ep.L, ep.C, ep.x_stride_b, ep.x_stride_l, ep.ldo_act, ep.eps = 2, 7, 2056, 7 * 2056, 2056, 2056, 1e-5
    assert lib.aptp_eos_pool_ln(ctypes.byref(ep), None) == -1 and b"bad extents" in err()
    ep.C, ep.x_stride_b, ep.x_stride_l, ep.ldo_act, ep.eos_mode = 128, 7 * 128, 128, 128, 2
    assert lib.aptp_eos_pool_ln(ctypes.byref(ep), None) == -1 and b"eos_mode" in err()
    ep.eos_mode, ep.x_stride_l = 1, 120
    assert lib.aptp_eos_pool_ln(ctypes.byref(ep), None) == -1 and b"strides" in err()
    ep.x_stride_l, ep.ldo_act = 128, 132
    assert lib.aptp_eos_pool_ln(ctypes.byref(ep), None) == -1 and b"ldo_act" in err()
    ep.ldo_act, ep.eps = 128, 0.0
    assert lib.aptp_eos_pool_ln(ctypes.byref(ep), None) == -1 and b"eps" in err()
    ep.eps, ep.gamma = 1e-5, (3 << 20) + 4
    assert lib.aptp_eos_pool_ln(ctypes.byref(ep), None) == -1 and b"alignment" in err()

    pc = _lib.PairedCosineParams()
    assert lib.aptp_paired_cosine(ctypes.byref(pc), None) == -1 and b"null pointer" in err()
    pc.a, pc.b, pc.cos_out, pc.sum_out = (i << 20 for i in range(1, 5))
    pc.n, pc.D, pc.lda, pc.ldb = 4, 6, 8, 8
    assert lib.aptp_paired_cosine(ctypes.byref(pc), None) == -1 and b"multiple of 4" in err()
    pc.D, pc.lda = 8, 4
    assert lib.aptp_paired_cosine(ctypes.byref(pc), None) == -1 and b"row strides" in err()
    pc.lda, pc.n = 8, 0
    assert lib.aptp_paired_cosine(ctypes.byref(pc), None) == -1 and b"bad extents" in err()
    pc.n, pc.sum_out = 4, (4 << 20) + 4
    assert lib.aptp_paired_cosine(ctypes.byref(pc), None) == -1 and b"alignment" in err()
