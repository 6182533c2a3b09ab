"""The CLIP score path on the GPU: the PIL-exact image front end against the integer oracle (itself pinned to PIL on every pixel),
the pooled LayerNorm and the paired cosine against fp64, the text tower with its projection against the CPU oracle in bf16 and on
the fp32 parity path, graph replay, and the whole score of a tiny CLIPModel against an fp64 evaluation of the reference's formula.
Margins go through tests.margins.check, which keeps the measured values.

  CLIP score, tiny CLIPModel, 24 pairs (measured on MI355X, profiles/clip_score_parity_margins.json): fp64 oracle
  4.325290, fp32 parity path 4.325292 (3.1e-7 relative), bf16 path 4.287803 (0.0375 lower; largest per-pair cosine error 2.1e-3)."""
import numpy as np
import pytest
import torch

from tests import clip_score_oracle as O
from tests.helpers import rel_l2
from tests.margins import check
from tests.test_clip_score_host import PRE_CASES, PRE_GOLDEN, TEXT_TINY, VISION_TINY, model_golden

pytestmark = pytest.mark.gpu

LN_BF16_TOL = 4e-3              # tests/test_ops_gpu.py's budget of ops.layernorm
LN_F32_TOL = 1e-5               # tests/test_fp32_parity_gpu.py's budget of one fp32 op
ENC_BF16_TOL = 2e-2             # tests/test_text_encoder_gpu.py's budgets of the whole SD-2.1 tower
ENC_F32_TOL = 1e-4
COS_TOL = 1e-6
SCORE_F32_RTOL = 1e-4
SCORE_BF16_COS_TOL = 4e-2       # |d cos| <= |d a| + |d b| for unit vectors, each embedding within ENC_BF16_TOL


# ---------------------------------------------------------------------------------------------------------------------
# aptp_image_patches_pil
# ---------------------------------------------------------------------------------------------------------------------
def _unpatchify(rows, B, S, P):
    G = S // P
    return rows[:, :3 * P * P].reshape(B, G, G, 3, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, S, S)


def _pil_cases():
    z = np.load(PRE_GOLDEN)
    cases = [(name, z[f"in_{name}"][None], int(z[f"size_{name}"]), 16 if name == "64x64" else 4) for name in PRE_CASES]
    rs = np.random.RandomState(5)
    for name, B, H, W, S, P in (("256x256", 2, 256, 256, 224, 32), ("512x512", 2, 512, 512, 224, 14), ("300x400", 1, 300, 400, 224, 14)):
        img = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
        pick = rs.rand(B, H, W, 3)
        img[pick < 0.1], img[pick > 0.9] = 0, 255
        cases.append((name, img, S, P))
    return cases


@pytest.fixture(scope="module")
def pil_cases():
    """(name, uint8 images, size, patch, the oracle's uint8 output [B, size, size, 3]) -- computed once"""
    return {name: (img, S, P, np.stack([O.clip_preprocess_u8(im, S) for im in img])) for name, img, S, P in _pil_cases()}


@pytest.mark.parametrize("name", list(PRE_CASES) + ["256x256", "512x512", "300x400"])
def test_image_patches_pil_is_pil_on_every_pixel(cuda, pil_cases, name):
    from diffusion_pruning_amd import ops
    img, S, P, ref_u8 = pil_cases[name]
    if name in PRE_CASES:
        assert np.array_equal(ref_u8[0], np.load(PRE_GOLDEN)[f"out_{name}"])            # the oracle is PIL here
    B = img.shape[0]
    K, kpad = 3 * P * P, (3 * P * P + 63) // 64 * 64
    x = torch.from_numpy(img).to(cuda)
    out = ops.image_patches_pil(x, S, P, out_f32=True)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (B * (S // P) ** 2, kpad)
    px = _unpatchify(out.cpu(), B, S, P)
    mean, std = (torch.tensor(v, dtype=torch.float32).view(1, 3, 1, 1) for v in (O.CLIP_MEAN, O.CLIP_STD))
    back = torch.round((px.double() * std.double() + mean.double()) * 255).to(torch.int64).permute(0, 2, 3, 1)
    mismatches = int((back != torch.from_numpy(ref_u8).to(torch.int64)).sum())
    assert mismatches == 0, (name, mismatches, back.numel())
    want = (torch.from_numpy(ref_u8).permute(0, 3, 1, 2).float() / 255 - mean) / std           # torchvision's fp32 formula
    assert bool(((px - want).abs() <= 1e-6 * want.abs()).all()), float(((px - want).abs() / want.abs()).max())
    if kpad > K:
        assert torch.equal(out[:, K:].cpu(), torch.zeros(out.shape[0], kpad - K))
    bf = ops.image_patches_pil(x, S, P)
    assert bf.dtype == torch.bfloat16 and torch.equal(bf, out.to(torch.bfloat16))
    for _ in range(5):
        assert torch.equal(ops.image_patches_pil(x, S, P, out_f32=True), out)


def test_image_patches_pil_pads_and_feeds_encode_patches(cuda, pil_cases):
    """a patch size whose rows need zero padding (3 * 14^2 = 588 -> 640), consumed unchanged by the image tower"""
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd.image_encoder import CLIPVisionConfig, CLIPVisionModelWithProjection
    img, S, P, ref_u8 = pil_cases["512x512"]
    assert (3 * P * P) % 64 != 0
    m = CLIPVisionModelWithProjection(CLIPVisionConfig(**{**VISION_TINY, "image_size": S})).init_synthetic(2).to(cuda)
    x = torch.from_numpy(img).to(cuda)
    emb, _ = m.encode_patches(ops.image_patches_pil(x, S, P), img.shape[0])
    px = _unpatchify(ops.image_patches_pil(x, S, P, out_f32=True), img.shape[0], S, P)          # the same values as pixel_values
    assert torch.equal(emb, m(px.contiguous()).image_embeds)


def test_image_patches_pil_refuses_a_table_that_is_too_narrow(cuda):
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd._lib import AptpError
    x = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device=cuda)
    b, w = ops.pil_bicubic_table(64, 56)
    tb = (torch.from_numpy(b).to(cuda), torch.from_numpy(w[:, :5].copy()).to(cuda))
    with pytest.raises(AptpError, match="wider than"):
        ops.image_patches_pil(x, 56, 14, tables=(tb, tb))
    with pytest.raises(ValueError):
        ops.image_patches_pil(x, 56, 14, tables=((tb[0][:10], tb[1][:10]), tb))


# ---------------------------------------------------------------------------------------------------------------------
# aptp_eos_pool_ln
# ---------------------------------------------------------------------------------------------------------------------
EOS = 777


def _pool_case(B, L, C, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 700, (B, L), generator=g)
    if L >= 9:
        for b in range(B):
            if b % 2 == 0:                       # the largest id twice; the first EOS at 2 (and another one later)
                ids[b, L // 3], ids[b, 2 * L // 3] = 999, 999
                ids[b, 2], ids[b, L - 1] = EOS, EOS
            else:                                # the largest id once, in the middle; no EOS
                ids[b, L // 2] = 998
    x = torch.randn(B, L, C, generator=g) * 1.5 + 0.4
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    return ids, x, gamma, beta


@pytest.mark.parametrize("C", [128, 512])
@pytest.mark.parametrize("L", [1, 9, 77])
@pytest.mark.parametrize("B", [1, 5])
def test_eos_pool_ln(cuda, B, L, C):
    from diffusion_pruning_amd import ops
    ids, x, gamma, beta = _pool_case(B, L, C, B * 1000 + L * 10 + C)
    for dtype in (torch.float32, torch.bfloat16):
        xs = x.to(dtype)
        xd = xs.to(cuda)
        for mode, eos in (("argmax", 2), ("first_eos", EOS)):
            ref, at = O.pooled_ln(xs, ids, gamma, beta, 1e-5, eos)
            out, act, idx = ops.eos_pool_ln(ids.to(cuda), xd, gamma.to(cuda), beta.to(cuda), 1e-5, eos_mode=mode, eos_token_id=eos,
                                            return_index=True)
            torch.cuda.synchronize()
            assert idx.cpu().tolist() == at.tolist(), (mode, idx.cpu().tolist(), at.tolist())
            if mode == "argmax":
                assert at.tolist() == ids.argmax(-1).tolist()
            assert out.dtype == torch.float32 and act.dtype == dtype and tuple(out.shape) == tuple(act.shape) == (B, C)
            what = f"eos_pool_ln {mode} {'fp32' if dtype == torch.float32 else 'bf16'} B={B} L={L} C={C}"
            check(rel_l2(out, ref), LN_F32_TOL, what + " fp32 output")
            check(rel_l2(act, ref), LN_F32_TOL if dtype == torch.float32 else LN_BF16_TOL, what + " GEMM operand")
            assert torch.equal(act, out.to(dtype))
            if dtype == torch.float32:             # CLIPTextModel's way: LayerNorm of all B * L rows, then the gather
                allrows = ops.layernorm(xd, gamma.to(cuda), beta.to(cuda), 1e-5)[torch.arange(B), at.to(cuda)]
                check(rel_l2(out, allrows), LN_F32_TOL, what + " vs LayerNorm of all rows, gathered")
    if L >= 9 and B >= 2:
        assert ids[0].tolist().count(999) == 2 and ids[0].tolist().count(EOS) == 2 and EOS not in ids[1].tolist()


def test_eos_pool_ln_reads_a_strided_stream(cuda):
    from diffusion_pruning_amd import ops
    ids, x, gamma, beta = _pool_case(3, 9, 128, 4)
    wide = torch.zeros(3, 9, 256, dtype=torch.bfloat16)
    wide[..., 128:] = x.to(torch.bfloat16)
    ref, at = O.pooled_ln(wide[..., 128:], ids, gamma, beta, 1e-5)
    out, _, idx = ops.eos_pool_ln(ids.to(cuda), wide.to(cuda)[..., 128:], gamma.to(cuda), beta.to(cuda), return_index=True)
    assert idx.cpu().tolist() == at.tolist()
    check(rel_l2(out, ref), LN_F32_TOL, "eos_pool_ln on a column slice of a wider buffer")


# ---------------------------------------------------------------------------------------------------------------------
# aptp_paired_cosine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 512, 768])
@pytest.mark.parametrize("n", [1, 3, 257])
def test_paired_cosine(cuda, n, D):
    from diffusion_pruning_amd import ops
    g = torch.Generator().manual_seed(n * 1000 + D)
    a = torch.randn(n, D, generator=g) * 3.0
    b = 0.6 * a + torch.randn(n, D, generator=g) * (1.0 + torch.arange(n).float().view(n, 1) % 5)       # cosines from ~0.2 to ~0.9
    ref = O.cosines(a, b)
    cos, s = ops.paired_cosine(a.to(cuda), b.to(cuda))
    torch.cuda.synchronize()
    assert cos.dtype == torch.float32 and s.dtype == torch.float64 and tuple(cos.shape) == (n,) and s.dim() == 0
    check(float((cos.cpu().double() - ref).abs().max()), COS_TOL, f"paired_cosine n={n} D={D}, max |cos - fp64|")
    assert abs(float(s) - float(cos.cpu().double().sum())) <= 1e-12 * n            # the fp64 sum of the fp32 cosines it stored
    assert abs(float(s) - float(ref.sum())) <= COS_TOL * n
    for _ in range(5):
        c2, s2 = ops.paired_cosine(a.to(cuda), b.to(cuda))
        assert torch.equal(c2, cos) and torch.equal(s2, s)
    total = torch.full((), 2.5, dtype=torch.float64, device=cuda)
    _, t = ops.paired_cosine(a.to(cuda), b.to(cuda), total=total)
    assert t is total and float(total) == 2.5 + float(s)


# ---------------------------------------------------------------------------------------------------------------------
# the text tower with its projection
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def towers():
    """(config name -> (module, its state dict, ids [2, 77], the fp64 oracle's text_embeds and last_hidden_state))"""
    from diffusion_pruning_amd.clip_model import CLIPTextModelWithProjection, CLIPTextProjectionConfig
    out = {}
    for name, cfg in (("tiny", CLIPTextProjectionConfig(**TEXT_TINY)), ("vit_b_32", CLIPTextProjectionConfig())):
        m = CLIPTextModelWithProjection(cfg).init_synthetic(0)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        ids = torch.randint(3, cfg.vocab_size, (2, 77), generator=torch.Generator().manual_seed(11))
        emb, h = O.clip_text_embeds(sd, ids, heads=cfg.num_attention_heads, layers=cfg.num_hidden_layers, hidden_act=cfg.hidden_act)
        out[name] = (m, sd, ids, emb, h)
    return out


@pytest.mark.parametrize("name", ["tiny", "vit_b_32"])
def test_text_tower_bf16_against_oracle(cuda, towers, name):
    m, _, ids, emb, h = towers[name]
    m.to(cuda)
    out = m(ids)
    cfg = m.config
    assert out.text_embeds.dtype == torch.float32 and tuple(out.text_embeds.shape) == (2, cfg.projection_dim)
    assert out.last_hidden_state.dtype == torch.float32 and tuple(out.last_hidden_state.shape) == (2, 77, cfg.hidden_size)
    check(rel_l2(out.text_embeds, emb), ENC_BF16_TOL, f"CLIP text tower {name} bf16 text_embeds")
    check(rel_l2(out.last_hidden_state, h), ENC_BF16_TOL, f"CLIP text tower {name} bf16 last_hidden_state")
    assert torch.equal(m.embed_ids(ids.to(cuda)), out.text_embeds)
    t = m(ids, return_dict=False)
    assert isinstance(t, tuple) and torch.equal(t[0], out[0]) and torch.equal(t[1], out[1])


@pytest.mark.parametrize("name", ["tiny", "vit_b_32"])
def test_text_tower_fp32_parity_path(cuda, towers, monkeypatch, name):
    from diffusion_pruning_amd import ops
    m, _, ids, emb, h = towers[name]
    monkeypatch.setattr(ops, "ACT_DTYPE", torch.float32)
    m.to(cuda)
    out = m(ids)
    check(rel_l2(out.text_embeds, emb), ENC_F32_TOL, f"CLIP text tower {name} fp32 parity text_embeds")
    check(rel_l2(out.last_hidden_state, h), ENC_F32_TOL, f"CLIP text tower {name} fp32 parity last_hidden_state")
    m.invalidate()


@pytest.mark.parametrize("name", ["tiny", "vit_b_32"])
def test_text_tower_graph_replay_is_bit_equal_to_eager(cuda, towers, name):
    m, _, ids, _, _ = towers[name]
    m.to(cuda)
    ids = ids.to(cuda)
    eager = m(ids)
    e_emb, e_h = eager.text_embeds.clone(), eager.last_hidden_state.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(ids)                            # warm-up on the capture stream (packs, workspaces)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(ids)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.text_embeds, e_emb) and torch.equal(out.last_hidden_state, e_h)


@pytest.mark.parametrize("eos", [2, 200])
def test_text_tower_pools_like_transformers_on_the_fixture(cuda, monkeypatch, eos):
    """the golden ids: the largest id in the middle, the largest id twice, and (eos 200) a row without the EOS id"""
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd.clip_model import CLIPTextModelWithProjection, CLIPTextProjectionConfig
    z, _, params = model_golden()
    m = CLIPTextModelWithProjection(CLIPTextProjectionConfig(**{**TEXT_TINY, "eos_token_id": eos}))
    m.load_text_state_dict({k: v.float() for k, v in params.items()}).to(cuda)
    assert m.eos_mode == ("argmax" if eos == 2 else "first_eos")
    tag = "" if eos == 2 else "_eos200"
    for L in (1, 9, 77):
        ids = torch.from_numpy(z[f"ids_L{L}"])
        ref = torch.from_numpy(z[f"text_embeds{tag}_L{L}"])
        monkeypatch.setattr(ops, "ACT_DTYPE", torch.bfloat16)
        check(rel_l2(m.embed_ids(ids), ref), ENC_BF16_TOL, f"CLIP text tower fixture eos={eos} L={L} bf16 text_embeds")
        monkeypatch.setattr(ops, "ACT_DTYPE", torch.float32)
        check(rel_l2(m.embed_ids(ids), ref), ENC_F32_TOL, f"CLIP text tower fixture eos={eos} L={L} fp32 text_embeds")
    m.invalidate()


# ---------------------------------------------------------------------------------------------------------------------
# the whole score
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def score_case():
    """the tiny CLIPModel of the fixtures, 24 seeded uint8 images of 40 x 56, 24 id rows, and the fp64 oracle's score"""
    from diffusion_pruning_amd.clip_model import CLIPModel, CLIPTextModelWithProjection, CLIPTextProjectionConfig
    from diffusion_pruning_amd.image_encoder import CLIPVisionConfig, CLIPVisionModelWithProjection
    z, _, params = model_golden()
    f32 = {k: v.float() for k, v in params.items()}
    model = CLIPModel(CLIPTextModelWithProjection(CLIPTextProjectionConfig(**TEXT_TINY)).load_text_state_dict(f32),
                      CLIPVisionModelWithProjection(CLIPVisionConfig(**VISION_TINY)).load_vision_state_dict(f32), float(z["logit_scale"]))
    rs = np.random.RandomState(24)
    images = rs.randint(0, 256, (24, 40, 56, 3)).astype(np.uint8)
    ids = torch.from_numpy(rs.randint(3, 256, (24, 16)).astype(np.int64))
    scale = float(np.exp(float(z["logit_scale"])))
    text = dict(heads=2, layers=2, hidden_act="quick_gelu", eos_token_id=2)
    vision = dict(heads=2, layers=2, patch=14, image_size=56, hidden_act="quick_gelu")
    score, cos = O.clip_score(params, images, ids, text=text, vision=vision, logit_scale=scale)
    feats, _ = O.clip_text_embeds(params, ids, 2, 2, "quick_gelu", 2)
    return model, images, ids, scale, score, cos, feats


def test_clip_score_end_to_end_fp32(cuda, score_case):
    from diffusion_pruning_amd import metrics
    model, images, ids, scale, ref, ref_cos, feats = score_case
    sm = metrics.ClipScoreModel(model.to(cuda), precision="fp32")
    assert abs(sm.logit_scale - scale) <= 1e-9 * scale
    got, cos = sm.score(images, ids, batch_size=10, return_cosines=True)           # chunks of 10, 10 and 4 pairs
    assert got.dtype == torch.float64 and tuple(cos.shape) == (24,)
    print(f"CLIP score fp32: {float(got):.6f} vs fp64 oracle {ref:.6f}, relative deviation {abs(float(got) - ref) / abs(ref):.3e}; "
          f"max |cos - oracle| {float((cos.cpu().double() - ref_cos).abs().max()):.3e}")
    check(abs(float(got) - ref) / abs(ref), SCORE_F32_RTOL, "CLIP score fp32 path, relative deviation from the fp64 oracle")
    check(float((cos.cpu().double() - ref_cos).abs().max()), SCORE_F32_RTOL, "CLIP score fp32 path, max |cos - oracle|")
    one = sm.score(images, ids, batch_size=64)
    assert abs(float(one) - float(got)) <= 1e-12 * abs(float(got)) + 1e-9           # the chunking only reorders an fp64 sum
    pre = sm.score(images, text_features=feats.float().numpy(), batch_size=10)     # the .npy rows of clip_features, any norm
    check(abs(float(pre) - ref) / abs(ref), SCORE_F32_RTOL, "CLIP score fp32 path with precomputed text features")
    tf, imf = sm.text_features(ids, batch_size=7), sm.image_features(images, batch_size=7)
    assert torch.allclose(tf.norm(dim=1), torch.ones(24, device=cuda), atol=1e-6)
    assert torch.allclose(imf.norm(dim=1), torch.ones(24, device=cuda), atol=1e-6)
    assert abs(float(metrics.clip_score(imf, tf, logit_scale=scale)) - float(got)) <= 1e-4 * abs(float(got))
    model.text_model.invalidate()
    model.vision_model.invalidate()


def test_clip_score_end_to_end_bf16(cuda, score_case):
    from diffusion_pruning_amd import metrics
    model, images, ids, scale, ref, ref_cos, _ = score_case
    sm = metrics.ClipScoreModel(model.to(cuda))
    assert sm.precision == "bf16"
    got, cos = sm.score(images, ids, batch_size=10, return_cosines=True)
    print(f"CLIP score bf16: {float(got):.6f} vs fp64 oracle {ref:.6f}, deviation {abs(float(got) - ref):.3e} "
          f"(bound {scale * SCORE_BF16_COS_TOL:.3e}); max |cos - oracle| {float((cos.cpu().double() - ref_cos).abs().max()):.3e}")
    check(abs(float(got) - ref), scale * SCORE_BF16_COS_TOL, "CLIP score bf16 path, |score - fp64 oracle| (logit_scale x 4e-2)")
    check(float((cos.cpu().double() - ref_cos).abs().max()), SCORE_BF16_COS_TOL, "CLIP score bf16 path, max |cos - oracle|")
    again, cos2 = sm.score(images, ids, batch_size=10, return_cosines=True)
    assert torch.equal(again, got) and torch.equal(cos2, cos)
