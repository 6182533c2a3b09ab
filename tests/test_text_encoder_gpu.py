"""The HIP CLIP text encoder on the GPU: the causal attention kernel against fp64 causal SDPA, the GELU epilogue on every
tile the linear path accepts (and split-K), the token embedding bit for bit, the whole SD-2.1-size encoder against the CPU
oracle (tests/clip_text_oracle.py) in bf16 and on the fp32 parity path, causality, graph replay, determinism, and the
pipeline's prompt_ids path.  Margins go through tests.margins.check, which keeps the measured values."""
import pytest
import torch
import torch.nn.functional as F

from tests import tiles
from tests.clip_text_oracle import clip_text_forward
from tests.helpers import rel_l2
from tests.margins import check

pytestmark = pytest.mark.gpu

ATTN_BF16_TOL = 4e-3
ATTN_F32_TOL = 1e-5
LIN_BF16_TOL = 4e-3
LIN_F32_TOL = 1e-5
ENC_BF16_TOL = 2e-2
ENC_F32_TOL = 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# aptp_attention_causal
# ---------------------------------------------------------------------------------------------------------------------
def _causal_ref(q, k, v, heads):
    B, L, _ = q.shape
    sh = lambda t: t.double().cpu().reshape(B, L, heads, 64).transpose(1, 2)      # noqa: E731
    o = F.scaled_dot_product_attention(sh(q), sh(k), sh(v), is_causal=True, scale=0.125)
    return o.transpose(1, 2).reshape(B, L, heads * 64)


@pytest.mark.parametrize("L", [1, 7, 64, 77, 128])
@pytest.mark.parametrize("heads", [1, 16])
@pytest.mark.parametrize("B", [1, 2, 64])
def test_attention_causal_bf16(cuda, B, heads, L):
    from diffusion_pruning_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + heads * 10 + L)
    C = heads * 64
    qkv = (torch.randn(B, L, 3 * C, generator=g) * 1.5).to(torch.bfloat16).to(cuda)    # the fused q|k|v layout, read in place
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    o = ops.attention_causal(q, k, v, heads)
    torch.cuda.synchronize()
    check(rel_l2(o, _causal_ref(q, k, v, heads)), ATTN_BF16_TOL, f"attention_causal bf16 B={B} heads={heads} L={L}")


@pytest.mark.parametrize("L", [1, 7, 64, 77, 128])
@pytest.mark.parametrize("heads", [1, 16])
def test_attention_causal_fp32_parity(cuda, heads, L):
    from diffusion_pruning_amd import ops
    g = torch.Generator().manual_seed(heads * 10 + L)
    C = heads * 64
    qkv = (torch.randn(2, L, 3 * C, generator=g) * 1.5).to(cuda)
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    o = ops.attention_causal(q, k, v, heads)
    torch.cuda.synchronize()
    check(rel_l2(o, _causal_ref(q, k, v, heads)), ATTN_F32_TOL, f"attention_causal fp32 heads={heads} L={L}")


def test_attention_causal_separate_strided_tensors(cuda):
    """q, k, v from three different buffers with different row strides, and the output into a column slice"""
    from diffusion_pruning_amd import ops
    g = torch.Generator().manual_seed(5)
    B, L, heads = 3, 77, 2
    C = heads * 64
    q = torch.randn(B, L, C + 64, generator=g).to(torch.bfloat16).to(cuda)[..., 64:]
    k = torch.randn(B, L, 2 * C, generator=g).to(torch.bfloat16).to(cuda)[..., :C]
    v = torch.randn(B, L, C, generator=g).to(torch.bfloat16).to(cuda)
    big = torch.zeros(B, L, 2 * C, dtype=torch.bfloat16, device=cuda)
    ops.attention_causal(q, k, v, heads, out=big[..., C:])
    torch.cuda.synchronize()
    assert torch.equal(big[..., :C], torch.zeros_like(big[..., :C]))
    check(rel_l2(big[..., C:], _causal_ref(q, k, v, heads)), ATTN_BF16_TOL, "attention_causal strided views")


def test_attention_causal_checks_its_output(cuda):
    from diffusion_pruning_amd import ops
    qkv = torch.zeros(2, 7, 3 * 128, dtype=torch.bfloat16, device=cuda)
    q, k, v = qkv[..., :128], qkv[..., 128:256], qkv[..., 256:]
    for bad in (torch.empty(2, 7, 64, dtype=torch.bfloat16, device=cuda), torch.empty(2, 6, 128, dtype=torch.bfloat16, device=cuda),
                torch.empty(2, 7, 128, dtype=torch.float32, device=cuda), torch.empty(2, 7, 128, dtype=torch.bfloat16),
                torch.empty(2, 128, 7, dtype=torch.bfloat16, device=cuda).transpose(1, 2)):
        with pytest.raises(ValueError):
            ops.attention_causal(q, k, v, 2, out=bad)
    with pytest.raises(ValueError):
        ops.attention_causal(q, k.cpu(), v, 2)


def test_attention_causal_refuses_long_sequences(cuda):
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd._lib import AptpError
    x = torch.zeros(1, 129, 3 * 64, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(AptpError):
        ops.attention_causal(x[..., :64], x[..., 64:128], x[..., 128:], 1)


# ---------------------------------------------------------------------------------------------------------------------
# GELU epilogue (APTP_ACT_GELU)
# ---------------------------------------------------------------------------------------------------------------------
HALO_TILES = tiles.HALO


def _gelu_case(cuda, dtype, seed, M=154, K=256, N=512):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, M // 2, K, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) * 0.3
    res = torch.randn(2, M // 2, N, generator=g)
    if dtype == torch.bfloat16:
        x, w, res = x.to(torch.bfloat16).float(), w.to(torch.bfloat16).float(), res.to(torch.bfloat16).float()
    ref = F.gelu(x.double() @ w.double().t() + b.double()) + res.double()
    return x.to(dtype).to(cuda), w, b, res.to(dtype).to(cuda), ref


@pytest.mark.parametrize("general", [False, True])
def test_gelu_linear_every_tile_bf16(cuda, monkeypatch, general):
    """every tile: the lean linear kernel where it takes the launch, and (general=True) the general register-staged / LDS-DMA /
    stream-K kernels; the halo tiles refuse a linear layer"""
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd._lib import AptpError
    monkeypatch.setattr(ops, "EPILOGUE", 2 if general else 0)
    x, w, b, res, ref = _gelu_case(cuda, torch.bfloat16, 11)
    pw = ops.pack_weight(w, b, device=cuda)
    for tile in tiles.ALL:
        if tile in HALO_TILES:
            with pytest.raises(AptpError):
                ops.linear(x, pw, act=ops.ACT_GELU, residual=res, tile=tile)
            continue
        y = ops.linear(x, pw, act=ops.ACT_GELU, residual=res, tile=tile)
        torch.cuda.synchronize()
        check(rel_l2(y, ref), LIN_BF16_TOL, f"GELU linear bf16 tile {tile}{' general' if general else ''}")
    y = ops.linear(x, pw, act=ops.ACT_GELU, residual=res)
    check(rel_l2(y, ref), LIN_BF16_TOL, "GELU linear bf16 auto tile")


@pytest.mark.parametrize("split_k", [2, 4, 8])
@pytest.mark.parametrize("in_kernel", [True, False])
def test_gelu_linear_split_k_bf16(cuda, monkeypatch, split_k, in_kernel):
    """GELU after the K-slices are summed, on every tile that takes a linear layer: by the last-arriving workgroup (tile
    counters; the stream-K tiles always combine this way) or by the reduce launch"""
    from diffusion_pruning_amd import ops
    monkeypatch.setattr(ops, "SPLITK_IN_KERNEL", in_kernel)
    x, w, b, res, ref = _gelu_case(cuda, torch.bfloat16, 12, K=1024)
    pw = ops.pack_weight(w, b, device=cuda)
    for tile in (t for t in tiles.ALL if t not in HALO_TILES):
        y = ops.linear(x, pw, act=ops.ACT_GELU, residual=res, tile=tile, split_k=split_k)
        torch.cuda.synchronize()
        check(rel_l2(y, ref), LIN_BF16_TOL, f"GELU linear bf16 tile {tile} split_k {split_k} in_kernel {in_kernel}")


@pytest.mark.parametrize("split_k", [1, 2, 8])
def test_gelu_linear_fp32_parity(cuda, monkeypatch, split_k):
    from diffusion_pruning_amd import ops
    monkeypatch.setattr(ops, "ACT_DTYPE", torch.float32)
    x, w, b, res, ref = _gelu_case(cuda, torch.float32, 13, K=512)
    pw = ops.pack_weight(w, b, device=cuda)
    for tile in (0,) + tiles.REG:
        y = ops.linear(x, pw, act=ops.ACT_GELU, residual=res, tile=tile, split_k=split_k)
        torch.cuda.synchronize()
        check(rel_l2(y, ref), LIN_F32_TOL, f"GELU linear fp32 tile {tile} split_k {split_k}")
    for tile in (t for t in tiles.ALL if t not in tiles.REG):     # the parity path runs on the register-staged tiles only
        with pytest.raises(ValueError):
            ops.linear(x, pw, act=ops.ACT_GELU, residual=res, tile=tile, split_k=split_k)


def test_gelu_3x3_conv_leaves_the_lean_kernel(cuda):
    """conv_lean.hip has no GELU: a 3x3 launch with ACT_GELU takes the general kernel of the same tile and applies it"""
    from diffusion_pruning_amd import ops
    g = torch.Generator().manual_seed(14)
    x = torch.randn(2, 16, 16, 64, generator=g).to(torch.bfloat16)
    w = (torch.randn(64, 64, 3, 3, generator=g) * (64 * 9) ** -0.5).to(torch.bfloat16).float()
    b = torch.randn(64, generator=g) * 0.3
    y = ops.conv_gemm(x.to(cuda), ops.pack_weight(w, b, device=cuda), act=ops.ACT_GELU, tile=18)
    torch.cuda.synchronize()
    ref = F.gelu(F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1)
    check(rel_l2(y, ref), LIN_BF16_TOL, "GELU 3x3 conv bf16 tile 18")


def test_conv_gemm_refuses_an_unknown_act(cuda):
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd._lib import AptpError
    x, w, b, res, _ = _gelu_case(cuda, torch.bfloat16, 15)
    pw = ops.pack_weight(w, b, device=cuda)
    for act in (4, 99, -1):
        with pytest.raises(AptpError):
            ops.linear(x, pw, act=act)


# ---------------------------------------------------------------------------------------------------------------------
# token_embed
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(1, 1), (2, 77), (64, 77), (3, 5)])
def test_token_embed_is_bit_exact(cuda, B, L):
    from diffusion_pruning_amd import ops
    g = torch.Generator().manual_seed(B + L)
    tok = torch.randn(1000, 1024, generator=g)
    pos = torch.randn(77, 1024, generator=g)
    ids = torch.randint(0, 1000, (B, L), generator=g)
    ref = tok[ids] + pos[:L]
    y = ops.token_embed(ids.to(cuda), tok.to(cuda), pos.to(cuda))
    y32 = ops.token_embed(ids.to(cuda), tok.to(cuda), pos.to(cuda), out_f32=True)
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and torch.equal(y.cpu(), ref.to(torch.bfloat16))
    assert torch.equal(y32.cpu(), ref)


def test_token_embed_out_of_range_id_gives_a_nan_row(cuda):
    from diffusion_pruning_amd import ops
    g = torch.Generator().manual_seed(9)
    tok = torch.randn(1000, 128, generator=g)
    pos = torch.randn(77, 128, generator=g)
    ids = torch.randint(0, 1000, (2, 7), generator=g)
    ids[1, 3] = 1000
    y = ops.token_embed(ids.to(cuda), tok.to(cuda), pos.to(cuda)).float().cpu()
    torch.cuda.synchronize()
    assert torch.isnan(y[1, 3]).all()
    ok = torch.ones(2, 7, dtype=torch.bool)
    ok[1, 3] = False
    assert torch.equal(y[ok], (tok[ids.clamp(max=999)] + pos[:7]).to(torch.bfloat16).float()[ok])


# ---------------------------------------------------------------------------------------------------------------------
# the whole encoder
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd21():
    from diffusion_pruning_amd.text_encoder import CLIPTextModel
    m = CLIPTextModel().init_synthetic(0)
    return m, {k: v.clone() for k, v in m.state_dict().items()}


def _ids(B, L, seed):
    return torch.randint(3, 49408, (B, L), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("B,L", [(2, 77), (64, 77), (1, 1)])
def test_encoder_bf16_against_oracle(cuda, sd21, B, L):
    m, sd = sd21
    m.to(cuda)
    ids = torch.tensor([[100]]) if (B, L) == (1, 1) else _ids(B, L, B)
    out = m(ids)                                  # CPU ids, as trainer.py:1443 passes them
    h, pooled = clip_text_forward(sd, ids, heads=16, layers=23, dtype=torch.float32)
    assert out[0].dtype == torch.float32 and out[0].shape == (B, L, 1024) and out.pooler_output.shape == (B, 1024)
    check(rel_l2(out.last_hidden_state, h), ENC_BF16_TOL, f"CLIP text encoder bf16 B={B} L={L}")
    check(rel_l2(out.pooler_output, pooled), ENC_BF16_TOL, f"CLIP text encoder bf16 pooler B={B} L={L}")
    t = m(ids.to(cuda), return_dict=False)
    assert isinstance(t, tuple) and torch.equal(t[0], out[0]) and torch.equal(t[1], out[1])


def test_encoder_folded_and_separate_layernorm_agree(cuda, sd21, monkeypatch):
    from diffusion_pruning_amd import text_encoder as T
    m, sd = sd21
    m.to(cuda)
    for B in (2, 16):
        ids = _ids(B, 77, 21)
        monkeypatch.setattr(T, "FOLD_LN_MAX_ROWS", 1 << 30)
        folded = m(ids)[0]
        monkeypatch.setattr(T, "FOLD_LN_MAX_ROWS", 0)
        sep = m(ids)[0]
        h, _ = clip_text_forward(sd, ids, heads=16, layers=23, dtype=torch.float32)
        check(rel_l2(folded, h), ENC_BF16_TOL, f"CLIP text encoder bf16 B={B}, folded LayerNorms")
        check(rel_l2(sep, h), ENC_BF16_TOL, f"CLIP text encoder bf16 B={B}, stand-alone LayerNorms")
        check(rel_l2(folded, sep), ENC_BF16_TOL, f"CLIP text encoder bf16 B={B}, folded vs stand-alone LayerNorms")


def test_encoder_fp32_parity_path(cuda, sd21, monkeypatch):
    from diffusion_pruning_amd import ops
    m, sd = sd21
    monkeypatch.setattr(ops, "ACT_DTYPE", torch.float32)
    m.to(cuda)
    ids = _ids(2, 77, 3)
    out = m(ids)
    h, pooled = clip_text_forward(sd, ids, heads=16, layers=23)
    check(rel_l2(out.last_hidden_state, h), ENC_F32_TOL, "CLIP text encoder fp32 parity B=2 L=77")
    check(rel_l2(out.pooler_output, pooled), ENC_F32_TOL, "CLIP text encoder fp32 parity pooler")
    m.invalidate()


def test_encoder_rejects_out_of_range_ids_and_lengths(cuda, sd21):
    m, _ = sd21
    m.to(cuda)
    with pytest.raises(ValueError):
        m(torch.tensor([[0, 49408]]))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 78, dtype=torch.long))


def test_encoder_is_causal(cuda, sd21):
    m, _ = sd21
    m.to(cuda)
    ids = _ids(2, 77, 4)
    base = m(ids)[0]
    for j in (1, 40, 76):
        other = ids.clone()
        other[:, j:] = _ids(2, 77 - j, 100 + j)
        y = m(other)[0]
        assert torch.equal(y[:, :j], base[:, :j]), j
        assert not torch.equal(y[:, j:], base[:, j:]), j


def _capture(m, ids):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(ids)                            # warm-up on the capture stream (packs, workspaces)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(ids)[0]
    return graph, out


def test_graph_of_one_layernorm_form_survives_a_capture_of_the_other(cuda, sd21, monkeypatch):
    """what tools/bench_text_encoder.py does: a graph per LayerNorm form of one model; flipping the form and capturing again
    (torch.cuda.graph empties the allocator cache) must leave the first graph's packed weights in place"""
    from diffusion_pruning_amd import text_encoder as T
    m, _ = sd21
    m.to(cuda)
    ids = _ids(2, 77, 6).to(cuda)
    outs = {}
    for fold in (True, False):
        monkeypatch.setattr(T, "FOLD_LN_MAX_ROWS", (1 << 30) if fold else 0)
        eager = m(ids)[0].clone()
        graph, out = _capture(m, ids)
        outs[fold] = (eager, graph, out)
    for fold in (True, False, True):
        eager, graph, out = outs[fold]
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), fold


@pytest.mark.parametrize("B", [1, 2, 16, 64])
@pytest.mark.parametrize("form", ["default", "folded", "separate"])
def test_layernorm_form_and_launch_count(cuda, sd21, monkeypatch, B, form):
    """folded: every producer emits row statistics (split-K launches combine in-kernel), so an encode has two stand-alone
    LayerNorm launches -- layer 0's LN1 and final_layer_norm; separate: 2 x 23 + 1.  By default encodes of up to
    FOLD_LN_MAX_ROWS tokens fold (the pipeline's 2 x 77), larger ones (16 x 77, the training batch 64 x 77) do not"""
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd import text_encoder as T
    if form != "default":
        monkeypatch.setattr(T, "FOLD_LN_MAX_ROWS", (1 << 30) if form == "folded" else 0)
    m, _ = sd21
    m.to(cuda)
    ids = _ids(B, 77, 7).to(cuda)
    m(ids)
    calls = []
    real = ops.layernorm
    monkeypatch.setattr(ops, "layernorm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    m(ids)
    fold = form == "folded" or (form == "default" and B * 77 <= T.FOLD_LN_MAX_ROWS)
    assert len(calls) == (2 if fold else 47)


def test_encoder_graph_replay_and_determinism(cuda, sd21):
    m, _ = sd21
    m.to(cuda)
    ids = _ids(2, 77, 5).to(cuda)
    eager = m(ids)[0].clone()
    assert torch.equal(m(ids)[0], eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(ids)                            # warm-up on the capture stream (packs, workspaces)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(ids)[0]
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("use_graph", [False, True])
def test_pipeline_encodes_prompt_ids(cuda, use_graph):
    from diffusion_pruning_amd.pipeline import PruningDenoiseLoop
    from diffusion_pruning_amd.text_encoder import CLIPTextConfig, CLIPTextModel
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    from oracle import unet_oracle as O
    cfg = O.TINY
    unet = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                     cross_attention_dim=cfg.cross_attention_dim).init_synthetic(seed=0).to(cuda)
    te = CLIPTextModel(CLIPTextConfig(vocab_size=1000, hidden_size=cfg.cross_attention_dim, intermediate_size=256,
                                      num_hidden_layers=2, num_attention_heads=1)).init_synthetic(1).to(cuda)
    loop = PruningDenoiseLoop(unet, text_encoder=te)
    g = torch.Generator().manual_seed(0)
    B = 2
    lat = torch.randn(B, 4, 16, 16, generator=g).to(cuda)
    ids = torch.randint(3, 1000, (B, 77), generator=g).to(cuda)
    neg = torch.randint(3, 1000, (B, 77), generator=g).to(cuda)
    e = te(torch.cat([neg, ids]))[0]
    ref = loop(e[B:], lat, num_inference_steps=3, negative_prompt_embeds=e[:B], use_graph=use_graph).latents.clone()
    got = loop(prompt_ids=ids, negative_prompt_ids=neg, latents=lat, num_inference_steps=3, use_graph=use_graph).latents
    assert torch.equal(got, ref)
    single = loop(prompt_ids=ids, latents=lat, num_inference_steps=3, use_graph=use_graph).latents
    assert torch.equal(single, loop(te(ids)[0], lat, num_inference_steps=3, use_graph=use_graph).latents)
