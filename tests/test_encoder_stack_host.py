"""Host tests of what the forward-only encoders share (modules.py): the launch sequence of each encoder, pinned call by call
with the ``ops`` entry points replaced by recording fakes; ``init_synthetic`` against a restatement of the per-model loops it
replaced; the plan cache's one home; ``invalidate()`` / ``.to()`` on every model that keeps plans.

A fake records (op, operands, keywords) and returns an empty tensor of the shape and dtype the kernel would return, so the models'
own code -- plans, packs (``ops.pack_weight`` runs for real on the CPU), views, keyword choices -- runs unchanged.  A record is one
line: tensors as ``shape/strides:dtype@producer`` (producer: the index of the call that returned the storage, ``in`` for an
argument of the encode), anything the plan holds by its path in the plan.  The expected lines were recorded from the code before
the shared module existed and are written out below, so they pin the sequence, not the code under test.
"""
import pytest
import torch

from diffusion_pruning_amd import modules as M
from diffusion_pruning_amd import ops, prompt_encoder, text_encoder, unet
from diffusion_pruning_amd.clip_model import CLIPTextModelWithProjection, CLIPTextProjectionConfig
from diffusion_pruning_amd.image_encoder import CLIPVisionModelWithProjection
from diffusion_pruning_amd.prompt_encoder import MPNetModel
from diffusion_pruning_amd.text_encoder import CLIPTextModel
from diffusion_pruning_amd.vae import AutoencoderKL, VAEConfig

CPU = torch.device("cpu")
_DT = {torch.bfloat16: "bf16", torch.float32: "f32", torch.int64: "i64"}


class Recorder:
    """the fakes' log; every tensor a fake returns stays alive here, so a storage address names its producer"""

    def __init__(self):
        self.calls, self.keep, self.src = [], [], {}

    def out(self, *shape, dtype):
        t = torch.empty(*shape, dtype=dtype)
        self.keep.append(t)
        self.src[t.untyped_storage().data_ptr()] = len(self.calls) - 1          # (the call was logged before it returns)
        return t

    def call(self, op, **args):
        self.calls.append((op, args))

    def lines(self, plan):
        names = {}

        def walk(v, path):
            if isinstance(v, dict):
                for k, x in v.items():
                    walk(x, f"{path}.{k}" if path else str(k))
            elif isinstance(v, (list, tuple)):
                for i, x in enumerate(v):
                    walk(x, f"{path}.{i}" if isinstance(v, list) else f"{path}[{i}]")
            elif isinstance(v, (torch.Tensor, ops.PackedWeight)):
                names[id(v)] = path
        walk(plan, "")

        def show(v):
            if id(v) in names:
                return names[id(v)]
            if isinstance(v, torch.Tensor):
                dims = "x".join(map(str, v.shape))
                strides = ",".join(map(str, v.stride()))
                return f"{dims}/{strides}:{_DT[v.dtype]}@{self.src.get(v.untyped_storage().data_ptr(), 'in')}"
            if isinstance(v, tuple):
                return "(" + ", ".join(show(x) for x in v) + ")"
            return repr(v)
        return [f"{op}(" + ", ".join(f"{k}={show(v)}" for k, v in args.items()) + ")" for op, args in self.calls]


@pytest.fixture
def rec(monkeypatch):
    """``ops`` with the entry points the encoders call replaced by recording fakes; no stream is capturing"""
    R = Recorder()
    act = lambda f32: torch.float32 if f32 else torch.bfloat16      # noqa: E731

    def token_embed(ids, tok, pos, out_f32=False):
        R.call("token_embed", ids=ids, tok=tok, pos=pos, out_f32=out_f32)
        return R.out(*ids.shape, tok.shape[1], dtype=act(out_f32))

    def embed_ln(ids, word, pos, gamma, beta, eps=1e-5, pad_id=1, out_f32=False):
        R.call("embed_ln", ids=ids, word=word, pos=pos, gamma=gamma, beta=beta, eps=eps, pad_id=pad_id, out_f32=out_f32)
        return R.out(*ids.shape, word.shape[1], dtype=act(out_f32))

    def image_patches(x, size, patch, *, resize=True, out_f32=False):
        R.call("image_patches", x=x, size=size, patch=patch, resize=resize, out_f32=out_f32)
        return R.out(x.shape[0] * (size // patch) ** 2, ops.round_up(3 * patch * patch, 64), dtype=act(out_f32))

    def vit_embed_ln(patches, B, cls, pos, gamma, beta, eps=1e-5, out_f32=False):
        R.call("vit_embed_ln", patches=patches, B=B, cls=cls, pos=pos, gamma=gamma, beta=beta, eps=eps, out_f32=out_f32)
        return R.out(B, pos.shape[0], cls.shape[0], dtype=act(out_f32))

    def layernorm(x, gamma, beta, eps=1e-5):
        R.call("layernorm", x=x, gamma=gamma, beta=beta, eps=eps)
        return R.out(*x.shape, dtype=x.dtype)

    def linear(x, pw, **kw):
        R.call("linear", x=x, pw=pw, **kw)
        y = R.out(x.shape[0], x.shape[1], pw.N, dtype=torch.float32 if kw.get("out_f32") else x.dtype)
        if "rowstats" in kw:          # ops.linear: a pair whenever the keyword is given, (y, None) when it is False
            return (y, R.out(x.shape[0] * x.shape[1], 2, dtype=torch.float32) if kw["rowstats"] and R.stats else None)
        return y

    def attn(op):
        def f(q, k, v, heads, *more):
            R.call(op, q=q, k=k, v=v, heads=heads, **dict(zip(("relbias", "key_mask"), more)))
            return R.out(q.shape[0], q.shape[1], heads * 64, dtype=q.dtype)
        return f

    def eos_pool_ln(ids, x, gamma, beta, eps=1e-5, *, eos_mode="argmax", eos_token_id=2):
        R.call("eos_pool_ln", ids=ids, x=x, gamma=gamma, beta=beta, eps=eps, eos_mode=eos_mode, eos_token_id=eos_token_id)
        return R.out(x.shape[0], x.shape[2], dtype=torch.float32), R.out(x.shape[0], x.shape[2], dtype=x.dtype)

    def masked_mean(x, mask=None):
        R.call("masked_mean", x=x, mask=mask)
        return R.out(x.shape[0], x.shape[2], dtype=torch.float32)

    R.stats = True                    # False: a producer that could not emit row statistics
    for name, f in dict(token_embed=token_embed, embed_ln=embed_ln, image_patches=image_patches, vit_embed_ln=vit_embed_ln,
                        layernorm=layernorm, linear=linear, attention=attn("attention"), attention_causal=attn("attention_causal"),
                        attention_bias=attn("attention_bias"), eos_pool_ln=eos_pool_ln, masked_mean=masked_mean).items():
        monkeypatch.setattr(ops, name, f)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return R


TEXT = dict(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
            max_position_embeddings=77)
MPNET = dict(vocab_size=64, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
             max_position_embeddings=40)
VISION = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, patch_size=8, image_size=32,
              projection_dim=64)


def _ids(B, L):
    return (torch.arange(B * L, dtype=torch.int64).reshape(B, L) * 7 + 3) % 64


def _text_tower():
    return CLIPTextModel(**TEXT).init_synthetic(0)


def _text_projection():
    return CLIPTextModelWithProjection(CLIPTextProjectionConfig(**TEXT, hidden_act="quick_gelu", projection_dim=64)).init_synthetic(0)


def _vision():
    return CLIPVisionModelWithProjection(**VISION).init_synthetic(0)


def _mpnet():
    return MPNetModel(**MPNET).init_synthetic(0)


def _layer_folded(i, x, act):
    """layer i >= 1 of the folded text stack; x: the index of the fc2 call that produced its input (statistics included)"""
    return [f"linear(x=2x9x128/1152,128,1:bf16@{x}, pw=layers.{i}.qkv_ln, ln=(18x2/2,1:f32@{x}, 1e-05))",
            f"attention_causal(q=2x9x128/3456,384,1:bf16@{x + 1}, k=2x9x128/3456,384,1:bf16@{x + 1}, v=2x9x128/3456,384,1:bf16@{x + 1}, heads=2)",
            f"linear(x=2x9x128/1152,128,1:bf16@{x + 2}, pw=layers.{i}.out, residual=2x9x128/1152,128,1:bf16@{x}, rowstats=True)",
            f"linear(x=2x9x128/1152,128,1:bf16@{x + 3}, pw=layers.{i}.fc1_ln, ln=(18x2/2,1:f32@{x + 3}, 1e-05), act={act})",
            f"linear(x=2x9x256/2304,256,1:bf16@{x + 4}, pw=layers.{i}.fc2, residual=2x9x128/1152,128,1:bf16@{x + 3}, rowstats=True)"]


# 1. text tower, folded: no LayerNorm launch inside the stack but layer 0's LN1
TEXT_FOLDED = [
    "token_embed(ids=2x9/9,1:i64@in, tok=tok, pos=pos, out_f32=False)",
    "layernorm(x=2x9x128/1152,128,1:bf16@0, gamma=layers.0.ln1[0], beta=layers.0.ln1[1], eps=1e-05)",
    "linear(x=2x9x128/1152,128,1:bf16@1, pw=layers.0.qkv)",
    "attention_causal(q=2x9x128/3456,384,1:bf16@2, k=2x9x128/3456,384,1:bf16@2, v=2x9x128/3456,384,1:bf16@2, heads=2)",
    "linear(x=2x9x128/1152,128,1:bf16@3, pw=layers.0.out, residual=2x9x128/1152,128,1:bf16@0, rowstats=True)",
    f"linear(x=2x9x128/1152,128,1:bf16@4, pw=layers.0.fc1_ln, ln=(18x2/2,1:f32@4, 1e-05), act={ops.ACT_GELU})",
    "linear(x=2x9x256/2304,256,1:bf16@5, pw=layers.0.fc2, residual=2x9x128/1152,128,1:bf16@4, rowstats=True)",
    "linear(x=2x9x128/1152,128,1:bf16@6, pw=layers.1.qkv_ln, ln=(18x2/2,1:f32@6, 1e-05))",
    "attention_causal(q=2x9x128/3456,384,1:bf16@7, k=2x9x128/3456,384,1:bf16@7, v=2x9x128/3456,384,1:bf16@7, heads=2)",
    "linear(x=2x9x128/1152,128,1:bf16@8, pw=layers.1.out, residual=2x9x128/1152,128,1:bf16@6, rowstats=True)",
    f"linear(x=2x9x128/1152,128,1:bf16@9, pw=layers.1.fc1_ln, ln=(18x2/2,1:f32@9, 1e-05), act={ops.ACT_GELU})",
    "linear(x=2x9x256/2304,256,1:bf16@10, pw=layers.1.fc2, residual=2x9x128/1152,128,1:bf16@9, rowstats=True)",
    "layernorm(x=2x9x128/1152,128,1:bf16@11, gamma=final[0], beta=final[1], eps=1e-05)",
]


def test_text_tower_folded_sequence(rec):
    te = _text_tower()
    y = te.encode_nhwc(_ids(2, 9))
    assert rec.lines(te.plan(CPU, True)) == TEXT_FOLDED
    assert TEXT_FOLDED[7:12] == _layer_folded(1, 6, ops.ACT_GELU)       # (the helper the projection tower's test uses)
    assert tuple(y.shape) == (2, 9, 128) and len(te._plans) == 1


# 2. text tower, stand-alone LayerNorms: every pack the plain one, rowstats passed as False
TEXT_SEPARATE = [
    "token_embed(ids=2x9/9,1:i64@in, tok=tok, pos=pos, out_f32=False)",
    "layernorm(x=2x9x128/1152,128,1:bf16@0, gamma=layers.0.ln1[0], beta=layers.0.ln1[1], eps=1e-05)",
    "linear(x=2x9x128/1152,128,1:bf16@1, pw=layers.0.qkv)",
    "attention_causal(q=2x9x128/3456,384,1:bf16@2, k=2x9x128/3456,384,1:bf16@2, v=2x9x128/3456,384,1:bf16@2, heads=2)",
    "linear(x=2x9x128/1152,128,1:bf16@3, pw=layers.0.out, residual=2x9x128/1152,128,1:bf16@0, rowstats=False)",
    "layernorm(x=2x9x128/1152,128,1:bf16@4, gamma=layers.0.ln2[0], beta=layers.0.ln2[1], eps=1e-05)",
    f"linear(x=2x9x128/1152,128,1:bf16@5, pw=layers.0.fc1, act={ops.ACT_GELU})",
    "linear(x=2x9x256/2304,256,1:bf16@6, pw=layers.0.fc2, residual=2x9x128/1152,128,1:bf16@4, rowstats=False)",
    "layernorm(x=2x9x128/1152,128,1:bf16@7, gamma=layers.1.ln1[0], beta=layers.1.ln1[1], eps=1e-05)",
    "linear(x=2x9x128/1152,128,1:bf16@8, pw=layers.1.qkv)",
    "attention_causal(q=2x9x128/3456,384,1:bf16@9, k=2x9x128/3456,384,1:bf16@9, v=2x9x128/3456,384,1:bf16@9, heads=2)",
    "linear(x=2x9x128/1152,128,1:bf16@10, pw=layers.1.out, residual=2x9x128/1152,128,1:bf16@7, rowstats=False)",
    "layernorm(x=2x9x128/1152,128,1:bf16@11, gamma=layers.1.ln2[0], beta=layers.1.ln2[1], eps=1e-05)",
    f"linear(x=2x9x128/1152,128,1:bf16@12, pw=layers.1.fc1, act={ops.ACT_GELU})",
    "linear(x=2x9x256/2304,256,1:bf16@13, pw=layers.1.fc2, residual=2x9x128/1152,128,1:bf16@11, rowstats=False)",
    "layernorm(x=2x9x128/1152,128,1:bf16@14, gamma=final[0], beta=final[1], eps=1e-05)",
]


def test_text_tower_separate_sequence(rec, monkeypatch):
    monkeypatch.setattr(text_encoder, "FOLD_LN_MAX_ROWS", 0)
    te = _text_tower()
    te.encode_nhwc(_ids(2, 9))
    pl = te.plan(CPU, False)
    assert rec.lines(pl) == TEXT_SEPARATE
    assert all("qkv_ln" not in e and "fc1_ln" not in e and "fc1_make" not in e for e in pl["layers"])


# 3. a folded plan whose producers emitted no statistics: the plain packs are made on demand, never during a capture
def test_text_tower_folded_plan_without_statistics_makes_the_plain_packs(rec, monkeypatch):
    te = _text_tower()
    pl = te.plan(CPU, True)
    assert all("fc1" not in e and "fc1_make" in e for e in pl["layers"]) and "qkv" not in pl["layers"][1]
    rec.stats = False
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="CLIPTextModel: run one eager encode of this shape before capturing it"):
        te.encode_stream(_ids(2, 9))
    assert "fc1" not in pl["layers"][0]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    rec.calls.clear()
    te.encode_nhwc(_ids(2, 9))
    assert te.plan(CPU, True) is pl and all("fc1" in e and "qkv" in e for e in pl["layers"])
    # the stand-alone sequence on the lazily made plain packs, except that the producers were still asked for statistics
    assert rec.lines(pl) == [s.replace("rowstats=False", "rowstats=True") for s in TEXT_SEPARATE]
    # and under a capture the same encode now finds every pack
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    te.encode_stream(_ids(2, 9))


# 4. the projection tower: the same stack with QuickGELU, then the pooled row's LayerNorm and the projection
def test_text_projection_tower_sequence(rec, monkeypatch):
    tp = _text_projection()
    monkeypatch.setattr(tp, "_device_ids", lambda ids: ids)          # (its first check: the model is on a GPU)
    emb = tp.embed_ids(_ids(2, 9))
    q = ops.ACT_QUICK_GELU
    assert q != ops.ACT_GELU
    assert rec.lines(tp.plan(CPU, True)) == (
        TEXT_FOLDED[:5] + [TEXT_FOLDED[5].replace(f"act={ops.ACT_GELU}", f"act={q}"), TEXT_FOLDED[6]] + _layer_folded(1, 6, q) + [
            "eos_pool_ln(ids=2x9/9,1:i64@in, x=2x9x128/1152,128,1:bf16@11, gamma=final[0], beta=final[1], eps=1e-05, "
            "eos_mode='argmax', eos_token_id=2)",
            "linear(x=1x2x128/256,128,1:bf16@12, pw=proj, out_f32=True)"])
    assert tuple(emb.shape) == (2, 64) and emb.dtype == torch.float32


# 5. vision tower: stand-alone LayerNorms, plain packs, no ln= and no rowstats anywhere
VISION_SEQ = [
    "image_patches(x=2x3x32x32/3072,1024,32,1:f32@in, size=32, patch=8, resize=False, out_f32=False)",
    "linear(x=2x16x192/3072,192,1:bf16@0, pw=patch, out_f32=True)",
    "vit_embed_ln(patches=32x128/128,1:f32@1, B=2, cls=cls, pos=pos, gamma=pre[0], beta=pre[1], eps=1e-05, out_f32=False)",
    "layernorm(x=2x17x128/2176,128,1:bf16@2, gamma=layers.0.ln1[0], beta=layers.0.ln1[1], eps=1e-05)",
    "linear(x=2x17x128/2176,128,1:bf16@3, pw=layers.0.qkv)",
    "attention(q=2x17x128/6528,384,1:bf16@4, k=2x17x128/6528,384,1:bf16@4, v=2x17x128/6528,384,1:bf16@4, heads=2)",
    "linear(x=2x17x128/2176,128,1:bf16@5, pw=layers.0.out, residual=2x17x128/2176,128,1:bf16@2)",
    "layernorm(x=2x17x128/2176,128,1:bf16@6, gamma=layers.0.ln2[0], beta=layers.0.ln2[1], eps=1e-05)",
    f"linear(x=2x17x128/2176,128,1:bf16@7, pw=layers.0.fc1, act={ops.ACT_QUICK_GELU})",
    "linear(x=2x17x256/4352,256,1:bf16@8, pw=layers.0.fc2, residual=2x17x128/2176,128,1:bf16@6)",
    "layernorm(x=2x17x128/2176,128,1:bf16@9, gamma=layers.1.ln1[0], beta=layers.1.ln1[1], eps=1e-05)",
    "linear(x=2x17x128/2176,128,1:bf16@10, pw=layers.1.qkv)",
    "attention(q=2x17x128/6528,384,1:bf16@11, k=2x17x128/6528,384,1:bf16@11, v=2x17x128/6528,384,1:bf16@11, heads=2)",
    "linear(x=2x17x128/2176,128,1:bf16@12, pw=layers.1.out, residual=2x17x128/2176,128,1:bf16@9)",
    "layernorm(x=2x17x128/2176,128,1:bf16@13, gamma=layers.1.ln2[0], beta=layers.1.ln2[1], eps=1e-05)",
    f"linear(x=2x17x128/2176,128,1:bf16@14, pw=layers.1.fc1, act={ops.ACT_QUICK_GELU})",
    "linear(x=2x17x256/4352,256,1:bf16@15, pw=layers.1.fc2, residual=2x17x128/2176,128,1:bf16@13)",
    "layernorm(x=1x2x128/4352,2176,1:bf16@16, gamma=post[0], beta=post[1], eps=1e-05)",          # the class rows, strided
    "linear(x=1x2x128/256,128,1:bf16@17, pw=proj, out_f32=True)",
]


def test_vision_tower_sequence(rec, monkeypatch):
    vm = _vision()
    monkeypatch.setattr(vm, "_device", lambda: CPU)                  # (its only check: the model is on a GPU)
    out = vm(torch.zeros(2, 3, 32, 32))
    pl = vm.plan(CPU)
    assert rec.lines(pl) == VISION_SEQ
    assert all(sorted(e) == ["fc1", "fc2", "ln1", "ln2", "out", "qkv"] for e in pl["layers"])
    assert tuple(out.image_embeds.shape) == (2, 64) and tuple(out.last_hidden_state.shape) == (2, 17, 128)


# 6. MPNet: post-LayerNorm layers, every bf16 linear pinned to its lean tile unless the knob or the dtype says otherwise
def _mpnet_seq(dt, pin):
    a, f32 = ("f32", True) if dt == torch.float32 else ("bf16", False)
    seq = [f"embed_ln(ids=3x12/12,1:i64@in, word=word, pos=pos, gamma=eln[0], beta=eln[1], eps=1e-05, pad_id=1, out_f32={f32})"]
    for i, x in ((0, 0), (1, 7)):
        seq += [f"linear(x=3x12x128/1536,128,1:{a}@{x}, pw=layers.{i}.qkv{pin})",
                f"attention_bias(q=3x12x128/4608,384,1:{a}@{x + 1}, k=3x12x128/4608,384,1:{a}@{x + 1}, v=3x12x128/4608,384,1:{a}@{x + 1}, "
                "heads=2, relbias=bias.12, key_mask=3x12/12,1:f32@in)",
                f"linear(x=3x12x128/1536,128,1:{a}@{x + 2}, pw=layers.{i}.o, residual=3x12x128/1536,128,1:{a}@{x}{pin})",
                f"layernorm(x=3x12x128/1536,128,1:{a}@{x + 3}, gamma=layers.{i}.ln1[0], beta=layers.{i}.ln1[1], eps=1e-05)",
                f"linear(x=3x12x128/1536,128,1:{a}@{x + 4}, pw=layers.{i}.in, act={ops.ACT_GELU}{pin})",
                f"linear(x=3x12x256/3072,256,1:{a}@{x + 5}, pw=layers.{i}.out, residual=3x12x128/1536,128,1:{a}@{x + 4}{pin})",
                f"layernorm(x=3x12x128/1536,128,1:{a}@{x + 6}, gamma=layers.{i}.ln2[0], beta=layers.{i}.ln2[1], eps=1e-05)"]
    return seq + [f"masked_mean(x=3x12x128/1536,128,1:{a}@14, mask=3x12/12,1:f32@in)"]


@pytest.mark.parametrize("case", ["bf16", "fp32", "not_invariant"])
def test_mpnet_sequence(rec, monkeypatch, case):
    from diffusion_pruning_amd.launch_policy import _lean_tile
    dt = torch.float32 if case == "fp32" else torch.bfloat16
    monkeypatch.setattr(ops, "ACT_DTYPE", dt)
    monkeypatch.setattr(prompt_encoder, "BATCH_INVARIANT", case != "not_invariant")
    mp = _mpnet()
    monkeypatch.setattr(mp, "_check_inputs", lambda ids, mask: (ids, mask))      # (its first check: the model is on a GPU)
    mask = torch.ones(3, 12)
    mask[1, 8:] = 0
    z = mp.encode(_ids(3, 12), mask)
    pin = f", tile={_lean_tile(36)!r}, split_k=1" if case == "bf16" else ""
    assert rec.lines(mp.plan(CPU)) == _mpnet_seq(dt, pin)
    assert tuple(z.shape) == (3, 128)
    # the bias table of a new length cannot be built during a capture
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    mp.encode(_ids(3, 12), mask)
    with pytest.raises(RuntimeError, match="MPNetModel: run one eager encode of this shape before capturing it"):
        mp.encode(_ids(3, 13), None)


# 7. init_synthetic: the loops as each model spelled them out before they shared one
def _old_init_clip_text(model, seed):
    g = torch.Generator().manual_seed(seed)
    for name, p in model.named_parameters():
        if "embedding" in name:
            p.copy_(0.5 * torch.randn(p.shape, generator=g))
        elif name.endswith("bias"):
            p.copy_(0.02 * torch.randn(p.shape, generator=g))
        elif p.dim() == 1:                                   # LayerNorm gamma
            p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
        else:
            scale = 0.5 if (".out_proj." in name or ".fc2." in name) else 1.0
            p.copy_(scale * p.shape[1] ** -0.5 * torch.randn(p.shape, generator=g))


def _old_init_clip_vision(model, seed):
    g = torch.Generator().manual_seed(seed)
    for name, p in model.named_parameters():
        if "patch_embedding" in name:
            p.copy_(p[0].numel() ** -0.5 * torch.randn(p.shape, generator=g))
        elif "embedding" in name:
            p.copy_(0.5 * torch.randn(p.shape, generator=g))
        elif name.endswith("bias"):
            p.copy_(0.02 * torch.randn(p.shape, generator=g))
        elif p.dim() == 1:                                   # LayerNorm gamma
            p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
        else:
            scale = 0.5 if (".out_proj." in name or ".fc2." in name) else 1.0
            p.copy_(scale * p.shape[1] ** -0.5 * torch.randn(p.shape, generator=g))


def _old_init_mpnet(model, seed):
    g = torch.Generator().manual_seed(seed)
    for name, p in model.named_parameters():
        if name == "encoder.relative_attention_bias.weight":
            p.copy_(torch.randn(p.shape, generator=g))
        elif "embeddings.weight" in name:
            p.copy_(0.5 * torch.randn(p.shape, generator=g))
        elif name.endswith("bias"):
            p.copy_(0.02 * torch.randn(p.shape, generator=g))
        elif p.dim() == 1:                                   # LayerNorm gamma
            p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
        else:
            scale = 0.5 if (".attn.o." in name or ".output.dense." in name) else 1.0
            p.copy_(scale * p.shape[1] ** -0.5 * torch.randn(p.shape, generator=g))


MODELS = {"text": (_text_tower, _old_init_clip_text), "text_projection": (_text_projection, _old_init_clip_text),
          "vision": (_vision, _old_init_clip_vision), "mpnet": (_mpnet, _old_init_mpnet)}


@pytest.mark.parametrize("seed", [0, 3])
@pytest.mark.parametrize("which", sorted(MODELS))
def test_init_synthetic_draws_what_the_per_model_loops_drew(which, seed):
    make, old = MODELS[which]
    got, want = make(), make()
    with torch.no_grad():
        for p in want.parameters():
            p.fill_(float("nan"))
        old(want, seed)
    assert got.init_synthetic(seed) is got
    sd, ref = got.state_dict(), want.state_dict()
    assert list(sd) == list(ref) and len(sd) > 30
    for k in sd:
        assert torch.equal(sd[k], ref[k]), k
    if seed:
        assert not torch.equal(sd[next(iter(sd))], make().state_dict()[next(iter(sd))])


# 8. what the models share
def test_plan_cache_has_one_home():
    assert unet._PlanCache is M._PlanCache and unet._versions is M._versions and unet.LinearP is M.LinearP


def _vae():
    return AutoencoderKL(VAEConfig(block_out_channels=(32, 64), layers_per_block=1)).init_synthetic(0)


@pytest.mark.parametrize("which", sorted(MODELS) + ["vae"])
def test_to_and_invalidate_release_plans_and_the_parameter_list(which):
    m = _vae() if which == "vae" else MODELS[which][0]()
    plan = (lambda: m.plan(CPU, True)) if which.startswith("text") else (lambda: m.plan(CPU))
    for release in (m.invalidate, lambda: m.to("cpu"), lambda: m.float()):
        pl = plan()
        assert plan() is pl and len(m._plans) == 1 and "_vparams" in m.__dict__
        release()
        assert len(m._plans) == 0 and not m._plans.parked and "_vparams" not in m.__dict__
