"""Host tests of the MPNet prompt encoder: the oracle against the golden fixture (made by transformers' MPNetModel), the
host-side relative-position table and position ids, the configuration, strict loading, FLOP counts, the new C-ABI structs
and the argument checks of the pipeline's router_ids and train_step's router ids."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from diffusion_pruning_amd.pipeline import PruningDenoiseLoop
from diffusion_pruning_amd.prompt_encoder import (MPNetConfig, MPNetModel, MPNetModelOutput, assign_experts,
                                                  prompt_encoder_flops, relative_bias_table, relative_position_bucket)
from diffusion_pruning_amd.train_step import batch_from_images, router_embeddings
from tests.helpers import rel_l2, write_safetensors
from tests.mpnet_oracle import mpnet_forward, position_bias, position_ids

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mpnet_tiny.npz")
TINY = dict(vocab_size=96, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
            max_position_embeddings=204)
# sentence-transformers/all-mpnet-base-v2, config.json
BASE_CONFIG = {"_name_or_path": "microsoft/mpnet-base", "architectures": ["MPNetForMaskedLM"], "attention_probs_dropout_prob": 0.1,
               "bos_token_id": 0, "eos_token_id": 2, "hidden_act": "gelu", "hidden_dropout_prob": 0.1, "hidden_size": 768,
               "initializer_range": 0.02, "intermediate_size": 3072, "layer_norm_eps": 1e-05, "max_position_embeddings": 514,
               "model_type": "mpnet", "num_attention_heads": 12, "num_hidden_layers": 12, "pad_token_id": 1,
               "relative_attention_num_buckets": 32, "transformers_version": "4.8.2", "vocab_size": 30527}
# the fixture stores fp32: its own rounding is 2^-24 per element.  The fp64 oracle must sit there; the fp32 oracle adds a few
# fp32 roundings per element over two layers (every LayerNorm renormalises, so they do not grow): 2e-6 is ~30 fp32 epsilons.
ORACLE_F64_TOL = 1e-7
ORACLE_F32_TOL = 2e-6


def _golden():
    z = np.load(GOLDEN)
    params = {k: torch.from_numpy(z[k].astype(np.float64)) for k in z.files if k.startswith(("embeddings.", "encoder."))}
    return z, params


@pytest.mark.parametrize("dtype,tol", [(torch.float64, ORACLE_F64_TOL), (torch.float32, ORACLE_F32_TOL)])
def test_oracle_reproduces_the_golden_fixture(dtype, tol):
    z, params = _golden()
    for n in "abc":
        ids, mask = torch.from_numpy(z[f"ids_{n}"]), torch.from_numpy(z[f"mask_{n}"].astype(np.int64))
        h, pooled = mpnet_forward(params, ids, mask, heads=2, layers=2, dtype=dtype)
        v = mask.bool()
        eh = rel_l2(h[v], torch.from_numpy(z[f"last_hidden_state_{n}"])[v])
        ep = rel_l2(pooled, torch.from_numpy(z[f"pooled_{n}"]))
        print(f"mpnet oracle {dtype} batch {n}: hidden {eh:.3e} pooled {ep:.3e}")
        assert eh <= tol and ep <= tol, (n, eh, ep)


def test_fixture_has_the_cases_it_promises():
    z, _ = _golden()
    la = z["mask_a"].sum(1).tolist()
    assert 1 in la and len(set(la)) == len(la)                                 # ragged, including length 1
    assert z["ids_b"].shape[1] > 128 and z["mask_b"][0].all()                   # distances in the saturated buckets
    m = z["mask_c"][0]
    assert m[-1] == 1 and (m == 0).any()                                        # not a prefix
    assert (z["ids_c"][1][:13] == 1).any()                                      # an interior pad token


@pytest.mark.parametrize("L", [1, 7, 128, 129, 512])
def test_host_bias_table_equals_the_fixture_buckets(L):
    z, _ = _golden()
    want = torch.from_numpy(z[f"bucket_L{L}"].astype(np.int64))
    rel = torch.arange(-(L - 1), L)
    assert torch.equal(relative_position_bucket(rel, 32), want)
    w = torch.randn(32, 12, generator=torch.Generator().manual_seed(L))
    t = relative_bias_table(w, L)
    assert t.shape == (12, 2 * L - 1) and t.dtype == torch.float32 and t.is_contiguous()
    assert torch.equal(t, w[want].t())
    # the [heads, L, L] bias transformers builds is this table read at j - i + L - 1
    ar = torch.arange(L)
    full = position_bias(w, L)
    assert torch.equal(t[:, (ar[None, :] - ar[:, None]) + L - 1], full)


def test_buckets_are_exact_below_8_log_spaced_and_saturate_at_128():
    b = relative_position_bucket(torch.arange(-600, 601), 32)
    at = lambda d: int(b[d + 600])      # noqa: E731
    assert [at(-d) for d in range(8)] == list(range(8))                         # n = -rel >= 0: buckets 0..7 exact
    assert [at(d) for d in range(1, 8)] == [16 + d for d in range(1, 8)]
    assert at(-127) <= 15 and at(-128) == 15 and at(-600) == 15 and at(128) == 31 and at(600) == 31
    assert int(b.min()) == 0 and int(b.max()) == 31


def test_position_ids_with_interior_pads():
    ids = torch.tensor([[5, 1, 7, 1, 1, 9], [1, 1, 4, 5, 6, 1], [3, 4, 5, 6, 7, 8]])
    assert position_ids(ids).tolist() == [[2, 1, 3, 1, 1, 4], [1, 1, 2, 3, 4, 1], [2, 3, 4, 5, 6, 7]]


def test_base_config_and_parameter_count():
    cfg = MPNetConfig.from_dict(BASE_CONFIG)                                    # unknown keys are ignored
    assert cfg == MPNetConfig()
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.head_dim) == (768, 3072, 12, 12, 64)
    assert (cfg.vocab_size, cfg.max_position_embeddings, cfg.pad_token_id, cfg.layer_norm_eps, cfg.max_length) == (30527, 514, 1, 1e-5, 512)
    m = MPNetModel(cfg)
    # word 30527 x 768 + position 514 x 768 + LayerNorm 2 x 768 + 12 layers x 7,087,872 + bias table 32 x 12
    assert sum(p.numel() for p in m.parameters()) == 30527 * 768 + 514 * 768 + 1536 + 12 * 7_087_872 + 384


def test_prompt_encoder_flops():
    cfg = MPNetConfig()
    H, I = 768, 3072
    for L in (1, 32, 512):
        assert prompt_encoder_flops(cfg, L) == 12 * (2.0 * L * (4 * H * H + 2 * H * I) + 4.0 * H * L * L)
    assert abs(prompt_encoder_flops(cfg, 32) - 5.473566720e9) < 1.0             # linears 5.436 GFLOP + attention 0.038 GFLOP
    tiny = MPNetConfig(**TINY)
    assert prompt_encoder_flops(tiny, 10) == 2 * (2.0 * 10 * (4 * 128 * 128 + 2 * 128 * 128) + 4.0 * 128 * 100)


@pytest.mark.parametrize("bad", [dict(hidden_act="gelu_new"), dict(hidden_size=192, num_attention_heads=2),
                                 dict(max_position_embeddings=1026), dict(relative_attention_num_buckets=30)])
def test_unsupported_configs_raise(bad):
    with pytest.raises(NotImplementedError):
        MPNetModel(MPNetConfig(**{**TINY, **bad}))


@pytest.mark.parametrize("kw", [dict(position_ids=torch.arange(4)[None]), dict(output_hidden_states=True),
                                dict(output_attentions=True), dict(inputs_embeds=torch.zeros(1, 4, 128)),
                                dict(head_mask=torch.ones(2))])
def test_unsupported_forward_arguments_raise(kw):
    m = MPNetModel(MPNetConfig(**TINY))
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 4, dtype=torch.long), **kw)


def test_forward_and_encode_need_a_gpu_and_integer_ids():
    m = MPNetModel(MPNetConfig(**TINY)).init_synthetic(0)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="GPU"):
        m.encode(torch.zeros(1, 4, dtype=torch.long), torch.ones(1, 4))


def test_output_indexing_follows_transformers():
    h = torch.zeros(1, 2, 3)
    o = MPNetModelOutput(last_hidden_state=h)
    assert o[0] is h and o["last_hidden_state"] is h and o.to_tuple() == (h,)


def test_golden_parameters_load_into_the_module():
    _, params = _golden()
    m = MPNetModel(MPNetConfig(**TINY)).load_mpnet_state_dict({k: v.float() for k, v in params.items()})
    assert set(m.state_dict()) == set(params)
    for k, v in params.items():
        assert torch.equal(m.state_dict()[k], v.float()), k


def _folder(tmp_path, sd, cfg=None):
    d = tmp_path / "mpnet"
    d.mkdir()
    (d / "config.json").write_text(json.dumps({**(cfg or TINY), "hidden_act": "gelu", "model_type": "mpnet", "bos_token_id": 0}))
    write_safetensors(str(d / "model.safetensors"), sd)
    return str(tmp_path)


@pytest.mark.parametrize("prefix", ["", "mpnet."])
def test_from_pretrained_accepts_the_pooler_and_position_ids(tmp_path, prefix):
    src = MPNetModel(MPNetConfig(**TINY)).init_synthetic(3)
    sd = {prefix + k: v for k, v in src.state_dict().items()}
    sd[prefix + "pooler.dense.weight"] = torch.zeros(128, 128)
    sd[prefix + "pooler.dense.bias"] = torch.zeros(128)
    sd[prefix + "embeddings.position_ids"] = torch.arange(204)[None]
    m = MPNetModel.from_pretrained(_folder(tmp_path, sd), subfolder="mpnet")
    assert m.config == MPNetConfig(**TINY)
    for k, v in src.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    assert MPNetModel.from_pretrained(os.path.join(str(tmp_path), "mpnet")).config == m.config      # subfolder=None


@pytest.mark.parametrize("change", ["missing", "extra", "shape", "bias_table"])
def test_from_pretrained_is_strict(tmp_path, change):
    sd = dict(MPNetModel(MPNetConfig(**TINY)).init_synthetic(3).state_dict())
    if change == "missing":
        sd.pop("encoder.layer.1.output.dense.bias")
    elif change == "extra":
        sd["encoder.layer.1.output.dense2.bias"] = torch.zeros(128)
    elif change == "shape":
        sd["embeddings.LayerNorm.weight"] = torch.zeros(64)
    else:
        sd["encoder.relative_attention_bias.weight"] = torch.zeros(32, 12)
    with pytest.raises((KeyError, ValueError)):
        MPNetModel.from_pretrained(_folder(tmp_path, sd), subfolder="mpnet")


def test_every_layer_changes_the_stream_and_the_bias_is_order_one_under_init_synthetic():
    m = MPNetModel(MPNetConfig(**{**TINY, "num_hidden_layers": 4})).init_synthetic(0)
    sd = m.state_dict()
    assert 0.5 < float(sd["encoder.relative_attention_bias.weight"].std()) < 2.0
    ids = torch.randint(3, 96, (2, 30), generator=torch.Generator().manual_seed(1))
    outs = [mpnet_forward(sd, ids, None, heads=2, layers=n, dtype=torch.float32)[0] for n in range(5)]
    for i in range(1, 5):
        rel = float((outs[i] - outs[i - 1]).norm() / outs[i - 1].norm())
        assert rel >= 0.05, (i, rel)
    # and the bias matters: without it the output moves
    sd0 = {**sd, "encoder.relative_attention_bias.weight": torch.zeros(32, 2)}
    assert rel_l2(mpnet_forward(sd0, ids, None, heads=2, layers=4, dtype=torch.float32)[0], outs[4]) > 0.01


def test_new_ctypes_layouts_match_the_c_header(tmp_path):
    import subprocess
    from diffusion_pruning_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {"AptpAttentionBiasParams": _lib.AttentionBiasParams, "AptpEmbedLnParams": _lib.EmbedLnParams,
               "AptpMaskedMeanParams": _lib.MaskedMeanParams}
    body = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(root, "include", "aptp_hip.h")}"', "int main(void){"]
    want = []
    for cname, cls in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            body.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            want.append(getattr(cls, fname).offset)
    body.append("return 0;}")
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(body))
    subprocess.run(["cc", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want


def test_c_entry_points_refuse_bad_extents_before_launching():
    """never dereferenced pointers: each launch is refused by the argument checks"""
    from diffusion_pruning_amd import _lib
    lib = _lib.load()
    p = _lib.AttentionBiasParams()
    assert lib.aptp_attention_bias(ctypes.byref(p), None) == -1 and b"null pointer" in lib.aptp_last_error()
    p.q, p.k, p.v, p.o, p.relbias = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20
    for f in ("q", "k", "v", "o"):
        setattr(p, f + "_stride_l", 128)
        setattr(p, f + "_stride_b", 128 * 513)
    p.B, p.heads, p.scale = 1, 2, 0.125
    for L in (0, 513):
        p.L = L
        assert lib.aptp_attention_bias(ctypes.byref(p), None) == -1 and b"outside [1, 512]" in lib.aptp_last_error()
    p.L, p.k_stride_l = 16, 132
    assert lib.aptp_attention_bias(ctypes.byref(p), None) == -1 and b"row stride" in lib.aptp_last_error()
    p.k_stride_l, p.v = 128, (3 << 20) + 8
    assert lib.aptp_attention_bias(ctypes.byref(p), None) == -1 and b"16-byte aligned" in lib.aptp_last_error()
    e = _lib.EmbedLnParams()
    e.ids, e.word, e.pos, e.gamma, e.beta, e.out = (i << 20 for i in range(1, 7))
    e.ldo, e.B, e.L, e.C, e.vocab, e.pos_rows, e.pad_id, e.eps = 64, 1, 513, 64, 100, 514, 1, 1e-5
    assert lib.aptp_embed_ln(ctypes.byref(e), None) == -1 and b"position rows" in lib.aptp_last_error()
    mm = _lib.MaskedMeanParams()
    mm.x, mm.out, mm.B, mm.L, mm.C, mm.x_stride_l, mm.x_stride_b = 1 << 20, 2 << 20, 1, 4, 6, 6, 24
    assert lib.aptp_masked_mean(ctypes.byref(mm), None) == -1 and b"multiple of 4" in lib.aptp_last_error()


class _Spy:
    """stands in for a prompt encoder: remembers what encode was given"""

    def __init__(self):
        self.calls = []

    def encode(self, ids, mask=None):
        self.calls.append((ids, mask))
        return torch.full((ids.shape[0], 8), 0.5)


def test_pipeline_router_argument_checks():
    loop = PruningDenoiseLoop(unet=None)
    lat, ehs = torch.zeros(1, 4, 8, 8), torch.zeros(1, 77, 16)
    ids, mask = torch.zeros(1, 12, dtype=torch.long), torch.ones(1, 12, dtype=torch.long)
    with pytest.raises(ValueError, match="prompt_encoder"):
        loop(ehs, lat, router_ids=ids)                                          # no prompt_encoder
    loop = PruningDenoiseLoop(unet=None, prompt_encoder=_Spy())
    with pytest.raises(ValueError, match="not both"):
        loop(ehs, lat, hyper_net_input=torch.zeros(1, 8), router_ids=ids)       # embedding and ids
    with pytest.raises(ValueError, match="needs router_ids"):
        loop(ehs, lat, router_attention_mask=mask)                              # a mask alone
    with pytest.raises(TypeError):
        loop(ehs, lat, 50, 7.5, None, None, True, "latent", ids)                # keyword-only
    assert loop.prompt_encoder.calls == []


def test_train_step_router_argument_checks():
    ids, mask = torch.zeros(2, 12, dtype=torch.long), torch.ones(2, 12, dtype=torch.long)
    px, ehs, emb = torch.zeros(2, 3, 16, 16), torch.zeros(2, 77, 16), torch.zeros(2, 8)
    with pytest.raises(ValueError, match="exactly one"):
        batch_from_images(None, px, ehs)                                        # neither
    with pytest.raises(ValueError, match="exactly one"):
        batch_from_images(None, px, ehs, emb, router_ids=ids, prompt_encoder=_Spy())
    with pytest.raises(ValueError, match="needs router_ids"):
        batch_from_images(None, px, ehs, emb, router_attention_mask=mask)
    with pytest.raises(ValueError, match="prompt_encoder"):
        batch_from_images(None, px, ehs, router_ids=ids, router_attention_mask=mask)
    with pytest.raises(ValueError, match="prompt_encoder"):
        router_embeddings(None, ids, mask)
    spy = _Spy()
    z = router_embeddings(spy, ids, mask)
    assert z.shape == (2, 8) and spy.calls[0][0] is ids and spy.calls[0][1] is mask


class _Head(torch.nn.Module):
    def forward(self, z):
        assert not self.training
        return z


class _Codes(torch.nn.Module):
    def get_cosine_sim_min_encoding_indices(self, z):
        assert not self.training
        return torch.arange(z.shape[0], dtype=torch.int32)


def test_assign_experts_chunks_restores_modes_and_checks_arguments():
    spy, hn, vq = _Spy(), _Head().train(), _Codes().eval()
    ids, mask = torch.zeros(5, 12, dtype=torch.long), torch.ones(5, 12, dtype=torch.long)
    idx = assign_experts(spy, hn, vq, ids, mask, batch_size=2)
    assert idx.dtype == torch.int64 and idx.tolist() == [0, 1, 0, 1, 0]
    assert [c[0].shape[0] for c in spy.calls] == [2, 2, 1] and [c[1].shape[0] for c in spy.calls] == [2, 2, 1]
    assert hn.training and not vq.training
    assert assign_experts(spy, hn, vq, ids).tolist() == [0, 1, 2, 3, 4] and spy.calls[-1][1] is None
    with pytest.raises(ValueError):
        assign_experts(spy, hn, vq, ids[0])
    with pytest.raises(ValueError):
        assign_experts(spy, hn, vq, ids, batch_size=0)
