"""CPU checks behind tests/test_attention_grad_gpu.py: the fp64 reference's gradients are right, the reference and its format
model stay inside their own bounds on every case of the GPU list, the metrics see each seeded defect of a kind a kernel could
have (and pass the harmless one), and the host-side rules of aptp_attention / aptp_attention_bwd (no kernel launch: every failing
call returns before it would launch).  The figures measured here are printed as one table by the last test of the module."""
import ctypes
import math
import os

import pytest
import torch

from tests import attention_model as AM

SEEDS = (0, 1, 2, 3)
SPREAD_LIMIT = 1.6       # between model(fp64) and model(fp32, shift 0.37) on smooth cases; the GPU tests allow 2
TABLE = {"use": {}, "spread": {}, "defects": {}}


def _table_lines():
    out = []
    w = out.append
    w("attention model, reference alone (worst over 4 seeds): hard_use of model(fp64) | model(fp32, shift 0.37) per output; "
      "block-ratio spread between the two")
    w(f"{'case':28s} " + " ".join(f"{k:>11s}" for k in AM.KEYS) + "   spread " + " ".join(f"{k:>5s}" for k in AM.RATIO_KEYS))
    for cid, use in TABLE["use"].items():
        sp = TABLE["spread"].get(cid)
        w(f"{cid:28s} " + " ".join(f"{use[k][0]:5.2f}|{use[k][1]:5.2f}" for k in AM.KEYS) + "          " +
          " ".join(f"{sp[k]:5.2f}" for k in AM.RATIO_KEYS) + ("" if AM.CASES[use['index']].smooth else "  (spiked: not asserted)"))
    if TABLE["use"]:
        def worst(smooth):
            return max([max(TABLE["spread"][c][k] for k in AM.RATIO_KEYS) for c, u in TABLE["use"].items()
                        if AM.CASES[u["index"]].smooth == smooth], default=float("nan"))
        w(f"worst hard_use {max(max(max(u[k]) for k in AM.KEYS) for u in TABLE['use'].values()):.3f} (limit 1); worst spread on "
          f"smooth cases {worst(True):.3f} (limit {SPREAD_LIMIT}); on spiked cases {worst(False):.3f}")
    for name, txt in TABLE["defects"].items():
        w(f"defect {name:42s} {txt}")
    return out


def _heads(t, B, L, h):
    return t.view(B, L, h, 64).transpose(1, 2)


@pytest.mark.parametrize("shape", [(2, 2, 5, 7), (1, 3, 70, 33), (1, 1, 129, 65)])
def test_ref64_gradients_equal_fp64_autograd(shape):
    B, h, Lq, Lk = shape
    g = torch.Generator().manual_seed(Lq * 1000 + Lk)
    q, k, v, do = (torch.randn(B, h, L, 64, generator=g).bfloat16().double() for L in (Lq, Lk, Lk, Lq))
    for scale in (0.125, 0.3):
        qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
        o = torch.softmax((qa @ ka.transpose(-1, -2)) * scale, dim=-1) @ va
        o.backward(do)
        ref, _ = AM.ref64(q, k, v, do, scale)
        for name, want in (("o", o.detach()), ("dq", qa.grad), ("dk", ka.grad), ("dv", va.grad)):
            rel = float((ref[name] - want).abs().max() / want.abs().max())
            assert rel <= 1e-12, (name, rel)
        lse = torch.logsumexp((q @ k.transpose(-1, -2)) * scale, dim=-1) / math.log(2.0)
        assert float((ref["lse"] - lse).abs().max()) <= 1e-12 * float(lse.abs().max())


@pytest.mark.parametrize("index", range(len(AM.CASES)), ids=[c.id for c in AM.CASES])
def test_reference_alone_stays_inside_its_own_conditions(index):
    case = AM.CASES[index]
    use = {k: [0.0, 0.0] for k in AM.KEYS}
    spread = {k: 0.0 for k in AM.RATIO_KEYS}
    for seed in SEEDS:
        ins, ref, bound, m64 = AM.case_reference(index, seed)
        m32 = AM.model(*ins, case.eff_scale, torch.float32, shift=0.37)
        for j, m in enumerate((m64, m32)):
            for k in AM.KEYS:
                use[k][j] = max(use[k][j], AM.hard_use(m[k], ref[k], bound[k]))
        for k in AM.RATIO_KEYS:
            spread[k] = max(spread[k], float(AM.block_ratio(m32[k], m64[k], ref[k], bound[k]).max()),
                            float(AM.block_ratio(m64[k], m32[k], ref[k], bound[k]).max()))
    use["index"] = index
    TABLE["use"][case.id] = use
    TABLE["spread"][case.id] = spread
    for k in AM.KEYS:
        assert max(use[k]) <= AM.HARD_LIMIT, (case.id, k, use[k])
    if case.smooth:
        for k in AM.RATIO_KEYS:
            assert spread[k] <= SPREAD_LIMIT, (case.id, k, spread[k])


def _caught_by(got, index, seed=0):
    """the checks of the GPU test that ``got`` fails on this case: hard bound per output, lse bound, block ratio (smooth only)"""
    case = AM.CASES[index]
    _, ref, bound, mdl = AM.case_reference(index, seed)
    res = AM.measure(got, ref, bound, mdl)
    fails = []
    for k, (hu, br) in res.items():
        if hu > AM.HARD_LIMIT:
            fails.append(("lse bound" if k == "lse" else f"hard bound {k}") + f" {hu:.3g}")
        if case.smooth and br is not None and br > AM.RATIO_LIMIT:
            fails.append(f"block ratio {k} {br:.3g}")
    return fails


@pytest.mark.parametrize("name", list(AM.broken_models))
def test_metrics_see_the_seeded_defects(name):
    caught = {}
    for index, case in enumerate(AM.CASES):
        ins = AM.make_inputs(index, 0)
        got = AM.broken_models[name](*ins, case.eff_scale, torch.float32)
        fails = _caught_by(got, index)
        if fails:
            caught[case.id] = fails
    if name == AM.HARMLESS:
        TABLE["defects"][name] = "passes every case (harmless)" if not caught else f"FAILS {caught}"
        assert not caught, caught
        return
    first = next(iter(caught.items())) if caught else None
    TABLE["defects"][name] = (f"caught on {len(caught)} of {len(AM.CASES)} cases; first {first[0]}: " + ", ".join(first[1][:3])) if caught else "NOT CAUGHT"
    assert caught, name


def test_sound_fp32_model_is_not_caught():
    """the control of the defect test: the same fp32 model without a defect fails nothing"""
    for index, case in enumerate(AM.CASES):
        got = AM.model(*AM.make_inputs(index, 0), case.eff_scale, torch.float32)
        assert not _caught_by(got, index), case.id


# ---------------------------------------------------------------------------------------------------------------------
# host rules of the library
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from diffusion_pruning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _bwd_params(B=1, heads=2, Lq=100, Lk=77):
    """valid but never launched: every pointer is a fake 16-byte aligned address"""
    from diffusion_pruning_amd import _lib
    p = _lib.AttentionBwdParams()
    for n in ("q", "k", "v", "o", "dout", "dq", "dk", "dv"):
        setattr(p, n, 4096)
        setattr(p, n + "_stride_l", heads * 64)
        setattr(p, n + "_stride_b", heads * 64 * max(Lq, Lk))
    p.lse = p.delta = 4096
    p.B, p.heads, p.Lq, p.Lk, p.scale = B, heads, Lq, Lk, 0.125
    return p


def test_q_split_rule_and_workspace(lib):
    def split(B, h, Lq, Lk):
        return lib.aptp_attention_bwd_q_split(ctypes.byref(_bwd_params(B, h, Lq, Lk)))
    assert split(1, 2, 1024, 77) == 8
    assert lib.aptp_attention_bwd_q_split(None) == 1
    for B in (1, 2, 4, 16):
        for h in (1, 2, 5, 20):
            for Lq in (1, 64, 960, 961, 1024, 4096, 5000):
                for Lk in (1, 77, 128, 129, 1024, 4096):
                    s = split(B, h, Lq, Lk)
                    wgs, tiles = -(-Lk // 128) * h * B, -(-Lq // 64)
                    if wgs >= 128 or tiles < 16:
                        assert s == 1, (B, h, Lq, Lk, s)
                    else:
                        assert 1 <= s <= tiles // 2, (B, h, Lq, Lk, s)
    p = _bwd_params(2, 3, 1024, 77)
    for s in (-1, 0, 1):
        assert lib.aptp_attention_bwd_workspace_bytes(ctypes.byref(p), s) == 0
    for s in (2, 3, 8):
        assert lib.aptp_attention_bwd_workspace_bytes(ctypes.byref(p), s) == s * 2 * 3 * 77 * 512
    assert lib.aptp_attention_bwd_workspace_bytes(None, 4) == 0


def test_attention_bwd_rejects_bad_arguments_without_launching(lib):
    def rejected(why, **fields):
        p = _bwd_params()
        for k, v in fields.items():
            setattr(p, k, v)
        assert lib.aptp_attention_bwd(ctypes.byref(p), None) == -1, fields
        assert why in lib.aptp_last_error(), (fields, lib.aptp_last_error())

    assert lib.aptp_attention_bwd(None, None) == -1
    for n in ("q", "k", "v", "o", "dout", "dq", "dk", "dv", "lse", "delta"):
        rejected(b"null pointer", **{n: None})
    for n in ("q", "k", "v", "o", "dout", "dq", "dk", "dv"):
        rejected(b"multiples of 8", **{n + "_stride_l": 132})
        rejected(b"multiples of 8", **{n + "_stride_b": 128 * 100 + 4})
        rejected(b"16-byte aligned", **{n: 4096 + 8})
        rejected(b"row stride < heads*64", **{n + "_stride_l": 120})
        rejected(b"row stride < heads*64", **{n + "_stride_l": 64})
    rejected(b"bad extents", Lq=0)
    rejected(b"bad extents", Lk=0)
    rejected(b"q_split", q_split=2)                              # no workspace
    rejected(b"q_split", q_split=2, workspace=4096 + 4)          # misaligned workspace
    rejected(b"q_split", q_split=3, workspace=4096)              # Lq = 100: two query tiles
    for s in (0.0, -0.125, float("nan")):
        rejected(b"scale must be positive", scale=s)


def test_attention_rejects_non_positive_scale_without_launching(lib):
    from diffusion_pruning_amd import _lib
    for s in (0.0, -0.125, float("nan")):
        p = _lib.AttentionParams()
        for n in ("q", "k", "v", "o"):
            setattr(p, n, 4096)
            setattr(p, n + "_stride_l", 128)
            setattr(p, n + "_stride_b", 128 * 100)
        p.B, p.heads, p.Lq, p.Lk, p.scale = 1, 2, 100, 77, s
        for variant in (0, 5, 6):
            p.variant = variant
            assert lib.aptp_attention(ctypes.byref(p), None) == -1
            assert b"scale must be positive" in lib.aptp_last_error()


def test_print_the_measured_table(capsys):
    """last in the module: the figures the tests above measured, shown even when output is captured"""
    with capsys.disabled():
        print()
        for line in _table_lines():
            print(line)
