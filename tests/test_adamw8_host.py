"""CPU checks of the block-wise 8-bit AdamW state (csrc/optim8.hip, packed_train.PackedAdamW(optim_bits=8)): the two
code maps, the numpy model that defines the format (tests/adamw8_model.py), the C layout of the new structs, argument
validation that fails without launching, and the partition rule with its byte count."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import adamw8_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aptp_hip.h")


@pytest.fixture(scope="module")
def lib():
    from diffusion_pruning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---- the maps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [True, False])
def test_maps(signed):
    q = M.MAP_SIGNED if signed else M.MAP_UNSIGNED
    assert q.dtype == np.float32 and q.shape == (256,)
    assert np.all(np.diff(q.astype(np.float64)) > 0)                     # strictly increasing: 256 distinct values
    assert q[-1] == np.float32(1.0) and 0.0 in q
    zero = M.ZERO_SIGNED if signed else M.ZERO_UNSIGNED
    assert (zero, q[zero]) == ((127, 0.0) if signed else (0, 0.0))
    gaps = np.diff(q.astype(np.float64))
    if signed:
        assert q[128] == np.float32(5.5e-7) and q[126] == np.float32(-5.5e-7)              # decade 0: one midpoint, both signs
        assert q[0] == np.float32(-(1.0 - 0.9 / 128)) == np.float32(-0.99296875)
        assert q[254] == np.float32(0.99296875)                                            # +1.0 has no mirror image
        assert abs(gaps.min() - 5.5e-7) < 1e-9 and abs(gaps.max() / 2 - 0.9 / 128) < 1e-7          # 64 steps in the top decade
    else:
        assert q[1] == np.float32(3.25e-7) and q[2] == np.float32(7.75e-7)                 # decade 0: two midpoints
        assert abs(gaps.min() - 3.25e-7) < 1e-9 and abs(gaps.max() / 2 - 0.9 / 256) < 1e-7         # 128 steps in the top decade


def test_the_package_builds_the_same_maps():
    from diffusion_pruning_amd.packed_train import adam8_code_map
    assert np.array_equal(adam8_code_map(True).numpy(), M.MAP_SIGNED)
    assert np.array_equal(adam8_code_map(False).numpy(), M.MAP_UNSIGNED)


# ---- the model's quantiser ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [True, False])
def test_model_quantiser(signed):
    q = M.MAP_SIGNED if signed else M.MAP_UNSIGNED
    assert np.array_equal(M.quantise(q, q.astype(np.float64)), np.arange(256))             # every code is its value's code
    rng = np.random.default_rng(3 + signed)
    x = rng.uniform(-1.0 if signed else 0.0, 1.0, 100000)
    x[:4] = [1.0, -1.0 if signed else 0.0, 0.0, 1e-9]
    codes = M.quantise(q, x)
    best = np.abs(x[:, None] - q.astype(np.float64)[None, :]).min(axis=1)                  # brute force over the whole map
    assert np.array_equal(np.abs(q.astype(np.float64)[codes] - x), best)
    assert np.array_equal(M.nearest_distance(q, x), best)


# ---- the model's step ----------------------------------------------------------------------------------------------------------------
def test_model_zero_block_stays_zero():
    n = 3 * M.BLOCK + 5
    rng = np.random.default_rng(0)
    g = rng.standard_normal(n)
    g[M.BLOCK:2 * M.BLOCK] = 0.0
    out = M.step(rng.standard_normal(n), g, *M.initial_state(n), 0)
    assert out["absmax_m"][1] == 0.0 and out["absmax_v"][1] == 0.0
    assert np.all(out["m8"][M.BLOCK:2 * M.BLOCK] == 127) and np.all(out["v8"][M.BLOCK:2 * M.BLOCK] == 0)
    assert all(np.isfinite(out[k]).all() for k in ("p", "m", "v", "absmax_m", "absmax_v"))
    assert np.all(out["absmax_m"][[0, 2, 3]] > 0) and out["absmax_m"].shape == (4,)
    # the block maximum has the code of 1.0 (255), and the first moment's may be the code of the most negative value instead
    blk = slice(0, M.BLOCK)
    assert out["v8"][blk].max() == 255 and (out["m8"][blk].max() == 255 or out["m8"][blk].min() == 0)


def test_model_nan_gradient_poisons_its_block_only():
    n = 3 * M.BLOCK
    rng = np.random.default_rng(1)
    p, g = rng.standard_normal(n), rng.standard_normal(n)
    clean = M.step(p, g, *M.initial_state(n), 4)
    g2 = g.copy()
    g2[M.BLOCK + 7] = np.nan
    out = M.step(p, g2, *M.initial_state(n), 4)
    assert np.isnan(out["absmax_m"][1]) and np.isnan(out["absmax_v"][1]) and np.isnan(out["p"][M.BLOCK + 7])
    for k in ("absmax_m", "absmax_v"):
        assert np.array_equal(out[k][[0, 2]], clean[k][[0, 2]])
    keep = np.r_[0:M.BLOCK, 2 * M.BLOCK:n]
    for k in ("p", "m8", "v8"):
        assert np.array_equal(out[k][keep], clean[k][keep])


def test_model_first_step_is_adamw():
    """zero state: p of the model = torch.optim.AdamW's first step, stated in fp64"""
    n = 700
    rng = np.random.default_rng(2)
    p, g = rng.standard_normal(n), rng.standard_normal(n) * 1e-3
    h = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)
    out = M.step(p, g, *M.initial_state(n), 0, **h)
    m, v = (1 - h["beta1"]) * g, (1 - h["beta2"]) * g * g
    ref = p * (1 - h["lr"] * h["weight_decay"]) - h["lr"] * (m / (1 - h["beta1"])) / (np.sqrt(v / (1 - h["beta2"])) + h["eps"])
    assert np.max(np.abs(out["p"] - ref)) <= 1e-14
    # and the stored state dequantises to the moments within half the widest gap of each map, times the block's scale
    m_back = M.dequantise(M.MAP_SIGNED, out["m8"], out["absmax_m"])
    v_back = M.dequantise(M.MAP_UNSIGNED, out["v8"], out["absmax_v"])
    assert np.all(np.abs(m_back - m) <= 7.1e-3 * np.repeat(out["absmax_m"], M.BLOCK)[:n])
    assert np.all(np.abs(v_back - v) <= 3.6e-3 * np.repeat(out["absmax_v"], M.BLOCK)[:n])


# ---- layout --------------------------------------------------------------------------------------------------------------------------
def test_ctypes_layout_of_the_adamw8_structs():
    from diffusion_pruning_amd import _lib
    structs = {"AptpAdamW8Item": _lib.AdamW8Item, "AptpAdamW8Params": _lib.AdamW8Params}
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
    assert ctypes.sizeof(_lib.AdamW8Item) == 64
    # AptpAdamWParams' fields first, at AptpAdamWParams' offsets
    for fname, _ in _lib.AdamWParams._fields_:
        assert getattr(_lib.AdamW8Params, fname).offset == getattr(_lib.AdamWParams, fname).offset, fname


@pytest.mark.parametrize("n", [-5, 0, 1, 4095, 4096, 4097, 2 ** 33])
def test_blocks_agree_with_the_fp32_pass(lib, n):
    assert lib.aptp_adamw8_blocks(n) == lib.aptp_adamw_blocks(n)


# ---- argument errors -----------------------------------------------------------------------------------------------------------------
def _good(n=4096):
    from diffusion_pruning_amd import _lib
    items = (_lib.AdamW8Item * 1)()
    it = items[0]
    it.p, it.g, it.m8, it.v8, it.absmax_m, it.absmax_v, it.shadow, it.n = 4096, 8192, 12288, 16384, 20480, 24576, 28672, n
    q = _lib.AdamW8Params()
    q.items_dev, q.starts_dev, q.step_dev, q.n_items, q.total_blocks = 4096, 4096, 4096, 1, (n + 4095) // 4096
    q.lr, q.beta1, q.beta2, q.eps, q.weight_decay = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    q.qmap_signed_dev, q.qmap_unsigned_dev = 4096, 8192
    q.items_host = ctypes.cast(items, ctypes.c_void_p)
    return q, items


BAD_PARAMS = [("items_dev", None, b"bad arguments"), ("starts_dev", None, b"bad arguments"), ("step_dev", None, b"bad arguments"),
              ("n_items", 0, b"bad arguments"), ("total_blocks", 0, b"bad arguments"),
              ("qmap_signed_dev", None, b"null code map"), ("qmap_unsigned_dev", None, b"null code map"),
              ("qmap_signed_dev", 4098, b"misaligned code map"),
              ("lr", -1.0, b"hyper-parameters"), ("beta1", 1.0, b"hyper-parameters"), ("beta2", -0.1, b"hyper-parameters"),
              ("eps", 0.0, b"hyper-parameters"), ("grad_scale", -1.0, b"grad_scale"), ("warmup_steps", -1.0, b"warmup_steps"),
              ("total_blocks", 2, b"total_blocks")]
BAD_ITEMS = [("n", 0, b"n must be"), ("n", -3, b"n must be"), ("p", None, b"null pointer"), ("m8", None, b"null pointer"),
             ("absmax_v", None, b"null pointer"), ("m8", 12289, b"code arrays"), ("v8", 16386, b"code arrays"),
             ("absmax_m", 20482, b"scale arrays"), ("absmax_v", 24577, b"scale arrays"), ("p", 4100, b"16-byte"),
             ("g", 8200, b"16-byte"), ("shadow", 28676, b"16-byte")]


def test_bad_arguments_return_an_error_without_launching(lib):
    """every refusal happens before the launch (null stream, made-up addresses: a launch would not come back clean)"""
    assert lib.aptp_adamw8_many(None, None, None) != 0
    for field, value, msg in BAD_PARAMS:
        q, items = _good()
        setattr(q, field, value)
        assert lib.aptp_adamw8_many(ctypes.byref(q), None, None) != 0 and msg in lib.aptp_last_error(), field
    for field, value, msg in BAD_ITEMS:
        q, items = _good()
        setattr(items[0], field, value)
        assert lib.aptp_adamw8_many(ctypes.byref(q), None, None) != 0 and msg in lib.aptp_last_error(), field
    q, items = _good()
    assert lib.aptp_adamw8_many(ctypes.byref(q), 4098, None) != 0 and b"grad_scale_dev" in lib.aptp_last_error()


# ---- the partition rule --------------------------------------------------------------------------------------------------------------
def test_partition_rule_and_state_bytes():
    from diffusion_pruning_amd import packed_train as PT
    assert PT.ADAM8_MIN_SIZE == M.MIN_8BIT_SIZE == 4096 and PT.ADAM8_BLOCK == M.BLOCK == 256
    assert not PT.adam8_uses_8bit(4095) and PT.adam8_uses_8bit(4096)
    assert not PT.adam8_uses_8bit(10 ** 6, optim_bits=32)
    assert PT.adam8_uses_8bit(100, min_8bit_size=100) and not PT.adam8_uses_8bit(99, min_8bit_size=100)
    sizes = [4095, 4096, 4097, 5]
    assert PT.adam_state_bytes(sizes, 32) == 8 * sum(sizes)
    # by hand: 4095 and 5 stay fp32; 4096 -> 2 * 4096 codes + 2 * 16 scales * 4 B; 4097 -> 2 * 4097 codes + 2 * 17 scales * 4 B
    assert PT.adam_state_bytes(sizes, 8) == 8 * 4095 + 8 * 5 + (8192 + 128) + (8194 + 136)
    assert PT.adam_state_bytes([396_000_000], 8) / 396e6 == pytest.approx(2.03125)
