"""The seeded normal stream on the host: the numpy oracle (tests/philox_oracle.py) against the Random123 known answers, the
kernel's own header (csrc/philox_normal.h) compiled for the CPU against the oracle, and the statistics of the oracle's stream.

Bound of the normals, as tests/test_philox_gpu.py derives it: the uniforms are exact, |z| <= sqrt(48 ln 2) = 5.77, the fp32
logf / sqrtf / sin / cos are good to 1-2 ulp, so a few ulp of the factors stays under ~2e-6; the bound is twice that."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import philox_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "diffusion_pruning_amd", "csrc", "philox_normal.h")
NORMAL_TOL = 4e-6

# Random123's kat_vectors for philox4x32, 10 rounds: (counter, key, output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
TRIPLES = [(0, 0, 0), (1234, 1, 0), (1234, 1, 3), (2 ** 63 - 1, 2 ** 40 + 3, 2 ** 34 - 4), (-1, 2 ** 32, 5)]   # (seed, draw, offset)
N_PROBE = 13


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_oracle_reproduces_the_known_answers(ctr, key, want):
    got = [int(v) for v in PO.philox4x32_10(ctr, key)]
    assert got == list(want), [hex(v) for v in got]


def test_oracle_maps_seed_draw_and_element_as_defined():
    """element g of (seed, draw) is word g & 3 of the block with counter (g >> 2, draw) and key seed, 64 bits each"""
    seed, draw, off = 0x299f31d0a4093822, 0x0370734413198a2e, 2 ** 34 - 4
    got = PO.bits(seed, draw, off, 8)
    for e in range(8):
        g = off + e
        x = PO.philox4x32_10((g >> 2 & 0xffffffff, g >> 34, draw & 0xffffffff, draw >> 32), (seed & 0xffffffff, seed >> 32))
        assert int(got[e]) == int(x[g & 3])
    assert (2 ** 34 - 4) >> 34 == 0 and (2 ** 34) >> 34 == 1               # the carry into the high word is inside these 8
    # a negative seed is its two's complement
    assert np.array_equal(PO.bits(-1, 0, 0, 8), PO.bits(2 ** 64 - 1, 0, 0, 8))


def test_header_compiled_for_the_cpu_matches_the_oracle(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    body = ['#include <stdio.h>', '#include <inttypes.h>', f'#include "{HEADER}"', "int main(void){", "uint32_t x[4]; float z[4];"]
    for ctr, key, _ in KAT:
        body.append("x[0]=%uu;x[1]=%uu;x[2]=%uu;x[3]=%uu; aptp_philox4x32_10(x,%uu,%uu);" % (ctr + key))
        body.append('printf("K %08x %08x %08x %08x\\n", x[0], x[1], x[2], x[3]);')
    for seed, draw, off in TRIPLES:
        body.append("for (uint64_t e = 0; e < %d; ++e) { uint64_t g = %dull + e; aptp_philox_block(%dull, %dull, g >> 2, x);"
                    % (N_PROBE, off, seed & (2 ** 64 - 1), draw))
        body.append("aptp_philox_normals4(x, z);")
        body.append('printf("E %08x %.9g %.9g\\n", x[g & 3], (double)z[g & 3], (double)aptp_philox_normal1(x, (int)(g & 3))); }')
    body.append("return 0;}")
    src, exe = tmp_path / "p.cpp", tmp_path / "p"
    src.write_text("\n".join(body))
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", str(exe), str(src), "-lm"], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    kat = [ln.split()[1:] for ln in lines if ln.startswith("K")]
    assert kat == [["%08x" % v for v in want] for _, _, want in KAT]
    elems = [ln.split()[1:] for ln in lines if ln.startswith("E")]
    assert len(elems) == len(TRIPLES) * N_PROBE
    worst = 0.0
    for t, (seed, draw, off) in enumerate(TRIPLES):
        rows = elems[t * N_PROBE:(t + 1) * N_PROBE]
        assert [int(r[0], 16) for r in rows] == [int(v) for v in PO.bits(seed, draw, off, N_PROBE)]
        ref = PO.normals(seed, draw, off, N_PROBE)
        assert [r[1] for r in rows] == [r[2] for r in rows]                # the single-element path gives the same values
        worst = max(worst, float(np.abs(np.array([float(r[1]) for r in rows]) - ref).max()))
    print(f"host header vs oracle: max abs error {worst:.3e}")
    assert worst <= NORMAL_TOL


N_STAT = 2 ** 20
PAIRS = [(0, 0), (1234, 0), (1234, 1), (2 ** 63 - 1, 7), (7, 0), (11, 3)]
_Z = {}


def z_of(seed, draw):
    if (seed, draw) not in _Z:
        _Z[(seed, draw)] = PO.normals(seed, draw, 0, N_STAT)
    return _Z[(seed, draw)]


def corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("seed,draw", PAIRS)
def test_statistics_of_the_stream(seed, draw):
    """each statistic in units of its own standard error under N(0, 1): the inputs are fixed, so nothing is left to chance"""
    z, N = z_of(seed, draw), N_STAT
    d = z - z.mean()
    var = float((d * d).mean())
    stats = {"mean": abs(float(z.mean())) * np.sqrt(N), "var": abs(var - 1.0) * np.sqrt(N / 2),
             "kurtosis": abs(float((d ** 4).mean()) / var ** 2 - 3.0) * np.sqrt(N / 24),
             "lag1": abs(corr(z[:-1], z[1:])) * np.sqrt(N)}
    print(seed, draw, {k: round(float(v), 3) for k, v in stats.items()})
    assert np.isfinite(z).all() and float(np.abs(z).max()) <= np.sqrt(48 * np.log(2.0))
    for k, v in stats.items():
        assert v <= 4.0, (k, v)


def test_draws_and_seeds_are_uncorrelated():
    a = abs(corr(z_of(1234, 0), z_of(1234, 1))) * np.sqrt(N_STAT)
    b = abs(corr(z_of(1234, 0), PO.normals(1235, 0, 0, N_STAT))) * np.sqrt(N_STAT)
    print(f"draw 0 vs 1: {a:.3f}, seed 1234 vs 1235: {b:.3f}")
    assert a <= 4.0 and b <= 4.0


# ---- the C ABI of aptp_philox_normal ------------------------------------------------------------------------------------------
def test_philox_ctypes_layout_matches_the_c_header(tmp_path):
    import ctypes
    from diffusion_pruning_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    header = os.path.join(ROOT, "include", "aptp_hip.h")
    cls = _lib.PhiloxNormalParams
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){",
            'printf("%zu\\n", sizeof(AptpPhiloxNormalParams));']
    for fname, _ in cls._fields_:
        body.append(f'printf("%zu\\n", offsetof(AptpPhiloxNormalParams, {fname}));')
    body.append('printf("%d %d %d\\n", (int)APTP_PHILOX_F32, (int)APTP_PHILOX_BF16, (int)APTP_PHILOX_RAW);')
    body.append("return 0;}")
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(body))
    subprocess.run([cc, "-std=c99", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(cls)
    assert [int(v) for v in out[1:1 + len(cls._fields_)]] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert [int(v) for v in out[-3:]] == [_lib.PHILOX_F32, _lib.PHILOX_BF16, _lib.PHILOX_RAW]


def test_philox_refuses_before_launching():
    """made-up addresses: every refusal returns APTP_EINVAL (-1) with its reason before anything is launched"""
    import ctypes
    from diffusion_pruning_amd import _lib
    lib = _lib.load()

    def refused(needle, **kw):
        p = _lib.PhiloxNormalParams()
        p.out, p.seeds_dev, p.n, p.b, p.out_kind, p.scale = 0x10000, 0x20000, 64, 2, _lib.PHILOX_F32, 1.0
        for k, v in kw.items():
            setattr(p, k, v)
        assert lib.aptp_philox_normal(ctypes.byref(p), None) == -1
        assert needle in lib.aptp_last_error(), lib.aptp_last_error()

    assert lib.aptp_philox_normal(None, None) == -1 and b"null pointer" in lib.aptp_last_error()
    refused(b"null pointer", out=None)
    refused(b"null pointer", seeds_dev=None)
    refused(b"unknown out_kind", out_kind=3)
    refused(b"bad extents", n=0)
    refused(b"bad extents", b=0)
    refused(b"bad extents", b=65536)
    refused(b"bad extents", n=(1 << 40))
    refused(b"offset", offset=-1)
    refused(b"draw", draw=-1)
    refused(b"raw words", out_kind=_lib.PHILOX_RAW, base=0x30000)
    refused(b"raw words", out_kind=_lib.PHILOX_RAW, scale_dev=0x30000)
    refused(b"alignment", out=0x10002)
    refused(b"alignment", out=0x10001, out_kind=_lib.PHILOX_BF16)
    refused(b"alignment", seeds_dev=0x20004)
    refused(b"alignment", draw_dev=0x30004)
    refused(b"alignment", scale_dev=0x30002)
    refused(b"alignment", base=0x30002)
