"""CPU checks of the gradient-accumulation window and the learning-rate warm-up (csrc/optim.hip): the two parameter blocks
have the C compiler's layout, the exported grid size of aptp_grad_accumulate follows its block size, argument validation
fails without launching, and the warm-up factor is `constant_with_warmup` counted in optimizer steps."""
import ctypes
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aptp_hip.h")
ELEMS_PER_BLOCK = 4096            # csrc/optim.hip: 256 threads x 4 float4 per trip


@pytest.fixture(scope="module")
def lib():
    from diffusion_pruning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_param_blocks_match_the_c_header():
    from diffusion_pruning_amd import _lib
    structs = {"AptpGradAccumParams": _lib.GradAccumParams, "AptpAdamWParams": _lib.AdamWParams}
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        body.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            body.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    body.append('printf("modes %d %d %d\\n", APTP_GRAD_ACCUM_STORE, APTP_GRAD_ACCUM_ADD, APTP_GRAD_ACCUM_FINAL);')
    body.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(body))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    lines = [line.split() for line in out.strip().splitlines()]
    got = {k[0]: k[1] for k in lines if len(k) == 2}
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert _lib.AdamWParams._fields_[-1][0] == "warmup_steps"              # appended: the earlier fields keep their offsets
    modes = [k for k in lines if k[0] == "modes"][0][1:]
    assert [int(m) for m in modes] == [_lib.GRAD_ACCUM_STORE, _lib.GRAD_ACCUM_ADD, _lib.GRAD_ACCUM_FINAL]


@pytest.mark.parametrize("n", [0, 1, 4096, 4097, 2 ** 33])
def test_grad_accumulate_blocks(lib, n):
    """the grid covers n with trips of ELEMS_PER_BLOCK elements per block: never more blocks than trips, one block per trip
    while the range is small, and a bounded grid (the rest is a grid stride) for an arena beyond 2^31 elements"""
    b = lib.aptp_grad_accumulate_blocks(n)
    trips = (n + ELEMS_PER_BLOCK - 1) // ELEMS_PER_BLOCK
    if n == 0:
        assert b == 0
        return
    assert 1 <= b <= trips
    if n <= 4097:
        assert b == trips
    assert b <= 1 << 16                      # a launch of the whole arena stays a few waves of resident blocks
    assert lib.aptp_grad_accumulate_blocks(-5) == 0


def test_grad_accumulate_validation_does_not_launch(lib):
    from diffusion_pruning_amd import _lib
    p = _lib.GradAccumParams()
    assert lib.aptp_grad_accumulate(ctypes.byref(p), None) != 0 and b"null pointer" in lib.aptp_last_error()
    p.acc, p.g, p.n, p.mode = 4096, 8192, 0, 0
    assert lib.aptp_grad_accumulate(ctypes.byref(p), None) != 0 and b"n must be" in lib.aptp_last_error()
    p.n, p.mode = 8, 3
    assert lib.aptp_grad_accumulate(ctypes.byref(p), None) != 0 and b"mode" in lib.aptp_last_error()
    p.mode, p.g = 1, 8192 + 4
    assert lib.aptp_grad_accumulate(ctypes.byref(p), None) != 0 and b"aligned" in lib.aptp_last_error()
    q = _lib.AdamWParams()
    q.items_dev, q.starts_dev, q.step_dev, q.n_items, q.total_blocks = 4096, 4096, 4096, 1, 1
    q.lr, q.beta1, q.beta2, q.eps, q.warmup_steps = 1e-3, 0.9, 0.999, 1e-8, -1.0
    assert lib.aptp_adamw_many(ctypes.byref(q), None) != 0 and b"warmup_steps" in lib.aptp_last_error()


def warmup_factor(step: int, W: int) -> float:
    """the kernel's factor on lr at the step that follows `step` applied ones (0 = no warm-up)"""
    return 1.0 if W <= 0 else min(1.0, step / W)


def test_warmup_factor_is_constant_with_warmup():
    assert [warmup_factor(k, 4) for k in range(6)] == [0.0, 0.25, 0.5, 0.75, 1.0, 1.0]
    assert [warmup_factor(k, 0) for k in range(3)] == [1.0, 1.0, 1.0]
    # diffusers' get_constant_schedule_with_warmup: LambdaLR(lambda k: k / max(1, W) if k < W else 1)
    lam = lambda k, W: float(k) / float(max(1.0, W)) if k < W else 1.0          # noqa: E731
    for W in (1, 4, 250):
        assert all(warmup_factor(k, W) == lam(k, W) for k in range(0, 2 * W + 2))
