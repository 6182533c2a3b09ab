"""CPU checks of the learning-rate schedules: the plain-Python model (tests/lr_schedule_model.py) against
transformers.optimization.get_scheduler, packed_train.LrSchedule and csrc/lr_schedule.h (compiled for the host) against the model,
LrSchedule's validation, and train_step.scaled_lr."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import lr_schedule_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_LR = 2e-4          # the rate of the one parameter group; the optimizer's default rate is M.LR_INIT, as in the reference's runs


def _oracle(kind, W, T, kw, steps):
    """get_last_lr()[0] before any scheduler.step() and after each of `steps` of them: the rate at k = 0 .. steps"""
    from transformers.optimization import get_scheduler
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([{"params": [p], "lr": GROUP_LR}], lr=M.LR_INIT)
    spec = {k: (int(v) if k == "num_cycles" else v) for k, v in kw.items()}
    sched = get_scheduler(kind, opt, num_warmup_steps=W, num_training_steps=T, scheduler_specific_kwargs=spec or None)
    out = [sched.get_last_lr()[0]]
    for _ in range(steps):
        opt.step()
        sched.step()
        out.append(sched.get_last_lr()[0])
    return out


@pytest.mark.parametrize("kind", M.KINDS)
def test_model_matches_transformers(kind):
    """the expressions are the library's, so fp64 equality is expected; 4 ulp of fp64 are allowed"""
    worst = 0
    for _, W, T, kw in [g for g in M.grid() if g[0] == kind]:
        want = _oracle(kind, W, T, kw, max(M.GRID_STEPS))
        for k in M.GRID_STEPS:
            got = GROUP_LR * M.multiplier(kind, k, W, T, **kw)
            d = M.ulps64(got, want[k])
            worst = max(worst, d)
            assert d <= 4, (kind, W, T, kw, k, got, want[k])
    print(f"{kind}: worst distance to transformers {worst} ulp of fp64")


def test_lr_schedule_class_is_the_model():
    from diffusion_pruning_amd.packed_train import LrSchedule
    for kind, W, T, kw in M.grid():
        s = LrSchedule(kind, warmup_steps=W, training_steps=T, **kw)
        for k in M.GRID_STEPS:
            assert s.multiplier(k) == M.multiplier(kind, k, W, T, **kw), (kind, W, T, kw, k)
            for lr in (GROUP_LR, 1e-5, 0.1):
                a, b = np.float32(s.rate(lr, k)), M.rate(kind, lr, k, W, T, **kw)
                assert a.tobytes() == np.float32(b).tobytes(), (kind, W, T, kw, k, lr, a, b)
    # the defaults of the library
    assert LrSchedule("cosine", 0, 10).num_cycles == 0.5 and LrSchedule("cosine_with_restarts", 0, 10).num_cycles == 1.0
    p = LrSchedule("polynomial", 0, 10)
    assert (p.power, p.lr_end, p.lr_init) == (1.0, 1e-7, 1e-3)
    # the cosine rises again past T: the library's behaviour
    c = LrSchedule("cosine", 2, 6)
    assert c.multiplier(6) < 1e-30 and c.multiplier(8) > 0.1
    # constant_with_warmup is the older warm-up's expression
    w = LrSchedule("constant_with_warmup", 4)
    assert [w.rate(1e-2, k) for k in range(6)] == [float(np.float32(1e-2) * min(np.float32(1), np.float32(k) / np.float32(4))) for k in range(6)]


def test_lr_schedule_validation_and_round_trip():
    from diffusion_pruning_amd.packed_train import LrSchedule, as_lr_schedule
    with pytest.raises(ValueError, match="piecewise_constant"):
        LrSchedule("piecewise_constant")
    with pytest.raises(ValueError, match="unknown lr_scheduler"):
        LrSchedule("inverse_sqrt")
    for kind in ("linear", "cosine", "cosine_with_restarts", "polynomial"):
        with pytest.raises(ValueError, match="training_steps"):
            LrSchedule(kind, warmup_steps=2)
        with pytest.raises(ValueError):
            LrSchedule(kind, warmup_steps=5, training_steps=4)
    for bad in (dict(name="constant_with_warmup", warmup_steps=-1), dict(name="linear", warmup_steps=0, training_steps=1 << 24),
                dict(name="cosine", training_steps=10, num_cycles=0), dict(name="cosine_with_restarts", training_steps=10, num_cycles=1.5),
                dict(name="polynomial", training_steps=10, power=0.0), dict(name="polynomial", training_steps=10, lr_end=1e-3),
                dict(name="polynomial", training_steps=10, lr_end=1e-4, lr_init=1e-5), dict(name="polynomial", warmup_steps=4, training_steps=4)):
        with pytest.raises(ValueError):
            LrSchedule(**bad)
    assert LrSchedule("linear", 4, 4).multiplier(4) == 0.0           # T == W is the library's max(1, T - W)
    for kind, W, T, kw in M.grid():
        s = LrSchedule(kind, warmup_steps=W, training_steps=T, **kw)
        d = s.as_dict()
        assert set(d) == {"name", "warmup_steps", "training_steps", "num_cycles", "power", "lr_end", "lr_init"}
        t = LrSchedule(**d)
        assert t == s and t.as_dict() == d and as_lr_schedule(d) == s and as_lr_schedule(s) is s
    assert as_lr_schedule(None) is None


def test_scaled_lr_is_the_reference_rule():
    from diffusion_pruning_amd.train_step import scaled_lr
    for lr, batch, accum, world in ((1e-5, 16, 4, 8), (2e-4, 64, 1, 1), (1e-3, 3, 2, 5)):
        # pdm/training/trainer.py:806-812 and 1521-1527: scaling_factor = accumulation * batch * processes; lr * sqrt(scaling_factor)
        scaling_factor = accum * batch * world
        assert scaled_lr(lr, batch, accum, world) == lr * math.sqrt(scaling_factor)
    assert scaled_lr(1e-5, 4) == 1e-5 * math.sqrt(4)


HOST_MAIN = r"""
#include <cstdio>
#include <cstring>
#include "lr_schedule.h"
int main() {
  int kind, W, T; double nc, power; float lr, k;
  while (std::scanf("%d %d %d %lf %lf %f %f", &kind, &W, &T, &nc, &power, &lr, &k) == 7) {
    AptpLrsCurve c{kind, (double)W, (double)T, nc, power, 1e-7, 1e-3};
    if (aptp_lrs_invalid(c)) { std::printf("invalid\n"); continue; }
    const float r = aptp_lrs_rate(c, lr, k);
    const double m = aptp_lrs_multiplier(c, (double)k);
    unsigned ru; unsigned long long mu;
    std::memcpy(&ru, &r, 4); std::memcpy(&mu, &m, 8);
    std::printf("%08x %016llx\n", ru, mu);
  }
  return 0;
}
"""


def test_header_on_the_host_is_the_model():
    """csrc/lr_schedule.h through the host compiler: the warm-up ramps, constant, constant_with_warmup and linear bit for bit; the
    cosines and polynomial bit for bit in m when the C library's cos / pow are Python's (they are the same libm), and within 1 ulp
    of fp32 in the rate in any case"""
    from diffusion_pruning_amd import _lib
    rows, lines = [], []
    for kind, W, T, kw in M.grid():
        nc = kw.get("num_cycles", 1 if kind == "cosine_with_restarts" else 0.5)
        for k in M.GRID_STEPS:
            rows.append((kind, W, T, kw, k))
            lines.append(f"{_lib.LR_KINDS[kind]} {W} {T} {float(nc)!r} {float(kw.get('power', 1.0))!r} {GROUP_LR!r} {float(k)!r}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "m.cpp"), os.path.join(d, "m")
        open(src, "w").write(HOST_MAIN)
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "diffusion_pruning_amd", "csrc"),
                        "-o", exe, src], check=True)
        run = lambda text: subprocess.run([exe], input=text + "\n", check=True, capture_output=True, text=True).stdout      # noqa: E731
        out = run("\n".join(lines)).split("\n")
        # what the kernel's entry point refuses, from the same function
        bad = ["7 0 10 0.5 1.0 1e-3 0.0", "2 5 4 0.5 1.0 1e-3 0.0", "3 0 10 0.0 1.0 1e-3 0.0", "5 0 10 0.5 0.0 1e-3 0.0",
               "5 4 4 0.5 1.0 1e-3 0.0", "1 -1 0 0.5 1.0 1e-3 0.0", "2 0 16777216 0.5 1.0 1e-3 0.0"]
        assert run("\n".join(bad)).split() == ["invalid"] * len(bad)
    assert len(out) >= len(rows)
    for (kind, W, T, kw, k), line in zip(rows, out):
        r_hex, m_hex = line.split()
        got_r = np.array([int(r_hex, 16)], dtype=np.uint32).view(np.float32)[0]
        got_m = np.array([int(m_hex, 16)], dtype=np.uint64).view(np.float64)[0]
        want_r, want_m = M.rate(kind, GROUP_LR, k, W, T, **kw), M.multiplier(kind, k, W, T, **kw)
        exact = kind in ("constant", "constant_with_warmup", "linear") or k < W
        assert M.ulps32(got_r, want_r) <= (0 if exact else 1), (kind, W, T, kw, k, got_r, want_r)
        assert M.ulps64(got_m, want_m) <= (0 if exact else 4), (kind, W, T, kw, k, got_m, want_m)
