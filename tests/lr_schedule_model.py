"""The definition of the device-side learning-rate schedules (csrc/lr_schedule.h, packed_train.LrSchedule) in plain
Python: m(k) in fp64, expression by expression as transformers.optimization evaluates it, and the rule by which a rate is stored
as fp32.  tests/test_lr_schedule_host.py holds it against transformers' get_scheduler; the GPU tests hold the kernel against it.

k = applied optimizer steps so far: the step that follows runs at lr * m(k).  W = num_warmup_steps, T = num_training_steps."""
import math

import numpy as np

KINDS = ("constant", "constant_with_warmup", "linear", "cosine", "cosine_with_restarts", "polynomial")
GRID_WT = ((0, 10), (3, 10), (9, 10), (3, 4))
GRID_STEPS = range(13)                    # 0 .. 12: k = T and k > T are covered for every (W, T)
LR_INIT = 1e-3                            # torch.optim.AdamW's default rate: what `polynomial` divides by in the reference's runs


def multiplier(kind, k, W=0, T=0, num_cycles=None, power=1.0, lr_end=1e-7, lr_init=LR_INIT):
    k, W, T = float(k), float(W), float(T)
    if kind == "constant":
        return 1.0
    if k < W:
        return k / max(1.0, W)
    if kind == "constant_with_warmup":
        return 1.0
    if kind == "linear":
        return max(0.0, (T - k) / max(1.0, T - W))
    prog = (k - W) / max(1.0, T - W)
    if kind == "cosine":
        nc = 0.5 if num_cycles is None else float(num_cycles)
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * nc * 2.0 * prog)))
    if kind == "cosine_with_restarts":
        nc = 1.0 if num_cycles is None else float(num_cycles)
        if prog >= 1.0:
            return 0.0
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((nc * prog) % 1.0))))
    if kind == "polynomial":
        if k > T:
            return lr_end / lr_init
        pct = 1.0 - (k - W) / (T - W)
        return ((lr_init - lr_end) * pct ** power + lr_end) / lr_init
    raise ValueError(kind)


def rate(kind, lr, k, W=0, T=0, **kw):
    """the fp32 value stored for the fp32 base rate lr: (float)((double)lr * m), except constant (lr itself) and
    constant_with_warmup (the fp32 expression of the older warm-up path, lr * min(1, k / W))"""
    lr = np.float32(lr)
    if kind == "constant":
        return lr
    if kind == "constant_with_warmup":
        return lr * min(np.float32(1.0), np.float32(k) / np.float32(W)) if W > 0 else lr
    return np.float32(float(lr) * multiplier(kind, k, W, T, **kw))


def variants(kind):
    """the keyword sets the grid runs a kind with"""
    if kind == "cosine_with_restarts":
        return [dict(num_cycles=1), dict(num_cycles=2)]
    if kind == "polynomial":
        return [dict(power=1.0), dict(power=2.0)]
    return [dict()]


def grid():
    """(kind, W, T, kw) of every curve of the grid"""
    return [(kind, W, T, kw) for kind in KINDS for (W, T) in GRID_WT for kw in variants(kind)]


def ulps32(a, b):
    """distance of two finite fp32 values in units in the last place (0 = the same bits, +0 == -0 aside)"""
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    ia, ib = (x if x >= 0 else -(x & 0x7FFFFFFF) for x in (ia, ib))
    return abs(ia - ib)


def ulps64(a, b):
    ia, ib = (int(np.float64(x).view(np.int64)) for x in (a, b))
    ia, ib = (x if x >= 0 else -(x & 0x7FFFFFFFFFFFFFFF) for x in (ia, ib))
    return abs(ia - ib)
