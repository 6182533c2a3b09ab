"""fp64 statement of aptp_ema_many (csrc/ema.hip): the decay rule of diffusers' EMAModel and one update.  tests/test_ema_host.py
holds it against hand values, tests/test_ema_gpu.py holds the kernel and packed_train.PackedEMA against it."""
import numpy as np

DEFAULTS = dict(decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2.0 / 3.0)


def ema_decay(count, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2.0 / 3.0):
    """the decay of the update that follows `count` applied ones"""
    n = float(count) + 1.0
    s = max(0.0, n - float(update_after_step) - 1.0)
    if s <= 0.0:
        return 0.0
    base = 1.0 - (1.0 + s / float(inv_gamma)) ** (-float(power)) if use_ema_warmup else (1.0 + s) / (10.0 + s)
    return max(float(min_decay), min(base, float(decay)))


def ema_update(ema, p, count, **kw):
    """(new ema, decay) of one applied update; ema and p are arrays of any float type, the result is fp64"""
    d = ema_decay(count, **kw)
    ema, p = np.asarray(ema, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return ema - (1.0 - d) * (ema - p), d


def ema_trajectory(p0, masters, **kw):
    """the average after every update of a run that starts as a clone of p0 and sees `masters` one after the other"""
    ema, out = np.asarray(p0, dtype=np.float64), []
    for k, p in enumerate(masters):
        ema, _ = ema_update(ema, p, k, **kw)
        out.append(ema)
    return out
