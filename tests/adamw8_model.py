"""The block-wise 8-bit AdamW state of csrc/optim8.hip, stated in numpy: THE definition of the format.

It follows the published construction of the block-wise "dynamic" 8-bit maps of bitsandbytes; that library is not a
dependency and equality with it is neither claimed nor tested.  Two maps of 256 fp32 values (signed for the first moment,
unsigned for the second), quantisation blocks of 256 consecutive elements of a tensor with one fp32 absmax per moment,
moment = map[code] * absmax.  One step dequantises, applies the AdamW element of csrc/packed_pass.h (p moves by the
UNQUANTISED new moments) and quantises the new moments; everything here is fp64 apart from the maps' values, which are the
fp32 numbers the kernel reads.  A value exactly between two map values may take either code: nothing pins ties."""
import numpy as np

BLOCK = 256               # elements per quantisation block
MIN_8BIT_SIZE = 4096      # tensors below this keep fp32 moments (also the elements of one workgroup of the kernel)
ZERO_SIGNED, ZERO_UNSIGNED = 127, 0
DEFAULTS = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)


def _decades(signed):
    vals = []
    for i in range(7):
        k = 2 ** i if signed else 2 ** (i + 1)
        edges = np.linspace(0.1, 1.0, k + 1, dtype=np.float64)
        mid = (edges[:-1] + edges[1:]) / 2.0 * 10.0 ** (i - 6)
        vals += mid.tolist()
        if signed:
            vals += (-mid).tolist()
    return vals


def make_map(signed):
    """256 ascending fp32 values: built in fp64, rounded to fp32, sorted"""
    vals = np.asarray(_decades(signed) + [0.0, 1.0], dtype=np.float64).astype(np.float32)
    vals = np.sort(vals)
    assert vals.shape == (256,)
    return vals


MAP_SIGNED, MAP_UNSIGNED = make_map(True), make_map(False)


def nearest_distance(qmap, x):
    """distance from every x to the nearest map value (fp64)"""
    q = qmap.astype(np.float64)
    x = np.asarray(x, dtype=np.float64)
    i = np.clip(np.searchsorted(q, x), 1, 255)
    return np.minimum(np.abs(x - q[i - 1]), np.abs(q[i] - x))


def quantise(qmap, x):
    """a nearest code for every x (fp64 comparison against the fp32 map values)"""
    q = qmap.astype(np.float64)
    x = np.asarray(x, dtype=np.float64)
    i = np.clip(np.searchsorted(q, x), 1, 255)
    return np.where(np.abs(q[i] - x) < np.abs(x - q[i - 1]), i, i - 1).astype(np.uint8)


def n_blocks(n):
    return (int(n) + BLOCK - 1) // BLOCK


def dequantise(qmap, codes, absmax):
    """fp64 moments of one tensor: map[code] * absmax of the element's block"""
    codes = np.asarray(codes).reshape(-1)
    scale = np.repeat(np.asarray(absmax, dtype=np.float64), BLOCK)[:codes.size]
    return qmap.astype(np.float64)[codes] * scale


def quantise_blocks(qmap, x, zero_code):
    """(codes uint8 [n], absmax fp64 [ceil(n / 256)]) of the new moment x of one tensor.  absmax == 0: the zero code, no
    division; a block with a non-finite value: absmax NaN (its codes mean nothing: zero code here)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    nb = n_blocks(x.size)
    rows = np.zeros(nb * BLOCK, dtype=np.float64)                   # (the short last block: padded with zeros, which change no max)
    rows[:x.size] = x
    rows = rows.reshape(nb, BLOCK)
    poisoned = ~np.isfinite(rows).all(axis=1)
    with np.errstate(invalid="ignore"):
        absmax = np.where(poisoned, np.nan, np.abs(rows).max(axis=1))
    live = ~poisoned & (absmax > 0.0)
    codes = np.full((nb, BLOCK), zero_code, dtype=np.uint8)
    codes[live] = quantise(qmap, rows[live] / absmax[live, None])
    return codes.reshape(-1)[:x.size], absmax


def warmup_lr(lr, applied, warmup):
    return lr * min(1.0, applied / warmup) if warmup > 0 else lr


def adamw_element(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale=1.0, warmup_steps=0):
    """csrc/packed_pass.h's adamw_element in fp64 for the step that follows `step` applied ones -> (p, m, v)"""
    t = step + 1.0
    lr = warmup_lr(lr, step, warmup_steps)
    g = np.asarray(g, dtype=np.float64) * grad_scale
    p = np.asarray(p, dtype=np.float64) * (1.0 - lr * weight_decay)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    with np.errstate(invalid="ignore", divide="ignore"):
        p = p - (lr / (1.0 - beta1 ** t)) * m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps)
    return p, m, v


def step(p, g, m8, v8, absmax_m, absmax_v, step_count, **hyper):
    """one step on one tensor -> dict(p, m, v: fp64 unquantised results; m8, v8, absmax_m, absmax_v: the new state)"""
    h = dict(DEFAULTS)
    h.update(hyper)
    m0 = dequantise(MAP_SIGNED, m8, absmax_m)
    v0 = dequantise(MAP_UNSIGNED, v8, absmax_v)
    with np.errstate(invalid="ignore"):
        p1, m1, v1 = adamw_element(np.asarray(p).reshape(-1), np.asarray(g).reshape(-1), m0, v0, float(step_count), **h)
    cm, am = quantise_blocks(MAP_SIGNED, m1, ZERO_SIGNED)
    cv, av = quantise_blocks(MAP_UNSIGNED, v1, ZERO_UNSIGNED)
    return dict(p=p1, m=m1, v=v1, m8=cm, v8=cv, absmax_m=am, absmax_v=av)


def initial_state(n):
    """(m8, v8, absmax_m, absmax_v) of a fresh tensor of n elements: zero codes (127 for the first moment), zero scales"""
    return (np.full(n, ZERO_SIGNED, np.uint8), np.full(n, ZERO_UNSIGNED, np.uint8),
            np.zeros(n_blocks(n)), np.zeros(n_blocks(n)))
