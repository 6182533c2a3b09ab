"""numpy fp64 restatement of the seeded training batch (csrc/train_noise.h) on top of tests/philox_oracle.py.  The fp32
inputs (moments or latents, the [T, 2] table) are taken as given, the host scalars as the fp32 values the kernel receives.

Sub-draw k of a call with draw d is Philox draw 8 d + k of the sample's seed:
    k = 0  words x0, x1, x2 of block 0: top = (x0 (H1 - R + 1)) >> 32, left = (x1 (W1 - R + 1)) >> 32, flip = x2 >> 31
    k = 1  posterior eps, k = 2 noise, k = 4 input perturbation: element e = c hw + y w + x of the sample's [4, h, w]
    k = 3  offset noise: element c;      k = 5  timestep: t = (x0 T) >> 32, x0 word 0 of block 0
    x0 = s (mean + exp(0.5 clamp(logvar, -30, 20)) z1) | latents;  n = z2 + noise_offset z3[c];  m = n + input_perturbation z4
    noisy = sa x0 + so m;  target = n (epsilon) | sa n - so x0 (v_prediction),  (sa, so) = table[t]

``sample`` also returns the per-element tolerances the issue derives (u = 2^-24, delta = 4e-6 the bound on a device normal):
    E_x0 = |s| sigma (delta + 4u |z1|) + 3u |s| (|mean| + sigma |z1|)            (0 with latents given)
    E_n  = delta (1 + |noise_offset|) + 2u (|z2| + |noise_offset z3|)
    E_m  = E_n + |input_perturbation| delta + 2u (|n| + |input_perturbation z4|)
    tol(noisy)  = 2 (sa E_x0 + so E_m + 3u (|sa x0| + |so m|))
    tol(target) = 2 E_n (epsilon) | 2 (sa E_n + so E_x0 + 3u (|sa n| + |so x0|)) (v);   tol(latents) = 2 E_x0, tol(noise) = 2 E_n"""
import numpy as np

from tests import philox_oracle as PO

U = 2.0 ** -24
DELTA = 4e-6
SUBDRAWS = 8


def subdraw(draw, k):
    return SUBDRAWS * int(draw) + k


def words_of_seeds(seeds, draw, block=0):
    """uint32 [len(seeds), 4]: the words of one block for many seeds (the key vectorised; philox_oracle's takes one key)"""
    key = np.array([int(s) & (2 ** 64 - 1) for s in seeds], dtype=np.uint64)
    k0, k1 = key & PO.MASK, key >> PO.S32
    one = np.ones_like(key)
    c = [one * np.uint64(block & 0xFFFFFFFF), one * np.uint64(block >> 32), one * np.uint64(draw & 0xFFFFFFFF),
         one * np.uint64(draw >> 32)]
    for _ in range(10):
        p0, p1 = PO.M0 * c[0], PO.M1 * c[2]
        c = [(p1 >> PO.S32) ^ c[1] ^ k0, p1 & PO.MASK, (p0 >> PO.S32) ^ c[3] ^ k1, p0 & PO.MASK]
        k0, k1 = (k0 + np.uint64(PO.W0)) & PO.MASK, (k1 + np.uint64(PO.W1)) & PO.MASK
    return np.stack(c, 1).astype(np.uint32)


def timestep(seed, draw, T):
    return (int(PO.bits(seed, subdraw(draw, 5), 0, 1)[0]) * int(T)) >> 32


def timesteps_of_seeds(seeds, draw, T):
    return (words_of_seeds(seeds, subdraw(draw, 5))[:, 0].astype(np.uint64) * np.uint64(T)) >> np.uint64(32)


def crop_flip(seed, draw, H1, W1, R, center_crop=False, random_flip=True):
    x = [int(v) for v in PO.bits(seed, subdraw(draw, 0), 0, 4)]
    if center_crop:
        top, left = int(round((H1 - R) / 2.0)), int(round((W1 - R) / 2.0))
    else:
        top, left = (x[0] * (H1 - R + 1)) >> 32, (x[1] * (W1 - R + 1)) >> 32
    return top, left, (x[2] >> 31) if random_flip else 0


def sample(seed, draw, table, *, moments=None, latents=None, scale=1.0, noise_offset=0.0, input_perturbation=0.0,
           prediction="v_prediction"):
    """one sample: moments fp32 [8, h, w] or latents fp32 [4, h, w], table fp32 [T, 2] -> dict of fp64 arrays [4, h, w] (noisy,
    target, latents, noise and tol_* of each) and the int ``t``"""
    assert (moments is None) != (latents is None) and prediction in ("epsilon", "v_prediction")
    src = moments if moments is not None else latents
    assert src.dtype == np.float32 and table.dtype == np.float32
    _, h, w = src.shape
    hw = h * w
    s, no, ip = (float(np.float32(v)) for v in (scale, noise_offset, input_perturbation))
    t = timestep(seed, draw, table.shape[0])
    sa, so = float(table[t, 0]), float(table[t, 1])
    z = {k: PO.normals(seed, subdraw(draw, k), 0, 4 * hw).reshape(4, h, w) for k in (1, 2, 4)}
    z3 = PO.normals(seed, subdraw(draw, 3), 0, 4).reshape(4, 1, 1)
    if moments is not None:
        mean, logvar = moments[:4].astype(np.float64), moments[4:].astype(np.float64)
        sigma = np.exp(0.5 * np.clip(logvar, -30.0, 20.0))
        x0 = s * (mean + sigma * z[1])
        e_x0 = abs(s) * sigma * (DELTA + 4 * U * np.abs(z[1])) + 3 * U * abs(s) * (np.abs(mean) + sigma * np.abs(z[1]))
    else:
        x0 = latents.astype(np.float64)
        e_x0 = np.zeros_like(x0)
    n = z[2] + no * z3                                         # (no == 0: the same values)
    m = n + ip * z[4] if ip != 0.0 else n
    noisy = sa * x0 + so * m
    e_n = DELTA * (1 + abs(no)) + 2 * U * (np.abs(z[2]) + np.abs(no * z3))
    e_m = e_n + abs(ip) * DELTA + 2 * U * (np.abs(n) + np.abs(ip * z[4]))
    tol_noisy = 2 * (sa * e_x0 + so * e_m + 3 * U * (np.abs(sa * x0) + np.abs(so * m)))
    if prediction == "epsilon":
        target, tol_target = n, 2 * e_n
    else:
        target = sa * n - so * x0
        tol_target = 2 * (sa * e_n + so * e_x0 + 3 * U * (np.abs(sa * n) + np.abs(so * x0)))
    return {"t": t, "noisy": noisy, "target": target, "latents": x0, "noise": n, "tol_noisy": tol_noisy, "tol_target": tol_target,
            "tol_latents": 2 * e_x0, "tol_noise": 2 * e_n}


def batch(seeds, draw, table, *, moments=None, latents=None, **kw):
    """the samples stacked: arrays [B, 4, h, w], ``t`` int64 [B]"""
    rows = [sample(s, draw, table, moments=None if moments is None else moments[r], latents=None if latents is None else latents[r],
                   **kw) for r, s in enumerate(seeds)]
    out = {k: np.stack([row[k] for row in rows]) for k in rows[0] if k != "t"}
    out["t"] = np.array([row["t"] for row in rows], dtype=np.int64)
    return out


def worst_used(got, ref, name):
    """max over elements of |got - ref| / tol, and the tolerance is never zero where an error is allowed"""
    err = np.abs(got.astype(np.float64) - ref[name])
    tol = ref["tol_" + name]
    if not (tol > 0).all():                                    # latents given: x0 is a copy, exact
        assert float(err[tol == 0].max(initial=0.0)) == 0.0, name
        tol = np.where(tol > 0, tol, 1.0)
    return float((err / tol).max())


def make_inputs(B, h, w, seed=0, from_moments=True):
    """fp32 inputs with every edge the statements have: means of a few units, and sample 0's first logvar row spanning
    [-35, 6] with one more at 25, so both clamps are hit (the rest in [-8, 1], the range a trained VAE emits)"""
    rs = np.random.RandomState(1000 * seed + 16 * h + w)
    if not from_moments:
        return (rs.randn(B, 4, h, w) * 1.5).astype(np.float32)
    mom = np.empty((B, 8, h, w), np.float32)
    mom[:, :4] = (rs.randn(B, 4, h, w) * 3.0).astype(np.float32)
    mom[:, 4:] = rs.uniform(-8.0, 1.0, (B, 4, h, w)).astype(np.float32)
    mom[0, 4, 0, :] = np.linspace(-35.0, 6.0, w, dtype=np.float32) if w > 1 else np.float32(-35.0)
    mom[0, 5, 0, 0], mom[0, 6, 0, 0] = np.float32(6.0), np.float32(25.0)
    return mom
