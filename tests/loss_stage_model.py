"""fp64 numpy model of the masked loss stage (include/aptp_hip.h: aptp_loss_stage, aptp_loss_stage_bwd; csrc/loss_stage.hip), in the
kernel's index order, and the operation counts its fp32 results are bounded with.  Never imported by the package.

A term is a dict: a, b (arrays [B, ...] of one shape), group, scale, weighted.  Parameters the kernel holds as fp32 (scale,
group_coef, group_div, w, valid) enter at their fp32 values, so that the model differs from the kernel by the kernel's own
roundings only."""
import numpy as np

EPS = 2.0 ** -24                  # unit roundoff of fp32


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def unit_means(terms):
    """[T][B]: mean((a - b)^2) of every sample of every term, in fp64"""
    out = []
    for t in terms:
        a, b = np.asarray(t["a"], dtype=np.float64), np.asarray(t["b"], dtype=np.float64)
        d = (a - b).reshape(a.shape[0], -1)
        out.append((d * d).mean(axis=1))
    return np.array(out)


def forward(terms, valid, w, group_coef, group_div=None, units=None):
    """{"units", "terms", "groups", "total", "n"}.  units: [T][B] values to combine (default: unit_means(terms)); samples with
    valid[b] == 0 are skipped, whatever their unit values are"""
    valid = _f32(valid)
    B, G = len(valid), len(group_coef)
    units = unit_means(terms) if units is None else np.asarray(units, dtype=np.float64)
    w = None if w is None else _f32(w)
    n = 0.0
    for b in range(B):
        n += valid[b]
    tv = []
    for t, T in enumerate(terms):
        s = 0.0
        for b in range(B):
            if valid[b] != 0:
                s += (w[b] if T.get("weighted") else 1.0) * units[t][b]
        tv.append(s * (1.0 / n) if n != 0 else 0.0)
    groups = [0.0] * G
    for t, T in enumerate(terms):
        groups[T["group"]] += tv[t] * float(_f32(T.get("scale", 1.0)))
    total = 0.0
    for g in range(G):
        d = float(_f32(group_div[g])) if group_div is not None else 0.0
        if d != 0:
            groups[g] = groups[g] / d
        total += float(_f32(group_coef[g])) * groups[g]
    return {"units": units, "terms": tv, "groups": groups, "total": total, "n": n}


def coefficients(terms, t, valid, w, group_coef, group_div=None, g=1.0):
    """c_t[b] of the header, the upstream gradient g included: fp64 [B]"""
    valid = _f32(valid)
    T = terms[t]
    n = float(valid.sum())
    B = len(valid)
    if n == 0:
        return np.zeros(B)
    E = float(np.asarray(T["a"]).size // B)
    d = float(_f32(group_div[T["group"]])) if group_div is not None else 0.0
    d = d if d != 0 else 1.0
    wv = _f32(w) if T.get("weighted") else np.ones(B)
    return float(_f32(g)) * 2.0 * float(_f32(group_coef[T["group"]])) * float(_f32(T.get("scale", 1.0))) * valid * wv / (n * E * d)


def backward(terms, items, valid, w, group_coef, group_div=None, g=1.0):
    """items: (t0, t1 or None) per gradient.  Per item (grad, bound): grad[b] = c0[b] (a - b0) + c1[b] (a - b1) in fp64, rows of
    samples with valid[b] == 0 exactly zero whatever they hold; bound = |c0 (a - b0)| + |c1 (a - b1)|, what the fp32 roundings of
    the kernel are relative to"""
    valid = _f32(valid)
    out = []
    for t0, t1 in items:
        a = np.asarray(terms[t0]["a"], dtype=np.float64)
        grad, bound = np.zeros(a.shape), np.zeros(a.shape)
        for t in (t0, t1):
            if t is None:
                continue
            c = coefficients(terms, t, valid, w, group_coef, group_div, g)
            bt = np.asarray(terms[t]["b"], dtype=np.float64)
            for b in range(a.shape[0]):
                if valid[b] != 0:
                    x = c[b] * (a[b] - bt[b])
                    grad[b] += x
                    bound[b] += np.abs(x)
        out.append((grad, bound))
    return out


# ---- how many fp32 roundings lie on the path of a value (all summands are >= 0: each rounding is at most EPS relative) ----------
def mse_nblocks(rows, C):
    """aptp_mse_nblocks"""
    nvec = rows * (C // 8)
    return max(1, min(1024, (nvec + 511) // 512))


def unit_ops(rows_per_sample, C):
    """longest chain of roundings from an element to its unit mean: the difference (counted twice: it is squared), the square,
    the 8 additions of a vector, the additions of a thread's vectors, 6 shuffle steps, 2 additions over the waves, the
    additions of a finish thread, 8 tree levels, the product with inv_n and the 2 roundings inside inv_n"""
    nvec = rows_per_sample * (C // 8)
    nblk = mse_nblocks(rows_per_sample, C)
    per_thread = -(-nvec // (nblk * 256))
    per_finish = -(-nblk // 256)
    return 3 + 8 + per_thread + 6 + 2 + per_finish + 8 + 1 + 2


def term_ops(B, weighted):
    """unit values -> term: the weight product, at most B additions, the reciprocal of n and the product with it"""
    return (1 if weighted else 0) + B + 2


def group_ops(n_terms_in_group, has_div):
    """terms -> group: the scale product, the additions, the division"""
    return 1 + n_terms_in_group + (1 if has_div else 0)


def total_ops(n_groups):
    """groups -> total: the coefficient product and the additions"""
    return 1 + n_groups
