"""fp64 numpy model of the masked router stage (csrc/router_stage.hip): the Sinkhorn assignment, the contrastive loss and the
three MAC losses over the valid samples of a batch, forward and backward.  Written from the formulas of include/aptp_hip.h, not
from the kernel: no sample that is not valid is ever read (its rows may hold NaN)."""
import numpy as np

RESOURCE_TYPES = ("log", "mae", "mse")


def _valid_index(valid):
    return [b for b, v in enumerate(np.asarray(valid).tolist()) if v != 0]


def first_argmax(row):
    """torch.argmax of one row: the first maximum, a NaN counting as the maximum"""
    row = np.asarray(row, dtype=np.float64)
    nan = np.isnan(row)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(row))


def sinkhorn_assign(scores, valid, eps, iters):
    """(idx int64 [B], Q fp64 [B, K]): masked quantizer._sinkhorn + argmax; rows that are not valid get the argmax of their raw
    scores and a Q row of zeros"""
    scores = np.asarray(scores, dtype=np.float64)
    B, K = scores.shape
    V = _valid_index(valid)
    n = len(V)
    Q = np.zeros((B, K))
    idx = np.zeros(B, dtype=np.int64)
    if n:
        q = np.exp(scores[V] / eps)                    # [n, K]: the reference's Q transposed
        q /= q.sum()
        for _ in range(iters):
            q /= q.sum(axis=0, keepdims=True)          # per code, over the samples
            q /= K
            q /= q.sum(axis=1, keepdims=True)          # per sample
            q /= n
        q *= n
        Q[V] = q
    for b in range(B):
        idx[b] = first_argmax(Q[b]) if (n and b in V) else first_argmax(scores[b])
    return idx, Q


def _softmax_rows(s):
    e = np.exp(s - s.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _resource(rbar, p, kind):
    if kind == "log":
        return np.log(rbar / p) if rbar > p else np.log(p / rbar)
    if kind == "mae":
        return abs(rbar - p)
    assert kind == "mse", kind
    return (rbar - p) ** 2


def forward(text, arch, ratios, valid, tau_arch, tau_text, p, resource_type, weights):
    """weights = (resource, contrastive, std, max).  Returns a dict of the eight outputs, plus what the backward needs"""
    V = _valid_index(valid)
    n = len(V)
    keys = ("contrastive", "resource", "max_loss", "std_loss", "router_loss", "mean_ratio")
    if n == 0:
        return {**{k: 0.0 for k in keys}, "n": 0, "n_max": 0, "V": V}
    A = np.asarray(arch, dtype=np.float64)[V]
    Z = np.asarray(text, dtype=np.float64)[V]
    r = np.asarray(ratios, dtype=np.float64)[V]
    na = np.linalg.norm(A, axis=1, keepdims=True)
    Ah, Zh = A / na, Z / np.linalg.norm(Z, axis=1, keepdims=True)
    P, T = _softmax_rows(Ah @ Ah.T / tau_arch), _softmax_rows(Zh @ Zh.T / tau_text)
    with np.errstate(divide="ignore"):
        logP, log1mP = np.maximum(np.log(P), -100.0), np.maximum(np.log(1.0 - P), -100.0)
    contrastive = float(-(T * logP + (1.0 - T) * log1mP).sum() / (n * n))
    rbar, rmax = float(r.mean()), float(r.max())
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = float(np.sqrt(((r - rbar) ** 2).sum() / np.float64(n - 1)))
    resource = float(_resource(rbar, p, resource_type))
    w_res, w_con, w_std, w_max = weights
    max_loss, std_loss = 1.0 - rmax, -sd
    router = w_res * resource + w_con * contrastive + w_std * std_loss + w_max * max_loss
    return dict(contrastive=contrastive, resource=resource, max_loss=max_loss, std_loss=std_loss, router_loss=router,
                mean_ratio=rbar, n=n, n_max=int((r == rmax).sum()), V=V, P=P, T=T, Ah=Ah, na=na, r=r, sd=sd, rmax=rmax)


def backward(text, arch, ratios, valid, tau_arch, tau_text, p, resource_type, weights, g=1.0):
    """(d_arch [B, E], d_ratios [B]) of g * router_loss; exactly zero on the rows that are not valid"""
    arch = np.asarray(arch, dtype=np.float64)
    B, E = arch.shape
    d_arch, d_ratios = np.zeros((B, E)), np.zeros(B)
    f = forward(text, arch, ratios, valid, tau_arch, tau_text, p, resource_type, weights)
    n, V = f["n"], f["V"]
    if n == 0:
        return d_arch, d_ratios
    w_res, w_con, w_std, w_max = weights
    P, T, Ah = f["P"], f["T"], f["Ah"]
    dP = (P - T) / np.maximum(P * (1.0 - P), 1e-12) / (n * n) * (g * w_con)       # binary_cross_entropy_backward
    dS = P * (dP - (dP * P).sum(axis=1, keepdims=True)) / tau_arch
    dAh = (dS + dS.T) @ Ah
    d_arch[V] = (dAh - Ah * (dAh * Ah).sum(axis=1, keepdims=True)) / f["na"]
    rbar, r, sd = f["mean_ratio"], f["r"], f["sd"]
    if resource_type == "log":
        dres = 1.0 / rbar if rbar > p else -1.0 / rbar
    elif resource_type == "mae":
        dres = float(np.sign(rbar - p))
    else:
        dres = 2.0 * (rbar - p)
    d = np.full(n, w_res * dres / n)
    if sd != 0.0:                                      # torch's std backward: nothing flows where the deviation is exactly 0
        with np.errstate(invalid="ignore", divide="ignore"):
            d = d + w_std * (-(r - rbar) / (np.float64(n - 1) * sd))
    d = d + w_max * np.where(r == f["rmax"], -1.0 / f["n_max"], 0.0)
    d_ratios[V] = g * d
    return d_arch, d_ratios
