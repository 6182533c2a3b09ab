"""fp64 statement of ONE call of aptp_group_adamw (csrc/router_optim.hip): parameter groups with their own rate, weight decay and
warm-up, a step count per item, the gate, the gradient scan, grad_scale and zero_grad.  Not a test: tests/test_router_optim_host.py
holds it against torch.optim.AdamW + LambdaLR, tests/test_router_optim_gpu.py holds the kernel against it."""
import math

import torch


def step(items, groups, counters, betas, eps, gate=None, grad_scale=1.0, zero_grad=False):
    """items:    list of dicts {"p", "g", "m", "v": tensors of one shape, "step": float, "group": int} -- the table of the call
    groups:   list of (lr, weight_decay, warmup_steps)
    counters: [applied, skipped, flag, reserved]
    Returns (new items, new counters); the inputs are left alone.  Every tensor of the result is float64."""
    d = torch.float64
    b1, b2 = float(betas[0]), float(betas[1])
    gs = 1.0 if grad_scale == 0 else float(grad_scale)
    applied, skipped = float(counters[0]), float(counters[1])
    skip = gate is not None and not math.isfinite(float(gate))
    for it in items:
        skip = skip or not bool(torch.isfinite(it["g"]).all())
    out = []
    for it in items:
        p, g, m, v = (it[k].to(d).clone() for k in ("p", "g", "m", "v"))
        s = float(it["step"])
        if not skip:
            lr, wd, W = (float(x) for x in groups[it["group"]])
            if W > 0:
                lr = lr * min(1.0, applied / W)
            t = s + 1.0
            bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
            gg = g * gs
            p = p * (1.0 - lr * wd)
            m = b1 * m + (1.0 - b1) * gg
            v = b2 * v + (1.0 - b2) * gg * gg
            p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
            s = t
        if zero_grad:
            g = torch.zeros_like(g)
        out.append({"p": p, "g": g, "m": m, "v": v, "step": s, "group": it["group"]})
    new = [applied + (0.0 if skip else 1.0), skipped + (1.0 if skip else 0.0), 0.0, float(counters[3])]
    return out, new
