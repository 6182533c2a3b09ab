"""GPU checks of the masked router stage (csrc/router_stage.hip, ops.sinkhorn_assign, ops.RouterStage, autograd.router_stage)
against the fp64 model of tests/router_stage_model.py.

The bound of every value and gradient is measured, not derived: the kernels' paths go through exp, log and a division per
element, whose fp32 roundings do not reduce to an operation count.  The project's existing fp32 torch formulas (quantizer._sinkhorn,
losses.ContrastiveLoss, losses.ResourceLoss, torch.std / torch.max and autograd) run on the GPU on the valid rows alone, both are
compared with the fp64 model, and the kernel's error may be at most twice torch's (another summation order over E and n terms,
not another algorithm) plus 64 * 2^-24 * |value| for inputs where torch happens to be exact.  Samples that are not valid reach no
output, whatever their rows hold (NaN in one case per shape), and get gradient rows of exact zeros.  Nothing here provokes a
fault: bad tables are refused by the host validation (tests/test_router_stage_host.py)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import router_stage_model as M

pytestmark = pytest.mark.gpu
from tests.margins import check  # noqa: E402

FLOOR = 64 * 2.0 ** -24
TAU_A, TAU_Z, P_TARGET = 0.7, 1.3, 0.6
WEIGHTS = (2.0, 0.5, 0.3, 0.2)            # resource, contrastive, std, max
EPS, ITERS = 0.05, 3
NAMES = ("contrastive", "resource", "max_loss", "std_loss", "router_loss", "mean_ratio")


def patterns(B):
    """name -> 0 / 1 list"""
    if B == 1:
        return {"all": [1]}
    holes = [0 if b % 3 == 1 or b == B - 1 else 1 for b in range(B)]
    if B == 5:
        return {"all": [1] * 5, "prefix": [1, 1, 1, 0, 0], "holes": [1, 0, 1, 1, 0], "one": [0, 0, 1, 0, 0], "none": [0] * 5}
    if B == 65:
        return {"prefix": [1] * 41 + [0] * 24, "holes": holes}
    return {"prefix": [1] * 37 + [0] * (B - 37)}


# (B, K, E, D, seed): the seeds are pinned to ones that meet the Sinkhorn test's precondition (a relative gap >= 1e-3 between the
# two largest entries of every valid row of the model's Q) under every pattern of the shape
SHAPES = [(1, 4, 40, 32, 0), (5, 4, 40, 32, 0), (65, 8, 130, 70, 0), (64, 8, 1634, 768, 0)]
CASES = [(B, K, E, D, seed, name) for B, K, E, D, seed in SHAPES for name in patterns(B)]
IDS = ["B%d-K%d-E%d-D%d-%s" % (c[0], c[1], c[2], c[3], c[5]) for c in CASES]
# every case with finite rows; every case that has a row outside the mask once more with NaN in those rows
NAN_CASES = [c + (False,) for c in CASES] + [c + (True,) for c in CASES if not all(patterns(c[0])[c[5]])]
NAN_IDS = ["%s-%s" % (IDS[CASES.index(c[:6])], "nan-rows" if c[6] else "finite") for c in NAN_CASES]


def make_inputs(B, K, E, D, seed):
    """arch and the codebook |randn| rows, scores the cosines of the normalised rows, text randn, ratios uniform in [0.3, 0.9];
    fp32 tensors on the host (the model reads exactly these values)"""
    g = torch.Generator().manual_seed(seed)
    arch = torch.randn(B, E, generator=g, dtype=torch.float64).abs()
    codes = torch.randn(K, E, generator=g, dtype=torch.float64).abs()
    text = torch.randn(B, D, generator=g, dtype=torch.float64)
    ratios = 0.3 + 0.6 * torch.rand(B, generator=g, dtype=torch.float64)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)          # noqa: E731
    return text.float(), arch.float(), ratios.float(), (unit(arch) @ unit(codes).T).float()


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _dirty(t, valid):
    t = t.clone()
    for b, v in enumerate(valid):
        if not v:
            t[b] = float("nan")
    return t


def _rel_l2(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def sinkhorn_gap(q, valid):
    """smallest relative gap between the two largest entries of a valid row of the model's Q"""
    gaps = [1.0]
    for b, v in enumerate(valid):
        if v:
            top = np.sort(q[b])[::-1]
            gaps.append((top[0] - top[1]) / top[0])
    return min(gaps)


@pytest.mark.parametrize("B,K,E,D,seed,name,nan_rows", NAN_CASES, ids=NAN_IDS)
def test_sinkhorn_assignment_is_the_model(cuda, B, K, E, D, seed, name, nan_rows):
    from diffusion_pruning_amd import ops
    from diffusion_pruning_amd.quantizer import StructureVectorQuantizer as SVQ
    valid = patterns(B)[name]
    scores = make_inputs(B, K, E, D, seed)[3]
    want_idx, want_q = M.sinkhorn_assign(_np(scores), valid, EPS, ITERS)
    if sum(valid) == 1:
        # one sample alone: the code normalisation makes its row exactly 1 / K in every entry (K a power of two: exact in fp32 and
        # fp64 alike), so there is no gap to ask for -- the tie is exact and the first maximum is code 0 on both sides
        b = valid.index(1)
        assert K & (K - 1) == 0 and (want_q[b] == 1.0 / K).all() and want_idx[b] == 0
    else:
        gap = sinkhorn_gap(want_q, valid)
        print("%s: smallest relative gap of the model's Q %.3e" % (name, gap))
        assert gap >= 1e-3, "precondition: pick another seed"
    given = _dirty(scores, valid) if nan_rows else scores
    if nan_rows:
        want_idx = M.sinkhorn_assign(_np(given), valid, EPS, ITERS)[0]
    v = torch.tensor(valid, dtype=torch.float32, device=cuda)
    q = torch.full((B, K), float("nan"), device=cuda)
    idx = ops.sinkhorn_assign(given.to(cuda), v, EPS, ITERS, q=q)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int64 and idx.cpu().tolist() == want_idx.tolist()             # every row, valid or not
    keep = [b for b, x in enumerate(valid) if x]
    for b in range(B):
        if b not in keep:
            assert float(q[b].abs().max()) == 0.0
    if keep:
        ref = SVQ._sinkhorn(SimpleNamespace(sinkhorn_epsilon=EPS, sinkhorn_iterations=ITERS), scores.to(cuda)[keep].clone(), False)
        scale = float(np.abs(want_q).max())
        e_torch = float(np.abs(_np(ref) - want_q[keep]).max())
        e_kernel = float(np.abs(_np(q)[keep] - want_q[keep]).max())
        print("%s: Q max error kernel %.3e torch %.3e (scale %.3e)" % (name, e_kernel, e_torch, scale))
        check(e_kernel, 2 * e_torch + FLOOR * scale, "sinkhorn Q vs fp64 (%s)" % name)


def _torch_reference(text, arch, ratios, keep, resource_type, g):
    """the project's fp32 formulas on the GPU on the rows `keep`: the six values and the two gradients"""
    from diffusion_pruning_amd.losses import ContrastiveLoss, ResourceLoss
    a, r = arch.clone().requires_grad_(), ratios.clone().requires_grad_()
    con = ContrastiveLoss(TAU_A, TAU_Z)(text[keep], a[keep])
    rk = r[keep]
    res = ResourceLoss(P_TARGET, resource_type)(rk.mean())
    max_loss, std_loss = 1.0 - torch.max(rk), -torch.std(rk)
    w_res, w_con, w_std, w_max = WEIGHTS
    router = w_res * res + w_con * con + w_std * std_loss + w_max * max_loss
    (g * router).backward()
    vals = dict(contrastive=con, resource=res, max_loss=max_loss, std_loss=std_loss, router_loss=router, mean_ratio=rk.mean())
    return {k: float(v.detach()) for k, v in vals.items()}, a.grad, r.grad


def _stage(ops, text, arch, ratios, valid, resource_type):
    return ops.RouterStage(text, arch, ratios, valid, arch_temperature=TAU_A, text_temperature=TAU_Z, p=P_TARGET,
                           resource_type=resource_type, resource_weight=WEIGHTS[0], contrastive_weight=WEIGHTS[1],
                           std_weight=WEIGHTS[2], max_weight=WEIGHTS[3])


@pytest.mark.parametrize("B,K,E,D,seed,name,nan_rows", NAN_CASES, ids=NAN_IDS)
def test_router_stage_is_the_model(cuda, B, K, E, D, seed, name, nan_rows):
    from diffusion_pruning_amd import ops
    valid = patterns(B)[name]
    resource_type = M.RESOURCE_TYPES[(B + len(name)) % 3]          # all three types over the cases
    text, arch, ratios, _ = make_inputs(B, K, E, D, seed)
    keep = [b for b, x in enumerate(valid) if x]
    n = len(keep)
    args = (_np(text), _np(arch), _np(ratios), valid, TAU_A, TAU_Z, P_TARGET, resource_type, WEIGHTS)
    fw = M.forward(*args)
    want_da, want_dr = M.backward(*args, g=0.75)
    given = [_dirty(t, valid).to(cuda) if nan_rows else t.to(cuda) for t in (text, arch, ratios)]
    v = torch.tensor(valid, dtype=torch.float32, device=cuda)
    g = torch.tensor(0.75, device=cuda)
    stage = _stage(ops, *given, v, resource_type)
    stage.d_arch.fill_(float("nan"))
    stage.d_ratios.fill_(float("nan"))
    out = stage.run().clone()
    d_arch, d_ratios = [x.clone() for x in stage.backward(g)]
    torch.cuda.synchronize()
    what = "%s %s%s" % (IDS[CASES.index((B, K, E, D, seed, name))], resource_type, " nan" if nan_rows else "")
    assert float(out[6]) == n == float(stage.n_valid) and float(out[7]) == fw["n_max"]
    for b in range(B):
        if b not in keep:
            assert float(d_arch[b].abs().max()) == 0.0 and float(d_ratios[b]) == 0.0        # written, as exact zeros
    if n == 0:
        assert float(out.abs().max()) == 0.0
        return
    if n == 1:
        assert bool(torch.isnan(out[3])) and bool(torch.isnan(out[4])) and np.isnan(fw["std_loss"])
        for i in (0, 1, 2, 5):
            check(abs(float(out[i]) - fw[NAMES[i]]), FLOOR * abs(fw[NAMES[i]]) + 1e-30, "%s: %s vs fp64 (n = 1)" % (what, NAMES[i]))
        # the backward on the one valid row: P = T = 1 gives no contrastive gradient, the NaN deviation reaches d_ratios
        assert float(d_arch[keep[0]].abs().max()) == 0.0 and bool(torch.isnan(d_ratios[keep[0]])) and np.isnan(want_dr[keep[0]])
        return
    ref_vals, ref_da, ref_dr = _torch_reference(text.to(cuda), arch.to(cuda), ratios.to(cuda), keep, resource_type, 0.75)
    for i, k in enumerate(NAMES):
        e_kernel, e_torch = abs(float(out[i]) - fw[k]), abs(ref_vals[k] - fw[k])
        print("%s: %s error kernel %.3e torch %.3e (value %.6e)" % (what, k, e_kernel, e_torch, fw[k]))
        check(e_kernel, 2 * e_torch + FLOOR * abs(fw[k]), "%s: %s vs fp64" % (what, k))
    assert float(stage.router_loss) == float(out[4]) and float(stage.contrastive) == float(out[0])
    for label, got, ref, want in (("d_arch", d_arch, ref_da, want_da), ("d_ratios", d_ratios, ref_dr, want_dr)):
        e_kernel, e_torch = _rel_l2(_np(got)[keep], want[keep]), _rel_l2(_np(ref)[keep], want[keep])
        print("%s: %s rel-L2 kernel %.3e torch %.3e" % (what, label, e_kernel, e_torch))
        check(e_kernel, 2 * e_torch + FLOOR, "%s: %s rel-L2 vs fp64" % (what, label))


def test_equal_ratios_share_the_gradient_of_the_maximum(cuda):
    from diffusion_pruning_amd import ops
    text, arch, _, _ = make_inputs(5, 4, 40, 32, 0)
    ratios = torch.full((5,), 0.625)
    valid = [1, 0, 1, 1, 0]
    stage = ops.RouterStage(text.to(cuda), arch.to(cuda), ratios.to(cuda), torch.tensor(valid, dtype=torch.float32, device=cuda),
                            resource_weight=0.0, contrastive_weight=0.0, std_weight=0.3, max_weight=1.0)
    out = stage.run()
    _, d_ratios = stage.backward(torch.tensor(1.0, device=cuda))
    assert float(out[2]) == 0.375 and float(out[3]) == 0.0 and float(out[7]) == 3.0
    third = float(np.float32(-1.0) / np.float32(3.0))
    assert d_ratios.cpu().tolist() == [third, 0.0, third, third, 0.0]


def test_autograd_node_hands_both_gradients_back(cuda):
    from diffusion_pruning_amd import autograd as A, ops
    text, arch, ratios, _ = [t.to(cuda) for t in make_inputs(5, 4, 40, 32, 0)]
    leaf_a, leaf_r = arch.clone().requires_grad_(), ratios.clone().requires_grad_()
    a, r = leaf_a * 1.0, leaf_r * 1.0
    valid = torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0], device=cuda)
    stage = _stage(ops, text, a, r, valid, "log")
    loss = A.router_stage(stage)
    (loss * 0.75).backward()
    want = _stage(ops, text, arch, ratios, valid, "log")
    want.run()
    da, dr = want.backward(torch.tensor(0.75, device=cuda))
    assert float(loss) == float(want.router_loss) and torch.equal(leaf_a.grad, da) and torch.equal(leaf_r.grad, dr)
    with pytest.raises(AssertionError, match="text must not require grad"):
        A.router_stage(_stage(ops, text.clone().requires_grad_(), a, r, valid, "log"))


def test_captured_stage_replays_to_the_same_bits_and_follows_valid(cuda):
    from diffusion_pruning_amd import ops
    B, K, E, D, seed = 65, 8, 130, 70, 0
    text, arch, ratios, scores = [t.to(cuda) for t in make_inputs(B, K, E, D, seed)]
    first, second = patterns(B)["prefix"], patterns(B)["holes"]
    valid = torch.tensor(first, dtype=torch.float32, device=cuda)
    g = torch.tensor(0.5, device=cuda)
    stage = _stage(ops, text, arch, ratios, valid, "log")
    idx, q = torch.empty(B, dtype=torch.int64, device=cuda), torch.empty(B, K, device=cuda)

    def run():
        ops.sinkhorn_assign(scores, valid, EPS, ITERS, out=idx, q=q)
        stage.run()
        stage.backward(g)

    def snapshot():
        torch.cuda.synchronize()
        return [t.clone() for t in (idx, q, stage.out, stage.d_arch, stage.d_ratios)]
    eager = {}
    for name, pat in (("first", first), ("second", second)):
        valid.copy_(torch.tensor(pat, dtype=torch.float32))
        run()
        eager[name] = snapshot()
    valid.copy_(torch.tensor(first, dtype=torch.float32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for name, pat in (("first", first), ("first", first), ("second", second), ("first", first)):
        valid.copy_(torch.tensor(pat, dtype=torch.float32))
        for t in (q, stage.out, stage.d_arch, stage.d_ratios):
            t.fill_(float("nan"))
        graph.replay()
        got = snapshot()
        assert all(torch.equal(x, y) for x, y in zip(got, eager[name])), name
    assert not torch.equal(eager["first"][2], eager["second"][2])
