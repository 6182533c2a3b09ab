"""CPU checks of the masked router stage (csrc/router_stage.hip, ops.RouterStage, ops.sinkhorn_assign,
GraphedPrunerStep(short_batches=True)): the fp64 model of tests/router_stage_model.py is the project's own Sinkhorn assignment,
contrastive loss, resource loss and MAC statistics -- and their autograd gradients -- on the valid samples alone, the parameter
blocks have the C compiler's layout, bad tables are refused without a launch, and the staging of the prompt embeddings of a short
batch pads with the batch's own first row."""
import ctypes
import os
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import router_stage_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aptp_hip.h")
PATTERNS = {"all": [1, 1, 1, 1, 1], "prefix": [1, 1, 1, 0, 0], "holes": [1, 0, 1, 1, 0], "one": [0, 0, 1, 0, 0], "none": [0, 0, 0, 0, 0]}
B, K, E, D = 5, 4, 40, 32
TAU_A, TAU_Z, P_TARGET = 0.7, 1.3, 0.6
WEIGHTS = (2.0, 0.5, 0.3, 0.2)            # resource, contrastive, std, max
EPS, ITERS = 0.05, 3


@pytest.fixture(scope="module")
def lib():
    from diffusion_pruning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    arch = torch.randn(B, E, generator=g, dtype=torch.float64).abs()
    codes = torch.randn(K, E, generator=g, dtype=torch.float64).abs()
    text = torch.randn(B, D, generator=g, dtype=torch.float64)
    ratios = 0.3 + 0.6 * torch.rand(B, generator=g, dtype=torch.float64)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)          # noqa: E731
    return text, arch, ratios, unit(arch) @ unit(codes).T


def _keep(pattern):
    return [b for b, v in enumerate(PATTERNS[pattern]) if v]


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_model_sinkhorn_is_the_quantizer_on_the_valid_rows(pattern):
    from diffusion_pruning_amd.quantizer import StructureVectorQuantizer as Q
    keep = _keep(pattern)
    for seed in range(5):
        scores = _inputs(seed)[3]
        idx, q = M.sinkhorn_assign(scores.numpy(), PATTERNS[pattern], EPS, ITERS)
        raw = torch.argmax(scores, dim=-1)
        for b in range(B):
            if b not in keep:
                assert idx[b] == int(raw[b]) and float(np.abs(q[b]).max()) == 0.0
        if keep:
            want = Q._sinkhorn(SimpleNamespace(sinkhorn_epsilon=EPS, sinkhorn_iterations=ITERS), scores[keep].clone(), False)
            assert float(np.abs(q[keep] - want.numpy()).max()) <= 1e-12 * float(want.abs().max())
            assert idx[keep].tolist() == torch.argmax(want, dim=-1).tolist()


def _torch_losses(text, arch, ratios, keep, resource_type):
    """the project's own formulas (losses.py, PrunerStep._mac_losses, GraphedPrunerStep._router_loss) on the rows `keep`"""
    from diffusion_pruning_amd.losses import ContrastiveLoss, ResourceLoss
    con = ContrastiveLoss(TAU_A, TAU_Z)(text[keep], arch[keep])
    r = ratios[keep]
    res = ResourceLoss(P_TARGET, resource_type)(r.mean())
    max_loss, std_loss = 1.0 - torch.max(r), -torch.std(r)
    w_res, w_con, w_std, w_max = WEIGHTS
    return dict(contrastive=con, resource=res, max_loss=max_loss, std_loss=std_loss, mean_ratio=r.mean(),
                router_loss=w_res * res + w_con * con + w_std * std_loss + w_max * max_loss)


@pytest.mark.parametrize("resource_type", M.RESOURCE_TYPES)
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_model_is_the_project_losses_and_autograd_on_the_valid_rows(pattern, resource_type):
    keep = _keep(pattern)
    text, arch, ratios, _ = _inputs(1)
    args = (text.numpy(), arch.numpy(), ratios.numpy(), PATTERNS[pattern], TAU_A, TAU_Z, P_TARGET, resource_type, WEIGHTS)
    fw = M.forward(*args)
    d_arch, d_ratios = M.backward(*args, g=0.75)
    assert fw["n"] == len(keep)
    if not keep:
        assert all(fw[k] == 0.0 for k in ("contrastive", "resource", "max_loss", "std_loss", "router_loss", "mean_ratio"))
        assert float(np.abs(d_arch).max()) == 0.0 and float(np.abs(d_ratios).max()) == 0.0
        return
    a, r = arch.clone().requires_grad_(), ratios.clone().requires_grad_()
    want = _torch_losses(text, a, r, keep, resource_type)
    if len(keep) == 1:
        assert np.isnan(fw["std_loss"]) and np.isnan(fw["router_loss"]) and bool(torch.isnan(want["std_loss"]))
        for k in ("contrastive", "resource", "max_loss", "mean_ratio"):
            assert abs(fw[k] - float(want[k].detach())) <= 1e-12 * abs(float(want[k].detach())) + 1e-15, k
        return
    for k, v in want.items():
        assert abs(fw[k] - float(v.detach())) <= 1e-12 * abs(float(v.detach())), (k, fw[k])
    (0.75 * want["router_loss"]).backward()
    for got, leaf in ((d_arch, a), (d_ratios, r)):
        ref = leaf.grad.numpy()
        assert float(np.abs(got - ref).max()) <= 1e-10 * float(np.abs(ref).max())
        for b in range(B):
            if b not in keep:
                assert float(np.abs(got[b]).max()) == 0.0 and float(np.abs(ref[b]).max()) == 0.0      # exactly zero, both


@pytest.mark.parametrize("pattern", ["prefix", "holes", "one", "none"])
def test_model_ignores_what_invalid_rows_hold(pattern):
    text, arch, ratios, scores = _inputs(2)
    valid = PATTERNS[pattern]
    args = lambda t, a, r: (t.numpy(), a.numpy(), r.numpy(), valid, TAU_A, TAU_Z, P_TARGET, "log", WEIGHTS)      # noqa: E731
    fw, gr = M.forward(*args(text, arch, ratios)), M.backward(*args(text, arch, ratios))
    q = M.sinkhorn_assign(scores.numpy(), valid, EPS, ITERS)[1]
    dirty = [t.clone() for t in (text, arch, ratios, scores)]
    for t in dirty:
        for b, v in enumerate(valid):
            if not v:
                t[b] = float("nan")
    fw2, gr2 = M.forward(*args(*dirty[:3])), M.backward(*args(*dirty[:3]))
    for k in ("contrastive", "resource", "max_loss", "std_loss", "router_loss", "mean_ratio", "n"):
        assert fw2[k] == fw[k] or (np.isnan(fw2[k]) and np.isnan(fw[k])), k
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(gr, gr2))
    idx2, q2 = M.sinkhorn_assign(dirty[3].numpy(), valid, EPS, ITERS)
    assert np.array_equal(q, q2) and all(idx2[b] == 0 for b, v in enumerate(valid) if not v)


@pytest.mark.parametrize("pattern", ["all", "prefix", "holes"])
def test_equal_ratios_share_the_gradient_of_the_maximum(pattern):
    keep = _keep(pattern)
    text, arch, _, _ = _inputs(3)
    ratios = torch.full((B,), 0.625, dtype=torch.float64)
    weights = (0.0, 0.0, 0.3, 1.0)
    _, d_ratios = M.backward(text.numpy(), arch.numpy(), ratios.numpy(), PATTERNS[pattern], TAU_A, TAU_Z, P_TARGET, "log", weights)
    r = ratios.clone().requires_grad_()
    (weights[2] * -torch.std(r[keep]) + weights[3] * (1.0 - torch.max(r[keep]))).backward()
    assert np.array_equal(d_ratios, r.grad.numpy())
    assert d_ratios[keep].tolist() == [-1.0 / len(keep)] * len(keep)


def test_param_blocks_match_the_c_header():
    from diffusion_pruning_amd import _lib
    structs = {"AptpSinkhornParams": _lib.SinkhornParams, "AptpRouterStageParams": _lib.RouterStageParams}
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        body.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            body.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    body.append('printf("consts %d/%d/%d/%d/%d/%d\\n", APTP_ROUTER_STAGE_MAX_B, APTP_ROUTER_STAGE_MAX_FEATURES, APTP_SINKHORN_MAX_K, '
                'APTP_RESOURCE_LOG, APTP_RESOURCE_MAE, APTP_RESOURCE_MSE);')
    body.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(body))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.strip().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    t = _lib.RESOURCE_TYPES
    assert got["consts"] == "/".join(map(str, (_lib.ROUTER_STAGE_MAX_B, _lib.ROUTER_STAGE_MAX_FEATURES, _lib.SINKHORN_MAX_K,
                                               t["log"], t["mae"], t["mse"]))) == "1024/4096/64/0/1/2"


def stage_table(**kw):
    from diffusion_pruning_amd import _lib
    p = _lib.RouterStageParams()
    for name in ("text", "arch", "ratios", "valid", "g", "work", "out", "d_arch", "d_ratios"):
        setattr(p, name, 4096)
    p.B, p.E, p.D, p.ld_text, p.ld_arch, p.ld_darch = 5, 40, 32, 32, 40, 40
    p.tau_arch, p.tau_text, p.p, p.resource_type = 1.0, 1.0, 0.6, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def sinkhorn_table(**kw):
    from diffusion_pruning_amd import _lib
    p = _lib.SinkhornParams()
    p.scores, p.valid, p.idx, p.q = 4096, 4096, 4096, 4096
    p.B, p.K, p.ld, p.iters, p.eps = 5, 4, 4, 3, 0.05
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_bad_tables_are_refused_without_a_launch(lib):
    """(no GPU here: a refusal that came after a HIP call would not come back as APTP_EINVAL with these messages)"""
    stage = [("B 0", b"B must be", False, dict(B=0)), ("B above 1024", b"B must be", False, dict(B=1025)),
             ("E 0", b"E must be", False, dict(E=0)), ("E above 4096", b"E must be", False, dict(E=4097, ld_arch=4097, ld_darch=4097)),
             ("D above 4096", b"D must be", False, dict(D=4097, ld_text=4097)),
             ("null text", b"null operand", False, dict(text=None)), ("null arch", b"null operand", False, dict(arch=None)),
             ("null ratios", b"null operand", False, dict(ratios=None)), ("null valid", b"null operand", False, dict(valid=None)),
             ("null work", b"work", False, dict(work=None)), ("null out", b"out", False, dict(out=None)),
             ("text pitch", b"pitch", False, dict(ld_text=31)), ("arch pitch", b"pitch", False, dict(ld_arch=39)),
             ("resource type", b"resource type", False, dict(resource_type=3)),
             ("temperature", b"temperatures", False, dict(tau_arch=0.0)),
             ("null g", b"needs g", True, dict(g=None)), ("null d_arch", b"d_arch", True, dict(d_arch=None)),
             ("null d_ratios", b"d_ratios", True, dict(d_ratios=None)), ("d_arch pitch", b"d_arch pitch", True, dict(ld_darch=39))]
    for what, word, bwd_only, kw in stage:
        p = stage_table(**kw)
        if not bwd_only:
            assert lib.aptp_router_stage(ctypes.byref(p), None) == -1, what
            assert word in lib.aptp_last_error(), (what, lib.aptp_last_error())
        assert lib.aptp_router_stage_bwd(ctypes.byref(p), None) == -1, what
        assert word in lib.aptp_last_error(), (what, lib.aptp_last_error())
    assert lib.aptp_router_stage(None, None) == -1 and lib.aptp_router_stage_bwd(None, None) == -1
    sink = [("B 0", b"B must be", dict(B=0)), ("B above 1024", b"B must be", dict(B=1025)), ("K 0", b"K must be", dict(K=0)),
            ("K above 64", b"K must be", dict(K=65, ld=65)), ("iters", b"iters", dict(iters=-1)), ("eps", b"eps", dict(eps=0.0)),
            ("null scores", b"null pointer", dict(scores=None)), ("null valid", b"null pointer", dict(valid=None)),
            ("null idx", b"null pointer", dict(idx=None)), ("null q", b"null pointer", dict(q=None)), ("pitch", b"pitch", dict(ld=3))]
    for what, word, kw in sink:
        assert lib.aptp_sinkhorn_assign(ctypes.byref(sinkhorn_table(**kw)), None) == -1, what
        assert word in lib.aptp_last_error(), (what, lib.aptp_last_error())
    assert lib.aptp_sinkhorn_assign(None, None) == -1
    assert lib.aptp_router_stage_work_floats(5, 40, 32) == 5 * 40 + 5 * 32 + 3 * 25 + 2 * 5 + 2
    assert lib.aptp_router_stage_work_floats(1025, 40, 32) == 0 and lib.aptp_router_stage_work_floats(5, 0, 32) == 0


def test_short_prompt_embeddings_are_padded_with_their_own_first_row():
    from diffusion_pruning_amd.train_step import _stage_short_rows
    g = torch.Generator().manual_seed(4)
    static = torch.full((4, 8), float("nan"))
    assert _stage_short_rows(static, torch.empty(0, 8)) == 0 and bool(static.isnan().all())
    rows = torch.randn(2, 8, generator=g)
    assert _stage_short_rows(static, rows) == 2
    assert torch.equal(static[:2], rows) and torch.equal(static[2], rows[0]) and torch.equal(static[3], rows[0])
    full = torch.randn(4, 8, generator=g)
    assert _stage_short_rows(static, full) == 4 and torch.equal(static, full)
    with pytest.raises(ValueError, match="does not fit"):
        _stage_short_rows(static, torch.randn(5, 8, generator=g))
