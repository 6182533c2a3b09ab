"""CPU checks of the masked loss stage (csrc/loss_stage.hip, ops.LossStage, GraphedFineTunerStep(short_batches=True)): the fp64
model of tests/loss_stage_model.py is the reference's fine-tuning loss (pdm/training/trainer.py:1736-1763) and its autograd
gradient on the valid samples alone, the parameter block has the C compiler's layout, bad tables are refused without a launch,
and the staging of a short batch pads with the batch's own first row."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import loss_stage_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aptp_hip.h")
COEF, N_BLOCKS = (0.01, 0.5, 0.5), 3
PATTERNS = {"all": [1, 1, 1, 1, 1], "prefix3": [1, 1, 1, 0, 0], "holes": [1, 0, 1, 1, 0], "none": [0, 0, 0, 0, 0]}


@pytest.fixture(scope="module")
def lib():
    from diffusion_pruning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _tensors(seed=0, B=5):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    pred, target, full = r(B, 4, 6, 6), r(B, 4, 6, 6), r(B, 4, 6, 6)
    acts_s = [r(B, 8, 6, 6), r(B, 16, 3, 3), r(B, 8, 6, 6)]
    acts_t = [r(B, 8, 6, 6), r(B, 16, 3, 3), r(B, 8, 6, 6)]
    w = torch.rand(B, generator=g, dtype=torch.float64).float().double() + 0.1
    return pred, target, full, acts_s, acts_t, w.float().double()


def _terms(pred, target, full, acts_s, acts_t):
    n = lambda t: t.detach().numpy()                                          # noqa: E731
    terms = [dict(a=n(pred), b=n(target), group=0, scale=1.0, weighted=True)]
    terms += [dict(a=n(s), b=n(t), group=1, scale=1.0, weighted=False) for s, t in zip(acts_s, acts_t)]
    terms.append(dict(a=n(pred), b=n(full), group=2, scale=1.0, weighted=False))
    items = [(0, len(terms) - 1)] + [(1 + i, None) for i in range(len(acts_s))]
    return terms, items


def _reference(pred, target, full, acts_s, acts_t, w, keep):
    """trainer.py:1736-1763 on the samples `keep` alone: (total, diffusion, distillation, block)"""
    pred, target, full, w = pred[keep], target[keep], full[keep], w[keep]
    loss = F.mse_loss(pred, target, reduction="none")
    loss = (loss.mean(dim=list(range(1, loss.dim()))) * w).mean()
    diff = loss.detach().clone()
    loss = loss * float(np.float32(COEF[0]))
    block = torch.zeros((), dtype=torch.float64)
    for s, t in zip(acts_s, acts_t):
        block = block + F.mse_loss(s[keep], t[keep].detach(), reduction="mean")
    block = block / len(acts_s)
    loss = loss + float(np.float32(COEF[1])) * block
    dist = F.mse_loss(pred, full, reduction="mean")
    loss = loss + float(np.float32(COEF[2])) * dist
    return loss, diff, dist.detach(), block.detach()


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_model_is_the_reference_loss_on_the_valid_samples(pattern):
    valid = PATTERNS[pattern]
    keep = [b for b, v in enumerate(valid) if v]
    pred, target, full, acts_s, acts_t, w = _tensors()
    terms, items = _terms(pred, target, full, acts_s, acts_t)
    div = (0.0, float(N_BLOCKS), 0.0)
    fw = M.forward(terms, valid, w.numpy(), COEF, div)
    grads = M.backward(terms, items, valid, w.numpy(), COEF, div, g=1.0)
    assert fw["n"] == len(keep)
    if not keep:
        assert fw["total"] == 0.0 and fw["groups"] == [0.0, 0.0, 0.0]
        assert all(float(np.abs(g).max()) == 0.0 for g, _ in grads)
        return
    leaves = [pred.clone().requires_grad_()] + [s.clone().requires_grad_() for s in acts_s]
    total, diff, dist, block = _reference(leaves[0], target, full, leaves[1:], acts_t, w, keep)
    total.backward()
    for got, want in zip([fw["total"], fw["groups"][0], fw["groups"][2], fw["groups"][1]], [total, diff, dist, block]):
        assert abs(got - float(want.detach())) <= 1e-13 * abs(float(want.detach())), pattern
    for (g, bound), leaf in zip(grads, leaves):
        want = leaf.grad.numpy()
        assert float(np.abs(g - want).max()) <= 1e-13 * float(np.abs(want).max())
        assert (bound >= np.abs(g) * (1 - 1e-12)).all()
        for b, v in enumerate(valid):
            if not v:
                assert float(np.abs(g[b]).max()) == 0.0 and float(np.abs(want[b]).max()) == 0.0      # exactly zero, both


@pytest.mark.parametrize("pattern", ["prefix3", "holes", "none"])
def test_model_ignores_what_invalid_rows_hold(pattern):
    valid = PATTERNS[pattern]
    pred, target, full, acts_s, acts_t, w = _tensors()
    terms, items = _terms(pred, target, full, acts_s, acts_t)
    div = (0.0, float(N_BLOCKS), 0.0)
    fw = M.forward(terms, valid, w.numpy(), COEF, div)
    grads = M.backward(terms, items, valid, w.numpy(), COEF, div, g=0.5)
    for fill in (float("nan"), 1e30):
        dirty = [t.clone() for t in (pred, target, full, *acts_s, *acts_t)]
        for t in dirty:
            for b, v in enumerate(valid):
                if not v:
                    t[b] = fill
        k = len(acts_s)
        terms2, _ = _terms(dirty[0], dirty[1], dirty[2], dirty[3:3 + k], dirty[3 + k:])
        with np.errstate(all="ignore"):
            fw2 = M.forward(terms2, valid, w.numpy(), COEF, div)
            grads2 = M.backward(terms2, items, valid, w.numpy(), COEF, div, g=0.5)
        assert fw2["total"] == fw["total"] and fw2["groups"] == fw["groups"] and fw2["n"] == fw["n"]
        for (g, _), (g2, _) in zip(grads, grads2):
            assert np.array_equal(g, g2)


def test_operation_counts_follow_the_table_sizes():
    assert M.mse_nblocks(1, 8) == 1 and M.mse_nblocks(64, 64) == 1 and M.mse_nblocks(65, 64) == 2
    assert M.unit_ops(1, 8) == 3 + 8 + 1 + 6 + 2 + 1 + 8 + 3
    assert M.unit_ops(2048, 64) - M.unit_ops(1, 8) == 1            # 16384 vectors on 32 workgroups: 2 per thread
    assert M.term_ops(5, True) == 8 and M.group_ops(3, True) == 5 and M.total_ops(3) == 4


def test_param_blocks_match_the_c_header():
    from diffusion_pruning_amd import _lib
    structs = {"AptpLossStageTerm": _lib.LossStageTerm, "AptpLossStageGrad": _lib.LossStageGrad,
               "AptpLossStageParams": _lib.LossStageParams}
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        body.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            body.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    body.append('printf("maxb %d\\n", APTP_LOSS_STAGE_MAX_B);')
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
    assert int(got["maxb"]) == _lib.LOSS_STAGE_MAX_B == 1024


def _term(q, B, rps, C, group=0, a=4096, b=8192, lda=None, ldb=None, weighted=0):
    q.a, q.b, q.rows, q.C, q.rows_per_sample, q.group, q.scale, q.weighted = a, b, B * rps, C, rps, group, 1.0, weighted
    q.lda, q.ldb = (C if lda is None else lda), (C if ldb is None else ldb)


def table(n_terms=1, n_groups=1, n_grads=1):
    from diffusion_pruning_amd import _lib
    p = _lib.LossStageParams()
    p.n_terms, p.n_groups, p.n_grads = n_terms, n_groups, n_grads
    p.valid, p.w, p.partial, p.out, p.g = 4096, 4096, 4096, 4096, 4096
    for i in range(min(n_terms, 16)):
        _term(p.terms[i], 3, 4, 16)
    for i in range(min(n_grads, 16)):
        p.grads[i].grad_out, p.grads[i].ldg, p.grads[i].term0, p.grads[i].term1 = 4096, 0, max(0, min(i, n_terms - 1)), -1
    return p


def bad_tables():
    """(what, parameter block, word of the message, True where only the backward entry refuses it)"""
    cases = []

    def add(what, word, bwd_only=False, **kw):
        p = table(**kw)
        cases.append((what, p, word, bwd_only))
        return p
    add("no terms", b"n_terms", n_terms=0)
    add("17 terms", b"n_terms", n_terms=17)
    add("no groups", b"n_groups", n_groups=0)
    _term(add("null a", b"null operand").terms[0], 3, 4, 16, a=0)
    _term(add("null b", b"null operand").terms[0], 3, 4, 16, b=0)
    _term(add("C % 8", b"multiple of 8").terms[0], 3, 4, 12)
    _term(add("pitch below C", b"leading dimensions").terms[0], 3, 4, 16, lda=8)
    _term(add("pitch % 8", b"leading dimensions").terms[0], 3, 4, 16, ldb=20)
    _term(add("a alignment", b"16-byte aligned").terms[0], 3, 4, 16, a=4096 + 8)
    _term(add("b alignment", b"16-byte aligned").terms[0], 3, 4, 16, b=8192 + 4)
    _term(add("group", b"group").terms[0], 3, 4, 16, group=1)
    add("rows_per_sample 0", b"rows_per_sample").terms[0].rows_per_sample = 0
    add("rows % rows_per_sample", b"rows_per_sample").terms[0].rows = 13
    _term(add("B differs", b"B differs", n_terms=2).terms[1], 4, 4, 16)
    _term(add("B above 1024", b"samples").terms[0], 1025, 4, 16)
    p = add("weighted without w", b"w is null")
    p.terms[0].weighted, p.w = 1, None
    add("null valid", b"valid").valid = None
    add("no gradient items", b"n_grads", True, n_grads=0)
    add("17 gradient items", b"n_grads", True, n_grads=17)
    add("term index", b"term index", True).grads[0].term0 = 1
    add("same term twice", b"term index", True).grads[0].term1 = 0
    p = add("different first operands", b"different first operands", True, n_terms=2)
    _term(p.terms[1], 3, 4, 16, a=4096 + 64)
    p.grads[0].term1 = 1
    add("null grad_out", b"grad_out", True).grads[0].grad_out = None
    add("grad_out alignment", b"grad_out", True).grads[0].grad_out = 4096 + 8
    add("gradient pitch", b"leading dimension", True).grads[0].ldg = 12
    add("null g", b"g", True).g = None
    return cases


def test_bad_tables_are_refused_without_a_launch(lib):
    cases = bad_tables()
    assert len(cases) >= 20
    for what, p, word, bwd_only in cases:
        if not bwd_only:
            assert lib.aptp_loss_stage(ctypes.byref(p), None) == -1, what
            assert word in lib.aptp_last_error(), (what, lib.aptp_last_error())
            assert lib.aptp_loss_stage_nblocks(ctypes.byref(p)) == 0 and lib.aptp_loss_stage_scratch_floats(ctypes.byref(p)) == 0
        assert lib.aptp_loss_stage_bwd(ctypes.byref(p), None) == -1, what
        assert word in lib.aptp_last_error(), (what, lib.aptp_last_error())
    good = table(2, 1, 1)
    good.grads[0].term1 = 1
    want = 2 * 3 * lib.aptp_mse_nblocks(4, 16)
    assert lib.aptp_loss_stage_nblocks(ctypes.byref(good)) == want
    assert lib.aptp_loss_stage_scratch_floats(ctypes.byref(good)) == want + 2 * 3
    assert lib.aptp_loss_stage_bwd_nblocks(ctypes.byref(good)) == 3


def _static(B=4):
    g = torch.Generator().manual_seed(1)
    st = {"noisy_latents": torch.randn(B, 4, 2, 2, generator=g), "timesteps": torch.arange(B), "target": torch.randn(B, 4, 2, 2, generator=g),
          "encoder_hidden_states": torch.randn(B, 3, 8, generator=g), "valid": torch.full((B,), 7.0)}
    return st


def _batch(n, seed):
    g = torch.Generator().manual_seed(seed)
    return {"noisy_latents": torch.randn(n, 4, 2, 2, generator=g), "timesteps": torch.arange(10, 10 + n),
            "target": torch.randn(n, 4, 2, 2, generator=g), "encoder_hidden_states": torch.randn(n, 3, 8, generator=g)}


def test_a_short_batch_is_padded_with_its_own_first_row():
    from diffusion_pruning_amd.train_step import _BATCH_KEYS, _stage_short_batch
    st = _static()
    st["target"][3] = float("nan")                       # what an earlier batch left behind
    before = {k: v.clone() for k, v in st.items()}
    assert _stage_short_batch(st, _batch(0, 2)) == 0
    assert all(torch.equal(st[k], before[k]) or k == "target" for k in st) and bool(st["target"][3].isnan().all())
    b = _batch(2, 3)
    assert _stage_short_batch(st, b) == 2
    for k in _BATCH_KEYS:
        assert torch.equal(st[k][:2], b[k]) and torch.equal(st[k][2], b[k][0]) and torch.equal(st[k][3], b[k][0])
        assert bool(torch.isfinite(st[k].double()).all())
    assert st["valid"].tolist() == [1.0, 1.0, 0.0, 0.0]
    b = _batch(4, 4)
    assert _stage_short_batch(st, tuple(b[k] for k in _BATCH_KEYS)) == 4 and st["valid"].tolist() == [1.0] * 4
    b["valid"] = torch.tensor([1.0, 0.0, 1.0, 1.0])
    assert _stage_short_batch(st, b) == 4 and st["valid"].tolist() == [1.0, 0.0, 1.0, 1.0]
    b3 = _batch(3, 5)
    b3["valid"] = torch.tensor([0.0, 1.0, 1.0])
    assert _stage_short_batch(st, b3) == 3 and st["valid"].tolist() == [0.0, 1.0, 1.0, 0.0]
    with pytest.raises(ValueError, match="does not fit"):
        _stage_short_batch(st, _batch(5, 6))
    with pytest.raises(ValueError, match="empty batch"):
        _stage_short_batch(st, _batch(0, 7), data_parallel=True)
