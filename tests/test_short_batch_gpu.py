"""GPU checks of GraphedFineTunerStep(short_batches=True): the captured batch size is a maximum, the losses are means over the
samples present (ops.LossStage as one autograd node), and the rows behind them are padding that reaches nothing.  Tiny expert
(O.TINY), 16x16 latents, captured for B = 4 -- the set-up of tests/test_grad_accum_gpu.py."""
import contextlib
import gc

import numpy as np
import pytest
import torch

from oracle import unet_oracle as O
from tests import loss_stage_model as M
from tests import test_grad_accum_gpu as GA

pytestmark = pytest.mark.gpu
from tests.margins import check  # noqa: E402

KW = GA.KW
FROZEN = dict(lr=0.0, weight_decay=0.0)          # such a step never moves its parameters: its gradients are a pure function of the batch
B = 4


@contextlib.contextmanager
def _gc_off():
    """a module fixture is set up before the per-test fixture that turns the collector off: a capture inside it must not meet
    a collection either (tests/conftest.py says why)"""
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def _students(cuda, n):
    """n pruned students with the same weights and mask, and their dense teacher"""
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    mask = O.random_mask(O.TINY, 0.6, 9, n_depth_off=1)
    built = [GA.build(cuda, mask) for _ in range(n)]
    cfg, params = built[0][0], built[0][2]
    teacher = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                        cross_attention_dim=cfg.cross_attention_dim)
    teacher.load_state_dict({k: v.detach() for k, v in params.items()})
    teacher.to(cuda).freeze()
    teacher.set_structure({k: [v.to(cuda) for v in vs] for k, vs in O.ones_mask(cfg).items()})
    return cfg, [b[1] for b in built], teacher


def _batches(cuda, cfg, seeds, n=B):
    from diffusion_pruning_amd.train_step import synthetic_batch
    return [synthetic_batch(n, 16, cuda, seed=s, cross_dim=cfg.cross_attention_dim) for s in seeds]


def _rows(batch, n):
    return {k: v[:n].clone() for k, v in batch.items()}


def _grads(step):
    return [p.grad.detach().flatten().clone() for p in step.trainer.parameters()]


def _losses(out):
    return [out[k].clone() for k in ("loss", "diff_loss", "distillation_loss", "block_loss")]


@pytest.fixture(scope="module")
def frozen(cuda):
    """three steps that never move (lr = 0) on identical students: the switch on at B = 4, the default step at B = 4 and at B = 3"""
    from diffusion_pruning_amd import graph_utils
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    cfg, (s_on, s_off4, s_off3), teacher = _students(cuda, 3)
    batches = _batches(cuda, cfg, (4, 5, 6))
    graph_utils.KEEP_GRAPHS = True
    try:
        with _gc_off():
            on = GraphedFineTunerStep(s_on, teacher, short_batches=True, **FROZEN).capture(batches[0])
            off4 = GraphedFineTunerStep(s_off4, teacher, **FROZEN).capture(batches[0])
            off3 = GraphedFineTunerStep(s_off3, teacher, **FROZEN).capture(_rows(batches[0], 3))
    finally:
        graph_utils.KEEP_GRAPHS = False
    return dict(on=on, off4=off4, off3=off3, batches=batches, cfg=cfg)


def test_switch_off_is_the_existing_step(cuda):
    from diffusion_pruning_amd import graph_utils
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    cfg, (sa, sb), teacher = _students(cuda, 2)
    batches = _batches(cuda, cfg, (4, 5))
    graph_utils.KEEP_GRAPHS = True
    try:
        plain = GraphedFineTunerStep(sa, teacher, **KW).capture(batches[0])
        off = GraphedFineTunerStep(sb, teacher, short_batches=False, **KW).capture(batches[0])
    finally:
        graph_utils.KEEP_GRAPHS = False
    nodes = plain.graph_nodes()
    assert nodes == off.graph_nodes() and nodes["student_bwd"] is not None and nodes["student_bwd"] > 0
    assert "valid" not in off._cap["st"] and "stage" not in off._cap and off.short_batches is False
    for b in batches:
        o1, o2 = plain.train_step(None, b), off.train_step(None, b)
        assert set(o1) == set(o2) and "n_valid" not in o2
        assert all(torch.equal(x, y) for x, y in zip(_losses(o1), _losses(o2)))
    torch.cuda.synchronize()
    assert GA._state_equal(off, GA._state(plain)) and float(off.optimizer.step_t) == 2.0
    with pytest.raises(RuntimeError):
        off.train_step(None, _rows(batches[0], 3))          # the default step takes the captured size only


def test_padding_reaches_nothing(frozen):
    """n = 3 of 4 through an explicit `valid`: the fourth row handed over differs, losses and every packed gradient do not"""
    S, batches = frozen["on"], frozen["batches"]
    valid = torch.tensor([1.0, 1.0, 1.0, 0.0], device=batches[0]["target"].device)
    got = []
    for other in (batches[1], batches[2]):
        b = {k: v.clone() for k, v in batches[0].items()}
        for k in b:
            b[k][3] = other[k][1]
        b["valid"] = valid
        out = S.train_step(None, b)
        torch.cuda.synchronize()
        assert float(out["n_valid"]) == 3.0 and out["skipped"] is False
        got.append((_losses(out), _grads(S)))
    assert not torch.equal(batches[1]["target"][1], batches[2]["target"][1])
    assert all(torch.equal(x, y) for x, y in zip(got[0][0], got[1][0]))
    assert all(torch.equal(x, y) for x, y in zip(got[0][1], got[1][1]))
    assert sum(float(g.abs().max()) > 0 for g in got[0][1]) >= len(got[0][1]) // 2
    # and the same three samples through the normal path (padding: their own first row) give the same bits again
    out = S.train_step(None, _rows(batches[0], 3))
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(_losses(out), got[0][0]))
    assert all(torch.equal(x, y) for x, y in zip(_grads(S), got[0][1]))


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def test_losses_of_a_short_batch_against_the_fp64_model(frozen):
    """n = 3 through the normal path; the four losses against the fp64 model on the step's own captured tensors, rows 0..2.
    Bound: the fp32 roundings on each value's path, counted from the stage's table (tests/loss_stage_model.py), times 2^-24"""
    S, batches = frozen["on"], frozen["batches"]
    out = S.train_step(None, _rows(batches[1], 3))
    torch.cuda.synchronize()
    assert float(out["n_valid"]) == 3.0 and out["applied"] is True
    cap, cfg = S._cap, S.cfg
    assert cap["st"]["valid"].tolist() == [1.0, 1.0, 1.0, 0.0]
    for k in ("noisy_latents", "target", "encoder_hidden_states", "timesteps"):
        assert torch.equal(cap["st"][k][3], batches[1][k][0])                  # the pad is this batch's first row
    keys = list(cap["student_acts"])
    terms = [dict(a=_np(cap["pred"][:3]), b=_np(cap["st"]["target"][:3]), group=0, scale=1.0, weighted=True)]
    terms += [dict(a=_np(cap["student_acts"][k][:3]), b=_np(cap["teacher_acts"][k][:3]), group=1, scale=1.0, weighted=False) for k in keys]
    terms.append(dict(a=_np(cap["pred"][:3]), b=_np(cap["full_pred"][:3]), group=2, scale=1.0, weighted=False))
    coef = (cfg.diffusion_weight, cfg.block_weight, cfg.distillation_weight)
    fw = M.forward(terms, [1.0] * 3, _np(cap["st"]["snr_w"][:3]), coef, (0.0, float(len(keys)), 0.0))
    p = cap["stage"]._p
    assert p.n_terms == len(terms) and len(keys) >= 3
    path = [M.unit_ops(p.terms[t].rows_per_sample, p.terms[t].C) + M.term_ops(B, bool(p.terms[t].weighted)) for t in range(p.n_terms)]
    bounds = {"diff_loss": path[0] + M.group_ops(1, False), "block_loss": max(path[1:-1]) + M.group_ops(len(keys), True),
              "distillation_loss": path[-1] + M.group_ops(1, False)}
    bounds["loss"] = max(bounds.values()) + M.total_ops(3)
    exact = {"diff_loss": fw["groups"][0], "block_loss": fw["groups"][1], "distillation_loss": fw["groups"][2], "loss": fw["total"]}
    for k, want in exact.items():
        err = abs(float(out[k]) - want) / want
        print("%s: %.9g vs %.9g, rel err %.3e of %.3e" % (k, float(out[k]), want, err, bounds[k] * M.EPS))
        check(err, bounds[k] * M.EPS, "short batch 3 of 4: %s vs fp64 on the captured tensors" % k)


def _compare(step, ref, what):
    names = [n for n, _ in step.trainer.named_parameters()]
    errs, got_all, ref_all = {}, [], []
    for name, got, want in zip(names, _grads(step), _grads(ref)):
        assert torch.isfinite(got).all() and got.shape == want.shape, name
        errs[name] = GA.rel_l2(got, want)
        got_all.append(got)
        ref_all.append(want)
    e_all = GA.rel_l2(torch.cat(got_all), torch.cat(ref_all))
    worst = sorted(errs.items(), key=lambda kv: -kv[1])
    print("%s: all tensors %.3e; worst %s" % (what, e_all, [(n, "%.3e" % e) for n, e in worst[:5]]))
    check(e_all, 0.12, what + ": all packed gradients")
    check(worst[0][1], 0.12, what + ": worst packed tensor " + worst[0][0])


def test_gradients_of_a_short_batch_against_the_exact_batch(frozen):
    """3 of 4 with the switch on against the default step captured at exactly B = 3 on the same samples.  Cap 0.12 = the triangle
    bound of two bf16-pipeline gradients budgeted at 6e-2 each (test_window_against_one_large_batch)"""
    S, R, batches = frozen["on"], frozen["off3"], frozen["batches"]
    three = _rows(batches[2], 3)
    o1, _ = S.train_step(None, three), R.train_step(None, three)
    torch.cuda.synchronize()
    assert float(o1["n_valid"]) == 3.0
    _compare(S, R, "3 of 4 vs the step captured at 3")


def test_full_batch_against_the_default_step(frozen):
    S, D, batches = frozen["on"], frozen["off4"], frozen["batches"]
    o1, _ = S.train_step(None, batches[1]), D.train_step(None, batches[1])
    torch.cuda.synchronize()
    assert float(o1["n_valid"]) == 4.0
    _compare(S, D, "4 of 4 vs the default step")
    on, off = S.graph_nodes(), D.graph_nodes()
    print("loss-and-backward graph nodes: default %s, short_batches %s" % (off["student_bwd"], on["student_bwd"]))
    assert on["teacher"] == off["teacher"] and on["student_fwd"] == off["student_fwd"]
    assert on["student_bwd"] < off["student_bwd"]           # one fused stage in place of two or three launches per term and sample


@pytest.fixture(scope="module")
def live(cuda):
    """a step that trains, switch on, captured for B = 4"""
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    cfg, (s,), teacher = _students(cuda, 1)
    batches = _batches(cuda, cfg, (4, 5, 6, 7))
    with _gc_off():
        step = GraphedFineTunerStep(s, teacher, short_batches=True, **KW).capture(batches[0])
    return step, batches


def test_empty_batch_touches_nothing(live):
    L, batches = live
    L.train_step(None, batches[0])
    torch.cuda.synchronize()
    snap, t0 = GA._state(L), float(L.optimizer.step_t)
    out = L.train_step(None, _rows(batches[1], 0))
    torch.cuda.synchronize()
    assert out["skipped"] is True and out["applied"] is False and out["accum_index"] == 0 and float(out["n_valid"]) == 0.0
    assert float(out["loss"]) == 0.0 and GA._state_equal(L, snap) and L.accum_index == 0
    out = L.train_step(None, batches[1])
    torch.cuda.synchronize()
    assert out["skipped"] is False and out["applied"] is True and float(out["n_valid"]) == 4.0 and torch.isfinite(out["loss"])
    assert float(L.optimizer.step_t) == t0 + 1.0
    moved = sum(float((p.detach() - s).abs().max()) > 0 for p, s in zip(L.trainer.parameters(), snap[0]))
    assert moved >= len(snap[0]) // 2


def test_nan_sample_skips_the_step_and_does_not_linger(live):
    L, batches = live
    L.train_step(None, batches[0])
    torch.cuda.synchronize()
    snap, t0 = GA._state(L), float(L.optimizer.step_t)
    bad = _rows(batches[2], 3)
    bad["target"][1, 0, 0, 0] = float("nan")
    out = L.train_step(None, bad)
    torch.cuda.synchronize()
    assert not torch.isfinite(out["loss"]) and float(out["n_valid"]) == 3.0
    assert GA._state_equal(L, snap)                          # the NaN guard: parameters, moments and step count as they were
    out = L.train_step(None, _rows(batches[3], 2))           # rows 2 and 3 are padded with THIS batch's first row
    torch.cuda.synchronize()
    assert torch.isfinite(out["loss"]) and float(out["n_valid"]) == 2.0 and float(L.optimizer.step_t) == t0 + 1.0
    assert all(torch.isfinite(p).all() for p in L.trainer.parameters())
    assert bool(torch.isfinite(L._cap["st"]["target"]).all())
    moved = sum(float((p.detach() - s).abs().max()) > 0 for p, s in zip(L.trainer.parameters(), snap[0]))
    assert moved >= len(snap[0]) // 2


def test_a_window_with_a_short_micro_batch_is_the_sum_of_its_parts(cuda, frozen):
    """accumulation_steps = 2, a full micro-batch and one of 3: the arena after the window is the sum of the two single-step
    gradients, bit for bit (what test_window_is_the_sum_of_its_micro_batches asserts), and the optimizer applies half of it:
    the mean of the micro-batches' means"""
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    S, batches = frozen["on"], frozen["batches"]
    cfg, (sa,), teacher = _students(cuda, 1)
    A = GraphedFineTunerStep(sa, teacher, accumulation_steps=2, short_batches=True, **KW).capture(batches[0])
    arena, offs = A.trainer.grad_arena, A.trainer.grad_offsets
    micro = [batches[1], _rows(batches[2], 3)]

    def gather(step, loss):
        flat = torch.zeros_like(arena)
        flat[0] = loss
        for p, o in zip(step.trainer.parameters(), offs):
            flat[o:o + p.numel()] = p.grad.reshape(-1)
        return flat
    gs = []
    for b in micro:
        out = S.train_step(None, b)
        torch.cuda.synchronize()
        gs.append(gather(S, out["loss"]))
    init = GA._state(A)
    for i, b in enumerate(micro):
        out = A.train_step(None, b)
        torch.cuda.synchronize()
        assert out["accum_index"] == i and out["applied"] is (i == 1) and float(out["n_valid"]) == (4.0, 3.0)[i]
        if i == 0:
            assert GA._state_equal(A, init)
    total = gs[0] + gs[1]
    assert torch.equal(arena[64:], total[64:]) and torch.equal(arena[0], total[0])
    assert torch.equal(arena[64:] * 0.5, (gs[0][64:] + gs[1][64:]) * 0.5)
    assert float(A.optimizer.step_t) == 1.0 and A.accum_index == 0
    # an empty micro-batch inside a window leaves the window where it is
    A.train_step(None, micro[0])
    out = A.train_step(None, _rows(batches[0], 0))
    assert out["skipped"] is True and out["accum_index"] == 1 and A.accum_index == 1
    out = A.train_step(None, micro[1])
    torch.cuda.synchronize()
    assert out["applied"] is True and float(A.optimizer.step_t) == 2.0


def test_bad_batches_raise(cuda, live):
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    L, batches = live
    snap = GA._state(L)
    five = {k: torch.cat([v, v[:1]], 0) for k, v in batches[0].items()}
    with pytest.raises(ValueError, match="does not fit"):
        L.train_step(None, five)
    torch.cuda.synchronize()
    assert GA._state_equal(L, snap)
    cfg, (s,), teacher = _students(cuda, 1)
    dp = GraphedFineTunerStep(s, teacher, data_parallel=True, bucket_bytes=1 << 20, short_batches=True, **KW).capture(batches[0])
    with pytest.raises(ValueError, match="empty batch"):
        dp.train_step(None, _rows(batches[0], 0))
    out = dp.train_step(None, _rows(batches[1], 3))
    torch.cuda.synchronize()
    assert float(out["n_valid"]) == 3.0 and torch.isfinite(out["loss"]) and float(dp.optimizer.step_t) == 1.0
