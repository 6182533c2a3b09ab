"""GPU checks of the seeded router noise in the pruning steps (GraphedPrunerStep(router_seed=), PrunerStep.step(seeds=); DESIGN
6za).  The set-up is tests/test_pruner_short_batch_gpu.py's: tiny U-Net, 16 x 16 latents, n_e = 4, B = 4.  The switch off is the
existing step; the captured seeded router equals the eager seeded one; a short step equals the eager step on those samples with
their own seeds, nothing shared by hand; the host generator is never touched; a run resumes bit for bit from state_dict()s and
`noise_steps`; the seeded router graph is smaller; what cannot be served is refused.
Tolerances where two different computations are compared are the project's own for captured-against-eager pruning steps: losses
2e-3 * |x| + 1e-5, rel-L2 2e-2."""
import copy

import pytest
import torch

from tests.test_pruner_short_batch_gpu import B, LOSSES, cut, done, params_of, world  # noqa: F401  (world: the module's fixture)
from tests.test_train_step_gpu import rel_l2

pytestmark = pytest.mark.gpu
from tests.margins import check  # noqa: E402

ROUTER_SEED = 4242
SEEDS = [[(1 << 33) + 17 * i + 100 * k for i in range(B)] for k in range(4)]      # one list per batch, above 2^32
DRAWS = [0, 5, 6, 9]


def make(world, *, router_seed=ROUTER_SEED, short=None, captured=True, overlap=True, state=None, **kw):
    """a fresh copy of the router (or of `state` = (hyper-net, quantiser, optimizer) state_dict()s) under a GraphedPrunerStep
    captured for B = 4, and its RouterAdamW"""
    from diffusion_pruning_amd.router_optim import RouterAdamW
    from diffusion_pruning_amd.train_step import GraphedPrunerStep
    hn, qz = copy.deepcopy(world["hn"]), copy.deepcopy(world["qz"])
    if state is not None:
        hn.load_state_dict(state[0])
        qz.load_state_dict(state[1])
    kw = dict(kw, **({} if short is None else {"short_batches": short}))
    if router_seed != "default":
        kw["router_seed"] = router_seed
    step = GraphedPrunerStep(world["unet"], hn, qz, **kw)
    step.overlap_router = overlap
    step.count_macs(16)
    opt = RouterAdamW([{"params": [p for p in hn.parameters() if p.requires_grad], "lr": 1e-3, "weight_decay": 0.0},
                       {"params": [p for p in qz.parameters() if p.requires_grad], "lr": 1e-3, "weight_decay": 0.0}])
    if state is not None:
        opt.load_state_dict(state[2])
    torch.manual_seed(77)
    step.capture(world["batches"][0], optimizer=opt if captured else None)
    return step, opt


def seeded(world, i, cuda, n=B, rows=None):
    """batch i (mod 3) with its seeds on the device and its draw; `rows`: the samples kept (default: the first n)"""
    rows = list(range(n)) if rows is None else rows
    b = {k: v[rows] for k, v in world["batches"][i % 3].items()}
    b["seeds"] = torch.tensor([SEEDS[i][r] for r in rows], dtype=torch.int64, device=cuda)
    b["draw"] = DRAWS[i]
    return b


def test_switch_off_is_the_existing_step(cuda, world, monkeypatch):
    from diffusion_pruning_amd import graph_utils
    monkeypatch.setattr(graph_utils, "KEEP_GRAPHS", True)
    runs = []
    for router_seed in ("default", None):
        step, opt = make(world, router_seed=router_seed)
        nodes = step.graph_nodes()
        torch.manual_seed(99)
        losses = []
        for b in world["batches"]:
            o = step.train_step(opt, b)                                # no "seeds" in the batch: none are asked for
            losses.append([o[k].clone() for k in LOSSES])
        step.finish()
        torch.cuda.synchronize()
        ph = step._cap["router"][False]
        assert ph["tape"] is not None and ph["noise"] is None and "noise" not in step._cap["st"] and step.noise_steps == 0
        runs.append((nodes, losses, params_of(step)))
        done(step)
    (na, la, pa), (nb, lb, pb) = runs
    assert na == nb and all(v is not None for v in na.values()), (na, nb)
    assert all(torch.equal(x, y) for a, b in zip(la, lb) for x, y in zip(a, b)) and torch.equal(pa, pb)


def _three_steps(world, cuda, captured, overlap=True, sizes=(4, 4, 4), short=None):
    step, opt = make(world, captured=captured, overlap=overlap, short=short)
    p0 = params_of(step)
    losses, grads = [], []
    for i, n in enumerate(sizes):
        o = step.train_step(opt, seeded(world, i, cuda, n))
        step.finish()
        losses.append({k: o[k].clone() for k in LOSSES})
        grads.append((step._cap["grad"].clone(), o["arch_vector_quantized"].clone()))
    step.finish()
    torch.cuda.synchronize()
    assert step.noise_steps == len(sizes)
    out = (losses, params_of(step), p0, grads, step.graph_nodes())
    done(step)
    return out


def _compare(la, pa, p0, lb, pb, what):
    for i, (a, b) in enumerate(zip(la, lb)):
        for k in LOSSES:
            check(abs(float(a[k]) - float(b[k])), 2e-3 * abs(float(a[k])) + 1e-5, "%s: step %d %s" % (what, i, k))
    assert float((pa - p0).abs().max()) > 0
    check(rel_l2(pb - p0, pa - p0), 2e-2, "%s: parameter change rel-L2" % what)


def test_captured_seeded_router_equals_the_eager_seeded_router(cuda, world, monkeypatch):
    from diffusion_pruning_amd import graph_utils
    monkeypatch.setattr(graph_utils, "KEEP_GRAPHS", True)
    la, pa, p0, ga, _ = _three_steps(world, cuda, captured=False)
    lb, pb, _, gb, nodes = _three_steps(world, cuda, captured=True)
    _compare(la, pa, p0, lb, pb, "seeded: captured vs eager router")
    check(rel_l2(gb[0][0], ga[0][0]), 2e-2, "seeded: captured vs eager router: cap['grad'] of step 0")
    # the router's gradients of the first step, through its effect: one AdamW step from equal parameters and zero moments
    bit_equal = all(torch.equal(a[k], b[k]) for a, b in zip(la, lb) for k in LOSSES) and torch.equal(pa, pb)
    print("seeded captured vs eager router: bit-equal losses and parameters: %s" % bit_equal)
    print("seeded captured vs eager: same codes at every step: %s" % all(torch.equal(x[1], y[1]) for x, y in zip(ga, gb)))
    lc, pc, _, _, _ = _three_steps(world, cuda, captured=True, overlap=False)
    assert all(torch.equal(b[k], c[k]) for b, c in zip(lb, lc) for k in LOSSES) and torch.equal(pb, pc)
    # the seeded router graph against the unseeded one: strictly fewer nodes (reported, not bounded otherwise)
    plain, _ = make(world, router_seed=None)
    n0 = plain.graph_nodes()
    done(plain)
    print("graph nodes unseeded %s seeded %s" % (n0, nodes))
    assert nodes["router_fwd"] < n0["router_fwd"], (nodes, n0)
    assert {k: nodes[k] for k in ("teacher", "student_fwd", "student_bwd")} == {k: n0[k] for k in ("teacher", "student_fwd", "student_bwd")}


def test_router_gradients_of_a_seeded_step(cuda, world):
    """the eager-router step of a GraphedPrunerStep against the plain PrunerStep, both seeded: losses, the gradient w.r.t. the
    code and the router's own gradients"""
    from diffusion_pruning_amd.train_step import PrunerStep
    step, _ = make(world, captured=False)
    b = seeded(world, 1, cuda)
    args = [b[k] for k in ("noisy_latents", "timesteps", "encoder_hidden_states", "mpnet_embeddings", "target")]
    for p in step.trainable_parameters():
        p.grad = None
    o = step.step(*args, seeds=b["seeds"], draw=b["draw"], noise_step=3)
    step.backward(o)
    torch.cuda.synchronize()
    got = {k: float(o[k]) for k in LOSSES}
    got_codes = o["arch_vector_quantized"].clone()
    got_grads = [None if p.grad is None else p.grad.clone() for p in step.trainable_parameters()]
    resource_p = step.resource.p
    done(step)
    eager = PrunerStep(world["unet"], copy.deepcopy(world["hn"]), copy.deepcopy(world["qz"]), router_seed=ROUTER_SEED)
    eager.resource.p = resource_p
    eager.count_macs(16)
    w = eager.step(*args, seeds=b["seeds"].tolist(), draw=b["draw"], noise_step=3)
    w["loss"].backward()
    torch.cuda.synchronize()
    assert torch.equal(got_codes, w["arch_vector_quantized"])          # the same noise: the same codes, bit for bit
    for k in LOSSES:
        check(abs(got[k] - float(w[k])), 2e-3 * abs(float(w[k])) + 1e-5, "seeded graphed vs plain eager step: %s" % k)
    both = [(g, p.grad) for g, p in zip(got_grads, eager.trainable_parameters()) if p.grad is not None]
    assert both and all(g is not None for g, _ in both)
    check(rel_l2(torch.cat([g.flatten() for g, _ in both]), torch.cat([r.flatten() for _, r in both])), 2e-2,
          "seeded graphed vs plain eager step: router gradients")
    # another noise_step moves the codebook's noise only; another draw the samples'
    w2 = eager.step(*args, seeds=b["seeds"].tolist(), draw=b["draw"], noise_step=4)
    assert not torch.equal(w2["arch_vector_quantized"], w["arch_vector_quantized"])
    with pytest.raises(ValueError, match="seeds for"):
        eager.step(*args, seeds=b["seeds"].tolist()[:3], draw=0, noise_step=0)
    plain = PrunerStep(world["unet"], eager.hyper_net, eager.quantizer)
    with pytest.raises(ValueError, match="router_seed"):
        plain.step(*args, seeds=b["seeds"].tolist())
    plain.remove_hooks()
    eager.remove_hooks()


@pytest.mark.parametrize("pretrain", [True, False])
def test_short_seeded_step_is_the_step_on_those_samples(cuda, world, pretrain):
    """3 of 4: no noise rows are shared by hand -- each sample's noise comes from its own seed in either step"""
    from diffusion_pruning_amd.train_step import PrunerStep
    short, _ = make(world, short=True, captured=False)
    b3 = seeded(world, 1, cuda, 3)
    args = [b3[k] for k in ("noisy_latents", "timesteps", "encoder_hidden_states", "mpnet_embeddings", "target")]
    for p in short.trainable_parameters():
        p.grad = None
    o = short.step(*args, pretrain=pretrain, seeds=b3["seeds"], draw=b3["draw"], noise_step=7)
    short.backward(o)
    torch.cuda.synchronize()
    got = {k: float(o[k]) for k in LOSSES}
    got_codes = o["arch_vector_quantized"][:3].clone()
    got_grads = [None if p.grad is None else p.grad.clone() for p in short.trainable_parameters()]
    assert float(o["n_valid"]) == 3.0
    staged = short._cap["st"]["noise"].seeds_dev.tolist()
    assert staged == b3["seeds"].tolist() + [int(b3["seeds"][0])]     # the row behind the batch repeats seed 0 of the batch
    resource_p = short.resource.p
    done(short)
    eager = PrunerStep(world["unet"], copy.deepcopy(world["hn"]), copy.deepcopy(world["qz"]), router_seed=ROUTER_SEED)
    eager.resource.p = resource_p
    eager.count_macs(16)
    w = eager.step(*args, pretrain=pretrain, seeds=b3["seeds"], draw=b3["draw"], noise_step=7)
    w["loss"].backward()
    torch.cuda.synchronize()
    assert torch.equal(got_codes, w["arch_vector_quantized"]), "the three samples were assigned other codes"
    for k in LOSSES:
        print("pretrain=%s %s: short %.6e eager on 3 rows %.6e" % (pretrain, k, got[k], float(w[k])))
        check(abs(got[k] - float(w[k])), 2e-3 * abs(float(w[k])) + 1e-5, "seeded short step vs eager step on the 3 samples: %s (pretrain=%s)" % (k, pretrain))
    both = [(g, p.grad) for g, p in zip(got_grads, eager.trainable_parameters()) if p.grad is not None]
    assert all(g is not None for g, _ in both) and both
    e = rel_l2(torch.cat([g.flatten() for g, _ in both]), torch.cat([r.flatten() for _, r in both]))
    print("pretrain=%s router gradients rel-L2 %.3e" % (pretrain, e))
    check(e, 2e-2, "seeded short step vs eager step on the 3 samples: router gradients (pretrain=%s)" % pretrain)
    eager.remove_hooks()


def test_a_samples_noise_does_not_depend_on_who_was_dropped(cuda, world):
    """two captured short steps that keep samples 0 and 1 and drop another one each: the kept samples' noise rows -- of the
    relaxation and of the assignment -- are the same bits, and those of a batch of one"""
    from diffusion_pruning_amd import ops
    step, opt = make(world, short=True)
    ph = step._cap["router"][False]
    E = step.quantizer.vq_embed_dim
    seen = []
    for rows in ([0, 1, 2], [0, 1, 3]):
        step.noise_steps = 5
        b = seeded(world, 1, cuda, rows=rows)
        o = step.train_step(opt, b)
        step.finish()
        torch.cuda.synchronize()
        assert float(o["n_valid"]) == 3.0 and ph["noise"].seeds_dev.tolist() == b["seeds"].tolist() + [int(b["seeds"][0])]
        assert ph["noise"].draw_dev.tolist() == [DRAWS[1]] and ph["noise"].step_dev.tolist() == [5] and step.noise_steps == 6
        seen.append([ops.philox_gumbel((B, E), ph["noise"].seeds_dev, ph["noise"].draw_dev, sub).clone() for sub in (6, 7)])
    for a, b_ in zip(*seen):
        assert torch.equal(a[:2], b_[:2]) and not torch.equal(a[2], b_[2])
    alone = ops.philox_gumbel((1, E), [SEEDS[1][1]], DRAWS[1], 7, device=cuda)
    assert torch.equal(alone[0], seen[0][1][1])
    done(step)


def test_the_host_generator_is_untouched(cuda, world):
    torch.manual_seed(2024)
    before = torch.get_rng_state()
    step, opt = make(world, short=True)
    # (make() seeds the generator itself before capture(): the state to compare with is the one right after that)
    torch.manual_seed(77)
    at_capture = torch.get_rng_state()
    step2, opt2 = make(world)
    assert torch.equal(torch.get_rng_state(), at_capture)              # capture() drew nothing and restored nothing
    step2.capture_router(world["batches"][0], True)
    for i in range(3):
        step2.train_step(opt2, seeded(world, i, cuda), pretrain=(i == 1))
        step.train_step(opt, seeded(world, i, cuda, 4 - i))
    step.finish()
    step2.finish()
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), at_capture) and not torch.equal(before, at_capture)
    for s in (step, step2):
        rt = s._cap["router"]
        for ph in (rt[k] for k in (True, False) if k in rt):
            assert ph["tape"] is None and ph["noise"] is not None
        done(s)


def test_resume_is_bit_exact(cuda, world):
    def run(step, opt, first, count):
        last = None
        for i in range(first, first + count):
            last = step.train_step(opt, seeded(world, i, cuda))
        step.finish()
        torch.cuda.synchronize()
        return {k: last[k].clone() for k in LOSSES}
    whole, opt = make(world)
    l4 = run(whole, opt, 0, 4)
    p4 = params_of(whole)
    done(whole)
    first, opt1 = make(world)
    run(first, opt1, 0, 2)
    assert first.noise_steps == 2
    state = (copy.deepcopy(first.hyper_net.state_dict()), copy.deepcopy(first.quantizer.state_dict()), copy.deepcopy(opt1.state_dict()))
    done(first)
    torch.manual_seed(31337)                                            # the host generator carries nothing of the run
    second, opt2 = make(world, state=state)
    second.noise_steps = 2
    l22 = run(second, opt2, 2, 2)
    assert second.noise_steps == 4
    assert torch.equal(params_of(second), p4)
    assert all(torch.equal(l4[k], l22[k]) for k in LOSSES), (l4, l22)
    done(second)


def test_refusals(cuda, world, monkeypatch):
    from diffusion_pruning_amd.train_step import GraphedPrunerStep
    step, opt = make(world, short=True)
    step.train_step(opt, seeded(world, 0, cuda))
    step.finish()
    torch.cuda.synchronize()
    p0, static = params_of(step), {k: v.clone() for k, v in step._cap["st"].items() if torch.is_tensor(v)}
    ph = step._cap["router"][False]
    staged = [t.clone() for t in ph["noise"]] + [ph["text"].clone()]
    counters = opt.counters.clone()
    with pytest.raises(ValueError, match="seeds"):
        step.train_step(opt, world["batches"][1])                      # no "seeds": before any staging or replay
    bad = seeded(world, 1, cuda)
    bad["seeds"] = bad["seeds"][:3]
    with pytest.raises(ValueError, match="seeds"):
        step.train_step(opt, bad)
    bad = seeded(world, 1, cuda)
    bad["draw"] = 1 << 59
    with pytest.raises(ValueError, match="draw"):
        step.train_step(opt, bad)
    o = step.train_step(opt, seeded(world, 1, cuda, 0))                 # an empty batch advances nothing
    assert o["skipped"] is True
    step.finish()
    torch.cuda.synchronize()
    assert step.noise_steps == 1 and torch.equal(params_of(step), p0) and torch.equal(opt.counters, counters)
    assert all(torch.equal(v, static[k]) for k, v in step._cap["st"].items() if torch.is_tensor(v))
    assert all(torch.equal(a, b) for a, b in zip(staged, list(ph["noise"]) + [ph["text"]]))
    done(step)
    with pytest.raises(ValueError, match="router_seed"):
        GraphedPrunerStep(world["unet"], world["hn"], world["qz"], router_seed=1.5)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    with pytest.raises(NotImplementedError, match="process group"):
        GraphedPrunerStep(world["unet"], world["hn"], world["qz"], router_seed=7)
