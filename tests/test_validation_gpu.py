"""GPU checks of the validation pass of both training steps (train_step.py: FineTunerStep.eval_step,
GraphedFineTunerStep.capture_validation / validate, PrunerStep.eval_step / validate) against what a user could do before it
existed: `step` under torch.no_grad().  Block and distillation losses are the training step's, bit for bit; the diffusion loss
differs only by the order of its B-term weighted sum."""
import pytest
import torch

from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
from tests.margins import check  # noqa: E402

EPS = 2.0 ** -24
KEYS = ("loss", "diff_loss", "distillation_loss", "block_loss")
DEPTH_ORDER = [-1, -2, 0, 1, -3, -4, 2, 3, -5, -6, 4, 5, -7, 6]


# ---- the small builders of tests/test_finetune_gpu.py ------------------------------------------------------------------------
def build(cuda, mask):
    from diffusion_pruning_amd.unet import UNet2DConditionModelPruned
    cfg = O.TINY
    pm = UNet2DConditionModelPruned(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                    cross_attention_dim=cfg.cross_attention_dim).init_synthetic(seed=0)
    params = {k: v.detach().clone().requires_grad_() for k, v in pm.state_dict().items()}
    pm.to(cuda)
    pm.prune({k: [v.clone().to(cuda) for v in vs] for k, vs in mask.items()})
    return cfg, pm, params


def _two_students(cuda, mask):
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    cfg, a, params = build(cuda, mask)
    _, b, _ = build(cuda, mask)
    teacher = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                        cross_attention_dim=cfg.cross_attention_dim)
    teacher.load_state_dict({k: v.detach() for k, v in params.items()})
    teacher.to(cuda).freeze()
    teacher.set_structure({k: [v.to(cuda) for v in vs] for k, vs in O.ones_mask(cfg).items()})
    return cfg, a, b, teacher


def _batch(B, cuda, seed):
    from diffusion_pruning_amd.train_step import synthetic_batch
    return synthetic_batch(B, 16, cuda, seed=seed, cross_dim=O.TINY.cross_attention_dim)


def _args(b):
    return b["noisy_latents"], b["timesteps"], b["encoder_hidden_states"], b["target"]


def _diff_bound(B):
    """(1/B) sum_b w_b m_b from the same fp32 means and weights in two fp32 summation orders (the kernel: sequential
    multiply-adds and a scale; torch: products, its own sum, a division): B products, B - 1 additions and one scale of
    positive numbers -- (B + 2) 2^-24 relative, the bound of tests/test_loss_terms_gpu.py::test_weighted_term"""
    return (B + 2) * EPS


def test_eager_eval_step_against_step_under_no_grad(cuda):
    from diffusion_pruning_amd.packed_train import PackedTrainer
    from diffusion_pruning_amd.train_step import FineTunerStep, _min_snr_weights
    from diffusion_pruning_amd.losses import compute_snr
    mask = O.random_mask(O.TINY, 0.5, 8, n_depth_off=1)
    cfg, _, sb, teacher = _two_students(cuda, mask)
    B = 2
    batch = _batch(B, cuda, 4)
    step = FineTunerStep(sb, teacher)
    pk = PackedTrainer(sb).attach().materialize(*_args(batch)[:3])
    opt = torch.optim.SGD(pk.parameters(), lr=5e-2)
    for _ in range(2):
        step.train_step(opt, batch)
    with torch.no_grad():
        want = {k: v.clone() for k, v in step.step(*_args(batch)).items()}              # the parent's path
    got = step.eval_step(*_args(batch))
    torch.cuda.synchronize()
    assert set(got) == set(KEYS) and all(v.dim() == 0 and v.is_cuda and not v.requires_grad for v in got.values())
    assert torch.equal(got["distillation_loss"], want["distillation_loss"])
    assert torch.equal(got["block_loss"], want["block_loss"]) and float(got["block_loss"]) > 0
    # the fp32 weights of the two sides: step's inline expression against the helper eval_step calls
    ts, lc = batch["timesteps"], step.cfg
    snr = compute_snr(step.schedule, ts) + 1
    w_step = torch.stack([snr, lc.snr_gamma * torch.ones_like(ts)], dim=1).min(dim=1)[0] / snr
    w_eval = _min_snr_weights(lc, step.schedule, ts)
    w_diff = float(((w_step.double() - w_eval.double()).abs() / w_step.double()).max())
    assert w_step.dtype == torch.float32
    assert w_diff == 0.0          # measured on MI355X: the same torch expression on both sides, no term to add to the bound
    d, dw = float(got["diff_loss"]), float(want["diff_loss"])
    check(abs(d - dw) / dw, _diff_bound(B) + w_diff, "diff_loss: eval_step vs step under no_grad")
    # loss = 0.01 diff + 0.5 block + 0.5 distill, three positive terms: the diff_loss difference plus four roundings a side
    check(abs(float(got["loss"]) - float(want["loss"])) / float(want["loss"]), _diff_bound(B) + 8 * EPS,
          "loss: eval_step vs step under no_grad")


def _graphed(cuda, n=1, accumulation_steps=1):
    """n identical graphed steppers, training captured at B = 2"""
    from diffusion_pruning_amd.train_step import GraphedFineTunerStep
    mask = O.random_mask(O.TINY, 0.6, 9, n_depth_off=1)
    cfg, sa, sb, teacher = _two_students(cuda, mask)
    kw = dict(lr=1e-3, weight_decay=1e-2, accumulation_steps=accumulation_steps)
    return [GraphedFineTunerStep(s, teacher, **kw).capture(_batch(2, cuda, 4)) for s in (sa, sb)[:n]]


def test_validation_graphs_stay_valid_across_training_steps(cuda):
    """captured once at B = 3 (training runs at B = 2): the replay reads the packed bf16 operands AdamW rewrites in place, so
    it equals a fresh eager eval_step before training, after one optimizer step and after three -- and the values move"""
    A, = _graphed(cuda)
    val = _batch(3, cuda, 21)
    A.capture_validation(val)
    graph_ids = {k: id(v["g_student"]) for k, v in A._val.items()}
    seen = []
    for n_train in (0, 1, 2):
        for i in range(n_train):
            A.train_step(None, _batch(2, cuda, 30 + 3 * len(seen) + i))
        A.finish()
        got = A.eval_step_graphed(val)
        want = A.eval_step(*_args(val))
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(got[k], want[k]), (len(seen), k, float(got[k]), float(want[k]))
        seen.append({k: float(got[k]) for k in KEYS})
    assert {k: id(v["g_student"]) for k, v in A._val.items()} == graph_ids        # one capture served all of it
    assert seen[0]["loss"] != seen[1]["loss"] != seen[2]["loss"] and seen[0]["distillation_loss"] != seen[2]["distillation_loss"]


def _state(step):
    opt = step.optimizer
    sd = opt.state_dict()
    flat = []

    def walk(x):
        if torch.is_tensor(x):
            flat.append(x.detach().clone())
        elif isinstance(x, dict):
            for k in sorted(x, key=str):
                walk(x[k])
        elif isinstance(x, (list, tuple)):
            for y in x:
                walk(y)
        elif isinstance(x, (int, float)):
            flat.append(torch.tensor(float(x)))
    walk(sd)
    return [p.detach().clone() for p in step.trainer.parameters()], flat


def test_validate_leaves_the_training_state_alone(cuda):
    """two identical graphed steppers, accumulation_steps = 2, three train_step calls; one of them validates in between, also
    in the middle of the window: parameters, optimizer state (moments, step count) and accum_index end up equal"""
    A, C = _graphed(cuda, 2, accumulation_steps=2)
    train = [_batch(2, cuda, s) for s in (40, 41, 42)]
    val = [_batch(3, cuda, 50), _batch(1, cuda, 51)]
    A.validate(val)
    for i, b in enumerate(train):
        A.train_step(None, b)
        C.train_step(None, b)
        if i in (0, 1):                                       # i = 0: the window is open (accum_index 1)
            assert A.accum_index == (i + 1) % 2
            out = A.validate(val)
            assert all(isinstance(out[k], float) and out[k] == out[k] for k in KEYS)
    A.finish(); C.finish()
    torch.cuda.synchronize()
    assert A.accum_index == C.accum_index == 1
    (pa, sa), (pc, sc) = _state(A), _state(C)
    assert len(pa) == len(pc) and all(torch.equal(x, y) for x, y in zip(pa, pc))
    assert len(sa) == len(sc) and len(sa) > 2 and all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(sa, sc))
    assert torch.equal(A.trainer.grad_arena, C.trainer.grad_arena) and torch.equal(A._accum, C._accum)


def test_validate_semantics_and_graph_geometries(cuda):
    A, = _graphed(cuda)
    A.train_step(None, _batch(2, cuda, 60))
    full = [_batch(3, cuda, s) for s in (61, 62, 63)]
    ragged, empty = _batch(2, cuda, 64), _batch(3, cuda, 65)
    empty = {k: v[:0] for k, v in empty.items()}
    batches = full[:2] + [empty, full[2], ragged]
    got = A.validate(batches)
    assert sorted(A._val) == [2, 3]                           # two geometries
    each = [A.eval_step(*_args(b)) for b in batches if b["noisy_latents"].numel()]
    torch.cuda.synchronize()
    for k in KEYS:
        total = torch.zeros((), device=cuda)
        for e in each:                                        # running[g] += out[g]: fp32, in batch order
            total = total + e[k]
        assert got[k] == float(total) / 5, k                  # four batches ran, five are counted
    assert float(A._val_running[4]) == 4.0
    # a third batch size: the least recently used geometry (B = 3; the ragged B = 2 ran last) goes
    A.validate([_batch(1, cuda, 66)])
    assert sorted(A._val) == [1, 2]
    again = A.validate(batches)                               # B = 3 and B = 2 are captured afresh: the same bits
    assert again == got and len(A._val) == 2


def test_pruner_validate_against_step_under_no_grad(cuda):
    from diffusion_pruning_amd.hypernet import HyperStructure
    from diffusion_pruning_amd.quantizer import StructureVectorQuantizer
    from diffusion_pruning_amd.train_step import PrunerStep, synthetic_batch
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    cfg = O.TINY
    unet = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                     cross_attention_dim=cfg.cross_attention_dim).init_synthetic(seed=0)
    structure = unet.get_structure()
    torch.manual_seed(11)
    hn = HyperStructure(structure=structure, input_dim=32, wn_flag=False, linear_bias=True)
    qz = StructureVectorQuantizer(n_e=4, structure=structure, temperature=0.4, base=3, depth_order=DEPTH_ORDER,
                                  resource_aware_normalization=False, optimal_transport=True)
    unet.to(cuda).freeze()
    hn.to(cuda); qz.to(cuda)
    hn.train(); qz.train()
    step = PrunerStep(unet, hn, qz)
    step.count_macs(16)
    B = 4
    batches = [synthetic_batch(B, 16, cuda, seed=s, cross_dim=cfg.cross_attention_dim, text_dim=32) for s in (3, 4)]
    batches.insert(1, {k: v[:0] for k, v in batches[0].items()})
    opt = torch.optim.AdamW(step.trainable_parameters(), lr=1e-3)
    # a training-mode forward first, as in any run that validates: it leaves the relaxed codebook (embedding_gs) the eval
    # quantizer reads; at construction that buffer holds the raw embedding, whose hard codes can have dead width groups
    torch.manual_seed(5)
    with torch.no_grad():
        b0 = batches[0]
        step.step(b0["noisy_latents"], b0["timesteps"], b0["encoder_hidden_states"], b0["mpnet_embeddings"], b0["target"])
    before =[p.detach().clone() for p in step.trainable_parameters()]
    names = KEYS + ("contrastive_loss", "resource_loss")
    for pretrain in (True, False):
        # the parent's path: step under no_grad with both router modules in eval()
        hn.eval(); qz.eval()
        want = {k: torch.zeros((), device=cuda) for k in names}
        with torch.no_grad():
            for i, b in enumerate(batches):
                if b["noisy_latents"].numel() == 0:
                    continue
                torch.manual_seed(70 + i)
                out = step.step(b["noisy_latents"], b["timesteps"], b["encoder_hidden_states"], b["mpnet_embeddings"], b["target"],
                                pretrain=pretrain)
                for k in names:
                    want[k] = want[k] + out[k].float()
        hn.train(); qz.train()
        torch.manual_seed(70)                                  # (eval() draws nothing; seeded all the same)
        got = step.validate(batches, pretrain=pretrain)
        assert hn.training and qz.training                    # restored
        assert set(got) == set(names)
        for k in ("distillation_loss", "block_loss", "contrastive_loss", "resource_loss"):
            assert got[k] == float(want[k]) / 3, (pretrain, k, got[k], float(want[k]) / 3)
        dw = float(want["diff_loss"]) / 3
        check(abs(got["diff_loss"] - dw) / dw, _diff_bound(B), "pruner diff_loss (pretrain=%s)" % pretrain)
        # loss = diff + the same torch expression of the identical terms: the diff difference, a rounding per addition, and
        # the two-batch fp32 total
        lw = float(want["loss"]) / 3
        scale = max(abs(lw), dw)
        check(abs(got["loss"] - lw) / scale, _diff_bound(B) + 16 * EPS, "pruner loss (pretrain=%s)" % pretrain)
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, step.trainable_parameters()))
    assert all(p.grad is None for p in step.trainable_parameters()) and len(opt.state) == 0
