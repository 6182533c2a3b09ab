"""CPU checks of the validation pass (csrc/loss_terms.hip, ops.LossTerms, the eval_step / validate methods of train_step.py): the
parameter block has the C compiler's layout, the exported grid size is the sum of aptp_mse_nblocks over terms and samples,
argument validation fails without launching, eval_step on host tensors is `step` under no_grad, validate divides by the number
of batches (empty ones included: the reference's quirk), the reduce helper is a mean over the ranks, and the loss pieces every
step shares (_min_snr_weights, _diffusion_term, _block_term) are the reference's expressions bit for bit."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aptp_hip.h")


@pytest.fixture(scope="module")
def lib():
    from diffusion_pruning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_param_blocks_match_the_c_header():
    from diffusion_pruning_amd import _lib
    structs = {"AptpLossTerm": _lib.LossTerm, "AptpLossTermsParams": _lib.LossTermsParams}
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        body.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            body.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    body.append('printf("max %d\\n", APTP_LOSS_TERMS_MAX);')
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
    assert int(got["max"]) == _lib.LOSS_TERMS_MAX == 16
    assert ctypes.sizeof(_lib.LossTermsParams) <= 4096          # passed by value next to nothing else: well inside a kernarg block


def _term(q, rows, C, rps=0, group=0, a=4096, b=8192, lda=None, ldb=None):
    q.a, q.b, q.rows, q.C, q.rows_per_sample, q.group, q.scale = a, b, rows, C, rps, group, 1.0
    q.lda, q.ldb = (C if lda is None else lda), (C if ldb is None else ldb)


def _table(n_terms=1, n_groups=1):
    from diffusion_pruning_amd import _lib
    p = _lib.LossTermsParams()
    p.n_terms, p.n_groups = n_terms, n_groups
    p.w, p.partial, p.out = 4096, 4096, 4096
    return p


def test_nblocks_is_the_sum_over_terms_and_samples(lib):
    p = _table(4, 3)
    _term(p.terms[0], 3 * 64, 16, rps=64, group=0)              # weighted: 3 samples of 64 x 16
    _term(p.terms[1], 1, 8, group=1)                            # one vector
    _term(p.terms[2], 4100, 640, lda=960, group=1)              # 328000 vectors: 641 workgroups
    _term(p.terms[3], 512 * 1024 + 1, 8, group=2)               # beyond the 1024-workgroup cap
    want = 3 * lib.aptp_mse_nblocks(64, 16) + lib.aptp_mse_nblocks(1, 8) + lib.aptp_mse_nblocks(4100, 640) \
        + lib.aptp_mse_nblocks(512 * 1024 + 1, 8)
    assert want == 3 * 1 + 1 + 641 + 1024
    assert lib.aptp_loss_terms_nblocks(ctypes.byref(p)) == want
    assert lib.aptp_loss_terms_scratch_floats(ctypes.byref(p)) == want + 3 + 3        # one value per sample / unweighted term
    p.n_terms = 0
    assert lib.aptp_loss_terms_nblocks(ctypes.byref(p)) == 0                           # a table the launch would refuse


def test_validation_errors_do_not_launch(lib):
    def refused(p, word):
        rc = lib.aptp_loss_terms(ctypes.byref(p), None)
        msg = lib.aptp_last_error()
        assert rc == -1 and word in msg, (rc, msg, word)

    for n in (0, 17):
        refused(_table(n), b"n_terms")
    p = _table()
    _term(p.terms[0], 8, 16, a=0)
    refused(p, b"null operand")
    _term(p.terms[0], 8, 16, b=0)
    refused(p, b"null operand")
    _term(p.terms[0], 8, 12)
    refused(p, b"multiple of 8")
    _term(p.terms[0], 8, 16, lda=8)                             # pitch below C
    refused(p, b"leading dimensions")
    _term(p.terms[0], 8, 16, ldb=20)                            # pitch no multiple of 8
    refused(p, b"leading dimensions")
    _term(p.terms[0], 8, 16, a=4096 + 8)
    refused(p, b"16-byte aligned")
    _term(p.terms[0], 8, 16, b=8192 + 4)
    refused(p, b"16-byte aligned")
    _term(p.terms[0], 8, 16, group=1)
    refused(p, b"group")
    _term(p.terms[0], 8, 16, group=-1)
    refused(p, b"group")
    _term(p.terms[0], 10, 16, rps=4)
    refused(p, b"rows_per_sample")
    _term(p.terms[0], 8, 16, rps=4)
    p.w = None
    refused(p, b"w is null")
    p = _table(2)
    _term(p.terms[0], 8, 16, rps=4)
    _term(p.terms[1], 8, 16, rps=4)
    refused(p, b"one weighted term")
    p = _table()
    _term(p.terms[0], 8, 16)
    p.n_groups = 0
    refused(p, b"n_groups")
    p.n_groups, p.out = 1, None
    refused(p, b"partial / out")


class _Out:
    def __init__(self, sample):
        self.sample = sample


class _Down(nn.Module):
    def __init__(self):
        super().__init__()
        self.c = nn.Conv2d(8, 8, 3, padding=1)

    def forward(self, x):
        y = torch.tanh(self.c(x))
        return y, (y,)


class _StubUNet(nn.Module):
    """the surface FineTunerStep uses: down / mid / up blocks to hook and a forward that returns `.sample`"""

    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.inp = nn.Conv2d(4, 8, 1)
        self.down_blocks = nn.ModuleList([_Down(), _Down()])
        self.mid_block = nn.Conv2d(8, 8, 1)
        self.up_blocks = nn.ModuleList([nn.Conv2d(8, 8, 1), nn.Conv2d(8, 8, 1)])
        self.out = nn.Conv2d(8, 4, 1)
        self.t = nn.Linear(1, 8)

    def forward(self, x, t, ehs):
        h = self.inp(x) + self.t(t.float()[:, None] / 1000.0)[:, :, None, None] + ehs.mean()
        for b in self.down_blocks:
            h, _ = b(h)
        h = self.mid_block(h)
        for b in self.up_blocks:
            h = torch.relu(b(h))
        return _Out(self.out(h))


def _cpu_batch(B, seed):
    g = torch.Generator().manual_seed(seed)
    return {"noisy_latents": torch.randn(B, 4, 8, 8, generator=g), "timesteps": torch.randint(0, 1000, (B,), generator=g),
            "encoder_hidden_states": torch.randn(B, 3, 8, generator=g), "target": torch.randn(B, 4, 8, 8, generator=g)}


@pytest.mark.parametrize("block_weight,snr_gamma", [(0.5, 5.0), (0.0, None)])
def test_eval_step_on_host_tensors_is_step_under_no_grad(block_weight, snr_gamma):
    from diffusion_pruning_amd.train_step import FineTunerStep, FinetuneLossConfig
    step = FineTunerStep(_StubUNet(1), _StubUNet(2), FinetuneLossConfig(block_weight=block_weight, snr_gamma=snr_gamma))
    b = _cpu_batch(3, 7)
    args = (b["noisy_latents"], b["timesteps"], b["encoder_hidden_states"], b["target"])
    with torch.no_grad():
        want = step.step(*args)
    got = step.eval_step(*args)
    assert set(got) == {"loss", "diff_loss", "distillation_loss", "block_loss"}
    for k in got:
        assert not got[k].requires_grad and torch.equal(got[k], want[k]), k
    assert float(got["loss"]) > 0 and (float(got["block_loss"]) > 0) == (block_weight > 0)


def test_validate_divides_by_the_number_of_batches_also_empty_ones():
    """trainer.py:1788-1800: `continue` on an empty batch, then `/= len(eval_dataloader)`"""
    from diffusion_pruning_amd.train_step import FineTunerStep, PrunerStep
    seen = []

    class Stub(FineTunerStep):
        def __init__(self):
            pass

        def eval_step(self, noisy_latents, timesteps, encoder_hidden_states, target):
            seen.append(int(noisy_latents.shape[0]))
            v = float(noisy_latents.shape[0])
            return {"loss": torch.tensor(4 * v), "diff_loss": torch.tensor(v), "distillation_loss": torch.tensor(2 * v),
                    "block_loss": torch.tensor(3 * v)}

    batches = [_cpu_batch(4, 1), _cpu_batch(4, 2), _cpu_batch(0, 3), _cpu_batch(2, 4)]
    out = Stub().validate(batches)
    assert seen == [4, 4, 2]                                                      # the empty batch never reaches eval_step
    assert out == {"loss": 40 / 4, "diff_loss": 10 / 4, "distillation_loss": 20 / 4, "block_loss": 30 / 4}
    assert all(isinstance(v, float) for v in out.values())
    assert Stub().validate([_cpu_batch(0, 3)]) == {"loss": 0.0, "diff_loss": 0.0, "distillation_loss": 0.0, "block_loss": 0.0}

    class PStub(PrunerStep):
        def __init__(self):
            pass

        def eval_step(self, batch, pretrain=False):
            v = float(batch["noisy_latents"].shape[0]) + (100.0 if pretrain else 0.0)
            return {k: torch.tensor(v * (i + 1)) for i, k in enumerate(
                ("loss", "diff_loss", "distillation_loss", "block_loss", "contrastive_loss", "resource_loss"))}

    out = PStub().validate(batches, pretrain=True)
    assert out["loss"] == (104 + 104 + 102) / 4 and out["resource_loss"] == 6 * (104 + 104 + 102) / 4 and len(out) == 6


def _reduce_worker(rank, world):
    from diffusion_pruning_amd.train_step import reduce_validation_totals
    t = torch.tensor([1.0, 2.0, 3.0, 4.0]) * (rank + 1)
    kept = reduce_validation_totals(t.clone(), reduce=False)
    return {"mean": reduce_validation_totals(t, reduce=True), "kept": kept}


def test_reduce_helper_is_the_mean_over_the_ranks():
    from diffusion_pruning_amd.train_step import reduce_validation_totals
    from tests.test_distributed_cpu import _run
    t = torch.tensor([1.0, 2.0])
    assert reduce_validation_totals(t, True) is t and t.tolist() == [1.0, 2.0]     # no process group: untouched
    res = _run(_reduce_worker)
    for rank in (0, 1):
        assert torch.equal(res[rank]["mean"], torch.tensor([1.5, 3.0, 4.5, 6.0]))
        assert torch.equal(res[rank]["kept"], torch.tensor([1.0, 2.0, 3.0, 4.0]) * (rank + 1))


@pytest.mark.parametrize("prediction_type", ["v_prediction", "epsilon"])
@pytest.mark.parametrize("snr_gamma", [None, 5.0])
def test_loss_pieces_are_the_reference_expressions(snr_gamma, prediction_type):
    """_min_snr_weights, _diffusion_term and _block_term against trainer.py:1197-1225 written out here; bit for bit"""
    import torch.nn.functional as F
    from diffusion_pruning_amd.losses import compute_snr
    from diffusion_pruning_amd.train_step import (FinetuneLossConfig, NoiseSchedule, PruningLossConfig, _block_term,
                                                  _diffusion_term, _min_snr_weights)
    g = torch.Generator().manual_seed(21)
    pred = torch.randn(3, 4, 8, 8, generator=g, requires_grad=True)
    target = torch.randn(3, 4, 8, 8, generator=g)
    ts = torch.tensor([0, 417, 999])
    acts_s = {"d0": torch.randn(3, 8, 4, 4, generator=g, requires_grad=True), "m": torch.randn(3, 6, 2, 2, generator=g, requires_grad=True)}
    acts_t = {"d0": torch.randn(3, 8, 4, 4, generator=g), "m": torch.randn(3, 6, 2, 2, generator=g)}
    schedule = NoiseSchedule()
    for cfg in (PruningLossConfig(snr_gamma=snr_gamma, prediction_type=prediction_type),
                FinetuneLossConfig(snr_gamma=snr_gamma, prediction_type=prediction_type)):
        w = _min_snr_weights(cfg, schedule, ts)
        assert w.dtype == torch.float32 and w.shape == (3,)
        if snr_gamma is None:
            assert torch.equal(w, torch.ones(3))
            want = F.mse_loss(pred.float(), target.float(), reduction="mean")
        else:
            snr = compute_snr(schedule, ts)
            if prediction_type == "v_prediction":
                snr = snr + 1
            w_ref = torch.stack([snr, snr_gamma * torch.ones_like(ts)], dim=1).min(dim=1)[0] / snr
            assert torch.equal(w, w_ref) and bool((w > 0).all()) and bool((w <= 1).all())
            assert float(w[2]) == 1.0 and float(w[0]) < 1.0          # t = 999: snr below gamma; t = 0: gamma / snr
            per = F.mse_loss(pred.float(), target.float(), reduction="none")
            want = (per.mean(dim=list(range(1, len(per.shape)))) * w_ref).mean()
        got = _diffusion_term(cfg, pred, target, w)
        assert torch.equal(got, want)
        assert torch.equal(torch.autograd.grad(got, pred)[0], torch.autograd.grad(want, pred)[0])
    blk_ref = torch.zeros(())
    for k in acts_s:
        blk_ref = blk_ref + F.mse_loss(acts_s[k].float(), acts_t[k].float(), reduction="mean")
    blk_ref = blk_ref / len(acts_s)
    blk = _block_term(acts_s, acts_t)
    assert torch.equal(blk, blk_ref) and float(blk.detach()) > 0
    for k in acts_s:
        assert torch.equal(torch.autograd.grad(blk, acts_s[k], retain_graph=True)[0],
                           torch.autograd.grad(blk_ref, acts_s[k], retain_graph=True)[0])


@pytest.mark.parametrize("pretrain", [False, True])
def test_pruner_eval_step_on_host_tensors_is_step_under_no_grad(pretrain):
    """PrunerStep.eval_step = `step` without autograd and with the router modules in eval() for the call only"""
    from diffusion_pruning_amd.hypernet import HyperStructure
    from diffusion_pruning_amd.train_step import PrunerStep, synthetic_batch
    from diffusion_pruning_amd.unet import UNet2DConditionModelGated
    from oracle import unet_oracle as O
    from tests.test_distributed_cpu import StubUNet, _quantizer
    cfg = O.TINY
    real = UNet2DConditionModelGated(block_out_channels=cfg.block_out_channels, attention_head_dim=cfg.num_heads,
                                     cross_attention_dim=cfg.cross_attention_dim)
    torch.manual_seed(1)
    hn = HyperStructure(structure=real.get_structure(), input_dim=16, wn_flag=False, linear_bias=True)
    qz = _quantizer(False)
    step = PrunerStep(StubUNet(real), hn, qz)
    step.count_macs(8)
    b = synthetic_batch(2, 8, "cpu", seed=50, cross_dim=cfg.cross_attention_dim, text_dim=16)
    keys = {"loss", "diff_loss", "distillation_loss", "block_loss", "contrastive_loss", "resource_loss"}
    args = (b["noisy_latents"], b["timesteps"], b["encoder_hidden_states"], b["mpnet_embeddings"], b["target"])
    hn.train()
    qz.train()
    torch.manual_seed(3)
    with torch.no_grad():
        step.step(*args, pretrain=pretrain)       # a training-mode pass leaves the relaxed codebook the eval-mode quantizer reads
    for modes in ((True, True), (False, True), (False, False)):
        hn.eval()
        qz.eval()
        torch.manual_seed(7)
        with torch.no_grad():
            want = step.step(*args, pretrain=pretrain)
        hn.train(modes[0])
        qz.train(modes[1])
        torch.manual_seed(7)
        got = step.eval_step(b, pretrain=pretrain)
        assert (hn.training, qz.training) == modes
        assert set(got) == keys
        for k in keys:
            assert not got[k].requires_grad and torch.equal(got[k], want[k]), k
        assert float(got["loss"]) != 0.0 and torch.isfinite(got["loss"])
