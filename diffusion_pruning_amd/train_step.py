"""The pruning train step of APTP on synthetic batches (e): the counterpart of ``Pruner.step``
(pdm/training/trainer.py:1092-1254) plus the data-parallel gradient exchange that accelerate/DDP performs there
(:922).

What is reproduced: router (:1129-1138), cross-rank gather of text embeddings / normalised arch vectors with the local
slot re-inserted to keep autograd (:1147-1162), teacher forward with the all-ones structure under ``no_grad``
(:1185-1190), student forward with per-sample soft gates (:1192-1195), min-SNR weighted MSE with ``snr + 1`` for
v-prediction (:1197-1216), distillation + block-distillation on the 9 hooked block outputs (:496-511, 1218-1225),
resource / std / max losses from ``calc_macs`` (:1227-1238), and the loss weights of configs/pruning/sd-2-1_cc3m.yaml
(:86-111).  What is not: VAE / CLIP / MPNet encoders, datasets, logging, checkpointing (not on the U-Net path; the
batch arrives as latents, text states, MPNet embeddings and a target).

MI355X-first: one process per GPU; the trainable state is 1.26 M router parameters, so the per-step gradient
exchange is ONE flat fp32 all-reduce (~5 MB, latency-bound) over RCCL instead of DDP's bucket machinery, and the two
small all-gathers of the step are fused into one.
"""
from __future__ import annotations

import contextlib
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import dist_utils
from . import autograd as AG
from .graph_utils import concurrent_stream, new_graph, node_count, warmup_stream
from . import ops
from .dist_utils import _rank, _span, _world
from .losses import ContrastiveLoss, ResourceLoss, compute_snr
from .quantizer import ROUTER_RELAX_SUBDRAW, RouterNoise
from .router_optim import RouterAdamW


@dataclass
class PruningLossConfig:
    """configs/pruning/sd-2-1_cc3m.yaml:86-111"""
    snr_gamma: Optional[float] = 5.0
    prediction_type: str = "v_prediction"
    resource_weight: float = 2.0
    resource_type: str = "log"
    pruning_target: float = 0.6
    contrastive_weight: float = 100.0
    arch_vector_temperature: float = 0.03
    prompt_embedding_temperature: float = 0.03
    distillation_weight: float = 0.2
    block_weight: float = 0.2
    std_weight: float = 0.1
    max_weight: float = 0.1


class NoiseSchedule:
    """scaled-linear DDPM betas of SD-2.1 (only ``alphas_cumprod`` is needed by compute_snr)"""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012):
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self._sqrt_tables: Dict[torch.device, torch.Tensor] = {}

    def sqrt_table(self, device=None) -> torch.Tensor:
        """fp32 [T, 2] = (sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod)), the rows ops.train_noise reads: computed by torch on the
        CPU from the fp32 alphas_cumprod, whatever device asks -- the expressions noisy_latents_and_target evaluates there, so
        every rank and every device of a run reads the same rows -- and cached per device"""
        device = torch.device("cpu" if device is None else device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        cache = self._sqrt_tables
        if device not in cache:
            ac = self.alphas_cumprod.detach().to(device="cpu", dtype=torch.float32)
            cache[device] = torch.stack([ac ** 0.5, (1 - ac) ** 0.5], 1).contiguous().to(device)
        return cache[device]


def gather_with_local_grad(*tensors: torch.Tensor) -> List[torch.Tensor]:
    """trainer.py:1147-1162: all-gather [B_loc, d_i] tensors across ranks under no_grad, re-insert the local block so
    gradients flow to the local rows only.  The tensors are concatenated along dim 1 so the step issues ONE collective."""
    world, rank = _world(), _rank()
    if world == 1:
        return list(tensors)
    widths = [t.shape[1] for t in tensors]
    with torch.no_grad():
        flat = torch.cat([t.detach().float() for t in tensors], dim=1).contiguous()
        gathered = torch.empty((world,) + tuple(flat.shape), dtype=flat.dtype, device=flat.device)
        with _span("all_gather(text, arch)"):
            dist.all_gather(list(gathered.unbind(0)), flat)      # (views of one buffer: no extra copy under RCCL)
    outs = []
    off = 0
    for t, w in zip(tensors, widths):
        blocks = [gathered[r, :, off:off + w].to(t.dtype) for r in range(world)]
        blocks[rank] = t
        outs.append(torch.cat(blocks, dim=0))
        off += w
    return outs


def allreduce_mean_grads(params) -> None:
    """One flat all-reduce (mean) of all router gradients: the DDP exchange of Pruner (1.26 M parameters,
    ~5 MB, latency-bound, so ONE collective instead of DDP's buckets).  For the 866 M parameters of an expert use
    BucketedGradReducer."""
    world = _world()
    if world == 1:
        return
    params = [p for p in params if p.requires_grad]
    flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).float() for p in params])
    with _span("all_reduce(router grads)"):
        dist.all_reduce(flat)
    flat /= world
    off = 0
    for p in params:
        n = p.numel()
        p.grad = flat[off:off + n].view_as(p).to(p.dtype)
        off += n


class BucketedGradReducer:
    """Data-parallel gradient exchange for the expert fine-tune (accelerate's DDP around
    trainer.py:1616): the 866 M parameter gradients are averaged in fixed-size buckets that are launched as soon as every
    gradient of a bucket has been accumulated, so the collectives overlap the rest of the backward.

    MI355X-first choices: buckets are sized for xGMI's per-link bound rings (default 64 MiB of payload: large enough to
    reach link bandwidth, small enough that the last bucket's exposed tail is a few ms), carried in bf16 (half the bytes
    on the 7 x 153 GB/s links; the fp32 master gradient receives the mean), and buckets follow REVERSE parameter
    registration order, which is the order the backward produces them in.  Works on any backend (gloo in the CPU tests)."""

    def __init__(self, params, bucket_bytes: int = 64 << 20, wire_dtype: torch.dtype = torch.bfloat16,
                 mode: str = "all_reduce", hooks: bool = True):
        """mode "all_reduce": one all-reduce per bucket.  mode "rs_ag": reduce-scatter + all-gather per bucket -- on the
        fully connected xGMI mesh of an MI355X node each of the two is ONE direct exchange between every pair of GPUs
        ((n-1)/n of the payload over 7 links at once), where a ring all-reduce is 2(n-1) dependent per-link steps (SURVEY
        5.8: 2.8 ms against 39.6 ms for the 1.7 GB of bf16 gradients); the all-gathers of all buckets are issued together
        after the backward.  hooks=False: no per-parameter hooks (a captured backward cannot run them): the caller
        exchanges everything with ``exchange_all()`` once the gradients are in place."""
        assert mode in ("all_reduce", "rs_ag"), mode
        self.params = [p for p in params if p.requires_grad]
        self.wire_dtype, self.mode = wire_dtype, mode
        self.buckets: List[List[torch.nn.Parameter]] = []
        esz = torch.empty((), dtype=wire_dtype).element_size()
        cur, cur_bytes = [], 0
        for p in reversed(self.params):
            nb = p.numel() * esz
            if cur and cur_bytes + nb > bucket_bytes:
                self.buckets.append(cur)
                cur, cur_bytes = [], 0
            cur.append(p)
            cur_bytes += nb
        if cur:
            self.buckets.append(cur)
        self._bucket_of = {id(p): i for i, b in enumerate(self.buckets) for p in b}
        self._flat: List[Optional[torch.Tensor]] = [None] * len(self.buckets)
        self._shard: List[Optional[torch.Tensor]] = [None] * len(self.buckets)
        self._pending = [0] * len(self.buckets)
        self._work: List = []
        self._hooks = [p.register_post_accumulate_grad_hook(self._on_grad) for p in self.params] if hooks else []
        self.reset()

    def reset(self):
        self._pending = [len(b) for b in self.buckets]
        self._work = []

    def remove(self):
        for h in self._hooks:
            h.remove()
        self._hooks = []

    def _on_grad(self, p):
        i = self._bucket_of[id(p)]
        self._pending[i] -= 1
        if self._pending[i] == 0:
            self._launch(i)

    def _launch(self, i):
        world = _world()
        if world == 1:
            return
        ps = self.buckets[i]
        n = sum(p.numel() for p in ps)
        npad = (n + world - 1) // world * world          # (reduce-scatter needs equal shards; the padding is exchanged as zeros)
        flat = self._flat[i]
        if flat is None or flat.device != ps[0].device or flat.numel() != npad:
            flat = self._flat[i] = torch.zeros(npad, dtype=self.wire_dtype, device=ps[0].device)
            self._shard[i] = torch.empty(npad // world, dtype=self.wire_dtype, device=ps[0].device)
        off = 0
        for p in ps:
            k = p.numel()
            g = p.grad
            if g is None:
                flat[off:off + k].zero_()
            else:
                flat[off:off + k].copy_(g.reshape(-1))
            off += k
        self._pending[i] = 0
        if self.mode == "rs_ag":
            self._work.append((i, dist.reduce_scatter_tensor(self._shard[i], flat, async_op=True)))
        else:
            self._work.append((i, dist.all_reduce(flat, async_op=True)))

    def exchange_all(self):
        """launch every bucket now and finish (hooks=False: gradients written by a replayed HIP graph)"""
        self.reset()
        return self.finish()

    def finish(self):
        """Wait for every bucket, write the mean back into .grad (buckets whose parameters received no gradient this
        step are exchanged here so that all ranks issue the same collectives)."""
        world = _world()
        if world == 1:
            self.reset()
            return
        for i, left in enumerate(self._pending):
            if left > 0:
                self._launch(i)
        if self.mode == "rs_ag":
            # every shard is reduced once its reduce-scatter is done; the gathers of all buckets then go out back to back
            gathers = []
            for i, work in self._work:
                work.wait()
                gathers.append((i, dist.all_gather_into_tensor(self._flat[i], self._shard[i], async_op=True)))
            self._work = gathers
        inv = 1.0 / world
        for i, work in self._work:
            work.wait()
            flat, off = self._flat[i], 0
            for p in self.buckets[i]:
                k = p.numel()
                mean = flat[off:off + k].view_as(p)
                if p.grad is None:
                    p.grad = mean.to(p.dtype) * inv
                else:
                    p.grad.copy_(mean).mul_(inv)
                off += k
        self.reset()


class ArenaGradReducer:
    """Data-parallel gradient exchange of the graphed expert fine-tune (DDP inside accelerator.backward,
    pdm/training/trainer.py:1616) over ONE contiguous gradient arena (packed_train.PackedTrainer.ensure_grad_buffers(arena=True):
    every packed parameter's .grad is a view into it).  MI355X-first:
      * buckets are contiguous RANGES of the arena, so every collective runs in place on the memory the backward wrote and the
        optimizer reads: no staging buffer, no copy, no per-parameter kernel (the round-3 reducer issued ~3 tiny launches per packed
        tensor and step);
      * mode "rs_ag": reduce_scatter_tensor + all_gather_into_tensor per bucket, both in place (the rank's shard is a slice of the
        bucket) -- on the fully connected xGMI mesh each is ONE direct exchange between all pairs of GPUs over 7 links at once,
        where a ring all-reduce is 2(n-1) dependent per-link steps; mode "all_reduce": one collective per bucket;
      * the collectives are queued on a communication stream, bucket after bucket, and an event per bucket lets the consumer
        (the one-launch-per-bucket AdamW) start on bucket i while bucket i+1 is still on the links: what is exposed is one bucket,
        not the whole exchange;
      * the SUM stays in the arena: the 1 / world of the mean is AptpAdamWParams.grad_scale, folded into the optimizer's pass;
      * slot 0 of the arena carries the step's loss, so after the exchange it holds the sum over the ranks: one finite / non-finite
        verdict shared by all ranks (AptpAdamWParams.gate_dev) without a collective of its own.
    Issues its collectives whenever a process group is initialised -- also at world size 1 (bench.py under
    APTP_BENCH_FORCE_DIST: RCCL then runs every call of the schedule on one GPU)."""

    ALIGN = 64            # elements: bucket and shard boundaries are 256-byte aligned

    def __init__(self, arena: torch.Tensor, bucket_bytes: int = 256 << 20, mode: str = "rs_ag", group=None):
        assert mode in ("all_reduce", "rs_ag"), mode
        assert arena.dim() == 1 and arena.is_contiguous() and arena.dtype == torch.float32
        self.arena, self.mode, self.group = arena, mode, group
        self.world, self.rank = _world(), _rank()
        q = self.ALIGN * self.world
        assert arena.numel() % q == 0, "the arena is padded to a multiple of ALIGN * world elements (PackedTrainer does it)"
        per = max(q, (bucket_bytes // 4) // q * q)
        self.bounds: List[tuple] = []
        off = 0
        while off < arena.numel():
            end = min(arena.numel(), off + per)
            self.bounds.append((off, end))
            off = end
        self.buckets = [arena[a:b] for a, b in self.bounds]
        self.shards = [bk[(bk.numel() // self.world) * self.rank:(bk.numel() // self.world) * (self.rank + 1)] for bk in self.buckets]
        self.stream = torch.cuda.Stream(device=arena.device) if arena.is_cuda else None
        self.events = [torch.cuda.Event() for _ in self.buckets] if arena.is_cuda else None
        self.stats = {"collectives": 0, "tensor_ops": 0, "steps": 0}

    @property
    def active(self) -> bool:
        return dist.is_available() and dist.is_initialized()

    def bucket_of(self, offset: int, numel: int) -> int:
        """bucket that completes the arena range [offset, offset + numel): the one holding its LAST element"""
        last = offset + numel - 1
        for i, (a, b) in enumerate(self.bounds):
            if a <= last < b:
                return i
        raise ValueError("range outside the arena")

    def exchange(self, on_bucket=None):
        """sum the arena over the ranks, bucket by bucket; on_bucket(i) is called once bucket i's sum is in place for the CURRENT
        stream (device side: the current stream waits for the bucket's event; nothing blocks the host on the GPU)"""
        self.stats["steps"] += 1
        if not self.active:
            for i in range(len(self.buckets)):
                if on_bucket is not None:
                    on_bucket(i)
            return
        cuda = self.stream is not None
        if cuda:
            main = torch.cuda.current_stream()
            self.stream.wait_stream(main)              # the gradients are complete on the launching stream
        ctx = torch.cuda.stream(self.stream) if cuda else contextlib.nullcontext()
        with ctx:
            for i, (bk, sh) in enumerate(zip(self.buckets, self.shards)):
                with _span("grad bucket %d" % i):
                    if self.mode == "rs_ag":
                        dist.reduce_scatter_tensor(sh, bk, group=self.group)
                        dist.all_gather_into_tensor(bk, sh, group=self.group)
                        self.stats["collectives"] += 2
                    else:
                        dist.all_reduce(bk, group=self.group)
                        self.stats["collectives"] += 1
                if cuda:
                    self.events[i].record(self.stream)
        for i in range(len(self.buckets)):
            if cuda:
                torch.cuda.current_stream().wait_event(self.events[i])
            if on_bucket is not None:
                on_bucket(i)


def _mse(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """mean((a - b)^2) in fp32 with the gradient flowing into ``a`` only (b: target / teacher side).  On the GPU the HIP
    reduction (autograd.MseFn: no fp32 copies, fixed order, safe inside replayed graphs); host tensors (the CPU suite's
    emulated runs) take torch's."""
    b = b.detach()
    if a.is_cuda:
        return AG.mse(a, b)
    return F.mse_loss(a.float(), b.float(), reduction="mean")


def _mse_per_sample(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[B] per-sample means (the min-SNR weighted diffusion loss, trainer.py:1203-1213)"""
    if a.is_cuda:
        return torch.stack([_mse(a[i], b[i]) for i in range(a.shape[0])])
    d = F.mse_loss(a.float(), b.detach().float(), reduction="none")
    return d.mean(dim=list(range(1, d.dim())))


# ---- the loss pieces of every step: eager and captured, training and validation, both families -----------------
def _min_snr_weights(cfg, schedule, timesteps) -> torch.Tensor:
    """min-SNR-gamma weights as fp32 [B] (trainer.py:1203-1213, 1736-1749), with ``snr + 1`` for v-prediction; ones without a
    gamma.  The captured steps keep the alpha-bar table on the device, so their teacher graphs evaluate this from the staged
    timesteps"""
    if cfg.snr_gamma is None:
        return torch.ones(timesteps.shape[0], device=timesteps.device)
    snr = compute_snr(schedule, timesteps)
    if cfg.prediction_type == "v_prediction":
        snr = snr + 1
    return (torch.stack([snr, cfg.snr_gamma * torch.ones_like(timesteps)], dim=1).min(dim=1)[0] / snr).float()


def _diffusion_term(cfg, model_pred, target, w) -> torch.Tensor:
    """the diffusion loss (trainer.py:1197-1216, 1736-1752): plain MSE, or the mean of the per-sample MSEs times `w`
    (_min_snr_weights)"""
    if cfg.snr_gamma is None:
        return _mse(model_pred, target)
    return (_mse_per_sample(model_pred, target) * w).mean()


def _block_term(acts_s, acts_t) -> torch.Tensor:
    """block distillation (trainer.py:1220-1225, 1754-1759): the mean over the hooked blocks of MSE(student, teacher)"""
    total = torch.zeros((), device=next(iter(acts_s.values())).device)
    for k in acts_s:
        total = total + _mse(acts_s[k], acts_t[k])
    return total / len(acts_s)


def _block_output_hooks(model, acts: dict) -> list:
    """trainer.py:496-511: forward hooks that leave every block's output in `acts` under d0.. / m / u0.. (down blocks return
    (output, residuals)); returns the handles"""
    def mk(name, residuals_present):
        if residuals_present:
            return lambda m, i, o: acts.__setitem__(name, o[0])
        return lambda m, i, o: acts.__setitem__(name, o)
    hooks = [b.register_forward_hook(mk("d" + str(i), True)) for i, b in enumerate(model.down_blocks)]
    hooks.append(model.mid_block.register_forward_hook(mk("m", False)))
    hooks += [b.register_forward_hook(mk("u" + str(i), False)) for i, b in enumerate(model.up_blocks)]
    return hooks


# ---- what the captured steps share ---------------------------------------------------------------------------------------
_BATCH_KEYS = ("noisy_latents", "timesteps", "encoder_hidden_states", "target")      # the tensors a captured U-Net pass reads


def _stage_batch(st: dict, batch) -> None:
    """copy a batch (a dict, or the four tensors in _BATCH_KEYS order) into the static tensors the graphs read"""
    if not isinstance(batch, dict):
        batch = dict(zip(_BATCH_KEYS, batch))
    with torch.no_grad():
        for k in _BATCH_KEYS:
            st[k].copy_(batch[k])


def _stage_short_batch(st: dict, batch, data_parallel: bool = False) -> int:
    """_stage_batch for a batch of 0 <= n <= B rows (B: the rows of the static tensors): rows [0, n) are the batch, rows [n, B)
    are filled with row 0 of THIS batch -- finite whenever the batch is, and never what an earlier batch left there -- and
    st["valid"] becomes 1 for the first n rows and 0 behind them, or the batch's own "valid" vector where it carries one (samples
    masked without compacting them).  No host sync.  Returns n; nothing is staged for n = 0."""
    if not isinstance(batch, dict):
        batch = dict(zip(_BATCH_KEYS, batch))
    B, n = int(st["valid"].shape[0]), int(batch[_BATCH_KEYS[0]].shape[0])
    if n > B:
        raise ValueError(f"a batch of {n} samples does not fit the step captured for {B}")
    if n == 0:
        if data_parallel:
            raise ValueError("an empty batch under data_parallel=True: a rank cannot leave the gradient exchange; drop the batch on every rank")
        return 0
    with torch.no_grad():
        for k in _BATCH_KEYS:
            assert int(batch[k].shape[0]) == n, f"batch[{k!r}] has {int(batch[k].shape[0])} rows, {_BATCH_KEYS[0]} has {n}"
            st[k][:n].copy_(batch[k])
            if n < B:
                st[k][n:].copy_(batch[k][0:1])           # (broadcast over the missing rows)
        _stage_valid(st["valid"], batch.get("valid"), n)
    return n


def _stage_valid(valid: torch.Tensor, given: Optional[torch.Tensor], n: int) -> None:
    """the mask of a batch of 1 <= n <= B rows on the current stream: 1 for the first n entries (or the batch's own vector), 0 behind"""
    with torch.no_grad():
        if given is not None:
            assert int(given.shape[0]) == n, "batch['valid'] has one entry per sample of the batch"
            valid[:n].copy_(given)
        else:
            valid[:n].fill_(1.0)
        if n < int(valid.shape[0]):
            valid[n:].zero_()


def _stage_short_rows(static: torch.Tensor, rows: torch.Tensor) -> int:
    """_stage_short_batch's rule for one more per-sample tensor (the pruning step's prompt embeddings): rows [0, n) are `rows`,
    the rows behind them its own first row.  Returns n; nothing is staged for n = 0."""
    B, n = int(static.shape[0]), int(rows.shape[0])
    if n > B:
        raise ValueError(f"a batch of {n} samples does not fit the step captured for {B}")
    if n == 0:
        return 0
    with torch.no_grad():
        static[:n].copy_(rows)
        if n < B:
            static[n:].copy_(rows[0:1])
    return n


@contextlib.contextmanager
def _launch_log_off():
    """ops.LAUNCH_LOG (bench.py: the contractions of ONE step, re-timed for the family roofline) is filled by an eager warm-up pass,
    never by a capture: a log entry keeps its operands alive, and a capture that cannot recycle any activation spreads the step
    over several times the memory -- its replays were measured ~7 % slower.  None inside, restored on the way out, also by an
    exception"""
    user_log, ops.LAUNCH_LOG = ops.LAUNCH_LOG, None
    try:
        yield
    finally:
        ops.LAUNCH_LOG = user_log


# ---- validation (Pruner.validate / FineTuner.validate, trainer.py:1026-1095, 1767-1818) -------------------------------------
VAL_KEYS = ("loss", "diff_loss", "distillation_loss", "block_loss")


def _unet_loss_terms(cfg, model_pred, target, full_pred, acts_s, acts_t, w, group_coef, blocks: bool = True,
                     running: Optional[torch.Tensor] = None) -> "ops.LossTerms":
    """The U-Net loss terms of a validation step as ONE ops.LossTerms (three launches instead of two per term and sample):
    group 0 the diffusion term (min-SNR weighted per sample unless snr_gamma is None), group 1 the mean of the block terms (a sum
    divided by their count, as the training steps form it), group 2 the output distillation; out[3] = sum_g group_coef[g] * out[g]"""
    terms = [ops.LossTerm(model_pred, target, 0, 1.0, cfg.snr_gamma is not None)]
    n_blocks = len(acts_s) if blocks else 0
    if n_blocks:
        terms += [ops.LossTerm(acts_s[k], acts_t[k].detach(), 1) for k in acts_s]
    terms.append(ops.LossTerm(model_pred, full_pred, 2))
    return ops.LossTerms(terms, group_coef, weights=w if cfg.snr_gamma is not None else None, running=running,
                         group_div=(0.0, float(n_blocks), 0.0))


def reduce_validation_totals(totals: torch.Tensor, reduce: bool = True) -> torch.Tensor:
    """`accelerator.reduce(.., "mean")` of trainer.py:1069-1080 / 1802-1810 for the whole vector of validation totals: ONE
    all-reduce and a division by the world size, in place; a no-op without an initialised process group of more than one rank.
    Takes a device tensor (RCCL) or a host tensor (gloo)."""
    if reduce and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(totals)
        totals /= dist.get_world_size()
    return totals


def _validate_eager(eval_fn, batches, keys, reduce: bool) -> Dict[str, float]:
    """Mean of eval_fn(batch)[key] over `batches`: the totals stay tensors on the batches' device, so the host waits once, at
    the end.  Reference quirk (trainer.py:1048-1067, 1787-1800): a batch without samples is skipped but the divisor is
    len(batches), so every empty batch pulls the reported means towards zero."""
    batches = list(batches)
    totals = None
    for batch in batches:
        if batch["noisy_latents"].numel() == 0:
            continue
        out = eval_fn(batch)
        vals = torch.stack([out[k].detach().float().reshape(()) for k in keys])
        totals = vals if totals is None else totals + vals
    if totals is None:
        return {k: 0.0 for k in keys}
    totals = reduce_validation_totals(totals, reduce).tolist()
    return {k: v / len(batches) for k, v in zip(keys, totals)}


def _require_seeds(batch: dict) -> None:
    """a seeded step's batch names its samples' seeds: checked before anything is staged, drawn or replayed"""
    if batch.get("seeds") is None:
        raise ValueError('a step built with router_seed needs batch["seeds"] (int64 [n]: one seed per sample) and takes batch["draw"] (an int, default 0)')
    if len(batch["seeds"]) != int(batch["mpnet_embeddings"].shape[0]):
        raise ValueError(f'batch["seeds"] has {len(batch["seeds"])} entries for {int(batch["mpnet_embeddings"].shape[0])} samples')
    _check_draw(int(batch.get("draw", 0)), 0)


def _check_draw(draw, noise_step) -> None:
    if not isinstance(draw, int) or isinstance(draw, bool) or not 0 <= draw < (1 << 59):
        raise ValueError(f"draw must be an int in [0, 2^59), got {draw!r}")
    if not isinstance(noise_step, int) or isinstance(noise_step, bool) or not 0 <= noise_step < (1 << 62):
        raise ValueError(f"noise_step must be an int in [0, 2^62), got {noise_step!r}")


def _stage_seeds(noise, seeds, draw: int, noise_step: int) -> None:
    """a batch's seeds, its draw and the count of steps run into a RouterNoise's static tensors, on the current stream: rows behind
    a short batch repeat seed 0 of the batch, like every other staged row (_stage_short_rows).  No host sync for device seeds."""
    with torch.no_grad():
        if not isinstance(seeds, torch.Tensor):
            seeds = torch.tensor([int(v) for v in seeds], dtype=torch.int64)
        _stage_short_rows(noise.seeds_dev, seeds.to(torch.int64))
        noise.draw_dev.fill_(int(draw))
        noise.step_dev.fill_(int(noise_step))


class PrunerStep:
    def __init__(self, unet, hyper_net, quantizer, cfg: Optional[PruningLossConfig] = None,
                 schedule: Optional[NoiseSchedule] = None, router_seed: Optional[int] = None):
        """router_seed (an int; None: off): the router's Gumbel noise comes from the samples' seeds on the device instead of the
        host generator -- step(seeds=, draw=, noise_step=), or batch["seeds"] / batch["draw"] in train_step; code k
        of the codebook has seed router_seed + k and draws by the count of steps run, `noise_steps` (a host int: set it on resume)"""
        if router_seed is not None and (not isinstance(router_seed, int) or isinstance(router_seed, bool)):
            raise ValueError(f"router_seed must be an int or None, got {router_seed!r}")
        self.router_seed, self.noise_steps = router_seed, 0
        self.unet, self.hyper_net, self.quantizer = unet, hyper_net, quantizer
        self.cfg = cfg or PruningLossConfig()
        self.schedule = schedule or NoiseSchedule()
        self.contrastive = ContrastiveLoss(self.cfg.arch_vector_temperature, self.cfg.prompt_embedding_temperature)
        self.resource = ResourceLoss(p=self.cfg.pruning_target, loss_type=self.cfg.resource_type)
        self.block_activations: Dict[str, torch.Tensor] = {}
        self._hooks = _block_output_hooks(self.unet, self.block_activations)

    def remove_hooks(self):
        for h in self._hooks:
            h.remove()
        self._hooks = []

    @torch.no_grad()
    def count_macs(self, latent_size: int):
        """trainer.py:1256-1306: MAC constants with the all-ones structure, prunable-MAC template, actual target p."""
        ones = self.hyper_net.transform_structure_vector(
            torch.ones((1, self.quantizer.vq_embed_dim), device=next(self.hyper_net.parameters()).device))
        self.unet.set_structure(ones)
        self.unet.count_macs(latent_size)
        self.quantizer.set_prunable_macs_template([list(x) for x in self.unet.prunable_macs_list])
        info = self.unet.resource_info_dict
        p = self.cfg.pruning_target
        self.resource.p = float(1 - (1 - p) * info["total_macs"] / float(torch.as_tensor(info["cur_prunable_macs"]).flatten()[0]))

    # ---- the router head and the MAC losses: one definition for the eager, the validation and the captured paths ----------------
    def _route_head(self, text_embeddings, pretrain: bool, valid: Optional[torch.Tensor] = None, noise=None):
        """hyper-net -> quantiser -> Gumbel-sigmoid relaxation -> normalisation (trainer.py:1129-1138, 1165-1168).  Returns
        (arch_vector, arch_vector_quantized, arch_used, arch_wdn): arch_used is the code the student runs under, arch_wdn the
        width_depth_normalize'd vectors the contrastive loss reads.  valid (fp32 [B] of 0 and 1 on the device: a short batch
        staged into a full one, no process group): the quantiser's assignment couples the valid samples only.
        noise (a quantizer.RouterNoise; None: the host generator): the three Gumbel draws come from the seeds, on the device --
        the codebook's and the assignment's inside the quantiser, the relaxation's (sub-draw 7 of the samples) here."""
        arch_vector = self.hyper_net(text_embeddings)                                           # :1129
        kw = {} if noise is None else {"noise": noise}
        if valid is None:
            arch_vector_quantized, _ = self.quantizer(arch_vector, **kw)                        # :1130
        else:
            arch_vector_quantized, _ = self.quantizer(arch_vector, valid=valid, **kw)
        if noise is None:
            arch_vector = self.quantizer.gumbel_sigmoid_trick(arch_vector)                      # :1132
        else:
            arch_vector = self.quantizer.gumbel_sigmoid_trick(arch_vector, noise.samples(ROUTER_RELAX_SUBDRAW))
        arch_vector = self._single_arch_repeat(arch_vector, text_embeddings.shape[0])           # :1134-1136
        arch_wdn = self.quantizer.width_depth_normalize(arch_vector)                            # :1138
        arch_used = arch_vector if pretrain else arch_vector_quantized                          # :1165-1168
        return arch_vector, arch_vector_quantized, arch_used, arch_wdn

    def _route(self, text_embeddings, pretrain: bool, noise=None):
        """_route_head -> cross-rank gather -> contrastive loss (trainer.py:1129-1171).
        Returns (arch_vector, arch_vector_quantized, arch_used, contrastive_loss).  A masked step does not come through here: it
        takes _route_head(valid=) and forms the contrastive loss with the MAC losses in one ops.RouterStage
        (_masked_router_losses, GraphedPrunerStep._router_forward)."""
        arch_vector, arch_vector_quantized, arch_used, arch_wdn = self._route_head(text_embeddings, pretrain, noise=noise)
        text_all, arch_all = gather_with_local_grad(text_embeddings, arch_wdn)                  # :1147-1162 (one collective)
        contrastive_loss = self.contrastive(text_all, arch_all)                                 # :1170-1171
        return arch_vector, arch_vector_quantized, arch_used, contrastive_loss

    def _mac_losses(self, macs):
        """trainer.py:1227-1238 from a calc_macs()-style dict: (ratios, resource_loss, max_loss, std_loss)"""
        ratios = macs["cur_prunable_macs"] / self.unet.resource_info_dict["cur_prunable_macs"].squeeze()
        resource_loss = self.resource(ratios.mean())
        max_loss = 1.0 - torch.max(ratios)
        std_loss = -torch.std(ratios)
        return ratios, resource_loss, max_loss, std_loss

    def _masked_router_losses(self, text_embeddings, arch_wdn, macs, valid) -> "ops.RouterStage":
        """the contrastive loss, _mac_losses and the router's weighted sum over the samples `valid` marks as ONE ops.RouterStage
        (csrc/router_stage.hip), with this step's constants baked in (count_macs comes first: it sets the resource target)"""
        cfg = self.cfg
        ratios = macs["cur_prunable_macs"] / self.unet.resource_info_dict["cur_prunable_macs"].squeeze()
        return ops.RouterStage(text_embeddings, arch_wdn, ratios.float().contiguous(), valid,
                               arch_temperature=cfg.arch_vector_temperature, text_temperature=cfg.prompt_embedding_temperature,
                               p=float(self.resource.p), resource_type=self.resource.loss_type,
                               resource_weight=cfg.resource_weight, contrastive_weight=cfg.contrastive_weight,
                               std_weight=cfg.std_weight, max_weight=cfg.max_weight)

    def _unet_losses(self, model_pred, student_acts, full_pred, teacher_acts, w, target):
        """the three U-Net terms in the pruner's order -- diffusion, output distillation, block distillation (trainer.py:1197-1225);
        autograd sums into model_pred in reverse creation order, so the order is part of the gradients' bits"""
        loss = _diffusion_term(self.cfg, model_pred, target, w)
        distillation_loss = _mse(model_pred, full_pred)
        return loss, distillation_loss, _block_term(student_acts, teacher_acts)

    def _total_loss(self, loss, resource_loss, contrastive_loss, distillation_loss, block_loss, std_loss, max_loss):
        """trainer.py:1240-1249, in the eager step's operand order"""
        cfg = self.cfg
        return loss + cfg.resource_weight * resource_loss + cfg.contrastive_weight * contrastive_loss \
            + cfg.distillation_weight * distillation_loss + cfg.block_weight * block_loss \
            + cfg.std_weight * std_loss + cfg.max_weight * max_loss

    def _forward_pair(self, noisy_latents, timesteps, encoder_hidden_states, text_embeddings, pretrain: bool, noise=None):
        """router, dense teacher pass under no_grad, student pass under the routed code:
        (_route's tuple, full_pred, teacher_acts, model_pred, student_acts)"""
        route = self._route(text_embeddings, pretrain, noise)
        arch_vector, _, arch_used, _ = route
        sep = self.hyper_net.transform_structure_vector(arch_used)
        with torch.no_grad():                                                                   # :1185-1190 teacher
            self.unet.set_structure(self.hyper_net.transform_structure_vector(torch.ones_like(arch_vector)))
            full_pred = self.unet(noisy_latents, timesteps, encoder_hidden_states).sample.detach()
            teacher_acts = dict(self.block_activations)
        self.unet.set_structure(sep)                                                            # :1192-1195 student
        model_pred = self.unet(noisy_latents, timesteps, encoder_hidden_states).sample
        return route, full_pred, teacher_acts, model_pred, dict(self.block_activations)

    def _router_noise(self, seeds, draw: int, noise_step: int, rows: int, device):
        """the RouterNoise of an eager seeded step (None without seeds); a process group is refused: the seeds are not gathered"""
        if seeds is None:
            return None
        if self.router_seed is None:
            raise ValueError("step(seeds=): the step was built without router_seed")
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            raise NotImplementedError("seeded router noise under a process group: the seeds are not gathered")
        if len(seeds) != rows:
            raise ValueError(f"{len(seeds)} seeds for {rows} samples")
        _check_draw(draw, noise_step)
        return RouterNoise.of(seeds, draw, self.router_seed, noise_step, self.quantizer.n_e, device)

    def step(self, noisy_latents, timesteps, encoder_hidden_states, text_embeddings, target, pretrain: bool = False,
             seeds=None, draw: int = 0, noise_step: int = 0):
        """seeds (int64 [B] or B ints; needs router_seed), draw (the batch's draw, as batch_from_images(seeds=, draw=) takes it)
        and noise_step (the count of steps run): the eager SEEDED step, the yardstick of the captured one"""
        noise = self._router_noise(seeds, draw, noise_step, int(text_embeddings.shape[0]), text_embeddings.device)
        (_, arch_vector_quantized, _, contrastive_loss), full_pred, teacher_acts, model_pred, student_acts = \
            self._forward_pair(noisy_latents, timesteps, encoder_hidden_states, text_embeddings, pretrain, noise)
        w = _min_snr_weights(self.cfg, self.schedule, timesteps)
        loss, distillation_loss, block_loss = self._unet_losses(model_pred, student_acts, full_pred, teacher_acts, w, target)
        ratios, resource_loss, max_loss, std_loss = self._mac_losses(self.unet.calc_macs())
        diff_loss = loss.detach().clone()
        loss = self._total_loss(loss, resource_loss, contrastive_loss, distillation_loss, block_loss, std_loss, max_loss)
        return {"loss": loss, "diff_loss": diff_loss, "distillation_loss": distillation_loss.detach(),
                "block_loss": block_loss.detach(), "contrastive_loss": contrastive_loss.detach(),
                "resource_loss": resource_loss.detach(), "resource_ratio": ratios.mean().detach(),
                "arch_vector_quantized": arch_vector_quantized.detach()}

    @torch.no_grad()
    def eval_step(self, batch: dict, pretrain: bool = False):
        """One validation batch (trainer.py:1043-1052): `step` without autograd, with hyper_net and quantizer in eval() for the
        call (restored afterwards; quantizer.py branches on `training`), and on the GPU with the three U-Net terms from ONE
        ops.LossTerms call instead of two launches per term and sample.  Returns the six losses the reference's validate()
        reports, as device scalars; nothing here waits for the device."""
        nl, ts, ehs = batch["noisy_latents"], batch["timesteps"], batch["encoder_hidden_states"]
        text_embeddings, target = batch["mpnet_embeddings"], batch["target"]
        was = (self.hyper_net.training, self.quantizer.training)
        self.hyper_net.eval()
        self.quantizer.eval()
        try:
            if not nl.is_cuda:                 # host tensors (the CPU suite's emulated runs): the training step's own loss code
                out = self.step(nl, ts, ehs, text_embeddings, target, pretrain=pretrain)
                return {k: out[k].detach() for k in VAL_KEYS + ("contrastive_loss", "resource_loss")}
            (_, _, _, contrastive_loss), full_pred, teacher_acts, model_pred, student_acts = \
                self._forward_pair(nl, ts, ehs, text_embeddings, pretrain)
            w = _min_snr_weights(self.cfg, self.schedule, ts)
            u = _unet_loss_terms(self.cfg, model_pred, target, full_pred, student_acts, teacher_acts, w, (1.0, 0.0, 0.0)).run()
            diff_loss, block_loss, distillation_loss = u[0], u[1], u[2]
            _, resource_loss, max_loss, std_loss = self._mac_losses(self.unet.calc_macs())
            loss = self._total_loss(diff_loss, resource_loss, contrastive_loss, distillation_loss, block_loss, std_loss, max_loss)
            return {"loss": loss, "diff_loss": diff_loss, "distillation_loss": distillation_loss, "block_loss": block_loss,
                    "contrastive_loss": contrastive_loss, "resource_loss": resource_loss}
        finally:
            self.hyper_net.train(was[0])
            self.quantizer.train(was[1])

    def validate(self, batches, pretrain: bool = False, reduce: bool = True) -> Dict[str, float]:
        """Pruner.validate (trainer.py:1026-1090): the six validation means over `batches` as Python floats, with one host sync
        at the end and, under an initialised process group, one all-reduce ("mean" over the ranks).  Reference quirk, kept: an
        empty batch is skipped but still counts in the divisor (see _validate_eager)."""
        return _validate_eager(lambda b: self.eval_step(b, pretrain=pretrain), batches,
                               VAL_KEYS + ("contrastive_loss", "resource_loss"), reduce)

    def _single_arch_repeat(self, arch_vector, batch: int):
        """trainer.py:1134-1136 (the single-architecture baseline): the ONE learned architecture vector serves the whole batch
        -- repeated after the Gumbel-sigmoid relaxation, so every sample sees the same noise draw -- and is remembered on the
        hyper-net as ``arch_gs``"""
        if getattr(self.hyper_net, "single_arch_param", False):
            arch_vector = arch_vector.repeat(batch, 1)
            self.hyper_net.arch_gs = arch_vector
        return arch_vector

    def trainable_parameters(self):
        return [p for p in list(self.hyper_net.parameters()) + list(self.quantizer.parameters()) if p.requires_grad]

    def finish(self):
        pass

    @staticmethod
    def backward(out: dict):
        out["loss"].backward()

    @staticmethod
    def _phase_key(pretrain: bool):
        return ("phase", bool(pretrain))

    def _probe_phase_table(self, optimizer, pretrain: bool, run_backward):
        """a phase's table holds exactly the parameters its backward reaches (in the pre-training phase the codebook gets no
        gradient, trainer.py:1165-1168: like a torch parameter whose .grad is None it keeps value, moments and step count, weight
        decay included): one backward with every .grad = None tells.  The probing gradients are moved into the static tensors."""
        key = self._phase_key(pretrain)
        if key in optimizer.tables:
            return key, False
        for p in optimizer.params:
            p.grad = None
        run_backward()
        reached = [p for p in optimizer.params if p.grad is not None]
        optimizer.adopt_grads()
        optimizer.add_table(key, reached)
        return key, True

    def _train_step_eager_router_hip(self, optimizer, batch: dict, pretrain: bool):
        """the router run eagerly under a RouterAdamW (no router graphs for this phase, a process group, or eval()): the same
        per-phase table, gate and skip rule as the captured step"""
        self.finish()
        out = {}

        def run():
            out.update(self._step_on(batch, pretrain))
            self.backward(out)
        key, probed = self._probe_phase_table(optimizer, pretrain, run)
        if not probed:
            optimizer.zero_grad()
            run()
        allreduce_mean_grads(self.trainable_parameters())
        optimizer.adopt_grads()
        gate = out["loss"].detach().to(torch.float32).reshape(1).clone()
        with torch.no_grad():
            before = optimizer.counters[0:1].clone()
            optimizer.step(table=key, gate=gate)
            out["applied"] = optimizer.counters[0:1] - before
            if optimizer.grad_norm is not None:
                out["grad_norm"] = optimizer.grad_norm.norm.clone()
        return out

    def _seed_args(self, batch: dict) -> dict:
        """step()'s seeded arguments from a batch (nothing without router_seed); the count of steps run advances by one"""
        if self.router_seed is None:
            return {}
        _require_seeds(batch)
        kw = dict(seeds=batch["seeds"], draw=int(batch.get("draw", 0)), noise_step=self.noise_steps)
        self.noise_steps += 1
        return kw

    def _step_on(self, batch: dict, pretrain: bool):
        return self.step(batch["noisy_latents"], batch["timesteps"], batch["encoder_hidden_states"],
                         batch["mpnet_embeddings"], batch["target"], pretrain=pretrain, **self._seed_args(batch))

    def train_step(self, optimizer, batch: dict, pretrain: bool = False):
        """forward + backward + fused gradient all-reduce + optimizer step (trainer.py:913-933)"""
        if self.router_seed is not None:
            _require_seeds(batch)
        if isinstance(optimizer, RouterAdamW):
            return self._train_step_eager_router_hip(optimizer, batch, bool(pretrain))
        optimizer.zero_grad(set_to_none=True)
        out = self._step_on(batch, pretrain)
        out["loss"].backward()
        allreduce_mean_grads(self.trainable_parameters())
        optimizer.step()
        return out


class GraphedPrunerStep(PrunerStep):
    """PrunerStep with the two U-Net passes replayed from HIP graphs.

    The pruning step is host-bound when run eagerly (≈10^4 launches per step at SD-2.1 size: two U-Net forwards, one
    backward, autograd glue).  Everything that touches the U-Net has static shapes, so it is captured once:

    * ``g_teacher``: the all-ones (dense) forward under no_grad -> ``full_pred`` and the 9 block activations;
    * ``g_student``: forward with the architecture code read from STATIC gate buffers;
    * ``g_student_bwd``: the three U-Net loss terms (min-SNR diffusion MSE, output distillation, block distillation:
      trainer.py:1197-1225) and the backward down to the gradient of those terms w.r.t. every gate buffer.

    Each step the router runs eagerly (it draws host-side Gumbel noise, quirk Q6, and is tiny), its architecture code is
    copied into the static buffer the 84 gate views alias, the graphs are replayed, and the chain rule is closed eagerly:
    ``autograd.backward([router-only losses, arch code], [None, captured gradient w.r.t. the code])``.
    Losses and router gradients equal the eager step's (tests/test_train_step_gpu.py).

    short_batches=True: capture(batch) fixes the LARGEST batch; step / train_step then take any 0 <= n <= B samples (or B samples
    with a "valid" vector) through the same graphs.  The three U-Net terms come from one masked ops.LossStage, the router's
    batch-coupled pieces -- Sinkhorn assignment, contrastive loss, MAC losses -- from ops.sinkhorn_assign and one ops.RouterStage,
    all reading `valid` on the device; the rows behind a short batch are its own first row and reach nothing.  The dict gains
    "n_valid" and "skipped"; an empty batch replays nothing, draws no noise and touches no state.  The Gumbel draws stay B rows
    per call from the host generator: the host stream advances by the same amount whatever n is, which is NOT the stream an eager
    n-row step would consume, unless `router_seed` is given.  Not under a process group.

    router_seed=<int>: the router's Gumbel noise is drawn on the device from batch["seeds"] (int64 [n]) and batch["draw"] (an int,
    default 0) by ONE launch per relaxation (ops.GumbelRelax): a sample's noise is the same in any batch, the host
    generator is neither read nor restored, no NoiseTape is made, and `noise_steps` (a host int, advanced once per non-empty
    call, set it on resume) is the only state the noise adds.  Not under a process group (the seeds are not gathered)."""

    def __init__(self, *a, short_batches: bool = False, router_seed: Optional[int] = None, **k):
        if short_batches and torch.distributed.is_available() and torch.distributed.is_initialized():
            raise NotImplementedError("GraphedPrunerStep(short_batches=True) under a process group: the router runs eagerly there, "
                                      "its collectives are not captured and `valid` is not gathered")
        if router_seed is not None and torch.distributed.is_available() and torch.distributed.is_initialized():
            raise NotImplementedError("GraphedPrunerStep(router_seed=) under a process group: the router runs eagerly there and "
                                      "the seeds are not gathered")
        super().__init__(*a, router_seed=router_seed, **k)
        self.short_batches = bool(short_batches)
        self._cap = None
        self.stream_probe = []          # what graph_utils.concurrent_stream measured when it chose the teacher's / router's side streams
        self.overlap_router = os.environ.get("APTP_OVERLAP_ROUTER", "1") != "0"
        self._finish_hooks = []

    def remove_hooks(self):
        super().remove_hooks()
        for h in self._finish_hooks:
            h.remove()
        self._finish_hooks = []

    # ---- capture ------------------------------------------------------------------------------------------------
    def _schedule_on(self, device):
        # keep the alpha-bar table on the device: a pageable host->device copy per step would make the host wait for the
        # previous step's graphs
        if self.schedule.alphas_cumprod.device != device:
            self.schedule.alphas_cumprod = self.schedule.alphas_cumprod.to(device)

    # the captured step's total is router_loss.detach() + unet_loss: the eager sum (_total_loss) split where the graphs split it
    def _router_loss(self, resource_loss, contrastive_loss, std_loss, max_loss):
        cfg = self.cfg
        return cfg.resource_weight * resource_loss + cfg.contrastive_weight * contrastive_loss \
            + cfg.std_weight * std_loss + cfg.max_weight * max_loss

    def _unet_loss(self, loss, distillation_loss, block_loss):
        return loss + self.cfg.distillation_weight * distillation_loss + self.cfg.block_weight * block_loss

    def capture(self, batch: dict, optimizer=None, pretrain: bool = False):
        """Capture the graphs for this batch geometry (call once; later batches must have the same shapes).
        optimizer: a CAPTURABLE optimizer over trainable_parameters() (torch.optim.AdamW(..., capturable=True)).  When given
        (and no process group is initialised: the router's collectives stay eager), the ROUTER is captured too -- hyper-net,
        quantiser incl. Sinkhorn, Gumbel relaxation, MAC losses as one graph ahead of the student's forward, and the chain rule
        into the router + the optimizer step as one graph behind the U-Net backward (trainer.py:1129-1138, :922-931) -- for this
        value of `pretrain`; its Gumbel noise keeps coming from the host generator (estimation_utils.NoiseTape) unless `router_seed`
        is given: then the captured relaxations draw it on the device from static seeds / draw / step tensors.
        A torch optimizer here is for a FRESH optimizer at a CONSTANT rate (the capture zeroes its state and bakes the rate in); a
        router_optim.RouterAdamW serves both phases, a warm-up, the NaN batch skip and a resume from one capture."""
        cfg = self.cfg
        dev = batch["noisy_latents"].device
        st = {k: batch[k].clone() for k in _BATCH_KEYS}
        self._schedule_on(dev)
        st["snr_w"] = _min_snr_weights(cfg, self.schedule, st["timesteps"])
        B = st["noisy_latents"].shape[0]
        short = self.short_batches
        if short:
            st["valid"] = torch.ones(int(B), dtype=torch.float32, device=dev)
            st["text"] = batch["mpnet_embeddings"].clone()         # what the eager router reads; a captured phase has its own
        if self.router_seed is not None:
            st["noise"] = self._static_noise(int(B), dev)         # likewise: seeds / draw / step of the eager router
        ones = torch.ones((B, self.quantizer.vq_embed_dim), device=dev)
        full = self.hyper_net.transform_structure_vector(ones)
        # ONE static buffer holds the student's architecture code, SEGMENT-MAJOR: gate j's [B, w_j] block is contiguous, so
        # the 84 gate tensors the U-Net reads are contiguous autograd LEAVES aliasing it (a column slice of a [B, 1634]
        # matrix would make every kernel wrapper take a strided -> contiguous copy of its gate: 231 five-microsecond copies
        # per replay).  No autograd edge outside the captured region (a view node recorded on the legacy default stream would
        # make the captured backward hop streams).  A step installs a new code with one gather (`install_code`), and the
        # captured backward ends by concatenating the 84 gate gradients and gathering them back into [B, 1634] order.
        widths = list(self.hyper_net.width_list)
        n_depth = sum(self.hyper_net.depth_list)
        E = sum(widths) + n_depth
        assert E == self.quantizer.vq_embed_dim
        col = torch.arange(E)
        perm, s0 = [], 0
        for w in widths + [1] * n_depth:                          # position in the flat buffer -> index into arch.reshape(-1)
            perm.append((torch.arange(B)[:, None] * E + col[s0:s0 + w][None, :]).reshape(-1))
            s0 += w
        perm = torch.cat(perm)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(perm.numel())
        perm, inv = perm.to(dev), inv.to(dev)
        ga = torch.ones(B * E, device=dev)
        gw, gd, s0 = [], [], 0
        for w in widths:
            gw.append(ga[s0:s0 + B * w].view(B, w).detach().requires_grad_(True))
            s0 += B * w
        for _ in range(n_depth):
            gd.append(ga[s0:s0 + B].detach().requires_grad_(True))
            s0 += B

        def install_code(arch):
            torch.index_select(arch.detach().reshape(-1), 0, perm, out=ga)
        from .macs import VectorizedMacs
        vmacs = VectorizedMacs(self.unet, device=dev)

        keep_stage = []                                    # the masked loss stage of the last student_bwd call (short_batches)

        def teacher():
            # own split-K counters / scratch: this graph replays NEXT TO the student's forward (ops.scratch_domain)
            with torch.no_grad(), ops.scratch_domain("teacher"):
                # the min-SNR weights of this batch: a dozen tiny launches that only the loss terms read -- inside this graph they
                # run on the side stream next to the router instead of ahead of everything on the caller's stream (0.8 ms of a step)
                st["snr_w"].copy_(_min_snr_weights(cfg, self.schedule, st["timesteps"]))
                pred = self.unet(st["noisy_latents"], st["timesteps"], st["encoder_hidden_states"]).sample.detach()
                return pred, dict(self.block_activations)

        def student_fwd():
            pred = self.unet(st["noisy_latents"], st["timesteps"], st["encoder_hidden_states"]).sample
            return pred, dict(self.block_activations)

        def student_bwd(pred, acts, full_pred, teacher_acts):
            if short:
                # _unet_losses and _unet_loss as ONE masked stage, in the pruner's term order: diffusion, distillation, blocks
                weighted = cfg.snr_gamma is not None
                terms = [ops.LossTerm(pred, st["target"], 0, 1.0, weighted), ops.LossTerm(pred, full_pred.detach(), 1)]
                terms += [ops.LossTerm(acts[k], teacher_acts[k].detach(), 2) for k in acts]
                stage = ops.LossStage(terms, (1.0, cfg.distillation_weight, cfg.block_weight), weights=st["snr_w"] if weighted else None,
                                      valid=st["valid"], group_div=(0.0, 0.0, float(len(acts))))
                grads = torch.autograd.grad(AG.loss_stage(stage), gw + gd, allow_unused=True)
                flat = torch.cat([(torch.zeros_like(t) if g is None else g).reshape(-1) for g, t in zip(grads, gw + gd)])
                o = stage.out                              # [diffusion, distillation, block, total, n]
                keep_stage.append(stage)
                return o[0], o[1], o[2], flat[inv].view(B, E)
            loss, dist, blk = self._unet_losses(pred, acts, full_pred, teacher_acts, st["snr_w"], st["target"])
            grads = torch.autograd.grad(self._unet_loss(loss, dist, blk), gw + gd, allow_unused=True)
            flat = torch.cat([(torch.zeros_like(t) if g is None else g).reshape(-1) for g, t in zip(grads, gw + gd)])
            grad = flat[inv].view(B, E)                        # back to the architecture vector's [B, 1634] order
            return loss.detach(), dist.detach(), blk.detach(), grad

        # warm-up on a side stream (allocator / plan caches), then capture: the module state at capture time decides what
        # is baked in, so the structure is installed right before each capture
        # ops.LAUNCH_LOG is filled by this eager pass, never by the captures (_launch_log_off)
        user_log = ops.LAUNCH_LOG
        log0 = None if user_log is None else len(user_log)
        with warmup_stream():
            self.unet.set_structure({"width": list(full["width"]), "depth": list(full["depth"])})
            fp, ta = teacher()
            self.unet.set_structure({"width": list(gw), "depth": list(gd)})
            student_bwd(*student_fwd(), fp, ta)
        launch_log = None if user_log is None else user_log[log0:]

        # THREE graphs.  The student's forward does not read the teacher (only the loss terms do), so it is its own graph:
        # at replay it starts as soon as the router has produced the code, NEXT TO the teacher graph that has been running
        # on the side stream since the batch arrived; the loss + backward graph joins the two.  Graphs that replay
        # concurrently must not share a memory pool (a pool hands one capture's freed scratch to the next capture, which is
        # only safe when replays are serialised in capture order): the teacher has its own, the two student graphs share one.
        with _launch_log_off():
            self.unet.set_structure({"width": list(full["width"]), "depth": list(full["depth"])})
            g_teacher = new_graph()
            with torch.cuda.graph(g_teacher):
                full_pred, teacher_acts = teacher()
            self.unet.set_structure({"width": list(gw), "depth": list(gd)})
            g_student = new_graph()
            with torch.cuda.graph(g_student):
                pred, acts = student_fwd()
            g_student_bwd = new_graph()
            with torch.cuda.graph(g_student_bwd, pool=g_student.pool()):
                loss, dist, blk, grad = student_bwd(pred, acts, full_pred, teacher_acts)
        # (everything a captured kernel reads must outlive the graphs: `inv` is an operand of the gather that ends g_student_bwd)
        self._cap = dict(st=st, ga=ga, install_code=install_code, perm=perm, inv=inv, full=full, pred=pred, acts=acts, teacher_acts=teacher_acts, gw=gw, gd=gd, g_teacher=g_teacher, g_student=g_student, g_student_bwd=g_student_bwd,
                         loss=loss, dist=dist, blk=blk, grad=grad, full_pred=full_pred, side=concurrent_stream(log=self.stream_probe), vmacs=vmacs,
                         launch_log=launch_log, router=None)
        if short:
            self._cap["loss_stage"] = keep_stage[-1]
            self._cap["n_valid"] = keep_stage[-1].out[4]
        if optimizer is not None and not (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self._capture_router(batch, optimizer, pretrain)           # (`dist` is the distillation loss in this scope)
        return self

    def _static_noise(self, B: int, device) -> RouterNoise:
        """the static seeds / draw / step tensors a seeded router reads (zeros until a batch is staged) and the codes' seeds"""
        return RouterNoise.of([0] * B, 0, self.router_seed, 0, self.quantizer.n_e, device)

    # ---- the router as two more graphs per training phase -------------------------------------------
    def _router_forward(self, text_embeddings, pretrain: bool, valid: Optional[torch.Tensor] = None, noise=None):
        """the router head and its own losses, MACs from the router-connected code (step() up to the student's code); with
        `valid` everything that couples the samples of the batch runs masked (quantiser, one ops.RouterStage); with `noise` (a
        RouterNoise) the Gumbel draws come from the seeds on the device"""
        if valid is not None:
            _, arch_vector_quantized, arch_used, arch_wdn = self._route_head(text_embeddings, pretrain, valid, noise)
            stage = self._masked_router_losses(text_embeddings, arch_wdn, self._cap["vmacs"](arch_used), valid)
            router_loss = AG.router_stage(stage)
            return dict(arch_used=arch_used, arch_vector_quantized=arch_vector_quantized, contrastive_loss=stage.contrastive,
                        resource_loss=stage.resource, ratios=stage.grad_inputs[1], resource_ratio=stage.mean_ratio,
                        std_loss=stage.std_loss, router_loss=router_loss, stage=stage)
        _, arch_vector_quantized, arch_used, contrastive_loss = self._route(text_embeddings, pretrain, noise)
        # MAC accounting is differentiable in the gates (calc_macs family): VectorizedMacs evaluates it on the router-connected
        # architecture vector directly (same numbers as unet.calc_macs() after set_structure, tests/test_macs_pinned.py) in
        # ~10 kernels instead of ~2,000, before the student replay is queued, so the host never waits on the graphs.
        ratios, resource_loss, max_loss, std_loss = self._mac_losses(self._cap["vmacs"](arch_used))
        return dict(arch_used=arch_used, arch_vector_quantized=arch_vector_quantized, contrastive_loss=contrastive_loss,
                    resource_loss=resource_loss, ratios=ratios,
                    router_loss=self._router_loss(resource_loss, contrastive_loss, std_loss, max_loss))

    def capture_router(self, batch: dict, pretrain: bool, optimizer=None):
        """Capture the router graphs of the OTHER training phase next to the ones capture(batch, optimizer=RouterAdamW, pretrain=)
        made: train_step(optimizer, batch, pretrain=) then picks a set by its argument, so the switch at
        hypernet_pretraining_steps (trainer.py:892) costs nothing.  Legal in any state of the run: parameters, moments, step
        counts, counters and the host generator are as before afterwards."""
        assert self._cap is not None, "capture_router: call capture(batch, ...) first"
        rt = self._cap.get("router")
        optimizer = optimizer if optimizer is not None else (rt or {}).get("optimizer")
        assert isinstance(optimizer, RouterAdamW), "capture_router: the router is captured per phase under a router_optim.RouterAdamW"
        assert not rt or (rt["hip"] and rt["optimizer"] is optimizer), "capture_router: another optimizer was captured"
        assert not (torch.distributed.is_available() and torch.distributed.is_initialized()), \
            "capture_router: with a process group the router stays eager (its collectives are not captured)"
        self._capture_router(batch, optimizer, pretrain)
        return self

    def _capture_router(self, batch, optimizer, pretrain):
        """One phase of the router as g_fwd (router -> code installed for the student) and g_bwd (chain rule into the router +
        optimizer step) in one pool, under either kind of optimizer.  cap["router"] holds optimizer, stream, events and `pending`;
        each captured phase sits under its bool(pretrain).  A torch optimizer (capturable, fresh, constant rate) has one phase: a
        capture under it replaces the record.  A RouterAdamW adds phases to its record and gates the step on the total loss."""
        from . import estimation_utils as EU
        cap, pretrain = self._cap, bool(pretrain)
        hip = isinstance(optimizer, RouterAdamW)
        rt = cap.get("router")
        params = self.trainable_parameters()
        if hip:
            assert not rt or rt["hip"], "capture: the router was already captured under a torch optimizer"
            assert set(map(id, params)) == set(map(id, optimizer.params)), "capture: the RouterAdamW must hold exactly trainable_parameters()"
            optimizer.before_access = self.finish
            self.finish()
        else:
            assert optimizer.defaults.get("capturable", False), "GraphedPrunerStep.capture(optimizer=): the optimizer must be capturable"
            rt = None
        text = batch["mpnet_embeddings"].clone()
        # a phase's router graphs replay on the router's stream next to the NEXT step's staging on the caller's: they read a mask of
        # their own, staged on that stream like `text` (st["valid"] belongs to the loss stage and the eager router, on the caller's)
        valid = torch.ones_like(cap["st"]["valid"]) if self.short_batches else None
        # a seeded router draws nothing on the host: no tape, and the host generator is neither read nor restored; its seeds, draw
        # and step are this phase's own, staged on the router's stream like `text` and `valid`
        seeded = self.router_seed is not None
        noise = self._static_noise(int(text.shape[0]), text.device) if seeded else None
        tape = None if seeded else EU.NoiseTape()
        host_rng = None if seeded else torch.get_rng_state()
        # (the MAC constants of count_macs are operands of the captured MAC losses: the phase keeps them alive, so that a later
        #  count_macs on a U-Net that several steps share cannot free what these graphs read)
        ph = dict(text=text, tape=tape, valid=valid, noise=noise, resource_info=self.unet.resource_info_dict)

        def fwd():
            if seeded:
                r = self._router_forward(text, pretrain, valid, noise)
            else:
                tape.begin()
                EU.NOISE_TAPE = tape
                try:
                    r = self._router_forward(text, pretrain) if valid is None else self._router_forward(text, pretrain, valid)
                finally:
                    EU.NOISE_TAPE = None
            with torch.no_grad():
                cap["install_code"](r["arch_used"])
            return r

        def backward_only(r):
            ts = [r["arch_used"]] if r["arch_used"].requires_grad else []
            torch.autograd.backward([r["router_loss"]] + ts, [None] + ([cap["grad"]] if ts else []))

        # The warm-up (allocator, caches -- gather indices, segment maps --, the optimizer's state tensors) takes optimizer steps;
        # capturing must cost the training run nothing, so they are undone IN PLACE (the addresses go into the graphs).
        if hip:
            # in any state of the run: everything the warm-up changes is snapshotted and put back, nothing is blanket-zeroed
            ph["gate"] = gate = torch.zeros(1, dtype=torch.float32, device=text.device)     # the step's total loss: AptpGroupAdamWParams.gate_dev
            ph["applied"] = applied = torch.zeros(1, dtype=torch.float32, device=text.device)   # 1: the step was applied, 0: skipped
            snap = optimizer._snapshot()

            def optimizer_step(r):                    # (the backward accumulated into the static, zero-filled .grad tensors in place)
                with torch.no_grad():
                    gate.copy_((r["router_loss"].detach() + self._unet_loss(cap["loss"], cap["dist"], cap["blk"])).reshape(1))
                    applied.copy_(optimizer.counters[0:1])
                    optimizer.step(table=ph["table"], gate=gate)
                    torch.sub(optimizer.counters[0:1], applied, out=applied)

            def undo_warmup():
                optimizer._restore(snap)
                torch.cuda.synchronize()
        else:
            # a fresh optimizer: parameters back to their values, moments and step counts to zero
            saved_p = [p.detach().clone() for p in params]

            def optimizer_step(r):
                optimizer.step()

            def undo_warmup():
                with torch.no_grad():
                    for p, s0 in zip(params, saved_p):
                        p.copy_(s0)
                    for stt in optimizer.state.values():
                        for v in stt.values():
                            if torch.is_tensor(v):
                                v.zero_()
                for p in params:
                    p.grad = None

        def bwd(r):
            backward_only(r)
            optimizer_step(r)

        with warmup_stream():
            if hip:
                ph["table"], _ = self._probe_phase_table(optimizer, pretrain, lambda: backward_only(fwd()))
                optimizer.zero_grad()
            for _ in range(2):
                if not hip:
                    for p in params:
                        p.grad = None
                bwd(fwd())
        undo_warmup()
        ph["g_fwd"] = new_graph()
        with torch.cuda.graph(ph["g_fwd"]):
            ph["out"] = fwd()
        ph["g_bwd"] = new_graph()
        with torch.cuda.graph(ph["g_bwd"], pool=ph["g_fwd"].pool()):
            bwd(ph["out"])
        if host_rng is not None:
            torch.set_rng_state(host_rng)
        if not rt:
            rt = cap["router"] = dict(hip=hip, optimizer=optimizer, stream=concurrent_stream(log=self.stream_probe),
                                      ev_entry=torch.cuda.Event(), ev_code=torch.cuda.Event(), ev_bwd=torch.cuda.Event(),
                                      ev_tail=torch.cuda.Event(), pending=False)
        rt[pretrain] = ph
        if not self._finish_hooks:
            # anything that reads the router's parameters outside the captured step first waits for the pending optimizer step
            for m in (self.hyper_net, self.quantizer):
                self._finish_hooks.append(m.register_forward_pre_hook(lambda *_a, **_k: self.finish()))
                self._finish_hooks.append(m.register_state_dict_pre_hook(lambda *_a, **_k: self.finish()))

    def graph_nodes(self):
        """nodes (kernel launches + torch's few memcpy / memset nodes) of the three captured graphs, when they were kept
        (graph_utils.KEEP_GRAPHS): {"teacher", "student_fwd", "student_bwd"}; with a captured router also "router_fwd" and
        "router_bwd_and_optimizer" (under a RouterAdamW: of the main phase when it was captured, else of the pre-training phase,
        whose own pair is then also reported with the suffix "_pretrain")"""
        cap = self._cap
        if cap is None:
            return None
        n = {"teacher": node_count(cap["g_teacher"]), "student_fwd": node_count(cap["g_student"]),
             "student_bwd": node_count(cap["g_student_bwd"])}
        rt = cap.get("router")
        if rt:
            if rt["hip"] and True in rt:
                n["router_fwd_pretrain"] = node_count(rt[True]["g_fwd"])
                n["router_bwd_and_optimizer_pretrain"] = node_count(rt[True]["g_bwd"])
            ph = rt.get(False, rt.get(True))
            n["router_fwd"] = node_count(ph["g_fwd"])
            n["router_bwd_and_optimizer"] = node_count(ph["g_bwd"])
        return n

    # ---- one step -------------------------------------------------------------------------------------------------------
    def step(self, noisy_latents, timesteps, encoder_hidden_states, text_embeddings, target, pretrain: bool = False,
             valid: Optional[torch.Tensor] = None, seeds=None, draw: int = 0, noise_step: int = 0):
        """valid: short_batches only -- one entry per sample of this batch (samples masked without compacting them).
        seeds / draw / noise_step: router_seed only -- as PrunerStep.step takes them"""
        if self._cap is None:
            assert valid is None and not self.short_batches, "GraphedPrunerStep(short_batches=True): call capture(batch) first"
            return super().step(noisy_latents, timesteps, encoder_hidden_states, text_embeddings, target, pretrain,
                                seeds=seeds, draw=draw, noise_step=noise_step)
        cap = self._cap
        assert valid is None or self.short_batches, "step(valid=): only under short_batches=True"
        noise = None
        if self.router_seed is not None:
            if seeds is None:
                raise ValueError("GraphedPrunerStep(router_seed=).step: seeds= is required (one seed per sample)")
            if len(seeds) != int(text_embeddings.shape[0]):
                raise ValueError(f"{len(seeds)} seeds for {int(text_embeddings.shape[0])} samples")
            _check_draw(draw, noise_step)
            noise = cap["st"]["noise"]
        elif seeds is not None:
            raise ValueError("step(seeds=): the step was built without router_seed")
        # The teacher depends on the batch only: its graph replays on a side stream WHILE the router (launch-bound kernels of a
        # few microseconds each, during which the GPU is mostly idle) is being issued on this stream.
        # Order on the device: batch copies -> [teacher graph || router] -> student graph.
        if self.short_batches:
            batch = dict(zip(_BATCH_KEYS, (noisy_latents, timesteps, encoder_hidden_states, target)))
            if valid is not None:
                batch["valid"] = valid
            if _stage_short_batch(cap["st"], batch) == 0:
                return self._skipped_step()
            _stage_short_rows(cap["st"]["text"], text_embeddings)
            if noise is not None:
                _stage_seeds(noise, seeds, draw, noise_step)
            self._launch_teacher()
            r = self._router_forward(cap["st"]["text"], pretrain, cap["st"]["valid"], noise)
        else:
            self._stage_batch_and_launch_teacher(noisy_latents, timesteps, encoder_hidden_states, target)
            if noise is not None:
                _stage_seeds(noise, seeds, draw, noise_step)
            r = self._router_forward(text_embeddings, pretrain, None, noise)
        with torch.no_grad():
            cap["install_code"](r["arch_used"])
        cap["g_student"].replay()                                     # forward: needs the code only
        torch.cuda.current_stream().wait_stream(cap["side"])          # teacher outputs ready
        cap["g_student_bwd"].replay()                                 # losses against the teacher + backward to the code
        return {**self._captured_losses(r["router_loss"]),
                "contrastive_loss": r["contrastive_loss"].detach(), "resource_loss": r["resource_loss"].detach(),
                "resource_ratio": self._resource_ratio(r), "arch_vector_quantized": r["arch_vector_quantized"].detach(),
                "_router_loss": r["router_loss"], "_gate_tensors": [r["arch_used"]], "_gate_grads": [cap["grad"]],
                **self._short_batch_report(r)}

    @staticmethod
    def _resource_ratio(r):
        """the mean prunable-MAC ratio a step reports: over the samples present where the router ran masked"""
        return r["resource_ratio"].detach().clone() if "stage" in r else r["ratios"].mean().detach()

    def _short_batch_report(self, r):
        if not self.short_batches:
            return {}
        return {"n_valid": self._cap["n_valid"].clone(), "skipped": False, "std_loss": r["std_loss"].detach().clone()}

    def _skipped_step(self):
        """an empty batch under short_batches: nothing was staged, replayed or drawn"""
        zero = torch.zeros((), dtype=torch.float32, device=self._cap["st"]["valid"].device)
        keys = ("loss", "diff_loss", "distillation_loss", "block_loss", "contrastive_loss", "resource_loss", "resource_ratio", "n_valid")
        return {**{k: zero.clone() for k in keys}, "applied": zero.reshape(1).clone(), "skipped": True}

    def _captured_losses(self, router_loss):
        """the step's total and the three U-Net terms as clones of g_student_bwd's static outputs (the next replay overwrites them)"""
        cap = self._cap
        return {"loss": (router_loss.detach() + self._unet_loss(cap["loss"], cap["dist"], cap["blk"])).clone(),
                "diff_loss": cap["loss"].clone(), "distillation_loss": cap["dist"].clone(), "block_loss": cap["blk"].clone()}

    def _stage_batch_and_launch_teacher(self, noisy_latents, timesteps, encoder_hidden_states, target):
        _stage_batch(self._cap["st"], (noisy_latents, timesteps, encoder_hidden_states, target))
        self._launch_teacher()

    def _launch_teacher(self):
        cap = self._cap
        side = cap["side"]                       # (the min-SNR weights are computed from the staged timesteps inside g_teacher)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            cap["g_teacher"].replay()

    @staticmethod
    def backward(out: dict):
        """Close the chain rule: d(total)/d(router) = d(router-only terms) + sum_g dL_unet/dgate_g * dgate_g/d(router)."""
        if "_router_loss" not in out:
            out["loss"].backward()
            return
        ts = [t for t in out["_gate_tensors"] if t.requires_grad]
        gs = [g for t, g in zip(out["_gate_tensors"], out["_gate_grads"]) if t.requires_grad]
        torch.autograd.backward([out["_router_loss"]] + ts, [None] + gs)

    def _step_on(self, batch: dict, pretrain: bool):
        return self.step(batch["noisy_latents"], batch["timesteps"], batch["encoder_hidden_states"],
                         batch["mpnet_embeddings"], batch["target"], pretrain=pretrain,
                         valid=batch.get("valid") if self.short_batches else None, **self._seed_args(batch))

    def train_step(self, optimizer, batch: dict, pretrain: bool = False):
        if self.router_seed is not None:
            _require_seeds(batch)                        # before anything runs
        if self.short_batches:
            assert self._cap is not None, "GraphedPrunerStep(short_batches=True): call capture(batch) first"
            B, n = int(self._cap["st"]["valid"].shape[0]), int(batch["noisy_latents"].shape[0])
            if n > B:
                raise ValueError(f"a batch of {n} samples does not fit the step captured for {B}")
            if n == 0:
                return self._skipped_step()              # before anything: no probe, no zero_grad, no noise, no replay
        rt = self._cap.get("router") if self._cap is not None else None
        ph = rt.get(bool(pretrain)) if rt and rt["optimizer"] is optimizer else None
        if ph is not None and self.hyper_net.training:
            return self._train_step_captured_router(batch, ph)
        if isinstance(optimizer, RouterAdamW):
            return self._train_step_eager_router_hip(optimizer, batch, bool(pretrain))
        self.finish()
        optimizer.zero_grad(set_to_none=True)
        out = self._step_on(batch, pretrain)
        self.backward(out)
        allreduce_mean_grads(self.trainable_parameters())
        optimizer.step()
        return out

    def _train_step_captured_router(self, batch: dict, ph: dict):
        """the whole step from five graphs: [teacher || router] -> student forward -> losses + U-Net backward -> chain rule into the
        router + optimizer.  The host only stages the batch and refills the Gumbel uniforms from its generator (under router_seed:
        stages the seeds, and draws nothing).

        The two router graphs are chains of a few hundred tiny launches (0.9 + 1.3 ms during which the chip idles).  With
        overlap_router (default) they replay on a stream of their own: the NEXT step's batch staging and teacher forward do not
        queue behind this step's router backward + optimizer, they run next to it; the student's forward waits for the code
        (ev_code), the router backward for the U-Net backward (ev_bwd).  Reading router parameters on another stream afterwards
        needs finish() -- the router modules' forward / state_dict hooks and the eager train_step call it.
        ph: the graph set of this training phase; captured under a RouterAdamW, the returned dict also has "applied", a device flag
        written on the router's stream (1: the step was applied, 0: skipped) -- call finish() before reading it."""
        cap = self._cap
        rt = cap["router"]
        main = torch.cuda.current_stream()
        rs = rt["stream"] if self.overlap_router else main
        rt["ev_entry"].record(main)                           # the batch tensors were produced on the caller's stream
        if self.short_batches:
            _stage_short_batch(cap["st"], batch)              # (train_step returned before this for an empty batch)
            self._launch_teacher()
        else:
            self._stage_batch_and_launch_teacher(batch["noisy_latents"], batch["timesteps"], batch["encoder_hidden_states"], batch["target"])
        with torch.cuda.stream(rs):
            rs.wait_event(rt["ev_entry"])
            if self.short_batches:
                # both operands of the router graphs are written HERE, on the stream that replays them: behind the previous step's
                # g_bwd (same stream), ahead of this step's g_fwd, and behind ev_entry (the batch's own tensors)
                _stage_short_rows(ph["text"], batch["mpnet_embeddings"])
                _stage_valid(ph["valid"], batch.get("valid"), int(batch["mpnet_embeddings"].shape[0]))
            else:
                with torch.no_grad():
                    ph["text"].copy_(batch["mpnet_embeddings"])
            if ph["noise"] is not None:
                # the seeds, the draw and the count of steps run, staged where `text` is: nothing is drawn on the host
                _stage_seeds(ph["noise"], batch["seeds"], int(batch.get("draw", 0)), self.noise_steps)
                self.noise_steps += 1
            else:
                ph["tape"].refill()                           # host-RNG stream, consumed exactly as the eager calls consume it
            ph["g_fwd"].replay()                              # router -> architecture code installed for the student
            rt["ev_code"].record(rs)
        main.wait_event(rt["ev_code"])
        cap["g_student"].replay()
        main.wait_stream(cap["side"])
        cap["g_student_bwd"].replay()
        rt["ev_bwd"].record(main)
        with torch.cuda.stream(rs):
            rs.wait_event(rt["ev_bwd"])
            ph["g_bwd"].replay()                              # d(router losses + U-Net terms)/d(router), optimizer step
            applied = ph["applied"].clone() if "applied" in ph else None
            gn = rt["optimizer"].grad_norm if rt["hip"] else None
            grad_norm = gn.norm.clone() if gn is not None else None
            rt["ev_tail"].record(rs)
        rt["pending"] = rs is not main
        r = ph["out"]
        # (the router graph's outputs were complete at ev_code; the next router forward, which overwrites them, waits for the next
        #  step's ev_entry, i.e. for these clones.  Under short_batches nothing the router graphs read is written on this stream:
        #  ph["text"] and ph["valid"] are staged on the router's stream, st["valid"] is read by g_student_bwd on this one only)
        out = {**self._captured_losses(r["router_loss"]),
               "contrastive_loss": r["contrastive_loss"].detach().clone(), "resource_loss": r["resource_loss"].detach().clone(),
               "resource_ratio": self._resource_ratio(r), "arch_vector_quantized": r["arch_vector_quantized"].detach().clone(),
               **self._short_batch_report(r)}
        if applied is not None:
            applied.record_stream(main)
            out["applied"] = applied
        if grad_norm is not None:
            grad_norm.record_stream(main)
            out["grad_norm"] = grad_norm
        return out

    def finish(self):
        """make the current stream wait for the router backward + optimizer of the last captured step (they run on the router's own
        stream); called by the router modules' forward / state_dict hooks and by the eager paths of this class"""
        rt = self._cap.get("router") if self._cap is not None else None
        if rt is not None and rt.get("pending"):
            torch.cuda.current_stream().wait_event(rt["ev_tail"])
            rt["pending"] = False


def scaled_lr(lr: float, batch: int, accumulation: int = 1, world: int = 1) -> float:
    """`scale_lr` of the recipes (pdm/training/trainer.py:806-812, 1521-1527): the configured rate times the square root of the
    effective batch, lr * sqrt(accumulation * batch * world)"""
    import math
    return lr * math.sqrt(accumulation * batch * world)


def synthetic_batch(batch: int, latent: int, device, seed: int = 1234, cross_dim: int = 1024, text_dim: int = 768):
    """SURVEY §8d synthetic CC3M-shape batch: latents/target N(0,1), text states N(0,1), MPNet embeddings 0.05*N(0,1),
    random integer timesteps."""
    g = torch.Generator().manual_seed(seed)
    return {
        "noisy_latents": torch.randn(batch, 4, latent, latent, generator=g).to(device),
        "target": torch.randn(batch, 4, latent, latent, generator=g).to(device),
        "encoder_hidden_states": torch.randn(batch, 77, cross_dim, generator=g).to(device),
        "mpnet_embeddings": (0.05 * torch.randn(batch, text_dim, generator=g)).to(device),
        "timesteps": torch.randint(0, 1000, (batch,), generator=g).to(device),
    }


def noisy_latents_and_target(latents: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor,
                             alphas_cumprod: torch.Tensor, prediction_type: str = "v_prediction"):
    """diffusers DDPMScheduler.add_noise and the training target (trainer.py:1097-1122):
    noisy = sqrt(ac[t]) x0 + sqrt(1 - ac[t]) noise; target = sqrt(ac[t]) noise - sqrt(1 - ac[t]) x0 (v_prediction,
    DDPMScheduler.get_velocity) or noise (epsilon)"""
    ac = alphas_cumprod.to(device=latents.device, dtype=latents.dtype)
    t = timesteps.to(latents.device)
    sa = (ac[t] ** 0.5).flatten().reshape(-1, *([1] * (latents.dim() - 1)))
    so = ((1 - ac[t]) ** 0.5).flatten().reshape(-1, *([1] * (latents.dim() - 1)))
    noisy = sa * latents + so * noise
    if prediction_type == "epsilon":
        target = noise
    elif prediction_type == "v_prediction":
        target = sa * noise - so * latents
    else:
        raise ValueError(f"unknown prediction_type {prediction_type!r}")
    return noisy, target


def router_embeddings(prompt_encoder, router_ids: torch.Tensor, router_attention_mask: Optional[torch.Tensor] = None):
    """batch["mpnet_embeddings"] from the router's token ids (pdm/utils/data_utils.py:158-172): fp32 [B, 768] =
    prompt_encoder.encode(router_ids, router_attention_mask) on the HIP MPNet encoder (prompt_encoder.MPNetModel)"""
    if prompt_encoder is None:
        raise ValueError("router_ids need a prompt_encoder (diffusion_pruning_amd.prompt_encoder.MPNetModel)")
    return prompt_encoder.encode(router_ids, router_attention_mask)


def _check_noise_knobs(what: str, schedule: NoiseSchedule, noise_offset, input_perturbation, max_scheduler_steps) -> int:
    """the three reference knobs (model.unet.noise_offset / input_perturbation / max_scheduler_steps) -> T of the timestep draw"""
    for name, v in (("noise_offset", noise_offset), ("input_perturbation", input_perturbation)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or abs(v) == float("inf"):
            raise ValueError(f"{what}: {name} must be a finite number, got {v!r}")
    T = int(schedule.alphas_cumprod.shape[0])
    if max_scheduler_steps is None:
        return T
    if isinstance(max_scheduler_steps, bool) or not isinstance(max_scheduler_steps, int) or not 1 <= max_scheduler_steps <= T:
        raise ValueError(f"{what}: max_scheduler_steps must be an int in 1..{T}, got {max_scheduler_steps!r}")
    return max_scheduler_steps


def batch_from_images(vae, pixel_values: torch.Tensor, encoder_hidden_states: torch.Tensor,
                      mpnet_embeddings: Optional[torch.Tensor] = None,
                      schedule: Optional[NoiseSchedule] = None, prediction_type: str = "v_prediction", generator=None, *,
                      router_ids: Optional[torch.Tensor] = None, router_attention_mask: Optional[torch.Tensor] = None,
                      prompt_encoder=None, seeds=None, draw: int = 0, noise_offset: float = 0.0, input_perturbation: float = 0.0,
                      max_scheduler_steps: Optional[int] = None):
    """A training batch (synthetic_batch's keys) from images, as the reference's training steps build it
    (trainer.py:1097-1122): latents = vae.encode(pixel_values).latent_dist.sample() * scaling_factor (vae.encode_latents, one
    pass on the HIP encoder), then noise and timesteps, drawn in that order from ``generator``, add_noise and the target.
    pixel_values: NCHW [B, 3, H, W] in [-1, 1] on the GPU; H and W multiples of 8.
    The router's input is either ``mpnet_embeddings`` [B, 768] or ``router_ids`` (+ ``router_attention_mask``), the MPNet token
    ids, which ``prompt_encoder`` encodes (router_embeddings); exactly one of the two.
    ``noise_offset``, ``input_perturbation`` and ``max_scheduler_steps`` are the reference's ``model.unet.*`` keys
    (trainer.py:1100-1123): drawn from ``generator`` in its order -- noise, offset randn(B, C, 1, 1), perturbation randn_like,
    randint(0, max_scheduler_steps) -- and, at their defaults, not at all.  The target is built from the noise with its offset,
    the noisy latents from the perturbed noise.
    With ``seeds`` (an int, B ints or a device int64 [B] tensor) and ``draw`` (an epoch or a global step in [0, 2^59)) nothing
    comes from a generator: the encoder returns its moments and ONE launch (ops.train_noise) samples the posterior,
    the noise and the timesteps, each sample's a pure function of (its seed, draw), whatever batch or rank it sits in."""
    if (mpnet_embeddings is None) == (router_ids is None):
        raise ValueError("give exactly one of mpnet_embeddings and router_ids")
    if router_ids is None and router_attention_mask is not None:
        raise ValueError("router_attention_mask needs router_ids")
    schedule = schedule or NoiseSchedule()
    T = _check_noise_knobs("batch_from_images", schedule, noise_offset, input_perturbation, max_scheduler_steps)
    if prediction_type not in ("epsilon", "v_prediction"):
        raise ValueError(f"unknown prediction_type {prediction_type!r}")
    if seeds is not None:
        from .data import check_train_draw
        if generator is not None:
            raise ValueError("batch_from_images: give seeds or a generator, not both")
        check_train_draw(draw, "batch_from_images")
    elif draw != 0:
        raise ValueError("batch_from_images: draw needs seeds")
    if router_ids is not None:
        mpnet_embeddings = router_embeddings(prompt_encoder, router_ids, router_attention_mask)
    if seeds is not None:
        moments = vae.encode(pixel_values).latent_dist.parameters
        out = ops.train_noise(moments, sqrt_table=schedule.sqrt_table(moments.device)[:T], seeds=seeds, draw=draw,
                              scale=vae.config.scaling_factor, noise_offset=noise_offset, input_perturbation=input_perturbation,
                              prediction_type=prediction_type)
        return {"noisy_latents": out["noisy_latents"], "target": out["target"], "encoder_hidden_states": encoder_hidden_states,
                "mpnet_embeddings": mpnet_embeddings, "timesteps": out["timesteps"]}
    from .vae import randn_tensor
    latents = vae.encode_latents(pixel_values, generator=generator)
    dev = latents.device
    noise = randn_tensor(latents.shape, generator=generator, device=dev, dtype=latents.dtype)
    if noise_offset:
        noise = noise + noise_offset * randn_tensor((latents.shape[0], latents.shape[1], 1, 1), generator=generator, device=dev,
                                                    dtype=latents.dtype)
    new_noise = noise
    if input_perturbation:
        new_noise = noise + input_perturbation * randn_tensor(latents.shape, generator=generator, device=dev, dtype=latents.dtype)
    tdev = generator.device if generator is not None else dev
    timesteps = torch.randint(0, T, (latents.shape[0],), generator=generator, device=tdev).to(dev)
    noisy, target = noisy_latents_and_target(latents, noise, timesteps, schedule.alphas_cumprod, prediction_type)
    if input_perturbation:
        noisy, _ = noisy_latents_and_target(latents, new_noise, timesteps, schedule.alphas_cumprod, "epsilon")
    return {"noisy_latents": noisy, "target": target, "encoder_hidden_states": encoder_hidden_states,
            "mpnet_embeddings": mpnet_embeddings, "timesteps": timesteps}


def batch_from_uint8(vae, images, *, resolution: int, center_crop: bool = False, random_flip: bool = True,
                     transform_generator=None, prompt_ids: Optional[torch.Tensor] = None, text_encoder=None,
                     encoder_hidden_states: Optional[torch.Tensor] = None, mpnet_embeddings: Optional[torch.Tensor] = None,
                     schedule: Optional[NoiseSchedule] = None, prediction_type: str = "v_prediction", generator=None,
                     router_ids: Optional[torch.Tensor] = None, router_attention_mask: Optional[torch.Tensor] = None,
                     prompt_encoder=None, seeds=None, draw: int = 0, noise_offset: float = 0.0, input_perturbation: float = 0.0,
                     max_scheduler_steps: Optional[int] = None):
    """batch_from_images from raw inputs: ``images`` is a list of decoded uint8 [H, W, 3] tensors of any sizes, which the
    dataloader's transform (data.TrainTransform: bilinear Resize(resolution), RandomCrop or CenterCrop, RandomHorizontalFlip,
    ToTensor, Normalize(0.5, 0.5); its draws from ``transform_generator``, a CPU generator) turns into pixel_values on the GPU;
    the cross-attention input is either ``encoder_hidden_states`` or ``prompt_ids``, the CLIP token ids [B, 77], which
    ``text_encoder`` (text_encoder.CLIPTextModel) encodes as the reference's steps do (trainer.py:1097-1126:
    ``text_encoder(ids)[0]``); exactly one of the two.  Everything else is batch_from_images' and goes to it unchanged; with
    ``seeds`` the crop and the flip of each image come from its seed too (data.draw_crop_flip_seeded), and neither generator is
    taken."""
    if (prompt_ids is None) == (encoder_hidden_states is None):
        raise ValueError("give exactly one of prompt_ids and encoder_hidden_states")
    if prompt_ids is not None and text_encoder is None:
        raise ValueError("prompt_ids need a text_encoder (diffusion_pruning_amd.text_encoder.CLIPTextModel)")
    if seeds is not None and (transform_generator is not None or generator is not None):
        raise ValueError("batch_from_uint8: give seeds or generators, not both")
    from .data import TrainTransform
    transform = TrainTransform(resolution, center_crop=center_crop, random_flip=random_flip)
    sizes = transform.resized_sizes(images)                    # the images are checked before anything runs
    if seeds is not None:
        from .data import seed_list, check_train_draw
        check_train_draw(draw, "batch_from_uint8")
        seed_list(seeds, len(sizes), "batch_from_uint8")      # and so are the seeds
    elif draw != 0:
        raise ValueError("batch_from_uint8: draw needs seeds")
    if prompt_ids is not None:
        encoder_hidden_states = text_encoder(prompt_ids)[0]
    pixel_values = transform(images, generator=transform_generator, seeds=seeds, draw=draw)
    return batch_from_images(vae, pixel_values, encoder_hidden_states, mpnet_embeddings, schedule, prediction_type, generator,
                             router_ids=router_ids, router_attention_mask=router_attention_mask, prompt_encoder=prompt_encoder,
                             seeds=seeds, draw=draw, noise_offset=noise_offset, input_perturbation=input_perturbation,
                             max_scheduler_steps=max_scheduler_steps)


class SeededBatchBuilder:
    """The seeded batch assembly as a captured step would embed it: static ``seeds`` int64 [B], ``draw`` int64 [1] and output
    buffers on the device, ``build(moments)`` ONE launch (ops.train_noise) into them with no host value but the constructor's, and
    ``set(seeds, draw)`` two copies into the static tensors -- so a captured ``build`` follows them from replay to replay.
    ``latent_shape`` is (4, h, w); ``scale`` the VAE's scaling_factor; the other knobs are batch_from_images'."""

    def __init__(self, schedule: Optional[NoiseSchedule], batch: int, latent_shape, device, prediction_type: str = "v_prediction",
                 noise_offset: float = 0.0, input_perturbation: float = 0.0, scale: float = 1.0,
                 max_scheduler_steps: Optional[int] = None):
        schedule = schedule or NoiseSchedule()
        T = _check_noise_knobs("SeededBatchBuilder", schedule, noise_offset, input_perturbation, max_scheduler_steps)
        if prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"unknown prediction_type {prediction_type!r}")
        shape = tuple(int(v) for v in latent_shape)
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1 or len(shape) != 3 or shape[0] != 4 or min(shape) < 1:
            raise ValueError(f"SeededBatchBuilder: batch >= 1 and latent_shape (4, h, w), got {batch!r} and {latent_shape!r}")
        device = torch.device(device)
        self.batch, self.latent_shape, self.prediction_type = batch, shape, prediction_type
        self.noise_offset, self.input_perturbation, self.scale = float(noise_offset), float(input_perturbation), float(scale)
        self.sqrt_table = schedule.sqrt_table(device)[:T]
        self.seeds = torch.zeros(batch, dtype=torch.int64, device=device)
        self.draw = torch.zeros(1, dtype=torch.int64, device=device)
        self.out = {"noisy_latents": torch.empty((batch,) + shape, dtype=torch.float32, device=device),
                    "target": torch.empty((batch,) + shape, dtype=torch.float32, device=device),
                    "timesteps": torch.empty(batch, dtype=torch.int64, device=device)}

    def set(self, seeds, draw: int):
        """new seeds (an int, B ints or an int64 [B] tensor) and a new draw, copied into the static tensors on the current stream"""
        from .data import seed_list, check_train_draw
        check_train_draw(draw, "SeededBatchBuilder.set")
        if isinstance(seeds, torch.Tensor):
            if seeds.dtype != torch.int64 or tuple(seeds.shape) != (self.batch,):
                raise ValueError(f"SeededBatchBuilder.set: a seeds tensor must be int64 [{self.batch}]")
            self.seeds.copy_(seeds, non_blocking=True)
        else:
            vals = seed_list(seeds, self.batch, "SeededBatchBuilder.set")
            self.seeds.copy_(torch.tensor([v - (1 << 64) if v >= (1 << 63) else v for v in vals], dtype=torch.int64))
        self.draw.copy_(torch.tensor([draw], dtype=torch.int64))
        return self

    def build(self, moments: torch.Tensor) -> dict:
        """moments fp32 [B, 8, h, w] -> the static {"noisy_latents", "target", "timesteps"}"""
        return ops.train_noise(moments, sqrt_table=self.sqrt_table, seeds=self.seeds, draw=0, draw_dev=self.draw, scale=self.scale,
                               noise_offset=self.noise_offset, input_perturbation=self.input_perturbation,
                               prediction_type=self.prediction_type, out=self.out)


@dataclass
class FinetuneLossConfig:
    """configs/finetuning/sd-2-1_cc3m.yaml:86-95"""
    snr_gamma: Optional[float] = 5.0
    prediction_type: str = "v_prediction"
    diffusion_weight: float = 0.01
    block_weight: float = 0.5
    distillation_weight: float = 0.5


class FineTunerStep:
    """Expert fine-tuning step (pdm/training/trainer.py:1683-1765, config 5): teacher = dense ungated U-Net under
    no_grad, student = physically pruned expert (UNet2DConditionModelPruned) with every parameter trainable;
    loss = w_d * minSNR-MSE + w_b * block-MSE + w_k * distill-MSE.  Experts never communicate ("one expert per GPU" =
    independent processes, scripts/aptp/finetune.py:27-28); ``data_parallel=True`` covers the optional case of one
    expert on several GPUs with BucketedGradReducer."""

    def __init__(self, student, teacher, cfg: Optional[FinetuneLossConfig] = None, schedule: Optional[NoiseSchedule] = None,
                 data_parallel: bool = False, bucket_bytes: int = 64 << 20, reduce_mode: str = "all_reduce"):
        self.student, self.teacher = student, teacher
        # data_parallel: ONE expert trained on several GPUs: bf16 gradient buckets all-reduced while the
        # backward is still running; the default is the reference's "one expert per GPU", which never communicates
        self._dp, self._bucket_bytes, self._reduce_mode, self._reducer_packed = data_parallel, bucket_bytes, reduce_mode, False
        self.reducer = BucketedGradReducer([p for p in student.parameters() if p.requires_grad], bucket_bytes, mode=reduce_mode) \
            if data_parallel else None
        self.cfg = cfg or FinetuneLossConfig()
        self.schedule = schedule or NoiseSchedule()
        self.acts_s: Dict[str, torch.Tensor] = {}
        self.acts_t: Dict[str, torch.Tensor] = {}
        self._hooks = _block_output_hooks(student, self.acts_s) + _block_output_hooks(teacher, self.acts_t)

    def _losses(self, model_pred, full_pred, w, target):
        """(total, diffusion, distillation, block) in the fine-tuner's order -- diffusion, block (skipped without a block weight),
        output distillation (trainer.py:1736-1763); autograd sums into model_pred in reverse creation order, so the order is part
        of the gradients' bits.  The block term reads the hooked activations of the last teacher and student passes."""
        cfg = self.cfg
        loss = _diffusion_term(cfg, model_pred, target, w)
        total = loss * cfg.diffusion_weight
        if cfg.block_weight > 0:
            blk = _block_term(self.acts_s, self.acts_t)
            total = total + cfg.block_weight * blk
        else:
            blk = torch.zeros((), device=model_pred.device)
        dist_l = _mse(model_pred, full_pred)
        total = total + cfg.distillation_weight * dist_l
        return total, loss.detach(), dist_l.detach(), blk.detach()

    def step(self, noisy_latents, timesteps, encoder_hidden_states, target):
        with torch.no_grad():
            full_pred = self.teacher(noisy_latents, timesteps, encoder_hidden_states).sample.detach()      # :1726-1727
        model_pred = self.student(noisy_latents, timesteps, encoder_hidden_states).sample                  # :1729
        w = _min_snr_weights(self.cfg, self.schedule, timesteps)
        loss, diff_loss, distillation_loss, block_loss = self._losses(model_pred, full_pred, w, target)
        return {"loss": loss, "diff_loss": diff_loss.clone(), "distillation_loss": distillation_loss, "block_loss": block_loss}

    def _loss_stage(self, model_pred, full_pred, w, target, valid) -> "ops.LossStage":
        """_losses as ONE ops.LossStage over the samples `valid` marks: group 0 the diffusion term (min-SNR weighted unless
        snr_gamma is None), group 1 the mean of the block terms (skipped without a block weight), group 2 the output
        distillation, with _losses' coefficients; every term a per-sample mean, averaged over the samples present"""
        cfg = self.cfg
        weighted = cfg.snr_gamma is not None
        terms = [ops.LossTerm(model_pred, target.detach(), 0, 1.0, weighted)]
        n_blocks = len(self.acts_s) if cfg.block_weight > 0 else 0
        if n_blocks:
            terms += [ops.LossTerm(self.acts_s[k], self.acts_t[k].detach(), 1) for k in self.acts_s]
        terms.append(ops.LossTerm(model_pred, full_pred.detach(), 2))
        return ops.LossStage(terms, self._group_coef(), weights=w if weighted else None, valid=valid,
                             group_div=(0.0, float(n_blocks), 0.0))

    def _group_coef(self):
        cfg = self.cfg
        return (cfg.diffusion_weight, cfg.block_weight if cfg.block_weight > 0 else 0.0, cfg.distillation_weight)

    @torch.no_grad()
    def eval_step(self, noisy_latents, timesteps, encoder_hidden_states, target):
        """One validation batch (FineTuner.validate's call of step, trainer.py:1787-1794): teacher and student forward without
        autograd -- under an attached PackedTrainer the student reads the packed, trained state (unet._ft_mode) -- and every loss
        term from ONE ops.LossTerms call: three launches where `step` under no_grad issues two per term and per sample plus the
        torch glue.  Returns the four device scalars under the keys of `step`; distillation and block loss have step's bits, the
        diffusion loss differs by the order of its B-term weighted sum.  Host tensors take `step` itself."""
        if not noisy_latents.is_cuda:
            out = self.step(noisy_latents, timesteps, encoder_hidden_states, target)
            return {k: out[k].detach() for k in VAL_KEYS}
        full_pred = self.teacher(noisy_latents, timesteps, encoder_hidden_states).sample
        model_pred = self.student(noisy_latents, timesteps, encoder_hidden_states).sample
        w = _min_snr_weights(self.cfg, self.schedule, timesteps)
        o = _unet_loss_terms(self.cfg, model_pred, target, full_pred, self.acts_s, self.acts_t, w, self._group_coef(),
                             blocks=self.cfg.block_weight > 0).run()
        return {"loss": o[3], "diff_loss": o[0], "distillation_loss": o[2], "block_loss": o[1]}

    def validate(self, batches, reduce: bool = True) -> Dict[str, float]:
        """FineTuner.validate (trainer.py:1767-1818): the four validation means over `batches` as Python floats; one host sync
        at the end and, under an initialised process group, one all-reduce ("mean" over the ranks).  Reference quirk, kept: an
        empty batch is skipped but still counts in the divisor (see _validate_eager)."""
        return _validate_eager(lambda b: self.eval_step(b["noisy_latents"], b["timesteps"], b["encoder_hidden_states"], b["target"]),
                               batches, VAL_KEYS, reduce)

    def _packed_reducer(self):
        """Under a PackedTrainer the gradients the optimizer consumes are those of the PACKED tensors (the diffusers-layout
        parameters receive none): the data-parallel exchange must run over them, or the ranks silently diverge."""
        pk = self.student.__dict__.get("_pk")
        if self._dp and pk is not None and not self._reducer_packed:
            assert pk.parameters(), "FineTunerStep(data_parallel=True): call PackedTrainer.materialize() before the first step"
            if self.reducer is not None:
                self.reducer.remove()
            self.reducer = BucketedGradReducer(pk.parameters(), self._bucket_bytes, mode=self._reduce_mode)
            self._reducer_packed = True

    def train_step(self, optimizer, batch: dict):
        self._packed_reducer()
        optimizer.zero_grad(set_to_none=True)
        out = self.step(batch["noisy_latents"], batch["timesteps"], batch["encoder_hidden_states"], batch["target"])
        out["loss"].backward()
        if self.reducer is not None:
            self.reducer.finish()
        optimizer.step()
        pk = self.student.__dict__.get("_pk")
        if pk is not None:
            pk.refresh_()                     # packed masters (packed_train.py): one multi-tensor cast, no re-pack
        else:
            # the bf16 packs follow the fp32 masters through the parameters' version counters (unet._PlanCache): the next
            # forward re-packs what the optimizer changed; dropping the old packs now only returns their memory earlier
            self.student.invalidate_plans()
        return out


class GraphedFineTunerStep(FineTunerStep):
    """Expert fine-tuning with the trainable state in the kernels' layout (packed_train.PackedTrainer): dense teacher forward,
    pruned student forward, the three loss terms (trainer.py:1730-1763) and the backward replayed from THREE HIP graphs --
    teacher (side stream, own pool) next to the student's forward, then losses + backward -- followed by the batched weight
    gradients, the deferred folds, AdamW (trainer.py:1529-1540) and the refresh of the bf16 operands as a handful of launches
    (ops.WgradBatch, ops.FoldBatch, packed_train.PackedAdamW).  The ~10^4 launches of the eager step (which is host-bound)
    cost their device time only.  Same numbers as FineTunerStep on packed masters with the same optimizer, bit for bit
    (tests/test_finetune_gpu.py).

    accumulation_steps=N > 1 (gradient_accumulation_steps of configs/finetuning/sd-2-1_cc3m.yaml): every train_step call is one
    micro-batch through the same graphs; calls i = 0 .. N-1 form a window whose gradients are summed on the device
    (ops.grad_accumulate: STORE, ADD .., FINAL), and the gradient exchange, AdamW and the operand refresh run once, on the call
    that closes the window, on the mean over the window (and the ranks).  Arena slot 0 carries the sum of the window's losses,
    so one non-finite micro-batch skips the whole window on every rank.  The window position lives in this object only:
    PackedAdamW.state_dict() and PackedTrainer.export_() hold parameters, moments and the count of applied steps, so a
    checkpoint taken in the middle of a window drops the micro-batches accumulated so far (``accum_index`` tells where a
    window stands: save at 0).
    lr_warmup_steps=W > 0: `constant_with_warmup` over W optimizer steps (PackedAdamW(warmup_steps=W)).
    lr_scheduler=NAME (training.optim.lr_scheduler of the recipes: constant, constant_with_warmup, linear, cosine,
    cosine_with_restarts, polynomial) with max_train_steps=T, lr_num_cycles, lr_power: the rate follows that curve over the applied
    optimizer steps, W = lr_warmup_steps (packed_train.LrSchedule; one small launch in front of AdamW on the call that closes a
    window).  log_lr=True: the dict gains "lr", the rate that step ran at (device scalar; None inside an open window).
    ema=True or a dict of PackedEMA's arguments: an exponential moving average of the packed state (`use_ema` of the reference's
    interface), one launch behind AdamW on the call that closes a window, under the same gate; validate(use_ema=True),
    export_ema_() and save_ema_pretrained() read it through a swap of masters and averages.
    max_grad_norm=X: clip_grad_norm_(X) on the device in front of AdamW (ops.GradNorm: two launches); the dict gains
    "grad_norm" and a window whose norm is not finite is skipped like one whose loss is not; log_grad_norm=True: the norm alone.
    use_8bit_adam=True: both AdamW moments as block-wise 8-bit codes (PackedAdamW(optim_bits=8), csrc/optim8.hip).
    short_batches=True: capture(batch) fixes the LARGEST batch; train_step then takes any 0 <= n <= B samples (or a full batch
    with a "valid" vector) through the same graphs: the losses are means over the samples present, the dict gains "n_valid" and
    "skipped", and an empty batch touches nothing."""

    def __init__(self, student, teacher, cfg: Optional[FinetuneLossConfig] = None, schedule: Optional[NoiseSchedule] = None,
                 lr: float = 1e-5, weight_decay: float = 1e-2, betas=(0.9, 0.999), eps: float = 1e-8,
                 data_parallel: bool = False, bucket_bytes: int = 256 << 20, reduce_mode: str = "rs_ag", nan_guard: bool = True,
                 accumulation_steps: int = 1, lr_warmup_steps: int = 0, ema=None, max_grad_norm: Optional[float] = None,
                 log_grad_norm: bool = False, use_8bit_adam: bool = False, short_batches: bool = False,
                 lr_scheduler: Optional[str] = None, max_train_steps: Optional[int] = None, lr_num_cycles=None, lr_power: float = 1.0,
                 log_lr: bool = False):
        assert int(accumulation_steps) >= 1 and lr_warmup_steps >= 0
        # lr_scheduler: the curve of get_scheduler(name, num_warmup_steps=lr_warmup_steps, num_training_steps=max_train_steps), both in
        # optimizer steps, evaluated on the device from the count of applied steps (PackedAdamW(lr_schedule=)).  None: nothing is
        # allocated or launched and lr_warmup_steps is the warm-up of PackedAdamW(warmup_steps=).  DESIGN 6y.
        self.lr_schedule = None
        if lr_scheduler is not None:
            from .packed_train import LrSchedule
            self.lr_schedule = LrSchedule(lr_scheduler, warmup_steps=lr_warmup_steps, training_steps=max_train_steps,
                                          num_cycles=lr_num_cycles, power=lr_power)
        assert not log_lr or self.lr_schedule is not None, "GraphedFineTunerStep: log_lr reads the device-side rate of an lr_scheduler"
        self.log_lr = bool(log_lr)
        super().__init__(student, teacher, cfg, schedule)       # (registers hooks: after everything that can refuse the arguments)
        # short_batches: the captured batch size is a MAXIMUM; train_step takes 0 <= n <= B samples (the loader drops samples
        # it cannot decode and ends every epoch on a short batch).  The loss terms become ONE autograd node over the fused
        # masked loss stage (ops.LossStage, csrc/loss_stage.hip) whose mean runs over the samples present; the rows behind them
        # are finite padding with loss weight, hence gradient, exactly zero.  False: nothing is allocated or launched and the
        # captured graphs are the ones without the argument.  DESIGN 6x.
        self.short_batches = bool(short_batches)
        # use_8bit_adam (training.optim.use_8bit_adam of the reference's configs): PackedAdamW(optim_bits=8) -- block-wise 8-bit
        # moments for the tensors of at least 4096 elements, a second launch for them; parameters, operands and gradients keep
        # their type and address, so everything else of the step is as without it.  DESIGN 6u.
        self.use_8bit_adam = bool(use_8bit_adam)
        # max_grad_norm X: clip_grad_norm_(X) of the diffusers training scripts, on the device, where AdamW reads the gradients
        # (after the FINAL accumulate and any exchange); log_grad_norm: the norm without a threshold.  Either adds two launches
        # (ops.GradNorm), a "grad_norm" entry to train_step's dict and the skip of a window whose norm is not finite.  Neither:
        # nothing is built and nothing launched.  DESIGN 6t.
        assert max_grad_norm is None or max_grad_norm > 0, "GraphedFineTunerStep: max_grad_norm"
        self.max_grad_norm, self.log_grad_norm = max_grad_norm, bool(log_grad_norm)
        # ema: None = no average (no allocation, no launch); True = packed_train.PackedEMA with its defaults; a dict = its keyword
        # arguments (decay, min_decay, update_after_step, use_ema_warmup, inv_gamma, power).  Built by capture() as self.ema.
        assert ema is None or ema is True or isinstance(ema, dict), "GraphedFineTunerStep: ema is None, True or a dict of PackedEMA's arguments"
        self._ema_kw, self.ema = (None if ema is None else ({} if ema is True else dict(ema))), None
        # accumulation_steps > 1: the gradients live in the arena (also without data_parallel) and one more fp32 tensor of its
        # size holds the running sum of the window; allocated by capture()
        self.accumulation_steps, self.lr_warmup_steps = int(accumulation_steps), lr_warmup_steps
        self._accum, self.accum_index = None, 0
        # data_parallel (one expert on several GPUs): the replayed graph and the batched weight-gradient launches
        # leave this rank's gradients in ONE contiguous arena; ArenaGradReducer sums it over the ranks in place, bucket by bucket
        # on a communication stream, and the optimizer follows bucket by bucket (the mean is its grad_scale)
        self._dp_graphed, self._bucket_bytes, self._reduce_mode = data_parallel, bucket_bytes, reduce_mode
        # nan_guard: a step whose loss is not finite leaves parameters, moments and the step count untouched (device-side:
        # AptpAdamWParams.gate_dev; reference: the batch skip of pdm/training/trainer.py:921-929)
        self.nan_guard = nan_guard
        self.defer_folds, self.direct_grads, self._folds = True, True, None
        self.defer_wgrads, self._wgrads = True, None
        self.overlap_teacher = os.environ.get("APTP_FT_OVERLAP_TEACHER", "1") != "0"   # teacher graph on a side stream next to the student's forward
        self.overlap_tail = os.environ.get("APTP_FT_OVERLAP_TAIL", "0") == "1"   # measured: 28.9 steps/s with, 29.9 without (HBM-bound tail next to the teacher: contention)
        from .packed_train import PackedTrainer
        self.trainer = PackedTrainer(student).attach()
        self.opt_kw = dict(lr=lr, weight_decay=weight_decay, betas=betas, eps=eps)
        self.optimizer = None
        self._cap = None
        self.stream_probe = []          # what graph_utils.concurrent_stream measured when it chose the teacher's / router's side streams
        self._val, self._val_running = {}, None      # forward-only validation graphs by batch size (capture_validation), their totals

    def capture(self, batch: dict, warmup_iters: int = 2, offload_masters: bool = False):
        """Build the packed trainable state, the three HIP graphs (teacher forward | student forward | losses + backward) for this
        batch geometry, and the one-launch AdamW over the gradients the backward graph and the batched launches leave behind."""
        dev = batch["noisy_latents"].device
        st = {k: batch[k].clone() for k in _BATCH_KEYS}
        if self.schedule.alphas_cumprod.device != dev:
            self.schedule.alphas_cumprod = self.schedule.alphas_cumprod.to(dev)
        st["snr_w"] = _min_snr_weights(self.cfg, self.schedule, st["timesteps"])
        if self.short_batches:
            st["valid"] = torch.ones(int(st["noisy_latents"].shape[0]), dtype=torch.float32, device=dev)
        self.trainer.materialize(st["noisy_latents"], st["timesteps"], st["encoder_hidden_states"])
        # the block-output hooks kept the materialising forward's autograd graph (and through it every AccumulateGrad node)
        # alive: drop it before the warm-up builds the graphs the capture will re-use
        self.acts_s.clear()
        self.acts_t.clear()
        if offload_masters:
            self.trainer.offload_masters_()
            torch.cuda.empty_cache()
        params = self.trainer.parameters()
        out = {}
        # direct-gradient mode (ops.GRAD_DIRECT): persistent gradient buffers written by the kernels / the deferred folds; nothing
        # to reset between steps -- every parameter's live region is overwritten by each backward
        direct = self.direct_grads
        if direct:
            self.trainer.ensure_grad_buffers(arena=self._dp_graphed or self.accumulation_steps > 1, world=_world())

        def teacher_fwd():
            # own split-K counters / scratch: this graph replays NEXT TO the previous step's optimizer tail (ops.scratch_domain)
            with torch.no_grad(), ops.scratch_domain("teacher"):
                st["snr_w"].copy_(_min_snr_weights(self.cfg, self.schedule, st["timesteps"]))      # (min-SNR weights: read by the loss terms only)
                fp = self.teacher(st["noisy_latents"], st["timesteps"], st["encoder_hidden_states"]).sample.detach()
            return fp, dict(self.acts_t)

        def student_fwd():
            if not direct:
                for p in params:
                    p.grad = None
            pred = self.student(st["noisy_latents"], st["timesteps"], st["encoder_hidden_states"]).sample
            return pred, dict(self.acts_s)

        def student_bwd(pred, student_acts, full_pred, teacher_acts):
            self.acts_s.clear()
            self.acts_s.update(student_acts)
            self.acts_t.clear()
            self.acts_t.update(teacher_acts)
            if self.short_batches:
                stage = self._loss_stage(pred, full_pred, st["snr_w"], st["target"], st["valid"])
                AG.loss_stage(stage).backward()
                o = stage.out                    # [diffusion, block, distillation, total, n]
                out.update(total=o[3], diff=o[0], dist=o[2], blk=o[1], n_valid=o[4], stage=stage)
                return
            total, diff, dist_l, blk = self._losses(pred, full_pred, st["snr_w"], st["target"])
            total.backward()
            out.update(total=total.detach(), diff=diff, dist=dist_l, blk=blk)

        def fwd_bwd():
            fp, ta = teacher_fwd()
            student_bwd(*student_fwd(), fp, ta)

        # warm-up (allocator, plan caches, autograd's stream anchors) runs forward + backward only: nothing to undo afterwards
        # (ops.LAUNCH_LOG is filled by the last eager iteration, never by the captures: _launch_log_off)
        user_log, log0 = ops.LAUNCH_LOG, None
        ops.GRAD_DIRECT = direct
        try:
            with warmup_stream():
                for i in range(max(1, warmup_iters)):
                    if user_log is not None:
                        log0 = len(user_log)
                    fwd_bwd()
        finally:
            ops.GRAD_DIRECT = False
        launch_log = None if user_log is None else user_log[log0:]
        # TWO graphs.  The teacher's forward reads no trainable state, so step i+1's teacher pass does not have to wait for step
        # i's optimizer: it is its own graph (own memory pool: it replays NEXT TO the tail of the previous step, whose kernels
        # still read tensors of the student graph's pool), and train_step() issues the tail -- batched weight gradients, folds,
        # AdamW, operand refresh: 6.7 of 33.8 ms, HBM-bound for the most part -- on a second stream.
        g_teacher, graph, g_bwd = new_graph(), new_graph(), new_graph()
        # The slab folds of the split weight gradients (and the chunk folds of the norm-affine gradients) are only RECORDED while
        # the backward is captured and run as ONE launch behind every replay (ops.FoldBatch: 357 launches of ~8 us otherwise):
        # nothing reads a parameter gradient before the optimizer.
        # Likewise the stride-1 weight gradients: recorded, then ONE launch per filter size behind the replay (ops.WgradBatch),
        # with pixel slices sized for the batch instead of for a chip-filling launch each (most weights: no slabs, no fold).
        try:
            with _launch_log_off():
                with torch.cuda.graph(g_teacher):
                    full_pred, teacher_acts = teacher_fwd()
                ops.FOLD_DEFER = [] if (self.defer_folds and direct) else None
                ops.WGRAD_DEFER = [] if (self.defer_wgrads and self.defer_folds and direct) else None
                ops.GRAD_DIRECT = direct
                # the student's forward does not read the teacher (only the loss terms do): its own graph, replayed NEXT TO the
                # teacher graph on the side stream; the loss + backward graph joins the two (same pool as the forward: replayed in
                # capture order)
                with torch.cuda.graph(graph):
                    pred, student_acts = student_fwd()
                with torch.cuda.graph(g_bwd, pool=graph.pool()):
                    student_bwd(pred, student_acts, full_pred, teacher_acts)
            folds, wgrads = ops.FOLD_DEFER, ops.WGRAD_DEFER
        finally:
            ops.FOLD_DEFER = None
            ops.WGRAD_DEFER = None
            ops.GRAD_DIRECT = False
        self._wgrads = ops.WgradBatch(wgrads) if wgrads else None
        self._folds = ops.FoldBatch(folds) if folds else None
        # The optimizer is ONE launch over every trainable tensor and writes the bf16 operands in the same pass
        # (packed_train.PackedAdamW, csrc/optim.hip); its table holds the addresses of the gradients the captured backward
        # left in `.grad`, which every replay re-writes in place.  It runs right behind the graph, followed by the one-launch
        # refresh of the data-gradient operands: three launches, no host work worth capturing.
        from .packed_train import PackedAdamW
        group_of = None
        if self._dp_graphed:
            assert direct, "the data-parallel graphed step exchanges the gradient arena of the direct-gradient mode"
            self.reducer = ArenaGradReducer(self.trainer.grad_arena, self._bucket_bytes, mode=self._reduce_mode)
            off = {id(p_): o for p_, o in zip(self.trainer.parameters(), self.trainer.grad_offsets)}
            group_of = lambda p_: self.reducer.bucket_of(off[id(p_)], p_.numel())          # noqa: E731
        self.optimizer = PackedAdamW(self.trainer, lr=self.opt_kw["lr"], betas=self.opt_kw["betas"], eps=self.opt_kw["eps"],
                                     weight_decay=self.opt_kw["weight_decay"], group_of=group_of,
                                     warmup_steps=0 if self.lr_schedule is not None else self.lr_warmup_steps,
                                     max_grad_norm=self.max_grad_norm, log_grad_norm=self.log_grad_norm,
                                     optim_bits=8 if self.use_8bit_adam else 32, lr_schedule=self.lr_schedule)
        if self._ema_kw is not None:
            from .packed_train import PackedEMA
            self.ema = PackedEMA(self.trainer, self.optimizer, **self._ema_kw)
        if self.accumulation_steps > 1:
            assert direct, "gradient accumulation sums the gradient arena of the direct-gradient mode"
            self._accum, self.accum_index = torch.empty_like(self.trainer.grad_arena), 0      # (STORE writes it before any read)
        self._cap = dict(st=st, graph=graph, g_bwd=g_bwd, g_teacher=g_teacher, full_pred=full_pred, teacher_acts=teacher_acts,
                         pred=pred, student_acts=student_acts, side=concurrent_stream(log=self.stream_probe),
                         tail_stream=torch.cuda.Stream(), ev_bwd=torch.cuda.Event(), ev_tail=None, launch_log=launch_log, **out)
        self.trainer.sync = self.finish          # (export_ / state_dict read the parameters: after the pending optimizer tail)
        return self

    def finish(self):
        """make the current stream wait for the optimizer tail of the last train_step (it runs on its own stream so that the next
        step's teacher forward overlaps it); call before reading parameters on the current stream -- PackedTrainer.export_ does"""
        cap = self._cap
        if cap is not None and cap.get("ev_tail") is not None:
            torch.cuda.current_stream().wait_event(cap["ev_tail"])

    MAX_VALIDATION_GEOMETRIES = 2      # the full validation batch and the ragged last one

    def capture_validation(self, batch: dict, warmup_iters: int = 1):
        """Forward-only HIP graphs of one validation batch of this geometry: teacher forward (side stream, own pool, own scratch
        domain) next to the student forward, then ONE loss-terms call that also adds the batch to the running totals.  The student
        graph reads the packed bf16 operands, which PackedAdamW rewrites IN PLACE after every optimizer step: the addresses the
        capture baked in stay the model, so one capture serves the whole run.  Graphs are kept per batch size, at most
        MAX_VALIDATION_GEOMETRIES of them; the least recently used one goes.  Call after capture()."""
        assert self._cap is not None, "call capture(batch) first: validation reads the packed state it builds"
        self.finish()
        B = int(batch["noisy_latents"].shape[0])
        dev = batch["noisy_latents"].device
        st = {k: batch[k].clone() for k in _BATCH_KEYS}
        st["snr_w"] = _min_snr_weights(self.cfg, self.schedule, st["timesteps"])
        if self._val_running is None:
            self._val_running = torch.zeros(len(VAL_KEYS) + 1, dtype=torch.float32, device=dev)      # [diff, block, distill, loss, batches]

        def teacher_fwd():
            with torch.no_grad(), ops.scratch_domain("val_teacher"):
                st["snr_w"].copy_(_min_snr_weights(self.cfg, self.schedule, st["timesteps"]))
                fp = self.teacher(st["noisy_latents"], st["timesteps"], st["encoder_hidden_states"]).sample
            return fp, dict(self.acts_t)

        def student_fwd():
            with torch.no_grad():
                pred = self.student(st["noisy_latents"], st["timesteps"], st["encoder_hidden_states"]).sample
            return pred, dict(self.acts_s)

        def losses(pred, student_acts, full_pred, teacher_acts, running):
            with torch.no_grad():
                lt = _unet_loss_terms(self.cfg, pred, st["target"], full_pred, student_acts, teacher_acts, st["snr_w"],
                                      self._group_coef(), blocks=self.cfg.block_weight > 0, running=running)
                lt.run()
            return lt

        try:
            with _launch_log_off():
                with warmup_stream():
                    for _ in range(max(1, warmup_iters)):          # allocator and plan caches of this geometry; totals untouched
                        fp, ta = teacher_fwd()
                        losses(*student_fwd(), fp, ta, None)
                g_teacher, g_student, g_loss = new_graph(), new_graph(), new_graph()
                with torch.cuda.graph(g_teacher):
                    full_pred, teacher_acts = teacher_fwd()
                with torch.cuda.graph(g_student):
                    pred, student_acts = student_fwd()
                with torch.cuda.graph(g_loss, pool=g_student.pool()):
                    lt = losses(pred, student_acts, full_pred, teacher_acts, self._val_running)
        finally:
            self.acts_s.clear()
            self.acts_t.clear()
        self._val.pop(B, None)
        while len(self._val) >= self.MAX_VALIDATION_GEOMETRIES:
            self._val.pop(next(iter(self._val)))               # (dicts keep insertion order: the first key is the least recently used)
        self._val[B] = dict(st=st, g_teacher=g_teacher, g_student=g_student, g_loss=g_loss, lt=lt, full_pred=full_pred,
                            teacher_acts=teacher_acts, pred=pred, student_acts=student_acts, side=self._cap["side"])
        return self

    def _replay_validation(self, batch: dict):
        """one validation batch through the graphs of its batch size (captured on first use); adds it to the running totals"""
        B = int(batch["noisy_latents"].shape[0])
        if B not in self._val:
            self.capture_validation(batch)
        cap = self._val[B] = self._val.pop(B)                 # most recently used: to the end
        _stage_batch(cap["st"], batch)
        main, side = torch.cuda.current_stream(), cap["side"]
        side.wait_stream(main)
        with torch.cuda.stream(side):
            cap["g_teacher"].replay()
        cap["g_student"].replay()
        main.wait_stream(side)
        cap["g_loss"].replay()
        return cap["lt"].out

    def _ema_applied(self, use_ema: bool):
        """context of a validation pass: with use_ema the packed state holds the average inside (PackedEMA.applied: one swap
        launch in, one out in a `finally`).  The validation graphs read pw.w, the fp32 biases and the affines at fixed addresses,
        so the SAME graphs score the average: nothing is re-captured."""
        import contextlib
        if not use_ema:
            return contextlib.nullcontext()
        assert self.ema is not None, "use_ema=True needs GraphedFineTunerStep(ema=...) and capture()"
        self.finish()
        return self.ema.applied()

    def eval_step_graphed(self, batch: dict, use_ema: bool = False):
        """the four losses of one batch from the validation graphs, as clones of the graphs' static outputs (what eval_step
        returns, replayed); the running totals of validate() take this batch too.  use_ema: of the averaged weights."""
        self.finish()
        with self._ema_applied(use_ema):
            o = self._replay_validation(batch).clone()
        return {"loss": o[3], "diff_loss": o[0], "distillation_loss": o[2], "block_loss": o[1]}

    def validate(self, batches, reduce: bool = True, use_ema: bool = False) -> Dict[str, float]:
        """FineTuner.validate (trainer.py:1767-1818) from the validation graphs: finish() the pending optimizer tail, zero the
        device totals, replay every batch (staged copies + three graph replays, no host wait), then ONE host sync; under an
        initialised process group one all-reduce of the totals ("mean" over the ranks).  Returns the four means as Python floats.
        Reference quirk, kept (trainer.py:1788-1800): a batch without samples is skipped but the divisor is len(batches), so every
        empty batch pulls the means towards zero.  Forward-only: parameters, moments, step count, the gradient arena, the
        accumulator and accum_index are left as they are, also in the middle of an accumulation window.
        use_ema=True: the means of the averaged weights (self.ema): one swap launch, the same pass over the same graphs, one swap
        back; the trained state returns bit for bit."""
        with self._ema_applied(use_ema):
            return self._validate(batches, reduce)

    def _validate(self, batches, reduce: bool) -> Dict[str, float]:
        batches = list(batches)
        self.finish()
        if not batches:
            return {k: 0.0 for k in VAL_KEYS}
        if self._val_running is not None:
            self._val_running.zero_()
        for batch in batches:
            if batch["noisy_latents"].numel() == 0:
                continue
            self._replay_validation(batch)
        if self._val_running is None:                        # nothing but empty batches
            return {k: 0.0 for k in VAL_KEYS}
        diff, blk, dist_l, loss = reduce_validation_totals(self._val_running[:4].clone(), reduce).tolist()
        n = len(batches)
        return {"loss": loss / n, "diff_loss": diff / n, "distillation_loss": dist_l / n, "block_loss": blk / n}

    def export_ema_(self):
        """write the AVERAGED weights into the diffusers-named parameters of the student and return it: PackedTrainer.export_()
        under PackedEMA.applied().  The packed state is back at the trained values on return (the second swap); the model's
        diffusers-named tensors hold the average until the next ``trainer.export_()`` -- which ``model.state_dict()`` runs itself
        under an attached trainer, so read the tensors through ``named_parameters()``, or save with save_ema_pretrained."""
        assert self.ema is not None, "export_ema_ needs GraphedFineTunerStep(ema=...) and capture()"
        self.finish()
        with self.ema.applied():
            model = self.trainer.export_()
        return model

    def save_ema_pretrained(self, root: str, subfolder: str = "unet_ema", arch_vector=None) -> str:
        """``<root>/unet_ema`` in the layout of checkpoint.save_pretrained (arch_vector.pt beside it, as for `unet`) from the
        averaged weights.  Written while the packed state is swapped: save_pretrained reads ``model.state_dict()``, which exports
        the packed state -- the average, then.  Afterwards the packed state and the diffusers-named tensors are the trained ones."""
        from . import checkpoint
        assert self.ema is not None, "save_ema_pretrained needs GraphedFineTunerStep(ema=...) and capture()"
        self.finish()
        try:
            with self.ema.applied():
                return checkpoint.save_pretrained(self.student, root, subfolder=subfolder, arch_vector=arch_vector)
        finally:
            self.trainer.export_()

    def validation_graph_nodes(self):
        """nodes of the validation graphs by batch size, for those captured while graph_utils.KEEP_GRAPHS was set"""
        return {B: {"teacher": node_count(c["g_teacher"]), "student_fwd": node_count(c["g_student"]), "losses": node_count(c["g_loss"])}
                for B, c in self._val.items()}

    def graph_nodes(self):
        """nodes of the captured teacher + student forward / backward graph, when it was kept (graph_utils.KEEP_GRAPHS)"""
        if self._cap is None:
            return None
        n = {"teacher": node_count(self._cap["g_teacher"]), "student_fwd": node_count(self._cap["graph"]),
             "student_bwd": node_count(self._cap["g_bwd"])}
        if self._wgrads is not None:
            n["batched_wgrad_launches"] = self._wgrads.launches()
        if self._folds is not None:
            n["deferred_folds_launch"] = 1
        return n

    def train_step(self, optimizer=None, batch: Optional[dict] = None):
        """one replayed step on `batch` (same shapes as the captured one); `optimizer` is ignored: the fused AdamW built at
        capture time is part of the graph"""
        cap = self._cap
        assert cap is not None, "call capture(batch) first"
        if self.ema is not None and self.ema.swapped:
            raise RuntimeError("GraphedFineTunerStep.train_step: the masters hold the EMA (swap_() back first): a step would train it")
        if self.short_batches:
            if _stage_short_batch(cap["st"], batch, self._dp_graphed) == 0:
                # nothing to learn from: no replay, no accumulation, no optimizer; the window stays where it is
                zero = torch.zeros((), dtype=torch.float32, device=cap["st"]["valid"].device)
                return {"loss": zero, "diff_loss": zero.clone(), "distillation_loss": zero.clone(), "block_loss": zero.clone(),
                        "applied": False, "accum_index": self.accum_index, "n_valid": zero.clone(), "skipped": True,
                        **({"lr": None} if self.log_lr else {})}
        else:
            _stage_batch(cap["st"], batch)
        main = torch.cuda.current_stream()       # (the min-SNR weights are computed from the staged timesteps inside g_teacher)
        side = cap["side"] if self.overlap_teacher else main
        side.wait_stream(main)                   # (the batch copies above)
        with torch.cuda.stream(side):
            cap["g_teacher"].replay()            # reads no trainable state; own pool, own scratch domain: next to the student's forward
        if cap["ev_tail"] is not None:
            main.wait_event(cap["ev_tail"])      # parameters and operands of the previous step are in place
        cap["graph"].replay()                    # student forward
        main.wait_stream(side)                   # teacher outputs ready
        cap["g_bwd"].replay()                    # losses against the teacher + backward
        cap["ev_bwd"].record(main)
        tail = cap["tail_stream"] if self.overlap_tail else main
        with torch.cuda.stream(tail):
            tail.wait_event(cap["ev_bwd"])
            if self._wgrads is not None:
                self._wgrads.run()               # every stride-1 weight gradient of the backward: one launch per filter size
            if self._folds is not None:
                self._folds.run()                # every deferred slab / chunk fold of the backward: one launch
            N, idx = self.accumulation_steps, self.accum_index
            applied = idx == N - 1
            if N > 1:
                # one micro-batch of a window: its loss goes into arena slot 0 and the whole arena into the running sum; the
                # call that closes the window gets the sum back in the arena (FINAL), where the exchange and AdamW read
                arena = self.trainer.grad_arena
                arena[0:1].copy_(cap["total"].reshape(1))
                ops.grad_accumulate(self._accum, arena, "store" if idx == 0 else ("final" if applied else "add"))
                self.accum_index = 0 if applied else idx + 1
            if not applied:
                pass                             # no exchange, no AdamW, no operand refresh, no step count: the window is open
            elif self._dp_graphed and self.reducer is not None:
                # sum over the ranks in place, bucket by bucket on the communication stream; AdamW follows bucket by bucket with
                # grad_scale = 1 / world; arena slot 0 = sum of the ranks' losses = their common finite / non-finite verdict
                arena = self.trainer.grad_arena
                if N == 1:
                    arena[0:1].copy_(cap["total"].reshape(1))
                gate = arena[0:1] if self.nan_guard else None
                scale = 1.0 / (N * self.reducer.world)       # mean over the window's micro-batches and the ranks
                if self.optimizer.grad_norm is None:
                    self.reducer.exchange(lambda i: self.optimizer.step_group(i, gate, scale))
                    self.optimizer.finish_step(gate)
                else:
                    # the norm needs every bucket's sum: the whole exchange first, then the norm over the summed arena and ONE
                    # AdamW launch -- the bucket-by-bucket overlap of exchange and optimizer is what the clip costs here
                    self.reducer.exchange()
                    gate = self.optimizer.step(gate, grad_scale=scale)
            elif N > 1:
                # slot 0 = sum of the window's losses: one non-finite micro-batch skips the window
                gate = self.trainer.grad_arena[0:1] if self.nan_guard else None
                gate = self.optimizer.step(gate, grad_scale=1.0 / N)
            else:
                gate = cap["total"] if self.nan_guard else None
                gate = self.optimizer.step(gate)
            # (with a gradient norm, `gate` is now its verdict: finite norm and finite loss)
            grad_norm = self.optimizer.grad_norm.norm.clone() if (applied and self.optimizer.grad_norm is not None) else None
            lr_now = self.optimizer.lr_t.reshape(()).clone() if (applied and self.log_lr) else None
            if applied and self.ema is not None:
                # the average follows the optimizer on its stream, under its gate: one launch + the device-side count.  Local to
                # the rank in data-parallel mode (identical masters give identical averages: no collective)
                self.ema.step(gate)
            ev = cap["ev_tail"] or torch.cuda.Event()
            ev.record(tail)
            cap["ev_tail"] = ev
        # (clones: the graph's static outputs are overwritten by the next replay, and callers accumulate losses over steps)
        # the four losses are this micro-batch's; applied: this call ran the exchange and the optimizer (always, without
        # accumulation; whether the step took effect is the device-side NaN verdict); accum_index: its place in the window
        out = {"loss": cap["total"].clone(), "diff_loss": cap["diff"].clone(), "distillation_loss": cap["dist"].clone(),
               "block_loss": cap["blk"].clone(), "applied": applied, "accum_index": idx}
        if self.optimizer.grad_norm is not None:
            # the norm of the mean gradient the optimizer saw, before clipping (device scalar; NaN-free only when the window
            # was applied: compare ops.GradNorm.verdict); None inside an open window
            out["grad_norm"] = grad_norm
        if self.log_lr:
            # the rate the optimizer step of this call ran at -- or would have: a skipped window leaves it for the next one
            out["lr"] = lr_now
        if self.short_batches:
            out["n_valid"], out["skipped"] = cap["n_valid"].clone(), False          # (device scalar: the samples the losses average)
        return out
