"""Packed-parameter training of a pruned expert (BASELINE configs[4]; the counterpart of FineTuner's
optimizer state, pdm/training/trainer.py:1529-1540).

MI355X-first: during fine-tuning the trainable state lives in the KERNELS' layout.  For every contraction of the expert the
optimizer owns one fp32 tensor in the packed order ``[N][taps][cin_pad]`` -- compact: only the live rows / columns of the
architecture code -- and the bf16 operand the kernels read is its shadow:

  * the weight-gradient kernel (aptp_conv_wgrad) already produces ``[N][taps][C]``: the gradient needs no scatter into a
    full-shape OIHW tensor (three full-size passes per weight in the diffusers layout);
  * after ``optimizer.step()`` the shadows are refreshed with ONE multi-tensor cast (``torch._foreach_copy_``) plus one
    strided copy per data-gradient operand (the 180-degree-rotated transpose), instead of re-packing every weight from a
    diffusers-layout master (gather + permute + cast + pad: ~10 launches per weight, ~7,000 per step);
  * dead channels / heads / FF chunks / dropped blocks carry no optimizer state at all;
  * nothing in the step depends on the host, so forward + backward replay from HIP graphs and the optimizer + refresh follow as three launches
    (train_step.GraphedFineTunerStep).

Biases and norm affine parameters are compact fp32 tensors that the kernels read directly (no shadow).  The diffusers-named
full-shape parameters stay the checkpoint interface: ``export_()`` writes the packed values back into them.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import _lib
from . import autograd as AG
from . import ops


def _order_by_name(saved_names, own_names, who):
    """for every own name the position of the same name in a saved state (resume: whatever order the modules first ran in)"""
    pos = {n: i for i, n in enumerate(saved_names)}
    missing = [n for n in own_names if n not in pos]
    assert not missing and len(pos) == len(saved_names) == len(own_names), \
        f"{who}: the saved state belongs to another expert / tensor list (missing {missing[:3]}, " \
        f"{len(saved_names)} saved vs {len(own_names)} here)"
    return [pos[n] for n in own_names]


class _Gemm:
    """one contraction: packed fp32 master ``P`` [N, taps, cin_pad], optional compact bias ``Pb`` [N] (aliased by the pack),
    bf16 shadow ``pw`` (forward operand) and ``pwb`` (data-gradient operand, built on first use)"""

    def __init__(self, weight, bias: Optional[nn.Parameter], pw: ops.PackedWeight,
                 lo: Optional[torch.Tensor], li: Optional[torch.Tensor]):
        assert not pw.geglu and pw.ln_colsum is None and pw.Cin2 == 0, "packed training uses the plain packs of the ft path"
        # `weight` may be a tuple of equally shaped parameters that share the input (to_q | to_k | to_v of an attention block):
        # ONE contraction whose output rows are the parts' live rows back to back; `lo` / `li` apply to every part
        self.weights = tuple(weight) if isinstance(weight, (tuple, list)) else (weight,)
        assert bias is None or len(self.weights) == 1
        self.weight, self.bias, self.pw, self.lo, self.li = self.weights[0], bias, pw, lo, li
        dev = pw.w.device
        ws = []
        for wp in self.weights:
            w = wp.detach().to(device=dev, dtype=torch.float32)
            if w.dim() == 2:
                w = w[:, :, None, None]
            if lo is not None:
                w = w[lo.to(dev)]
            if li is not None:
                w = w[:, li.to(dev)]
            ws.append(w)
        self.n_part = ws[0].shape[0]
        w = torch.cat(ws, 0) if len(ws) > 1 else ws[0]
        self.n_live, self.c_live, self.KH, self.KW = w.shape
        assert self.n_live <= pw.N and self.c_live <= pw.Cin and (self.KH, self.KW) == (pw.KH, pw.KW)
        P = torch.zeros(pw.w.shape, dtype=torch.float32, device=dev)
        P[:self.n_live, :, :self.c_live] = w.permute(0, 2, 3, 1).reshape(self.n_live, self.KH * self.KW, self.c_live)
        self.P = nn.Parameter(P)
        self.Pb = None
        if pw.bias is not None:
            # the pack's fp32 bias becomes the trainable tensor, read directly by the kernels (a fresh tensor: an un-gathered
            # pack bias can alias the diffusers-layout master, whose storage and version counter must stay untouched)
            self.Pb = nn.Parameter(pw.bias.detach().clone())
            pw.bias = self.Pb.data
        pw.w.copy_(P)                                  # shadow = bf16(master), exactly what a re-pack would give
        self.pwb: Optional[ops.PackedWeight] = None

    def get_bwd(self) -> ops.PackedWeight:
        if self.pwb is None:
            w4 = self.P.detach()[:, :, :self.pw.Cin].reshape(self.pw.N, self.KH, self.KW, self.pw.Cin).permute(0, 3, 1, 2)
            self.pwb = ops.pack_weight_dgrad(w4, device=self.P.device)
        return self.pwb

    def refresh_bwd_(self):
        if self.pwb is not None:
            ops.pack_dgrad_from_packed(self.pw, self.pwb)          # one tiled transpose (was: flip + strided copy)

    def parts(self):
        """(parameter, row range of P / P.grad it owns) for every weight of the contraction"""
        return [(wp, slice(i * self.n_part, (i + 1) * self.n_part)) for i, wp in enumerate(self.weights)]

    @torch.no_grad()
    def export_(self):
        for wp, rows in self.parts():
            g = self.P.detach()[rows, :, :self.c_live].permute(0, 2, 1).reshape(self.n_part, self.c_live, self.KH, self.KW)
            full = wp.data
            g = g.to(device=full.device, dtype=full.dtype)
            if full.dim() == 2:
                g = g.reshape(self.n_part, self.c_live)
            ro = self.lo.to(full.device) if self.lo is not None else torch.arange(full.shape[0], device=full.device)
            ci = self.li.to(full.device) if self.li is not None else torch.arange(full.shape[1], device=full.device)
            full[ro[:, None], ci[None, :]] = g
        if self.bias is not None and self.Pb is not None:
            b = self.Pb.detach()[:self.n_live].to(device=self.bias.device, dtype=self.bias.dtype)
            if self.lo is not None:
                self.bias.data[self.lo.to(self.bias.device)] = b
            else:
                self.bias.data.copy_(b)


class _Affine:
    """compact fp32 (gamma, beta) of a GroupNorm / LayerNorm, read directly by the kernels"""

    def __init__(self, gamma_p: nn.Parameter, beta_p: nn.Parameter, gamma: torch.Tensor, beta: torch.Tensor,
                 live: Optional[torch.Tensor]):
        self.gamma_p, self.beta_p, self.live = gamma_p, beta_p, live
        self.Pg, self.Pb = nn.Parameter(gamma.detach().float().clone()), nn.Parameter(beta.detach().float().clone())

    @torch.no_grad()
    def export_(self):
        for P, full in ((self.Pg, self.gamma_p), (self.Pb, self.beta_p)):
            v = P.detach().to(device=full.device, dtype=full.dtype)
            if self.live is not None:
                full.data[self.live.to(full.device)] = v
            else:
                full.data.copy_(v)


class PackedTrainer:
    """Registry of the packed trainable state of one expert.  ``attach`` switches the model's fine-tuning forward to it;
    entries are created the first time a module runs (call ``materialize`` with one batch before building the optimizer)."""

    def __init__(self, model):
        self.model = model
        self.gemms: Dict[int, _Gemm] = {}
        self.affines: Dict[int, _Affine] = {}

    def attach(self):
        for m in self.model.modules():
            m.__dict__["_pk"] = self
        return self

    def detach(self):
        for m in self.model.modules():
            m.__dict__.pop("_pk", None)

    # ---- called by the model's fine-tuning forward in place of AG.conv_w / AG.GroupNormWFn / AG.LayerNormWFn -----------------
    def conv(self, x, weight, bias, pw, get_bwd, stride=1, pad=None, ups=0, out_f32=False, live_out=None, live_in=None,
             residual=None, rowbias=None):
        key = id(weight[0]) if isinstance(weight, (tuple, list)) else id(weight)
        e = self.gemms.get(key)
        if e is None:
            e = self.gemms[key] = _Gemm(weight, bias, pw, live_out, live_in)
        assert e.pw is pw, "the plan's packs were rebuilt under a packed trainer (call PackedTrainer after the last set_structure)"
        return AG.conv_p(x, e.P, e.Pb, e.pw, e.get_bwd, stride=stride, pad=pad, ups=ups, out_f32=out_f32, residual=residual,
                         rowbias=rowbias)

    def groupnorm(self, x, gamma_p, beta_p, gamma, beta, groups, eps, silu, C, live, fork=False):
        a = self.affines.get(id(gamma_p))
        if a is None:
            a = self.affines[id(gamma_p)] = _Affine(gamma_p, beta_p, gamma, beta, live)
        return AG.GroupNormWFn.apply(x, a.Pg, a.Pb, a.Pg, a.Pb, groups, eps, silu, C, None, fork)

    def layernorm(self, x, gamma_p, beta_p, gamma, beta, eps, fork=False):
        a = self.affines.get(id(gamma_p))
        if a is None:
            a = self.affines[id(gamma_p)] = _Affine(gamma_p, beta_p, gamma, beta, None)
        return AG.LayerNormWFn.apply(x, a.Pg, a.Pb, a.Pg, a.Pb, eps, fork)

    # ---- optimizer-facing API ---------------------------------------------------------------------------------------------------
    def materialize(self, *forward_args, **forward_kwargs):
        """one forward + backward (on a zero loss scale) so that every entry, including the data-gradient operands, exists.
        Runs on a side stream: autograd anchors a parameter's AccumulateGrad node to the stream of its first backward and
        re-uses the node while any graph that reached it is alive; a node anchored to the legacy default stream cannot take
        part in a later HIP-graph capture (hipStreamEndCapture dies on the cross-stream edge)."""
        if torch.cuda.is_available():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                out = self.model(*forward_args, **forward_kwargs).sample
                (out.float().sum() * 0.0).backward()
                del out
            torch.cuda.current_stream().wait_stream(side)
        else:
            out = self.model(*forward_args, **forward_kwargs).sample
            (out.float().sum() * 0.0).backward()
            del out
        for p in self.parameters():
            p.grad = None
        return self

    def parameters(self) -> List[nn.Parameter]:
        ps: List[nn.Parameter] = []
        for e in self.gemms.values():
            ps.append(e.P)
            if e.Pb is not None:
                ps.append(e.Pb)
        for a in self.affines.values():
            ps += [a.Pg, a.Pb]
        return ps

    def entries(self):
        """(fp32 master, bf16 shadow or None) of every packed tensor, in the order of parameters(): what the table-driven passes
        (PackedAdamW, PackedEMA) walk.  They call it, and _sync, as PackedTrainer.entries(trainer): anything with ``gemms`` and
        ``affines`` serves as a trainer"""
        out = []
        for e in self.gemms.values():
            out.append((e.P, e.pw.w))
            if e.Pb is not None:
                out.append((e.Pb, None))
        for a in self.affines.values():
            out += [(a.Pg, None), (a.Pb, None)]
        return out

    def _sync(self):
        """wait for a pending optimizer tail (a graphed step runs it on its own stream and installs ``sync``) before the packed
        state is read or rewritten from the current stream"""
        sync = getattr(self, "sync", None)
        if sync is not None:
            sync()

    @torch.no_grad()
    def ensure_grad_buffers(self, arena: bool = False, world: int = 1):
        """persistent, zero-initialised .grad for every packed tensor (direct-gradient mode, ops.GRAD_DIRECT): the kernels write
        the live region of each buffer every step and never touch the pad columns.
        arena=True: all of them are views into ONE contiguous fp32 buffer (``self.grad_arena``; ``self.grad_offsets`` = element
        offset per parameter, in self.parameters() order), laid out in REVERSE registration order -- the order a backward
        produces gradients in -- with 256-byte aligned views; slot 0 (the first 64 elements) is reserved for the step's loss
        (train_step.ArenaGradReducer: the data-parallel exchange then runs in place on contiguous ranges, and its sum of the losses
        is the ranks' common NaN verdict); the total is padded to a multiple of 64 * world elements (equal shards)."""
        ps = self.parameters()
        if not arena:
            for p in ps:
                if p.grad is None or p.grad.shape != p.shape:
                    p.grad = torch.zeros_like(p)
            return self
        if getattr(self, "grad_arena", None) is not None and len(self.grad_offsets) == len(ps) and self._arena_world == world:
            return self
        A = 64
        offs, off = [0] * len(ps), A                    # [0, 64): loss slot
        for i in reversed(range(len(ps))):
            offs[i] = off
            off += (ps[i].numel() + A - 1) // A * A
        q = A * max(1, world)
        total = (off + q - 1) // q * q
        buf = torch.zeros(total, dtype=torch.float32, device=ps[0].device)
        for p, o in zip(ps, offs):
            assert p.dtype == torch.float32 and p.is_contiguous()
            p.grad = buf[o:o + p.numel()].view_as(p)
        self.grad_arena, self.grad_offsets, self._arena_world = buf, offs, world
        return self

    def named_parameters(self):
        """(stable name, packed tensor) pairs: the diffusers name of the parameter an entry was packed from + the kind of the
        packed tensor, so optimizer state can be matched by NAME on resume (the registry's own order is the first-run order
        of the modules)"""
        names = {id(p): n for n, p in self.model.named_parameters()}
        out = []
        for e in self.gemms.values():
            base = names.get(id(e.weight), f"<unnamed weight {tuple(e.weight.shape)}>")
            for wp in e.weights[1:]:                  # a fused contraction: "...attn1.to_q.weight+to_k.weight+to_v.weight"
                base += "+" + ".".join(names.get(id(wp), "?").split(".")[-2:])
            out.append((base + "::packed", e.P))
            if e.Pb is not None:
                out.append((base + "::packed_bias", e.Pb))
        for a in self.affines.values():
            base = names.get(id(a.gamma_p), f"<unnamed affine {tuple(a.gamma_p.shape)}>")
            out += [(base + "::gamma", a.Pg), (base + "::beta", a.Pb)]
        return out

    def n_trainable(self) -> int:
        return sum(p.numel() for p in self.parameters())

    @torch.no_grad()
    def offload_masters_(self):
        """Move the diffusers-layout masters of the model to host memory (they are only the checkpoint interface while the
        packed state trains; ``export_`` writes into them wherever they live): -3.5 GB of HBM for an SD-2.1 expert."""
        for p in self.model.parameters():
            if p.device.type != "cpu":
                p.data = p.data.cpu()
        return self

    @torch.no_grad()
    def refresh_(self, shadows_done: bool = False):
        """shadows <- masters: one multi-tensor cast for the forward operands (skipped when the optimizer wrote them:
        PackedAdamW), ONE launch for all data-gradient operands (ops.PackDgradBatch: a table of the weights in device memory,
        rebuilt when an operand appears or moves)"""
        es = list(self.gemms.values())
        if not shadows_done:
            torch._foreach_copy_([e.pw.w for e in es], [e.P.detach() for e in es])
        pairs = [(e.pw, e.pwb) for e in es if e.pwb is not None]
        if not pairs:
            return
        key = tuple((pw.w.data_ptr(), pwb.w.data_ptr()) for pw, pwb in pairs)
        batch = self.__dict__.get("_dgrad_batch")
        if batch is None or batch.key != key:
            if torch.cuda.is_current_stream_capturing():
                # (the table is uploaded with a host->device copy: never while capturing; GraphedFineTunerStep's warm-up
                # iterations run first, so this only happens when a new operand shows up mid-capture)
                for e in es:
                    e.refresh_bwd_()
                return
            batch = self._dgrad_batch = ops.PackDgradBatch(pairs)
        batch.run()

    @torch.no_grad()
    def export_(self):
        """write the packed values back into the diffusers-named full-shape parameters (checkpoint interface)"""
        self._sync()
        for e in self.gemms.values():
            e.export_()
        for a in self.affines.values():
            a.export_()
        return self.model


ADAM8_BLOCK = 256           # elements per quantisation block of the 8-bit state (csrc/optim8.hip)
ADAM8_MIN_SIZE = 4096       # tensors below this keep fp32 moments: bitsandbytes' rule, and one workgroup of the kernel


def adam8_code_map(signed: bool) -> torch.Tensor:
    """The 256 ascending fp32 values a code of the 8-bit AdamW state stands for (times its block's absmax): the block-wise
    "dynamic" map in its published construction -- per decade i = 0..6 the midpoints of 2^i (signed; 2^(i+1) unsigned) equal
    steps of [0.1, 1] times 10^(i-6), with both signs for the signed map, plus 0 and 1.  Built in fp64, rounded to fp32, sorted.
    tests/adamw8_model.py is the definition; DESIGN 6u."""
    vals = [0.0, 1.0]
    for i in range(7):
        k = 2 ** i if signed else 2 ** (i + 1)
        step = (1.0 - 0.1) / k
        edges = [0.1 + j * step for j in range(k)] + [1.0]
        for a, b in zip(edges[:-1], edges[1:]):
            mid = (a + b) / 2.0 * 10.0 ** (i - 6)
            vals += [mid, -mid] if signed else [mid]
    out = torch.tensor(vals, dtype=torch.float64).to(torch.float32).sort().values
    assert out.numel() == 256
    return out


def adam8_uses_8bit(numel: int, optim_bits: int = 8, min_8bit_size: int = ADAM8_MIN_SIZE) -> bool:
    """the partition rule of PackedAdamW(optim_bits=8): a tensor of at least min_8bit_size elements keeps 8-bit moments"""
    return optim_bits == 8 and int(numel) >= int(min_8bit_size)


def adam_state_bytes(sizes, optim_bits: int = 32, min_8bit_size: int = ADAM8_MIN_SIZE) -> int:
    """bytes of both moments of tensors of these sizes, the scales of the 8-bit ones included (fp32: 8 B per element; 8-bit:
    2 B per element + 8 B per block of 256)"""
    total = 0
    for n in sizes:
        n = int(n)
        total += 2 * n + 8 * ((n + ADAM8_BLOCK - 1) // ADAM8_BLOCK) if adam8_uses_8bit(n, optim_bits, min_8bit_size) else 8 * n
    return total


class LrSchedule:
    """The curve `lr_scheduler` names in the recipes (training.optim.lr_scheduler -> get_scheduler, pdm/training/trainer.py:376-383)
    as a function of the count k of APPLIED optimizer steps: the step that follows k applied ones runs at lr * m(k), the first at
    m(0), and a skipped step does not advance k.  warmup_steps W and training_steps T are optimizer steps (the single-process
    curve: DESIGN 6n).  The expressions are transformers.optimization's (csrc/lr_schedule.h holds them for the device):
    constant, constant_with_warmup, linear, cosine (num_cycles, default 0.5), cosine_with_restarts (num_cycles an integer,
    default 1), polynomial (power, lr_end; lr_init is the OPTIMIZER's default rate, which the library divides by -- the reference
    builds its optimizers from groups, so torch.optim.AdamW's 1e-3 -- not the rate the curve is applied to).
    ``multiplier(k)`` is m(k) in host fp64, ``rate(lr, k)`` the fp32 value aptp_lr_schedule stores; ``launch`` is that kernel."""

    KINDS = tuple(_lib.LR_KINDS)
    NEEDS_T = ("linear", "cosine", "cosine_with_restarts", "polynomial")
    MAX_STEPS = 1 << 24         # the count is an fp32 scalar: every integer below 2^24 is exact

    def __init__(self, name: str, warmup_steps: int = 0, training_steps: Optional[int] = None, num_cycles=None, power: float = 1.0,
                 lr_end: float = 1e-7, lr_init: float = 1e-3):
        name = str(getattr(name, "value", name))
        if name == "piecewise_constant":
            raise ValueError("LrSchedule: piecewise_constant is diffusers-only and takes a rule string; it is not built here "
                             "(DESIGN 6y) -- use one of " + ", ".join(self.KINDS))
        if name not in _lib.LR_KINDS:
            raise ValueError(f"LrSchedule: unknown lr_scheduler {name!r}; one of " + ", ".join(self.KINDS))
        self.name, self.kind = name, _lib.LR_KINDS[name]
        W = int(warmup_steps)
        if W != warmup_steps or not 0 <= W < self.MAX_STEPS:
            raise ValueError("LrSchedule: warmup_steps is an integer in [0, 2^24)")
        if name in self.NEEDS_T:
            if training_steps is None:
                raise ValueError(f"LrSchedule: {name} needs training_steps")
            T = int(training_steps)
            if T != training_steps or not 0 <= T < self.MAX_STEPS:
                raise ValueError("LrSchedule: training_steps is an integer in [0, 2^24)")
            if T < W or (name == "polynomial" and T == W):
                raise ValueError(f"LrSchedule: {name} with training_steps {T} and warmup_steps {W} (polynomial divides by T - W)")
        else:
            T = 0 if training_steps is None else int(training_steps)
            if not 0 <= T < self.MAX_STEPS:
                raise ValueError("LrSchedule: training_steps is an integer in [0, 2^24)")
        self.warmup_steps, self.training_steps = W, T
        if num_cycles is None:
            num_cycles = 1 if name == "cosine_with_restarts" else 0.5
        if name == "cosine_with_restarts" and int(num_cycles) != num_cycles:
            raise ValueError("LrSchedule: cosine_with_restarts takes an integer num_cycles")
        self.num_cycles, self.power, self.lr_end, self.lr_init = float(num_cycles), float(power), float(lr_end), float(lr_init)
        if name in ("cosine", "cosine_with_restarts") and not self.num_cycles > 0:
            raise ValueError("LrSchedule: num_cycles must be > 0")
        if name == "polynomial":
            if not self.power > 0:
                raise ValueError("LrSchedule: power must be > 0")
            if not self.lr_init > self.lr_end:
                raise ValueError(f"LrSchedule: lr_end ({lr_end}) must be smaller than lr_init ({lr_init}), the optimizer's default rate")

    def as_dict(self):
        return {"name": self.name, "warmup_steps": self.warmup_steps, "training_steps": self.training_steps,
                "num_cycles": self.num_cycles, "power": self.power, "lr_end": self.lr_end, "lr_init": self.lr_init}

    @classmethod
    def from_dict(cls, d):
        return cls(**d)

    def __eq__(self, other):
        return isinstance(other, LrSchedule) and self.as_dict() == other.as_dict()

    def __repr__(self):
        return "LrSchedule(" + ", ".join(f"{k}={v!r}" for k, v in self.as_dict().items()) + ")"

    def multiplier(self, k) -> float:
        """m(k), host fp64, expression by expression as the library evaluates it"""
        import math
        k, W, T, name = float(k), float(self.warmup_steps), float(self.training_steps), self.name
        if name == "constant":
            return 1.0
        if k < W:
            return k / max(1.0, W)
        if name == "constant_with_warmup":
            return 1.0
        if name == "linear":
            return max(0.0, (T - k) / max(1.0, T - W))
        if name == "polynomial":
            if k > T:
                return self.lr_end / self.lr_init
            pct = 1.0 - (k - W) / (T - W)
            return ((self.lr_init - self.lr_end) * pct ** self.power + self.lr_end) / self.lr_init
        prog = (k - W) / max(1.0, T - W)
        if name == "cosine":
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * self.num_cycles * 2.0 * prog)))
        if prog >= 1.0:
            return 0.0
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((self.num_cycles * prog) % 1.0))))

    def rate(self, lr: float, k) -> float:
        """what the kernel stores for base rate lr (as fp32) after k applied steps: (float)((double)lr * m(k)), except that constant
        stores lr itself and constant_with_warmup the fp32 expression of ``warmup_steps=W``, lr * min(1, k / W)"""
        f32 = lambda x: torch.tensor(x, dtype=torch.float64).to(torch.float32)      # noqa: E731
        lr32 = f32(float(lr))
        if self.name == "constant":
            return float(lr32)
        if self.name == "constant_with_warmup":
            W = self.warmup_steps
            return float(lr32 * torch.clamp(f32(float(k)) / f32(float(W)), max=1.0)) if W > 0 else float(lr32)
        return float(f32(float(lr32) * self.multiplier(k)))

    def launch(self, count: torch.Tensor, base: torch.Tensor, out: torch.Tensor, out_stride: int = 1, mult: Optional[torch.Tensor] = None):
        """one aptp_lr_schedule launch on the current stream: out[i * out_stride] <- rate(base[i], count) for every base rate"""
        assert count.dtype == base.dtype == out.dtype == torch.float32 and base.is_contiguous() and count.numel() == 1
        n = base.numel()
        assert out.numel() >= (n - 1) * out_stride + 1, "LrSchedule.launch: out is too small"
        q = _lib.LrScheduleParams()
        q.kind, q.warmup_steps, q.training_steps, q.n = self.kind, self.warmup_steps, self.training_steps, n
        q.num_cycles, q.power, q.lr_end, q.lr_init = self.num_cycles, self.power, self.lr_end, self.lr_init
        q.count_dev, q.base_dev, q.out_dev, q.out_stride = count.data_ptr(), base.data_ptr(), out.data_ptr(), int(out_stride)
        q.mult_dev = None if mult is None else mult.data_ptr()
        _lib.check(_lib.load().aptp_lr_schedule(ctypes.byref(q), ops._stream()), "aptp_lr_schedule")


def as_lr_schedule(s) -> Optional[LrSchedule]:
    """None, an LrSchedule or its as_dict()"""
    return s if (s is None or isinstance(s, LrSchedule)) else LrSchedule.from_dict(s)


class PackedAdamW:
    """torch.optim.AdamW's arithmetic over a PackedTrainer's state as ONE launch that also writes the bf16 operands
    (csrc/optim.hip).  The gradient tensors must exist and stay where they are (``.grad`` of every parameter as left by the
    captured backward of GraphedFineTunerStep: the graph re-writes the same addresses at every replay)."""

    def __init__(self, trainer: PackedTrainer, lr: float = 1e-5, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 group_of=None, warmup_steps: int = 0, max_grad_norm: Optional[float] = None, log_grad_norm: bool = False,
                 optim_bits: int = 32, min_8bit_size: int = ADAM8_MIN_SIZE, lr_schedule=None):
        """group_of: optional map parameter -> group index (e.g. the gradient bucket that completes it, ArenaGradReducer.bucket_of):
        the table is built per group and ``step_group(i)`` applies one group per launch, so the optimizer can follow a
        bucketed gradient exchange bucket by bucket; ``step()`` applies all groups.
        warmup_steps W > 0: the rate of the step that follows k applied steps is lr * min(1, k / W) -- `constant_with_warmup` of
        the fine-tune recipe (configs/finetuning/sd-2-1_cc3m.yaml:108-109) counted in optimizer steps; the kernel reads k from
        the device-side step count, so a gated (skipped) step does not advance the ramp.  0: constant lr.
        max_grad_norm X: torch.nn.utils.clip_grad_norm_(parameters, X) in front of every ``step()``, on the device (ops.GradNorm over
        the gradients of the table: two launches; the kernel multiplies the gradients by the coefficient it reads from device
        memory, they are not rewritten), and a non-finite norm skips the step as a non-finite gate does.  log_grad_norm=True: the
        norm is taken (and gates) without a threshold.  Neither: no GradNorm, no extra launch.
        optim_bits=8 (`use_8bit_adam` of the reference's recipe): tensors of at least min_8bit_size elements keep both
        moments as uint8 codes with one fp32 absmax per moment and 256 elements (``self.m`` / ``self.v`` hold the codes,
        ``self.absmax1`` / ``self.absmax2`` the scales) and take their step in a second launch (csrc/optim8.hip) under the same
        gate and factors; smaller tensors keep fp32 moments and the fp32 kernel.  32: nothing of this exists.
        lr_schedule: an LrSchedule (or its as_dict()): the rate follows that curve over the applied steps.  ``lr`` becomes
        a base rate in device memory (``lr_base_t``; set_lr rewrites it) and one aptp_lr_schedule launch in front of every step's
        AdamW launches writes ``lr_t`` from ``step_t``; the AdamW kernels read it (aptp_adamw_many_lr).  Not together with
        warmup_steps > 0: the schedule has its own.  None: neither tensor exists, nothing more is launched."""
        assert optim_bits in (32, 8), "PackedAdamW: optim_bits is 32 or 8"
        assert int(min_8bit_size) >= 1, "PackedAdamW: min_8bit_size"
        self.optim_bits, self.min_8bit_size = int(optim_bits), int(min_8bit_size)
        self.trainer, self.lr, self.betas, self.eps, self.weight_decay = trainer, lr, betas, eps, weight_decay
        self.group_of = group_of
        assert warmup_steps >= 0, "PackedAdamW: warmup_steps"
        self.warmup_steps = warmup_steps
        self.lr_schedule = as_lr_schedule(lr_schedule)
        assert self.lr_schedule is None or warmup_steps == 0, \
            "PackedAdamW: lr_schedule and warmup_steps > 0 (give the warm-up to the schedule: LrSchedule(name, warmup_steps=W, ...))"
        assert max_grad_norm is None or max_grad_norm > 0, "PackedAdamW: max_grad_norm"
        self.max_grad_norm, self._want_norm, self.grad_norm = max_grad_norm, (max_grad_norm is not None or log_grad_norm), None
        entries = [(p, sh) for p, sh in PackedTrainer.entries(trainer) if p.grad is not None]   # (entries no backward reaches have nothing to apply)
        assert entries, "PackedAdamW: run one backward first (the gradient addresses go into the kernel's table)"
        dev = entries[0][0].device
        self.entries = entries
        self.params = [p for p, _ in entries]
        by_id = {id(p): n for n, p in trainer.named_parameters()} if hasattr(trainer, "named_parameters") else {}
        self.names = [by_id.get(id(p), f"#{i}") for i, p in enumerate(self.params)]
        self.is8 = [adam8_uses_8bit(p.numel(), self.optim_bits, self.min_8bit_size) for p in self.params]
        self.m = [torch.full((p.numel(),), 127, dtype=torch.uint8, device=dev) if q else torch.zeros_like(p.data)
                  for p, q in zip(self.params, self.is8)]         # (the first moment's zero is code 127)
        self.v = [torch.zeros(p.numel(), dtype=torch.uint8, device=dev) if q else torch.zeros_like(p.data)
                  for p, q in zip(self.params, self.is8)]
        nqb = [(p.numel() + ADAM8_BLOCK - 1) // ADAM8_BLOCK for p in self.params]
        self.absmax1 = [torch.zeros(b, dtype=torch.float32, device=dev) if q else None for b, q in zip(nqb, self.is8)]
        self.absmax2 = [torch.zeros(b, dtype=torch.float32, device=dev) if q else None for b, q in zip(nqb, self.is8)]
        self.qmap1 = self.qmap2 = None
        if self.optim_bits == 8:                                  # both maps, uploaded once
            self.qmap1, self.qmap2 = adam8_code_map(True).to(dev), adam8_code_map(False).to(dev)
        self.step_t = torch.zeros((), dtype=torch.float32, device=dev)
        self.lr_base_t = self.lr_t = None
        if self.lr_schedule is not None:
            self.lr_base_t = torch.full((1,), float(lr), dtype=torch.float32, device=dev)
            self.lr_t = torch.zeros(1, dtype=torch.float32, device=dev)
        self.rebind_()

    def rebind_(self):
        """(re)build the kernel's table from the parameters' CURRENT gradient tensors (state is kept): once for a captured
        backward, whose replays re-write the same addresses; before every step of an eager loop, whose backward allocates"""
        lib = _lib.load()
        self.grads = [p.grad for p in self.params]      # keeps the addresses in the table alive
        idx32 = [i for i, q in enumerate(self.is8) if not q]         # (optim_bits = 32: every tensor, in order)
        idx8 = [i for i, q in enumerate(self.is8) if q]
        items, items8 = (_lib.AdamWItem * len(idx32))(), (_lib.AdamW8Item * len(idx8))()
        for it, i in list(zip(items, idx32)) + list(zip(items8, idx8)):
            (p, sh), m, v = self.entries[i], self.m[i], self.v[i]
            g = p.grad
            assert g is not None, f"PackedAdamW.rebind_: {self.names[i]} has no gradient (every tensor of the table needs one)"
            assert g.is_contiguous() and p.data.is_contiguous() and g.dtype == torch.float32 and p.dtype == torch.float32
            assert p.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0 and m.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0
            it.p, it.g, it.n = p.data_ptr(), g.data_ptr(), p.numel()
            if self.is8[i]:
                a1, a2 = self.absmax1[i], self.absmax2[i]
                assert m.dtype == v.dtype == torch.uint8 and a1.data_ptr() % 4 == 0 and a2.data_ptr() % 4 == 0
                it.m8, it.v8, it.absmax_m, it.absmax_v = m.data_ptr(), v.data_ptr(), a1.data_ptr(), a2.data_ptr()
            else:
                it.m, it.v = m.data_ptr(), v.data_ptr()
            if sh is not None:
                assert sh.dtype == torch.bfloat16 and sh.is_contiguous() and sh.numel() == p.numel() and sh.data_ptr() % 8 == 0
                it.shadow = sh.data_ptr()
        dev = self.params[0].device
        self.table = _lib.BlockTable(items, [lib.aptp_adamw_blocks(self.params[i].numel()) for i in idx32], dev) if idx32 else None
        self.table8 = _lib.BlockTable(items8, [lib.aptp_adamw8_blocks(self.params[i].numel()) for i in idx8], dev) if idx8 else None
        # per-group tables (bucketed data-parallel exchange): the same descriptors, regrouped, with block prefixes of their own
        self.groups, self.groups8 = None, None
        if self.group_of is not None:
            by, by8 = {}, {}
            for k, i in enumerate(idx32):
                by.setdefault(int(self.group_of(self.params[i])), []).append(k)
            for k, i in enumerate(idx8):
                by8.setdefault(int(self.group_of(self.params[i])), []).append(k)
            self.groups = {gi: self.table.subset(idx) for gi, idx in sorted(by.items())}
            self.groups8 = {gi: self.table8.subset(idx) for gi, idx in sorted(by8.items())}
        if self._want_norm:
            clipped = None if self.grad_norm is None else self.grad_norm.clipped.clone()
            self.grad_norm = ops.GradNorm(self.grads, self.params[0].device, max_norm=self.max_grad_norm)
            if clipped is not None:
                self.grad_norm.clipped.copy_(clipped)
        return self

    def _launch_rate(self):
        """lr_t <- the rate of the step that follows step_t applied ones (one small launch; nothing without a schedule)"""
        if self.lr_schedule is not None:
            self.lr_schedule.launch(self.step_t, self.lr_base_t, self.lr_t)

    def _launch(self, table, gate, grad_scale, grad_scale_dev=None):
        lib = _lib.load()
        q = _lib.AdamWParams()
        q.items_dev, q.starts_dev, q.n_items, q.total_blocks = table.args()
        q.lr, q.beta1, q.beta2, q.eps, q.weight_decay = self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay
        q.step_dev = self.step_t.data_ptr()
        q.gate_dev = None if gate is None else gate.data_ptr()
        q.grad_scale = float(grad_scale)
        q.warmup_steps = float(self.warmup_steps)
        if self.lr_t is not None:     # (the rate from device memory: what _launch_rate stored for this step)
            _lib.check(lib.aptp_adamw_many_lr(ctypes.byref(q), None if grad_scale_dev is None else grad_scale_dev.data_ptr(),
                                              self.lr_t.data_ptr(), ops._stream()), "aptp_adamw_many_lr")
        elif grad_scale_dev is None:
            _lib.check(lib.aptp_adamw_many(ctypes.byref(q), ops._stream()), "aptp_adamw_many")
        else:       # (the clip coefficient of ops.GradNorm, read from device memory as one more factor of grad_scale)
            _lib.check(lib.aptp_adamw_many_scaled(ctypes.byref(q), grad_scale_dev.data_ptr(), ops._stream()), "aptp_adamw_many_scaled")

    def _launch8(self, table, gate, grad_scale, grad_scale_dev=None):
        """the 8-bit tensors of `table`: the same step under the same gate and factors (csrc/optim8.hip)"""
        lib = _lib.load()
        q = _lib.AdamW8Params()
        q.items_dev, q.starts_dev, q.n_items, q.total_blocks = table.args()
        q.lr, q.beta1, q.beta2, q.eps, q.weight_decay = self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay
        q.step_dev = self.step_t.data_ptr()
        q.gate_dev = None if gate is None else gate.data_ptr()
        q.grad_scale = float(grad_scale)
        q.warmup_steps = float(self.warmup_steps)
        q.qmap_signed_dev, q.qmap_unsigned_dev = self.qmap1.data_ptr(), self.qmap2.data_ptr()
        q.items_host = ctypes.cast(table.host, ctypes.c_void_p)
        gs = None if grad_scale_dev is None else grad_scale_dev.data_ptr()
        if self.lr_t is not None:
            _lib.check(lib.aptp_adamw8_many_lr(ctypes.byref(q), gs, self.lr_t.data_ptr(), ops._stream()), "aptp_adamw8_many_lr")
        else:
            _lib.check(lib.aptp_adamw8_many(ctypes.byref(q), gs, ops._stream()), "aptp_adamw8_many")

    def _check_grads(self):
        for p, g in zip(self.params, self.grads):
            assert p.grad is g, "PackedAdamW: a gradient tensor was replaced (its address is part of the kernel's table)"

    @torch.no_grad()
    def step(self, gate: torch.Tensor = None, grad_scale: float = 1.0):
        """one AdamW step over every tensor (one launch).  gate: optional fp32 device scalar (the step's loss): the whole step
        -- parameters, moments, operands and the step count -- is skipped unless it is finite (reference: the batch skip of
        pdm/training/trainer.py:921-929); grad_scale multiplies the gradients first (1 / world after a summed exchange).
        With a gradient norm (max_grad_norm, log_grad_norm): the norm of the scaled gradients first, then AdamW with the clip
        coefficient as one more factor, gated by the norm's verdict (finite norm and finite gate).  Returns the gate the step
        ran under -- that verdict, else `gate` -- for whatever follows the optimizer under the same predicate (PackedEMA.step)."""
        self._check_grads()
        coef = None
        if self.grad_norm is not None:
            self.grad_norm.run(grad_scale, gate)
            gate, coef = self.grad_norm.verdict, self.grad_norm.coef
        self._launch_rate()
        if self.table is not None:
            self._launch(self.table, gate, grad_scale, coef)
        if self.table8 is not None:
            self._launch8(self.table8, gate, grad_scale, coef)
        self.finish_step(gate)
        return gate

    def set_max_grad_norm(self, value: Optional[float]):
        """another threshold for the steps to come, captured ones included (a device scalar); None: measure only"""
        assert self.grad_norm is not None, "PackedAdamW.set_max_grad_norm: built without max_grad_norm / log_grad_norm"
        self.max_grad_norm = value
        self.grad_norm.set_max_norm(value)

    @torch.no_grad()
    def set_lr(self, value: float):
        """another (base) rate for the steps to come.  With a schedule it is rewritten in device memory, behind a pending step"""
        self.lr = float(value)
        if self.lr_base_t is not None:
            PackedTrainer._sync(self.trainer)
            self.lr_base_t.fill_(float(value))

    def last_lr(self) -> float:
        """the rate of the NEXT step, as get_last_lr() reports it after scheduler.step() (host read of the step count: logging only)"""
        PackedTrainer._sync(self.trainer)
        k = float(self.step_t)
        sched = self.lr_schedule if self.lr_schedule is not None else LrSchedule("constant_with_warmup", self.warmup_steps)
        return sched.rate(self.lr, k)

    def last_grad_norm(self) -> float:
        """the norm the last step() measured, before clipping (host read: logging only)"""
        assert self.grad_norm is not None, "PackedAdamW.last_grad_norm: built without max_grad_norm / log_grad_norm"
        PackedTrainer._sync(self.trainer)
        return float(self.grad_norm.norm)

    def clipped_steps(self) -> int:
        """applied steps whose gradients were scaled down (host read: logging only)"""
        assert self.grad_norm is not None, "PackedAdamW.clipped_steps: built without max_grad_norm / log_grad_norm"
        PackedTrainer._sync(self.trainer)
        return int(self.grad_norm.clipped)

    @torch.no_grad()
    def step_group(self, gi: int, gate: torch.Tensor = None, grad_scale: float = 1.0):
        """the tensors of group gi only (no step-count update: call finish_step() after the last group).  No clip: the norm needs
        every group's gradients (a caller with a norm configured exchanges first and calls step())"""
        assert self.grad_norm is None, "PackedAdamW.step_group: a gradient norm covers all groups -- exchange first, then step()"
        self._launch_rate()         # (step_t moves in finish_step only: every group launch of a step stores the same bits)
        if gi in self.groups:
            self._launch(self.groups[gi], gate, grad_scale)
        if gi in self.groups8:
            self._launch8(self.groups8[gi], gate, grad_scale)

    @torch.no_grad()
    def finish_step(self, gate: torch.Tensor = None):
        if gate is None:
            self.step_t += 1.0
        else:
            self.step_t += torch.isfinite(gate.reshape(())).to(torch.float32)
        self.trainer.refresh_(shadows_done=True)

    def state_dict(self):
        """step count and both moments, keyed by the stable names of PackedTrainer.named_parameters() (resume:
        load_state_dict on an optimizer built over the same expert, whatever order its modules first ran in)"""
        clone = lambda ts: [None if t is None else t.clone() for t in ts]       # noqa: E731
        return {"step": self.step_t.clone(), "names": list(self.names),
                # the curve this optimizer was built with (None: none), for the record: load_state_dict keeps the constructed
                # optimizer's schedule, and the position on it is "step"
                "lr_schedule": None if self.lr_schedule is None else self.lr_schedule.as_dict(),
                "exp_avg": [m.clone() for m in self.m], "exp_avg_sq": [v.clone() for v in self.v],
                # optim_bits = 8: uint8 codes above for the 8-bit tensors, their scales and both maps here (None: fp32 moments)
                "optim_bits": self.optim_bits, "absmax1": clone(self.absmax1), "absmax2": clone(self.absmax2),
                "qmap1": None if self.qmap1 is None else self.qmap1.clone(), "qmap2": None if self.qmap2 is None else self.qmap2.clone()}

    @torch.no_grad()
    def load_state_dict(self, sd):
        assert len(sd["exp_avg"]) == len(sd["exp_avg_sq"]), "PackedAdamW: malformed state"
        names = sd.get("names")
        if names is None:                       # (states written before entries were named: positional)
            assert len(sd["exp_avg"]) == len(self.m), "PackedAdamW: different tensor list"
            order = list(range(len(self.m)))
        else:
            order = _order_by_name(names, self.names, "PackedAdamW")
        bits = int(sd.get("optim_bits", 32))
        assert bits == self.optim_bits, \
            f"PackedAdamW: the saved state holds {bits}-bit moments, this optimizer {self.optim_bits}-bit ones (no conversion on load)"
        if self.optim_bits == 8:
            for key, own in (("qmap1", self.qmap1), ("qmap2", self.qmap2)):
                assert sd.get(key) is not None and torch.equal(sd[key].to(own.device), own), \
                    f"PackedAdamW: the saved state's code map {key} is not this optimizer's: its codes mean other values"
            for i, j in enumerate(order):
                saved8 = sd["exp_avg"][j].dtype == torch.uint8
                assert saved8 == self.is8[i] and (sd["absmax1"][j] is not None) == self.is8[i], \
                    f"PackedAdamW: {self.names[i]}: saved with {'8-bit' if saved8 else 'fp32'} moments, {'8-bit' if self.is8[i] else 'fp32'} " \
                    f"here -- another partition (min_8bit_size = {self.min_8bit_size} here)"
        for i, j in enumerate(order):
            ma, va = sd["exp_avg"][j], sd["exp_avg_sq"][j]
            assert self.m[i].shape == ma.shape and self.v[i].shape == va.shape, \
                f"PackedAdamW: {self.names[i]}: saved moments {tuple(ma.shape)} / {tuple(va.shape)} vs {tuple(self.m[i].shape)}"
        self.step_t.copy_(sd["step"])
        for i, j in enumerate(order):
            self.m[i].copy_(sd["exp_avg"][j])    # in place: the moments' addresses are part of the kernel's table
            self.v[i].copy_(sd["exp_avg_sq"][j])
            if self.is8[i]:
                self.absmax1[i].copy_(sd["absmax1"][j])
                self.absmax2[i].copy_(sd["absmax2"][j])

    @torch.no_grad()
    def dequantized_state(self):
        """both moments of every tensor as fp32 in the tensor's shape, in torch.optim.AdamW's layout -- {"names": [...], "state":
        {i: {"step", "exp_avg", "exp_avg_sq"}}} in the order of ``self.params`` -- for whoever continues with another
        optimizer.  torch ops only: map[code] * absmax of the element's block (fp32 moments: clones)."""
        PackedTrainer._sync(self.trainer)
        state = {}
        for i, p in enumerate(self.params):
            if self.is8[i]:
                scale = lambda a: a.repeat_interleave(ADAM8_BLOCK)[:p.numel()]      # noqa: E731
                m = (self.qmap1[self.m[i].long()] * scale(self.absmax1[i])).view_as(p)
                v = (self.qmap2[self.v[i].long()] * scale(self.absmax2[i])).view_as(p)
            else:
                m, v = self.m[i].clone(), self.v[i].clone()
            state[i] = {"step": self.step_t.clone(), "exp_avg": m, "exp_avg_sq": v}
        return {"names": list(self.names), "state": state}

    def state_bytes(self) -> int:
        """bytes of the moment state: both moments of every tensor, the scales of the 8-bit ones included"""
        ts = self.m + self.v + [a for a in self.absmax1 + self.absmax2 if a is not None]
        return sum(t.numel() * t.element_size() for t in ts)


class PackedEMA:
    """Exponential moving average of a PackedTrainer's state (`use_ema` of the reference's interface, pdm/utils/arg_utils.py:50-54;
    the decay rule of diffusers' EMAModel) kept in the packed layout next to the masters: one fp32 tensor per ``_Gemm.P``,
    ``_Gemm.Pb``, ``_Affine.Pg`` and ``_Affine.Pb``, initialised as a clone -- +4 B per trainable element -- and keyed by the names of
    ``PackedTrainer.named_parameters()``.  ``step`` is ONE launch over a device table built once (csrc/ema.hip), gated and counted
    on the device like PackedAdamW; ``swap_`` exchanges masters and averages in one launch and rewrites the bf16 forward operands,
    so everything that reads the packed state at fixed addresses (validation graphs, ``export_``) reads the average."""

    def __init__(self, trainer: PackedTrainer, optimizer: Optional[PackedAdamW] = None, decay: float = 0.9999, min_decay: float = 0.0,
                 update_after_step: int = 0, use_ema_warmup: bool = False, inv_gamma: float = 1.0, power: float = 2.0 / 3.0):
        lib = _lib.load()
        assert 0.0 <= decay <= 1.0 and 0.0 <= min_decay <= decay and int(update_after_step) >= 0 and inv_gamma > 0 and power > 0, \
            "PackedEMA: hyper-parameters"
        self.trainer, self.optimizer = trainer, optimizer
        self.decay, self.min_decay, self.update_after_step = float(decay), float(min_decay), int(update_after_step)
        self.use_ema_warmup, self.inv_gamma, self.power = bool(use_ema_warmup), float(inv_gamma), float(power)
        entries = PackedTrainer.entries(trainer)
        assert entries, "PackedEMA: the trainer has no packed tensors yet (PackedTrainer.materialize)"
        by_id = {id(p): n for n, p in trainer.named_parameters()}
        self.entries = entries
        self.params = [p for p, _ in entries]
        self.names = [by_id[id(p)] for p in self.params]
        self.ema = [p.detach().clone() for p in self.params]
        dev = self.params[0].device
        self.count = torch.zeros((), dtype=torch.float32, device=dev)
        self._cur_decay = torch.zeros((), dtype=torch.float32, device=dev)
        self.swapped = False
        items = (_lib.EmaItem * len(entries))()
        for i, ((p, sh), a) in enumerate(zip(entries, self.ema)):
            assert p.dtype == torch.float32 and p.data.is_contiguous() and a.is_contiguous() and p.numel() >= 1
            assert p.data_ptr() % 16 == 0 and a.data_ptr() % 16 == 0
            it = items[i]
            it.p, it.ema, it.n = p.data_ptr(), a.data_ptr(), p.numel()
            if sh is not None:
                assert sh.dtype == torch.bfloat16 and sh.is_contiguous() and sh.numel() == p.numel() and sh.data_ptr() % 8 == 0
                it.shadow = sh.data_ptr()
        self.table = _lib.BlockTable(items, [lib.aptp_adamw_blocks(p.numel()) for p in self.params], dev)

    def n_elements(self) -> int:
        return sum(p.numel() for p in self.params)

    def _launch(self, mode: int, gate: Optional[torch.Tensor] = None):
        lib = _lib.load()
        q = _lib.EmaParams()
        q.items_dev, q.starts_dev, q.n_items, q.total_blocks = self.table.args()
        q.mode = mode
        q.count_dev = self.count.data_ptr()
        q.gate_dev = None if gate is None else gate.data_ptr()
        q.decay, q.min_decay, q.update_after_step = self.decay, self.min_decay, self.update_after_step
        q.use_warmup, q.inv_gamma, q.power = int(self.use_ema_warmup), self.inv_gamma, self.power
        q.cur_decay_dev = self._cur_decay.data_ptr()
        _lib.check(lib.aptp_ema_many(ctypes.byref(q), ops._stream()), "aptp_ema_many")

    @torch.no_grad()
    def step(self, gate: torch.Tensor = None):
        """one EMA update over every tensor (one launch), then the count on the device.  gate: optional fp32 device scalar (the
        step's loss): averages, decay and count stay as they are unless it is finite -- PackedAdamW's predicate.  No host sync."""
        assert not self.swapped, "PackedEMA.step: the masters hold the average (swap_() back first)"
        self._launch(_lib.EMA_UPDATE, gate)
        if gate is None:
            self.count += 1.0
        else:
            self.count += torch.isfinite(gate.reshape(())).to(torch.float32)

    @torch.no_grad()
    def swap_(self):
        """masters <-> averages in one launch; the bf16 forward operands follow the masters.  The data-gradient operands (pwb)
        are NOT rewritten: only a backward reads them, no step runs while swapped, and the swap back returns the masters bit for
        bit, so they are valid again."""
        PackedTrainer._sync(self.trainer)
        self._launch(_lib.EMA_SWAP)
        self.swapped = not self.swapped
        return self

    def applied(self):
        """context manager: the packed state holds the average inside, the trained values again afterwards"""
        import contextlib

        @contextlib.contextmanager
        def cm():
            self.swap_()
            try:
                yield self
            finally:
                self.swap_()
        return cm()

    def cur_decay(self) -> float:
        """the decay of the last applied update (host read: logging only)"""
        return float(self._cur_decay)

    def steps(self) -> int:
        """applied updates (host read: logging only)"""
        return int(self.count)

    def state_dict(self):
        """count and averages, keyed by the stable names of PackedTrainer.named_parameters()"""
        assert not self.swapped, "PackedEMA.state_dict: swapped (the averages sit in the masters)"
        PackedTrainer._sync(self.trainer)
        return {"count": self.count.clone(), "cur_decay": self._cur_decay.clone(), "names": list(self.names),
                "ema": [a.clone() for a in self.ema]}

    @torch.no_grad()
    def load_state_dict(self, sd):
        assert not self.swapped, "PackedEMA.load_state_dict: swapped (the averages sit in the masters)"
        names = sd["names"]
        assert len(sd["ema"]) == len(names), "PackedEMA: malformed state"
        order = _order_by_name(names, self.names, "PackedEMA")
        for i, j in enumerate(order):
            assert self.ema[i].shape == sd["ema"][j].shape, \
                f"PackedEMA: {self.names[i]}: saved average {tuple(sd['ema'][j].shape)} vs {tuple(self.ema[i].shape)}"
        PackedTrainer._sync(self.trainer)
        self.count.copy_(sd["count"])
        if "cur_decay" in sd:
            self._cur_decay.copy_(sd["cur_decay"])
        for i, j in enumerate(order):
            self.ema[i].copy_(sd["ema"][j])      # in place: the averages' addresses are part of the kernel's table
