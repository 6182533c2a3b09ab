"""RouterAdamW: the optimizer of the pruning stage's router (hyper-net + quantizer) as one call into csrc/router_optim.hip.

Everything a schedule changes -- the rate and weight decay of each parameter group, the warm-up, the count of applied steps, the
step count of every tensor -- lives in device memory, so ONE captured launch serves the whole recipe of
configs/pruning/sd-2-1_cc3m.yaml (pdm/training/trainer.py:804-834, 892-933): two parameter groups, `constant_with_warmup`, the
hyper-net pre-training phase in which the codebook gets no gradient, the skip of a batch whose backward produced NaNs, and a
resume from a checkpoint.  DESIGN 6p.

The state travels in torch's format: state_dict() has the layout of torch.optim.AdamW.state_dict() and load_state_dict() takes a
dict a torch.optim.AdamW wrote.  The two conversions (export_state_dict, adopt_state_dict) are pure functions of tensors on any
device."""
from __future__ import annotations

import ctypes

import torch

EXTRA_KEY = "router_adamw"          # top-level key next to torch's "state" and "param_groups": applied, skipped, warm-up


# ---- torch's state-dict layout <-> (step, exp_avg, exp_avg_sq) per parameter ------------------------------------------------------
def export_state_dict(steps, exp_avg, exp_avg_sq, groups, extra=None):
    """(step_i, m_i, v_i) of every parameter, in the order of the flattened groups -> the layout of torch.optim.AdamW.state_dict().
    steps: list of 0-d tensors (or numbers); groups: list of dicts {"n": parameters in the group, "lr", "weight_decay", "betas",
    "eps"}.  `extra` goes under EXTRA_KEY (torch's load_state_dict ignores keys it does not know)."""
    assert len(steps) == len(exp_avg) == len(exp_avg_sq) == sum(g["n"] for g in groups), "export_state_dict: malformed state"
    state = {}
    for i, (s, m, v) in enumerate(zip(steps, exp_avg, exp_avg_sq)):
        s = s.detach().clone().reshape(()).to(torch.float32) if torch.is_tensor(s) else torch.tensor(float(s), dtype=torch.float32, device=m.device)
        state[i] = {"step": s, "exp_avg": m.detach().clone(), "exp_avg_sq": v.detach().clone()}
    pgs, k = [], 0
    for g in groups:
        pgs.append({"lr": float(g["lr"]), "betas": (float(g["betas"][0]), float(g["betas"][1])), "eps": float(g["eps"]),
                    "weight_decay": float(g["weight_decay"]), "amsgrad": False, "maximize": False,
                    "params": list(range(k, k + g["n"]))})
        k += g["n"]
    sd = {"state": state, "param_groups": pgs}
    if extra is not None:
        sd[EXTRA_KEY] = dict(extra)
    return sd


def adopt_state_dict(sd, like):
    """a dict in torch.optim.AdamW's layout -> (steps, exp_avg, exp_avg_sq): lists over the flattened groups of NEW fp32 tensors on
    the device of `like`.  like: list (one entry per group) of lists of tensors giving shape and device.  A parameter without an
    entry in sd["state"] (torch creates state at a parameter's first gradient) gets zero moments and step 0.  Refused: another
    number of groups, another number of tensors in a group, an entry for a tensor that does not exist, another shape."""
    pgs = sd["param_groups"]
    if len(pgs) != len(like):
        raise ValueError(f"RouterAdamW: the saved state has {len(pgs)} parameter groups, this optimizer {len(like)}")
    ids = []
    for gi, (pg, ts) in enumerate(zip(pgs, like)):
        if len(pg["params"]) != len(ts):
            raise ValueError(f"RouterAdamW: different tensor list: group {gi} has {len(pg['params'])} saved tensors, {len(ts)} here")
        ids += list(pg["params"])
    flat = [t for ts in like for t in ts]
    if len(set(ids)) != len(ids) or set(sd["state"]) - set(ids):
        raise ValueError("RouterAdamW: different tensor list: the saved state names tensors its groups do not hold")
    steps, ms, vs = [], [], []
    for pid, t in zip(ids, flat):
        st = sd["state"].get(pid)
        if st is None:
            steps.append(torch.zeros((), dtype=torch.float32, device=t.device))
            ms.append(torch.zeros(t.shape, dtype=torch.float32, device=t.device))
            vs.append(torch.zeros(t.shape, dtype=torch.float32, device=t.device))
            continue
        m, v = st["exp_avg"], st["exp_avg_sq"]
        if tuple(m.shape) != tuple(t.shape) or tuple(v.shape) != tuple(t.shape):
            raise ValueError(f"RouterAdamW: tensor {pid}: saved moments {tuple(m.shape)} / {tuple(v.shape)} vs {tuple(t.shape)}")
        s = st["step"]
        steps.append(torch.as_tensor(float(s), dtype=torch.float32).to(t.device))
        ms.append(m.detach().to(device=t.device, dtype=torch.float32).clone())
        vs.append(v.detach().to(device=t.device, dtype=torch.float32).clone())
    return steps, ms, vs


class RouterAdamW:
    """torch.optim.AdamW's arithmetic over the router's parameters as one call of aptp_group_adamw.

    param_groups: torch's shape, [{"params": [...], "lr": ..., "weight_decay": ...}, ...]; fp32 contiguous parameters on the GPU.
    warmup_steps W > 0: `constant_with_warmup` counted in APPLIED steps -- the step that follows k applied ones runs at
    lr_g * min(1, k / W), the first at 0; a skipped step does not advance the ramp.

    Every parameter gets a zero-filled ``.grad`` that autograd accumulates into in place and that never moves: its address goes
    into the kernel's tables, which are therefore built before any capture, and the kernel writes the gradients back to zero
    after use.  ``add_table(key, params)`` builds a table over a subset (a training phase whose backward does not reach every
    parameter: a tensor outside the table keeps its value, moments and step count, weight decay included, as a torch parameter
    without a gradient does).

    An ITEM of a table is a run of parameters of one group that lie back to back in memory and have the same step count: the
    hyper-net keeps the weights (and the biases) of its 84 heads as row ranges of one buffer (hypernet.HyperStructure._flat_heads),
    so a single head starts at any multiple of 4 bytes, while the kernel reads float4 and refuses a pointer that is not 16-byte
    aligned.  A run starts where the buffer starts; its gradients and moments are one buffer each in the same order, the
    parameters' ``.grad`` / ``exp_avg`` / ``exp_avg_sq`` are views of them, and its tensors share one step count (they can only
    have been stepped together).  The arithmetic is per element, so it is what per-tensor items would compute.  The runs follow
    the parameters: when a parameter's storage has moved (module.to(), the hyper-net's first forward) the next step() outside a
    capture rebuilds them and keeps the state (rebind_()).

    A step is skipped -- parameters, moments, step counts and the warm-up untouched, ``skipped_steps()`` + 1 -- when ``gate`` is
    non-finite or any gradient element of the table is NaN or +-Inf (reference: trainer.py:921-929 under anomaly detection, which
    raises on NaN; Inf is skipped here as well).

    max_grad_norm X: torch.nn.utils.clip_grad_norm_(all parameters of the table, X) in front of the step, on the device: ONE norm
    over both groups (ops.GradNorm, csrc/grad_norm.hip: two more launches inside step(), so a captured step holds them); the
    update kernel multiplies the gradients by the coefficient it reads from device memory.  A zero-filled gradient (the codebook's
    during the pre-training) contributes nothing.  The threshold is a device scalar (set_max_grad_norm: no recapture); the
    clip has no state beyond a counter, so state_dict() is what it was.  log_grad_norm=True: the norm without a threshold.

    lr_schedule: a packed_train.LrSchedule (or its as_dict()): every group's rate follows that curve over the APPLIED steps (DESIGN
    6y).  The groups' rates become base rates in a table of their own next to ``groups_dev`` (``base_lr_dev``; set_lr writes it),
    and one aptp_lr_schedule launch inside step(), in front of the norm and the scan, rewrites the lr column of ``groups_dev``
    from counters[0] -- so a captured step holds it; the warm-up column stays 0.  Not together with warmup_steps > 0.  None: no
    base table, no launch."""

    def __init__(self, param_groups, betas=(0.9, 0.999), eps: float = 1e-8, warmup_steps: int = 0, max_grad_norm=None,
                 log_grad_norm: bool = False, lr_schedule=None):
        param_groups = list(param_groups)
        assert param_groups and all(isinstance(g, dict) and "params" in g for g in param_groups), \
            "RouterAdamW: param_groups = [{'params': [...], 'lr': ..., 'weight_decay': ...}, ...]"
        assert warmup_steps >= 0, "RouterAdamW: warmup_steps"
        self.betas, self.eps, self.warmup_steps = (float(betas[0]), float(betas[1])), float(eps), float(warmup_steps)
        self.defaults = {"lr": 1e-3, "betas": self.betas, "eps": self.eps, "weight_decay": 1e-2, "warmup_steps": self.warmup_steps}
        self.param_groups = []
        for g in param_groups:
            ps = list(g["params"])
            assert ps, "RouterAdamW: an empty parameter group"
            self.param_groups.append({"params": ps, "lr": float(g.get("lr", self.defaults["lr"])),
                                      "weight_decay": float(g.get("weight_decay", self.defaults["weight_decay"])),
                                      "betas": self.betas, "eps": self.eps, "warmup_steps": self.warmup_steps})
        self.params = [p for g in self.param_groups for p in g["params"]]
        self.group_index = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        assert len({id(p) for p in self.params}) == len(self.params), "RouterAdamW: a parameter appears twice"
        dev = self.params[0].device
        for p in self.params:
            assert p.is_leaf and p.dtype == torch.float32 and p.data.is_contiguous() and p.device == dev and p.numel() >= 1, \
                "RouterAdamW: fp32 contiguous leaf parameters on one device"
        self.device = dev
        self.counters = torch.zeros(4, dtype=torch.float32, device=dev)      # applied, skipped, bad-gradient flag, reserved
        self.groups_dev = torch.tensor([[g["lr"], g["weight_decay"], self.warmup_steps] for g in self.param_groups],
                                       dtype=torch.float32).to(dev)
        from .packed_train import as_lr_schedule
        self.lr_schedule, self.base_lr_dev = as_lr_schedule(lr_schedule), None
        if self.lr_schedule is not None:
            assert warmup_steps == 0, \
                "RouterAdamW: lr_schedule and warmup_steps > 0 (give the warm-up to the schedule: LrSchedule(name, warmup_steps=W, ...))"
            assert len(self.param_groups) <= 16, "RouterAdamW: lr_schedule serves at most 16 parameter groups (aptp_lr_schedule)"
            self.base_lr_dev = self.groups_dev[:, 0].clone()
        self.before_access = None      # GraphedPrunerStep.finish: orders the current stream behind a step pending on the router's stream
        self.grads = self.m = self.v = None
        assert max_grad_norm is None or max_grad_norm > 0, "RouterAdamW: max_grad_norm"
        self.max_grad_norm, self._want_norm = max_grad_norm, (max_grad_norm is not None or bool(log_grad_norm))
        self.grad_norm, self.norms = None, {}     # the GradNorm whose out / threshold every table's GradNorm shares; one per table
        self.table_keys = {None: list(range(len(self.params)))}
        self.rebind_()

    def _wait(self):
        if self.before_access is not None:
            self.before_access()

    # ---- runs and tables --------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def rebind_(self, steps=None):
        """(re)build the runs, their gradient / moment buffers and every table from where the parameters lie NOW; gradients,
        moments and step counts keep their values.  Never inside a capture, and graphs captured before it hold stale addresses.
        steps: per-parameter step counts to install (load_state_dict, _restore)."""
        self._wait()
        n = len(self.params)
        old = None if self.grads is None else (self.grads, self.m, self.v)
        steps = [0.0] * n if (steps is None and old is None) else (self.steps.tolist() if steps is None else [float(x) for x in steps])
        order = sorted(range(n), key=lambda i: (self.group_index[i], self.params[i].data_ptr()))
        runs = []
        for i in order:
            p = self.params[i]
            r = runs[-1] if runs else None
            if r is not None and r["group"] == self.group_index[i] and r["end"] == p.data_ptr() and r["step"] == steps[i]:
                r["idx"].append(i)
                r["end"] += p.numel() * 4
                r["n"] += p.numel()
            else:
                runs.append({"group": self.group_index[i], "ptr": p.data_ptr(), "end": p.data_ptr() + p.numel() * 4, "n": p.numel(),
                             "idx": [i], "step": steps[i]})
        self.grads, self.m, self.v, self.run_of = [None] * n, [None] * n, [None] * n, [0] * n
        for ri, r in enumerate(runs):
            assert r["ptr"] % 16 == 0, \
                "RouterAdamW: a parameter (or a run of parameters sharing a buffer and a step count) is not 16-byte aligned"
            flat = [torch.zeros(r["n"], dtype=torch.float32, device=self.device) for _ in range(3)]
            r["g"], r["m"], r["v"] = flat
            off = 0
            for i in r["idx"]:
                p = self.params[i]
                for dst, f in zip((self.grads, self.m, self.v), flat):
                    dst[i] = f[off:off + p.numel()].view(p.shape)
                off += p.numel()
                self.run_of[i] = ri
        if old is not None:
            for new_l, old_l in zip((self.grads, self.m, self.v), old):
                for a, b in zip(new_l, old_l):
                    a.copy_(b)
        for i, (p, g) in enumerate(zip(self.params, self.grads)):
            if old is None or p.grad is None or p.grad is old[0][i]:
                p.grad = g              # (any other tensor is a gradient from elsewhere: adopt_grads() moves it in)
        self.runs = runs
        self.run_steps = torch.tensor([r["step"] for r in runs], dtype=torch.float32).to(self.device)
        self._gather = torch.tensor(self.run_of, dtype=torch.int64).to(self.device)
        self.ptrs = [p.data_ptr() for p in self.params]
        self.tables, self.norms = {}, {}
        for key, idx in self.table_keys.items():
            self._build_table(key, idx)
        return self

    @property
    def steps(self):
        """the step count of every parameter (fp32 [n_params]; a copy)"""
        return self.run_steps[self._gather]

    def _build_table(self, key, idx):
        from . import _lib
        lib = _lib.load()
        want = set(idx)
        runs = [ri for ri, r in enumerate(self.runs) if want & set(r["idx"])]
        for ri in runs:
            assert set(self.runs[ri]["idx"]) <= want, \
                "RouterAdamW.add_table: parameters that share a buffer (the hyper-net's heads) go into a table together"
        assert runs, "RouterAdamW.add_table: no parameters"
        items = (_lib.GroupAdamWItem * len(runs))()
        for it, ri in zip(items, runs):
            r = self.runs[ri]
            it.p, it.g, it.m, it.v, it.n = r["ptr"], r["g"].data_ptr(), r["m"].data_ptr(), r["v"].data_ptr(), r["n"]
            it.step, it.group = self.run_steps.data_ptr() + 4 * ri, r["group"]
        self.tables[key] = _lib.BlockTable(items, [lib.aptp_group_adamw_blocks(self.runs[ri]["n"]) for ri in runs], self.device)
        if self._want_norm:
            from . import ops
            self.norms[key] = ops.GradNorm([self.runs[ri]["g"] for ri in runs], self.device, max_norm=self.max_grad_norm,
                                           share=self.grad_norm)
            if self.grad_norm is None:
                self.grad_norm = self.norms[key]

    def add_table(self, key, params):
        """a descriptor table over a subset of the parameters (device memory; built once, before any capture)"""
        pos = {id(p): i for i, p in enumerate(self.params)}
        self.table_keys[key] = sorted({pos[id(p)] for p in params})
        if self._moved():
            self.rebind_()
        else:
            self._build_table(key, self.table_keys[key])
        return self

    def table_params(self, key=None):
        return [self.params[i] for i in self.table_keys[key]]

    def _moved(self):
        return any(p.data_ptr() != ptr for p, ptr in zip(self.params, self.ptrs))

    # ---- stepping -------------------------------------------------------------------------------------------------------------
    def _check(self):
        if self._moved():
            assert not torch.cuda.is_current_stream_capturing(), \
                "RouterAdamW: a parameter moved (module.to(), the hyper-net's first forward) -- run one step before capturing"
            self.rebind_()
        for p, g in zip(self.params, self.grads):
            assert p.grad is g, "RouterAdamW: a gradient tensor was replaced (its address is part of the kernel's table): adopt_grads()"

    @torch.no_grad()
    def step(self, table=None, gate: torch.Tensor = None, grad_scale: float = 1.0):
        """one AdamW step over the tensors of `table` (default: all): ONE call, three launches on the current stream, nothing on
        the host.  gate: optional fp32 device scalar (the step's total loss).  The gradients are zero afterwards.  With a
        gradient norm: two launches in front, over the gradients of this table; the step runs under the norm's verdict."""
        from . import _lib, ops
        assert self.device.type == "cuda", "RouterAdamW.step: the kernel runs on the GPU"
        self._check()
        tb = self.tables[table]
        q = _lib.GroupAdamWParams()
        q.items_dev, q.starts_dev, q.n_items, q.total_blocks = tb.args()
        q.groups_dev, q.n_groups, q.counters_dev = self.groups_dev.data_ptr(), len(self.param_groups), self.counters.data_ptr()
        q.beta1, q.beta2, q.eps, q.grad_scale, q.zero_grad = self.betas[0], self.betas[1], self.eps, float(grad_scale), 1
        if gate is not None:
            assert gate.dtype == torch.float32 and gate.device == self.device and gate.numel() == 1
            q.gate_dev = gate.data_ptr()
        q.items_host = ctypes.cast(tb.host, ctypes.c_void_p)
        if self.lr_schedule is not None:      # the lr column of groups_dev <- base rates x m(applied): read by this step's update launch
            self.lr_schedule.launch(self.counters[0:1], self.base_lr_dev, self.groups_dev, out_stride=3)
        if self._want_norm:
            gn = self.norms[table]
            gn.run(grad_scale, gate)
            q.gate_dev, q.grad_scale_dev = gn.verdict.data_ptr(), gn.coef.data_ptr()
        _lib.check(_lib.load().aptp_group_adamw(ctypes.byref(q), ops._stream()), "aptp_group_adamw")

    @torch.no_grad()
    def zero_grad(self, set_to_none: bool = True):
        """the static gradient tensors are written to zero and stay (set_to_none would drop addresses the tables hold)"""
        for r in self.runs:
            r["g"].zero_()
        for p, g in zip(self.params, self.grads):
            p.grad = g

    @torch.no_grad()
    def adopt_grads(self):
        """gradients that landed in other tensors (a probing backward with .grad = None, an all-reduce that replaced .grad) are
        moved into the static ones, which become .grad again; a parameter without a gradient gets zeros"""
        if self._moved():
            self.rebind_()
        for p, g in zip(self.params, self.grads):
            if p.grad is not g:
                if p.grad is None:
                    g.zero_()
                else:
                    g.copy_(p.grad)
                p.grad = g

    # ---- schedule ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def set_lr(self, group: int, value: float):
        """the rate of one group, written into the device table: replays of a captured step read it (no recapture, no host wait)"""
        self._wait()
        self.param_groups[group]["lr"] = float(value)
        if self.base_lr_dev is not None:      # (with a schedule the lr column is what the rate launch derives from this)
            self.base_lr_dev[group] = float(value)
        else:
            self.groups_dev[group, 0] = float(value)

    @torch.no_grad()
    def set_weight_decay(self, group: int, value: float):
        self._wait()
        self.param_groups[group]["weight_decay"] = float(value)
        self.groups_dev[group, 1] = float(value)

    @torch.no_grad()
    def set_max_grad_norm(self, value):
        """the clip threshold, written into device memory: replays of a captured step read it.  None: measure only."""
        assert self.grad_norm is not None, "RouterAdamW.set_max_grad_norm: built without max_grad_norm / log_grad_norm"
        self._wait()
        self.max_grad_norm = value
        self.grad_norm.set_max_norm(value)

    def last_grad_norm(self) -> float:
        """the norm the last step measured, before clipping (waits for the device: logging)"""
        assert self.grad_norm is not None, "RouterAdamW.last_grad_norm: built without max_grad_norm / log_grad_norm"
        self._wait()
        return float(self.grad_norm.norm)

    def clipped_steps(self) -> int:
        assert self.grad_norm is not None, "RouterAdamW.clipped_steps: built without max_grad_norm / log_grad_norm"
        self._wait()
        return int(self.grad_norm.clipped)

    def applied_steps(self) -> int:
        """(waits for the device: logging and checkpoints)"""
        self._wait()
        return int(self.counters[0].item())

    def skipped_steps(self) -> int:
        self._wait()
        return int(self.counters[1].item())

    def last_lr(self):
        """the rate of each group for the NEXT step, as LambdaLR.get_last_lr() reports it after scheduler.step()"""
        k, W = self.applied_steps(), self.warmup_steps
        if self.lr_schedule is not None:
            return [self.lr_schedule.rate(g["lr"], k) for g in self.param_groups]
        return [g["lr"] * (min(1.0, k / W) if W > 0 else 1.0) for g in self.param_groups]

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def _snapshot(self):
        """everything a step changes, for GraphedPrunerStep's capture warm-up (restored in place by _restore)"""
        self._wait()
        return dict(p=[p.detach().clone() for p in self.params], m=[m.clone() for m in self.m], v=[v.clone() for v in self.v],
                    steps=self.steps.clone(), counters=self.counters.clone(), groups=self.groups_dev.clone(),
                    norm=None if self.grad_norm is None else self.grad_norm.out.clone())

    @torch.no_grad()
    def _restore(self, snap):
        self._wait()
        for dst, src in zip(list(self.params) + self.m + self.v, snap["p"] + snap["m"] + snap["v"]):
            dst.copy_(src)
        self._install_steps(snap["steps"])
        self.counters.copy_(snap["counters"])
        if snap.get("groups") is not None:      # (the lr column a scheduled warm-up step rewrote)
            self.groups_dev.copy_(snap["groups"])
        if snap.get("norm") is not None:
            self.grad_norm.out.copy_(snap["norm"])
        self.zero_grad()

    def _install_steps(self, steps):
        """per-parameter step counts -> the runs (in place when every run is still uniform, else the runs are rebuilt)"""
        per = [float(x) for x in (steps.tolist() if torch.is_tensor(steps) else steps)]
        if self._moved() or any(len({per[i] for i in r["idx"]}) != 1 for r in self.runs):
            self.rebind_(steps=per)
        else:
            self.run_steps.copy_(torch.tensor([per[r["idx"][0]] for r in self.runs], dtype=torch.float32))

    def _extra(self, c):
        ex = {"applied": c[0], "skipped": c[1], "warmup_steps": self.warmup_steps}
        if self.lr_schedule is not None:      # (for the record: load_state_dict keeps the constructed optimizer's schedule)
            ex["lr_schedule"] = self.lr_schedule.as_dict()
        return ex

    def state_dict(self):
        """torch.optim.AdamW.state_dict()'s layout (state[i] = {step, exp_avg, exp_avg_sq}, param_groups) plus one key,
        "router_adamw": {applied, skipped, warmup_steps[, lr_schedule]}; param_groups hold the BASE rates"""
        groups = [{"n": len(g["params"]), "lr": g["lr"], "weight_decay": g["weight_decay"], "betas": self.betas, "eps": self.eps}
                  for g in self.param_groups]
        self._wait()
        c = self.counters.tolist()
        return export_state_dict(list(self.steps.unbind(0)), self.m, self.v, groups,
                                 extra=self._extra(c))

    @torch.no_grad()
    def load_state_dict(self, sd):
        """takes state_dict()'s output or a torch.optim.AdamW's; in place (the addresses are in the tables; only parameters that
        share a buffer but not a step count make the runs, and with them the tables, change -- load before capturing).  Rates and
        weight decay come from the saved groups.  A torch dict has no count of applied steps: the largest step of any tensor
        stands in (every applied step advances at least one tensor), which places a resumed warm-up where the scheduler was."""
        steps, ms, vs = adopt_state_dict(sd, [g["params"] for g in self.param_groups])
        self._wait()
        if self._moved():
            self.rebind_()
        for i in range(len(self.params)):
            self.m[i].copy_(ms[i])
            self.v[i].copy_(vs[i])
        self._install_steps([float(x) for x in steps])
        for gi, pg in enumerate(sd["param_groups"]):
            self.set_lr(gi, pg["lr"])
            self.set_weight_decay(gi, pg["weight_decay"])
        ex = sd.get(EXTRA_KEY)
        applied = float(ex["applied"]) if ex is not None else max(float(x) for x in steps)
        self.counters.copy_(torch.tensor([applied, float(ex["skipped"]) if ex is not None else 0.0, 0.0, 0.0]))
