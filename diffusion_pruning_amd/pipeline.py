"""Denoise-loop glue of StableDiffusionPruningPipeline (pdm/pipelines/pruning_pipelines.py:746-759, 787-824), SURVEY §8
row a21 / f.2: route the prompt batch once -> ``unet.set_structure`` -> per step: CFG batch doubling -> U-Net ->
``uncond + s*(text - uncond)`` -> scheduler step.  Token ids are encoded by the HIP CLIP text encoder (``text_encoder=``,
``prompt_ids=``), the router's MPNet token ids by the HIP prompt encoder (``prompt_encoder=``, ``router_ids=``) and latents
decoded by the HIP VAE (``vae=``); the safety checker is not reproduced.

MI355X-first differences:
  * the cross-attention K/V projections depend only on the text states, so they are computed ONCE per prompt batch
    (``UNet2DConditionModelGated.precompute_context``) and reused by every step;
  * one step (U-Net + CFG combine + DDIM update, all on the device, timestep and scheduler coefficients read from
    device tensors) is captured into a HIP graph and replayed ``num_inference_steps`` times;
  * a hard, batch-shared architecture code (one expert per call, as in generate_fid_images.py) takes the
    compacted-weight fast path of the U-Net; per-prompt codes fall back to fused per-sample gates in PruningDenoiseLoop;
  * ExpertDispatchLoop instead groups a routed batch by expert and runs every group through that expert's compacted
    weights, one captured step per (expert, bucket size), results back in the caller's prompt order;
  * ``fused_step=True`` replaces everything after the U-Net call of a step -- guidance, the optional guidance rescale, the
    scheduler update -- by one launch (ops.guided_step, csrc/sched_step.hip);
  * ``seeds=`` draws the latents on the device (ops.randn, csrc/philox_normal.hip: every normal a pure function of the
    sample's seed, the draw index and the element, so a prompt's noise does not depend on its batch), and the stochastic
    samplers -- DDIM with eta > 0, SDE-DPM-Solver++ -- add their step noise inside the captured step (ops.add_noise, one
    more launch whose seeds, draw index and scale live in device memory).
"""
from __future__ import annotations

import contextlib
from collections import OrderedDict
from dataclasses import dataclass
from typing import Optional

import torch


def rescale_noise_cfg(noise_cfg: torch.Tensor, noise_pred_text: torch.Tensor, guidance_rescale: float = 0.0) -> torch.Tensor:
    """Guidance rescale of Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed" (2023), section 3.4, as
    the reference applies it after classifier-free guidance (pruning_pipelines.py:809-811, diffusers' ``rescale_noise_cfg``):
    the guided output is scaled to the text branch's per-sample standard deviation (over all non-batch elements, unbiased as
    ``Tensor.std``) and blended with the unscaled one by ``guidance_rescale``.
    PARITY PIN: diffusers is absent, so this is restated from the reference's call site and the paper (eq. 15-16) --
    unpinned against a live run; tests pin it against an fp64 evaluation written out in the test."""
    dims = list(range(1, noise_pred_text.ndim))
    std_text = noise_pred_text.std(dim=dims, keepdim=True)
    std_cfg = noise_cfg.std(dim=dims, keepdim=True)
    rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * rescaled + (1 - guidance_rescale) * noise_cfg


def _fused(kind: str, scheduler, noise, sample, state, guidance_scale, guidance_rescale, do_cfg):
    from . import ops
    if sample.dtype != torch.float32:
        raise ValueError(f"fused_step: the sample must be fp32, got {sample.dtype}")
    return ops.guided_step(noise if noise.is_contiguous() else noise.contiguous(), sample.contiguous(), state, scheduler=kind,
                           prediction_type=scheduler.prediction_type, guidance_scale=guidance_scale,
                           guidance_rescale=guidance_rescale, do_cfg=do_cfg)


def _noise_state(sch, state: dict, latents: torch.Tensor, seeds) -> dict:
    """the per-call entries a stochastic scheduler adds to its state: the noise scale and the draw index of this call (device
    tensors that ``load_step`` refreshes) and the per-sample seeds (absent without seeds: ``step`` then needs ``noise=``)"""
    dev = latents.device
    state["noise_scale"] = sch.noise_coef[0:1].to(dev).clone()
    state["draw"] = sch.draws[0:1].to(dev).clone()
    if seeds is not None:
        if not isinstance(seeds, torch.Tensor):
            seeds = torch.tensor([int(v) for v in ([seeds] * latents.shape[0] if isinstance(seeds, int) else seeds)], dtype=torch.int64)
        if seeds.dtype != torch.int64 or tuple(seeds.shape) != (latents.shape[0],):
            raise ValueError(f"make_state: seeds must be int64 [{latents.shape[0]}], got {seeds.dtype} {tuple(seeds.shape)}")
        state["seeds"] = seeds.to(dev).clone()
    return state


def _load_noise_step(sch, state: dict, i: int):
    state["noise_scale"].copy_(sch.noise_coef[i:i + 1])
    state["draw"].copy_(sch.draws[i:i + 1])                      # call i uses draw i + 1; draw 0 is the initial latents


def _add_noise(out: torch.Tensor, state: dict, noise) -> torch.Tensor:
    """out + noise_scale z, a multiply then an add: z given (plain torch, any device) or drawn on the device from the state's
    seeds and draw index, in place (ops.add_noise)"""
    if noise is not None:
        return out + state["noise_scale"] * noise.to(out.dtype)
    if "seeds" not in state:
        raise ValueError("a stochastic step needs seeds (make_state(latents, seeds)) or an explicit noise=")
    from . import ops
    return ops.add_noise(out, state["seeds"], state["draw"], state["noise_scale"], out=out)


class DDIMSchedulerLite:
    """Minimal DDIM for SD-2.1's schedule: scaled-linear betas 0.00085..0.012 over 1000 steps, "leading"
    timestep spacing with steps_offset 1, v-prediction or epsilon.  Plain tensor math (device-agnostic), restated
    from the published DDIM update; the reference uses diffusers' DDIM/PNDM schedulers (pruning_pipelines.py:805-814).
    eta = 0 (the default) is the deterministic sampler.  eta > 0 is the stochastic one of Song et al. 2021, eq. 12 / 16, as
    diffusers' ``DDIMScheduler.step`` writes it: var = (1 - a_prev) / (1 - a_t) (1 - a_t / a_prev), std = eta sqrt(var), the
    next sample sqrt(a_prev) x0 + sqrt(1 - a_prev - std^2) eps + std z.  The table's fourth column and ``noise_coef`` (std per
    call) are then evaluated in fp64 on the host (``table``, ``noise_table``); z comes from the project's seeded device stream
    (ops.add_noise: seed of the sample, draw i + 1 at call i), one more launch after the update."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 prediction_type: str = "v_prediction", steps_offset: int = 1, eta: float = 0.0):
        if not 0.0 <= float(eta) <= 1.0:
            raise ValueError(f"eta must be in [0, 1], got {eta!r}")
        self.eta = float(eta)
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = self.alphas_cumprod[0]
        self.num_train_timesteps = num_train_timesteps
        self.prediction_type = prediction_type
        self.steps_offset = steps_offset
        self.init_noise_sigma = 1.0
        self.timesteps = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        ratio = self.num_train_timesteps // num_inference_steps
        ts = (torch.arange(0, num_inference_steps) * ratio).round().flip(0).long() + self.steps_offset
        self.num_inference_steps = num_inference_steps
        self.timesteps = ts.to(device) if device is not None else ts
        prev = ts - ratio
        a_t = self.alphas_cumprod[ts]
        a_prev = torch.where(prev >= 0, self.alphas_cumprod[prev.clamp(min=0)], self.final_alpha_cumprod)
        # per-step coefficient table [steps, 4]: sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)
        self.coef = torch.stack([a_t.sqrt(), (1 - a_t).sqrt(), a_prev.sqrt(), (1 - a_prev).sqrt()], dim=1)
        self.noise_coef = torch.zeros(num_inference_steps, dtype=torch.float32)
        if self.stochastic:
            a_t, a_prev = a_t.double(), a_prev.double()
            std = self.eta * ((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)).sqrt()
            self.table = torch.stack([a_t.sqrt(), (1 - a_t).sqrt(), a_prev.sqrt(), (1 - a_prev - std * std).sqrt()], dim=1)
            self.noise_table = std
            self.coef, self.noise_coef = self.table.float(), std.float()
        self.draws = torch.arange(1, num_inference_steps + 1, dtype=torch.int64)
        if device is not None:
            self.coef, self.noise_coef, self.draws = self.coef.to(device), self.noise_coef.to(device), self.draws.to(device)
        return self.timesteps

    @property
    def stochastic(self) -> bool:
        return self.eta > 0.0

    def step_coef(self, model_output: torch.Tensor, coef: torch.Tensor, sample: torch.Tensor) -> torch.Tensor:
        """x_{t-1} from the model output with coefficients coef = [sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)]"""
        sa, sb, sap, sbp = coef[0], coef[1], coef[2], coef[3]
        if self.prediction_type == "v_prediction":
            x0 = sa * sample - sb * model_output
            eps = sa * model_output + sb * sample
        else:
            eps = model_output
            x0 = (sample - sb * eps) / sa
        return sap * x0 + sbp * eps

    # ---- per-step state interface shared with PNDMSchedulerLite (everything a step reads lives in static device tensors, so
    # one captured step serves the whole loop) -------------------------------------------------------------------------------
    def n_model_calls(self) -> int:
        return self.num_inference_steps

    def make_state(self, latents: torch.Tensor, seeds=None) -> dict:
        state = {"coef": self.coef[0].clone()}
        return _noise_state(self, state, latents, seeds) if self.stochastic else state

    def load_step(self, state: dict, i: int):
        state["coef"].copy_(self.coef[i])
        if self.stochastic:
            _load_noise_step(self, state, i)

    def step(self, model_output: torch.Tensor, sample: torch.Tensor, state: dict, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``noise``: an explicit z for the stochastic form instead of the device stream (plain torch, any device)"""
        out = self.step_coef(model_output, state["coef"], sample)
        return _add_noise(out, state, noise) if self.stochastic else out

    def fused_step(self, noise: torch.Tensor, sample: torch.Tensor, state: dict, *, guidance_scale: float = 1.0,
                   guidance_rescale: float = 0.0, do_cfg: bool = False) -> torch.Tensor:
        """guidance (noise [2b, ...] = [uncond; text] with do_cfg), the optional rescale and ``step`` in one HIP launch"""
        out = _fused("ddim", self, noise, sample, state, guidance_scale, guidance_rescale, do_cfg)
        return _add_noise(out, state, None) if self.stochastic else out


class PNDMSchedulerLite:
    """PNDM / PLMS as StableDiffusionPruningPipeline runs it (configs/img_generation/sd-2-1_cc3m.yaml:50; scheduler call
    pruning_pipelines.py:810-814): pseudo linear multi-step with ``skip_prk_steps=True``, scaled-linear betas, "leading"
    spacing with steps_offset 1, epsilon or v-prediction.  N inference steps are N + 1 U-Net calls: the second call repeats
    the second timestep and redoes the first transfer with the average of the two outputs (the PLMS warm start), then
    2-, 3- and 4-term Adams-Bashforth combinations of the stored outputs feed the transfer
        x_prev = sqrt(a_prev / a_t) x - (a_prev - a_t) eps / (a_t sqrt(1 - a_prev) + sqrt(a_t (1 - a_t) a_prev)).
    PARITY PIN: diffusers==0.23.1 is absent, so this is restated from the published algorithm (Liu et al., "Pseudo Numerical
    Methods for Diffusion Models on Manifolds", 2022, eq. 9 and 12; diffusers' ``scheduling_pndm.py`` step_plms /
    _get_prev_sample) -- unpinned against a live run; tests pin it against DDIMSchedulerLite (identical transfer for a
    constant model output) and against a plain-Python restatement with explicit history lists.
    Graph-friendly form: the history is a 5-slot device ring, and which slot is written, the combination weights, the
    transfer coefficients and the two warm-start switches are per-step TABLES copied into static buffers, so one captured
    step serves all N + 1 calls."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 prediction_type: str = "v_prediction", steps_offset: int = 1):
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = self.alphas_cumprod[0]
        self.num_train_timesteps = num_train_timesteps
        self.prediction_type = prediction_type
        self.steps_offset = steps_offset
        self.init_noise_sigma = 1.0
        self.timesteps = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        N = num_inference_steps
        ratio = self.num_train_timesteps // N
        base = (torch.arange(0, N) * ratio).round().long() + self.steps_offset          # ascending
        plms = torch.cat([base[:-1], base[-2:-1], base[-1:]]).flip(0)                    # [t_N-1, t_N-2, t_N-2, t_N-3, ..., t_0]
        self.num_inference_steps = N
        self.timesteps = plms.to(device) if device is not None else plms
        # per-call tables: slot written (0..3 history ring, 4 = scratch), weights over the 5 slots, (a_t, a_prev) of the
        # transfer, use_saved (call 1 restarts from the sample saved at call 0), save (call 0 saves its sample)
        slots, W, coef, use_saved, save = [], [], [], [], []
        hist = []                                      # ring slots of the stored outputs, newest last
        nxt = 0
        for c in range(N + 1):
            t = int(plms[c])
            w = [0.0] * 5
            if c == 1:
                slot, t_from, t_to = 4, t + ratio, t
                w[hist[-1]], w[4] = 0.5, 0.5
            else:
                slot, t_from, t_to = nxt, t, t - ratio
                nxt = (nxt + 1) % 4
                hist = (hist + [slot])[-4:]
                if len(hist) == 1:
                    w[hist[-1]] = 1.0
                elif len(hist) == 2:
                    w[hist[-1]], w[hist[-2]] = 1.5, -0.5
                elif len(hist) == 3:
                    w[hist[-1]], w[hist[-2]], w[hist[-3]] = 23.0 / 12, -16.0 / 12, 5.0 / 12
                else:
                    w[hist[-1]], w[hist[-2]], w[hist[-3]], w[hist[-4]] = 55.0 / 24, -59.0 / 24, 37.0 / 24, -9.0 / 24
            a_t = float(self.alphas_cumprod[t_from])
            a_p = float(self.alphas_cumprod[t_to]) if t_to >= 0 else float(self.final_alpha_cumprod)
            slots.append(slot); W.append(w); coef.append([a_t, a_p])
            use_saved.append(1.0 if c == 1 else 0.0); save.append(1.0 if c == 0 else 0.0)
        self.tab = {"slot": torch.tensor(slots, dtype=torch.long), "w": torch.tensor(W, dtype=torch.float32),
                    "coef": torch.tensor(coef, dtype=torch.float32),
                    "flags": torch.tensor(list(zip(use_saved, save)), dtype=torch.float32)}
        if device is not None:
            self.tab = {k: v.to(device) for k, v in self.tab.items()}
        return self.timesteps

    def n_model_calls(self) -> int:
        return self.num_inference_steps + 1

    def make_state(self, latents: torch.Tensor) -> dict:
        z = torch.zeros_like(latents, dtype=torch.float32)
        return {"slot": self.tab["slot"][0:1].clone(), "w": self.tab["w"][0].clone(), "coef": self.tab["coef"][0].clone(),
                "flags": self.tab["flags"][0].clone(), "E": torch.zeros((5,) + tuple(latents.shape), dtype=torch.float32, device=latents.device),
                "saved": z}

    def load_step(self, state: dict, i: int):
        state["slot"].copy_(self.tab["slot"][i:i + 1])
        state["w"].copy_(self.tab["w"][i])
        state["coef"].copy_(self.tab["coef"][i])
        state["flags"].copy_(self.tab["flags"][i])

    def step(self, model_output: torch.Tensor, sample: torch.Tensor, state: dict) -> torch.Tensor:
        E, w, flags = state["E"], state["w"], state["flags"]
        x = sample.float()
        E.index_copy_(0, state["slot"], model_output.float()[None])
        state["saved"].add_(flags[1] * (x - state["saved"]))                 # call 0: remember the sample
        base = x + flags[0] * (state["saved"] - x)                           # call 1: restart from it
        comb = (w.view(5, *([1] * x.dim())) * E).sum(dim=0)
        a_t, a_p = state["coef"][0], state["coef"][1]
        if self.prediction_type == "v_prediction":
            comb = a_t.sqrt() * comb + (1 - a_t).sqrt() * base
        denom = a_t * (1 - a_p).sqrt() + (a_t * (1 - a_t) * a_p).sqrt()
        out = (a_p / a_t).sqrt() * base - (a_p - a_t) * comb / denom
        return out.to(sample.dtype)

    def fused_step(self, noise: torch.Tensor, sample: torch.Tensor, state: dict, *, guidance_scale: float = 1.0,
                   guidance_rescale: float = 0.0, do_cfg: bool = False) -> torch.Tensor:
        """guidance (noise [2b, ...] = [uncond; text] with do_cfg), the optional rescale and ``step`` in one HIP launch;
        the ring ``E`` and ``saved`` are left as ``step`` would leave them"""
        return _fused("pndm", self, noise, sample, state, guidance_scale, guidance_rescale, do_cfg)


class DPMSolverMultistepSchedulerLite:
    """DPM-Solver++ (2M): the multistep second-order solver in the data-prediction form, midpoint variant, that the model
    card of stabilityai/stable-diffusion-2-1 swaps in (``DPMSolverMultistepScheduler``), on exactly DDIMSchedulerLite's grid:
    scaled-linear betas, "leading" spacing with steps_offset 1, ``prev = t - ratio``, ``alphas_cumprod[0]`` past the end;
    epsilon or v-prediction; N inference steps are N U-Net calls.  With alpha = sqrt(a), sigma = sqrt(1 - a),
    lambda = log(alpha / sigma), a step from s to t has h = lambda_t - lambda_s, A = alpha_t (1 - exp(-h)) and
        first order    x_t = (sigma_t / sigma_s) x + A x0_s                                        (this is DDIM, eta = 0)
        second order   x_t = (sigma_t / sigma_s) x + A (1 + 1 / (2 r)) x0_s - A / (2 r) x0_s',     r = (lambda_s - lambda_s') / h
    where s' is the step before s and x0 the data prediction (``DDIMSchedulerLite.step_coef``'s statements).  Call 0 is first
    order, every call with ``solver_order=1``, the last one with ``lower_order_final`` and N < 15, and the last one with
    ``final_sigma="zero"``, which takes it to a_prev = 1 where the update returns the predicted x0 (``"alpha0"``, the default,
    ends at ``alphas_cumprod[0]`` like DDIM).  Other spacings and Karras sigmas are not built.
    ``algorithm_type="sde-dpmsolver++"`` is the stochastic variant (diffusers 0.23.1, midpoint) on the same grid and history
    rule: with A2 = alpha_t (1 - exp(-2h)) the row is c_x = (sigma_t / sigma_s) exp(-h), c_0 = A2 (first order) or
    A2 (1 + 1 / (2 r)), c_1 = 0 or -A2 / (2 r), and sigma_t sqrt(1 - exp(-2h)) z is added (``noise_coef`` per call, 0 on a
    ``final_sigma="zero"`` last call; ``noise_table`` in fp64); z comes from the project's seeded device stream
    (ops.add_noise: seed of the sample, draw i + 1 at call i), one more launch after the update.
    PARITY PIN: diffusers is absent, so this is restated from the published algorithm (Lu et al., "DPM-Solver++: Fast Solver
    for Guided Sampling of Diffusion Probabilistic Models", 2022, Algorithm 2; diffusers'
    ``multistep_dpm_solver_second_order_update``) -- unpinned against a live run; tests pin order 1 against
    DDIMSchedulerLite, order 2 against a plain-Python restatement with explicit history lists, and the table's order of
    convergence against an exact probability-flow solution.
    Graph-friendly form: ``set_timesteps`` evaluates everything above in fp64 on the host into a per-call table
    ``[alpha_s, sigma_s, c_x, c_0, c_1, 0]`` (``table``, fp64, CPU; ``coef`` is its fp32 device copy), and a step is
    ``out = (c_x x + c_0 x0) + c_1 prev; prev <- x0`` with the row copied into a static buffer, so one captured step serves
    every call and every N.  ``prev`` starts zero-filled: c_1 = 0 on call 0, and 0 * NaN is NaN."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 prediction_type: str = "v_prediction", steps_offset: int = 1, solver_order: int = 2,
                 lower_order_final: bool = True, final_sigma: str = "alpha0", algorithm_type: str = "dpmsolver++"):
        if algorithm_type not in ("dpmsolver++", "sde-dpmsolver++"):
            raise ValueError(f"algorithm_type must be 'dpmsolver++' or 'sde-dpmsolver++', got {algorithm_type!r}")
        self.algorithm_type = algorithm_type
        if solver_order not in (1, 2):
            raise ValueError(f"solver_order must be 1 or 2, got {solver_order!r}")
        if final_sigma not in ("alpha0", "zero"):
            raise ValueError(f"final_sigma must be 'alpha0' or 'zero', got {final_sigma!r}")
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = self.alphas_cumprod[0]
        self.num_train_timesteps = num_train_timesteps
        self.prediction_type = prediction_type
        self.steps_offset = steps_offset
        self.solver_order = solver_order
        self.lower_order_final = lower_order_final
        self.final_sigma = final_sigma
        self.init_noise_sigma = 1.0
        self.timesteps = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        import math
        N = num_inference_steps
        ratio = self.num_train_timesteps // N
        ts = (torch.arange(0, N) * ratio).round().flip(0).long() + self.steps_offset
        self.num_inference_steps = N
        self.timesteps = ts.to(device) if device is not None else ts
        acp = self.alphas_cumprod.double()

        def lam(a):
            return 0.5 * math.log(a / (1.0 - a))

        rows, a_before = [], None                          # a_before: alphas_cumprod of the step before this one (s')
        noise = []
        for i in range(N):
            t = int(ts[i])
            a_s = float(acp[t])
            a_t = float(acp[t - ratio]) if t - ratio >= 0 else float(acp[0])
            al_s, sg_s = math.sqrt(a_s), math.sqrt(1.0 - a_s)
            last = i == N - 1
            if last and self.final_sigma == "zero":
                rows.append([al_s, sg_s, 0.0, 1.0, 0.0, 0.0])
                noise.append(0.0)
            else:
                h = lam(a_t) - lam(a_s)
                A = math.sqrt(a_t) * -math.expm1(-h)
                c_x = math.sqrt(1.0 - a_t) / sg_s
                if self.stochastic:
                    A = math.sqrt(a_t) * -math.expm1(-2.0 * h)
                    c_x = c_x * math.exp(-h)
                    noise.append(math.sqrt(1.0 - a_t) * math.sqrt(-math.expm1(-2.0 * h)))
                else:
                    noise.append(0.0)
                first = i == 0 or self.solver_order == 1 or (last and self.lower_order_final and N < 15)
                if first:
                    c0, c1 = A, 0.0
                else:
                    r = (lam(a_s) - lam(a_before)) / h
                    c0, c1 = A * (1.0 + 0.5 / r), -A * 0.5 / r
                rows.append([al_s, sg_s, c_x, c0, c1, 0.0])
            a_before = a_s
        self.table = torch.tensor(rows, dtype=torch.float64)
        self.coef = self.table.float()
        self.noise_table = torch.tensor(noise, dtype=torch.float64)
        self.noise_coef = self.noise_table.float()
        self.draws = torch.arange(1, N + 1, dtype=torch.int64)
        if device is not None:
            self.coef, self.noise_coef, self.draws = self.coef.to(device), self.noise_coef.to(device), self.draws.to(device)
        return self.timesteps

    @property
    def stochastic(self) -> bool:
        return self.algorithm_type == "sde-dpmsolver++"

    def n_model_calls(self) -> int:
        return self.num_inference_steps

    def make_state(self, latents: torch.Tensor, seeds=None) -> dict:
        state = {"coef": self.coef[0].clone(), "prev": torch.zeros_like(latents, dtype=torch.float32)}
        return _noise_state(self, state, latents, seeds) if self.stochastic else state

    def load_step(self, state: dict, i: int):
        state["coef"].copy_(self.coef[i])
        if self.stochastic:
            _load_noise_step(self, state, i)

    def step(self, model_output: torch.Tensor, sample: torch.Tensor, state: dict, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``noise``: an explicit z for the stochastic form instead of the device stream (plain torch, any device)"""
        c = state["coef"]
        x, g = sample.float(), model_output.float()
        if self.prediction_type == "v_prediction":
            x0 = c[0] * x - c[1] * g
        else:
            x0 = (x - c[1] * g) / c[0]
        out = (c[2] * x + c[3] * x0) + c[4] * state["prev"]
        state["prev"].copy_(x0)
        if self.stochastic:
            out = _add_noise(out, state, noise)
        return out.to(sample.dtype)

    def fused_step(self, noise: torch.Tensor, sample: torch.Tensor, state: dict, *, guidance_scale: float = 1.0,
                   guidance_rescale: float = 0.0, do_cfg: bool = False) -> torch.Tensor:
        """guidance (noise [2b, ...] = [uncond; text] with do_cfg), the optional rescale and ``step`` in one HIP launch;
        ``prev`` is left as ``step`` would leave it"""
        out = _fused("dpmpp", self, noise, sample, state, guidance_scale, guidance_rescale, do_cfg)
        return _add_noise(out, state, None) if self.stochastic else out


@dataclass
class PipelineOutput:
    latents: torch.Tensor
    arch_indices: Optional[torch.Tensor]
    arch_vectors_quantized: Optional[torch.Tensor]
    resource_ratios: Optional[torch.Tensor] = None
    images: Optional[object] = None      # decoded images for output_type "pt" / "np" / "pil" (None for "latent")


@dataclass
class DispatchOutput(PipelineOutput):
    """PipelineOutput of ExpertDispatchLoop: the parent's fields (latents / images in the caller's prompt order) plus the groups
    the batch ran as"""
    groups: Optional[list] = None        # [(expert index, row indices, bucket size, graph_was_reused)]
    lanes: Optional[list] = None         # the stream lane every entry of ``groups`` ran on, in that order (None: built with lanes=1)


class PruningDenoiseLoop:
    def __init__(self, unet, hyper_net=None, quantizer=None, scheduler=None, vae=None, text_encoder=None,
                 prompt_encoder=None):
        self.unet, self.hyper_net, self.quantizer = unet, hyper_net, quantizer
        self.vae = vae                   # diffusion_pruning_amd.vae.AutoencoderKL: decodes for output_type != "latent"
        self.text_encoder = text_encoder  # diffusion_pruning_amd.text_encoder.CLIPTextModel: encodes prompt_ids
        self.prompt_encoder = prompt_encoder  # diffusion_pruning_amd.prompt_encoder.MPNetModel: encodes router_ids
        self.scheduler = scheduler or DDIMSchedulerLite()
        self._graph = None
        self._graph_key = None

    @torch.no_grad()
    def route(self, hyper_net_input: torch.Tensor):
        """pruning_pipelines.py:746-759: hyper_net -> quantizer (eval: cosine assignment, hard code) -> split -> set"""
        self.hyper_net.eval()
        self.quantizer.eval()
        arch = self.hyper_net(hyper_net_input)
        arch_q, (_, _, idx) = self.quantizer(arch)
        sep = self.hyper_net.transform_structure_vector(arch_q)
        self.unet.set_structure(sep)
        return arch_q, idx

    def _one_step(self, latents, t, state, ctx, guidance_scale, do_cfg, guidance_rescale=0.0, fused_step=False, unet=None):
        x = torch.cat([latents] * 2) if do_cfg else latents                       # pruning_pipelines.py:792
        noise = (self.unet if unet is None else unet)(x, t, ctx, return_dict=False)[0]   # :796-802
        if fused_step:                                                           # :805-814 in one launch
            return self.scheduler.fused_step(noise, latents, state, guidance_scale=guidance_scale,
                                             guidance_rescale=guidance_rescale if do_cfg else 0.0, do_cfg=do_cfg)
        if do_cfg:
            uncond, text = noise.chunk(2)
            noise = uncond + guidance_scale * (text - uncond)                    # :805-807
            if guidance_rescale > 0.0:
                noise = rescale_noise_cfg(noise, text, guidance_rescale)         # :809-811
        return self.scheduler.step(noise, latents, state)                        # :810-814

    @torch.no_grad()
    def __call__(self, prompt_embeds: Optional[torch.Tensor] = None, latents: Optional[torch.Tensor] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, hyper_net_input: Optional[torch.Tensor] = None,
                 negative_prompt_embeds: Optional[torch.Tensor] = None, use_graph: bool = True,
                 output_type: str = "latent", *, prompt_ids: Optional[torch.Tensor] = None,
                 negative_prompt_ids: Optional[torch.Tensor] = None, router_ids: Optional[torch.Tensor] = None,
                 router_attention_mask: Optional[torch.Tensor] = None, guidance_rescale: float = 0.0,
                 fused_step: bool = False, seeds=None, latent_shape=None) -> PipelineOutput:
        """prompt_embeds [B,77,X] (+ negative_prompt_embeds for CFG, concatenated as [uncond, cond] like the
        reference, :765); latents [B,4,h,w] ~ N(0,1) on the device.  output_type "latent" returns the latents only;
        "pt" (fp32 [B,3,H,W] in [0, 1]), "np" (fp32 [B,H,W,3] numpy) and "pil" (list of PIL images) also decode them
        through ``vae`` and postprocess like the reference (:826-839, do_denormalize always true).
        prompt_ids / negative_prompt_ids (int64 [B, L] token ids) instead of the embeddings: encode_prompt (:735-744) on
        ``text_encoder`` -- [negative_prompt_ids; prompt_ids] in ONE encoder call with CFG, prompt_ids alone without --
        then the same loop as with the embeddings.
        router_ids (+ router_attention_mask): the MPNet token ids of the prompts instead of hyper_net_input, which is then
        ``prompt_encoder.encode(router_ids, router_attention_mask)`` (get_mpnet_embeddings, pdm/utils/data_utils.py:130-155).
        guidance_rescale > 0 (with CFG): ``rescale_noise_cfg`` on the guided output (:809-811).  fused_step: guidance, rescale
        and the scheduler update of every step as ONE HIP launch (ops.guided_step) instead of the tensor expressions; both are
        part of the captured step's key, and the defaults leave the step exactly as it was.
        seeds (an int, or one int per prompt) with latent_shape=(4, h, w) instead of latents: the latents are
        ``ops.randn((B,) + latent_shape, seeds, draw=0)`` in fp32, the project's seeded device stream -- prompt i with seed s
        starts from the same latents whichever batch it is in.  A stochastic scheduler (DDIM with eta > 0, SDE-DPM-Solver++)
        needs seeds, with or without latents: call i adds draw i + 1 of every sample's seed, one more launch in the step."""
        prompt_embeds, negative_prompt_embeds, hyper_net_input = self._inputs(
            prompt_embeds, latents, hyper_net_input, negative_prompt_embeds, output_type, prompt_ids, negative_prompt_ids,
            router_ids, router_attention_mask, guidance_scale, seeds, latent_shape)
        latents, seeds = self._noise_source(latents, seeds, latent_shape, prompt_embeds)
        dev = latents.device
        arch_q = idx = None
        if self.hyper_net is not None and hyper_net_input is not None:
            arch_q, idx = self.route(hyper_net_input.to(dev))
        do_cfg = guidance_scale > 1.0 and negative_prompt_embeds is not None
        ehs = torch.cat([negative_prompt_embeds, prompt_embeds]) if do_cfg else prompt_embeds
        ctx = self.unet.precompute_context(ehs.to(dev))                           # cross-attn K/V once per prompt batch
        ts = self.scheduler.set_timesteps(num_inference_steps, device=dev)
        latents = latents * self.scheduler.init_noise_sigma
        B = latents.shape[0] * (2 if do_cfg else 1)
        extra = (float(guidance_rescale), bool(fused_step))
        if not use_graph:
            latents = self._eager(latents, ts, ctx, B, guidance_scale, do_cfg, *extra, seeds=seeds)
        else:
            # one captured step per (scheduler, shapes, CFG, guidance, installed architecture): later calls with the same key
            # (the FID-generation loop: many prompt batches through one expert) only refresh the static buffers
            key = (type(self.scheduler).__name__, self.scheduler.prediction_type, tuple(latents.shape), latents.dtype, do_cfg,
                   float(guidance_scale), str(dev), ctx.key, getattr(self.unet, "_structure_epoch", None)) + extra \
                + (self._stochastic(),)                                           # (a stochastic step has one more node)
            if ctx.key is None or self._graph_key != key:
                self._graph = self._capture(latents, ts, ctx, B, guidance_scale, do_cfg, *extra, seeds=seeds)
                self._graph_key = key if ctx.key is not None else None
            latents = self._replay(self._graph, latents, ts, ctx, B, seeds=seeds)
        ratios = None
        if getattr(self.unet, "resource_info_dict", None) is not None:
            # pruning_pipelines.py:822-824
            ratios = self.unet.calc_macs()["cur_prunable_macs"] / self.unet.resource_info_dict["cur_prunable_macs"]
        images = None
        if output_type != "latent":
            images = self.decode_latents(latents, output_type)
        return PipelineOutput(latents=latents, arch_indices=idx, arch_vectors_quantized=arch_q, resource_ratios=ratios,
                              images=images)

    def _stochastic(self) -> bool:
        return bool(getattr(self.scheduler, "stochastic", False))

    def _state(self, latents, seeds):
        """the scheduler's per-step state; a stochastic one also carries the seeds"""
        return self.scheduler.make_state(latents, seeds) if self._stochastic() else self.scheduler.make_state(latents)

    def _noise_source(self, latents, seeds, latent_shape, prompt_embeds):
        """(latents, seeds as a device int64 [B] tensor or None) of a call whose arguments ``_inputs`` has accepted: the
        latents are drawn here when only seeds were given"""
        if seeds is None:
            return latents, None
        from . import ops
        nB = prompt_embeds.shape[0]
        if latents is not None:
            dev = latents.device
        else:
            dev = next((p.device for p in self.unet.parameters()), prompt_embeds.device) if hasattr(self.unet, "parameters") \
                else prompt_embeds.device
        seeds = ops._seed_tensor(seeds, nB, dev, "seeds")
        if latents is None:
            latents = ops.randn((nB,) + tuple(int(v) for v in latent_shape), seeds, draw=0)
        return latents, seeds

    def _eager(self, latents, ts, ctx, B, guidance_scale, do_cfg, guidance_rescale=0.0, fused_step=False, unet=None, seeds=None):
        state = self._state(latents, seeds)
        for i in range(self.scheduler.n_model_calls()):
            self.scheduler.load_step(state, i)
            latents = self._one_step(latents, ts[i].expand(B), state, ctx, guidance_scale, do_cfg, guidance_rescale, fused_step, unet)
        return latents

    def _replay(self, g, latents, ts, ctx, B, seeds=None):
        """refresh a captured step's static buffers (the seeds of a stochastic scheduler among them) and replay it once per
        model call"""
        g["lat"].copy_(latents)
        g["ctx"].ehs.copy_(ctx.ehs)
        for k_, v_ in ctx.kv.items():
            g["ctx"].kv[k_].copy_(v_)
        for name, t_ in self._state(latents, seeds).items():
            g["state"][name].copy_(t_)
        for i in range(self.scheduler.n_model_calls()):
            g["t"].copy_(ts[i].expand(B))
            self.scheduler.load_step(g["state"], i)
            g["graph"].replay()
            g["lat"].copy_(g["out"])
        return g["lat"].clone()

    def _inputs(self, prompt_embeds, latents, hyper_net_input, negative_prompt_embeds, output_type, prompt_ids, negative_prompt_ids,
                router_ids, router_attention_mask, guidance_scale, seeds=None, latent_shape=None):
        """argument checks of a call, and the encoders: token ids -> text states (one CLIP call for the whole batch), MPNet
        token ids -> the router's input.  Returns (prompt_embeds, negative_prompt_embeds, hyper_net_input)."""
        if router_ids is not None or router_attention_mask is not None:
            if hyper_net_input is not None:
                raise ValueError("give either hyper_net_input or router_ids / router_attention_mask, not both")
            if router_ids is None:
                raise ValueError("router_attention_mask needs router_ids")
            if self.prompt_encoder is None:
                raise ValueError("router_ids need a prompt_encoder (PruningDenoiseLoop(..., prompt_encoder=MPNetModel))")
        if prompt_ids is not None or negative_prompt_ids is not None:
            if prompt_embeds is not None or negative_prompt_embeds is not None:
                raise ValueError("give either prompt_embeds / negative_prompt_embeds or prompt_ids / negative_prompt_ids, not both")
            if prompt_ids is None:
                raise ValueError("negative_prompt_ids needs prompt_ids")
            if self.text_encoder is None:
                raise ValueError("prompt_ids need a text_encoder (PruningDenoiseLoop(..., text_encoder=CLIPTextModel))")
        elif prompt_embeds is None:
            raise ValueError("prompt_embeds or prompt_ids is required")
        if latents is None and seeds is None:
            raise ValueError("latents is required")
        if seeds is not None:
            # exactly one source of noise: latents or seeds; a stochastic scheduler draws its step noise from the seeds either way
            if latents is not None and not self._stochastic():
                raise ValueError("give either latents or seeds, not both (the scheduler is deterministic: seeds would only draw the latents)")
            if latents is None and (latent_shape is None or len(tuple(latent_shape)) != 3 or any(int(v) < 1 for v in latent_shape)):
                raise ValueError(f"seeds without latents need latent_shape=(4, h, w), got {latent_shape!r}")
            n_prompts = (prompt_ids if prompt_ids is not None else prompt_embeds).shape[0]
            if latents is not None and latents.shape[0] != n_prompts:
                raise ValueError(f"{latents.shape[0]} latents for {n_prompts} prompts")
            n_seeds = n_prompts if isinstance(seeds, int) and not isinstance(seeds, bool) else len(seeds)
            if n_seeds != n_prompts:
                raise ValueError(f"{n_seeds} seeds for {n_prompts} prompts")
        elif self._stochastic():
            raise ValueError(f"{type(self.scheduler).__name__} is stochastic here: it needs seeds=")
        if prompt_ids is not None:
            if guidance_scale > 1.0 and negative_prompt_ids is not None:
                if tuple(negative_prompt_ids.shape) != tuple(prompt_ids.shape):
                    raise ValueError(f"negative_prompt_ids {tuple(negative_prompt_ids.shape)} and prompt_ids "
                                     f"{tuple(prompt_ids.shape)} differ in shape")
                e = self.text_encoder(torch.cat([negative_prompt_ids, prompt_ids]))[0]
                negative_prompt_embeds, prompt_embeds = e[:prompt_ids.shape[0]], e[prompt_ids.shape[0]:]
            else:
                prompt_embeds = self.text_encoder(prompt_ids)[0]
        if output_type not in ("latent", "pt", "np", "pil"):
            raise ValueError(f"output_type {output_type!r}: expected 'latent', 'pt', 'np' or 'pil'")
        if output_type != "latent" and self.vae is None:
            raise ValueError(f"output_type {output_type!r} needs a vae (PruningDenoiseLoop(..., vae=AutoencoderKL))")
        if router_ids is not None:
            hyper_net_input = self.prompt_encoder.encode(router_ids, router_attention_mask)
        return prompt_embeds, negative_prompt_embeds, hyper_net_input

    @torch.no_grad()
    def decode_latents(self, latents: torch.Tensor, output_type: str = "pt"):
        """vae.decode(latents / scaling_factor) + postprocess (pruning_pipelines.py:826-839) on the HIP decoder; the
        postprocess runs in the decoder's image epilogue kernel"""
        z = latents / self.vae.config.scaling_factor
        if output_type == "pil":
            from PIL import Image
            u8 = self.vae.decode_images(z, "uint8").cpu().numpy()
            return [Image.fromarray(im) for im in u8]
        img = self.vae.decode_images(z, "pt")
        if output_type == "np":
            return img.permute(0, 2, 3, 1).float().cpu().numpy()
        return img

    def _capture(self, latents, ts, ctx, B, guidance_scale, do_cfg, guidance_rescale=0.0, fused_step=False, unet=None, seeds=None):
        lat_buf = latents.clone()
        t_buf = ts[0].expand(B).clone()
        state = self._state(latents, seeds)
        self.scheduler.load_step(state, 0)
        # warm-up on a side stream (builds packed-weight plans), then capture one step
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._one_step(lat_buf, t_buf, state, ctx, guidance_scale, do_cfg, guidance_rescale, fused_step, unet)
        torch.cuda.current_stream().wait_stream(side)
        from . import graph_utils
        graph = graph_utils.new_graph()            # (torch.cuda.CUDAGraph(); kept inspectable under graph_utils.KEEP_GRAPHS)
        with torch.cuda.graph(graph):
            out = self._one_step(lat_buf, t_buf, state, ctx, guidance_scale, do_cfg, guidance_rescale, fused_step, unet)
        return {"graph": graph, "lat": lat_buf, "t": t_buf, "state": state, "out": out, "ctx": ctx}


def plan_groups(idx_list, group_sizes=(1, 2, 4, 8)):
    """Group the prompts of a routed batch by expert: ``idx_list[i]`` is prompt i's expert index; returns
    ``[(expert, rows, bucket)]`` -- experts in ascending index, the rows of one expert in ascending prompt order, cut into
    chunks of at most the largest bucket, each chunk in the smallest bucket of ``group_sizes`` that holds it.  Every row
    appears exactly once.  Pure host logic, deterministic."""
    sizes = sorted({int(s) for s in group_sizes})
    if not sizes or sizes[0] < 1:
        raise ValueError(f"plan_groups: group_sizes must be positive integers, got {group_sizes!r}")
    by_expert = {}
    for row, e in enumerate(idx_list):
        by_expert.setdefault(int(e), []).append(row)
    groups = []
    for e in sorted(by_expert):
        rows = by_expert[e]
        for s in range(0, len(rows), sizes[-1]):
            chunk = rows[s:s + sizes[-1]]
            groups.append((e, chunk, next(b for b in sizes if b >= len(chunk))))
    return groups


MAX_LANES = 4      # a process opens four hardware queues (HIP's default): a lane beyond that only queues behind another


def plan_lanes(groups, n_lanes, key_of, pinned=None, cost=None):
    """The stream lane of every group of a plan (``plan_groups``' ``(expert, rows, bucket)`` tuples): a list of lane indices
    in ``range(n_lanes)``, one per group, in plan order.  Pure host logic, deterministic.

    Groups with equal ``key_of(group)`` get the same lane -- the chunks of an expert whose rows were cut at the largest bucket
    share one captured step and its static buffers, so they must run in order on one stream.  A key found in ``pinned``
    (``{key: lane}``: a captured step replays only on the lane it was captured for) keeps that lane.  The remaining keys are
    placed longest first on the lane that is least loaded so far; equal costs go by plan order, equal loads to the lowest
    lane.  The cost of a key is the sum of ``cost(bucket)`` over its groups.

    ``cost`` defaults to ``4 + bucket``: a rough relative model read off three per-call times of the U-Net under CFG (4.4 /
    4.8 / 12.1 ms at buckets 1 / 2 / 8).  Nobody has measured it for this purpose.  It steers where time goes, never
    what is computed."""
    n_lanes = int(n_lanes)
    if n_lanes < 1:
        raise ValueError(f"plan_lanes: n_lanes must be at least 1, got {n_lanes}")
    cost = cost or (lambda bucket: 4 + bucket)
    pinned = pinned or {}
    keys = [key_of(g) for g in groups]
    total = {}                                     # key -> summed cost, in order of first appearance
    for g, k in zip(groups, keys):
        total[k] = total.get(k, 0) + cost(g[2])
    load = [0] * n_lanes
    lane_of = {}
    for k, c in total.items():
        if k in pinned:
            lane = int(pinned[k])
            if not 0 <= lane < n_lanes:
                raise ValueError(f"plan_lanes: a key is pinned to lane {lane}, outside range({n_lanes})")
            lane_of[k] = lane
            load[lane] += c
    order = {k: i for i, k in enumerate(total)}
    for k in sorted((k for k in total if k not in lane_of), key=lambda k: (-total[k], order[k])):
        lane = min(range(n_lanes), key=lambda j: (load[j], j))
        lane_of[k] = lane
        load[lane] += total[k]
    return [lane_of[k] for k in keys]


def plan_waves(keys, max_keys):
    """Cut a plan into waves of consecutive groups with at most ``max_keys`` distinct keys each: ``keys[i]`` is group i's key;
    returns lists of group indices.  A wave's captured steps all fit the LRU at once.  Pure host logic."""
    max_keys = int(max_keys)
    if max_keys < 1:
        raise ValueError(f"plan_waves: max_keys must be at least 1, got {max_keys}")
    waves, cur, seen = [], [], set()
    for i, k in enumerate(keys):
        if k not in seen and len(seen) == max_keys:
            waves.append(cur)
            cur, seen = [], set()
        cur.append(i)
        seen.add(k)
    if cur:
        waves.append(cur)
    return waves


def round_robin(queues):
    """The order in which the host issues the work of a wave: ``queues[lane]`` is that lane's groups in plan order, each a list
    of items in order; yields ``(lane, item)``, one item per lane in turn (lanes ascending) until every lane is empty.  Per
    lane the items keep their order across groups.  Pure host logic."""
    flat = [[item for group in lane for item in group] for lane in queues]
    pos = [0] * len(flat)
    left = sum(len(f) for f in flat)
    while left:
        for lane, f in enumerate(flat):
            if pos[lane] < len(f):
                yield lane, f[pos[lane]]
                pos[lane] += 1
                left -= 1


_side_streams = {}     # device index -> (side streams, probe record): chosen once per device and process, shared by every loop


class ExpertDispatchLoop(PruningDenoiseLoop):
    """The routed call of StableDiffusionPruningPipeline (pruning_pipelines.py:746-759: route, ``set_structure``, loop) for a
    batch whose prompts go to MORE than one expert, at each expert's own cost: the batch is routed once, grouped by expert
    (``plan_groups``), and every group runs the whole denoise loop with that expert's hard code installed as a batch-shared
    structure -- the compacted-weight path of the U-Net (gated semantics, exact through the border table) instead of dense
    compute with per-sample gates.  A group is padded to a bucket size of ``group_sizes`` by repeating its last row (samples
    are independent: the padded rows are computed and dropped), so a handful of captured steps serves any split.  Results
    come back in the caller's prompt order.  Every step is the fused one (``fused_step`` of the scheduler).

    lanes=1 (the default): groups run one after another on the current stream.

    lanes in 2..4 (graph path only): groups of different experts run SIDE BY SIDE on stream lanes.  At the small batch of a
    group the forward is a chain of dependent launches that leaves the chip mostly idle, and groups of different experts
    cannot be merged into one chain, so a second chain fills the gaps of the first.  Lane 0 is the caller's current stream,
    lanes 1.. are side streams that a spin-kernel probe found to overlap it and each other
    (``graph_utils.concurrent_streams``; once per device and process, so every loop shares them).  When the probe finds fewer
    than asked for, the loop runs with the lanes it has; ``stream_probe`` says so and ``lane_streams`` holds the streams of the
    last call.  A caller's stream that happens to be the very stream of a side lane only serialises that lane.  How a call
    runs:
      * the prologue is the one of lanes=1 (route, one device-to-host copy, ``plan_groups``, encoders); then every side lane
        waits for the caller's stream;
      * the groups are cut into waves of at most ``max_graphs`` distinct keys (``plan_waves``) and every wave is spread over
        the lanes by ``plan_lanes``; the host synchronises a wave's lanes before the next wave starts;
      * set-up of a wave, serial on the host, each group on its lane's stream and, for lanes >= 1, under
        ``ops.scratch_domain(("dispatch", lane))`` (lane 0 keeps the caller's domain: its graphs are the graphs of lanes=1):
        install, row gathers, ``precompute_context``, look-up or capture.  A group's set-up waits for the previous group's,
        so packs built for one lane are complete before another lane reads them.  All captures of a wave precede its
        replays (``torch.cuda.graph`` synchronises the device).  A captured step records its lane and replays only there for
        as long as it lives -- its scratch belongs to that domain;
      * replay: per group the items [refresh the static buffers, one item per model call, collect the result]; the host
        issues one item per lane in turn (``round_robin``).  Groups of one key share a lane, so a refresh never overtakes the
        previous group's collect.  Every lane replays whole graphs; lanes are never merged into one graph;
      * join: the caller's stream waits for every lane, then scatters the rows back and fills the ratios;
      * a graph is evicted or replaced only after the host has synchronised the lane it ran on.
    Overlapping replays share nothing but what scratch.py hands out per (stream, domain): every other buffer a replay writes
    is in its own graph pool or is one of its static buffers; packs and tables are only read.  The results are those of
    lanes=1 bit for bit; whether lanes save time is a measurement, not a promise.

    experts: ``{index: UNet2DConditionModelPruned | UNet2DConditionModelGated}`` -- fine-tuned experts with weights of their
    own (checkpoint.from_pretrained).  Group e then runs on ``experts[e]`` as it is installed, without ``set_structure``;
    routing still comes from ``hyper_net`` / ``quantizer``; an index the router picks that is missing raises KeyError.

    Captured steps: one per (expert identity, the bytes of its hard code, bucket, scheduler class, prediction type, latent
    shape, dtype, CFG, guidance scale, guidance rescale, device, stochastic or not), in an LRU of at most ``max_graphs`` entries.  A capture
    pins the packed-weight plans it touched in the modules' plan caches until ``invalidate_plans()`` / ``clear()``: evicting
    a graph here does NOT free its packs.  Re-installing a code finds its pinned plans again, so the bound is at most
    ``max_graphs`` pinned plans per module for as long as no more than ``max_graphs`` distinct codes are captured between
    two ``invalidate_plans()``; every further distinct code that is captured pins one more."""

    def __init__(self, unet, hyper_net=None, quantizer=None, scheduler=None, vae=None, text_encoder=None, prompt_encoder=None,
                 experts=None, group_sizes=(1, 2, 4, 8), max_graphs: int = 16, lanes: int = 1):
        super().__init__(unet, hyper_net, quantizer, scheduler, vae, text_encoder, prompt_encoder)
        if not isinstance(lanes, int) or not 1 <= lanes <= MAX_LANES:
            raise ValueError(f"lanes must be an int in 1..{MAX_LANES}, got {lanes!r}")
        self.lanes = lanes
        self.lane_streams = []                     # the streams of the last call with lanes > 1: [caller's, side lanes ...]
        self.stream_probe = None                   # what the choice of the side lanes measured (set by the first such call)
        self.experts = None if experts is None else dict(experts)
        self.group_sizes = tuple(sorted({int(s) for s in group_sizes}))
        if not self.group_sizes or self.group_sizes[0] < 1:
            raise ValueError(f"group_sizes must be positive integers, got {group_sizes!r}")
        if max_graphs < 1:
            raise ValueError(f"max_graphs must be at least 1, got {max_graphs}")
        self.max_graphs = int(max_graphs)
        self._graphs = OrderedDict()               # key -> captured step, least recently used first
        self._installed = None                     # (structure epoch of self.unet, code bytes) this loop installed last

    @torch.no_grad()
    def route_indices(self, hyper_net_input: torch.Tensor):
        """hyper_net -> quantizer (eval) WITHOUT installing anything: (arch_q [B, D] hard codes, idx [B])"""
        self.hyper_net.eval()
        self.quantizer.eval()
        arch_q, (_, _, idx) = self.quantizer(self.hyper_net(hyper_net_input))
        return arch_q, idx

    def _install(self, code_row: torch.Tensor, code: bytes):
        """the expert's code as a batch-shared structure of self.unet (skipped when it is what this loop installed last
        and nobody has installed anything since)"""
        if self._installed == (getattr(self.unet, "_structure_epoch", None), code):
            return
        self.unet.set_structure(self.hyper_net.transform_structure_vector(code_row))
        self._installed = (self.unet._structure_epoch, code)

    @torch.no_grad()
    def __call__(self, prompt_embeds: Optional[torch.Tensor] = None, latents: Optional[torch.Tensor] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, hyper_net_input: Optional[torch.Tensor] = None,
                 negative_prompt_embeds: Optional[torch.Tensor] = None, use_graph: bool = True,
                 output_type: str = "latent", *, prompt_ids: Optional[torch.Tensor] = None,
                 negative_prompt_ids: Optional[torch.Tensor] = None, router_ids: Optional[torch.Tensor] = None,
                 router_attention_mask: Optional[torch.Tensor] = None, guidance_rescale: float = 0.0,
                 fused_step: bool = True, seeds=None, latent_shape=None) -> DispatchOutput:
        """The arguments of PruningDenoiseLoop.__call__; hyper_net_input or router_ids is required (there is nothing to
        dispatch on otherwise), and the step is always the fused one.  Returns latents / images in the caller's prompt order,
        ``arch_indices`` [B], ``resource_ratios`` [B], ``groups`` and, from a loop built with lanes > 1, ``lanes``."""
        if not fused_step:
            raise ValueError("ExpertDispatchLoop runs the fused step only")
        if self.lanes > 1 and not use_graph:
            raise ValueError(f"lanes={self.lanes} needs use_graph=True: the lanes overlap captured steps, eager groups run with lanes=1")
        if self.hyper_net is None or self.quantizer is None:
            raise ValueError("ExpertDispatchLoop needs a hyper_net and a quantizer to route with")
        prompt_embeds, negative_prompt_embeds, hyper_net_input = self._inputs(
            prompt_embeds, latents, hyper_net_input, negative_prompt_embeds, output_type, prompt_ids, negative_prompt_ids,
            router_ids, router_attention_mask, guidance_scale, seeds, latent_shape)
        if hyper_net_input is None:
            raise ValueError("ExpertDispatchLoop needs hyper_net_input or router_ids")
        latents, seeds = self._noise_source(latents, seeds, latent_shape, prompt_embeds)
        dev = latents.device
        nB = latents.shape[0]
        arch_q, idx = self.route_indices(hyper_net_input.to(dev))
        # ONE device-to-host copy: the indices and the hard codes (a byte per entry) together
        host = torch.cat([idx.to(torch.int16).view(torch.uint8).reshape(nB, 2), (arch_q >= 0.5).to(torch.uint8)], dim=1).cpu()
        idx_list = host[:, :2].contiguous().view(torch.int16).reshape(nB).tolist()
        codes = [bytes(host[i, 2:].tolist()) for i in range(nB)]
        groups = plan_groups(idx_list, self.group_sizes)
        if self.experts is not None:
            for e, _, _ in groups:
                if e not in self.experts:
                    raise KeyError(f"the router picked expert {e}, which is not in experts ({sorted(self.experts)})")
        do_cfg = guidance_scale > 1.0 and negative_prompt_embeds is not None
        prompt_embeds = prompt_embeds.to(dev)
        if do_cfg:
            negative_prompt_embeds = negative_prompt_embeds.to(dev)
        ts = self.scheduler.set_timesteps(num_inference_steps, device=dev)
        latents = latents * self.scheduler.init_noise_sigma
        out = torch.empty_like(latents)
        ratios = None
        report = []
        rescale = float(guidance_rescale) if do_cfg else 0.0
        if self.lanes > 1:
            report, lane_of, ratios = self._run_lanes(groups, codes, arch_q, latents, seeds, prompt_embeds, negative_prompt_embeds, ts,
                                                      out, do_cfg, guidance_scale, rescale)
            images = self.decode_latents(out, output_type) if output_type != "latent" else None
            return DispatchOutput(latents=out, arch_indices=idx, arch_vectors_quantized=arch_q, resource_ratios=ratios,
                                  images=images, groups=report, lanes=lane_of)
        for e, rows, bucket in groups:
            code = codes[rows[0]]
            assert all(codes[r] == code for r in rows), f"rows {rows} of expert {e} carry different codes"
            if self.experts is not None:
                model = self.experts[e]
            else:
                model = self.unet
                self._install(arch_q[rows[0]:rows[0] + 1], code)
            rows_t = torch.tensor(rows, dtype=torch.long, device=dev)
            take = torch.tensor(rows + [rows[-1]] * (bucket - len(rows)), dtype=torch.long, device=dev)
            lat_g = latents.index_select(0, take)
            seeds_g = None if seeds is None else seeds.index_select(0, take)      # (a padded row repeats its source row's seed)
            ehs = prompt_embeds.index_select(0, take)
            if do_cfg:
                ehs = torch.cat([negative_prompt_embeds.index_select(0, take), ehs])
            ctx = model.precompute_context(ehs)                                   # after the install: K/V packs are per structure
            Bm = bucket * (2 if do_cfg else 1)
            reused = False
            if not use_graph:
                res = self._eager(lat_g, ts, ctx, Bm, guidance_scale, do_cfg, rescale, True, model, seeds_g)
            else:
                key = (e, id(model), code, bucket, type(self.scheduler).__name__, self.scheduler.prediction_type,
                       tuple(lat_g.shape), lat_g.dtype, do_cfg, float(guidance_scale), rescale, str(dev), self._stochastic())
                g = self._graphs.get(key)
                reused = g is not None and ctx.key is not None and g["ctx"].key == ctx.key
                if not reused:
                    self._graphs.pop(key, None)
                    while len(self._graphs) >= self.max_graphs:
                        self._graphs.popitem(last=False)
                    g = self._capture(lat_g, ts, ctx, Bm, guidance_scale, do_cfg, rescale, True, model, seeds_g)
                    if ctx.key is not None:
                        self._graphs[key] = g
                else:
                    self._graphs.move_to_end(key)
                res = self._replay(g, lat_g, ts, ctx, Bm, seeds_g)
            out.index_copy_(0, rows_t, res[:len(rows)].to(out.dtype))
            if getattr(model, "resource_info_dict", None) is not None:
                # pruning_pipelines.py:822-824, per group
                r = model.calc_macs()["cur_prunable_macs"] / model.resource_info_dict["cur_prunable_macs"]
                if ratios is None:
                    ratios = torch.zeros(nB, dtype=torch.float32, device=dev)
                ratios.index_copy_(0, rows_t, torch.as_tensor(r, dtype=torch.float32, device=dev).reshape(-1)[:1].expand(len(rows)))
            report.append((e, list(rows), bucket, reused))
        images = None
        if output_type != "latent":
            images = self.decode_latents(out, output_type)
        return DispatchOutput(latents=out, arch_indices=idx, arch_vectors_quantized=arch_q, resource_ratios=ratios,
                              images=images, groups=report)

    # ---- lanes > 1 -----------------------------------------------------------------------------------------------------------
    def _lane_streams(self, dev):
        """[the caller's current stream, side lanes ...] of this call; the side lanes are probed for on the first call per
        device and process (always for MAX_LANES, a loop takes the first ``lanes - 1``)"""
        from . import graph_utils
        caller = torch.cuda.current_stream(dev)
        ent = _side_streams.get(caller.device.index)
        if ent is None:
            log = []
            sides = graph_utils.concurrent_streams(MAX_LANES, caller, log=log)
            ent = _side_streams[caller.device.index] = (sides, log[0])
        sides = ent[0][:self.lanes - 1]
        self.lane_streams = [caller] + sides
        self.stream_probe = dict(ent[1], lanes_asked=self.lanes, lanes_effective=len(self.lane_streams))
        return self.lane_streams

    def _replay_items(self, g, latents, ts, ctx, B, seeds, sink, caller):
        """``_replay`` cut into the items a lane issues one at a time -- the same launches in the same order: refresh the
        static buffers, one item per model call, collect (the result goes to ``sink``; the caller's stream will read it)"""
        def refresh():
            g["lat"].copy_(latents)
            g["ctx"].ehs.copy_(ctx.ehs)
            for k_, v_ in ctx.kv.items():
                g["ctx"].kv[k_].copy_(v_)
            for name, t_ in self._state(latents, seeds).items():
                g["state"][name].copy_(t_)

        def call(i):
            def item():
                g["t"].copy_(ts[i].expand(B))
                self.scheduler.load_step(g["state"], i)
                g["graph"].replay()
                g["lat"].copy_(g["out"])
            return item

        def collect():
            res = g["lat"].clone()
            res.record_stream(caller)
            sink(res)
        return [refresh] + [call(i) for i in range(self.scheduler.n_model_calls())] + [collect]

    def _run_lanes(self, groups, codes, arch_q, latents, seeds, prompt_embeds, negative_prompt_embeds, ts, out, do_cfg,
                   guidance_scale, rescale):
        """the groups of a routed batch on stream lanes (class docstring); fills ``out`` on the caller's stream and returns
        (groups report, lane of every group, resource ratios)"""
        from . import ops
        dev = latents.device
        nB = latents.shape[0]
        streams = self._lane_streams(dev)
        caller = streams[0]
        for s in streams[1:]:
            s.wait_stream(caller)

        def model_of(e):
            return self.unet if self.experts is None else self.experts[e]

        def key_of(group):
            e, rows, bucket = group
            return (e, id(model_of(e)), codes[rows[0]], bucket, type(self.scheduler).__name__, self.scheduler.prediction_type,
                    (bucket,) + tuple(latents.shape[1:]), latents.dtype, do_cfg, float(guidance_scale), rescale, str(dev),
                    self._stochastic())
        keys = [key_of(grp) for grp in groups]
        results, model_ratio = [None] * len(groups), [None] * len(groups)
        lane_of, reused_of = [None] * len(groups), [False] * len(groups)
        used = []
        for wave in plan_waves(keys, self.max_graphs):
            for s in used:
                s.synchronize()                    # the previous wave is done: its graphs may be evicted or replaced
            wave_keys = {keys[i] for i in wave}
            pinned = {k: self._graphs[k]["lane"] for k in wave_keys if k in self._graphs}
            plan = plan_lanes([groups[i] for i in wave], len(streams), key_of, pinned)
            queues = [[] for _ in streams]
            prev = None
            for i, lane in zip(wave, plan):
                e, rows, bucket = groups[i]
                stream = streams[lane]
                if prev is not None and prev is not stream:
                    stream.wait_stream(prev)       # set-up is in plan order on the device too: packs are built before they are read
                prev = stream
                with torch.cuda.stream(stream), (ops.scratch_domain(("dispatch", lane)) if lane else contextlib.nullcontext()):
                    code = codes[rows[0]]
                    assert all(codes[r] == code for r in rows), f"rows {rows} of expert {e} carry different codes"
                    model = model_of(e)
                    if self.experts is None:
                        self._install(arch_q[rows[0]:rows[0] + 1], code)
                    take = torch.tensor(rows + [rows[-1]] * (bucket - len(rows)), dtype=torch.long, device=dev)
                    lat_g = latents.index_select(0, take)
                    seeds_g = None if seeds is None else seeds.index_select(0, take)
                    ehs = prompt_embeds.index_select(0, take)
                    if do_cfg:
                        ehs = torch.cat([negative_prompt_embeds.index_select(0, take), ehs])
                    ctx = model.precompute_context(ehs)
                    Bm = bucket * (2 if do_cfg else 1)
                    g = self._graphs.get(keys[i])
                    reused = g is not None and ctx.key is not None and g["ctx"].key == ctx.key
                    if not reused:
                        # room is made before the capture; what leaves is no key of this wave (least recently used first) and is
                        # released only once the host has synchronised the lane it ran on
                        leaving = [self._graphs.pop(keys[i], None)]
                        while len(self._graphs) >= self.max_graphs:
                            leaving.append(self._graphs.pop(next(k for k in self._graphs if k not in wave_keys)))
                        for lane_ in {old["lane"] for old in leaving if old is not None}:
                            streams[lane_].synchronize()
                        g = None
                        del leaving
                        g = self._capture(lat_g, ts, ctx, Bm, guidance_scale, do_cfg, rescale, True, model, seeds_g)
                        g["lane"] = lane
                        if ctx.key is not None:
                            self._graphs[keys[i]] = g
                    else:
                        self._graphs.move_to_end(keys[i])
                    if getattr(model, "resource_info_dict", None) is not None:
                        # pruning_pipelines.py:822-824, per group, while the group's code is the installed one
                        model_ratio[i] = model.calc_macs()["cur_prunable_macs"] / model.resource_info_dict["cur_prunable_macs"]

                    def sink(res, i=i):
                        results[i] = res
                    queues[lane].append(self._replay_items(g, lat_g, ts, ctx, Bm, seeds_g, sink, caller))
                lane_of[i], reused_of[i] = lane, reused
            for lane, item in round_robin(queues):
                with torch.cuda.stream(streams[lane]):
                    item()
            used = [streams[lane] for lane in sorted(set(plan))]
        for s in streams[1:]:
            caller.wait_stream(s)
        ratios = None
        report = []
        for i, (e, rows, bucket) in enumerate(groups):
            rows_t = torch.tensor(rows, dtype=torch.long, device=dev)
            out.index_copy_(0, rows_t, results[i][:len(rows)].to(out.dtype))
            r = model_ratio[i]
            if r is not None:
                if ratios is None:
                    ratios = torch.zeros(nB, dtype=torch.float32, device=dev)
                if torch.is_tensor(r) and r.is_cuda:
                    r.record_stream(caller)
                ratios.index_copy_(0, rows_t, torch.as_tensor(r, dtype=torch.float32, device=dev).reshape(-1)[:1].expand(len(rows)))
            report.append((e, list(rows), bucket, reused_of[i]))
        return report, lane_of, ratios
