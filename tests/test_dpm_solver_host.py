"""pipeline.DPMSolverMultistepSchedulerLite on the host: DPM-Solver++ (2M) as a per-call coefficient table.

diffusers cannot be imported here, so the class is pinned from four sides: order 1 IS DDIM (an algebraic identity), order 2 against
a plain-Python fp64 restatement with explicit history lists (written in diffusers' D0 / D1 form, not the table's), a constant data
prediction (orders 1 and 2 must agree), and the order of convergence of the fp64 table on a problem with a known exact solution.

Tolerance of the fp32 runs: the project's rule from tests/test_guided_step_gpu.py, ``e <= 2 e_ref + 1e-7`` in rel-L2, where e_ref
is the error of the EXISTING DDIMSchedulerLite's own fp32 ``step`` against an fp64 restatement of DDIM on the same grid and model."""
import math

import pytest
import torch

from diffusion_pruning_amd import pipeline as P

SHAPE = (2, 4, 6, 10)


def rel_l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def stub(x, a_t):
    """a fixed nonlinear stand-in for the U-Net, in the dtype of x"""
    return torch.tanh(x) * math.sqrt(a_t) + 0.1 * x


def x_T(seed=0):
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(seed))


def grid(N, T=1000, offset=1):
    """DDIMSchedulerLite's grid: "leading" spacing; [(t, t - ratio)] from noise to data"""
    ratio = T // N
    return [((N - 1 - i) * ratio + offset, (N - 1 - i) * ratio + offset - ratio) for i in range(N)]


def x0_of(pred, x, g, al, sg):
    return al * x - sg * g if pred == "v_prediction" else (x - sg * g) / al


# ---- fp64 restatements --------------------------------------------------------------------------------------------------------
def ddim64(model, x, N, pred, acp):
    """DDIM, eta = 0, written out: x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev) eps"""
    x = x.double()
    for t, prev in grid(N):
        a_t = float(acp[t])
        a_p = float(acp[prev]) if prev >= 0 else float(acp[0])
        al, sg = math.sqrt(a_t), math.sqrt(1 - a_t)
        g = model(x, a_t)
        if pred == "v_prediction":
            x0, eps = al * x - sg * g, al * g + sg * x
        else:
            eps = g
            x0 = (x - sg * eps) / al
        x = math.sqrt(a_p) * x0 + math.sqrt(1 - a_p) * eps
    return x


def dpm64(model, x, N, pred, acp, order=2, lower_order_final=True, final_sigma="alpha0"):
    """DPM-Solver++ (2M), Lu et al. 2022, Algorithm 2, with explicit history lists and in diffusers' form
    x_t = (sigma_t / sigma_s) x - alpha_t (exp(-h) - 1) D0 - 0.5 alpha_t (exp(-h) - 1) D1,  D0 = m0,  D1 = (m0 - m1) / r0.
    model(x, a_s, i) -> the network's output at call i"""
    x = x.double()
    m, lams = [], []                                      # data predictions and half-log-SNRs of the calls so far
    for i, (t, prev) in enumerate(grid(N)):
        a_s = float(acp[t])
        a_t = float(acp[prev]) if prev >= 0 else float(acp[0])
        last = i == N - 1
        if last and final_sigma == "zero":
            a_t = 1.0
        al_s, sg_s = math.sqrt(a_s), math.sqrt(1 - a_s)
        m.append(x0_of(pred, x, model(x, a_s, i), al_s, sg_s))
        lams.append(math.log(al_s / sg_s))
        if a_t == 1.0:
            x = m[-1]                                     # sigma_t = 0, alpha_t = 1, exp(-h) = 0
            continue
        al_t, sg_t = math.sqrt(a_t), math.sqrt(1 - a_t)
        h = math.log(al_t / sg_t) - lams[-1]
        first = i == 0 or order == 1 or (last and lower_order_final and N < 15)
        x = (sg_t / sg_s) * x - al_t * (math.exp(-h) - 1.0) * m[-1]
        if not first:
            r0 = (lams[-1] - lams[-2]) / h
            x = x - 0.5 * al_t * (math.exp(-h) - 1.0) * ((m[-1] - m[-2]) / r0)
    return x


# ---- the classes through their own step, fp32 ---------------------------------------------------------------------------------
def run_class(sch, model, x, N):
    ts = sch.set_timesteps(N)
    state = sch.make_state(x)
    acp = sch.alphas_cumprod
    for i in range(sch.n_model_calls()):
        sch.load_step(state, i)
        x = sch.step(model(x, float(acp[int(ts[i])]), i), x, state)
    assert x.dtype == torch.float32
    return x


_E_DDIM = {}


def e_ddim(N, pred):
    """the existing class's own fp32 error against the fp64 restatement (computed once per case)"""
    if (N, pred) not in _E_DDIM:
        sch = P.DDIMSchedulerLite(prediction_type=pred)
        got = run_class(sch, lambda x, a, i: stub(x, a), x_T(), N)
        _E_DDIM[(N, pred)] = rel_l2(got, ddim64(stub, x_T(), N, pred, sch.alphas_cumprod.double()))
    return _E_DDIM[(N, pred)]


@pytest.mark.parametrize("pred", ["v_prediction", "epsilon"])
@pytest.mark.parametrize("N", [4, 25])
def test_order_one_is_ddim(N, pred):
    """x_t = (sigma_t / sigma_s) x + alpha_t (1 - exp(-h)) x0 is DDIM's transfer with eps eliminated"""
    sch = P.DPMSolverMultistepSchedulerLite(prediction_type=pred, solver_order=1)
    got = run_class(sch, lambda x, a, i: stub(x, a), x_T(), N)
    acp = sch.alphas_cumprod.double()
    ref = ddim64(stub, x_T(), N, pred, acp)
    # the identity itself, in fp64: the restatement of the solver at order 1 against the restatement of DDIM
    assert rel_l2(dpm64(lambda x, a, i: stub(x, a), x_T(), N, pred, acp, order=1), ref) <= 1e-14
    e_dpm, e_ref = rel_l2(got, ref), e_ddim(N, pred)
    print(f"N={N} {pred}: e_dpm {e_dpm:.3e} e_ddim {e_ref:.3e}")
    assert e_dpm <= 2 * e_ref + 1e-7, (e_dpm, e_ref)


@pytest.mark.parametrize("final_sigma", ["alpha0", "zero"])
@pytest.mark.parametrize("pred", ["v_prediction", "epsilon"])
@pytest.mark.parametrize("N", [4, 20])
def test_order_two_matches_the_restatement(N, pred, final_sigma):
    """N = 4: lower_order_final makes the last step first order; N = 20: it does not.  The rule above against the same e_ddim, with
    e_ddim scaled by the largest (|c_0| + |c_1|) / |c_0 + c_1| = 1 + 1 / r of the table (4.35 at N = 4, 5.10 at N = 20: the grid
    is uniform in t, not in lambda, so r falls well below 1 towards the data end) and no other slack: the second-order
    combination c_0 x0_s + c_1 x0_s' weighs the rounding errors of the two data predictions by |c_0| + |c_1| where DDIM's
    transfer weighs one by |c_0 + c_1|.  That alone breaks the unscaled rule in two cases: N = 20, epsilon, both final_sigma
    values, measure e_dpm 5.9e-7 and 6.0e-7 against 2 e_ddim + 1e-7 = 5.5e-7 (e_ddim 2.3e-7), while the fp64 table agrees with
    the restatement to 1e-13; the other six cases measure 1.9e-7 ... 4.5e-7 against e_ddim 1.0e-7 ... 3.5e-7 and pass unscaled."""
    sch = P.DPMSolverMultistepSchedulerLite(prediction_type=pred, final_sigma=final_sigma)
    got = run_class(sch, lambda x, a, i: stub(x, a), x_T(), N)
    ref = dpm64(lambda x, a, i: stub(x, a), x_T(), N, pred, sch.alphas_cumprod.double(), final_sigma=final_sigma)
    second = [i for i in range(N) if float(sch.table[i, 4]) != 0.0]
    assert second == (list(range(1, N - 1)) if N == 4 or final_sigma == "zero" else list(range(1, N)))
    # the table itself, in fp64, is the restatement
    x, prev = x_T().double(), torch.zeros(SHAPE, dtype=torch.float64)
    for i, (t, _) in enumerate(grid(N)):
        al, sg, cx, c0, c1, _z = sch.table[i].tolist()
        x0 = x0_of(pred, x, stub(x, float(sch.alphas_cumprod[t])), al, sg)
        x, prev = (cx * x + c0 * x0) + c1 * prev, x0
    assert rel_l2(x, ref) <= 1e-13
    e_dpm, e_ref = rel_l2(got, ref), e_ddim(N, pred)
    amp = float(((sch.table[:, 3].abs() + sch.table[:, 4].abs()) / (sch.table[:, 3] + sch.table[:, 4]).abs()).max())
    assert amp >= 1.0
    print(f"N={N} {pred} {final_sigma}: e_dpm {e_dpm:.3e} e_ddim {e_ref:.3e} amplification {amp:.3f}")
    assert e_dpm <= 2 * amp * e_ref + 1e-7, (e_dpm, e_ref, amp)


@pytest.mark.parametrize("pred", ["v_prediction", "epsilon"])
def test_constant_data_prediction_makes_the_orders_agree(pred):
    """the model answers with the output that corresponds to one fixed x0: then x0_s = x0_s', the second-order term cancels, and
    what is left is that c_0 + c_1 and A are rounded separately"""
    N = 20
    target = torch.randn(SHAPE, generator=torch.Generator().manual_seed(7))
    res = []
    for order in (1, 2):
        sch = P.DPMSolverMultistepSchedulerLite(prediction_type=pred, solver_order=order)

        def model(x, a, i):
            al, sg = sch.coef[i, 0], sch.coef[i, 1]
            return (al * x - target) / sg if pred == "v_prediction" else (x - al * target) / sg
        res.append(run_class(sch, model, x_T(), N))
    assert float(sch.table[:, 4].abs().max()) > 0.1                        # (order 2 did take second-order steps)
    e = rel_l2(res[1], res[0])
    print(f"{pred}: order 2 vs order 1 {e:.3e}")
    assert e <= 1e-6


def _gaussian_error(N, order):
    """data ~ N(0, 4 I): the optimal denoiser is x0 = alpha s2 x / (alpha^2 s2 + sigma^2) and the probability-flow solution scales
    x by sqrt(a s2 + 1 - a); the fp64 table, numpy, max-abs error relative to the exact end point"""
    import numpy as np
    s2 = 4.0
    sch = P.DPMSolverMultistepSchedulerLite(solver_order=order)
    ts = sch.set_timesteps(N)
    tab = sch.table.numpy()
    assert tab.dtype == np.float64
    x = np.array([1.3, -0.7, 0.2])
    a_start, a_end = float(sch.alphas_cumprod[int(ts[0])]), float(sch.alphas_cumprod[0])
    exact = x * math.sqrt((a_end * s2 + 1 - a_end) / (a_start * s2 + 1 - a_start))
    prev = np.zeros(3)
    for al, sg, cx, c0, c1, _z in tab:
        x0 = al * s2 * x / (al * al * s2 + sg * sg)
        x, prev = (cx * x + c0 * x0) + c1 * prev, x0
    return float(np.abs(x - exact).max() / np.abs(exact).max())


def test_the_table_is_second_order():
    e1 = {N: _gaussian_error(N, 1) for N in (20, 40)}
    e2 = {N: _gaussian_error(N, 2) for N in (20, 40)}
    print(f"order 1: {e1}, order 2: {e2}; ratios {e2[40] / e1[40]:.3f} {e2[20] / e2[40]:.2f} {e1[20] / e1[40]:.2f}")
    assert e2[40] <= 0.25 * e1[40]
    assert e2[20] / e2[40] >= 2.5
    assert e1[20] / e1[40] <= 2.2


def test_table_form_and_state_interface():
    ddim = P.DDIMSchedulerLite()
    for N in (1, 4, 14, 15, 50):
        for fs in ("alpha0", "zero"):
            sch = P.DPMSolverMultistepSchedulerLite(final_sigma=fs)
            ts = sch.set_timesteps(N)
            assert torch.equal(ts, ddim.set_timesteps(N)) and sch.n_model_calls() == N
            assert sch.table.dtype == torch.float64 and sch.table.device.type == "cpu" and tuple(sch.table.shape) == (N, 6)
            assert sch.coef.dtype == torch.float32 and torch.equal(sch.coef, sch.table.float())
            assert float((sch.table[:, :2] - ddim.coef[:, :2].double()).abs().max()) < 1e-7     # alpha_s, sigma_s of DDIM's grid
            assert float(sch.table[:, 5].abs().max()) == 0.0
            first = [i for i in range(N) if float(sch.table[i, 4]) == 0.0]
            want = {0} | ({N - 1} if fs == "zero" or N < 15 else set())
            assert first == sorted(want), (N, fs, first)
            if fs == "zero":
                assert sch.table[-1, 2:].tolist() == [0.0, 1.0, 0.0, 0.0]
            else:
                assert float(sch.table[-1, 2]) > 0.0
    sch = P.DPMSolverMultistepSchedulerLite(solver_order=1)
    sch.set_timesteps(20)
    assert float(sch.table[:, 4].abs().max()) == 0.0
    sch = P.DPMSolverMultistepSchedulerLite(lower_order_final=False)
    sch.set_timesteps(4)
    assert float(sch.table[-1, 4]) != 0.0
    assert sch.init_noise_sigma == 1.0 and sch.prediction_type == "v_prediction"
    state = sch.make_state(torch.randn(2, 4, 3, 3, dtype=torch.float16))
    assert sorted(state) == ["coef", "prev"] and state["coef"].shape == (6,) and state["coef"].dtype == torch.float32
    assert state["prev"].dtype == torch.float32 and state["prev"].shape == (2, 4, 3, 3) and not state["prev"].any()
    sch.load_step(state, 2)
    assert torch.equal(state["coef"], sch.coef[2])
    with pytest.raises(ValueError):
        P.DPMSolverMultistepSchedulerLite(solver_order=3)
    with pytest.raises(ValueError):
        P.DPMSolverMultistepSchedulerLite(final_sigma="karras")


def test_final_sigma_zero_returns_the_data_prediction():
    sch = P.DPMSolverMultistepSchedulerLite(final_sigma="zero")
    sch.set_timesteps(5)
    x, g = x_T(1), x_T(2)
    state = sch.make_state(x)
    state["prev"].copy_(x_T(3))
    sch.load_step(state, 4)
    out = sch.step(g, x, state)
    assert torch.equal(out, state["prev"]) and torch.equal(out, sch.coef[4, 0] * x - sch.coef[4, 1] * g)


class _StubUNet:
    def __call__(self, x, t, ctx, return_dict=False):
        return (torch.tanh(x * 0.7 + 0.1) + 0.001 * t.view(-1, 1, 1, 1).float() + ctx.mean(dim=(1, 2)).view(-1, 1, 1, 1),)


@pytest.mark.parametrize("do_cfg", [True, False])
def test_the_eager_loop_runs_the_solver_unchanged(do_cfg):
    """PruningDenoiseLoop's eager loop with this scheduler is guidance + ``step`` per call, and equals the fp64 restatement driven
    by the same stub to fp32 accuracy"""
    g = torch.Generator().manual_seed(3)
    b, s, N = 2, 4.0, 6
    sch = P.DPMSolverMultistepSchedulerLite()
    unet = _StubUNet()
    loop = P.PruningDenoiseLoop(unet, scheduler=sch)
    lat0 = torch.randn(b, 4, 6, 10, generator=g)
    ctx = torch.randn(2 * b if do_cfg else b, 77, 8, generator=g)
    B = 2 * b if do_cfg else b
    ts = sch.set_timesteps(N)
    got = loop._eager(lat0, ts, ctx, B, s, do_cfg)

    def model(x, a, i):
        xx = torch.cat([x, x]) if do_cfg else x
        out = unet(xx, ts[i].expand(B), ctx.double())[0]
        if do_cfg:
            u, t = out.chunk(2)
            out = u + s * (t - u)
        return out
    ref = dpm64(model, lat0, N, "v_prediction", sch.alphas_cumprod.double())
    assert got.dtype == torch.float32 and rel_l2(got, ref) < 5e-6


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_step_dpmpp_matches_the_c_header(tmp_path):
    import os
    import subprocess
    from diffusion_pruning_amd import _lib
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aptp_hip.h")
    src, exe = tmp_path / "c.c", tmp_path / "c"
    src.write_text(f'#include <stdio.h>\n#include "{header}"\nint main(void){{printf("%d %d %d\\n", (int)APTP_STEP_DDIM, '
                   f'(int)APTP_STEP_PNDM, (int)APTP_STEP_DPMPP);return 0;}}\n')
    subprocess.run(["cc", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [_lib.STEP_DDIM, _lib.STEP_PNDM, _lib.STEP_DPMPP] == [0, 1, 2]


def test_guided_step_refuses_a_dpm_call_without_its_state():
    """made-up addresses: every refusal returns APTP_EINVAL (-1) with its reason before anything is launched"""
    import ctypes
    from diffusion_pruning_amd import _lib
    lib = _lib.load()

    def params(**kw):
        p = _lib.GuidedStepParams()
        p.noise, p.sample, p.out, p.coef, p.saved = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
        p.n, p.b, p.noise_rows = 240, 2, 4
        p.noise_dtype, p.scheduler, p.prediction, p.do_cfg = _lib.STEP_NOISE_F32, _lib.STEP_DPMPP, _lib.STEP_V_PREDICTION, 1
        p.guidance_scale, p.guidance_rescale = 7.5, 0.0
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def refused(needle, **kw):
        assert lib.aptp_guided_step(ctypes.byref(params(**kw)), None) == -1
        assert needle in lib.aptp_last_error(), lib.aptp_last_error()

    refused(b"DPM-Solver needs", saved=None)
    refused(b"DPM-Solver needs", coef=None)
    refused(b"DPM-Solver needs", saved=0x50002)
    refused(b"DPM-Solver needs", coef=0x40001)
    refused(b"null pointer", out=None)
    refused(b"noise has 6 rows", noise_rows=6)
    refused(b"needs classifier-free guidance", do_cfg=0, noise_rows=2, guidance_rescale=0.7)
    refused(b"n >= 2", n=1, guidance_rescale=0.7)
    for unknown in (3, 5, -1):
        refused(b"unknown scheduler", scheduler=unknown)
