"""The stochastic forms of pipeline.DDIMSchedulerLite (eta > 0) and DPMSolverMultistepSchedulerLite ("sde-dpmsolver++") on the
host, through ``step(..., noise=z)`` with an explicit z: the deterministic defaults are bit for bit what they were, the tables keep
the marginal variance, the steps match plain-Python fp64 restatements with explicit history lists, and the loops refuse calls
without exactly one source of noise.

Tolerance of the fp32 runs: the rule of tests/test_dpm_solver_host.py, ``e <= 2 amp e_ddim + 1e-7`` in rel-L2, with e_ddim the
existing deterministic DDIM's own fp32 error on the same grid and model and amp = max (|c_0| + |c_1|) / |c_0 + c_1| of the table
(1 for DDIM)."""
import math

import pytest
import torch

from diffusion_pruning_amd import pipeline as P
from tests.test_dpm_solver_host import SHAPE, e_ddim, grid, rel_l2, stub, x0_of, x_T


def noises(N, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(SHAPE, generator=g) for _ in range(N)]


# ---- the deterministic defaults are untouched -----------------------------------------------------------------------------------
def parent_ddim_coef(sch, N):
    ratio = sch.num_train_timesteps // N
    ts = (torch.arange(0, N) * ratio).round().flip(0).long() + sch.steps_offset
    prev = ts - ratio
    a_t = sch.alphas_cumprod[ts]
    a_prev = torch.where(prev >= 0, sch.alphas_cumprod[prev.clamp(min=0)], sch.final_alpha_cumprod)
    return torch.stack([a_t.sqrt(), (1 - a_t).sqrt(), a_prev.sqrt(), (1 - a_prev).sqrt()], dim=1)


def parent_dpm_table(sch, N):
    """the table as the deterministic solver has always built it"""
    acp = sch.alphas_cumprod.double()

    def lam(a):
        return 0.5 * math.log(a / (1.0 - a))
    rows, a_before = [], None
    for i, (t, prev) in enumerate(grid(N)):
        a_s = float(acp[t])
        a_t = float(acp[prev]) if prev >= 0 else float(acp[0])
        al_s, sg_s = math.sqrt(a_s), math.sqrt(1.0 - a_s)
        last = i == N - 1
        if last and sch.final_sigma == "zero":
            rows.append([al_s, sg_s, 0.0, 1.0, 0.0, 0.0])
        else:
            h = lam(a_t) - lam(a_s)
            A = math.sqrt(a_t) * -math.expm1(-h)
            if i == 0 or sch.solver_order == 1 or (last and sch.lower_order_final and N < 15):
                c0, c1 = A, 0.0
            else:
                r = (lam(a_s) - lam(a_before)) / h
                c0, c1 = A * (1.0 + 0.5 / r), -A * 0.5 / r
            rows.append([al_s, sg_s, math.sqrt(1.0 - a_t) / sg_s, c0, c1, 0.0])
        a_before = a_s
    return torch.tensor(rows, dtype=torch.float64)


@pytest.mark.parametrize("N", [1, 5, 20, 50])
def test_the_deterministic_defaults_keep_their_tables_and_states(N):
    lat = torch.randn(2, 4, 3, 3)
    for sch in (P.DDIMSchedulerLite(), P.DDIMSchedulerLite(eta=0.0, prediction_type="epsilon")):
        sch.set_timesteps(N)
        assert not sch.stochastic and torch.equal(sch.coef, parent_ddim_coef(sch, N)) and sch.coef.dtype == torch.float32
        assert sch.noise_coef.shape == (N,) and not sch.noise_coef.any()
        assert sorted(sch.make_state(lat)) == ["coef"] and sorted(sch.make_state(lat, seeds=[1, 2])) == ["coef"]
    for fs in ("alpha0", "zero"):
        sch = P.DPMSolverMultistepSchedulerLite(final_sigma=fs)
        sch.set_timesteps(N)
        assert sch.algorithm_type == "dpmsolver++" and not sch.stochastic
        assert torch.equal(sch.table, parent_dpm_table(sch, N)) and torch.equal(sch.coef, sch.table.float())
        assert sch.noise_coef.shape == (N,) and not sch.noise_coef.any()
        assert sorted(sch.make_state(lat)) == ["coef", "prev"]
    assert not hasattr(P.PNDMSchedulerLite(), "stochastic")
    with pytest.raises(ValueError):
        P.DPMSolverMultistepSchedulerLite(algorithm_type="sde-dpmsolver")
    with pytest.raises(ValueError):
        P.DDIMSchedulerLite(eta=-0.1)


def test_the_deterministic_step_is_unchanged():
    x, g = x_T(1), x_T(2)
    for sch in (P.DDIMSchedulerLite(), P.DPMSolverMultistepSchedulerLite()):
        sch.set_timesteps(5)
        state = sch.make_state(x)
        sch.load_step(state, 2)
        c = state["coef"]
        x0 = c[0] * x - c[1] * g
        want = c[2] * x0 + c[3] * (c[0] * g + c[1] * x) if isinstance(sch, P.DDIMSchedulerLite) else (c[2] * x + c[3] * x0) + c[4] * 0
        assert torch.equal(sch.step(g, x, state), want)


# ---- the stochastic tables --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 20, 50])
@pytest.mark.parametrize("eta", [0.3, 1.0])
def test_ddim_eta_keeps_the_marginal_variance(N, eta):
    sch = P.DDIMSchedulerLite(eta=eta)
    sch.set_timesteps(N)
    acp = sch.alphas_cumprod.double()
    assert sch.stochastic and sch.table.dtype == torch.float64 and sch.noise_table.dtype == torch.float64
    assert torch.equal(sch.coef, sch.table.float()) and torch.equal(sch.noise_coef, sch.noise_table.float())
    assert float((sch.table[:, :3] - parent_ddim_coef(sch, N)[:, :3].double()).abs().max()) < 1e-7        # DDIM's grid
    for i, (t, prev) in enumerate(grid(N)):
        a_t, a_p = float(acp[t]), float(acp[prev]) if prev >= 0 else float(acp[0])
        std = eta * math.sqrt((1 - a_p) / (1 - a_t) * (1 - a_t / a_p))
        assert abs(float(sch.noise_table[i]) - std) <= 1e-12 and std > 0
        assert abs(float(sch.table[i, 3]) ** 2 + float(sch.noise_table[i]) ** 2 - (1 - a_p)) <= 1e-12


@pytest.mark.parametrize("fs", ["alpha0", "zero"])
@pytest.mark.parametrize("N", [5, 20, 50])
def test_sde_keeps_the_marginal_variance(N, fs):
    sch = P.DPMSolverMultistepSchedulerLite(algorithm_type="sde-dpmsolver++", final_sigma=fs)
    sch.set_timesteps(N)
    acp = sch.alphas_cumprod.double()
    det = P.DPMSolverMultistepSchedulerLite(final_sigma=fs)
    det.set_timesteps(N)
    assert sch.stochastic and sch.table.shape == (N, 6) and torch.equal(sch.table[:, :2], det.table[:, :2])
    assert [float(v) == 0.0 for v in sch.table[:, 4]] == [float(v) == 0.0 for v in det.table[:, 4]]     # the same history rule
    for i, (t, prev) in enumerate(grid(N)):
        a_t = float(acp[prev]) if prev >= 0 else float(acp[0])
        al_s, sg_s, c_x, c_0, c_1, _ = sch.table[i].tolist()
        ns = float(sch.noise_table[i])
        if fs == "zero" and i == N - 1:
            assert (c_x, c_0, c_1, ns) == (0.0, 1.0, 0.0, 0.0)
            continue
        assert abs((c_x * sg_s) ** 2 + ns ** 2 - (1 - a_t)) <= 1e-12
        h = math.log(math.sqrt(a_t / (1 - a_t))) - math.log(al_s / sg_s)
        assert abs((c_0 + c_1) - math.sqrt(a_t) * (1 - math.exp(-2 * h))) <= 1e-12


# ---- the steps against fp64 restatements ------------------------------------------------------------------------------------------
def ddim_eta64(model, x, N, pred, acp, eta, zs):
    """diffusers' DDIMScheduler.step with eta, written out"""
    x = x.double()
    for i, (t, prev) in enumerate(grid(N)):
        a_t = float(acp[t])
        a_p = float(acp[prev]) if prev >= 0 else float(acp[0])
        al, sg = math.sqrt(a_t), math.sqrt(1 - a_t)
        g = model(x, a_t)
        if pred == "v_prediction":
            x0, eps = al * x - sg * g, al * g + sg * x
        else:
            eps = g
            x0 = (x - sg * eps) / al
        var = (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
        std = eta * math.sqrt(var)
        x = math.sqrt(a_p) * x0 + math.sqrt(1 - a_p - std ** 2) * eps + std * zs[i].double()
    return x


def sde64(model, x, N, pred, acp, zs, final_sigma="alpha0", lower_order_final=True):
    """SDE-DPM-Solver++ (2M), midpoint, with explicit history lists, in diffusers' D0 / D1 form:
    x_t = (sigma_t / sigma_s) exp(-h) x + alpha_t (1 - exp(-2h)) D0 + 0.5 alpha_t (1 - exp(-2h)) D1 + sigma_t sqrt(1 - exp(-2h)) z"""
    x = x.double()
    m, lams = [], []
    for i, (t, prev) in enumerate(grid(N)):
        a_s = float(acp[t])
        a_t = float(acp[prev]) if prev >= 0 else float(acp[0])
        last = i == N - 1
        al_s, sg_s = math.sqrt(a_s), math.sqrt(1 - a_s)
        m.append(x0_of(pred, x, model(x, a_s), al_s, sg_s))
        lams.append(math.log(al_s / sg_s))
        if last and final_sigma == "zero":
            x = m[-1]
            continue
        al_t, sg_t = math.sqrt(a_t), math.sqrt(1 - a_t)
        h = math.log(al_t / sg_t) - lams[-1]
        first = i == 0 or (last and lower_order_final and N < 15)
        x = (sg_t / sg_s * math.exp(-h)) * x + al_t * (1 - math.exp(-2.0 * h)) * m[-1] \
            + sg_t * math.sqrt(1.0 - math.exp(-2.0 * h)) * zs[i].double()
        if not first:
            r0 = (lams[-1] - lams[-2]) / h
            x = x + 0.5 * al_t * (1 - math.exp(-2.0 * h)) * ((m[-1] - m[-2]) / r0)
    return x


def run_class(sch, x, N, zs):
    ts = sch.set_timesteps(N)
    state = sch.make_state(x)
    assert sorted(set(state) - {"coef", "prev"}) == ["draw", "noise_scale"]          # no seeds given: none kept
    assert state["noise_scale"].dtype == torch.float32 and state["noise_scale"].shape == (1,)
    assert state["draw"].dtype == torch.int64 and state["draw"].shape == (1,)
    for i in range(sch.n_model_calls()):
        sch.load_step(state, i)
        assert int(state["draw"]) == i + 1 and float(state["noise_scale"]) == float(sch.noise_coef[i])
        x = sch.step(stub(x, float(sch.alphas_cumprod[int(ts[i])])), x, state, noise=zs[i])
    assert x.dtype == torch.float32
    return x


@pytest.mark.parametrize("pred", ["v_prediction", "epsilon"])
@pytest.mark.parametrize("eta", [0.3, 1.0])
@pytest.mark.parametrize("N", [5, 20])
def test_ddim_eta_matches_the_restatement(N, eta, pred):
    sch = P.DDIMSchedulerLite(prediction_type=pred, eta=eta)
    zs = noises(N)
    got = run_class(sch, x_T(), N, zs)
    ref = ddim_eta64(stub, x_T(), N, pred, sch.alphas_cumprod.double(), eta, zs)
    e, e_ref = rel_l2(got, ref), e_ddim(N, pred)
    print(f"N={N} eta={eta} {pred}: e {e:.3e} e_ddim {e_ref:.3e}")
    assert e <= 2 * e_ref + 1e-7, (e, e_ref)
    # the noise matters: another z, another sample
    assert rel_l2(run_class(sch, x_T(), N, noises(N, seed=6)), ref) > 1e-2


@pytest.mark.parametrize("fs", ["alpha0", "zero"])
@pytest.mark.parametrize("pred", ["v_prediction", "epsilon"])
@pytest.mark.parametrize("N", [5, 20])
def test_sde_matches_the_restatement(N, pred, fs):
    sch = P.DPMSolverMultistepSchedulerLite(prediction_type=pred, final_sigma=fs, algorithm_type="sde-dpmsolver++")
    zs = noises(N)
    got = run_class(sch, x_T(), N, zs)
    ref = sde64(stub, x_T(), N, pred, sch.alphas_cumprod.double(), zs, final_sigma=fs)
    # the table itself, in fp64, is the restatement
    x, prev = x_T().double(), torch.zeros(SHAPE, dtype=torch.float64)
    for i, (t, _) in enumerate(grid(N)):
        al, sg, cx, c0, c1, _z = sch.table[i].tolist()
        x0 = x0_of(pred, x, stub(x, float(sch.alphas_cumprod[t])), al, sg)
        x, prev = (cx * x + c0 * x0) + c1 * prev + float(sch.noise_table[i]) * zs[i].double(), x0
    assert rel_l2(x, ref) <= 1e-13
    e, e_ref = rel_l2(got, ref), e_ddim(N, pred)
    amp = float(((sch.table[:, 3].abs() + sch.table[:, 4].abs()) / (sch.table[:, 3] + sch.table[:, 4]).abs()).max())
    print(f"N={N} {pred} {fs}: e {e:.3e} e_ddim {e_ref:.3e} amplification {amp:.3f}")
    assert e <= 2 * amp * e_ref + 1e-7, (e, e_ref, amp)


def test_state_carries_the_seeds_and_step_needs_a_source():
    sch = P.DPMSolverMultistepSchedulerLite(algorithm_type="sde-dpmsolver++")
    sch.set_timesteps(4)
    lat = torch.randn(3, 4, 2, 2)
    state = sch.make_state(lat, seeds=[5, -1, 2 ** 63 - 1])
    assert sorted(state) == ["coef", "draw", "noise_scale", "prev", "seeds"]
    assert state["seeds"].dtype == torch.int64 and state["seeds"].tolist() == [5, -1, 2 ** 63 - 1]
    with pytest.raises(ValueError):
        sch.make_state(lat, seeds=[1, 2])
    with pytest.raises(ValueError, match="seeds"):
        sch.step(lat, lat, sch.make_state(lat))


# ---- the loops refuse before anything runs ----------------------------------------------------------------------------------------
class _NeverUNet:
    def __call__(self, *a, **k):
        raise AssertionError("the U-Net ran")

    def precompute_context(self, *a, **k):
        raise AssertionError("the U-Net ran")


@pytest.mark.parametrize("dispatch", [False, True])
def test_loops_take_exactly_one_source_of_noise(dispatch):
    cls = P.ExpertDispatchLoop if dispatch else P.PruningDenoiseLoop
    emb, lat = torch.randn(3, 77, 8), torch.randn(3, 4, 8, 8)
    extra = {"hyper_net_input": torch.randn(3, 16)} if dispatch else {}

    def make(sch):
        return cls(_NeverUNet(), hyper_net=object(), quantizer=object(), scheduler=sch) if dispatch else cls(_NeverUNet(), scheduler=sch)
    sde = P.DPMSolverMultistepSchedulerLite(algorithm_type="sde-dpmsolver++")
    for sch in (sde, P.DDIMSchedulerLite(eta=0.5)):
        with pytest.raises(ValueError, match="needs seeds"):
            make(sch)(emb, lat, 4, **extra)                                          # stochastic, no seeds
        with pytest.raises(ValueError, match="2 seeds for 3 prompts"):
            make(sch)(emb, lat, 4, seeds=[1, 2], **extra)
    for sch in (P.DDIMSchedulerLite(), P.PNDMSchedulerLite(), P.DPMSolverMultistepSchedulerLite()):
        with pytest.raises(ValueError, match="latents is required"):
            make(sch)(emb, None, 4, **extra)                                         # neither
        with pytest.raises(ValueError, match="either latents or seeds"):
            make(sch)(emb, lat, 4, seeds=[1, 2, 3], **extra)                         # both
        with pytest.raises(ValueError, match="4 seeds for 3 prompts"):
            make(sch)(emb, None, 4, seeds=[1, 2, 3, 4], latent_shape=(4, 8, 8), **extra)
        with pytest.raises(ValueError, match="latent_shape"):
            make(sch)(emb, None, 4, seeds=7, **extra)
        with pytest.raises(ValueError, match="latent_shape"):
            make(sch)(emb, None, 4, seeds=7, latent_shape=(8, 8), **extra)
    with pytest.raises(ValueError, match="latents is required"):
        make(sde)(emb, None, 4, **extra)
