"""Host checks of the router's optimizer (csrc/router_optim.hip, diffusion_pruning_amd/router_optim.py): the fp64 model of the kernel
(tests/router_adamw_model.py) against torch.optim.AdamW + LambdaLR, the state-dict conversions on CPU tensors against a real
torch.optim.AdamW, and the ctypes layout of the new ABI structs."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from tests import router_adamw_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aptp_hip.h")


def test_model_matches_torch_adamw_with_lambda_lr():
    """six steps, two groups with their own rate and decay, constant_with_warmup over W = 4, one parameter without a gradient for
    the first three steps (torch gives it no state and no step): values to 1e-12 relative, per-item step counts equal torch's"""
    g = torch.Generator().manual_seed(5)
    shapes = [(7, 3), (5,), (4, 4), (9,)]
    group_of = [0, 0, 1, 1]
    late = 3                                        # this parameter (group 1) gets its first gradient at step 3
    W = 4
    groups = [(2e-2, 1e-2, W), (5e-3, 1e-1, W)]
    betas, eps = (0.9, 0.999), 1e-8
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g, dtype=torch.float64)) for s in shapes]
    opt = torch.optim.AdamW([{"params": ps[:2], "lr": groups[0][0], "weight_decay": groups[0][1]},
                             {"params": ps[2:], "lr": groups[1][0], "weight_decay": groups[1][1]}], betas=betas, eps=eps)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: min(1.0, k / W))
    items = [{"p": p.detach().clone(), "g": None, "m": torch.zeros_like(p.data), "v": torch.zeros_like(p.data), "step": 0.0,
              "group": gi} for p, gi in zip(ps, group_of)]
    counters = [0.0, 0.0, 0.0, 0.0]
    for k in range(6):
        grads = [torch.randn(*s, generator=g, dtype=torch.float64) for s in shapes]
        table = [i for i in range(len(ps)) if not (i == late and k < 3)]
        for i, p in enumerate(ps):
            p.grad = grads[i].clone() if i in table else None
        opt.step()
        sched.step()
        for i in table:
            items[i]["g"] = grads[i]
        new, counters = M.step([items[i] for i in table], groups, counters, betas, eps)
        for i, it in zip(table, new):
            items[i] = it
        for i, p in enumerate(ps):
            assert float((items[i]["p"] - p.detach()).abs().max()) <= 1e-12 * float(p.detach().abs().max()), (k, i)
            st = opt.state.get(p, {})
            assert items[i]["step"] == float(st.get("step", 0.0)), (k, i)
            if st:
                for a, b in ((items[i]["m"], st["exp_avg"]), (items[i]["v"], st["exp_avg_sq"])):
                    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), (k, i)
        assert counters == [k + 1.0, 0.0, 0.0, 0.0]
    assert items[late]["step"] == 3.0 and items[0]["step"] == 6.0
    # the first step ran at rate 0: LambdaLR's factor at scheduler step 0
    assert sched.get_last_lr() == [groups[0][0], groups[1][0]]


def test_model_skip_gate_scale_and_zero_grad():
    it = {"p": torch.tensor([1.0, -2.0]), "g": torch.tensor([0.5, 0.25]), "m": torch.zeros(2), "v": torch.zeros(2), "step": 2.0, "group": 0}
    groups = [(1e-2, 0.0, 0.0)]
    for gate, g in ((float("nan"), it["g"]), (float("inf"), it["g"]), (1.0, torch.tensor([0.5, float("nan")])), (1.0, torch.tensor([-float("inf"), 0.0]))):
        new, c = M.step([dict(it, g=g)], groups, [3.0, 1.0, 0.0, 0.0], (0.9, 0.999), 1e-8, gate=gate, zero_grad=True)
        assert torch.equal(new[0]["p"], it["p"].double()) and new[0]["step"] == 2.0 and c == [3.0, 2.0, 0.0, 0.0]
        assert torch.equal(new[0]["g"], torch.zeros(2, dtype=torch.float64))
    a, _ = M.step([dict(it, g=it["g"] * 4)], groups, [3.0, 0.0, 0.0, 0.0], (0.9, 0.999), 1e-8, grad_scale=0.25)
    b, c = M.step([it], groups, [3.0, 0.0, 0.0, 0.0], (0.9, 0.999), 1e-8, grad_scale=0.0)
    assert torch.equal(a[0]["p"], b[0]["p"]) and b[0]["step"] == 3.0 and c[0] == 4.0 and torch.equal(b[0]["g"], it["g"].double())


def _torch_optimizer(ps):
    return torch.optim.AdamW([{"params": ps[:2], "lr": 1e-2, "weight_decay": 0.05}, {"params": ps[2:], "lr": 3e-3, "weight_decay": 0.0}],
                             betas=(0.8, 0.99), eps=1e-6)


def test_state_dict_conversions_against_torch_adamw():
    from diffusion_pruning_amd.router_optim import EXTRA_KEY, adopt_state_dict, export_state_dict
    g = torch.Generator().manual_seed(9)
    shapes = [(3, 4), (6,), (2, 2), (5,)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]
    opt = _torch_optimizer(ps)
    for k in range(2):
        for i, p in enumerate(ps):
            p.grad = None if i == 3 else torch.randn(*shapes[i], generator=g)       # the last tensor never gets a gradient
        opt.step()
    sd = opt.state_dict()
    assert 3 not in sd["state"]
    like = [ps[:2], ps[2:]]
    steps, ms, vs = adopt_state_dict(sd, like)
    assert [float(s) for s in steps] == [2.0, 2.0, 2.0, 0.0]
    assert not ms[3].any() and not vs[3].any() and ms[3].shape == ps[3].shape          # a missing entry: zeros and step 0
    for i in range(3):
        assert torch.equal(ms[i], sd["state"][i]["exp_avg"]) and torch.equal(vs[i], sd["state"][i]["exp_avg_sq"])
    groups = [{"n": 2, "lr": 1e-2, "weight_decay": 0.05, "betas": (0.8, 0.99), "eps": 1e-6},
              {"n": 2, "lr": 3e-3, "weight_decay": 0.0, "betas": (0.8, 0.99), "eps": 1e-6}]
    back = export_state_dict(steps, ms, vs, groups, extra={"applied": 2.0, "skipped": 0.0, "warmup_steps": 0.0})
    assert back[EXTRA_KEY]["applied"] == 2.0 and [pg["params"] for pg in back["param_groups"]] == [[0, 1], [2, 3]]
    # our own layout converts back to the same tensors
    steps2, ms2, vs2 = adopt_state_dict(back, like)
    assert all(torch.equal(a, b) for a, b in zip(steps + ms + vs, steps2 + ms2 + vs2))
    # a fresh torch optimizer over copies of the parameters accepts it (torch adopts the dict's tensors) and takes the third step of the original
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = _torch_optimizer(qs)
    opt2.load_state_dict(back)
    for i in range(3):
        st = opt2.state[qs[i]]
        assert torch.equal(st["exp_avg"], sd["state"][i]["exp_avg"]) and torch.equal(st["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
        assert float(st["step"]) == 2.0
    for i, (p, q) in enumerate(zip(ps, qs)):
        gr = torch.randn(*shapes[i], generator=g)
        p.grad, q.grad = gr.clone(), gr.clone()
    opt.step()
    opt2.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach())


def test_state_dict_of_another_tensor_list_is_refused():
    from diffusion_pruning_amd.router_optim import adopt_state_dict
    g = torch.Generator().manual_seed(9)
    shapes = [(3, 4), (6,), (2, 2), (5,)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]
    opt = _torch_optimizer(ps)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    sd = opt.state_dict()
    adopt_state_dict(sd, [ps[:2], ps[2:]])
    with pytest.raises(ValueError, match="tensor list"):
        adopt_state_dict(sd, [ps[:1], ps[1:]])                       # same tensors, other grouping
    with pytest.raises(ValueError, match="tensor list"):
        adopt_state_dict(sd, [ps[:2], ps[2:3]])                      # one tensor fewer
    with pytest.raises(ValueError, match="parameter groups"):
        adopt_state_dict(sd, [ps])
    wrong = [ps[:2], [ps[2], torch.zeros(6)]]
    with pytest.raises(ValueError, match="saved moments"):
        adopt_state_dict(sd, wrong)                                  # a wrong shape
    extra = {"state": {**sd["state"], 7: sd["state"][0]}, "param_groups": sd["param_groups"]}
    with pytest.raises(ValueError, match="tensor list"):
        adopt_state_dict(extra, [ps[:2], ps[2:]])                    # state for a tensor no group holds


def test_ctypes_layout_of_the_group_adamw_structs():
    from diffusion_pruning_amd import _lib
    structs = {"AptpGroupAdamWItem": _lib.GroupAdamWItem, "AptpAdamWGroup": _lib.AdamWGroup, "AptpGroupAdamWParams": _lib.GroupAdamWParams}
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        body.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            body.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
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
    assert ctypes.sizeof(_lib.GroupAdamWItem) == 56 and ctypes.sizeof(_lib.AdamWGroup) == 12


def test_bad_arguments_are_refused_on_the_host():
    """every refusal happens before any launch, so it can be seen without a GPU"""
    from diffusion_pruning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert lib.aptp_group_adamw_blocks(0) == 0 and lib.aptp_group_adamw_blocks(1) == 1 and lib.aptp_group_adamw_blocks(4097) == 2
    assert lib.aptp_group_adamw(None, None) == -1
    q = _lib.GroupAdamWParams()
    assert lib.aptp_group_adamw(ctypes.byref(q), None) == -1 and b"null pointer" in lib.aptp_last_error()
