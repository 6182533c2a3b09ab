"""CPU checks of the EMA of the expert fine-tune: the fp64 model of tests/ema_model.py against hand values of the decay rule
(diffusers' EMAModel), and the ctypes mirror of AptpEmaParams / AptpEmaItem against the C compiler's layout of the header."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import ema_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aptp_hip.h")


def test_decay_rule_hand_values():
    assert M.ema_decay(0) == 0.0                                    # n = 1: the first applied step copies the parameters
    assert M.ema_decay(1) == pytest.approx(2.0 / 11.0, abs=1e-15)   # n = 2
    assert M.ema_decay(2) == pytest.approx(3.0 / 12.0, abs=1e-15)   # n = 3
    assert M.ema_decay(4) == pytest.approx(5.0 / 14.0, abs=1e-15)
    # the cap: (1 + s) / (10 + s) reaches 0.9999 at s = 89,990
    assert M.ema_decay(89_988) < 0.9999 and M.ema_decay(89_992) == 0.9999 and M.ema_decay(10 ** 7) == 0.9999
    assert M.ema_decay(9, decay=0.5) == 0.5 and M.ema_decay(7, decay=0.5) == pytest.approx(8.0 / 17.0, abs=1e-15)
    # min_decay lifts a small base but never the d = 0 of the first step
    assert M.ema_decay(1, min_decay=0.5) == 0.5 and M.ema_decay(0, min_decay=0.5) == 0.0
    assert M.ema_decay(29_999, min_decay=0.5) == pytest.approx(30_000.0 / 30_009.0, abs=1e-15)


def test_update_after_step():
    kw = dict(update_after_step=3)
    assert [M.ema_decay(c, **kw) for c in range(4)] == [0.0, 0.0, 0.0, 0.0]        # s = max(0, n - 4) = 0 up to n = 4
    assert M.ema_decay(4, **kw) == pytest.approx(2.0 / 11.0, abs=1e-15)             # n = 5: s = 1
    assert M.ema_decay(5, **kw) == pytest.approx(3.0 / 12.0, abs=1e-15)


def test_warmup_form():
    kw = dict(use_ema_warmup=True, inv_gamma=1.0, power=2.0 / 3.0)
    assert M.ema_decay(0, **kw) == 0.0
    assert M.ema_decay(1, **kw) == pytest.approx(1.0 - 2.0 ** (-2.0 / 3.0), abs=1e-15)          # s = 1
    assert M.ema_decay(3, inv_gamma=2.0, power=1.0, use_ema_warmup=True) == pytest.approx(1.0 - 1.0 / 2.5, abs=1e-15)
    assert M.ema_decay(10 ** 9, **kw) == 0.9999


def test_update_and_trajectory():
    ema, p = np.array([1.0, -2.0, 0.5]), np.array([3.0, 2.0, 0.5])
    out, d = M.ema_update(ema, p, 0)
    assert d == 0.0 and np.array_equal(out, p)
    out, d = M.ema_update(ema, p, 2)
    assert d == 0.25 and np.allclose(out, 0.25 * ema + 0.75 * p, rtol=0, atol=1e-15)
    masters = [p, 2 * p, 3 * p]
    traj = M.ema_trajectory(ema, masters)
    want = p                                               # step 1 copies
    want = want - (1 - 2.0 / 11.0) * (want - 2 * p)
    assert np.allclose(traj[1], want, rtol=0, atol=1e-15)
    want = want - (1 - 0.25) * (want - 3 * p)
    assert np.allclose(traj[2], want, rtol=0, atol=1e-15) and len(traj) == 3
    assert traj[0].dtype == np.float64


def test_model_defaults_are_the_constructor_defaults():
    import inspect
    from diffusion_pruning_amd.packed_train import PackedEMA
    sig = inspect.signature(PackedEMA.__init__).parameters
    assert list(sig)[:3] == ["self", "trainer", "optimizer"] and sig["optimizer"].default is None
    for k, v in M.DEFAULTS.items():
        assert sig[k].default == v, k
    assert list(sig)[3:] == list(M.DEFAULTS)


def test_ema_struct_layout_matches_the_header():
    from diffusion_pruning_amd import _lib
    structs = {"AptpEmaItem": _lib.EmaItem, "AptpEmaParams": _lib.EmaParams}
    body = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs.items():
        body.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            body.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    body.append('printf("modes %d %d\\n", (int)APTP_EMA_UPDATE, (int)APTP_EMA_SWAP);')
    body.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(body))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    lines = [line.split() for line in out.strip().splitlines()]
    got = {ln[0]: ln[1:] for ln in lines}
    for cname, cls in structs.items():
        assert int(got[cname][0]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"][0]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert [int(x) for x in got["modes"]] == [_lib.EMA_UPDATE, _lib.EMA_SWAP]
    # field ORDER: the names of the header's struct bodies, in the order they are declared
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for cname, cls in structs.items():
        m = re.search(r"typedef struct \{([^}]*)\}\s*" + cname + r"\s*;", text)
        assert m, cname
        names = []
        for decl in m.group(1).split(";"):
            decl = decl.strip()
            if decl:                                       # "int32_t n_items, total_blocks": the last identifier of every part
                names += [re.findall(r"\w+", part)[-1] for part in decl.split(",")]
        assert names == [f for f, _ in cls._fields_], (cname, names)
