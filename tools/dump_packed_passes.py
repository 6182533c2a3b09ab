"""Every output buffer of the three table-driven passes over the packed trainable state -- aptp_adamw_many, aptp_group_adamw,
aptp_ema_many -- on seeded inputs, written to an .npz: run it at two commits and compare, every array must be bit-equal.

  python tools/dump_packed_passes.py --out a.npz [--root TREE]     # TREE: another checkout of this repository (default: this one)
  python tools/dump_packed_passes.py --compare a.npz b.npz

Only the C entry points are driven (ctypes blocks of diffusion_pruning_amd._lib), so the same file runs against any commit that
has them.  No gate lies in (3.0e38, FLT_MAX]: that is where DESIGN 6s changed the kernels' answer on purpose."""
import argparse
import ctypes
import os
import sys

import numpy as np

SIZES = [1, 3, 4, 5, 1023, 4096, 4097, 3 * 4096 + 7]
SHADOW = [i % 2 == 0 for i in range(len(SIZES))]


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), "different sets of arrays"
    bad = [k for k in A.files if A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes()]      # (bits: a NaN equals itself)
    print(f"{a} vs {b}: {len(A.files)} arrays, {sum(A[k].size for k in A.files)} elements, {len(bad)} differ {bad[:8]}")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from diffusion_pruning_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = lambda: torch.cuda.current_stream().cuda_stream
    out = {}

    def rnd(n, seed, scale=1.0):
        return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)

    def scalar(x):
        return torch.tensor(float(x), dtype=torch.float32, device=dev)

    def upload(items, blocks):
        starts = np.concatenate([[0], np.cumsum(blocks)]).astype(np.int32)
        return torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(dev), torch.from_numpy(starts).to(dev), int(starts[-1])

    def put(tag, **tensors):
        torch.cuda.synchronize()
        for k, ts in tensors.items():
            for i, t in enumerate(ts if isinstance(ts, (list, tuple)) else [ts]):
                if t is not None:
                    out[f"{tag}/{k}{i}"] = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).detach().cpu().numpy().copy()

    def shadows():
        return [torch.zeros(n, dtype=torch.bfloat16, device=dev) if s else None for n, s in zip(SIZES, SHADOW)]

    # ---- aptp_adamw_many: 4 steps; warm-up 0 / 4, grad_scale 1 / 1/3, gate absent / 0.25 / NaN at the second step ------------------
    for warm in (0, 4):
        for gs in (1.0, 1.0 / 3.0):
            for gname, gates in (("none", [None] * 4), ("finite", [0.25] * 4), ("nan", [0.25, float("nan"), 0.25, 0.25])):
                p = [rnd(n, 100 + i) for i, n in enumerate(SIZES)]
                g = [torch.zeros(n, device=dev) for n in SIZES]
                m = [torch.zeros(n, device=dev) for n in SIZES]
                v = [torch.zeros(n, device=dev) for n in SIZES]
                sh = shadows()
                step = scalar(0)
                items = (_lib.AdamWItem * len(SIZES))()
                for i, n in enumerate(SIZES):
                    it = items[i]
                    it.p, it.g, it.m, it.v, it.n = p[i].data_ptr(), g[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr(), n
                    it.shadow = None if sh[i] is None else sh[i].data_ptr()
                idev, sdev, total = upload(items, [lib.aptp_adamw_blocks(n) for n in SIZES])
                for k, gate in enumerate(gates):
                    for i, n in enumerate(SIZES):
                        g[i].copy_(rnd(n, 1000 * (k + 1) + i, 0.1))
                    gt = None if gate is None else scalar(gate)
                    q = _lib.AdamWParams()
                    q.items_dev, q.starts_dev, q.n_items, q.total_blocks = idev.data_ptr(), sdev.data_ptr(), len(SIZES), total
                    q.lr, q.beta1, q.beta2, q.eps, q.weight_decay = 1e-2, 0.9, 0.999, 1e-8, 1e-2
                    q.step_dev, q.gate_dev = step.data_ptr(), None if gt is None else gt.data_ptr()
                    q.grad_scale, q.warmup_steps = gs, float(warm)
                    _lib.check(lib.aptp_adamw_many(ctypes.byref(q), stream()), "aptp_adamw_many")
                    if gate is None or np.isfinite(gate):
                        step += 1.0
                put(f"adamw/w{warm}/s{gs:.3f}/{gname}", p=p, m=m, v=v, sh=sh, step=step)

    # ---- aptp_group_adamw: 6 steps over two groups; a NaN gradient at the third, a finite gate at the fifth; zero_grad on and off ---
    p = [rnd(n, 200 + i) for i, n in enumerate(SIZES)]
    g = [torch.zeros(n, device=dev) for n in SIZES]
    m = [torch.zeros(n, device=dev) for n in SIZES]
    v = [torch.zeros(n, device=dev) for n in SIZES]
    steps = torch.zeros(len(SIZES), dtype=torch.float32, device=dev)
    counters = torch.zeros(4, dtype=torch.float32, device=dev)
    groups = torch.tensor([[1e-2, 1e-2, 0.0], [3e-3, 0.0, 3.0]], dtype=torch.float32).to(dev)      # lr, weight decay, warm-up
    items = (_lib.GroupAdamWItem * len(SIZES))()
    for i, n in enumerate(SIZES):
        it = items[i]
        it.p, it.g, it.m, it.v, it.n = p[i].data_ptr(), g[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr(), n
        it.step, it.group = steps.data_ptr() + 4 * i, i % 2
    idev, sdev, total = upload(items, [lib.aptp_group_adamw_blocks(n) for n in SIZES])
    for k in range(6):
        for i, n in enumerate(SIZES):
            g[i].copy_(rnd(n, 2000 * (k + 1) + i, 0.1))
        if k == 2:
            g[6][4096] = float("nan")
        gt = scalar(0.25) if k == 4 else None
        q = _lib.GroupAdamWParams()
        q.items_dev, q.starts_dev, q.n_items, q.total_blocks = idev.data_ptr(), sdev.data_ptr(), len(SIZES), total
        q.groups_dev, q.n_groups, q.counters_dev = groups.data_ptr(), 2, counters.data_ptr()
        q.beta1, q.beta2, q.eps, q.grad_scale, q.zero_grad = 0.9, 0.999, 1e-8, 0.5 if k == 5 else 1.0, int(k % 2 == 0)
        q.gate_dev = None if gt is None else gt.data_ptr()
        q.items_host = ctypes.cast(items, ctypes.c_void_p)
        _lib.check(lib.aptp_group_adamw(ctypes.byref(q), stream()), "aptp_group_adamw")
        put(f"group/step{k}", p=p, g=g, m=m, v=v, steps=steps, counters=counters)

    # ---- aptp_ema_many: UPDATE at four counts in both decay forms, then SWAP twice ------------------------------------------------
    for warm in (0, 1):
        for count in (0, 1, 7, 29999):
            p = [rnd(n, 300 + i) for i, n in enumerate(SIZES)]
            e = [rnd(n, 400 + i) for i, n in enumerate(SIZES)]
            sh = shadows()
            cnt, cur = scalar(count), scalar(-1)
            items = (_lib.EmaItem * len(SIZES))()
            for i, n in enumerate(SIZES):
                it = items[i]
                it.p, it.ema, it.n = p[i].data_ptr(), e[i].data_ptr(), n
                it.shadow = None if sh[i] is None else sh[i].data_ptr()
            idev, sdev, total = upload(items, [lib.aptp_adamw_blocks(n) for n in SIZES])
            for k, mode in enumerate((_lib.EMA_UPDATE, _lib.EMA_SWAP, _lib.EMA_SWAP)):
                q = _lib.EmaParams()
                q.items_dev, q.starts_dev, q.n_items, q.total_blocks = idev.data_ptr(), sdev.data_ptr(), len(SIZES), total
                q.mode, q.count_dev, q.cur_decay_dev = mode, cnt.data_ptr(), cur.data_ptr()
                q.decay, q.min_decay, q.update_after_step = 0.9999, 0.0, 0
                q.use_warmup, q.inv_gamma, q.power = warm, 1.0, 2.0 / 3.0
                _lib.check(lib.aptp_ema_many(ctypes.byref(q), stream()), "aptp_ema_many")
                put(f"ema/w{warm}/c{count}/call{k}", p=p, ema=e, sh=sh, cur=cur)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez(a.out, **out)
    print(f"{a.out}: {len(out)} arrays, {sum(x.size for x in out.values())} elements, library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
