"""numpy model of csrc/grad_norm.hip: the exact summation order of the two launches and the finalise formulas, so that a test can
ask for the kernel's four output floats bit for bit.  No test lives here.

The order (include/aptp_hip.h, aptp_grad_norm): an item of n elements takes ceil(n / 4096) blocks of 256 threads; thread t of a
block adds, in fp64, the squares of the elements e .. e + 3 at e = base + (i * 256 + t) * 4 for the trips i = 0, 1, 2, 3 (an item's
last quad may be short); each wave of 64 folds by a butterfly over the lane offsets 32, 16, 8, 4, 2, 1; the four wave sums are added
as ((w0 + w1) + w2) + w3.  The finalise block lets thread j add partials[j], partials[j + 256], ... and folds the same way."""
import numpy as np

THREADS, ELEMS_PER_BLOCK = 256, 4096


SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 5]      # scalar tail only, float4 + tail, whole blocks, more than one block


def tables():
    """name -> list of item sizes: every size alone, all in one table, 300 tiny items (more than 256 blocks: the finalise loop makes
    a second trip), 2100 tiny items (more than 8 x 256 blocks: the finalise loop's eight-loads-ahead trip and its remainder), one item
    of 489 blocks"""
    t = {f"n{n}": [n] for n in SIZES}
    t["all"] = list(SIZES)
    t["300_tiny"] = [1 + (i * 5) % 7 for i in range(300)]
    t["2100_tiny"] = [1 + (i * 3) % 7 for i in range(2100)]
    t["2e6+3"] = [2 * 10 ** 6 + 3]
    return t


def items_of(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n).astype(np.float32) for n in sizes]


def blocks_of(n: int) -> int:
    return 0 if n <= 0 else (n + ELEMS_PER_BLOCK - 1) // ELEMS_PER_BLOCK


def block_tree(s: np.ndarray) -> np.ndarray:
    """[..., 256] fp64 per-thread sums -> [...] block sums in the kernel's order"""
    assert s.dtype == np.float64 and s.shape[-1] == THREADS
    w = s.reshape(s.shape[:-1] + (4, 64)).copy()
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lanes ^ off]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def partials(items) -> np.ndarray:
    """list of fp32 arrays (one per item of the table) -> fp64 [total_blocks]"""
    out = []
    with np.errstate(all="ignore"):
        for g in items:
            g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
            nb = blocks_of(g.size)
            # elements past the end contribute nothing in the kernel; here they are zeros (s + 0.0 == s bit for bit, s >= +0)
            sq = np.zeros(nb * ELEMS_PER_BLOCK, dtype=np.float64)
            sq[:g.size] = g.astype(np.float64) * g.astype(np.float64)
            sq = sq.reshape(nb, 4, THREADS, 4)                      # [block, trip, thread, element of the quad]
            s = np.zeros((nb, THREADS), dtype=np.float64)
            for i in range(4):
                for j in range(4):
                    s = s + sq[:, i, :, j]
            out.append(block_tree(s))
    return np.concatenate(out)


def total_sum(parts: np.ndarray) -> np.float64:
    """the finalise block's sum of the partials"""
    parts = np.asarray(parts, dtype=np.float64)
    trips = (parts.size + THREADS - 1) // THREADS
    padded = np.zeros(trips * THREADS, dtype=np.float64)
    padded[:parts.size] = parts
    s = np.zeros(THREADS, dtype=np.float64)
    with np.errstate(all="ignore"):
        for row in padded.reshape(trips, THREADS):
            s = s + row
        return block_tree(s)


def finalise(S, grad_scale=1.0, max_norm=None, gate=None, clipped_before=0.0) -> np.ndarray:
    """fp32 [4] = {total_norm, clip_coef, verdict, clipped_count} as thread 0 of the finalise block computes them"""
    gs = np.float32(grad_scale)
    gs = np.float32(1.0) if gs == 0 else gs
    with np.errstate(all="ignore"):
        total = np.sqrt(np.float64(S)) * np.float64(gs)
        total_f = np.float32(total)
        coef = np.float32(1.0)
        if max_norm is not None:
            r = np.float64(np.float32(max_norm)) / (total + np.float64(1e-6))
            if r < 1.0:
                coef = np.float32(max(r, np.float64(0.0)))
    finite = bool(np.isfinite(total_f)) and (gate is None or bool(np.isfinite(np.float32(gate))))
    clipped = np.float32(clipped_before)
    if not finite:
        coef = np.float32(1.0)
    elif coef < np.float32(1.0):
        clipped = np.float32(clipped + np.float32(1.0))
    return np.array([total_f, coef, total_f if finite else np.float32("nan"), clipped], dtype=np.float32)


def grad_norm(items, grad_scale=1.0, max_norm=None, gate=None, clipped_before=0.0) -> np.ndarray:
    return finalise(total_sum(partials(items)), grad_scale, max_norm, gate, clipped_before)


def reference_norm(items, grad_scale=1.0) -> np.float32:
    """numpy's own fp64 norm of everything, rounded once to fp32: what the kernel's total_norm may miss by one ulp"""
    with np.errstate(all="ignore"):
        flat = np.concatenate([np.asarray(g, dtype=np.float64).reshape(-1) for g in items])
        return np.float32(np.linalg.norm(flat) * np.float64(np.float32(grad_scale)))


def ulps(a, b) -> int:
    """distance of two finite fp32 values of one sign in units of the last place"""
    ia, ib = np.float32(a).view(np.int32), np.float32(b).view(np.int32)
    return abs(int(ia) - int(ib))
