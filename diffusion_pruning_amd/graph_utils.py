"""HIP-graph helpers shared by the captured steps (train_step.py, pipeline.py) and the benchmark.

``new_graph()`` is ``torch.cuda.CUDAGraph()``; with ``KEEP_GRAPHS`` set (bench.py does, before capturing) the captured
hipGraph_t is kept next to its executable so that ``node_count`` can ask the runtime how many nodes -- kernel launches and
the few memcpy / memset nodes torch adds -- one replay issues.  ``warmup_stream()`` is the eager pass ahead of a capture and
``concurrent_stream()`` picks the side stream a replayed graph overlaps on (``concurrent_streams()``: several, for the lanes of
the expert dispatch); nothing else here touches the device unless a graph exists."""
from __future__ import annotations

import contextlib
import ctypes
from typing import Optional

import torch

KEEP_GRAPHS = False
_hip = None


def new_graph() -> "torch.cuda.CUDAGraph":
    return torch.cuda.CUDAGraph(keep_graph=True) if KEEP_GRAPHS else torch.cuda.CUDAGraph()


def node_count(graph) -> Optional[int]:
    """nodes of a captured graph (None when the graph was not kept or the runtime cannot be asked)"""
    global _hip
    try:
        raw = graph.raw_cuda_graph()
    except Exception:  # noqa: BLE001  (not captured with keep_graph)
        return None
    try:
        if _hip is None:
            _hip = ctypes.CDLL("libamdhip64.so")
            _hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
            _hip.hipGraphGetNodes.restype = ctypes.c_int
        n = ctypes.c_size_t(0)
        rc = _hip.hipGraphGetNodes(ctypes.c_void_p(int(raw)), None, ctypes.byref(n))
        return int(n.value) if rc == 0 else None
    except Exception:  # noqa: BLE001
        return None


@contextlib.contextmanager
def warmup_stream():
    """The eager warm-up ahead of a capture (allocator, plan caches, autograd's stream anchors) runs inside: on a fresh side
    stream that waits for the current one; on the way out the current stream joins it and the host waits for the device"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        yield side
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def concurrent_stream(main: Optional["torch.cuda.Stream"] = None, tries: int = 12, spin_ms: float = 0.4, log=None) -> "torch.cuda.Stream":
    """A side stream whose work really runs NEXT TO `main` (default: the current stream).

    Round 4 traced the "capture-order variance" of the training steps (the same captured step replaying 6-10 % faster or
    slower depending on when in the process it was captured) to this: the three graphs of a step take the
    same time whichever capture they belong to, but the teacher graph on the side stream overlaps the student's forward only
    for SOME side streams -- torch hands out streams from a pool, the runtime maps them onto a few hardware queues, and a side
    stream that shares its queue with the launching stream serialises behind it.  So the side stream is chosen by measurement:
    candidates are tried with two spin kernels, one per stream, until their total time says they overlapped."""
    main = main or torch.cuda.current_stream()
    dev = main.device
    cycles = int(spin_ms * 1e-3 * 2.0e9)

    def timed(side):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(main):
            e0.record(main)
            if side is not None:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    torch.cuda._sleep(cycles)
            torch.cuda._sleep(cycles)
            if side is not None:
                main.wait_stream(side)
            e1.record(main)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)
    timed(None)
    single = min(timed(None), timed(None))
    best, best_ratio, seen = None, 1e9, []
    for _ in range(tries):
        s = torch.cuda.Stream(device=dev)
        timed(s)
        r = min(timed(s), timed(s)) / single
        seen.append(round(r, 2))
        if r < best_ratio:
            best, best_ratio = s, r
        if r < 1.3:
            break
    if log is not None:
        log.append({"single_ms": round(single, 3), "ratios_tried": seen, "chosen_ratio": round(best_ratio, 2)})
    return best


def concurrent_streams(n: int, main: Optional["torch.cuda.Stream"] = None, tries: int = 12, spin_ms: float = 0.4, log=None) -> list:
    """Up to ``n - 1`` side streams whose work runs next to `main` (default: the current stream) AND next to each other: the
    spin-kernel probe of ``concurrent_stream`` for more than one side stream (the lanes of pipeline.ExpertDispatchLoop).

    The streams are chosen one at a time.  A candidate is timed with one spin kernel on `main`, one on every stream chosen so
    far and one on itself, all released together; it is accepted when that takes less than 1.3x one spin kernel alone, i.e. when
    it shares a hardware queue with none of them (two kernels on one queue would take 2x).  At most ``tries`` candidates are
    timed per stream that is still wanted.  Unlike ``concurrent_stream``, which hands back its best candidate whatever its
    ratio, only accepted streams are returned, so the list may be shorter than ``n - 1`` (empty for n <= 1): the caller runs
    with what it got.  ``log``: a list that receives one dict -- the time of one spin kernel, every ratio tried in order, the
    ratios of the accepted streams, how many were wanted and found."""
    main = main or torch.cuda.current_stream()
    dev = main.device
    cycles = int(spin_ms * 1e-3 * 2.0e9)
    chosen, chosen_ratios, seen = [], [], []

    def timed(sides):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(main):
            e0.record(main)
            for side in sides:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    torch.cuda._sleep(cycles)
            torch.cuda._sleep(cycles)
            for side in sides:
                main.wait_stream(side)
            e1.record(main)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)
    single = None
    if n > 1:
        timed([])
        single = min(timed([]), timed([]))
        for _ in range(tries * (n - 1)):
            s = torch.cuda.Stream(device=dev)
            if any(s.cuda_stream == c.cuda_stream for c in chosen + [main]):
                continue                               # (torch hands out streams from a pool: this one is already taken)
            timed(chosen + [s])
            r = min(timed(chosen + [s]), timed(chosen + [s])) / single
            seen.append(round(r, 2))
            if r < 1.3:
                chosen.append(s)
                chosen_ratios.append(round(r, 2))
                if len(chosen) == n - 1:
                    break
    if log is not None:
        log.append({"single_ms": None if single is None else round(single, 3), "ratios_tried": seen, "chosen_ratios": chosen_ratios,
                    "wanted": max(0, n - 1), "found": len(chosen)})
    return chosen
