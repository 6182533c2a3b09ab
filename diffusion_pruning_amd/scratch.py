"""Launch scratch: the device memory a launch needs besides its operands -- split-K arrival counters, grow-only workspaces and
the unit-statistics arena of a forward.  ops.py re-exports what its callers use (``ops.scratch_domain``, ``ops._tile_counters``,
``ops._workspace``, ``ops.ustat_begin`` ...).

One key, ``key(device)`` = (device index, handle of the current stream, ``domain()``, capturing):
* launches on one stream serialise, so everything is per launching stream;
* every ``torch.cuda.graph`` capture runs on a capture stream of its own choosing, so graphs that will REPLAY concurrently
  are captured under different ``scratch_domain``s;
* a workspace or arena first asked for during capture lives in that graph's private pool, hence the capture flag.  Counters
  ignore it: eager and captured launches of one stream and domain share a slab (every launch leaves it zero).

One lifetime rule: a buffer handed out during capture is never released (``capture_keep``) -- its address is baked into the
graph, see ``workspace``.

The counter pool grows in chunks of ``N_SLABS`` slabs, outside capture only, and a slab handed out keeps its address for the life
of the process.  The number of keys is bounded: torch hands out stream handles from a fixed pool per device and the domains are
a few literals ("teacher", "val_teacher", the VAE's) and ("dispatch", lane) for the at most three side lanes of
pipeline.ExpertDispatchLoop; a slab is 256 KiB.
"""
from __future__ import annotations

import os
import threading
from collections import namedtuple

import torch

Key = namedtuple("Key", "device_index stream_handle domain capturing")

_tls = threading.local()
_lock = threading.Lock()
capture_keep = []          # see workspace


class scratch_domain:
    """``with ops.scratch_domain("teacher"): ...`` -- launches issued (or CAPTURED) inside use their own split-K counters and
    scratch buffers.  Scratch is keyed by the launching stream, which is enough for eager concurrency; but every
    ``torch.cuda.graph`` capture runs on the same capture stream, so two graphs that will REPLAY concurrently on different
    streams (the pruning step's teacher next to the student forward) must be captured under different domains."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.prev = getattr(_tls, "domain", None)
        _tls.domain = self.name
        return self

    def __exit__(self, *exc):
        _tls.domain = self.prev
        return False


def domain():
    return getattr(_tls, "domain", None)


# the module's reads of torch.cuda, and its one wait (host tests replace them)
def _stream_handle() -> int:
    return torch.cuda.current_stream().cuda_stream


def _capturing() -> bool:
    return torch.cuda.is_current_stream_capturing()


def _current_device() -> int:
    return torch.cuda.current_device()


def _sync_stream():
    torch.cuda.current_stream().synchronize()


def _alloc(n, dtype, device, zero: bool) -> torch.Tensor:
    return (torch.zeros if zero else torch.empty)(n, dtype=dtype, device=device)


def key(device: torch.device) -> Key:
    index = device.index
    return Key(index if index is not None else _current_device(), _stream_handle(), domain(), _capturing())


# ---- split-K arrival counters
N_COUNTERS = 1 << 16       # int32 words per slab
N_SLABS = int(os.environ.get("APTP_N_SLABS", "16"))        # slabs per chunk
_LOW = max(1, N_SLABS // 2)
_pools = {}                # device index -> {"chunks": [tensor], "free": [slab], "slab": {(stream, domain): slab}}


def counters(device):
    """Zero-initialised arrival counters of the split-K launches issued on the CURRENT stream under the current domain (every
    launch leaves them zero): each (stream, domain) is handed its own slab on first use -- a host-side table lookup, legal
    during capture -- so forwards running concurrently never share counters.

    Outside capture the pool is topped up first whenever fewer than half a chunk is free (that also creates it), so a capture,
    which must not allocate (a fill recorded into a graph would only run at replay), finds free slabs for its new keys.  Inside
    capture a known key gets its slab, a new key a free one; None (= use the separate reduce launch) when there is none."""
    k = key(device)
    with _lock:
        pool = _pools.get(k.device_index)
        if not k.capturing and (pool is None or len(pool["free"]) < _LOW):
            if pool is None:
                pool = _pools[k.device_index] = {"chunks": [], "free": [], "slab": {}}
            # a new tensor: the slabs already handed out keep their addresses, graphs have baked them in
            chunk = _alloc((N_SLABS, N_COUNTERS), torch.int32, device, zero=True)
            pool["chunks"].append(chunk)
            pool["free"].extend(chunk)
            # another stream may be the first to use one of these slabs, and nothing else orders that use behind the fill
            _sync_stream()
        if pool is None:
            return None
        sid = k[:3]
        slab = pool["slab"].get(sid)
        if slab is None and pool["free"]:
            slab = pool["slab"][sid] = pool["free"].pop(0)
        return slab


def counter_keys(device) -> int:
    """how many counter slabs of the device have been handed out"""
    pool = _pools.get(key(device).device_index)
    return 0 if pool is None else len(pool["slab"])


# ---- grow-only workspaces
_ws = {}


def workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch buffer per key: stream-ordered reuse, kernels on one stream serialise; forwards that run concurrently
    on different streams must not share split-K slabs or GroupNorm partials."""
    k = key(device)
    with _lock:
        buf = _ws.get(k)
        if buf is None or buf.numel() < nbytes:
            size = max(nbytes, 1 << 20)
            if k.capturing and buf is not None:
                size = max(size, buf.numel() + buf.numel() // 2)      # (kept forever, below: grow geometrically so the kept set stays small)
            buf = _alloc(size, torch.uint8, device, zero=False)
            if k.capturing:
                # Allocated while a stream is capturing: the block comes from that graph's private pool and its address is baked into
                # every launch captured with it -- possibly into graphs captured LATER on the same stream, which may outlive the graph
                # that owns the pool.  torch.cuda.graph.__enter__ empties the cache, so once the owning graph is gone and a larger
                # request has replaced the buffer here, the block would be returned to the device while a younger graph still
                # writes to it (seen as "Memory access fault ... write access to a read-only page" when a code object was mapped
                # there, and only for some test orders).  A capture-time scratch buffer is therefore never released: a few grow
                # steps per (stream, domain), bounded by the largest request.
                capture_keep.append(buf)
            _ws[k] = buf
        return buf


# ---- unit-statistics arena
# Round 4: GroupNorm statistics WITHOUT a finalise launch.  A producer that emits column statistics also adds per-(sample, channel
# unit) fixed-point sums to a slice of a zeroed arena (AptpConvGemmParams.ustat_out: 64-bit integer atomics, order-independent);
# when every producer of a GroupNorm's input left them, the apply pass finishes mean / rstd itself (AptpGroupNormColStats.ustats).
# The arena belongs to ONE forward: the model calls ustat_begin() at the top of its forward (that zeroes it: one fill launch, also
# inside a captured graph) and ustat_end() at the end; outside such a bracket nothing is emitted.  USTAT_UNIT = channels per unit:
# it must divide every GroupNorm group size of the model (SD-2.1: 320 / 32 = 10); 0 = off.
USTAT = os.environ.get("APTP_USTAT", "1") != "0"
USTAT_NREP = int(os.environ.get("APTP_USTAT_NREP", "8"))
_USTAT_WORDS = 1 << 17            # int64 words per arena (1 MiB): ~35 producers x 8 replicas x 4 samples x <= 128 units x 2
_arenas = {}


def ustat_begin(device, unit: int):
    """open the unit-statistics arena of the forward that starts now on the current stream (zeroed here); unit <= 0 or
    APTP_USTAT=0: no arena, producers emit column statistics only"""
    device = torch.device(device)
    if not USTAT or unit <= 0 or device.type != "cuda":
        _tls.ustat = None
        return
    k = key(device)
    with _lock:
        ent = _arenas.get(k)
        if ent is None:
            # (allocated inside a capture, the zero fill is part of the graph: every replay starts from a clean arena; such a buffer is
            #  never released -- its address is baked into the graph, see workspace)
            ent = _arenas[k] = {"buf": _alloc(_USTAT_WORDS, torch.int64, device, zero=True), "used": 0}
            if k.capturing:
                capture_keep.append(ent["buf"])
                ent["used"] = _USTAT_WORDS          # a second capture on this stream zeroes everything: it cannot know what the first used
        elif ent["used"]:
            ent["buf"][:ent["used"]].zero_()        # what the previous forward on this arena added to
    _tls.ustat = {"buf": ent["buf"], "off": 0, "unit": int(unit), "ent": ent}


def ustat_end():
    st = getattr(_tls, "ustat", None)
    if st is not None and not st.get("closed"):
        st["closed"] = True
        st["ent"]["used"] = max(st["ent"]["used"], st["off"])


def ustat_alloc(B: int, nout: int):
    st = getattr(_tls, "ustat", None)
    if st is None or st.get("closed"):
        return None
    unit = st["unit"]
    units = (nout + unit - 1) // unit
    nrep = USTAT_NREP                 # replicas spread the same-address contention; more samples already spread it
    while nrep > 1 and nrep * B > 4 * USTAT_NREP:
        nrep //= 2
    n = nrep * B * units * 2
    if st["off"] + n > st["buf"].numel():
        return None
    u = st["buf"][st["off"]:st["off"] + n]
    st["off"] += n
    return u, unit, units, nrep
