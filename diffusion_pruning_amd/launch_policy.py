"""Which kernel an ``ops.conv_gemm`` launch gets: tile id, split-K depth, how the K-slices are combined, workgroup order."""
# Pure host logic (no torch, no shared library): the tuning table with its derived caches, and choose_launch, the rules
# layered on top of it.  ops.conv_gemm calls choose_launch once per launch; tests/test_host_logic.py pins every rule on the
# CPU.  The switches below are read here at call time (ops re-exports them for readers only).
import json
import math
import os
import re

from . import _lib as L             # ACT_GEGLU and the TILE_* ids of include/aptp_hip.h

BK = 64                             # K-step of every tile: channels are padded to it
DMA_TILE_FIRST = L.TILE_DMA_128x128  # every tile past the six register-staged ones is an LDS-DMA tile ...
DMA_MAX_CHANNELS = 4032             # ... whose channel steps address at most this many channels per tap (csrc)
SK_TILE_FIRST = L.TILE_SK_256x160   # APTP_TILE_SK_*: persistent stream-K macro-tiles (csrc/conv_gemm_sk.hip)
SK_MAX_CHANNELS = 32704             # channels per tap of a stream-K tile
_HALO_TILES = (L.TILE_HALO_128x160, L.TILE_HALO_128x128)
# tiles csrc/lin_gemm.hip instantiates (the LIN rows of csrc/conv_gemm_tiles.h; tests/test_host_logic.py compares the two)
_LEAN_TILES = frozenset(getattr(L, "TILE_" + t) for t in (
    "DMA_64x128 DMA_128x64 DMA_64x64 DMA3_64x128 DMA3_128x64 DMA3_64x64 DMA4_64x128 DMA4_64x64 DMA4_128x64 DMA6_64x64 DMA8S_64x64 "
    "DMA6_64x128 DMA6_128x64 KU2S4_64x64 KU2S6_64x64 KU2S4_64x128 KU2S6_64x128 KU2S4_128x64").split())

TUNING_NEAREST = os.environ.get("APTP_TUNING_NEAREST", "1") != "0"
TUNING_MAX_DIST = 2.0
LEAN_REMAP = os.environ.get("APTP_LEAN_REMAP", "1") != "0"
SK_AUTO = os.environ.get("APTP_SK_AUTO", "1") == "1"
SK_AUTO_MIN_OUTPUTS = 256 * 256 * 160
SK_AUTO_MIN_KSTEPS = 16
SPLITK_FORCE_IN_KERNEL = os.environ.get("APTP_SPLITK_FORCE_INKERNEL", "0") == "1"
# a split-K launch whose output feeds a GroupNorm combines its slices in-kernel (and emits the statistics) up to this many slices
COLS_SPLIT_MAX = int(os.environ.get("APTP_COLS_SPLIT_MAX", "2"))

_KEY = re.compile(r"M(\d+)_N(\d+)_C(\d+)_T(\d+)_s(\d+)u(\d+)g(\d+)(?:x(\d+))?$")


def tuning_key(M, N, Cin, taps, stride, ups, geglu, Cin2: int = 0) -> str:
    return f"M{M}_N{N}_C{Cin}_T{taps}_s{stride}u{ups}g{int(bool(geglu))}" + (f"x{Cin2}" if Cin2 else "")


def parse_key(key: str):
    """inverse of tuning_key: (M, N, Cin, taps, stride, ups, geglu as 0 / 1, Cin2), or None for a string that is no key"""
    m = _KEY.match(key)
    return m and tuple(int(t) if t else 0 for t in m.groups())


def key_of(p) -> str:
    """the table key of a filled ConvGemmParams"""
    return tuning_key(p.B * p.Hout * p.Wout, p.N, p.Cin, p.KH * p.KW, p.stride, p.ups, p.act == L.ACT_GEGLU, p.Cin2 if p.x2 else 0)


# (tile, split_k) per GEMM shape measured on MI355X by tools/tune_convs.py.  The table holds the shapes of the headline
# mask, the dense model and the pruning step; every OTHER architecture code (config 5's experts, real APTP experts with
# irregular widths) produces shapes that are not in it.  Those take the entry of the NEAREST tuned shape of the same class
# (taps, stride, upsampling, GEGLU, second operand) in log-space distance over (M, N, K) -- the tile engine's behaviour
# changes smoothly with the extents, while the library heuristic only knows the generic non-DMA tiles (measured on a
# 55 %-keep expert: 29 us per launch on conv_gemm_kernel<64,128> where the neighbours' DMA tiles take ~20).  Beyond
# TUNING_MAX_DIST the heuristic (aptp_conv_gemm_suggest_split_k / pick_tile) decides.  APTP_TUNING_NEAREST=0 disables.
# The dict object is never replaced (ops.TUNING is this very dict); the class index and the nearest-shape cache are derived
# from it, so every change goes through set_tuning / set_entry, or is followed by invalidate().
# (APTP_TUNING=<file> substitutes another table: A/B timing of tuning runs)
_path = os.environ.get("APTP_TUNING") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuning_gfx950.json")
TUNING = {}
if os.path.exists(_path):
    with open(_path) as _f:
        TUNING.update(json.load(_f))
_classes = None       # (taps, stride, ups, geglu, has x2) -> [(M, N, K, entry), ...]
_near = {}            # key without an entry -> nearest entry, or None (cached too: the experts ask for the same missing shapes every step)


def invalidate():
    """drop what was derived from TUNING (after editing it in place)"""
    global _classes
    _classes = None
    _near.clear()


def set_tuning(table):
    """replace the table's contents (an empty one: heuristics only)"""
    table = dict(table)
    TUNING.clear()
    TUNING.update(table)
    invalidate()


def set_entry(key: str, entry):
    """set one entry, or remove it (entry None)"""
    if entry is None:
        TUNING.pop(key, None)
    else:
        TUNING[key] = entry
    invalidate()


def _nearest(key, M, N, Cin, taps, stride, ups, geglu, Cin2):
    global _classes
    if key in _near:
        return _near[key]
    if _classes is None:
        _classes = {}
        for k, v in TUNING.items():
            s = parse_key(k)
            if s is not None:
                _classes.setdefault((s[3], s[4], s[5], s[6], s[7] > 0), []).append((s[0], s[1], s[3] * s[2] + s[7], v))
    K = taps * Cin + Cin2
    best, bd = None, TUNING_MAX_DIST
    for (M2, N2, K2, v) in _classes.get((taps, stride, ups, int(bool(geglu)), Cin2 > 0), ()):
        if v["tile"] in _HALO_TILES and M2 != M:
            continue                      # the halo-in-LDS tiles are tied to the map width
        if v["tile"] >= DMA_TILE_FIRST and max(Cin, Cin2) > DMA_MAX_CHANNELS:
            continue
        # (more rows than the tuned shape is the benign direction -- the same tile, more of them: a U-Net batch of 16 takes the
        #  entries tuned at batch 4 instead of falling back to the register-staged heuristic tiles, which bench.py's infer_bs16 leg
        #  measured at 0.08 of the MFMA peak on 48 launches)
        dm = math.log2(M / M2)
        d = (0.5 * dm if dm > 0 else -1.5 * dm) + abs(math.log2(N / N2)) + abs(math.log2(K / K2))
        if d < bd:
            best, bd = v, d
    if best is not None:
        nK = (K + BK - 1) // BK
        best = dict(best)
        best["split_k"] = max(1, min(int(best["split_k"]), nK // 4 if nK >= 8 else 1))
    _near[key] = best
    return best


def tuning_lookup(M, N, Cin, taps, stride, ups, geglu, Cin2: int = 0):
    """exact entry (the table's own dict), else a copy of the nearest tuned shape's with split_k clamped to this K, else None"""
    key = tuning_key(M, N, Cin, taps, stride, ups, geglu, Cin2)
    hit = TUNING.get(key)
    if hit is None and TUNING_NEAREST:
        hit = _nearest(key, M, N, Cin, taps, stride, ups, geglu, Cin2)
    return hit


def _lean_tile(M):
    # the lean tile the in-situ pass over the inference forward preferred at this row count (profiles/r4_tune_insitu_lean.txt)
    return L.TILE_DMA_128x64 if M >= 8192 else (L.TILE_DMA3_64x64 if M >= 2048 else L.TILE_KU2S4_64x64)


# A contraction of M rows, N packed weight rows and KH*KW taps of Cin (padded: cin_pad) channels plus a second operand of Cin2
# (cin2_pad).  In the result tile 0 means the library's pick_tile, split_k None "ask aptp_conv_gemm_suggest_split_k", in_kernel
# None splitk_in_kernel's default.  plain_linear: a layer the lean kernel of csrc/lin_gemm.hip can take (ops.conv_gemm computes it
# from its arguments, after aptp_lin_eligible).  tile / split_k / order: what the caller of ops.conv_gemm asked for.
def choose_launch(M, N, Cin, cin_pad, KH, KW, stride, ups, act, Cin2, cin2_pad, *, plain_linear, f32, tile, split_k, order):
    """-> (tile, split_k, in_kernel, order) of one launch; the numbered rules are applied in this order"""
    if split_k is not None or tile != 0 or f32:
        return tile, split_k, None, order          # 1. the caller's choice, and the fp32 parity path (tiles 1..6, no tables)
    taps, geglu = KH * KW, act == L.ACT_GEGLU
    channels = max(cin_pad, cin2_pad)
    sk_sized = SK_AUTO and M * N >= SK_AUTO_MIN_OUTPUTS and taps * (cin_pad // BK) + cin2_pad // BK >= SK_AUTO_MIN_KSTEPS
    lean = LEAN_REMAP and plain_linear and cin_pad <= DMA_MAX_CHANNELS
    # 2. the table: exact entry, else the nearest tuned shape of the same class
    key = tuning_key(M, N, Cin, taps, stride, ups, geglu, Cin2)
    tuned = TUNING.get(key)
    if tuned is None and TUNING_NEAREST:
        tuned = _nearest(key, M, N, Cin, taps, stride, ups, geglu, Cin2)
        if tuned is not None and sk_sized:
            tuned = None                   # 3. only a NEIGHBOUR's entry, and the shape is in the stream-K macro-tiles' range (6.)
    if tuned is not None and tuned["tile"] >= DMA_TILE_FIRST \
            and channels > (SK_MAX_CHANNELS if tuned["tile"] >= SK_TILE_FIRST else DMA_MAX_CHANNELS):
        tuned = None                       # 3. the LDS-DMA tiles address at most 4032 channels per tap (a neighbour's tile may be one)
    if tuned is not None:
        tile = tuned["tile"]
        if lean and tile not in _LEAN_TILES and tuned["split_k"] == 1 and "insitu" not in tuned:
            # 4. a plain linear layer whose table entry (tuned before csrc/lin_gemm.hip existed: the training steps' shapes) names a
            # tile the lean kernel has no instantiation of -- the 160-wide and the intra-workgroup K-split tiles
            tile = _lean_tile(M)
        # (tables tuned before the XCD-aware orders existed mean the legacy order)
        return tile, tuned["split_k"], bool(tuned.get("in_kernel", 0)), order or tuned.get("order", 1)
    if lean and not (M <= 512 and cin_pad >= 1280):
        # 5. an untuned plain linear layer: a lean tile by row count instead of the library's register-staged pick
        # (tiny M with a long K wants a K split: the library heuristic decides)
        return _lean_tile(M), 1, None, order
    if sk_sized and channels <= SK_MAX_CHANNELS:
        # 6. no table entry: contractions with >= SK_AUTO_MIN_OUTPUTS outputs (a chip-filling number of 256 x 160 macro-tiles) and
        # a long K take the persistent stream-K macro-tiles -- measured 1.28-1.42x the best per-tile launch on such shapes
        # (tools/bench_sk.py: 16384 x 1280 x 11520 at 1,093 TFLOP/s; 8192^3 at 995 against 744) -- and nothing below that
        # size does (0.5-0.98x on every launch of the bs=4 forward, which is why the table holds none)
        return (L.TILE_SK_256x128 if geglu else L.TILE_SK_256x160), 2, True, order or 3      # 256 x 128 for GEGLU's (h, g) column pairs
    return 0, None, None, order            # 7. the library decides


# in_kernel: choose_launch's answer; explicit: the caller gave split_k; reduce_launch: the reduce launch is needed anyway (it
# applies the fused GroupNorm; ops.conv_gemm refuses gn= together with rowstats and clears colstats, so nothing is lost by
# answering first for it); rowstats / colstats: the launch is to emit row / column statistics
def splitk_in_kernel(split_k, in_kernel, *, explicit, reduce_launch, rowstats, colstats) -> bool:
    """whether a launch of split_k > 1 slices combines them itself (True) or leaves them to the reduce launch"""
    if reduce_launch:
        return False
    if SPLITK_FORCE_IN_KERNEL:
        return True                        # (A/B switch: every split launch combines its slices itself, no reduce launches)
    if in_kernel is None:
        in_kernel = split_k <= 4 or explicit       # tuned per shape; untuned shapes combine in-kernel up to 4 slices
    # only the workgroup that combines the slices can emit row / column statistics.  Column statistics are worth the
    # in-kernel form up to 2 slices (beyond that it loses more than the GroupNorm statistics pass it saves: measured
    # +8 us on the 4-slice level-32 convs against a 6.5 us pass + a kernel boundary)
    return in_kernel or rowstats or (colstats and split_k <= COLS_SPLIT_MAX)
