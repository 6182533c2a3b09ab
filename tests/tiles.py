"""The rows of csrc/conv_gemm_tiles.h, the one table of aptp_conv_gemm's tile ids, for tests and tools: TILES is a list of
records in id order (TILES[0] is id 1), BY_ID maps id -> record.  No library needed, so modules can use it at collection."""
import os
import re
from collections import namedtuple

Tile = namedtuple("Tile", "id name family bm bn wm wn stages ku ks lin c3")

TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffusion_pruning_amd", "csrc", "conv_gemm_tiles.h")
_ROW = re.compile(r"^\s*X\((\w+),\s*(\w+)," + r"\s*(\d+)," * 8 + r"\s*(\d+)\)", re.M)

TILES = [Tile(i + 1, m[0], m[1], *map(int, m[2:])) for i, m in enumerate(_ROW.findall(open(TABLE).read()))]
BY_ID = {t.id: t for t in TILES}
ALL = tuple(t.id for t in TILES)                              # every id a launch can ask for (0 = auto is none of them)


def ids(pred):
    """ids of the tiles with a property, in id order: ids(lambda t: t.family == "HALO")"""
    return tuple(t.id for t in TILES if pred(t))


REG = ids(lambda t: t.family == "REG")                        # register-staged: the only ones with an fp32 parity instantiation
HALO = ids(lambda t: t.family == "HALO")                      # 3x3 / stride-1 / pad-1, widths 16 / 32 / 64 only
SK = ids(lambda t: t.family in ("SK", "SKL"))                 # persistent stream-K (conv_gemm_sk.hip)
WIDE160 = ids(lambda t: t.bn == 160)                          # GEGLU refuses them
LIN = ids(lambda t: t.lin)                                    # lin_gemm.hip has a lean instantiation
C3 = ids(lambda t: t.c3)                                      # conv_lean.hip has one
