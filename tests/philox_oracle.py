"""numpy restatement of the project's seeded normal stream (csrc/philox_normal.h): Philox4x32-10 in uint32 / uint64, the two
uniforms of a pair exactly as the kernel forms them (they are exact in fp32, so also in fp64), and Box-Muller in fp64.
    key      (seed & 0xffffffff, seed >> 32), the seed read as uint64
    element  g = offset + e, blk = g >> 2, lane = g & 3
    counter  (blk & 0xffffffff, blk >> 32, draw & 0xffffffff, draw >> 32)
    lanes    ra cos(2 pi u2a), ra sin(2 pi u2a), rb cos(2 pi u2b), rb sin(2 pi u2b),  r = sqrt(-2 ln u1)
             u1 = ((x >> 8) + 1) 2^-24,  u2 = (x >> 8) 2^-24 from (x0, x1) and (x2, x3)"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints), key: two; returns the four uint32 output arrays"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                                  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def _blocks(seed, draw, offset, n):
    """the words of every block that elements offset .. offset + n - 1 touch: (x [4, nblocks] uint32, first block, g)"""
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    g = np.arange(n, dtype=np.uint64) + np.uint64(offset)
    b0, b1 = int(offset) >> 2, (int(offset) + n - 1) >> 2
    blk = np.arange(b1 - b0 + 1, dtype=np.uint64) + np.uint64(b0)
    x = philox4x32_10([blk & MASK, blk >> S32, draw & 0xFFFFFFFF, draw >> 32], (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(x), b0, g


def bits(seed, draw, offset, n):
    """uint32 [n]: the word behind every element"""
    x, b0, g = _blocks(seed, draw, offset, n)
    return x[(g & np.uint64(3)).astype(np.int64), ((g >> np.uint64(2)) - np.uint64(b0)).astype(np.int64)]


def normals(seed, draw, offset, n):
    """float64 [n]: the normals, Box-Muller in fp64 on the exact uniforms"""
    x, b0, g = _blocks(seed, draw, offset, n)
    two24 = 2.0 ** -24
    z = np.empty((4, x.shape[1]))
    for pair in (0, 1):
        u1 = ((x[2 * pair] >> np.uint32(8)).astype(np.float64) + 1.0) * two24
        u2 = (x[2 * pair + 1] >> np.uint32(8)).astype(np.float64) * two24
        r = np.sqrt(-2.0 * np.log(u1))
        z[2 * pair], z[2 * pair + 1] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
    return z[(g & np.uint64(3)).astype(np.int64), ((g >> np.uint64(2)) - np.uint64(b0)).astype(np.int64)]


def normals_rows(seeds, draw, offset, n):
    """float64 [len(seeds), n]"""
    return np.stack([normals(s, draw, offset, n) for s in seeds])


def bits_rows(seeds, draw, offset, n):
    return np.stack([bits(s, draw, offset, n) for s in seeds])
