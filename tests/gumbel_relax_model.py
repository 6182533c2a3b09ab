"""fp64 restatement of the router's seeded Gumbel-sigmoid relaxation (csrc/gumbel_relax.h) on tests/philox_oracle.py:
the stream (row seed, Philox draw, element -> word -> u in (0, 1] -> G), the forward in torch fp64 (so autograd gives the backward)
and the non-zero-width decision with the margin it was taken at.
    draw    8 d + sub for sample rows (sub 6: assignment, 7: relaxation);  2^63 | noise_step for codebook rows
    element c for width column c;  nw + j for the depth entry at sorted position j
    G       -log(1e-20 - log(u)),  u = ((word >> 8) + 1) 2^-24
    width   w = sigmoid((z + G + base) / T);  a segment with no w >= 0.5 gets + 0.5 on its first entry
    depth   p = flip(cumsum(softmax(zd))),  x = log(p + 1e-6) - log1p(-(p - 1e-6)),  d_sorted = sigmoid((x + G + base) / T),
            out[nw + depth_order[j]] = d_sorted[j]"""
import numpy as np
import torch

from tests import philox_oracle as PO

SUB_ASSIGN, SUB_RELAX = 6, 7
CODEBOOK_BIT = 1 << 63


def philox_draw(d: int, sub: int, codebook: bool = False) -> int:
    return (CODEBOOK_BIT | int(d)) if codebook else 8 * int(d) + int(sub)


def words(seeds, draw: int, n: int, offset: int = 0) -> np.ndarray:
    """uint32 [len(seeds), n]: the word behind every value, `draw` the Philox draw (philox_draw)"""
    return PO.bits_rows([int(s) for s in seeds], draw, offset, n)


def uniforms(w: np.ndarray) -> np.ndarray:
    return ((w >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24


def gumbel(w: np.ndarray) -> np.ndarray:
    """float64: the Gumbel values of the words"""
    return -np.log(1e-20 - np.log(uniforms(w)))


def seg_starts(widths):
    return [0] + np.cumsum(list(widths)).tolist()


def forward(z: torch.Tensor, G: torch.Tensor, widths, depth_order, T: float, base: float, non_zero_width: bool = True):
    """z, G fp64 [R, nw + nd] (G in ELEMENT order: width columns, then sorted depth positions) -> out fp64 [R, nw + nd], differentiable
    in z; also dead bool [R, n_seg] (the rule's decision) and margin fp64 [R, n_seg] (min over the segment of |z + G + base|)"""
    nw, nd = int(sum(widths)), len(depth_order)
    zw, zd = z[:, :nw], z[:, nw:]
    lw = zw + G[:, :nw] + base
    w = torch.sigmoid(lw / T)
    starts = seg_starts(widths)
    dead = torch.stack([(lw[:, a:b] < 0).all(dim=1) for a, b in zip(starts[:-1], starts[1:])], dim=1) if widths else \
        torch.zeros((z.shape[0], 0), dtype=torch.bool)
    margin = torch.stack([lw[:, a:b].detach().abs().min(dim=1).values for a, b in zip(starts[:-1], starts[1:])], dim=1) if widths else \
        torch.zeros((z.shape[0], 0), dtype=torch.float64)
    if non_zero_width and widths:
        bump = torch.zeros_like(w)
        bump[:, starts[:-1]] = 0.5 * dead.to(w.dtype)
        w = w + bump
    if nd:
        p = torch.flip(torch.cumsum(torch.softmax(zd, dim=1), dim=1), dims=[1])
        x = torch.log(p + 1e-6) - torch.log1p(-(p - 1e-6))
        d_sorted = torch.sigmoid((x + G[:, nw:] + base) / T)
        order = torch.as_tensor([int(o) % nd for o in depth_order], dtype=torch.long)
        d = torch.zeros_like(d_sorted).index_copy(1, order, d_sorted)
    else:
        d = zd
    return torch.cat([w, d], dim=1), dead, margin


def relax(z, seeds, d: int, sub: int, widths, depth_order, T, base, non_zero_width=True, codebook=False):
    """the whole stage from the seeds: (out, dead, margin, G) with z given in any float dtype (read as fp64)"""
    z64 = z.detach().double().cpu()
    E = z64.shape[1]
    G = torch.from_numpy(gumbel(words(seeds, philox_draw(d, sub, codebook), E)))
    out, dead, margin = forward(z64, G, widths, depth_order, T, base, non_zero_width)
    return out, dead, margin, G


def blocks_order(G: torch.Tensor, nw: int) -> torch.Tensor:
    """the noise in the order estimation_utils.sample_gumbel_blocks hands it to gumbel_sigmoid_trick: depth block first"""
    return torch.cat([G[:, nw:], G[:, :nw]], dim=1)


def make_quantizer(widths, depth_order, T: float, base: float, non_zero_width: bool = True, structure=None):
    """a StructureVectorQuantizer whose relaxation has this geometry (the first len(depth_order) blocks carry a depth gate)"""
    from diffusion_pruning_amd.quantizer import StructureVectorQuantizer
    nd = len(depth_order)
    if structure is None:
        assert nd <= len(widths)
        structure = {"width": [[int(w)] for w in widths], "depth": [[1] if i < nd else [0] for i in range(len(widths))]}
    torch.manual_seed(0)
    return StructureVectorQuantizer(n_e=2, structure=structure, temperature=T, base=base, depth_order=list(depth_order),
                                    non_zero_width=non_zero_width, resource_aware_normalization=False).train()


def torch_noise(w: np.ndarray, device="cpu") -> torch.Tensor:
    """the existing fp32 noise formula (estimation_utils.sample_gumbel_blocks) on the exact uniforms of the words"""
    u = torch.from_numpy(uniforms(w)).float().to(device)
    return -torch.log(1e-20 - torch.log(u + 1e-20))


def torch_relax(qz, z: torch.Tensor, G32: torch.Tensor) -> torch.Tensor:
    """quantizer.gumbel_sigmoid_trick -- the function the reference's golden vectors pin -- on injected noise (G32 in element order)"""
    from diffusion_pruning_amd import quantizer as QZ
    nw = sum(qz.width_list)
    real = QZ.sample_gumbel_blocks
    QZ.sample_gumbel_blocks = lambda batch, widths, **kw: blocks_order(G32, nw)[:batch].to(z.device)
    try:
        return qz.gumbel_sigmoid_trick(z)
    finally:
        QZ.sample_gumbel_blocks = real
