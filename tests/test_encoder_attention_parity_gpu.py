"""Elementwise and per-block accuracy of the three attention kernels outside the U-Net -- ops.attention_causal (CLIP text),
ops.attention_bias (MPNet) and ops.attention_wide (VAE mid-block), bf16 and their fp32 parity instantiations -- against the fp64
reference, the hard bounds and the bf16 format models of tests/encoder_attention_model.py.  tests/test_encoder_attention_model_host.py
proves on the CPU that these metrics pass the sound forms of the model and fail each seeded defect, among them a truncating bf16
store, a truncated P and a row lost at B = 64, which the whole-tensor rel-L2 of the older tests lets through.

What the cases reach (ids name the kernel, the shape, and for the bias kernel the mask and the table):
  causal   L at and around the strip and 32-key-step edges (15/16/17, 31/32/33), L = 33 (stage_kv rounds up to 64 rows, the odd
           tile count writes a zero tile), L = 112 (seven strips: wave 3 has one), 127 / 128, key 0 as an attention sink, and the
           training batch 64 x 16 x 77
  bias     mask_late*: the first 128-key chunk fully masked (the muse = 0 path of attn_bias_kernel, then the first finite maximum);
           mask_middle*: a fully masked chunk between two others; table_rising: the running maximum moves at every chunk change
           (alpha ~ e^-10); table_falling: it never moves and later chunks are rounded far below it; prefix masks with kend at
           1 / 16 / 17 / 128 / 129, among them query blocks with qbase >= kend; an all-masked sample beside valid ones
  wide     Lk odd (the clamped partner of the last key pair), Lk <= 16 (half of the waves see only masked keys), Lk one past a
           tile, one spiked key, explicit scales
Every output buffer is NaN-filled before the launch, so a row that is not written fails the hard bound.  Every assertion goes
through margins.check; no launch is repeated.  The committed record is profiles/encoder_attention_parity_margins.json."""
import pytest
import torch

from tests import encoder_attention_model as EM
from tests import margins

pytestmark = pytest.mark.gpu

BY_ID = {c.id: c for c in EM.CASES}
F32_IDS = [c.id for c in EM.CASES if c.f32]
EXACT = 0.5          # the tolerance of a count that must be zero (margins records measured / tolerance, so not 0)
SENTINEL = {torch.bfloat16: (torch.int16, 0x5A5B), torch.float32: (torch.int32, 0x5A5B5A5B)}


@pytest.fixture(scope="module")
def ops(cuda):
    from diffusion_pruning_amd import ops as o
    o._lib.load()
    return o


def _operands(case, ins, dtype, cuda):
    """q, k, v as contiguous [B, L, heads * D] tensors of ``dtype`` on the device, the fp32 table and mask (or None)"""
    q, k, v = (EM.from_heads(ins[n]).to(dtype).to(cuda) for n in ("q", "k", "v"))
    rb = None if ins["relbias"] is None else ins["relbias"].float().contiguous().to(cuda)
    km = None if ins["mask"] is None else ins["mask"].float().contiguous().to(cuda)
    return q, k, v, rb, km


def _launch(ops, case, q, k, v, rb, km, out):
    if case.kind == "causal":
        return ops.attention_causal(q, k, v, case.heads, scale=case.scale, out=out)
    if case.kind == "bias":
        return ops.attention_bias(q, k, v, case.heads, rb, km, scale=case.scale, out=out)
    return ops.attention_wide(q, k, v, scale=case.scale, out=out)


def _nan_out(case, dtype, cuda):
    return torch.full((case.B, case.Lq, case.heads * case.D), float("nan"), dtype=dtype, device=cuda)


def _heads(case, o):
    return EM.to_heads(o.double().cpu(), case.heads)


def _assert_bf16(case, got, what):
    """got: [B, heads, Lq, D] fp64 on the CPU"""
    _, ref, mdl = EM.case_reference(case)
    hu, br = EM.measure(case, got, ref, mdl)
    print(f"{what}: hard_use {hu:.4f} block_ratio {br:.4f}")
    margins.check(hu, EM.HARD_LIMIT, what + " hard_use")
    if case.ratio:
        margins.check(br, EM.RATIO_LIMIT, what + " block_ratio")
    else:
        margins.check(hu, EM.HARD_LIMIT, what + f" hard_use again: block_ratio {br:.3f} recorded only ({case.why})")
    zr = ref["zero_rows"]
    if zr is not None:
        # the padding contract: whole strips at or past kend (and so every strip of a query block with qbase >= kend) exactly zero
        rows = zr[:, None, :, None].expand_as(got)
        margins.check(float((got[rows] != 0).sum()), EXACT, what + f" nonzero elements in the {int(zr.sum())} zero rows")


def _assert_f32(case, got, what):
    _, ref, _ = EM.case_reference(case, f32=True)
    hu = EM.hard_use(got, ref["o"], ref["b32"])
    print(f"{what}: fp32 hard_use {hu:.4f}")
    margins.check(hu, EM.HARD_LIMIT, what + " fp32 hard_use")


@pytest.mark.parametrize("cid", list(BY_ID))
def test_bf16_elementwise_and_per_block(ops, cuda, cid):
    case = BY_ID[cid]
    ins, _, _ = EM.case_reference(case)
    out = _nan_out(case, torch.bfloat16, cuda)
    _launch(ops, case, *_operands(case, ins, torch.bfloat16, cuda), out)
    torch.cuda.synchronize()
    _assert_bf16(case, _heads(case, out), cid)


@pytest.mark.parametrize("cid", F32_IDS)
def test_fp32_parity_instantiation_elementwise(ops, cuda, cid):
    """the fp32 kernels compute every row below L (no zero strips); held to the fp32 bound, five orders below one dropped key"""
    case = BY_ID[cid]
    ins, _, _ = EM.case_reference(case, f32=True)
    out = _nan_out(case, torch.float32, cuda)
    _launch(ops, case, *_operands(case, ins, torch.float32, cuda), out)
    torch.cuda.synchronize()
    _assert_f32(case, _heads(case, out), cid)


# ---------------------------------------------------------------------------------------------------------------------
# strided views
# ---------------------------------------------------------------------------------------------------------------------
STRIDED = ["causal-B2-h3-L77-amp1", "bias-B3-h3-L200-mask_prefix1_16_17-table_randn-amp1", "wide-B2-h1-L70x333-amp1"]


def _sentinel_buffer(shape, dtype, cuda):
    it, pat = SENTINEL[dtype]
    return torch.full(shape, pat, dtype=it, device=cuda).view(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cid", STRIDED)
def test_strided_views_bit_equal_and_nothing_outside_the_view_is_touched(ops, cuda, cid, dtype):
    """q, k, v: column (and row) slices of three NaN-filled buffers with different row and batch strides; out: a slice of a
    buffer holding a sentinel bit pattern"""
    case = BY_ID[cid]
    f32 = dtype == torch.float32
    ins, _, _ = EM.case_reference(case, f32=f32)
    q, k, v, rb, km = _operands(case, ins, dtype, cuda)
    B, Lq, Lk, C = case.B, case.Lq, case.Lk, case.heads * case.D
    plain = _nan_out(case, dtype, cuda)
    _launch(ops, case, q, k, v, rb, km, plain)

    def nan_buf(*shape):
        return torch.full(shape, float("nan"), dtype=dtype, device=cuda)

    qb, kb, vb = nan_buf(B, Lq + 3, C + 64), nan_buf(B, Lk, 2 * C + 16), nan_buf(B + 1, Lk + 1, C + 8)
    qv, kv, vv = qb[:, 1:Lq + 1, 64:64 + C], kb[:, :, 8:8 + C], vb[:B, 1:Lk + 1, :C]
    qv.copy_(q), kv.copy_(k), vv.copy_(v)
    ob = _sentinel_buffer((B + 1, Lq + 2, C + 24), dtype, cuda)
    ov = ob[:B, 1:Lq + 1, 8:8 + C]
    assert len({t.stride(1) for t in (qv, kv, vv, ov)}) == 4 and len({t.stride(0) for t in (qv, kv, vv, ov)}) == 4
    _launch(ops, case, qv, kv, vv, rb, km, ov)
    torch.cuda.synchronize()
    it, pat = SENTINEL[dtype]
    what = f"{cid} {'fp32' if f32 else 'bf16'} strided views"
    margins.check(float((ov.contiguous().view(it) != plain.view(it)).sum()), EXACT, what + ": elements that differ in a bit from the contiguous call")
    outside = ob.view(it).clone()
    outside[:B, 1:Lq + 1, 8:8 + C] = pat
    margins.check(float((outside != pat).sum()), EXACT, what + ": sentinel elements changed outside the view")
    (_assert_f32 if f32 else _assert_bf16)(case, _heads(case, ov), what)


# ---------------------------------------------------------------------------------------------------------------------
# the padding contract of the bias kernel
# ---------------------------------------------------------------------------------------------------------------------
PADDING = ["bias-B3-h3-L200-mask_prefix1_16_17-table_randn-amp1", "bias-B3-h3-L384-mask_prefix17_129_128-table_rising-amp1",
           "bias-B3-h3-L200-mask_allmasked-table_randn-amp1"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cid", PADDING)
def test_bias_padding_contract(ops, cuda, cid, dtype):
    """Into a NaN-filled slice of a sentinel buffer.  bf16: every row below L is written; whole strips at or past kend, and every
    strip of a query block with qbase >= kend, are exactly zero; the rows past kend inside the straddling strip hold attention
    values (they meet the bound).  fp32: every row below L is written and meets the fp32 bound.  Nothing outside the view changes."""
    case = BY_ID[cid]
    f32 = dtype == torch.float32
    ins, ref, _ = EM.case_reference(case, f32=f32)
    q, k, v, rb, km = _operands(case, ins, dtype, cuda)
    B, L, C = case.B, case.Lq, case.heads * 64
    ob = _sentinel_buffer((B, L + 16, C + 16), dtype, cuda)
    ov = ob[:, 8:L + 8, 8:8 + C]
    ov.fill_(float("nan"))
    ops.attention_bias(q, k, v, case.heads, rb, km, out=ov)
    torch.cuda.synchronize()
    it, pat = SENTINEL[dtype]
    what = f"{cid} {'fp32' if f32 else 'bf16'} padding contract"
    margins.check(float(torch.isnan(ov.float()).sum()), EXACT, what + ": elements below L left unwritten")
    outside = ob.view(it).clone()
    outside[:, 8:L + 8, 8:8 + C] = pat
    margins.check(float((outside != pat).sum()), EXACT, what + ": sentinel elements changed outside the view")
    got = _heads(case, ov)
    if f32:
        _assert_f32(case, got, what)
        return
    _assert_bf16(case, got, what)                       # (zero rows exactly zero; every other row inside the bound)
    zr = ref["zero_rows"]
    kend = (ins["mask"] != 0).double().mul(torch.arange(1, L + 1)).amax(-1)
    straddle = (torch.arange(L)[None, :] >= kend[:, None]) & ~zr                     # past kend, inside the straddling strip
    assert int(zr.sum()) > 0 and int(straddle.sum()) > 0
    nz = got[straddle[:, None, :, None].expand_as(got)]
    margins.check(float((nz == 0).double().mean()), 0.01, what + f": share of exact zeros in the {int(straddle.sum())} straddling rows past kend")
    if "384" in cid:                                                                  # sample 0: kend = 17, blocks at 128 and 256
        margins.check(float((got[0, :, 128:] != 0).sum()), EXACT, what + ": nonzero elements in query blocks with qbase >= kend")


# ---------------------------------------------------------------------------------------------------------------------
# masked keys
# ---------------------------------------------------------------------------------------------------------------------
MASKED = ["bias-B2-h3-L200-mask_late139-table_rising-amp1", "bias-B2-h1-L300-mask_late130-table_randn-amp2",
          "bias-B2-h3-L300-mask_middle128_255-table_falling-amp1"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cid", MASKED)
def test_masked_keys_weigh_exactly_zero_under_whole_masked_chunks(ops, cuda, cid, dtype):
    """K and V at masked keys replaced by junk of magnitude 1e4: no bit of any row changes (every row here has valid keys)"""
    case = BY_ID[cid]
    ins, _, _ = EM.case_reference(case)
    q, k, v, rb, km = _operands(case, ins, dtype, cuda)
    base = ops.attention_bias(q, k, v, case.heads, rb, km, out=_nan_out(case, dtype, cuda))
    dead = (km == 0)[..., None]
    g = torch.Generator().manual_seed(9)
    junk = (1e4 * torch.randn(v.shape, generator=g)).to(dtype).to(cuda)
    other = ops.attention_bias(q, torch.where(dead, junk, k).contiguous(), torch.where(dead, -junk, v).contiguous(), case.heads, rb, km,
                               out=_nan_out(case, dtype, cuda))
    torch.cuda.synchronize()
    it = SENTINEL[dtype][0]
    what = f"{cid} {'fp32' if dtype == torch.float32 else 'bf16'} junk at masked keys"
    margins.check(float(torch.isnan(base.float()).sum()), EXACT, what + ": non-finite outputs")
    margins.check(float((base.view(it) != other.view(it)).sum()), EXACT, what + ": elements that change in a bit")
