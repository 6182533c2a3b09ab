"""The decoder half of SD-2.1's ``AutoencoderKL`` (diffusers 0.23.1 semantics) on the HIP kernels of this package.

The reference turns latents into images with ``vae.decode(latents / vae.config.scaling_factor)`` followed by
``image_processor.postprocess`` (pdm/pipelines/pruning_pipelines.py:826-839).  This module keeps diffusers' parameter names
(``post_quant_conv``, ``decoder.conv_in``, ``decoder.mid_block.{resnets,attentions}``, ``decoder.up_blocks.i.{resnets,
upsamplers}``, ``decoder.conv_norm_out``, ``decoder.conv_out``) and the ``decode(z, return_dict=True).sample`` call, and runs
every layer through the existing kernels:

  * GroupNorm(32, eps 1e-6) (+SiLU): ``ops.groupnorm``, fed by the column statistics its producing convolution emitted;
  * 3x3 convolutions: ``ops.conv_gemm``; nearest x2 upsampling folded into the gather (``ups=1``); a resnet's 1x1
    ``conv_shortcut`` as a second K-segment of conv2 (``pack_weight_cat``); the identity residual in the epilogue;
  * mid-block attention: one fused q|k|v linear with bias, ``ops.attention_wide`` (one head of width 512), ``to_out`` with
    the residual in its epilogue;
  * ``conv_out`` with an fp32 output, then ``ops.unet_epilogue`` (NCHW ``.sample``) or ``ops.image_out`` (postprocessed).

The encoder half (``AutoencoderKL(with_encoder=True)``: ``encoder.*`` and ``quant_conv``, ``encode(x).latent_dist``) runs
the same way: ``ops.image_in`` writes the 3x3 im2col of the image so that ``encoder.conv_in`` is a 1x1 contraction over 32
channels; resnets and the mid-block as in the decoder; Downsample2D (``F.pad(x, (0, 1, 0, 1))`` + a stride-2, pad-0 3x3
convolution) is ``ops.conv_gemm(stride=2, pad=0, pad_end=1)``; ``conv_out`` with an fp32 output, then ``ops.latent_dist``
applies ``quant_conv`` and writes diffusers' moments (and, for ``encode_latents``, the scaled sample) in one launch.

The latents' NCHW -> NHWC change (4 channels, zero padded to 8) is the only torch arithmetic on the decode path.
With ``ops.ACT_DTYPE = torch.float32`` the same code runs the fp32 parity instantiations of every kernel.

Batch slicing: the convolution kernels address an operand with 32-bit byte offsets (buffer resources; ``aptp_conv_gemm``
refuses an operand of 2 GiB or more) and the GroupNorm kernels with 64-bit offsets.  ``slice_plan`` splits the batch so
that no activation of one slice reaches ``MAX_TENSOR_BYTES`` -- diffusers' VAE slicing, done automatically.
"""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .loading import load_strict, read_pretrained, read_safetensors  # noqa: F401  (vae.read_safetensors: the old home)
from .modules import LinearP, PlannedModule, _PlanCache, _versions
from .unet import Conv2dP, NormP


@dataclass(frozen=True)
class VAEConfig:
    """SD-2.1 ``vae/config.json`` (the fields the decoder uses)."""
    in_channels: int = 3
    out_channels: int = 3
    latent_channels: int = 4
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    scaling_factor: float = 0.18215
    sample_size: int = 768

    @classmethod
    def from_dict(cls, d: dict) -> "VAEConfig":
        kw = {f.name: d[f.name] for f in fields(cls) if f.name in d}
        if "block_out_channels" in kw:
            kw["block_out_channels"] = tuple(kw["block_out_channels"])
        return cls(**kw)


GN_EPS = 1e-6
# largest activation of one decode slice the kernels were verified for (bytes): aptp_conv_gemm's buffer-resource offsets are
# 32-bit and it rejects operands of >= 2 GiB; every other kernel on the path uses 64-bit offsets
MAX_TENSOR_BYTES = (1 << 31) - (1 << 20)


def _largest(ch: List[int], H: int, W: int, first: int, up: bool) -> int:
    """largest H x W x channels product along the levels ``ch``, starting from ``first`` channels at H x W"""
    big = H * W * first
    prev = ch[0]
    for i, c in enumerate(ch):
        big = max(big, H * W * max(prev, c))
        prev = c
        if i < len(ch) - 1:
            H, W = (2 * H, 2 * W) if up else (H // 2, W // 2)
            big = max(big, H * W * c)
    return big


def largest_activation_elements(cfg: VAEConfig, h: int, w: int) -> int:
    """elements of the largest activation of ONE image (the input of the last level's first resnet for SD-2.1:
    8h x 8w x 256)"""
    ch = list(reversed(cfg.block_out_channels))
    return _largest(ch, h, w, max(ch[0], cfg.latent_channels), True)


def encoder_largest_activation_elements(cfg: VAEConfig, H: int, W: int) -> int:
    """elements of the largest activation of ONE H x W image in the encoder (image_in's 32 columns or conv_in's output at
    full resolution for SD-2.1: H x W x 128)"""
    ch = list(cfg.block_out_channels)
    return _largest(ch, H, W, max(32, ch[0]), False)


def _slices(per: int, batch: int, what: str) -> List[int]:
    """batch sizes of the slices of a pass whose largest activation is ``per`` bytes per image: as few as possible, each
    below MAX_TENSOR_BYTES in every activation"""
    if per >= MAX_TENSOR_BYTES:
        raise ValueError(f"{what} image needs a {per} B activation, above the verified {MAX_TENSOR_BYTES} B")
    n = max(1, MAX_TENSOR_BYTES // per)
    return [min(n, batch - s) for s in range(0, batch, n)]


def slice_plan(cfg: VAEConfig, batch: int, h: int, w: int, elem_bytes: int = 2) -> List[int]:
    """batch sizes of the decode slices"""
    return _slices(largest_activation_elements(cfg, h, w) * elem_bytes, batch, f"decode: one {8 * h}x{8 * w}")


def encoder_slice_plan(cfg: VAEConfig, batch: int, H: int, W: int, elem_bytes: int = 2) -> List[int]:
    """batch sizes of the encode slices"""
    return _slices(encoder_largest_activation_elements(cfg, H, W) * elem_bytes, batch, f"encode: one {H}x{W}")


def _vae_macs(cfg: VAEConfig, H: int, W: int, encoder: bool) -> Tuple[int, int]:
    """the layer table of one half at H x W (the decoder's latent, the encoder's image): one MAC = one multiply-add; the
    two attention contractions are 2 (hw)^2 C"""
    macs = 0
    ch = list(cfg.block_out_channels) if encoder else list(reversed(cfg.block_out_channels))
    lc = cfg.latent_channels

    def conv(ci, co, k):
        nonlocal macs
        macs += H * W * ci * co * k * k

    def res(ci, co):
        conv(ci, co, 3)
        conv(co, co, 3)
        if ci != co:
            conv(ci, co, 1)

    def mid(c):
        nonlocal macs
        res(c, c)
        for _ in range(4):
            conv(c, c, 1)
        attn = 2 * (H * W) ** 2 * c
        macs += attn
        res(c, c)
        return attn

    def levels(layers):
        nonlocal H, W
        prev = ch[0]
        for i, c in enumerate(ch):
            for j in range(layers):
                res(prev if j == 0 else c, c)
            prev = c
            if i < len(ch) - 1:               # Downsample2D: pad (0, 1, 0, 1), 3x3 stride 2 -> H / 2 for even H
                H, W = (H // 2, W // 2) if encoder else (2 * H, 2 * W)
                conv(c, c, 3)
    if encoder:
        conv(cfg.in_channels, ch[0], 3)
        levels(cfg.layers_per_block)
        attn = mid(ch[-1])
        conv(ch[-1], 2 * lc, 3)
        conv(2 * lc, 2 * lc, 1)
    else:
        conv(lc, lc, 1)
        conv(lc, ch[0], 3)
        attn = mid(ch[0])
        levels(cfg.layers_per_block + 1)
        conv(ch[-1], cfg.out_channels, 3)
    return macs, attn


def vae_decoder_macs(cfg: VAEConfig, h: int, w: int) -> Tuple[int, int]:
    """(MACs per image, attention MACs per image) of the decoder at an h x w latent"""
    return _vae_macs(cfg, h, w, False)


def vae_encoder_macs(cfg: VAEConfig, H: int, W: int) -> Tuple[int, int]:
    """(MACs per image, attention MACs per image) of the encoder plus quant_conv on an H x W image (conv_in counted with
    its 3 real input channels)"""
    return _vae_macs(cfg, H, W, True)


# ----------------------------------------------------------------------------------------------------------------
# parameter containers (diffusers names and shapes)
# ----------------------------------------------------------------------------------------------------------------
class ResnetBlock2DP(nn.Module):
    def __init__(self, cin: int, cout: int, groups: int):
        super().__init__()
        self.in_channels, self.out_channels = cin, cout
        self.norm1 = NormP(cin, GN_EPS, groups)
        self.conv1 = Conv2dP(cin, cout, 3)
        self.norm2 = NormP(cout, GN_EPS, groups)
        self.conv2 = Conv2dP(cout, cout, 3)
        self.conv_shortcut = Conv2dP(cin, cout, 1) if cin != cout else None


class AttentionP(nn.Module):
    def __init__(self, c: int, groups: int):
        super().__init__()
        self.group_norm = NormP(c, GN_EPS, groups)
        self.to_q = LinearP(c, c)
        self.to_k = LinearP(c, c)
        self.to_v = LinearP(c, c)
        self.to_out = nn.ModuleList([LinearP(c, c)])


class UNetMidBlock2DP(nn.Module):
    def __init__(self, c: int, groups: int):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2DP(c, c, groups), ResnetBlock2DP(c, c, groups)])
        self.attentions = nn.ModuleList([AttentionP(c, groups)])


class Upsample2DP(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.conv = Conv2dP(c, c, 3)


class UpDecoderBlock2DP(nn.Module):
    def __init__(self, cin: int, cout: int, layers: int, groups: int, add_upsample: bool):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2DP(cin if j == 0 else cout, cout, groups) for j in range(layers)])
        self.upsamplers = nn.ModuleList([Upsample2DP(cout)]) if add_upsample else None


class DecoderP(nn.Module):
    def __init__(self, cfg: VAEConfig):
        super().__init__()
        ch = list(reversed(cfg.block_out_channels))
        g = cfg.norm_num_groups
        self.conv_in = Conv2dP(cfg.latent_channels, ch[0], 3)
        self.mid_block = UNetMidBlock2DP(ch[0], g)
        blocks, prev = [], ch[0]
        for i, c in enumerate(ch):
            blocks.append(UpDecoderBlock2DP(prev, c, cfg.layers_per_block + 1, g, i < len(ch) - 1))
            prev = c
        self.up_blocks = nn.ModuleList(blocks)
        self.conv_norm_out = NormP(ch[-1], GN_EPS, g)
        self.conv_out = Conv2dP(ch[-1], cfg.out_channels, 3)


class Downsample2DP(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.conv = Conv2dP(c, c, 3)


class DownEncoderBlock2DP(nn.Module):
    def __init__(self, cin: int, cout: int, layers: int, groups: int, add_downsample: bool):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2DP(cin if j == 0 else cout, cout, groups) for j in range(layers)])
        self.downsamplers = nn.ModuleList([Downsample2DP(cout)]) if add_downsample else None


class EncoderP(nn.Module):
    def __init__(self, cfg: VAEConfig):
        super().__init__()
        ch = list(cfg.block_out_channels)
        g = cfg.norm_num_groups
        self.conv_in = Conv2dP(cfg.in_channels, ch[0], 3)
        blocks, prev = [], ch[0]
        for i, c in enumerate(ch):
            blocks.append(DownEncoderBlock2DP(prev, c, cfg.layers_per_block, g, i < len(ch) - 1))
            prev = c
        self.down_blocks = nn.ModuleList(blocks)
        self.mid_block = UNetMidBlock2DP(ch[-1], g)
        self.conv_norm_out = NormP(ch[-1], GN_EPS, g)
        self.conv_out = Conv2dP(ch[-1], 2 * cfg.latent_channels, 3)      # double_z


@dataclass
class DecoderOutput:
    sample: torch.Tensor


def randn_tensor(shape, generator=None, device=None, dtype=torch.float32) -> torch.Tensor:
    """diffusers.utils.torch_utils.randn_tensor: a CPU generator draws on the CPU and the result moves to ``device``; a list of
    generators draws one sample each"""
    device = torch.device(device) if device is not None else torch.device("cpu")
    if isinstance(generator, (list, tuple)):
        if len(generator) == 1:
            generator = generator[0]
        else:
            return torch.cat([randn_tensor((1,) + tuple(shape[1:]), g, device, dtype) for g in generator], 0)
    rand_device = device
    if generator is not None and generator.device.type != device.type and generator.device.type == "cpu":
        rand_device = torch.device("cpu")
    return torch.randn(tuple(shape), generator=generator, device=rand_device, dtype=dtype).to(device)


class DiagonalGaussianDistribution:
    """diffusers 0.23.1 ``DiagonalGaussianDistribution``.  ``parameters`` are the moments [B, 2z, h, w] (mean | logvar).
    On the GPU ``sample`` draws eps like ``randn_tensor`` and runs ``ops.latent_dist`` (identity quant_conv, scale 1), so
    that it is the same kernel arithmetic as ``AutoencoderKL.encode_latents``; on the CPU it is diffusers' torch formula."""

    def __init__(self, parameters: torch.Tensor, deterministic: bool = False):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        if self.deterministic:
            self.var = self.std = torch.zeros_like(self.mean, device=self.parameters.device, dtype=self.parameters.dtype)

    def sample(self, generator=None) -> torch.Tensor:
        eps = randn_tensor(self.mean.shape, generator=generator, device=self.parameters.device, dtype=self.parameters.dtype)
        p = self.parameters
        if p.is_cuda and p.dtype == torch.float32 and p.shape[1] == 8 and not self.deterministic:
            y = p.permute(0, 2, 3, 1).contiguous()                 # moments as [B, h, w, 8]: quant_conv = identity
            eye = torch.eye(8, dtype=torch.float32, device=p.device)
            _, lat = ops.latent_dist(y, eye, torch.zeros(8, dtype=torch.float32, device=p.device), eps=eps.contiguous(),
                                     scale=1.0, moments=False)
            return lat
        return self.mean + self.std * eps

    def kl(self, other: Optional["DiagonalGaussianDistribution"] = None) -> torch.Tensor:
        if self.deterministic:
            return torch.Tensor([0.0])
        if other is None:
            return 0.5 * torch.sum(torch.pow(self.mean, 2) + self.var - 1.0 - self.logvar, dim=[1, 2, 3])
        return 0.5 * torch.sum(torch.pow(self.mean - other.mean, 2) / other.var + self.var / other.var - 1.0 - self.logvar
                               + other.logvar, dim=[1, 2, 3])

    def nll(self, sample: torch.Tensor, dims=(1, 2, 3)) -> torch.Tensor:
        if self.deterministic:
            return torch.Tensor([0.0])
        logtwopi = np.log(2.0 * np.pi)
        return 0.5 * torch.sum(logtwopi + self.logvar + torch.pow(sample - self.mean, 2) / self.var, dim=list(dims))

    def mode(self) -> torch.Tensor:
        return self.mean


@dataclass
class AutoencoderKLOutput:
    latent_dist: DiagonalGaussianDistribution


_DEPRECATED_ATTN = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}


def _rename_deprecated(name: str) -> str:
    head, _, leaf = name.rpartition(".")           # leaf = weight / bias
    mod_path, _, mod = head.rpartition(".")
    if mod in _DEPRECATED_ATTN and ".attentions." in name:
        return f"{mod_path}.{_DEPRECATED_ATTN[mod]}.{leaf}"
    return name


def _flatten_1x1(name: str, t: torch.Tensor) -> torch.Tensor:
    """attention weights some checkpoints keep as 1x1 convolutions -> linear weights"""
    if ".attentions." in name and name.endswith("weight") and t.dim() == 4 and t.shape[2:] == (1, 1):
        return t[:, :, 0, 0]
    return t


# ----------------------------------------------------------------------------------------------------------------
# packed weights of the layers both halves are made of
# ----------------------------------------------------------------------------------------------------------------
def _f32(t: torch.Tensor, dev) -> torch.Tensor:
    return t.detach().float().to(dev).contiguous()


def _pack_conv(m, dev) -> ops.PackedWeight:
    return ops.pack_weight(m.weight.detach(), m.bias.detach(), device=dev)


def _pack_gn(m, dev):
    return _f32(m.weight, dev), _f32(m.bias, dev)


def _pack_res(r, dev) -> dict:
    e = {"g1": _pack_gn(r.norm1, dev), "g2": _pack_gn(r.norm2, dev), "w1": _pack_conv(r.conv1, dev)}
    w2 = _pack_conv(r.conv2, dev)
    if r.conv_shortcut is not None:
        w2 = ops.pack_weight_cat(w2, r.conv_shortcut.weight.detach(), r.conv_shortcut.bias.detach())
    e["w2"], e["shortcut"] = w2, r.conv_shortcut is not None
    return e


def _pack_mid(mid, dev) -> dict:
    """the mid-block's entries of a plan: resnet, attention (q|k|v as one linear), resnet"""
    a = mid.attentions[0]
    wqkv = torch.cat([a.to_q.weight, a.to_k.weight, a.to_v.weight], 0).detach()
    bqkv = torch.cat([a.to_q.bias, a.to_k.bias, a.to_v.bias], 0).detach()
    return {"mid0": _pack_res(mid.resnets[0], dev),
            "attn": {"g": _pack_gn(a.group_norm, dev), "qkv": ops.pack_weight(wqkv, bqkv, device=dev),
                     "out": _pack_conv(a.to_out[0], dev)},
            "mid1": _pack_res(mid.resnets[1], dev)}


def _act_bytes() -> int:
    return torch.tensor([], dtype=ops.ACT_DTYPE).element_size()


def _sliced(domain: str, sizes: List[int], one):
    """one(b0, b1) for every batch slice, under the scratch domain ``domain``"""
    with ops.scratch_domain(domain):
        b0 = 0
        for n in sizes:
            one(b0, b0 + n)
            b0 += n


def _nhwc_padded(x: torch.Tensor, cin: int) -> torch.Tensor:
    """NCHW [B, C, H, W] -> ops.ACT_DTYPE NHWC [B, H, W, cin] with zero padding channels"""
    B, C, H, W = x.shape
    y = torch.zeros(B, H, W, cin, dtype=ops.ACT_DTYPE, device=x.device)
    y[..., :C] = x.permute(0, 2, 3, 1)
    return y


# ----------------------------------------------------------------------------------------------------------------
# the module
# ----------------------------------------------------------------------------------------------------------------
class AutoencoderKL(PlannedModule):
    """Decode half of diffusers' AutoencoderKL.  ``decode(z)`` equals diffusers' ``vae.decode(z)`` (z = latents /
    scaling_factor, NCHW); ``decode_images`` returns the postprocessed image in one more launch.
    ``with_encoder=True`` adds ``encoder`` and ``quant_conv``: ``encode(x).latent_dist`` equals diffusers' ``vae.encode(x)``
    (x = pixel_values in [-1, 1], NCHW), ``encode_latents(x, g)`` is the trainer's ``encode(x).latent_dist.sample() *
    scaling_factor`` in one pass."""

    def __init__(self, config: Optional[VAEConfig] = None, with_encoder: bool = False, **kw):
        super().__init__()
        cfg = config or VAEConfig(**kw)
        self.config = cfg
        lc = cfg.latent_channels
        self.post_quant_conv = Conv2dP(lc, lc, 1)
        self.decoder = DecoderP(cfg)
        self.with_encoder = bool(with_encoder)
        if self.with_encoder:
            self.encoder = EncoderP(cfg)
            self.quant_conv = Conv2dP(2 * lc, 2 * lc, 1)
        # encoder.conv_in as a 1x1 contraction over ops.image_in's im2col columns (False: a 3x3 convolution over the image
        # zero padded to 8 channels -- the A/B form of tools/bench_vae_encode.py)
        self.conv_in_im2col = True
        # both halves' plans; 2 dtypes x (decoder + 2 conv_in forms of the encoder) fit unpinned
        self._plans = _PlanCache(cap=8)

    # ---- weights ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def init_synthetic(self, seed: int = 0) -> "AutoencoderKL":
        """Deterministic weights that keep activations O(1) through the 33 3x3 convolutions: He-like convolution weights
        (std 1 / sqrt(fan_in)), GroupNorm affine near identity, small biases; conv2 of every resnet scaled by 0.5 so that the
        15 residual additions grow the stream slowly."""
        g = torch.Generator().manual_seed(seed)
        ge = torch.Generator().manual_seed(seed + 0x5EED)        # encoder weights: the decoder's draws stay as without them
        for name, p in self.named_parameters():
            gen = ge if name.startswith("encoder.") or name.startswith("quant_conv.") else g
            if name.endswith("bias"):
                p.copy_(0.02 * torch.randn(p.shape, generator=gen))
            elif p.dim() == 1:                                   # GroupNorm gamma
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=gen))
            else:
                fan_in = p[0].numel()
                std = fan_in ** -0.5 * (0.5 if name.endswith("conv2.weight") else 1.0)
                p.copy_(std * torch.randn(p.shape, generator=gen))
        self.invalidate()
        return self

    def load_decoder_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Load diffusers VAE weights: ``encoder.*`` / ``quant_conv.*`` are ignored, the deprecated attention names
        (query / key / value / proj_attn) are accepted, 1x1-conv-shaped attention weights are flattened.  Missing or
        mis-shaped keys raise."""
        return load_strict(self, sd, _rename_deprecated, lambda n: n.startswith(("encoder.", "quant_conv.")), _flatten_1x1)

    def load_vae_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Load a whole diffusers VAE state dict (encoder, quant_conv, post_quant_conv, decoder) strictly: every key of this
        module must be present with its shape and no other key may be; the deprecated attention names (query / key / value /
        proj_attn) are accepted in both mid-blocks, 1x1-conv-shaped attention weights are flattened."""
        return load_strict(self, sd, _rename_deprecated, fixup=_flatten_1x1)

    @classmethod
    def from_pretrained(cls, root: str, subfolder: Optional[str] = "vae", with_encoder: bool = False) -> "AutoencoderKL":
        """Read ``config.json`` and ``diffusion_pytorch_model.safetensors`` of a diffusers VAE folder (with_encoder: the
        encoder and quant_conv too, strictly)."""
        cfg, sd = read_pretrained(VAEConfig, root, subfolder, "diffusion_pytorch_model.safetensors")
        m = cls(cfg, with_encoder=with_encoder)
        return m.load_vae_state_dict(sd) if with_encoder else m.load_decoder_state_dict(sd)

    # ---- packed weights ---------------------------------------------------------------------------------------------
    def plan(self, device) -> dict:
        """packed decoder weights, cached per (device, ops.ACT_DTYPE) in the _PlanCache"""
        def make():
            dec, dev = self.decoder, device
            return {"pq": _pack_conv(self.post_quant_conv, dev),
                    "conv_in": _pack_conv(dec.conv_in, dev),
                    **_pack_mid(dec.mid_block, dev),
                    "up": [{"res": [_pack_res(r, dev) for r in blk.resnets],
                            "ups": _pack_conv(blk.upsamplers[0].conv, dev) if blk.upsamplers is not None else None}
                           for blk in dec.up_blocks],
                    "gn_out": _pack_gn(dec.conv_norm_out, dev),
                    "conv_out": _pack_conv(dec.conv_out, dev)}
        return self._plans.lookup(("decoder", str(device), ops.ACT_DTYPE), _versions(self), make)

    def encoder_plan(self, device) -> dict:
        """packed encoder weights (cached like plan(), per conv_in form too)"""
        if not self.with_encoder:
            raise NotImplementedError("AutoencoderKL.encode: this instance holds the decoder only "
                                      "(AutoencoderKL(with_encoder=True) / from_pretrained(..., with_encoder=True))")

        def make():
            enc, dev = self.encoder, device
            ci = enc.conv_in
            return {"conv_in": (ops.pack_conv_in_im2col(ci.weight, ci.bias, device=dev) if self.conv_in_im2col
                                else _pack_conv(ci, dev)),
                    "down": [{"res": [_pack_res(r, dev) for r in blk.resnets],
                              "down": _pack_conv(blk.downsamplers[0].conv, dev) if blk.downsamplers is not None else None}
                             for blk in enc.down_blocks],
                    **_pack_mid(enc.mid_block, dev),
                    "gn_out": _pack_gn(enc.conv_norm_out, dev),
                    "conv_out": _pack_conv(enc.conv_out, dev),
                    "wq": _f32(self.quant_conv.weight[:, :, 0, 0], dev),
                    "bq": _f32(self.quant_conv.bias, dev)}
        return self._plans.lookup(("encoder", str(device), ops.ACT_DTYPE, self.conv_in_im2col), _versions(self), make)

    # ---- forward ----------------------------------------------------------------------------------------------------
    def _resnet(self, x, e):
        G = self.config.norm_num_groups
        a1 = ops.groupnorm(x, e["g1"][0], e["g1"][1], G, GN_EPS, True)
        h = ops.conv_gemm(a1, e["w1"], colstats=True)
        a2 = ops.groupnorm(h, e["g2"][0], e["g2"][1], G, GN_EPS, True)
        if e["shortcut"]:
            return ops.conv_gemm(a2, e["w2"], x2=x, colstats=True)      # conv2(a2) + conv_shortcut(x): one GEMM
        return ops.conv_gemm(a2, e["w2"], residual=x, colstats=True)

    def _attention(self, x, e):
        B, H, W, C = x.shape
        a = ops.groupnorm(x, e["g"][0], e["g"][1], self.config.norm_num_groups, GN_EPS, False)
        qkv = ops.linear(a.reshape(B, H * W, C), e["qkv"])                     # [B, HW, 3C]: to_q | to_k | to_v
        o = ops.attention_wide(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:])
        y = ops.linear(o, e["out"], residual=x.reshape(B, H * W, C), colstats=True)
        return y.reshape(B, H, W, C)

    def _decode_nhwc(self, z: torch.Tensor) -> torch.Tensor:
        """z [B, 4, h, w] -> conv_out's fp32 [B, 8h, 8w, 8] (3 real channels)"""
        pl = self.plan(z.device)
        x = _nhwc_padded(z, pl["pq"].Cin)                                         # the 4-channel layout change
        x = ops.conv_gemm(x, pl["pq"], pad=0)                                     # post_quant_conv (bias: not folded
        x = ops.conv_gemm(x, pl["conv_in"], colstats=True)                        #  across conv_in's zero border)
        x = self._resnet(x, pl["mid0"])
        x = self._attention(x, pl["attn"])
        x = self._resnet(x, pl["mid1"])
        for blk in pl["up"]:
            for e in blk["res"]:
                x = self._resnet(x, e)
            if blk["ups"] is not None:
                x = ops.conv_gemm(x, blk["ups"], ups=1, colstats=True)            # Upsample2D: nearest x2 + 3x3 conv
        g, b = pl["gn_out"]
        a = ops.groupnorm(x, g, b, self.config.norm_num_groups, GN_EPS, True)
        return ops.conv_gemm(a, pl["conv_out"], out_f32=True)

    def _encode_nhwc(self, x: torch.Tensor, pl: dict) -> torch.Tensor:
        """pixel_values [B, 3, H, W] -> conv_out's fp32 [B, H/8, W/8, 8] (diffusers' moments before quant_conv)"""
        f32 = ops.ACT_DTYPE == torch.float32
        if self.conv_in_im2col:
            h = ops.conv_gemm(ops.image_in(x, out_f32=f32), pl["conv_in"], pad=0, colstats=True)   # conv_in: 1x1 over the im2col
        else:
            h = ops.conv_gemm(_nhwc_padded(x, pl["conv_in"].Cin), pl["conv_in"], colstats=True)
        for blk in pl["down"]:
            for e in blk["res"]:
                h = self._resnet(h, e)
            if blk["down"] is not None:                                          # Downsample2D: F.pad (0, 1, 0, 1), 3x3 / 2
                h = ops.conv_gemm(h, blk["down"], stride=2, pad=0, pad_end=1, colstats=True)
        h = self._resnet(h, pl["mid0"])
        h = self._attention(h, pl["attn"])
        h = self._resnet(h, pl["mid1"])
        g, b = pl["gn_out"]
        a = ops.groupnorm(h, g, b, self.config.norm_num_groups, GN_EPS, True)
        return ops.conv_gemm(a, pl["conv_out"], out_f32=True)

    def _check_pixels(self, x: torch.Tensor):
        if not (x.is_cuda and x.dim() == 4 and x.shape[1] == self.config.in_channels
                and x.dtype in (torch.float32, torch.bfloat16)):
            raise ValueError(f"AutoencoderKL.encode: expected CUDA fp32 / bf16 pixel_values [B, {self.config.in_channels}, H, W], "
                             f"got {x.dtype} {tuple(x.shape)} on {x.device}")
        if x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f"AutoencoderKL.encode: H and W must be multiples of 8, got {x.shape[2]}x{x.shape[3]}")

    @torch.no_grad()
    def _encode(self, x: torch.Tensor, eps: Optional[torch.Tensor] = None, scale: float = 1.0, moments: bool = True,
                latents_dtype: torch.dtype = torch.float32):
        """encode slice by slice (encoder_slice_plan) -> (moments fp32 [B, 8, h, w] or None, latents [B, 4, h, w] or None)"""
        pl = self.encoder_plan(x.device)                   # (raises NotImplementedError on a decoder-only instance)
        self._check_pixels(x)
        x = x.contiguous()
        B, _, H, W = x.shape
        h, w = H // 8, W // 8
        z2 = 2 * self.config.latent_channels
        mom = torch.empty(B, z2, h, w, dtype=torch.float32, device=x.device) if moments else None
        lat = None
        if eps is not None:
            if tuple(eps.shape) != (B, z2 // 2, h, w):
                raise ValueError(f"AutoencoderKL.encode: eps shape {tuple(eps.shape)} != {(B, z2 // 2, h, w)}")
            eps = eps.to(device=x.device, dtype=torch.float32).contiguous()
            lat = torch.empty(B, z2 // 2, h, w, dtype=latents_dtype, device=x.device)

        def one(b0, b1):
            ops.latent_dist(self._encode_nhwc(x[b0:b1], pl), pl["wq"], pl["bq"], eps=None if eps is None else eps[b0:b1],
                            scale=scale, moments=moments, latents_dtype=latents_dtype,
                            moments_out=None if mom is None else mom[b0:b1], latents_out=None if lat is None else lat[b0:b1])
        # its own scratch domain: never shares a GroupNorm arena with a captured decode
        _sliced("vae_encoder", encoder_slice_plan(self.config, B, H, W, _act_bytes()), one)
        return mom, lat

    def encode(self, x: torch.Tensor, return_dict: bool = True):
        """diffusers AutoencoderKL.encode: pixel_values [B, 3, H, W] in [-1, 1] -> AutoencoderKLOutput(latent_dist)"""
        mom, _ = self._encode(x)
        dist = DiagonalGaussianDistribution(mom)
        return AutoencoderKLOutput(latent_dist=dist) if return_dict else (dist,)

    def encode_latents(self, x: torch.Tensor, generator=None, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """the trainer's ``vae.encode(x).latent_dist.sample(generator) * scaling_factor`` with the scale folded into the
        sampling launch; eps is drawn like randn_tensor.  With fp32 output it equals the two-step form bit for bit."""
        if not self.with_encoder:
            self.encoder_plan(x.device)                      # raises NotImplementedError
        B, _, H, W = x.shape
        eps = randn_tensor((B, self.config.latent_channels, H // 8, W // 8), generator=generator, device=x.device,
                           dtype=torch.float32)
        _, lat = self._encode(x, eps=eps, scale=self.config.scaling_factor, moments=False, latents_dtype=dtype)
        return lat

    def _check_latents(self, z: torch.Tensor):
        if not (z.is_cuda and z.dim() == 4 and z.shape[1] == self.config.latent_channels):
            raise ValueError(f"AutoencoderKL.decode: expected CUDA latents [B, {self.config.latent_channels}, h, w], "
                             f"got {tuple(z.shape)} on {z.device}")

    @torch.no_grad()
    def _run(self, z: torch.Tensor, finish):
        """decode slice by slice (slice_plan); finish(y_slice, b0, b1) writes the slice's result"""
        self._check_latents(z)
        B, _, h, w = z.shape
        _sliced("vae", slice_plan(self.config, B, h, w, _act_bytes()), lambda b0, b1: finish(self._decode_nhwc(z[b0:b1]), b0, b1))

    def decode(self, z: torch.Tensor, return_dict: bool = True):
        """diffusers AutoencoderKL.decode: z = latents / scaling_factor -> DecoderOutput(sample fp32 [B, 3, 8h, 8w])"""
        B, _, h, w = z.shape
        sample = torch.empty(B, self.config.out_channels, 8 * h, 8 * w, dtype=torch.float32, device=z.device)
        self._run(z, lambda y, b0, b1: ops.unet_epilogue(y, self.config.out_channels, torch.float32, out=sample[b0:b1]))
        return DecoderOutput(sample=sample) if return_dict else (sample,)

    def decode_images(self, z: torch.Tensor, output: str = "pt") -> torch.Tensor:
        """decode + diffusers postprocess (do_denormalize) in the image epilogue kernel: "pt" -> fp32 [B, 3, H, W] in [0, 1],
        "uint8" -> uint8 [B, H, W, 3] rounded like numpy_to_pil"""
        if self.config.out_channels != 3:
            raise ValueError("decode_images: the image epilogue writes 3 channels")
        B, _, h, w = z.shape
        if output == "pt":
            img = torch.empty(B, 3, 8 * h, 8 * w, dtype=torch.float32, device=z.device)
            self._run(z, lambda y, b0, b1: ops.image_out(y, torch.float32, out=img[b0:b1]))
        elif output == "uint8":
            img = torch.empty(B, 8 * h, 8 * w, 3, dtype=torch.uint8, device=z.device)
            self._run(z, lambda y, b0, b1: ops.image_out(y, torch.uint8, out=img[b0:b1]))
        else:
            raise ValueError(f"decode_images: output {output!r} is 'pt' or 'uint8'")
        return img

    def forward(self, z, return_dict: bool = True):
        return self.decode(z, return_dict=return_dict)
