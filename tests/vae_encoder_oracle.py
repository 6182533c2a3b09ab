"""CPU oracle of the AutoencoderKL encoder -- TEST INFRASTRUCTURE ONLY.

A from-scratch restatement, in plain torch modules (run in fp32 or fp64), of diffusers 0.23.1's ``AutoencoderKL.encode``
for SD-2.1's VAE, built from the decoder oracle's blocks (tests/vae_oracle.py).  The semantics restated here:

  encode(x)          = DiagonalGaussianDistribution(quant_conv(encoder(x)))                (autoencoder_kl.py, encode)
  Encoder            = conv_in -> down_blocks[0..3] -> mid_block -> conv_norm_out -> SiLU -> conv_out (double_z: 2 x 4 out)
  DownEncoderBlock2D = resnets[0..1] (-> Downsample2D on blocks 0-2)
  Downsample2D       = F.pad(x, (0, 1, 0, 1)) then a 3x3, stride-2, padding-0 convolution (use_conv, padding=0)
  DiagonalGaussianDistribution: mean, logvar = chunk(parameters, 2, dim=1); logvar = clamp(logvar, -30, 20);
                       std = exp(0.5 logvar); var = exp(logvar); sample = mean + std * eps

``EncoderOracle.state_dict()`` keys are diffusers' ``encoder.*`` and ``quant_conv.*`` keys.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.vae_oracle import ResnetBlock2D, UNetMidBlock2D


class Downsample2D(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, stride=2, padding=0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1), mode="constant", value=0))


class DownEncoderBlock2D(nn.Module):
    def __init__(self, cin: int, cout: int, layers: int, groups: int, add_downsample: bool):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if j == 0 else cout, cout, groups) for j in range(layers)])
        self.downsamplers = nn.ModuleList([Downsample2D(cout)]) if add_downsample else None

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        if self.downsamplers is not None:
            x = self.downsamplers[0](x)
        return x


class Encoder(nn.Module):
    def __init__(self, block_out_channels=(128, 256, 512, 512), layers_per_block=2, in_channels=3, latent_channels=4,
                 groups=32):
        super().__init__()
        ch = list(block_out_channels)
        self.conv_in = nn.Conv2d(in_channels, ch[0], 3, padding=1)
        blocks, prev = [], ch[0]
        for i, c in enumerate(ch):
            blocks.append(DownEncoderBlock2D(prev, c, layers_per_block, groups, i < len(ch) - 1))
            prev = c
        self.down_blocks = nn.ModuleList(blocks)
        self.mid_block = UNetMidBlock2D(ch[-1], groups)
        self.conv_norm_out = nn.GroupNorm(groups, ch[-1], eps=1e-6)
        self.conv_out = nn.Conv2d(ch[-1], 2 * latent_channels, 3, padding=1)

    def forward(self, x):
        x = self.conv_in(x)
        for blk in self.down_blocks:
            x = blk(x)
        x = self.mid_block(x)
        return self.conv_out(F.silu(self.conv_norm_out(x)))


class EncoderOracle(nn.Module):
    """Encoder + quant_conv with diffusers' parameter names; forward(x) = encode(x).latent_dist.parameters (the moments)"""

    def __init__(self, block_out_channels=(128, 256, 512, 512), layers_per_block=2, in_channels=3, latent_channels=4,
                 groups=32):
        super().__init__()
        self.encoder = Encoder(block_out_channels, layers_per_block, in_channels, latent_channels, groups)
        self.quant_conv = nn.Conv2d(2 * latent_channels, 2 * latent_channels, 1)

    def forward(self, x):
        return self.quant_conv(self.encoder(x))


class DiagonalGaussianDistribution:
    def __init__(self, parameters: torch.Tensor, deterministic: bool = False):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        if deterministic:
            self.var = self.std = torch.zeros_like(self.mean)

    def sample(self, eps: torch.Tensor) -> torch.Tensor:
        return self.mean + self.std * eps

    def kl(self, other=None):
        if self.deterministic:
            return torch.Tensor([0.0])
        if other is None:
            return 0.5 * torch.sum(torch.pow(self.mean, 2) + self.var - 1.0 - self.logvar, dim=[1, 2, 3])
        return 0.5 * torch.sum(torch.pow(self.mean - other.mean, 2) / other.var + self.var / other.var - 1.0 - self.logvar
                               + other.logvar, dim=[1, 2, 3])

    def nll(self, sample, dims=(1, 2, 3)):
        if self.deterministic:
            return torch.Tensor([0.0])
        return 0.5 * torch.sum(np.log(2.0 * np.pi) + self.logvar + torch.pow(sample - self.mean, 2) / self.var, dim=list(dims))

    def mode(self):
        return self.mean
