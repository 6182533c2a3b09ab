"""The training dataloader's transform (pdm/utils/data_utils.py:61-82) for a batch of decoded images, on the HIP path.

The reference transforms each PIL image on a CPU worker with torchvision::

    Resize(resolution, BILINEAR) -> RandomCrop(resolution) | CenterCrop(resolution) -> RandomHorizontalFlip | identity
    -> ToTensor -> Normalize(0.5, 0.5)

Here the random draws are made on the host (``draw_crop_flip``) and everything that touches pixels runs in two launches for the
whole ragged batch (``ops.train_images``): ``TrainTransform`` is the two together.  Decoding files, datasets and tokenisation
are out of scope: the input is a list of uint8 ``[H, W, 3]`` tensors.

torchvision is not installed where this project is developed or run, so the ORDER of the draws below is a restatement of its
source, not a call into it: ``RandomCrop.get_params`` (transforms.py: ``i = torch.randint(0, h - th + 1, size=(1,)).item()``
then ``j = torch.randint(0, w - tw + 1, size=(1,)).item()``, and no draw at all when ``h == th and w == tw``),
``RandomHorizontalFlip.forward`` (``torch.rand(1) < self.p``) and ``CenterCrop`` for PIL images
(``int(round((h - th) / 2.0))``).  tests/golden/make_train_image_golden.py checks it against torchvision wherever that imports.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from . import ops


def draw_crop_flip(resized_sizes: Sequence[Tuple[int, int]], R: int, center_crop: bool = False, random_flip: bool = True,
                   generator: Optional[torch.Generator] = None):
    """(tops, lefts, flips), three lists of ints, for images already resized to ``resized_sizes`` [(h, w)]: per image, in the
    order a dataset applies its transform to one sample after the other,

      * the crop: ``center_crop`` -> ``int(round((extent - R) / 2.0))`` per axis and no draw; otherwise RandomCrop -- nothing
        drawn and (0, 0) when ``h == R and w == R``, else ``torch.randint(0, h - R + 1, (1,))`` then
        ``torch.randint(0, w - R + 1, (1,))``;
      * the flip: ``random_flip`` -> ``torch.rand(1) < 0.5``; otherwise no draw and no flip.

    ``generator`` is a CPU generator (None: torch's global one, as torchvision uses)."""
    if not isinstance(R, int) or R < 1:
        raise ValueError(f"draw_crop_flip: R must be a positive int, got {R!r}")
    tops: List[int] = []
    lefts: List[int] = []
    flips: List[int] = []
    for i, (h, w) in enumerate(resized_sizes):
        h, w = int(h), int(w)
        if h < R or w < R:
            raise ValueError(f"draw_crop_flip: image {i} is {h} x {w}, smaller than the crop {R}")
        if center_crop:
            top, left = int(round((h - R) / 2.0)), int(round((w - R) / 2.0))
        elif h == R and w == R:
            top, left = 0, 0
        else:
            top = int(torch.randint(0, h - R + 1, (1,), generator=generator).item())
            left = int(torch.randint(0, w - R + 1, (1,), generator=generator).item())
        flip = int(bool(torch.rand(1, generator=generator) < 0.5)) if random_flip else 0
        tops.append(top)
        lefts.append(left)
        flips.append(flip)
    return tops, lefts, flips


class TrainTransform:
    """``get_transforms``' train_transform for a batch: ``TrainTransform(resolution, center_crop, random_flip)(images,
    generator)`` -> pixel_values NCHW [B, 3, resolution, resolution] on the GPU, fp32 (bf16 with ``out_f32=False``).
    ``random_flip=False`` is the reference's validation_transform."""

    def __init__(self, resolution: int, center_crop: bool = False, random_flip: bool = True, out_f32: bool = True):
        if not isinstance(resolution, int) or resolution < 1:
            raise ValueError(f"TrainTransform: resolution must be a positive int, got {resolution!r}")
        self.resolution, self.center_crop, self.random_flip, self.out_f32 = resolution, bool(center_crop), bool(random_flip), out_f32

    def resized_sizes(self, images) -> List[Tuple[int, int]]:
        """Resize(resolution) of each image: the shorter side to resolution, the longer one to int(resolution * long / short)"""
        for i, im in enumerate(images):
            if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.shape[0] < 1 \
                    or im.shape[1] < 1:
                got = f"{im.dtype} {tuple(im.shape)}" if isinstance(im, torch.Tensor) else type(im).__name__
                raise ValueError(f"TrainTransform: image {i} must be a uint8 [H, W, 3] tensor, got {got}")
        return [ops.pil_resized_size(int(im.shape[0]), int(im.shape[1]), self.resolution)[:2] for im in images]

    def draw(self, images, generator: Optional[torch.Generator] = None):
        return draw_crop_flip(self.resized_sizes(images), self.resolution, self.center_crop, self.random_flip, generator)

    def __call__(self, images, generator: Optional[torch.Generator] = None, out: Optional[torch.Tensor] = None,
                 device=None) -> torch.Tensor:
        tops, lefts, flips = self.draw(images, generator)
        return ops.train_images(images, self.resolution, tops, lefts, flips, out_f32=self.out_f32, out=out, device=device)
