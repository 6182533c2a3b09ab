"""The training dataloader's transform (pdm/utils/data_utils.py:61-82) for a batch of decoded images, on the HIP path.

The reference transforms each PIL image on a CPU worker with torchvision::

    Resize(resolution, BILINEAR) -> RandomCrop(resolution) | CenterCrop(resolution) -> RandomHorizontalFlip | identity
    -> ToTensor -> Normalize(0.5, 0.5)

Here the random draws are made on the host (``draw_crop_flip``) and everything that touches pixels runs in two launches for the
whole ragged batch (``ops.train_images``): ``TrainTransform`` is the two together.  Decoding files, datasets and tokenisation
are out of scope: the input is a list of uint8 ``[H, W, 3]`` tensors.

With ``seeds=`` the draws come from the project's counter-based stream instead of a generator (``draw_crop_flip_seeded``,
``philox_words``): image i's crop and flip are a function of (seeds[i], draw) alone, the host half of the seeded training batch
(csrc/train_noise.h).

torchvision is not installed where this project is developed or run, so the ORDER of the draws below is a restatement of its
source, not a call into it: ``RandomCrop.get_params`` (transforms.py: ``i = torch.randint(0, h - th + 1, size=(1,)).item()``
then ``j = torch.randint(0, w - tw + 1, size=(1,)).item()``, and no draw at all when ``h == th and w == tw``),
``RandomHorizontalFlip.forward`` (``torch.rand(1) < self.p``) and ``CenterCrop`` for PIL images
(``int(round((h - th) / 2.0))``).  tests/golden/make_train_image_golden.py checks it against torchvision wherever that imports.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
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


_M0, _M1, _MASK, _S32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF), np.uint64(32)


def _philox_words_many(seeds: Sequence[int], draw: int, block: int = 0):
    """uint64 [4, len(seeds)] holding the four uint32 words of (seed, draw, block) for every seed (ints in [0, 2^64))"""
    key = np.array(seeds, dtype=np.uint64)
    k0, k1 = key & _MASK, key >> _S32
    one = np.ones_like(key)
    c = [one * np.uint64(block & 0xFFFFFFFF), one * np.uint64(block >> 32), one * np.uint64(draw & 0xFFFFFFFF),
         one * np.uint64(draw >> 32)]
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                                # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _MASK, (k1 + np.uint64(0xBB67AE85)) & _MASK
    return np.stack(c)


def philox_words(seed: int, draw: int, block: int = 0):
    """The four uint32 words (as Python ints) of block ``block`` of Philox draw ``draw`` of the sample whose seed is ``seed``: the
    project's stream (csrc/philox_normal.h: Philox4x32-10, key = the seed read as uint64, counter = (block, draw), 64 bits each),
    in numpy uint64 arithmetic -- the host half of what the device kernels draw."""
    for name, v in (("seed", seed), ("draw", draw), ("block", block)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"philox_words: {name} must be an int, got {v!r}")
    seed, draw, block = int(seed), int(draw), int(block)
    if not -(1 << 63) <= seed < (1 << 64) or not 0 <= draw < (1 << 64) or not 0 <= block < (1 << 64):
        raise ValueError(f"philox_words: seed in [-2^63, 2^64), draw and block in [0, 2^64), got {seed}, {draw}, {block}")
    return [int(v) for v in _philox_words_many([seed & ((1 << 64) - 1)], draw, block)[:, 0]]


TRAIN_SUBDRAWS = 8           # sub-draws a training call reserves per sample (csrc/train_noise.h): Philox draw 8 draw + k


def seed_list(seeds, n: int, what: str) -> List[int]:
    """the seeds of n samples as Python ints: an int (shared by all), n ints, or an int64 [n] tensor (read back to the host)"""
    if isinstance(seeds, torch.Tensor):
        if seeds.dtype != torch.int64 or seeds.dim() != 1:
            raise ValueError(f"{what}: a seeds tensor must be int64 [B], got {seeds.dtype} {tuple(seeds.shape)}")
        vals = [int(v) for v in seeds.tolist()]
    elif isinstance(seeds, int) and not isinstance(seeds, bool):
        vals = [seeds] * n
    else:
        vals = list(seeds)
    if len(vals) != n:
        raise ValueError(f"{what}: {len(vals)} seeds for {n} samples")
    for v in vals:
        if not isinstance(v, int) or isinstance(v, bool) or not -(1 << 63) <= v < (1 << 64):
            raise ValueError(f"{what}: a seed must be an int in [-2^63, 2^64), got {v!r}")
    return vals


def check_train_draw(draw, what: str) -> int:
    """a training call's draw, an epoch or a global step: 8 draw + 7 must stay a Philox draw below 2^62"""
    if not isinstance(draw, int) or isinstance(draw, bool) or draw < 0 or draw >= (1 << 59):
        raise ValueError(f"{what}: draw must be an int in [0, 2^59), got {draw!r}")
    return draw


def draw_crop_flip_seeded(resized_sizes: Sequence[Tuple[int, int]], R: int, seeds, draw: int, center_crop: bool = False,
                          random_flip: bool = True):
    """``draw_crop_flip`` from per-sample seeds instead of a generator: image i's crop and flip are a pure function of
    (seeds[i], draw), whatever its place in the batch.  They come from words x0, x1, x2 of block 0 of sub-draw 0 of the training
    draw map (Philox draw ``8 draw`` of the seed, csrc/train_noise.h)::

        top = (x0 (h - R + 1)) >> 32,  left = (x1 (w - R + 1)) >> 32,  flip = x2 >> 31

    The three words are always the same: ``center_crop`` ignores x0 and x1 (``int(round((extent - R) / 2.0))`` per axis),
    ``random_flip=False`` ignores x2, and no draw shifts another.  ``h == R and w == R`` gives (0, 0) by the formula itself."""
    if not isinstance(R, int) or R < 1:
        raise ValueError(f"draw_crop_flip_seeded: R must be a positive int, got {R!r}")
    check_train_draw(draw, "draw_crop_flip_seeded")
    sizes = [(int(h), int(w)) for h, w in resized_sizes]
    vals = seed_list(seeds, len(sizes), "draw_crop_flip_seeded")
    tops: List[int] = []
    lefts: List[int] = []
    flips: List[int] = []
    for i, (h, w) in enumerate(sizes):
        if h < R or w < R:
            raise ValueError(f"draw_crop_flip_seeded: image {i} is {h} x {w}, smaller than the crop {R}")
    words = _philox_words_many([v & ((1 << 64) - 1) for v in vals], TRAIN_SUBDRAWS * draw, 0) if vals else np.zeros((4, 0), np.uint64)
    for i, (h, w) in enumerate(sizes):
        x = [int(v) for v in words[:3, i]]
        if center_crop:
            top, left = int(round((h - R) / 2.0)), int(round((w - R) / 2.0))
        else:
            top, left = (x[0] * (h - R + 1)) >> 32, (x[1] * (w - R + 1)) >> 32
        tops.append(top)
        lefts.append(left)
        flips.append(x[2] >> 31 if random_flip else 0)
    return tops, lefts, flips


class TrainTransform:
    """``get_transforms``' train_transform for a batch: ``TrainTransform(resolution, center_crop, random_flip)(images,
    generator)`` -> pixel_values NCHW [B, 3, resolution, resolution] on the GPU, fp32 (bf16 with ``out_f32=False``).
    ``random_flip=False`` is the reference's validation_transform.  With ``seeds=`` (an int, B ints or an int64 [B] tensor) and
    ``draw=`` instead of a generator, the crop and flip of each image come from its own seed (draw_crop_flip_seeded)."""

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

    def draw(self, images, generator: Optional[torch.Generator] = None, *, seeds=None, draw: int = 0):
        if seeds is None:
            if draw != 0:
                raise ValueError("TrainTransform: draw needs seeds")
            return draw_crop_flip(self.resized_sizes(images), self.resolution, self.center_crop, self.random_flip, generator)
        if generator is not None:
            raise ValueError("TrainTransform: give seeds or a generator, not both")
        return draw_crop_flip_seeded(self.resized_sizes(images), self.resolution, seeds, draw, self.center_crop, self.random_flip)

    def __call__(self, images, generator: Optional[torch.Generator] = None, out: Optional[torch.Tensor] = None,
                 device=None, *, seeds=None, draw: int = 0) -> torch.Tensor:
        tops, lefts, flips = self.draw(images, generator, seeds=seeds, draw=draw)
        return ops.train_images(images, self.resolution, tops, lefts, flips, out_f32=self.out_f32, out=out, device=device)
