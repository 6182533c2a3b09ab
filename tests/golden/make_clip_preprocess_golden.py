"""Generator of clip_preprocess_tiny.npz: uint8 images run through the installed PIL exactly as OpenAI CLIP's ``preprocess`` runs
them before ToTensor -- ``Resize(size, BICUBIC)`` (the shorter side to ``size``, the longer one to ``int(size * long / short)``)
and ``CenterCrop(size)`` (offsets ``int(round((extent - size) / 2.0))``) -- the fixture that pins the integer resampler of
tests/clip_score_oracle.py on every pixel, on machines without PIL too.

    python tests/golden/make_clip_preprocess_golden.py

Cases (H x W -> size): 37x53 -> 32 and 53x37 -> 32 (odd sizes, a crop of either axis, an odd crop margin), 64x64 -> 48, 40x96 -> 32
(scale 1.25, an even margin), 24x24 -> 32 (an upscale: support 2), 32x32 -> 32 (no pass at all).  The images are uniform noise
with a quarter of the samples forced to 0 or 255, so that the filter's overshoot meets both clamps.  Stored per case ``in_{name}``
(uint8 [H, W, 3]), ``out_{name}`` (uint8 [size, size, 3]) and ``size_{name}``; ``pil_version`` names the PIL that wrote them.
Where torchvision imports, its transforms are run too and must agree."""
import os

import numpy as np

CASES = (("37x53", 37, 53, 32), ("53x37", 53, 37, 32), ("64x64", 64, 64, 48), ("40x96", 40, 96, 32), ("24x24", 24, 24, 32),
         ("32x32", 32, 32, 32))


def preprocess_pil(a, size):
    from PIL import Image
    h, w = a.shape[:2]
    h1, w1 = (size, int(size * w / h)) if h <= w else (int(size * h / w), size)
    r = np.asarray(Image.fromarray(a).resize((w1, h1), Image.BICUBIC))
    top, left = int(round((h1 - size) / 2.0)), int(round((w1 - size) / 2.0))
    return np.ascontiguousarray(r[top:top + size, left:left + size])


def main():
    import PIL
    rs = np.random.RandomState(20240)
    out = {"pil_version": np.array(PIL.__version__)}
    for name, h, w, size in CASES:
        a = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        pick = rs.rand(h, w, 3)
        a[pick < 0.125] = 0
        a[pick > 0.875] = 255
        ref = preprocess_pil(a, size)
        try:
            from PIL import Image
            import torchvision.transforms as T
            tv = T.Compose([T.Resize(size, interpolation=T.InterpolationMode.BICUBIC), T.CenterCrop(size)])(Image.fromarray(a))
            assert np.array_equal(np.asarray(tv), ref), name
        except ImportError:
            pass
        out[f"in_{name}"], out[f"out_{name}"], out[f"size_{name}"] = a, ref, np.array(size)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_preprocess_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
