"""Generator of train_image_tiny.npz: uint8 images run through the installed PIL exactly as the reference's training transform
runs them before the crop (pdm/utils/data_utils.py:61-82) -- ``Resize(R, BILINEAR)``: the shorter side to ``R``, the longer one to
``int(R * long / short)``, ``Image.resize((W1, H1), Image.BILINEAR)`` -- the fixture that pins the integer resampler of
tests/train_image_oracle.py and ``ops.pil_bilinear_table`` on every pixel, on machines without PIL too.

    python tests/golden/make_train_image_golden.py

Cases (H x W -> R), the smallest at which each code path can go wrong: 37x53 -> 16 (landscape, a non-integer downscale, a crop
along x), 53x37 -> 16 (portrait, a crop along y), 16x40 -> 16 (one axis untouched, a crop along x only), 16x16 -> 16 (no pass, no
draw), 9x11 -> 16 (an upscale: the filter's support stays 1, three taps), 64x48 -> 16 (scale 3: wide windows).  The images are
uniform noise with a quarter of the samples forced to 0 or 255.  Stored per case ``in_{name}`` (uint8 [H, W, 3]),
``resized_{name}`` (the FULL resized image, uint8 [H1, W1, 3]: every crop window is cut from it) and ``size_{name}``;
``pil_version`` names the PIL that wrote them.

Where torchvision imports, two more things are checked (nothing of them is stored): its ``Resize`` gives the same pixels, and
its ``RandomCrop`` + ``RandomHorizontalFlip`` / ``CenterCrop`` under ``torch.manual_seed`` pick the windows and flips that
``diffusion_pruning_amd.data.draw_crop_flip`` draws from the same seed."""
import os
import sys

import numpy as np

CASES = (("37x53", 37, 53, 16), ("53x37", 53, 37, 16), ("16x40", 16, 40, 16), ("16x16", 16, 16, 16), ("9x11", 9, 11, 16),
         ("64x48", 64, 48, 16))


def resize_pil(a, size):
    from PIL import Image
    h, w = a.shape[:2]
    h1, w1 = (size, int(size * w / h)) if h <= w else (int(size * h / w), size)
    return np.ascontiguousarray(np.asarray(Image.fromarray(a).resize((w1, h1), Image.BILINEAR)))


def check_torchvision(images, resized, size):
    """torchvision's own transforms against the stored pixels and against draw_crop_flip's order of draws"""
    import torch
    import torchvision.transforms as T
    from PIL import Image
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from diffusion_pruning_amd.data import draw_crop_flip
    rs = T.Resize(size, interpolation=T.InterpolationMode.BILINEAR)
    for a, r in zip(images, resized):
        assert np.array_equal(np.asarray(rs(Image.fromarray(a))), r)
    for center, flip in ((False, True), (False, False), (True, True), (True, False)):
        tf = T.Compose([rs, T.CenterCrop(size) if center else T.RandomCrop(size),
                        T.RandomHorizontalFlip() if flip else T.Lambda(lambda x: x)])
        for seed in range(8):
            torch.manual_seed(seed)
            got = [np.asarray(tf(Image.fromarray(a))) for a in images]              # one sample after the other, as a dataset does
            torch.manual_seed(seed)
            tops, lefts, flips = draw_crop_flip([r.shape[:2] for r in resized], size, center_crop=center, random_flip=flip)
            for g, r, t, l, f in zip(got, resized, tops, lefts, flips):
                win = r[t:t + size, l:l + size]
                assert np.array_equal(g, win[:, ::-1] if f else win), (center, flip, seed)


def main():
    import PIL
    rs = np.random.RandomState(20241)
    out = {"pil_version": np.array(PIL.__version__)}
    images, resized = [], []
    for name, h, w, size in CASES:
        a = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        pick = rs.rand(h, w, 3)
        a[pick < 0.125] = 0
        a[pick > 0.875] = 255
        r = resize_pil(a, size)
        images.append(a)
        resized.append(r)
        out[f"in_{name}"], out[f"resized_{name}"], out[f"size_{name}"] = a, r, np.array(size)
    try:
        import torchvision  # noqa: F401
    except ImportError:
        print("torchvision does not import: its transforms were not compared")
    else:
        check_torchvision(images, resized, CASES[0][3])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_image_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
