"""Host tests of the training dataloader's transform: the oracle (tests/train_image_oracle.py) and ops.pil_bilinear_table against
the PIL fixture, the unchanged bicubic tables, the order of draw_crop_flip's draws, the arguments ops.train_images and
batch_from_uint8 refuse before touching a device, and the C ABI of aptp_train_images."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from diffusion_pruning_amd import _lib, data, ops
from diffusion_pruning_amd.train_step import batch_from_uint8
from tests import clip_score_oracle as C
from tests import train_image_oracle as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "train_image_tiny.npz")
CLIP_GOLDEN = os.path.join(HERE, "golden", "clip_preprocess_tiny.npz")
CASES = ("37x53", "53x37", "16x40", "16x16", "9x11", "64x48")
R = 16
RESIZED = {"37x53": (16, 22), "53x37": (22, 16), "16x40": (16, 40), "16x16": (16, 16), "9x11": (16, 19), "64x48": (21, 16)}


# ---------------------------------------------------------------------------------------------------------------------
# the resampler and its tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [ops.pil_bilinear_table, T.bilinear_table], ids=["ops.pil_bilinear_table", "oracle.bilinear_table"])
def test_integer_resampler_reproduces_pil_bilinear_on_every_pixel(table):
    z = np.load(GOLDEN)
    assert sorted(k[3:] for k in z.files if k.startswith("in_")) == sorted(CASES)
    for name in CASES:
        img, ref = z[f"in_{name}"], z[f"resized_{name}"]
        assert int(z[f"size_{name}"]) == R and img.shape == tuple(int(v) for v in name.split("x")) + (3,)
        h1, w1 = T.resized_size(img.shape[0], img.shape[1], R)
        assert (h1, w1) == RESIZED[name] == ops.pil_resized_size(img.shape[0], img.shape[1], R)[:2] == ref.shape[:2]
        got = T.resize(img, h1, w1, table=table)
        assert got.dtype == np.uint8 and got.shape == ref.shape
        assert int((got != ref).sum()) == 0, name
    assert np.array_equal(z["in_16x16"], z["resized_16x16"]) and np.array_equal(z["in_16x40"], z["resized_16x40"])   # untouched
    assert z["resized_9x11"].min() == 0 and z["resized_9x11"].max() == 255


@pytest.mark.parametrize("n_in,n_out", [(53, 22), (37, 16), (11, 19), (9, 16), (64, 21), (48, 16), (500, 341), (375, 256), (1, 7), (7, 1)])
def test_bilinear_table_builder_equals_the_oracle(n_in, n_out):
    b, w = ops.pil_bilinear_table(n_in, n_out)
    ob, ow = T.bilinear_table(n_in, n_out)
    assert b.dtype == np.int32 and w.dtype == np.int32
    assert np.array_equal(b, ob) and np.array_equal(w, ow)
    ksize = 2 * int(np.ceil(max(n_in / n_out, 1.0))) + 1                   # support 1 * max(scale, 1)
    assert w.shape == (n_out, ksize) and b[:, 1].max() <= ksize and b[:, 1].min() >= 1
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all()
    assert (w >= 0).all() and np.abs(w.sum(1) - (1 << 22)).max() <= ksize   # the triangle has no negative lobe
    for i in range(n_out):
        assert not w[i, b[i, 1]:].any()


def test_bilinear_window_widths():
    assert ops.pil_bilinear_table(9, 16)[1].shape[1] == 3                    # an upscale: support stays 1
    assert ops.pil_bilinear_table(64, 21)[1].shape[1] == 9                   # scale 3.05: ceil -> 4, 2 * 4 + 1
    assert ops.pil_bilinear_table(500, 341)[1].shape[1] == 5
    with pytest.raises(ValueError):
        ops.pil_bilinear_table(0, 4)


@pytest.mark.parametrize("n_in,n_out", [(256, 224), (512, 224), (24, 32), (53, 45), (96, 76), (1, 7), (7, 1)])
def test_bicubic_tables_are_unchanged(n_in, n_out):
    b, w = ops.pil_bicubic_table(n_in, n_out)
    ob, ow = C.coeff_table(n_in, n_out)
    assert np.array_equal(b, ob) and np.array_equal(w, ow)


def test_bicubic_tables_still_reproduce_the_clip_fixture(monkeypatch):
    """the existing CLIP fixture through the existing oracle, its tables replaced by ops.pil_bicubic_table's"""
    monkeypatch.setattr(C, "coeff_table", ops.pil_bicubic_table)
    z = np.load(CLIP_GOLDEN)
    names = sorted(k[3:] for k in z.files if k.startswith("in_"))
    assert len(names) == 6
    for name in names:
        got = C.clip_preprocess_u8(z[f"in_{name}"], int(z[f"size_{name}"]))
        assert int((got != z[f"out_{name}"]).sum()) == 0, name


def test_oracle_values_are_single_fp32_operations():
    r = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, 2)
    v = T.crop_flip_normalize(r, 1, 0, 200, 0)
    assert v.dtype == torch.float32 and tuple(v.shape) == (3, 1, 1)
    want = (np.float32(200) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)
    assert float(v[0, 0, 0]) == float(want)
    full = T.crop_flip_normalize(np.arange(48, dtype=np.uint8).reshape(4, 4, 3), 2, 1, 2, 1)
    want = (np.array([21, 22, 23], np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)          # row 1, column 3
    assert np.array_equal(full[:, 0, 0].numpy(), want) and tuple(full.shape) == (3, 2, 2)


# ---------------------------------------------------------------------------------------------------------------------
# draw_crop_flip
# ---------------------------------------------------------------------------------------------------------------------
SIZES = [RESIZED[n] for n in CASES]


def test_draws_are_made_in_torchvisions_order():
    g = torch.Generator().manual_seed(7)
    tops, lefts, flips = data.draw_crop_flip(SIZES, R, generator=g)
    h = torch.Generator().manual_seed(7)
    for i, (hh, ww) in enumerate(SIZES):
        if (hh, ww) == (R, R):
            top, left = 0, 0                                                 # RandomCrop.get_params returns before drawing
        else:
            top = int(torch.randint(0, hh - R + 1, (1,), generator=h))
            left = int(torch.randint(0, ww - R + 1, (1,), generator=h))
        flip = int(bool(torch.rand(1, generator=h) < 0.5))
        assert (tops[i], lefts[i], flips[i]) == (top, left, flip), i
    assert torch.equal(g.get_state(), h.get_state())                         # not one draw more or less
    assert all(isinstance(v, int) for v in tops + lefts + flips)


def test_no_draw_for_an_image_that_needs_none():
    g = torch.Generator().manual_seed(3)
    before = g.get_state().clone()
    assert data.draw_crop_flip([(R, R)], R, random_flip=False, generator=g) == ([0], [0], [0])
    assert torch.equal(g.get_state(), before)
    assert data.draw_crop_flip(SIZES, R, center_crop=True, random_flip=False, generator=g)[2] == [0] * len(SIZES)
    assert torch.equal(g.get_state(), before)                                # centre crop without flip: nothing random
    tops, lefts, flips = data.draw_crop_flip([(R, R)], R, generator=g)       # only the flip's draw
    h = torch.Generator().manual_seed(3)
    assert (tops, lefts) == ([0], [0]) and flips == [int(bool(torch.rand(1, generator=h) < 0.5))]
    assert torch.equal(g.get_state(), h.get_state())


def test_centre_offsets_are_python_rounds():
    sizes = [(16, 22), (22, 16), (16, 19), (21, 16), (16, 17), (16, 21), (16, 16), (19, 23)]
    tops, lefts, flips = data.draw_crop_flip(sizes, R, center_crop=True, random_flip=False)
    assert tops == [int(round((h - R) / 2.0)) for h, _ in sizes] == [0, 3, 0, 2, 0, 0, 0, 2]
    assert lefts == [int(round((w - R) / 2.0)) for _, w in sizes] == [3, 0, 2, 0, 0, 2, 0, 4]       # halves go to the even side
    assert flips == [0] * len(sizes)


def test_offsets_stay_inside_the_resized_image():
    g = torch.Generator().manual_seed(11)
    seen_top, seen_left, seen_flip = set(), set(), set()
    for _ in range(200):
        tops, lefts, flips = data.draw_crop_flip(SIZES, R, generator=g)
        for (h, w), t, l, f in zip(SIZES, tops, lefts, flips):
            assert 0 <= t <= h - R and 0 <= l <= w - R and f in (0, 1)
        seen_top.add(tops[1]); seen_left.add(lefts[0]); seen_flip.add(flips[0])
    assert seen_top == set(range(7)) and seen_left == set(range(7)) and seen_flip == {0, 1}      # both ends are reached
    with pytest.raises(ValueError, match="smaller than the crop"):
        data.draw_crop_flip([(15, 20)], R)
    with pytest.raises(ValueError):
        data.draw_crop_flip([(16, 16)], 0)


# ---------------------------------------------------------------------------------------------------------------------
# refused arguments: none of these reaches a device
# ---------------------------------------------------------------------------------------------------------------------
def _img(h, w, c=3, dtype=torch.uint8):
    return torch.zeros(h, w, c, dtype=dtype)


def test_train_images_refuses_bad_arguments():
    ok = [_img(20, 30), _img(16, 16)]
    with pytest.raises(ValueError, match="uint8"):
        ops.train_images([_img(20, 30, dtype=torch.float32)], R, [0], [0], [0])
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        ops.train_images([_img(20, 30, c=4)], R, [0], [0], [0])
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        ops.train_images([torch.zeros(1, 20, 30, 3, dtype=torch.uint8)], R, [0], [0], [0])
    with pytest.raises(ValueError, match="non-empty"):
        ops.train_images([], R, [], [], [])
    with pytest.raises(ValueError, match="non-empty"):
        ops.train_images(torch.zeros(2, 16, 16, 3, dtype=torch.uint8), R, [0, 0], [0, 0], [0, 0])
    with pytest.raises(ValueError, match="entries"):
        ops.train_images(ok, R, [0], [0, 0], [0, 0])
    with pytest.raises(ValueError, match="positive"):
        ops.train_images(ok, 0, [0, 0], [0, 0], [0, 0])
    with pytest.raises(ValueError, match="smaller than the crop"):          # R larger than a resized side
        ops.train_images(ok, R, [0, 0], [0, 0], [0, 0], resized_sizes=[(16, 24), (16, 15)])
    with pytest.raises(ValueError, match="crop window"):                    # 20x30 -> 16x24: left at most 8
        ops.train_images(ok, R, [0, 0], [9, 0], [0, 0])
    with pytest.raises(ValueError, match="crop window"):
        ops.train_images(ok, R, [1, 0], [0, 0], [0, 0])
    with pytest.raises(ValueError, match="crop window"):
        ops.train_images(ok, R, [0, 0], [-1, 0], [0, 0])
    with pytest.raises(ValueError, match="flip"):
        ops.train_images(ok, R, [0, 0], [0, 0], [2, 0])
    with pytest.raises(ValueError, match="out must be"):
        ops.train_images(ok, R, [0, 0], [0, 0], [0, 0], out=torch.zeros(2, 3, R, R))
    with pytest.raises(ValueError, match="HIP kernels only"):
        ops.train_images(ok, R, [0, 0], [0, 0], [0, 0], device="cpu")


class _Spy:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a, **k):
        self.calls += 1
        raise AssertionError("must not be reached")

    encode_latents = __call__


def test_batch_from_uint8_refuses_bad_arguments():
    imgs = [_img(20, 30), _img(16, 16)]
    ids = torch.zeros(2, 77, dtype=torch.int64)
    ehs = torch.zeros(2, 77, 32)
    emb = torch.zeros(2, 32)
    vae, te = _Spy(), _Spy()
    with pytest.raises(ValueError, match="exactly one of prompt_ids and encoder_hidden_states"):
        batch_from_uint8(vae, imgs, resolution=R, mpnet_embeddings=emb)
    with pytest.raises(ValueError, match="exactly one of prompt_ids and encoder_hidden_states"):
        batch_from_uint8(vae, imgs, resolution=R, prompt_ids=ids, text_encoder=te, encoder_hidden_states=ehs, mpnet_embeddings=emb)
    with pytest.raises(ValueError, match="text_encoder"):
        batch_from_uint8(vae, imgs, resolution=R, prompt_ids=ids, mpnet_embeddings=emb)
    with pytest.raises(ValueError, match="uint8"):
        batch_from_uint8(vae, [_img(20, 30, dtype=torch.float32)], resolution=R, prompt_ids=ids, text_encoder=te, mpnet_embeddings=emb)
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        batch_from_uint8(vae, [_img(20, 30, c=4)], resolution=R, encoder_hidden_states=ehs, mpnet_embeddings=emb)
    with pytest.raises(ValueError, match="positive"):
        batch_from_uint8(vae, imgs, resolution=0, encoder_hidden_states=ehs, mpnet_embeddings=emb)
    assert vae.calls == 0 and te.calls == 0
    g = torch.Generator().manual_seed(0)
    before = g.get_state().clone()
    with pytest.raises(ValueError):
        data.TrainTransform(R)([_img(20, 30, c=4)], generator=g)
    assert torch.equal(g.get_state(), before)                                # refused before a draw was made


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_train_images_export_is_declared_and_bound():
    import re
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aptp_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(aptp_[a-z_0-9]+)\s*\(", src))
    bound = {n for n, _, _ in _lib.EXPORTS}
    assert "aptp_train_images" in declared and "aptp_train_images" in bound and declared == bound
    assert _lib.load().aptp_train_images is not None
    mk = open(os.path.join(ROOT, "diffusion_pruning_amd", "csrc", "Makefile")).read()
    assert "train_image_ops.hip" in mk


def test_train_images_ctypes_layouts_match_the_c_header(tmp_path):
    structs = {"AptpTrainImageDesc": _lib.TrainImageDesc, "AptpTrainImagesParams": _lib.TrainImagesParams}
    body = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "aptp_hip.h")}"', "int main(void){"]
    want = []
    for cname, cls in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(ctypes.sizeof(cls))
        for fname, _ in cls._fields_:
            body.append(f'printf("%zu\\n", offsetof({cname}, {fname}));')
            want.append(getattr(cls, fname).offset)
    body.append('printf("%d\\n", (int)APTP_TRAIN_NO_TABLE);')
    want.append(_lib.TRAIN_NO_TABLE)
    body.append("return 0;}")
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(body))
    subprocess.run(["cc", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert ctypes.sizeof(_lib.TrainImageDesc) == 80


def good_params(n=2):
    """a descriptor table the entry would accept, over made-up device addresses: image 0 is 37 x 53 -> 16 x 22 (both passes), image
    1 is 16 x 16 (none).  Returns (params, desc array); the checks refuse each mutation before anything is dereferenced on a device"""
    desc = (_lib.TrainImageDesc * n)()
    d = desc[0]
    d.src_off, d.H, d.W, d.H1, d.W1, d.top, d.left, d.flip = 0, 37, 53, 16, 22, 0, 6, 1
    d.xtab_off, d.xk, d.ytab_off, d.yk = 0, 7, 22 * 9, 7
    d.row0, d.nrows, d.scratch_off = 0, 37, 0
    if n > 1:
        e = desc[1]
        e.src_off, e.H, e.W, e.H1, e.W1 = 37 * 53 * 3, 16, 16, 16, 16
        e.xtab_off = e.ytab_off = _lib.TRAIN_NO_TABLE
    p = _lib.TrainImagesParams()
    p.images, p.images_bytes = 1 << 20, 37 * 53 * 3 + 16 * 16 * 3
    p.desc, p.desc_dev = ctypes.addressof(desc), 2 << 20
    p.tables, p.tables_count = 3 << 20, 22 * 9 + 16 * 9
    p.scratch, p.scratch_bytes = 4 << 20, 37 * 16 * 3
    p.out, p.B, p.R, p.out_f32 = 5 << 20, n, 16, 1
    return p, desc


BAD = [
    ("null pointer", lambda p, d: setattr(p, "out", None)),
    ("null pointer", lambda p, d: setattr(p, "desc_dev", None)),
    ("null pointer", lambda p, d: setattr(p, "images", None)),
    ("bad extents", lambda p, d: setattr(p, "R", 0)),
    ("bad extents", lambda p, d: setattr(p, "B", 0)),
    ("alignment", lambda p, d: setattr(p, "out", (5 << 20) + 2)),
    ("leave the image buffer", lambda p, d: setattr(d[1], "src_off", 37 * 53 * 3 + 1)),
    ("leave the image buffer", lambda p, d: setattr(d[0], "src_off", -3)),
    ("leave the image buffer", lambda p, d: setattr(p, "images_bytes", 37 * 53 * 3 + 16 * 16 * 3 - 1)),
    ("crop window", lambda p, d: setattr(d[0], "top", 1)),                       # top + R > H1
    ("crop window", lambda p, d: setattr(d[0], "left", 7)),                      # left + R > W1
    ("crop window", lambda p, d: setattr(d[0], "left", -1)),
    ("crop window", lambda p, d: setattr(d[1], "top", 1)),
    ("flip is 2", lambda p, d: setattr(d[0], "flip", 2)),
    ("exactly when its size changes", lambda p, d: setattr(d[0], "xtab_off", _lib.TRAIN_NO_TABLE)),
    ("exactly when its size changes", lambda p, d: setattr(d[1], "ytab_off", 0)),
    ("horizontal table", lambda p, d: setattr(d[0], "xtab_off", 16 * 9 + 1)),
    ("horizontal table", lambda p, d: setattr(d[0], "xk", 0)),
    ("vertical table", lambda p, d: setattr(d[0], "ytab_off", 22 * 9 + 1)),
    ("vertical table", lambda p, d: setattr(d[0], "yk", 8)),
    ("vertical table", lambda p, d: setattr(p, "tables_count", 22 * 9 + 16 * 9 - 1)),
    ("tables is needed", lambda p, d: setattr(p, "tables", None)),
    ("leave the image of 37 rows", lambda p, d: setattr(d[0], "nrows", 38)),
    ("leave the image of 37 rows", lambda p, d: setattr(d[0], "row0", -1)),
    ("scratch is needed", lambda p, d: setattr(p, "scratch", None)),
    ("leave the scratch buffer", lambda p, d: setattr(d[0], "scratch_off", 1)),
    ("leave the scratch buffer", lambda p, d: setattr(p, "scratch_bytes", 37 * 16 * 3 - 1)),
    ("extents", lambda p, d: setattr(d[0], "H", 0)),
    ("extents", lambda p, d: setattr(d[0], "W1", 1 << 20)),
]


@pytest.mark.parametrize("i", range(len(BAD)), ids=[f"{i}-{m[0].replace(' ', '_')}" for i, m in enumerate(BAD)])
def test_c_entry_refuses_bad_descriptors_before_launching(i):
    """made-up device addresses: a launch would fault, so a return of -1 with the message shows that nothing was launched"""
    lib = _lib.load()
    msg, mutate = BAD[i]
    p, desc = good_params()
    mutate(p, desc)
    assert lib.aptp_train_images(ctypes.byref(p), None) == -1
    assert msg.encode() in lib.aptp_last_error(), lib.aptp_last_error()


def test_c_entry_refuses_a_window_that_misses_the_computed_rows():
    lib = _lib.load()
    p, desc = good_params(1)
    d = desc[0]                                                                  # 16 x 40 -> 16 x 24: a horizontal pass only
    d.H, d.W, d.H1, d.W1, d.top, d.left, d.ytab_off, d.xk = 16, 40, 16, 24, 0, 8, _lib.TRAIN_NO_TABLE, 5
    d.row0, d.nrows = 1, 15
    assert lib.aptp_train_images(ctypes.byref(p), None) == -1 and b"do not hold the crop window" in lib.aptp_last_error()
    assert lib.aptp_train_images(None, None) == -1 and b"null pointer" in lib.aptp_last_error()
