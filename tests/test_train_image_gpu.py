"""The training dataloader's transform on the GPU: aptp_train_images against the PIL fixture (tests/golden/train_image_tiny.npz)
through the oracle's float32 crop / flip / ToTensor / Normalize -- every comparison an equality, since the resampler is integer
arithmetic and ToTensor / Normalize are single IEEE fp32 operations -- the crop window's independence of the work skipped around
it, TrainTransform and batch_from_uint8 against batch_from_images fed with the oracle's pixel_values, and the C entry's refusal of
descriptors that leave their buffers."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import train_image_oracle as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "train_image_tiny.npz")
CASES = ("37x53", "53x37", "16x40", "16x16", "9x11", "64x48")
R = 16
# resized: 16x22, 22x16, 16x40, 16x16, 16x19, 21x16
SETTINGS = {
    "zero": ([0] * 6, [0] * 6, [0] * 6),
    "max_flipped": ([0, 6, 0, 0, 0, 5], [6, 0, 24, 0, 3, 0], [1] * 6),
    "mixed": ([0, 3, 0, 0, 0, 2], [2, 0, 17, 0, 1, 0], [1, 0, 1, 0, 0, 1]),
}


@pytest.fixture(scope="module")
def fixture():
    """(images, the fixture's PIL-resized images, {setting: the oracle's float32 pixel_values}), computed once"""
    z = np.load(GOLDEN)
    images = [z[f"in_{n}"] for n in CASES]
    resized = [z[f"resized_{n}"] for n in CASES]
    assert SETTINGS["max_flipped"][0] == [r.shape[0] - R for r in resized]          # the largest offsets there are
    assert SETTINGS["max_flipped"][1] == [r.shape[1] - R for r in resized]
    refs = {k: T.pixel_values(images, R, *v, resized=resized) for k, v in SETTINGS.items()}
    return [torch.from_numpy(a) for a in images], resized, refs


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_ragged_batch_is_pil_on_every_pixel(cuda, fixture, setting):
    from diffusion_pruning_amd import ops
    images, _, refs = fixture
    tops, lefts, flips = SETTINGS[setting]
    ref = refs[setting]
    out = ops.train_images(images, R, tops, lefts, flips, device=cuda)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (6, 3, R, R) and out.device.type == "cuda"
    for b, name in enumerate(CASES):
        assert torch.equal(out[b].cpu(), ref[b]), (setting, name, int((out[b].cpu() != ref[b]).sum()))
    assert float(ref.min()) == -1.0 and float(ref.max()) == 1.0
    # each case alone gives the rows it has in the ragged batch
    for b, name in enumerate(CASES):
        one = ops.train_images([images[b]], R, [tops[b]], [lefts[b]], [flips[b]], device=cuda)
        assert torch.equal(one[0], out[b]), (setting, name)
    # bf16 is the fp32 result rounded once
    bf = ops.train_images(images, R, tops, lefts, flips, out_f32=False, device=cuda)
    assert bf.dtype == torch.bfloat16 and torch.equal(bf, out.to(torch.bfloat16))
    # out=, images already on the GPU, and a mix of both
    buf = torch.full((6, 3, R, R), 7.0, device=cuda)
    assert ops.train_images(images, R, tops, lefts, flips, out=buf) is buf and torch.equal(buf, out)
    on_gpu = [im.to(cuda) for im in images]
    assert torch.equal(ops.train_images(on_gpu, R, tops, lefts, flips), out)
    assert torch.equal(ops.train_images(on_gpu[:3] + images[3:], R, tops, lefts, flips), out)
    bbuf = torch.zeros(6, 3, R, R, dtype=torch.bfloat16, device=cuda)
    ops.train_images(on_gpu, R, tops, lefts, flips, out_f32=False, out=bbuf)
    assert torch.equal(bbuf, bf)


def test_a_crop_window_does_not_depend_on_what_is_skipped_around_it(cuda, fixture):
    """two windows of the same resized images, shifted by 3 along the axis with room: where they overlap they hold the same
    values, although each run resampled other columns and other source rows"""
    from diffusion_pruning_amd import ops
    images, _, _ = fixture
    imgs = [images[0], images[1], images[2], images[5]]             # room along x, y, x, y
    a = ops.train_images(imgs, R, [0, 1, 0, 1], [1, 0, 5, 0], [0] * 4, device=cuda)
    b = ops.train_images(imgs, R, [0, 4, 0, 4], [4, 0, 8, 0], [0] * 4, device=cuda)
    torch.cuda.synchronize()
    for i in (0, 2):
        assert torch.equal(a[i, :, :, 3:], b[i, :, :, :R - 3]), i
        assert not torch.equal(a[i], b[i])
    for i in (1, 3):
        assert torch.equal(a[i, :, 3:, :], b[i, :, :R - 3, :]), i
        assert not torch.equal(a[i], b[i])
    # a flipped window shows the same pixels mirrored
    f = ops.train_images(imgs, R, [0, 1, 0, 1], [1, 0, 5, 0], [1] * 4, device=cuda)
    assert torch.equal(f, a.flip(-1))


def test_one_pass_only_and_more_than_one_workgroup(cuda, fixture):
    """resized sizes given by the caller: a horizontal pass without a vertical one and the reverse, which Resize(R) itself never
    asks for; and R = 40 on 90 x 131 and 131 x 90 images: 1600 outputs, seven workgroups per image, the last one partly empty"""
    from diffusion_pruning_amd import ops
    images, _, _ = fixture
    a = images[2].numpy()                                              # 16 x 40
    at = np.ascontiguousarray(a.transpose(1, 0, 2))
    sizes, tops, lefts, flips = [(16, 24), (24, 16)], [0, 5], [7, 0], [1, 0]
    out = ops.train_images([torch.from_numpy(a), torch.from_numpy(at)], R, tops, lefts, flips, resized_sizes=sizes, device=cuda)
    ref = T.pixel_values([a, at], R, tops, lefts, flips, resized=[T.resize(a, 16, 24), T.resize(at, 24, 16)])
    assert torch.equal(out.cpu(), ref)

    rs = np.random.RandomState(5)
    big = [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in ((90, 131), (131, 90), (40, 40))]
    tops, lefts, flips = [0, 11, 0], [13, 0, 0], [1, 0, 1]
    out = ops.train_images([torch.from_numpy(x) for x in big], 40, tops, lefts, flips, device=cuda)
    ref = T.pixel_values(big, 40, tops, lefts, flips, table=ops.pil_bilinear_table)
    assert tuple(out.shape) == (3, 3, 40, 40) and torch.equal(out.cpu(), ref)


# ---------------------------------------------------------------------------------------------------------------------
# TrainTransform and batch_from_uint8
# ---------------------------------------------------------------------------------------------------------------------
RES = 64
SHAPES = ((70, 100), (100, 70), (64, 64), (64, 90))


@pytest.fixture(scope="module")
def raw_batch():
    rs = np.random.RandomState(9)
    return [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in SHAPES]


def _oracle_pixels(raw, seed, center_crop=False, random_flip=True):
    """the oracle's pixel_values for the draws TrainTransform makes from ``seed``, restated by hand"""
    g = torch.Generator().manual_seed(seed)
    tops, lefts, flips = [], [], []
    for a in raw:
        h, w = T.resized_size(a.shape[0], a.shape[1], RES)
        if center_crop:
            tops.append(int(round((h - RES) / 2.0))); lefts.append(int(round((w - RES) / 2.0)))
        elif (h, w) == (RES, RES):
            tops.append(0); lefts.append(0)
        else:
            tops.append(int(torch.randint(0, h - RES + 1, (1,), generator=g)))
            lefts.append(int(torch.randint(0, w - RES + 1, (1,), generator=g)))
        flips.append(int(bool(torch.rand(1, generator=g) < 0.5)) if random_flip else 0)
    return T.pixel_values(raw, RES, tops, lefts, flips), (tops, lefts, flips)


def test_train_transform_equals_the_oracle(cuda, raw_batch):
    from diffusion_pruning_amd.data import TrainTransform
    imgs = [torch.from_numpy(a) for a in raw_batch]
    for seed in (0, 1):
        ref, draws = _oracle_pixels(raw_batch, seed)
        got = TrainTransform(RES)(imgs, generator=torch.Generator().manual_seed(seed), device=cuda)
        assert torch.equal(got.cpu(), ref), (seed, draws)
    ref, draws = _oracle_pixels(raw_batch, 0, center_crop=True, random_flip=False)
    assert draws[2] == [0] * 4 and draws[1][0] == int(round((91 - RES) / 2.0))
    val = TrainTransform(RES, center_crop=True, random_flip=False)(imgs, device=cuda)          # the validation form draws nothing
    assert torch.equal(val.cpu(), ref)
    ref, _ = _oracle_pixels(raw_batch, 3, random_flip=False)
    got = TrainTransform(RES, random_flip=False)(imgs, generator=torch.Generator().manual_seed(3), device=cuda)
    assert torch.equal(got.cpu(), ref)


def test_batch_from_uint8_equals_batch_from_images_on_oracle_pixels(cuda, raw_batch):
    from diffusion_pruning_amd.text_encoder import CLIPTextConfig, CLIPTextModel
    from diffusion_pruning_amd.train_step import batch_from_images, batch_from_uint8
    from diffusion_pruning_amd.vae import AutoencoderKL
    vae = AutoencoderKL(with_encoder=True).init_synthetic(seed=0).to(cuda)
    imgs = [torch.from_numpy(a) for a in raw_batch]
    g = torch.Generator().manual_seed(2)
    ehs = torch.randn(4, 77, 64, generator=g).to(cuda)
    emb = (0.05 * torch.randn(4, 32, generator=g)).to(cuda)
    px, _ = _oracle_pixels(raw_batch, 21)
    want = batch_from_images(vae, px.to(cuda), ehs, emb, generator=torch.Generator().manual_seed(5))
    got = batch_from_uint8(vae, imgs, resolution=RES, transform_generator=torch.Generator().manual_seed(21),
                           encoder_hidden_states=ehs, mpnet_embeddings=emb, generator=torch.Generator().manual_seed(5))
    torch.cuda.synchronize()
    assert set(got) == set(want) == {"noisy_latents", "target", "encoder_hidden_states", "mpnet_embeddings", "timesteps"}
    assert tuple(got["noisy_latents"].shape) == (4, 4, RES // 8, RES // 8)
    for k in want:
        assert torch.equal(got[k], want[k]), k

    te = CLIPTextModel(CLIPTextConfig(vocab_size=1000, hidden_size=64, intermediate_size=256, num_hidden_layers=2,
                                      num_attention_heads=1)).init_synthetic(1).to(cuda)
    ids = torch.randint(3, 1000, (4, 77), generator=g).to(cuda)
    states = te(ids)[0]
    got = batch_from_uint8(vae, imgs, resolution=RES, center_crop=True, random_flip=False, prompt_ids=ids, text_encoder=te,
                           mpnet_embeddings=emb, generator=torch.Generator().manual_seed(5))
    px, _ = _oracle_pixels(raw_batch, 0, center_crop=True, random_flip=False)
    want = batch_from_images(vae, px.to(cuda), states, emb, generator=torch.Generator().manual_seed(5))
    torch.cuda.synchronize()
    assert torch.equal(got["encoder_hidden_states"], states) and tuple(states.shape) == (4, 77, 64)
    for k in want:
        assert torch.equal(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# the C entry on real buffers: the host-side check only
# ---------------------------------------------------------------------------------------------------------------------
def test_c_entry_refuses_descriptors_that_leave_their_buffers(cuda, fixture):
    """every call below is refused by the host-side check: -1, a message, and an output buffer nobody wrote to"""
    from diffusion_pruning_amd import _lib, ops
    lib = _lib.load()
    images, _, _ = fixture
    imgs = images[:2]
    shapes = [(int(im.shape[0]), int(im.shape[1])) for im in imgs]
    sizes = [ops.pil_resized_size(h, w, R)[:2] for h, w in shapes]
    flat = torch.cat([im.reshape(-1) for im in imgs]).to(cuda)
    out = torch.full((2, 3, R, R), 7.0, device=cuda)

    def call(mutate):
        desc, tables, scratch_len = ops._train_images_plan(shapes, sizes, R, [0, 0], [0, 0], [0, 0], cuda)
        scratch = torch.empty(scratch_len, dtype=torch.uint8, device=cuda)
        p = _lib.TrainImagesParams()
        p.images, p.images_bytes = flat.data_ptr(), flat.numel()
        p.tables, p.tables_count = tables.data_ptr(), tables.numel()
        p.scratch, p.scratch_bytes = scratch.data_ptr(), scratch_len
        p.out, p.B, p.R, p.out_f32 = out.data_ptr(), 2, R, 1
        mutate(p, desc)
        desc_dev = torch.frombuffer(desc, dtype=torch.uint8).to(cuda)
        p.desc, p.desc_dev = ctypes.addressof(desc), desc_dev.data_ptr()
        rc = lib.aptp_train_images(ctypes.byref(p), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, lib.aptp_last_error()

    for msg, mutate in ((b"leave the image buffer", lambda p, d: setattr(d[1], "src_off", d[1].src_off + 1)),
                        (b"crop window", lambda p, d: setattr(d[1], "top", 7)),                  # 53x37 -> 22x16: top + R > H1
                        (b"crop window", lambda p, d: setattr(d[0], "left", 7)),
                        (b"vertical table", lambda p, d: setattr(d[0], "ytab_off", p.tables_count - 1)),
                        (b"leave the scratch buffer", lambda p, d: setattr(d[1], "scratch_off", d[1].scratch_off + 1)),
                        (b"bad extents", lambda p, d: setattr(p, "R", 0))):
        rc, err = call(mutate)
        assert rc == -1 and msg in err, (rc, err)
        assert bool((out == 7.0).all())
    rc, _ = call(lambda p, d: None)                                  # the unmodified descriptors run
    assert rc == 0 and not bool((out == 7.0).any())
    assert torch.equal(out, ops.train_images(imgs, R, [0, 0], [0, 0], [0, 0], device=cuda))
