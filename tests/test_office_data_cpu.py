"""CPU-side checks of the Office input pipeline (include/alignq.h: alignq_data_crop_batch; alignq_amd/data.py: the office presets,
read_image_folder, pair_plan / PairLoader; OfficeTrainStep.set_producer): the ABI boundary and every argument rule, the ImageNet
table against torch's ToTensor / Normalize arithmetic, the centre offset, the statistics of the span-way draws (on
tests/office_data_oracle.py, the NumPy statement of the header), the iteration arithmetic of the two pairing modes and the
ImageFolder-ordered reader.

The bounds of the distribution test are derived, not tuned: of N independent draws a cell of probability p holds
N p +- sqrt(N p (1 - p)); an axis has 33 cells of p = 1/33 (N = 2 817: 85.4 +- 9.1, 5 sigma: 45.5; N = 50 000: 1 515.2 +- 38.3,
5 sigma: 191.7), the flip p = 1/2.  The sample correlation of two independent axes is ~ N(0, 1/N): |rho| sqrt(N) < 5."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import office_data_oracle as OO


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_symbol_declared_mirrored_exported_and_argument_validation():
    """alignq_data_crop_batch: in the header, in the ctypes table, in the library; every refusal of the header comes back before
    anything touches a device (this runs without one) and nothing is written."""
    from alignq_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "alignq.h")).read(), flags=re.S)
    lib = L.load()
    name = "alignq_data_crop_batch"
    assert re.search(r"\b%s\s*\(" % name, header) and name in L.SIGNATURES and hasattr(lib, name)
    assert len(L.SIGNATURES[name][1]) == 20
    assert lib.alignq_abi_version() == 23
    # host buffers stand in for device pointers: every call below must be refused before a launch
    side, crop = 12, 8
    img = (ctypes.c_uint8 * (side * side * 3))()
    lab, perm, y = (ctypes.c_int64 * 1)(), (ctypes.c_int64 * 1)(), (ctypes.c_int64 * 1)()
    cur = (ctypes.c_int32 * 4)()
    buf = (ctypes.c_float * (768 + 3 * crop * crop + 8))()
    lut = (ctypes.addressof(buf) + 15) & ~15
    x = lut + 768 * 4
    a = lambda t: ctypes.addressof(t)                                         # noqa: E731
    good = dict(images=a(img), labels=a(lab), perm=a(perm), cursor=a(cur), advance=1, lut=lut, N=1, side=side, crop=crop, span=5, off0=0,
                B=1, rank=0, world=1, seed=0, flip=1, x_out=x, nhwc=0, y_out=a(y), stream=None)
    order = list(good)

    def call(**kw):
        args = dict(good, **kw)
        return lib.alignq_data_crop_batch(*[args[k] for k in order])

    bad = [dict(images=None), dict(labels=None), dict(cursor=None), dict(lut=None), dict(x_out=None), dict(y_out=None),
           dict(x_out=x + 4), dict(lut=lut + 8), dict(labels=a(lab) + 4), dict(perm=a(perm) + 4), dict(y_out=a(y) + 4), dict(cursor=a(cur) + 2),
           dict(crop=6, span=1), dict(crop=10, span=1), dict(crop=0, span=1), dict(crop=-4, span=1), dict(crop=16, span=1),
           dict(side=1028, crop=1028, span=1), dict(side=2048, span=1),
           dict(span=0), dict(span=-1), dict(span=256, side=1024), dict(span=6), dict(off0=-1), dict(off0=1), dict(off0=5, span=1),
           dict(off0=2 ** 31 - 1, span=2), dict(span=1, off0=4, crop=12),
           dict(flip=2), dict(flip=-1), dict(nhwc=2), dict(nhwc=-1),
           dict(B=0), dict(B=-3), dict(rank=1), dict(rank=2, world=2), dict(rank=-1), dict(world=0), dict(N=0), dict(advance=-1)]
    for kw in bad:
        assert call(**kw) == L.EINVAL, kw
    assert call(B=70000) == L.EUNSUPPORTED and call(N=(1 << 30) + 1) == L.EUNSUPPORTED
    assert call(advance=(1 << 30) + 1) == L.EUNSUPPORTED
    assert list(cur) == [0, 0, 0, 0] and not any(buf) and list(y) == [0]


def test_imagenet_table_is_totensor_normalize_bit_for_bit():
    from alignq_amd import data as D
    for preset in ("office_train", "office_test"):
        p = D.PRESETS[preset]
        assert p["mean"] == (0.485, 0.456, 0.406) and p["std"] == (0.229, 0.224, 0.225) and p["crop"] == 224
        lut = D.normalise_table(p["mean"], p["std"])
        assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256) and lut.is_contiguous()
        # torchvision's own sequence on a whole image holding every byte: ToTensor = byte -> float32, div(255); Normalize =
        # sub_(mean[:, None, None]).div_(std[:, None, None]) with float32 mean / std tensors
        img = torch.arange(256, dtype=torch.uint8).view(1, 16, 16).expand(3, 16, 16)
        t = img.to(torch.float32).div(255)
        t = t.clone().sub_(torch.as_tensor(p["mean"], dtype=torch.float32).view(-1, 1, 1)).div_(
            torch.as_tensor(p["std"], dtype=torch.float32).view(-1, 1, 1))
        assert np.array_equal(bits(lut.numpy()), bits(t.reshape(3, 256).numpy()))          # all 768 entries
        assert np.array_equal(bits(OO.normalise_table(p["mean"], p["std"])), bits(lut.numpy()))
    tr, te = D.PRESETS["office_train"], D.PRESETS["office_test"]
    assert tr["flip"] and tr["shuffle"] and tr["window"] == "random"
    assert not te["flip"] and not te["shuffle"] and te["window"] == "center"


@pytest.mark.parametrize("diff", [0, 5, 7, 32])
def test_centre_offset_is_center_crops(diff):
    from alignq_amd import data as D
    crop = 224
    assert D.center_offset(crop + diff, crop) == int(round(diff / 2.0)) == {0: 0, 5: 2, 7: 4, 32: 16}[diff]
    assert OO.window(crop + diff, crop, False) == (1, D.center_offset(crop + diff, crop))
    assert OO.window(crop + diff, crop, True) == (diff + 1, 0)


@pytest.mark.parametrize("N", [2817, 50_000])
@pytest.mark.parametrize("epoch", [0, 1, 2])
@pytest.mark.parametrize("seed", [0, 1, 7, 12345])
def test_span33_draws_are_uniform_and_uncorrelated_within_five_sigma(seed, epoch, N):
    span = 33
    dy, dx, f = OO.draws(seed, epoch, np.arange(N), span)
    assert dy.min() >= 0 and dy.max() <= span - 1 and dx.min() >= 0 and dx.max() <= span - 1 and set(np.unique(f)) == {0, 1}
    p = 1.0 / span
    bound = 5.0 * math.sqrt(N * p * (1 - p))
    worst = 0.0
    for axis in (dy, dx):
        cells = np.bincount(axis, minlength=span)
        assert len(cells) == span
        worst = max(worst, np.abs(cells - N * p).max() / (bound / 5.0))
        assert np.abs(cells - N * p).max() <= bound
    flip_bound = 5.0 * math.sqrt(N * 0.25)
    worst = max(worst, abs(int(f.sum()) - N / 2) / (flip_bound / 5.0))
    assert abs(int(f.sum()) - N / 2) <= flip_bound
    rho = float(np.corrcoef(dy, dx)[0, 1])
    print("seed %d epoch %d N %d: worst cell / flip deviation %.2f sigma, rho sqrt(N) %.2f" % (seed, epoch, N, worst, rho * math.sqrt(N)))
    assert abs(rho) * math.sqrt(N) < 5.0
    # no flip asked for: none drawn; span 1 (the test pipeline): no offset
    assert not OO.draws(seed, epoch, np.arange(64), span, flip=False)[2].any()
    d1 = OO.draws(seed, epoch, np.arange(64), 1)
    assert not d1[0].any() and not d1[1].any()


def test_pair_plan_iteration_counts_and_batch_sizes():
    from alignq_amd import data as D
    assert D._pass_sizes(20, 6) == [6, 6, 6, 2] and D._pass_sizes(15, 6) == [6, 6, 3] and D._pass_sizes(12, 6) == [6, 6]
    # DANN: zip stops at the shorter loader; the third iteration is 6 + 3 rows
    assert D.pair_plan((20, 6), (15, 6), "zip") == [(6, 6, False, False), (6, 6, False, False), (6, 3, False, False)]
    # DSAN: max(len) iterations; the target's short third batch is replaced by the first of a new pass, then the source's short
    # fourth batch meets the target's full one and is replaced too
    assert D.pair_plan((20, 6), (15, 6), "cycle") == [(6, 6, False, False), (6, 6, False, False), (6, 6, False, True), (6, 6, True, False)]
    # Amazon -> Webcam at batch 28: 101 and 29 batches per pass (100 x 28 + 17, 28 x 28 + 11)
    z = D.pair_plan((2817, 28), (795, 28), "zip")
    assert len(z) == 29 and z[:28] == [(28, 28, False, False)] * 28 and z[28] == (28, 11, False, False)
    c = D.pair_plan((2817, 28), (795, 28), "cycle")
    assert len(c) == 101 and all(row[:2] == (28, 28) for row in c)
    assert [i for i, row in enumerate(c) if row[3]] == [28, 56, 84] and [i for i, row in enumerate(c) if row[2]] == [100]
    # the other way round, and equal short batches (no pass begins: both are 3)
    assert [i for i, row in enumerate(D.pair_plan((795, 28), (2817, 28), "cycle")) if row[2]] == [28, 56, 84]
    assert D.pair_plan((15, 6), (15, 6), "cycle") == [(6, 6, False, False), (6, 6, False, False), (3, 3, False, False)]
    # a loader without a short batch that runs out begins a new pass where the reference would stop
    assert D.pair_plan((20, 6), (12, 6), "cycle") == [(6, 6, False, False), (6, 6, False, False), (6, 6, False, True), (6, 6, True, False)]
    with pytest.raises(ValueError):
        D.pair_plan((20, 6), (15, 6), "chain")


def test_office_step_takes_a_pair_producer():
    from alignq_amd import data as D
    from alignq_amd.resnet_office import DANN, DSAN, Bottleneck, ResNet
    from alignq_amd.train_step import DSANTrainStep, OfficeTrainStep
    for cls, step_cls in ((DANN, OfficeTrainStep), (DSAN, DSANTrainStep)):
        net = cls(lambda w, a, s: ResNet(w, a, s, Bottleneck, [1, 1, 1, 1], width_per_group=8), 4, 4, "aligned")
        step = step_cls(net, lr=0.004)
        assert step.set_producer(None) is step and step._producer is None
        for wrong in (object(), "loader", 3):
            with pytest.raises(TypeError):
                step.set_producer(wrong)
        with pytest.raises(RuntimeError, match="set_producer"):
            step.next()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.DeviceImages.office(np.zeros((2, 256, 256, 3), np.uint8), np.zeros(2, np.int64), device="cpu")


def test_read_image_folder_order_labels_and_resize(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from alignq_amd import data as D
    rng = np.random.default_rng(3)
    written = {}
    # class directories and files created out of order; one nested directory; a non-image file that must be ignored
    for cls, files in (("mug", ["b.png", "a.png"]), ("bike", ["z.png", "sub/c.png", "m.png"]), ("desk", ["only.png"])):
        for k, rel in enumerate(files):
            path = tmp_path / cls / rel
            os.makedirs(path.parent, exist_ok=True)
            h, w = int(rng.integers(5, 23)), int(rng.integers(5, 23))
            mode = "L" if (cls, k) == ("mug", 0) else "RGB"                       # a grey image goes through convert("RGB")
            arr = rng.integers(0, 256, (h, w) if mode == "L" else (h, w, 3), dtype=np.uint8)
            Image.fromarray(arr).save(path)
            written[(cls, rel)] = path
    (tmp_path / "bike" / "notes.txt").write_text("not an image")
    images, labels, classes = D.read_image_folder(str(tmp_path), side=16)
    assert classes == ["bike", "desk", "mug"]
    # ImageFolder: classes sorted; within a class os.walk's directories sorted by path, files sorted by name
    order = [("bike", "m.png"), ("bike", "z.png"), ("bike", "sub/c.png"), ("desk", "only.png"), ("mug", "a.png"), ("mug", "b.png")]
    assert images.dtype == np.uint8 and images.shape == (6, 16, 16, 3) and images.flags["C_CONTIGUOUS"]
    assert labels.dtype == np.int64 and labels.tolist() == [0, 0, 0, 1, 2, 2]
    for n, key in enumerate(order):
        with open(written[key], "rb") as fh:
            exp = np.asarray(Image.open(fh).convert("RGB").resize((16, 16), Image.BILINEAR))
        assert np.array_equal(images[n], exp), key
    assert D.OFFICE_SIDE == 256 and D.OFFICE_CROP == 224
