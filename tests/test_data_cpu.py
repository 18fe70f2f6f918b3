"""CPU-side checks of the device input pipeline (include/alignq.h: alignq_data_batch; alignq_amd/data.py): the normalisation
table against torch's ToTensor / Normalize arithmetic, the statistical and structural properties of the specified random draws
(on tests/data_oracle.py, the NumPy statement of the specification), the CIFAR-10 batch reader, and the ABI boundary.

There is no reference-generated fixture for this feature: torchvision is not available to the tests and the reference's data
modules cannot be imported without it.  The pin is the table identity plus the element-wise semantics of the header, which are
torchvision's documented ones.

The bounds of the distribution test are derived, not tuned: with N = 50 000 independent draws a cell of probability p holds
N p +- sqrt(N p (1 - p)): p = 1/81 gives 617.3 +- 24.7 (5 sigma: 124), p = 1/2 gives 25 000 +- 111.8 (5 sigma: 559)."""
import math
import os
import pickle

import numpy as np
import pytest
import torch

from tests import data_oracle as DO

N = 50_000
SEEDS = (0, 1, 20240607)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("preset", ["cifar10_train", "cifar10_test", "svhn"])
def test_table_is_totensor_normalize_bit_for_bit(preset):
    from alignq_amd import data as D
    p = D.PRESETS[preset]
    lut = D.normalise_table(p["mean"], p["std"])
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256) and lut.is_contiguous()
    for c in range(3):
        # the issue's statement of the arithmetic, with Python scalars ...
        exp = torch.arange(256, dtype=torch.uint8).float().div(255).sub(p["mean"][c]).div(p["std"][c])
        assert np.array_equal(bits(lut[c].numpy()), bits(exp.numpy())), (preset, c)
        # ... and torchvision's own sequence on a whole image of that byte: ToTensor = byte -> float32, div(255); Normalize =
        # sub_(mean[:, None, None]).div_(std[:, None, None]) with float32 mean / std tensors
        img = torch.arange(256, dtype=torch.uint8).view(1, 16, 16).expand(3, 16, 16)
        t = img.to(torch.float32).div(255)
        t = t.clone().sub_(torch.as_tensor(p["mean"], dtype=torch.float32).view(-1, 1, 1)).div_(
            torch.as_tensor(p["std"], dtype=torch.float32).view(-1, 1, 1))
        assert np.array_equal(bits(lut[c].numpy()), bits(t[c].reshape(-1).numpy())), (preset, c)
        # the padded value is the table's entry of byte 0, (0 - mean) / std, not 0.0
        pad_value = (torch.zeros((), dtype=torch.float32) - torch.tensor(p["mean"][c], dtype=torch.float32)) / \
            torch.tensor(p["std"][c], dtype=torch.float32)
        assert bits(lut[c, 0].numpy()) == bits(pad_value.numpy()) and float(lut[c, 0]) != 0.0
    assert np.array_equal(bits(DO.normalise_table(p["mean"], p["std"])), bits(lut.numpy()))


@pytest.mark.parametrize("seed", SEEDS)
def test_draws_are_uniform_within_five_sigma(seed):
    pos = np.arange(N)
    dy, dx, f = DO.draws(seed, 0, pos)
    assert dy.min() == 0 and dy.max() == 8 and dx.min() == 0 and dx.max() == 8 and set(np.unique(f)) == {0, 1}
    cells = np.bincount(dy * 9 + dx, minlength=81)
    p = 1.0 / 81
    bound = 5.0 * math.sqrt(N * p * (1 - p))
    print("seed %d: offsets %d..%d of %.1f +- %.1f; flips %d of %d +- %.1f" % (seed, cells.min(), cells.max(), N * p, bound,
                                                                          int(f.sum()), N // 2, 5.0 * math.sqrt(N * 0.25)))
    assert len(cells) == 81 and np.abs(cells - N * p).max() <= bound
    assert abs(int(f.sum()) - N / 2) <= 5.0 * math.sqrt(N * 0.25)
    # without augmentation nothing is drawn
    dy0, dx0, f0 = DO.draws(seed, 0, pos, pad=0, flip=False)
    assert not dy0.any() and not dx0.any() and not f0.any()


def test_draws_depend_on_seed_and_epoch_and_repeat():
    pos = np.arange(N)
    base = np.stack(DO.draws(7, 3, pos))
    assert np.array_equal(base, np.stack(DO.draws(7, 3, pos)))                 # the same pair: the same bits
    for other in (DO.draws(7, 4, pos), DO.draws(8, 3, pos)):
        same = (np.stack(other) == base).all(axis=0).mean()
        # independent draws agree on all of (dy, dx, f) with probability 1 / 162: 0.0062 +- 0.00035
        assert abs(same - 1 / 162) < 5 * math.sqrt((1 / 162) * (161 / 162) / N), same
    # a position's draw does not depend on which positions are asked for with it
    sub = np.array([5, 49_999, 128, 127])
    assert np.array_equal(np.stack(DO.draws(7, 3, sub)), base[:, sub])


def _synthetic(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8), rng.integers(0, 10, n).astype(np.int64)


def test_every_sample_once_and_batching_does_not_change_the_epoch():
    """One epoch of the oracle over a seeded set: every sample exactly once, and the image at a position is the same whether the
    epoch is cut into batches of 128, of 100, or of 2 x 64 (two ranks)."""
    from alignq_amd import data as D
    n = N
    images, labels = _synthetic(n, 5)
    lut = D.normalise_table(D.CIFAR10_MEAN, D.CIFAR10_STD).numpy()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(11)).numpy()
    assert np.array_equal(np.sort(perm), np.arange(n))
    seed, epoch = 3, 2

    def epoch_of(B, world):
        ys, firsts = [], []
        xs = {}
        first = 0
        while first < n:
            left = n - first
            b = min(B, -(-left // world))
            for rank in range(world):
                x, y = DO.batch(images, labels, perm, lut, first, b, rank, world, seed, epoch, 4, True)
                assert x.shape[0] == b and y.shape[0] == b
                ys.append(y)
                if first in keep_firsts or first + world * b >= n:
                    xs[(first, rank)] = x
            firsts.append(first)
            first += world * b
        return np.concatenate(ys), xs, firsts

    keep_firsts = {0, 6400, 32000}          # common batch boundaries of 128, 100 and 2 x 64
    y128, x128, f128 = epoch_of(128, 1)
    y100, x100, f100 = epoch_of(100, 1)
    y264, x264, f264 = epoch_of(64, 2)
    assert len(f128) == 391 and len(f264) == 391 and len(f100) == 500
    # every sample once: the labels of the epoch in position order are the permuted labels
    for ys in (y128, y100, y264):
        assert np.array_equal(ys, labels[perm])
    for first in keep_firsts:
        a = x128[(first, 0)]
        assert np.array_equal(bits(a[:100]), bits(x100[(first, 0)]))
        assert np.array_equal(bits(a[:64]), bits(x264[(first, 0)])) and np.array_equal(bits(a[64:]), bits(x264[(first, 1)]))
    # the short last batch: 80 of 128, = 2 x 40, and the last 80 positions of the batches of 100
    last = x128[(49920, 0)]
    assert last.shape[0] == 80
    assert np.array_equal(bits(last[:40]), bits(x264[(49920, 0)])) and np.array_equal(bits(last[40:]), bits(x264[(49920, 1)]))
    assert np.array_equal(bits(last), bits(x100[(49900, 0)][20:]))
    # sampled images against a third, scalar statement of the element rule of the header
    dy, dx, f = DO.draws(seed, epoch, np.arange(n))
    rng = np.random.default_rng(0)
    for pos in (0, 1, 127, 49_999):
        x = x128[(pos // 128 * 128, 0)][pos % 128] if (pos // 128 * 128, 0) in x128 else None
        if x is None:
            continue
        for _ in range(200):
            c, h, w = rng.integers(0, 3), rng.integers(0, 32), rng.integers(0, 32)
            sh = h + dy[pos] - 4
            sw = (31 - w if f[pos] else w) + dx[pos] - 4
            byte = images[perm[pos], sh, sw, c] if (0 <= sh < 32 and 0 <= sw < 32) else 0
            assert bits(x[c, h, w]) == bits(lut[c][byte])


def test_oracle_pads_with_the_zero_byte_value():
    """An all-255 image shifted fully into a corner: the border holds lut[c][0], the inside lut[c][255]."""
    from alignq_amd import data as D
    lut = D.normalise_table(D.CIFAR10_MEAN, D.CIFAR10_STD).numpy()
    images = np.full((1, 32, 32, 3), 255, dtype=np.uint8)
    for pos in range(400):
        dy, dx, f = (int(v[0]) for v in DO.draws(1, 0, [pos]))
        x, _ = DO.batch(np.repeat(images, pos + 1, 0), np.zeros(pos + 1, np.int64), None, lut, pos, 1, 0, 1, 1, 0, 4, True)
        inside = np.zeros((32, 32), dtype=bool)
        inside[max(0, 4 - dy):min(32, 36 - dy), max(0, 4 - dx):min(32, 36 - dx)] = True
        if f:
            inside = inside[:, ::-1]
        for c in range(3):
            assert np.array_equal(bits(x[0, c][inside]), np.full(inside.sum(), bits(lut[c][255])))
            assert np.array_equal(bits(x[0, c][~inside]), np.full((~inside).sum(), bits(lut[c][0])))


def test_read_cifar10_dir(tmp_path):
    from alignq_amd import data as D
    rng = np.random.default_rng(1)
    root = tmp_path / "cifar-10-batches-py"
    os.makedirs(root)
    planes, labels = [], []
    for name in ["data_batch_%d" % i for i in range(1, 6)] + ["test_batch"]:
        d = rng.integers(0, 256, (7, 3072), dtype=np.uint8)
        lab = [int(v) for v in rng.integers(0, 10, 7)]
        with open(root / name, "wb") as fh:
            pickle.dump({b"data": d, b"labels": lab, b"batch_label": name.encode(), b"filenames": [b"x"] * 7}, fh, protocol=2)
        planes.append(d)
        labels.append(lab)
    for where in (tmp_path, root):
        images, lab = D.read_cifar10_dir(str(where), train=True)
        assert images.dtype == np.uint8 and images.shape == (35, 32, 32, 3) and images.flags["C_CONTIGUOUS"]
        assert lab.dtype == np.int64 and lab.tolist() == sum(labels[:5], [])
        # plane order R, G, B of 1024 row-major pixels each -> HWC
        for n, (b, i) in enumerate((b, i) for b in range(5) for i in range(7)):
            for c in range(3):
                assert np.array_equal(images[n, :, :, c], planes[b][i, 1024 * c:1024 * (c + 1)].reshape(32, 32))
        test_images, test_lab = D.read_cifar10_dir(str(where), train=False)
        assert test_images.shape == (7, 32, 32, 3) and test_lab.tolist() == labels[5]
        assert np.array_equal(test_images[3, 5, 9], planes[5][3, [5 * 32 + 9, 1024 + 5 * 32 + 9, 2048 + 5 * 32 + 9]])


def test_no_cpu_fallback():
    from alignq_amd import data as D
    images, labels = _synthetic(4, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.DeviceImages(images, labels, D.CIFAR10_MEAN, D.CIFAR10_STD, device="cpu")
    assert D.PRESETS["cifar10_train"]["pad"] == 4 and D.PRESETS["cifar10_train"]["flip"] and D.PRESETS["cifar10_train"]["shuffle"]
    assert D.PRESETS["cifar10_test"] == dict(mean=D.CIFAR10_MEAN, std=D.CIFAR10_STD, pad=0, flip=False, shuffle=False)
    assert D.PRESETS["svhn"]["mean"] == (0.5, 0.5, 0.5) == D.PRESETS["svhn"]["std"] and D.PRESETS["svhn"]["pad"] == 0


def test_symbols_declared_mirrored_exported_and_argument_validation():
    """alignq_data_batch: in the header, in the ctypes table, in the library; bad arguments come back as
    ALIGNQ_EINVAL before anything touches a device (this runs without one)."""
    import ctypes
    import re
    from alignq_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "alignq.h")).read(), flags=re.S)
    lib = L.load()
    for name in ("alignq_data_batch",):
        assert re.search(r"\b%s\s*\(" % name, header) and name in L.SIGNATURES and hasattr(lib, name)
    assert lib.alignq_abi_version() == 23
    # host buffers stand in for device pointers: every call below must be refused before a launch
    img = (ctypes.c_uint8 * 3072)()
    lab, perm, y = (ctypes.c_int64 * 1)(), (ctypes.c_int64 * 1)(), (ctypes.c_int64 * 1)()
    cur = (ctypes.c_int32 * 4)()
    buf = (ctypes.c_float * (768 + 3072 + 8))()
    base = ctypes.addressof(buf)
    lut = (base + 15) & ~15
    x = lut + 768 * 4
    a = lambda t: ctypes.addressof(t)                                         # noqa: E731
    good = dict(images=a(img), labels=a(lab), perm=a(perm), cursor=a(cur), advance=1, lut=lut, N=1, B=1, rank=0, world=1, seed=0, pad=4, flip=1,
                x_out=x, nhwc=0, y_out=a(y), stream=None)
    order = list(good)

    def call(**kw):
        args = dict(good, **kw)
        return lib.alignq_data_batch(*[args[k] for k in order])

    bad = [dict(B=0), dict(B=-3), dict(pad=1), dict(pad=8), dict(pad=-4), dict(rank=1), dict(rank=2, world=2), dict(rank=-1),
           dict(world=0), dict(N=0), dict(advance=-1), dict(flip=2), dict(nhwc=2), dict(images=None), dict(labels=None), dict(cursor=None),
           dict(lut=None), dict(x_out=None), dict(y_out=None), dict(x_out=x + 4), dict(lut=lut + 8)]
    for kw in bad:
        assert call(**kw) == L.EINVAL, kw
    assert call(B=70000) == L.EUNSUPPORTED and call(N=(1 << 30) + 1) == L.EUNSUPPORTED
    assert call(advance=(1 << 30) + 1) == L.EUNSUPPORTED
    assert list(cur) == [0, 0, 0, 0] and not any(buf)
