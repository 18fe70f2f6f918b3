"""NumPy restatement of the Office input pipeline's specification (include/alignq.h: alignq_data_crop_batch), written from the
header's text and torchvision's documented semantics, not from the kernel: RandomCrop(crop) cuts a crop x crop window at a
uniform offset in 0..side-crop per axis (CenterCrop: at int(round((side - crop) / 2.0))), RandomHorizontalFlip mirrors the cropped
window, ToTensor + Normalize map byte v of channel c to ((v / 255) - mean_c) / std_c in fp32.  The batch is formed image by image
by slicing (the kernel computes indices instead)."""
import numpy as np

from tests.data_oracle import GOLDEN, mix64, normalise_table  # noqa: F401  (the draw sequence and the table are shared)


def draws(seed, epoch, pos, span, flip=True):
    """(dy, dx, f) int arrays for the sample positions `pos` of epoch `epoch`: dy, dx in 0..span-1"""
    pos = np.asarray(pos, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = mix64(mix64(np.uint64(seed)) + np.uint64(np.uint32(epoch)))
        r = mix64(key + GOLDEN * (pos + np.uint64(1)))
    m24 = np.uint64(0xFFFFFF)
    dy = ((r & m24) * np.uint64(span)) >> np.uint64(24)
    dx = (((r >> np.uint64(24)) & m24) * np.uint64(span)) >> np.uint64(24)
    f = (r >> np.uint64(48)) & np.uint64(1)
    dy, dx, f = dy.astype(np.int64), dx.astype(np.int64), f.astype(np.int64)
    if not flip:
        f = np.zeros_like(f)
    return dy, dx, f


def window(side, crop, train):
    """(span, off0) of the two pipelines"""
    return (side - crop + 1, 0) if train else (1, int(round((side - crop) / 2.0)))


def batch(images, labels, perm, lut, first, B, rank, world, seed, epoch, crop, span, off0, flip):
    """(x [rows, 3, crop, crop] fp32, y [rows] int64, kept [rows] bool) of the batch whose first position is `first`: rows = the
    positions below N; kept[i] is False where the permutation's entry lies outside the set (such a row is not written)."""
    N = len(images)
    positions = first + rank * B + np.arange(B)
    positions = positions[(positions >= 0) & (positions < N)]
    s = positions if perm is None else np.asarray(perm)[positions]
    kept = (s >= 0) & (s < N)
    dy, dx, f = draws(seed, epoch, positions, span, flip)
    x = np.zeros((len(positions), 3, crop, crop), dtype=np.float32)
    y = np.zeros(len(positions), dtype=np.int64)
    for n in np.nonzero(kept)[0]:
        oy, ox = off0 + dy[n], off0 + dx[n]
        win = images[s[n]][oy:oy + crop, ox:ox + crop]
        assert win.shape == (crop, crop, 3)
        if f[n]:
            win = win[:, ::-1]
        for c in range(3):
            x[n, c] = lut[c][win[..., c]]
        y[n] = labels[s[n]]
    return x, y, kept
