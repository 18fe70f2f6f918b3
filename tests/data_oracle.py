"""NumPy restatement of the device input pipeline's specification (include/alignq.h: alignq_data_batch), written from the
header's text and torchvision's documented semantics, not from the kernel: RandomCrop(32, padding=4) pads the uint8 image with
zero BYTES and cuts a 32 x 32 window at a uniform offset in 0..8 per axis, RandomHorizontalFlip mirrors the cropped image,
ToTensor + Normalize map byte v of channel c to ((v / 255) - mean_c) / std_c in fp32.  The batch is formed image by image with
the padded array actually built and sliced (the kernel computes shifted indices instead)."""
import numpy as np
import torch

M1, M2, GOLDEN = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB), np.uint64(0x9E3779B97F4A7C15)


def mix64(z):
    z = np.asarray(z, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= M1
        z ^= z >> np.uint64(27)
        z *= M2
        z ^= z >> np.uint64(31)
    return z


def draws(seed, epoch, pos, pad=4, flip=True):
    """(dy, dx, f) int arrays for the sample positions `pos` of epoch `epoch`"""
    pos = np.asarray(pos, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = mix64(mix64(np.uint64(seed)) + np.uint64(np.uint32(epoch)))
        r = mix64(key + GOLDEN * (pos + np.uint64(1)))
    m24 = np.uint64(0xFFFFFF)
    dy = ((r & m24) * np.uint64(9)) >> np.uint64(24)
    dx = (((r >> np.uint64(24)) & m24) * np.uint64(9)) >> np.uint64(24)
    f = (r >> np.uint64(48)) & np.uint64(1)
    dy, dx, f = dy.astype(np.int64), dx.astype(np.int64), f.astype(np.int64)
    if pad == 0:
        dy, dx = np.zeros_like(dy), np.zeros_like(dx)
    if not flip:
        f = np.zeros_like(f)
    return dy, dx, f


def normalise_table(mean, std):
    """[3][256] fp32 with torch in the arithmetic of transforms.ToTensor (byte -> float32, div(255)) and transforms.Normalize
    (sub_(mean).div_(std) with float32 mean / std tensors)"""
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    return np.stack([v.clone().sub_(torch.as_tensor(m, dtype=torch.float32)).div_(torch.as_tensor(s, dtype=torch.float32)).numpy()
                     for m, s in zip(mean, std)])


def augmented_bytes(images, perm, positions, seed, epoch, pad, flip):
    """uint8 [n, 32, 32, 3]: the cropped and flipped images of the given epoch positions, and the samples they came from"""
    positions = np.asarray(positions, dtype=np.int64)
    s = positions if perm is None else np.asarray(perm)[positions]
    dy, dx, f = draws(seed, epoch, positions, pad, flip)
    out = np.empty((len(positions), 32, 32, 3), dtype=np.uint8)
    for n, (sample, a, b, fl) in enumerate(zip(s, dy, dx, f)):
        img = np.pad(images[sample], ((pad, pad), (pad, pad), (0, 0)))          # zero bytes
        img = img[a:a + 32, b:b + 32]
        out[n] = img[:, ::-1] if fl else img
    return out, s


def batch(images, labels, perm, lut, first, B, rank, world, seed, epoch, pad, flip):
    """(x [rows, 3, 32, 32] fp32, y [rows] int64) of the batch whose first position is `first`: rows = the positions below N"""
    N = len(images)
    positions = first + rank * B + np.arange(B)
    positions = positions[positions < N]
    u8, s = augmented_bytes(images, perm, positions, seed, epoch, pad, flip)
    x = np.empty((len(positions), 3, 32, 32), dtype=np.float32)
    for c in range(3):
        x[:, c] = lut[c][u8[..., c]]
    return x, np.asarray(labels, dtype=np.int64)[s]
