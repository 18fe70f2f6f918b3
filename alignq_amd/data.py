"""The reference's input pipeline (cdf_alignment_admm/resnet-20-cifar-10/data/cifar10.py:11-33: RandomCrop(32, padding=4),
RandomHorizontalFlip(), ToTensor(), Normalize(mean, std) in a shuffling DataLoader without drop_last;
cdf_alignment/resnet-20-svhn/data/svhn.py:14-34: ToTensor(), Normalize) on the device: the data set lives in device memory as
bytes, and ONE launch (alignq_data_batch, csrc/data_kernels.hip) gathers, crops, flips, normalises and lays out a batch directly
in the tensors a captured step reads.  Attached to a step (`step.set_producer(loader)`) the launch is the first node of the
step's HIP graph, and an epoch is ceil(N / B) replays with no host work per batch and no host-to-device traffic.

    train = DeviceImages.from_cifar10_dir(root, train=True, device="cuda")        # preset "cifar10_train"
    loader = DeviceLoader(train, 128, shuffle=True, seed=0)
    step = TrainStep(net, channels_last=True).set_producer(loader)
    step.capture(*loader.peek())
    for epoch in range(epochs):
        step.set_lr(lr_of(epoch))
        logits, ce, trans_loss = train_epoch(step, loader, epoch)

The Office trees (dann_office/data/office.py:13-38, the same in dsan_office: Resize((256, 256)), RandomCrop(224),
RandomHorizontalFlip, ToTensor, Normalize(ImageNet mean, std), shuffle, no drop_last) use the same objects on larger images: the
set is resized ONCE at load time (Resize is deterministic) and kept as bytes [N, 256, 256, 3]; alignq_data_crop_batch cuts the
224 x 224 window.  A PairLoader (a source and a target DeviceLoader) is the producer of an OfficeTrainStep / DSANTrainStep:

    src = DeviceImages.from_image_folder(amazon_root, train=True, device="cuda")  # preset "office_train"
    tgt = DeviceImages.from_image_folder(webcam_root, train=True, device="cuda")
    pair = PairLoader(DeviceLoader(src, 28, seed=0, channels_last=True), DeviceLoader(tgt, 28, seed=1, channels_last=True), "zip")
    step = OfficeTrainStep(net, channels_last=True, device_hyper=True).set_producer(pair)
    step.set_schedule(schedule.office_dann(lr, num_epochs, max(len(pair.src), len(pair.tgt))))
    step.capture(*pair.peek())
    for epoch in range(start_epoch, num_epochs):
        train_epoch_office(step, pair, epoch, epoch_index=epoch - start_epoch)

The random draws are a stateless function of (seed, epoch, position in the epoch) - include/alignq.h states it - so an epoch does
not depend on the batch size, the rank or the world size.  No CPU fallback: tensors that are not on a CUDA / ROCm device raise."""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch

from . import _lib as L

CIFAR10_MEAN, CIFAR10_STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
OFFICE_SIDE, OFFICE_CROP = 256, 224
# the reference pipelines (shuffle: the DataLoader's default for this split)
PRESETS = {
    "cifar10_train": dict(mean=CIFAR10_MEAN, std=CIFAR10_STD, pad=4, flip=True, shuffle=True),
    "cifar10_test": dict(mean=CIFAR10_MEAN, std=CIFAR10_STD, pad=0, flip=False, shuffle=False),
    "svhn": dict(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), pad=0, flip=False, shuffle=True),
    # dann_office / dsan_office data/office.py:13-38.  The reference shuffles its test loader too; only the order in which the
    # metrics are summed depends on that, and `evaluate` wants an unshuffled loader.
    "office_train": dict(mean=IMAGENET_MEAN, std=IMAGENET_STD, flip=True, shuffle=True, crop=OFFICE_CROP, window="random"),
    "office_test": dict(mean=IMAGENET_MEAN, std=IMAGENET_STD, flip=False, shuffle=False, crop=OFFICE_CROP, window="center"),
}


def center_offset(side, crop):
    """Where torchvision's CenterCrop starts its window: int(round((side - crop) / 2.0)) (Python's round: halves go to even)."""
    return int(round((side - crop) / 2.0))


def normalise_table(mean, std):
    """[3][256] fp32 on the host: the value of byte v in channel c in exactly the arithmetic of torchvision's ToTensor
    (`img.to(float32).div(255)`) and Normalize (`tensor.sub_(mean).div_(std)`, mean / std as float32 tensors).  The kernel only
    gathers from it, so what it writes is bit-equal to the reference's transforms by construction; a pixel of the padding (byte 0)
    gets table[c][0] = (0 - mean_c) / std_c, not 0.0."""
    mean_t = torch.as_tensor(mean, dtype=torch.float32).view(3, 1)
    std_t = torch.as_tensor(std, dtype=torch.float32).view(3, 1)
    if (std_t == 0).any():
        raise ValueError("normalise_table: std must be non-zero")
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    return v.repeat(3, 1).sub_(mean_t).div_(std_t).contiguous()


def read_cifar10_dir(root, train=True):
    """(images uint8 [N, 32, 32, 3], labels int64 [N]) from the CIFAR-10 python batches under `root` (or root/cifar-10-batches-py):
    data_batch_1..5 or test_batch, pickled dicts with b'data' uint8 [10000, 3072] in plane order R, G, B and b'labels'; reordered
    to HWC as torchvision's CIFAR10.data.  Standard library only; nothing is downloaded."""
    sub = os.path.join(root, "cifar-10-batches-py")
    base = sub if os.path.isdir(sub) else root
    names = ["data_batch_%d" % i for i in range(1, 6)] if train else ["test_batch"]
    data, labels = [], []
    for name in names:
        with open(os.path.join(base, name), "rb") as fh:
            entry = pickle.load(fh, encoding="bytes")
        data.append(np.asarray(entry[b"data"], dtype=np.uint8).reshape(-1, 3, 32, 32))
        labels.extend(entry[b"labels"] if b"labels" in entry else entry[b"fine_labels"])
    images = np.ascontiguousarray(np.concatenate(data).transpose(0, 2, 3, 1))
    return images, np.asarray(labels, dtype=np.int64)


IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")      # torchvision's ImageFolder


def read_image_folder(root, side=OFFICE_SIDE):
    """(images uint8 [N, side, side, 3], labels int64 [N], class names) of a directory of class directories in the order of
    torchvision's ImageFolder: the sorted class directories map to 0, 1, ...; within a class the files of os.walk(followlinks)
    with sorted directory and file names.  Every image is opened as ImageFolder's loader does (PIL, convert("RGB")) and resized
    to side x side with PIL's bilinear filter: transforms.Resize((side, side)) on a PIL image, done ONCE here because it is
    deterministic.  PIL is needed by this function only."""
    from PIL import Image
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"read_image_folder: no class directories under {root}")
    images, labels = [], []
    for index, name in enumerate(classes):
        for folder, _, files in sorted(os.walk(os.path.join(root, name), followlinks=True)):
            for fname in sorted(files):
                if not fname.lower().endswith(IMG_EXTENSIONS):
                    continue
                with open(os.path.join(folder, fname), "rb") as fh:
                    img = Image.open(fh).convert("RGB")
                images.append(np.asarray(img.resize((side, side), Image.BILINEAR), dtype=np.uint8))
                labels.append(index)
    if not images:
        raise FileNotFoundError(f"read_image_folder: no image files under {root}")
    return np.ascontiguousarray(np.stack(images)), np.asarray(labels, dtype=np.int64), classes


def _cuda_device(device, who):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"alignq_amd: {who} needs a CUDA/ROCm device, got {dev} (there is no CPU fallback in the product path)")
    return dev


class DeviceImages:
    """An RGB data set resident on the device: uint8 [N, side, side, 3] (HWC), int64 labels [N], the normalisation table, and the
    augmentation of its pipeline.  Without `crop`: a 32 x 32 set (pad: 0 or 4 = RandomCrop(32, padding=pad); flip:
    RandomHorizontalFlip), produced by alignq_data_batch.  With `crop`: a crop x crop window of the stored image, window="random"
    (RandomCrop(crop): span = side - crop + 1 offsets per axis from off0 = 0) or "center" (CenterCrop(crop): span = 1, off0 =
    center_offset(side, crop)), produced by alignq_data_crop_batch."""

    def __init__(self, images_u8, labels, mean, std, device="cuda", pad=0, flip=False, shuffle=False, crop=None, window=None):
        dev = _cuda_device(device, "DeviceImages")
        images_u8, labels = torch.as_tensor(images_u8), torch.as_tensor(labels)
        if crop is None:
            if window is not None:
                raise ValueError("DeviceImages: window needs crop")
            if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or tuple(images_u8.shape[1:]) != (32, 32, 3):
                raise TypeError(f"DeviceImages: images must be uint8 [N, 32, 32, 3] (HWC), got {images_u8.dtype} {tuple(images_u8.shape)}")
        elif images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[1] != images_u8.shape[2] or images_u8.shape[3] != 3:
            raise TypeError(f"DeviceImages: images must be uint8 [N, side, side, 3] (HWC), got {images_u8.dtype} {tuple(images_u8.shape)}")
        if labels.dim() != 1 or labels.shape[0] != images_u8.shape[0] or labels.dtype.is_floating_point:
            raise TypeError("DeviceImages: labels must be one integer per image")
        if images_u8.shape[0] < 1 or images_u8.shape[0] > (1 << 30):
            raise ValueError("DeviceImages: 1 <= N <= 2^30")
        if pad not in (0, 4):
            raise ValueError("DeviceImages: pad must be 0 or 4")
        self.side = int(images_u8.shape[1])
        if crop is None:
            self.crop, self.span, self.off0 = self.side, None, None
        else:
            crop = int(crop)
            if pad or crop < 4 or crop % 4 or crop > self.side or self.side > 1024:
                raise ValueError("DeviceImages: a cropped set needs pad = 0, crop a multiple of 4 in [4, side] and side <= 1024")
            if window not in ("random", "center"):
                raise ValueError('DeviceImages: window must be "random" or "center"')
            self.crop = crop
            self.span, self.off0 = (self.side - crop + 1, 0) if window == "random" else (1, center_offset(self.side, crop))
            if self.span > 255:
                raise ValueError("DeviceImages: at most 255 window offsets per axis (side - crop <= 254)")
        self.images = images_u8.to(dev).contiguous()
        self.labels = labels.to(dev, torch.int64).contiguous()
        self.lut = normalise_table(mean, std).to(dev)
        self.pad, self.flip, self.shuffle = int(pad), bool(flip), bool(shuffle)
        self.device = dev

    def __len__(self):
        return int(self.images.shape[0])

    @property
    def out_shape(self):
        """(3, H, W) of one produced image"""
        return (3, self.crop, self.crop)

    @classmethod
    def preset(cls, name, images_u8, labels, device="cuda"):
        """One of PRESETS: "cifar10_train", "cifar10_test", "svhn", "office_train", "office_test"."""
        return cls(images_u8, labels, device=device, **PRESETS[name])

    @classmethod
    def from_cifar10_dir(cls, root, train=True, device="cuda"):
        images, labels = read_cifar10_dir(root, train)
        return cls.preset("cifar10_train" if train else "cifar10_test", images, labels, device)

    @classmethod
    def office(cls, images_u8, labels, train=True, device="cuda"):
        """images_u8 [N, 256, 256, 3]: an Office domain already resized (read_image_folder)."""
        return cls.preset("office_train" if train else "office_test", images_u8, labels, device)

    @classmethod
    def from_image_folder(cls, root, train=True, device="cuda"):
        images, labels, _ = read_image_folder(root, OFFICE_SIDE)
        return cls.office(images, labels, train, device)


class DeviceLoader:
    """Batches of a DeviceImages set in the reference loader's order of work: a fresh permutation per epoch (or the identity),
    ceil(N / (world * B)) batches including the short last one.  Data parallel: a global batch is world * B consecutive positions
    of the epoch, of which this rank takes B (every rank builds the same permutation from (seed, epoch); N must then be a multiple
    of world so that the short last batch has the same size on every rank).

    The permutation and the cursor {epoch, position} are persistent device buffers: begin_epoch rewrites them in place and is the
    only host write; `fill` enqueues one batch and the launch itself moves the cursor on (its last workgroup to have read it), so a
    HIP graph that holds a `fill` produces batch n on its n-th replay after begin_epoch."""

    def __init__(self, images: DeviceImages, batch_size, shuffle=None, seed=0, rank=0, world=1, channels_last=False):
        if not isinstance(images, DeviceImages):
            raise TypeError("DeviceLoader: images must be a DeviceImages")
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("DeviceLoader: batch_size >= 1 and 0 <= rank < world")
        if world > 1 and len(images) % world:
            raise ValueError("DeviceLoader: with world > 1 the set size must be a multiple of world")
        self.images = images
        self.batch_size, self.rank, self.world = int(batch_size), int(rank), int(world)
        self.shuffle = images.shuffle if shuffle is None else bool(shuffle)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        dev = images.device
        self.perm = torch.arange(len(images), dtype=torch.int64, device=dev)
        self.cursor = torch.zeros(4, dtype=torch.int32, device=dev)          # {epoch, position, the launch's ticket, unused}
        self._gen = torch.Generator(device=dev)
        fmt = torch.channels_last if channels_last else torch.contiguous_format
        self._x = torch.empty(self.batch_size, *images.out_shape, dtype=torch.float32, device=dev).contiguous(memory_format=fmt)
        self._y = torch.empty(self.batch_size, dtype=torch.int64, device=dev)
        self.epoch, self._pos = 0, 0
        self.begin_epoch(0)

    # ------------------------------------------------------------------------------------------- the epoch
    def __len__(self):
        span = self.world * self.batch_size
        return (len(self.images) + span - 1) // span

    def begin_epoch(self, epoch):
        """The epoch's sample order written IN PLACE into the persistent permutation buffer (torch.randperm of a generator seeded
        with (seed, epoch); the identity without shuffle) and the cursor reset to {epoch, 0}."""
        epoch = int(epoch)
        if not 0 <= epoch < (1 << 31):
            raise ValueError("DeviceLoader.begin_epoch: 0 <= epoch < 2^31")
        if self.shuffle:
            self._gen.manual_seed((self.seed * 1000003 + epoch) & 0x7FFFFFFFFFFFFFFF)
            self.perm.copy_(torch.randperm(len(self.images), generator=self._gen, device=self.perm.device))
        self._set_cursor(epoch, 0)
        self.epoch, self._pos = epoch, 0
        return self

    def _set_cursor(self, epoch, pos):
        self.cursor.copy_(torch.tensor([epoch, pos, 0, 0], dtype=torch.int32))

    def next_batch_size(self):
        """Rows of this rank in the coming batch (0: the epoch is exhausted)"""
        left = len(self.images) - self._pos
        return max(0, min(self.batch_size, -(-left // self.world)))

    def skip(self, rows):
        """Host bookkeeping for a batch of `rows` rows per rank that a replayed graph produced (the device cursor moved by itself)."""
        self._pos += self.world * int(rows)

    # ------------------------------------------------------------------------------------------- one batch
    def record(self, x_out, y_out):
        """Enqueue one batch of x_out.shape[0] rows into the given tensors (layout taken from x_out's memory format); the launch
        itself moves the cursor on.  No synchronisation, no allocation, no host state: this is what a capture records."""
        im = self.images
        if not (torch.is_tensor(x_out) and torch.is_tensor(y_out) and x_out.is_cuda and y_out.is_cuda):
            raise RuntimeError("alignq_amd: DeviceLoader fills CUDA/ROCm tensors (there is no CPU fallback in the product path)")
        if x_out.dtype != torch.float32 or x_out.dim() != 4 or tuple(x_out.shape[1:]) != im.out_shape:
            raise TypeError(f"DeviceLoader: x_out must be float32 [B, {', '.join(map(str, im.out_shape))}], got {x_out.dtype} "
                            f"{tuple(x_out.shape)}")
        if y_out.dtype != torch.int64 or y_out.dim() != 1 or y_out.shape[0] != x_out.shape[0] or not y_out.is_contiguous():
            raise TypeError("DeviceLoader: y_out must be a contiguous int64 [B]")
        if x_out.is_contiguous():
            nhwc = 0
        elif x_out.is_contiguous(memory_format=torch.channels_last):
            nhwc = 1
        else:
            raise TypeError("DeviceLoader: x_out must be contiguous or channels-last")
        B = int(x_out.shape[0])
        if im.span is not None:
            L.check(L.load().alignq_data_crop_batch(L.ptr(im.images), L.ptr(im.labels), L.ptr(self.perm) if self.shuffle else None,
                                                    L.ptr(self.cursor), self.world * B, L.ptr(im.lut), len(im), im.side, im.crop,
                                                    im.span, im.off0, B, self.rank, self.world, self.seed, int(im.flip),
                                                    L.ptr(x_out), nhwc, L.ptr(y_out), L.stream_ptr()),
                    "alignq_data_crop_batch")
            return
        L.check(L.load().alignq_data_batch(L.ptr(im.images), L.ptr(im.labels), L.ptr(self.perm) if self.shuffle else None,
                                           L.ptr(self.cursor), self.world * B, L.ptr(im.lut), len(im), B, self.rank, self.world,
                                           self.seed, im.pad, int(im.flip), L.ptr(x_out), nhwc, L.ptr(y_out), L.stream_ptr()),
                "alignq_data_batch")

    def fill(self, x_out, y_out):
        """`record` plus the host's count of where the epoch stands (what iteration and `next_batch_size` go by)."""
        self.record(x_out, y_out)
        self.skip(x_out.shape[0])

    def next_batch(self):
        """(x, y) of the coming batch, filled eagerly into the loader's own buffers (views of them for the short last batch): valid
        until the next batch is produced.  None when the epoch is exhausted."""
        b = self.next_batch_size()
        if b == 0:
            return None
        x, y = self._x[:b], self._y[:b]
        self.fill(x, y)
        return x, y

    def peek(self):
        """Tensors of a full batch's shape and layout holding the epoch's first batch WITHOUT consuming it: what `capture` wants as
        its example inputs."""
        keep = self._pos
        self._set_cursor(self.epoch, 0)
        x, y = torch.empty_like(self._x), torch.empty_like(self._y)
        self.record(x, y)
        self._set_cursor(self.epoch, keep)
        return x, y

    def __iter__(self):
        if self._pos >= len(self.images):
            self.begin_epoch(self.epoch + 1)
        while True:
            xy = self.next_batch()
            if xy is None:
                return
            yield xy


def _pass_sizes(n, batch, world=1):
    """Rows per rank of the batches of one pass over n samples (DeviceLoader.next_batch_size along the pass)"""
    sizes, pos = [], 0
    while pos < n:
        rows = min(batch, -(-(n - pos) // world))
        sizes.append(rows)
        pos += world * rows
    return sizes


def pair_plan(src, tgt, mode):
    """The iterations of one Office epoch as pure arithmetic.  src, tgt: (set size, batch size[, world]).  Returns one
    (source rows, target rows, source begins a new pass, target begins a new pass) per iteration.
    "zip": dann_office/main.py:340-343, `zip(src_loader, tgt_loader)`: min(len) iterations, no pass begins inside the epoch.
    "cycle": dsan_office/main.py:335-377: max(len) iterations; a loader whose coming batch is smaller than the other's begins a new
    pass and supplies that pass's first batch instead - first the target (:363-369), then the source against the target's
    final batch (:371-377).  (A loader that is exhausted begins a new pass too, where the reference would stop.)"""
    ss, ts = _pass_sizes(*src), _pass_sizes(*tgt)
    if mode == "zip":
        return [(a, b, False, False) for a, b in zip(ss, ts)]
    if mode != "cycle":
        raise ValueError('PairLoader: mode must be "zip" or "cycle"')
    plan, i, j = [], 0, 0
    for _ in range(max(len(ss), len(ts))):
        new_s, new_t = i == len(ss), j == len(ts)
        i, j = (0 if new_s else i), (0 if new_t else j)
        if ts[j] < ss[i]:
            j, new_t = 0, True
        if ts[j] > ss[i]:
            i, new_s = 0, True
        plan.append((ss[i], ts[j], new_s, new_t))
        i, j = i + 1, j + 1
    return plan


class PairLoader:
    """The producer of an Office step: a source and a target DeviceLoader (each with its own permutation, cursor and seed) walked
    together as the reference walks its two loaders (`pair_plan`: mode "zip" = DANN, "cycle" = DSAN).  `record` is two launches:
    the source batch with its labels, the target images (their labels go to the target loader's own buffer; neither tree reads
    them).  A pass of a loader is numbered epoch * (len(self) + 1) + k, k counting the passes begun inside the epoch: that number
    seeds its permutation and is the `epoch` of its draws, so a run can be resumed at any epoch.
    Not reproduced: DSAN's re-insertion of the short remainder into a later batch picked by the host's
    random.choice (dsan_office/main.py:353-366)."""

    def __init__(self, src: DeviceLoader, tgt: DeviceLoader, mode="zip"):
        if not (isinstance(src, DeviceLoader) and isinstance(tgt, DeviceLoader)) or src is tgt:
            raise TypeError("PairLoader: src and tgt must be two DeviceLoaders")
        if src.images.out_shape != tgt.images.out_shape:
            raise ValueError("PairLoader: both loaders must produce images of one shape")
        self.src, self.tgt, self.mode = src, tgt, mode
        self._plan = pair_plan((len(src.images), src.batch_size, src.world), (len(tgt.images), tgt.batch_size, tgt.world), mode)
        self._stride = len(self._plan) + 1
        self.epoch, self._it, self._begun = 0, 0, False
        self.begin_epoch(0)

    def __len__(self):
        return len(self._plan)

    def iterations(self, epoch=0):
        """[(source rows, target rows)] of an epoch's iterations (the same in every epoch): host arithmetic only"""
        return [(a, b) for a, b, _, _ in self._plan]

    def begin_epoch(self, epoch):
        """Both loaders begin pass 0 of `epoch` (the host's only writes besides the passes "cycle" begins inside an epoch)."""
        epoch = int(epoch)
        if not 0 <= epoch < (1 << 31) // self._stride:
            raise ValueError("PairLoader.begin_epoch: epoch out of range")
        self.src.begin_epoch(epoch * self._stride)
        self.tgt.begin_epoch(epoch * self._stride)
        self.epoch, self._it, self._begun = epoch, 0, False
        self._passes = [0, 0]
        return self

    def next_batch_sizes(self):
        """(source rows, target rows) of the coming iteration, (0, 0) when the epoch is exhausted.  In mode "cycle" this is where a
        loader begins the new pass the coming iteration needs (once per iteration), in front of the launches that produce it."""
        if self._it >= len(self._plan):
            return 0, 0
        rows_s, rows_t, new_s, new_t = self._plan[self._it]
        if not self._begun:
            self._begun = True
            for k, (loader, new) in enumerate(((self.src, new_s), (self.tgt, new_t))):
                if new:
                    self._passes[k] += 1
                    loader.begin_epoch(self.epoch * self._stride + self._passes[k])
        return rows_s, rows_t

    def skip(self, rows_s, rows_t):
        """Host bookkeeping for an iteration a replayed graph produced (the device cursors moved by themselves)."""
        self.src.skip(rows_s)
        self.tgt.skip(rows_t)
        self._it, self._begun = self._it + 1, False

    def record(self, xs, ys, xt):
        """Enqueue one iteration's batches into the given tensors: two launches, each of which moves its loader's cursor on.  No
        synchronisation, no allocation, no host state: this is what a capture records."""
        if xt.shape[0] > self.tgt.batch_size:
            raise ValueError("PairLoader: the target batch is larger than the target loader's batch size")
        self.src.record(xs, ys)
        self.tgt.record(xt, self.tgt._y[:xt.shape[0]])

    def next_batch(self):
        """(xs, ys, xt) of the coming iteration filled eagerly into the loaders' own buffers; None when the epoch is exhausted."""
        rows_s, rows_t = self.next_batch_sizes()
        if rows_s == 0:
            return None
        xs, ys, xt = self.src._x[:rows_s], self.src._y[:rows_s], self.tgt._x[:rows_t]
        self.record(xs, ys, xt)
        self.skip(rows_s, rows_t)
        return xs, ys, xt

    def peek(self):
        """(xs, ys, xt) of full batches holding each loader's first batch of its current pass WITHOUT consuming anything: what
        `capture` wants as its example inputs."""
        xs, ys = self.src.peek()
        return xs, ys, self.tgt.peek()[0]

    def __iter__(self):
        if self._it >= len(self._plan):
            self.begin_epoch(self.epoch + 1)
        while True:
            batch = self.next_batch()
            if batch is None:
                return
            yield batch


def _captured_with(step, loader):
    return getattr(step, "_producer", None) is loader and step._graph is not None


def train_epoch_office(step, pair, epoch, epoch_index=None):
    """One epoch of the Office trees' training loop (dann_office/main.py:340-456, dsan_office/main.py:335-478) over `pair` (a
    PairLoader) through `step` (an OfficeTrainStep / DSANTrainStep): with the pair inside the step's graph an iteration is one
    replay (`step.next()`), otherwise the batches go through `step(xs, ys, xt)`.  With a schedule table attached (set_schedule)
    the step first seeks to row epoch_index * max(len(src), len(tgt)) (epoch_index: epochs since the table's start_epoch,
    default `epoch`): the reference computes num_iterations from the LONGER loader while `zip` stops at the shorter one
    (schedule.office_dann's row layout), so an epoch of "zip" uses only the first rows of its block.  Without a table the caller
    stages new_epoch / alpha / lambd itself (set_lambd), and every iteration runs with the values in force.  Returns the last
    iteration's outputs."""
    from .train_step import _CapturedStep
    pair.begin_epoch(epoch)
    if step._schedule is not None:
        step.seek((epoch if epoch_index is None else int(epoch_index)) * max(len(pair.src), len(pair.tgt)))
    outs = None
    if _captured_with(step, pair):
        for _ in range(len(pair)):
            outs = step.next()
    else:
        for xs, ys, xt in pair:
            outs = _CapturedStep.__call__(step, xs, ys, xt)
    return outs


def train_epoch(step, loader, epoch):
    """One epoch of the reference's training loop (cdf_alignment_admm/resnet-20-cifar-10/main.py:278-378) over `loader`: every
    batch through `step` (a TrainStep), the short last one included.  With the loader inside the step's graph
    (`step.set_producer(loader)` before `capture`) a batch is one replay.  Returns the last iteration's (logits, ce, trans_loss)."""
    loader.begin_epoch(epoch)
    outs = None
    if _captured_with(step, loader):
        for _ in range(len(loader)):
            outs = step.next()
    else:
        for x, y in loader:
            outs = step(x, y)
    return outs


def evaluate(eval_step, loader):
    """The reference's test() (main.py:405-441) over `loader` (an unshuffled, unaugmented DeviceLoader): every batch through
    `eval_step` (an EvalStep; begun here unless the caller already did, e.g. to capture it), one host read at the end.  Returns
    EvalStep.result(): (mean cross-entropy, Prec@1, Prec@5, n)."""
    own = eval_step._saved is None
    if own:
        eval_step.begin()
    try:
        loader.begin_epoch(0)
        if _captured_with(eval_step, loader):
            for _ in range(len(loader)):
                eval_step.next()
        else:
            for x, y in loader:
                eval_step(x, y)
        return eval_step.result()
    finally:
        if own:
            eval_step.end()
