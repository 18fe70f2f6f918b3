"""Scalar hyper-parameters of a captured training step in DEVICE memory, so that one HIP graph follows a schedule.

The reference changes its scalars all the time: MultiStepLR steps the CIFAR trees' learning rate per epoch
(cdf_alignment_admm/resnet-20-cifar-10/main.py:97,126), the Office trees build a new SGD with new group rates every epoch
(dann_office/main.py:321-328, dsan_office/main.py:316-329) and recompute DANN's gradient-reversal coefficient (dann_office/
main.py:346-348) and DSAN's LMMD weight (dsan_office/main.py:381-382,410) every iteration.  A graph bakes kernel ARGUMENTS in; what
a kernel reads through a pointer it reads at replay time.  `HyperBlock` is that memory: one float32 row

    [lr_0 ... lr_{G-1}, alpha, coef, fresh]

whose slots the `_dev` SGD launchers (include/alignq.h), ReverseLayerF and the DSAN loss read.  The row is written either by the
host (`HyperBlock.set`: one small non-blocking copy) or, with a table, by `alignq_hyper_advance` as the first node of the graph:
row n of the table in iteration n, no host write at all.

The table builders form every value in Python floats exactly as the reference's lines do and round ONCE to float32 - the
rounding a by-value kernel argument gets - so a table-driven run computes the bits of a run that passes the same numbers by value."""
from __future__ import annotations

import bisect
import math

import numpy as np
import torch

from . import _lib as L
from . import config

N_EXTRA = 3            # alpha, coef, fresh behind the group rates
MAX_COLS = 64          # alignq_hyper_advance: one workgroup of 64 threads copies a row
_RING = 8              # staging rows in flight before `set` has to wait for the oldest copy


class HyperBlock:
    """The device row and its pinned host staging.  `lr(g)`, `alpha`, `coef` and `fresh` are 1-element views of the row (fixed
    addresses: what the captured kernels read)."""

    def __init__(self, device, n_groups):
        n_groups = int(n_groups)
        if n_groups < 1 or n_groups + N_EXTRA > MAX_COLS:
            raise ValueError(f"HyperBlock: 1 <= n_groups <= {MAX_COLS - N_EXTRA}")
        self.device = torch.device(device)
        self.n_groups, self.cols = n_groups, n_groups + N_EXTRA
        self.row = torch.zeros(self.cols, dtype=torch.float32, device=self.device)
        self.alpha, self.coef, self.fresh = (self.row[n_groups + j:n_groups + j + 1] for j in range(N_EXTRA))
        # the host's view of the row (float32: rounded once, as a by-value kernel argument is).  An asynchronous copy reads its
        # source when the device gets to it, so each staged row has a pinned buffer of its own until its copy has run
        pin = self.device.type == "cuda"
        self.host = torch.zeros(self.cols, dtype=torch.float32)
        self._ring = [torch.zeros(self.cols, dtype=torch.float32, pin_memory=pin) for _ in range(_RING)]
        self._events = [None] * _RING
        self._next = 0
        self._dirty = True          # the device row is not known to equal `host` (fresh block, or a table wrote it)
        self.copies = 0             # staged copies so far (tests: an unchanged row stages nothing)

    def lr(self, g):
        return self.row[g:g + 1]

    def values(self):
        """The host's mirror as a dict (what `set` staged last; a table-driven row is read with `read`)."""
        h, G = self.host.tolist(), self.n_groups
        return dict(lr=h[:G], alpha=h[G], coef=h[G + 1], fresh=h[G + 2])

    def set(self, lr=None, alpha=None, coef=None, fresh=None):
        """Stage the given slots (lr: one number for every group or one per group) for the work enqueued AFTER this call on the
        current stream: one non-blocking copy of the row, none when nothing changed.  Never inside a stream capture."""
        new, G = self.host.clone(), self.n_groups
        if lr is not None:
            lrs = [float(v) for v in lr] if isinstance(lr, (list, tuple)) else [float(lr)] * G
            if len(lrs) != G:
                raise ValueError(f"HyperBlock.set: {len(lrs)} rates for {G} parameter groups")
            new[:G] = torch.tensor(lrs, dtype=torch.float64).to(torch.float32)
        for j, v in enumerate((alpha, coef, fresh)):
            if v is not None:
                new[G + j] = torch.tensor(float(v), dtype=torch.float64).to(torch.float32)
        if not self._dirty and torch.equal(new.view(torch.int32), self.host.view(torch.int32)):
            return self
        self.host = new
        k = self._next
        self._next = (k + 1) % _RING
        if self._events[k] is not None:
            self._events[k].synchronize()       # (returns at once unless the host is _RING staged rows ahead of the device)
        self._ring[k].copy_(new)
        self.row.copy_(self._ring[k], non_blocking=True)
        if self.device.type == "cuda":
            self._events[k] = torch.cuda.Event()
            self._events[k].record()
        self._dirty = False
        self.copies += 1
        return self

    def invalidate(self):
        """The device row was written by someone else (alignq_hyper_advance): the next `set` stages whatever it is given."""
        self._dirty = True

    def read(self):
        """The DEVICE row as a dict: one host read (a synchronisation), for logs and tests."""
        h, G = self.row.cpu().tolist(), self.n_groups
        return dict(lr=h[:G], alpha=h[G], coef=h[G + 1], fresh=h[G + 2])


# ------------------------------------------------------------------------------------------------ the reference's formulas
def ramp(num_iters, num_epochs, num_iterations):
    """dann_office/main.py:347-348 (alpha) and dsan_office/main.py:381-382 (lambd): the same two lines.  train_step.dann_alpha and
    dsan_lambd are this function, so the tables and the by-hand path cannot drift apart."""
    p = float(num_iters) / num_epochs / num_iterations
    return 2. / (1. + np.exp(-10 * p) + 1e-6) - 1


def office_rate(lr, epoch, num_epochs):
    """LEARNING_RATE of dann_office/main.py:321 and dsan_office/main.py:316.  (As there, epoch 0 of a run of 10 epochs or fewer
    has no rate: the base is zero or negative and Python raises.)"""
    return lr / math.pow((1 + 10 * (epoch - 1) / num_epochs), 0.75)


def _table(rows):
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32).contiguous()


def multistep(lr, milestones, gamma, epochs, iters_per_epoch):
    """[epochs * iters_per_epoch, 4] rows (lr, 0, 0, fresh) of MultiStepLR as the CIFAR trees drive it (resnet-20-cifar-10/
    main.py:97,126: `scheduler.step(epoch)` in front of every epoch, i.e. lr * gamma ** (milestones <= epoch)).  `fresh` is 1 in
    row 0 only: the run starts with a new optimizer."""
    ms = sorted(int(m) for m in milestones)
    rows = []
    for epoch in range(int(epochs)):
        rate = lr * gamma ** bisect.bisect_right(ms, epoch)
        for i in range(int(iters_per_epoch)):
            rows.append([rate, 0.0, 0.0, 1.0 if (epoch == 0 and i == 0) else 0.0])
    return _table(rows)


def office_dann(lr, num_epochs, num_iterations, start_epoch=0):
    """[(num_epochs - start_epoch) * num_iterations, 6] rows (rate / 10, rate, rate, alpha, 0, fresh) of dann_office/main.py: the
    three parameter groups of :324-328 at LEARNING_RATE of :321, alpha of :346-348 with i counting from 1 (`enumerate(.., 1)`,
    :341-345), fresh = 1 where the reference has just built the epoch's SGD.  Epochs run over range(start_epoch, num_epochs)
    (:143)."""
    rows = []
    for epoch in range(int(start_epoch), int(num_epochs)):
        rate = office_rate(lr, epoch, num_epochs)
        for i in range(1, int(num_iterations) + 1):
            alpha = ramp(num_iterations * epoch + i, num_epochs, num_iterations)
            rows.append([rate / 10, rate, rate, alpha, 0.0, 1.0 if i == 1 else 0.0])
    return _table(rows)


def office_dsan(lr, num_epochs, num_iterations, param=None, start_epoch=0, bottle_neck=True):
    """[(num_epochs - start_epoch) * num_iterations, 6] rows (rate / 10, rate, rate, 0, coef, fresh) of dsan_office/main.py: the
    groups of :319-323 (feature_layers, bottle, cls_fc; without the bottleneck two groups, 5 columns), coef = args.param * lambd
    of :381-382,410 with i counting from 0 (:345-347).  param: args.param (default: config.args.param)."""
    param = config.args.param if param is None else param
    rows = []
    for epoch in range(int(start_epoch), int(num_epochs)):
        rate = office_rate(lr, epoch, num_epochs)
        for i in range(int(num_iterations)):
            lambd = ramp(num_iterations * epoch + i, num_epochs, num_iterations)
            rows.append([rate / 10] + [rate] * (2 if bottle_neck else 1) + [0.0, float(param * lambd), 1.0 if i == 0 else 0.0])
    return _table(rows)


class Schedule:
    """A table on the device with its cursor: `advance` launches alignq_hyper_advance (row min(cursor, rows - 1) into the block's
    row, cursor + 1) on the current stream; inside a capture that launch becomes a node of the graph."""

    def __init__(self, block, table):
        table = torch.as_tensor(table)
        if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] != block.cols:
            raise ValueError(f"schedule table: expected [rows >= 1, {block.cols}] (the block's row: {block.n_groups} rates, alpha, "
                             f"coef, fresh), got {tuple(table.shape)}")
        if table.dtype != torch.float32:
            raise TypeError("schedule table: float32 (build it with alignq_amd.schedule's builders: rounded once from Python floats)")
        self.block = block
        self.table = table.to(block.device).contiguous()
        self.rows, self.cols = int(table.shape[0]), int(table.shape[1])
        self.cursor = torch.zeros(1, dtype=torch.int32, device=block.device)

    def advance(self):
        L.check(L.load().alignq_hyper_advance(L.ptr(self.table), self.rows, self.cols, L.ptr(self.cursor), L.ptr(self.block.row),
                                              L.stream_ptr()), "alignq_hyper_advance")
        self.block.invalidate()

    def seek(self, i):
        self.cursor.fill_(int(i))

    def position(self):
        """The cursor (one host read): the number of iterations run since seek(0)."""
        return int(self.cursor.item())
