"""Drop-in for utils/mmd.py of both DSAN trees (cdf_alignment_admm/dsan_office, cdf_alignment/dsan_office; identical apart from
the device): `lmmd` with the reference's signature and its [1]-shaped result, computed by alignq_lmmd_fwd / _bwd
(csrc/lmmd_kernels.hip) on the device.  The reference pulls the labels and target probabilities to NumPy every call to build
the class weights (utils/Weight.py:10-54, mmd.py:24-29); here the weights are formed on chip, so a step that calls `lmmd` has
no host synchronisation and can be captured into a graph.  Nothing flows back to `s_label` or `t_label` (the reference reads
them through `.data` / NumPy)."""
from __future__ import annotations

import torch

from . import _lib as L


def _check_args(source, target, s_label, t_label, kernel_num, fix_sigma):
    if source.dim() != 2 or target.dim() != 2 or source.shape[1] != target.shape[1]:
        raise ValueError(f"lmmd: source / target must be [B, D] of one width, got {tuple(source.shape)} and {tuple(target.shape)}")
    if source.shape[0] != target.shape[0]:
        # the reference's weights are B x B from the source batch and are multiplied with the B x B target block
        raise ValueError(f"lmmd: source and target batches must have equal size ({source.shape[0]} != {target.shape[0]})")
    B = source.shape[0]
    if s_label.shape != (B,) or t_label.dim() != 2 or t_label.shape[0] != B:
        raise ValueError(f"lmmd: s_label must be [{B}] and t_label [{B}, C], got {tuple(s_label.shape)} and "
                         f"{tuple(t_label.shape)}")
    if fix_sigma is not None and fix_sigma < 0:
        raise ValueError("lmmd: fix_sigma must be positive (or None / 0 for the data bandwidth)")
    if int(kernel_num) < 1:
        raise ValueError("lmmd: kernel_num must be >= 1")


def _lmmd_fwd(ctx, xs, xt, s_label, t_label, kernel_mul, kernel_num, fix_sigma):
    lib = L.load()
    B, D = xs.shape
    labels = s_label.to(device=xs.device, dtype=torch.int64).contiguous()
    p = L.dev_f32(t_label.detach(), "t_label")
    ws = torch.empty(max(int(lib.alignq_lmmd_ws_bytes(B, D)), 1), dtype=torch.uint8, device=xs.device)
    loss = torch.empty(1, dtype=torch.float32, device=xs.device)
    L.check(lib.alignq_lmmd_fwd(L.ptr(xs), L.ptr(xt), L.ptr(labels), L.ptr(p), B, D, p.shape[1], float(kernel_mul),
                                int(kernel_num), float(fix_sigma or 0.0), L.ptr(loss), L.ptr(ws), L.stream_ptr()),
            "alignq_lmmd_fwd")
    ctx.ws, ctx.B, ctx.D = ws, B, D
    return loss


def _lmmd_bwd(ctx, g, xs, xt, dxs, dxt):
    g = L.dev_f32(g, "grad").reshape(-1)
    L.check(L.load().alignq_lmmd_bwd(L.ptr(g), L.ptr(xs), L.ptr(xt), L.ptr(ctx.ws), ctx.B, ctx.D, L.ptr(dxs), L.ptr(dxt),
                                     L.stream_ptr()), "alignq_lmmd_bwd")


class LMMDFn(torch.autograd.Function):
    """loss [1] of (source [B, D], target [B, D]); gradients for both."""

    @staticmethod
    def forward(ctx, source, target, s_label, t_label, kernel_mul, kernel_num, fix_sigma):
        xs, xt = L.dev_f32(source, "source"), L.dev_f32(target, "target")
        loss = _lmmd_fwd(ctx, xs, xt, s_label, t_label, kernel_mul, kernel_num, fix_sigma)
        ctx.save_for_backward(xs, xt)
        return loss

    @staticmethod
    def backward(ctx, g):
        xs, xt = ctx.saved_tensors
        dxs, dxt = torch.empty_like(xs), torch.empty_like(xt)
        _lmmd_bwd(ctx, g, xs, xt, dxs, dxt)
        return dxs, dxt, None, None, None, None, None


class LMMDPairFn(torch.autograd.Function):
    """The same loss over the two halves of ONE [2B, D] tensor (DSAN.forward_dual: the source rows, then the target rows):
    the kernels read both halves in place and the backward writes one [2B, D] gradient, without slicing nodes."""

    @staticmethod
    def forward(ctx, total, s_label, t_label, kernel_mul, kernel_num, fix_sigma):
        x = L.dev_f32(total, "features")
        B = x.shape[0] // 2
        loss = _lmmd_fwd(ctx, x[:B], x[B:], s_label, t_label, kernel_mul, kernel_num, fix_sigma)
        ctx.save_for_backward(x)
        return loss

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        B = ctx.B
        _lmmd_bwd(ctx, g, x[:B], x[B:], dx[:B], dx[B:])
        return dx, None, None, None, None, None


def lmmd(source, target, s_label, t_label, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """utils/mmd.py:24-41: the local MMD between `source` and `target` [B, D] under the class weights of the source labels
    `s_label` [B] and the target class probabilities `t_label` [B, C]; returns a [1] tensor.  Labels outside [0, C) belong to
    no class.  fix_sigma None (or 0): the bandwidth comes from the data, detached, as in the reference."""
    _check_args(source, target, s_label, t_label, kernel_num, fix_sigma)
    return LMMDFn.apply(source, target, s_label, t_label, kernel_mul, kernel_num, fix_sigma)


def lmmd_pair(total, s_label, t_label, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """`lmmd(total[:B], total[B:], ...)` for a [2B, D] tensor that holds the source rows, then the target rows."""
    if total.dim() != 2 or total.shape[0] % 2:
        raise ValueError(f"lmmd_pair: expected [2B, D] features, got {tuple(total.shape)}")
    B = total.shape[0] // 2
    _check_args(total[:B], total[B:], s_label, t_label, kernel_num, fix_sigma)
    return LMMDPairFn.apply(total, s_label, t_label, kernel_mul, kernel_num, fix_sigma)
