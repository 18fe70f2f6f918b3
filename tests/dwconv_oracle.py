"""The depthwise 3x3 convolution (padding 1, stride 1 or 2) and its two gradients in NumPy, as include/alignq.h states them.

Layouts are PyTorch's logical ones: x, dx [B, C, H, W]; y, dy [B, C, Ho, Wo]; w, dw [C, 3, 3] (a [C, 1, 3, 3] filter is reshaped);
Ho = (H - 1) // s + 1.  The float32 forward and data gradient reproduce the kernels' arithmetic bit for bit: the accumulator starts
at +0, taps run in row-major (ky, kx) order, every product and every sum is rounded to float32, a tap in the padding is skipped
(which, from a +0 start, equals adding +0: the accumulator can never be -0).  All three operations also exist in float64, and the
magnitude sums that the error bounds of the tests are stated in."""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    """Higham's gamma_n for float32: the relative error bound of n chained roundings."""
    return n * U / (1.0 - n * U)


def out_size(n, s):
    return (n - 1) // s + 1


def _w3(w):
    w = np.asarray(w)
    return w.reshape(w.shape[0], 3, 3)


def _taps(H, W, s):
    """For every tap: (ky, kx, output rows, output cols, input rows, input cols) of the (output, input) pixel pairs it joins."""
    Ho, Wo = out_size(H, s), out_size(W, s)
    for ky in range(3):
        ho = np.array([o for o in range(Ho) if 0 <= o * s + ky - 1 < H], dtype=np.int64)
        for kx in range(3):
            wo = np.array([o for o in range(Wo) if 0 <= o * s + kx - 1 < W], dtype=np.int64)
            yield ky, kx, ho, wo, ho * s + ky - 1, wo * s + kx - 1


def _fwd(x, w, s, dt, absolute=False):
    x, w = np.asarray(x).astype(dt), _w3(w).astype(dt)
    if absolute:
        x, w = np.abs(x), np.abs(w)
    B, C, H, W = x.shape
    y = np.zeros((B, C, out_size(H, s), out_size(W, s)), dt)
    for ky, kx, ho, wo, hi, wi in _taps(H, W, s):
        if len(ho) and len(wo):
            prod = (x[:, :, hi[:, None], wi[None, :]] * w[None, :, ky, kx, None, None]).astype(dt)
            y[:, :, ho[:, None], wo[None, :]] = (y[:, :, ho[:, None], wo[None, :]] + prod).astype(dt)
    return y


def _dgrad(dy, w, s, H, W, dt, absolute=False):
    dy, w = np.asarray(dy).astype(dt), _w3(w).astype(dt)
    if absolute:
        dy, w = np.abs(dy), np.abs(w)
    B, C = dy.shape[:2]
    dx = np.zeros((B, C, H, W), dt)
    # the input pixel (hi, wi) meets tap (ky, kx) of output (ho, wo) with hi = ho * s + ky - 1, i.e. hh = hi + 1 - ky = ho * s:
    # per input pixel the taps are visited in row-major (ky, kx) order, as in the kernel
    for ky, kx, ho, wo, hi, wi in _taps(H, W, s):
        if len(ho) and len(wo):
            prod = (dy[:, :, ho[:, None], wo[None, :]] * w[None, :, ky, kx, None, None]).astype(dt)
            dx[:, :, hi[:, None], wi[None, :]] = (dx[:, :, hi[:, None], wi[None, :]] + prod).astype(dt)
    return dx


def _wgrad(x, dy, s, dt, absolute=False):
    x, dy = np.asarray(x).astype(dt), np.asarray(dy).astype(dt)
    if absolute:
        x, dy = np.abs(x), np.abs(dy)
    B, C, H, W = x.shape
    dw = np.zeros((C, 3, 3), dt)
    for ky, kx, ho, wo, hi, wi in _taps(H, W, s):
        if len(ho) and len(wo):
            dw[:, ky, kx] = (x[:, :, hi[:, None], wi[None, :]] * dy[:, :, ho[:, None], wo[None, :]]).sum(axis=(0, 2, 3))
    return dw


def fwd32(x, w, s):
    return _fwd(x, w, s, np.float32)


def dgrad32(dy, w, s, H, W):
    return _dgrad(dy, w, s, H, W, np.float32)


def fwd64(x, w, s):
    return _fwd(x, w, s, np.float64)


def dgrad64(dy, w, s, H, W):
    return _dgrad(dy, w, s, H, W, np.float64)


def wgrad64(x, dy, s):
    return _wgrad(x, dy, s, np.float64)


def fwd_mag(x, w, s):
    """sum |x * w| per output element, float64"""
    return _fwd(x, w, s, np.float64, True)


def dgrad_mag(dy, w, s, H, W):
    """sum |dy * w| per input element, float64"""
    return _dgrad(dy, w, s, H, W, np.float64, True)


def wgrad_mag(x, dy, s):
    """sum |x * dy| per filter element, float64"""
    return _wgrad(x, dy, s, np.float64, True)


def fwd_bound(x, w, s):
    """|y32 - y64| <= gamma_10 * sum |x * w|: one rounding per product and at most nine additions."""
    return gamma(10) * fwd_mag(x, w, s)


def dgrad_bound(dy, w, s, H, W):
    return gamma(10) * dgrad_mag(dy, w, s, H, W)


def wgrad_bound(x, dy, s):
    """|dw32 - dw64| <= gamma_{N+1} * sum |x * dy|, N = B * Ho * Wo: holds for ANY summation order."""
    B, _, Ho, Wo = np.asarray(dy).shape
    return gamma(B * Ho * Wo + 1) * wgrad_mag(x, dy, s)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
