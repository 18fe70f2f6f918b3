"""Float64 NumPy statement of the weight quantiser's statistics and backward, the stand-alone cdf's backward and the SGD step,
written from the reference's formulas (model/quantization.py:41-85, utils/optimizer.py:6-13,212-255, restated line by line in
oracle/alignq_oracle.c :149-202 and :371-398), not from the kernels.  Inputs are the float32 tensors the kernels see; every product
and sum here is float64, so the results serve as the exact value both the HIP kernels and the float32 C oracle are measured
against.  The forward given (m, s) is not restated: the C oracle's weight_quant_fwd is its bit-level specification."""
import numpy as np

SQRT_2PI = np.sqrt(2.0 * np.pi)


def _f64(a):
    return np.asarray(a, dtype=np.float64).reshape(-1)


def weight_stats64(w):
    """(mean, unbiased std) of all elements, two passes: torch.mean / torch.std of model/quantization.py:78"""
    w = _f64(w)
    n = w.size
    m = w.sum() / n
    d = w - m
    return m, np.sqrt((d * d).sum() / (n - 1))


def weight_quant_bwd64(g, w, m, s):
    """dW_i = g_i P_i - mean_j(g_j P_j) - z_i sum_j(g_j P_j z_j) / (n - 1),  P = 2 N(w; m, s),  z = (w - m) / s: the autograd of
    W_q (straight-through) through cdf(mean(W), std(W))(W)"""
    g, w, m, s = _f64(g), _f64(w), float(m), float(s)
    n = w.size
    z = (w - m) / s
    P = 2.0 / (s * SQRT_2PI) * np.exp(-0.5 * z * z)
    gp = g * P
    return gp - gp.sum() / n - z * (gp * z).sum() / (n - 1)


def cdf_bwd64(gc, gp, x, m, s, kc):
    """Backward of cdf(m, s, src)(x) = (c, pdf) with c = kc * Phi(z) + const, pdf = 2 N(x; m, s), z = (x - m) / s, for upstream
    gradients gc of c and gp of pdf (either may be None): returns dx and (dm, ds) (ops.CdfFn: kc = d c / d Phi)."""
    x, m, s = _f64(x), float(m), float(s)
    z = (x - m) / s
    phi = np.exp(-0.5 * z * z) / (s * SQRT_2PI)
    a = np.zeros_like(x) if gc is None else _f64(gc) * kc * phi          # gc dc/dx
    b = np.zeros_like(x) if gp is None else _f64(gp) * 2.0 * phi / s     # gp 2 phi_s / s
    dx = a - b * z
    return dx, np.array([-dx.sum(), (b * (z * z - 1.0) - a * z).sum()])


def sgd_step64(p, g, buf, lr, mom, damp, wd, nesterov, first):
    """d = g + wd p;  buf = d (first) | mom buf + (1 - damp) d;  dir = d + mom buf (nesterov) | buf | d (mom == 0);  p -= lr dir.
    The hyper-parameters enter as the float32 values the kernels receive.  Returns (p, dir, buf); buf is None when mom == 0."""
    p, g = _f64(p), _f64(g)
    lr, mom, damp, wd = (float(np.float32(v)) for v in (lr, mom, damp, wd))
    d = g + wd * p if wd != 0.0 else g.copy()
    dirn, b = d, None
    if mom != 0.0:
        b = d.copy() if first else mom * _f64(buf) + (1.0 - damp) * d
        dirn = d + mom * b if nesterov else b
    return p - lr * dirn, dirn, b


def sgd_grad_approx64(dirn, w_cdf, w_pdf, bitW, lam, lam2, a=None):
    """p.grad of a tensor in `idx`: dir * sigmoid_d(transform(w_cdf)) * w_pdf with transform(c) = (((c + 0.5)(2^bitW - 1)) % 1) lam2 2
    and sigmoid_d(t) = sigmoid(t)(1 - sigmoid(t)) lam.  `a` (optional) replaces (c + 0.5)(2^bitW - 1): the float32 value a
    float32 evaluation takes the discontinuous `% 1` of."""
    nlev = float((1 << int(bitW)) - 1)
    a = (_f64(w_cdf) + 0.5) * nlev if a is None else _f64(a)
    fr = a - np.floor(a)
    sg = 1.0 / (1.0 + np.exp(-(fr * float(lam2) * 2.0)))
    return _f64(dirn) * (sg * (1.0 - sg) * float(lam)) * _f64(w_pdf)
