"""NumPy restatement of include/alignq_mobile.h (MobileNet-V2's folded evaluation sites), built from the pieces the other tests
trust: eval_inputs.ab_numpy for the coefficients, oracle/alignq_oracle.c (tests/oracle_c.py) for the quantiser - fed x through the
identity coefficients a = 1, b = 0, for which its fmaf(a, x, b) returns x itself, as tests/test_gpu_eval.py does -, and
tests/dwconv_oracle.py for the depthwise sum.  Tensors are channels-last in memory: [..., C] arrays, channel = last axis.

The clamps, stated once:
    relu(v)  = v > 0 ? v : +0
    relu6(v) = v > 0 ? (v < 6 ? v : 6) : +0            NaN and -0 give +0 (torch.nn.ReLU6 keeps both)"""
import os
import sys

import numpy as np

from tests import dwconv_oracle as D
from tests import oracle_c as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from eval_inputs import ab_numpy  # noqa: E402

ADMM, CDF = 0, 1
NONE, RELU, RELU6 = 0, 1, 2
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def clamp(v, mode):
    v = np.asarray(v, dtype=np.float32)
    if mode == NONE:
        return v
    with np.errstate(invalid="ignore"):
        pos = v > 0
        top = np.where(v < 6, v, F32(6.0)).astype(np.float32) if mode == RELU6 else v
    return np.where(pos, top, F32(0.0)).astype(np.float32)


def affine(z, gamma, beta, mean, var, eps):
    """x = (a_c * z) + b_c, every operation rounded to fp32 on its own; z [..., C]"""
    a, b = ab_numpy(gamma, beta, mean, var, eps)
    return ((a * z.astype(np.float32)).astype(np.float32) + b).astype(np.float32)


def quant(x, k, r, formula):
    """the quantiser of alignq_act_quant_fwd on x [..., C] (k == 32: none)"""
    if k == 32:
        return x
    C = x.shape[-1]
    x2 = np.ascontiguousarray(x, dtype=np.float32).reshape(1, -1)
    ident = np.stack([np.ones(C, np.float32), np.zeros(C, np.float32)])
    if formula == ADMM:
        xq = O.act_quant_fwd(x2, k, r, ADMM)[0]
    else:
        xq = O.act_quant_fwd(O.bn_apply(x2, C, 1, ident), k, r, CDF)[0]
    return np.asarray(xq, dtype=np.float32).reshape(x.shape)


def finish(xq, mode, residual=None):
    """clamp(xq [+ residual])"""
    v = xq if residual is None else (xq + residual).astype(np.float32)
    return clamp(v, mode)


def site(z, vecs, eps, k, r, formula, mode, residual=None):
    """alignq_site_eval_fwd; vecs = (gamma, beta, mean, var)"""
    return finish(quant(affine(z, *vecs, eps), k, r, formula), mode, residual)


def twin(zA, vecsA, epsA, kA, zB, vecsB, epsB, kB, modeB, r, formula):
    """alignq_site_eval_twin_fwd: q_A(..) + clamp_B(q_B(..))"""
    tmp = site(zB, vecsB, epsB, kB, r, formula, modeB)
    return site(zA, vecsA, epsA, kA, r, formula, NONE, residual=tmp)


def dw(x_nhwc, w, stride):
    """alignq_dwconv3x3_nhwc_fwd's sum on a channels-last array [B, H, W, C]; w (C, 1, 3, 3)"""
    y = D.fwd32(np.ascontiguousarray(x_nhwc.transpose(0, 3, 1, 2)), w, stride)
    return np.ascontiguousarray(y.transpose(0, 2, 3, 1))


def dw_site(x_nhwc, w, stride, vecs, eps, k, r, formula, mode):
    """alignq_dwconv3x3_site_eval_fwd"""
    return site(dw(x_nhwc, w, stride), vecs, eps, k, r, formula, mode)
