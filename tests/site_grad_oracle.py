"""Float64 restatement of the ADMM site's backward, and the scale its correlation term is checked at (no GPU).

The site (include/alignq.h, "fused ADMM site") is, for x [B,F]:

    t = r * erf(x / sqrt 2)                      (= act_range * (2 Phi(x) - 1), the pre-round transform)
    corr(v) = Vh Vh^T / F,  Vh = (v - mean_b v) / (std_b v + eps)        (std unbiased, over the batch)
    D = corr(t) - corr(x)
    dx = d/dx [ sum(dD o D) + sum(g o x_q) ],   d x_q / d x = d t / d x  (straight-through rounding)

`ref_dx` is exactly that, by torch autograd in float64; dD is NOT assumed symmetric.  `formula_dx` is the same gradient
written out term by term (the form the kernels and oracle/alignq_oracle.c evaluate), with switches that each break it in
one way: the CPU test proves the two agree, and that every defect is far outside the bar at the inputs the GPU tests use.

The scale.  Per column f, the correlation gradient is a difference of terms

    dx_bf = jac_bf * rho_f * (dVh_bf - mean_b dVh_f - vh_bf * proj_f),   dVh = (dD + dD^T) Vh / F,
    proj_f = sum_b dVh_bf vh_bf / (B - 1) * (std + eps)/std

for v = t (jac = dt/dx, sign +) and for v = x (jac = 1, sign -), rho = 1 / (std + eps).  |Vh[:, f]|_2 = sqrt(B - 1), so each
term is at most about max|dD| * 2 sqrt(B) / F * rho_f * jac in magnitude:

    term_f = max|dD| * 2 sqrt(B) / F * max(rho_x_f, rho_t_f * max_b jac_bf)

is the size of what cancels (tests/test_gpu_parity.py::test_corr_vs_oracle_shapes uses the x half of it).  The kernels carry
16 mantissa bits on the operands of S * Vh (split bf16, hi + lo), an error of about 2^-16 * term; the bar on a
pure-correlation dx (g = None) is

    |dx - ref|_bf <= BAR * term_f,   BAR = 2^-15.

Columns the backward's operands cannot hold to that.  The statistics (mean_f, rho_f: `stats`, include/alignq.h) come from the
FORWARD, which forms t with the project's table-driven ALIGNQ-ERF32; every backward kernel re-forms t from x with the
rational erf of alignq_amd/csrc/alignq_math.h (act_transform / act_transform_rcp: "the rational form's own error is 1.5e-7",
on erf, so r * 1.5e-7 on t) and standardises it with those stored fp32 statistics.  A standardised operand therefore carries
an absolute error of up to

    delta_t_f = rho_t_f * (r * 1.5e-7 + 2 u max_b |t_bf|)      (the transform; one fp32 rounding of t and one of the mean)
    delta_x_f = rho_x_f * u max_b |x_bf|                       (x is exact: the rounding of the stored mean)      u = 2^-24

and - samples that nearly coincide see nearly the SAME error - not a random one.  Pushed through the three terms with all
signs against us: dVh_bf = sum_b' S_bb' vh_b'f / F moves by at most max|S| B delta / F = sqrt(B)/2 * delta in units of
term_f / (rho jac), its mean by no more, and vh * proj by at most 2 delta (delta * proj + vh * delta proj, |proj| <= 1 in
those units): (sqrt(B) + 2) * delta * term_f in all.  With samples of O(1) spread rho is about 1 and this is a tenth of BAR
or less; it passes BAR where rho_t_f > 100 / (sqrt(B) + 2), a column whose transformed samples all lie within a few percent
of each other - among thousands of columns of B = 2 samples there are such columns (two draws 1e-5 apart: rho 1e5; the
analytic gradient there is still exactly zero, but only for operands that are exactly +-1/sqrt 2).  The per-column bar is

    |dx - ref|_bf <= max(BAR, (sqrt(B) + 2) * max(delta_t_f, delta_x_f)) * term_f          (`col_bar`)

which IS BAR * term_f on every well-conditioned column; the second member is derived from the operand accuracy the source
states, not from what the kernels were seen to give (measured: tests/test_gpu_site_corr_grad.py prints both).

Through the batch-norm.  With x = a_c z + b_c, a_c = gamma_c * invstd_c, b_c = beta_c - mean_c * a_c (training-mode batch-norm,
biased variance + bn_eps, channel c of column f) the remaining backward is LINEAR in dx (n = B * HW elements per channel,
zhat = (z - mean_c) * invstd_c):

    dbeta_c  = sum_{b, f in c} dx_bf
    dgamma_c = sum_{b, f in c} dx_bf * zhat_bf
    dz_bf    = a_c * (dx_bf - dbeta_c / n - zhat_bf * dgamma_c / n)

so an error of at most e_f = BAR * term_f in every dx_bf becomes at most (sum of |coefficient| * e)

    bar(dbeta_c)  = B * sum_{f in c} e_f
    bar(dgamma_c) = sum_{f in c} e_f * sum_b |zhat_bf|
    bar(dz_bf)    = |a_c| * (e_f + bar(dbeta_c) / n + |zhat_bf| * bar(dgamma_c) / n)

(`bn_bars`).  The masked upstream gradient dres is a copy and is compared for equality.
"""
import math

import numpy as np
import torch

BAR = 2.0 ** -15
SQRT2 = math.sqrt(2.0)
JAC0 = 2.0 / math.sqrt(2.0 * math.pi)        # dt/dx = r * JAC0 * exp(-x^2 / 2)

DEFECTS = ("corr_dropped", "xx_sign_flipped", "mean_kept", "proj_dropped", "dD_not_symmetrised", "jac_dropped")


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _corr(v, eps):
    vh = (v - v.mean(0, keepdim=True)) / (v.std(0, unbiased=True, keepdim=True) + eps)
    return vh @ vh.T / v.shape[1]


def _site_objective(x, dD, g, r, eps, t_at=None):
    t = r * torch.erf(x / SQRT2)
    if t_at is not None:                     # same graph, values of t replaced (see ref_dx)
        t = t + (t_at - t).detach()
    obj = (dD * (_corr(t, eps) - _corr(x, eps))).sum()
    if g is not None:
        obj = obj + (g * t).sum()            # d x_q / d x = d t / d x
    return obj


def ref_dx(x, dD, g, r, eps, t_at=None):
    """dx [B,F] (float64) of sum(dD o D) + sum(g o x_q) by autograd; g may be None.
    t_at (or None): take the derivative AT these values of t (the fp32 transform the project specifies, ALIGNQ-ERF32, which the
    kernels and the C oracle share bit for bit) instead of at the float64 r * erf(x / sqrt 2): the correlation of t is
    ill-conditioned in t where a column's samples nearly coincide, and a caller that compares two users of the SAME fp32 t
    need not pay for that; dt/dx stays the analytic one."""
    B = x.shape[0]
    xt = _t64(np.asarray(x).reshape(B, -1)).requires_grad_(True)
    obj = _site_objective(xt, _t64(dD), None if g is None else _t64(np.asarray(g).reshape(B, -1)), float(r), float(eps),
                          None if t_at is None else _t64(np.asarray(t_at).reshape(B, -1)))
    (dx,) = torch.autograd.grad(obj, xt)
    return dx.numpy()


def jac(x, r):
    x = np.asarray(x, np.float64)
    return float(r) * JAC0 * np.exp(-0.5 * x * x)


def _stats(v, eps):
    mu = v.mean(0)
    sd = v.std(0, ddof=1)
    return mu, sd, 1.0 / (sd + eps)


def term(x, dD, r, eps):
    """term_f [F]: the per-column size of the cancelling terms of the correlation gradient (module docstring)."""
    x = np.asarray(x, np.float64).reshape(x.shape[0], -1)
    B, F = x.shape
    t = float(r) * torch.erf(_t64(x) / SQRT2).numpy()
    rho_x, rho_t = _stats(x, eps)[2], _stats(t, eps)[2]
    return np.abs(np.asarray(dD)).max() * 2.0 * math.sqrt(B) / F * np.maximum(rho_x, rho_t * jac(x, r).max(0))


ERF_RATIONAL_ERR = 1.5e-7      # alignq_amd/csrc/alignq_math.h, act_transform_rcp: "the rational form's own error is 1.5e-7"


def col_bar(x, r, eps):
    """per-column bar in units of term_f: max(BAR, (sqrt(B) + 2) max(delta_t, delta_x)) (module docstring); BAR on every
    well-conditioned column"""
    x = np.asarray(x, np.float64).reshape(x.shape[0], -1)
    B, u = x.shape[0], 2.0 ** -24
    t = float(r) * torch.erf(_t64(x) / SQRT2).numpy()
    d_t = _stats(t, eps)[2] * (float(r) * ERF_RATIONAL_ERR + 2.0 * u * np.abs(t).max(0))
    d_x = _stats(x, eps)[2] * u * np.abs(x).max(0)
    return np.maximum(BAR, (math.sqrt(B) + 2.0) * np.maximum(d_t, d_x))


def _branch(S, v, eps, defect):
    B, F = v.shape
    mu, sd, rho = _stats(v, eps)
    vh = (v - mu) * rho
    dvh = S @ vh / F
    mean = 0.0 if defect == "mean_kept" else dvh.mean(0)
    proj = 0.0 if defect == "proj_dropped" else (dvh * vh).sum(0) / (B - 1) / (sd * rho)
    return rho * (dvh - mean - vh * proj)


def formula_dx(x, dD, g, r, eps, defect=None):
    """The same gradient in closed form (float64 numpy); `defect` (one of DEFECTS) breaks it in one named way."""
    assert defect is None or defect in DEFECTS
    x = np.asarray(x, np.float64).reshape(x.shape[0], -1)
    dD = np.asarray(dD, np.float64)
    j = jac(x, r)
    dx = np.zeros_like(x) if g is None else np.asarray(g, np.float64).reshape(x.shape) * j
    if defect == "corr_dropped":
        return dx
    S = 2.0 * dD if defect == "dD_not_symmetrised" else dD + dD.T
    t = float(r) * torch.erf(_t64(x) / SQRT2).numpy()
    dt = _branch(S, t, eps, defect)
    dxx = _branch(S, x, eps, defect)
    return dx + (dt if defect == "jac_dropped" else dt * j) + (dxx if defect == "xx_sign_flipped" else -dxx)


def worst(dx, ref, term_f, bar_f=None):
    """max over elements of |dx - ref| / term_f: the figure the bar BAR is set on (bar_f: in units of col_bar instead)."""
    B = ref.shape[0]
    scale = term_f if bar_f is None else term_f * bar_f
    return float((np.abs(np.asarray(dx, np.float64).reshape(B, -1) - ref) / scale[None, :]).max())


# ---------------------------------------------------------------------------------------------- batch-norm folded form
def channel_of(F, C, nhwc):
    f = np.arange(F)
    return f % C if nhwc else f // (F // C)


def ref_bn(z, dD, g, gamma, beta, C, nhwc, r, eps, bn_eps=1e-5, mask=None, x_at=None):
    """The site behind a training-mode batch-norm: z [B,F] in memory order (channel = f % C if nhwc else f // HW),
    x = a_c z + b_c with (a, b) from the batch statistics of z, objective sum(dD o D(x)) + sum(g o mask o x_q(x)).
    mask (or None): the ReLU mask [y > 0] of the stored y = relu(x_q [+ residual]); the residual's gradient is dres = g o mask.
    x_at (or None): evaluate the site's derivative AT these values of x (the fp32 x the kernels form with one fma from the
    fp32 (a, b)) instead of at the float64 a_c z + b_c; the graph through the batch-norm is unchanged.
    Returns dict(dz, dgamma, dbeta, dres, dx, x, zhat, a), float64; dx = gradient w.r.t. the batch-norm output."""
    B = z.shape[0]
    zt = _t64(np.asarray(z).reshape(B, -1)).requires_grad_(True)
    F = zt.shape[1]
    ch = torch.from_numpy(channel_of(F, C, nhwc))
    gam, bet = _t64(gamma).requires_grad_(True), _t64(beta).requires_grad_(True)
    n = B * (F // C)
    mean = torch.zeros(C, dtype=torch.float64).index_add_(0, ch, zt.sum(0)) / n
    var = torch.zeros(C, dtype=torch.float64).index_add_(0, ch, ((zt - mean[ch]) ** 2).sum(0)) / n
    invstd = 1.0 / torch.sqrt(var + bn_eps)
    zhat = (zt - mean[ch]) * invstd[ch]
    x = zhat * gam[ch] + bet[ch]
    if x_at is not None:
        x = x + (_t64(np.asarray(x_at).reshape(B, -1)) - x).detach()
    x.retain_grad()
    gm = None
    if g is not None:
        gm = _t64(np.asarray(g).reshape(B, -1))
        if mask is not None:
            gm = gm * torch.from_numpy(np.asarray(mask).reshape(B, -1).astype(np.float64))
    _site_objective(x, _t64(dD), gm, float(r), float(eps)).backward()
    return dict(dz=zt.grad.numpy(), dgamma=gam.grad.numpy(), dbeta=bet.grad.numpy(), dres=None if gm is None else gm.numpy(),
                dx=x.grad.numpy(), x=x.detach().numpy(), zhat=zhat.detach().numpy(), a=(gam * invstd).detach().numpy())


def bn_bars(term_f, zhat, a, C, nhwc, bar=BAR):
    """(bar_dz [B,F], bar_dgamma [C], bar_dbeta [C]) from the per-column bar on dx (derivation: module docstring); bar: a
    scalar or col_bar's per-column array, in units of term_f."""
    B, F = zhat.shape
    ch = channel_of(F, C, nhwc)
    n = B * (F // C)
    e = bar * term_f
    bar_db = B * np.bincount(ch, weights=e, minlength=C)
    bar_dg = np.bincount(ch, weights=e * np.abs(zhat).sum(0), minlength=C)
    bar_dz = np.abs(a)[ch][None, :] * (e[None, :] + bar_db[ch][None, :] / n + np.abs(zhat) * bar_dg[ch][None, :] / n)
    return bar_dz, bar_dg, bar_db


# ---------------------------------------------------------------------------------------------- the matrix and its inputs
# One row per launch form of the pair backward (the smallest shapes that select it; the dispatch is geom(), bwd_tile_features(),
# bwd_vec(), launch_bwd / launch_bwd4 / launch_bwd1 of alignq_amd/csrc).  (form, B, F)
PLAIN = (
    # B <= 32, launch_bwd1: F not a multiple of 4, aligned, more 128-feature tiles than the 1024-workgroup cap
    [("bwd1", B, F) for B in (2, 5, 28, 32) for F in (70, 4096, 131072 + 384)]
    # 32 < B <= 64, site_bwd_kernel<2, true>: ragged, aligned, more 64-feature tiles than the 2048-workgroup grid
    + [("bwd2", B, F) for B in (33, 48, 64) for F in (70, 4096, 131072 + 64)]
    # 64 < B <= 128: site_bwd4_kernel<32> (F < 16384), <64> (F >= 16384), the looped <64> form (B = 128, 513 tiles over 256
    # workgroups: trip counts 3 and 2), and the scalar-access path (F % 4 != 0)
    + [("bwd4", B, F) for B in (65, 100, 128) for F in (96, 4096, 8192, 16384, 32832, 4098)]
    # B > 128: the pair kernels of the blocked Gram: corrl_bwd_kernel<2, 4, true> (up to 256 rows), <4, 4, true> (up to 512: 300),
    # <4, 8, true> (above)
    + [("large", 130, 70), ("large", 192, 384), ("large", 300, 72), ("large", 513, 72)]
)
# folded batch-norm forms, (B, C, H): channel count C, H x H pixels
BN4 = ((128, 16, 16), (100, 32, 16), (128, 64, 8))          # 64 < B <= 128: site_bwd4_kernel<TF, true, true>
# the same kernels at the channel counts and partial forms the fold admits beyond those three (bn_shape_ok: channels-last at any
# power-of-two C in [4, 256] with F % 64 == 0, NCHW at any C with HW % 64 == 0), (B, C, HW) with HW not a square; what each row selects:
# tests/test_gpu_bn_forms.py.  Lists of their own: the BN4 test asserts filler slots that the large rows do not have.
BN4_CL = ((65, 4, 16), (128, 8, 8), (100, 64, 1), (128, 256, 1), (65, 128, 33), (100, 4, 1040), (128, 256, 64), (128, 256, 129))
BN4_NCHW = ((65, 1, 64), (128, 3, 128), (100, 5, 832), (128, 3, 11008))
BN4_HARD = {1: (128, 8, 8), 0: (128, 3, 128)}               # per layout: the row that also runs with a channel of mean 30, std 0.5
BN1 = ((6, 64, 4), (28, 256, 2))                            # B <= 32: the site1 groups kernels (channels-last)
AB1 = (28, 64, 4)                                           # alignq_site_bwd_apply_ab[_relu]


def plain_eps(B):
    """The Office tree's eps = 1e-5 on the rows with B % 4 == 0, the ADMM tree's 0 elsewhere.  B = 2 runs at eps = 0, where both
    standardised values of a column are +-1/sqrt 2 whatever x is; with eps > 0 a column whose two samples nearly coincide makes
    the result depend on the last bit of the fp32 transform t, which is conditioning of the expression, not arithmetic."""
    return 1e-5 if B % 4 == 0 else 0.0


def plain_inputs(B, F):
    """x [B,F] (std 1.1, mean 0.15: |x| reaches the flat part of erf) and a NON-symmetric standard-normal dD."""
    rng = np.random.default_rng(100003 * B + F)
    x = (rng.standard_normal((B, F)) * 1.1 + 0.15).astype(np.float32)
    dD = rng.standard_normal((B, B)).astype(np.float32)
    return x, dD


def bn_inputs(B, C, H, seed=0, HW=None):
    """z [B, C*H*H] (C*HW where HW is given: H only seeds then) in memory order, gamma, beta, a non-symmetric dD."""
    rng = np.random.default_rng(1009 * B + 31 * C + H + seed)
    F = C * (H * H if HW is None else HW)
    z = (rng.standard_normal((B, F)) * 1.7 + 0.3).astype(np.float32)
    gamma = (rng.random(C) + 0.5).astype(np.float32)
    beta = (rng.standard_normal(C) * 0.2).astype(np.float32)
    dD = rng.standard_normal((B, B)).astype(np.float32)
    return z, gamma, beta, dD


def admm_params(B, dim, seed):
    """alterD, gamma [dim,dim] for the forms that rebuild dD from (D, alterD, gamma, scal): |alterD| in [0.3, 1] with random
    signs keeps every D - alterD (|D| is a few 1e-2 at most) far from 0, so sign(D - alterD) in the loss gradient
    rho/2 (D - alterD)/(n rms) + gamma sign(D - alterD)/n is the same for the kernel's D and the oracle's (they differ by 1e-6)."""
    rng = np.random.default_rng(seed)
    A = ((rng.random((dim, dim)) * 0.7 + 0.3) * rng.choice([-1.0, 1.0], (dim, dim))).astype(np.float32)
    G = rng.random((dim, dim)).astype(np.float32)
    return A, G
