"""The site backward's CORRELATION gradient, d(corr(t,t) - corr(x,x))/dx, by value at its own scale, in every launch form.

The other site tests feed the ADMM loss's own dD (1e-3 and below) and compare dx at atol 1e-5: the whole correlation gradient
is smaller than that tolerance there, so a backward that wrote g * dt/dx and nothing else would pass them
(tests/test_site_grad_oracle_cpu.py pins that sentence).  Here there is NO upstream x_q gradient and dD is O(1): either an
explicit non-symmetric standard-normal dD (alignq_site_bwd through ops.SiteDFn / ops.SiteLargeFn) or, for the forms that
rebuild dD from (D, alterD, gamma, scal), the loss's upstream gradient dD_scale = B^2.  dx is compared with the float64
restatement of tests/site_grad_oracle.py at

    |dx - ref|_bf <= 2^-15 * term_f          (G.BAR; derivation in that module's docstring)

(G.col_bar: a column whose transformed samples all lie within a few percent of each other - 1 / std_t above 100 / (sqrt(B) + 2),
which the inputs here produce at B = 2 and, in a handful of columns out of 131456, at B = 5 - is held to the accuracy of the
operand the backward kernels re-form, the rational erf of alignq_math.h standardised with the forward's statistics, instead of
to 2^-15; each check prints how many columns that concerns.  Measured on an MI355X at B = 2: 5.9e-4 term at F = 4096 and
5.3e-2 term at F = 131456 in such columns, where the analytic gradient is exactly zero.)

and dz / dgamma / dbeta of the folded batch-norm at that bar pushed through the linear batch-norm backward (G.bn_bars).
Each case adds: a run with a non-zero g (std 1e-2) so that the SUM of both terms stays covered - the STE term at the older
tests' bar (atol 1e-5, rtol 1e-4), the correlation term at its own, the two bars added; dalterD / dgamma of the ADMM loss at
1e-4 of their own maximum (they scale with dD_scale); a second run that must give the same bits.

One row per launch form; the shapes are the smallest that select it (geom(), bwd_tile_features(), bwd_vec(), launch_bwd /
launch_bwd4 / launch_bwd1 in alignq_amd/csrc).  Every check prints its worst |dx - ref| / term before asserting."""
import ctypes

import numpy as np
import pytest
import torch

from tests import oracle_c as O
from tests import site_fwd_oracle as SF
from tests import site_grad_oracle as G
from tests.test_gpu_bench_path import _SiteRun, _dev_like, _mem

pytestmark = pytest.mark.gpu
R, K, MU, RHO = 2.0, 8, 0.2, 0.3
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def npy(t):
    return t.detach().cpu().numpy()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _ids(rows):
    return ["-".join(str(v) for v in r) for r in rows]


def scale(x, dD, eps):
    """(term_f, bar_f): the per-column scale and the bar in its units (G.col_bar; G.BAR on every well-conditioned column)"""
    return G.term(x, dD, R, eps), G.col_bar(x, R, eps)


def check_corr(tag, dx, ref, tb):
    """the pure correlation gradient at its bar; tb = scale(...)"""
    term, bar_f = tb
    w, wb = G.worst(dx, ref, term), G.worst(dx, ref, term, bar_f)
    wide = int((bar_f > G.BAR).sum())
    print(f"[site-corr-grad] {tag}: worst |dx - ref| / term = {w:.3e}; worst error / bar = {wb:.3f} "
          f"({wide} of {bar_f.size} columns held to the operand bar instead of 2^-15)")
    assert np.isfinite(dx).all() and wb <= 1.0, (tag, w, wb)


def check_sum(tag, dx, ref_corr, g_ste, tb):
    """both terms: the STE term g * dt/dx at the older tests' bar, the correlation term at its own"""
    term, bar_f = tb
    ref = ref_corr + g_ste
    err = np.abs(np.asarray(dx, np.float64).reshape(ref.shape) - ref)
    bar = TOL + 1e-4 * np.abs(g_ste) + (bar_f * term)[None, :]
    print(f"[site-corr-grad] {tag} (g != 0): worst error / bar = {float((err / bar).max()):.3f}")
    assert (err <= bar).all(), (tag, float((err / bar).max()))


def check_rel(tag, a, ref):
    """dalterD / dgamma of the ADMM loss: 1e-4 of their own maximum"""
    m = float(np.abs(ref).max())
    e = float(np.abs(a - ref).max())
    print(f"[site-corr-grad] {tag}: max error {e:.3e}, 1e-4 * max |ref| = {1e-4 * m:.3e}")
    assert m > 0 and e <= 1e-4 * m, (tag, e, m)


def rebuilt_dD(D_o, A0, G0, B):
    """the loss gradient the rebuilt forms form on the device, times dD_scale = B^2, from the ORACLE's D"""
    _, odD, odA, odG = O.admm_loss(D_o, A0, G0, MU, RHO)
    s = float(B * B)
    return odD.astype(np.float64) * s, odA.astype(np.float64) * s, odG.astype(np.float64) * s


# ------------------------------------------------------------------------------------------------ plain pair forms
# F = 4096 behind a base pointer offset by 4 bytes: 16-byte accesses are off (bwd_vec), the scalar path of the <32> kernel
PLAIN_ROWS = list(G.PLAIN) + [("bwd4+4bytes", B, 4096) for B in (65, 100, 128)]


@pytest.mark.parametrize("form,B,F", PLAIN_ROWS, ids=_ids(PLAIN_ROWS))
def test_plain_site_correlation_gradient(dev, form, B, F):
    """launch_bwd1 (B <= 32), site_bwd_kernel<2, true> (B <= 64), site_bwd4_kernel<32 | 64 | looped 64> (B <= 128) and the
    blocked pair kernels (B > 128): explicit dD with no g (ops.SiteDFn), explicit dD with g (ops.SiteLargeFn: alignq_site_fwd /
    alignq_site_bwd at any B; the D it returns is held to the forward's own bar, tests/site_fwd_oracle.py), and up to 128 rows the
    rebuilt form (ops.SiteFn: alignq_site_bwd_fused, dD_scale = B^2)."""
    from alignq_amd import ops
    x0, dD0 = G.plain_inputs(B, F)
    eps = G.plain_eps(B)
    ref = G.ref_dx(x0, dD0, None, R, eps)
    term = scale(x0, dD0, eps)

    def leaf():
        if not form.endswith("+4bytes"):
            return cu(x0, dev).requires_grad_(True)
        buf = torch.empty(B * F + 4, device=dev)
        buf[1:1 + B * F] = cu(x0.reshape(-1), dev)
        t = buf[1:1 + B * F].view(B, F).detach()
        assert t.data_ptr() % 16 == 4
        return t.requires_grad_(True)

    def explicit():
        xt = leaf()
        ops.SiteDFn.apply(xt, K, R, eps).backward(cu(dD0, dev))
        return npy(xt.grad)

    dx = explicit()
    check_corr(f"{form} {B}x{F} explicit dD", dx, ref, term)
    assert bits_equal(dx, explicit()), "second run differs"

    g0 = (np.random.default_rng(B + F).standard_normal((B, F)) * 1e-2).astype(np.float32)
    xt = leaf()
    xq, D = ops.SiteLargeFn.apply(xt, K, R, eps)
    torch.autograd.backward([xq, D], [cu(g0, dev), cu(dD0, dev)])
    # the forward's D at ITS own scale (tests/site_fwd_oracle.py): BAR * s_ij of the form this shape selects
    fname = SF.form(B, F, False, not form.endswith("+4bytes"))
    t0 = SF.transform(x0)
    fref = SF.reference(x0, t0, eps)
    d_err = np.abs(npy(D).astype(np.float64) - fref["D"]) / SF.d_bar(fname, fref, SF.cond_allowance(x0, t0, eps, SF.acc_of(B)))
    print(f"[site-corr-grad] {form} {B}x{F} forward D ({fname}): worst error / bar = {float(d_err.max()):.3f}")
    assert d_err.max() <= 1.0, (form, B, F, fname, float(d_err.max()))
    check_sum(f"{form} {B}x{F} explicit dD", npy(xt.grad), ref, g0.astype(np.float64) * G.jac(x0, R), term)

    if B > 128:
        return
    A0, G0 = G.admm_params(B, 128, B + F)
    _, D_o = O.site_fwd(x0, K, R, eps)
    dD2, dA_ref, dG_ref = rebuilt_dD(D_o, A0, G0, B)
    ref2 = G.ref_dx(x0, dD2, None, R, eps)
    term2 = scale(x0, dD2, eps)

    def rebuilt():
        xt, A, Gm = leaf(), cu(A0, dev).requires_grad_(True), cu(G0, dev).requires_grad_(True)
        _, loss, _ = ops.SiteFn.apply(xt, A, Gm, K, R, eps, MU, RHO)
        (loss * float(B * B)).backward()
        return npy(xt.grad), npy(A.grad), npy(Gm.grad)

    dx2, dA, dG = rebuilt()
    check_corr(f"{form} {B}x{F} rebuilt dD", dx2, ref2, term2)
    check_rel(f"{form} {B}x{F} dalterD", dA, dA_ref)
    check_rel(f"{form} {B}x{F} dgamma", dG, dG_ref)
    again = rebuilt()
    assert all(bits_equal(a, b) for a, b in zip((dx2, dA, dG), again)), "second run differs"


# ------------------------------------------------------------------------------------------------ 64 < B <= 128, folded batch-norm
def _bn_checks(tag, run, ref, term, C, nhwc, g_parts=None):
    """dx, dz, dgamma, dbeta of one _SiteRun against ref_bn; g_parts = (ref of g = None, STE dx) for a run with g"""
    bar_dz, bar_dg, bar_db = G.bn_bars(term[0], ref["zhat"], ref["a"], C, nhwc, bar=term[1])
    dx, dz = _mem(run.dx, nhwc), _mem(run.dz, nhwc)
    dg, db = npy(run.dgam).astype(np.float64), npy(run.dbet).astype(np.float64)
    n = dz.shape[0] * (dz.shape[1] // C)
    if g_parts is None:
        check_corr(tag, dx, ref["dx"], term)
        extra_dz, extra_c = 0.0, 0.0
    else:
        ref0, g_ste = g_parts
        check_sum(tag, dx, ref0["dx"], g_ste, term)
        extra_dz = TOL + 1e-4 * np.abs(ref["dz"])           # the older tests' bars on the STE share
        extra_c = TOL * np.sqrt(n)
    for name, a, r_, bar in (("dz", dz, ref["dz"], bar_dz + extra_dz), ("dgamma", dg, ref["dgamma"], bar_dg + extra_c),
                             ("dbeta", db, ref["dbeta"], bar_db + extra_c)):
        w = float((np.abs(a - r_) / bar).max())
        print(f"[site-corr-grad] {tag} {name}: worst error / bar = {w:.3f}")
        assert np.isfinite(a).all() and w <= 1.0, (tag, name, w)


@pytest.mark.parametrize("nhwc", [0, 1])
@pytest.mark.parametrize("B,C,H", G.BN4, ids=_ids(G.BN4))
def test_bn_folded_site_correlation_gradient(dev, B, C, H, nhwc):
    """site_bwd4_kernel<32, true, true> behind alignq_site_prep_fused (dD_scale = B^2), both layouts: no g; g with the ReLU
    mask from y, a residual and dres; g with the mask from int8 level indices (k = 4); alignq_site_bwd_apply_bn_fill carrying a
    filter-gradient reduction; alignq_site_bwd_apply_bn_twin with a second site whose dD_scale is twice the first's."""
    from alignq_amd import _lib as L
    lib = L.load()
    F, HW, shape = C * H * H, H * H, (B, C, H, H)
    zm, gamma, beta, _ = G.bn_inputs(B, C, H, seed=nhwc)
    rng = np.random.default_rng(B + C + H + nhwc)
    gm = (rng.standard_normal((B, F)) * 1e-2).astype(np.float32)
    rm_ = (rng.standard_normal((B, F)) * 0.7).astype(np.float32)
    A0, G0 = G.admm_params(B, 128, B + C)
    z, g, res = (_dev_like(a, shape, nhwc, dev) for a in (zm, gm, rm_))
    tg, tb, A, Gm = (cu(a, dev) for a in (gamma, beta, A0, G0))
    ab_o, save_o, _ = O.bn_fold_ab(zm, C, nhwc, gamma, beta, 1e-5)
    s = float(B * B)

    refs = {}
    for k, relu, with_res in ((K, True, True), (4, True, False)):
        y_o, D_o, x_o = O.bn_site_fwd(zm, C, nhwc, ab_o, k, R, 0.0, rm_ if with_res else None, relu)
        if k == K:                                       # D does not depend on k: one reference dD for all variants
            dD, dA_ref, dG_ref = rebuilt_dD(D_o, A0, G0, B)
            term = scale(x_o, dD, 0.0)
            ref0 = G.ref_bn(zm, dD, None, gamma, beta, C, nhwc, R, 0.0, x_at=x_o)
        refs[k] = (y_o, G.ref_bn(zm, dD, gm, gamma, beta, C, nhwc, R, 0.0, mask=y_o > 0, x_at=x_o))

    def site(k, with_res, bins):
        run = _SiteRun(dev, z, tg, tb, k, True, res if with_res else None, nhwc)
        run.mask_from_bins = bins
        return run.forward("ab_in", ab_o.copy(), save_o.copy(), want_bins=bins).reduce_loss(A, Gm, MU, RHO)

    tag = f"bn4 {B}x{C}x{H}x{H} nhwc={nhwc}"
    run = site(K, True, False)
    run.backward(None, s).bn_backward()
    torch.cuda.synchronize()
    _bn_checks(tag, run, ref0, term, C, nhwc)
    check_rel(tag + " dalterD", npy(run.dA), dA_ref)
    check_rel(tag + " dgamma(ADMM)", npy(run.dG), dG_ref)
    first = [npy(t).copy() for t in (run.dx, run.dz, run.dgam, run.dbet, run.dA, run.dG)]
    run.backward(None, s).bn_backward()
    torch.cuda.synchronize()
    assert all(bits_equal(a, npy(t)) for a, t in zip(first, (run.dx, run.dz, run.dgam, run.dbet, run.dA, run.dG))), "second run differs"

    for k, with_res, bins in ((K, True, False), (4, False, True)):
        y_o, ref_g = refs[k]
        rg = site(k, with_res, bins)
        if bins:
            assert rg.bins.dtype == torch.int8
        rg.backward(g, s).bn_backward()
        torch.cuda.synchronize()
        g_ste = ref_g["dres"] * G.jac(ref_g["x"], R)
        _bn_checks(tag + (" ybins mask" if bins else " y mask + residual"), rg, ref_g, term, C, nhwc, (ref0, g_ste))
        if rg.dres is not None:                  # a copy of the masked g (by value: a masked-out negative g is +0 there, -0 in the product)
            assert np.array_equal(_mem(rg.dres, nhwc), ref_g["dres"].astype(np.float32))

    # ---- the filler role: one filter-gradient slab reduction rides in the launch; dx at the bar, dW the reduction's own bits
    assert lib.alignq_site_bwd_fill_slots(B, F) >= 1
    n_slabs, n_elem = 5, 9 * 16 * 16
    slabs = torch.randn(n_slabs, n_elem, device=dev)
    dw_ref, dw = torch.empty(n_elem, device=dev), torch.full((n_elem,), float("nan"), device=dev)
    L.check(lib.alignq_conv3x3_wgrad_reduce_multi(1, L.ptr_array([slabs]), L.ptr_array([dw_ref]), (ctypes.c_int * 1)(n_slabs),
                                                  (ctypes.c_int * 1)(n_elem), L.stream_ptr()), "wgrad_reduce_multi")
    dx_f, part_f = torch.full_like(run.dx, float("nan")), torch.zeros_like(run.part)
    L.check(lib.alignq_site_bwd_apply_bn_fill(None, L.ptr(run.S), L.ptr(z), L.ptr(run.ab), L.ptr(run.save), C, HW, int(nhwc),
                                              L.ptr(run.y), None, 0, None, L.ptr(run.stats), B, F, R, 0.0, L.ptr(dx_f),
                                              L.ptr(part_f), 1, L.ptr_array([slabs]), L.ptr_array([dw]), (ctypes.c_int * 1)(n_slabs),
                                              (ctypes.c_int * 1)(n_elem), L.stream_ptr()), "alignq_site_bwd_apply_bn_fill")
    torch.cuda.synchronize()
    check_corr(tag + " with a filler", _mem(dx_f, nhwc), ref0["dx"], term)
    assert bits_equal(npy(dw), npy(dw_ref)) and bits_equal(npy(dx_f), first[0])

    # ---- the twin launch: site b = the same site behind a preparation with dD_scale = 2 B^2 (dx is linear in dD)
    run_b = site(K, True, False)
    run_b.backward(None, 2.0 * s)
    structs, outs = [], []
    for q in (run, run_b):
        dx_t, part_t = torch.full_like(q.dx, float("nan")), torch.zeros_like(q.part)
        structs.append(L.SiteBwdBnArgs(None, L.ptr(q.S), L.ptr(z), L.ptr(q.ab), L.ptr(q.save), C, HW, int(nhwc), L.ptr(q.y), None, 0,
                                       None, L.ptr(q.stats), B, F, R, 0.0, L.ptr(dx_t), L.ptr(part_t)))
        outs.append((dx_t, part_t))
    L.check(lib.alignq_site_bwd_apply_bn_twin(ctypes.byref(structs[0]), ctypes.byref(structs[1]), L.stream_ptr()), "bwd twin")
    torch.cuda.synchronize()
    check_corr(tag + " twin a", _mem(outs[0][0], nhwc), ref0["dx"], term)
    check_corr(tag + " twin b", _mem(outs[1][0], nhwc), 2.0 * ref0["dx"], (2.0 * term[0], term[1]))
    for q, (dx_t, part_t) in zip((run, run_b), outs):           # and through the batch-norm backward, from the twin's sums
        q.dx, q.part = dx_t, part_t
        q.bn_backward()
    torch.cuda.synchronize()
    _bn_checks(tag + " twin a", run, ref0, term, C, nhwc)
    ref_b = {k_: (2.0 * v if k_ in ("dx", "dz", "dgamma", "dbeta") else v) for k_, v in ref0.items()}
    _bn_checks(tag + " twin b", run_b, ref_b, (2.0 * term[0], term[1]), C, nhwc)


# ------------------------------------------------------------------------------------------------ B <= 32, folded (a, b)
class _Site1:
    """`groups` batch slices of one small-batch site, channels-last, through the C ABI: alignq_site1_groups_fwd_m ->
    alignq_site1_groups_reduce_loss -> alignq_site1_groups_prep (dD_scale = B^2, one scalar for all slices)."""

    def __init__(self, dev, B, C, H, groups, seed):
        from alignq_amd import _lib as L
        self.L, self.lib, self.dev = L, L.load(), dev
        lib, p = self.lib, L.ptr
        self.B, self.C, self.F, self.groups, self.eps = B, C, C * H * H, groups, 1e-5
        F, Gn = self.F, groups
        rng = np.random.default_rng(seed)
        self.gamma, self.beta = (rng.random(C) + 0.5).astype(np.float32), (rng.standard_normal(C) * 0.2).astype(np.float32)
        self.zm = [(rng.standard_normal((B, F)) * 1.4 + 0.3).astype(np.float32) for _ in range(Gn)]
        self.rm = [np.maximum(rng.standard_normal((B, F)), 0).astype(np.float32) - 0.3 for _ in range(Gn)]
        self.gm = [(rng.standard_normal((B, F)) * 1e-2).astype(np.float32) for _ in range(Gn)]
        self.A0, self.G0 = G.admm_params(B, B, seed + 1)
        fold = [O.bn_fold_ab(zg, C, 1, self.gamma, self.beta, 1e-5) for zg in self.zm]
        self.ab_o, self.save_o = [f[0] for f in fold], [f[1] for f in fold]
        st = lambda parts: cu(np.stack(parts), dev)          # noqa: E731
        self.z, self.res, self.g = st(self.zm), st(self.rm), st(self.gm)
        self.ab, self.save = st(self.ab_o), st(self.save_o)
        self.A, self.Gm = cu(self.A0, dev), cu(self.G0, dev)
        self.y = torch.empty_like(self.z)
        self.stats = torch.empty(Gn, 4, F, device=dev)
        ws = torch.empty(lib.alignq_site_ws_bytes(B, F) * Gn, dtype=torch.uint8, device=dev)
        self.mask = torch.zeros(lib.alignq_site1_mask_bytes(B, F, Gn), dtype=torch.uint8, device=dev)
        L.check(lib.alignq_site1_groups_fwd_m(p(self.z), p(self.ab), C, B, F, Gn, K, R, self.eps, p(self.res), 1, p(self.y),
                                              p(self.stats), p(ws), p(self.mask), L.stream_ptr()), "alignq_site1_groups_fwd_m")
        self.D, self.scal = torch.empty(Gn, B, B, device=dev), torch.empty(Gn, 4, device=dev)
        L.check(lib.alignq_site1_groups_reduce_loss(p(ws), B, F, Gn, p(self.D), p(self.A), p(self.Gm), B, MU, RHO, p(self.scal),
                                                    L.stream_ptr()), "alignq_site1_groups_reduce_loss")
        self.gl = torch.tensor(float(B * B), device=dev)
        self.S = torch.zeros(lib.alignq_site_bwd_ws_bytes(B) * Gn, dtype=torch.uint8, device=dev)
        self.dA, self.dG = torch.empty_like(self.A), torch.empty_like(self.Gm)
        L.check(lib.alignq_site1_groups_prep(p(self.D), p(self.A), p(self.Gm), B, p(self.scal), MU, p(self.gl), 0, B, F, Gn, p(self.S),
                                             p(self.dA), p(self.dG), L.stream_ptr()), "alignq_site1_groups_prep")
        torch.cuda.synchronize()
        # the references, per slice
        self.ref0, self.ref_g, self.term, self.dA_ref, self.dG_ref = [], [], [], 0.0, 0.0
        for i in range(Gn):
            y_o, D_o, x_o = O.bn_site_fwd(self.zm[i], C, 1, self.ab_o[i], K, R, self.eps, self.rm[i], True)
            assert bits_equal(npy(self.y[i]), y_o)
            dD, dA_r, dG_r = rebuilt_dD(D_o, self.A0, self.G0, B)
            self.dA_ref, self.dG_ref = self.dA_ref + dA_r, self.dG_ref + dG_r
            self.term.append(scale(x_o, dD, self.eps))
            kw = dict(x_at=x_o)
            self.ref0.append(G.ref_bn(self.zm[i], dD, None, self.gamma, self.beta, C, 1, R, self.eps, **kw))
            self.ref_g.append(G.ref_bn(self.zm[i], dD, self.gm[i], self.gamma, self.beta, C, 1, R, self.eps, mask=y_o > 0, **kw))

    def bwd(self, fn, with_g, bn):
        """alignq_site1_groups_bwd (bn = None), _bwd_bn (bn = 'y') or _bwd_bn_m (bn = 'mask'); returns numpy outputs"""
        L, lib, p = self.L, self.lib, self.L.ptr
        B, C, F, Gn = self.B, self.C, self.F, self.groups
        g = self.g if with_g else None
        out, dres = torch.full_like(self.z, float("nan")), torch.full_like(self.z, float("nan"))
        if bn is None:
            L.check(fn(p(g), None, p(self.y if with_g else None), p(self.S), p(self.z), p(self.ab), C, p(self.stats), B, F, Gn, R,
                       self.eps, p(out), p(dres), L.stream_ptr()), "alignq_site1_groups_bwd")
            torch.cuda.synchronize()
            return npy(out), npy(dres)
        dg, db = torch.empty(C, device=self.dev), torch.empty(C, device=self.dev)
        cols = torch.empty(lib.alignq_site1_cols_bytes(F, Gn), dtype=torch.uint8, device=self.dev)
        ws_bn = torch.empty(lib.alignq_bnq_ws_bytes(C, Gn), dtype=torch.uint8, device=self.dev)
        m = (self.mask if bn == "mask" else self.y) if with_g else None
        L.check(fn(p(g), None, p(m), p(self.S), p(self.z), p(self.ab), p(self.save), C, p(self.stats), B, F, Gn, R, self.eps, p(out),
                   p(dres), p(dg), p(db), p(cols), p(ws_bn), L.stream_ptr()), "alignq_site1_groups_bwd_bn")
        torch.cuda.synchronize()
        return npy(out), npy(dres), npy(dg).astype(np.float64), npy(db).astype(np.float64)


@pytest.mark.parametrize("B,C,H", G.BN1, ids=_ids(G.BN1))
def test_small_batch_groups_correlation_gradient(dev, B, C, H):
    """launch_bwd1 with the folded (a, b), two batch slices per launch: alignq_site1_groups_bwd (dx), _bwd_bn (dz, dgamma,
    dbeta from the per-column sums) and _bwd_bn_m (the one-bit ReLU mask), each with no g and with g (mask, dres)."""
    s1 = _Site1(dev, B, C, H, 2, 7 * B + C)
    lib, n = s1.lib, B * H * H
    tag = f"site1 groups {B}x{C}x{H}x{H}"
    check_rel(tag + " dalterD", npy(s1.dA), s1.dA_ref)
    check_rel(tag + " dgamma(ADMM)", npy(s1.dG), s1.dG_ref)
    for with_g in (False, True):
        refs = s1.ref_g if with_g else s1.ref0
        dx, dres = s1.bwd(lib.alignq_site1_groups_bwd, with_g, None)
        for i in range(2):
            if with_g:
                g_ste = refs[i]["dres"] * G.jac(refs[i]["x"], R)
                check_sum(f"{tag} bwd slice {i}", dx[i], s1.ref0[i]["dx"], g_ste, s1.term[i])
                assert np.array_equal(dres[i], refs[i]["dres"].astype(np.float32))
            else:
                check_corr(f"{tag} bwd slice {i}", dx[i], refs[i]["dx"], s1.term[i])
        assert bits_equal(dx, s1.bwd(lib.alignq_site1_groups_bwd, with_g, None)[0]), "second run differs"
        for fn, bn in ((lib.alignq_site1_groups_bwd_bn, "y"), (lib.alignq_site1_groups_bwd_bn_m, "mask")):
            dz, dres, dg, db = s1.bwd(fn, with_g, bn)
            bars = [G.bn_bars(s1.term[i][0], refs[i]["zhat"], refs[i]["a"], C, 1, bar=s1.term[i][1]) for i in range(2)]
            extra_c = TOL * np.sqrt(n) if with_g else 0.0              # the older tests' bar on the STE share of the sums
            for i in range(2):
                bar = bars[i][0] + ((TOL + 1e-4 * np.abs(refs[i]["dz"])) if with_g else 0.0)
                w = float((np.abs(dz[i] - refs[i]["dz"]) / bar).max())
                print(f"[site-corr-grad] {tag} bwd_bn[{bn}] g={with_g} slice {i} dz: worst error / bar = {w:.3f}")
                assert np.isfinite(dz[i]).all() and w <= 1.0, (tag, bn, i, w)
                if with_g:
                    assert np.array_equal(dres[i], refs[i]["dres"].astype(np.float32))
            for name, a, key, j in (("dgamma", dg, "dgamma", 1), ("dbeta", db, "dbeta", 2)):
                r_ = refs[0][key] + refs[1][key]                       # the sums over the slices
                w = float((np.abs(a - r_) / (bars[0][j] + bars[1][j] + 2 * extra_c)).max())
                print(f"[site-corr-grad] {tag} bwd_bn[{bn}] g={with_g} {name}: worst error / bar = {w:.3f}")
                assert w <= 1.0, (tag, bn, name, w)


def test_small_batch_folded_ab_correlation_gradient(dev):
    """alignq_site_bwd_apply_ab and alignq_site_bwd_apply_ab_relu (B = 28, C = 64, H = 4; the latter is reached through the C
    ABI only): dx w.r.t. x = a z + b.  _ab_relu requires g: zeros for the pure correlation run, then g with the mask and dres."""
    B, C, H = G.AB1
    s1 = _Site1(dev, B, C, H, 1, 99)
    L, lib, p = s1.L, s1.lib, s1.L.ptr
    F, ref0, ref_g, term = s1.F, s1.ref0[0], s1.ref_g[0], s1.term[0]
    z, y, g, ab, stats = s1.z[0], s1.y[0], s1.g[0], s1.ab[0], s1.stats[0]

    def ab_plain(gt):
        dx = torch.full_like(z, float("nan"))
        L.check(lib.alignq_site_bwd_apply_ab(p(gt), p(s1.S), p(z), p(ab), C, p(stats), B, F, R, s1.eps, p(dx), L.stream_ptr()),
                "alignq_site_bwd_apply_ab")
        torch.cuda.synchronize()
        return npy(dx)

    def ab_relu(gt):
        dx, dres = torch.full_like(z, float("nan")), torch.full_like(z, float("nan"))
        L.check(lib.alignq_site_bwd_apply_ab_relu(p(gt), p(y), p(s1.S), p(z), p(ab), C, p(stats), B, F, R, s1.eps, p(dx), p(dres),
                                                  L.stream_ptr()), "alignq_site_bwd_apply_ab_relu")
        torch.cuda.synchronize()
        return npy(dx), npy(dres)

    dx = ab_plain(None)
    check_corr("apply_ab 28x64x4x4", dx, ref0["dx"], term)
    assert bits_equal(dx, ab_plain(None)), "second run differs"
    dx = ab_plain(g)                                                   # no mask in this entry point: the whole g
    check_sum("apply_ab 28x64x4x4", dx, ref0["dx"], s1.gm[0].astype(np.float64) * G.jac(ref0["x"], R), term)

    dx, dres = ab_relu(torch.zeros_like(g))
    check_corr("apply_ab_relu 28x64x4x4 (g = 0)", dx, ref0["dx"], term)
    assert not dres.any()
    assert bits_equal(dx, ab_relu(torch.zeros_like(g))[0]), "second run differs"
    dx, dres = ab_relu(g)
    check_sum("apply_ab_relu 28x64x4x4", dx, ref0["dx"], ref_g["dres"] * G.jac(ref_g["x"], R), term)
    assert np.array_equal(dres, ref_g["dres"].astype(np.float32))
    check_rel("apply_ab dalterD", npy(s1.dA), s1.dA_ref)
    check_rel("apply_ab dgamma(ADMM)", npy(s1.dG), s1.dG_ref)
