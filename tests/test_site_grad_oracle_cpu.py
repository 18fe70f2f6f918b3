"""The float64 restatement of the site backward (tests/site_grad_oracle.py) against the C oracle, and proof that the inputs
of tests/test_gpu_site_corr_grad.py make its bar bite.  Runs anywhere.

Why this file exists: at the inputs of the older site tests (the ADMM loss's own dD, max|dD| about 1e-3 and below) and
their bar (atol 1e-5, rtol 1e-4), a backward that wrote g * dt/dx and NOTHING ELSE passes: the whole correlation gradient is
smaller than the absolute tolerance (test_old_bar_does_not_see_a_dropped_correlation_term pins that).  The GPU tests built on
this helper therefore check the correlation gradient alone (g = None) with an O(1) dD at BAR * term_f per column."""
import math

import numpy as np
import pytest

from tests import oracle_c as O
from tests import site_grad_oracle as G

R, K = 2.0, 8
ORACLE_BAR = 1e-6            # the C oracle (fp32 table erf for t, fp32 outputs) against float64, in units of term_f


def _eps(B):
    return G.plain_eps(B)


def _ids(rows):
    return ["-".join(str(v) for v in r) for r in rows]


@pytest.mark.parametrize("form,B,F", G.PLAIN, ids=_ids(G.PLAIN))
def test_c_oracle_agrees_with_float64_restatement(form, B, F):
    """O.site_bwd (g = None) within 1e-6 * term_f of autograd in float64, at every row of the GPU matrix; the closed form
    (the carrier of the mutants below) agrees with autograd to rounding."""
    x, dD = G.plain_inputs(B, F)
    eps = _eps(B)
    ref = G.ref_dx(x, dD, None, R, eps)
    term = G.term(x, dD, R, eps)
    w_formula = G.worst(G.formula_dx(x, dD, None, R, eps), ref, term)
    # the oracle's t is the project's fp32 transform: hold it to 2^-22 of r * erf(x / sqrt 2) here, and take the float64
    # derivative at that t (G.ref_dx: where a column's samples nearly coincide corr(t) amplifies the last bit of t)
    _, t32, _ = O.act_quant_fwd(x, K, R, O.FORMULA_ADMM)
    t64 = R * np.vectorize(math.erf)(x.astype(np.float64) / math.sqrt(2.0)) if x.size < 10000 else None
    if t64 is not None:
        assert np.abs(t32 - t64).max() <= 2.0 ** -22
    w_oracle = G.worst(O.site_bwd(None, dD, x, R, eps), G.ref_dx(x, dD, None, R, eps, t_at=t32), term)
    print(f"{form} {B}x{F}: closed form {w_formula:.2e}, C oracle {w_oracle:.2e} (units of term)")
    assert w_formula <= 1e-9        # float64 rounding times the conditioning of a column whose samples nearly coincide
    assert w_oracle <= ORACLE_BAR
    if B == 2 and eps == 0.0:       # both standardised columns are +-1/sqrt 2 whatever x is: the gradient is analytically zero
        assert np.abs(ref).max() <= 1e-9 * term.max()


@pytest.mark.parametrize("form,B,F", G.PLAIN, ids=_ids(G.PLAIN))
def test_every_defect_is_far_outside_the_bar(form, B, F):
    """Each single defect of the closed form moves some element by more than 100 bars at the GPU tests' inputs.  At B = 2 the
    true gradient is zero BECAUSE the three terms cancel, so only the defects that break the cancellation (mean, proj) can
    show; the others leave zero and are exempt there."""
    x, dD = G.plain_inputs(B, F)
    eps = _eps(B)
    ref = G.formula_dx(x, dD, None, R, eps)      # equal to autograd to rounding (the test above)
    term, bar_f = G.term(x, dD, R, eps), G.col_bar(x, R, eps)
    for defect in G.DEFECTS:
        if B == 2 and defect not in ("mean_kept", "proj_dropped"):
            continue
        bars = G.worst(G.formula_dx(x, dD, None, R, eps, defect), ref, term, bar_f)
        assert bars > 100.0, (defect, bars)


@pytest.mark.parametrize("B,C,H,nhwc", [(b, c, h, n) for (b, c, h) in G.BN4 for n in (0, 1)]
                         + [(b, c, h, 1) for (b, c, h) in G.BN1 + (G.AB1,)])
def test_c_oracle_bn_fold_agrees_with_float64_restatement(B, C, H, nhwc):
    """O.bn_site_bwd (g = None) against autograd through the batch-norm: dx at 1e-6 * term_f, dz / dgamma / dbeta at that bar
    pushed through the linear batch-norm backward (G.bn_bars).  The site's derivative is taken at the oracle's fp32 x."""
    z, gamma, beta, dD = G.bn_inputs(B, C, H)
    ab, save, _ = O.bn_fold_ab(z, C, nhwc, gamma, beta, 1e-5)
    x32 = O.bn_apply(z, C, nhwc, ab)
    dz, dg, db, _, dx = O.bn_site_bwd(None, dD, z, C, nhwc, ab, save, None, R, 0.0)
    ref = G.ref_bn(z, dD, None, gamma, beta, C, nhwc, R, 0.0, x_at=x32)
    term = G.term(x32, dD, R, 0.0)
    bar_dz, bar_dg, bar_db = G.bn_bars(term, ref["zhat"], ref["a"], C, nhwc, bar=ORACLE_BAR)
    assert G.worst(dx, ref["dx"], term) <= ORACLE_BAR
    assert (np.abs(dz - ref["dz"]) <= bar_dz).all(), float((np.abs(dz - ref["dz"]) / bar_dz).max())
    assert (np.abs(dg - ref["dgamma"]) <= bar_dg).all(), float((np.abs(dg - ref["dgamma"]) / bar_dg).max())
    assert (np.abs(db - ref["dbeta"]) <= bar_db).all(), float((np.abs(db - ref["dbeta"]) / bar_db).max())
    # and the bars bite: without the correlation term every output is zero (g = None): dz more than 100 bars away somewhere;
    # dgamma is a sum of n = B * HW terms of random sign held to the worst-case bound n * e, sqrt(n) looser, still bars away
    b_dz, b_dg, _ = G.bn_bars(term, ref["zhat"], ref["a"], C, nhwc)
    assert (np.abs(ref["dz"]) / b_dz).max() > 100.0
    assert (np.abs(ref["dgamma"]) / b_dg).max() > 5.0


@pytest.mark.parametrize("B,C,H,W,k", [(128, 64, 8, 8, 2), (28, 8, 14, 14, 8), (100, 16, 16, 16, 4)])
def test_old_bar_does_not_see_a_dropped_correlation_term(B, C, H, W, k):
    """The inputs of tests/test_gpu_parity.py::test_site_vs_oracle_shapes (same generator, same order of draws) and its bar:
    the backward with the correlation term dropped PASSES np.testing.assert_allclose(atol=1e-5, rtol=1e-4) against the
    oracle.  The same defect at the new scale (g = None, per-column bar) is thousands of bars out."""
    rng = np.random.default_rng(B + C + H)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32).reshape(B, -1)
    gq = (rng.standard_normal((B, C, H, W)) * 0.01).astype(np.float32).reshape(B, -1)
    A0, G0 = rng.random((128, 128)).astype(np.float32), rng.random((128, 128)).astype(np.float32)
    _, oD = O.site_fwd(x, k, R, 0.0)
    _, odD, _, _ = O.admm_loss(oD, A0, G0, 0.2, 0.3)
    odx = O.site_bwd(gq, odD, x, R, 0.0)
    dropped = G.formula_dx(x, odD, gq, R, 0.0, "corr_dropped")
    np.testing.assert_allclose(dropped, odx, atol=1e-5, rtol=1e-4)          # the old bar is blind to it
    ref = G.ref_dx(x, odD, None, R, 0.0)
    term = G.term(x, odD, R, 0.0)
    assert G.worst(np.zeros_like(ref), ref, term) / G.BAR > 100.0            # the new one is not
