"""tests/weights_oracle.py (the float64 statement of the weight statistics / backward, the cdf backward and the SGD step) pinned
on the CPU: against the reference's own data (fixtures G2 and G7, at the bars the GPU tests hold the kernels to), against the C
oracle on the tensors and hyper-parameter sets of tests/test_gpu_weights_optim.py, and one mutation per operation showing that
the bar of that GPU test sees a plausible error.  The case tables and seeded inputs of both files live here; what the tables
say about launch forms (chunks, alignment, passes) matters to the GPU file only: on the CPU every tensor is just its values."""
import numpy as np
import pytest
import torch

from tests import oracle_c as O
from tests import weights_oracle as W
from tests.conftest import load_golden

# ------------------------------------------------------------------------------------------------ shared cases and inputs
MS, MS_STRESS = (0.01, 0.05), (1.0, 1e-3)       # N(m, s) of the filters; the stress pair has a mean 1000 x its spread
# csrc/multi_tensor_kernels.hip: blocks_for caps a tensor's grid row at kMaxBlk = 256 workgroups of kThreads = 256 threads with
# kU = 8 loads in flight each, so ONE pass of MT_FOR_ELEMENTS covers 256 * 256 * 8 = 524288 elements
PASS = 256 * 256 * 8
FUSED_MAX = 9 * 4 * 1024                         # kFusedMaxN: the largest filter of the one-launch form
# mt_sgd_admm_kernel strides by kAdmmThreads = 1024 threads: one pass of its (at most kMaxBlk = 256) workgroups, kU = 8 each
PASS_ADMM = 256 * 1024 * 8
H_CYCLE = [16, 144, 432, 2304, 435]


def h_sizes(T, odd_chunks):
    """T sizes cycling through H_CYCLE; 435 (n % 4 != 0: the two-launch form) only in the 64-tensor chunks listed, the other
    chunks are all multiples of 4 (the fused form)"""
    out = []
    for i in range(T):
        cyc = H_CYCLE if (i // 64) in odd_chunks else H_CYCLE[:4]
        out.append(cyc[i % len(cyc)])
    return out


# name -> (sizes, (m, s), first element's offset from a 16-byte boundary)
FWD_CASES = {
    "a432": ([432], MS, 0), "a36864": ([FUSED_MAX], MS, 0), "a4": ([4], MS, 0),
    "b": ([432, FUSED_MAX, 16, 2304], MS, 0),
    "c": ([FUSED_MAX + 4], MS, 0),
    "d435": ([435], MS, 0), "d3": ([3], MS, 0), "d2": ([2], MS, 0),
    "e": ([432, 435, FUSED_MAX], MS, 0),
    "f": ([432], MS, 1),
    "g1": ([PASS + 1000], MS, 0), "g2": ([2 * PASS + 7], MS, 0),
    "h65": (h_sizes(65, {1}), MS, 0), "h130": (h_sizes(130, {0, 2}), MS, 0), "h130b": (h_sizes(130, {1}), MS, 0),
    "i36864": ([FUSED_MAX], MS_STRESS, 0), "i36868": ([FUSED_MAX + 4], MS_STRESS, 0),
}
BWD_CASES = [c for c in FWD_CASES if c[0] not in "fi"]
PER_TENSOR_CASES = [c for c in FWD_CASES if c[0] in "acdg"]
G_SCALES = (1.0, 1e-3)                            # upstream gradients N(0, 1) and at the convolution gradients' scale
CDF_BWD_SHAPES = (435, FUSED_MAX, PASS + 1000)

# (lr, momentum, dampening, weight_decay, nesterov)
SGD_HYPER = [(0.04, 0.9, 0.0, 1e-4, 0), (0.1, 0.0, 0.0, 0.0, 0), (0.04, 0.9, 0.0, 5e-4, 1), (0.04, 0.9, 0.1, 1e-4, 0)]
SGD_CYCLE = [16, 64, 432, 2304, 10]
SGD_LISTS = {
    "six": [10, 16, 432, FUSED_MAX, 64, 1],
    "t73": [SGD_CYCLE[i % 5] for i in range(73)],
    "t150": [SGD_CYCLE[i % 5] for i in range(150)],
    "big": [PASS + 1000],
}
ADMM_LIST = [10, 16, 432, FUSED_MAX, 1, PASS_ADMM + 5]
LAM, LAM2 = 1.0, 4.0                              # fixture G7's


def _seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


def filters(name):
    """the seeded float32 filters of one FWD_CASES entry (case f has case a432's values)"""
    sizes, (m, s), _ = FWD_CASES[name]
    rng = np.random.default_rng(_seed("a432" if name == "f" else name))
    return [(m + s * rng.standard_normal(n)).astype(np.float32) for n in sizes]


def upstream(name, scale):
    rng = np.random.default_rng(_seed(name) + 7)
    return [(scale * rng.standard_normal(n)).astype(np.float32) for n in FWD_CASES[name][0]]


def cdf_bwd_inputs(n, scale):
    rng = np.random.default_rng(n)
    x = (MS[0] + MS[1] * rng.standard_normal(n)).astype(np.float32)
    gc, gp = ((scale * rng.standard_normal(n)).astype(np.float32) for _ in range(2))
    return x, np.array(W.weight_stats64(x), np.float32), gc, gp


def sgd_inputs(sizes, seed):
    """per tensor: p, three steps' gradients, and for every second tensor the (w_cdf, w_pdf) the ADMM-tree weight quantiser leaves
    for a filter of that size (None for the others), w_cdf rounded to the grid of 2^-12.

    Why the grid: transform() ends in `% 1`, so where a = (c + 0.5)(2^bitW - 1) comes within a float32 rounding of an integer
    the rewritten gradient jumps by its whole range (sigmoid_d(0) = 0.25 against sigmoid_d(8) = 3e-4), in ANY float32
    evaluation: the reference's own formula in plain float32 NumPy misses G7's bar 330-fold at 15 of 524288 + 1000 elements
    for bitW = 8 when c is arbitrary.  On the grid c + 0.5 has at most 14 significant bits and a at most 22, both exact in
    float32 for every bitW <= 8, the fractional part is exact (0 and 4095/4096 included), and no element needs excusing."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(sizes):
        p = (MS[0] + MS[1] * rng.standard_normal(n)).astype(np.float32)
        gs = [(1e-2 * rng.standard_normal(n)).astype(np.float32) for _ in range(3)]
        cdf = pdf = None
        if i % 2 == 0:
            _, cdf, pdf, _ = O.weight_quant_fwd(p, np.array(MS, np.float32), 32, O.FORMULA_ADMM)
            cdf = (np.round(cdf.astype(np.float64) * 4096.0) / 4096.0).astype(np.float32)
        out.append((p, gs, cdf, pdf))
    return out


def ulp(x):
    """one unit in the last place of the largest magnitude in x, as a float32"""
    return float(np.spacing(np.float32(np.max(np.abs(x)))))


def sgd_bar(o32, ref64):
    """the SGD bar of the GPU tests: twice the float32 C oracle's largest error against float64 on the same inputs (a fused and
    an unfused multiply-add round at different points), at least one ulp of the tensor's largest magnitude"""
    return max(2.0 * float(np.max(np.abs(o32.astype(np.float64) - ref64))), ulp(ref64))


def bwd_tol(ref64, gmax, atol_scale=1.0):
    """the project's bar for G2's dW (atol 2e-5, rtol 1e-4), the absolute part scaled by the upstream gradient's size"""
    return 2e-5 * gmax * atol_scale + 1e-4 * np.abs(ref64)


def grad_tol(ref64, dir64, pdf):
    """G7's gradout bar (atol 1e-5, rtol 1e-5), the absolute part scaled by the size of dir * pdf"""
    return 1e-5 * float(np.max(np.abs(dir64 * pdf.reshape(-1).astype(np.float64)))) + 1e-5 * np.abs(ref64)


# ------------------------------------------------------------------------------------------------ the reference's own data
@pytest.mark.parametrize("fname", ["g2_weight_quant_admm", "g2_weight_quant_cdfonly"])
def test_statement_vs_reference_weights(fname):
    """G2, both trees: (m, s) and dW at the bars of test_weight_quant (2e-6 relative; atol 2e-5, rtol 1e-4).  One backward serves
    both: the ADMM tree rounds t = 2c - 1 (slope 1 in t), the CDF tree takes 2 round(c) - 1 (slope 2 in c), 2 phi_s either way."""
    g = load_golden(fname)
    si = 0
    while f"W_s{si}" in g:
        w = g[f"W_s{si}"]
        m, s = W.weight_stats64(w)
        np.testing.assert_allclose(m, g[f"m_s{si}"], rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(s, g[f"s_s{si}"], rtol=2e-6)
        for k in (2, 4, 8):
            dw = W.weight_quant_bwd64(g[f"g_s{si}"], w, m, s)
            ref = g[f"dW_s{si}_k{k}"].reshape(-1)
            np.testing.assert_allclose(dw, ref, atol=2e-5, rtol=1e-4)
        si += 1
    assert si >= 2


def test_statement_vs_reference_sgd():
    """G7, both steps: p, buf and the gradient left in p.grad at the bars of test_sgd_step_vs_reference"""
    g = load_golden("g7_sgd_step")
    bitW, lam, lam2 = int(g["bitW"]), float(g["lam"]), float(g["lam2"])
    for i in range(3):
        p, buf = g[f"p{i}_0"], None
        for step in (1, 2):
            p64, d64, b64 = W.sgd_step64(p, g[f"grad{i}_{step}"], buf, 0.04, 0.9, 0.0, 1e-4, 0, step == 1)
            if i == 1:
                d64 = W.sgd_grad_approx64(d64, g["w_cdf"], g["w_pdf"], bitW, lam, lam2)
            np.testing.assert_allclose(p64, g[f"p{i}_{step}"].reshape(-1), atol=1e-6)
            np.testing.assert_allclose(b64, g[f"buf{i}_{step}"].reshape(-1), atol=1e-6, rtol=1e-6)
            np.testing.assert_allclose(d64, g[f"gradout{i}_{step}"].reshape(-1), atol=1e-5, rtol=1e-5)
            p, buf = g[f"p{i}_{step}"], g[f"buf{i}_{step}"]      # the reference's own float32 state carries the next step


# ------------------------------------------------------------------------------------------------ the C oracle, every GPU shape
@pytest.mark.parametrize("name", list(FWD_CASES))
def test_statement_vs_c_oracle_weights(name):
    """weight statistics at the bar of check 1 (this is also the confirmation that the C oracle's own weight_stats meets that
    bar at the stress statistics of case i and the long filters of case g: measured 6e-8 relative, float32 rounding of the
    result, so the bar is not widened anywhere), and the backward at the GPU test's bar for both gradient scales."""
    for t, w in enumerate(filters(name)):
        m64, s64 = W.weight_stats64(w)
        ms = O.weight_stats(w)
        assert abs(ms[0] - m64) <= 2e-6 * abs(m64) + 1e-9 and abs(ms[1] - s64) <= 2e-6 * s64, (name, t, ms, m64, s64)
        if name in BWD_CASES:
            for scale in G_SCALES:
                g = upstream(name, scale)[t]
                ref = W.weight_quant_bwd64(g, w, ms[0], ms[1])
                err = np.abs(O.weight_quant_bwd(g, w, ms) - ref)
                assert np.all(err <= bwd_tol(ref, np.abs(g).max())), (name, t, scale, err.max())


@pytest.mark.parametrize("n", CDF_BWD_SHAPES)
def test_cdf_backward_statement_vs_float64_autograd(n):
    """cdf_bwd64 against torch's float64 autograd of Normal(m, s).cdf / log_prob (what the reference's cdf module is made of),
    for both values of kc the trees use"""
    x, ms, gc, gp = cdf_bwd_inputs(n, 1.0)
    for kc in (1.0, 2.0):
        xt = torch.from_numpy(x).double().requires_grad_(True)
        m = torch.tensor(float(ms[0]), dtype=torch.float64, requires_grad=True)
        s = torch.tensor(float(ms[1]), dtype=torch.float64, requires_grad=True)
        nd = torch.distributions.Normal(m, s)
        c, pdf = kc * nd.cdf(xt) - (kc - 1.0), torch.exp(nd.log_prob(xt)) * 2
        torch.autograd.backward([c, pdf], [torch.from_numpy(gc).double(), torch.from_numpy(gp).double()])
        dx, dms = W.cdf_bwd64(gc, gp, x, ms[0], ms[1], kc)
        np.testing.assert_allclose(dx, xt.grad.numpy(), rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(dms, [float(m.grad), float(s.grad)], rtol=1e-9, atol=1e-7)


@pytest.mark.parametrize("hyper", SGD_HYPER)
@pytest.mark.parametrize("lname", list(SGD_LISTS) + ["admm"])
def test_statement_vs_c_oracle_sgd(lname, hyper):
    """two steps of the float32 C oracle against the float64 statement on the same inputs.  The kernels' bar for p, buf and dir
    (sgd_bar) is DEFINED by the oracle's error, so the oracle meets it by construction; what is checked here instead is that the
    yardstick itself is sound: the oracle rounds at most four times on the way to any output (d, buf * mom, (1 - damp) * d and
    their sum; one product and one sum more for p and a nesterov direction), each time by half an ulp of a value no larger than
    the output's largest magnitude times two, so four ulps bound its error.  The rewritten gradient is compared at the GPU
    test's bar."""
    lr, mom, damp, wd, nest = hyper
    sizes = ADMM_LIST if lname == "admm" else SGD_LISTS[lname]
    for t, (p, gs, cdf, pdf) in enumerate(sgd_inputs(sizes, _seed(lname))):
        buf = None
        for step in (0, 1):
            p64, d64, b64 = W.sgd_step64(p, gs[step], buf, lr, mom, damp, wd, nest, step == 0)
            po, do, bo = O.sgd_step(p, gs[step], buf, lr, mom, damp, wd, nest, step == 0)
            assert np.max(np.abs(po - p64)) <= 4 * ulp(p64) and np.max(np.abs(do - d64)) <= 4 * ulp(d64)
            if mom != 0.0:
                assert np.max(np.abs(bo - b64)) <= 4 * ulp(b64)
            if cdf is not None:
                for bitW in (2, 4, 8):
                    ref = W.sgd_grad_approx64(do, cdf, pdf, bitW, LAM, LAM2)
                    err = np.abs(O.sgd_grad_approx(do, cdf, pdf, bitW, LAM, LAM2) - ref)
                    assert np.all(err <= grad_tol(ref, do.astype(np.float64), pdf)), (lname, t, bitW, err.max())
            p, buf = po, (bo if mom != 0.0 else None)


# ------------------------------------------------------------------------------------------------ mutations
def _exceeds(mutant, ref, tol):
    return bool(np.any(np.abs(np.asarray(mutant) - np.asarray(ref)) > 10.0 * tol))


def test_the_bars_see_a_wrong_divisor_in_the_dot_term():
    """n for n - 1 under sum(g P z): the two differ by z S / (n (n - 1)), which at n = 432 is below ten times the bar's relative
    part for most elements, so the shape is case b's 16-element filter, where it is 0.4 % of z S."""
    w, g = filters("b")[2], upstream("b", 1.0)[2]
    m, s = W.weight_stats64(w)
    ref = W.weight_quant_bwd64(g, w, m, s)
    z = (w.astype(np.float64) - m) / s
    gp = g * 2.0 / (s * W.SQRT_2PI) * np.exp(-0.5 * z * z)
    mutant = gp - gp.sum() / w.size - z * (gp * z).sum() / w.size
    assert _exceeds(mutant, ref, bwd_tol(ref, np.abs(g).max()))
    for scale in G_SCALES:                       # ... at either gradient scale (the bar scales with it)
        gs = upstream("b", scale)[2]
        r2 = W.weight_quant_bwd64(gs, w, m, s)
        gp2 = gs * 2.0 / (s * W.SQRT_2PI) * np.exp(-0.5 * z * z)
        assert _exceeds(gp2 - gp2.sum() / w.size - z * (gp2 * z).sum() / w.size, r2, bwd_tol(r2, np.abs(gs).max()))


def test_the_bars_see_a_biased_variance():
    w = filters("a432")[0].astype(np.float64)
    _, s = W.weight_stats64(w)
    assert abs(np.std(w) - s) > 10.0 * 2e-6 * s          # std with ddof = 0: smaller by 1 / (2 n) = 1.2e-3 relative at n = 432


def _sgd_case():
    (p, gs, _, _), = sgd_inputs([432], 5)
    buf = (1e-2 * np.random.default_rng(6).standard_normal(432)).astype(np.float32)
    return p, gs[0], buf


def test_the_bars_see_a_nesterov_direction_without_nesterov():
    p, g, buf = _sgd_case()
    lr, mom, damp, wd, _ = SGD_HYPER[0]
    p64, d64, b64 = W.sgd_step64(p, g, buf, lr, mom, damp, wd, 0, False)
    o = O.sgd_step(p, g, buf, lr, mom, damp, wd, 0, False)
    pm, dm, _ = W.sgd_step64(p, g, buf, lr, mom, damp, wd, 1, False)      # dir = d + mom b where b was meant
    assert _exceeds(dm, d64, sgd_bar(o[1], d64)) and _exceeds(pm, p64, sgd_bar(o[0], p64))


def test_the_bars_see_a_dropped_dampening():
    p, g, buf = _sgd_case()
    lr, mom, damp, wd, _ = SGD_HYPER[3]
    p64, d64, b64 = W.sgd_step64(p, g, buf, lr, mom, damp, wd, 0, False)
    o = O.sgd_step(p, g, buf, lr, mom, damp, wd, 0, False)
    pm, dm, bm = W.sgd_step64(p, g, buf, lr, mom, 0.0, wd, 0, False)
    assert _exceeds(bm, b64, sgd_bar(o[2], b64)) and _exceeds(pm, p64, sgd_bar(o[0], p64))


@pytest.mark.parametrize("bitW", [2, 4, 8])
def test_the_bars_see_a_wrong_level_count(bitW):
    """nlev = 2^k for 2^k - 1 in transform(): the fractional part moves by c + 0.5"""
    (p, gs, cdf, pdf), = sgd_inputs([432], 5)
    d = gs[0].astype(np.float64)
    ref = W.sgd_grad_approx64(d, cdf, pdf, bitW, LAM, LAM2)
    a = (cdf.astype(np.float64) + 0.5) * float(1 << bitW)
    sg = 1.0 / (1.0 + np.exp(-((a - np.floor(a)) * LAM2 * 2.0)))
    assert _exceeds(d * (sg * (1.0 - sg) * LAM) * pdf, ref, grad_tol(ref, d, pdf))
