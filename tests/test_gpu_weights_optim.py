"""The weight quantiser (csrc/multi_tensor_kernels.hip: fused, two-launch and per-tensor forms; csrc/quant_kernels.hip), the
stand-alone cdf backward and the SGD step (three launchers, csrc/admm_sgd_kernels.hip) against the float64 statement of
tests/weights_oracle.py, at every launch form, chunk boundary, block cap and pass count named in tests/test_weights_cpu.py's
case tables (which pin that statement to the reference's data on the CPU).  Reference ops: weight_quantize_fn.forward
(model/quantization.py:71-85), cdf (:41-59) and SGD.step (utils/optimizer.py:212-255).

Every tensor a kernel writes is a window into an arena filled with a NaN bit pattern, at least 64 elements from its neighbours:
an element the kernel skips stays NaN and fails the comparison, an element written outside a window breaks the pattern."""
import numpy as np
import pytest
import torch

from tests import oracle_c as O
from tests import test_weights_cpu as C
from tests import weights_oracle as W

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC05A5A         # a quiet NaN no kernel here produces
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class Arena:
    """windows of the given sizes in one sentinel-filled device buffer; window starts sit `misalign` elements past a 16-byte
    boundary"""

    def __init__(self, dev, sizes, misalign=0):
        self.offs, off = [], 0
        for n in sizes:
            off = (off + GUARD + 3) // 4 * 4 + misalign
            self.offs.append(off)
            off += n
        self.sizes, self.total = list(sizes), off + GUARD
        self.inside = np.zeros(self.total, bool)
        for o, n in zip(self.offs, self.sizes):
            self.inside[o:o + n] = True
        self.buf = torch.full((self.total,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[o:o + n] for o, n in zip(self.offs, self.sizes)]

    def reset(self):
        self.buf.view(torch.int32).fill_(SENTINEL)

    def put(self, arrays):
        host = np.full(self.total, SENTINEL, np.uint32).view(np.float32)
        for o, n, a in zip(self.offs, self.sizes, arrays):
            host[o:o + n] = a.reshape(-1)
        self.buf.copy_(torch.from_numpy(host))

    def get(self):
        """the windows' contents; asserts that everything outside them still holds the sentinel bit for bit"""
        host = self.buf.cpu().numpy()
        assert np.all(host.view(np.uint32)[~self.inside] == SENTINEL), "a kernel wrote outside its tensor"
        return [host[o:o + n].copy() for o, n in zip(self.offs, self.sizes)]


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def done(rc, what):
    """every launch: return code, then synchronise (raises on a device error) before anything else is enqueued"""
    from alignq_amd import _lib as L
    L.check(rc, what)
    torch.cuda.synchronize()


def byte_ws(dev, nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


# ------------------------------------------------------------------------------------------------ weight forward
class FwdRig:
    def __init__(self, dev, name):
        from alignq_amd import _lib as L
        self.L, self.lib, self.dev = L, L.load(), dev
        self.sizes, _, mis = C.FWD_CASES[name]
        self.T = len(self.sizes)
        self.w_host = C.filters(name)
        self.w = Arena(dev, self.sizes, misalign=mis)
        self.w.put(self.w_host)
        assert all(v.data_ptr() % 16 == 4 * mis for v in self.w.views)
        self.q, self.c, self.pdf = (Arena(dev, self.sizes) for _ in range(3))
        self.ms = Arena(dev, [2 * self.T])
        self.ws = byte_ws(dev, self.lib.alignq_weight_multi_ws_bytes(self.T))

    def run(self, k, formula):
        L = self.L
        for a in (self.q, self.c, self.pdf, self.ms):
            a.reset()
        done(self.lib.alignq_weight_quant_fwd_multi(self.T, L.ptr_array(self.w.views), L.ptr_array(self.q.views),
                                                    L.ptr_array(self.c.views), L.ptr_array(self.pdf.views), L.i64_array(self.sizes),
                                                    L.ptr(self.ms.views[0]), k, formula, L.ptr(self.ws), L.stream_ptr()),
             "alignq_weight_quant_fwd_multi")
        return self.q.get(), self.c.get(), self.pdf.get(), self.ms.get()[0].reshape(self.T, 2)


@pytest.mark.parametrize("name", list(C.FWD_CASES))
def test_weight_forward_every_launch_form_vs_float64_and_oracle(dev, name):
    """alignq_weight_quant_fwd_multi, k in {2, 4, 8}, both formulas: (m, s) against the two-pass float64 statistics at
    test_weight_quant's bar (unwidened for the stress statistics of case i: tests/test_weights_cpu.py shows the C oracle meets
    it there with 6e-8), W_q and cdf bit-equal to the C oracle evaluated at the DEVICE's (m, s), pdf at the existing bar; the
    per-tensor entry points give the same bits (cases a, c, d, g); the misaligned filter of case f gives case a's."""
    from alignq_amd import ops
    rig = FwdRig(dev, name)
    twin = FwdRig(dev, "a432") if name == "f" else None
    for formula in (0, 1):
        for k in (2, 4, 8):
            q, c, pdf, ms = rig.run(k, formula)
            for t, w in enumerate(rig.w_host):
                m64, s64 = W.weight_stats64(w)
                assert abs(ms[t, 0] - m64) <= 2e-6 * abs(m64) + 1e-9 and abs(ms[t, 1] - s64) <= 2e-6 * s64, (t, ms[t], m64, s64)
                oq, oc, opdf, _ = O.weight_quant_fwd(w, ms[t], k, formula)
                assert bits_equal(q[t], oq) and bits_equal(c[t], oc), (name, k, formula, t)
                np.testing.assert_allclose(pdf[t], opdf, rtol=1e-6, atol=1e-7)
                if name in C.PER_TENSOR_CASES:
                    ms1 = ops.weight_stats(rig.w.views[t])
                    torch.cuda.synchronize()
                    q1, c1, _, _ = ops.weight_quant_given_stats(rig.w.views[t], ms1, k, formula)
                    torch.cuda.synchronize()
                    assert bits_equal(ms1.cpu().numpy(), ms[t]), (name, t, ms1, ms[t])
                    assert bits_equal(q1.cpu().numpy(), q[t]) and bits_equal(c1.cpu().numpy(), c[t])
            if twin is not None:
                qa, ca, pa, msa = twin.run(k, formula)
                assert bits_equal(msa, ms) and bits_equal(qa[0], q[0]) and bits_equal(ca[0], c[0]) and bits_equal(pa[0], pdf[0])


# ------------------------------------------------------------------------------------------------ weight backward
@pytest.mark.parametrize("scale", C.G_SCALES)
@pytest.mark.parametrize("name", C.BWD_CASES)
def test_weight_backward_multi_and_per_tensor_vs_float64(dev, name, scale, record_property):
    """alignq_weight_quant_bwd_multi and alignq_weight_quant_bwd against weight_quant_bwd64 at the device's own (m, s):
    atol 2e-5 max|g|, rtol 1e-4 (G2's dW bar scaled by the gradient's size)"""
    rig = FwdRig(dev, name)
    L, lib = rig.L, rig.lib
    _, _, _, ms = rig.run(4, 0)
    g_host = C.upstream(name, scale)
    g = Arena(dev, rig.sizes)
    g.put(g_host)
    dw, dw1 = Arena(dev, rig.sizes), Arena(dev, rig.sizes)
    done(lib.alignq_weight_quant_bwd_multi(rig.T, L.ptr_array(g.views), L.ptr_array(rig.w.views), L.ptr(rig.ms.views[0]),
                                           L.ptr_array(dw.views), L.i64_array(rig.sizes), L.ptr(rig.ws), L.stream_ptr()),
         "alignq_weight_quant_bwd_multi")
    ws1 = byte_ws(dev, lib.alignq_weight_ws_bytes(max(rig.sizes)))
    for t, n in enumerate(rig.sizes):
        done(lib.alignq_weight_quant_bwd(L.ptr(g.views[t]), L.ptr(rig.w.views[t]), rig.ms.views[0][2 * t:].data_ptr(),
                                         L.ptr(dw1.views[t]), n, L.ptr(ws1), L.stream_ptr()), "alignq_weight_quant_bwd")
    worst = 0.0
    for what, out in (("multi", dw.get()), ("per-tensor", dw1.get())):
        for t, (w, gt) in enumerate(zip(rig.w_host, g_host)):
            ref = W.weight_quant_bwd64(gt, w, ms[t, 0], ms[t, 1])
            gmax = float(np.abs(gt).max())
            err = np.abs(out[t] - ref)
            worst = max(worst, float(err.max()) / gmax)
            assert np.all(err <= C.bwd_tol(ref, gmax)), (what, name, t, float(err.max()), gmax)
    record_property("max_abs_err_over_max_g", worst)
    print("weight backward", name, scale, "max |dW - dW64| / max|g| =", worst)


@pytest.mark.parametrize("scale", C.G_SCALES)
@pytest.mark.parametrize("n", C.CDF_BWD_SHAPES)
def test_cdf_backward_vs_float64(dev, n, scale, record_property):
    """alignq_cdf_bwd: dx at the weight backward's bar; dm and ds are sums over n terms, their absolute part scales by sqrt(n)"""
    from alignq_amd import _lib as L
    lib = L.load()
    x, ms, gc, gp = C.cdf_bwd_inputs(n, scale)
    ins = Arena(dev, [n, n, n, 2])
    ins.put([x, gc, gp, ms])
    xd, gcd, gpd, msd = ins.views
    dx, dms = Arena(dev, [n]), Arena(dev, [2])
    ws = byte_ws(dev, lib.alignq_weight_ws_bytes(n))
    gmax = float(max(np.abs(gc).max(), np.abs(gp).max()))
    worst = 0.0
    for kc in (1.0, 2.0):
        for with_gp in (True, False):
            dx.reset(); dms.reset()
            done(lib.alignq_cdf_bwd(L.ptr(gcd), L.ptr(gpd) if with_gp else None, L.ptr(xd), L.ptr(msd), kc, L.ptr(dx.views[0]),
                                    L.ptr(dms.views[0]), n, L.ptr(ws), L.stream_ptr()), "alignq_cdf_bwd")
            rdx, rdms = W.cdf_bwd64(gc, gp if with_gp else None, x, ms[0], ms[1], kc)
            err = np.abs(dx.get()[0] - rdx)
            worst = max(worst, float(err.max()) / gmax)
            assert np.all(err <= C.bwd_tol(rdx, gmax)), (kc, with_gp, float(err.max()))
            errs = np.abs(dms.get()[0] - rdms)
            assert np.all(errs <= C.bwd_tol(rdms, gmax, np.sqrt(n))), (kc, with_gp, errs, rdms)
    record_property("max_abs_err_over_max_g", worst)
    print("cdf backward", n, scale, "max |dx - dx64| / max|g| =", worst)


# ------------------------------------------------------------------------------------------------ SGD
class SgdRig:
    """device state of one parameter list: p, g, buf in guarded arenas, (w_cdf, w_pdf) for every second tensor"""

    def __init__(self, dev, sizes, seed):
        from alignq_amd import _lib as L
        self.L, self.lib, self.dev, self.sizes, self.T = L, L.load(), dev, list(sizes), len(sizes)
        self.inputs = C.sgd_inputs(sizes, seed)
        self.p, self.g, self.buf, self.gout = (Arena(dev, sizes) for _ in range(4))
        self.has = [c is not None for _, _, c, _ in self.inputs]
        aux_sizes = [n for n, h in zip(sizes, self.has) if h]
        self.cdf_a, self.pdf_a = Arena(dev, aux_sizes), Arena(dev, aux_sizes)
        self.cdf_a.put([c for _, _, c, _ in self.inputs if c is not None])
        self.pdf_a.put([f for _, _, _, f in self.inputs if f is not None])
        ci, fi = iter(self.cdf_a.views), iter(self.pdf_a.views)
        self.cdf = [next(ci) if h else None for h in self.has]
        self.pdf = [next(fi) if h else None for h in self.has]
        self.p_host = [p for p, _, _, _ in self.inputs]
        self.buf_host = [np.full(n, np.nan, np.float32) for n in sizes]       # poison: a first step must not read it
        self.p.put(self.p_host)
        self.buf.put(self.buf_host)

    def prefix(self, hyper, firsts, bitW):
        L = self.L
        lr, mom, damp, wd, nest = hyper
        return (self.T, L.ptr_array(self.p.views), L.ptr_array(self.g.views), L.ptr_array(self.buf.views) if mom != 0 else None,
                L.i64_array(self.sizes), L.ptr_array(self.cdf), L.ptr_array(self.pdf), L.i32_array(firsts), lr, mom, damp, wd, nest,
                bitW, C.LAM, C.LAM2)

    def launch_multi(self, hyper, firsts, bitW):
        done(self.lib.alignq_sgd_step_multi(*self.prefix(hyper, firsts, bitW), self.L.stream_ptr()), "alignq_sgd_step_multi")

    def launch_per_tensor(self, hyper, firsts, bitW):
        L, lib = self.L, self.lib
        lr, mom, damp, wd, nest = hyper
        for t, n in enumerate(self.sizes):
            done(lib.alignq_sgd_step(L.ptr(self.p.views[t]), L.ptr(self.g.views[t]), L.ptr(self.buf.views[t]) if mom != 0 else None, n,
                                     lr, mom, damp, wd, nest, int(firsts[t]), L.stream_ptr()), "alignq_sgd_step")
            if self.has[t]:
                done(lib.alignq_sgd_grad_approx(L.ptr(self.g.views[t]), L.ptr(self.cdf[t]), L.ptr(self.pdf[t]), L.ptr(self.gout.views[t]),
                                                n, bitW, C.LAM, C.LAM2, L.stream_ptr()), "alignq_sgd_grad_approx")
                self.g.views[t].copy_(self.gout.views[t])
                torch.cuda.synchronize()

    def step(self, launch, step, hyper, firsts, bitW, record=None):
        """one step from the device's current state: launches, reads p / g / buf back (guards checked) and compares each tensor
        with sgd_step64 / sgd_grad_approx64 of the float32 state the kernel started from"""
        lr, mom, damp, wd, nest = hyper
        g_host = [gs[step] for _, gs, _, _ in self.inputs]
        self.g.put(g_host)
        for t, f in enumerate(firsts):
            if f:
                self.buf_host[t] = np.full(self.sizes[t], np.nan, np.float32)
        self.buf.put(self.buf_host)
        launch(hyper, firsts, bitW)
        p_out, g_out, b_out = self.p.get(), self.g.get(), self.buf.get()
        self.gout.get()
        for t in range(self.T):
            first = bool(firsts[t])
            b_in = None if (first or mom == 0) else self.buf_host[t]
            p64, d64, b64 = W.sgd_step64(self.p_host[t], g_host[t], b_in, lr, mom, damp, wd, nest, first)
            po, do, bo = O.sgd_step(self.p_host[t], g_host[t], b_in, lr, mom, damp, wd, nest, first)
            ctx = (t, self.sizes[t], step, hyper, first)
            assert np.max(np.abs(p_out[t] - p64)) <= C.sgd_bar(po, p64), ("p",) + ctx
            if mom != 0:
                assert np.max(np.abs(b_out[t] - b64)) <= C.sgd_bar(bo, b64), ("buf",) + ctx
            else:
                assert np.all(np.isnan(b_out[t]))           # no buffer pointer went in: the poison is untouched
            if not self.has[t]:
                assert np.max(np.abs(g_out[t] - d64)) <= C.sgd_bar(do, d64), ("dir",) + ctx
            else:
                ref = W.sgd_grad_approx64(d64, self.inputs[t][2], self.inputs[t][3], bitW, C.LAM, C.LAM2)
                tol = C.grad_tol(ref, d64, self.inputs[t][3])
                err = np.abs(g_out[t] - ref)
                if record is not None:
                    record.append(float(np.max(err / tol)))
                assert np.all(err <= tol), ("grad",) + ctx + (float(err.max()),)
        self.p_host, self.buf_host = p_out, (b_out if mom != 0 else self.buf_host)
        return p_out, g_out, b_out


def three_steps(rig, launch, hyper, bitW, record=None):
    """first = 1 everywhere on poisoned buffers, a second step on the live ones, then `first` mixed within one call"""
    out = [rig.step(launch, 0, hyper, [1] * rig.T, bitW, record), rig.step(launch, 1, hyper, [0] * rig.T, bitW, record),
           rig.step(launch, 2, hyper, [int(t % 3 == 0) for t in range(rig.T)], bitW, record)]
    return out


@pytest.mark.parametrize("hi", range(len(C.SGD_HYPER)))
@pytest.mark.parametrize("lname", list(C.SGD_LISTS))
def test_sgd_step_multi_vs_float64(dev, lname, hi, record_property):
    """alignq_sgd_step_multi: p, buf and dir within twice the float32 C oracle's own error against float64 (floor: one ulp of
    the tensor's largest magnitude), the rewritten gradient at G7's bar scaled by max|dir pdf|; lists cross the 72-parameter
    chunk once and twice and the 524288-element pass"""
    rig = SgdRig(dev, C.SGD_LISTS[lname], C._seed(lname))
    rec = []
    three_steps(rig, rig.launch_multi, C.SGD_HYPER[hi], (2, 4, 8)[hi % 3] if lname != "big" else 8, rec)
    record_property("max_grad_err_over_bar", max(rec))
    print("sgd", lname, C.SGD_HYPER[hi], "rewritten gradient: largest error / bar =", max(rec))


@pytest.mark.parametrize("n", [432, C.FUSED_MAX, C.PASS + 1000])
def test_gradient_rewrite_with_arbitrary_cdf_at_the_float32_level_position(dev, n):
    """The lists above keep w_cdf on the 2^-12 grid (tests/test_weights_cpu.py: sgd_inputs), where `% 1` has no tie zone.  Here
    w_cdf is the quantiser's own, arbitrary, output, and the float64 reference takes `% 1` of the FLOAT32 a = (c + 0.5) nlev (the
    library is built without multiply-add contraction, so that is the value the kernels have); everything after it is float64.
    alignq_sgd_grad_approx and alignq_sgd_step_multi (lr only: dir = g) at G7's bar, and bit-equal to each other."""
    from alignq_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(n + 1)
    w = (C.MS[0] + C.MS[1] * rng.standard_normal(n)).astype(np.float32)
    g = (1e-2 * rng.standard_normal(n)).astype(np.float32)
    _, cdf, pdf, _ = O.weight_quant_fwd(w, np.array(C.MS, np.float32), 32, O.FORMULA_ADMM)
    ins = Arena(dev, [n, n, n])
    ins.put([g, cdf, pdf])
    gd, cd, fd = ins.views
    out, p, gm = Arena(dev, [n]), Arena(dev, [n]), Arena(dev, [n])
    for bitW in (2, 4, 8):
        out.reset()
        done(lib.alignq_sgd_grad_approx(L.ptr(gd), L.ptr(cd), L.ptr(fd), L.ptr(out.views[0]), n, bitW, C.LAM, C.LAM2, L.stream_ptr()),
             "alignq_sgd_grad_approx")
        p.put([w]); gm.put([g])
        done(lib.alignq_sgd_step_multi(1, L.ptr_array(p.views), L.ptr_array(gm.views), None, L.i64_array([n]), L.ptr_array([cd]),
                                       L.ptr_array([fd]), L.i32_array([0]), 0.1, 0.0, 0.0, 0.0, 0, bitW, C.LAM, C.LAM2, L.stream_ptr()),
             "alignq_sgd_step_multi")
        a32 = (cdf + np.float32(0.5)) * np.float32((1 << bitW) - 1)
        ref = W.sgd_grad_approx64(g, cdf, pdf, bitW, C.LAM, C.LAM2, a=a32)
        got, got_m = out.get()[0], gm.get()[0]
        p.get()
        assert np.all(np.abs(got - ref) <= C.grad_tol(ref, g.astype(np.float64), pdf)), (bitW, float(np.abs(got - ref).max()))
        assert bits_equal(got, got_m)
    assert all(bits_equal(a, b) for a, b in zip(ins.get(), [g, cdf, pdf]))


@pytest.mark.parametrize("hi", range(len(C.SGD_HYPER)))
def test_sgd_three_launchers_agree_bit_for_bit(dev, hi):
    """alignq_sgd_step_multi, alignq_sgd_admm_step_multi (SGD role) and alignq_sgd_step + alignq_sgd_grad_approx: one arithmetic"""
    hyper, bitW = C.SGD_HYPER[hi], (8, 4, 2)[hi % 3]
    results = []
    for which in ("multi", "admm", "per_tensor"):
        rig = SgdRig(dev, C.SGD_LISTS["six"], C._seed("six"))
        if which == "admm":
            site = Arena(dev, [64, 64, 64])
            site.put([np.linspace(-0.1, 0.1, 64, dtype=np.float32)] * 3)
            D, A, G = site.views

            def launch(hyper, firsts, bitW, rig=rig, D=D, A=A, G=G):
                L = rig.L
                done(rig.lib.alignq_sgd_admm_step_multi(*rig.prefix(hyper, firsts, bitW), 1, L.ptr_array([D]), L.ptr_array([A]),
                                                        L.ptr_array([G]), 8, 8, 0.2, 0.3, L.stream_ptr()), "alignq_sgd_admm_step_multi")
        else:
            launch = rig.launch_multi if which == "multi" else rig.launch_per_tensor
        results.append(three_steps(rig, launch, hyper, bitW))
    for other in results[1:]:
        for s0, s1 in zip(results[0], other):
            for a0, a1 in zip(s0, s1):            # p, g, buf
                assert all(bits_equal(x, y) for x, y in zip(a0, a1))


@pytest.mark.parametrize("hi", range(len(C.SGD_HYPER)))
def test_sgd_admm_step_multi_both_roles(dev, hi):
    """alignq_sgd_admm_step_multi with 6 parameters (one a single element past one pass of its 1024-thread stride) and 2 sites
    of dim = b = 8: the SGD role as above, the site role against the oracle's ADMM update at test_admm_loss_and_update's bar"""
    hyper, mu, rho = C.SGD_HYPER[hi], 0.2, 0.3
    rig = SgdRig(dev, C.ADMM_LIST, C._seed("admm"))
    rng = np.random.default_rng(hi)
    sites = [[(0.1 * rng.standard_normal(64)).astype(np.float32) for _ in range(3)] for _ in range(2)]
    Da, Aa, Ga = (Arena(dev, [64, 64]) for _ in range(3))
    for arena, j in ((Da, 0), (Aa, 1), (Ga, 2)):
        arena.put([s_[j] for s_ in sites])

    def launch(hyper, firsts, bitW):
        L = rig.L
        done(rig.lib.alignq_sgd_admm_step_multi(*rig.prefix(hyper, firsts, bitW), 2, L.ptr_array(Da.views), L.ptr_array(Aa.views),
                                                L.ptr_array(Ga.views), 8, 8, mu, rho, L.stream_ptr()), "alignq_sgd_admm_step_multi")

    for step in (0, 1):
        rig.step(launch, step, hyper, [1 - step] * rig.T, (4, 8, 2)[hi % 3])
        A_out, G_out = Aa.get(), Ga.get()
        assert all(bits_equal(d, s_[0]) for d, s_ in zip(Da.get(), sites))
        for i, (D, A, G) in enumerate(sites):
            oA, oG = O.admm_update(D.reshape(8, 8), A.reshape(8, 8), G.reshape(8, 8), mu, rho)
            np.testing.assert_allclose(A_out[i], oA.reshape(-1), atol=1e-5)
            np.testing.assert_allclose(G_out[i], oG.reshape(-1), atol=1e-5)
            sites[i] = [D, A_out[i], G_out[i]]


def test_optimizer_sgd_at_bitw_32_leaves_the_direction_in_grad(dev):
    """optimizer.SGD with config.args.bitW = 32: `idx` is ignored and p.grad leaves as dir for every tensor"""
    from alignq_amd import config
    from alignq_amd.optimizer import SGD
    lr, mom, damp, wd, nest = C.SGD_HYPER[0]
    inputs = C.sgd_inputs([10, 432, C.FUSED_MAX], 32)
    ps = [torch.nn.Parameter(torch.from_numpy(p).to(dev)) for p, _, _, _ in inputs]
    cdf, pdf = torch.from_numpy(inputs[0][2]).to(dev), torch.from_numpy(inputs[0][3]).to(dev)
    p_host, b_host = [p for p, _, _, _ in inputs], [None] * 3
    config.args.bitW = 32
    try:
        opt = SGD(ps, lr=lr, momentum=mom, weight_decay=wd)
        for step in (0, 1):
            for p, (_, gs, _, _) in zip(ps, inputs):
                p.grad = torch.from_numpy(gs[step]).to(dev)
            opt.step([0], [cdf], [pdf], C.LAM, C.LAM2)
            torch.cuda.synchronize()
            for t, p in enumerate(ps):
                p64, d64, b64 = W.sgd_step64(p_host[t], inputs[t][1][step], b_host[t], lr, mom, damp, wd, nest, step == 0)
                po, do, bo = O.sgd_step(p_host[t], inputs[t][1][step], b_host[t], lr, mom, damp, wd, nest, step == 0)
                got_p, got_d = p.detach().cpu().numpy(), p.grad.cpu().numpy()
                got_b = opt.state[p]["momentum_buffer"].cpu().numpy()
                assert np.max(np.abs(got_p - p64)) <= C.sgd_bar(po, p64)
                assert np.max(np.abs(got_d - d64)) <= C.sgd_bar(do, d64)
                assert np.max(np.abs(got_b - b64)) <= C.sgd_bar(bo, b64)
                p_host[t], b_host[t] = got_p, got_b
    finally:
        config.args.bitW = 8
