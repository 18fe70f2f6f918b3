"""The ADMM site's FORWARD by value at its own scale, in every launch form, through the C ABI.

The other site tests compare D with the C oracle at atol 1e-5 (0.2 % .. 1 % of D's rms at the sizes they run), never compare `stats`
with anything and check one element of `scal`.  Here, per row of tests/site_fwd_oracle.py's matrix (one row per instantiation of
site1_kernels.hip, site_kernels.hip, site4_kernels.hip and the blocked Gram of corr_large_kernels.hip, at the smallest shape that
selects it; the CPU test pins which form a shape selects):

    x_q (and the level indices)  bit for bit against the C oracle
    stats [4][F]                 at the bars derived from u = 2^-24 and the kernels' operation counts (S.stats_bars); a constant
                                 column at eps > 0: mean exactly the value, 1/(std + eps) exactly 1/eps
    D                            from alignq_site_fwd and from alignq_site_partials + alignq_site_reduce_loss: the same bits; against
                                 float64 at BAR * s_ij (S.d_bar: BAR_SPLIT = 1.15e-4, BAR_FP32 = 3.2e-6 of the root-sum-square of
                                 the added terms); D == D^T bit for bit where the source promises a mirrored store
    scal [4]                     at D's bar pushed through the loss (S.scal_bars)

Every output lies in a NaN-filled window between sentinel guards (tests/test_gpu_dwconv.py's Arena; the workspace is excluded):
every window fully written, nothing outside touched, and a second launch gives the same bits.  Each check prints its worst
error / bar before asserting.  Then the folded batch-norm forms, alignq_corr_fwd, the multi-site reduction, the filler and twin
launches against the stand-alone ones, and a captured partials -> reduce_loss chain per geometry class.

Found by this file: alignq_corr_fwd at [128, 32832] "G differs on the second launch" - the corr-only instantiation of the
512-thread looped forward was not reproducible (6 of 119 repeated launches; NOTES.md); launch_fwd4_tf no longer launches it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import bn_oracle as N
from tests import oracle_c as O
from tests import site_fwd_oracle as S
from tests import site_grad_oracle as G
from tests.test_gpu_bench_path import _expected_y
from tests.test_gpu_dwconv import SENTINEL, Arena

pytestmark = pytest.mark.gpu
R, K, MU, RHO = S.R, S.K, S.MU, S.RHO
DIM = 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits_equal(a, b):
    return np.array_equal(bits(a), bits(b))


def offset_by_4_bytes(a, dev):
    """the same values behind a base pointer that is 4 bytes off a 16-byte boundary"""
    buf = torch.empty(a.size + 4, device=dev)
    buf[1:1 + a.size] = cu(a.reshape(-1), dev)
    t = buf[1:1 + a.size]
    assert t.data_ptr() % 16 == 4
    return t


def windows(names, arena):
    """one run's windows by name; Arena.get asserts that nothing outside them was touched"""
    return dict(zip(names, arena.get()))


def assert_written_and_repeatable(tag, first, second):
    for n, w in first.items():
        assert not (bits(w) == SENTINEL).any(), f"{tag}: {n} not fully written"
        assert np.array_equal(bits(w), bits(second[n])), f"{tag}: {n} differs on the second launch"


# ------------------------------------------------------------------------------------------------ host references
class Host:
    """x [B,F] (fp32, in memory order) with everything the checks need, computed once"""

    def __init__(self, x, eps, const=None, k=K):
        self.x, self.eps, self.const, self.k = x, eps, const, k
        self.B, self.F = x.shape
        self.t = S.transform(x)
        self.xq, _, self.bins = O.act_quant_fwd(x, k, R, O.FORMULA_ADMM)
        self.ref = S.reference(x, self.t, eps)
        self.acc = S.acc_of(self.B)
        self.allow = S.cond_allowance(x, self.t, eps, self.acc)
        self.sbars, self.live = S.stats_bars(x, self.t, eps, self.acc)


@functools.lru_cache(maxsize=2)
def plain_host(B, F):
    x, eps, const = S.row_inputs(B, F)
    return Host(x, eps, const)


def check_stats(tag, h, stats, rows=4):
    st = np.asarray(stats, np.float64).reshape(rows, h.F)
    w = np.abs(st - h.ref["stats"][:rows])[:, h.live] / h.sbars[:rows][:, h.live]
    print(f"[site-fwd] {tag} stats: worst error / bar = " + " ".join(f"{v:.3f}" for v in w.max(1)))
    assert np.isfinite(st).all() and (w <= 1.0).all(), (tag, w.max(1))
    dead = ~h.live
    if dead.any():
        assert h.eps > 0, "a constant column at eps = 0 is outside the statement"
        raw = np.asarray(stats, np.float32).reshape(rows, h.F)
        for i in range(0, rows, 2):
            assert np.array_equal(raw[i][dead], (h.x if i == 0 else h.t)[0][dead]), f"{tag}: mean of a constant column"
            assert (raw[i + 1][dead] == S.const_rho(h.eps)).all(), f"{tag}: 1/(std + eps) of a constant column is not 1/eps"


def check_D(tag, name, h, D, half="s"):
    D = np.asarray(D, np.float32).reshape(h.B, h.B)
    ref = h.ref["D"] if half == "s" else h.ref["corr_x"]
    bar = S.d_bar(name, h.ref, h.allow) if half == "s" else S.corr_bar(name, h.ref, h.B, h.F)
    err = np.abs(D.astype(np.float64) - ref)
    print(f"[site-fwd] {tag} D: worst error / bar = {float((err / bar).max()):.3f} (|D - D64| max {err.max():.2e} = "
          f"{float((err / h.ref[half]).max()):.2e} s; rms D {np.sqrt((ref ** 2).mean()):.2e})")
    assert np.isfinite(D).all() and (err <= bar).all(), (tag, float((err / bar).max()))
    if name.startswith("fwd4"):                  # the packed triangle is mirrored by the reduction
        assert np.array_equal(bits(D), bits(D.T)), f"{tag}: D != D^T"
    elif name.startswith("large"):               # the blocked Gram mirrors the off-diagonal 128 x 128 blocks
        for i0 in range(0, h.B, 128):
            for j0 in range(i0 + 128, h.B, 128):
                assert np.array_equal(bits(D[i0:i0 + 128, j0:j0 + 128]), bits(D[j0:j0 + 128, i0:i0 + 128].T)), f"{tag}: block mirror"
    return bar


def check_scal(tag, h, bar, scal, A0, G0):
    ref = S.scal_reference(h.ref["D"], A0, G0)
    sb = S.scal_bars(h.ref["D"], bar, A0, G0)
    w = np.abs(np.asarray(scal, np.float64) - ref) / sb
    print(f"[site-fwd] {tag} scal: worst error / bar = " + " ".join(f"{v:.3f}" for v in w))
    assert (w <= 1.0).all(), (tag, w, ref, scal)


# ------------------------------------------------------------------------------------------------ the matrix, plain sites
@pytest.mark.parametrize("row", S.ROWS, ids=[S.row_id(r) for r in S.ROWS])
def test_plain_site_forward(dev, row):
    from alignq_amd import _lib as L
    lib, p, st = L.load(), L.ptr, L.stream_ptr()
    name, B, F, aligned = row
    h = plain_host(B, F)
    tag = S.row_id(row)
    xd = cu(h.x, dev) if aligned else offset_by_4_bytes(h.x, dev)
    chain = B <= 128                             # alignq_site_partials / _reduce_loss stop at 128 rows
    names = ["xq", "stats", "D"] + (["xq2", "stats2", "D2", "scal"] if chain else [])
    arena = Arena(dev, [B * F, 4 * F, B * B] + ([B * F, 4 * F, B * B, 4] if chain else []))
    ws = torch.empty(lib.alignq_site_ws_bytes(B, F), dtype=torch.uint8, device=dev)
    A0, G0 = G.admm_params(B, DIM, B + F)
    A, Gm = cu(A0, dev), cu(G0, dev)

    def run():
        arena.reset()
        v = dict(zip(names, arena.views))
        L.check(lib.alignq_site_fwd(p(xd), B, F, K, R, h.eps, p(v["xq"]), p(v["D"]), p(v["stats"]), p(ws), st), "alignq_site_fwd")
        if chain:
            L.check(lib.alignq_site_partials(p(xd), B, F, K, R, h.eps, p(v["xq2"]), p(v["stats2"]), p(ws), st), "alignq_site_partials")
            L.check(lib.alignq_site_reduce_loss(p(ws), B, F, p(v["D2"]), p(A), p(Gm), DIM, MU, RHO, p(v["scal"]), st),
                    "alignq_site_reduce_loss")
        torch.cuda.synchronize()
        return windows(names, arena)

    first = run()
    assert_written_and_repeatable(tag, first, run())
    assert np.array_equal(bits(first["xq"]), bits(h.xq.reshape(-1))), f"{tag}: x_q differs from the oracle"
    check_stats(tag, h, first["stats"])
    bar = check_D(tag, name, h, first["D"])
    if chain:
        for a, b in (("xq", "xq2"), ("stats", "stats2"), ("D", "D2")):
            assert np.array_equal(bits(first[a]), bits(first[b])), f"{tag}: {a} of alignq_site_fwd and of the two-launch chain differ"
        check_scal(tag, h, bar, first["scal"], A0, G0)


# ------------------------------------------------------------------------------------------------ alignq_corr_fwd (PAIR off)
CORR_ROWS = S.CORR_ROWS


@pytest.mark.parametrize("name,B,F", CORR_ROWS, ids=[f"{n}-{B}x{F}" for n, B, F in CORR_ROWS])
def test_corr_forward_at_the_x_half_of_the_scale(dev, name, B, F):
    """corr(x) alone against float64 at S.corr_bar: BAR * s_x plus, for a diagonal that no second Gram cancels, the fp32
    accumulation and the split forms' dropped lo * lo term at the size of the entry"""
    from alignq_amd import _lib as L
    lib, p, st = L.load(), L.ptr, L.stream_ptr()
    assert S.form(B, F, pair=False) == name
    h = plain_host(B, F)
    names = ["G", "stats"]
    arena = Arena(dev, [B * B, 2 * F])
    ws = torch.empty(lib.alignq_site_ws_bytes(B, F), dtype=torch.uint8, device=dev)
    xd = cu(h.x, dev)

    def run():
        arena.reset()
        v = dict(zip(names, arena.views))
        L.check(lib.alignq_corr_fwd(p(xd), B, F, h.eps, p(v["G"]), p(v["stats"]), p(ws), st), "alignq_corr_fwd")
        torch.cuda.synchronize()
        return windows(names, arena)

    first = run()
    tag = f"corr {name} {B}x{F}"
    assert_written_and_repeatable(tag, first, run())
    check_stats(tag, h, first["stats"], rows=2)
    check_D(tag, name, h, first["G"], half="s_x")


# ------------------------------------------------------------------------------------------------ 64 < B <= 128, folded batch-norm
class Fold:
    """alignq_site_partials_bn + alignq_site_reduce_loss on z [B,F] (memory order), every output in an arena window"""

    def __init__(self, dev, B, C, H, nhwc, zd, gamma, beta):
        from alignq_amd import _lib as L
        self.L, self.lib, self.dev = L, L.load(), dev
        self.B, self.C, self.HW, self.F, self.nhwc = B, C, H * H, C * H * H, nhwc
        self.zd, self.tg, self.tb = zd, cu(gamma, dev), cu(beta, dev)
        self.ws = torch.empty(self.lib.alignq_site_ws_bytes(B, self.F), dtype=torch.uint8, device=dev)
        self.A0, self.G0 = G.admm_params(B, DIM, B + C)
        self.A, self.Gm = cu(self.A0, dev), cu(self.G0, dev)

    def stats_part(self):
        L, lib, p = self.L, self.lib, self.L.ptr
        if self.nhwc:
            part = torch.empty(lib.alignq_bn_nhwc_ws_bytes(self.C), dtype=torch.uint8, device=self.dev)
            L.check(lib.alignq_bn_partial_stats_nhwc(p(self.zd), self.B, self.C, self.HW, p(part), L.stream_ptr()), "bn_partial_stats_nhwc")
        else:
            part = torch.empty(lib.alignq_bn_ws_bytes(self.C), dtype=torch.uint8, device=self.dev)
            L.check(lib.alignq_bn_partial_stats(p(self.zd), self.B, self.C, self.HW, p(part), L.stream_ptr()), "bn_partial_stats")
        return part

    def run(self, k, relu, res, ab=None, part=None, conv_parts=0, bins=False, eps=0.0):
        """two launches of the chain; returns the first run's windows (ab / save among them when the kernel finalises them)"""
        L, lib, p, dev = self.L, self.lib, self.L.ptr, self.dev
        B, C, F = self.B, self.C, self.F
        names, sizes = ["y", "stats", "D", "scal"], [B * F, 4 * F, B * B, 4]
        if ab is None:
            names, sizes = names + ["ab", "save"], sizes + [2 * C, 2 * C]
        nbytes = lib.alignq_bin_bytes(k, R, 0) if bins else 0
        if bins:
            names, sizes = names + ["bins"], sizes + [B * F * nbytes // 4]
        arena = Arena(dev, sizes)
        ab_in = None if ab is None else (cu(ab[0], dev), cu(ab[1], dev))

        def once():
            arena.reset()
            v = dict(zip(names, arena.views))
            abt, savet = (v["ab"], v["save"]) if ab is None else ab_in
            rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
            nbt = torch.zeros((), dtype=torch.int64, device=dev)
            L.check(lib.alignq_site_partials_bn(p(self.zd), p(part), p(self.tg), p(self.tb), p(rm), p(rv), p(nbt), 0.1, 1e-5, p(abt),
                                                p(savet), C, self.HW, B, F, k, R, eps, int(relu), p(res), int(self.nhwc),
                                                int(conv_parts), p(v["y"]), p(v.get("bins")), p(v["stats"]), p(self.ws),
                                                L.stream_ptr()), "alignq_site_partials_bn")
            L.check(lib.alignq_site_reduce_loss(p(self.ws), B, F, p(v["D"]), p(self.A), p(self.Gm), DIM, MU, RHO, p(v["scal"]),
                                                L.stream_ptr()), "alignq_site_reduce_loss")
            torch.cuda.synchronize()
            return windows(names, arena)

        first = once()
        assert_written_and_repeatable(f"fold {B}x{C} nhwc={self.nhwc} k={k}", first, once())
        first["bin_bytes"] = nbytes
        return first


def check_fold(tag, name, zm, C, nhwc, ab, out, k, relu, res, hosts):
    """one folded run against the restatement at x = a z + b with the (a, b) the launch used; hosts: cache by (a, b) bits"""
    x = O.bn_apply(zm, C, nhwc, ab)
    key = (ab.tobytes(), k)
    if key not in hosts:
        base = next((h for (kb, _), h in hosts.items() if kb == ab.tobytes()), None)
        if base is None:
            hosts[key] = Host(x, 0.0, None, k)
        else:                                    # D and stats do not depend on k: only x_q and the indices are re-formed
            h = Host.__new__(Host)
            h.__dict__.update(base.__dict__)
            h.k = k
            h.xq, _, h.bins = O.act_quant_fwd(x, k, R, O.FORMULA_ADMM)
            hosts[key] = h
    h = hosts[key]
    y_ref, bins_ref = _expected_y(x, k, R, res, relu)
    assert np.array_equal(bits(out["y"]), bits(y_ref.reshape(-1))), f"{tag}: y differs from the oracle"
    if "bins" in out:
        dt = {1: np.int8, 2: np.int16}[out["bin_bytes"]]
        got = out["bins"].view(dt).astype(np.int32)
        want = np.maximum(bins_ref, 0) if relu else bins_ref
        assert np.array_equal(got, want.reshape(-1)), f"{tag}: level indices differ from the oracle"
    check_stats(tag, h, out["stats"])
    bar = check_D(tag, name, h, out["D"])
    return h, bar


FOLD_SHAPES = tuple(G.BN4) + (S.FOLD_LOOP,)


@pytest.mark.parametrize("nhwc", [0, 1])
@pytest.mark.parametrize("B,C,H", FOLD_SHAPES, ids=["x".join(map(str, s)) for s in FOLD_SHAPES])
def test_folded_site_forward(dev, B, C, H, nhwc):
    """site_fwd4_kernel with the batch-norm fold, both layouts: (a, b) given with ReLU and a residual; finalised in the kernel
    from alignq_bn_partial_stats[_nhwc]; int8 (k = 4) and int16 (k = 8) level indices with the ReLU.  The looped row
    (128, 16, 48) runs the 1024-thread tile loop (576 tiles on 512 workgroups)."""
    F = C * H * H
    name = S.form(B, F, True)
    looped = (B, C, H) == S.FOLD_LOOP
    assert name == ("fwd4-loopNT" if looped else ("fwd4-32-full" if B == 128 else "fwd4-64"))
    zm, gamma, beta, _ = G.bn_inputs(B, C, H, seed=nhwc)
    rm_ = (np.random.default_rng(B + C + H + nhwc).standard_normal((B, F)) * 0.7).astype(np.float32)
    f = Fold(dev, B, C, H, nhwc, cu(zm, dev), gamma, beta)
    res = cu(rm_, dev)
    ab_o, save_o, _ = O.bn_fold_ab(zm, C, nhwc, gamma, beta, 1e-5)
    tag = f"fold {name} {B}x{C}x{H}x{H} nhwc={nhwc}"
    hosts = {}
    out = f.run(K, True, res, ab=(ab_o, save_o))
    h, bar = check_fold(tag + " (a, b) given, ReLU + residual", name, zm, C, nhwc, ab_o, out, K, True, rm_, hosts)
    check_scal(tag, h, bar, out["scal"], f.A0, f.G0)
    if looped:                                   # the other variants change nothing the tile loop sees
        return
    out = f.run(K, False, None, part=f.stats_part())
    ab_k = out["ab"].reshape(2, C)
    np.testing.assert_allclose(ab_k, ab_o, rtol=3e-6, atol=1e-7)
    np.testing.assert_allclose(out["save"].reshape(2, C), save_o, rtol=3e-6, atol=1e-7)
    # and against float64 at the bars derived from the arithmetic (tests/bn_oracle.py: 1.4 to 55 times tighter than the line above at these inputs)
    ref = N.forward(zm, C, nhwc, gamma, beta)
    nbar = N.fwd_bars(ref, invstd_fp32=bool(nhwc))
    sv = out["save"].reshape(2, C)
    w = [N.worst(got, ref[n], nbar[n]) for got, n in ((ab_k[0], "a"), (ab_k[1], "b"), (sv[0], "mean"), (sv[1], "invstd"))]
    print(f"[site-fwd] {tag} a, b, mean, invstd: worst error / derived bar = " + " ".join(f"{v:.3f}" for v in w))
    assert max(w) <= 1.0, (tag, w)
    h, bar = check_fold(tag + " finalised from the statistics kernel", name, zm, C, nhwc, ab_k, out, K, False, None, hosts)
    check_scal(tag, h, bar, out["scal"], f.A0, f.G0)
    for k in (4, 8):
        out = f.run(k, True, None, ab=(ab_o, save_o), bins=True)
        assert out["bin_bytes"] == (1 if k == 4 else 2)
        check_fold(tag + f" int{8 * out['bin_bytes']} indices", name, zm, C, nhwc, ab_o, out, k, True, None, hosts)


CONV_SHAPES = ((100, 32, 16), (128, 64, 8), (128, 32, 16))      # shapes alignq_conv3x3_nhwc leaves batch-norm partials for


@pytest.mark.parametrize("B,C,H", CONV_SHAPES, ids=["x".join(map(str, s)) for s in CONV_SHAPES])
def test_folded_site_forward_from_the_convolution_epilogue(dev, B, C, H):
    """channels-last: (a, b) finalised from the float partials alignq_conv3x3_nhwc leaves in its epilogue (conv_parts > 0)"""
    from alignq_amd import _lib as L
    lib, p = L.load(), L.ptr
    F = C * H * H
    name = S.form(B, F, True)
    torch.manual_seed(B + C)
    n = 2 ** K - 1
    cl = torch.channels_last
    x = (torch.randn(B, C, H, H, device=dev) * 1.1).contiguous(memory_format=cl)
    wq = (torch.round(torch.tanh(torch.randn(C, C, 3, 3)) * n) / n).to(dev).contiguous(memory_format=cl)
    z = torch.empty_like(x)
    n_parts = lib.alignq_conv3x3_bn_parts(B, H, H, C)
    assert n_parts > 0
    part = torch.empty(C, n_parts, 2, device=dev)
    L.check(lib.alignq_conv3x3_nhwc(p(x), p(wq), p(z), B, H, H, C, K, 0, None, p(part), None, 0, 0, L.stream_ptr()), "conv fwd")
    torch.cuda.synchronize()
    zm = z.permute(0, 2, 3, 1).reshape(B, F).cpu().numpy()
    rng = np.random.default_rng(B + C)
    gamma, beta = (rng.random(C) + 0.5).astype(np.float32), (rng.standard_normal(C) * 0.1).astype(np.float32)
    rm_ = (rng.standard_normal((B, F)) * 0.7).astype(np.float32)
    f = Fold(dev, B, C, H, 1, z, gamma, beta)
    out = f.run(K, True, cu(rm_, dev), part=part, conv_parts=n_parts)
    ab_o, save_o, _ = O.bn_fold_ab(zm, C, 1, gamma, beta, 1e-5)
    ab_k = out["ab"].reshape(2, C)
    np.testing.assert_allclose(ab_k, ab_o, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(out["save"].reshape(2, C), save_o, rtol=1e-5, atol=2e-6)
    tag = f"fold {name} {B}x{C}x{H}x{H} conv partials"
    h, bar = check_fold(tag, name, zm, C, 1, ab_k, out, K, True, rm_, {})
    check_scal(tag, h, bar, out["scal"], f.A0, f.G0)


# ------------------------------------------------------------------------------------------------ B <= 32: residual, (a, b), groups
@pytest.mark.parametrize("B,C,H", G.BN1, ids=["x".join(map(str, s)) for s in G.BN1])
def test_small_batch_site_forward_forms(dev, B, C, H):
    """site1_kernels.hip behind its four other entry points, channels-last, eps = 1e-5: alignq_site_partials_res (x, residual,
    ReLU), alignq_site_partials_res_ab (x = a z + b on load) and alignq_site1_groups_fwd / _fwd_m at groups = 2 with
    alignq_site1_groups_reduce_loss; per slice y bit for bit, stats, D and scal at their bars, and _fwd_m the same bits as _fwd."""
    from alignq_amd import _lib as L
    lib, p, st = L.load(), L.ptr, L.stream_ptr()
    F, Gn, eps = C * H * H, 2, 1e-5
    name = S.form(B, F)                          # site1_fwd_kernel at B = 6, site1_fwd64_kernel at B = 28
    rng = np.random.default_rng(7 * B + C)
    gamma, beta = (rng.random(C) + 0.5).astype(np.float32), (rng.standard_normal(C) * 0.2).astype(np.float32)
    zm = [(rng.standard_normal((B, F)) * 1.4 + 0.3).astype(np.float32) for _ in range(Gn)]
    rm_ = [np.maximum(rng.standard_normal((B, F)), 0).astype(np.float32) - 0.3 for _ in range(Gn)]
    ab = [O.bn_fold_ab(zg, C, 1, gamma, beta, 1e-5)[0] for zg in zm]
    hosts = [Host(O.bn_apply(zm[i], C, 1, ab[i]), eps) for i in range(Gn)]
    A0, G0 = G.admm_params(B, B, 11 * B + C)
    A, Gm = cu(A0, dev), cu(G0, dev)
    wsb = lib.alignq_site_ws_bytes(B, F)
    ws = torch.empty(wsb * Gn, dtype=torch.uint8, device=dev)
    zd, rd, abd = cu(np.stack(zm), dev), cu(np.stack(rm_), dev), cu(np.stack(ab), dev)
    xd = cu(hosts[0].x, dev)
    names = ["y", "stats", "D", "scal"]

    def single(which):
        arena = Arena(dev, [B * F, 4 * F, B * B, 4])

        def once():
            arena.reset()
            v = dict(zip(names, arena.views))
            if which == "res":
                L.check(lib.alignq_site_partials_res(p(xd), B, F, K, R, eps, p(rd[0]), 1, p(v["y"]), p(v["stats"]), p(ws), st), "partials_res")
            else:
                L.check(lib.alignq_site_partials_res_ab(p(zd[0]), p(abd[0]), C, B, F, K, R, eps, p(rd[0]), 1, p(v["y"]), p(v["stats"]),
                                                        p(ws), st), "partials_res_ab")
            L.check(lib.alignq_site_reduce_loss(p(ws), B, F, p(v["D"]), p(A), p(Gm), B, MU, RHO, p(v["scal"]), st), "reduce_loss")
            torch.cuda.synchronize()
            return windows(names, arena)
        first = once()
        assert_written_and_repeatable(which, first, once())
        return first

    def check_slice(tag, h, res, out):
        y_ref, _ = _expected_y(h.x, K, R, res, True)
        assert np.array_equal(bits(out["y"]), bits(y_ref.reshape(-1))), f"{tag}: y differs from the oracle"
        check_stats(tag, h, out["stats"])
        bar = check_D(tag, name, h, out["D"])
        check_scal(tag, h, bar, out["scal"], A0, G0)

    outs = {w: single(w) for w in ("res", "res_ab")}
    for w, out in outs.items():
        check_slice(f"site1 {w} {B}x{C}x{H}x{H}", hosts[0], rm_[0], out)
    for n in names:
        assert np.array_equal(bits(outs["res"][n]), bits(outs["res_ab"][n])), f"{n}: x given and x = a z + b formed on load differ"

    def groups(masked):
        arena = Arena(dev, [Gn * B * F, Gn * 4 * F, Gn * B * B, Gn * 4])
        mask = torch.zeros(lib.alignq_site1_mask_bytes(B, F, Gn), dtype=torch.uint8, device=dev)

        def once():
            arena.reset()
            v = dict(zip(names, arena.views))
            if masked:
                L.check(lib.alignq_site1_groups_fwd_m(p(zd), p(abd), C, B, F, Gn, K, R, eps, p(rd), 1, p(v["y"]), p(v["stats"]), p(ws),
                                                      p(mask), st), "alignq_site1_groups_fwd_m")
            else:
                L.check(lib.alignq_site1_groups_fwd(p(zd), p(abd), C, B, F, Gn, K, R, eps, p(rd), 1, p(v["y"]), p(v["stats"]), p(ws), st),
                        "alignq_site1_groups_fwd")
            L.check(lib.alignq_site1_groups_reduce_loss(p(ws), B, F, Gn, p(v["D"]), p(A), p(Gm), B, MU, RHO, p(v["scal"]), st),
                    "alignq_site1_groups_reduce_loss")
            torch.cuda.synchronize()
            return windows(names, arena)
        first = once()
        assert_written_and_repeatable(f"groups masked={masked}", first, once())
        return first

    g0, g1 = groups(False), groups(True)
    for n in names:
        assert np.array_equal(bits(g0[n]), bits(g1[n])), f"{n}: _fwd and _fwd_m differ"
    for i in range(Gn):
        sl = {n: g0[n].reshape(Gn, -1)[i] for n in names}
        check_slice(f"site1 groups {B}x{C}x{H}x{H} slice {i}", hosts[i], rm_[i], sl)
    for n in names:                              # slice 0 of the groups launch is the single launch
        assert np.array_equal(bits(g0[n].reshape(Gn, -1)[0]), bits(outs["res_ab"][n])), f"{n}: groups slice 0 != the single launch"


# ------------------------------------------------------------------------------------------------ multi, filler, twin: bit for bit
def _partials(lib, L, xd, B, F, ws, dev):
    xq, stats = torch.empty(B * F, device=dev), torch.empty(4 * F, device=dev)
    L.check(lib.alignq_site_partials(L.ptr(xd), B, F, K, R, 0.0, L.ptr(xq), L.ptr(stats), L.ptr(ws), L.stream_ptr()), "alignq_site_partials")


MULTI_F = (96, 4096, 8192)


def _open_sites(dev, B, lib, L):
    """three plain sites of one B left open behind alignq_site_partials, and each one's stand-alone D / scal"""
    sites = []
    for F in MULTI_F:
        h = plain_host(B, F)
        xd = cu(h.x, dev)
        ws = torch.empty(lib.alignq_site_ws_bytes(B, F), dtype=torch.uint8, device=dev)
        A0, G0 = G.admm_params(B, DIM, B + F)
        A, Gm = cu(A0, dev), cu(G0, dev)
        _partials(lib, L, xd, B, F, ws, dev)
        D, scal = torch.empty(B * B, device=dev), torch.empty(4, device=dev)
        L.check(lib.alignq_site_reduce_loss(L.ptr(ws), B, F, L.ptr(D), L.ptr(A), L.ptr(Gm), DIM, MU, RHO, L.ptr(scal), L.stream_ptr()),
                "alignq_site_reduce_loss")
        torch.cuda.synchronize()
        sites.append(dict(F=F, xd=xd, ws=ws, A=A, Gm=Gm, D=D.cpu().numpy(), scal=scal.cpu().numpy()))
    return sites


@pytest.mark.parametrize("B", [100, 128])
def test_multi_site_reduction_equals_the_per_site_launches(dev, B):
    from alignq_amd import _lib as L
    lib = L.load()
    sites = _open_sites(dev, B, lib, L)
    n = len(sites)
    arena = Arena(dev, [B * B] * n + [4] * n)
    for _ in range(2):
        arena.reset()
        Dv, sv = arena.views[:n], arena.views[n:]
        L.check(lib.alignq_site_reduce_loss_multi(n, L.ptr_array([s["ws"] for s in sites]), L.ptr_array(Dv),
                                                  L.ptr_array([s["A"] for s in sites]), L.ptr_array([s["Gm"] for s in sites]),
                                                  L.ptr_array(sv), L.i64_array([s["F"] for s in sites]), B, DIM, MU, RHO,
                                                  L.stream_ptr()), "alignq_site_reduce_loss_multi")
        torch.cuda.synchronize()
        got = arena.get()
        for i, s in enumerate(sites):
            assert np.array_equal(bits(got[i]), bits(s["D"])), f"D of site {i} (F = {s['F']})"
            assert np.array_equal(bits(got[n + i]), bits(s["scal"])), f"scal of site {i} (F = {s['F']})"


@pytest.mark.parametrize("n_fill", [1, 3])
def test_filler_launch_equals_the_stand_alone_launches(dev, n_fill):
    """alignq_site_partials_bn_fill at (128, 64, 8) channels-last (128 workgroups: three filler slots) carrying the reductions of
    1 and 3 earlier sites: the site's own outputs and every filler's D / scal equal the stand-alone launches bit for bit"""
    from alignq_amd import _lib as L
    lib, p = L.load(), L.ptr
    B, C, H = 128, 64, 8
    F = C * H * H
    assert lib.alignq_site_fill_slots(B, F) == S.site_fill_slots(B, F) == 3
    zm, gamma, beta, _ = G.bn_inputs(B, C, H, seed=1)
    f = Fold(dev, B, C, H, 1, cu(zm, dev), gamma, beta)
    part = f.stats_part()
    alone = f.run(K, True, None, part=part)
    sites = _open_sites(dev, B, lib, L)[:n_fill]
    for s in sites:                              # leave every filler's workspace open again
        _partials(lib, L, s["xd"], B, s["F"], s["ws"], dev)
    names = ["y", "stats", "ab", "save", "D", "scal"] + [f"fD{i}" for i in range(n_fill)] + [f"fscal{i}" for i in range(n_fill)]
    arena = Arena(dev, [B * F, 4 * F, 2 * C, 2 * C, B * B, 4] + [B * B] * n_fill + [4] * n_fill)
    v = dict(zip(names, arena.views))
    rm, rv, nbt = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
    L.check(lib.alignq_site_partials_bn_fill(p(f.zd), p(part), p(f.tg), p(f.tb), p(rm), p(rv), p(nbt), 0.1, 1e-5, p(v["ab"]),
                                             p(v["save"]), C, H * H, B, F, K, R, 0.0, 1, None, 1, 0, p(v["y"]), None, p(v["stats"]),
                                             p(f.ws), n_fill, L.ptr_array([s["ws"] for s in sites]),
                                             L.ptr_array([v[f"fD{i}"] for i in range(n_fill)]),
                                             L.ptr_array([s["A"] for s in sites]), L.ptr_array([s["Gm"] for s in sites]),
                                             L.ptr_array([v[f"fscal{i}"] for i in range(n_fill)]),
                                             L.i64_array([s["F"] for s in sites]), DIM, MU, RHO, L.stream_ptr()),
            "alignq_site_partials_bn_fill")
    L.check(lib.alignq_site_reduce_loss(p(f.ws), B, F, p(v["D"]), p(f.A), p(f.Gm), DIM, MU, RHO, p(v["scal"]), L.stream_ptr()),
            "alignq_site_reduce_loss")
    torch.cuda.synchronize()
    got = windows(names, arena)
    for n in ("y", "stats", "ab", "save", "D", "scal"):
        assert np.array_equal(bits(got[n]), bits(alone[n])), f"{n}: the site's own output changes with {n_fill} filler(s)"
    for i, s in enumerate(sites):
        assert np.array_equal(bits(got[f"fD{i}"]), bits(s["D"])) and np.array_equal(bits(got[f"fscal{i}"]), bits(s["scal"])), f"filler {i}"


def test_twin_launch_equals_the_stand_alone_launches(dev):
    """alignq_site_partials_bn_twin at (128, 64, 8) channels-last: site a with the ReLU, site b without and with other inputs"""
    from alignq_amd import _lib as L
    lib, p = L.load(), L.ptr
    B, C, H = 128, 64, 8
    F = C * H * H
    folds, alone, parts = [], [], []
    for i, relu in enumerate((True, False)):
        zm, gamma, beta, _ = G.bn_inputs(B, C, H, seed=10 + i)
        f = Fold(dev, B, C, H, 1, cu(zm, dev), gamma, beta)
        parts.append(f.stats_part())
        alone.append(f.run(K, relu, None, part=parts[i]))
        folds.append(f)
    names = [f"{n}{i}" for i in range(2) for n in ("y", "stats", "ab", "save", "D", "scal")]
    arena = Arena(dev, [B * F, 4 * F, 2 * C, 2 * C, B * B, 4] * 2)
    v = dict(zip(names, arena.views))
    keep, args = [], []
    for i, (f, relu) in enumerate(zip(folds, (True, False))):
        rm, rv, nbt = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
        keep.append((rm, rv, nbt))
        args.append(L.SiteBnArgs(p(f.zd), p(parts[i]), p(f.tg), p(f.tb), p(rm), p(rv), p(nbt), 0.1, 1e-5, p(v[f"ab{i}"]),
                                 p(v[f"save{i}"]), C, H * H, B, F, K, R, 0.0, int(relu), None, 1, 0, p(v[f"y{i}"]), None,
                                 p(v[f"stats{i}"]), p(f.ws)))
    L.check(lib.alignq_site_partials_bn_twin(ctypes.byref(args[0]), ctypes.byref(args[1]), L.stream_ptr()), "alignq_site_partials_bn_twin")
    for i, f in enumerate(folds):
        L.check(lib.alignq_site_reduce_loss(p(f.ws), B, F, p(v[f"D{i}"]), p(f.A), p(f.Gm), DIM, MU, RHO, p(v[f"scal{i}"]),
                                            L.stream_ptr()), "alignq_site_reduce_loss")
    torch.cuda.synchronize()
    got = windows(names, arena)
    for i in range(2):
        for n in ("y", "stats", "ab", "save", "D", "scal"):
            assert np.array_equal(bits(got[f"{n}{i}"]), bits(alone[i][n])), f"twin site {i}: {n}"


# ------------------------------------------------------------------------------------------------ captured chains
CHAINS = [("fwd1", 5, 4096), ("fwd1-64", 28, 70), ("fwd2", 48, 70), ("fwd4-32", 100, 96), ("fwd4-64-full", 128, 8192), ("fwd4-loop512", 128, 32832)]


@pytest.mark.parametrize("name,B,F", CHAINS, ids=[f"{n}-{B}x{F}" for n, B, F in CHAINS])
def test_captured_chain_replays_to_the_eager_bits(dev, name, B, F):
    """alignq_site_partials -> alignq_site_reduce_loss captured on one stream, one chain per geometry class; two replays"""
    from alignq_amd import _lib as L
    lib, p = L.load(), L.ptr
    assert S.form(B, F) == name
    h = plain_host(B, F)
    xd = cu(h.x, dev)
    A0, G0 = G.admm_params(B, DIM, B + F)
    A, Gm = cu(A0, dev), cu(G0, dev)
    names = ["xq", "stats", "D", "scal"]
    arena = Arena(dev, [B * F, 4 * F, B * B, 4])                 # arena and workspace exist before the capture
    ws = torch.empty(lib.alignq_site_ws_bytes(B, F), dtype=torch.uint8, device=dev)

    def chain():
        v = dict(zip(names, arena.views))
        st = L.stream_ptr()
        return [lib.alignq_site_partials(p(xd), B, F, K, R, h.eps, p(v["xq"]), p(v["stats"]), p(ws), st),
                lib.alignq_site_reduce_loss(p(ws), B, F, p(v["D"]), p(A), p(Gm), DIM, MU, RHO, p(v["scal"]), st)]

    assert chain() == [0, 0]
    torch.cuda.synchronize()
    eager = windows(names, arena)
    arena.reset()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert L.stream_ptr() == side.cuda_stream
        rcs = chain()
    assert rcs == [0, 0]
    for _ in range(2):
        arena.reset()
        graph.replay()
        torch.cuda.synchronize()
        got = windows(names, arena)
        for n in names:
            assert np.array_equal(bits(got[n]), bits(eager[n])), f"{n}: replay differs from the eager launch"
