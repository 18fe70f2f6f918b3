"""The stand-alone batch-norm kernels of the fold (csrc/bn_kernels.hip: alignq_bn_partial_stats, alignq_bn_stats,
alignq_bn_partial_stats_nhwc, alignq_bn_bwd_totals, alignq_bn_bwd_apply in both layouts) through the C ABI against tests/bn_oracle.py,
one row per launch form.  Every output lies in a NaN-filled window between sentinel guards, everything is written and nothing outside
is touched, every launch runs twice and must give the same bits.  Bars: bn_oracle's docstring (u = 2^-24, 2^-53 for the double sums,
operation counts); every check prints its worst error / bar.  The refusals the header states leave every window untouched.

Then the chain at the channel counts and partial forms bn_shape_ok admits beyond the ResNet-20/56 sites (G.BN4_CL, G.BN4_NCHW):
alignq_site_partials_bn finalising (a, b), save, the running statistics and the counter in the kernel - from the statistics kernel's
double partials and, channels-last, from float partials synthesised on both sides of a load round - with y bit for bit at the kernel's
own (a, b) and stats / D / scal through test_gpu_site_fwd_forms.check_fold; alignq_site_prep_fused -> alignq_site_bwd_apply_bn with
every entry of dx_part against the float64 sums of the kernel's own dx, then alignq_bn_bwd_apply / alignq_bn_bwd_totals on those
partials at G.bn_bars; one row per layout again with a channel of mean 30, standard deviation 0.5; fused.bn_site through autograd
at C = 128 (channels-last) and C = 3 (NCHW).

Measured on an MI355X (worst error / bar per family, the planted defects each row catches): NOTES.md, "The batch-norm fold per
launch form".
"""
import functools

import numpy as np
import pytest
import torch

from tests import bn_oracle as N
from tests import oracle_c as O
from tests import site_fwd_oracle as S
from tests import site_grad_oracle as G
from tests.test_gpu_bench_path import _SiteRun, _dev_like, _mem
from tests.test_gpu_dwconv import SENTINEL, Arena
from tests.test_gpu_site_corr_grad import _bn_checks, rebuilt_dD, scale
from tests.test_gpu_site_fwd_forms import check_fold, check_scal

pytestmark = pytest.mark.gpu

EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def ptr(t):
    return None if t is None else t.data_ptr()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def untouched(a):
    return bool((words(a) == SENTINEL).all())


def written(a):
    return bool((words(a) != SENTINEL).all())


def same(a, b):
    return np.array_equal(words(a), words(b))


class Windows:
    """named windows of one sentinel-filled arena; run(fn) resets it, launches, synchronises and returns {name: numpy copy}"""

    def __init__(self, dev, **sizes):
        self.names = list(sizes)
        self.arena = Arena(dev, [sizes[n] for n in self.names])
        self.v = dict(zip(self.names, self.arena.views))

    def run(self, launch, preset=None, rc=0):
        from alignq_amd import _lib as L
        self.arena.reset()
        for n, a in (preset or {}).items():
            self.v[n].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.float32).ravel()).to(self.v[n].device))
        got = launch(self.v, L.load(), L.stream_ptr())
        torch.cuda.synchronize()
        assert got == rc, f"return code {got}, expected {rc}"
        return dict(zip(self.names, self.arena.get()))                     # (asserts the guards)

    def twice(self, launch, preset=None):
        a, b = self.run(launch, preset), self.run(launch, preset)
        for n in self.names:
            assert same(a[n], b[n]), f"second launch differs in {n}"
        return a


def f64(a):
    return np.ascontiguousarray(a).view(np.float64)


def report(tag, **w):
    print(f"[bn-forms] {tag}: " + "  ".join(f"{k} {v:.3f}" for k, v in w.items()))
    for k, v in w.items():
        assert v <= 1.0, f"{tag}: {k} is {v:.3f} x its bar"


# ------------------------------------------------------------------------------------------------ NCHW statistics
@pytest.mark.parametrize("row", [r for r, _ in N.STATS_NCHW_ROWS], ids=N.row_id)
def test_nchw_partial_stats_and_stand_alone_finalisation(dev, row):
    B, C, HW = row
    z, gamma, beta, rm, rv = N.stats_inputs(B, C, HW)
    zd, gd, bd = cu(z, dev), cu(gamma, dev), cu(beta, dev)
    win = Windows(dev, ws=C * 64, ab=2 * C, save=2 * C, rm=C, rv=C, nbt=2)
    ref_parts, abs_parts, cnt = N.double_parts_nchw(z, C)

    out = win.twice(lambda v, lib, st: lib.alignq_bn_partial_stats(ptr(zd), B, C, HW, ptr(v["ws"]), st))
    assert written(out["ws"]) and all(untouched(out[n]) for n in win.names[1:])
    parts = f64(out["ws"]).reshape(C, N.K_SPLIT, 2)
    w_part = N.worst(parts, ref_parts, N.part_bar(abs_parts, cnt))
    empty = cnt == 0
    assert np.all(parts[:, empty] == 0.0), "an empty split holds something"

    nbt0 = np.array([41], np.int64)
    w = dict(part=w_part)
    variants = [("full-m0.1", True, True, True, 0.1), ("full-m1.0", True, True, True, 1.0), ("no-affine", False, True, True, 0.1),
                ("no-running", True, False, True, 0.1), ("no-counter", True, True, False, 0.1), ("bare", False, False, False, 0.1)]
    for tag, affine, running, counter, mom in variants:
        def launch(v, lib, st):
            return lib.alignq_bn_stats(ptr(zd), B, C, HW, ptr(gd) if affine else None, ptr(bd) if affine else None,
                                       ptr(v["rm"]) if running else None, ptr(v["rv"]) if running else None,
                                       ptr(v["nbt"]) if counter else None, mom, EPS, ptr(v["ab"]), ptr(v["save"]), ptr(v["ws"]), st)
        o = win.twice(launch, preset=dict(rm=rm, rv=rv, nbt=nbt0))
        assert same(o["ws"], out["ws"]), f"{tag}: alignq_bn_stats' partials differ from alignq_bn_partial_stats'"
        assert written(o["ab"]) and written(o["save"])
        ref = N.forward(z, C, 0, gamma if affine else None, beta if affine else None, rm, rv, 41, mom, EPS)
        bars = N.fwd_bars(ref, invstd_fp32=False)
        ab, save = o["ab"].reshape(2, C), o["save"].reshape(2, C)
        ww = dict(a=N.worst(ab[0], ref["a"], bars["a"]), b=N.worst(ab[1], ref["b"], bars["b"]),
                  mean=N.worst(save[0], ref["mean"], bars["mean"]), invstd=N.worst(save[1], ref["invstd"], bars["invstd"]))
        if running:
            ww["rmean"] = N.worst(o["rm"], ref["running_mean"], bars["running_mean"])
            ww["rvar"] = N.worst(o["rv"], ref["running_var"], bars["running_var"])
        else:
            assert same(o["rm"], rm) and same(o["rv"], rv), f"{tag}: running statistics written through a NULL argument's neighbour"
        assert int(o["nbt"].view(np.int64)[0]) == (42 if counter else 41), f"{tag}: counter"
        for k, val in ww.items():
            w[k] = max(w.get(k, 0.0), val)
    report(N.row_id(row), **w)


# ------------------------------------------------------------------------------------------------ channels-last statistics
@pytest.mark.parametrize("row", [r for r, _ in N.STATS_NHWC_ROWS], ids=N.row_id)
def test_nhwc_partial_stats(dev, row):
    B, C, HW = row
    z = N.stats_inputs(B, C, HW)[0]
    zd = cu(z, dev)
    win = Windows(dev, ws=C * N.NHWC_PARTS * 4)
    out = win.twice(lambda v, lib, st: lib.alignq_bn_partial_stats_nhwc(ptr(zd), B, C, HW, ptr(v["ws"]), st))
    assert written(out["ws"])
    parts = f64(out["ws"]).reshape(C, N.NHWC_PARTS, 2)
    ref_parts, abs_parts, cnt = N.double_parts_nhwc(z, C)
    assert np.all(parts[:, cnt == 0] == 0.0), "an empty block holds something"
    ref = N.forward(z, C, 1)
    tot_bar = (ref["n"] + 64.0) * N.V * np.stack([ref["abs1"], ref["sq"]], 1) + N.TINY
    report(N.row_id(row), part=N.worst(parts, ref_parts, N.part_bar(abs_parts, cnt)),
           total=N.worst(parts.sum(1), np.stack([ref["mean"] * ref["n"], ref["sq"]], 1), tot_bar))


# ------------------------------------------------------------------------------------------------ backward
def _bwd_case(B, C, HW, nhwc):
    dx, z, ab, save = N.bwd_inputs(B, C, HW)
    bw = N.backward(dx, z, C, nhwc, ab[0], save)
    part = N.synth_dx_part(dx, bw["zhat"], C, nhwc)
    tot, abs_ = N.totals_from_dx_part(part, B, C, HW, nhwc)
    return dx, z, ab, save, bw, part, tot, abs_


def _check_totals(bw, part, abs_, out, C):
    cnt = part.shape[0]
    w = {}
    for j, (name, key) in enumerate((("dbeta", "dbeta"), ("dgamma", "dgamma"))):
        bar, kbar = N.totals_bar(bw[name], abs_[:, j], cnt, bw["n"])
        w[name] = N.worst(out[key], bw[name], bar)
        if "ktot" in out and written(out["ktot"]):
            w["k%d" % j] = N.worst(out["ktot"].reshape(2, C)[j], bw["k%d" % j], kbar)
    return w


@pytest.mark.parametrize("row", [r for r, _ in N.BWD_NHWC_ROWS], ids=N.row_id)
def test_nhwc_backward_totals_and_apply(dev, row):
    B, C, HW = row
    dx, z, ab, save, bw, part, tot, abs_ = _bwd_case(B, C, HW, 1)
    dxd, zd, abd, sd, pd = (cu(a, dev) for a in (dx, z, ab, save, part))
    win = Windows(dev, dz=B * C * HW, dgamma=C, dbeta=C, ktot=2 * C)

    def totals(full):
        return lambda v, lib, st: lib.alignq_bn_bwd_totals(ptr(pd), B, C, HW, ptr(v["ktot"]), ptr(v["dgamma"]) if full else None,
                                                           ptr(v["dbeta"]) if full else None, st)

    def apply(full):
        return lambda v, lib, st: lib.alignq_bn_bwd_apply(ptr(dxd), ptr(zd), ptr(abd), ptr(sd), ptr(pd), B, C, HW, 1, ptr(v["dz"]),
                                                          ptr(v["dgamma"]) if full else None, ptr(v["dbeta"]) if full else None, st)

    t_full, t_lean = win.twice(totals(True)), win.twice(totals(False))
    assert written(t_full["ktot"]) and written(t_full["dgamma"]) and written(t_full["dbeta"]) and untouched(t_full["dz"])
    assert untouched(t_lean["dgamma"]) and untouched(t_lean["dbeta"]) and same(t_lean["ktot"], t_full["ktot"])
    a_full, a_lean = win.twice(apply(True)), win.twice(apply(False))
    assert written(a_full["dz"]) and written(a_full["dgamma"]) and written(a_full["dbeta"]) and untouched(a_full["ktot"])
    assert untouched(a_lean["dgamma"]) and untouched(a_lean["dbeta"]) and same(a_lean["dz"], a_full["dz"])
    assert same(a_full["dgamma"], t_full["dgamma"]) and same(a_full["dbeta"], t_full["dbeta"]), "apply and totals disagree"
    w = _check_totals(bw, part, abs_, t_full, C)
    # against the float64 sum of the partials as given: only the double accumulation and one rounding remain
    for j, name in enumerate(("dbeta", "dgamma")):
        bar, kbar = N.totals_bar(tot[:, j], abs_[:, j], part.shape[0], bw["n"], exact_parts=True)
        w[name + "|parts"] = N.worst(t_full[name], tot[:, j], bar)
        w["k%d|parts" % j] = N.worst(t_full["ktot"].reshape(2, C)[j], tot[:, j] / bw["n"], kbar)
    k = t_full["ktot"].reshape(2, C)
    ref_dz, bar_dz = N.dz_ref_and_bar(dx, z, C, 1, ab[0], save, k[0], k[1])
    w["dz"] = N.worst(a_full["dz"], ref_dz, bar_dz)
    report(N.row_id(row), **w)


@pytest.mark.parametrize("row", [r for r, _ in N.BWD_NCHW_ROWS], ids=N.row_id)
def test_nchw_backward_apply(dev, row):
    B, C, HW = row
    dx, z, ab, save, bw, part, tot, abs_ = _bwd_case(B, C, HW, 0)
    dxd, zd, abd, sd, pd = (cu(a, dev) for a in (dx, z, ab, save, part))
    win = Windows(dev, dz=B * C * HW, dgamma=C, dbeta=C)

    def apply(full):
        return lambda v, lib, st: lib.alignq_bn_bwd_apply(ptr(dxd), ptr(zd), ptr(abd), ptr(sd), ptr(pd), B, C, HW, 0, ptr(v["dz"]),
                                                          ptr(v["dgamma"]) if full else None, ptr(v["dbeta"]) if full else None, st)

    a_full, a_lean = win.twice(apply(True)), win.twice(apply(False))
    assert written(a_full["dz"]) and written(a_full["dgamma"]) and written(a_full["dbeta"])
    assert untouched(a_lean["dgamma"]) and untouched(a_lean["dbeta"]) and same(a_lean["dz"], a_full["dz"])
    w = _check_totals(bw, part, abs_, a_full, C)
    tpc = part.shape[0] // C
    for j, name in enumerate(("dbeta", "dgamma")):
        bar, _ = N.totals_bar(tot[:, j], abs_[:, j], tpc, bw["n"], exact_parts=True)
        w[name + "|parts"] = N.worst(a_full[name], tot[:, j], bar)
    ref_dz, bar_dz = N.dz_ref_and_bar(dx, z, C, 0, ab[0], save, tot[:, 0] / bw["n"], tot[:, 1] / bw["n"], k_rounded=True)
    w["dz"] = N.worst(a_full["dz"], ref_dz, bar_dz)
    report(N.row_id(row), **w)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_every_window_untouched(dev):
    from alignq_amd import _lib as L
    EINVAL, EUNSUP = L.EINVAL, L.EUNSUPPORTED
    big = 8192
    src = torch.ones(4 * big + 4, device=dev)
    assert src.data_ptr() % 16 == 0
    z, dx, abt, sv = (src[i * big:(i + 1) * big] for i in range(4))
    off = src[1:big + 1]                                   # 4-byte but not 16-byte aligned
    part = torch.ones(big, device=dev)
    win = Windows(dev, ws=4 * big, ab=big, save=big, rm=big, rv=big, nbt=2, dz=big, dgamma=big, dbeta=big, ktot=big)

    def refused(tag, rc, launch):
        out = win.run(launch, rc=rc)
        for n in win.names:
            assert untouched(out[n]), f"{tag}: {n} was written"

    def stats(zp, B, C, HW, **null):
        def launch(v, lib, st):
            g = lambda n: None if null.get(n) else ptr(v[n])        # noqa: E731
            return lib.alignq_bn_stats(None if null.get("z") else zp, B, C, HW, None, None, ptr(v["rm"]), ptr(v["rv"]), ptr(v["nbt"]),
                                       0.1, EPS, g("ab"), g("save"), g("ws"), st)
        return launch

    def pstats(zp, B, C, HW, nhwc, **null):
        def launch(v, lib, st):
            fn = lib.alignq_bn_partial_stats_nhwc if nhwc else lib.alignq_bn_partial_stats
            return fn(None if null.get("z") else zp, B, C, HW, None if null.get("ws") else ptr(v["ws"]), st)
        return launch

    def totals(B, C, HW, **null):
        def launch(v, lib, st):
            return lib.alignq_bn_bwd_totals(None if null.get("part") else ptr(part), B, C, HW, None if null.get("ktot") else ptr(v["ktot"]),
                                            ptr(v["dgamma"]), ptr(v["dbeta"]), st)
        return launch

    def apply(B, C, HW, nhwc, **null):
        def launch(v, lib, st):
            a = dict(dx=ptr(dx), z=ptr(z), ab=ptr(abt), save=ptr(sv), part=ptr(part), dz=ptr(v["dz"]))
            a.update({n: None for n in null})
            return lib.alignq_bn_bwd_apply(a["dx"], a["z"], a["ab"], a["save"], a["part"], B, C, HW, nhwc, a["dz"], ptr(v["dgamma"]),
                                           ptr(v["dbeta"]), st)
        return launch

    # channels-last channel counts that are no power of two in [4, 256]
    for C in (3, 6, 512):
        refused(f"nhwc stats C={C}", EUNSUP, pstats(ptr(z), 2, C, 2, 1))
        refused(f"nhwc totals C={C}", EUNSUP, totals(2, C, 64))
        refused(f"nhwc apply C={C}", EUNSUP, apply(2, C, 64, 1))
    # C * HW no multiple of the backward tile
    refused("nhwc totals F=16", EUNSUP, totals(2, 4, 4))
    refused("nhwc apply F=16", EUNSUP, apply(2, 4, 4, 1))
    # NCHW: a tile must lie inside one channel
    refused("nchw apply HW=32", EUNSUP, apply(2, 2, 32, 0))
    # NCHW statistics read float4
    for fn_tag, mk in (("stats", stats), ("partial_stats", lambda zp, B, C, HW, **kw: pstats(zp, B, C, HW, 0, **kw))):
        refused(f"{fn_tag} HW=6", EUNSUP, mk(ptr(z), 2, 2, 6))
        refused(f"{fn_tag} misaligned z", EUNSUP, mk(ptr(off), 2, 2, 8))
        refused(f"{fn_tag} HW=2", EINVAL, mk(ptr(z), 2, 2, 2))
        refused(f"{fn_tag} B=0", EINVAL, mk(ptr(z), 0, 2, 8))
        refused(f"{fn_tag} C=0", EINVAL, mk(ptr(z), 2, 0, 8))
        refused(f"{fn_tag} z NULL", EINVAL, mk(ptr(z), 2, 2, 8, z=True))
        refused(f"{fn_tag} ws NULL", EINVAL, mk(ptr(z), 2, 2, 8, ws=True))
    refused("stats ab NULL", EINVAL, stats(ptr(z), 2, 2, 8, ab=True))
    refused("stats save NULL", EINVAL, stats(ptr(z), 2, 2, 8, save=True))
    refused("nhwc stats misaligned z", EUNSUP, pstats(ptr(off), 2, 4, 2, 1))
    refused("nhwc stats z NULL", EINVAL, pstats(ptr(z), 2, 4, 2, 1, z=True))
    refused("nhwc stats ws NULL", EINVAL, pstats(ptr(z), 2, 4, 2, 1, ws=True))
    refused("nhwc stats HW=0", EINVAL, pstats(ptr(z), 2, 4, 0, 1))
    refused("totals part NULL", EINVAL, totals(2, 4, 16, part=True))
    refused("totals ktot NULL", EINVAL, totals(2, 4, 16, ktot=True))
    refused("totals HW=0", EINVAL, totals(2, 4, 0))
    for nhwc, (B, C, HW) in ((1, (2, 4, 16)), (0, (2, 2, 64))):
        for n in ("dx", "z", "ab", "save", "part", "dz"):
            refused(f"apply nhwc={nhwc} {n} NULL", EINVAL, apply(B, C, HW, nhwc, **{n: True}))
        refused(f"apply nhwc={nhwc} HW=0", EINVAL, apply(B, C, 0, nhwc))         # (NCHW: launched with n = 0 before this was pinned)
        refused(f"apply nhwc={nhwc} B=0", EINVAL, apply(0, C, HW, nhwc))
        refused(f"apply nhwc={nhwc} C=0", EINVAL, apply(B, 0, HW, nhwc))


# ================================================================================================ the chain, at the channel counts and
# partial forms the fold admits beyond the ResNet-20/56 sites: alignq_site_partials_bn finalising (a, b) in the kernel, then
# alignq_site_prep_fused -> alignq_site_bwd_apply_bn -> alignq_bn_bwd_apply / alignq_bn_bwd_totals.  Rows: G.BN4_CL / G.BN4_NCHW.
R, K, MU, RHO, DIM = S.R, S.K, S.MU, S.RHO, 128
CL_WHAT = {
    (65, 4, 16): "F = 64: nch 4, twelve idle waves",
    (128, 8, 8): "F = 64: complete rows, nch 8",
    (100, 64, 1): "F = 64: C above the 32-feature tile, two publishing tiles, n = B",
    (128, 256, 1): "F = 256: eight publishing tiles",
    (65, 128, 33): "F = 4224: 64-feature tiles, four passes per wave, two channel groups; backward tile 32, cyc 4",
    (100, 4, 1040): "F = 4160: 64-feature tiles, nch 4",
    (128, 256, 64): "F = 16384: backward 64-feature partials, cp 64, cyc 4",
    (128, 256, 129): "F = 33024: 516 tiles on 512 workgroups, the tile loop",
}
NCHW_WHAT = {
    (65, 1, 64): "F = 64: one channel, two tiles",
    (128, 3, 128): "F = 384: C not a power of two",
    (100, 5, 832): "F = 4160: 64-feature tiles",
    (128, 3, 11008): "F = 33024: the tile loop",
}
assert tuple(CL_WHAT) == G.BN4_CL and tuple(NCHW_WHAT) == G.BN4_NCHW


def float_part_counts(row):
    """the n_parts a channels-last row runs its finalisation from synthesised float partials at: an odd count (float2 loads), an
    even one (float4), and the two counts behind the first load round (256 partials on 32-feature tiles, 512 on 64-feature ones)"""
    tf, _, _, looped = N.fwd_tiles(row[1] * row[2])
    if looped:
        return (2, 515)
    return (1, 2, 7, 258, 259) if tf == 32 else (2, 7, 514, 515)


def _chain_cases():
    cases = []
    for row in G.BN4_CL:
        cases += [(1, row, False, src) for src in ("stats",) + float_part_counts(row)]
    cases += [(0, row, False, "stats") for row in G.BN4_NCHW]
    cases += [(1, G.BN4_HARD[1], True, src) for src in ("stats",) + float_part_counts(G.BN4_HARD[1])]
    cases += [(0, G.BN4_HARD[0], True, "stats")]
    return cases


def _case_id(c):
    nhwc, row, hard, src = c
    return ("cl-" if nhwc else "nchw-") + N.row_id(row) + ("-hard" if hard else "") + "-" + str(src)


@functools.lru_cache(maxsize=2)
def chain_inputs(nhwc, row, hard):
    B, C, HW = row
    zm, gamma, beta, _ = G.bn_inputs(B, C, 0, seed=nhwc, HW=HW)
    if hard:
        zm = N.place_hard_channel(zm, C, nhwc)
    rng = np.random.default_rng(B + C + HW)
    rm0, rv0 = (rng.standard_normal(C) * 0.3).astype(np.float32), (rng.random(C) + 0.5).astype(np.float32)
    return zm, gamma, beta, rm0, rv0


class ChainFwd:
    """alignq_site_partials_bn with the finalisation in the kernel + alignq_site_reduce_loss, every output in a window"""

    def __init__(self, dev, row, nhwc, zm, gamma, beta):
        from alignq_amd import _lib as L
        self.L, self.lib, self.dev = L, L.load(), dev
        self.B, self.C, self.HW = row
        self.F, self.nhwc = self.C * self.HW, nhwc
        self.zd, self.tg, self.tb = cu(zm, dev), cu(gamma, dev), cu(beta, dev)
        self.ws = torch.empty(self.lib.alignq_site_ws_bytes(self.B, self.F), dtype=torch.uint8, device=dev)
        self.A0, self.G0 = G.admm_params(self.B, DIM, self.B + self.C)
        self.A, self.Gm = cu(self.A0, dev), cu(self.G0, dev)

    def stats_part(self):
        L, lib = self.L, self.lib
        fn, nbytes = ((lib.alignq_bn_partial_stats_nhwc, lib.alignq_bn_nhwc_ws_bytes(self.C)) if self.nhwc
                      else (lib.alignq_bn_partial_stats, lib.alignq_bn_ws_bytes(self.C)))
        part = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        L.check(fn(ptr(self.zd), self.B, self.C, self.HW, ptr(part), L.stream_ptr()), "statistics")
        return part

    def run(self, k, relu, res, part, conv_parts, rm0, rv0, bins=False):
        B, C, F = self.B, self.C, self.F
        sizes = dict(y=B * F, stats=4 * F, D=B * B, scal=4, ab=2 * C, save=2 * C, rm=C, rv=C, nbt=2)
        nbytes = self.lib.alignq_bin_bytes(k, R, 0) if bins else 0
        if bins:
            sizes["bins"] = B * F * nbytes // 4
        win = Windows(self.dev, **sizes)

        def launch(v, lib, st):
            rc = lib.alignq_site_partials_bn(ptr(self.zd), ptr(part), ptr(self.tg), ptr(self.tb), ptr(v["rm"]), ptr(v["rv"]),
                                             ptr(v["nbt"]), 0.1, EPS, ptr(v["ab"]), ptr(v["save"]), C, self.HW, B, F, k, R, 0.0,
                                             int(relu), ptr(res), int(self.nhwc), int(conv_parts), ptr(v["y"]), ptr(v.get("bins")),
                                             ptr(v["stats"]), ptr(self.ws), st)
            return rc or lib.alignq_site_reduce_loss(ptr(self.ws), B, F, ptr(v["D"]), ptr(self.A), ptr(self.Gm), DIM, MU, RHO,
                                                     ptr(v["scal"]), st)

        out = win.twice(launch, preset=dict(rm=rm0, rv=rv0, nbt=np.array([41], np.int64)))
        for n in win.names:
            assert written(out[n]), f"{n} has unwritten elements"
        out["bin_bytes"] = nbytes
        return out


def check_finalised(tag, out, ref, bars, C):
    ab, save = out["ab"].reshape(2, C), out["save"].reshape(2, C)
    w = dict(a=N.worst(ab[0], ref["a"], bars["a"]), b=N.worst(ab[1], ref["b"], bars["b"]),
             mean=N.worst(save[0], ref["mean"], bars["mean"]), invstd=N.worst(save[1], ref["invstd"], bars["invstd"]),
             rmean=N.worst(out["rm"], ref["running_mean"], bars["running_mean"]),
             rvar=N.worst(out["rv"], ref["running_var"], bars["running_var"]))
    assert int(out["nbt"].view(np.int64)[0]) == 42, f"{tag}: counter {int(out['nbt'].view(np.int64)[0])}, expected 41 + 1"
    report(tag, **w)
    return ab


@pytest.mark.parametrize("case", _chain_cases(), ids=_case_id)
def test_chain_forward_finalised_in_the_kernel(dev, case):
    nhwc, row, hard, src = case
    B, C, HW = row
    F = C * HW
    zm, gamma, beta, rm0, rv0 = chain_inputs(nhwc, row, hard)
    name = S.form(B, F, True)
    tf, n_tiles, grid, looped = N.fwd_tiles(F)
    assert name == ("fwd4-loopNT" if looped else f"fwd4-{tf}" + ("-full" if B == 128 else ""))
    f = ChainFwd(dev, row, nhwc, zm, gamma, beta)
    ref = N.forward(zm, C, nhwc, gamma, beta, rm0, rv0, 41, 0.1, EPS)
    tag = _case_id(case)
    hosts = {}
    if src == "stats":
        bars = N.fwd_bars(ref, invstd_fp32=bool(nhwc))
        part = f.stats_part()
        res_m = None if looped else (np.random.default_rng(B + C).standard_normal((B, F)) * 0.7).astype(np.float32)
        out = f.run(K, not looped, cu(res_m, dev), part, 0, rm0, rv0)
        ab_k = check_finalised(tag, out, ref, bars, C)
        h, bar = check_fold(tag, name, zm, C, nhwc, ab_k, out, K, not looped, res_m, hosts)
        check_scal(tag, h, bar, out["scal"], f.A0, f.G0)
        if not looped:                              # the index output rides on the same finalisation
            outb = f.run(4, True, None, part, 0, rm0, rv0, bins=True)
            assert same(outb["ab"], out["ab"]) and same(outb["save"], out["save"]) and same(outb["rm"], out["rm"])
            check_fold(tag + " int8 indices", name, zm, C, nhwc, ab_k, outb, 4, True, None, hosts)
    else:
        fp = N.synth_float_parts(zm, C, src)
        bars = N.fwd_bars(ref, invstd_fp32=True, float_parts=fp)
        out = f.run(K, False, None, cu(fp, dev), src, rm0, rv0)
        ab_k = check_finalised(tag, out, ref, bars, C)
        h, bar = check_fold(tag, name, zm, C, nhwc, ab_k, out, K, False, None, hosts)
        check_scal(tag, h, bar, out["scal"], f.A0, f.G0)


BWD_CASES = ([(1, r, False) for r in G.BN4_CL] + [(0, r, False) for r in G.BN4_NCHW]
             + [(1, G.BN4_HARD[1], True), (0, G.BN4_HARD[0], True)])


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: _case_id(c + ("bwd",)))
def test_chain_backward_partials_totals_and_apply(dev, case):
    from alignq_amd import _lib as L
    lib = L.load()
    nhwc, row, hard = case
    B, C, HW = row
    F, shape = C * HW, (B, C, HW, 1)
    zm, gamma, beta, _, _ = chain_inputs(nhwc, row, hard)
    A0, G0 = G.admm_params(B, DIM, B + C)
    z = _dev_like(zm, shape, nhwc, dev)
    tg, tb, A, Gm = (cu(a, dev) for a in (gamma, beta, A0, G0))
    ab_o, save_o, _ = O.bn_fold_ab(zm, C, nhwc, gamma, beta, EPS)
    _, D_o, x_o = O.bn_site_fwd(zm, C, nhwc, ab_o, K, R, 0.0, None, False)
    dD, _, _ = rebuilt_dD(D_o, A0, G0, B)
    term = scale(x_o, dD, 0.0)
    ref0 = G.ref_bn(zm, dD, None, gamma, beta, C, nhwc, R, 0.0, x_at=x_o)
    tag = _case_id(case + ("bwd",))

    run = _SiteRun(dev, z, tg, tb, K, False, None, nhwc).forward("ab_in", ab_o.copy(), save_o.copy()).reduce_loss(A, Gm, MU, RHO)
    run.backward(None, float(B * B))
    run.bn_backward()
    torch.cuda.synchronize()
    # ---- every entry of dx_part against the float64 sums of the kernel's own dx over that tile and channel
    dxk = _mem(run.dx, nhwc)
    shp = N.dx_part_shape(B, C, HW, nhwc)
    part = run.part.view(torch.float32)[:int(np.prod(shp))].cpu().numpy().reshape(shp)
    zhat = N.zhat_of(zm, C, nhwc, save_o)
    w = dict(dx_part=N.worst(part, N.dx_part_exact(dxk, zhat, C, nhwc), N.dx_part_bar(dxk, zhat, C, nhwc)))
    # ---- the batch-norm backward on those partials: dz, dgamma, dbeta at the correlation gradient's bar pushed through it
    _bn_checks(tag, run, ref0, term, C, nhwc)
    tot, abs_ = N.totals_from_dx_part(part, B, C, HW, nhwc)
    n = B * HW
    cnt = shp[0]
    dgam, dbet = run.dgam.cpu().numpy(), run.dbet.cpu().numpy()
    for j, (nm, got) in enumerate((("dbeta", dbet), ("dgamma", dgam))):
        bar, kbar = N.totals_bar(tot[:, j], abs_[:, j], cnt, n, exact_parts=True)
        w[nm + "|parts"] = N.worst(got, tot[:, j], bar)
    if nhwc:
        ktot = torch.full((2, C), float("nan"), device=dev)
        dg2, db2 = torch.empty(C, device=dev), torch.empty(C, device=dev)
        L.check(lib.alignq_bn_bwd_totals(ptr(run.part), B, C, HW, ptr(ktot), ptr(dg2), ptr(db2), L.stream_ptr()), "bn_bwd_totals")
        torch.cuda.synchronize()
        assert same(dg2.cpu().numpy(), dgam) and same(db2.cpu().numpy(), dbet), "alignq_bn_bwd_totals and _apply disagree"
        k = ktot.cpu().numpy()
        for j in range(2):
            _, kbar = N.totals_bar(tot[:, j], abs_[:, j], cnt, n, exact_parts=True)
            w["k%d" % j] = N.worst(k[j], tot[:, j] / n, kbar)
        ref_dz, bar_dz = N.dz_ref_and_bar(dxk, zm, C, 1, ab_o[0], save_o, k[0], k[1])
    else:
        ref_dz, bar_dz = N.dz_ref_and_bar(dxk, zm, C, 0, ab_o[0], save_o, tot[:, 0] / n, tot[:, 1] / n, k_rounded=True)
    w["dz|dx"] = N.worst(_mem(run.dz, nhwc), ref_dz, bar_dz)
    report(tag, **w)


# ------------------------------------------------------------------------------------------------ through Python
@pytest.mark.parametrize("nhwc,C,H", [(1, 128, 2), (0, 3, 8)], ids=["cl-72x128x2x2", "nchw-72x3x8x8"])
def test_bn_site_autograd_at_new_channel_counts(dev, nhwc, C, H):
    """fused.bn_site against the composition it falls back to, act(bn(z)), at the bars tests/test_gpu_parity.py holds that pair to
    (test_bn_folded_site_matches_unfused), with the module's running statistics, counter and parameter gradients"""
    import alignq_amd.cdf_alignment_admm as A
    from alignq_amd import config
    from alignq_amd.fused import bn_site, bn_site_fusable
    B, k = 72, 8
    config.args.bitW = config.args.abitW = k
    try:
        torch.manual_seed(B + C)
        z = torch.randn(B, C, H, H, device=dev) * 1.7 + 0.3
        gq = torch.randn(B, C, H, H, device=dev) * 0.01
        if nhwc:
            z, gq = z.contiguous(memory_format=torch.channels_last), gq.contiguous(memory_format=torch.channels_last)
        outs = []
        for fused in (False, True):
            torch.manual_seed(1)
            bn = torch.nn.BatchNorm2d(C).to(dev).train()
            with torch.no_grad():
                bn.weight.copy_(torch.rand(C, device=dev) + 0.5)
                bn.bias.copy_(torch.randn(C, device=dev) * 0.2)
                bn.running_mean.copy_(torch.randn(C, device=dev) * 0.3)
                bn.running_var.copy_(torch.rand(C, device=dev) + 0.5)
                bn.num_batches_tracked.fill_(41)
            admm = A.ADMM(128).to(dev)
            act = A.activation_quantize_fn(k, "second", admm)
            zz = z.clone(memory_format=torch.preserve_format).requires_grad_(True)
            if fused:
                assert bn_site_fusable(bn, act, zz) and zz.is_contiguous() == (not nhwc)
                xq, loss = bn_site(bn, act, zz, relu=True)
            else:
                xq, loss = act(bn(zz))
                xq = torch.nn.functional.relu(xq)
            (loss + (xq * gq).sum()).backward()
            npy = lambda t: t.detach().cpu().numpy()        # noqa: E731
            outs.append(dict(xq=npy(xq), loss=float(loss.detach()), D=npy(admm.D), dz=npy(zz.grad), dw=npy(bn.weight.grad),
                             db=npy(bn.bias.grad), rm=npy(bn.running_mean), rv=npy(bn.running_var),
                             nbt=int(bn.num_batches_tracked), dA=npy(admm.alterD.grad)))
        u, f = outs
        flips = np.abs(u["xq"] - f["xq"]) * (2 ** k - 1)
        assert flips.max() <= 1.0 + 1e-3 and (flips > 0.5).mean() < 1e-3          # tie-zone flips only
        np.testing.assert_allclose(f["D"], u["D"], atol=1e-5)
        np.testing.assert_allclose(f["loss"], u["loss"], atol=1e-5)
        np.testing.assert_allclose(f["rm"], u["rm"], atol=1e-6, rtol=1e-5)
        np.testing.assert_allclose(f["rv"], u["rv"], atol=1e-6, rtol=1e-5)
        assert f["nbt"] == u["nbt"] == 42
        np.testing.assert_allclose(f["dA"], u["dA"], atol=1e-7, rtol=1e-4)
        np.testing.assert_allclose(f["dz"], u["dz"], atol=2e-5, rtol=1e-3)
        np.testing.assert_allclose(f["dw"], u["dw"], atol=2e-4, rtol=1e-3)
        np.testing.assert_allclose(f["db"], u["db"], atol=2e-4, rtol=1e-3)
    finally:
        config.args.bitW = config.args.abitW = 8
