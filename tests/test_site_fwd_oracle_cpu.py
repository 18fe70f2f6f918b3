"""tests/site_fwd_oracle.py checked without a GPU: the float64 restatement of the site forward against the C oracle and a
torch.double statement of corr, its restatement of the dispatch against the library's own host-side queries, the conditions the
bars on D were chosen under (every figure recomputed from the emulation, never from a kernel), each planted defect's margin per
row, and the refusals of the forward entry points that need no device."""
import numpy as np
import pytest
import torch

from tests import oracle_c as O
from tests import site_fwd_oracle as S
from tests import site_grad_oracle as G

ROWS = S.aligned_rows()
IDS = [S.row_id(r) for r in ROWS]


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("B,F", [(2, 70), (5, 70), (28, 70), (33, 70), (64, 200), (65, 96), (128, 96), (130, 40)])
def test_restatement_matches_the_c_oracle_and_torch_double(B, F):
    x, eps, const = S.row_inputs(B, F)
    t = S.transform(x)
    assert np.array_equal(t, O.act_quant_fwd(x, S.K, S.R, O.FORMULA_ADMM)[1]), "the pre-round transform does not depend on k"
    ref = S.reference(x, t, eps)
    xq_o, D_o = O.site_fwd(x, S.K, S.R, eps)
    assert np.array_equal(xq_o, O.act_quant_fwd(x, S.K, S.R, O.FORMULA_ADMM)[0])
    np.testing.assert_allclose(ref["D"], D_o, atol=S.OLD_TOL, rtol=0)
    np.testing.assert_allclose(ref["corr_x"], O.corr_fwd(x, eps), atol=S.OLD_TOL, rtol=0)
    # torch.double: corr as the reference model states it (std unbiased, + eps), from the same fp32 x and t
    xt, tt = torch.from_numpy(x).double(), torch.from_numpy(t).double()
    D_t = (G._corr(tt, eps) - G._corr(xt, eps)).numpy()
    np.testing.assert_allclose(ref["D"], D_t, atol=1e-13, rtol=0)
    st = ref["stats"]
    np.testing.assert_allclose(st[0], xt.mean(0).numpy(), atol=1e-15)
    live = np.ones(F, bool)
    if const is not None:
        live[const] = False
        assert st[1][const] == st[3][const] == 1.0 / eps
    np.testing.assert_allclose(st[3][live], 1.0 / (tt.std(0, unbiased=True).numpy()[live] + eps), rtol=1e-12)
    assert np.array_equal(ref["D"], ref["D"].T) and (ref["s"] > 0).all() and (ref["s_x"] <= ref["s"]).all()
    # scal against the C oracle's loss
    A, Gm = G.admm_params(B, max(B, 128), B + F)
    sc = S.scal_reference(ref["D"], A, Gm)
    loss_o = O.admm_loss(D_o, A, Gm, S.MU, S.RHO)[0]
    assert abs(sc[0] - loss_o) <= S.OLD_TOL and sc[2] == 1.0 / (B * B) and np.isclose(sc[1], 0.5 * S.RHO / (B * B * sc[3]))


@pytest.mark.parametrize("nhwc", [0, 1])
def test_folded_restatement_matches_the_c_oracle(nhwc):
    B, C, H = 12, 8, 8
    z, gamma, beta, _ = G.bn_inputs(B, C, H, seed=nhwc)
    ab, _, _ = O.bn_fold_ab(z, C, nhwc, gamma, beta, 1e-5)
    x = O.bn_apply(z, C, nhwc, ab)
    _, D_o, x_o = O.bn_site_fwd(z, C, nhwc, ab, S.K, S.R, 0.0, None, False)
    assert np.array_equal(x, x_o)
    np.testing.assert_allclose(S.reference(x, S.transform(x), 0.0)["D"], D_o, atol=S.OLD_TOL, rtol=0)


# ------------------------------------------------------------------------------------------------ the dispatch
def test_every_row_selects_the_form_it_claims():
    names = set()
    for name, B, F, aligned in S.ROWS:
        assert S.form(B, F, False, aligned) == name, (name, B, F, aligned)
        names.add(name)
    assert names == {"fwd1", "fwd1-capped", "fwd1-64", "fwd1-64-capped", "fwd2", "fwd2-capped", "fwd4-32", "fwd4-32-full", "fwd4-64", "fwd4-64-full",
                     "fwd4-loop512", "fwd4-loopNT", "large-ks1", "large-ksN"}
    # what the comments of the matrix say about the geometry
    assert S.geom(5, 131072 + 384)["grid"] == 1024 and (131072 + 384 + 127) // 128 == 1027
    # site1_fwd64_kernel (B = 28, 32): a wave per 64-feature tile, so only more than 4 * 1024 tiles make it loop
    assert (131072 + 384 + 63) // 64 == 2054 and (262144 + 192) // 64 == 4099 and S.form(28, 262144) == "fwd1-64"
    assert S.form(28, 4096, pair=False) == "fwd1" and S.form(27, 4096) == "fwd1"
    assert S.geom(48, 131072 + 64)["n_tiles"] == 2049 and S.geom(48, 131072 + 64)["grid"] == 2048
    assert S.geom(128, 96)["n_tiles"] == 3 and S.geom(128, 4096)["n_tiles"] == 128 and S.geom(128, 4098)["tf"] == 64
    assert S.geom(128, 16384)["grid"] == 256 and S.geom(128, 32768)["grid"] == S.geom(128, 32768)["n_tiles"] == 512
    assert S.geom(128, 32832)["n_tiles"] == 513 and S.geom(128, 32832)["grid"] == 512
    assert S.corrl_ksplit(130, 40) == 1 and S.corrl_ksplit(130, 70) == 2
    assert S.n_pairs(1024) == 36 and (1024 + 127) // 128 == 8
    # the folded rows: G.BN4 are one-tile forms, the looped one runs the 1024-thread loop (no 512-thread form with a fold)
    assert [S.form(B, C * H * H, True) for B, C, H in G.BN4] == ["fwd4-32-full", "fwd4-64", "fwd4-32-full"]
    B, C, H = S.FOLD_LOOP
    assert S.form(B, C * H * H, True) == "fwd4-loopNT" and S.form(B, C * H * H, False) == "fwd4-loop512"
    # F = 32768 is ONE tile per workgroup (the older docstring of test_bn_folded_site_kernels_vs_oracle said otherwise)
    assert S.form(128, 32768, True) == "fwd4-64-full" and S.form(128, 36864, True) == "fwd4-loopNT"
    assert [S.form(B, C * H * H) for B, C, H in G.BN1] == ["fwd1", "fwd1-64"]


def test_dispatch_restatement_equals_the_library_queries():
    from alignq_amd import _lib
    lib = _lib.load()
    shapes = {(B, F) for _, B, F, _ in S.ROWS} | {(B, C * H * H) for B, C, H in G.BN4 + G.BN1 + (S.FOLD_LOOP,)}
    shapes |= {(1, 64), (2, 1), (32, 128), (32, 129), (64, 131072), (128, 4097), (128, 16385), (129, 64), (256, 16384),
               (1024, 16384), (1025, 64), (128, 0), (512, 1024)}
    for B, F in sorted(shapes):
        assert lib.alignq_site_ws_bytes(B, F) == S.ws_bytes(B, F), (B, F)
        assert lib.alignq_site_fill_slots(B, F) == S.site_fill_slots(B, F), (B, F)
        if B >= 2:
            assert lib.alignq_site_bwd_ws_bytes(B) == S.bwd_ws_bytes(B), B
    # the K split shows in the workspace: one 128 x 128 slab per (block pair, split)
    for B, F in ((130, 40), (130, 70), (300, 72), (1024, 136), (256, 16384), (1024, 16384)):
        assert lib.alignq_site_ws_bytes(B, F) == S.n_pairs(B) * S.corrl_ksplit(B, F) * 128 * 128 * 4
    assert lib.alignq_site_bwd_ws_bytes(300) == 320 * S.corrl_s_width(300) * 4 and S.corrl_s_width(300) == 512


# ------------------------------------------------------------------------------------------------ the bars on D
def test_bar_constants_are_four_times_the_emulations_worst_ratio():
    worst = {"split": 0.0, "fp32": 0.0}
    for row in ROWS:
        sch = S.scheme_of(row[0])
        worst[sch] = max(worst[sch], S.measure(row)["ratio"])
    print(f"[site-fwd-oracle] worst |emulate_D - D64| / s: split {worst['split']:.3e}, fp32 {worst['fp32']:.3e}")
    assert 4.0 * worst["split"] <= S.BAR_SPLIT <= 4.2 * worst["split"], worst
    assert 4.0 * worst["fp32"] <= S.BAR_FP32 <= 4.2 * worst["fp32"], worst


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_bar_conditions_and_defect_margins(row):
    name, B, F, _ = row
    m, rid = S.measure(row), S.row_id(row)
    print(f"[site-fwd-oracle] {rid}: emulation {m['ratio']:.2e} s ({m['emu_abs']:.2e} abs), worst BAR * s {m['bar_max']:.2e} "
          f"(off the diagonal {m['bar_max_off']:.2e}), allowance {m['allowance_max']:.2e}, margins "
          + ", ".join(f"{d} {v:.1f}" for d, v in m["margins"].items()))
    assert m["ratio"] * 4.0 <= S.bar_of(name)
    # against the older absolute bar: exactly the rows the module names are 4 x tighter at their worst entry; no row with
    # F >= 4096 is looser than the old bar anywhere, and from F = 4096 on every row is 4 x tighter off the diagonal but for 6 %
    assert (m["bar_max"] <= S.OLD_TOL / 4) == (rid in S.TIGHTER_THAN_OLD)
    if F >= 4096:
        assert m["bar_max"] + m["allowance_max"] < S.OLD_TOL / 2 and m["bar_max_off"] <= 1.07 * S.OLD_TOL / 4
    assert m["allowance_max"] == 0.0 or B == 2, "ill-conditioned columns are expected at B = 2 only"
    # every planted defect that applies is at least 4 x the bar at some entry, but for the pairs the module lists - exactly those
    below = tuple(d for d, v in m["margins"].items() if v < 4.0)
    assert below == S.NOT_RESOLVING.get(rid, ()), (rid, m["margins"])
    if F <= 4100:
        assert "inv_Fm1" not in below or (F >= 4096 and S.scheme_of(name) == "split"), "F - 1 must resolve at small F"
    for d in ("last_tile_dropped", "biased_std", "t_mean_from_x", "one_slab_dropped", "lohi_dropped"):
        assert d not in below


def test_the_listed_exceptions_name_rows_of_the_matrix():
    ids = set(IDS)
    assert set(S.NOT_RESOLVING) <= ids and S.TIGHTER_THAN_OLD <= ids
    for rid, ds in S.NOT_RESOLVING.items():
        assert set(ds) <= {"inv_Fm1", "eps_dropped_t", "eps_dropped_x", "last_feature_dropped"}, rid


@pytest.mark.parametrize("name,B,F", S.CORR_ROWS, ids=[f"{n}-{B}x{F}" for n, B, F in S.CORR_ROWS])
def test_corr_bar_holds_for_the_emulation_and_resolves_the_defects(name, B, F):
    assert S.form(B, F, pair=False) == name
    x, eps, _ = S.row_inputs(B, F)
    ref = S.reference(x, S.transform(x), eps)
    bar = S.corr_bar(name, ref, B, F)
    err = np.abs(S.emulate_corr(x, eps, S.scheme_of(name)) - ref["corr_x"])
    w, on_diag = float((err / bar).max()), float((np.diag(err) / np.diag(bar)).max())
    print(f"[site-fwd-oracle] corr {name} {B}x{F}: emulation / bar = {w:.3f} (diagonal {on_diag:.3f}), depth {S.acc_depth(B, F)}")
    assert w <= 0.5                                   # the emulation, which has no fp32 accumulation, leaves half the bar or more
    assert S.acc_depth(B, F) <= 200
    # the diagonal of corr is about (B - 1) / B: dividing by F - 1 (up to F = 16384) and a biased std move it by far more than the
    # bar; a dropped eps (2 eps relative) does not clear the split forms' 2^-16 and is left to `stats`
    d = np.diag(ref["corr_x"])
    assert (d / (F - 1) > 4 * np.diag(bar)).all() or F > 16384
    assert (d / (B - 1) > 100 * np.diag(bar)).all()


# ------------------------------------------------------------------------------------------------ the bars on stats and scal
@pytest.mark.parametrize("B,F", [(2, 4096), (5, 70), (28, 4096), (64, 70), (100, 96), (128, 4096), (300, 72)])
def test_stats_bars_hold_for_the_emulated_statistics_and_resolve_the_defects(B, F):
    x, eps, const = S.row_inputs(B, F)
    t = S.transform(x)
    ref = S.reference(x, t, eps)["stats"]
    acc = S.acc_of(B)
    bars, live = S.stats_bars(x, t, eps, acc)
    assert live.sum() == F - (const is not None)
    emu = []
    for v in (x, t):
        m, rho, _ = S._stats32(v, eps, acc=acc)
        emu += [m, rho]
    emu = np.stack(emu).astype(np.float64)
    w = np.abs(emu - ref)[:, live] / bars[:, live]
    print(f"[site-fwd-oracle] stats {B}x{F}: emulated error / bar = {w.max(1)}")
    assert (w <= 1.0).all()
    if const is not None:
        assert emu[1][const] == emu[3][const] == float(S.const_rho(eps)) and emu[0][const] == emu[2][const] == 0.0
    # 1/(std + eps): a biased std, a dropped eps and the mean of the other operand are all outside the bar
    for kw, rows in ((dict(biased=True), (1, 3)), (dict(drop_eps=True), (1, 3) if eps > 0 else ())):
        for i, v in ((1, x), (3, t)):
            if i in rows:
                bad = S._stats32(v, eps, acc=acc, **kw)[1].astype(np.float64)
                assert (np.abs(bad - ref[i])[live] > bars[i][live]).mean() > 0.99, (kw, i)
    assert (np.abs(ref[0] - ref[2])[live] > bars[2][live]).mean() > 0.99


def test_scal_bars_follow_the_bar_on_D():
    B, F = 28, 70
    x, eps, _ = S.row_inputs(B, F)
    t = S.transform(x)
    ref = S.reference(x, t, eps)
    A, Gm = G.admm_params(B, 128, 5)
    bar = S.d_bar("fwd1", ref, 0.0)
    sb = S.scal_bars(ref["D"], bar, A, Gm)
    sc = S.scal_reference(ref["D"], A, Gm)
    rng = np.random.default_rng(0)
    for _ in range(20):                  # any D inside its bar leaves scal inside its own
        D = ref["D"] + bar * rng.uniform(-1, 1, bar.shape)
        assert (np.abs(S.scal_reference(D, A, Gm) - sc) <= sb).all()
    assert (sb[[0, 1, 3]] < 1e-4 * np.abs(sc[[0, 1, 3]])).all() and sb[2] == S.U * sc[2]
    # scal[1..3] are not loose: a loss formed with n = B (B - 1), or an rms without the 1/n, is far outside
    assert abs(0.5 * S.RHO / (B * (B - 1) * sc[3]) - sc[1]) > 100 * sb[1] and abs(sc[3] * B - sc[3]) > 100 * sb[3]


# ------------------------------------------------------------------------------------------------ refusals
def test_forward_entry_points_refuse_without_touching_a_device():
    """every call below returns from the argument checks (site_kernels.hip) before anything is launched; P stands for a non-null
    pointer that is never dereferenced"""
    from alignq_amd import _lib as L
    lib = L.load()
    P, EI, EU = 64, L.EINVAL, L.EUNSUPPORTED
    assert lib.alignq_site_fwd(None, 128, 64, 8, 2.0, 0.0, None, P, None, P, None) == EI             # x
    assert lib.alignq_site_fwd(P, 128, 64, 8, 2.0, 0.0, None, None, None, P, None) == EI             # D
    assert lib.alignq_site_fwd(P, 128, 64, 8, 2.0, 0.0, None, P, None, None, None) == EI             # ws
    assert lib.alignq_site_fwd(P, 128, 0, 8, 2.0, 0.0, None, P, None, P, None) == EI                 # F = 0
    assert lib.alignq_site_fwd(P, 1, 64, 8, 2.0, 0.0, None, P, None, P, None) == EU                  # B = 1
    assert lib.alignq_site_fwd(P, 1025, 64, 8, 2.0, 0.0, None, P, None, P, None) == EU               # beyond the blocked Gram
    assert lib.alignq_site_fwd(P, 128, 64, 17, 2.0, 0.0, None, P, None, P, None) == EI               # k
    assert lib.alignq_site_fwd(P, 128, 64, 0, 2.0, 0.0, None, P, None, P, None) == EI
    assert lib.alignq_site_fwd(P, 300, 64, 8, 2.0, 0.0, None, P, None, P, None) == EI                # above 128 rows stats is required
    assert lib.alignq_site_fwd(P, 300, 64, 17, 2.0, 0.0, None, P, P, P, None) == EI
    assert lib.alignq_site_partials(None, 128, 64, 8, 2.0, 0.0, None, None, P, None) == EI
    assert lib.alignq_site_partials(P, 128, 64, 8, 2.0, 0.0, None, None, None, None) == EI
    assert lib.alignq_site_partials(P, 129, 64, 8, 2.0, 0.0, None, None, P, None) == EU              # the chain stops at 128 rows
    assert lib.alignq_site_partials(P, 128, 64, 31, 2.0, 0.0, None, None, P, None) == EI
    assert lib.alignq_site_reduce(None, 128, 64, P, None) == EI and lib.alignq_site_reduce(P, 128, 64, None, None) == EI
    assert lib.alignq_site_reduce(P, 129, 64, P, None) == EU and lib.alignq_site_reduce(P, 128, 0, P, None) == EI
    assert lib.alignq_site_reduce_loss(P, 128, 64, P, P, P, 127, 0.2, 0.3, P, None) == EI            # dim < B
    assert lib.alignq_site_reduce_loss(P, 128, 64, P, None, P, 128, 0.2, 0.3, P, None) == EI
    assert lib.alignq_site_reduce_loss(P, 128, 64, P, P, P, 128, 0.2, 0.3, None, None) == EI         # scal
    assert lib.alignq_site_reduce_loss(P, 300, 64, P, P, P, 512, 0.2, 0.3, P, None) == EU
    # the small-batch forms stop at 32 rows; C must be a power of two that divides F
    assert lib.alignq_site_partials_res(P, 33, 64, 8, 2.0, 0.0, None, 1, P, None, P, None) == EU
    assert lib.alignq_site_partials_res(P, 28, 64, 8, 2.0, 0.0, None, 1, None, None, P, None) == EI  # y
    assert lib.alignq_site_partials_res_ab(P, P, 8, 33, 64, 8, 2.0, 0.0, None, 1, P, None, P, None) == EU
    assert lib.alignq_site_partials_res_ab(P, P, 6, 28, 60, 8, 2.0, 0.0, None, 1, P, None, P, None) == EI
    assert lib.alignq_site_partials_res_ab(P, P, 8, 28, 60, 8, 2.0, 0.0, None, 1, P, None, P, None) == EI
    assert lib.alignq_site_partials_res_ab(P, None, 8, 28, 64, 8, 2.0, 0.0, None, 1, P, None, P, None) == EI
    assert lib.alignq_site1_groups_fwd(P, P, 8, 28, 64, 0, 8, 2.0, 0.0, None, 1, P, None, P, None) == EI      # groups
    assert lib.alignq_site1_groups_fwd(P, P, 8, 33, 64, 2, 8, 2.0, 0.0, None, 1, P, None, P, None) == EU
    assert lib.alignq_site1_groups_fwd_m(P, P, 8, 28, 64, 2, 8, 2.0, 0.0, None, 1, P, None, P, None, None) == EI   # the mask
    # alignq_corr_fwd: any batch up to 1024, stats required above 128
    assert lib.alignq_corr_fwd(None, 128, 64, 0.0, P, None, P, None) == EI
    assert lib.alignq_corr_fwd(P, 300, 64, 0.0, P, None, P, None) == EI
    assert lib.alignq_corr_fwd(P, 1025, 64, 0.0, P, P, P, None) == EU
    # multi-site reduction: 64 < B <= 128 only; fillers only where alignq_site_fill_slots offers them
    arr = L.ptr_array([None])
    f1 = L.i64_array([64])
    assert lib.alignq_site_reduce_loss_multi(0, arr, arr, arr, arr, arr, f1, 128, 128, 0.2, 0.3, None) == EI
    assert lib.alignq_site_reduce_loss_multi(1, arr, arr, arr, arr, arr, f1, 64, 128, 0.2, 0.3, None) == EU
    assert lib.alignq_site_reduce_loss_multi(1, arr, arr, arr, arr, arr, f1, 128, 128, 0.2, 0.3, None) == EI  # a null site
    assert lib.alignq_site_partials_bn_twin(None, None, None) == EI
    assert S.site_fill_slots(128, 16384) == 0
    assert lib.alignq_site_partials_bn_fill(P, None, None, None, None, None, None, 0.1, 1e-5, P, P, 16, 1024, 128, 16384, 8, 2.0,
                                            0.0, 0, None, 1, 0, P, None, P, P, 1, arr, arr, arr, arr, arr, f1, 128, 0.2, 0.3,
                                            None) == EI
    assert lib.alignq_site_partials_bn_fill(P, None, None, None, None, None, None, 0.1, 1e-5, P, P, 16, 256, 128, 4096, 8, 2.0,
                                            0.0, 0, None, 1, 0, P, None, P, P, 4, arr, arr, arr, arr, arr, f1, 128, 0.2, 0.3,
                                            None) == EI
