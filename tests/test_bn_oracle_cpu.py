"""tests/bn_oracle.py against torch.nn.BatchNorm2d in double and oracle_c.bn_fold_ab; the launch form every row of its matrix claims;
the synthesised layouts against the totals; and every named defect, applied to the restatement, against the bar at the rows meant to
catch it (no GPU)."""
import numpy as np
import pytest
import torch

from tests import bn_oracle as N
from tests import oracle_c as O

TORCH_ROWS = [(17, 3, 4, 0), (5, 65, 8, 0), (3, 16, 21, 1), (7, 128, 19, 1), (2, 8, 33, 1)]


def _to_nchw(z, B, C, HW, nhwc):
    t = torch.from_numpy(np.asarray(z, np.float64))
    return (t.reshape(B, HW, C).permute(0, 2, 1) if nhwc else t.reshape(B, C, HW)).reshape(B, C, HW, 1)


def _from_nchw(t, B, C, HW, nhwc):
    t = t.reshape(B, C, HW)
    return (t.permute(0, 2, 1) if nhwc else t).reshape(B, C * HW).numpy()


@pytest.mark.parametrize("B,C,HW,nhwc", TORCH_ROWS)
@pytest.mark.parametrize("momentum", [0.1, 1.0])
def test_statement_matches_torch_batchnorm_in_double(B, C, HW, nhwc, momentum):
    z, gamma, beta, rm, rv = N.stats_inputs(B, C, HW)
    dx = N.bwd_inputs(B, C, HW)[0]
    bn = torch.nn.BatchNorm2d(C, eps=float(np.float32(1e-5)), momentum=float(np.float32(momentum))).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma.astype(np.float64)))
        bn.bias.copy_(torch.from_numpy(beta.astype(np.float64)))
        bn.running_mean.copy_(torch.from_numpy(rm.astype(np.float64)))
        bn.running_var.copy_(torch.from_numpy(rv.astype(np.float64)))
        bn.num_batches_tracked.fill_(41)
    zt = _to_nchw(z, B, C, HW, nhwc).clone().requires_grad_(True)
    y = bn(zt)
    (y * _to_nchw(dx, B, C, HW, nhwc)).sum().backward()
    ref = N.forward(z, C, nhwc, gamma, beta, rm, rv, 41, momentum, 1e-5)
    ch = N.channel_of(C * HW, C, nhwc)
    x = ref["a"][ch][None, :] * z.astype(np.float64) + ref["b"][ch][None, :]
    np.testing.assert_allclose(x, _from_nchw(y.detach(), B, C, HW, nhwc), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["running_mean"], bn.running_mean.numpy(), rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(ref["running_var"], bn.running_var.numpy(), rtol=1e-13, atol=1e-14)
    assert ref["counter"] == int(bn.num_batches_tracked) == 42
    bw = N.backward(dx, z, C, nhwc, ref["a"], np.stack([ref["mean"], ref["invstd"]]))
    np.testing.assert_allclose(bw["dz"], _from_nchw(zt.grad, B, C, HW, nhwc), rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(bw["dgamma"], bn.weight.grad.numpy(), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(bw["dbeta"], bn.bias.grad.numpy(), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(bw["k0"] * bw["n"], bw["dbeta"], rtol=1e-15)
    np.testing.assert_allclose(bw["k1"] * bw["n"], bw["dgamma"], rtol=1e-15)


def test_gamma_beta_none_are_one_and_zero():
    z = N.stats_inputs(5, 8, 4)[0]
    a = N.forward(z, 8, 1)
    b = N.forward(z, 8, 1, np.ones(8, np.float32), np.zeros(8, np.float32))
    assert np.array_equal(a["a"], b["a"]) and np.array_equal(a["b"], b["b"])
    assert a["running_mean"] is None and a["running_var"] is None


@pytest.mark.parametrize("B,C,HW,nhwc", TORCH_ROWS)
def test_statement_matches_the_c_oracle(B, C, HW, nhwc):
    z, gamma, beta, _, _ = N.stats_inputs(B, C, HW)
    ref = N.forward(z, C, nhwc, gamma, beta)
    bars = N.fwd_bars(ref, invstd_fp32=True)
    ab, save, vu = O.bn_fold_ab(z, C, nhwc, gamma, beta, 1e-5)
    assert N.worst(ab[0], ref["a"], bars["a"]) <= 1.0 and N.worst(ab[1], ref["b"], bars["b"]) <= 1.0
    assert N.worst(save[0], ref["mean"], bars["mean"]) <= 1.0 and N.worst(save[1], ref["invstd"], bars["invstd"]) <= 1.0
    n = ref["n"]
    assert N.worst(vu, ref["vu"], N.SECOND * (2 * N.U * ref["vu"] + bars["dvar"] * n / (n - 1))) <= 1.0


# ---------------------------------------------------------------------------------------------- the forms the rows claim
def test_tile_rules():
    assert N.fwd_tiles(64) == (32, 2, 2, False) and N.fwd_tiles(4096) == (32, 128, 128, False)
    assert N.fwd_tiles(4160) == (64, 65, 65, False) and N.fwd_tiles(16384) == (64, 256, 256, False)
    assert N.fwd_tiles(33024) == (64, 516, 512, True)
    assert [N.bwd_tile_features(F) for F in (32, 16383, 16384, 33024)] == [32, 32, 64, 64]
    assert [N.nhwc_channels_ok(C) for C in (3, 4, 6, 256, 512)] == [False, True, False, True, False]


def test_nchw_statistics_rows_select_their_forms():
    rows = dict((r, N.split_rows(r[0])) for r, _ in N.STATS_NCHW_ROWS)
    assert [b - a for a, b in rows[(1, 1, 4)]] == [1] + [0] * 15
    assert [b - a for a, b in rows[(17, 3, 4)]] == [2] * 8 + [1] + [0] * 7                 # splits 9 to 15 empty
    assert 1028 // 4 == 257 > 256                                                            # a second trip of the row loop
    assert (65 + 63) // 64 == 2                                                              # the finaliser's second block
    for B in (1, 5, 16, 17, 128):
        sp = N.split_rows(B)
        assert sp[0][0] == 0 and all(a <= b for a, b in sp) and sum(b - a for a, b in sp) == B


def test_nhwc_statistics_rows_select_their_forms():
    f = {r: N.nhwc_loop_form(*r) for r, _ in N.STATS_NHWC_ROWS}
    assert f[(1, 4, 1)]["C4"] == 1 and f[(1, 4, 1)]["slots"] == 256 and f[(1, 4, 1)]["empty"] == 63
    assert f[(1, 256, 1)]["C4"] == 64 and f[(1, 256, 1)]["slots"] == 4 and f[(1, 256, 1)]["empty"] == 63
    assert f[(3, 16, 21)]["per"] == 1 and f[(3, 16, 21)]["empty"] == 1
    assert f[(2, 8, 33)]["per"] == 2 and f[(2, 8, 33)]["empty"] == 31
    assert f[(1, 4, 131077)]["per"] == 2049 and f[(1, 4, 131077)]["trips"] == 2 and f[(1, 4, 131077)]["ragged"]
    assert f[(1, 256, 2051)]["per"] == 33 and f[(1, 256, 2051)]["trips"] == 2
    assert sorted(v["C4"] for v in f.values()) == [1, 1, 2, 4, 8, 16, 32, 64, 64]
    for (B, C, HW), _ in N.STATS_NHWC_ROWS:
        rng = N.pixel_ranges(B * HW)
        assert len(rng) == 64 and sum(b - a for a, b in rng) == B * HW


def test_backward_rows_select_their_forms():
    f = {r: N.bwd_stage1_form(*r) for r, _ in N.BWD_NHWC_ROWS}
    a = f[(2, 4, 16)]
    assert (a["cp"], a["cnt"], a["groups"], a["cyc"]) == (4, 2, 64, 1) and a["cnt"] < a["groups"]
    a = f[(3, 256, 1)]
    assert (a["cp"], a["cyc"], a["cnt"], a["groups"]) == (32, 8, 1, 1)
    a = f[(2, 256, 9)]
    assert a["cnt"] == 9 and a["groups"] == 1 and a["rounds"] == 2
    a = f[(2, 64, 256)]
    assert (a["tile"], a["cp"], a["cyc"]) == (64, 64, 1)
    a = f[(1, 4, 8208)]
    assert a["tile"] == 64 and a["cnt"] == 513 and a["groups"] == 64 and a["rounds"] == 2      # cnt > 8 * groups
    a = f[(5, 16, 20)]
    assert a["per"] == 4 and a["idle_blocks"] == 28
    a = f[(2, 256, 1025)]
    assert a["per"] == 1025 and a["stage2_trips"] == 2 and (a["tile"], a["cyc"]) == (64, 4)
    assert {f[r]["cyc"] for r in f} == {1, 4, 8}
    for (B, C, HW), _ in N.BWD_NCHW_ROWS:
        assert HW % 64 == 0
    tpc = {r: r[2] // N.bwd_tile_features(r[1] * r[2]) for r, _ in N.BWD_NCHW_ROWS}
    assert tpc[(1, 1, 64)] == 2 and tpc[(2, 1, 16384)] == 256 and 1088 // 4 == 272 > 256
    assert N.bwd_tile_features(1 * 16384) == 64


# ---------------------------------------------------------------------------------------------- layouts sum back to the totals
@pytest.mark.parametrize("row", [r for r, _ in N.STATS_NCHW_ROWS], ids=N.row_id)
def test_nchw_double_parts_sum_to_the_totals(row):
    B, C, HW = row
    z = N.stats_inputs(B, C, HW)[0]
    parts, _, cnt = N.double_parts_nchw(z, C)
    ref = N.forward(z, C, 0)
    assert cnt.sum() == B * HW
    np.testing.assert_allclose(parts[:, :, 0].sum(1), ref["mean"] * ref["n"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(parts[:, :, 1].sum(1), ref["sq"], rtol=1e-12)


@pytest.mark.parametrize("row", [r for r, _ in N.STATS_NHWC_ROWS if r[2] < 5000], ids=N.row_id)
def test_nhwc_parts_sum_to_the_totals(row):
    B, C, HW = row
    z = N.stats_inputs(B, C, HW)[0]
    ref = N.forward(z, C, 1)
    parts, _, cnt = N.double_parts_nhwc(z, C)
    assert cnt.sum() == B * HW
    np.testing.assert_allclose(parts[:, :, 1].sum(1), ref["sq"], rtol=1e-12)
    for n_parts in (1, 2, 7, 258, 515):
        fp = N.synth_float_parts(z, C, n_parts)
        assert fp.shape == (C, n_parts, 2) and fp.dtype == np.float32
        tot = N.finalize_from_parts(fp, ref["n"], C, 32)
        assert np.all(np.abs(tot[:, 1] - ref["sq"]) <= N.U * np.abs(fp[:, :, 1].astype(np.float64)).sum(1) * 1.01 + 1e-300)
        assert np.all(np.abs(tot[:, 0] - ref["mean"] * ref["n"]) <= N.U * np.abs(fp[:, :, 0].astype(np.float64)).sum(1) * 1.01 + 1e-300)


@pytest.mark.parametrize("nhwc,row", [(1, r) for r, _ in N.BWD_NHWC_ROWS] + [(0, r) for r, _ in N.BWD_NCHW_ROWS],
                         ids=lambda v: N.row_id(v) if isinstance(v, tuple) else str(v))
def test_dx_part_sums_to_the_totals(nhwc, row):
    B, C, HW = row
    dx, z, ab, save = N.bwd_inputs(B, C, HW)
    bw = N.backward(dx, z, C, nhwc, ab[0], save)
    exact = N.dx_part_exact(dx, bw["zhat"], C, nhwc)
    assert exact.shape == N.dx_part_shape(B, C, HW, nhwc)
    tot, _ = N.totals_from_dx_part(exact, B, C, HW, nhwc)
    np.testing.assert_allclose(tot[:, 0], bw["dbeta"], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(tot[:, 1], bw["dgamma"], rtol=1e-10, atol=1e-14)
    # the channels-last entry of channel c: restated independently, feature by feature
    if nhwc and B * C * HW <= 20000:
        tf = N.bwd_tile_features(C * HW)
        cols = dx.astype(np.float64).sum(0)
        again = np.zeros(exact.shape[:2])
        for f in range(C * HW):
            again[f // tf, (f % C) % tf] += cols[f]
        np.testing.assert_allclose(again, exact[:, :, 0], rtol=1e-12, atol=1e-15)
    part = N.synth_dx_part(dx, bw["zhat"], C, nhwc)
    tot32, ab32 = N.totals_from_dx_part(part, B, C, HW, nhwc)
    for j, name in enumerate(("dbeta", "dgamma")):
        bar, _ = N.totals_bar(bw[name], ab32[:, j], part.shape[0], bw["n"])
        assert N.worst(tot32[:, j], bw[name], bar) <= 1.0


# ---------------------------------------------------------------------------------------------- the defects leave the bars
WIDE = 20.0


@pytest.mark.parametrize("row", [(1, 4, 131077), (1, 256, 2051)], ids=N.row_id)
def test_defect_last_load_of_the_round_dropped(row):
    B, C, HW = row
    z = N.stats_inputs(B, C, HW)[0]
    good, abs_, cnt = N.double_parts_nhwc(z, C)
    bad, _, _ = N.double_parts_nhwc(z, C, defect="nhwc_last_load_dropped")
    assert N.worst(bad, good, N.part_bar(abs_, cnt)) > 1e6
    # every other row of the matrix ends inside the first seven loads of the first round: the defect is silent there
    for (b, c, hw), _ in N.STATS_NHWC_ROWS:
        f = N.nhwc_loop_form(b, c, hw)
        assert (f["per"] > 7 * f["slots"]) == ((b, c, hw) in ((1, 4, 131077), (1, 256, 2051)))


@pytest.mark.parametrize("B,C,HW", [(100, 64, 1), (128, 256, 1), (128, 32, 16)])
def test_defect_second_channel_of_a_pair_reads_the_first(B, C, HW):
    z, gamma, beta, _, _ = N.stats_inputs(B, C, HW)
    ref = N.forward(z, C, 1, gamma, beta)
    parts, _, _ = N.double_parts_nhwc(z, C)
    tile = N.fwd_tiles(C * HW)[0]
    assert tile == 32
    bars = N.fwd_bars(ref, invstd_fp32=True)
    mean, var = N.moments_from_totals(N.finalize_from_parts(parts, ref["n"], C, tile), ref["n"])
    assert N.worst(mean, ref["mean"], bars["mean"]) <= 1.0
    mean, var = N.moments_from_totals(N.finalize_from_parts(parts, ref["n"], C, tile, defect="pair_reads_first"), ref["n"])
    assert N.worst(mean, ref["mean"], bars["mean"]) > 1e3


@pytest.mark.parametrize("B,C,HW,n_parts", [(100, 64, 1, 258), (100, 64, 1, 259), (65, 128, 33, 514), (65, 128, 33, 515)])
def test_defect_float_partial_loop_runs_one_round(B, C, HW, n_parts):
    z, gamma, beta, _, _ = N.stats_inputs(B, C, HW)
    ref = N.forward(z, C, 1, gamma, beta)
    tile = N.fwd_tiles(C * HW)[0]
    fp = N.synth_float_parts(z, C, n_parts)
    bars = N.fwd_bars(ref, invstd_fp32=True, float_parts=fp)
    assert n_parts > (256 if tile == 32 else 512)
    _, var = N.moments_from_totals(N.finalize_from_parts(fp, ref["n"], C, tile), ref["n"])
    assert float((np.abs(var - ref["var"]) / bars["dvar"]).max()) <= 1.01
    _, var = N.moments_from_totals(N.finalize_from_parts(fp, ref["n"], C, tile, defect="float_parts_one_round"), ref["n"])
    assert float((np.abs(var - ref["var"]) / bars["dvar"]).min()) > WIDE


@pytest.mark.parametrize("row", [r for r, _ in N.BWD_NHWC_ROWS if N.bwd_stage1_form(*r)["cyc"] > 1], ids=N.row_id)
def test_defect_t_first_zero(row):
    B, C, HW = row
    assert row in ((3, 256, 1), (2, 256, 9), (2, 256, 1025))
    dx, z, ab, save = N.bwd_inputs(B, C, HW)
    bw = N.backward(dx, z, C, 1, ab[0], save)
    part = N.synth_dx_part(dx, bw["zhat"], C, 1)
    tot, abs_ = N.totals_from_dx_part(part, B, C, HW, 1, defect="t_first_zero")
    for j, name in enumerate(("dbeta", "dgamma")):
        bar, _ = N.totals_bar(bw[name], abs_[:, j], part.shape[0], bw["n"])
        ratio = np.abs(tot[:, j] - bw[name]) / bar
        cp = N.bwd_stage1_form(B, C, HW)["cp"]                     # every channel behind the first tile of a cycle is wrong
        assert float(ratio[cp:].min() if name == "dbeta" else np.median(ratio[cp:])) > WIDE


@pytest.mark.parametrize("row", [r for r, _ in N.BWD_NCHW_ROWS], ids=N.row_id)
def test_defect_one_tile_short_in_the_nchw_backward(row):
    B, C, HW = row
    dx, z, ab, save = N.bwd_inputs(B, C, HW)
    bw = N.backward(dx, z, C, 0, ab[0], save)
    part = N.synth_dx_part(dx, bw["zhat"], C, 0)
    tot, abs_ = N.totals_from_dx_part(part, B, C, HW, 0, defect="tpc_minus_one")
    bar, _ = N.totals_bar(bw["dbeta"], abs_[:, 0], part.shape[0], bw["n"])
    assert float((np.abs(tot[:, 0] - bw["dbeta"]) / bar).min()) > WIDE      # dx has mean 0.002: the missing tile's sum is never small


@pytest.mark.parametrize("row", [r for r, _ in N.STATS_NCHW_ROWS], ids=N.row_id)
@pytest.mark.parametrize("momentum", [0.1, 1.0])
def test_defect_running_var_from_the_biased_variance(row, momentum):
    B, C, HW = row
    z, gamma, beta, rm, rv = N.stats_inputs(B, C, HW)
    ref = N.forward(z, C, 0, gamma, beta, rm, rv, 0, momentum)
    bad = N.forward(z, C, 0, gamma, beta, rm, rv, 0, momentum, defect="running_var_biased")
    bars = N.fwd_bars(ref, invstd_fp32=False)
    assert float((np.abs(bad["running_var"] - ref["running_var"]) / bars["running_var"]).min()) > WIDE
