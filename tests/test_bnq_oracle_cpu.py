"""tests/bnq_oracle.py checked on the CPU: the case table selects the launch forms it names, its inputs keep the statistics exact,
the restated statistics and the float64 backward agree with independent statements (longdouble two-pass, torch.autograd), a
float32 evaluation of the kernels' operations stays below every bar and the planted defects exceed them."""
import numpy as np
import pytest
import torch

from tests import bnq_oracle as B

ROW_IDS = [B.row_id(r) for r in B.ROWS]
SMALL = [i for i, r in enumerate(B.ROWS) if r[0] * r[1] * r[2] <= 300_000]


def test_every_branch_is_taken_by_a_row():
    taken = set()
    for row in B.ROWS:
        d = B.row_dict(row)
        t = B.branches(d["groups"], d["P"], d["C"])
        assert d["branch"] in t, (row, sorted(t))            # the row selects the branch its comment names
        assert not B.bad_c(d["C"]) and 1 <= d["groups"] <= B.MAX_GROUPS and d["P"] >= 2
        if d["bins"]:
            assert d["formula"] == 0 and not d["residual"] and d["k"] <= 14 and d["r"] * (2 ** d["k"] - 1) <= 32767
        taken |= t
    for groups, cp in B.PARTS_ROWS:
        taken |= B.branches(groups, B.PARTS_P, B.PARTS_C, cp)
    assert B.fin_small(B.PARTS_P, B.PARTS_C, 1)
    missing = [b for b in B.REQUIRED_BRANCHES if b not in taken]
    assert not missing, missing
    # the geometry the issue's comments name
    assert B.fin_parts(4100, 64) == 32 and B.fin_parts(70000, 4) == 34
    assert B.parts_for(70000, 64) == B.parts_for(9000, 512) == B.K_PARTS and B.parts_for(3000, 1024) == 256
    assert B.parts_for(700, 2048) == 128 and B.parts_for(2, 2048) == 1 and B.threads_for(2048) == 512 and B.threads_for(1024) == 256
    assert 65536 * 64 == 4 << 20 and B.fin_small(65536, 64, 1) and not B.fin_small(70000, 64, 1)
    assert [B.finalize_u(n) for n in (1, 63, 512, 513, 686, 768, 769, 1100)] == [8, 8, 8, 12, 12, 12, 8, 8]
    assert max(r[0] * r[1] * r[2] for r in B.ROWS) < 6.2e6


def test_every_mode_appears_in_every_family():
    fam = {"in": [], "gen": [], "512": []}
    for row in B.ROWS:
        d = B.row_dict(row)
        key = "in" if B.fin_small(d["P"], d["C"], d["groups"]) else ("512" if B.threads_for(d["C"]) == 512 else "gen")
        fam[key].append(d)
    for key, rows in fam.items():
        for field, values in (("formula", (0, 1)), ("relu", (0, 1)), ("residual", (1,)), ("mask", (1,)), ("bins", ("y", "noy")),
                              ("k", (1, 2, 4, 8, 16, 32)), ("r", (2.0, 10.0)), ("nulls", (1,))):
            for v in values:
                assert any(d[field] == v for d in rows), (key, field, v)


@pytest.mark.parametrize("i", range(len(B.ROWS)), ids=ROW_IDS)
def test_inputs_keep_the_statistics_exact_and_restatement_matches_two_pass(i):
    case = B.case_of(B.ROWS[i], i)
    z = case["z"]
    assert np.array_equal(z * 256.0, np.round(z * 256.0)) and np.abs(z).max() <= 8.0
    assert B.sum_q_units(z) < 2.0 ** 53 and case["P"] <= 2 ** 20
    st = B.case_stats(case)
    zl = z.astype(np.longdouble)
    mean = zl.mean(axis=1)
    var = ((zl - mean[:, None, :]) ** 2).mean(axis=1)
    ch = case["ch"]
    assert np.all(st["var"][:, ch["const"]] == 0.0)                                   # the clamp (or an exact 0)
    if case["P"] >= 30:
        assert np.all(np.abs(np.sqrt(st["var"][:, ch["cancel"]]) * 64.0 - 1.0) < 0.5)
    assert np.all(np.abs(mean[:, ch["cancel"]] - 6.0) < 0.1)
    np.testing.assert_allclose(st["save"][:, 0], mean.astype(np.float64), rtol=2.0 ** -23, atol=2.0 ** -30)
    invstd = 1.0 / np.sqrt(var + np.longdouble(B.BN_EPS))
    rel = np.abs(1.0 / np.sqrt(st["var"] + np.float64(B.BN_EPS)) - invstd) / invstd
    relv = np.abs(st["var"] - var) / np.where(var > 0, var, 1.0)
    print(f"{B.row_id(B.ROWS[i])}: one-pass vs two-pass longdouble, worst relative difference: variance {float(relv.max()):.2e}, "
          f"invstd {float(rel.max()):.2e}")
    assert float(rel.max()) <= 1e-9 and float(relv.max()) <= 1e-9
    if case["gamma"] is not None:
        assert case["gamma"][ch["gamma0"]] == 0 and abs(case["gamma"][ch["tiny"]]) == np.float32(1e-3) * abs(case["beta"][ch["tiny"]])


def test_partials_sum_to_the_totals_exactly():
    z = B.make_z(3, B.PARTS_P, B.PARTS_C, 5)
    for cp in (1, 63, 1100):
        part = B.random_partials(z, cp, cp)
        s, q = B.totals(z)
        assert np.array_equal(part[..., 0].sum(axis=1), s) and np.array_equal(part[..., 1].sum(axis=1), q)
        assert np.array_equal(part[:, ::-1, :, 0].sum(axis=1), s)                     # in any order


def _device_like(i):
    """(row, case, statistics, g, pos, x, zhat, a): what the GPU test forms, with the restated (a, b) in the device's place"""
    row = B.ROWS[i]
    d, case = B.row_dict(row), B.case_of(row, i)
    st = B.case_stats(case)
    y, _, _ = B.fwd_ref(case["z"], st["ab"], d["formula"], d["relu"], d["k"], d["r"], case["res"])
    pos = (y > 0) if d["relu"] else None
    g = B.make_g(case["z"], st["save"], i)
    x, zhat, a = B.ref_inputs(case["z"], st["ab"], st["save"])
    return d, case, st, g, pos, x, zhat, a


@pytest.mark.parametrize("i", [2, 10, 14], ids=[ROW_IDS[i] for i in (2, 10, 14)])
def test_float64_backward_agrees_with_torch_autograd(i):
    d, case, st, g, pos, _, _, _ = _device_like(i)
    z, groups, P, C = case["z"], case["groups"], case["P"], case["C"]
    dz, dgam, dbet = np.empty(z.shape), np.zeros(C), np.zeros(C)
    s, q = B.totals(z)
    mean = s / P
    # two-pass variance like torch's (the one-pass form's 1e-11 on the cancellation channel is the statistics test's subject)
    invstd = 1.0 / np.sqrt(((z - mean[:, None, :]) ** 2).mean(axis=1) + np.float64(B.BN_EPS))
    gam64, bet64 = case["gamma"].astype(np.float64), case["beta"].astype(np.float64)
    a = gam64 * invstd
    x = a[:, None, :] * (z - mean[:, None, :]) + bet64
    zhat = (z - mean[:, None, :]) * invstd[:, None, :]
    ref = B.bwd_ref(g, x, zhat, a, pos, d["r"])
    for gi in range(groups):
        bn = torch.nn.BatchNorm2d(C, eps=float(B.BN_EPS)).double().train()
        with torch.no_grad():
            bn.weight.copy_(torch.from_numpy(gam64)); bn.bias.copy_(torch.from_numpy(bet64))
        zt = torch.from_numpy(z[gi].astype(np.float64).T.reshape(1, C, P, 1).copy()).requires_grad_(True)
        t = d["r"] * torch.erf(bn(zt) / np.sqrt(2.0))
        m = torch.ones_like(t) if pos is None else torch.from_numpy(pos[gi].T.reshape(1, C, P, 1).astype(np.float64))
        (t * m * torch.from_numpy(g[gi].astype(np.float64).T.reshape(1, C, P, 1).copy())).sum().backward()
        dz[gi] = zt.grad.numpy().reshape(C, P).T
        dgam += bn.weight.grad.numpy(); dbet += bn.bias.grad.numpy()
    ok = np.ones(C, bool)
    ok[case["ch"]["const"]] = False      # var == 0: torch's invstd comes from its own variance pass; compared separately below
    scale = np.abs(ref["dz"][:, :, ok]).max()
    assert np.abs(dz - ref["dz"])[:, :, ok].max() <= 1e-12 * scale
    assert np.abs(dz - ref["dz"])[:, :, ~ok].max() <= 1e-9 * np.abs(ref["dz"][:, :, ~ok]).max()
    np.testing.assert_allclose(dgam[ok], ref["dgamma"][ok], rtol=1e-12, atol=1e-12 * np.abs(ref["dgamma"]).max())
    np.testing.assert_allclose(dbet, ref["dbeta"], rtol=1e-12, atol=1e-12 * np.abs(ref["dbeta"]).max())


@pytest.mark.parametrize("i", SMALL, ids=[ROW_IDS[i] for i in SMALL])
def test_float32_evaluation_stays_below_every_bar(i):
    d, case, st, g, pos, x, zhat, a = _device_like(i)
    if pos is not None and case["C"] >= 16:
        ch = case["ch"]
        vary = np.ones(case["C"], bool)
        vary[[ch["const"], ch["gamma0"], ch["tiny"]]] = False          # x is one value per channel there: all or nothing
        zeros = 1.0 - pos[:, :, vary].mean()
        print(f"{ROW_IDS[i]}: {100 * zeros:.1f} % of the mask is zero on the channels whose x varies")
        assert 0.4 <= zeros <= 0.6
    for from_dx in (False, True):
        ref = B.bwd_ref(g, x, zhat, a, pos, d["r"], from_dx)
        emu = B.emulate32(g, case["z"], st["ab"], st["save"], pos, d["r"], from_dx)
        w = {n: B.worst(emu[n], ref[n], ref["bar_" + n]) for n in ("dz", "dgamma", "dbeta")}
        print(f"{ROW_IDS[i]} from_dx={from_dx}: worst error / bar " + ", ".join(f"{n} {v:.3f}" for n, v in w.items()))
        assert max(w.values()) < 1.0, w
        if case["gamma"] is not None:
            assert not emu["dz"][:, :, case["ch"]["gamma0"]].any()                     # +0 or -0


@pytest.mark.parametrize("i", range(len(B.ROWS)), ids=ROW_IDS)
def test_planted_defects_exceed_the_bar(i):
    d, case, st, g, pos, x, zhat, a = _device_like(i)
    ref = B.bwd_ref(g, x, zhat, a, pos, d["r"])
    assert B.worst(ref["dz"], ref["dz"], ref["bar_dz"]) == 0.0
    for name in B.DEFECTS:
        bad = B.planted(name, ref, zhat, a, pos, g, x, d["r"], case["P"], case["C"], case["groups"])
        if bad is None:
            continue
        w = B.worst(bad, ref["dz"], ref["bar_dz"])
        print(f"{ROW_IDS[i]} {name}: worst error / bar = {w:.3e}")
        assert w > 100.0, (name, w)


def test_every_defect_exists_on_some_row_and_forward_defects_change_bits():
    assert any(r[0] >= 3 and r[0] % 2 for r in B.ROWS) and any(r[4] for r in B.ROWS)
    # the forward's side of two of them: a skipped partial or the neighbouring slice's statistics change (a, b) in their bits
    case = B.make_case(3, 130, 256, 0, 0, 14)
    st = B.case_stats(case)
    s, q = B.totals(case["z"])
    p0 = B.last_partial(130, 256, 3)
    s2, q2 = B.totals(case["z"][:, :p0])
    assert p0 < 130 and not np.array_equal(B.case_stats(case, (s2, q2))["ab"].view(np.uint32), st["ab"].view(np.uint32))
    assert not np.array_equal(st["ab"][2].view(np.uint32), st["ab"][1].view(np.uint32))


def test_mask_layout():
    y = np.zeros((2, 75, 4), np.float32)
    y[0, 0, 1] = 1.0; y[0, 64, 3] = 2.0; y[1, 74, 0] = 3.0; y[1, 5, 2] = -1.0
    m = B.mask_ref(y)
    assert m.shape == (2, B.mask_words(75)) == (2, 8)
    want = np.zeros((2, 8), np.uint64)
    want[0, 1] = 1; want[0, 4 + 3] = 1; want[1, 4 + 0] = 1 << 10
    assert np.array_equal(m, want)
