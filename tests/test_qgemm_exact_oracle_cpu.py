"""The oracle of tests/test_gpu_qgemm_exact.py, checked without a GPU: the new references against float64 conv2d /
convolution_backward, the float64 large-case form against the int64 form, and - for EVERY case of the shared table
(tests/qgemm_exact_oracle.py) - the 2^24 budget, the term classes the operands claim, the sparse pixels' placement and the
round trip of every level tensor.  The large dense cases' budgets are checked analytically (max|activation| * the largest sum of
|bins| over a contraction), not with a full convolution."""
import pytest
import torch
import torch.nn.functional as F

from tests import qgemm_exact_oracle as O


def _ids(cases):
    return [c["id"] for c in cases]


# --------------------------------------------------------------------------------------- references against float64 torch
@pytest.mark.parametrize("B,h,w", [(1, 8, 8), (2, 9, 11), (2, 12, 10)])
def test_stem7_references_match_float64_conv2d(B, h, w):
    g = torch.Generator().manual_seed(h)
    x = torch.randint(-9, 10, (B, h, w, 3), generator=g, dtype=torch.int64)
    b = torch.randint(-9, 10, (64, 7, 7, 3), generator=g, dtype=torch.int64)
    xt, bt = x.permute(0, 3, 1, 2).double(), b.permute(0, 3, 1, 2).double().requires_grad_(True)
    y = F.conv2d(xt, bt, stride=2, padding=3)
    ref = O.stem7_fwd_i64(x, b)
    assert tuple(ref.shape) == (B, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 64)
    assert torch.equal(y.detach().permute(0, 2, 3, 1), ref.double())
    dy = torch.randint(-9, 10, ref.shape, generator=g, dtype=torch.int64)
    y.backward(dy.permute(0, 3, 1, 2).double())
    assert torch.equal(bt.grad.permute(0, 2, 3, 1).reshape(-1), O.stem7_wgrad_i64(x, dy).double())


@pytest.mark.parametrize("ks,stride,h,w", [(1, 1, 5, 7), (1, 2, 7, 7), (1, 2, 7, 8), (3, 1, 3, 5), (3, 2, 4, 6), (3, 2, 7, 9)])
def test_references_on_odd_grids_and_the_float64_form(ks, stride, h, w):
    """the generic int64 references at the odd sizes this table uses (Ho = (H - 1) / stride + 1), against convolution_backward, and
    the float64 large-case form equal to the int64 form"""
    g = torch.Generator().manual_seed(ks + stride + h)
    pad = (ks - 1) // 2
    x = torch.randint(-99, 100, (2, h, w, 8), generator=g, dtype=torch.int64)
    b = torch.randint(-99, 100, (6, ks, ks, 8), generator=g, dtype=torch.int64)
    xt, bt = x.permute(0, 3, 1, 2).double(), b.permute(0, 3, 1, 2).double()
    y = F.conv2d(xt, bt, stride=stride, padding=pad).permute(0, 2, 3, 1)
    ref = O.conv_i64(x, b, stride, pad)
    assert tuple(ref.shape) == (2, (h - 1) // stride + 1, (w - 1) // stride + 1, 6)
    assert torch.equal(y, ref.double()) and torch.equal(O.conv_f64(x, b, stride, pad), ref.double())
    dy = torch.randint(-99, 100, ref.shape, generator=g, dtype=torch.int64)
    dx, dw = torch.ops.aten.convolution_backward(dy.permute(0, 3, 1, 2).double(), xt, bt, None, (stride, stride), (pad, pad), (1, 1),
                                                 False, (0, 0), 1, (True, True, False))[:2]
    di = O.dgrad_i64(dy, b, stride, pad, h, w)
    assert torch.equal(dx.permute(0, 2, 3, 1), di.double()) and torch.equal(O.dgrad_f64(dy, b, stride, pad, h, w), di.double())
    assert torch.equal(dw.permute(0, 2, 3, 1), O.wgrad_i64(x, dy, ks, stride, pad).double())


def test_quotient_is_one_fp32_division():
    t = torch.tensor([0, 1, 254, 255, 65279, (1 << 24) - 1, -12345], dtype=torch.int64)
    q = O.quotient(t, 255.0)
    assert q.dtype == torch.float32 and torch.equal(q, t.float() / torch.tensor(255.0))
    assert torch.equal(O.quotient(t, 255.0, 255.0), t.float() / torch.tensor(65025.0))
    assert torch.equal(O.quotient(t.double(), 1.0), t.float())


# --------------------------------------------------------------------------------- forward and data gradient (qgemm_kernel)
@pytest.mark.parametrize("c", O.G_CASES + O.BN, ids=_ids(O.G_CASES + O.BN))
def test_forward_and_data_gradient_cases_keep_the_budget_and_their_classes(c):
    a, b = O.g_operands(c)
    nlev = int(O.nlev_of(c))
    assert int(b.abs().max()) <= nlev and c["cin"] % 64 == 0 and c["cout"] % 64 == 0
    if c["big"] or c["set"] == "dense":
        worst = O.g_budget_bound(c, a, b)
        assert worst < O.TWO24, worst
    if not c["big"]:
        p = O.pad_of(c)
        if c["op"] == "fwd":
            O.assert_exact_budget(O.conv_i64, a, b, stride=c["stride"], pad=p)
        else:
            O.assert_exact_budget(O.dgrad_i64, a, b, stride=c["stride"], pad=p, h_in=c["h"], w_in=c["w"])
    if c["set"] == "act3":
        second, third = O.class_fractions(a)
        assert second == 1.0 and third > 0.3
        # every 64-column tile of the output meets a non-zero bin in every tap and every 64-channel chunk of the contraction
        bb = b if c["op"] == "fwd" else b.permute(3, 1, 2, 0)          # [output column, ky, kx, contraction channel]
        nz = (bb != 0).reshape(bb.shape[0] // 64, 64, c["ks"] ** 2, bb.shape[3] // 64, 64)
        assert bool(nz.any(dim=4).any(dim=1).all())
    elif c["mode"] == "f32":
        assert O.class_fractions(a) == (0.0, 0.0)                      # class 1: one bf16 term
    else:
        assert int(a.min()) >= 0 and 1024 < int(a.max()) <= O.IDX_TOP         # f16 holds every index exactly
        assert torch.equal(a.to(torch.float16).to(torch.int64), a)
        x = a.to(torch.float32) / torch.tensor(O.XLEV_FWD)
        assert torch.equal(torch.round(x * torch.tensor(O.XLEV_FWD)).to(torch.int64), a)
    if c in O.BN:          # y, y^2 and a lane's sum of four of them are exact fp32 integers
        K = O.contraction(c)
        assert nlev == 1 and 4 * (3 * K) ** 2 < O.TWO24


def test_batch_norm_partials_reference_sums_each_tile():
    y = torch.arange(2 * 5 * 7 * 2, dtype=torch.int64).reshape(2, 5, 7, 2) - 30
    e = O.bn_expected(y, 2, 16)
    assert tuple(e.shape) == (2, 3, 2, 2)
    rows = y.reshape(2, 35, 2)
    assert torch.equal(e[1, 2, :, 0], rows[1, 32:35].sum(0)) and torch.equal(e[0, 1, :, 1], (rows[0, 16:32] ** 2).sum(0))
    assert torch.equal(e.sum(1)[..., 0], rows.sum(1))
    s = O.stem_bn_expected(torch.ones(2, 19, 21, 64, dtype=torch.int64), 2)          # Mg = 399: 25 tiles, 7 workgroups per group
    assert tuple(s.shape) == (2, 7, 64, 2) and int(s[..., 0].sum()) == 2 * 399 * 64
    assert int(s[0, 0, 0, 0]) == 64 and int(s[0, 6, 0, 0]) == 15          # tiles 0-3 | tile 24 with 15 rows


# ------------------------------------------------------------------------------------------------------- filter gradient
@pytest.mark.parametrize("c", O.ALL_WGRAD + O.STEM_WGRAD + O.STEM_WGRAD_PAIRS, ids=_ids(O.ALL_WGRAD + O.STEM_WGRAD + O.STEM_WGRAD_PAIRS))
def test_filter_gradient_cases_keep_the_budget_and_their_classes(c):
    stem = c["op"] == "stem_wgrad"
    x, dy = O.stem_operands(c) if stem else O.wgrad_operands(c)
    O.assert_exact_budget(O.wgrad_i64, x, dy, ks=c["ks"], stride=c["stride"], pad=O.pad_of(c))
    ho, wo = O.out_hw(c)
    M = c["B"] * ho * wo
    assert (stem or (M % 32 and M % c["per"])) and M <= c["splits"] * c["per"]
    assert (c["splits"] - 1) * c["per"] < M or (stem and c["splits"] == 512 and c["per"] == 32 * -(-(-(-M // 32)) // 512))
    s = c["set"]
    if s in ("dense", "lev255"):
        assert O.class_fractions(dy) == (0.0, 0.0)
    if c["mode"] != "f32":
        xlev = torch.tensor(O.wgrad_xlev(c))
        xt = x.to(torch.float32) / xlev
        assert torch.equal(torch.round(xt * xlev).to(torch.int64), x) and int(x.min()) >= 0 and int(x.max()) < 1 << 15
        if float(xlev) == 256.0:
            assert torch.equal(xt.double() * 256.0, x.double())          # idx / 256 is exact
        hi, lo, rest = O.bf16_terms(x)
        assert torch.equal(hi.double() + lo.double(), x.double()) and not bool(rest.any())      # two exact bf16 terms
    if s == "lev22":
        assert O.class_fractions(dy) == (1.0, 0.0) and O.class_fractions(x)[0] == 1.0 and int(x.min()) >= 257 and int(x.max()) >= 1024
    if s == "lev3":
        assert O.class_fractions(dy)[1] > 0.3 and int(x.max()) == 3 and O.class_fractions(x) == (0.0, 0.0)
    if s.startswith("dy"):
        want = {1: (0.0, 0.0), 2: (1.0, 0.0)}
        for cls, t in ((int(s[2]), dy), (int(s[5]), x)):
            f = O.class_fractions(t)
            assert (f[0] == 1.0 and f[1] > 0.3) if cls == 3 else f == want[cls]
    if s.startswith("dy") or s in ("lev22", "lev3"):
        nzp = (dy.reshape(M, -1) != 0)
        assert int(nzp.sum(0).max()) <= O.SPARSE_K and int(nzp.sum(0).min()) >= 5
        hit = nzp.any(1)
        per = c["per"]
        kinds = [0, wo - 1, (ho - 1) * wo, ho * wo - 1, M - 1, per - 1, per]
        assert all(bool(hit[p]) for p in kinds)
        for blk in range(8):          # every 4-pixel row block of the step; every row of it in some channel (lev22 keeps a third)
            rows = hit[per + 4 * blk:per + 4 * blk + 4]
            assert bool(rows.any() if s == "lev22" else rows.all())


def test_pixel_chooser_places_what_it_says():
    c = O.WGRAD_SHAPES[6]          # 3x3 stride 2, dy 4 x 5, B = 5: M = 100, per = 64
    for co in (0, 1, 5, 127):
        px = O.wgrad_pixels(c, co)
        assert {0, 4, 15, 19, 99, 63, 64} <= set(px) and len(px) <= O.SPARSE_K
        assert sorted({(p - 64) // 4 for p in px if 64 <= p < 96}) == list(range(8))


# --------------------------------------------------------------------------------------------------------------- the stem
@pytest.mark.parametrize("c", O.STEM_FWD + O.STEM_BN, ids=_ids(O.STEM_FWD + O.STEM_BN))
def test_stem_forward_cases_keep_the_budget_and_their_classes(c):
    x, b = O.stem_operands(c)
    O.assert_exact_budget(O.conv_i64, x, b, stride=2, pad=3)
    assert int(b.abs().max()) <= int(O.nlev_of(c))
    if c["set"] == "act3":
        second, third = O.class_fractions(x)
        assert second == 1.0 and third > 0.3
        assert bool((b != 0).any(0).all())          # every tap and input channel meets a non-zero bin in some output channel
    else:
        assert O.class_fractions(x) == (0.0, 0.0)
    if c["w_bit"] == 1:          # a lane's sums over its (at most two) tiles, then over the four waves: 8 values of y^2 <= (3 * 147)^2
        ho, wo = O.out_hw(c)
        assert c["B"] // c["groups"] * ho * wo <= 2 * 16 * 2048 and 8 * (3 * 147) ** 2 < O.TWO24
