"""The exact-integer oracle of the convolution gradient tests, checked without a GPU: each int64 reference against
torch.nn.functional.conv2d (forward and autograd) in float64, the bf16 split, and - for EVERY parametrised case of
tests/test_gpu_conv_grads_exact.py, from the shared case table - that the generated operands have the term class they claim and
stay inside the 2^24 budget that makes the GPU comparison independent of the accumulation order."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_exact_oracle as O


def _ids(cases):
    return [c["id"] for c in cases]


# --------------------------------------------------------------------------------------- references against float64 torch
GEOMS = [(3, 1, 1, 5, 4, 6, 6), (3, 2, 1, 4, 6, 8, 6), (1, 2, 0, 4, 6, 8, 6), (3, 1, 1, 3, 16, 4, 32)]   # last: the stem's


@pytest.mark.parametrize("ks,stride,pad,cin,cout,h,w", GEOMS)
def test_int64_references_match_float64_conv2d(ks, stride, pad, cin, cout, h, w):
    g = torch.Generator().manual_seed(ks * 10 + stride)
    x = torch.randint(-9, 10, (2, h, w, cin), generator=g, dtype=torch.int64)
    b = torch.randint(-9, 10, (cout, ks, ks, cin), generator=g, dtype=torch.int64)
    xt = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    bt = b.permute(0, 3, 1, 2).double().requires_grad_(True)
    y = F.conv2d(xt, bt, stride=stride, padding=pad)
    ref = O.conv_i64(x, b, stride, pad)
    assert tuple(ref.shape) == (2, h // stride, w // stride, cout)
    assert torch.equal(y.detach().permute(0, 2, 3, 1), ref.double())
    dy = torch.randint(-9, 10, ref.shape, generator=g, dtype=torch.int64)
    y.backward(dy.permute(0, 3, 1, 2).double())
    assert torch.equal(xt.grad.permute(0, 2, 3, 1), O.dgrad_i64(dy, b, stride, pad, h, w).double())
    assert torch.equal(bt.grad.permute(0, 2, 3, 1), O.wgrad_i64(x, dy, ks, stride, pad).double())


def test_stride1_data_gradient_is_the_flipped_convolution():
    from tests.test_gpu_conv_sched import _dgrad_i64
    g = torch.Generator().manual_seed(5)
    dy = torch.randint(-9, 10, (2, 6, 5, 4), generator=g, dtype=torch.int64)
    b = torch.randint(-9, 10, (4, 3, 3, 4), generator=g, dtype=torch.int64)
    assert torch.equal(O.dgrad_i64(dy, b, 1, 1, 6, 5), _dgrad_i64(dy, b))


def test_transition_data_gradient_sums_both_filters():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64).round().requires_grad_(True)
    b3 = torch.randint(-9, 10, (6, 3, 3, 4), generator=g, dtype=torch.int64)
    b1 = torch.randint(-9, 10, (6, 1, 1, 4), generator=g, dtype=torch.int64)
    dy3 = torch.randint(-9, 10, (2, 4, 4, 6), generator=g, dtype=torch.int64)
    dy1 = torch.randint(-9, 10, (2, 4, 4, 6), generator=g, dtype=torch.int64)
    y3 = F.conv2d(x, b3.permute(0, 3, 1, 2).double(), stride=2, padding=1)
    y1 = F.conv2d(x, b1.permute(0, 3, 1, 2).double(), stride=2, padding=0)
    torch.autograd.backward([y3, y1], [dy3.permute(0, 3, 1, 2).double(), dy1.permute(0, 3, 1, 2).double()])
    assert torch.equal(x.grad.permute(0, 2, 3, 1), O.transition_dgrad_i64(dy3, b3, dy1, b1, 8, 8).double())


# ------------------------------------------------------------------------------------------------------------ bf16 terms
def test_bf16_terms_sum_back_exactly():
    g = torch.Generator().manual_seed(7)
    v = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-20, 20, (1 << 16,), generator=g).float())
    h, m, l = O.bf16_terms(v)
    assert torch.equal((h.double() + m.double()) + l.double(), v.double())
    for t in (h, m, l):                          # each term is a bf16 value
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    assert (m.abs() <= h.abs() * 2.0 ** -8).all() and (l.abs() <= m.abs() * 2.0 ** -8).all()


def test_generators_have_their_class():
    assert int(O.term_counts(O.gen_class1((4096,), -255, 255, 1)).max()) == 1
    c2 = O.term_counts(O.gen_class2((4096,), 2))
    assert int(c2.min()) == 2 and int(c2.max()) == 2
    v3 = O.gen_class3((4096,), 3)
    assert int(v3.abs().max()) < O.CLASS_MAG[3] and O.class_fractions(v3)[1] >= 0.25
    b = O.sparse_bins(32, 3, 16, 2, 3, "ci", 4)
    assert int((b != 0).sum(3).max()) == 2 and int(b.abs().max()) <= 3
    b = O.sparse_bins(32, 3, 16, 2, 3, "co", 4)
    assert int((b != 0).sum(0).max()) == 2


def _assert_class(t, cls):
    """a class-2 / class-3 tensor: at least a quarter of its non-zero elements carry a non-zero second / third term; no element
    needs more terms than the class allows"""
    n = O.term_counts(t)
    assert int(n.max()) <= cls
    if cls >= 2:
        f2, f3 = O.class_fractions(t)
        assert (f2 if cls == 2 else f3) >= 0.25


# ------------------------------------------------------------------------------- the conditions every GPU case relies on
@pytest.mark.parametrize("c", O.DENSE_BODY + O.DENSE_GEN + O.DENSE_STEM, ids=_ids(O.DENSE_BODY + O.DENSE_GEN + O.DENSE_STEM))
def test_dense_filter_gradient_cases_are_exact(c):
    x, dy = O.dense_operands(c)
    _assert_class(x, 1)
    _assert_class(dy, 1)
    assert int(x.min()) >= 0 and int(x.max()) == 255 and int(dy.abs().max()) == c.get("dy_amp", 15)
    O.assert_exact_budget(O.wgrad_i64, x, dy, ks=c["ks"], stride=c["stride"], pad=c["pad"])
    if c["kind"] == "body":                      # the one-launch backward's data-gradient role runs on the same dy
        b = O.gen_class1((c["cout"], 3, 3, c["cin"]), -255, 255, 9)
        O.assert_exact_budget(O.dgrad_i64, dy, b, stride=1, pad=1, h_in=c["h"], w_in=c["w"])
    n_tiles = c["B"] * c["ho"] * c["wo"] // c["pt"]
    assert n_tiles * c["pt"] == c["B"] * c["ho"] * c["wo"] and n_tiles > 1
    assert (c["ho"] * c["wo"]) % c["pt"] == 0 or c["pt"] % (c["ho"] * c["wo"]) == 0      # a tile never straddles two images


@pytest.mark.parametrize("c", O.DENSE_TRANSITION, ids=_ids(O.DENSE_TRANSITION))
def test_transition_cases_are_exact(c):
    x, dy3, dy1, b3, b1 = O.transition_operands(c)
    for t in (x, dy3, dy1, b3, b1):
        _assert_class(t, 1)
    O.assert_exact_budget(O.wgrad_i64, x, dy3, ks=3, stride=2, pad=1)
    O.assert_exact_budget(O.wgrad_i64, x, dy1, ks=1, stride=2, pad=0)
    O.assert_exact_budget(O.dgrad_i64, dy3, b3, stride=2, pad=1, h_in=c["h"], w_in=c["w"])
    O.assert_exact_budget(O.dgrad_i64, dy1, b1, stride=2, pad=0, h_in=c["h"], w_in=c["w"])
    O.assert_exact_budget(O.transition_dgrad_i64, dy3, b3, dy1, b1, h_in=c["h"], w_in=c["w"])


@pytest.mark.parametrize("c", O.PAIR_CASES, ids=_ids(O.PAIR_CASES))
def test_term_pair_cases_are_exact_and_placed(c):
    x, dy = O.pair_operands(c)
    _assert_class(x, c["x_cls"])
    _assert_class(dy, c["dy_cls"])
    assert c["dy_cls"] + c["x_cls"] <= 4          # every non-zero term pair is one of the six the kernel keeps
    O.assert_exact_budget(O.wgrad_i64, x, dy, ks=c["ks"], stride=c["stride"], pad=c["pad"])
    ho, wo, pt = c["ho"], c["wo"], c["pt"]
    in_group = set()
    for co in range(c["cout"]):
        px = torch.nonzero(dy.reshape(-1, c["cout"])[:, co]).flatten()
        assert 0 < len(px) <= O.SPARSE_K and px.tolist() == O.sparse_pixels(c, co)
        oh, ow = (px // wo) % ho, px % wo
        assert {0, ho - 1} <= set(oh.tolist()) and {0, wo - 1} <= set(ow.tolist())      # first and last row and column
        tiles = set((px // pt).tolist())
        assert {0, 1} <= tiles and len(tiles) >= 3                                      # both sides of a boundary; several ranges
        in_step = px[(px // 32) == (pt + 32) // 32]
        assert set(((in_step % 32) // 8).tolist()) == {0, 1, 2, 3}                      # all four lane groups of one k step
        in_group |= set((in_step % 8).tolist())
    assert in_group == set(range(8))                                                    # every position inside a lane group


@pytest.mark.parametrize("C,W,nbytes,a_bit", O.BINS_CASES)
def test_index_operand_cases_are_exact(C, W, nbytes, a_bit):
    idx, dy = O.bins_operands(C, W, nbytes, a_bit)
    assert int(idx.min()) >= 0 and int(dy.min()) >= 0 and int(dy.max()) == 15
    assert int(idx.max()) == min((1 << a_bit) - 1, 127 if nbytes == 1 else 65535)
    assert int(O.term_counts(idx).max()) <= 2     # an index is exact in the two terms the index form keeps
    O.assert_exact_budget(O.wgrad_i64, idx, dy, ks=3, stride=1, pad=1)


@pytest.mark.parametrize("c", O.ACT3_CASES, ids=_ids(O.ACT3_CASES))
def test_class3_activation_cases_are_exact(c):
    a, b = O.act3_operands(c)
    _assert_class(a, 3)
    _assert_class(b, 1)
    if c["op"] == "fwd":
        worst = O.assert_exact_budget(O.conv_i64, a, b, stride=c["stride"], pad=c["pad"])
    else:
        worst = O.assert_exact_budget(O.dgrad_i64, a, b, stride=c["stride"], pad=c["pad"], h_in=c["h"], w_in=c["w"])
    assert worst >= 1 << 19                      # the sums are not trivially small: several products meet in an output
    assert int((b != 0).sum()) >= c["cout"] * c["ks"] * c["ks"]      # every (co, tap) / (ci, tap) has live bins
