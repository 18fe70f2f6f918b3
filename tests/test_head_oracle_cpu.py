"""tests/head_oracle.py on the CPU: the float64 statement against torch.double autograd at every row, its out-of-range rule by hand,
that every row of the table selects the launch form its comment claims, the exactness precondition of the exact rows, and the
argument sets the head's entry points refuse before any launch (never-dereferenced pointers: no GPU on this path)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_oracle as H

IDS = [H.row_id(s) for s, _ in H.ALL_ROWS]


@pytest.mark.parametrize("i", range(len(H.ALL_ROWS)), ids=IDS)
def test_oracle_equals_torch_double_autograd(i):
    shape, _ = H.ALL_ROWS[i]
    B, HW, C, K = shape
    case = H.make_case(shape, i, exact=i >= len(H.ROWS))
    assert H.valid_rows(case["target"], K).all()
    feat = torch.from_numpy(case["feat"]).double().requires_grad_(True)
    lin = torch.nn.Linear(C, K).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(case["W"]))
        lin.bias.copy_(torch.from_numpy(case["bias"]))
    pooled = F.adaptive_avg_pool2d(feat.permute(0, 2, 1).reshape(B, C, HW, 1), 1).flatten(1)
    logits = lin(pooled)
    ce = F.cross_entropy(logits, torch.from_numpy(case["target"]))
    g = 0.37
    (ce * float(np.float32(g))).backward()
    fw = H.forward(case)
    tol = dict(rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(fw["pooled"], pooled.detach().numpy(), **tol)
    np.testing.assert_allclose(fw["logits"], logits.detach().numpy(), **tol)
    np.testing.assert_allclose(fw["probs"], torch.softmax(logits, 1).detach().numpy(), **tol)
    np.testing.assert_allclose(fw["loss"], F.cross_entropy(logits, torch.from_numpy(case["target"]), reduction="none").detach().numpy(),
                               **tol)
    np.testing.assert_allclose(fw["ce_mean"], float(ce.detach()), **tol)
    bw = H.backward(g, fw["probs"], fw["pooled"], case["W"], case["target"], HW)
    np.testing.assert_allclose(np.broadcast_to(bw["dfeat"][:, None, :], (B, HW, C)), feat.grad.numpy(), **tol)
    np.testing.assert_allclose(bw["dW"], lin.weight.grad.numpy(), **tol)
    np.testing.assert_allclose(bw["dbias"], lin.bias.grad.numpy(), **tol)
    for name in ("dfeat", "dW", "dbias"):
        assert bw["bar_" + name].shape == bw[name].shape and (bw["bar_" + name] > 0).all()


def test_out_of_range_rule_by_hand():
    """three rows, K = 2, targets (1, 2, -1): rows 1 and 2 have loss 0, still count in the divisor, and have no gradient"""
    logits = np.log(np.array([[1.0, 3.0], [1.0, 1.0], [2.0, 6.0]]))
    target = np.array([1, 2, -1], np.int64)
    loss, probs, ce = H.softmax_ref(logits, target)
    np.testing.assert_allclose(probs, [[0.25, 0.75], [0.5, 0.5], [0.25, 0.75]], rtol=1e-15)
    np.testing.assert_allclose(loss, [np.log(4.0 / 3.0), 0.0, 0.0], rtol=1e-15)
    assert loss[1] == 0.0 and loss[2] == 0.0
    np.testing.assert_allclose(ce, np.log(4.0 / 3.0) / 3.0, rtol=1e-15)
    dl = H.dl_ref(1.0, probs, target)
    np.testing.assert_allclose(dl[0], [0.25 / 3, -0.25 / 3], rtol=1e-15)
    assert not dl[1:].any()
    pooled = np.array([[1.0, 2.0], [10.0, 20.0], [100.0, 200.0]])
    W = np.array([[1.0, 0.0], [0.0, 1.0]])
    bw = H.backward(1.0, probs, pooled, W, target, HW=4)
    assert not bw["dfeat"][1:].any()
    np.testing.assert_allclose(bw["dW"], np.outer(dl[0], pooled[0]), rtol=1e-15)       # rows 1 and 2 add nothing
    np.testing.assert_allclose(bw["dbias"], dl[0], rtol=1e-15)
    for shape in ((80, 64, 64, 10), (1025, 1, 4, 3)):
        case = H.make_case(shape, 0, oor=True)
        K = shape[3]
        assert [int(case["target"][r]) for r in H.oor_rows(shape[0])] == [-1, K, -100]
        assert (~H.valid_rows(case["target"], K)).sum() == 3
        rows = H.partition(shape[0], shape[2])
        first = rows["sizes"][0]
        assert 3 < 8 * (first // 8) <= 16 < first                     # row 3 in an unrolled round, row 16 in the first part's tail


def test_rows_select_the_forms_their_comments_claim():
    P = H.partition
    shapes = [s for s, _ in H.ALL_ROWS]
    assert len(shapes) == len(set(shapes)) == 11
    assert all(1 <= C <= H.MAX_C and 1 <= K <= H.MAX_K for _, _, C, K in shapes)
    # CIFAR: everything divides
    pix, bat = P(64, 64), P(128, 64)
    assert pix["parts"] == 4 and not pix["idle"] and set(pix["loops"]) == {(2, 0)} and set(bat["loops"]) == {(4, 0)}
    assert set(P(80, 64)["loops"]) == {(2, 4)}                        # the short last batch: rounds and a tail
    one = P(1, 1)
    assert one["parts"] == 256 and one["sizes"] == [1] + [0] * 255
    odd = P(5, 3)
    assert odd["parts"] == 85 and odd["parts"] > 5 and odd["idle"] == [255] and odd["sizes"][:6] == [1] * 5 + [0]
    rag = P(49, 100)
    assert rag["parts"] == 2 and len(rag["idle"]) == 56 and rag["loops"] == [(3, 1), (3, 0)]
    assert P(7, 100)["loops"] == [(0, 4), (0, 3)]
    wide = P(200, 256)
    assert wide["parts"] == 1 and wide["loops"] == [(25, 0)] and P(5, 256)["loops"] == [(0, 5)]
    assert P(1, 256)["sizes"] == [1] and shapes[6] == (2, 1, 256, 64)
    tail = P(130, 8)
    assert tail["parts"] == 32 and tail["per"] == 5 and tail["loops"][:26] == [(0, 5)] * 26 and tail["sizes"][26:] == [0] * 6
    big = P(1025, 4)
    assert 1025 > H.STAGED_MAX_B and big["parts"] == 64 and big["per"] == 17 and big["loops"][0] == (2, 1) and big["sizes"][60:] == [5, 0, 0, 0]
    assert all(B <= H.STAGED_MAX_B for B, _, _, _ in shapes if B != 1025)
    assert set(P(64, 32)["loops"]) == {(1, 0)} and P(32, 256)["loops"] == [(4, 0)]          # the exact rows
    assert {K for _, _, _, K in shapes} >= {1, 64} and {C for _, _, C, _ in shapes} >= {1, 256}


@pytest.mark.parametrize("i", range(len(H.EXACT_ROWS)), ids=IDS[len(H.ROWS):])
def test_exact_rows_are_exact_in_fp32(i):
    shape, _ = H.EXACT_ROWS[i]
    case = H.make_case(shape, len(H.ROWS) + i, exact=True)
    assert np.abs(case["feat"]).max() <= 2 and np.abs(case["W"]).max() <= 1 and np.abs(case["bias"]).max() <= 1
    pool_units, chain_units = H.exactness_margin(case)
    assert 0 < pool_units < 2 ** 24 and 0 < chain_units < 2 ** 24, (pool_units, chain_units)
    fw = H.forward(case)
    # float64 holds them exactly too: rounding to fp32 changes nothing, in any summation order
    for name in ("pooled", "logits"):
        assert np.array_equal(fw[name].astype(np.float32).astype(np.float64), fw[name])
    rev = H.logits_ref(fw["pooled"][:, ::-1], case["W"][:, ::-1], case["bias"])[0]
    assert np.array_equal(rev, fw["logits"])
    with pytest.raises(AssertionError):
        H.exactness_margin(H.make_case(shape, 0, exact=False))


def test_bars_scale_with_the_operation_counts():
    assert H.gamma(1) == H.U / (1 - H.U) and H.gamma(1030) < 6.2e-5
    case = H.make_case((7, 49, 100, 31), 4)
    fw = H.forward(case)
    _, bar = H.pooled_ref(case["feat"])
    np.testing.assert_allclose(bar, H.gamma(50) * np.abs(case["feat"].astype(np.float64)).mean(axis=1) + H.TINY)
    # a float32 evaluation in another order stays inside every bar (the bars are no tighter than fp32 arithmetic allows)
    pooled32 = (case["feat"][:, ::-1].sum(axis=1, dtype=np.float32) / np.float32(49)).astype(np.float32)
    assert H.worst(pooled32, *H.pooled_ref(case["feat"])) <= 1.0
    logits32 = (pooled32 @ case["W"].T + case["bias"]).astype(np.float32)
    assert H.worst(logits32, *H.logits_ref(pooled32, case["W"], case["bias"])) <= 1.0
    t, bar_t = H.trans_ref(np.arange(8, dtype=np.float32), 2)
    assert t == 4.0 and bar_t < 3e-7


# ------------------------------------------------------------------------------------------------ refusals
def test_head_entry_points_refuse_before_any_launch():
    """head_kernels.hip:45-47, 56-57; site_kernels.hip:749-755, 777-781; site4_kernels.hip:2352.  Every call below carries a defect
    the entry point checks before it launches; the pointers are never dereferenced."""
    from alignq_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUP = _lib.EINVAL, _lib.EUNSUPPORTED
    p = ctypes.c_void_p(256)
    seen = []

    def expect(code, rc):
        seen.append(rc)
        assert rc == code, (len(seen), rc, code)

    def fwd(ptrs=None, B=8, HW=4, C=16, K=10, ce=None, counter=None, scal=None, n_sites=0, trans=None):
        feat, W, target, pooled, logits, probs, loss = ptrs or [p] * 7
        return lib.alignq_head_ce_fwd(feat, W, p, target, B, HW, C, K, pooled, logits, probs, loss, ce, counter, scal, n_sites, trans, None)

    def bwd(ptrs=None, B=8, HW=4, C=16, K=10):
        g, probs, target, pooled, W, dfeat, dW = ptrs or [p] * 7
        return lib.alignq_head_ce_bwd(g, probs, target, pooled, W, B, HW, C, K, dfeat, dW, p, None)

    for f in (fwd, bwd):
        for i in range(7):
            ptrs = [p] * 7
            ptrs[i] = None
            expect(EINVAL, f(ptrs=ptrs))
        expect(EINVAL, f(B=0)); expect(EINVAL, f(HW=0)); expect(EINVAL, f(B=-3))
        for C in (0, 257):
            expect(EUNSUP, f(C=C))
        for K in (0, 65):
            expect(EUNSUP, f(K=K))
    expect(EINVAL, fwd(ce=p))                                               # ce_mean without its counter
    expect(EINVAL, fwd(scal=p, n_sites=3, trans=p, counter=p))              # site_scal without ce_mean
    expect(EINVAL, fwd(scal=p, n_sites=3, ce=p, counter=p))                 # ... without trans_total
    expect(EINVAL, fwd(scal=p, n_sites=0, ce=p, counter=p, trans=p))        # ... with n_sites < 1

    # ---- the two roles: S sites described by host arrays of (never dereferenced) device pointers
    S = 2
    arr = (ctypes.c_void_p * S)(256, 256)
    hole = (ctypes.c_void_p * S)(256, None)
    Fs, F0 = (ctypes.c_int64 * S)(64, 64), (ctypes.c_int64 * S)(64, 0)

    def red(S=S, ws=arr, D=arr, A=arr, G=arr, scal=arr, F=Fs, B=128, dim=128, head=None, HB=8, HW=4, C=16, K=10, ce=p, hc=p,
            scal_all=p, n_sites=S, trans=p, sc=p):
        feat, W, target, pooled, logits, probs, loss = head or [p] * 7
        return lib.alignq_site_reduce_loss_multi_head(S, ws, D, A, G, scal, F, B, dim, 0.2, 0.3, feat, W, p, target, HB, HW, C, K,
                                                      pooled, logits, probs, loss, ce, hc, scal_all, n_sites, trans, sc, None)

    expect(EINVAL, red(S=0)); expect(EINVAL, red(dim=127))
    for name in ("ws", "D", "A", "G", "scal"):
        expect(EINVAL, red(**{name: None})); expect(EINVAL, red(**{name: hole}))
    expect(EINVAL, red(F=None)); expect(EINVAL, red(F=F0))
    expect(EUNSUP, red(B=64, dim=128)); expect(EUNSUP, red(B=129, dim=129))
    for i in range(7):
        head = [p] * 7
        head[i] = None
        expect(EINVAL, red(head=head))
    for kw in (dict(ce=None), dict(hc=None), dict(HB=0), dict(HW=0), dict(scal_all=None), dict(n_sites=S - 1), dict(trans=None),
               dict(sc=None)):
        expect(EINVAL, red(**kw))
    for kw in (dict(C=0), dict(C=257), dict(K=0), dict(K=65)):
        expect(EUNSUP, red(**kw))

    def prep(head=None, HB=8, HW=4, C=16, K=10, S=S, D=arr, A=arr, G=arr, scal=arr, F=Fs, B=128, dim=128, So=arr, dA=arr, dG=arr):
        g, probs, target, pooled, W, dfeat, dW = head or [p] * 7
        return lib.alignq_head_ce_bwd_site_prep(g, probs, target, pooled, W, HB, HW, C, K, dfeat, dW, p, S, D, A, G, scal, p, F, B, dim,
                                                0.2, So, dA, dG, None)

    for i in range(7):
        head = [p] * 7
        head[i] = None
        expect(EINVAL, prep(head=head))
    expect(EINVAL, prep(HB=0)); expect(EINVAL, prep(HW=0)); expect(EINVAL, prep(S=0)); expect(EINVAL, prep(dim=127))
    for name in ("D", "A", "G", "scal", "So", "dA", "dG"):
        expect(EINVAL, prep(**{name: None})); expect(EINVAL, prep(**{name: hole}))
    expect(EINVAL, prep(F=None)); expect(EINVAL, prep(F=F0))
    for kw in (dict(C=0), dict(C=257), dict(K=0), dict(K=65)):
        expect(EUNSUP, prep(**kw))
    assert len(seen) == 2 * 14 + 4 + 2 + 10 + 2 + 2 + 7 + 8 + 4 + 7 + 4 + 14 + 2 + 4
