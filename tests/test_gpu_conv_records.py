"""What the Conv2d_Q autograd nodes of ops leave beside their outputs: every family's `apply_with_stats` hangs a named record on the
output (fused.ConvStats / fused.ConvStatsQ) whose partial sums are the output's per-channel sums, at the smallest shape each family
takes; and the lazy batch-norm records travel with the tensors (a LazyLink per output), not through global state: two chains whose
sites run in the other order give the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _wq(shape, k, dev, seed, grad):
    n = 2 ** k - 1
    w = torch.round(torch.tanh(torch.randn(shape, generator=torch.Generator().manual_seed(seed))) * n) / n
    return w.to(dev).contiguous(memory_format=CL).requires_grad_(grad)


def _x(shape, dev, seed, grad):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 1.1
    return x.to(dev).contiguous(memory_format=CL).requires_grad_(grad)


def _npy(t):
    return t.detach().double().cpu().numpy()


def _check_float_stats(y, C, lazy):
    """the record's type, the tensor's shape and dtype, lazy / link, and the partials against the output's own sums
    (the tolerances of test_conv_epilogue_bn_statistics_feed_the_fold)"""
    from alignq_amd import fused
    rec = y._alignq_bn_part
    assert isinstance(rec, fused.ConvStats) and rec.n_parts > 0
    assert tuple(rec.part.shape) == (C, rec.n_parts, 2) and rec.part.dtype == torch.float32
    assert rec.lazy == lazy and (isinstance(rec.link, fused.LazyLink) if lazy else rec.link is None)
    yd = y.detach().double()
    np.testing.assert_allclose(_npy(rec.part[:, :, 0].double().sum(1)), _npy(yd.sum((0, 2, 3))), rtol=1e-5, atol=1e-2)
    np.testing.assert_allclose(_npy(rec.part[:, :, 1].double().sum(1)), _npy((yd * yd).sum((0, 2, 3))), rtol=1e-5)


def _check_double_stats(y, C, groups):
    from alignq_amd import fused
    rec = y._alignq_bnq_part
    assert isinstance(rec, fused.ConvStatsQ) and rec.groups == groups and rec.n_parts > 0
    assert tuple(rec.part.shape) == (groups, rec.n_parts, C, 2) and rec.part.dtype == torch.float64
    assert fused.conv_partials(y, groups) == (rec.part, rec.n_parts) and fused.conv_partials(y, groups + 1) is None
    yd = y.detach().double().reshape(groups, y.shape[0] // groups, C, -1)
    tot = rec.part.sum(1)
    np.testing.assert_allclose(_npy(tot[..., 0]), _npy(yd.sum((1, 3))), rtol=1e-5, atol=1e-2)
    np.testing.assert_allclose(_npy(tot[..., 1]), _npy((yd * yd).sum((1, 3))), rtol=1e-5)


@pytest.mark.parametrize("x_grad,w_grad,lazy", [(True, True, 2), (False, True, 1), (False, False, 0)])
def test_body_3x3_leaves_a_conv_stats_record(dev, x_grad, w_grad, lazy):
    from alignq_amd import ops
    x, w = _x((2, 16, 8, 32), dev, 1, x_grad), _wq((16, 16, 3, 3), 8, dev, 2, w_grad)
    assert ops.qconv3x3_supported(x, w, (1, 1), (1, 1), (1, 1), 1, None, 8)
    y = ops.QConv3x3Fn.apply_with_stats(x, w, 8)
    _check_float_stats(y, 16, lazy)
    y2, alias = ops.QConv3x3Fn.apply_with_stats(x, w, 8, True)          # tap: the record rides on the first output
    assert torch.equal(y2, y) and alias.data_ptr() == x.data_ptr() and not hasattr(alias, "_alignq_bn_part")
    _check_float_stats(y2, 16, lazy)
    assert not hasattr(ops.QConv3x3Fn.apply(x, w, 8), "_alignq_bn_part")


def _smallest_transition_h(kernel_sizes):
    from alignq_amd import _lib as L
    lib = L.load()
    return next(h for h in range(2, 34, 2) if all(lib.alignq_conv_gen_bn_parts(2, h, 32, 16, 32, ks, 2) > 0 for ks in kernel_sizes))


@pytest.mark.parametrize("x_grad,w_grad,lazy", [(True, True, 2), (False, True, 1), (False, False, 0)])
def test_transition_conv_leaves_a_conv_stats_record(dev, x_grad, w_grad, lazy):
    from alignq_amd import ops
    H = _smallest_transition_h((3,))
    x, w = _x((2, 16, H, 32), dev, 3, x_grad), _wq((32, 16, 3, 3), 8, dev, 4, w_grad)
    assert ops.qconv_gen_supported(x, w, (2, 2), (1, 1), (1, 1), 1, None, 8)
    y = ops.QConvGenFn.apply_with_stats(x, w, 8, 1)
    _check_float_stats(y, 32, lazy)
    assert torch.equal(ops.QConvGenFn.apply(x, w, 8, 1), y)


def test_fused_transition_leaves_a_record_on_both_outputs(dev):
    """QTransitionFn only ever runs with gradients for x and both filters (ops.transition_supported): lazy 2, a link per output"""
    from alignq_amd import ops
    H = _smallest_transition_h((3, 1))
    x, w3, w1 = _x((2, 16, H, 32), dev, 5, True), _wq((32, 16, 3, 3), 8, dev, 6, True), _wq((32, 16, 1, 1), 8, dev, 7, True)
    y3, y1 = ops.QTransitionFn.apply_with_stats(x, w3, w1, 8)
    _check_float_stats(y3, 32, 2)
    _check_float_stats(y1, 32, 2)
    assert y3._alignq_bn_part.link is not y1._alignq_bn_part.link
    assert y3._alignq_bn_part.part.data_ptr() != y1._alignq_bn_part.part.data_ptr()


@pytest.mark.parametrize("w_grad,lazy", [(True, 2), (False, 0)])
def test_stem_leaves_a_conv_stats_record(dev, w_grad, lazy):
    """the stem's image never needs a gradient (ops.qconv_stem_supported): its filter gradient is the node's only one and reduces the
    site backward's per-tile sums itself (2)"""
    from alignq_amd import ops
    x, w = _x((2, 3, 4, 32), dev, 8, False), _wq((16, 3, 3, 3), 8, dev, 9, w_grad)
    assert ops.qconv_stem_supported(x, w, (1, 1), (1, 1), (1, 1), 1, None, 8)
    _check_float_stats(ops.QConvStemFn.apply_with_stats(x, w, 8), 16, lazy)


def test_gemm_and_stem7_leave_a_conv_stats_q_record(dev):
    from alignq_amd import ops
    x, w = _x((6, 64, 6, 6), dev, 10, True), _wq((64, 64, 3, 3), 8, dev, 11, True)
    assert ops.qconv_gemm_supported(x, w, (2, 2), (1, 1), (1, 1), 1, None, 8)
    for groups in (1, 2):
        y = ops.QConvGemmFn.apply_with_stats(x, w, 8, 2, 0.0, groups)
        _check_double_stats(y, 64, groups)
    assert torch.equal(ops.QConvGemmFn.apply(x, w, 8, 2), y) and not hasattr(ops.QConvGemmFn.apply(x, w, 8, 2), "_alignq_bnq_part")
    x, w = _x((2, 3, 8, 8), dev, 12, False), _wq((64, 3, 7, 7), 2, dev, 13, True)
    assert ops.qconv_stem7_supported(x, w, (2, 2), (3, 3), (1, 1), 1, None, 2)
    for groups in (1, 2):
        _check_double_stats(ops.QConvStem7Fn.apply_with_stats(x, w, 2, groups), 64, groups)


class _Flush(torch.autograd.Function):
    """stands in for the weight quantiser's backward: flushes the deferred filter-gradient reductions before it reads dW"""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        from alignq_amd.fused import active_wgrads
        if active_wgrads() is not None:
            active_wgrads().flush()
        return g


def _two_chains(dev, site_order):
    """conv A, conv B (in that order) -> a folded batch-norm + ADMM site each, the sites run in `site_order`; one backward inside
    DeferredWgrads(fresh_grads=True).  Returns dx, dw, dgamma, dbeta of A and of B."""
    import alignq_amd.cdf_alignment_admm as A
    from alignq_amd import ops
    from alignq_amd.fused import DeferredWgrads, bn_site
    B, C, H, k = 80, 16, 32, 8
    xs = [_x((B, C, H, H), dev, 20 + i, True) for i in range(2)]
    ws = [_wq((C, C, 3, 3), k, dev, 30 + i, True) for i in range(2)]
    gq = [_x((B, C, H, H), dev, 40 + i, False) * 0.01 for i in range(2)]
    bns, acts = [], []
    for i in range(2):
        torch.manual_seed(50 + i)
        bn = torch.nn.BatchNorm2d(C).to(dev).train()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.1)
        bns.append(bn)
        acts.append(A.activation_quantize_fn(k, "second", A.ADMM(128).to(dev)))
    zs = [ops.QConv3x3Fn.apply_with_stats(xs[i], _Flush.apply(ws[i]), k) for i in range(2)]
    assert all(z._alignq_bn_part.lazy == 2 for z in zs) and zs[0]._alignq_bn_part.link is not zs[1]._alignq_bn_part.link
    total = 0.0
    for i in site_order:
        xq, loss = bn_site(bns[i], acts[i], zs[i], relu=True)
        total = total + loss + (xq * gq[i]).sum()
    with DeferredWgrads(fresh_grads=True) as wg:
        total.backward()
        wg.flush()
    torch.cuda.synchronize()
    return [t.grad.clone() for i in range(2) for t in (xs[i], ws[i], bns[i].weight, bns[i].bias)]


def test_lazy_records_belong_to_their_tensors_not_to_global_state(dev):
    from alignq_amd import config, fused, ops
    saved = (config.args.bitW, config.args.abitW)
    config.args.bitW = config.args.abitW = 8
    try:
        # a record nobody consumes (its producer's backward never runs) is still reported when the context closes - a host-side
        # RuntimeError - and leaves nothing behind for the backward passes below
        y = ops.QConv3x3Fn.apply_with_stats(_x((80, 16, 32, 32), dev, 60, False), _wq((16, 16, 3, 3), 8, dev, 61, False), 8)
        z = y.detach().clone(memory_format=CL).requires_grad_(True)
        link = fused.LazyLink()
        z._alignq_bn_part = y._alignq_bn_part._replace(lazy=1, link=link)
        import alignq_amd.cdf_alignment_admm as A
        bn = torch.nn.BatchNorm2d(16).to(dev).train()
        xq, loss = fused.bn_site(bn, A.activation_quantize_fn(8, "second", A.ADMM(128).to(dev)), z, relu=True)
        with pytest.raises(RuntimeError, match="never consumed"):
            with fused.DeferredWgrads(fresh_grads=True):
                (loss + xq.sum()).backward()
        assert link.record is None and fused.active_wgrads() is None
        forward_order = _two_chains(dev, (0, 1))
        other_order = _two_chains(dev, (1, 0))
        for name, a, b in zip(("dxA", "dwA", "dgammaA", "dbetaA", "dxB", "dwB", "dgammaB", "dbetaB"), forward_order, other_order):
            assert torch.isfinite(a).all() and torch.equal(a, b), name
    finally:
        config.args.bitW, config.args.abitW = saved
