"""The digit DANN's evaluation pass without a GPU: the seventh header and its table, the host side of
alignq_k5conv_site_pool_eval_fwd (every refusal returns before a launch), the `fuse_digit_eval` flag and EvalStep's construction."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("alignq.h", "alignq_mobile.h", "alignq_pointwise.h", "alignq_k3conv.h", "alignq_dense.h", "alignq_k5conv.h")


def test_the_seventh_header_yields_a_table_of_its_own():
    from alignq_amd import _header, _lib
    assert set(_lib.DIGIT_SIGNATURES) == {"alignq_k5conv_site_pool_eval_supported", "alignq_k5conv_site_pool_eval_fwd"}
    assert len(_lib.DIGIT_SIGNATURES["alignq_k5conv_site_pool_eval_fwd"][1]) == 16
    assert (_lib.DIGIT_OUT_NHWC, _lib.DIGIT_OUT_FLAT_CHW) == (0, 1) and not _lib._DIGIT_STRUCTS
    for h in OTHERS:
        fns, structs, consts = _header.read(os.path.join(ROOT, "include", h))
        assert not (set(_lib.DIGIT_SIGNATURES) | set(_lib._DIGIT_CONSTANTS)) & (set(fns) | set(structs) | set(consts)), h
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.DIGIT_SIGNATURES)


P16 = 0x10000          # 16-byte aligned, not NULL, never dereferenced


def _call(x=P16, xc=None, w=P16, bias=P16, y=P16, layout=0, B=2, H=12, W=12, cin=32, cout=48, w_bit=4, k=4, formula=1, clamp=1,
          mean=P16):
    from alignq_amd import _lib as L
    site = L.DenseSite(P16, P16, mean, P16, 1e-5, k, clamp)
    return L.load().alignq_k5conv_site_pool_eval_fwd(x, cin if xc is None else xc, w, bias, ctypes.byref(site), y, layout, B, H, W, cin,
                                                     cout, w_bit, 2.0, formula, None)


@pytest.mark.parametrize("bad", [dict(k=17), dict(k=0), dict(x=P16 + 4), dict(y=P16 + 8), dict(w=None), dict(bias=P16 + 2), dict(xc=2),
                                 dict(cin=3, xc=2), dict(xc=1), dict(layout=2), dict(clamp=0), dict(clamp=2), dict(formula=2),
                                 dict(w_bit=9), dict(mean=None)])
def test_a_bad_argument_is_einval_even_at_an_unsupported_shape(bad):
    from alignq_amd import _lib as L
    assert _call(**bad) == L.EINVAL
    assert _call(**dict(bad, H=5)) == L.EINVAL


@pytest.mark.parametrize("shape", [dict(H=5), dict(W=5), dict(B=0), dict(cout=6), dict(cin=6, xc=6), dict(cin=516, xc=516),
                                   dict(B=2 ** 20, H=64, W=64)])
def test_an_unsupported_shape_is_refused_before_any_launch(shape):
    from alignq_amd import _lib as L
    assert _call(**shape) == L.EUNSUPPORTED
    s = dict(B=2, H=12, W=12, cin=32, cout=48)
    s.update({k: v for k, v in shape.items() if k != "xc"})
    ok = L.load().alignq_k5conv_site_pool_eval_supported
    assert ok(s["B"], s["H"], s["W"], s["cin"], s["cout"]) == 0 and ok(64, 28, 28, 3, 32) == ok(1, 6, 6, 4, 4) == 1


def test_the_flag_is_declared_on_the_digit_model_only():
    from alignq_amd import densenet, digit, paths
    from tests.test_paths_cpu import MODELS, build
    assert "fuse_digit_eval" in paths.FLAGS
    net = digit.MNISTmodel_quant("org", 4, 4)
    assert [m for m in net.modules() if hasattr(type(m), "fuse_digit_eval")] == [net]
    assert net.fuse_digit_eval is False and "fuse_digit_eval" not in net.__dict__
    digit.use_hip_convs(net)
    assert net.fuse_digit_eval is False and "fuse_digit_eval" not in net.__dict__
    digit.use_hip_convs(net, eval_fused=True)
    assert net.fuse_digit_eval is True
    others = [build(name) for name, _ in MODELS] + [densenet.DenseNet(4, 4, "second", depth=10, compressionRate=1)]
    assert not any(hasattr(m, "fuse_digit_eval") for o in others for m in o.modules())


def test_eval_step_takes_the_digit_model():
    from alignq_amd import digit
    from alignq_amd.eval_step import EvalStep
    ev = EvalStep(digit.MNISTmodel_quant("org", 4, 4))
    assert ev._office is False and len(ev.all_convs) == 2
