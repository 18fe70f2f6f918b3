"""The 3x3 image-form convolution (include/alignq_k3image.h, csrc/k3image_kernels.hip) without a GPU: the eighth header and its
table, the host side of the entry points (every refusal returns before a launch), the slab rule and the `use_qconv_k3_image` flag."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("alignq.h", "alignq_mobile.h", "alignq_pointwise.h", "alignq_k3conv.h", "alignq_dense.h", "alignq_k5conv.h", "alignq_digit.h")
P16 = 0x10000          # 16-byte aligned, not NULL, never dereferenced
LIM = (1 << 31) - 1


def test_the_eighth_header_yields_a_table_of_its_own():
    from alignq_amd import _header, _lib
    assert set(_lib.K3IMAGE_SIGNATURES) == {"alignq_k3image_supported", "alignq_k3image_form", "alignq_k3image_fwd",
                                            "alignq_k3image_wgrad_ws_bytes", "alignq_k3image_wgrad"}
    assert (_lib.K3I_FWD, _lib.K3I_WGRAD) == (0, 1)
    for h in OTHERS:
        fns, structs, consts = _header.read(os.path.join(ROOT, "include", h))
        assert not (set(_lib.K3IMAGE_SIGNATURES) | set(_lib._K3IMAGE_CONSTANTS)) & (set(fns) | set(structs) | set(consts)), h
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.K3IMAGE_SIGNATURES)


def _fwd(x=P16, w=P16, y=P16, B=2, H=5, W=5, cout=24, ldy=None, k=4):
    from alignq_amd import _lib as L
    return L.load().alignq_k3image_fwd(x, w, y, B, H, W, cout, cout if ldy is None else ldy, k, None)


def _wgrad(x=P16, dy=P16, dw=P16, ws=P16, B=2, H=5, W=5, cout=24, ns=None):
    from alignq_amd import _lib as L
    return L.load().alignq_k3image_wgrad(x, dy, dw, ws, B, H, W, cout, ns, None)


def test_refusals_before_any_launch():
    from alignq_amd import _lib as L
    lib, EINVAL, EUNSUP = L.load(), L.EINVAL, L.EUNSUPPORTED
    for n in ("x", "w", "y"):
        assert _fwd(**{n: None}) == EINVAL and _fwd(**{n: P16 + 4}) == EINVAL and _fwd(**{n: P16 + 8}) == EINVAL, n
    assert _fwd(k=0) == EINVAL and _fwd(k=9) == EINVAL
    for n in ("x", "dy", "ws"):
        assert _wgrad(**{n: None}) == EINVAL and _wgrad(**{n: P16 + 8}) == EINVAL, n
    ns = ctypes.c_int(0)
    assert _wgrad(dw=None) == EINVAL and _wgrad(dw=P16 + 4, ns=ctypes.byref(ns)) == EINVAL
    for C in (0, 2, 6, 516):
        assert _fwd(cout=C) == EUNSUP and _wgrad(cout=C) == EUNSUP and _wgrad(dw=None, ns=ctypes.byref(ns), cout=C) == EUNSUP, C
        assert lib.alignq_k3image_supported(0, 2, 5, 5, C) == lib.alignq_k3image_supported(1, 2, 5, 5, C) == 0
        assert lib.alignq_k3image_form(0, 2, 5, 5, C) == -1 and lib.alignq_k3image_wgrad_ws_bytes(2, 5, 5, C) == 0
    assert _fwd(ldy=20) == EUNSUP and _fwd(ldy=26) == EUNSUP                            # ldy < COUT; ldy % 4 != 0
    for dim in ("B", "H", "W"):
        assert _fwd(**{dim: 0}) == EUNSUP and _wgrad(**{dim: 0}) == EUNSUP, dim
        assert lib.alignq_k3image_supported(0, *[0 if d == dim else 3 for d in ("B", "H", "W")], 24) == 0
    # B * H * W * ldy <= 2^31 - 1, also where B * H * W alone overflows 32 or 64 bits
    assert lib.alignq_k3image_supported(0, LIM // 512, 1, 1, 512) == 1 and lib.alignq_k3image_supported(0, LIM // 512 + 1, 1, 1, 512) == 0
    assert _fwd(B=LIM // 512 + 1, H=1, W=1, cout=512) == EUNSUP and _wgrad(B=1, H=LIM // 512 + 1, W=1, cout=512) == EUNSUP
    assert _fwd(B=LIM // 512, H=1, W=1, cout=4, ldy=516) == EUNSUP                      # the pitch counts, not COUT
    assert _fwd(B=LIM, H=LIM, W=LIM) == EUNSUP and _fwd(B=1 << 16, H=1 << 16, W=1) == EUNSUP
    # a bad argument is named before an unsupported shape
    assert _fwd(k=0, cout=6) == EINVAL and _fwd(x=None, B=0) == EINVAL and _fwd(y=P16 + 4, ldy=20) == EINVAL
    assert _wgrad(x=None, cout=6) == EINVAL and _wgrad(ws=P16 + 8, H=0) == EINVAL and ns.value == 0
    # an unknown op; the forms
    assert lib.alignq_k3image_supported(2, 2, 5, 5, 24) == 0 and lib.alignq_k3image_form(2, 2, 5, 5, 24) == -1
    assert [lib.alignq_k3image_form(0, 2, 5, 5, c) for c in (4, 24, 32, 64, 68)] == [0, 1, 1, 2, 0]
    assert lib.alignq_k3image_form(1, 2, 5, 5, 24) == 3


@pytest.mark.parametrize("B,H,W,cout", [(1, 4, 8, 4), (3, 9, 11, 24), (128, 32, 32, 68)])
def test_workspace_follows_the_slab_rule(B, H, W, cout):
    from alignq_amd import _lib as L
    T, C = B * -(-H // 4) * -(-W // 8), -(-cout // 64)
    s = max(1, min(-(-512 // C), -(-T // 2), 1024))
    per = -(-T // s)
    assert L.load().alignq_k3image_wgrad_ws_bytes(B, H, W, cout) == -(-T // per) * cout * 27 * 4


def test_the_flag_is_declared_on_densenets_class_only():
    from alignq_amd import densenet as D
    from alignq_amd import mobilenet as M
    from alignq_amd import paths
    assert "use_qconv_k3_image" in paths.FLAGS and paths.FLAGS[-1] == "fuse_dense_eval"
    assert paths.FLAGS.index("use_qconv_k3_image") < paths.FLAGS.index("fuse_digit_eval")
    torch.manual_seed(0)
    net = D.DenseNet(4, 4, "second", depth=10, compressionRate=1)
    convs = [m for m in net.modules() if hasattr(type(m), "use_qconv_k3_image")]
    assert len(convs) == 7 and all(type(m).__name__ == "Conv2d_Q3" for m in convs)
    assert all(m.use_qconv_k3_image is False and "use_qconv_k3_image" not in m.__dict__ for m in convs)
    D.use_hip_convs(net)
    assert all(m.use_qconv_k3_image is False and "use_qconv_k3_image" not in m.__dict__ for m in convs)
    D.use_hip_convs(net, stem=True)
    assert all(m.use_qconv_k3_image is True and m.use_qconv_k3 is True for m in convs)
    assert not any(hasattr(m, "use_qconv_k3_image") for m in M.mobile_v2(4, 4, "second").modules())
