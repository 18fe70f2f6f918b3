"""The pooled batch-norm fold (include/alignq_bnq_pool.h, csrc/bnq_pool_kernels.hip) without a GPU: the tenth header and its table, the
refusals of the entry points before any launch, and the `fuse_train_sites` flag on the digit DANN."""
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("alignq.h", "alignq_mobile.h", "alignq_pointwise.h", "alignq_k3conv.h", "alignq_dense.h", "alignq_k5conv.h", "alignq_digit.h",
          "alignq_k3image.h", "alignq_bnq_any.h")
P16 = 0x10000          # 16-byte aligned, not NULL, never dereferenced


def test_the_tenth_header_yields_a_table_of_its_own():
    from alignq_amd import _header, _lib
    assert set(_lib.BNQPOOL_SIGNATURES) == {"alignq_bnq_pool_supported", "alignq_bnq_pool_ws_bytes", "alignq_bnq_pool_code_bytes",
                                            "alignq_bnq_pool_fwd", "alignq_bnq_pool_bwd"}
    assert len(_lib.BNQPOOL_SIGNATURES["alignq_bnq_pool_fwd"][1]) == 21 and len(_lib.BNQPOOL_SIGNATURES["alignq_bnq_pool_bwd"][1]) == 15
    for h in OTHERS:
        fns, structs, consts = _header.read(os.path.join(ROOT, "include", h))
        assert not (set(_lib.BNQPOOL_SIGNATURES) | set(_lib._BNQPOOL_CONSTANTS)) & (set(fns) | set(structs) | set(consts)), h
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.BNQPOOL_SIGNATURES)


def test_refusals_before_any_launch():
    from alignq_amd import _lib as L
    lib = L.load()

    def fwd(z=P16, B=2, H=4, W=6, C=24, k=4, formula=0, ab=P16, save=P16, y=P16, code=P16, ws=P16):
        return lib.alignq_bnq_pool_fwd(z, B, H, W, C, None, None, None, None, None, 0.1, 1e-5, k, 2.0, formula, ab, save, y, code, ws, None)

    def bwd(g=P16, z=P16, code=P16, B=2, H=4, W=6, C=24, dz=P16, ws=P16):
        return lib.alignq_bnq_pool_bwd(g, z, code, P16, P16, B, H, W, C, 2.0, dz, None, None, ws, None)

    for n in ("z", "y", "code", "ws"):
        assert fwd(**{n: None}) == L.EINVAL and fwd(**{n: P16 + 8}) == L.EINVAL, n
    for n in ("g", "z", "code", "dz", "ws"):
        assert bwd(**{n: None}) == L.EINVAL and bwd(**{n: P16 + 4}) == L.EINVAL, n
    assert fwd(ab=None) == fwd(save=None) == fwd(k=0) == fwd(k=17) == fwd(formula=2) == fwd(B=0) == bwd(B=0) == bwd(H=0) == L.EINVAL
    for bad in (dict(H=5), dict(W=7), dict(C=1028), dict(C=2), dict(C=0), dict(C=6), dict(B=(1 << 40) // 24 + 1)):
        assert fwd(**bad) == bwd(**bad) == L.EUNSUPPORTED, bad
        shape = {**dict(B=2, H=4, W=6, C=24), **bad}
        assert [fn(shape["B"], shape["H"], shape["W"], shape["C"]) for fn in
                (lib.alignq_bnq_pool_supported, lib.alignq_bnq_pool_ws_bytes, lib.alignq_bnq_pool_code_bytes)] == [0, 0, 0], bad
    assert fwd(H=5, k=0) == L.EINVAL                     # a bad argument is named before an unsupported shape
    assert [lib.alignq_bnq_pool_supported(*s) for s in ((1, 2, 2, 4), (1, 2, 2, 1024), (1 << 36, 4, 4, 4), ((1 << 36) + 1, 4, 4, 4))] == [1, 1, 1, 0]
    assert lib.alignq_bnq_pool_code_bytes(64, 24, 24, 32) == 64 * 12 * 12 * 32


def test_the_flag_is_the_digit_models_alone():
    from alignq_amd import densenet as D
    from alignq_amd import digit, paths
    from alignq_amd import mobilenet as M
    torch.manual_seed(0)
    net = digit.MNISTmodel_quant("second", 4, 4)
    assert [type(m) for m in net.modules() if hasattr(type(m), "fuse_train_sites")] == [digit.MNISTmodel_quant]
    assert net.fuse_train_sites is False and "fuse_train_sites" not in net.__dict__
    assert digit.use_hip_convs(net).fuse_train_sites is False and digit.use_hip_convs(net, eval_fused=True).fuse_train_sites is False
    assert digit.use_hip_convs(net, train_sites=True).fuse_train_sites is True
    assert [m for m in net.modules() if "fuse_train_sites" in m.__dict__] == [net]
    # the other models: DenseNet's declaring classes as before, MobileNet-V2 without the flag
    dense = D.DenseNet(4, 4, "second", depth=10, compressionRate=1)
    assert {type(m) for m in dense.modules() if hasattr(type(m), "fuse_train_sites")} == {D.DenseBasicBlock, D.Transition, D.DenseNet}
    assert len(paths.apply(dense, fuse_train_sites=True)) == 9
    assert not any(hasattr(m, "fuse_train_sites") for m in M.mobile_v2(4, 4, "second").modules())

