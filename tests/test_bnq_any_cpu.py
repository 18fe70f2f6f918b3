"""The any-width batch-norm fold (include/alignq_bnq_any.h, csrc/bnq_any_kernels.hip) without a GPU: the ninth header and its table, the
host side of the entry points, the `fuse_train_sites` flag and fused.bn_act_any's refusals."""
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = ("alignq.h", "alignq_mobile.h", "alignq_pointwise.h", "alignq_k3conv.h", "alignq_dense.h", "alignq_k5conv.h", "alignq_digit.h",
          "alignq_k3image.h")
P16 = 0x10000          # 16-byte aligned, not NULL, never dereferenced


def test_the_ninth_header_yields_a_table_of_its_own():
    from alignq_amd import _header, _lib
    assert set(_lib.BNQANY_SIGNATURES) == {"alignq_bnq_any_supported", "alignq_bnq_any_ws_bytes", "alignq_bnq_any_mask_bytes",
                                           "alignq_bnq_any_fwd", "alignq_bnq_any_bwd"}
    assert len(_lib.BNQANY_SIGNATURES["alignq_bnq_any_fwd"][1]) == 20 and len(_lib.BNQANY_SIGNATURES["alignq_bnq_any_bwd"][1]) == 14
    for h in OTHERS:
        fns, structs, consts = _header.read(os.path.join(ROOT, "include", h))
        assert not (set(_lib.BNQANY_SIGNATURES) | set(_lib._BNQANY_CONSTANTS)) & (set(fns) | set(structs) | set(consts)), h
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in _lib.BNQANY_SIGNATURES)


def test_refusals_before_any_launch():
    from alignq_amd import _lib as L
    lib = L.load()

    def fwd(z=P16, P=64, C=24, k=4, formula=0, clamp=1, ab=P16, save=P16, y=P16, mask=P16, ws=P16):
        return lib.alignq_bnq_any_fwd(z, P, C, None, None, None, None, None, 0.1, 1e-5, k, 2.0, formula, clamp, ab, save, y, mask, ws, None)

    def bwd(g=P16, z=P16, mask=P16, P=64, C=24, clamp=1, dz=P16, ws=P16):
        return lib.alignq_bnq_any_bwd(g, z, mask, P16, P16, P, C, 2.0, clamp, dz, None, None, ws, None)

    for n in ("z", "y", "ws"):
        assert fwd(**{n: None}) == L.EINVAL and fwd(**{n: P16 + 8}) == L.EINVAL, n
    for n in ("g", "z", "dz", "ws"):
        assert bwd(**{n: None}) == L.EINVAL and bwd(**{n: P16 + 4}) == L.EINVAL, n
    assert fwd(ab=None) == fwd(save=None) == fwd(k=0) == fwd(k=17) == fwd(formula=2) == fwd(clamp=3) == fwd(P=1) == L.EINVAL
    assert fwd(mask=None) == fwd(clamp=0) == bwd(mask=None) == bwd(clamp=0) == bwd(clamp=-1) == bwd(P=1) == L.EINVAL
    for C in (0, 2, 6, 2052):
        assert fwd(C=C) == bwd(C=C) == L.EUNSUPPORTED and lib.alignq_bnq_any_supported(64, C) == 0, C
    assert fwd(C=6, k=0) == L.EINVAL                     # a bad argument is named before an unsupported shape
    assert [lib.alignq_bnq_any_supported(P, C) for P, C in ((2, 4), (1, 4), (64, 2048), (1 << 40, 4), ((1 << 40) + 1, 4))] == [1, 0, 1, 1, 0]


def test_the_flag_touches_exactly_the_declaring_classes():
    from alignq_amd import densenet as D
    from alignq_amd import mobilenet as M
    from alignq_amd import paths
    assert "fuse_train_sites" in paths.FLAGS
    torch.manual_seed(0)
    net = D.DenseNet(4, 4, "second", depth=10, compressionRate=1)
    declaring = [m for m in net.modules() if hasattr(type(m), "fuse_train_sites")]
    assert {type(m) for m in declaring} == {D.DenseBasicBlock, D.Transition, D.DenseNet} and len(declaring) == 6 + 2 + 1
    assert all(m.fuse_train_sites is False and "fuse_train_sites" not in m.__dict__ for m in declaring)
    rec = paths.apply(net, fuse_train_sites=True)
    assert len(rec) == 9 and all(m.fuse_train_sites is True for m in declaring)
    assert not any("fuse_train_sites" in m.__dict__ for m in net.modules() if m not in declaring)
    paths.restore(rec)
    assert not any("fuse_train_sites" in m.__dict__ for m in net.modules())
    D.use_hip_convs(net)
    assert not any(m.fuse_train_sites for m in declaring)
    D.use_hip_convs(net, train_sites=True)
    assert all(m.fuse_train_sites is True for m in declaring)
    assert not any(hasattr(m, "fuse_train_sites") for m in M.mobile_v2(4, 4, "second").modules())


def test_bn_act_any_refuses_what_it_cannot_fold():
    import alignq_amd.cdf_alignment as A
    from alignq_amd import fused
    bn, act = torch.nn.BatchNorm2d(24), A.activation_quantize_fn(a_bit=4, stage="second")
    z = torch.randn(2, 24, 4, 4).contiguous(memory_format=torch.channels_last)
    assert fused.bn_act_any(bn, act, z, fused.CLAMP_RELU) is None                        # a CPU tensor
    assert fused.bn_act_any(bn.eval(), act, z, fused.CLAMP_RELU) is None                 # evaluation
    assert fused.bn_act_any(bn.train(), A.activation_quantize_fn(a_bit=32, stage="second"), z, fused.CLAMP_RELU) is None
    assert fused.bn_act_any(torch.nn.BatchNorm2d(24, track_running_stats=False), act, z, fused.CLAMP_RELU) is None
    assert fused.bn_act_any(torch.nn.BatchNorm2d(24, momentum=None), act, z, fused.CLAMP_RELU) is None
