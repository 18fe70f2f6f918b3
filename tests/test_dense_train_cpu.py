"""CPU-side checks of DenseNet's training without concatenations (include/alignq_dense_train.h): the eleventh header's table, the
refusals that return before anything is launched, and the `fuse_dense_train` flag."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alignq_dense_train_supported", "alignq_dense_train_site_ws_bytes", "alignq_dense_train_wgrad_ws_bytes",
         "alignq_dense_train_stats", "alignq_dense_train_layer_fwd", "alignq_dense_train_dgrad", "alignq_dense_train_wgrad",
         "alignq_dense_train_site_bwd")
OTHERS = ("SIGNATURES", "MOBILE_SIGNATURES", "POINTWISE_SIGNATURES", "K3CONV_SIGNATURES", "DENSE_SIGNATURES", "K5CONV_SIGNATURES",
          "DIGIT_SIGNATURES", "K3IMAGE_SIGNATURES", "BNQANY_SIGNATURES", "BNQPOOL_SIGNATURES")
P16 = 0x10000            # 16-byte aligned, not NULL: never dereferenced, every refusal returns before a launch


def test_the_header_is_the_new_table_and_shares_no_name():
    from alignq_amd import _header, _lib
    fns, structs, consts = _header.read(os.path.join(ROOT, "include", "alignq_dense_train.h"))
    assert tuple(fns) == NAMES and fns == _lib.DENSETRAIN_SIGNATURES and structs == {} and consts == {}
    for table in OTHERS:
        assert not set(NAMES) & set(getattr(_lib, table)), table
    lib = _lib.load()
    assert all(list(getattr(lib, n).argtypes) == fns[n][1] for n in NAMES)


def _call(name, **kw):
    """the entry point on valid-looking arguments over garbage pointers, `kw` replacing some"""
    from alignq_amd import _lib
    a = dict(z=P16, x=P16, y=P16, dy=P16, gy=P16, G=P16, ab=P16, save=P16, w=P16, dw=P16, ws=P16, ld=40, P=180, B=2, H=9, W=10, cin=24,
             cout=12, w_bit=4, k=4, r=2.0, formula=1)
    a.update(kw)
    lib = _lib.load()
    if name == "stats":
        return lib.alignq_dense_train_stats(a["z"], a["ld"], a["P"], a["cin"], None, None, None, None, None, 0.1, 1e-5, a["ab"],
                                            a["save"], a["ws"], None)
    if name == "layer_fwd":
        return lib.alignq_dense_train_layer_fwd(a["x"], a["ld"], a["y"], a["ld"], a["ab"], a["w"], a["B"], a["H"], a["W"], a["cin"],
                                                a["cout"], a["w_bit"], a["k"], a["r"], a["formula"], None)
    if name == "dgrad":
        return lib.alignq_dense_train_dgrad(a["dy"], a["ld"], a["w"], a["gy"], a["B"], a["H"], a["W"], a["cin"], a["cout"], a["w_bit"], None)
    if name == "wgrad":
        return lib.alignq_dense_train_wgrad(a["z"], a["ld"], a["ab"], a["dy"], a["ld"], a["dw"], a["ws"], a["B"], a["H"], a["W"], a["cin"],
                                            a["cout"], a["k"], a["r"], a["formula"], None, None)
    return lib.alignq_dense_train_site_bwd(a["gy"], a["z"], a["ld"], a["ab"], a["save"], a["G"], a["ld"], a["P"], a["cin"], a["k"], a["r"],
                                           a["formula"], None, None, a["ws"], None)


LIM = (1 << 31) - 1
REFUSALS = [  # (entry point, arguments, "EINVAL" / "EUNSUPPORTED")
    ("stats", dict(z=None), "EINVAL"), ("stats", dict(z=P16 + 4), "EINVAL"), ("stats", dict(ab=None), "EINVAL"),
    ("stats", dict(P=1), "EINVAL"), ("stats", dict(ld=20), "EINVAL"), ("stats", dict(ld=26), "EINVAL"),
    ("stats", dict(cin=516, ld=516), "EUNSUPPORTED"), ("stats", dict(cin=6, ld=8), "EUNSUPPORTED"),
    ("stats", dict(P=LIM // 40 + 1), "EUNSUPPORTED"), ("stats", dict(ws=None, cin=6), "EINVAL"),
    ("layer_fwd", dict(y=P16 + 8), "EINVAL"), ("layer_fwd", dict(ab=None), "EINVAL"), ("layer_fwd", dict(w_bit=9), "EINVAL"),
    ("layer_fwd", dict(k=0), "EINVAL"), ("layer_fwd", dict(k=32), "EINVAL"), ("layer_fwd", dict(formula=2), "EINVAL"),
    ("layer_fwd", dict(ld=20), "EINVAL"), ("layer_fwd", dict(cout=10), "EUNSUPPORTED"), ("layer_fwd", dict(B=0), "EUNSUPPORTED"),
    ("layer_fwd", dict(B=LIM // 40 + 1, H=1, W=1), "EUNSUPPORTED"), ("layer_fwd", dict(k=17, B=0), "EINVAL"),
    ("dgrad", dict(dy=None), "EINVAL"), ("dgrad", dict(ld=8), "EINVAL"), ("dgrad", dict(w_bit=0), "EINVAL"),
    ("dgrad", dict(cin=520), "EUNSUPPORTED"), ("dgrad", dict(gy=P16 + 4, H=0), "EINVAL"),
    ("wgrad", dict(dw=None), "EINVAL"), ("wgrad", dict(ws=P16 + 12), "EINVAL"), ("wgrad", dict(k=17), "EINVAL"),
    ("wgrad", dict(ld=22), "EINVAL"), ("wgrad", dict(W=-1), "EUNSUPPORTED"), ("wgrad", dict(formula=-1, cout=2), "EINVAL"),
    ("site_bwd", dict(G=None), "EINVAL"), ("site_bwd", dict(save=None), "EINVAL"), ("site_bwd", dict(P=0), "EINVAL"),
    ("site_bwd", dict(k=0), "EINVAL"), ("site_bwd", dict(ld=23), "EINVAL"), ("site_bwd", dict(cin=0, ld=0), "EUNSUPPORTED"),
    ("site_bwd", dict(P=LIM // 40 + 1), "EUNSUPPORTED"), ("site_bwd", dict(gy=P16 + 4, cin=2), "EINVAL"),
]


@pytest.mark.parametrize("name,kw,code", REFUSALS, ids=[f"{n}-{'-'.join(f'{k}={v}' for k, v in kw.items())}" for n, kw, _ in REFUSALS])
def test_refusals_before_any_launch(name, kw, code):
    from alignq_amd import _lib
    assert _call(name, **kw) == getattr(_lib, code)


def test_support_and_workspace_queries():
    from alignq_amd import _lib
    lib = _lib.load()
    assert lib.alignq_dense_train_supported(2, 9, 10, 24, 12, 36) == 1 and lib.alignq_dense_train_supported(2, 9, 10, 24, 12, 20) == 0
    assert lib.alignq_dense_train_supported(2, 9, 10, 26, 12, 40) == 0 and lib.alignq_dense_train_supported(LIM // 40 + 1, 1, 1, 24, 12, 40) == 0
    assert lib.alignq_dense_train_site_ws_bytes(180, 36) == lib.alignq_bnq_any_ws_bytes(180, 36) > 0
    assert lib.alignq_dense_train_wgrad_ws_bytes(2, 9, 10, 36, 12) == lib.alignq_k3conv_wgrad_ws_bytes(2, 9, 10, 36, 12) > 0
    assert lib.alignq_dense_train_site_ws_bytes(180, 516) == 0 and lib.alignq_dense_train_wgrad_ws_bytes(2, 9, 10, 36, 10) == 0


def test_the_flag_is_declared_on_densenet_only_and_set_by_dense_train():
    from alignq_amd import densenet as D
    from alignq_amd import paths
    assert paths.FLAGS.index("fuse_dense_train") == len(paths.FLAGS) - 2 and paths.FLAGS[-1] == "fuse_dense_eval"
    torch.manual_seed(0)
    net = D.DenseNet(4, 4, "second", depth=10, compressionRate=1)
    assert D.DenseNet.fuse_dense_train is False
    assert [m for m in net.modules() if hasattr(type(m), "fuse_dense_train")] == [net] and "fuse_dense_train" not in net.__dict__
    D.use_hip_convs(net, dense_eval=True, stem=True, train_sites=True)
    assert net.fuse_dense_train is False and "fuse_dense_train" not in net.__dict__
    net = D.DenseNet(4, 4, "second", depth=10, compressionRate=1)
    D.use_hip_convs(net, dense_train=True)
    assert net.fuse_dense_train is True and net.fuse_dense_eval is False
    assert all(m.fuse_train_sites is True for m in net.modules() if hasattr(type(m), "fuse_train_sites"))      # implied
