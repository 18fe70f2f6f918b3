"""CPU-side checks of the depthwise convolution and the MobileNet-V2 model: the NumPy oracle against F.conv2d, fixture G19 against
the oracle, the new exports' host-side answers, and the model's state_dict layout against the reference's (fixture G19 (a))."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dwconv_oracle as D
from tests import oracle_c as O
from tests.conftest import load_golden


@pytest.fixture(scope="module")
def g19():
    return load_golden("g19_mobilenet")


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", [(2, 8, 5, 7), (2, 8, 6, 8), (3, 4, 1, 1), (1, 12, 2, 3)])
def test_oracle_agrees_with_conv2d(shape, stride):
    """Pins the oracle's geometry (H_out, the tap positions, the stride-2 zeros of the data gradient).  Both sides are fp32
    evaluations of the same sums, so the bound doubles."""
    B, C, H, W = shape
    rng = np.random.default_rng(7 + stride)
    x = rng.standard_normal(shape).astype(np.float32)
    w = rng.standard_normal((C, 1, 3, 3)).astype(np.float32)
    xt, wt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(w).requires_grad_(True)
    y = F.conv2d(xt, wt, None, stride, 1, 1, C)
    assert tuple(y.shape) == (B, C, D.out_size(H, stride), D.out_size(W, stride))
    dy = rng.standard_normal(tuple(y.shape)).astype(np.float32)
    y.backward(torch.from_numpy(dy))
    assert (np.abs(D.fwd32(x, w, stride) - y.detach().numpy()) <= 2 * D.fwd_bound(x, w, stride)).all()
    assert (np.abs(D.fwd32(x, w, stride) - D.fwd64(x, w, stride)) <= D.fwd_bound(x, w, stride)).all()
    dx = D.dgrad32(dy, w, stride, H, W)
    assert (np.abs(dx - xt.grad.numpy()) <= 2 * D.dgrad_bound(dy, w, stride, H, W)).all()
    assert (np.abs(dx - D.dgrad64(dy, w, stride, H, W)) <= D.dgrad_bound(dy, w, stride, H, W)).all()
    if stride == 2:                # input positions that no output reads: exactly +0 on both sides
        never = D.dgrad_mag(np.ones_like(dy), np.ones_like(w), stride, H, W) == 0
        assert (xt.grad.numpy()[never] == 0).all() and bool((dx[never] == 0).all()) and not np.signbit(dx[never]).any()
    dw = D.wgrad64(x, dy, stride).reshape(C, 1, 3, 3)
    assert (np.abs(dw - wt.grad.numpy()) <= D.wgrad_bound(x, dy, stride).reshape(C, 1, 3, 3)).all()


@pytest.mark.parametrize("i", range(4))
def test_fixture_layers_agree_with_oracle(g19, i):
    x, wq, dy, s = g19[f"dw{i}_x"], g19[f"dw{i}_wq"], g19[f"dw{i}_dy"], int(g19[f"dw{i}_stride"])
    H, W = x.shape[2:]
    assert (np.abs(g19[f"dw{i}_y"] - D.fwd64(x, wq, s)) <= D.fwd_bound(x, wq, s)).all()
    assert (np.abs(g19[f"dw{i}_dx"] - D.dgrad64(dy, wq, s, H, W)) <= D.dgrad_bound(dy, wq, s, H, W)).all()
    assert (np.abs(g19[f"dw{i}_dwq"].reshape(-1, 3, 3) - D.wgrad64(x, dy, s)) <= D.wgrad_bound(x, dy, s)).all()


@pytest.mark.parametrize("i", range(4))
def test_fixture_filters_quantise_bit_equal_through_the_c_oracle(g19, i):
    w = g19[f"dw{i}_w"]
    q = O.weight_quant_fwd(w, O.weight_stats(w), 4, O.FORMULA_CDF)[0]
    assert D.bits_equal(q, g19[f"dw{i}_wq"])
    assert float(g19["boundary_dist"][i]) >= float(g19["margin"]) == 1e-3


def test_exports_and_host_side_answers():
    from alignq_amd import _lib
    lib = _lib.load()
    for name in ("alignq_dwconv3x3_supported", "alignq_dwconv3x3_nhwc_fwd", "alignq_dwconv3x3_nhwc_dgrad",
                 "alignq_dwconv3x3_wgrad_ws_bytes", "alignq_dwconv3x3_nhwc_wgrad"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.alignq_abi_version() == 23
    sup = lib.alignq_dwconv3x3_supported
    assert sup(4, 1, 1, 4, 1) == 1 and sup(100, 32, 32, 144, 2) == 1
    assert sup(4, 8, 8, 6, 1) == 0 and sup(4, 8, 8, 2, 1) == 0 and sup(4, 8, 8, 8, 3) == 0 and sup(4, 0, 8, 8, 1) == 0
    assert sup(1 << 10, 1 << 10, 1 << 10, 4, 1) == 0          # 2^32 elements: beyond the int32 offsets the header states
    # null pointers: refused before anything touches a device
    assert lib.alignq_dwconv3x3_nhwc_fwd(None, None, None, 4, 8, 8, 8, 1, None) == _lib.EINVAL
    assert lib.alignq_dwconv3x3_nhwc_dgrad(None, None, None, 4, 8, 8, 8, 1, None) == _lib.EINVAL
    assert lib.alignq_dwconv3x3_nhwc_wgrad(None, None, None, None, 4, 8, 8, 8, 1, None) == _lib.EINVAL
    for shape in ((4, 1, 1, 4, 1), (100, 32, 32, 144, 2), (100, 32, 32, 32, 1), (100, 4, 4, 960, 1), (3, 5, 7, 20, 2)):
        n = lib.alignq_dwconv3x3_wgrad_ws_bytes(*shape)
        assert n > 0 and n % 256 == 0 and n >= shape[3] * 9 * 4, (shape, n)
    assert lib.alignq_dwconv3x3_wgrad_ws_bytes(4, 8, 8, 6, 1) == 0


def test_state_dict_layout_equals_the_reference(g19, monkeypatch):
    from alignq_amd import mobilenet as M
    net = M.mobile_v2(4, 4, "no_align")
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g19["keys_full"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g19["shapes_full"]]
    assert [tuple(r) for r in g19["cfg_full"]] == list(M.MobileNetV2.cfg)
    monkeypatch.setattr(M.MobileNetV2, "cfg", [tuple(int(v) for v in r) for r in g19["cfg_reduced"]])
    sd = M.mobile_v2(4, 4, "no_align").state_dict()
    assert list(sd.keys()) == [str(k) for k in g19["keys_reduced"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g19["shapes_reduced"]]


def test_stride1_block_with_equal_planes_keeps_its_shortcut_convolution():
    from alignq_amd import mobilenet as M
    blk = M.Block("no_align", 4, 4, 24, 24, 6, 1)
    assert blk.shortcut is not None and isinstance(blk.shortcut[0], torch.nn.Conv2d) and blk.shortcut[0].weight.shape == (24, 24, 1, 1)
    assert blk.shortcut[2] is blk.act_skip and isinstance(blk.shortcut[3], torch.nn.ReLU)
    assert blk.conv2.groups == 144 and blk.conv2.weight.shape == (144, 1, 3, 3) and isinstance(blk.relu, torch.nn.ReLU6)
    assert M.Block("no_align", 4, 4, 24, 32, 6, 2).shortcut is None
    net = M.mobile_v2(4, 4, "no_align", num_classes=10)
    assert isinstance(net.avg_pool2d, torch.nn.AvgPool2d) and net.linear.in_features == 1280
    assert net.layers[2].shortcut is not None          # (6, 24, 2, 1): second block, 24 -> 24
