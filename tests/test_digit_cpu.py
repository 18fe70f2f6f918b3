"""The digit-domain DANN (alignq_amd/digit.py) without a GPU: names and shapes against the reference's (G23 (a)), the wiring at
32W/32A against the reference's double outputs (G23 (b)), the `use_qconv_k5` flag, and the host side of alignq_k5conv_*.  Fixture:
tests/golden/gen_goldens_digit.py (cdf_alignment/dann_digit/model/dann.py:125-230)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.golden.digit_init import digit_init_

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def g23():
    return np.load(os.path.join(HERE, "golden", "g23_digit.npz"))


def test_state_dict_names_and_shapes_are_the_references(g23):
    from alignq_amd import digit
    sd = digit.MNISTmodel_quant(str(g23["stage"]), 4, 4).state_dict()
    assert list(sd.keys()) == list(g23["keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(g23["shapes"])


def test_wiring_at_32_bits_is_within_the_references_own_error(g23):
    from alignq_amd import digit
    net = digit_init_(digit.MNISTmodel_quant(str(g23["stage"]), 32, 32)).eval()
    with torch.no_grad():
        c, d = net(torch.from_numpy(g23["x"]), float(g23["alpha"]))
    e_ref = float(g23["e_ref"])
    err = max(float(np.abs(c.numpy().astype(np.float64) - g23["class64"]).max()),
              float(np.abs(d.numpy().astype(np.float64) - g23["domain64"]).max()))
    print(f"wiring: max |out - out64| {err:.3e}, e_ref {e_ref:.3e}")
    assert err <= e_ref


def test_the_flag_is_declared_on_the_digit_models_class_only():
    from alignq_amd import cdf_alignment, cdf_alignment_admm, densenet, digit, paths
    from tests.test_paths_cpu import MODELS, build
    assert "use_qconv_k5" in paths.FLAGS
    net = digit.MNISTmodel_quant("org", 4, 4)
    k5 = [m for m in net.modules() if hasattr(type(m), "use_qconv_k5")]
    assert [type(m).__name__ for m in k5] == ["Conv2d_Q5"] * 2 and all(m.kernel_size == (5, 5) and m.bias is not None for m in k5)
    assert all(m.use_qconv_k5 is False and "use_qconv_k5" not in m.__dict__ for m in k5)
    digit.use_hip_convs(net)
    assert all(m.use_qconv_k5 is True and m.use_qconv is True for m in k5)
    # both CIFAR ResNets, DANN- and DSAN-Office, MobileNet-V2, DenseNet, and Conv2d_Q of both namespaces
    others = [build(name) for name, _ in MODELS] + [densenet.DenseNet(4, 4, "second", depth=10, compressionRate=1)]
    assert not any(hasattr(m, "use_qconv_k5") for net in others for m in net.modules())
    assert not any(hasattr(ns.conv2d_Q_fn(4, "org"), "use_qconv_k5") for ns in (cdf_alignment, cdf_alignment_admm))


def test_supported_set_and_error_order_on_the_host():
    """alignq_k5conv_supported per operation, and EINVAL named before EUNSUPPORTED, both before any launch (no GPU is touched)"""
    from alignq_amd import _lib as L
    lib = L.load()
    ok = lambda op, *shape: lib.alignq_k5conv_supported(op, *shape)          # noqa: E731
    ops = (L.K5_FWD, L.K5_DGRAD, L.K5_WGRAD)
    assert [ok(op, 64, 12, 12, 32, 48) for op in ops] == [1, 1, 1]
    assert [ok(op, 64, 28, 28, 3, 32) for op in ops] == [1, 0, 1]                                    # image form: no data gradient
    assert [ok(op, 1, 5, 5, 4, 512) for op in ops] == [1, 1, 1]
    for bad in ((1, 4, 5, 4, 4), (1, 5, 4, 4, 4), (0, 5, 5, 4, 4), (1, 5, 5, 6, 4), (1, 5, 5, 4, 6), (1, 5, 5, 516, 4), (1, 5, 5, 1, 4),
                (1, 5, 5, 3, 6), (2 ** 20, 64, 64, 4, 4)):
        assert [ok(op, *bad) for op in ops] == [0, 0, 0], bad
    assert ok(3, 1, 5, 5, 4, 4) == 0 and lib.alignq_k5conv_form(3, 1, 5, 5, 4, 4) == -1
    assert lib.alignq_k5conv_form(L.K5_DGRAD, 1, 28, 28, 3, 32) == -1
    assert lib.alignq_k5conv_wgrad_ws_bytes(1, 4, 5, 4, 4) == 0
    assert lib.alignq_k5conv_wgrad_ws_bytes(64, 12, 12, 32, 48) == 64 * 48 * 25 * 32 * 4            # 128 steps, 2 tiles: 64 slabs
    buf = (ctypes.c_char * 80)()
    p = (ctypes.addressof(buf) + 15) & ~15                                                           # 16-byte aligned, never read
    unsupported = (1, 4, 4, 6, 6)
    assert lib.alignq_k5conv_fwd(p, p, None, p, *unsupported, 4, None) == L.EUNSUPPORTED
    assert lib.alignq_k5conv_fwd(p, p, None, p, *unsupported, 9, None) == L.EINVAL                   # w_bit before the shape
    assert lib.alignq_k5conv_fwd(p + 4, p, None, p, *unsupported, 4, None) == L.EINVAL               # alignment before the shape
    assert lib.alignq_k5conv_fwd(p, p, p + 2, p, *unsupported, 4, None) == L.EINVAL                  # bias: 4-byte aligned
    assert lib.alignq_k5conv_fwd(None, p, None, p, 1, 5, 5, 4, 4, 4, None) == L.EINVAL
    assert lib.alignq_k5conv_dgrad(p, p, p, 1, 28, 28, 3, 32, 4, None) == L.EUNSUPPORTED
    assert lib.alignq_k5conv_dgrad(p, None, p, 1, 28, 28, 3, 32, 4, None) == L.EINVAL
    assert lib.alignq_k5conv_wgrad(p, p, p, p, *unsupported, None, None) == L.EUNSUPPORTED
    assert lib.alignq_k5conv_wgrad(p, p, None, p, *unsupported, None, None) == L.EINVAL              # neither dw nor n_slabs_out
