"""CPU-side checks of the DenseNet model (alignq_amd/densenet.py): its state_dict layout against the reference's (fixture G21 (a)) at
depth 40 and at the reduced depth, a reference-named checkpoint loading strictly, the fixture's own conditions, and the new kernel-path
flag: paths.apply touches exactly the 3x3 convolution modules and paths.restore puts every instance __dict__ back.  No GPU: only
constructors run."""
import numpy as np
import pytest
import torch

from tests import oracle_c as O
from tests.conftest import load_golden
from tests.golden.densenet_init import REDUCED, TF_LAYERS, densenet_init_


@pytest.fixture(scope="module")
def g21():
    return load_golden("g21_densenet")


def _layout(net):
    sd = net.state_dict()
    return list(sd.keys()), [",".join(map(str, v.shape)) for v in sd.values()]


def test_state_dict_layout_equals_the_reference(g21):
    from alignq_amd import densenet as D
    keys, shapes = _layout(D.densenet_40_quant(4, 4, "no_align"))
    assert len(keys) == 236
    assert keys == [str(k) for k in g21["keys_full"]] and shapes == [str(s) for s in g21["shapes_full"]]
    keys, shapes = _layout(D.DenseNet(4, 4, "no_align", **REDUCED))
    assert keys == [str(k) for k in g21["keys_reduced"]] and shapes == [str(s) for s in g21["shapes_reduced"]]


def test_a_reference_named_state_dict_loads_strictly(g21):
    from alignq_amd import densenet as D
    g = torch.Generator().manual_seed(3)
    sd = {}
    for k, s in zip(g21["keys_full"], g21["shapes_full"]):
        shape = tuple(int(v) for v in str(s).split(",") if v)
        sd[str(k)] = torch.zeros(shape, dtype=torch.long) if str(k).endswith("num_batches_tracked") else torch.randn(shape, generator=g)
    net = D.densenet_40_quant(4, 4, "no_align")
    missing, unexpected = net.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    assert torch.equal(net.dense3[11].conv1.weight.detach(), sd["dense3.11.conv1.weight"])
    assert torch.equal(net.trans2.bn1.running_var, sd["trans2.bn1.running_var"])


def test_geometry_is_the_issue_s():
    """depth 40, compressionRate 1: 3x3 dense layers 24, 36, ..., 444 -> 12; transitions 168 -> 168 and 312 -> 312 (1x1); 456 features"""
    from alignq_amd import densenet as D
    net = D.densenet_40_quant(4, 4, "no_align")
    k3 = [m for m in net.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3)]
    assert [(m.in_channels, m.out_channels) for m in k3] == [(3, 24)] + [(c, 12) for s in (24, 168, 312) for c in range(s, s + 144, 12)]
    assert max(m.in_channels for m in k3) == 444 and all(m.padding == (1, 1) and m.stride == (1, 1) and m.bias is None for m in k3)
    assert [(t.conv1.in_channels, t.conv1.out_channels, t.conv1.kernel_size) for t in (net.trans1, net.trans2)] == \
        [(168, 168, (1, 1)), (312, 312, (1, 1))]
    assert net.fc.in_features == 456 and net.bn.num_features == 456
    small = D.DenseNet(4, 4, "no_align", **REDUCED)
    assert [m.in_channels for m in small.modules() if isinstance(m, torch.nn.Conv2d)] == [3, 24, 36, 48, 48, 60, 72, 72, 84]
    # compressionRate 2 halves at every transition; a depth that is not 3 n + 4 is refused
    assert D.DenseNet(4, 4, "no_align", depth=10).fc.in_features == 48          # 24 -> 48 -> 24 -> 48 -> 24 -> 48
    with pytest.raises(ValueError):
        D.DenseNet(4, 4, "no_align", depth=11)
    # dropout is applied where dropRate > 0
    torch.manual_seed(0)
    blk = D.DenseBasicBlock("no_align", 32, 32, 8, 8, None, dropRate=0.5).train()
    x = torch.randn(2, 8, 4, 4)
    out = blk(x)
    assert tuple(out.shape) == (2, 20, 4, 4) and torch.equal(out[:, :8], x) and int((out[:, 8:] == 0).sum()) > 20


def test_weight_initialisation_is_the_reference_s():
    """convolutions N(0, 2 / (k k C_out)), batch-norm gains 1 and biases 0"""
    from alignq_amd import densenet as D
    torch.manual_seed(1)
    net = D.densenet_40_quant(4, 4, "no_align")
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            assert bool((m.weight == 1).all()) and bool((m.bias == 0).all())
    w = torch.cat([m.conv1.weight.detach().reshape(-1) for m in net.dense3])
    assert abs(float(w.std()) / (2.0 / (9 * 12)) ** 0.5 - 1.0) < 0.02 and abs(float(w.mean())) < 1e-3
    t = net.trans1.conv1.weight.detach()
    assert abs(float(t.std()) / (2.0 / 168) ** 0.5 - 1.0) < 0.03


@pytest.mark.parametrize("i", range(4))
def test_fixture_filters_quantise_bit_equal_through_the_c_oracle(g21, i):
    w = g21[f"k{i}_w"]
    q = O.weight_quant_fwd(w, O.weight_stats(w), 4, O.FORMULA_CDF)[0]
    assert np.array_equal(q.view(np.uint32), g21[f"k{i}_wq"].view(np.uint32))
    assert float(g21["boundary_dist"][i]) >= float(g21["margin"]) == 1e-3
    stage, j = TF_LAYERS[i]
    assert w.shape == (12, {("dense1", 0): 24, ("dense2", 0): 48, ("dense2", 1): 60, ("dense3", 1): 84}[(stage, j)], 3, 3)
    assert g21[f"k{i}_x"].shape[0] == 1 and g21[f"k{i}_x"].shape[1] == w.shape[1]          # the first sample only


def test_fixture_layers_agree_with_an_fp64_convolution(g21):
    F = torch.nn.functional
    for i in range(4):
        x, wq, dy = (torch.from_numpy(g21[f"k{i}_{n}"]).double() for n in ("x", "wq", "dy"))
        x.requires_grad_(True)
        wq.requires_grad_(True)
        y = F.conv2d(x, wq, None, 1, 1)
        y.backward(dy)
        for name, got, want in (("y", g21[f"k{i}_y"], y), ("dx", g21[f"k{i}_dx"], x.grad), ("dwq", g21[f"k{i}_dwq"], wq.grad)):
            err = float((torch.from_numpy(got).double() - want.detach()).abs().max())
            assert err <= 1e-5 * max(1.0, float(want.detach().abs().max())), (i, name, err)
    assert 0.0 < float(g21["c_e_ref"]) < 1e-5


def own(model):
    """Every module's instance __dict__: its keys and the identity of each value."""
    return {n: {k: id(v) for k, v in m.__dict__.items()} for n, m in model.named_modules()}


@pytest.mark.parametrize("depth", [10, 40])
def test_apply_touches_exactly_the_3x3_convolutions_and_restore_puts_every_dict_back(depth):
    from alignq_amd import densenet as D
    from alignq_amd import paths
    torch.manual_seed(0)
    net = densenet_init_(D.DenseNet(4, 4, "no_align", depth=depth, compressionRate=1))
    k3 = [m for m in net.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3)]
    n = (depth - 4) // 3
    assert len(k3) == 3 * n + 1 and k3[0] is net.conv1
    assert k3[1:] == [blk.conv1 for stage in (net.dense1, net.dense2, net.dense3) for blk in stage]
    before = own(net)
    assert not any("use_qconv_k3" in m.__dict__ for m in net.modules())
    value = object()
    rec = paths.apply(net, use_qconv_k3=value)
    assert len(rec) == len(k3) and [r[0] for r in rec] == k3
    for m in net.modules():
        if any(m is c for c in k3):
            assert m.__dict__["use_qconv_k3"] is value
        else:
            assert not hasattr(m, "use_qconv_k3")
    # the class declares the flag next to Conv2d_Q's three, which the transitions' class declares alone
    assert all(type(m).__name__ == "Conv2d_Q3" and m.use_qconv is False and m.use_qconv_pw is False for m in k3)
    assert type(net.trans1.conv1).__name__ == "Conv2d_Q" and not hasattr(net.trans1.conv1, "use_qconv_k3")
    paths.restore(rec)
    assert own(net) == before and all(m.use_qconv_k3 is False for m in k3)
    # use_hip_convs: three flags on the convolutions; restore of a by-hand record brings the instance dicts back
    rec = paths.apply(net, use_qconv=True, use_qconv_pw=True, use_qconv_k3=True)
    assert len(rec) == 3 * len(k3) + 2 * 2
    paths.restore(rec)
    assert own(net) == before
    D.use_hip_convs(net)
    assert all(m.use_qconv and m.use_qconv_pw and m.use_qconv_k3 for m in k3)
    assert net.trans2.conv1.use_qconv is True and net.trans2.conv1.use_qconv_pw is True
    assert all(p.is_contiguous(memory_format=torch.channels_last) for p in net.parameters() if p.dim() == 4)
    with pytest.raises(TypeError, match="no such flag"):
        paths.apply(net, use_qconv_k33=True)
