"""DSAN on the CPU: an eager-torch restatement of the reference's LMMD (utils/mmd.py + utils/Weight.py of
cdf_alignment_admm/dsan_office) pinned to fixture G15, the argument checks and workspace sizes of alignq_lmmd_*, the drop-in
signature of alignq_amd.mmd.lmmd, the DSAN model's parameter names against G16, and DSANTrainStep's parameter groups."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from tests.conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def class_weights(s_label, p):
    """utils/Weight.py:10-54 in torch: (W_ss, W_tt, W_st) [B, B] fp32 and m.  Source columns: one-hot / count (fp64); target
    columns: p / column sum (fp32, as NumPy divides the fp32 probabilities); only classes present in the source labels AND the
    target argmax count; sums over classes in fp64.  A label outside [0, C) belongs to no class."""
    B, C = p.shape
    s_label = s_label.long().cpu()
    p = p.detach().cpu().float()
    valid = (s_label >= 0) & (s_label < C)
    onehot = torch.zeros(B, C, dtype=torch.float64)
    onehot[valid.nonzero().flatten(), s_label[valid]] = 1.0
    s_sum = onehot.sum(0)
    s_sum[s_sum == 0] = 100
    s_vec = onehot / s_sum
    t_sum = p.sum(0)
    t_sum[t_sum == 0] = 100
    t_vec = p / t_sum
    common = [c for c in range(C) if bool((s_label == c).any()) and bool((p.argmax(1) == c).any())]
    w_ss = torch.zeros(B, B, dtype=torch.float64)
    w_tt = torch.zeros(B, B, dtype=torch.float64)
    w_st = torch.zeros(B, B, dtype=torch.float64)
    for c in common:
        s, t = s_vec[:, c:c + 1], t_vec[:, c:c + 1]
        w_ss = w_ss + s @ s.T
        w_tt = w_tt + (t @ t.T).double()           # NumPy's dot of two fp32 columns is fp32
        w_st = w_st + s @ t.double().T
    m = len(common)
    if m:
        w_ss, w_tt, w_st = w_ss / m, w_tt / m, w_st / m
    return w_ss.float(), w_tt.float(), w_st.float(), m


def lmmd_restated(source, target, s_label, p, kernel_mul=2.0, kernel_num=5, fix_sigma=None, dtype=torch.float32):
    """utils/mmd.py:9-41 (the Gaussian kernels and the weighted sum) in eager torch, differentiable in source / target; the
    arithmetic in `dtype`.  Returns [1]."""
    B = source.shape[0]
    w_ss, w_tt, w_st, _ = class_weights(s_label, p)
    w_ss, w_tt, w_st = (w.to(dtype) for w in (w_ss, w_tt, w_st))
    total = torch.cat([source, target], 0).to(dtype)
    n = total.shape[0]
    L2 = ((total.unsqueeze(0) - total.unsqueeze(1)) ** 2).sum(2)
    bw = fix_sigma if fix_sigma else L2.detach().sum() / (n * n - n)
    bw = bw / kernel_mul ** (kernel_num // 2)
    K = sum(torch.exp(-L2 / (bw * kernel_mul ** k)) for k in range(kernel_num))
    loss = torch.zeros(1, dtype=dtype)
    if torch.isnan(K).any():
        return loss
    return loss + torch.sum(w_ss * K[:B, :B] + w_tt * K[B:, B:] - 2 * w_st * K[:B, B:])


def g15_case(g, ci):
    return dict(xs=g[f"xs_{ci}"], xt=g[f"xt_{ci}"], ys=g[f"ys_{ci}"], p=g[f"p_{ci}"], kernel_mul=float(g[f"kernel_mul_{ci}"]),
                kernel_num=int(g[f"kernel_num_{ci}"]), fix_sigma=float(g[f"fix_sigma_{ci}"]) or None)


def run_restated(case, dtype=torch.float32):
    s = torch.from_numpy(case["xs"]).to(dtype).requires_grad_(True)
    t = torch.from_numpy(case["xt"]).to(dtype).requires_grad_(True)
    loss = lmmd_restated(s, t, torch.from_numpy(case["ys"]), torch.from_numpy(case["p"]), case["kernel_mul"],
                         case["kernel_num"], case["fix_sigma"], dtype=dtype)
    if loss.requires_grad:
        loss.backward()
    ds = s.grad if s.grad is not None else torch.zeros_like(s)
    dt = t.grad if t.grad is not None else torch.zeros_like(t)
    return loss.detach().double().numpy(), ds.double().numpy(), dt.double().numpy()


G15_NAMES = ["b32", "b28", "d2048", "mul_num", "fix_sigma", "no_common", "identical", "one_class"]


@pytest.mark.parametrize("ci", range(len(G15_NAMES)), ids=G15_NAMES)
def test_restated_lmmd_equals_reference_fixture(ci):
    g = load_golden("g15_lmmd")
    assert list(g["names"]) == G15_NAMES
    case = g15_case(g, ci)
    loss, ds, dt = run_restated(case)
    ref = float(g[f"loss_{ci}"][0])
    if G15_NAMES[ci] in ("no_common", "identical"):
        assert ref == 0.0 and loss[0] == 0.0
        assert not ds.any() and not dt.any() and not g[f"ds_{ci}"].any() and not g[f"dt_{ci}"].any()
        return
    assert abs(loss[0] - ref) <= 1e-5 * abs(ref), (loss, ref)
    for got, key in ((ds, "ds"), (dt, "dt")):
        want = g[f"{key}_{ci}"]
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-5 * np.abs(want).max())


def test_lmmd_signature_matches_reference():
    from alignq_amd import mmd
    # utils/mmd.py:24: def lmmd(source, target, s_label, t_label, kernel_mul=2.0, kernel_num=5, fix_sigma=None)
    sig = inspect.signature(mmd.lmmd)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("source", inspect.Parameter.empty), ("target", inspect.Parameter.empty), ("s_label", inspect.Parameter.empty),
        ("t_label", inspect.Parameter.empty), ("kernel_mul", 2.0), ("kernel_num", 5), ("fix_sigma", None)]


def test_lmmd_rejects_unequal_batches_before_any_kernel():
    from alignq_amd import mmd
    with pytest.raises(ValueError, match="equal size"):
        mmd.lmmd(torch.zeros(4, 8), torch.zeros(5, 8), torch.zeros(4, dtype=torch.long), torch.zeros(5, 31))
    with pytest.raises(ValueError):
        mmd.lmmd(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, dtype=torch.long), torch.zeros(4, 31), fix_sigma=-1.0)


def test_lmmd_entry_points_validate_arguments_and_size_workspaces():
    from alignq_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUP = _lib.EINVAL, _lib.EUNSUPPORTED
    fake = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before a launch

    def fwd(B=32, D=256, C=31, mul=2.0, num=5, fix=0.0, ptrs=None):
        ptrs = ptrs or [fake] * 4 + [fake, fake]
        xs, xt, lab, p, loss, ws = ptrs
        return lib.alignq_lmmd_fwd(xs, xt, lab, p, B, D, C, mul, num, fix, loss, ws, None)

    for i in range(6):
        ptrs = [fake] * 6
        ptrs[i] = None
        assert fwd(ptrs=ptrs) == EINVAL, i
    assert fwd(B=0) == EINVAL and fwd(D=0) == EINVAL and fwd(C=0) == EINVAL and fwd(num=0) == EINVAL
    assert fwd(mul=0.0) == EINVAL and fwd(mul=float("inf")) == EINVAL and fwd(fix=float("nan")) == EINVAL
    assert fwd(B=65) == EUNSUP and fwd(B=1) == EUNSUP and fwd(C=65) == EUNSUP and fwd(num=9) == EUNSUP
    for i in range(6):
        ptrs = [fake] * 6
        ptrs[i] = None
        g, xs, xt, ws, dxs, dxt = ptrs
        assert lib.alignq_lmmd_bwd(g, xs, xt, ws, 32, 256, dxs, dxt, None) == EINVAL, i
    assert lib.alignq_lmmd_bwd(fake, fake, fake, fake, 65, 256, fake, fake, None) == EUNSUP
    assert lib.alignq_lmmd_bwd(fake, fake, fake, fake, 32, 0, fake, fake, None) == EINVAL
    # [slices][n][n] partial distances | [n][n] pair coefficients | flags (256 B); slices of 256 features, at most 16
    assert lib.alignq_lmmd_ws_bytes(32, 256) == 64 * 64 * 4 * 2 + 256
    assert lib.alignq_lmmd_ws_bytes(64, 2048) == 8 * 128 * 128 * 4 + 128 * 128 * 4 + 256
    assert lib.alignq_lmmd_ws_bytes(2, 1) == 256 + 256 + 256                     # 4 x 4 floats, each part 256-B aligned
    assert lib.alignq_lmmd_ws_bytes(64, 256 * 257) == 16 * 128 * 128 * 4 + 128 * 128 * 4 + 256
    assert lib.alignq_lmmd_ws_bytes(65, 256) == 0 and lib.alignq_lmmd_ws_bytes(1, 256) == 0
    assert lib.alignq_lmmd_ws_bytes(32, 0) == 0


def _tiny_dsan(stage):
    from alignq_amd.resnet_office import DSAN, Bottleneck, ResNet
    return DSAN(lambda w, a, s: ResNet(w, a, s, Bottleneck, [1, 1, 1, 1], width_per_group=8), 4, 4, stage)


def test_dsan_parameter_names_match_reference():
    from alignq_amd import config
    from alignq_amd.resnet_office import resnet50_dsan
    g = load_golden("g16_office_tiny_dsan")
    assert config.args.bottle_neck is True and config.args.param == 0.3
    net = _tiny_dsan(str(g["stage"]))
    assert [n for n, _ in net.named_parameters()] == list(g["names"])
    r50 = resnet50_dsan(4, 4, str(g["stage"]))
    assert [n for n, _ in r50.named_parameters()] == list(g["names_r50"])
    assert not hasattr(r50, "source") and not hasattr(r50, "target") and not hasattr(r50, "s_pred")


def test_dsan_lambd_ramp():
    from alignq_amd.train_step import dsan_lambd
    g = load_golden("g16_office_tiny_dsan")
    # the fixture's two values sit at p = 0.05 and 0.3 of the ramp: 0.05 = 5 / 10 / 10 (iteration 5 of 10 per epoch, 10 epochs)
    assert dsan_lambd(5, 10, 10) == g["lambd"][0] and dsan_lambd(30, 10, 10) == g["lambd"][1]
    assert abs(dsan_lambd(0, 10, 10)) < 1e-5
    assert int(g["m_0"]) >= 1 and int(g["m_1"]) >= 1        # both iterations' LMMD terms are live


def test_dsan_step_parameter_groups_and_epochs():
    """main.py:316-329: feature_layers at lr / 10, bottle and cls_fc at lr; new_epoch builds a fresh SGD with the decayed rate.
    OfficeTrainStep's groups for DANN are unchanged (feature, class head, domain head)."""
    from alignq_amd import config
    from alignq_amd.resnet_office import DANN, Bottleneck, ResNet
    from alignq_amd.train_step import DSANTrainStep, OfficeTrainStep
    config.args.bitW = config.args.abitW = 4
    config.args.train_batch_size = config.args.eval_batch_size = 6
    try:
        net = _tiny_dsan("aligned")
        step = DSANTrainStep(net, lr=0.004)
        groups = step.optimizer_t.param_groups
        assert [len(gr["params"]) for gr in groups] == [len(list(net.feature_layers.parameters())), 2, 2]
        assert [gr["lr"] for gr in groups] == [0.0004, 0.004, 0.004]
        assert groups[1]["params"][0] is net.bottle.weight and groups[2]["params"][0] is net.cls_fc.weight
        old = step.optimizer_t
        rate = step.new_epoch(2, 10, 0.004)
        assert step.optimizer_t is not old and rate == 0.004 / (1 + 10 * 1 / 10) ** 0.75
        assert [gr["lr"] for gr in step.optimizer_t.param_groups] == [rate / 10, rate, rate]
        named = list(net.named_parameters())
        want = [j for j, (n, _) in enumerate(named) if ("conv" in n or "downsample.0" in n) and "weight" in n][1:]
        assert step.idx == want and named[0][0] == "feature_layers.conv1.weight"
        assert len(step.blocks) == 4 and step.blocks[0] is net.feature_layers.layer1[0]
        dann = DANN(lambda w, a, s: ResNet(w, a, s, Bottleneck, [1, 1, 1, 1], width_per_group=8), 4, 4, "aligned")
        ostep = OfficeTrainStep(dann, lr=0.004)
        og = ostep.optimizer_t.param_groups
        assert [len(gr["params"]) for gr in og] == [len(list(dann.feature.parameters())), 2, 2]
        assert og[1]["params"][0] is dann.class_classifier.c_fc3.weight and og[2]["params"][0] is dann.domain_classifier.d_fc2.weight
        assert [gr["lr"] for gr in og] == [0.0004, 0.004, 0.004]
    finally:
        config.args.bitW = config.args.abitW = 8
        config.args.train_batch_size, config.args.eval_batch_size = 128, 100


if __name__ == "__main__":
    sys.exit(pytest.main([__file__, "-q"]))
