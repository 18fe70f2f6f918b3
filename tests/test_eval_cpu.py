"""CPU-side checks of the evaluation pass: the new entry points are exported with the declared arity and refuse bad arguments
before any HIP call, the Python layer exists (this import fails on a tree without the feature) and only acts inside its scope,
and the NumPy restatements the GPU tests use say what the reference's test() computes (torch's eval-mode batch-norm,
F.cross_entropy and utils.accuracy's topk)."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

from tests import oracle_c as O
from tests.conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import eval_inputs as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def test_eval_step_module_exists():
    import alignq_amd.eval_step as E                  # ModuleNotFoundError before the evaluation pass existed
    from alignq_amd.train_step import _CapturedStep
    assert issubclass(E.EvalStep, _CapturedStep)
    for name in ("begin", "end", "capture", "result", "__enter__", "__exit__", "__call__"):
        assert callable(getattr(E.EvalStep, name)), name


def test_eval_symbols_exported_with_declared_arity():
    from alignq_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "alignq_bnq_eval_fwd") and hasattr(lib, "alignq_eval_metrics")
    assert len(_lib.SIGNATURES["alignq_bnq_eval_fwd"][1]) == 17
    assert len(_lib.SIGNATURES["alignq_eval_metrics"][1]) == 6
    assert lib.alignq_abi_version() == 23             # exports were added, the version was not bumped
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "alignq.h")).read(), flags=re.S)
    for name, n_args in (("alignq_bnq_eval_fwd", 17), ("alignq_eval_metrics", 6)):
        decl = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(decl.split(",")) == n_args, name


def test_eval_argument_checks_before_any_hip_call():
    """Host pointers that are never dereferenced: every call below returns from the argument checks (no GPU on this path)."""
    import ctypes
    from alignq_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15           # 16-byte aligned
    EINVAL, EUNSUP = _lib.EINVAL, _lib.EUNSUPPORTED

    def bnq(z=p, P=16, C=8, mean=p, var=p, k=8, r=2.0, formula=0, res=None, y=p, bins=None, pack=0):
        return lib.alignq_bnq_eval_fwd(z, P, C, None, None, mean, var, 1e-5, k, r, formula, 1, res, y, bins, pack, None)

    assert bnq(z=None) == EINVAL and bnq(mean=None) == EINVAL and bnq(var=None) == EINVAL and bnq(P=0) == EINVAL
    assert bnq(y=None) == EINVAL                       # neither y nor bins
    assert bnq(k=0) == EINVAL and bnq(k=17) == EINVAL and bnq(formula=2) == EINVAL
    assert bnq(z=p + 4) == EINVAL                      # alignment
    assert bnq(pack=3, bins=p) == EINVAL and bnq(pack=1) == EINVAL and bnq(bins=p) == EINVAL
    assert bnq(pack=2, bins=p, formula=1) == EINVAL    # packed form: ADMM / Office formula only
    assert bnq(pack=2, bins=p, res=p) == EINVAL        # ... without a residual
    assert bnq(pack=1, bins=p, k=8) == EINVAL          # 8 bits at act_range 2 need int16
    assert bnq(pack=2, bins=p, k=32) == EINVAL
    for C in (0, 2, 12, 48, 4096):                     # not a power of two in [4, 2048]
        assert bnq(C=C) == EUNSUP, C
    assert lib.alignq_eval_metrics(None, p, 4, 10, p, None) == EINVAL
    assert lib.alignq_eval_metrics(p, None, 4, 10, p, None) == EINVAL
    assert lib.alignq_eval_metrics(p, p, 4, 10, None, None) == EINVAL
    assert lib.alignq_eval_metrics(p, p, 0, 10, p, None) == EINVAL and lib.alignq_eval_metrics(p, p, 4, 0, p, None) == EINVAL
    assert lib.alignq_eval_metrics(p, p, 4, 10, p + 4, None) == EINVAL
    assert lib.alignq_eval_metrics(p, p, 4, 1025, p, None) == EUNSUP


def test_eval_scope_is_scoped_and_per_thread():
    from alignq_amd import fused
    assert not fused.eval_active()
    seen = []
    with fused.eval_scope():
        assert fused.eval_active()
        with fused.eval_scope():
            assert fused.eval_active()
        assert fused.eval_active()
        t = threading.Thread(target=lambda: seen.append(fused.eval_active()))
        t.start()
        t.join()
    assert not fused.eval_active() and seen == [False]


def test_bare_eval_forward_is_not_rerouted():
    """Outside an EvalStep the eval-mode helpers keep today's composition: bn_only on an eval-mode batch-norm is the module."""
    from alignq_amd import fused
    bn = torch.nn.BatchNorm2d(8).eval()
    with torch.no_grad():
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
        z = torch.randn(3, 8, 4, 4).contiguous(memory_format=torch.channels_last)
        assert torch.equal(fused.bn_only(bn, z), bn(z))
        with fused.eval_scope():                       # a CPU tensor is outside the kernel's domain: still the module
            assert fused.bn_only_eval(bn, z) is None
            assert torch.equal(fused.bn_only(bn, z), bn(z))


def test_stated_coefficient_arithmetic_is_the_eval_batch_norm():
    """a = gamma / sqrt(var + eps), b = beta - a * mean, x = a z + b in fp32 (include/alignq.h) against nn.BatchNorm2d.eval()
    evaluated in float64: a handful of fp32 roundings apart."""
    ab_numpy = E.ab_numpy
    rng = np.random.default_rng(0)
    C = 16
    gamma, beta = (0.5 + rng.random(C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    mean, var = rng.standard_normal(C).astype(np.float32), (0.3 + 2 * rng.random(C)).astype(np.float32)
    z = rng.standard_normal((4, 5, 5, C)).astype(np.float32)
    a, b = ab_numpy(gamma, beta, mean, var, 1e-5)
    x = ((a * z).astype(np.float32) + b).astype(np.float32)
    bn = torch.nn.BatchNorm2d(C).double().eval()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(mean)); bn.running_var.copy_(torch.from_numpy(var))
        bn.eps = float(np.float32(1e-5))
        ref = bn(torch.from_numpy(z).double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
    scale = np.abs(a * z).astype(np.float64) + np.abs(b) + np.abs(ref)
    assert np.all(np.abs(x - ref) <= 4 * np.finfo(np.float32).eps * scale)


def test_metrics_restatement_is_cross_entropy_and_topk_accuracy():
    """The NumPy restatement the GPU tests hold alignq_eval_metrics to, against F.cross_entropy and the topk accuracy of the
    reference's utils/common.py:78-92 (continuous random logits: no ties)."""
    metrics_numpy = E.metrics_numpy
    g = torch.Generator().manual_seed(0)
    for B, K in ((100, 10), (28, 31), (64, 1000)):
        logits = torch.randn(B, K, generator=g) * 3
        target = torch.randint(0, K, (B,), generator=g)
        logits[torch.arange(0, B, 4), target[::4]] += 20.0        # every fourth row certainly correct, the others by chance
        ce, n1, n5, n = metrics_numpy(logits.numpy(), target.numpy())
        ref_ce = float(torch.nn.functional.cross_entropy(logits.double(), target, reduction="sum"))
        _, pred = logits.topk(5, 1, True, True)                   # utils.accuracy
        correct = pred.t().eq(target.view(1, -1).expand_as(pred.t()))
        assert n == B and n1 == int(correct[:1].sum()) and n5 == int(correct[:5].sum())
        assert 0 < n1 < B
        np.testing.assert_allclose(ce, ref_ce, rtol=1e-12)


# ------------------------------------------------------------------------------------------------ against the reference
TIE, TOL = 1e-4, 1e-5            # tests/test_oracle_c.py: bins exact outside the erf tie zone, one off inside; values to 1e-5


def _torch_ref():
    from oracle import torch_ref as R
    return R


@pytest.mark.parametrize("tree", ["admm", "cdf", "office"])
def test_oracles_reproduce_reference_site_g17(tree):
    """Fixture G17 (the reference's relu(act_q(bn.eval()(z)) + residual), k in {2, 4, 8}) by oracle/torch_ref.py - the same ATen
    operations, so bit for bit (the bar of test_oracle_torch.test_g3_act_quant) - and by the C oracle at test_oracle_c's bars."""
    R = _torch_ref()
    g = load_golden("g17_eval_site_" + tree)
    r = float(g["act_range"])
    z, res, *_ = E.site_inputs(tree)
    bn = E.site_bn(tree)
    cfg = R.Config(tree=tree, act_range=r, method="plain")
    formula = O.FORMULA_CDF if tree == "cdf" else O.FORMULA_ADMM
    with torch.no_grad():
        x = bn(z)
        pre, _ = R.cdf_transform(x, torch.zeros(1), torch.ones(1), "a", cfg)
    pre = pre.numpy()
    for k in (2, 4, 8):
        n = 2 ** k - 1
        with torch.no_grad():
            xq, tl = R.act_quant(x, k, "second", cfg, None)
            y = torch.relu(xq + res)
        assert tl == 0
        assert np.array_equal(xq.numpy().view(np.uint32), g[f"xq_k{k}"].view(np.uint32))
        assert np.array_equal(y.numpy().view(np.uint32), g[f"y_k{k}"].view(np.uint32))
        assert int(g[f"n_flip_ref_k{k}"]) >= 0
        oq, t, _ = O.act_quant_fwd(x.numpy(), k, r, formula)
        np.testing.assert_allclose(t, pre, atol=3e-7, rtol=0)
        yb = pre * n
        tie = np.abs((yb - np.floor(yb)) - 0.5) < TIE
        d = np.abs(E.levels(oq, k, r, tree) - E.levels(g[f"xq_k{k}"], k, r, tree))
        assert np.all(d[~tie] == 0) and np.all(d[tie] <= 1)
        oy = np.maximum(oq + res.numpy(), 0.0)
        np.testing.assert_allclose(oy[d == 0], g[f"y_k{k}"][d == 0], atol=TOL, rtol=0)


@pytest.mark.parametrize("tree", ["admm", "cdf", "office"])
def test_metrics_restatement_equals_reference_network_g18(tree):
    """The NumPy restatement of alignq_eval_metrics on fixture G18's logits: the reference's CrossEntropyLoss and the Prec@1 /
    Prec@5 of its own utils.accuracy; the fixture's targets keep every row's target logit more than 1e-3 from its top-1 and top-5
    boundaries, so no count hangs on a bin flip."""
    g = load_golden("g18_eval_net_" + tree)
    B = int(g["batch"])
    _, _, y = E.net_inputs(tree, int(g["target_seed"]))
    y = y.numpy()
    assert g["logits"].shape[0] == B == len(y)
    assert E.margins(g["logits"], y).min() > float(g["margin"])
    ce, n1, n5, n = E.metrics_numpy(g["logits"], y)
    assert n == B
    np.testing.assert_allclose(ce / n, float(g["ce"]), rtol=2e-6)             # the reference's mean is formed in fp32
    assert abs(100.0 * n1 / n - float(g["prec1"])) < 1e-4 and abs(100.0 * n5 / n - float(g["prec5"])) < 1e-4
