"""The weight quantiser hands a quantised filter to its convolution as ONE named record (fused.QuantizedFilter), parked with
weight_quantize_fn.park and read back with filter_of.  No GPU: a forward that is served from a parked record launches nothing, so a
Conv2d_Q runs on CPU tensors here; the bins and images are placeholders."""
import gc
import inspect
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F


def _conv():
    from alignq_amd import cdf_alignment_admm as admm
    torch.manual_seed(0)
    return admm.conv2d_Q_fn(4, "second")(4, 8, 3, padding=1, bias=False)


def _record(conv, **extras):
    from alignq_amd.fused import QuantizedFilter
    g = torch.Generator().manual_seed(1)
    q, cdf, pdf = (torch.randn(conv.weight.shape, generator=g) for _ in range(3))
    return QuantizedFilter(conv.weight, q, cdf, pdf, **extras)


def test_record_fields_and_defaults():
    from alignq_amd.fused import QuantizedFilter
    assert QuantizedFilter._fields == ("weight", "q", "cdf", "pdf", "bins", "image")
    w, q = object(), object()
    assert tuple(QuantizedFilter(w, q)) == (w, q, None, None, None, None)


def test_a_forward_consumes_the_parked_record():
    conv, x = _conv(), torch.randn(2, 4, 5, 5)
    rec = _record(conv)
    conv.quantize_fn.park(rec)
    assert conv.quantize_fn.parked is rec
    y = conv(x)
    assert torch.equal(y, F.conv2d(x, rec.q, padding=1))
    assert conv.quantize_fn.weight_cdf is rec.cdf and conv.quantize_fn.weight_pdf is rec.pdf
    assert conv.quantize_fn.weight_q.grad_fn is None and torch.equal(conv.quantize_fn.weight_q, rec.q)
    assert conv.quantize_fn.parked is None


def test_a_kept_record_serves_every_forward_until_unpark():
    conv, x = _conv(), torch.randn(2, 4, 5, 5)
    rec = _record(conv)
    conv.quantize_fn.park(rec, keep=True)
    want = F.conv2d(x, rec.q, padding=1)
    assert torch.equal(conv(x), want) and torch.equal(conv(x), want)
    assert conv.quantize_fn.parked is rec
    conv.quantize_fn.unpark()
    assert conv.quantize_fn.parked is None


def test_extras_go_to_the_very_tensor_the_forward_returned_not_to_its_address():
    conv = _conv()
    bins, image = (object(), object()), object()
    conv.quantize_fn.park(_record(conv, bins=bins, image=image))
    q = conv.quantize_fn(conv.weight)
    got = conv.quantize_fn.filter_of(q)
    assert got.q is q and got.bins is bins and got.image is image
    alias = q.detach()
    assert alias.data_ptr() == q.data_ptr() and alias is not q
    for other in (alias, torch.empty_like(q)):
        rec = conv.quantize_fn.filter_of(other)
        assert rec.q is other and rec.bins is None and rec.image is None


def _tensors(obj, seen):
    """every tensor reachable from obj through dicts, lists, tuples and records"""
    if id(obj) in seen:
        return
    seen.add(id(obj))
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors(v, seen)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _tensors(v, seen)


def test_the_quantiser_keeps_no_autograd_history():
    conv, x = _conv(), torch.randn(2, 4, 5, 5)
    q = conv.weight * 2
    assert q.grad_fn is not None
    alive = weakref.ref(q)
    from alignq_amd.fused import QuantizedFilter
    conv.quantize_fn.park(QuantizedFilter(conv.weight, q, bins=(object(), object()), image=object()))
    del q
    y = conv(x)
    assert y.grad_fn is not None and alive() is not None          # the output's graph holds q - nothing else may
    held = list(_tensors(vars(conv.quantize_fn), set()))
    assert held and all(t.grad_fn is None for t in held)
    del y
    gc.collect()
    assert alive() is None


def test_only_quantisers_that_declare_it_take_parked_filters():
    from alignq_amd import export
    from alignq_amd.quantization import make_uniform_admm_namespace
    from alignq_amd.resnet import resnet20_quant
    named = export.quantised_convs(resnet20_quant(8, 8))
    assert named and all(c.quantize_fn.parks_filters and name.endswith(".weight") for name, c in named)
    uniform = nn.Sequential(make_uniform_admm_namespace().conv2d_Q_fn(4, "second")(4, 8, 3, padding=1, bias=False))
    assert uniform[0].quantize_fn.w_bit == 4 and export.quantised_convs(uniform) == []
    assert len(export.quantised_convs(nn.Sequential(_conv()))) == 1


def test_the_positional_leftovers_are_gone():
    from alignq_amd import fused, ops
    assert list(inspect.signature(fused.WeightQuantAllFn.forward).parameters)[:4] == ["ctx", "k", "formula", "images"]
    for name, cls in inspect.getmembers(ops, inspect.isclass):
        forward = getattr(cls, "forward", None)
        if forward is not None:          # (no placeholder parameters: nothing a caller has to skip by position)
            assert not [p for p in inspect.signature(forward).parameters if p.startswith("_")], name


def test_every_family_refuses_cpu_tensors_before_it_reaches_for_the_library(monkeypatch):
    """ops.conv2d_q with every kernel-path flag on and CPU tensors: each family's smallest accepted case (the base cases of
    tests/golden/gen_goldens_conv_dispatch.py) gives torch's convolution bit for bit, from forward and from forward_with_shortcut, and
    no predicate has loaded the library: their cheap checks refuse first"""
    from alignq_amd import _lib, densenet
    from alignq_amd import cdf_alignment_admm as admm
    from tests.golden.gen_goldens_conv_dispatch import single_cases
    monkeypatch.setattr(_lib, "_lib", None)
    bases = [c for c in single_cases(Hg=16) if c["base"] is None and c["packed"] is None]
    assert {c["name"] for c in bases} >= {"body", "gen3", "gen1", "stem", "stem7", "gemm1", "gemm3s2", "dw", "pw", "k3", "body64"}
    cl = torch.channels_last
    for c in bases:
        cin, cout, ks, stride, pad, dil, groups, bias = c["conv"]
        make = densenet.conv2d_Q3_fn if c["kind"] == "Q3" else admm.conv2d_Q_fn
        conv = make(c["w_bit"], "second")(cin, cout, ks, stride, pad, dil, groups, bias).to(memory_format=cl)
        for flag in ("use_qconv", "use_qconv_pw", "use_qconv_k3", "emit_bn_stats"):
            if hasattr(type(conv), flag):
                setattr(conv, flag, True)
        x = torch.randn(c["x"], generator=torch.Generator().manual_seed(2)).contiguous(memory_format=cl).requires_grad_(c["x_grad"])
        rec = _record(conv)
        want = F.conv2d(x, rec.q, None, stride, pad, dil, groups)
        conv.quantize_fn.park(rec, keep=True)
        assert torch.equal(conv(x), want), c["name"]
        y, alias = conv.forward_with_shortcut(x)
        assert torch.equal(y, want) and alias is x, c["name"]
    assert _lib._lib is None
