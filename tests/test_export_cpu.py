"""Packed k-bit weight checkpoints without a GPU: the NumPy statement of the format (tests/packed_oracle.py) against itself and
against the reference's own quantised weights (fixture G2, both trees), the host-side queries and argument checks of the C ABI,
and the PackedModel container (save / load / sizes / apply) built by hand from oracle codes."""
import os

import numpy as np
import pytest
import torch

from tests import packed_oracle as PO
from tests.conftest import load_golden


# ------------------------------------------------------------------------------------------------------------ the format
@pytest.mark.parametrize("bits", range(1, 18))
def test_oracle_round_trip_and_zero_padding(bits):
    rng = np.random.default_rng(100 + bits)
    for n in (1, 31, 32, 33, 1000):
        c = rng.integers(0, 2 ** bits, size=n, dtype=np.uint64).astype(np.uint32)
        c[rng.integers(0, n)] = 2 ** bits - 1                     # every bit of a code set somewhere
        words = PO.pack(c, bits)
        assert words.dtype == np.uint32 and words.size == PO.packed_words(n, bits) == (n + 31) // 32 * bits
        assert np.array_equal(PO.unpack(words, n, bits), c)
        assert np.array_equal(PO.unpack_fast(words, n, bits), c)
        # the padding: the last group's bits past its last element are zero
        groups = (n + 31) // 32
        big = 0
        for w in range(bits):
            big |= int(words[(groups - 1) * bits + w]) << (32 * w)
        used = (n - 32 * (groups - 1)) * bits
        assert big >> used == 0
        # bit e*bits of the group integer is the element's lowest bit: an independent look at one element
        e = (n - 1) % 32
        assert (big >> (e * bits)) & (2 ** bits - 1) == int(c[-1])


@pytest.mark.parametrize("fname,formula", [("g2_weight_quant_admm", 0), ("g2_weight_quant_cdfonly", 1)])
def test_reference_weights_survive_the_packed_form(fname, formula):
    """G2: dequant(unpack(pack(codes(Wq)))) == Wq element for element, bit-equal to Wq + 0 (the ADMM tree's -0 comes back as +0)"""
    g = load_golden(fname)
    seen = 0
    for key in sorted(g):
        if not key.startswith("Wq_"):
            continue
        k = int(key.rsplit("_k", 1)[1])
        wq = g[key].astype(np.float32).reshape(-1)
        bits = PO.code_bits(k, formula)
        c = PO.codes(wq, k, formula)
        assert int(c.max()) < 2 ** bits
        back = PO.dequant(PO.unpack_fast(PO.pack(c, bits), wq.size, bits), k, formula)
        assert back.dtype == np.float32
        assert np.array_equal(back, wq)                                            # ==: -0 equals +0
        assert np.array_equal(back.view(np.uint32), (wq + np.float32(0)).view(np.uint32))
        if formula == 1:
            assert np.array_equal(back.view(np.uint32), wq.view(np.uint32))       # the CDF tree has no -0
        seen += 1
    assert seen == (9 if formula == 0 else 6)          # every Wq_* of the fixture: 3 (2) shapes x k in {2, 4, 8}


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_abi_queries_and_null_tables():
    from alignq_amd import _lib, export
    lib = _lib.load()
    assert lib.alignq_packed_bytes(0, 9) == 0 and lib.alignq_packed_bytes(1, 1) == 4
    assert lib.alignq_packed_bytes(33, 9) == 72 and lib.alignq_packed_bytes(36864, 9) == 41472
    assert lib.alignq_packed_bytes(5, 0) == 0 and lib.alignq_packed_bytes(5, 18) == 0 and lib.alignq_packed_bytes(-1, 9) == 0
    assert lib.alignq_weight_code_bits(8, 0) == 9 and lib.alignq_weight_code_bits(8, 1) == 8
    assert lib.alignq_weight_code_bits(1, 0) == 2 and lib.alignq_weight_code_bits(17, 0) == 0 and lib.alignq_weight_code_bits(0, 1) == 0
    for k in range(1, 17):
        for formula in (0, 1):
            assert lib.alignq_weight_code_bits(k, formula) == export.code_bits(k, formula) == PO.code_bits(k, formula)
    for n in (1, 31, 32, 33, 36864):
        assert lib.alignq_packed_bytes(n, 9) == export.packed_bytes(n, 9) == 4 * PO.packed_words(n, 9)
    assert lib.alignq_weight_pack_multi(1, None, None, 8, 0, None, None, None) == -1
    assert lib.alignq_weight_unpack_multi(1, None, None, 8, 0, None, None, None, None, None, None) == -1


# ------------------------------------------------------------------------------------------------------------ PackedModel
def _tiny(tree, seed, wbit=8):
    from alignq_amd import config
    from alignq_amd.resnet import PreActBlock_conv_Q, PreActResNet
    old = config.args.train_batch_size
    config.args.train_batch_size = 16
    try:
        torch.manual_seed(seed)
        return PreActResNet(PreActBlock_conv_Q, [1, 1, 1], wbit, 8, "second", 10, tree=tree)
    finally:
        config.args.train_batch_size = old


def _by_hand(net, seed):
    """a PackedModel of `net` whose codes are random valid codes packed by the oracle"""
    from alignq_amd import export
    rng = np.random.default_rng(seed)
    filters, raw = {}, {}
    for name, c in export.quantised_convs(net):
        k, formula = c.quantize_fn.w_bit, c.quantize_fn._formula
        bits = PO.code_bits(k, formula)
        top = 2 * (2 ** k - 1) if formula == 0 else 2 ** k - 1
        codes = rng.integers(0, top + 1, size=c.weight.numel(), dtype=np.uint64).astype(np.uint32)
        raw[name] = codes
        filters[name] = {"codes": torch.from_numpy(PO.pack(codes, bits).view(np.int32).copy()), "shape": list(c.weight.shape),
                         "w_bit": int(k), "formula": int(formula), "bits": bits}
    drop = set(filters) | export.admm_keys(net)
    rest = {k: v.detach().clone() for k, v in net.state_dict().items() if k not in drop}
    meta = {"format": export.FORMAT, "version": export.FORMAT_VERSION, "act_range": 2.0}
    return export.PackedModel(meta, filters, rest), raw


@pytest.mark.parametrize("tree", ["admm", "cdf"])
def test_packed_model_file_sizes_and_apply(tree, tmp_path):
    from alignq_amd import _lib, export
    lib = _lib.load()
    net = _tiny(tree, 1)
    with torch.no_grad():                                 # batch-norm state that differs from a fresh net's
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_()
                m.running_var.uniform_(0.5, 2.0)
                m.num_batches_tracked.fill_(7)
    pk, raw = _by_hand(net, 2)
    assert len(pk.filters) == 9                           # the stem, three blocks of two, two shortcut convolutions
    assert set(pk.filters) == {n for n, _ in export.quantised_convs(net)}
    if tree == "admm":
        assert export.admm_keys(net) and not (export.admm_keys(net) & set(pk.rest))
        # every name of an ADMM matrix (the block's and the activation quantiser's `opt`), and nothing else
        assert export.admm_keys(net) == {k for k in net.state_dict() if k.endswith((".alterD", ".gamma"))}
    assert not any(k.endswith((".alterD", ".gamma")) for k in pk.rest)
    # save -> load: equal tensors and meta, loadable with weights_only=True
    path = os.path.join(tmp_path, "tiny.alignq")
    pk.save(path)
    back = export.PackedModel.load(path)
    assert back.meta == pk.meta and back.meta["version"] == 1
    assert set(back.filters) == set(pk.filters) and set(back.rest) == set(pk.rest)
    for name, f in pk.filters.items():
        b = back.filters[name]
        assert torch.equal(b["codes"], f["codes"]) and b["codes"].dtype == torch.int32
        assert (list(b["shape"]), b["w_bit"], b["formula"], b["bits"]) == (list(f["shape"]), f["w_bit"], f["formula"], f["bits"])
        assert np.array_equal(PO.unpack_fast(b["codes"].numpy().view(np.uint32), raw[name].size, b["bits"]), raw[name])
    for name, v in pk.rest.items():
        assert torch.equal(back.rest[name], v) and back.rest[name].dtype == v.dtype
    # sizes
    want = sum(lib.alignq_packed_bytes(c.weight.numel(), pk.filters[n]["bits"]) for n, c in export.quantised_convs(net))
    want += sum(v.numel() * v.element_size() for v in pk.rest.values())
    assert pk.nbytes() == back.nbytes() == want
    assert pk.dense_nbytes() == sum(4 * c.weight.numel() for _, c in export.quantised_convs(net)) + \
        sum(v.numel() * v.element_size() for v in pk.rest.values())
    dense = os.path.join(tmp_path, "dense.pt")
    torch.save(net.state_dict(), dense)
    assert os.path.getsize(path) < os.path.getsize(dense)
    # apply: a fresh net's non-filter state becomes the packed model's; its filters stay
    fresh = _tiny(tree, 3)
    before = {n: c.weight.detach().clone() for n, c in export.quantised_convs(fresh)}
    assert not torch.equal(fresh.state_dict()["logit.weight"], net.state_dict()["logit.weight"])
    back.apply(fresh)
    sd, ref = fresh.state_dict(), net.state_dict()
    for name in pk.rest:
        assert torch.equal(sd[name], ref[name]), name
    for name, w in before.items():
        assert torch.equal(sd[name], w)
    # mismatches are named
    wrong_shape = export.PackedModel(pk.meta, pk.filters, dict(pk.rest, **{"logit.weight": torch.zeros(10, 32)}))
    with pytest.raises(ValueError, match="logit.weight"):
        wrong_shape.apply(_tiny(tree, 4))
    extra = export.PackedModel(pk.meta, pk.filters, dict(pk.rest, **{"nowhere.bias": torch.zeros(3)}))
    with pytest.raises(ValueError, match="nowhere.bias"):
        extra.apply(_tiny(tree, 4))
    missing = export.PackedModel(pk.meta, pk.filters, {k: v for k, v in pk.rest.items() if k != "bn.weight"})
    with pytest.raises(ValueError, match="bn.weight"):
        missing.apply(_tiny(tree, 4))
    wrong_filter = dict(pk.filters)
    wrong_filter["conv0.weight"] = dict(pk.filters["conv0.weight"], shape=[16, 3, 5, 5])
    with pytest.raises(ValueError, match="conv0.weight"):
        export.PackedModel(pk.meta, wrong_filter, pk.rest).apply(_tiny(tree, 4))


def test_load_refuses_other_files(tmp_path):
    from alignq_amd import export
    path = os.path.join(tmp_path, "plain.pt")
    torch.save({"a": torch.zeros(2)}, path)
    with pytest.raises(ValueError, match="format"):
        export.PackedModel.load(path)


def test_pack_model_needs_the_gpu():
    from alignq_amd import export
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        export.pack_model(_tiny("admm", 5))


def test_eval_step_checks_packed_weights_before_any_launch():
    """the ValueError paths of EvalStep(weights=) need no GPU: they are raised by the constructor"""
    from alignq_amd import export
    from alignq_amd.eval_step import EvalStep
    net = _tiny("admm", 6)
    pk, _ = _by_hand(net, 7)
    with pytest.raises(ValueError, match="channels_last"):
        EvalStep(_tiny("admm", 8), channels_last=False, weights=pk)
    with pytest.raises(ValueError, match="w_bit"):
        EvalStep(_tiny("admm", 8, wbit=4), weights=pk)
    fewer = export.PackedModel(pk.meta, {k: v for k, v in pk.filters.items() if k != "layers.1.conv1.weight"}, pk.rest)
    with pytest.raises(ValueError, match="layers.1.conv1.weight"):
        EvalStep(_tiny("admm", 8), weights=fewer)
    with pytest.raises(ValueError, match="formula"):
        EvalStep(_tiny("cdf", 8), weights=pk)
