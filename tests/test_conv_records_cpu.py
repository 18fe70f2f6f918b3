"""The lazy batch-norm record (fused.LazyBN) hands its tensors to the convolution backward kernels by POSITION: the order in which
`LazyBN.operands` yields them must be the order in which include/alignq.h declares the bn_* parameters of every entry point that
takes them.  No GPU: the header is read as text (like test_abi.py), the record is filled with placeholders."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# header parameter (prefix stripped) -> LazyBN field
FIELD = {"z": "z", "ab": "ab", "save": "save", "ktot": "ktot", "dx_part": "part", "dgamma": "dgamma", "dbeta": "dbeta"}


def _params(name):
    src = open(os.path.join(ROOT, "include", "alignq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % re.escape(name), src)
    assert m, name
    return [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", p)[-1] for p in m.group(1).split(",")]


def _records():
    """(record whose consumer reduces the per-tile sums itself: no totals; record with finished totals) - distinct placeholders"""
    from alignq_amd.fused import LazyBN
    tag = {f: object() for f in LazyBN._fields}
    return LazyBN(**dict(tag, ktot=None)), LazyBN(**dict(tag, part=None, dgamma=None, dbeta=None))


@pytest.mark.parametrize("name,prefixes,count", [
    ("alignq_conv3x3_nhwc_bwd_fill", ["bn_"], 7), ("alignq_conv3x3_nhwc_bwd_fill_img", ["bn_"], 7),
    ("alignq_conv_gen_nhwc_dgrad", ["bn_"], 7), ("alignq_conv_gen_nhwc_dgrad_img", ["bn_"], 7),
    ("alignq_conv_gen_nhwc_wgrad", ["bn_"], 5),            # the filter gradient takes the first five only
    ("alignq_conv_stem_nhwc_wgrad", ["bn_"], 7),
    ("alignq_transition_nhwc_bwd", ["bn3_", "bn1_"], 7), ("alignq_transition_nhwc_bwd_img", ["bn3_", "bn1_"], 7)])
def test_lazy_bn_operands_come_in_the_headers_order(name, prefixes, count):
    params = _params(name)
    for prefix in prefixes:
        declared = [p[len(prefix):] for p in params if p.startswith(prefix)]
        assert len(declared) == count and set(declared) <= set(FIELD), (name, declared)
        at = params.index(prefix + declared[0])
        assert params[at:at + count] == [prefix + d for d in declared], "the bn_* parameters are consecutive"
        for rec in _records():
            got = rec.operands()[:count]          # (what ops passes: all seven, or - alignq_conv_gen_nhwc_wgrad - the first five)
            assert len(got) == count
            for d, t in zip(declared, got):
                assert t is getattr(rec, FIELD[d]), (name, prefix + d)


def test_lazy_bn_record_fields_and_the_empty_record():
    from alignq_amd import fused
    assert fused.LazyBN._fields == ("g", "z", "ab", "save", "ktot", "part", "dgamma", "dbeta")
    assert fused.NO_LAZY_BN.operands() == (None,) * 7 and fused.NO_LAZY_BN.operands(True, 2, 16, 64) == (None,) * 7
    assert fused.take_lazy_dz(None, None) is fused.NO_LAZY_BN and fused.take_lazy_dz(fused.LazyLink(), None) is fused.NO_LAZY_BN
    with_totals = _records()[1]
    assert with_totals.operands(True, 2, 16, 64) == with_totals.operands()      # totals there: nothing to launch
    # per-tile sums ride along only while there are no totals (the kernels read bn_ktot == NULL as "reduce bn_dx_part yourself")
    both = with_totals._replace(part=object())
    assert both.operands()[3] is both.ktot and both.operands()[4] is None


def test_conv_stats_records_read_by_index_like_the_tuples_they_replace():
    from alignq_amd import fused
    part, link = object(), fused.LazyLink()
    assert tuple(fused.ConvStats(part, 4)) == (part, 4, 0, None)
    assert fused.ConvStats(part, 4, 2, link)[:3] == (part, 4, 2) and fused.ConvStats(part, 4, 2, link).link is link
    assert tuple(fused.ConvStatsQ(part, 4, 2)) == (part, 4, 2)
