"""Which kernel family a Conv2d_Q convolution gets is behaviour: several shapes are taken by more than one family and the order
decides.  tests/golden/g23_conv_dispatch.json records the choice (autograd node, by-product record, output shape) for every family's
smallest shape, one perturbation across every condition of every predicate, every flag combination, packed handles and the overlapping
shapes, plus the node counts of whole models; this file recomputes every row (tests/golden/gen_goldens_conv_dispatch.py holds the
cases) and compares.  Names and shapes only, no values."""
import json

import pytest
import torch

from tests.golden import gen_goldens_conv_dispatch as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def record():
    with open(G.PATH) as f:
        return json.load(f)


def _differences(got, want):
    got = json.loads(json.dumps(got))
    assert sorted(got) == sorted(want), "the cases and the recorded rows are not the same set: regenerate at the recorded commit"
    return {name: (got[name], want[name]) for name in want if got[name] != want[name]}


def test_single_convolutions_get_the_recorded_family(dev, record):
    got = {c["name"]: G.run_single(c, dev) for c in G.single_cases()}
    assert not _differences(got, record["single"])


def test_transition_pairs_get_the_recorded_node(dev, record):
    got = {c["name"]: G.run_transition(c, dev) for c in G.transition_cases()}
    assert not _differences(got, record["transition"])


def test_whole_models_reach_the_recorded_nodes(dev, record):
    assert not _differences(G.model_records(dev), record["models"])


def test_the_record_cannot_pass_by_testing_nothing(record):
    """every family's node occurs, and every perturbation leaves its base's path or states why not (the generator's own assertions,
    on the committed file)"""
    assert not G.problems(record)
