"""CPU-side checks of the case table of the 5x5 convolutions (tests/k5conv_exact_oracle.py; include/alignq_k5conv.h): every row keeps
the 2^24 budget and holds the operand classes it claims, the launch forms and slab counts restated in the oracle are what the library
answers, and the table reaches every launch form, both forms of the filter, every w_bit, every term class and pair, and every edge of
the tiles, the grid and the slabs."""
import os

import pytest
import torch

from tests import k5conv_exact_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ids(cases):
    return [c["id"] for c in cases]


def _geom(c):
    return c["B"], c["H"], c["W"], c["cin"], c["cout"]


def _by_id(cases):
    return {c["id"]: c for c in cases}


@pytest.mark.parametrize("c", O.G_CASES, ids=_ids(O.G_CASES))
def test_forward_and_data_gradient_rows_keep_the_budget_and_their_classes(c):
    a, b = O.g_operands(c)
    worst = O.g_budget(c, a, b)
    assert 0 < worst < O.TWO24
    assert int(b.abs().max()) <= O.nlev_of(c) and tuple(b.shape) == (c["cout"], 5, 5, c["cin"])
    ref = O.g_reference(c, a, b)
    assert tuple(ref.shape) == ((c["B"], c["h"], c["w"], c["cout"]) if c["op"] == "fwd" else (c["B"], c["H"], c["W"], c["cin"]))
    assert tuple(ref.shape[:3]) == (c["B"], c["h"], c["w"])          # the row's grid is the grid the operation tiles
    f2, f3 = O.class_fractions(a)
    if c["set"] == "dense":
        assert (f2, f3) == (0.0, 0.0) and int(a.abs().max()) <= 255          # class 1: one bf16 term
        assert int(b.abs().max()) == O.g_amps(c)[1]
    else:
        assert f2 == 1.0 and f3 > 0.3                                        # class 3: all three terms carry value
        # every (output, tap) contraction meets a non-zero bin: no tap is trivially absent
        assert bool((b.abs().sum(dim=3 if c["op"] == "fwd" else 0) > 0).all())


def test_dense_amplitudes_and_the_bias():
    """amp = 255 at K = 3 or 4, 73 at 36, 5 at 512, and never above n; the bias: distinct, not integer-valued, 1e-3 .. 1e3, both signs"""
    def amp(op, cin, cout, k):
        return O.g_amps(dict(op=op, cin=cin, cout=cout, w_bit=k))[1]
    assert amp("fwd", 3, 128, 8) == 255 and amp("dgrad", 512, 4, 8) == 255 and amp("fwd", 4, 4, 8) == 255
    assert amp("dgrad", 36, 48, 8) == 54 and amp("fwd", 512, 4, 8) == 5 and amp("dgrad", 4, 512, 4) == 5
    assert [amp("fwd", 36, 48, k) for k in (1, 2, 4, 8)] == [1, 3, 15, 73]
    assert {O.nlev_of(c) for c in O.G_CASES} == {1.0, 3.0, 15.0, 255.0}
    for cout in sorted({c["cout"] for c in O.FWD}):
        b = O.bias_of(cout)
        assert b.dtype == torch.float32 and len(set(b.tolist())) == cout and bool((b != b.round()).all())
        assert 1e-3 <= float(b.abs().min()) and float(b.abs().max()) <= 1e3 and (cout < 2 or (bool((b > 0).any()) and bool((b < 0).any())))
        assert torch.equal(b, O.bias_of(cout))
    q = torch.tensor([[1.0, 3.0]], dtype=torch.float32) / torch.tensor(3.0, dtype=torch.float32)
    assert torch.equal(O.with_bias(q, torch.tensor([0.5, -0.25])), torch.tensor([[q[0, 0] + 0.5, 0.75]]))


@pytest.mark.parametrize("c", O.ALL_WGRAD, ids=_ids(O.ALL_WGRAD))
def test_filter_gradient_rows_keep_the_budget_and_their_classes(c):
    x, dy = O.wgrad_operands(c)
    assert tuple(x.shape) == (c["B"], c["h"] + 4, c["w"] + 4, c["cin"]) and tuple(dy.shape) == (c["B"], c["h"], c["w"], c["cout"])
    worst = O.assert_exact_budget(O.wgrad_i64, x, dy, ks=5, stride=1, pad=0)
    assert 0 < worst < O.TWO24
    if c["set"] == "dense":
        assert O.class_fractions(x) == (0.0, 0.0) and O.class_fractions(dy) == (0.0, 0.0)
        return
    want = {1: (0.0, 0.0), 2: (1.0, 0.0)}
    for t, cls in ((dy, int(c["set"][2])), (x, int(c["set"][5]))):
        f2, f3 = O.class_fractions(t)
        if cls == 3:
            assert f2 == 1.0 and f3 > 0.3
        else:
            assert (f2, f3) == want[cls]
    # the sparse pixels, on the output grid: image corners, the last pixel, both sides of a step boundary each way, every 4-pixel
    # block of a step
    assert O.wgrad_steps(c) == 18
    for co in (0, c["cout"] - 1):
        px = O.wgrad_pixels(c, co)
        assert {(0, 0, 0), (c["B"] - 1, c["h"] - 1, c["w"] - 1), (0, 1, 7), (0, 1, 8), (0, 3, 2), (0, 4, 2)} <= set(px)
        assert {(8 * h + w) // 4 for b, h, w in px if b == 1} == set(range(8))
        assert all(int(dy[b, h, w, co]) != 0 for b, h, w in px) and int((dy[..., co] != 0).sum()) == O.SPARSE_K == 16


def test_pair_rows_cover_the_pairs_the_header_takes():
    """(dy, x) classes (1,3), (3,1), (2,2): x0d0 x1d0 x2d0 | x0d0 x0d1 x0d2 | x0d0 x1d0 x0d1 x1d1 - the six pairs of the header - at
    all three filter-gradient forms"""
    from tests.conv_exact_oracle import PAIR_CLASSES
    assert O.PAIR_CLASSES == PAIR_CLASSES
    assert {(c["form"], c["set"]) for c in O.WGRAD_PAIRS} == {(f, "dy%d_x%d" % p) for f in O.FORMS[O.K5_WGRAD] for p in PAIR_CLASSES}
    kept = set()
    for dcls, xcls in O.PAIR_CLASSES:          # a class-a operand has terms 0 .. a - 1
        kept |= {(xt, dt) for xt in range(xcls) for dt in range(dcls)}
    with open(os.path.join(ROOT, "include", "alignq_k5conv.h")) as f:
        text = f.read()
    order = "(x1,d1) (x0,d2) (x2,d0) (x0,d1) (x1,d0) (x0,d0)"
    assert order in text
    assert kept == {(int(p[2]), int(p[5])) for p in order.split()} and len(kept) == 6


def test_restated_forms_and_slab_counts_are_the_librarys():
    """alignq_k5conv_form and alignq_k5conv_wgrad_ws_bytes need no GPU: the set of values the library can return over every supported
    channel pair is the table's FORMS, and every row's form and slab count, computed in the oracle, is what the library answers"""
    from alignq_amd import _lib
    lib = _lib.load()
    seen = {op: set() for op in O.FORMS}
    for cin in [3] + list(range(4, 513, 4)):
        for cout in range(4, 513, 4):
            for op in O.FORMS:
                f = lib.alignq_k5conv_form(op, 3, 9, 9, cin, cout)
                if cin == 3 and op == O.K5_DGRAD:
                    assert f == -1 and lib.alignq_k5conv_supported(op, 3, 9, 9, cin, cout) == 0
                    continue
                want = {O.K5_FWD: O.gemm_form(cout), O.K5_DGRAD: O.gemm_form(cin), O.K5_WGRAD: O.wgrad_form(cin, cout)}[op]
                assert f == want, (op, cin, cout)
                seen[op].add(f)
    assert seen == O.FORMS
    for name, rows in (("fwd", O.FWD), ("dgrad", O.DGRAD), ("wgrad", O.ALL_WGRAD)):
        op = O.OPS[name]
        assert {c["form"] for c in rows} == O.FORMS[op], name          # N16 / N32 / N64 twice, W64X16 / W16X64 / WIMAGE
        for c in rows:
            assert c["op"] == name
            assert lib.alignq_k5conv_supported(op, *_geom(c)) == 1 and lib.alignq_k5conv_form(op, *_geom(c)) == c["form"], c["id"]
            if name == "wgrad":
                n_slabs, per = O.wgrad_slabs(c)
                assert (n_slabs - 1) * per < O.wgrad_steps(c) <= n_slabs * per, c["id"]          # no slab is empty
                assert lib.alignq_k5conv_wgrad_ws_bytes(*_geom(c)) == n_slabs * 4 * 25 * c["cin"] * c["cout"], c["id"]
    # the image form reaches every forward width too, and the body form every data-gradient width
    assert {c["form"] for c in O.FWD if O.is_image(c)} == O.FORMS[O.K5_FWD] == {c["form"] for c in O.FWD if not O.is_image(c)}
    assert not any(O.is_image(c) for c in O.DGRAD)
    assert lib.alignq_k5conv_form(3, 3, 9, 9, 12, 12) == -1 and lib.alignq_k5conv_form(O.K5_FWD, 3, 4, 9, 12, 12) == -1
    # spot values of the restated rules
    assert [O.gemm_form(n) for n in (4, 12, 20, 24, 32, 36, 48, 64, 68, 128, 512)] == [0, 0, 1, 1, 1, 0, 0, 2, 0, 2, 2]
    w = _by_id(O.ALL_WGRAD)
    assert O.wgrad_slabs(w["wgrad_24x12_B1H1W1_dense"]) == (1, 1) and O.wgrad_slabs(w["wgrad_24x12_B3H9W9_dense"]) == (9, 2)
    assert O.wgrad_slabs(w["wgrad_4x4_B16H64W64_dense"]) == (512, 4) == O.wgrad_slabs(w["wgrad_3x4_B16H64W64_dense"])
    assert O.wgrad_slabs(w["wgrad_24x12_B5H4W8_dense"]) == (3, 2) == O.wgrad_slabs(w["wgrad_3x68_B5H4W8_dense"])
    assert O.wgrad_channel_tiles(w["wgrad_36x48_B3H5W5_dense"]) == 3 and O.wgrad_channel_tiles(w["wgrad_48x36_B3H5W5_dense"]) == 3
    assert O.wgrad_channel_tiles(w["wgrad_8x128_B3H5W5_dense"]) == 2 and O.wgrad_channel_tiles(w["wgrad_128x8_B3H5W5_dense"]) == 2
    assert O.wgrad_channel_tiles(w["wgrad_512x4_B3H5W5_dense"]) == 8 and O.wgrad_channel_tiles(w["wgrad_3x68_B3H5W5_dense"]) == 2
    assert O.wgrad_channel_tiles(w["wgrad_12x132_B3H9W9_dy2_x2"]) == 3


def test_table_reaches_every_edge():
    # slab counts: one, above 256, an uneven last slab
    slabs = {c["id"]: O.wgrad_slabs(c) for c in O.ALL_WGRAD}
    assert min(n for n, _ in slabs.values()) == 1 and max(n for n, _ in slabs.values()) > 256
    assert any(O.wgrad_steps(c) % slabs[c["id"]][1] for c in O.ALL_WGRAD)
    for form in O.FORMS[O.K5_WGRAD]:
        rows = [c for c in O.ALL_WGRAD if c["form"] == form]
        assert {1, 3, 9} <= {slabs[c["id"]][0] for c in rows}, form
        assert any(O.wgrad_steps(c) == 5 and slabs[c["id"]] == (3, 2) for c in rows), form          # slabs of 2, 2 and 1 steps
    # the grid-stride cases lie beyond one pass of the grid cap and the write-through cases inside one pass; both inside the window
    # (1 MiB .. 64 MiB), every other row below it
    bigs = [c for c in O.G_CASES if (c["B"], c["h"], c["w"]) == O.GBIG]
    wts = [c for c in O.G_CASES if (c["B"], c["h"], c["w"]) == O.GWT]
    assert {(c["op"], c["cin"], c["cout"]) for c in bigs} == {("fwd", 4, 4), ("fwd", 3, 4), ("dgrad", 4, 4)}
    assert {(c["op"], c["cin"], c["cout"]) for c in wts} == {("fwd", 4, 4), ("fwd", 3, 4), ("dgrad", 4, 4)}
    assert all(O.grid_tiles(c) > O.GRID_TILES for c in bigs) and all(O.grid_tiles(c) <= O.GRID_TILES for c in wts)
    for c in O.G_CASES:
        nbytes = 4 * O.rows_of(c) * (c["cout"] if c["op"] == "fwd" else c["cin"])
        assert ((1 << 20) <= nbytes <= (64 << 20)) == (c in bigs or c in wts), c["id"]
    assert min(4 * O.rows_of(c) * c["cout"] for c in wts) == 1 << 20
    assert {(c["cin"], c["cout"]) for c in O.ALL_WGRAD if (c["B"], c["h"], c["w"]) == O.GWT} == {(4, 4), (3, 4)}
    # every channel pair at 3 x 5 x 5 (B > 1), the filter gradient at 3 x 9 x 9 too
    pairs = set(O.SHAPES)
    assert {(4, 4), (12, 24), (36, 48), (48, 36), (64, 64), (8, 128), (128, 8), (512, 4), (4, 512)} <= pairs
    image = {(3, co) for co in (4, 20, 32, 64, 68, 128)}
    at = lambda rows, grid, s="dense": {(c["cin"], c["cout"]) for c in rows if (c["B"], c["h"], c["w"]) == grid and c["set"] == s}  # noqa: E731
    assert at(O.FWD, O.G355) == pairs | image and at(O.DGRAD, O.G355) == pairs
    assert at(O.ALL_WGRAD, O.G355) == pairs | image == at(O.ALL_WGRAD, O.GPAIR)
    # the spatial edges on the tiled grid: one pixel, one row, one column (the data gradient: dy of one pixel, row, column) and
    # tile - 1, tile, tile + 1 each way, on one pair per form and on two image COUT
    for rows, small, extra in ((O.FWD, [O.G1, O.GROW, O.GCOL], []), (O.DGRAD, [O.D1, O.DROW, O.DCOL], []),
                               (O.ALL_WGRAD, [O.G1, O.GROW, O.GCOL], O.STEP_GRIDS + [O.GSLAB])):
        for grid in small + O.EDGE_GRIDS + extra:
            here = [c for c in rows if (c["B"], c["h"], c["w"]) == grid]
            assert {c["form"] for c in here} == O.FORMS[O.OPS[rows[0]["op"]]], grid
            assert rows is O.DGRAD or sum(O.is_image(c) for c in here) == 2, grid
    assert (O.D1, O.DROW, O.DCOL) == ((1, 5, 5), (2, 5, 9), (2, 9, 5)) and O.EDGE_GRIDS == [(1, 7, 9), (1, 8, 8), (1, 9, 7)]
    assert O.STEP_GRIDS == [(1, 3, 9), (1, 4, 8), (1, 5, 7)] and O.GSLAB == (5, 4, 8)
    # the operand sets: class-3 activations on the four body pairs both ways and on image COUT 20 and 64, one row at w_bit 4; a dense
    # body row and an image row at every w_bit; every other row alternates 4 and 8
    assert at(O.FWD, O.G355, "act3") == {(12, 24), (36, 48), (48, 36), (64, 64), (3, 20), (3, 64)}
    assert at(O.DGRAD, O.G355, "act3") == {(12, 24), (36, 48), (48, 36), (64, 64)} == at(O.DGRAD, O.GPAIR, "act3")
    for rows in (O.FWD, O.DGRAD):
        assert any(c["set"] == "act3" and c["w_bit"] == 4 for c in rows)
        assert {c["w_bit"] for c in rows if c["set"] == "dense" and not O.is_image(c)} == {1, 2, 4, 8}
        rest = [c["w_bit"] for c in rows if (c["B"], c["h"], c["w"]) != O.GBITS]
        assert set(rest) == {4, 8} and abs(rest.count(4) - rest.count(8)) <= 4
    assert {c["w_bit"] for c in O.FWD if c["set"] == "dense" and O.is_image(c)} == {1, 2, 4, 8}
    assert len(O.G_CASES) + len(O.ALL_WGRAD) < 300
