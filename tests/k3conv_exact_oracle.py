"""Exact-integer operand sets and the case table for the 3x3 convolutions of csrc/k3conv_kernels.hip (alignq_k3conv_fwd / _dgrad /
_wgrad, include/alignq_k3conv.h).  tests/test_k3conv_oracle_cpu.py proves every condition on the CPU, tests/test_gpu_k3conv_exact.py
runs the kernels.

The method is tests/conv_exact_oracle.py's: integer operands, sum of |products| below 2^24 per output element, so the kernel must
return fp32(int64 sum) / fp32(n) (forward, data gradient: one IEEE division) or fp32(int64 sum) (filter gradient), bit for bit,
whatever the tile, the tap, chunk or term order or the slab.  The references (conv_i64, dgrad_i64, wgrad_i64 at ks = 3, stride 1,
pad 1), the budget assertion, the bf16 term classes and the generators come from that module, the quotient from
tests/qgemm_exact_oracle.py.

The launchers' arithmetic, restated (the GPU test asserts it through alignq_k3conv_form, alignq_k3conv_wgrad_ws_bytes and n_slabs_out):
  forward / data gradient: N = COUT / CIN output columns, tiles of 8 x 8 pixels of one image x BN channels, BN the widest of 64, 32, 16
      with ceil(N / BN) BN == ceil(N / 16) 16 (form 2, 1, 0); at most 2048 spatial tiles in the grid, the rest by grid stride;
      K = CIN / COUT in 32-deep chunks, the tail zero; nine taps per chunk;
  filter gradient: a (CIN x COUT) tile of 64 x 16 channels where CIN >= COUT (form 0), else 16 x 64 (form 1); a step is a 4 x 8 pixel
      tile of one image: T = B ceil(H / 4) ceil(W / 8) steps; s = max(1, min(ceil(512 / channel tiles), ceil(T / 2), 1024)),
      per = ceil(T / s) steps per slab, n_slabs = ceil(T / per): no slab is empty.

Tensors are NHWC, filters [Cout, 3, 3, Cin], int64 on the CPU.  Nothing of the package is imported."""
import torch

from tests.conv_exact_oracle import (I64, TWO24, _gen, assert_exact_budget, bf16_terms, class_fractions, conv_i64, dgrad_i64,  # noqa: F401
                                     gen_by_class, gen_class1, gen_class2, gen_class3, sparse_bins, wgrad_i64)
from tests.qgemm_exact_oracle import quotient  # noqa: F401

K3_FWD, K3_DGRAD, K3_WGRAD = 0, 1, 2
TILE = 8                    # the forward / data-gradient tile is TILE x TILE pixels
GRID_TILES = 2048           # spatial tiles the grid holds
STEP_H, STEP_W = 4, 8       # the filter-gradient step is a STEP_H x STEP_W pixel tile
FORMS = {K3_FWD: {0, 1, 2}, K3_DGRAD: {0, 1, 2}, K3_WGRAD: {0, 1}}          # every value alignq_k3conv_form returns


def gemm_form(n):
    r16 = -(-n // 16) * 16
    return 2 if -(-n // 64) * 64 == r16 else (1 if -(-n // 32) * 32 == r16 else 0)


def wgrad_form(cin, cout):
    return 0 if cin >= cout else 1


# (CIN, COUT), the smallest shapes that reach each edge: one chunk's quarter (4), 12 = DenseNet's growth rate, 36 = one 32-deep chunk
# + 4, 444 = the longest DenseNet contraction (14 chunks, the last 28 deep) and, transposed, 7 x 64 output channels less 4, 64 x 64 =
# four full 16-wide blocks, 512 = the limit, (12, 24) = the forward's 32-wide tile
SHAPES = [(4, 4), (12, 12), (24, 12), (36, 12), (444, 12), (12, 444), (64, 64), (512, 4), (4, 512), (12, 24)]
# (B, h, w): one pixel (only the centre tap is live); one row; one column; 3 x 5 x 5 (B > 1: a halo that reads into the neighbouring
# image or row shows in the values); tile - 1, tile, tile + 1 in each of H and W for the 8 x 8 tile and for the 4 x 8 step
G1, GROW, GCOL, G355 = (1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 5, 5)
EDGE_GRIDS = [(1, 7, 9), (1, 8, 8), (1, 9, 7)]
STEP_GRIDS = [(1, 3, 9), (1, 4, 8), (1, 5, 7)]
GBIG = (33, 64, 64)         # 33 x 64 = 2112 tiles: beyond one pass of the grid cap (2.1 MiB at 4 channels: write-through, too)
GWT = (16, 64, 64)          # 1 MiB at 4 channels: the first size of the write-through window, one pass of the grid
EDGE_SHAPES = [(12, 12), (12, 24), (24, 12), (64, 64)]          # every forward and data-gradient form


def rows_of(c):
    return c["B"] * c["h"] * c["w"]


def _row(op, shape, grid, **kw):
    cin, cout = shape
    B, h, w = grid
    c = dict(op=op, cin=cin, cout=cout, B=B, h=h, w=w, set="dense", w_bit=8)
    c.update(kw)
    c["form"] = {"fwd": gemm_form(cout), "dgrad": gemm_form(cin), "wgrad": wgrad_form(cin, cout)}[op]
    c["id"] = "%s_%dx%d_B%dH%dW%d_%s" % (op, cin, cout, B, h, w, c["set"])
    return c


ACT3_SHAPES = [(12, 12), (24, 12), (36, 12), (444, 12), (12, 444), (64, 64)]


def _g_rows(op):
    rows = [_row(op, s, G355) for s in SHAPES]
    rows += [_row(op, s, g) for s in EDGE_SHAPES for g in [G1, GROW, GCOL] + EDGE_GRIDS]
    rows += [_row(op, (4, 4), GBIG), _row(op, (4, 4), GWT)]
    rows += [_row(op, s, G355, set="act3") for s in ACT3_SHAPES]
    rows += [_row(op, (36, 12), EDGE_GRIDS[2], set="act3", w_bit=4)]
    return rows


FWD, DGRAD = _g_rows("fwd"), _g_rows("dgrad")
G_CASES = FWD + DGRAD
ACT3_NNZ, ACT3_AMP = 2, 3          # 2^18 * 9 * 2 * 3 < 2^24


def nlev_of(c):
    return float((1 << c["w_bit"]) - 1)


def contraction(c):
    return 9 * (c["cin"] if c["op"] == "fwd" else c["cout"])


def g_amps(c):
    """(largest |activation|, largest |bin|) of a dense case: the bins shrink as K grows so that K * 255 * bin < 2^24"""
    return 255, max(1, min(int(nlev_of(c)), (TWO24 - 1) // (contraction(c) * 255)))


def g_operands(c, seed=0):
    """(activation, bins [cout, 3, 3, cin]) as int64: x [B, h, w, cin] for a forward, dy [B, h, w, cout] for a data gradient"""
    shape = (c["B"], c["h"], c["w"], c["cin"] if c["op"] == "fwd" else c["cout"])
    if c["set"] == "act3":
        return gen_class3(shape, 100 + seed), sparse_bins(c["cout"], 3, c["cin"], ACT3_NNZ, ACT3_AMP, "ci" if c["op"] == "fwd" else "co",
                                                          200 + seed)
    act, amp = g_amps(c)
    g = _gen(300 + seed)
    a = torch.randint(0 if c["op"] == "fwd" else -act, act + 1, shape, generator=g, dtype=I64)
    return a, torch.randint(-amp, amp + 1, (c["cout"], 3, 3, c["cin"]), generator=g, dtype=I64)


def g_reference(c, a, b):
    """the integer sums: y [B, h, w, cout] or dx [B, h, w, cin]"""
    return conv_i64(a, b, 1, 1) if c["op"] == "fwd" else dgrad_i64(a, b, 1, 1, c["h"], c["w"])


def g_budget(c, a, b):
    if c["op"] == "fwd":
        return assert_exact_budget(conv_i64, a, b, stride=1, pad=1)
    return assert_exact_budget(dgrad_i64, a, b, stride=1, pad=1, h_in=c["h"], w_in=c["w"])


def grid_tiles(c):
    return c["B"] * -(-c["h"] // TILE) * -(-c["w"] // TILE)


# --------------------------------------------------------------------------------------------------- filter gradient
def wgrad_channel_tiles(c):
    tc, tn = (64, 16) if wgrad_form(c["cin"], c["cout"]) == 0 else (16, 64)
    return -(-c["cin"] // tc) * -(-c["cout"] // tn)


def wgrad_steps(c):
    return c["B"] * -(-c["h"] // STEP_H) * -(-c["w"] // STEP_W)


def wgrad_slabs(c):
    """(n_slabs, steps per slab) by the rule in this module's docstring"""
    T = wgrad_steps(c)
    s = max(1, min(-(-512 // wgrad_channel_tiles(c)), -(-T // 2), 1024))
    per = -(-T // s)
    return -(-T // per), per


GPAIR = (3, 9, 9)           # 3 x 2 steps per image, 18 in all: nine slabs of two steps where the channel tiles are few
WGRAD_DENSE = [_row("wgrad", s, g) for s in SHAPES for g in (G355, GPAIR)]
WGRAD_DENSE += [_row("wgrad", s, g) for s in [(24, 12), (12, 444)] for g in [G1, GROW, GCOL] + EDGE_GRIDS + STEP_GRIDS]
WGRAD_DENSE += [_row("wgrad", (4, 4), GWT)]          # 2048 steps in 512 slabs
PAIR_CLASSES = [(1, 3), (3, 1), (2, 2)]          # (dy class, x class): x0d0 x1d0 x2d0 | x0d0 x0d1 x0d2 | x0d0 x1d0 x0d1 x1d1
PAIR_SHAPES = [(24, 12), (12, 444), (64, 64)]          # both filter-gradient forms; four waves along CIN and along COUT
WGRAD_PAIRS = [_row("wgrad", s, GPAIR, set="dy%d_x%d" % p) for s in PAIR_SHAPES for p in PAIR_CLASSES]
ALL_WGRAD = WGRAD_DENSE + WGRAD_PAIRS
SPARSE_K = 16          # 16 * 1023 * 1023 < 2^24 (class 2 x class 2); 16 * 3 * 2^18 < 2^24


def wgrad_pixels(c, co):
    """(b, h, w) where a sparse dy[.., co] is non-zero: three corners of the first image (their taps reach the padding), the last
    pixel of the batch, both sides of the first step boundary along w (7, 8) and along h (3, 4), and one pixel in each of the eight
    4-pixel blocks of the first step of the SECOND image (a lane reads the step's pixels 4 g + q and 16 + 4 g + q, pixel = 8 row +
    column; the place inside the block moves with co)."""
    B, H, W = c["B"], c["h"], c["w"]
    assert B >= 2 and H > STEP_H and W > STEP_W
    px = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, W - 1), (B - 1, H - 1, W - 1), (0, 1, STEP_W - 1), (0, 1, STEP_W), (0, STEP_H - 1, 2),
          (0, STEP_H, 2)]
    px += [(1, g >> 1, 4 * (g & 1) + (co + 3 * g) % 4) for g in range(8)]
    assert len(set(px)) == len(px) == SPARSE_K
    return px


def _sparse_dy(c, cls, seed):
    vals = gen_by_class(cls, (c["cout"], SPARSE_K), seed)
    if cls == 1:
        vals = torch.where(vals == 0, torch.ones_like(vals), vals)
    dy = torch.zeros(c["B"], c["h"], c["w"], c["cout"], dtype=I64)
    for co in range(c["cout"]):
        for j, (b, h, w) in enumerate(wgrad_pixels(c, co)):
            dy[b, h, w, co] = vals[co, j]
    return dy


def wgrad_operands(c, seed=0):
    """(x [B, h, w, cin], dy [B, h, w, cout]) as int64.  dense: x in [0, ax], dy in [-ad, ad] with M * ax * ad < 2^24."""
    xs, ds = (c["B"], c["h"], c["w"], c["cin"]), (c["B"], c["h"], c["w"], c["cout"])
    if c["set"] == "dense":
        ax, ad = (255, 15) if rows_of(c) <= 243 else (15, 7)
        g = _gen(400 + seed)
        return torch.randint(0, ax + 1, xs, generator=g, dtype=I64), torch.randint(-ad, ad + 1, ds, generator=g, dtype=I64)
    a, b = int(c["set"][2]), int(c["set"][5])
    return gen_by_class(b, xs, 600 + seed), _sparse_dy(c, a, 500 + seed)


def wgrad_reference(c, x, dy):
    """dW [cout, 3, 3, cin] as int64"""
    return wgrad_i64(x, dy, 3, 1, 1)


for _cs in (G_CASES, ALL_WGRAD):
    assert len({c["id"] for c in _cs}) == len(_cs), "case ids must be unique"
