"""Exact-integer operand sets and the case table for the 5x5 / stride 1 / padding 0 convolutions with a bias of
csrc/k5conv_kernels.hip and csrc/k5_fwd_body.h (alignq_k5conv_fwd / _dgrad / _wgrad, include/alignq_k5conv.h), in both forms (body:
channel counts that are multiples of 4; image: CIN = 3 folded with the taps).  tests/test_k5conv_oracle_cpu.py proves every condition
on the CPU, tests/test_gpu_k5conv_exact.py runs the kernels.

The method is tests/conv_exact_oracle.py's: integer operands, sum of |products| below 2^24 per output element, so the kernel must
return fp32(int64 sum) / fp32(n) with one IEEE division, then + bias[co] as one fp32 add (forward, where a bias is given; the data
gradient has none), or fp32(int64 sum) (filter gradient), bit for bit, whatever the tile, the tap, chunk, term or k-step order or the
slab.  The bias reference is the CPU's fp32 add of the fp32 quotient and the fp32 bias.  The references (conv_i64, dgrad_i64,
wgrad_i64 at ks = 5, stride 1, pad 0), the budget assertion, the bf16 term classes and the generators come from that module, the
quotient from tests/qgemm_exact_oracle.py, the sparse dy of the pair rows from tests/k3conv_exact_oracle.py.

The launchers' arithmetic, restated (the CPU test asserts it through alignq_k5conv_form and alignq_k5conv_wgrad_ws_bytes, the GPU test
through n_slabs_out too):
  forward / data gradient: N = COUT / CIN output columns, tiles of 8 x 8 OUTPUT pixels of one image (y: (H - 4) x (W - 4); dx: H x W)
      x BN channels, BN the widest of 64, 32, 16 with ceil(N / BN) BN == ceil(N / 16) 16 (form 2, 1, 0), in both forms; at most 2048
      spatial tiles in the grid, the rest by grid stride; body form: K = CIN / COUT in 32-deep chunks, the tail zero, 25 taps per
      chunk; image form: one K of 75 zero-tailed to 96;
  filter gradient: CIN == 3: 64 output channels x the 75 folded k per workgroup (form 2); else a (CIN x COUT) tile of 64 x 16
      channels where CIN >= COUT (form 0), else 16 x 64 (form 1); a step is a 4 x 8 tile of OUTPUT pixels of one image:
      T = B ceil((H - 4) / 4) ceil((W - 4) / 8) steps; with C channel tiles s = max(1, min(ceil(512 / C), ceil(T / 2), 1024)),
      per = ceil(T / s) steps per slab, n_slabs = ceil(T / per): no slab is empty.

A row's (B, h, w) is the grid the operation TILES: y for the forward and the filter gradient (the input is (h + 4) x (w + 4)), dx for
the data gradient (dy is (h - 4) x (w - 4)); H, W are the input's sizes, the arguments of the entry points.  Tensors are NHWC, filters
[Cout, 5, 5, Cin], int64 on the CPU.  Nothing of the package is imported."""
import torch

from tests.conv_exact_oracle import (I64, TWO24, _gen, assert_exact_budget, class_fractions, conv_i64, dgrad_i64,  # noqa: F401
                                     gen_by_class, gen_class3, sparse_bins, wgrad_i64)
from tests.k3conv_exact_oracle import SPARSE_K, _sparse_dy, wgrad_pixels  # noqa: F401
from tests.qgemm_exact_oracle import quotient  # noqa: F401

K5_FWD, K5_DGRAD, K5_WGRAD = 0, 1, 2
KS, NT = 5, 25
TILE = 8                    # the forward / data-gradient tile is TILE x TILE output pixels
GRID_TILES = 2048           # spatial tiles the grid holds
STEP_H, STEP_W = 4, 8       # the filter-gradient step is a STEP_H x STEP_W tile of output pixels
N16, N32, N64 = 0, 1, 2
W64X16, W16X64, WIMAGE = 0, 1, 2
FORMS = {K5_FWD: {N16, N32, N64}, K5_DGRAD: {N16, N32, N64}, K5_WGRAD: {W64X16, W16X64, WIMAGE}}      # what alignq_k5conv_form returns
OPS = {"fwd": K5_FWD, "dgrad": K5_DGRAD, "wgrad": K5_WGRAD}


def gemm_form(n):
    r16 = -(-n // 16) * 16
    return N64 if -(-n // 64) * 64 == r16 else (N32 if -(-n // 32) * 32 == r16 else N16)


def wgrad_form(cin, cout):
    return WIMAGE if cin == 3 else (W64X16 if cin >= cout else W16X64)


# (CIN, COUT) of the body form: one chunk's quarter (4); the forward's 32-wide tile (12, 24) and the data gradient's (24, 12); two
# 32-deep chunks with a tail each way and three 16-wide CIN tiles, the last of 4, in the filter gradient (36, 48) / (48, 36); four
# full 16-wide blocks (64, 64); two 64-wide channel tiles in the forward / data gradient and two workgroup tiles each way in the filter
# gradient (8, 128) / (128, 8); the limits (512, 4) / (4, 512)
SHAPES = [(4, 4), (12, 24), (24, 12), (36, 48), (48, 36), (64, 64), (8, 128), (128, 8), (512, 4), (4, 512)]
# COUT of the image form: 20 = an N tail whose filter tile is 4 rows of 75 halfwords; 68 = five 16-wide forward tiles and two
# filter-gradient tiles, the second with 4 live channels; 128 = two 64-wide tiles
IMAGE_COUT = [4, 20, 32, 64, 68, 128]
IMAGE_SHAPES = [(3, co) for co in IMAGE_COUT]
# (B, h, w) on the tiled grid: 3 x 5 x 5 (B > 1: a footprint that reads into the neighbouring image or row shows in the values); one
# pixel, one row, one column; tile - 1, tile, tile + 1 each way for the 8 x 8 tile and for the 4 x 8 step; five steps in three slabs of
# 2, 2 and 1
G1, GROW, GCOL, G355 = (1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 5, 5)
EDGE_GRIDS = [(1, 7, 9), (1, 8, 8), (1, 9, 7)]
STEP_GRIDS = [(1, 3, 9), (1, 4, 8), (1, 5, 7)]
GSLAB = (5, 4, 8)
# the data gradient's smallest tiled grid is 5 x 5 (dy is one pixel); dy of one row and of one column
D1, DROW, DCOL = (1, 5, 5), (2, 5, 9), (2, 9, 5)
GBIG = (33, 64, 64)         # 33 x 64 = 2112 tiles: beyond one pass of the grid cap (2.1 MiB at 4 channels: write-through, too)
GWT = (16, 64, 64)          # 1 MiB at 4 channels: the first size of the write-through window, one pass of the grid
GPAIR = (3, 9, 9)           # 3 x 2 steps per image, 18 in all: nine slabs of two steps where the channel tiles are few
GBITS = (2, 6, 7)           # the w_bit rows
FWD_EDGE_SHAPES = [(36, 48), (12, 24), (64, 64), (3, 20), (3, 68)]          # N16, N32, N64; image: N32 with a tail, N16 in five tiles
DGRAD_EDGE_SHAPES = [(36, 48), (24, 12), (64, 64)]                         # N16, N32, N64
WGRAD_EDGE_SHAPES = [(24, 12), (12, 24), (3, 20), (3, 68)]                 # W64X16, W16X64, WIMAGE in one and in two tiles
ACT3_SHAPES = [(12, 24), (36, 48), (48, 36), (64, 64)]
ACT3_IMAGE = [(3, 20), (3, 64)]


def _row(op, shape, grid, **kw):
    cin, cout = shape
    B, h, w = grid
    c = dict(op=op, cin=cin, cout=cout, B=B, h=h, w=w, set="dense", w_bit=8)
    c.update(kw)
    c["H"], c["W"] = (h, w) if op == "dgrad" else (h + KS - 1, w + KS - 1)
    c["form"] = {"fwd": gemm_form(cout), "dgrad": gemm_form(cin), "wgrad": wgrad_form(cin, cout)}[op]
    return c


def _finish(rows, bits):
    """ids; rows that do not fix their w_bit alternate 4 and 8 (the filter gradient does not divide: no w_bit)"""
    for i, c in enumerate(rows):
        if bits and not c.pop("fixed_bit", False):
            c["w_bit"] = (4, 8)[i & 1]
        c["id"] = "%s_%dx%d_B%dH%dW%d_%s" % (c["op"], c["cin"], c["cout"], c["B"], c["h"], c["w"], c["set"])
        if bits:
            c["id"] += "_k%d" % c["w_bit"]
    return rows


def _fwd_rows():
    op = "fwd"
    rows = [_row(op, s, G355) for s in SHAPES + IMAGE_SHAPES]
    rows += [_row(op, s, g) for s in FWD_EDGE_SHAPES for g in [G1, GROW, GCOL] + EDGE_GRIDS]
    # beyond the grid cap and the write-through window; the image form's grid stride fetches the next tile's patch ahead
    rows += [_row(op, s, g) for s in [(4, 4), (3, 4)] for g in (GBIG, GWT)]
    rows += [_row(op, s, G355, set="act3") for s in ACT3_SHAPES + ACT3_IMAGE]
    rows += [_row(op, (36, 48), EDGE_GRIDS[2], set="act3", w_bit=4, fixed_bit=True)]
    rows += [_row(op, s, GBITS, w_bit=k, fixed_bit=True) for s in [(36, 48), (3, 20)] for k in (1, 2, 4, 8)]
    return _finish(rows, True)


def _dgrad_rows():
    op = "dgrad"
    rows = [_row(op, s, G355) for s in SHAPES]
    rows += [_row(op, s, g) for s in DGRAD_EDGE_SHAPES for g in [D1, DROW, DCOL] + EDGE_GRIDS]
    rows += [_row(op, (4, 4), GBIG), _row(op, (4, 4), GWT)]
    # at 3 x 5 x 5 dy is one pixel and every dx pixel meets one tap; at 3 x 9 x 9 the centre pixel meets all 25
    rows += [_row(op, s, g, set="act3") for s in ACT3_SHAPES for g in (G355, GPAIR)]
    rows += [_row(op, (36, 48), EDGE_GRIDS[2], set="act3", w_bit=4, fixed_bit=True)]
    rows += [_row(op, (36, 48), GBITS, w_bit=k, fixed_bit=True) for k in (1, 2, 4, 8)]
    return _finish(rows, True)


FWD, DGRAD = _fwd_rows(), _dgrad_rows()
G_CASES = FWD + DGRAD
ACT3_NNZ, ACT3_AMP = 2, 1          # 2^18 * 25 * 2 * 1 < 2^24


def is_image(c):
    return c["cin"] == 3


def rows_of(c):
    """pixels of the tiled grid"""
    return c["B"] * c["h"] * c["w"]


def nlev_of(c):
    return float((1 << c["w_bit"]) - 1)


def contraction(c):
    """K, the contracted channel count"""
    return c["cin"] if c["op"] == "fwd" else c["cout"]


def g_amps(c):
    """(largest |activation|, largest |bin|) of a dense case: the bins shrink as K grows so that 25 K 255 amp < 2^24"""
    return 255, max(1, min(int(nlev_of(c)), (TWO24 - 1) // (NT * contraction(c) * 255)))


def g_operands(c, seed=0):
    """(activation, bins [cout, 5, 5, cin]) as int64: x [B, H, W, cin] for a forward, dy [B, H - 4, W - 4, cout] for a data gradient"""
    fwd = c["op"] == "fwd"
    shape = (c["B"], c["H"], c["W"], c["cin"]) if fwd else (c["B"], c["H"] - KS + 1, c["W"] - KS + 1, c["cout"])
    if c["set"] == "act3":
        return gen_class3(shape, 100 + seed), sparse_bins(c["cout"], KS, c["cin"], ACT3_NNZ, ACT3_AMP, "ci" if fwd else "co", 200 + seed)
    act, amp = g_amps(c)
    g = _gen(300 + seed)
    a = torch.randint(0 if fwd else -act, act + 1, shape, generator=g, dtype=I64)
    return a, torch.randint(-amp, amp + 1, (c["cout"], KS, KS, c["cin"]), generator=g, dtype=I64)


def g_reference(c, a, b):
    """the integer sums: y [B, H - 4, W - 4, cout] or dx [B, H, W, cin]"""
    return conv_i64(a, b, 1, 0) if c["op"] == "fwd" else dgrad_i64(a, b, 1, 0, c["H"], c["W"])


def g_budget(c, a, b):
    if c["op"] == "fwd":
        return assert_exact_budget(conv_i64, a, b, stride=1, pad=0)
    return assert_exact_budget(dgrad_i64, a, b, stride=1, pad=0, h_in=c["H"], w_in=c["W"])


def grid_tiles(c):
    return c["B"] * -(-c["h"] // TILE) * -(-c["w"] // TILE)


def bias_of(cout, seed=0):
    """fp32 [cout]: distinct, not integer-valued, magnitudes log-uniform in [1e-3, 1e3], both signs.  A bias added before the
    division, read at another channel or skipped on an N tail changes bits."""
    g = _gen(700 + seed)
    mag = torch.pow(torch.tensor(10.0, dtype=torch.float64), torch.rand(cout, generator=g, dtype=torch.float64) * 6.0 - 3.0)
    sign = (torch.arange(cout) % 2 * 2 - 1).to(torch.float64)
    return (mag * sign).to(torch.float32)


def with_bias(q, bias):
    """the epilogue's second step: ONE fp32 add of bias[co] to the fp32 quotient [.., cout] (on the CPU)"""
    assert q.dtype == torch.float32 and bias.dtype == torch.float32
    return q + bias


# --------------------------------------------------------------------------------------------------- filter gradient
def wgrad_channel_tiles(c):
    if is_image(c):
        return -(-c["cout"] // 64)
    tc, tn = (64, 16) if wgrad_form(c["cin"], c["cout"]) == W64X16 else (16, 64)
    return -(-c["cin"] // tc) * -(-c["cout"] // tn)


def wgrad_steps(c):
    return c["B"] * -(-c["h"] // STEP_H) * -(-c["w"] // STEP_W)


def wgrad_slabs(c):
    """(n_slabs, steps per slab) by the rule in this module's docstring"""
    T = wgrad_steps(c)
    s = max(1, min(-(-512 // wgrad_channel_tiles(c)), -(-T // 2), 1024))
    per = -(-T // s)
    return -(-T // per), per


WGRAD_DENSE = [_row("wgrad", s, g) for s in SHAPES + IMAGE_SHAPES for g in (G355, GPAIR)]
WGRAD_DENSE += [_row("wgrad", s, g) for s in WGRAD_EDGE_SHAPES for g in [G1, GROW, GCOL] + EDGE_GRIDS + STEP_GRIDS + [GSLAB]]
WGRAD_DENSE += [_row("wgrad", (4, 4), GWT), _row("wgrad", (3, 4), GWT)]          # 2048 steps in 512 slabs
PAIR_CLASSES = [(1, 3), (3, 1), (2, 2)]          # (dy class, x class): x0d0 x1d0 x2d0 | x0d0 x0d1 x0d2 | x0d0 x1d0 x0d1 x1d1
PAIR_SHAPES = [(24, 12), (12, 132), (64, 64), (3, 32), (3, 68)]          # the three forms; 132 = two 64-wide tiles and one of 4
WGRAD_PAIRS = [_row("wgrad", s, GPAIR, set="dy%d_x%d" % p) for s in PAIR_SHAPES for p in PAIR_CLASSES]
ALL_WGRAD = _finish(WGRAD_DENSE + WGRAD_PAIRS, False)
# SPARSE_K = 16 pixels per output channel (tests/k3conv_exact_oracle.py: wgrad_pixels, on the OUTPUT grid here):
# 16 * 1023 * 1023 < 2^24 (class 2 x class 2); 16 * 3 * 2^18 < 2^24


def wgrad_operands(c, seed=0):
    """(x [B, H, W, cin], dy [B, h, w, cout]) as int64.  dense: x in [0, ax], dy in [-ad, ad] with pixels * ax * ad < 2^24."""
    xs, ds = (c["B"], c["H"], c["W"], c["cin"]), (c["B"], c["h"], c["w"], c["cout"])
    if c["set"] == "dense":
        ax, ad = (255, 15) if rows_of(c) <= 243 else (15, 7)
        g = _gen(400 + seed)
        return torch.randint(0, ax + 1, xs, generator=g, dtype=I64), torch.randint(-ad, ad + 1, ds, generator=g, dtype=I64)
    a, b = int(c["set"][2]), int(c["set"][5])
    return gen_by_class(b, xs, 600 + seed), _sparse_dy(c, a, 500 + seed)


def wgrad_reference(c, x, dy):
    """dW [cout, 5, 5, cin] as int64"""
    return wgrad_i64(x, dy, KS, 1, 0)


for _cs in (G_CASES, ALL_WGRAD):
    assert len({c["id"] for c in _cs}) == len(_cs), "case ids must be unique"
