"""Exact-integer operand sets and the case table for the pointwise convolutions of csrc/pointwise_kernels.hip (alignq_pwconv_fwd /
_dgrad / _wgrad, include/alignq_pointwise.h).  tests/test_pointwise_oracle_cpu.py proves every condition on the CPU,
tests/test_gpu_pointwise_exact.py runs the kernels.

The method is tests/conv_exact_oracle.py's: integer operands, sum of |products| below 2^24 per output element, so the kernel must
return fp32(int64 sum) / fp32(n) (forward, data gradient: one IEEE division) or fp32(int64 sum) (filter gradient), bit for bit,
whatever the tile, the k order, the term order or the slab.  The references (conv_i64, dgrad_i64, wgrad_i64 at ks = 1, stride 1,
pad 0), the budget assertion, the bf16 term classes and the generators come from that module, the quotient from
tests/qgemm_exact_oracle.py.

The launchers' arithmetic, restated (the GPU test asserts it through alignq_pwconv_form, alignq_pwconv_wgrad_ws_bytes and n_slabs_out):
  forward / data gradient: N = COUT / CIN output columns, tiles of 64 pixels x BN channels, BN the widest of 64, 32, 16 with
      ceil(N / BN) BN == ceil(N / 16) 16 (form 2, 1, 0); at most 2048 row tiles in the grid, the rest by grid stride; K = CIN / COUT in
      64-deep steps of two 32-deep halves, the tail zero;
  filter gradient: a (CIN x COUT) tile of 32 (C <= 32) or 64 channels each way: form = (CIN > 32) + 2 (COUT > 32); tiles = ceil(CIN / tile)
      ceil(COUT / tile); n_slabs = min(ceil(512 / tiles), ceil(M / 64), 1024), at least 1; per = ceil(ceil(M / n_slabs) / 32) 32 pixels
      per slab, the last slabs empty (all zero) where n_slabs per > M + per.

Tensors are NHWC, filters [Cout, 1, 1, Cin], int64 on the CPU.  Nothing of the package is imported."""
import torch

from tests.conv_exact_oracle import (I64, TWO24, _gen, assert_exact_budget, bf16_terms, class_fractions, conv_i64, dgrad_i64,  # noqa: F401
                                     gen_by_class, gen_class1, gen_class2, gen_class3, sparse_bins, wgrad_i64)
from tests.qgemm_exact_oracle import quotient  # noqa: F401

PW_FWD, PW_DGRAD, PW_WGRAD = 0, 1, 2
TILE_ROWS = 64              # pixels per forward / data-gradient tile
GRID_ROW_TILES = 2048       # row tiles the grid holds
STEP = 32                   # pixels per filter-gradient step
FORMS = {PW_FWD: {0, 1, 2}, PW_DGRAD: {0, 1, 2}, PW_WGRAD: {0, 1, 2, 3}}          # every value alignq_pwconv_form returns

# (CIN, COUT) -> (forward form, data-gradient form, filter-gradient form), the smallest shapes that reach each edge:
SHAPES = {
    (8, 8): (0, 0, 0),            # K = 8: a quarter of one half step; N = 8: half a 16-wide tile
    (16, 96): (1, 0, 2),          # MobileNet's first expansion: N = 96 = 3 x 32
    (96, 24): (1, 1, 1),          # K = 96 = 64 + 32: the second step's second half is skipped; N = 24 = 16 + 8
    (24, 144): (0, 1, 2),         # N = 144 = 9 x 16
    (144, 32): (1, 0, 1),         # K = 144 = 2 x 64 + 16
    (40, 200): (0, 0, 3),         # K = 40: 8 into the second half; N = 200 = 12 x 16 + 8; data gradient N = 40 = 2 x 16 + 8
    (160, 320): (2, 1, 3),        # N = 320 = 5 x 64; data gradient N = 160 = 5 x 32
    (2048, 8): (0, 2, 1),         # the longest contraction (32 steps); data gradient N = 2048 = 32 x 64
    (8, 2048): (2, 0, 2),
}
# (B, h, w): M = 1; 75 (smaller than a tile, odd); 63 / 64 / 65 around one tile's rows; 189 (three filter-gradient slabs); one M
# beyond a single pass of the grid cap: 2048 x 64 = 131072 row tiles' rows + one full tile + 7 (at 8 channels: 4 MiB each way, which
# is also inside the write-through window of 1 MiB to 64 MiB; every other case here stores plainly)
M1, M75, M63, M64, M65, M189, MBIG = (1, 1, 1), (3, 5, 5), (1, 7, 9), (1, 8, 8), (1, 5, 13), (3, 7, 9), (1, 1, 131143)
EDGE_SHAPES = [(8, 8), (96, 24), (160, 320)]          # one per forward form


def rows_of(c):
    return c["B"] * c["h"] * c["w"]


def _row(op, shape, grid, **kw):
    cin, cout = shape
    B, h, w = grid
    c = dict(op=op, cin=cin, cout=cout, B=B, h=h, w=w, set="dense", w_bit=8)
    c.update(kw)
    f = SHAPES[shape]
    c["form"] = f[{"fwd": 0, "dgrad": 1, "wgrad": 2}[op]]
    c["id"] = "%s_%dx%d_M%d_%s" % (op, cin, cout, B * h * w, c["set"])
    return c


def _g_rows(op):
    rows = [_row(op, s, M75) for s in SHAPES]
    rows += [_row(op, s, g) for s in EDGE_SHAPES for g in (M1, M63, M64, M65)]
    rows += [_row(op, (8, 8), MBIG)]
    rows += [_row(op, s, M75, set="act3") for s in [(16, 96), (96, 24), (144, 32), (40, 200), (160, 320)]]
    rows += [_row(op, (8, 8), M65, set="act3")]
    return rows


FWD, DGRAD = _g_rows("fwd"), _g_rows("dgrad")
G_CASES = FWD + DGRAD
ACT3_NNZ, ACT3_AMP = 8, 3          # 2^18 * 8 * 3 < 2^24


def nlev_of(c):
    return float((1 << c["w_bit"]) - 1)


def contraction(c):
    return c["cin"] if c["op"] == "fwd" else c["cout"]


def g_amps(c):
    """(largest |activation|, largest |bin|) of a dense case: the bins shrink as K grows so that K * 255 * bin < 2^24"""
    return 255, max(1, min(255, (TWO24 - 1) // (contraction(c) * 255)))


def g_operands(c, seed=0):
    """(activation, bins [cout, 1, 1, cin]) as int64: x [B, h, w, cin] for a forward, dy [B, h, w, cout] for a data gradient"""
    shape = (c["B"], c["h"], c["w"], c["cin"] if c["op"] == "fwd" else c["cout"])
    if c["set"] == "act3":
        nnz = min(ACT3_NNZ, contraction(c))
        return gen_class3(shape, 100 + seed), sparse_bins(c["cout"], 1, c["cin"], nnz, ACT3_AMP, "ci" if c["op"] == "fwd" else "co", 200 + seed)
    act, amp = g_amps(c)
    g = _gen(300 + seed)
    a = torch.randint(0 if c["op"] == "fwd" else -act, act + 1, shape, generator=g, dtype=I64)
    return a, torch.randint(-amp, amp + 1, (c["cout"], 1, 1, c["cin"]), generator=g, dtype=I64)


def g_reference(c, a, b):
    """the integer sums: y [B, h, w, cout] or dx [B, h, w, cin]"""
    return conv_i64(a, b, 1, 0) if c["op"] == "fwd" else dgrad_i64(a, b, 1, 0, c["h"], c["w"])


def g_budget(c, a, b):
    if c["op"] == "fwd":
        return assert_exact_budget(conv_i64, a, b, stride=1, pad=0)
    return assert_exact_budget(dgrad_i64, a, b, stride=1, pad=0, h_in=c["h"], w_in=c["w"])


# --------------------------------------------------------------------------------------------------- filter gradient
def wgrad_tiles(c):
    tc, tn = (32 if c["cin"] <= 32 else 64), (32 if c["cout"] <= 32 else 64)
    return -(-c["cin"] // tc) * -(-c["cout"] // tn)


def wgrad_slabs(c):
    """(n_slabs, pixels per slab) by the rule in this module's docstring"""
    M = rows_of(c)
    s = max(1, min(-(-512 // wgrad_tiles(c)), -(-M // 64), 1024))
    return s, -(-(-(-M // s)) // STEP) * STEP


WGRAD_DENSE = [_row("wgrad", s, g) for s in SHAPES for g in (M75, M189)]
WGRAD_DENSE += [_row("wgrad", s, g) for s in [(8, 8), (40, 200)] for g in (M1, M63, M64, M65)]
WGRAD_DENSE += [_row("wgrad", (8, 8), MBIG)]
PAIR_CLASSES = [(1, 3), (3, 1), (2, 2)]          # (dy class, x class): x0d0 x1d0 x2d0 | x0d0 x0d1 x0d2 | x0d0 x1d0 x0d1 x1d1
PAIR_SHAPES = [(8, 8), (16, 96), (96, 24), (40, 200)]          # one per filter-gradient form
WGRAD_PAIRS = [_row("wgrad", s, M189, set="dy%d_x%d" % p) for s in PAIR_SHAPES for p in PAIR_CLASSES]
ALL_WGRAD = WGRAD_DENSE + WGRAD_PAIRS
SPARSE_K = 16          # 16 * 1023 * 1023 < 2^24 (class 2 x class 2); 16 * 3 * 2^18 < 2^24


def wgrad_pixels(c, co):
    """Flat pixel indices where a sparse dy[.., co] is non-zero: the first and the last pixel, both sides of the first step boundary
    (31, 32) and of the first slab boundary (per - 1, per), one pixel in each of the eight 4-pixel row blocks of the 32-pixel step
    that begins the second slab (a lane reads rows 4 g + q and 16 + 4 g + q; the place inside the block moves with co), and two pixels
    that depend on co."""
    M, per = rows_of(c), wgrad_slabs(c)[1]
    assert per + STEP <= M
    px = [0, M - 1, STEP - 1, STEP, per - 1, per]
    px += [per + 4 * g + (co + 3 * g) % 4 for g in range(8)]
    px += [(co * 997 + 131 * j + 29) % M for j in range(2)]
    out = sorted(set(px))
    assert len(out) <= SPARSE_K and out[-1] < M
    return out


def _sparse_dy(c, cls, seed):
    vals = gen_by_class(cls, (c["cout"], SPARSE_K), seed)
    if cls == 1:
        vals = torch.where(vals == 0, torch.ones_like(vals), vals)
    dy = torch.zeros(rows_of(c), c["cout"], dtype=I64)
    for co in range(c["cout"]):
        px = wgrad_pixels(c, co)
        dy[px, co] = vals[co, :len(px)]
    return dy.reshape(c["B"], c["h"], c["w"], c["cout"])


def wgrad_operands(c, seed=0):
    """(x [B, h, w, cin], dy [B, h, w, cout]) as int64.  dense: x in [0, ax], dy in [-ad, ad] with M * ax * ad < 2^24."""
    xs, ds = (c["B"], c["h"], c["w"], c["cin"]), (c["B"], c["h"], c["w"], c["cout"])
    if c["set"] == "dense":
        ax, ad = (255, 15) if rows_of(c) <= 189 else (15, 7)
        g = _gen(400 + seed)
        return torch.randint(0, ax + 1, xs, generator=g, dtype=I64), torch.randint(-ad, ad + 1, ds, generator=g, dtype=I64)
    a, b = int(c["set"][2]), int(c["set"][5])
    return gen_by_class(b, xs, 600 + seed), _sparse_dy(c, a, 500 + seed)


def wgrad_reference(c, x, dy):
    """dW [cout, 1, 1, cin] as int64"""
    return wgrad_i64(x, dy, 1, 1, 0)


for _cs in (G_CASES, ALL_WGRAD):
    assert len({c["id"] for c in _cs}) == len(_cs), "case ids must be unique"
