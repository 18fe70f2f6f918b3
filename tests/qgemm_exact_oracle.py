"""Exact-integer references, operand sets and the case table for the convolutions of csrc/qgemm_kernels.hip (alignq_qconv_fwd /
_dgrad / _wgrad / _stem7_fwd / _stem7_wgrad).  tests/test_qgemm_exact_oracle_cpu.py proves every condition on the CPU,
tests/test_gpu_qgemm_exact.py runs the kernels.

The method is tests/conv_exact_oracle.py's: integer operands, sum of |products| below 2^24 per output element, so the kernel must
return fp32(int64 sum) / fp32(den), one IEEE division, bit for bit, whatever the tile, the k order, the term order or the split.
The generic references (conv_i64, dgrad_i64, wgrad_i64), the budget assertion, the bf16 term classes and the generators come from
that module; this one adds the stem's 7x7 pair, a float64 form for the large cases, the quotient, the pixel chooser for this
file's filter-gradient geometry and ONE ROW PER LAUNCH FORM.

The comment next to a row is the launchers' arithmetic for it (pick_tile / pick_tile_conv / pick_ksplit / wgrad_geometry /
wgrad_splits of csrc/qgemm_kernels.hip, constants kWantBlocks = 1024, halved to 512 for the halo forms; 256 * OCC workgroup slots;
at least two 32-pixel steps per filter-gradient split); `bm`, `split`, `splits` state its result and the GPU test asserts them
through alignq_qconv_bn_parts, alignq_qconv_dgrad_ws_bytes, alignq_qconv_wgrad_ws_bytes and n_slabs_out.

Tensors are NHWC, filters [Cout, KS, KS, Cin], int64 on the CPU.  Nothing of the package is imported."""
import torch

from tests.conv_exact_oracle import (I64, TWO24, _gen, assert_exact_budget, bf16_terms, class_fractions, conv_i64, dgrad_i64,  # noqa: F401
                                     gen_by_class, gen_class1, gen_class2, gen_class3, sparse_bins, term_counts, wgrad_i64)

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------------------ references
def stem7_fwd_i64(x, b):
    """y [B, Ho, Wo, 64] of the 7x7 stride-2 padding-3 stem: x [B, H, W, 3], b [64, 7, 7, 3]"""
    return conv_i64(x, b, 2, 3)


def stem7_wgrad_i64(x, dy):
    """dW as alignq_qconv_stem7_wgrad leaves it: 64 * 147 numbers in the filter's own layout [64][7][7][3]"""
    return wgrad_i64(x, dy, 7, 2, 3).reshape(64 * 147)


def conv_f64(x, b, stride, pad):
    """conv_i64 contracted in float64 (exact while every sum stays below 2^53): for the cases whose int64 matmul is too slow"""
    B, H, W, Cin = x.shape
    Cout, KS = b.shape[0], b.shape[1]
    Ho, Wo = (H + 2 * pad - KS) // stride + 1, (W + 2 * pad - KS) // stride + 1
    xp = torch.zeros(B, H + 2 * pad, W + 2 * pad, Cin, dtype=F64)
    xp[:, pad:pad + H, pad:pad + W] = x.to(F64)
    bd = b.to(F64)
    out = torch.zeros(B * Ho * Wo, Cout, dtype=F64)
    for ky in range(KS):
        for kx in range(KS):
            xs = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            out += xs.reshape(-1, Cin).matmul(bd[:, ky, kx].t())
    return out.reshape(B, Ho, Wo, Cout)


def dgrad_f64(dy, b, stride, pad, h_in, w_in):
    """dgrad_i64 contracted in float64"""
    B, Ho, Wo, Cout = dy.shape
    KS, Cin = b.shape[1], b.shape[3]
    buf = torch.zeros(B, h_in + 2 * pad + stride, w_in + 2 * pad + stride, Cin, dtype=F64)
    d, bd = dy.reshape(-1, Cout).to(F64), b.to(F64)
    for ky in range(KS):
        for kx in range(KS):
            c = d.matmul(bd[:, ky, kx]).reshape(B, Ho, Wo, Cin)
            buf[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] += c
    return buf[:, pad:pad + h_in, pad:pad + w_in].contiguous()


def quotient(total, nlev, xlev=0.0):
    """The kernels' epilogue: fp32(sum) / fp32(den), one fp32 division on the CPU.  den = nlev for an fp32 operand, the fp32
    product nlev * xlev for a level operand; a split-K closing pass divides the added raw sums by the same den once."""
    den = torch.tensor(float(nlev), dtype=F32)
    if xlev:
        den = den * torch.tensor(float(xlev), dtype=F32)
    return total.to(F32) / den


# ------------------------------------------------------------------------------------------------------------- geometry
def out_hw(c):
    return (c["h"] - 1) // c["stride"] + 1, (c["w"] - 1) // c["stride"] + 1


def pad_of(c):
    return (c["ks"] - 1) // 2


def _row(op, B, h, w, cin, cout, ks, stride, **kw):
    c = dict(op=op, B=B, h=h, w=w, cin=cin, cout=cout, ks=ks, stride=stride, mode="f32", set="dense", w_bit=8, big=False, groups=1)
    c.update(kw)
    c["id"] = "%s_%dx%d_k%ds%d_B%d_%dx%d_%s_%s%s" % (op, cin, cout, ks, stride, B, h, w, c["mode"], c["set"],
                                                    ("_g%d" % c["groups"]) if c["groups"] > 1 else "")
    return c


def nlev_of(c):
    return float((1 << c["w_bit"]) - 1)


XLEV_FWD = 255.0          # forward level operands: x = idx / 255 (rint(x * 255) == idx is proved on the CPU)
IDX_TOP = 2040            # the largest index a level tensor carries (8 x 255)

# ------------------------------------------------------------------------------- forward / data gradient (qgemm_kernel)
# mode: f32 = MODE 0 (three bf16 terms); lev = MODE 1 from the fp32 level tensor; idx = MODE 1 from int16 indices (XI).
# km: 0 = 1x1, 1 = 3x3 gathered per tap (stride 2, or W > 56), 2 = 3x3 stride-1 halo image (W <= 56), 3 = parity classes.
# rows = B * Ho * Wo (forward) or the data gradient's row grid; N = output columns; blocks(bm, bn) = ceil(rows / bm) * (N / bn).
FWD = [
    # 128x128: N % 128 == 0 and blocks(128, 128) = ceil(16383 / 128) * 8 = 128 * 8 = 1024 >= 1024.  The last row tile holds 127 rows.
    _row("fwd", 1, 127, 129, 64, 1024, 1, 1, km=0, bm=128, bn=128, big=True),
    _row("fwd", 1, 127, 129, 64, 1024, 1, 1, km=0, bm=128, bn=128, big=True, mode="idx"),
    # 64x128: blocks(128, 128) = 64 * 8 = 512 < 1024; blocks(64, 128) = ceil(8190 / 64) * 8 = 128 * 8 = 1024 (rows 8129 .. 16256)
    _row("fwd", 1, 91, 90, 64, 1024, 1, 1, km=0, bm=64, bn=128, big=True),
    # 128x64: N = 320 is no multiple of 128; blocks(128, 64) = ceil(52441 / 128) * 5 = 410 * 5 = 2050 >= 2 * 1024 (rows >= 52353)
    _row("fwd", 1, 229, 229, 64, 320, 1, 1, km=0, bm=128, bn=64, big=True),
    # 64x64: everything below: 70 rows = two row tiles, the second with 6 rows
    _row("fwd", 2, 5, 7, 64, 64, 1, 1, km=0, bm=64, bn=64),
    # 1x1 stride 2: rows = 3 * 4 * 5 = 60, the row's pixel is (2 hr, 2 wr) of a 7 x 9 image; two k chunks
    _row("fwd", 3, 7, 9, 128, 64, 1, 2, km=0, bm=64, bn=64),
    # KM 1: 3x3 stride 2 on 4x4 (rows 5 * 2 * 2 = 20: one tile spans five images) and 3x5 (rows 30; N = 128: blocks(64, 128) = 1 and
    # blocks(128, 64) = 2 are below their bars: 64x64, two column tiles)
    _row("fwd", 5, 4, 4, 64, 64, 3, 2, km=1, bm=64, bn=64),
    _row("fwd", 5, 3, 5, 64, 128, 3, 2, km=1, bm=64, bn=64),
    # KM 1 at stride 1: W = 57 is one past the halo form's 56; 171 rows = three tiles (first, middle, last with 43 rows)
    _row("fwd", 1, 3, 57, 64, 64, 3, 1, km=1, bm=64, bn=64),
    # KM 2 (halo): 4x4 images, 144 rows = 2.25 tiles of nine images; 3x5 images, 75 rows, four 32-channel chunks; the widest W = 56
    _row("fwd", 9, 4, 4, 64, 64, 3, 1, km=2, bm=64, bn=64),
    _row("fwd", 5, 3, 5, 128, 64, 3, 1, km=2, bm=64, bn=64),
    _row("fwd", 1, 3, 56, 64, 64, 3, 1, km=2, bm=64, bn=64),
    # halo forms take want = 512.  128x128: ceil(8120 / 128) * 8 = 64 * 8 = 512.
    _row("fwd", 1, 145, 56, 64, 1024, 3, 1, km=2, bm=128, bn=128, big=True),
    # the same shape with a level operand is held to 64-row tiles: blocks(64, 128) = 127 * 8 >= 512: 64x128
    _row("fwd", 1, 145, 56, 64, 1024, 3, 1, km=2, bm=64, bn=128, big=True, mode="idx"),
    # halo 64x128: blocks(128, 128) = 32 * 8 = 256 < 512, blocks(64, 128) = ceil(4088 / 64) * 8 = 64 * 8 = 512
    _row("fwd", 1, 73, 56, 64, 1024, 3, 1, km=2, bm=64, bn=128, big=True),
    # halo 128x64: N = 320, blocks(128, 64) = ceil(26152 / 128) * 5 = 205 * 5 = 1025 >= 2 * 512
    _row("fwd", 1, 467, 56, 64, 320, 3, 1, km=2, bm=128, bn=64, big=True),
    # MODE 1 in the three k-forms, from the fp32 level tensor and from int16 indices (64x64 tiles)
    _row("fwd", 2, 5, 7, 128, 64, 1, 1, km=0, bm=64, bn=64, mode="lev"),
    _row("fwd", 2, 5, 7, 128, 64, 1, 1, km=0, bm=64, bn=64, mode="idx"),
    _row("fwd", 5, 4, 4, 64, 64, 3, 2, km=1, bm=64, bn=64, mode="lev"),
    _row("fwd", 5, 4, 4, 64, 64, 3, 2, km=1, bm=64, bn=64, mode="idx"),
    _row("fwd", 9, 4, 4, 128, 64, 3, 1, km=2, bm=64, bn=64, mode="lev"),
    _row("fwd", 9, 4, 4, 128, 64, 3, 1, km=2, bm=64, bn=64, mode="idx"),
]
# class-3 activations (all three bf16 terms) against sparse bins, one per k-form
FWD += [_row("fwd", 2, 5, 7, 128, 64, 1, 1, km=0, bm=64, bn=64, set="act3"),
        _row("fwd", 5, 4, 4, 64, 64, 3, 2, km=1, bm=64, bn=64, set="act3"),
        _row("fwd", 1, 3, 57, 64, 64, 3, 1, km=1, bm=64, bn=64, set="act3"),
        _row("fwd", 9, 4, 4, 64, 64, 3, 1, km=2, bm=64, bn=64, set="act3"),
        _row("fwd", 5, 3, 5, 128, 64, 3, 1, km=2, bm=64, bn=64, set="act3")]

# Data gradient: rows = input pixels (dy's pixels for the stride-2 forms), N = CIN, contraction over COUT.  `split` is what
# pick_ksplit takes WITH the scratch: cost(S) = ceil(blocks * S / (256 * OCC)) * (ceil(units / S) + 2), S <= 4 while units / S >= 2,
# taken when cost(best) <= 0.75 * cost(1).  OCC = 4 for 64x64 (2 for the halo form), units = COUT / 64 (1x1), 9 * COUT / 64 (KM 1),
# COUT / 32 (KM 2), 2 * COUT / 64 (KM 3).  With few blocks the first factor is 1.
DGRAD = [
    _row("dgrad", 1, 127, 129, 1024, 64, 1, 1, km=0, bm=128, bn=128, split=1, big=True),      # tiles as the forward's; units = 1
    _row("dgrad", 1, 91, 90, 1024, 64, 1, 1, km=0, bm=64, bn=128, split=1, big=True),
    _row("dgrad", 1, 229, 229, 320, 64, 1, 1, km=0, bm=128, bn=64, split=1, big=True),
    _row("dgrad", 2, 5, 7, 64, 64, 1, 1, km=0, bm=64, bn=64, split=1),                         # units = 1
    # one block, units = 4 / 6 / 8: costs (S = 1..4) 6,4 | 8,5,4 | 10,6,5,4: split 2 / 3 / 4
    _row("dgrad", 1, 8, 8, 64, 256, 1, 1, km=0, bm=64, bn=64, split=2),
    _row("dgrad", 1, 8, 8, 64, 384, 1, 1, km=0, bm=64, bn=64, split=3),
    _row("dgrad", 1, 8, 8, 64, 512, 1, 1, km=0, bm=64, bn=64, split=4),
    # the scattering 1x1 stride 2 on odd x odd, odd x even and even grids (units = 2: no split), and one split (units = 4)
    _row("dgrad", 3, 7, 7, 64, 128, 1, 2, km=0, bm=64, bn=64, split=1, scatter=True),
    _row("dgrad", 3, 7, 8, 64, 128, 1, 2, km=0, bm=64, bn=64, split=1, scatter=True),
    _row("dgrad", 3, 8, 8, 64, 128, 1, 2, km=0, bm=64, bn=64, split=1, scatter=True),
    _row("dgrad", 5, 7, 7, 64, 256, 1, 2, km=0, bm=64, bn=64, split=2, scatter=True),          # rows 80: two tiles
    # KM 1 (W = 57): rows 114 = 2 blocks, units = 9: costs 11, 7, 5, 5: split 3 (k steps 0-2, 3-5, 6-8)
    _row("dgrad", 1, 2, 57, 64, 64, 3, 1, km=1, bm=64, bn=64, split=3),
    # KM 2: units = COUT / 32 = 2: no split; 4: split 2 (whole 32-channel chunks of nine taps); the widest image
    _row("dgrad", 9, 4, 4, 64, 64, 3, 1, km=2, bm=64, bn=64, split=1),
    _row("dgrad", 5, 3, 5, 64, 128, 3, 1, km=2, bm=64, bn=64, split=2),
    _row("dgrad", 1, 3, 56, 64, 64, 3, 1, km=2, bm=64, bn=64, split=1),
    # halo 128x128 (want 512): ceil(8120 / 128) * 8 = 512; dx is above the 32 MB limit of the scratch: no split
    _row("dgrad", 1, 145, 56, 1024, 64, 3, 1, km=2, bm=128, bn=128, split=1, big=True),
    # KM 3: class size B * Ho * Wo; 2x2 (every pixel is each class's last row and column), 4x6, 6x6 with 72 rows per class (two
    # tiles, the second with 8 rows).  units = 2 * COUT / 64 = 2: no split; 4: split 2 (a one-tap class runs one k step per split);
    # 8: split 4.  The guard "ksplit > COUT / 64 cancels the split" cannot fire: pick_ksplit only tries S with units / S >= 2,
    # units = 2 * COUT / 64, so S <= COUT / 64 always (NOTES.md).
    _row("dgrad", 3, 2, 2, 64, 64, 3, 2, km=3, bm=64, bn=64, split=1),
    _row("dgrad", 3, 4, 6, 64, 64, 3, 2, km=3, bm=64, bn=64, split=1),
    _row("dgrad", 8, 6, 6, 64, 64, 3, 2, km=3, bm=64, bn=64, split=1),
    _row("dgrad", 3, 4, 6, 64, 128, 3, 2, km=3, bm=64, bn=64, split=2),
    _row("dgrad", 8, 6, 6, 128, 256, 3, 2, km=3, bm=64, bn=64, split=4),
]
DGRAD += [_row("dgrad", 2, 5, 7, 128, 64, 1, 1, km=0, bm=64, bn=64, split=1, set="act3"),
          _row("dgrad", 1, 8, 8, 64, 512, 1, 1, km=0, bm=64, bn=64, split=4, set="act3"),
          _row("dgrad", 3, 7, 7, 64, 128, 1, 2, km=0, bm=64, bn=64, split=1, scatter=True, set="act3"),
          _row("dgrad", 1, 2, 57, 64, 64, 3, 1, km=1, bm=64, bn=64, split=3, set="act3"),
          _row("dgrad", 5, 3, 5, 64, 128, 3, 1, km=2, bm=64, bn=64, split=2, set="act3"),
          _row("dgrad", 3, 4, 6, 64, 128, 3, 2, km=3, bm=64, bn=64, split=2, set="act3")]

ACT3_NNZ, ACT3_AMP = {1: 8, 3: 2}, 3          # 2^18 * ks^2 * nnz * amp: 2^18 * 24 (1x1), 2^18 * 54 (3x3) < 2^24


def contraction(c):
    return c["ks"] ** 2 * (c["cin"] if c["op"] == "fwd" else c["cout"])


def g_amps(c):
    """(largest |activation|, largest |bin|) of a dense case: the activation range is the operand's own (255, or the index
    range 2040); the bins shrink as K grows so that K * act * bin < 2^24"""
    nlev = int(nlev_of(c))
    act = IDX_TOP if c["mode"] != "f32" else (255 if nlev > 1 else 3)
    return act, max(1, min(nlev, (TWO24 - 1) // (contraction(c) * act)))


def g_operands(c, seed=0):
    """(activation, bins) as int64: the activation is x [B, h, w, cin] for a forward, dy [B, ho, wo, cout] for a data gradient"""
    ho, wo = out_hw(c)
    shape = (c["B"], c["h"], c["w"], c["cin"]) if c["op"] == "fwd" else (c["B"], ho, wo, c["cout"])
    fshape = (c["cout"], c["ks"], c["ks"], c["cin"])
    if c["set"] == "act3":
        a = gen_class3(shape, 100 + seed)
        b = sparse_bins(c["cout"], c["ks"], c["cin"], ACT3_NNZ[c["ks"]], ACT3_AMP, "ci" if c["op"] == "fwd" else "co", 200 + seed)
        return a, b
    act, amp = g_amps(c)
    g = _gen(300 + seed)
    lo = 0 if c["op"] == "fwd" else -act          # a forward's activations are relu outputs / indices; dy has both signs
    assert c["mode"] == "f32" or c["op"] == "fwd"
    a = torch.randint(lo, act + 1, shape, generator=g, dtype=I64)
    b = torch.randint(-amp, amp + 1, fshape, generator=g, dtype=I64)
    return a, b


def g_budget_bound(c, a, b):
    """max|activation| * the largest sum of |bins| over a contraction: an upper bound of every output's sum of |products|"""
    sums = b.abs().sum(dim=(1, 2, 3)) if c["op"] == "fwd" else b.abs().sum(dim=(0, 1, 2))
    return int(a.abs().max()) * int(sums.max())


def g_reference(c, a, b):
    """the integer sums (int64, or float64 for the big cases) of case c: y [B, ho, wo, cout] or dx [B, h, w, cin]"""
    p = pad_of(c)
    if c["op"] == "fwd":
        return (conv_f64 if c["big"] else conv_i64)(a, b, c["stride"], p)
    return (dgrad_f64 if c["big"] else dgrad_i64)(a, b, c["stride"], p, c["h"], c["w"])


def g_expected(c, a, b):
    return quotient(g_reference(c, a, b), nlev_of(c), XLEV_FWD if c["mode"] != "f32" else 0.0)


# Batch-norm partials: w_bit = 1 (nlev = 1, bins in {-1, 0, 1}), activations in [0, 3]: |y| <= 3 K, y^2 <= 9 K^2 and a lane's sum of
# at most four of them are integers far below 2^24; bn_part[group][tile][channel] = {sum y, sum y^2} over the tile's own rows
# [tile * bm, min((tile + 1) * bm, Mg)) of its group.
BN = [
    _row("fwd", 4, 5, 7, 64, 64, 1, 1, km=0, bm=64, bn=64, w_bit=1, groups=2),          # Mg = 70: tiles of 64 and 6 rows per group
    _row("fwd", 6, 7, 9, 64, 128, 3, 2, km=1, bm=64, bn=64, w_bit=1, groups=3),         # Mg = 2 * 20 = 40: 24 rows of each tile are beyond its group
    _row("fwd", 10, 4, 4, 64, 64, 3, 1, km=2, bm=64, bn=64, w_bit=1, groups=2),         # halo: Mg = 80: a tile's halo reaches into the other group
    # 128x128: blocks(128, 128) = ceil(16380 / 128) * 8 = 1024; Mg = 8190: 64 tiles per group, the last with 126 rows
    _row("fwd", 2, 91, 90, 64, 1024, 1, 1, km=0, bm=128, bn=128, w_bit=1, groups=2, big=True),
]


def bn_expected(y_i64, groups, bm):
    """[groups][tiles][C][2] int64 {sum y, sum y^2} per row tile of each group; y_i64 [B, ho, wo, C]"""
    C = y_i64.shape[-1]
    yg = y_i64.reshape(groups, -1, C)
    Mg = yg.shape[1]
    tiles = (Mg + bm - 1) // bm
    pad = torch.zeros(groups, tiles * bm - Mg, C, dtype=y_i64.dtype)
    yt = torch.cat([yg, pad], 1).reshape(groups, tiles, bm, C)
    return torch.stack([yt.sum(2), (yt * yt).sum(2)], -1)


# --------------------------------------------------------------------------------------------------- filter gradient
# M = B * Ho * Wo dy pixels.  tc / tn = 4 where CIN / COUT is a multiple of 128, else 2 (tile 32 tc x 32 tn); tiles = (CIN / 32 tc) *
# (COUT / 32 tn) * KS^2; splits = min(ceil(want / tiles), ceil(M / 64)) with want = 512 (1x1) / 1024 (3x3) - at these sizes always
# the second; per = ceil(ceil(M / splits) / 32) * 32.  Every M is no multiple of 32 and per does not divide it.
# kernel "tap": qgemm_wgrad_kernel<TC, TN, TX, GATHER>; "ring": qgemm_wgrad3_kernel (3x3 stride 1, W <= 56; 64x64 tiles, tiles =
# (CIN / 64)(COUT / 64), want 512), ring of R = 2 W + 34 rows.
def _w(B, h, w, cin, cout, ks, stride, kernel, splits, per, **kw):
    return _row("wgrad", B, h, w, cin, cout, ks, stride, kernel=kernel, splits=splits, per=per, **kw)


WGRAD_SHAPES = [
    # not gathered (1x1 stride 1): M = 189, ceil(189 / 64) = 3 splits of 64, 64, 61 pixels; TC / TN = 2,2  2,4  4,2  4,4
    _w(3, 7, 9, 64, 64, 1, 1, "tap", 3, 64), _w(3, 7, 9, 64, 128, 1, 1, "tap", 3, 64),
    _w(3, 7, 9, 128, 64, 1, 1, "tap", 3, 64), _w(3, 7, 9, 128, 128, 1, 1, "tap", 3, 64),
    # gathered, 3x3 with W = 57 (one past the ring kernel): M = 171: 3 splits (64, 64, 43)
    _w(1, 3, 57, 64, 64, 3, 1, "tap", 3, 64), _w(1, 3, 57, 128, 128, 3, 1, "tap", 3, 64),
    # gathered, 3x3 stride 2 on 7 x 9 (dy 4 x 5): M = 100: 2 splits (64, 36)
    _w(5, 7, 9, 64, 128, 3, 2, "tap", 2, 64), _w(5, 7, 9, 128, 64, 3, 2, "tap", 2, 64),
    # gathered, 1x1 stride 2: the same grid
    _w(5, 7, 9, 128, 64, 1, 2, "tap", 2, 64), _w(5, 7, 9, 64, 128, 1, 2, "tap", 2, 64),
    # ring kernel: W = 2 (R = 38: the ring wraps every step; M = 120: 2 splits), W = 7 (M = 147: 3 splits; 128 x 128: four tiles),
    # W = 56 (R = 146, M = 168: 3 splits), 3 x 5 images (M = 135: 3 splits)
    _w(30, 2, 2, 64, 64, 3, 1, "ring", 2, 64), _w(3, 7, 7, 64, 64, 3, 1, "ring", 3, 64), _w(3, 7, 7, 128, 128, 3, 1, "ring", 3, 64),
    _w(1, 3, 56, 64, 64, 3, 1, "ring", 3, 64), _w(9, 3, 5, 64, 64, 3, 1, "ring", 3, 64),
]
XLEV_W = 256.0          # level filter gradients: x = idx / 256, slab / 256 and the sum of the slabs are all exact


def _variant(c, **kw):
    d = dict(c)
    d.update(kw)
    return _row(**d)


def _strip(c):
    return {k: v for k, v in c.items() if k != "id"}


WGRAD_DENSE = [_variant(_strip(c), mode=m) for c in WGRAD_SHAPES for m in ("f32", "lev", "idx")]
# term pairs: one shape per kernel and gather form (tap 1x1, tap 3x3 stride 2, ring at W = 7 and on 3 x 5 images)
_PAIR_SHAPES = [WGRAD_SHAPES[0], WGRAD_SHAPES[6], WGRAD_SHAPES[11], WGRAD_SHAPES[14]]
PAIR_CLASSES = [(1, 3), (3, 1), (2, 2)]          # (dy class, x class): x0d0 x1d0 x2d0 | x0d0 x0d1 x0d2 | x0d0 x1d0 x0d1 x1d1
WGRAD_PAIRS = [_variant(_strip(c), set="dy%d_x%d" % p) for c in _PAIR_SHAPES for p in PAIR_CLASSES]
# level operands: lev22 = dy class 2 x odd indices of 9 to 11 bits (x0d0 x1d0 x0d1 x1d1); lev3 = dy class 3 x indices in [0, 3]
# (x0d2).  The sixth pair x1 d2 is 2^-8 x 2^-16 = 2^-24 of a product - the order of the pairs TX = 3 drops by design - and no operand
# set inside the 2^24 budget can pin it.
WGRAD_LEVEL = [_variant(_strip(c), mode=m, set=s) for c in _PAIR_SHAPES for m in ("lev", "idx") for s in ("lev22", "lev3")]
# x_levels = 255: slab / 255 rounds once per slab: held to the bound of the CIFAR index-operand test, not bit-exact
WGRAD_255 = [_variant(_strip(c), mode="lev", set="lev255") for c in (WGRAD_SHAPES[3], WGRAD_SHAPES[7], WGRAD_SHAPES[12])]
SPARSE_K = 18


def wgrad_pixels(c, co):
    """Flat dy-pixel indices where a sparse dy[.., co] is non-zero: the four corners of the first image, the last pixel M - 1,
    both sides of the first split boundary (per - 1, per), one pixel in each of the eight 4-pixel row blocks of the 32-pixel
    step that begins the second split (a lane reads rows 4 fg + fq and 16 + 4 fg + fq; the place inside the block moves with co),
    and three pixels that depend on co."""
    ho, wo = out_hw(c)
    M, per = c["B"] * ho * wo, c["per"]
    assert per + 32 <= M
    px = [0, wo - 1, (ho - 1) * wo, ho * wo - 1, M - 1, per - 1, per]
    px += [per + 4 * g + (co + 3 * g) % 4 for g in range(8)]
    px += [(co * 997 + 131 * j + 29) % M for j in range(3)]
    out = sorted(set(px))
    assert len(out) <= SPARSE_K and out[-1] < M
    return out


def _sparse_dy(c, cls, seed, thin=False):
    ho, wo = out_hw(c)
    vals = gen_by_class(cls, (c["cout"], SPARSE_K), seed)
    if cls == 1:
        vals = torch.where(vals == 0, torch.ones_like(vals), vals)
    dy = torch.zeros(c["B"] * ho * wo, c["cout"], dtype=I64)
    for co in range(c["cout"]):
        px = wgrad_pixels(c, co)
        if thin:                         # every third pixel, the phase moving with co: 6 pixels per channel, every kind in some channel
            px = px[co % 3::3]
        dy[px, co] = vals[co, :len(px)]
    return dy.reshape(c["B"], ho, wo, c["cout"])


def wgrad_operands(c, seed=0):
    """(x or its index, dy) as int64.  Level cases: the returned x IS the index; the tensor handed to the kernel is idx / xlev."""
    xs = (c["B"], c["h"], c["w"], c["cin"])
    ho, wo = out_hw(c)
    ds = (c["B"], ho, wo, c["cout"])
    s = c["set"]
    g = _gen(400 + seed)
    if s == "dense":            # M <= 189 pixels: 189 * 510 * 15 < 2^24
        top = 255 if c["mode"] == "f32" else 510
        return torch.randint(0, top + 1, xs, generator=g, dtype=I64), torch.randint(-15, 16, ds, generator=g, dtype=I64)
    if s == "lev255":           # nothing negative: every rounding is at most 2^-24 of the final value
        return torch.randint(0, 511, xs, generator=g, dtype=I64), torch.randint(0, 16, ds, generator=g, dtype=I64)
    if s == "lev22":            # 6 pixels * 2^10 * 2^11 < 2^24
        return torch.randint(128, 1024, xs, generator=g, dtype=I64) * 2 + 1, _sparse_dy(c, 2, 500 + seed, thin=True)
    if s == "lev3":             # 18 pixels * 2^18 * 3 < 2^24
        return torch.randint(0, 4, xs, generator=g, dtype=I64), _sparse_dy(c, 3, 500 + seed)
    a, b = int(s[2]), int(s[5])
    return gen_by_class(b, xs, 600 + seed), _sparse_dy(c, a, 500 + seed)


def wgrad_xlev(c):
    return 0.0 if c["mode"] == "f32" else (255.0 if c["set"] == "lev255" else XLEV_W)


def wgrad_reference(c, x, dy):
    return wgrad_i64(x, dy, c["ks"], c["stride"], pad_of(c))


def wgrad_expected(c, x, dy):
    """fp32(sum), over 256 for a level operand (exact: a power of two); not for the lev255 cases"""
    assert c["set"] != "lev255"
    t = wgrad_reference(c, x, dy).to(F32)
    return t / torch.tensor(XLEV_W, dtype=F32) if c["mode"] != "f32" else t


# ------------------------------------------------------------------------------------------------------------- the stem
# alignq_qconv_stem7_fwd: a wave walks 16-pixel tiles t = 4 wg + wave, + 4 wg_pg, ... of its group; wg_pg = min(ceil(ceil(Mg / 16) / 4),
# 512) workgroups per group (stem7_wgs), so workgroup wg of a group owns the rows of the tiles t with (t mod 4 wg_pg) div 4 == wg.
# alignq_qconv_stem7_wgrad: one workgroup (= one slab) per 32-pixel step while there are at most 512 steps; above that 512 slabs of
# ceil(steps / 512) steps each, the last ones empty (all-zero slabs).
def _s(op, B, h, w, **kw):
    return _row(op, B, h, w, 3, 64, 7, 2, **kw)


STEM_GRIDS = [(1, 8, 8), (2, 8, 8), (1, 37, 41), (2, 37, 41), (1, 64, 48), (2, 64, 48)]
STEM_FWD = [_s("stem_fwd", *g, set=s) for g in STEM_GRIDS for s in ("dense", "act3")]
STEM_BN = [_s("stem_fwd", B, h, w, w_bit=1, groups=gr) for B, h, w in STEM_GRIDS for gr in ((1, 2) if B == 2 else (1,))]
# 512 x 260: Mg = 256 * 130 = 33280 = 2080 tiles on 512 workgroups: waves 0 .. 31 walk a second tile (t + 2048)
STEM_BN += [_s("stem_fwd", 1, 512, 260, w_bit=1)]
STEM_WGRAD = [_s("stem_wgrad", *g, splits=-(-(g[0] * ((g[1] - 1) // 2 + 1) * ((g[2] - 1) // 2 + 1)) // 32), per=32) for g in STEM_GRIDS]
# 2 x 253 x 161: M = 2 * 127 * 81 = 20574 = 643 steps > 512: 512 slabs of 2 steps (64 pixels), 322 of them with pixels; dy in [-3, 3]
STEM_WGRAD += [_s("stem_wgrad", 2, 253, 161, splits=512, per=64, dy_amp=3)]
STEM_WGRAD_PAIRS = [_variant(_strip(c), set="dy%d_x%d" % p) for c in STEM_WGRAD[3:6] for p in PAIR_CLASSES]
STEM_NNZ = 20          # non-zero bins per output channel of the class-3 forward: 2^18 * 20 * 3 < 2^24


def stem_operands(c, seed=0):
    """stem_fwd: (x, bins [64, 7, 7, 3]); stem_wgrad: (x, dy)"""
    B, h, w = c["B"], c["h"], c["w"]
    ho, wo = out_hw(c)
    g = _gen(700 + seed)
    if c["op"] == "stem_fwd":
        if c["set"] == "act3":
            b = torch.zeros(64, 147, dtype=I64)
            for co in range(64):
                idx = torch.randperm(147, generator=g)[:STEM_NNZ]
                b[co, idx] = torch.randint(1, 4, (STEM_NNZ,), generator=g, dtype=I64) * (torch.randint(0, 2, (STEM_NNZ,), generator=g) * 2 - 1)
            return gen_class3((B, h, w, 3), 710 + seed), b.reshape(64, 7, 7, 3)
        n = int(nlev_of(c))          # dense: 147 * 255 * 255 < 2^24; w_bit = 1: x in [0, 3]
        top = 255 if n > 1 else 3
        return torch.randint(0, top + 1, (B, h, w, 3), generator=g, dtype=I64), torch.randint(-n, n + 1, (64, 7, 7, 3), generator=g, dtype=I64)
    if c["set"] == "dense":          # M <= 1536: 1536 * 255 * 15 < 2^24; M = 20574: 20574 * 255 * 3 < 2^24
        amp = c.get("dy_amp", 15)
        return torch.randint(0, 256, (B, h, w, 3), generator=g, dtype=I64), torch.randint(-amp, amp + 1, (B, ho, wo, 64), generator=g, dtype=I64)
    a, b = int(c["set"][2]), int(c["set"][5])
    return gen_by_class(b, (B, h, w, 3), 720 + seed), _sparse_dy(c, a, 730 + seed)


def stem_bn_expected(y_i64, groups):
    """[groups][wg_pg][64][2] int64 by the tile walk stated above; y_i64 [B, ho, wo, 64]"""
    yg = y_i64.reshape(groups, -1, 64)
    Mg = yg.shape[1]
    tiles = (Mg + 15) // 16
    wg_pg = min((tiles + 3) // 4, 512)
    owner = (torch.arange(Mg) // 16) % (4 * wg_pg) // 4
    out = torch.zeros(groups, wg_pg, 64, 2, dtype=I64)
    out[:, :, :, 0].index_add_(1, owner, yg)
    out[:, :, :, 1].index_add_(1, owner, yg * yg)
    return out


G_CASES = FWD + DGRAD
ALL_WGRAD = WGRAD_DENSE + WGRAD_PAIRS + WGRAD_LEVEL + WGRAD_255
for _cs in (G_CASES, BN, ALL_WGRAD, STEM_FWD, STEM_BN, STEM_WGRAD + STEM_WGRAD_PAIRS):
    assert len({c["id"] for c in _cs}) == len(_cs), "case ids must be unique"
