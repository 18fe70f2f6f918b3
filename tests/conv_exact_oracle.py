"""Exact-integer references, operand generators and the shared case table for the CIFAR convolution kernels' gradient tests
(tests/test_conv_exact_oracle_cpu.py proves the conditions on the CPU, tests/test_gpu_conv_grads_exact.py runs the kernels).

The method: every operand holds integers, and for every output element the sum of the MAGNITUDES of its products stays below
2^24.  Every partial sum, in any order and any grouping (k steps, lane groups, waves, slabs), is then an integer below 2^24,
which fp32 holds exactly: the kernel's result must equal the int64 sum cast to fp32, bit for bit.  A dropped, doubled or
misplaced product changes bits.

The kernels split an fp32 operand into three bf16 terms (bf16_terms).  Which term pairs a test exercises depends on how many
terms its operands need, so the generators come by TERM CLASS:
  class 1: at most 8 significant bits - the middle and low terms are zero (what integers up to 255 are);
  class 2: exactly two terms (here: odd 10-bit integers, h = a multiple of 4, m = +-1);
  class 3: a non-zero third term (here: odd 18-bit integers; about half of them leave a low term, the rest have two terms).
A product of a class-a and a class-b operand is exact in the filter gradient's six kept pairs (dy term, x term) hh, hm, mh, hl,
lh, mm when a + b <= 4 (1 x 3, 3 x 1, 2 x 2).  Class 2 x class 3 is not: ml, lm and ll are dropped by design.

Tensors are NHWC, filters [Cout, KS, KS, Cin].  NumPy / torch on the CPU only; nothing of the package is imported."""
import torch

from tests.test_gpu_conv_sched import _conv_i64

TWO24 = 1 << 24
I64 = torch.int64


# ------------------------------------------------------------------------------------------------------ int64 references
def conv_i64(x, b, stride, pad):
    """y[n, oh, ow, co] = sum_{ky, kx, ci} x[n, S oh + ky - pad, S ow + kx - pad, ci] * b[co, ky, kx, ci]"""
    return _conv_i64(x, b, stride, pad)


def dgrad_i64(dy, b, stride, pad, h_in, w_in):
    """dx [B, h_in, w_in, Cin] of conv_i64 (the transposed convolution): dx[n, S oh + ky - pad, S ow + kx - pad, ci] +=
    dy[n, oh, ow, co] * b[co, ky, kx, ci]"""
    B, Ho, Wo, Cout = dy.shape
    KS, Cin = b.shape[1], b.shape[3]
    buf = torch.zeros(B, h_in + 2 * pad + stride, w_in + 2 * pad + stride, Cin, dtype=I64)
    d = dy.reshape(-1, Cout)
    for ky in range(KS):
        for kx in range(KS):
            c = d.matmul(b[:, ky, kx]).reshape(B, Ho, Wo, Cin)
            buf[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] += c
    return buf[:, pad:pad + h_in, pad:pad + w_in].contiguous()


def transition_dgrad_i64(dy3, b3, dy1, b1, h_in, w_in):
    """the data gradient a transition block's input receives from its 3x3 (padding 1) and 1x1 (padding 0) stride-2 convolutions"""
    return dgrad_i64(dy3, b3, 2, 1, h_in, w_in) + dgrad_i64(dy1, b1, 2, 0, h_in, w_in)


def wgrad_i64(x, dy, ks, stride, pad):
    """dW[co, ky, kx, ci] = sum_{n, oh, ow} dy[n, oh, ow, co] * x[n, S oh + ky - pad, S ow + kx - pad, ci]
    (the stem is ks = 3, stride 1, pad 1 with Cin = 3: 27 columns per output channel)"""
    B, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    xp = torch.zeros(B, H + 2 * pad, W + 2 * pad, Cin, dtype=I64)
    xp[:, pad:pad + H, pad:pad + W] = x
    d = dy.reshape(-1, Cout).t().contiguous()
    out = torch.zeros(Cout, ks, ks, Cin, dtype=I64)
    for ky in range(ks):
        for kx in range(ks):
            xs = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            out[:, ky, kx] = d.matmul(xs.reshape(-1, Cin))
    return out


def assert_exact_budget(op, *operands, **geometry):
    """`op` is one of the references above.  The sum of |product| per output element is that reference on the operands'
    magnitudes; below 2^24 every accumulation order is exact.  Returns the largest sum."""
    worst = int(op(*[t.abs() for t in operands], **geometry).max())
    assert worst < TWO24, "sum of |products| %d reaches 2^24: the result would depend on the accumulation order" % worst
    return worst


# --------------------------------------------------------------------------------------------------------- bf16 terms
def bf16_terms(v):
    """The kernels' split, stated once: h = bf16(v), m = bf16(v - h), l = bf16(v - h - m), round-to-nearest-even (torch's
    bfloat16 conversion).  Returns the three terms as fp32; v == h + m + l exactly for every finite fp32 v."""
    v = v.to(torch.float32)
    h = v.to(torch.bfloat16).to(torch.float32)
    r1 = v - h
    m = r1.to(torch.bfloat16).to(torch.float32)
    r2 = r1 - m
    return h, m, r2.to(torch.bfloat16).to(torch.float32)


def term_counts(v):
    """per element: how many of the three terms are non-zero (0 for a zero)"""
    h, m, l = bf16_terms(v)
    return (h != 0).long() + (m != 0).long() + (l != 0).long()


def class_fractions(v):
    """(fraction of the non-zero elements with a non-zero second term, ... with a non-zero third term)"""
    n = term_counts(v)
    nz = int((n > 0).sum())
    return float((n >= 2).sum()) / max(nz, 1), float((n >= 3).sum()) / max(nz, 1)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _signs(shape, g):
    return torch.randint(0, 2, shape, generator=g, dtype=I64) * 2 - 1


def gen_class1(shape, lo, hi, seed):
    """integers in [lo, hi], |.| <= 255: one bf16 term"""
    assert max(abs(lo), abs(hi)) <= 255
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed), dtype=I64)


def gen_class2(shape, seed):
    """odd integers with exactly 10 significant bits, either sign: h keeps 8 bits (a multiple of 4), m = +-1, l = 0"""
    g = _gen(seed)
    return (torch.randint(256, 512, shape, generator=g, dtype=I64) * 2 + 1) * _signs(shape, g)


def gen_class3(shape, seed):
    """odd integers with exactly 18 significant bits, either sign: h keeps 8 bits, the remainder is odd and up to 512; where it
    exceeds 256 (about half of the elements) m cannot hold it and l != 0"""
    g = _gen(seed)
    return (torch.randint(1 << 16, 1 << 17, shape, generator=g, dtype=I64) * 2 + 1) * _signs(shape, g)


GEN_CLASS = {2: gen_class2, 3: gen_class3}
CLASS_MAG = {1: 3, 2: 1 << 10, 3: 1 << 18}          # exclusive bound of |value| (class 1 as the sparse tests use it: |v| <= 3)


def gen_by_class(cls, shape, seed):
    """the operand of the term-pair tests: class 1 there means integers in [-3, 3] (the partner has up to 18 bits)"""
    return gen_class1(shape, -3, 3, seed) if cls == 1 else GEN_CLASS[cls](shape, seed)


def sparse_bins(cout, ks, cin, nnz, amp, axis, seed):
    """Filter bins [cout, ks, ks, cin] with `nnz` non-zero entries in [-amp, amp] \\ {0} per (co, tap) over ci (axis = 'ci': a
    forward's contraction) or per (ci, tap) over co (axis = 'co': a data gradient's): the sum of |b| over a contraction is at
    most ks * ks * nnz * amp, which bounds the budget against class-3 activations of 18 bits."""
    g = _gen(seed)
    rows, cols = (cout, cin) if axis == "ci" else (cin, cout)
    m = torch.zeros(rows, ks * ks, cols, dtype=I64)
    for r in range(rows):
        for t in range(ks * ks):
            idx = torch.randperm(cols, generator=g)[:nnz]
            m[r, t, idx] = torch.randint(1, amp + 1, (nnz,), generator=g, dtype=I64) * _signs((nnz,), g)
    if axis == "co":
        m = m.permute(2, 1, 0)
    return m.reshape(cout, ks, ks, cin).contiguous()


# ------------------------------------------------------------------------------------------------------- the case table
# Geometry of the launches, read from the launchers of csrc/conv_kernels.hip: `pt` is the filter-gradient kernel's tile, in
# OUTPUT pixels (whole rows); a 32-pixel k step is four lane groups of 8 pixels; with at most 256 tiles every tile is a pixel
# range (slab) of its own.
def _case(kind, **kw):
    c = dict(kind=kind, ks=3, stride=1, pad=1, B=3)
    c.update(kw)
    c.setdefault("h", c["w"])
    c["ho"], c["wo"] = c["h"] // c["stride"], c["w"] // c["stride"]
    c["id"] = "%s_%dx%d_k%ds%d_B%dH%d" % (kind, c["cin"], c["cout"], c["ks"], c["stride"], c["B"], c["h"])
    return c


def body(C, W, **kw):
    return _case("body", cin=C, cout=C, w=W, pt={16: 128, 32: 128, 64: 64}[C], **kw)


def gen(CIN, COUT, W, ks, **kw):
    pt = {(16, 3): 64, (16, 1): 128, (32, 3): 64, (32, 1): 64}[(CIN, ks)]
    return _case("gen", cin=CIN, cout=COUT, w=W, ks=ks, stride=2, pad=1 if ks == 3 else 0, pt=pt, **kw)


def stem(**kw):
    return _case("stem", cin=3, cout=16, w=32, pt=128, **kw)


BODY_SHAPES = [(16, 32), (32, 16), (64, 8)]
TRANSITION_SHAPES = [(16, 32, 32), (32, 64, 16)]

# (a) dense class 1 x class 1: x in [0, 255], dy in [-dy_amp, dy_amp].  B = 3 with H = W (several tiles per image) and H = 8 (the
# smallest legal height: at C = 16 / 32 every 128-pixel tile touches an image boundary); C = 16 at B = 40 is 320 tiles over 256
# pixel ranges of unequal length, with dy in {-1, 0, 1} to keep the budget.
DENSE_BODY = [body(16, 32), body(32, 16), body(64, 8), body(16, 32, h=8), body(32, 16, h=8), body(16, 32, B=40, dy_amp=1)]
DENSE_GEN = [gen(16, 32, 32, 3), gen(16, 32, 32, 1), gen(32, 64, 16, 3), gen(32, 64, 16, 1), gen(16, 32, 32, 3, h=16),
             gen(16, 32, 32, 1, h=16)]
DENSE_STEM = [stem(), stem(h=8)]
DENSE_TRANSITION = [dict(cin=ci, cout=co, w=w, h=h, B=3, id="transition_%dx%d_B3H%d" % (ci, co, h))
                    for ci, co, w, h in [(16, 32, 32, 32), (32, 64, 16, 16), (16, 32, 32, 16)]]


def dense_operands(c, seed=0):
    """x [B, h, w, cin] in [0, 255], dy [B, ho, wo, cout] in [-dy_amp, dy_amp] (15 unless the case says otherwise)"""
    a = c.get("dy_amp", 15)
    x = gen_class1((c["B"], c["h"], c["w"], c["cin"]), 0, 255, 1000 + seed)
    dy = gen_class1((c["B"], c["ho"], c["wo"], c["cout"]), -a, a, 2000 + seed)
    return x, dy


def transition_operands(c, seed=0):
    """x, dy3, dy1 as dense_operands; b3 [cout, 3, 3, cin], b1 [cout, 1, 1, cin] in [-255, 255]"""
    sh = (c["B"], c["h"] // 2, c["w"] // 2, c["cout"])
    x = gen_class1((c["B"], c["h"], c["w"], c["cin"]), 0, 255, 3000 + seed)
    dy3, dy1 = gen_class1(sh, -15, 15, 3001 + seed), gen_class1(sh, -15, 15, 3002 + seed)
    b3 = gen_class1((c["cout"], 3, 3, c["cin"]), -255, 255, 3003 + seed)
    b1 = gen_class1((c["cout"], 1, 1, c["cin"]), -255, 255, 3004 + seed)
    return x, dy3, dy1, b3, b1


# (b) one case per kept term pair set: (dy class, x class) with a sparse dy.  One body shape per channel-blocking path (C = 16:
# the four waves' sum through LDS; C = 64: four (co, ci) blocks), one stride-2 3x3, one 1x1, the stem.
PAIR_CLASSES = [(1, 3), (3, 1), (2, 2)]          # covers hh hm hl | hh mh lh | hh hm mh mm
PAIR_SHAPES = [body(16, 32), body(64, 8), gen(16, 32, 32, 3), gen(16, 32, 32, 1), stem()]
PAIR_CASES = [dict(c, dy_cls=a, x_cls=b, id="%s_dy%d_x%d" % (c["id"], a, b)) for c in PAIR_SHAPES for a, b in PAIR_CLASSES]
SPARSE_K = 15                                    # non-zero pixels per output channel, at most


def sparse_pixels(c, co):
    """Flat output-pixel indices (n * ho * wo + oh * wo + ow) where dy[.., co] is non-zero: the four corners of the first image,
    the last pixel of the batch, both sides of the first tile boundary, one pixel in each of the four 8-pixel lane groups of a
    32-pixel k step of the second tile (another pixel range than the first tile's; the position inside the group moves with co),
    and three pixels that depend on co."""
    ho, wo, pt = c["ho"], c["wo"], c["pt"]
    n_pix = c["B"] * ho * wo
    px = [0, wo - 1, (ho - 1) * wo, ho * wo - 1, n_pix - 1, pt - 1, pt]
    px += [pt + 32 + 8 * g + (co + 3 * g) % 8 for g in range(4)]
    px += [(co * 997 + 131 * j + 29) % n_pix for j in range(3)]
    out = sorted(set(px))
    assert len(out) <= SPARSE_K and out[-1] < n_pix
    return out


def pair_operands(c, seed=0):
    """x dense of class x_cls, dy of class dy_cls at sparse_pixels and zero elsewhere"""
    x = gen_by_class(c["x_cls"], (c["B"], c["h"], c["w"], c["cin"]), 4000 + seed)
    vals = gen_by_class(c["dy_cls"], (c["cout"], SPARSE_K), 5000 + seed)
    if c["dy_cls"] == 1:
        vals = torch.where(vals == 0, torch.ones_like(vals), vals)
    dy = torch.zeros(c["B"] * c["ho"] * c["wo"], c["cout"], dtype=I64)
    for co in range(c["cout"]):
        px = sparse_pixels(c, co)
        dy[px, co] = vals[co, :len(px)]
    return x, dy.reshape(c["B"], c["ho"], c["wo"], c["cout"])


# (c) index-operand filter gradient: (C, W, bytes per index, a_bit); an int8 index holds at most 127
BINS_CASES = [(16, 32, 2, 8), (16, 32, 1, 8), (32, 16, 2, 8), (32, 16, 1, 4), (64, 8, 2, 8), (64, 8, 1, 8), (16, 32, 1, 1)]


def bins_operands(C, W, nbytes, a_bit, seed=0):
    """idx [3, W, W, C] in [0, min(2^a_bit - 1, 127 for int8)], dy in [0, 15]: every partial sum is non-negative"""
    top = min((1 << a_bit) - 1, 127 if nbytes == 1 else 1 << 15)
    idx = torch.randint(0, top + 1, (3, W, W, C), generator=_gen(6000 + seed + C + nbytes), dtype=I64)
    dy = torch.randint(0, 16, (3, W, W, C), generator=_gen(6100 + seed + C + nbytes), dtype=I64)
    return idx, dy


# (e) forward and data gradient with class-3 activations: 18-bit operands against sparse small filter bins.  A contraction meets
# at most ks * ks * ACT3_NNZ non-zero bins of magnitude <= ACT3_AMP: 2^18 * 9 * 2 * 3 < 2^24.
ACT3_NNZ, ACT3_AMP = 2, 3
ACT3_CASES = ([dict(body(C, W), op=op) for C, W in BODY_SHAPES for op in ("fwd", "dgrad")] + [dict(stem(), op="fwd")] +
              [dict(gen(ci, co, w, ks), op=op) for ci, co, w in TRANSITION_SHAPES for ks in (3, 1) for op in ("fwd", "dgrad")])
for _c in ACT3_CASES:
    _c["id"] = _c["id"] + "_" + _c["op"]


def act3_operands(c, seed=0):
    """(activation, bins): class-3 x [B, h, w, cin] for a forward, class-3 dy [B, ho, wo, cout] for a data gradient; the stem's 27
    columns take dense bins in [-2, 2] (27 * 2 < 64)"""
    if c["op"] == "fwd":
        a = gen_class3((c["B"], c["h"], c["w"], c["cin"]), 7000 + seed)
    else:
        a = gen_class3((c["B"], c["ho"], c["wo"], c["cout"]), 7100 + seed)
    if c["kind"] == "stem":
        b = gen_class1((16, 3, 3, 3), -2, 2, 7200 + seed)
    else:
        b = sparse_bins(c["cout"], c["ks"], c["cin"], ACT3_NNZ, ACT3_AMP, "ci" if c["op"] == "fwd" else "co", 7300 + seed)
    return a, b
