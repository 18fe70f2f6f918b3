"""NumPy restatement of include/alignq_dense.h (DenseNet's evaluation without concatenations) and the case table of its tests,
composed from statements the other tests trust: tests/mobile_eval_oracle.py `site` (the folded evaluation site) followed by an fp64
3x3 / stride 1 / padding 1 convolution, and the 2 x 2 pool in the order the header gives.  Tensors are channels-last: [B, H, W, C]
arrays.  tests/test_dense_eval_cpu.py checks the table, tests/test_gpu_dense_eval.py runs it."""
import numpy as np

from tests import k3conv_exact_oracle as K3
from tests import mobile_eval_oracle as MO

ADMM, CDF = MO.ADMM, MO.CDF
NONE, RELU = MO.NONE, MO.RELU
F32 = np.float32

# (CIN, COUT): one chunk, a tail of 4 (36) and of 28 (60, 444), many chunks, all three tile widths (16 / 32 / 64 output channels)
CHANNELS = [(4, 4), (24, 12), (36, 12), (60, 12), (444, 12), (12, 24), (64, 64)]
GRIDS = [(1, 1, 1), (1, 7, 9), (1, 8, 8), (1, 9, 7), (3, 5, 5)]
GBIG = K3.GBIG              # (33, 64, 64): 2112 tiles, past one pass of the grid cap
GWT = K3.GWT                # (16, 64, 64): 1 MiB at 4 channels, the first size of the write-through window
PITCHES = ["contiguous", "inplace", "inplace_spare"]          # x and y apart | y = x + CIN | the same with 8 spare channels behind y
SPARE = 8
KS = [4, 2, 8, 32]
WT_MIN_BYTES, WT_MAX_BYTES = 1 << 20, 64 << 20


def cases():
    """Every (CIN, COUT) x grid x pitch, the quantiser width, the formula and the clamp cycling through their sets so that every
    channel pair meets every k, both formulas and both clamps; gamma / beta NULL once per channel pair."""
    out = []
    for ci, (cin, cout) in enumerate(CHANNELS):
        grids = GRIDS + ([GBIG, GWT] if (cin, cout) == (4, 4) else [])
        i = 0
        for grid in grids:
            for pitch in PITCHES:
                out.append(dict(id="%dto%d_%s_%s" % (cin, cout, "x".join(map(str, grid)), pitch), cin=cin, cout=cout, grid=grid, pitch=pitch,
                                k=KS[(i + ci) % 4], formula=(ADMM, CDF)[(i // 4 + ci) % 2], clamp=NONE if i % 5 == 3 else RELU,
                                affine=i != 6, w_bit=(4, 8, 2)[i % 3], seed=1000 * ci + i))
                i += 1
    return out


CASES = cases()


def pitches(c):
    """(ldx, ldy, y's offset in floats from x or None for a buffer of its own) of one case"""
    cin, cout = c["cin"], c["cout"]
    if c["pitch"] == "contiguous":
        return cin, cout, None
    ld = cin + cout + (SPARE if c["pitch"] == "inplace_spare" else 0)
    return ld, ld, cin


def form(c):
    return K3.gemm_form(c["cout"])


def spatial_tiles(c):
    B, H, W = c["grid"]
    return B * ((H + K3.TILE - 1) // K3.TILE) * ((W + K3.TILE - 1) // K3.TILE)


def write_through(c):
    B, H, W = c["grid"]
    return WT_MIN_BYTES <= B * H * W * c["cout"] * 4 <= WT_MAX_BYTES


def operands(c, r=2.0):
    """x [B, H, W, CIN] fp32, the batch-norm vectors (gamma, beta, mean, var) with b_c = beta_c - a_c mean_c >= 0.2 for every channel -
    so that clamp(q(b_c)) > 0 and an unzeroed padding pixel or tail channel shows -, eps, and a quantised filter (COUT, CIN, 3, 3)
    whose bins are integers of w_bit bits"""
    rng = np.random.default_rng(c["seed"])
    B, H, W = c["grid"]
    cin, cout = c["cin"], c["cout"]
    x = (rng.standard_normal((B, H, W, cin)) * 1.3).astype(F32)
    gamma = rng.uniform(0.7, 1.3, cin).astype(F32) if c["affine"] else None
    beta = rng.uniform(0.0, 0.5, cin).astype(F32) if c["affine"] else None
    mean = rng.uniform(-1.0, -0.4, cin).astype(F32)
    var = rng.uniform(0.5, 1.5, cin).astype(F32)
    n = 2 ** c["w_bit"] - 1
    wq = (np.rint(np.tanh(rng.standard_normal((cout, cin, 3, 3))) * n) / n).astype(F32)
    return x, (gamma, beta, mean, var), 1e-5, wq


def vecs_filled(vecs):
    gamma, beta, mean, var = vecs
    return (np.ones_like(mean) if gamma is None else gamma, np.zeros_like(mean) if beta is None else beta, mean, var)


def site(x, vecs, eps, k, r, formula, mode):
    """alignq_site_eval_fwd's statement (tests/mobile_eval_oracle.py); gamma / beta None = 1 / 0"""
    return MO.site(x, vecs_filled(vecs), eps, k, r, formula, mode)


def conv3x3_f64(s, wq):
    """fp64 3x3 / stride 1 / padding 1 convolution of s [B, H, W, CIN] with wq (COUT, CIN, 3, 3): zeros around the image"""
    B, H, W, _ = s.shape
    pad = np.zeros((B, H + 2, W + 2, s.shape[3]), dtype=np.float64)
    pad[:, 1:-1, 1:-1] = s
    w = np.asarray(wq, dtype=np.float64)
    y = np.zeros((B, H, W, w.shape[0]), dtype=np.float64)
    for ky in range(3):
        for kx in range(3):
            y += pad[:, ky:ky + H, kx:kx + W] @ w[:, :, ky, kx].T
    return y


def layer(x, vecs, eps, k, r, formula, mode, wq):
    """alignq_dense_layer_eval_fwd in fp64 behind the site: the padding is zero AFTER the site"""
    return conv3x3_f64(site(x, vecs, eps, k, r, formula, mode), wq)


def pool(x):
    """alignq_avgpool2_nhwc_fwd: (((x00 + x01) + x10) + x11) * 0.25 in fp32, odd trailing rows and columns dropped; x [B, H, W, C]"""
    x = np.asarray(x, dtype=F32)
    Ho, Wo = x.shape[1] // 2, x.shape[2] // 2
    x = x[:, :2 * Ho, :2 * Wo]
    x00, x01, x10, x11 = x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]
    return ((((x00 + x01).astype(F32) + x10).astype(F32) + x11).astype(F32) * F32(0.25)).astype(F32)


POOL_SHAPES = [(1, 2, 2, 4), (2, 5, 7, 12), (3, 16, 16, 168)]          # (B, H, W, C)
