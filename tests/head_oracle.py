"""Float64 statement of the classifier head (csrc/head_body.h: alignq_head_ce_fwd / _bwd and its two roles in site4_kernels.hip),
the table of launch forms the GPU tests run (tests/test_gpu_head_forms.py) and the bars they hold the kernels to.

Statement (feat [B, HW, C] channels-last, W [K, C], bias [K] or None, target [B] int64, upstream scalar g):
    pooled = mean_p feat;  logits = pooled W^T + bias;  lse_b = log sum_j exp(logits_bj)
    loss_b = lse_b - logits[b, target_b], or 0 when target_b is outside [0, K);  probs = softmax(logits)
    ce_mean = sum_b loss_b / B over ALL B rows;  trans_total = sum_i site_scal[4 i]
    dl = g / B * (probs - onehot(target)), with ZERO rows where the target is outside [0, K) (the gradient of the constant 0)
    dfeat[b, p, :] = dl_b W / HW for every pixel p;  dW = dl^T pooled;  dbias = sum_b dl

Bars.  u = 2^-24 (fp32, round to nearest), gamma_n = n u / (1 - n u): a result that every term reaches through at most n rounded
operations differs from the exact one by at most gamma_n * sum |terms| (Higham, Accuracy and Stability, lemma 3.1); the library is
built with -ffp-contract=off and correctly rounded fp32 division (hipcc's default; csrc/Makefile sets no fast-math flag), so every
operation written in head_body.h is one rounding.  TINY = 2^-149 per operation covers results that round in the subnormal range.
  pooled  against float64 of feat: a term passes at most HW - 1 additions (pixels of one part, then the parts: empty parts add an
          exact 0) and the division: HW roundings.                                    bar = gamma_{HW+1} * mean_p |feat|
  logits  against float64 of the DEVICE's pooled: C fmas from the bias.               bar = gamma_{C+1} * (sum_c |pooled W| + |bias|)
  backward against float64 of the DEVICE's probs and pooled (inputs of alignq_head_ce_bwd).  dl costs three roundings (g / B, the
          difference, the product):
  dfeat   K fmas and the division by HW.                                              bar = gamma_{K+4} * sum_j |dl_j W_jc| / HW
  dW      the rows of one part through fmas, then the non-empty parts (q of them, each holding at most B - (q - 1) rows) through
          q - 1 additions: at most B roundings.                                       bar = gamma_{B+5} * sum_b |dl_b pooled_bc|
  dbias   B - 1 additions.                                                            bar = gamma_{B+4} * sum_b |dl_b|
  loss, probs, ce_mean go through the device's expf / logf, whose accuracy is not derived here: the bars the project already holds
          this kernel to (tests/test_gpu_transition.py), against float64 of the DEVICE's logits: |ce_mean - ref| and |loss_b - ref_b|
          <= 2e-6 * max(1, |ref|), |probs - ref| <= 2e-6, and ce_mean within 1e-6 of the float64 mean of the device's own loss.
  trans_total  the sum is formed in double and rounded once: u * |t| + n 2^-53 sum |scal|.
On the EXACT rows feat, W and bias are multiples of 2^-4 with |feat| <= 2, |W|, |bias| <= 1 and HW a power of two: every partial sum
of the pooling and of the fma chain is a multiple of 2^-4 resp. 2^-14 / HW below 2^24 units (exactness_margin() measures it), hence
exact in fp32 in any order, and pooled / logits must equal the float64 result rounded to fp32 bit for bit.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
MAX_C, MAX_K, STAGED_MAX_B = 256, 64, 1024


def gamma(n):
    return n * U / (1.0 - n * U)


# (B, HW, C, K): what the row selects
ROWS = [
    ((128, 64, 64, 10), "CIFAR: 4 parts of 16 pixels / 32 rows, unrolled rounds only"),
    ((80, 64, 64, 10), "the short last batch: 4 parts of 20 rows = 2 unrolled rounds + 4 tail"),
    ((1, 1, 1, 1), "the first ticket is the last; 256 parts of one channel, 255 of them empty"),
    ((3, 5, 3, 2), "85 parts > HW; thread 255 idle"),
    ((7, 49, 100, 31), "C does not divide 256 (56 idle threads); two parts of 25 / 24 pixels = 3 unrolled rounds + 1 tail"),
    ((5, 200, 256, 64), "one part; K fills the wave"),
    ((2, 1, 256, 64), "HW = 1 at the widest head"),
    ((130, 16, 8, 5), "batch parts of 5 rows: tail loop only, the last 6 of 32 parts empty"),
    ((1025, 1, 4, 3), "B > 1024: the unstaged dW / dbias path (64 parts of 17 rows = 2 unrolled rounds + 1 tail)"),
]
EXACT_ROWS = [
    ((128, 64, 32, 10), "exact inputs: 8 parts of 8 pixels, one unrolled round each"),
    ((16, 32, 256, 64), "exact inputs at the widest head: one part, the longest fma chain"),
]
ALL_ROWS = ROWS + EXACT_ROWS
OOR_VALUES = (-1, None, -100)            # None stands for K


def row_id(shape):
    return "x".join(map(str, shape))


def partition(n, C):
    """the kernel's split of n items (pixels of the pooling and of dfeat, batch rows of dW) over the 256 threads: thread -> (channel
    tid % C, part tid // C); returns parts, per, the item count of every part, the idle threads (part >= parts) and, per part, the
    (unrolled rounds of 8, tail) of the 8-wide loops"""
    parts = max(1, 256 // C)
    per = -(-n // parts)
    sizes = [max(0, min(n, (q + 1) * per) - q * per) for q in range(parts)]
    assert sum(sizes) == n
    idle = [t for t in range(256) if t // C >= parts]
    return dict(parts=parts, per=per, sizes=sizes, idle=idle, loops=[(s // 8, s % 8) for s in sizes])


def oor_rows(B):
    """where the out-of-range cases put their three targets: one row of an unrolled round, one of a tail (at the two shapes that carry
    them the first batch part ends at row 19 resp. 16), and the last row"""
    return (3, 16, B - 1)


def make_case(shape, seed, exact=False, bias=True, oor=False):
    B, HW, C, K = shape
    rng = np.random.default_rng(4600 + seed)
    if exact:
        feat = rng.integers(-32, 33, (B, HW, C)) / 16.0
        W = rng.integers(-16, 17, (K, C)) / 16.0
        b = rng.integers(-16, 17, K) / 16.0
    else:
        feat = rng.standard_normal((B, HW, C)) * 0.8 + 0.3
        W = rng.standard_normal((K, C)) * (1.5 / np.sqrt(C))
        b = rng.standard_normal(K) * 0.1
    target = rng.integers(0, K, B).astype(np.int64)
    if oor:
        for r, v in zip(oor_rows(B), OOR_VALUES):
            target[r] = K if v is None else v
    return dict(shape=shape, feat=feat.astype(np.float32), W=W.astype(np.float32), bias=b.astype(np.float32) if bias else None,
                target=target, exact=exact)


def exactness_margin(case):
    """largest |partial sum| any order can form, in units of the inputs' common grid, for the pooling and for the logits' fma
    chain; both must stay below 2^24 for fp32 to hold every partial sum exactly.  Raises if the inputs are off the 2^-4 grid."""
    B, HW, C, K = case["shape"]
    feat, W = case["feat"].astype(np.float64), case["W"].astype(np.float64)
    bias = np.zeros(K) if case["bias"] is None else case["bias"].astype(np.float64)
    for a in (feat, W, bias):
        assert np.array_equal(a * 16.0, np.round(a * 16.0)), "inputs are not multiples of 2^-4"
    assert HW & (HW - 1) == 0 and HW <= 64
    pool_units = float(np.abs(feat).sum(axis=1).max() * 16.0)
    pooled = feat.sum(axis=1) / HW                                        # multiples of 2^-4 / HW: exact in fp32 and in float64
    unit = 2.0 ** -8 / HW                                                 # grid of pooled * W and of the bias
    chain_units = float(((np.abs(pooled) @ np.abs(W).T) + np.abs(bias)).max() / unit)
    return pool_units, chain_units


def valid_rows(target, K):
    return (target >= 0) & (target < K)


def pooled_ref(feat):
    f = feat.astype(np.float64)
    return f.mean(axis=1), gamma(f.shape[1] + 1) * np.abs(f).mean(axis=1) + TINY


def logits_ref(pooled, W, bias):
    """float64 logits of the given (the device's) pooled and the bar"""
    p, w = pooled.astype(np.float64), W.astype(np.float64)
    b = np.zeros(w.shape[0]) if bias is None else bias.astype(np.float64)
    return p @ w.T + b, gamma(w.shape[1] + 1) * (np.abs(p) @ np.abs(w).T + np.abs(b)) + TINY


def softmax_ref(logits, target):
    """loss [B], probs [B, K], ce_mean in float64 from the given (the device's) logits"""
    lg = logits.astype(np.float64)
    B, K = lg.shape
    mx = lg.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(lg - mx).sum(axis=1))
    ok = valid_rows(target, K)
    loss = np.where(ok, lse - lg[np.arange(B), np.where(ok, target, 0)], 0.0)
    return loss, np.exp(lg - lse[:, None]), loss.sum() / B


def forward(case):
    """the whole forward in float64 from the inputs"""
    pooled, _ = pooled_ref(case["feat"])
    logits, _ = logits_ref(pooled, case["W"], case["bias"])
    loss, probs, ce = softmax_ref(logits, case["target"])
    return dict(pooled=pooled, logits=logits, loss=loss, probs=probs, ce_mean=ce)


def dl_ref(g, probs, target):
    p = probs.astype(np.float64)
    B, K = p.shape
    ok = valid_rows(target, K)
    onehot = np.zeros((B, K))
    onehot[np.arange(B)[ok], target[ok]] = 1.0
    return float(np.float32(g)) / B * (p - onehot) * ok[:, None]


def backward(g, probs, pooled, W, target, HW):
    """dfeat_row [B, C] (the value of every pixel of dfeat[b]), dW [K, C], dbias [K] in float64 from the given (the device's) probs
    and pooled, with their bars"""
    dl = dl_ref(g, probs, target)
    B, K = dl.shape
    w, pl = W.astype(np.float64), pooled.astype(np.float64)
    return dict(dl=dl, dfeat=dl @ w / HW, dW=dl.T @ pl, dbias=dl.sum(axis=0),
                bar_dfeat=gamma(K + 4) * (np.abs(dl) @ np.abs(w)) / HW + TINY,
                bar_dW=gamma(B + 5) * (np.abs(dl).T @ np.abs(pl)) + TINY,
                bar_dbias=gamma(B + 4) * np.abs(dl).sum(axis=0) + TINY)


def trans_ref(site_scal, n_sites):
    s = site_scal.astype(np.float64).reshape(-1, 4)[:n_sites, 0]
    return s.sum(), U * abs(s.sum()) + n_sites * 2.0 ** -53 * np.abs(s).sum() + TINY


def worst(got, ref, bar):
    """largest error / bar"""
    return float((np.abs(np.asarray(got, np.float64) - ref) / bar).max())
