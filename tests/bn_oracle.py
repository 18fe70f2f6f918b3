"""Float64 statement of the training-mode batch-norm fold (csrc/bn_kernels.hip, the finalisation inside site_fwd4_kernel and the
per-tile partials of site_bwd4_kernel in csrc/site4_kernels.hip), the partial layouts restated as index functions, the rows the GPU
tests run (tests/test_gpu_bn_forms.py) and the bars they hold the kernels to.  NumPy only; independent of oracle/alignq_oracle.c.

Statement.  z [B, F] in memory order, F = C * HW, channel of feature f: f % C (channels-last) or f // HW (NCHW); n = B * HW.
    mean_c = sum z / n;  var_c = sum z^2 / n - mean^2 (biased, clamped at 0);  invstd = 1 / sqrt(var + eps)
    a = gamma * invstd;  b = beta - mean * a             (gamma = 1, beta = 0 when None);   save = {mean, invstd}
    running_mean' = (1 - m) running_mean + m mean;  running_var' = (1 - m) running_var + m var n / (n - 1);  counter' = counter + 1
    backward for a given dx and a given save:  zhat = (z - save_mean) * save_invstd
    dbeta = sum dx;  dgamma = sum dx zhat;  k0 = dbeta / n;  k1 = dgamma / n;  dz = a (dx - k0 - zhat k1)
eps and the momentum m are the fp32 values the kernels receive, widened to double.

Layouts (index functions below):
    [C][16][2] doubles   alignq_bn_partial_stats: split s of kBnSplit = 16 holds batch rows [s r, min(B, (s + 1) r)), r = ceil(B / 16)
    [C][64][2] doubles   alignq_bn_partial_stats_nhwc: block g of kNhwcParts = 64 holds pixels [g p, min(B HW, (g + 1) p)),
                         p = ceil(B HW / 64)
    [C][n_parts][2] floats   the convolution epilogue's partials (any split of the pixels into n_parts sets)
    dx_part, NCHW        [F / tile][2], tile c * (HW / tile) + t = features [t tile, (t + 1) tile) of channel c
    dx_part, channels-last   [n_tiles][cp][2], cp = min(C, tile): tile t covers features [t tile, (t + 1) tile); channel c sits at
                         entry c % tile of the tiles t with t % (C / cp) == c // tile
    forward tile rule    32 features up to F = 4096, else 64; one tile per workgroup up to 256 tiles (F <= 16384), above that a tile
                         loop on at most 512 workgroups
    backward tile rule   bwd_tile_features: 64 from F = 16384, else 32

Bars.  u = 2^-24 (fp32), v = 2^-53 (double), round to nearest; the library is built with -ffp-contract=off and hipcc's default
correctly rounded fp32 division and square root, so every operation written in the sources is one rounding.  A sum of m terms formed
in any order in precision w differs from the exact sum by at most (m - 1) w sum|terms| to first order (Higham, Accuracy and
Stability, section 4.2); the bars below are first order, and every one is multiplied by SECOND = 1.01, which covers the products of
error terms as long as every relative error is below 1e-2 (`fwd_bars` asserts that).  TINY = 2^-126 u is added for results that
round in the subnormal range.
  double partial of m elements, against the float64 sum of the same range (the squares of fp32 numbers are exact in double):
        bar = (m + 8) v sum|terms|                 (m - 1 additions; the reference's own pairwise sum and the LDS tree: 8 more)
  totals  s = sum z, q = sum z^2 from double accumulation of n elements and at most 64 partials:
        ds = (n + 64) v sum|z|,  dq = (n + 64) v sum z^2;  from FLOAT partials s_p, q_p (each one rounding of an exact sum) in addition
        ds += u sum|s_p|,  dq += u sum|q_p|
  mean    = s / n (or s * (1 / n): two roundings):        dmean = ds / n + 2 v |mean|
  var     = q / n - mean^2:                               dvar = dq / n + 2 |mean| dmean + 4 v (q / n + mean^2)
          (with float partials this is the issue's  dvar <= u sum|q_p| / n + 2 |mean| dmean  plus the double terms)
  invstd  NCHW finalisation and bn_finalize_kernel: 1 / sqrt in double, one rounding to fp32:
              rel = dvar / (2 (var + eps)) + u + 4 v
          channels-last finalisation: (float)(var + eps), sqrtf, 1.0f / .: the first rounding enters halved through the root:
              rel = dvar / (2 (var + eps)) + u / 2 + u + u
  save_mean = (float) mean:                               bar = u |mean| + dmean
  a       = gamma * invstd, one rounding:                 rel_a = rel_invstd + u;  bar = |a| rel_a
  b       = beta - (float) mean * a: the product of two rounded factors, rounded, then the difference, rounded:
              bar = |a| (u |mean| + dmean) + |mean a| (rel_a + u) + u |b|
  running_mean' = fl(fl(fl(1 - m) rm) + fl(m fl(mean))):  bar = 2 u |(1 - m) rm| + m (2 u |mean| + dmean) + u |result|
  running_var'  with vu = (float)(var n / (n - 1)) formed in double:
              bar = 2 u |(1 - m) rv| + m (2 u vu + dvar n / (n - 1)) + u |result|
  counter  exact.
  backward totals from fp32 partials p_i (each one rounding of an exact sum), summed in double, rounded once, against the float64
  totals of dx itself:     bar(dbeta), bar(dgamma) = u sum|p_i| + u |total| + (cnt + 8) v sum|p_i|
          against the float64 sum of the GIVEN partials the first member drops out (`totals_bar(.., exact_parts=True)`).
  dx_part of the site backward (fp32 accumulation), every entry against the float64 sums of the kernel's own dx over that tile and
          channel: an entry adds m = B * tile / cp terms (B * tile in NCHW) in some order (m - 1 additions), and a term of the second
          sum is formed with three roundings (z - mean, * invstd, dx * zhat):   bar = (m + 3) u sum|terms|
  ktot    k = (float)(total / n):                         bar = (bar(total) - u |total|) / n + u |k|
  dz      per element, against a (dx - k0 - zhat k1) in float64 at the kernel's own fp32 (a, save, k0, k1): z - mean, * invstd, * k1 are
          three roundings of the second term, dx - k0 one, the difference r one, the product with a one:
              bar = u |a| (|dx - k0| + 3 |zhat k1| + 2 |r|)
          where the reference takes k from float64 (the NCHW kernel keeps k to itself), + |a| u (|k0| + |zhat k1|) for its rounding.
Nothing here is fitted to what a kernel returned; tests/test_gpu_bn_forms.py prints the worst error / bar per family.
"""
import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53
TINY = 2.0 ** -150
SECOND = 1.01
K_SPLIT = 16
NHWC_PARTS = 64

DEFECTS = ("nhwc_last_load_dropped", "pair_reads_first", "float_parts_one_round", "t_first_zero", "tpc_minus_one",
           "running_var_biased")


# ------------------------------------------------------------------------------------------------------------ geometry
def channel_of(F, C, nhwc):
    f = np.arange(F)
    return f % C if nhwc else f // (F // C)


def fwd_tiles(F):
    """(tile features, n_tiles, workgroups, looped) of the 64 < B <= 128 site forward"""
    tf = 64 if F > 4096 else 32
    n_tiles = -(-F // tf)
    looped = F > 16384
    cap = 512 if looped else 256
    return tf, n_tiles, min(n_tiles, cap), n_tiles > min(n_tiles, cap)


def bwd_tile_features(F):
    return 64 if F >= 16384 else 32


def nhwc_channels_ok(C):
    return 4 <= C <= 256 and C & (C - 1) == 0


def split_rows(B):
    """batch rows [b0, b1) of the 16 splits of alignq_bn_partial_stats / the NCHW backward"""
    r = -(-B // K_SPLIT)
    return [(min(B, s * r), min(B, (s + 1) * r)) for s in range(K_SPLIT)]


def pixel_ranges(npix, parts=NHWC_PARTS):
    """pixels [p0, p1) of the blocks of alignq_bn_partial_stats_nhwc"""
    p = -(-npix // parts)
    return [(min(npix, g * p), min(npix, (g + 1) * p)) for g in range(parts)]


def even_ranges(npix, parts):
    """n_parts contiguous ranges [floor(i npix / parts), floor((i + 1) npix / parts)): empty ones where parts > npix"""
    return [(i * npix // parts, (i + 1) * npix // parts) for i in range(parts)]


def nhwc_loop_form(B, C, HW):
    """what a row of the channels-last statistics selects: pixel slots per round, pixels per block, empty blocks, trips of the 8-deep
    load round of the fullest slot"""
    slots = 256 // (C // 4)
    rng = pixel_ranges(B * HW)
    per = rng[0][1] - rng[0][0]
    return dict(C4=C // 4, slots=slots, per=per, empty=sum(1 for a, b in rng if a == b), trips=-(-per // (slots * 8)),
                ragged=any(0 < b - a < per for a, b in rng))


def bwd_stage1_form(B, C, HW):
    """what a row of the channels-last backward's stage 1 selects"""
    F = C * HW
    tf = bwd_tile_features(F)
    assert F % tf == 0
    n_tiles = F // tf
    cp = min(C, tf)
    cyc = C // cp
    cnt, groups = n_tiles // cyc, 256 // C
    nvec = B * F // 4
    per = -(-nvec // 128)
    return dict(tile=tf, n_tiles=n_tiles, cp=cp, cyc=cyc, cnt=cnt, groups=groups, rounds=-(-cnt // (groups * 8)), per=per,
                stage2_trips=-(-per // 1024), idle_blocks=sum(1 for g in range(128) if g * per >= nvec))


# ------------------------------------------------------------------------------------------------------------ statement
def _z3(z, C, nhwc):
    """z [B, F] in memory order -> view [B, pixels, C] (channels-last) or [B, C, HW]; the channel axis"""
    z = np.asarray(z, np.float64)
    B = z.shape[0]
    HW = z.reshape(B, -1).shape[1] // C
    return (z.reshape(B, HW, C), 2) if nhwc else (z.reshape(B, C, HW), 1)


def _per_channel(z3, axis):
    return tuple(i for i in range(3) if i != axis)


def forward(z, C, nhwc, gamma=None, beta=None, running_mean=None, running_var=None, counter=0, momentum=0.1, eps=1e-5,
            defect=None):
    """the statement in float64; returns a dict of [C] arrays (mean, var, invstd, a, b, running_mean, running_var, vu), counter, n
    and the absolute sums the bars need (abs1 = sum|z|, sq = sum z^2)"""
    z3, ax = _z3(z, C, nhwc)
    red = _per_channel(z3, ax)
    n = z3.size // C
    m, e = float(np.float32(momentum)), float(np.float32(eps))
    s, q = z3.sum(red), (z3 * z3).sum(red)
    mean = s / n
    var = np.maximum(((z3 - np.expand_dims(mean, red)) ** 2).sum(red) / n, 0.0)      # the two-pass form: no cancellation
    invstd = 1.0 / np.sqrt(var + e)
    g = np.ones(C) if gamma is None else np.asarray(gamma, np.float64)
    bt = np.zeros(C) if beta is None else np.asarray(beta, np.float64)
    a = g * invstd
    vu = var if defect == "running_var_biased" else (var * n / (n - 1.0) if n > 1 else np.full(C, np.inf))
    out = dict(mean=mean, var=var, invstd=invstd, a=a, b=bt - mean * a, vu=vu, n=n, counter=counter + 1,
               abs1=np.abs(z3).sum(red), sq=q, eps=e, momentum=m)
    out["running_mean"] = None if running_mean is None else (1.0 - m) * np.asarray(running_mean, np.float64) + m * mean
    out["running_var"] = None if running_var is None else (1.0 - m) * np.asarray(running_var, np.float64) + m * vu
    out["rm0"] = None if running_mean is None else np.asarray(running_mean, np.float64)
    out["rv0"] = None if running_var is None else np.asarray(running_var, np.float64)
    return out


def zhat_of(z, C, nhwc, save):
    """zhat [B, F] (float64) from a given save = {mean[C], invstd[C]}"""
    z = np.asarray(z, np.float64)
    z = z.reshape(z.shape[0], -1)
    ch = channel_of(z.shape[1], C, nhwc)
    save = np.asarray(save, np.float64).reshape(2, C)
    return (z - save[0][ch][None, :]) * save[1][ch][None, :]


def backward(dx, z, C, nhwc, a, save):
    """dbeta, dgamma, k0, k1 [C] and dz [B, F] in float64 for a given dx, a [C] and save [2, C]"""
    dx = np.asarray(dx, np.float64)
    B = dx.shape[0]
    dx = dx.reshape(B, -1)
    F = dx.shape[1]
    ch = channel_of(F, C, nhwc)
    n = B * (F // C)
    zh = zhat_of(z, C, nhwc, save)
    dbeta = np.bincount(ch, weights=dx.sum(0), minlength=C)
    dgamma = np.bincount(ch, weights=(dx * zh).sum(0), minlength=C)
    k0, k1 = dbeta / n, dgamma / n
    a = np.asarray(a, np.float64)
    dz = a[ch][None, :] * (dx - k0[ch][None, :] - zh * k1[ch][None, :])
    return dict(dbeta=dbeta, dgamma=dgamma, k0=k0, k1=k1, dz=dz, zhat=zh, n=n)


# ------------------------------------------------------------------------------------------------------------ partial layouts
def double_parts_nchw(z, C):
    """[C][16][2] float64 {sum, sum of squares} over each split's own batch rows, and the element count of every split"""
    z3, _ = _z3(z, C, 0)
    out = np.zeros((C, K_SPLIT, 2))
    abs_ = np.zeros((C, K_SPLIT, 2))
    cnt = np.zeros(K_SPLIT, np.int64)
    for s, (b0, b1) in enumerate(split_rows(z3.shape[0])):
        blk = z3[b0:b1]
        out[:, s, 0], out[:, s, 1] = blk.sum((0, 2)), (blk * blk).sum((0, 2))
        abs_[:, s, 0], abs_[:, s, 1] = np.abs(blk).sum((0, 2)), out[:, s, 1]
        cnt[s] = (b1 - b0) * z3.shape[2]
    return out, abs_, cnt


def _pixel_parts(z, C, ranges, dropped=None):
    z3, _ = _z3(z, C, 1)
    px = z3.reshape(-1, C)
    out = np.zeros((C, len(ranges), 2))
    abs_ = np.zeros((C, len(ranges), 2))
    cnt = np.zeros(len(ranges), np.int64)
    for g, (p0, p1) in enumerate(ranges):
        blk = px[p0:p1]
        if dropped is not None and p1 > p0:
            blk = blk[~dropped(np.arange(p1 - p0))]
        out[:, g, 0], out[:, g, 1] = blk.sum(0), (blk * blk).sum(0)
        abs_[:, g, 0], abs_[:, g, 1] = np.abs(blk).sum(0), out[:, g, 1]
        cnt[g] = p1 - p0
    return out, abs_, cnt


def double_parts_nhwc(z, C, defect=None):
    """[C][64][2] float64 over each block's own pixel range (+ absolute sums, pixels per block).  defect nhwc_last_load_dropped: pixel
    j of a block goes to slot j % slots in load u = (j // slots) % 8 of its round; the eighth load is left out"""
    B = np.asarray(z).shape[0]
    npix = np.asarray(z).reshape(B, -1).shape[1] // C * B
    slots = 256 // (C // 4)
    dropped = (lambda j: (j // slots) % 8 == 7) if defect == "nhwc_last_load_dropped" else None
    return _pixel_parts(z, C, pixel_ranges(npix), dropped)


def synth_float_parts(z, C, n_parts):
    """[C][n_parts][2] float32: fp32-rounded float64 sums over n_parts contiguous pixel ranges (channels-last z)"""
    B = np.asarray(z).shape[0]
    npix = np.asarray(z).reshape(B, -1).shape[1] // C * B
    out, _, _ = _pixel_parts(z, C, even_ranges(npix, n_parts))
    return out.astype(np.float32)


def dx_part_shape(B, C, HW, nhwc):
    F = C * HW
    tf = bwd_tile_features(F)
    assert F % tf == 0
    return (F // tf, min(C, tf), 2) if nhwc else (F // tf, 2)


def dx_part_exact(dx, zhat, C, nhwc, absolute=False):
    """the backward's per-tile {sum dx, sum dx zhat} in float64, in the kernel's layout (absolute: the sums of the terms' magnitudes)"""
    dx = np.asarray(dx, np.float64)
    B = dx.shape[0]
    dx = dx.reshape(B, -1)
    F = dx.shape[1]
    tf = bwd_tile_features(F)
    prod = dx * np.asarray(zhat, np.float64).reshape(B, -1)
    cols = np.stack([np.abs(dx).sum(0), np.abs(prod).sum(0)] if absolute else [dx.sum(0), prod.sum(0)], 1)        # [F][2]
    if not nhwc:
        return cols.reshape(F // tf, tf, 2).sum(1)              # feature f of channel c, tile t: (c HW + t tf + j) // tf = c tpc + t
    cp = min(C, tf)
    # tile t, feature j: channel (t tf + j) % C, entry (t tf + j) % C % tf = j % cp (tf and C are powers of two)
    return cols.reshape(F // tf, tf // cp, cp, 2).sum(1)


def dx_part_bar(dx, zhat, C, nhwc):
    """bar on every entry of the site backward's dx_part against the float64 sums of the kernel's own dx (module docstring)"""
    dx = np.asarray(dx)
    B = dx.shape[0]
    F = dx.reshape(B, -1).shape[1]
    tf = bwd_tile_features(F)
    m = B * (tf // min(C, tf) if nhwc else tf)
    return SECOND * (m + 3.0) * U * dx_part_exact(dx, zhat, C, nhwc, absolute=True) + TINY


def synth_dx_part(dx, zhat, C, nhwc):
    return dx_part_exact(dx, zhat, C, nhwc).astype(np.float32)


def totals_from_dx_part(part, B, C, HW, nhwc, defect=None):
    """per-channel {sum, sum} [C][2] (float64) and sum of |partials| [C][2] from a dx_part in the kernel's layout, by the kernels' index
    arithmetic"""
    part = np.asarray(part, np.float64)
    F = C * HW
    tf = bwd_tile_features(F)
    tot, ab = np.zeros((C, 2)), np.zeros((C, 2))
    if not nhwc:
        tpc = HW // tf
        p = part.reshape(C, tpc, 2)
        if defect == "tpc_minus_one":
            p = p[:, :tpc - 1]
        return p.sum(1), np.abs(p).sum(1)
    cp = min(C, tf)
    cyc = C // cp
    p = part.reshape(F // tf // cyc, cyc, cp, 2)
    for c in range(C):
        t_first = 0 if defect == "t_first_zero" else c // cp
        tot[c], ab[c] = p[:, t_first, c % cp].sum(0), np.abs(p[:, t_first, c % cp]).sum(0)
    return tot, ab


def finalize_from_parts(parts, n, C, tile, defect=None):
    """{sum, sum of squares} [C][2] in float64 from partials [C][P][2] the way the channels-last finalisation of a `tile`-feature
    forward tile reads them (defects: the second channel of a pair reads the first one's partials - 32-feature tiles pair local
    channels cl and cl + 16; the float-partial loop stops after its first round of 256 (32-feature tiles) / 512 partials)"""
    parts = np.asarray(parts, np.float64)
    if defect == "float_parts_one_round":
        parts = parts[:, :256 if tile < 64 else 512]
    tot = parts.sum(1)
    if defect == "pair_reads_first" and tile < 64:
        nch = min(C, tile)
        for c in range(C):
            if c % nch >= 16:
                tot[c] = tot[c - 16]
    return tot


def moments_from_totals(tot, n):
    tot = np.asarray(tot, np.float64)
    mean = tot[:, 0] / n
    return mean, np.maximum(tot[:, 1] / n - mean * mean, 0.0)


# ------------------------------------------------------------------------------------------------------------ bars
def part_bar(abs_sums, counts):
    """bar on every double partial [C][P][2] against the float64 sum of its own range"""
    return (np.asarray(counts, np.float64)[None, :, None] + 8.0) * V * abs_sums + TINY


def fwd_bars(ref, invstd_fp32, float_parts=None):
    """bars (dict of [C] arrays: mean, invstd, a, b, running_mean, running_var) for `forward`'s result.  invstd_fp32: the channels-last
    finalisation's fp32 1 / sqrtf (else the double 1 / sqrt).  float_parts [C][P][2]: the fp32 partials the totals come from."""
    n = float(ref["n"])
    mean, var, e = ref["mean"], ref["var"], ref["eps"]
    ds, dq = (n + 64.0) * V * ref["abs1"], (n + 64.0) * V * ref["sq"]
    if float_parts is not None:
        fp = np.abs(np.asarray(float_parts, np.float64))
        ds, dq = ds + U * fp[:, :, 0].sum(1), dq + U * fp[:, :, 1].sum(1)
    dmean = ds / n + 2.0 * V * np.abs(mean)
    dvar = dq / n + 2.0 * np.abs(mean) * dmean + 4.0 * V * (ref["sq"] / n + mean * mean)
    rel_is = dvar / (2.0 * (var + e)) + (2.5 * U if invstd_fp32 else U + 4.0 * V)
    rel_a = rel_is + U
    assert float(rel_a.max()) < 1e-2, "the first-order bars need relative errors below 1e-2"
    a, b, m = ref["a"], ref["b"], ref["momentum"]
    bars = dict(mean=U * np.abs(mean) + dmean, invstd=ref["invstd"] * rel_is, a=np.abs(a) * rel_a,
                b=np.abs(a) * (U * np.abs(mean) + dmean) + np.abs(mean * a) * (rel_a + U) + U * np.abs(b), dvar=dvar)
    if ref["running_mean"] is not None:
        bars["running_mean"] = (2.0 * U * np.abs((1.0 - m) * ref["rm0"]) + m * (2.0 * U * np.abs(mean) + dmean)
                                + U * np.abs(ref["running_mean"]))
    if ref["running_var"] is not None:
        bars["running_var"] = (2.0 * U * np.abs((1.0 - m) * ref["rv0"]) + m * (2.0 * U * ref["vu"] + dvar * n / max(n - 1.0, 1.0))
                               + U * np.abs(ref["running_var"]))
    return {k: (v if k == "dvar" else SECOND * v + TINY) for k, v in bars.items()}


def totals_bar(total, abs_parts, cnt, n, exact_parts=False):
    """(bar on dbeta / dgamma, bar on ktot) for totals [C] from `cnt` fp32 partials per channel with sum of magnitudes abs_parts [C]"""
    total, abs_parts = np.abs(np.asarray(total, np.float64)), np.asarray(abs_parts, np.float64)
    inner = (0.0 if exact_parts else U * abs_parts) + (cnt + 8.0) * V * abs_parts
    return SECOND * (inner + U * total) + TINY, SECOND * (inner / n + U * total / n) + TINY


def dz_ref_and_bar(dx, z, C, nhwc, a, save, k0, k1, k_rounded=False):
    """(reference dz [B, F] in float64 at the given a, save, k0, k1; its per-element bar)"""
    dx = np.asarray(dx, np.float64)
    B = dx.shape[0]
    dx = dx.reshape(B, -1)
    ch = channel_of(dx.shape[1], C, nhwc)
    zh = zhat_of(z, C, nhwc, save)
    a, k0, k1 = (np.asarray(v, np.float64)[ch][None, :] for v in (a, k0, k1))
    t1, t2 = dx - k0, zh * k1
    r = t1 - t2
    bar = U * np.abs(a) * (np.abs(t1) + 3.0 * np.abs(t2) + 2.0 * np.abs(r))
    if k_rounded:
        bar = bar + np.abs(a) * U * (np.abs(k0) + np.abs(t2))
    return a * r, SECOND * bar + TINY


def worst(got, ref, bar):
    """max |got - ref| / bar (inf where a value is not finite)"""
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / bar).max())


# ------------------------------------------------------------------------------------------------------------ rows
# (B, C, HW): what the row selects
STATS_NCHW_ROWS = [
    ((1, 1, 4), "one element row: split 0 only, 15 empty splits, one float4"),
    ((17, 3, 4), "two rows per split, splits 9 to 15 empty"),
    ((16, 2, 1028), "257 float4 per row: a second trip of the 256-thread loop"),
    ((5, 65, 8), "the finaliser's second 64-thread block"),
]
STATS_NHWC_ROWS = [
    ((1, 4, 1), "one pixel, 63 empty blocks, C4 = 1 (256 pixel slots)"),
    ((1, 256, 1), "one pixel, 63 empty blocks, C4 = 64 (no butterfly, row = tid)"),
    ((3, 16, 21), "63 pixels: one per block, one empty block"),
    ((2, 8, 33), "66 pixels: two per block, ragged tail"),
    ((1, 4, 131077), "2049 pixels per block: second trip of the load round at 256 slots"),
    ((1, 256, 2051), "33 pixels per block: second trip at 4 slots"),
    ((7, 128, 19), "C4 = 32"),
    ((5, 32, 13), "C4 = 8"),
    ((9, 64, 7), "C4 = 16"),
]
BWD_NHWC_ROWS = [
    ((2, 4, 16), "cp 4, cnt 2, 64 groups"),
    ((3, 256, 1), "cp 32, cyc 8, cnt 1, one group"),
    ((2, 256, 9), "cnt 9 > 8: second load round at one group"),
    ((2, 64, 256), "F = 16384: 64-feature partials, cp 64"),
    ((1, 4, 8208), "F = 32832: cnt 513 > 512"),
    ((5, 16, 20), "most of the 128 workgroups own four float4 or none"),
    ((2, 256, 1025), "stage 2's second trip"),
]
BWD_NCHW_ROWS = [
    ((1, 1, 64), "tpc 2, B below the 16 splits"),
    ((17, 3, 128), "two rows per split"),
    ((3, 5, 1088), "272 float4 per row"),
    ((2, 1, 16384), "64-feature partials, tpc 256"),
]


def row_id(row):
    return "x".join(map(str, row))


def stats_inputs(B, C, HW, seed=0):
    """z [B, C * HW] (std 1.7, mean 0.3), gamma, beta, running statistics that are not the initial 0 / 1"""
    rng = np.random.default_rng(7919 * B + 101 * C + HW + seed)
    z = (rng.standard_normal((B, C * HW)) * 1.7 + 0.3).astype(np.float32)
    gamma = (rng.random(C) + 0.5).astype(np.float32)
    beta = (rng.standard_normal(C) * 0.2).astype(np.float32)
    rm = (rng.standard_normal(C) * 0.3).astype(np.float32)
    rv = (rng.random(C) + 0.5).astype(np.float32)
    return z, gamma, beta, rm, rv


def place_hard_channel(z, C, nhwc, c=0):
    """overwrite channel c of z with mean 30, standard deviation 0.5"""
    z = np.array(z, np.float32)
    ch = channel_of(z.shape[1], C, nhwc)
    rng = np.random.default_rng(z.shape[0] + z.shape[1])
    z[:, ch == c] = (rng.standard_normal((z.shape[0], int((ch == c).sum()))) * 0.5 + 30.0).astype(np.float32)
    return z


def bwd_inputs(B, C, HW, seed=0):
    """dx, z [B, C * HW], ab [2, C], save [2, C] (fp32; save near the statistics of z, not equal to them: the kernels take it as
    given)"""
    rng = np.random.default_rng(4099 * B + 53 * C + HW + seed)
    F = C * HW
    z = (rng.standard_normal((B, F)) * 1.3 + 0.2).astype(np.float32)
    dx = (rng.standard_normal((B, F)) * 0.01 + 0.002).astype(np.float32)
    ab = np.stack([rng.random(C) + 0.4, rng.standard_normal(C) * 0.2]).astype(np.float32)
    save = np.stack([rng.standard_normal(C) * 0.1 + 0.2, 1.0 / (1.3 + 0.1 * rng.random(C))]).astype(np.float32)
    return dx, z, ab, save
