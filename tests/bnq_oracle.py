"""NumPy / float64 statement of the folded batch-norm + quantiser family (alignq_amd/csrc/bnq_kernels.hip, exports alignq_bnq_*):
the case table, the launch geometry each row selects, the forward statistics one operation at a time, the float64 backward
and its bars.  tests/test_bnq_oracle_cpu.py checks this module; tests/test_gpu_bnq_forms.py holds the kernels to it.

FORWARD STATISTICS, BIT FOR BIT.  z holds multiples of 2^-8 with |z| <= 8, so sum z and sum z^2 over any P <= 2^20 pixels are
exact doubles in ANY order (z^2 <= 2^22 units of 2^-16; 2^20 of them stay below 2^53).  What bnq_sums_kernel<0> leaves and
bnq_finalize_kernel / fin_totals add up is therefore the exact total whatever the partition, and the rest is a fixed sequence of
correctly rounded operations (bnq_kernels.hip:210-225, :342-355; the file is built with -ffp-contract=off), restated by stats():
    mean = s / n;  var = max(q / n - mean * mean, 0);  invstd = f32(1 / sqrt(var + f64(f32 eps)))             (double)
    a = gamma * invstd;  b = beta - f32(mean) * a                                                            (float, two operations)
    running_mean = (1 - m) * rm + m * f32(mean);  running_var = (1 - m) * rv + m * f32(var * n / (n - 1))    (float), slice after slice
    num_batches_tracked += groups
This rests on the device's float64 divide and square root being correctly rounded.  On an MI355X every row, in every form, is
bit-equal to this restatement: no allowance of an ulp of invstd is made anywhere.

FORWARD OUTPUTS.  Given the (a, b) read back from the device, x = fma(a, z, b) (oracle_c.bn_apply) and y = [relu](quantise(x)
[+ residual]) (oracle_c.act_quant_fwd) bit for bit: no tie band, because nothing is compared at another (a, b).

BACKWARD, float64, from what the forward left (ab, save, the mask): with x as above, zhat = (z - mean) * invstd,
    dx = g * [y > 0] * r * 2 phi(x);  k0 = mean dx;  k1 = mean dx zhat;  dz = a (dx - k0 - zhat k1)
    dbeta = sum over slices and pixels of dx;  dgamma = ... of dx zhat;  dres = g * [y > 0]  (a copy: exact)
The bars count the roundings of the kernels' stated float32 operations, eps = 2^-24 (half an ulp):
  * dx = gm * (r * c * __expf(-0.5f * x * x)): the product x * x is rounded once (relative eps in the argument: x^2/2 eps in
    the result), the rest - the multiply by log2(e) inside __expf, the hardware exp2, the three products - is collected in c_exp:
        e_dx = |dx| (x^2 / 2 + c_exp) eps                                (0 for alignq_bnq_bwd_dx, where dx is given)
  * the sums run in double over the float values: their own error is 2^-53-sized and dropped; zhat = (z - mean) * invstd is two
    float operations (2 eps relative); k0 and k1 are rounded to float once:
        e_k0 = mean e_dx + |k0| eps
        e_k1 = mean(e_dx |zhat|) + 2 eps mean(|dx| |zhat|) + |k1| eps
  * dz = a * ((dx - k0) - zhat * k1): the operands' errors, 2 eps on zhat inside the product, and three roundings (product,
    two differences; the final product by a is the third relative eps on the whole) bounded by the sum of magnitudes:
        bar_dz = |a| (e_dx + e_k0 + |zhat| e_k1 + 2 eps |zhat k1| + 3 eps (|dx| + |k0| + |zhat k1|))
        bar_dbeta = sum e_dx + eps |dbeta|
        bar_dgamma = sum e_dx |zhat| + 2 eps sum |dx zhat| + eps |dgamma|
A channel with gamma == 0 has bar_dz == 0: its dz must be exactly +0 or -0.  emulate32() evaluates the kernels' stated
operations in float32 with an ideal exp2; it stays below every bar (test_bnq_oracle_cpu.py), the planted defects of DEFECTS
exceed them by orders of magnitude.

C_EXP is measured, not fitted to any bnq kernel: alignq_act_quant_bwd with g = 1 returns act_jac alone
(test_gpu_bnq_forms.py::test_fast_exponential_within_c_exp, 2^20 points of [-6, 6] and their neighbours against float64).
Measured on an MI355X: worst relative error 1.946 (x^2 / 2 + 1) eps at x = 0.838 with act_range 2 and 1.820 at x = -5.697 with
act_range 10 (MEASURED_EXP_UNITS = 1.95); C_EXP = twice that, rounded up = 4 (the margin covers arguments the grid misses).
The figure grows with x^2 / 2 + 1 as a whole (31.6 eps at |x| = 5.7: the product by log2(e) and that constant's own rounding
scale with the argument like the rounding of x * x does), so beyond |x| ~ 2.5 the error of ONE dx can exceed e_dx as stated
(x^2 / 2 + 4 = 20.2 eps at 5.7).  dx is then below 0.05 of its size at x = 0 and the bars of dz, dgamma and dbeta are carried by
their other terms: every row of the GPU test sits between 0.04 and 0.62 of its bar (alignq_bnq_bwd) and between 0.18 and 0.99
(alignq_bnq_bwd_dx, where bar_dbeta is the final rounding to float alone: at most 1 by construction).

OUT OF REACH.  tiles()' cap of 16384 workgroups needs 64 M elements (256 * 4 * 4 floats per workgroup) and parts_for's
`cap < 64` arm a channel count above 4096, which bad_c refuses: neither is run.  The largest row is 6.1 M floats."""
import functools

import numpy as np

from tests import oracle_c as O

EPS = 2.0 ** -24
MEASURED_EXP_UNITS = 1.95        # see the docstring; printed by test_fast_exponential_within_c_exp
C_EXP = 4
TWO_OVER_SQRT_2PI = 0.7978845608028654
MOMENTUM, BN_EPS = np.float32(0.1), np.float32(1e-5)
NBT0 = 7                         # num_batches_tracked before the call

# ------------------------------------------------------------------------------------------------ launch geometry
K_T, K_PARTS, K_US, K_UA = 256, 512, 4, 4                # bnq_kernels.hip:28-31
K_FIN_C, K_FIN_PARTS = 64, 128                           # :289
MAX_GROUPS = 8                                           # ALIGNQ_BNQ_MAX_GROUPS (include/alignq.h)


def bad_c(C):                                            # :510
    return C < 4 or C > 2048 or (C & (C - 1)) != 0


def threads_for(C):                                      # :511
    return 512 if (C >> 2) > K_T else K_T


def tiles(nvec, u, nt=K_T):                              # :512-516
    b = max((nvec + nt * u - 1) // (nt * u), 1)
    return min(b, 256 * 64)


def parts_for(P, C, taken=None):                         # :523-533 (sums_threads(C) == 512 for every C, :519-522)
    slots = 512 // (C >> 2)
    n = max(P // (slots * K_US), 1)
    cap = (4 << 20) // (C * 16)
    if n > cap:
        n = 64 if cap < 64 else cap
        if taken is not None:
            taken.add("parts: 4 MiB cap")
    if n > K_PARTS and taken is not None:
        taken.add("parts: kParts cap")
    return min(n, K_PARTS)


def fin_small(P, C, groups):                             # :596-598
    return groups == 1 and C <= K_FIN_C and P * C <= (4 << 20)


def fin_parts(P, C):                                     # :599-602
    return min(parts_for(P, C), min((64 * 1024) // (C * 16), K_FIN_PARTS))


def fin_grid(nvec, u):                                   # :603
    return min(tiles(nvec, u), 512)


def finalize_u(nparts):                                  # launch_finalize, :559-569
    return 12 if 64 * 8 < nparts <= 64 * 12 else 8


def mask_words(nvec):                                    # :53
    return ((nvec + 63) >> 6) * 4


def ws_bytes(C, groups):                                 # alignq_bnq_ws_bytes, :577-580
    return groups * (K_PARTS * C * 2 * 8 + 2 * C * 4)


def branches(groups, P, C, conv_parts=0):
    """the branches of the forward's launch path that (groups, P, C[, partials handed in]) selects, as a set of labels"""
    t = set()
    nvec = P * (C >> 2)
    if not conv_parts and fin_small(P, C, groups):
        t.add("in-kernel finalisation")
        grid = fin_grid(nvec, K_UA)
        t.add("in-kernel: one grid pass" if grid * K_T * K_UA >= nvec else "in-kernel: a second grid pass")
        t.add(f"in-kernel: {K_T // C} slices in fin_totals")
        if fin_parts(P, C) > 8 * (K_T // C):
            t.add("in-kernel: a second round of fin_totals")
        if P * C == (4 << 20):
            t.add("in-kernel: the P*C boundary")
        np_ = fin_parts(P, C)
    else:
        t.add("general")
        if groups == 1 and C <= K_FIN_C and not conv_parts:
            t.add("general: just past the P*C boundary")
        if conv_parts and fin_small(P, C, groups):
            t.add("general: partials handed in at an in-kernel shape")
        t.add(f"general: {threads_for(C)} threads")
        np_ = conv_parts if conv_parts else parts_for(P, C, t)
        u = finalize_u(np_)
        t.add(f"finalise: U = {u}, " + ("one round" if np_ <= 64 * u else "several rounds"))
        if groups % 2 and groups > 1:
            t.add("finalise: lone tail slice")
        if groups == MAX_GROUPS:
            t.add("finalise: ALIGNQ_BNQ_MAX_GROUPS slices")
    if np_ == 1:
        t.add("parts: one")
    if nvec % 64:
        t.add("mask: nvec % 64 != 0")
    return t


REQUIRED_BRANCHES = [
    "in-kernel finalisation", "in-kernel: one grid pass", "in-kernel: a second grid pass", "in-kernel: 4 slices in fin_totals",
    "in-kernel: 64 slices in fin_totals", "in-kernel: a second round of fin_totals", "in-kernel: the P*C boundary",
    "general", "general: just past the P*C boundary", "general: partials handed in at an in-kernel shape", "general: 256 threads",
    "general: 512 threads", "parts: one", "parts: kParts cap", "parts: 4 MiB cap", "finalise: U = 8, one round",
    "finalise: U = 12, one round", "finalise: U = 8, several rounds", "finalise: lone tail slice",
    "finalise: ALIGNQ_BNQ_MAX_GROUPS slices", "mask: nvec % 64 != 0",
]

# ------------------------------------------------------------------------------------------------ case table
# (groups, P, C, formula, relu, residual, mask, bins, k, act_range, nulls, the branch the row is there for)
# bins: "" none, "y" bins_out beside y, "noy" bins_out with y == NULL.  nulls: gamma / beta / running statistics / nbt all NULL.
_IN, _GEN = "in-kernel finalisation", "general"
ROWS = [
    # in-kernel finalisation (groups == 1, C <= 64, P*C <= 4 Mi)
    (1, 2, 4, 0, 1, 0, 1, "", 1, 2.0, 0, "parts: one"),
    (1, 2, 4, 1, 0, 1, 0, "", 32, 10.0, 0, _IN),
    (1, 75, 4, 0, 1, 0, 1, "y", 4, 2.0, 0, "mask: nvec % 64 != 0"),
    (1, 75, 4, 0, 0, 0, 0, "noy", 8, 2.0, 1, _IN),
    (1, 105, 16, 0, 1, 1, 1, "", 16, 10.0, 0, "in-kernel: one grid pass"),
    (1, 105, 16, 1, 1, 0, 1, "", 2, 2.0, 0, _IN),
    (1, 4100, 64, 0, 1, 0, 1, "y", 8, 2.0, 0, "in-kernel: 4 slices in fin_totals"),
    (1, 70000, 4, 1, 1, 1, 1, "", 4, 2.0, 0, "in-kernel: 64 slices in fin_totals"),
    (1, 40000, 64, 1, 1, 1, 1, "", 4, 2.0, 0, "in-kernel: a second grid pass"),       # the CDF-only CIFAR form
    (1, 65536, 64, 0, 1, 0, 1, "", 2, 2.0, 0, "in-kernel: the P*C boundary"),
    # general, 256 threads
    (2, 54, 4, 0, 1, 0, 1, "y", 4, 2.0, 0, _GEN),
    (2, 54, 4, 1, 0, 1, 0, "", 32, 10.0, 0, _GEN),
    (1, 33, 128, 0, 1, 1, 1, "", 16, 2.0, 0, "general: 256 threads"),
    (1, 33, 128, 0, 0, 0, 0, "noy", 8, 2.0, 1, _GEN),
    (3, 130, 256, 1, 1, 0, 1, "", 2, 2.0, 0, "finalise: lone tail slice"),
    (3, 130, 256, 0, 1, 0, 1, "y", 8, 10.0, 0, "finalise: lone tail slice"),
    (8, 9, 32, 0, 1, 0, 1, "", 1, 2.0, 0, "finalise: ALIGNQ_BNQ_MAX_GROUPS slices"),
    (8, 9, 32, 1, 1, 1, 1, "", 4, 2.0, 0, "finalise: ALIGNQ_BNQ_MAX_GROUPS slices"),
    (1, 70000, 64, 0, 1, 0, 1, "", 8, 2.0, 0, "parts: kParts cap"),                    # just past the P*C boundary: 546 -> kParts
    (1, 9000, 512, 1, 1, 0, 1, "", 4, 2.0, 0, "parts: 4 MiB cap"),                     # 562 -> 512: at C = 512 this cap EQUALS kParts
    (2, 3000, 1024, 0, 1, 1, 1, "", 8, 2.0, 0, "parts: 4 MiB cap"),
    # 512 threads
    (1, 2, 2048, 0, 1, 0, 1, "", 1, 2.0, 0, "general: 512 threads"),
    (1, 2, 2048, 1, 1, 1, 1, "", 2, 2.0, 0, "general: 512 threads"),
    (1, 2, 2048, 0, 1, 0, 1, "y", 4, 2.0, 0, "general: 512 threads"),
    (1, 2, 2048, 0, 0, 0, 0, "noy", 8, 2.0, 1, "general: 512 threads"),
    (1, 2, 2048, 0, 1, 0, 1, "", 16, 10.0, 0, "general: 512 threads"),
    (1, 2, 2048, 1, 0, 0, 0, "", 32, 10.0, 0, "general: 512 threads"),
    (2, 700, 2048, 0, 1, 0, 1, "", 8, 2.0, 0, "parts: 4 MiB cap"),                    # (cap 128)
]
ROW_FIELDS = ("groups", "P", "C", "formula", "relu", "residual", "mask", "bins", "k", "r", "nulls", "branch")
# partials handed in: alignq_bnq_stats_parts with z == NULL and alignq_bnq_fwd_parts, C = 64 (groups == 1: an in-kernel shape)
PARTS_P, PARTS_C = 70, 64
PARTS_ROWS = [(groups, cp) for groups in (1, 3) for cp in (1, 63, 512, 513, 686, 768, 769, 1100)]
# alignq_bnq_bwd_dx (no in-kernel form): P chosen per C so that every row has several partials
BWD_DX_ROWS = [(groups, P, C) for groups in (1, 2, 3) for P, C in ((5000, 4), (130, 256), (33, 2048))]
AFFINE_ROWS = [(1, 1, 4), (8, 1, 32), (1, 75, 4), (3, 130, 256), (8, 9, 32), (1, 5000, 64), (2, 33, 2048)]


def row_dict(row):
    return dict(zip(ROW_FIELDS, row))


def row_id(row):
    g, P, C, f, relu, res, mask, bins, k, r = row[:10]
    return f"{g}x{P}x{C}-f{f}-k{k}-r{int(r)}" + ("-relu" if relu else "") + ("-res" if res else "") + ("-mask" if mask else "") + \
        (f"-bins{bins}" if bins else "") + ("-nulls" if row[10] else "")


# ------------------------------------------------------------------------------------------------ inputs
def dyadic(rng, shape, mean=0.4, std=1.7):
    """multiples of 2^-8 within [-8, 8]"""
    return np.clip(np.round(rng.normal(mean, std, shape) * 256.0) / 256.0, -8.0, 8.0).astype(np.float32)


def channels_of(C):
    """the four special channels of every case: constant (var clamps to 0), mean 6 with standard deviation 2^-6 (one-pass
    cancellation), gamma == 0, |gamma| = 1e-3 |beta|"""
    return dict(const=0, cancel=1, gamma0=2, tiny=3) if C == 4 else dict(const=1, cancel=C // 2, gamma0=C - 1, tiny=C // 4 + 1)


def make_z(groups, P, C, seed):
    rng = np.random.default_rng(seed)
    z = dyadic(rng, (groups, P, C))
    ch = channels_of(C)
    z[:, :, ch["const"]] = 1.25
    z[:, :, ch["cancel"]] = (6.0 + np.round(rng.normal(0.0, 4.0, (groups, P))) / 256.0).astype(np.float32)
    return z


@functools.lru_cache(maxsize=2)
def make_case(groups, P, C, residual=0, nulls=0, seed=0):
    """z [groups, P, C], the parameters, the running statistics before the call, the residual (arrays are shared: do not
    write to them)"""
    rng = np.random.default_rng(1000 + seed)
    ch = channels_of(C)
    case = dict(groups=groups, P=P, C=C, z=make_z(groups, P, C, 77 * seed + P + C), ch=ch)
    if nulls:
        case.update(gamma=None, beta=None, rm=None, rv=None, nbt=None)
    else:
        gamma = (rng.random(C) + 0.5).astype(np.float32) * np.where(rng.random(C) < 0.25, -1, 1).astype(np.float32)
        beta = (rng.standard_normal(C) * 0.2).astype(np.float32)
        gamma[ch["gamma0"]] = 0.0
        beta[ch["tiny"]] = 0.75
        gamma[ch["tiny"]] = np.float32(1e-3) * beta[ch["tiny"]]
        case.update(gamma=gamma, beta=beta, rm=(rng.standard_normal(C) * 0.5).astype(np.float32),
                    rv=(rng.random(C) + 0.5).astype(np.float32), nbt=NBT0)
    case["res"] = (rng.standard_normal((groups, P, C)) * 0.7).astype(np.float32) if residual else None
    return case


def case_of(row, seed):
    d = row_dict(row)
    return make_case(d["groups"], d["P"], d["C"], d["residual"], d["nulls"], seed)


def make_g(z, save, seed):
    """g = N(0, 1) + 0.5 + 0.5 zhat: k0 and k1 are O(1) times the jacobian in every channel"""
    rng = np.random.default_rng(5000 + seed)
    zhat = (z.astype(np.float64) - save[:, None, 0, :].astype(np.float64)) * save[:, None, 1, :].astype(np.float64)
    return (rng.standard_normal(z.shape) + 0.5 + 0.5 * zhat).astype(np.float32)


def random_partials(z, conv_parts, seed):
    """[groups][conv_parts][C][2] doubles {sum z, sum z^2}: every pixel of z in one randomly chosen partial (exact sums)"""
    groups, P, C = z.shape
    rng = np.random.default_rng(seed)
    part = np.zeros((groups, conv_parts, C, 2))
    z64 = z.astype(np.float64)
    for g in range(groups):
        where = rng.integers(0, conv_parts, P)
        np.add.at(part[g, :, :, 0], where, z64[g])
        np.add.at(part[g, :, :, 1], where, z64[g] * z64[g])
    return part


# ------------------------------------------------------------------------------------------------ forward statistics
def totals(z):
    """{sum z, sum z^2} per slice and channel, exact for dyadic z (any order)"""
    z64 = z.astype(np.float64)
    return z64.sum(axis=1), (z64 * z64).sum(axis=1)


def sum_q_units(z):
    """max over channels of sum z^2 in units of 2^-16 (must stay below 2^53)"""
    return float(totals(z)[1].max() * 65536.0)


def stats(s, q, n, gamma, beta, rm, rv, nbt, momentum=MOMENTUM, eps=BN_EPS):
    """the finalisation, one correctly rounded operation at a time (bnq_kernels.hip:210-225); s, q: [groups, C] doubles.
    Returns ab [groups, 2, C], save [groups, 2, C], running_mean, running_var (None when not given), nbt, var [groups, C]"""
    f32 = np.float32
    groups, C = s.shape
    gm = np.ones(C, f32) if gamma is None else gamma.astype(f32)
    bt = np.zeros(C, f32) if beta is None else beta.astype(f32)
    rm_ = np.zeros(C, f32) if rm is None else rm.astype(f32).copy()
    rv_ = np.zeros(C, f32) if rv is None else rv.astype(f32).copy()
    m, nn = f32(momentum), np.float64(n)
    ab, save, var_all = np.empty((groups, 2, C), f32), np.empty((groups, 2, C), f32), np.empty((groups, C))
    for g in range(groups):
        mean = s[g] / nn
        sq = mean * mean
        var = q[g] / nn - sq
        var = np.where(var < 0, 0.0, var)
        invstd = (1.0 / np.sqrt(var + np.float64(f32(eps)))).astype(f32)
        a = gm * invstd
        meanf = mean.astype(f32)
        prod = meanf * a
        ab[g, 0], ab[g, 1] = a, bt - prod
        save[g, 0], save[g, 1] = meanf, invstd
        t0, t1 = (f32(1.0) - m) * rm_, m * meanf
        rm_ = t0 + t1
        vu = (var * nn / (nn - 1.0)).astype(f32)
        t0, t1 = (f32(1.0) - m) * rv_, m * vu
        rv_ = t0 + t1
        var_all[g] = var
    return dict(ab=ab, save=save, rm=None if rm is None else rm_, rv=None if rv is None else rv_,
                nbt=None if nbt is None else nbt + groups, var=var_all)


def case_stats(case, totals_sq=None):
    s, q = totals(case["z"]) if totals_sq is None else totals_sq
    return stats(s, q, case["P"], case["gamma"], case["beta"], case["rm"], case["rv"], case["nbt"])


# ------------------------------------------------------------------------------------------------ forward outputs
def bn_x(z, ab):
    """x = fma(a, z, b) per slice (float32, the C oracle's single fma)"""
    groups, P, C = z.shape
    return np.stack([O.bn_apply(z[g].reshape(P, C), C, 1, ab[g]).reshape(P, C) for g in range(groups)])


def fwd_ref(z, ab, formula, relu, k, r, res=None):
    """y [groups, P, C] float32 and the level index (clamped at 0 under relu) as int32, from the given (a, b)"""
    x = bn_x(z, ab)
    q, _, bins = O.act_quant_fwd(x, k, r, formula)
    if res is not None:
        q = q + res
    if relu:
        q = np.where(q > 0, q, np.float32(0.0)).astype(np.float32)
        bins = np.maximum(bins, 0)
    return q, bins, x


def mask_ref(y):
    """the one-bit ReLU mask of y [groups, P, C] as uint64 [groups, mask_words] (bnq_kernels.hip:43-53): per chunk of 64
    float4 four words, one per component, bit (i & 63) = [y > 0]; bits beyond nvec are 0"""
    groups = y.shape[0]
    pos = (y.reshape(groups, -1, 4) > 0)
    nvec = pos.shape[1]
    pad = (-nvec) % 64
    pos = np.concatenate([pos, np.zeros((groups, pad, 4), bool)], axis=1).reshape(groups, -1, 64, 4).transpose(0, 1, 3, 2)
    return np.packbits(pos, axis=-1, bitorder="little").reshape(groups, -1).view("<u8")


# ------------------------------------------------------------------------------------------------ backward
def ref_inputs(z, ab, save):
    """(x, zhat, a) in float64 from the float32 values the device's forward left"""
    x = bn_x(z, ab).astype(np.float64)
    zhat = (z.astype(np.float64) - save[:, None, 0, :].astype(np.float64)) * save[:, None, 1, :].astype(np.float64)
    return x, zhat, ab[:, 0, :].astype(np.float64)


def jac64(x, r):
    return r * TWO_OVER_SQRT_2PI * np.exp(-0.5 * x * x)


def proj(dx, zhat, a, k0, k1):
    return a[:, None, :] * (dx - k0 - zhat * k1)


def bwd_ref(g, x, zhat, a, pos, r, from_dx=False, c_exp=None):
    """float64 reference and bars; g, x, zhat: [groups, P, C]; a: [groups, C]; pos: the forward's [y > 0] (None: no ReLU)"""
    c_exp = C_EXP if c_exp is None else c_exp
    g = g.astype(np.float64)
    if from_dx:
        dres, dx, e_dx = None, g, np.zeros_like(g)
    else:
        dres = g if pos is None else np.where(pos, g, 0.0)
        dx = dres * jac64(x, r)
        e_dx = np.abs(dx) * (0.5 * x * x + c_exp) * EPS
    az, adx = np.abs(zhat), np.abs(dx)
    dxz = dx * zhat
    k0, k1 = dx.mean(axis=1, keepdims=True), dxz.mean(axis=1, keepdims=True)
    zk1 = np.abs(zhat * k1)
    e_k0 = e_dx.mean(axis=1, keepdims=True) + np.abs(k0) * EPS
    e_k1 = (e_dx * az).mean(axis=1, keepdims=True) + 2 * EPS * (adx * az).mean(axis=1, keepdims=True) + np.abs(k1) * EPS
    bar_dz = np.abs(a)[:, None, :] * (e_dx + e_k0 + az * e_k1 + 2 * EPS * zk1 + 3 * EPS * (adx + np.abs(k0) + zk1))
    dbeta, dgamma = dx.sum(axis=(0, 1)), dxz.sum(axis=(0, 1))
    return dict(dx=dx, dres=dres, k0=k0, k1=k1, dz=proj(dx, zhat, a, k0, k1), dbeta=dbeta, dgamma=dgamma, bar_dz=bar_dz,
                bar_dbeta=e_dx.sum(axis=(0, 1)) + EPS * np.abs(dbeta),
                bar_dgamma=(e_dx * az).sum(axis=(0, 1)) + 2 * EPS * np.abs(dxz).sum(axis=(0, 1)) + EPS * np.abs(dgamma))


def worst(got, want, bar):
    """max |got - want| / bar; where the bar is 0 the value must be exact (inf otherwise)"""
    err = np.abs(np.asarray(got, np.float64).reshape(want.shape) - want)
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(ratio.max()) if np.isfinite(np.asarray(got)).all() else float("inf")


def emulate32(g, z, ab, save, pos, r, from_dx=False):
    """the kernels' stated operations in float32 (bnq_kernels.hip:128-139, :491-503, :270-280) with an ideal exp2"""
    f32 = np.float32
    a, mean, invstd = ab[:, None, 0, :], save[:, None, 0, :], save[:, None, 1, :]
    P = z.shape[1]
    if from_dx:
        dx = g.astype(f32)
    else:
        x = bn_x(z, ab)
        gm = g if pos is None else np.where(pos, g, f32(0.0)).astype(f32)
        t = (f32(-0.5) * x) * x
        arg = t * f32(1.4426950408889634)
        e = np.exp2(arg.astype(np.float64)).astype(f32)
        dx = gm * ((f32(r) * f32(TWO_OVER_SQRT_2PI)) * e)
    zh = (z - mean) * invstd
    s0, s1 = dx.astype(np.float64).sum(axis=1), (dx.astype(np.float64) * zh.astype(np.float64)).sum(axis=1)
    k0, k1 = (s0 / P).astype(f32)[:, None, :], (s1 / P).astype(f32)[:, None, :]
    d0 = dx - k0
    dz = a * (d0 - zh * k1)
    return dict(dz=dz, dbeta=s0.sum(axis=0).astype(f32), dgamma=s1.sum(axis=0).astype(f32))


def last_partial(P, C, groups):
    """[p0, P): the pixels of the last non-empty partial of the backward's statistics pass (bnq_sums_kernel, :83-84)"""
    np_ = fin_parts(P, C) if fin_small(P, C, groups) else parts_for(P, C)
    per = (P + np_ - 1) // np_
    return ((P - 1) // per) * per


def planted(name, ref, zhat, a, pos, g, x, r, P, C, groups):
    """dz of the float64 reference with one defect planted (None where the defect does not exist on this row)"""
    dx, k0, k1 = ref["dx"], ref["k0"], ref["k1"]
    if name == "projection dropped":
        return a[:, None, :] * dx
    if name == "k1 of the neighbouring channel":
        return proj(dx, zhat, a, k0, np.roll(k1, 1, axis=2))
    if name == "k0 off by 5 %":
        return proj(dx, zhat, a, 1.05 * k0, k1)
    if name == "tail slice with the previous slice's statistics":
        if groups < 2:
            return None
        prev = lambda v: np.concatenate([v[:-1], v[-2:-1]], axis=0)      # noqa: E731
        return proj(dx, zhat, a, prev(k0), prev(k1))
    if name == "mask shifted by one float4":
        if pos is None:
            return None
        dx2 = np.where(np.roll(pos.reshape(groups, -1), 4, axis=1).reshape(pos.shape), g.astype(np.float64), 0.0) * jac64(x, r)
        return proj(dx2, zhat, a, dx2.mean(axis=1, keepdims=True), (dx2 * zhat).mean(axis=1, keepdims=True))
    if name == "last partial skipped":
        p0 = last_partial(P, C, groups)
        return proj(dx, zhat, a, dx[:, :p0].sum(axis=1, keepdims=True) / P, (dx * zhat)[:, :p0].sum(axis=1, keepdims=True) / P)
    raise KeyError(name)


DEFECTS = ["projection dropped", "k1 of the neighbouring channel", "k0 off by 5 %", "tail slice with the previous slice's statistics",
           "mask shifted by one float4", "last partial skipped"]


def exp_units(x, jac, r):
    """the fast exponential's relative error in units of (x^2 / 2 + 1) eps; x float32, jac = act_jac(x, r) from the device"""
    x64 = x.astype(np.float64)
    ref = jac64(x64, r)
    return np.abs(jac.astype(np.float64) - ref) / ref / ((0.5 * x64 * x64 + 1.0) * EPS)
