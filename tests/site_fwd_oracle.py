"""Float64 restatement of the ADMM site's FORWARD, the scale its outputs are checked at, an emulation of the arithmetic the kernel
sources document, and a Python restatement of the forward's dispatch (no GPU).

The site (include/alignq.h, "fused ADMM site"), for x [B,F] and its pre-round transform t = r * erf(x / sqrt 2):

    stats = [mean_x, 1/(std_x + eps), mean_t, 1/(std_t + eps)]   [4][F]   (std unbiased, over the batch)
    corr(v) = Vh Vh^T / F,  Vh = (v - mean_b v) / (std_b v + eps)
    D = corr(t) - corr(x)
    scal = {loss, rho/2/(n rms), 1/n, rms},  n = B^2,  Dm = D - alterD[:B,:B],  rms = sqrt(sum Dm^2 / n),
           loss = mu sum|alterD[:B,:B]| / n + rho/2 rms + sum(gamma[:B,:B] |Dm|) / n

`reference` evaluates that in float64 from the fp32 x and the fp32 t the project specifies (`transform`: tests/oracle_c.py's
act_quant_fwd at k = 32, the table-driven ALIGNQ-ERF32 the device transform is already pinned to bit for bit), so the reference
carries no transform error; folded rows take x = O.bn_apply(z, C, nhwc, ab), the one fma the kernels form.

The scale.  D_ij is a sum of 2 F products divided by F; the root-sum-square of what is added,

    s_ij = sqrt( sum_f (th_if th_jf)^2 + (xh_if xh_jf)^2 ) / F            (about sqrt(2 / F) off the diagonal)

is the size rounding errors of independent terms add up to (`reference`'s "s"; for alignq_corr_fwd only the x half, "s_x").

The emulation.  `emulate_D(x, t, eps, scheme)` follows what each source file's header says it does - the scheme of a kernel is
read there, not inferred from results:
    "split": fp32 mean (true division) and 1/(sqrt(ssq/(B-1)) + eps) from a two-pass fp32 variance, every standardised value split
             into hi = bf16(v), lo = bf16(v - hi), a product evaluated as hi*hi + hi*lo + lo*hi.  site4_kernels.hip ("Split-bf16
             Gram": site_fwd4_kernel, 64 < B <= 128) and site1_kernels.hip ("the 3-term split-bf16 Gram", B <= 32).
    "fp32" : the same statistics, exact fp32 products.  site_kernels.hip ("exact-fp32 MFMA": site_fwd_kernel<2>, 32 < B <= 64) and
             corr_large_kernels.hip ("exact fp32": the blocked Gram, B > 128; its statistics are accumulated in double).
The sums are formed in float64: the emulation does not model the fp32 accumulation nor the slab and tile order.

The bar on D.  BAR_SPLIT and BAR_FP32 are 4 x the worst |emulate_D - D64| / s_ij over the rows of their scheme (the emulation
against the float64 restatement, never a kernel; beyond `cond_allowance`, below), the factor covering what the emulation does not
model, rounded up to two digits.  Measured here (tests/test_site_fwd_oracle_cpu.py recomputes both and asserts
4 x worst <= BAR <= 4.2 x worst):

    split: worst ratio per row 9.8e-6 .. 2.84e-5 of s (the largest at 128 x 32768)          BAR_SPLIT = 1.15e-4
    fp32 : worst ratio per row 3.0e-7 .. 7.9e-7 of s (the largest at 48 x 131136)           BAR_FP32  = 3.2e-6

    |D - D64|_ij <= BAR * s_ij + cond_allowance_ij                                           (`d_bar`)

Ill-conditioned columns.  A column whose samples nearly coincide has a 1/(std + eps) so large that the ROUNDING OF ITS MEAN moves
the standardised values: by d_f = rho_f * (bar on the mean) absolutely, and 1/(std + eps) itself by q_f relatively (the stats bars
below).  That is conditioning of the expression, not arithmetic (tests/site_grad_oracle.py meets the same columns in the backward):
any fp32 evaluation has it, in an amount that depends on the order of the sum.  Where d_f or q_f exceeds ILL = 2^-12 (32 x the
split operand's 2^-17) the column's products are allowed to move as far as those bars let them,
(|a| + d)(|b| + d)(1 + q)^2 - |a||b| (`cond_allowance`); every other column gets nothing.  The inputs here have such columns at
B = 2 only (two draws whose transforms lie within 1.4e-3 of each other: 0.1 % of the columns; the allowance is 5.7e-7 at 2 x 4096
and 2.7e-6 at 2 x 131456, against BAR * s = 1.3e-6 and 2.2e-7), none from B = 5 on.  For the same reason the constant column of
the eps > 0 rows is ZERO: a sum of B equal fp32 numbers c is exact in every order only when every k c, k <= B, is representable, and
where it is not the mean differs from c by an ulp, std is an ulp instead of 0 and 1/(std + eps) falls short of 1/eps by up to 1 %
(measured with c = 0.7: the emulation's D moves by 2e-4 .. 3.6e-3 of s).  t(0) = 0 exactly, so both operands of that column are.

Against the older bar (atol 1e-5 on D).  BAR * s_ij <= 1e-5 / 4 at the worst entry holds on the rows `TIGHTER_THAN_OLD` names (the
CPU test asserts it is exactly that set): every fp32 row (1.1e-6 at most), every split row with F >= 16384, and 2 x 4096.  At
F = 4096 .. 8192 the other split rows hold it off the diagonal only or not quite (worst BAR * s 2.8e-6 .. 4.1e-6: s_ii =
sqrt(6 / F) is the kurtosis of the standardised values), and at F = 70 / 96 no split row can: s grows as 1 / sqrt(F), the split
emulation itself is 1.1e-6 .. 3.7e-6 away from float64 there, so the old absolute bar sits at 3 x the kernels' own error and
BAR * s (9.7e-6 at B = 2, 2.4e-5 .. 4.1e-5 above) is next to or above it.  D is held to BAR * s_ij on every row, the bar the
arithmetic supports; the older tests keep their absolute one.

Planted defects (`DEFECTS`, switches of the emulation) and the margin max_ij |D_defect - D64| / d_bar_ij each reaches on the rows it
applies to (`defects_for`).  At B = 2 and eps = 0 every column's standardised values are +-1/sqrt 2 for both operands whatever x
is, so D = 0 identically and only a defect that breaks that ("t_mean_from_x") applies.  Every margin is at least 4 except the
pairs `NOT_RESOLVING` lists, which the CPU test pins as exactly the set below 4:
    "inv_Fm1" (an error of D_ij / F against BAR sqrt(2 / F)) on every row with F >= 4096 but the three fp32 rows at F = 4096 (57 x
        and more): 0.1 .. 2.5 x the bar, so the condition "F - 1 resolves wherever F <= 4100" is NOT met by the split rows at
        F = 4096 / 4098; above 1 - the test fails, by less than 4 x - at F = 4096 / 4098 / 8192 from B = 28 on
        and on the fp32 rows at F = 131136.  It reaches 48 x and more wherever F <= 384.
    "eps_dropped_t" / "eps_dropped_x" on the split rows at F = 70 / 96 (0.7 .. 0.9): the defect moves the diagonal by 2 eps whatever
        F is, BAR * s_ii is 3e-5 .. 4e-5 there; `stats` resolves it on every row (eps / std = 7e-6 .. 9e-6 relative against a bar
        of (B / 2 + 5) u <= 4.1e-6), and D does by 4.5 x and more from F = 4096 on.
    "last_feature_dropped" on 5 x 131456 (3.1: one feature of 131456 seen by 25 entries).
The measured margins are in NOTES.md ("Site forward at its own scale").

Bars on stats and scal, from u = 2^-24 and the operation counts the kernels state (csrc/Makefile sets no fast-math flag and
-ffp-contract=off: every operation written is one rounding, division included):
    mean    a fp32 sum of B terms in some order, then a true division: every term passes at most B - 1 additions and the division.
            bar = gamma_B * mean_b |v_b|                                      (the blocked Gram's double sum: u |mean| + gamma64)
    rho     ssq = sum (v - m)^2 with the ROUNDED mean m: exactly B (m - mean)^2 more than the centred sum, then per term one
            subtraction, one product and at most B - 1 additions: gamma_{B+2}; times 1/(B-1) (a rounded constant, a product),
            square root, + eps, reciprocal: relative error of rho <= (gamma_{B+4} + B dm^2 / ssq) / 2 + 3 u, dm = the bar on mean.
            A column with ssq = 0 (constant) is excluded at eps = 0 and must be exactly fl(1 / fl(eps)) at eps > 0: its fp32 mean
            is the value itself (a sum of B equal fp32 numbers divided by B - the division is exact whenever the sum is).
    scal    D moves by at most e_ij = d_bar_ij + 2 u |D_ij| (the bar, the product with the rounded 1/F), so
            rms moves by at most |e|_2 / B (triangle inequality), sum gamma |Dm| by sum gamma e.  The three sums are fp32 per lane
            (at most 8 terms), then a 64-lane butterfly (6 levels), then double: with the terms' own roundings gamma_17 relative
            (all three sums have non-negative terms).  loss, c_con, 1/n and rms are rounded to fp32 once.

The dispatch.  `geom`, `form`, `site_fill_slots`, `corrl_ksplit`, `corrl_s_width`, `ws_bytes`, `bwd_ws_bytes` restate
site_internal.h (geom, site_fill_slots), site4_kernels.hip (launch_fwd4_tf, launch_partials4), site_kernels.hip
(alignq_site_ws_bytes) and corr_large_kernels.hip; the CPU test compares them with the library's own queries.
"""
import math

import numpy as np

from tests import oracle_c as O
from tests import site_grad_oracle as G

U = 2.0 ** -24
R, K, MU, RHO = 2.0, 8, 0.2, 0.3
OLD_TOL = 1e-5                   # the bar the older site tests hold D to (atol)
BAR_SPLIT = 1.15e-4              # in units of s_ij; 4 x the emulation's worst ratio (module docstring)
BAR_FP32 = 3.2e-6

DEFECTS = ("inv_Fm1", "eps_dropped_t", "eps_dropped_x", "last_feature_dropped", "last_tile_dropped", "one_slab_dropped",
           "lohi_dropped", "biased_std", "t_mean_from_x")


def gamma(n):
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------------------ dispatch
S1_CAP, KSLAB4 = 1024, 6 * 1024 + 2 * 32 * 33
TAIL_FLOATS = 1024 + 16


def geom(B, F):
    """site_internal.h geom(): dict(nb, tf, n_tiles, grid, slab_floats)"""
    nb = 1 if B <= 32 else (2 if B <= 64 else 4)
    if nb == 4:
        tf = 64 if F > 16 * 256 else 32
        n_tiles = (F + tf - 1) // tf
        cap = 512 if F > 64 * 256 else 256
        return dict(nb=nb, tf=tf, n_tiles=n_tiles, grid=min(n_tiles, cap), slab_floats=KSLAB4)
    n_tiles = (F + 63) // 64
    grid = min(n_tiles, 2048)
    if nb == 1:
        grid = min((F + 127) // 128, S1_CAP)
    return dict(nb=nb, tf=64, n_tiles=n_tiles, grid=grid, slab_floats=(32 * nb) ** 2)


def n_pairs(B):
    nb = (B + 127) // 128
    return nb * (nb + 1) // 2


def corrl_ksplit(B, F):
    """corr_large_kernels.hip corrl_ksplit(): K splits of the blocked Gram's launch"""
    np_, n_tiles = n_pairs(B), (F + 63) // 64
    best, best_cost = 1, 1e30
    for ks in range(1, min(n_tiles, 512) + 1):
        rounds, per_wg = (np_ * ks + 511) // 512, (n_tiles + ks - 1) // ks
        cost = float(rounds * per_wg) + 0.0064 * np_ * ks
        if cost < best_cost:
            best, best_cost = ks, cost
    return best


def corrl_s_width(B):
    nblk = (B + 31) // 32
    rb = (nblk + 3) // 4
    return 256 if rb <= 2 else (512 if rb <= 4 else 1024)


def ws_bytes(B, F):
    """alignq_site_ws_bytes"""
    if 128 < B <= 1024 and F > 0:
        return n_pairs(B) * corrl_ksplit(B, F) * 128 * 128 * 4
    if B < 2 or B > 128 or F <= 0:
        return 0
    g = geom(B, F)
    return (g["grid"] * g["slab_floats"] + TAIL_FLOATS) * 4


def bwd_ws_bytes(B):
    """alignq_site_bwd_ws_bytes"""
    return (B + 31) // 32 * 32 * corrl_s_width(B) * 4 if B > 128 else 2 * 128 * 128 * 4


def site_fill_slots(B, F):
    if B <= 64 or B > 128 or F < 1:
        return 0
    g = geom(B, F)
    return 3 if (g["n_tiles"] <= g["grid"] and g["grid"] <= 128) else 0


def form(B, F, fold=False, aligned=True, pair=True):
    """The forward instantiation a site of B x F selects (launch_partials / launch_partials1 / launch_fwd4_tf / launch_sitel_fwd).
    fold: a folded batch-norm, residual, ReLU or index output; aligned: 16-byte aligned x and x_q (F % 4 == 0 is checked here);
    pair = False: alignq_corr_fwd.  "fwd1-64[-capped]" is site1_fwd64_kernel, which launch_partials1 takes for the site (not for
    corr alone) at B = 28 and B = 32 with a bounded quantiser (k <= 16, |act_range| <= 8): one lane per feature column, a wave per
    64-feature tile, so the ceil(F / 128) workgroups hold twice the tiles there are (the upper half of the slabs is zero) and
    its waves loop only beyond 4 * 1024 tiles, F > 262144."""
    if B > 128:
        return "large-ks1" if corrl_ksplit(B, F) == 1 else "large-ksN"
    g = geom(B, F)
    if g["nb"] == 1:
        if pair and B in (28, 32):
            return "fwd1-64-capped" if (F + 63) // 64 > 4 * g["grid"] else "fwd1-64"
        return "fwd1-capped" if (F + 127) // 128 > g["grid"] else "fwd1"
    if g["nb"] == 2:
        return "fwd2-capped" if g["n_tiles"] > g["grid"] else "fwd2"
    al = aligned and F % 4 == 0
    if g["n_tiles"] <= g["grid"]:
        full = B == 128 and F % g["tf"] == 0 and al
        return f"fwd4-{g['tf']}" + ("-full" if full else "")
    assert g["tf"] == 64
    # the 512-thread loop: the plain SITE over complete tiles; corr alone runs the 1024-thread loop (launch_fwd4_tf says why)
    return "fwd4-loop512" if (pair and B == 128 and F % 64 == 0 and al and not fold) else "fwd4-loopNT"


def scheme_of(name):
    """which arithmetic the form's source file documents (module docstring)"""
    return "fp32" if name.startswith(("fwd2", "large")) else "split"


def bar_of(name):
    return BAR_FP32 if scheme_of(name) == "fp32" else BAR_SPLIT


def mirrored(name):
    """the forms whose source promises a mirrored store of the off-diagonal part (site4's packed triangle: every i != j; the
    blocked Gram: the off-diagonal 128 x 128 blocks)"""
    return name.startswith(("fwd4", "large"))


def slab_features(B, F):
    """(features per slab unit, grid) of the partial Gram: unit u of `features` consecutive columns goes to slab u % grid"""
    if B > 128:
        ks = corrl_ksplit(B, F)
        per = ((F + 63) // 64 + ks - 1) // ks
        return 64 * per, ks               # contiguous K ranges: handled by `slab_of`
    g = geom(B, F)
    if g["nb"] == 1:
        return (256 if B in (28, 32) else 128), g["grid"]        # four waves of 64- (site1_fwd64_kernel) or 32-feature sub-tiles
    return g["tf"], g["grid"]


def slab_of(B, F):
    """slab index of every feature column"""
    feat, grid = slab_features(B, F)
    unit = np.arange(F) // feat
    return unit if B > 128 else unit % grid


# ------------------------------------------------------------------------------------------------------------ the matrix
# (name of the form, B, F, aligned): one row per form at the smallest shape that selects it.  eps = G.plain_eps(B), inputs
# G.plain_inputs(B, F); on the eps > 0 rows column F // 3 is made constant.
def _rows():
    rows = []
    for B in (2, 5):                     # site1: ragged (one partly filled workgroup), aligned, 1027 workgroups' worth over the cap
        rows += [("fwd1", B, 70, True), ("fwd1", B, 4096, True), ("fwd1-capped", B, 131072 + 384, True)]
    for B in (28, 32):                   # site1_fwd64_kernel: the same three (none of them loops), and 4099 tiles on 4096 waves
        rows += [("fwd1-64", B, 70, True), ("fwd1-64", B, 4096, True), ("fwd1-64", B, 131072 + 384, True),
                 ("fwd1-64-capped", B, 262144 + 192, True)]
    for B in (33, 48, 64):               # site_fwd_kernel<2>: ragged, aligned, 2049 tiles over the 2048 cap
        rows += [("fwd2", B, 70, True), ("fwd2", B, 4096, True), ("fwd2-capped", B, 131072 + 64, True)]
    for B in (65, 100, 128):
        full = "-full" if B == 128 else ""
        rows += [("fwd4-32" + full, B, 96, True),            # 32-feature tiles, three of them
                 ("fwd4-32" + full, B, 4096, True),          # 128 tiles, complete only at B = 128
                 ("fwd4-64", B, 4098, True),                 # 64-feature tiles, scalar loads (F % 4 != 0), ragged
                 ("fwd4-64" + full, B, 8192, True),
                 ("fwd4-64" + full, B, 16384, True),         # 256 tiles
                 ("fwd4-64" + full, B, 32768, True),         # 512 one-tile workgroups
                 ("fwd4-loop512" if B == 128 else "fwd4-loopNT", B, 32832, True),      # 513 tiles on 512 workgroups
                 ("fwd4-loopNT", B, 32834, True),            # ragged loop
                 ("fwd4-32", B, 4096, False)]                # behind a base pointer offset by 4 bytes
    rows += [("large-ks1", 130, 40, True), ("large-ksN", 130, 70, True), ("large-ksN", 192, 384, True),
             ("large-ksN", 300, 72, True), ("large-ksN", 513, 72, True), ("large-ksN", 1024, 136, True)]
    return rows


ROWS = _rows()
FOLD_LOOP = (128, 16, 48)                # one looped folded row: F = 36864, 576 tiles on 512 workgroups


def row_id(row):
    name, B, F, aligned = row
    return f"{name}-{B}x{F}" + ("" if aligned else "+4bytes")


def row_inputs(B, F):
    """x (G.plain_inputs), eps (G.plain_eps) and the constant column (or None)"""
    x, _ = G.plain_inputs(B, F)
    eps = G.plain_eps(B)
    const = None
    if eps > 0:
        const = F // 3
        x = x.copy()
        x[:, const] = np.float32(0.0)      # the one constant every partial sum of which is exact in any order (module docstring)
    return x, eps, const


def transform(x, r=R):
    """the fp32 pre-round transform t as the C oracle forms it"""
    return O.act_quant_fwd(x, 32, r, O.FORMULA_ADMM)[1]


# ------------------------------------------------------------------------------------------------------------ float64 statement
def _standardise(v, eps):
    mu = v.mean(0)
    sd = v.std(0, ddof=1)
    with np.errstate(divide="ignore"):
        rho = 1.0 / (sd + eps)
    vh = (v - mu) * np.where(np.isfinite(rho), rho, 0.0)
    return mu, rho, vh


def reference(x, t, eps):
    """dict(stats [4,F], D, s, corr_x, s_x), float64, from the fp32 x and t [B,F]"""
    x64 = np.asarray(x, np.float64).reshape(x.shape[0], -1)
    t64 = np.asarray(t, np.float64).reshape(x64.shape)
    F = x64.shape[1]
    mx, rx, xh = _standardise(x64, eps)
    mt, rt, th = _standardise(t64, eps)
    cx, ct = xh @ xh.T / F, th @ th.T / F
    x2, t2 = xh * xh, th * th
    sx2, st2 = x2 @ x2.T, t2 @ t2.T
    return dict(stats=np.stack([mx, rx, mt, rt]), D=ct - cx, s=np.sqrt(sx2 + st2) / F, corr_x=cx, s_x=np.sqrt(sx2) / F)


def scal_reference(D, A, Gm, mu=MU, rho=RHO):
    """scal [4] (float64) as include/alignq.h states it"""
    B = D.shape[0]
    n = float(B * B)
    A, Gm = np.asarray(A, np.float64)[:B, :B], np.asarray(Gm, np.float64)[:B, :B]
    Dm = np.asarray(D, np.float64) - A
    rms = math.sqrt((Dm * Dm).sum() / n)
    loss = mu * np.abs(A).sum() / n + 0.5 * rho * rms + (Gm * np.abs(Dm)).sum() / n
    return np.array([loss, 0.5 * rho / (n * rms), 1.0 / n, rms])


# ------------------------------------------------------------------------------------------------------------ bars
def stats_bars(x, t, eps, acc="fp32"):
    """(bar [4,F] absolute, live [F]): the bar on every entry of stats and the columns it applies to; a constant column is not
    live (excluded at eps = 0, exactly 1/eps at eps > 0: `const_rho`).  acc: "fp32", or "fp64" for the blocked Gram's sums."""
    out, live = [], None
    for v in (x, t):
        v = np.asarray(v, np.float64).reshape(v.shape[0], -1)
        B = v.shape[0]
        mu = v.mean(0)
        ssq = ((v - mu) ** 2).sum(0)
        sd = np.sqrt(ssq / (B - 1))
        ok = ssq > 0
        live = ok if live is None else (live & ok)
        if acc == "fp32":
            dm = gamma(B) * np.abs(v).mean(0)
            rel_ssq = gamma(B + 4) + B * dm * dm / np.where(ok, ssq, 1.0)
        else:                            # double sums s, q; var = (q - s mean) / (B - 1): cancellation at 2^-53 of q
            dm = U * np.abs(mu) + (B + 1) * 2.0 ** -53 * np.abs(v).mean(0)
            rel_ssq = (B + 4) * 2.0 ** -52 * (v * v).sum(0) / np.where(ok, ssq, 1.0)
        rho = 1.0 / (np.where(ok, sd, 1.0) + eps)
        out += [dm, rho * (0.5 * rel_ssq + 3 * U)]
    return np.stack(out), live


ILL = 2.0 ** -12       # a column is ill-conditioned when the statistics' own bar moves its standardised values by more than this


def cond_allowance(x, t, eps, acc="fp32"):
    """[B,B]: what the ROUNDED statistics may add to |D - D64| through the ill-conditioned columns (module docstring): with
    d = rho * (bar on the mean) and q = (bar on rho) / rho, a product a b of standardised values becomes at most
    (|a| + d)(|b| + d)(1 + q)^2; summed over the columns where d or q exceeds ILL, for both operands, divided by F."""
    bars, _ = stats_bars(x, t, eps, acc)
    B = x.shape[0]
    out = np.zeros((B, B))
    for i, v in enumerate((x, t)):
        v = np.asarray(v, np.float64).reshape(B, -1)
        _, rho, vh = _standardise(v, eps)
        rho = np.where(np.isfinite(rho), rho, 0.0)
        d = rho * bars[2 * i]
        q = bars[2 * i + 1] / np.where(rho > 0, rho, 1.0)
        ill = (d > ILL) | (q > ILL)
        if ill.any():
            a = np.abs(vh[:, ill])
            p = (a + d[ill]) * (1.0 + q[ill])
            out += p @ p.T - a @ a.T
    return out / v.shape[1]


def const_rho(eps):
    """what a constant column's 1/(std + eps) must be at eps > 0, bit for bit"""
    return np.float32(1.0) / np.float32(eps)


def scal_bars(D64, dbar, A, Gm, mu=MU, rho=RHO):
    """bar [4] (absolute) on scal: D's bar dbar [B,B] (`d_bar`) pushed through the loss (module docstring)"""
    B = D64.shape[0]
    n = float(B * B)
    A, Gm = np.asarray(A, np.float64)[:B, :B], np.asarray(Gm, np.float64)[:B, :B]
    e = dbar + 2 * U * np.abs(D64)
    ref = scal_reference(D64, A, Gm, mu, rho)
    rms = ref[3]
    g17 = gamma(17)
    d_rms = math.sqrt((e * e).sum()) / B + 0.5 * g17 * rms
    d_loss = (mu * g17 * np.abs(A).sum() / n + 0.5 * rho * d_rms + ((Gm * e).sum() + g17 * (Gm * np.abs(D64 - A)).sum()) / n
              + U * abs(ref[0]))
    return np.array([d_loss, ref[1] * (d_rms / rms + U), U * ref[2], d_rms + U * rms])


# ------------------------------------------------------------------------------------------------------------ emulation
def _bf16(v):
    """round fp32 to bf16 (nearest even), returned as fp32"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000))
    return r.view(np.float32)


def _stats32(v, eps, biased=False, mean_from=None, drop_eps=False, acc="fp32"):
    """the documented statistics: fp32 mean by true division, two-pass fp32 variance, rho = 1 / (sqrt(ssq / (B - 1)) + eps); acc =
    "fp64" (the blocked Gram's sweep): sum and sum of squares in double, var = (q - s mean) / (B - 1), mean and sqrt(var) rounded"""
    B = v.shape[0]
    f = np.float32
    nb = B if biased else B - 1
    if acc == "fp64":
        v64 = v.astype(np.float64)
        a, q = v64.sum(0), (v64 * v64).sum(0)
        mean = a / B
        m = mean.astype(f) if mean_from is None else mean_from
        sd = np.sqrt(np.maximum((q - a * mean) / nb, 0.0)).astype(f)
        d = (v - m).astype(f)
    else:
        m = (v.sum(0, dtype=f) / f(B)).astype(f) if mean_from is None else mean_from
        d = (v - m).astype(f)
        ssq = (d * d).sum(0, dtype=f)
        sd = np.sqrt(ssq * (f(1.0) / f(nb))).astype(f)
    with np.errstate(divide="ignore"):
        rho = (f(1.0) / (sd + (f(0.0) if drop_eps else f(eps)))).astype(f)
    rho = np.where(np.isfinite(rho), rho, f(0.0)).astype(f)
    return m, rho, (d * rho).astype(f)


def _gram(vh, scheme, lohi=True):
    if scheme == "fp32":
        v = vh.astype(np.float64)
        return v @ v.T
    hi = _bf16(vh)
    lo = _bf16((vh - hi).astype(np.float32))
    h, l_ = hi.astype(np.float64), lo.astype(np.float64)
    g = h @ h.T + h @ l_.T
    return g + l_ @ h.T if lohi else g


def emulate_D(x, t, eps, scheme, defect=None, B_F=None):
    """D [B,B] (float64 sums of the documented operand arithmetic).  defect: one of DEFECTS; B_F = (B, F) of the launch whose
    tiling the tile and slab defects follow (default: x's own shape)."""
    assert scheme in ("split", "fp32") and (defect is None or defect in DEFECTS)
    x = np.ascontiguousarray(x, np.float32).reshape(x.shape[0], -1)
    t = np.ascontiguousarray(t, np.float32).reshape(x.shape)
    B, F = x.shape if B_F is None else B_F
    biased = defect == "biased_std"
    acc = acc_of(B)
    mx, _, xh = _stats32(x, eps, biased, drop_eps=defect == "eps_dropped_x", acc=acc)
    _, _, th = _stats32(t, eps, biased, mean_from=mx if defect == "t_mean_from_x" else None, drop_eps=defect == "eps_dropped_t",
                        acc=acc)
    keep = np.ones(x.shape[1], bool)
    if defect == "last_feature_dropped":
        keep[-1] = False
    elif defect == "last_tile_dropped":
        feat = slab_features(B, F)[0] if B <= 128 else 64
        keep[(x.shape[1] - 1) // feat * feat:] = False
    elif defect == "one_slab_dropped":
        sl = slab_of(B, F)[:x.shape[1]]
        keep[sl == sl.max()] = False
    if not keep.all():
        xh, th = xh[:, keep], th[:, keep]
    lohi = defect != "lohi_dropped"
    return (_gram(th, scheme, lohi) - _gram(xh, scheme, lohi)) / (F - 1 if defect == "inv_Fm1" else F)


def defects_for(name, B, eps):
    """the planted defects that apply to a row: eps only where there is one, a dropped slab where a workgroup holds more than one
    tile (capped and looped rows, and the blocked Gram's K split), the lo*hi term on the split rows"""
    if B == 2 and eps == 0:           # D = 0 identically (module docstring)
        return ["t_mean_from_x"]
    out = ["inv_Fm1", "last_feature_dropped", "last_tile_dropped", "biased_std", "t_mean_from_x"]
    if eps > 0:
        out += ["eps_dropped_t", "eps_dropped_x"]
    if name.endswith("capped") or "loop" in name or name == "large-ksN":
        out.append("one_slab_dropped")
    if scheme_of(name) == "split":
        out.append("lohi_dropped")
    return out


def ratio(D, ref, s):
    """max_ij |D - ref| / s_ij"""
    return float((np.abs(np.asarray(D, np.float64) - ref) / s).max())


def acc_of(B):
    """the precision the statistics' sums are formed in: double in the blocked Gram's sweep, fp32 elsewhere"""
    return "fp64" if B > 128 else "fp32"


def d_bar(name, ref, allowance, half="s"):
    """the bar on every entry of D (half = "s_x": of alignq_corr_fwd's corr(x))"""
    return bar_of(name) * ref[half] + allowance


def acc_depth(B, F):
    """additions a product passes on its way into an entry of the Gram, one rounding per matrix instruction: the K steps of a
    workgroup's (wave's) tiles, the K halves / waves combined, the slab reduction (16 groups of every 16th slab, then the 16
    groups) and the scale by 1/F"""
    if B > 128:
        ks = corrl_ksplit(B, F)
        return ((F + 63) // 64 + ks - 1) // ks * 32 + ks + 1
    g = geom(B, F)
    red = (g["grid"] + 15) // 16 + 16 + 1
    if g["nb"] == 4:
        return (g["n_tiles"] + g["grid"] - 1) // g["grid"] * (g["tf"] // 16 * 3) + 1 + red
    if g["nb"] == 2:
        return (g["n_tiles"] + g["grid"] - 1) // g["grid"] * 32 + red
    waves = 4 * g["grid"]
    return ((F + 31) // 32 + waves - 1) // waves * 6 + 4 + red


def corr_bar(name, ref, B, F):
    """the bar on every entry of alignq_corr_fwd's corr(x): BAR * s_x (the x half of the scale) plus what a sum that does NOT
    cancel adds.  D's two Grams share one accumulator and their diagonals (both about 1) cancel in it; corr(x) alone keeps a
    diagonal of (B - 1) / B, so (a) the fp32 accumulation, whose every addition rounds at u |partial sum|, is
    gamma_depth * |corr_ij| instead of a random walk at the size of s, and (b) on the split forms the lo * lo term the kernel
    drops ("< 2^-16 relative", site4_kernels.hip) has ONE sign on the diagonal, lo_i^2: 2^-16 |corr_ij|.  Off the diagonal
    both additions are a few percent of BAR * s."""
    extra = gamma(acc_depth(B, F)) + (2.0 ** -16 if scheme_of(name) == "split" else 0.0)
    return bar_of(name) * ref["s_x"] + extra * np.abs(ref["corr_x"])


def emulate_corr(x, eps, scheme):
    """corr(x) alone by the documented operand arithmetic (float64 sums)"""
    x = np.ascontiguousarray(x, np.float32).reshape(x.shape[0], -1)
    _, _, xh = _stats32(x, eps, acc=acc_of(x.shape[0]))
    return _gram(xh, scheme) / x.shape[1]


# alignq_corr_fwd (no transform, one operand): one row per geometry
CORR_ROWS = [("fwd1", 28, 70), ("fwd1-capped", 5, 131072 + 384), ("fwd2", 48, 4096), ("fwd4-32", 100, 96), ("fwd4-64", 65, 4098),
             ("fwd4-64-full", 128, 8192), ("fwd4-loopNT", 128, 32832), ("large-ksN", 300, 72)]

_MEASURED = {}


def measure(row):
    """The emulation against the float64 restatement on one row of the matrix (cached; never a kernel): dict(ratio = worst
    (|emulate_D - D64| - allowance)+ / s, bar_max = worst BAR * s, bar_max_off = the same off the diagonal, allowance_max,
    emu_abs = worst |emulate_D - D64|, rms_D, margins = {defect: worst |D_defect - D64| / d_bar})."""
    if row not in _MEASURED:
        name, B, F, _ = row
        x, eps, _ = row_inputs(B, F)
        t = transform(x)
        ref = reference(x, t, eps)
        al = cond_allowance(x, t, eps, acc_of(B))
        sch = scheme_of(name)
        err = np.abs(emulate_D(x, t, eps, sch) - ref["D"])
        bar = d_bar(name, ref, al)
        bs = bar_of(name) * ref["s"]
        margins = {d: float((np.abs(emulate_D(x, t, eps, sch, d) - ref["D"]) / bar).max()) for d in defects_for(name, B, eps)}
        _MEASURED[row] = dict(ratio=float((np.maximum(err - al, 0.0) / ref["s"]).max()), bar_max=float(bs.max()),
                              bar_max_off=float((bs - np.diag(np.diag(bs))).max()), allowance_max=float(al.max()),
                              emu_abs=float(err.max()), rms_D=float(np.sqrt((ref["D"] ** 2).mean())), margins=margins)
    return _MEASURED[row]


def aligned_rows():
    """the rows of the matrix by shape (an offset base pointer changes the access form, not the arithmetic)"""
    return [r for r in ROWS if r[3]]


# (row id, defect) pairs whose margin stays below 4 (module docstring); the CPU test asserts this is exactly that set
NOT_RESOLVING = {
    'fwd1-5x4096': ('inv_Fm1',),
    'fwd1-capped-5x131456': ('inv_Fm1', 'last_feature_dropped'),
    'fwd1-64-28x70': ('eps_dropped_t', 'eps_dropped_x'),
    'fwd1-64-28x4096': ('inv_Fm1',),
    'fwd1-64-28x131456': ('inv_Fm1',),
    'fwd1-64-capped-28x262336': ('inv_Fm1',),
    'fwd1-64-32x70': ('eps_dropped_t', 'eps_dropped_x'),
    'fwd1-64-32x4096': ('inv_Fm1',),
    'fwd1-64-32x131456': ('inv_Fm1',),
    'fwd1-64-capped-32x262336': ('inv_Fm1',),
    'fwd2-capped-33x131136': ('inv_Fm1',),
    'fwd2-capped-48x131136': ('inv_Fm1',),
    'fwd2-capped-64x131136': ('inv_Fm1',),
    'fwd4-32-65x4096': ('inv_Fm1',),
    'fwd4-64-65x4098': ('inv_Fm1',),
    'fwd4-64-65x8192': ('inv_Fm1',),
    'fwd4-64-65x16384': ('inv_Fm1',),
    'fwd4-64-65x32768': ('inv_Fm1',),
    'fwd4-loopNT-65x32832': ('inv_Fm1',),
    'fwd4-loopNT-65x32834': ('inv_Fm1',),
    'fwd4-32-100x96': ('eps_dropped_t', 'eps_dropped_x'),
    'fwd4-32-100x4096': ('inv_Fm1',),
    'fwd4-64-100x4098': ('inv_Fm1',),
    'fwd4-64-100x8192': ('inv_Fm1',),
    'fwd4-64-100x16384': ('inv_Fm1',),
    'fwd4-64-100x32768': ('inv_Fm1',),
    'fwd4-loopNT-100x32832': ('inv_Fm1',),
    'fwd4-loopNT-100x32834': ('inv_Fm1',),
    'fwd4-32-full-128x96': ('eps_dropped_t', 'eps_dropped_x'),
    'fwd4-32-full-128x4096': ('inv_Fm1',),
    'fwd4-64-128x4098': ('inv_Fm1',),
    'fwd4-64-full-128x8192': ('inv_Fm1',),
    'fwd4-64-full-128x16384': ('inv_Fm1',),
    'fwd4-64-full-128x32768': ('inv_Fm1',),
    'fwd4-loop512-128x32832': ('inv_Fm1',),
    'fwd4-loopNT-128x32834': ('inv_Fm1',),
}
# rows on which BAR * s_ij <= OLD_TOL / 4 at the worst entry (module docstring)
TIGHTER_THAN_OLD = frozenset((
    'fwd1-2x4096',
    'fwd1-capped-2x131456',
    'fwd1-capped-5x131456',
    'fwd1-64-28x131456',
    'fwd1-64-capped-28x262336',
    'fwd1-64-32x131456',
    'fwd1-64-capped-32x262336',
    'fwd2-33x70',
    'fwd2-33x4096',
    'fwd2-capped-33x131136',
    'fwd2-48x70',
    'fwd2-48x4096',
    'fwd2-capped-48x131136',
    'fwd2-64x70',
    'fwd2-64x4096',
    'fwd2-capped-64x131136',
    'fwd4-64-65x16384',
    'fwd4-64-65x32768',
    'fwd4-loopNT-65x32832',
    'fwd4-loopNT-65x32834',
    'fwd4-64-100x16384',
    'fwd4-64-100x32768',
    'fwd4-loopNT-100x32832',
    'fwd4-loopNT-100x32834',
    'fwd4-64-full-128x16384',
    'fwd4-64-full-128x32768',
    'fwd4-loop512-128x32832',
    'fwd4-loopNT-128x32834',
    'large-ks1-130x40',
    'large-ksN-130x70',
    'large-ksN-192x384',
    'large-ksN-300x72',
    'large-ksN-513x72',
    'large-ksN-1024x136',
))
