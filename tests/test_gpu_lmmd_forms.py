"""The LMMD kernels (csrc/lmmd_kernels.hip: alignq_lmmd_fwd / _bwd) through the C ABI, one row per regime of geometry(): a single
ragged chunk (D < 256), one chunk per slice (D <= 4096, the last slice short), several chunks per slice with a short last slice
(D > 4096); C and kernel_num at 1 and at their caps, a ragged last 16-row tile, a fixed bandwidth.  Reference:
tests.test_dsan_cpu.run_restated in float64; bars: the project's own (tests/test_gpu_dsan.py), loss within 1e-5 |ref|, each gradient
within 1e-5 max |ref gradient|; inputs as test_hip_lmmd_sweep_against_restatement makes them, seed 1000 B + D.  loss, dx_src,
dx_tgt and the workspace lie in NaN-filled windows between sentinel guards, g = 0.37 is read from device memory, a second forward +
backward must give the same bits, and mmd.lmmd / mmd.lmmd_pair must give the bits of the direct launches.  Then the edges, each at a
ragged D: no common class, identical rows (the NaN guard) with the data and with a fixed bandwidth, a zero probability column, a tie
in a target row's maximum, source labels outside [0, C).

Measured on an MI355X (error / bar of loss, dx_src, dx_tgt):
    2x1x1-k5                   .0164 .0085 .0084
    2x3x2-k5                   .0038 .0186 .0110
    3x255x31-k5                .0079 .0137 .0123
    16x256x31-k1               .0027 .0315 .0258
    17x257x64-k8               .0019 .0584 .0720
    33x4096x31-k5              .0043 .0328 .0418
    5x4097x31-k4               .0015 .0303 .0237
    64x4352x64-k5              .0006 .0380 .0649
    8x8200x31-k5               .0025 .0221 .0378
    64x300x5-k5                .0123 .0514 .0723
    32x66000x31-k5             .0044 .0391 .0751
    zero column, D 255         .0003 .0482 .0489
    zero column, D 4097        .0020 .0256 .0284
    tie, D 255                 .0030 .0153 .0129
    tie, D 4097                .0014 .0199 .0216
    labels -4 and C, D 255     .0085 .0302 .0283
    labels -4 and C, D 4097    .0086 .0173 .0232
Libraries with one planted defect each (lmmd_l2_kernel summing c < len - 1; the finishing kernel summing splits - 1 slices) failed 17 of
the 22 GPU cases here each: every row and every live edge; the not-live edges and the geometry check cannot see them.
"""
import numpy as np
import pytest
import torch

from tests.test_dsan_cpu import run_restated
from tests.test_gpu_dwconv import SENTINEL, Arena

pytestmark = pytest.mark.gpu
G = 0.37

# (B, D, C, kernel_mul, kernel_num, fix_sigma / D or None): what the row selects
ROWS = [
    ((2, 1, 1, 2.0, 5, None), "smallest case"),
    ((2, 3, 2, 2.0, 5, None), "D < 256"),
    ((3, 255, 31, 2.0, 5, None), "one chunk, one feature short"),
    ((16, 256, 31, 2.0, 1, None), "a single kernel"),
    ((17, 257, 64, 1.5, 8, None), "two slices, the second of one feature; C and kernel_num at their caps; 34 rows = three 16-row tiles"),
    ((33, 4096, 31, 2.0, 5, None), "16 slices of one chunk"),
    ((5, 4097, 31, 2.0, 4, None), "17 chunks, two per slice, nine slices, the last of one feature; even kernel_num"),
    ((64, 4352, 64, 2.0, 5, None), "the widest case, every cap at once"),
    ((8, 8200, 31, 2.0, 5, 1.7), "fixed bandwidth 1.7 D"),
    ((64, 300, 5, 2.0, 5, None), "many rows per class"),
    ((32, 66000, 31, 2.0, 5, None), "258 chunks, 17 per slice"),
]
ROW_IDS = ["x".join(str(v) for v in r[:3]) + f"-k{r[4]}" for r, _ in ROWS]


def geometry(B, D):
    """lmmd_kernels.hip: geometry() restated: (chunks, chunks per slice, slices)"""
    chunks = -(-D // 256)
    cps = -(-chunks // 16)
    return chunks, cps, -(-chunks // cps)


def test_rows_select_the_regimes_their_comments_claim():
    g = {r[:2]: geometry(*r[:2]) for r, _ in ROWS}
    assert g[(2, 1)] == g[(2, 3)] == g[(3, 255)] == g[(16, 256)] == (1, 1, 1)
    assert g[(17, 257)] == (2, 1, 2) and 257 - 256 == 1 and -(-34 // 16) == 3 and 34 % 16
    assert g[(33, 4096)] == (16, 1, 16)
    assert g[(5, 4097)] == (17, 2, 9) and 4097 - 8 * 512 == 1
    assert g[(64, 4352)] == (17, 2, 9) and g[(8, 8200)] == (33, 3, 11)
    assert g[(32, 66000)] == (258, 17, 16) and 66000 - 15 * 17 * 256 < 17 * 256
    assert {r[2] for r, _ in ROWS} >= {1, 64} and {r[4] for r, _ in ROWS} >= {1, 4, 8}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def make_inputs(B, D, C, seed=None):
    """test_hip_lmmd_sweep_against_restatement's recipe"""
    rng = np.random.default_rng(1000 * B + D if seed is None else seed)
    xs = (rng.standard_normal((B, D)) * 0.7 + 0.05).astype(np.float32)
    xt = (rng.standard_normal((B, D)) * 1.2 - 0.1).astype(np.float32)
    ys = rng.integers(0, C, B).astype(np.int64)
    logits = rng.standard_normal((B, C)) * 2.0
    logits[0, ys[0]] += 10.0                                  # at least one class in common
    p = np.exp(logits - logits.max(1, keepdims=True))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    return xs, xt, ys, p


class Launch:
    """alignq_lmmd_fwd + alignq_lmmd_bwd on one case; windows: loss, dx_src, dx_tgt, workspace"""

    def __init__(self, dev, case):
        from alignq_amd import _lib as L
        self.L, self.lib, self.dev, self.case = L, L.load(), dev, case
        self.B, self.D = case["xs"].shape
        self.C = case["p"].shape[1]
        self.ws_bytes = int(self.lib.alignq_lmmd_ws_bytes(self.B, self.D))
        n = 2 * self.B
        chunks, cps, splits = geometry(self.B, self.D)
        a256 = lambda b: (b + 255) // 256 * 256
        assert self.ws_bytes == a256(splits * n * n * 4) + a256(n * n * 4) + 256
        self.arena = Arena(dev, [1, self.B * self.D, self.B * self.D, self.ws_bytes // 4])
        self.xs, self.xt, self.ys, self.p = (cu(case[k], dev) for k in ("xs", "xt", "ys", "p"))
        self.g = torch.tensor([G], dtype=torch.float32, device=dev)

    def run(self):
        """returns loss [1], dx_src, dx_tgt [B, D] and the workspace's flags (live, m)"""
        c = self.case
        self.arena.reset()
        loss, dxs, dxt, ws = self.arena.views
        assert ws.data_ptr() % 16 == 0
        st = self.L.stream_ptr()
        rc = self.lib.alignq_lmmd_fwd(self.xs.data_ptr(), self.xt.data_ptr(), self.ys.data_ptr(), self.p.data_ptr(), self.B, self.D,
                                      self.C, float(c["kernel_mul"]), int(c["kernel_num"]), float(c["fix_sigma"] or 0.0), loss.data_ptr(),
                                      ws.data_ptr(), st)
        assert rc == 0, rc
        rc = self.lib.alignq_lmmd_bwd(self.g.data_ptr(), self.xs.data_ptr(), self.xt.data_ptr(), ws.data_ptr(), self.B, self.D,
                                      dxs.data_ptr(), dxt.data_ptr(), st)
        torch.cuda.synchronize()
        assert rc == 0, rc
        loss, dxs, dxt, ws = self.arena.get()                                   # (asserts the guards)
        for name, a in (("loss", loss), ("dx_src", dxs), ("dx_tgt", dxt)):
            assert (bits(a) != SENTINEL).all(), f"{name} has unwritten elements"
        flags = ws.view(np.int32)[self.ws_bytes // 4 - 64:][:2]
        return loss, dxs.reshape(self.B, self.D), dxt.reshape(self.B, self.D), (int(flags[0]), int(flags[1]))

    def twice(self):
        a, b = self.run(), self.run()
        assert same(a[0], b[0]) and same(a[1], b[1]) and same(a[2], b[2]) and a[3] == b[3], "second forward + backward differs"
        return a

    def through_autograd(self, pair):
        from alignq_amd import mmd
        c = self.case
        args = (self.ys, self.p, c["kernel_mul"], c["kernel_num"], c["fix_sigma"])
        if pair:
            x = torch.cat([self.xs, self.xt]).requires_grad_(True)
            loss = mmd.lmmd_pair(x, *args)
            (loss * self.g).backward()
            return loss.detach().cpu().numpy(), x.grad[:self.B].cpu().numpy(), x.grad[self.B:].cpu().numpy()
        s, t = self.xs.clone().requires_grad_(True), self.xt.clone().requires_grad_(True)
        loss = mmd.lmmd(s, t, *args)
        (loss * self.g).backward()
        return loss.detach().cpu().numpy(), s.grad.cpu().numpy(), t.grad.cpu().numpy()


def against_restatement(tag, got, case):
    """prints error / bar of (loss, dx_src, dx_tgt), then asserts the three"""
    loss, ds, dt, _ = got
    ref, rds, rdt = run_restated(case, torch.float64)
    assert ref[0] != 0.0
    e = [abs(float(loss[0]) - ref[0]) / (1e-5 * abs(ref[0])),
         float(np.abs(ds - G * rds).max() / (1e-5 * np.abs(G * rds).max())),
         float(np.abs(dt - G * rdt).max() / (1e-5 * np.abs(G * rdt).max()))]
    print(f"[lmmd-forms] {tag}: error / bar  loss {e[0]:.4f}  dx_src {e[1]:.4f}  dx_tgt {e[2]:.4f}")
    assert max(e) <= 1.0, (tag, e)


@pytest.mark.parametrize("i", range(len(ROWS)), ids=ROW_IDS)
def test_rows_against_the_float64_restatement(dev, i):
    (B, D, C, mul, num, fix), _ = ROWS[i]
    xs, xt, ys, p = make_inputs(B, D, C)
    case = dict(xs=xs, xt=xt, ys=ys, p=p, kernel_mul=mul, kernel_num=num, fix_sigma=None if fix is None else fix * D)
    run = Launch(dev, case)
    got = run.twice()
    assert got[3][0] == 1 and got[3][1] >= 1                     # live, at least the forced common class
    plain, pair = run.through_autograd(False), run.through_autograd(True)
    for a, b, c in zip(got[:3], plain, pair):
        assert same(a, b), "mmd.lmmd differs from the direct launches"
        assert same(b, c), "mmd.lmmd_pair differs from mmd.lmmd"
    against_restatement(ROW_IDS[i], got, case)


# ------------------------------------------------------------------------------------------------ edges, each at a ragged D
def _case(xs, xt, ys, p, fix_sigma=None):
    return dict(xs=xs, xt=xt, ys=ys, p=p, kernel_mul=2.0, kernel_num=5, fix_sigma=fix_sigma)


def _dead(got):
    loss, ds, dt, flags = got
    assert flags[0] == 0 and bits(loss)[0] == 0, "the loss must be exactly +0 and the workspace not live"
    for d in (ds, dt):
        assert not np.isnan(d).any() and not d.any(), "a not-live loss must give exact zero gradients over the full width"


@pytest.mark.parametrize("D", [255, 4097])
def test_no_common_class(dev, D):
    B, C = 6, 31
    xs, xt, ys, p = make_inputs(B, D, C)
    ys[:] = np.arange(B) % 3                                      # source classes 0..2
    p[:] = 0.02
    p[:, :3] = 0.0
    p[np.arange(B), 3 + np.arange(B)] = 0.9                       # target maxima at 3..8
    got = Launch(dev, _case(xs, xt, ys, p)).twice()
    assert got[3][1] == 0
    _dead(got)
    ref, rds, rdt = run_restated(_case(xs, xt, ys, p), torch.float64)
    assert ref[0] == 0.0 and not rds.any() and not rdt.any()


@pytest.mark.parametrize("D", [255, 4097])
def test_identical_rows_with_the_data_and_with_a_fixed_bandwidth(dev, D):
    B, C = 5, 31
    _, _, ys, p = make_inputs(B, D, C)
    row = np.random.default_rng(D).standard_normal((1, D)).astype(np.float32)
    xs = np.ascontiguousarray(np.broadcast_to(row, (B, D)))
    xt = xs.copy()
    got = Launch(dev, _case(xs, xt, ys, p)).twice()               # bandwidth 0: exp(-0 / 0) is NaN everywhere
    assert got[3][1] >= 1
    _dead(got)
    assert run_restated(_case(xs, xt, ys, p), torch.float64)[0][0] == 0.0
    loss, ds, dt, flags = Launch(dev, _case(xs, xt, ys, p, fix_sigma=1.7 * D)).twice()
    assert flags[0] == 1 and flags[1] >= 1, "a fixed bandwidth keeps the loss live"
    assert np.isfinite(loss).all() and np.isfinite(ds).all() and np.isfinite(dt).all()
    assert not ds.any() and not dt.any()                          # X_i - X_j = 0 in every term
    # every kernel entry is kernel_num: the loss is kernel_num * (sum W_ss + sum W_tt - 2 sum W_st), each sum 1 up to fp32 rounding
    ref = run_restated(_case(xs, xt, ys, p, fix_sigma=1.7 * D), torch.float64)[0][0]
    assert np.isfinite(ref) and abs(float(loss[0]) - ref) <= 1e-5 * 5 * 4


@pytest.mark.parametrize("D", [255, 4097])
def test_zero_probability_column(dev, D):
    B, C = 7, 31
    xs, xt, ys, p = make_inputs(B, D, C)
    col = int(ys[1]) if ys[1] != ys[0] else (int(ys[0]) + 1) % C
    ys[1] = col                                                   # the class is in the source labels, its target column sums to 0 (-> 100)
    p[:, col] = 0.0
    assert p[:, col].sum() == 0.0 and p.argmax(1)[0] == ys[0]
    case = _case(xs, xt, ys, p)
    got = Launch(dev, case).twice()
    assert got[3][0] == 1
    against_restatement(f"zero column, D {D}", got, case)


@pytest.mark.parametrize("D", [255, 4097])
def test_tie_in_a_target_maximum_takes_the_first_index(dev, D):
    """row 2's maximum is shared by classes 4 and 9; only class 4 is a source label and no other target row points at it: it is a
    common class if and only if the first index wins"""
    B, C = 6, 31
    xs, xt, _, p = make_inputs(B, D, C)
    ys = np.array([20, 4, 20, 21, 21, 20], np.int64)
    p[:] = 0.01
    p[:, 20] = 0.5                                                # every other row points at 20 (common)
    p[2, 20] = 0.01
    p[2, 4] = p[2, 9] = np.float32(0.4)
    assert sorted(np.flatnonzero(p[2] == p[2].max()).tolist()) == [4, 9] and 9 not in ys and (p.argmax(1) == 4).sum() == 1
    case = _case(xs, xt, ys, p)
    got = Launch(dev, case).twice()
    assert got[3] == (1, 2), "classes 20 and 4 are common"
    against_restatement(f"tie, D {D}", got, case)
    q = p.copy()
    q[2, 4] = np.float32(0.39)                                    # without the tie class 9 wins and 4 drops out
    assert Launch(dev, _case(xs, xt, ys, q)).run()[3] == (1, 1)


@pytest.mark.parametrize("D", [255, 4097])
def test_source_labels_outside_the_classes(dev, D):
    B, C = 8, 31
    xs, xt, ys, p = make_inputs(B, D, C)
    ys[3], ys[5] = -4, C
    case = _case(xs, xt, ys, p)
    got = Launch(dev, case).twice()
    assert got[3][0] == 1
    against_restatement(f"labels -4 and C, D {D}", got, case)
