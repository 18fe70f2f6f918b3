"""alignq_bnq_any_fwd / _bwd (include/alignq_bnq_any.h, csrc/bnq_any_kernels.hip) against tests/bnq_oracle.py, the restatement the
power-of-two family (alignq_bnq_*) is held to: statistics, y and mask bit for bit; dz, dgamma, dbeta within the oracle's derived bars;
every launch twice with the same bits.  Rows: the smallest shapes that reach every arm of the mapping (see ROWS)."""
import numpy as np
import pytest
import torch

from tests import bnq_oracle as B
from tests.test_gpu_bnq_forms import bits, cu, dev, floats, ptr, same, untouched  # noqa: F401  (dev: the fixture)
from tests.test_gpu_dwconv import Arena

pytestmark = pytest.mark.gpu
NONE, RELU, RELU6 = 0, 1, 2
# (P, C, formula, clamp, k, act_range, nulls)
ROWS = [
    (2, 4, 0, RELU, 1, 2.0, 0),            # the minimum: one quad, two pixels, 254 of 256 slots without a pixel
    (75, 4, 1, NONE, 4, 2.0, 0),           # P no multiple of the slot count; 75 float4: not a multiple of 64; no mask
    (9001, 4, 0, RELU6, 4, 10.0, 0),       # 4 partials, the last one shorter; values above 6 (ADMM formula, act_range 10)
    (75, 12, 0, RELU6, 8, 10.0, 0),        # 3 lanes per pixel, 64 slots of a 192 block
    (4099, 12, 1, RELU, 2, 2.0, 1),        # 8 partials, ragged; gamma, beta, running statistics and the counter all NULL
    (2, 36, 0, RELU, 4, 2.0, 0),
    (3001, 36, 0, RELU6, 4, 10.0, 0),      # 28 slots x 9 lanes, 4 lanes idle; 13 partials, ragged
    (75, 144, 1, RELU6, 4, 2.0, 0),
    (1100, 144, 0, RELU, 3, 2.0, 0),       # 7 slots x 36 lanes; 19 partials, ragged
    (33, 576, 0, RELU6, 4, 10.0, 0),       # 3 slots x 144 lanes of a 448 block
    (33, 1028, 0, RELU, 4, 2.0, 0),        # two quads per thread, odd quad count: the last lane has one
    (33, 1280, 1, RELU, 4, 2.0, 0),        # MobileNet-V2's head: one slot x 320 lanes x 2 quads
    (33, 1280, 0, NONE, 16, 2.0, 0),
    (33, 2048, 0, RELU6, 2, 10.0, 0),      # the limit: 256 lanes x 2 quads, two slots of a 512 block
    (2, 2048, 1, RELU, 4, 2.0, 0),
    (29200, 288, 0, RELU, 4, 2.0, 0),      # 2.1 M float4: a second grid pass of both elementwise kernels (their channel index steps
]                                          # by 8 of 72 quads between passes), 256 partials, write-through stores (33.6 MB)
IDS = [f"{P}x{C}-f{f}-c{c}-k{k}-r{int(r)}" + ("-nulls" if n else "") for P, C, f, c, k, r, n in ROWS]


def clamp_ref(q, clamp):
    """(y, pos): the clamp of alignq_mobile.h on the quantised values, and "the gradient passes" (None without a clamp)"""
    if clamp == NONE:
        return q, None
    pos = (q > 0) & (q < 6) if clamp == RELU6 else q > 0
    y = np.where(q > 0, np.minimum(q, np.float32(6.0)) if clamp == RELU6 else q, np.float32(0.0)).astype(np.float32)
    return y, pos


class Site:
    """one case on the device; windows: ab, save, y, mask, running_mean, running_var, dz, dgamma, dbeta, ws"""

    def __init__(self, dev, case, row):
        from alignq_amd import _lib as L
        self.L, self.lib, self.dev, self.case = L, L.load(), dev, case
        self.P, self.C, self.formula, self.clamp, self.k, self.r, _ = row
        P, C, n = self.P, self.C, self.P * self.C
        assert self.lib.alignq_bnq_any_supported(P, C) == 1
        self.mask_bytes = int(self.lib.alignq_bnq_any_mask_bytes(P, C))
        assert self.mask_bytes == 8 * B.mask_words(n // 4)
        self.arena = Arena(dev, [2 * C, 2 * C, n, floats(self.mask_bytes), C, C, n, C, C, floats(int(self.lib.alignq_bnq_any_ws_bytes(P, C)))])
        self.z, self.gamma, self.beta = cu(case["z"], dev), cu(case["gamma"], dev), cu(case["beta"], dev)

    def fwd(self):
        case, L = self.case, self.L
        self.arena.reset()
        ab, save, y, mask, rm, rv, _, _, _, ws = self.arena.views
        use_rs = case["rm"] is not None
        if use_rs:
            rm.copy_(cu(case["rm"], self.dev)); rv.copy_(cu(case["rv"], self.dev))
        nbt = None if case["nbt"] is None else torch.tensor([case["nbt"]], dtype=torch.int64, device=self.dev)
        rc = self.lib.alignq_bnq_any_fwd(ptr(self.z), self.P, self.C, ptr(self.gamma), ptr(self.beta), ptr(rm) if use_rs else None,
                                         ptr(rv) if use_rs else None, ptr(nbt), float(B.MOMENTUM), float(B.BN_EPS), self.k, self.r,
                                         self.formula, self.clamp, ptr(ab), ptr(save), ptr(y), ptr(mask) if self.clamp else None, ptr(ws),
                                         L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, rc
        ab, save, y, mask, rm, rv, dz, dgam, dbet, _ = self.arena.get()            # (asserts the guards)
        assert untouched(dz) and untouched(dgam) and untouched(dbet)
        return dict(ab=ab.reshape(1, 2, self.C), save=save.reshape(1, 2, self.C), y=y.reshape(1, self.P, self.C), mask=mask, rm=rm, rv=rv,
                    nbt=np.float32(-1 if nbt is None else nbt.item()))

    def bwd(self, g, fw, want_dgb=True):
        self.arena.reset()
        ab, save, _, mask, _, _, dz, dgam, dbet, ws = self.arena.views
        ab.copy_(cu(fw["ab"].reshape(-1), self.dev)); save.copy_(cu(fw["save"].reshape(-1), self.dev)); mask.copy_(cu(fw["mask"], self.dev))
        rc = self.lib.alignq_bnq_any_bwd(ptr(g), ptr(self.z), ptr(mask) if self.clamp else None, ptr(ab), ptr(save), self.P, self.C, self.r,
                                         self.clamp, ptr(dz), ptr(dgam) if want_dgb else None, ptr(dbet) if want_dgb else None, ptr(ws),
                                         self.L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, rc
        out = self.arena.get()
        return dict(dz=out[6].reshape(1, self.P, self.C), dgamma=out[7], dbeta=out[8])


def twice(run):
    out, again = run(), run()
    assert all(same(out[k_], again[k_]) for k_ in out), "a second launch gives other bits"
    return out


@pytest.mark.parametrize("i", range(len(ROWS)), ids=IDS)
def test_forward_and_backward(dev, i):
    row = ROWS[i]
    P, C, formula, clamp, k, r, nulls = row
    case, tag = B.make_case(1, P, C, 0, nulls, i), IDS[i]
    site = Site(dev, case, row)
    fw = twice(site.fwd)
    # ---- statistics: bit for bit (dyadic inputs: the sums are exact in any order)
    want = B.case_stats(case)
    for name in ("ab", "save"):
        assert same(fw[name], want[name]), f"{tag}: {name} differs from the restatement"
    if nulls:
        assert untouched(fw["rm"]) and untouched(fw["rv"])
    else:
        assert same(fw["rm"], want["rm"]) and same(fw["rv"], want["rv"]) and int(fw["nbt"]) == want["nbt"], f"{tag}: running statistics"
    # ---- y and the mask: bit for bit from the device's own (a, b)
    q, _, _ = B.fwd_ref(case["z"], fw["ab"], formula, 0, k, r)
    y_ref, pos = clamp_ref(q, clamp)
    nd = int((bits(fw["y"]) != bits(y_ref)).sum())
    assert nd == 0, f"{tag}: y differs in {nd} of {y_ref.size} elements"
    words = fw["mask"].view(np.uint32)
    if clamp:
        want_mask = B.mask_ref(pos.astype(np.float32)).reshape(-1)
        assert np.array_equal(words[:site.mask_bytes // 4].view(np.uint64), want_mask), f"{tag}: mask bits (tail bits zero)"
        assert untouched(words[site.mask_bytes // 4:].view(np.float32))
    else:
        assert untouched(fw["mask"]), f"{tag}: no clamp, but the mask window was written"
    # ---- backward in float64 from what the forward left
    g = B.make_g(case["z"], fw["save"], i)
    x, zhat, a = B.ref_inputs(case["z"], fw["ab"], fw["save"])
    ref = B.bwd_ref(g, x, zhat, a, pos, r)
    gd = cu(g, dev)
    out = twice(lambda: site.bwd(gd, fw))
    w = {n: B.worst(out[n], ref[n], ref["bar_" + n]) for n in ("dz", "dgamma", "dbeta")}
    print(f"[bnq-any] {tag}: worst error / bar  dz {w['dz']:.3f}  dgamma {w['dgamma']:.3f}  dbeta {w['dbeta']:.3f}")
    assert max(w.values()) <= 1.0, (tag, w)
    lean = site.bwd(gd, fw, want_dgb=False)
    assert same(lean["dz"], out["dz"]) and untouched(lean["dgamma"]) and untouched(lean["dbeta"]), "dgamma / dbeta NULL"


def test_same_bits_as_the_power_of_two_family(dev):
    """C = 64 with ReLU: ab, save, y and the mask of alignq_bnq_any_fwd equal alignq_bnq_fwd's"""
    from alignq_amd import _lib as L
    row = (300, 64, 0, RELU, 4, 2.0, 0)
    case = B.make_case(1, 300, 64, 0, 0, 3)
    site = Site(dev, case, row)
    fw = site.fwd()
    lib, n = L.load(), 300 * 64
    arena = Arena(dev, [128, 128, n, floats(site.mask_bytes), 64, 64, floats(int(lib.alignq_bnq_ws_bytes(64, 1)))])
    ab, save, y, mask, rm, rv, ws = arena.views
    rm.copy_(cu(case["rm"], dev)); rv.copy_(cu(case["rv"], dev))
    nbt = torch.tensor([case["nbt"]], dtype=torch.int64, device=dev)
    rc = lib.alignq_bnq_fwd(ptr(site.z), 300, 64, 1, ptr(site.gamma), ptr(site.beta), ptr(rm), ptr(rv), ptr(nbt), float(B.MOMENTUM),
                            float(B.BN_EPS), 4, 2.0, 0, 1, None, ptr(ab), ptr(save), ptr(y), ptr(mask), ptr(ws), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    old = dict(zip(("ab", "save", "y", "mask", "rm", "rv"), arena.get()))
    for name in old:
        assert same(fw[name].reshape(-1), old[name]), name


@pytest.mark.parametrize("P,C,code", [(75, 6, "EUNSUPPORTED"), (75, 2052, "EUNSUPPORTED"), (75, 0, "EUNSUPPORTED"), (1, 4, "EINVAL")])
def test_refusals_write_nothing(dev, P, C, code):
    from alignq_amd import _lib as L
    lib = L.load()
    assert lib.alignq_bnq_any_supported(P, C) == 0 and lib.alignq_bnq_any_ws_bytes(P, C) == 0 and lib.alignq_bnq_any_mask_bytes(P, C) == 0
    arena = Arena(dev, [4200] * 8)
    a = [ptr(v) for v in arena.views]
    nbt = torch.tensor([B.NBT0], dtype=torch.int64, device=dev)
    assert lib.alignq_bnq_any_fwd(a[0], P, C, None, None, a[1], a[2], ptr(nbt), 0.1, 1e-5, 4, 2.0, 0, RELU, a[3], a[4], a[5], a[6], a[7],
                                  L.stream_ptr()) == getattr(L, code)
    assert lib.alignq_bnq_any_bwd(a[0], a[1], a[6], a[3], a[4], P, C, 2.0, RELU, a[5], a[2], a[2], a[7], L.stream_ptr()) == getattr(L, code)
    torch.cuda.synchronize()
    assert all(untouched(v) for v in arena.get()) and int(nbt.item()) == B.NBT0
