"""alignq_bnq_pool_fwd / _bwd (include/alignq_bnq_pool.h, csrc/bnq_pool_kernels.hip) against tests/bnq_oracle.py: statistics, y and the
code bit for bit; dz, dgamma, dbeta within the oracle's derived bars for the gradient scattered to the selected positions; every launch
twice with the same bits.  The only reference code of its own: the first maximum of a 2 x 2 window and that scatter."""
import numpy as np
import pytest
import torch

from tests import bnq_oracle as O
from tests.test_gpu_bnq_forms import bits, cu, dev, floats, ptr, same, untouched  # noqa: F401  (dev: the fixture)
from tests.test_gpu_dwconv import Arena

pytestmark = pytest.mark.gpu
# (B, H, W, C, formula, k, act_range, nulls)
ROWS = [
    (1, 2, 2, 4, 0, 1, 2.0, 0),            # one window, one quad: one thread of each window kernel, one slot with a pixel
    (3, 6, 10, 12, 1, 4, 2.0, 0),          # three lanes per pixel, odd pooled extents 3 x 5
    (7, 14, 18, 36, 0, 4, 10.0, 0),        # 28 slots x 9 lanes, 4 lanes idle; several ragged partials each way
    (2, 24, 24, 32, 1, 4, 2.0, 0),         # the network's first site
    (5, 8, 8, 48, 0, 8, 2.0, 0),           # its second site: 16 slots of a 192 block
    (1, 2, 2, 1024, 0, 4, 2.0, 0),         # the channel limit: 256 lanes, one slot
    (3, 6, 10, 12, 0, 3, 2.0, 1),          # gamma, beta, running statistics and the counter all NULL
    (2, 10, 6, 20, 1, 2, 2.0, 0),          # four levels: nearly every window ties
]
IDS = [f"{b}x{h}x{w}x{c}-f{f}-k{k}-r{int(r)}" + ("-nulls" if n else "") for b, h, w, c, f, k, r, n in ROWS]


def windows(a, B, H, W):
    """[1, P, C] -> [B * H/2 * W/2, 4, C], a window's positions in the order (0,0), (0,1), (1,0), (1,1)"""
    C = a.shape[-1]
    return a.reshape(B, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(-1, 4, C)


def scatter(v, sel, B, H, W):
    """v [PP, C] at the selected position of its window, zero at the other three, back as [1, P, C]"""
    out = np.zeros((v.shape[0], 4, v.shape[1]), v.dtype)
    np.put_along_axis(out, sel[:, None, :], v[:, None, :], axis=1)
    return np.ascontiguousarray(out.reshape(B, H // 2, W // 2, 2, 2, -1).transpose(0, 1, 3, 2, 4, 5)).reshape(1, B * H * W, -1)


class Site:
    """one case on the device; windows: ab, save, y, code, running_mean, running_var, dz, dgamma, dbeta, ws"""

    def __init__(self, dev, case, row):
        from alignq_amd import _lib as L
        self.L, self.lib, self.dev, self.case = L, L.load(), dev, case
        self.B, self.H, self.W, self.C, self.formula, self.k, self.r, _ = row
        self.shape = (self.B, self.H, self.W, self.C)
        P, C = self.B * self.H * self.W, self.C
        assert self.lib.alignq_bnq_pool_supported(*self.shape) == 1
        self.code_bytes = int(self.lib.alignq_bnq_pool_code_bytes(*self.shape))
        assert self.code_bytes == P // 4 * C
        self.arena = Arena(dev, [2 * C, 2 * C, P // 4 * C, floats(self.code_bytes), C, C, P * C, C, C,
                                 floats(int(self.lib.alignq_bnq_pool_ws_bytes(*self.shape)))])
        self.z, self.gamma, self.beta = cu(case["z"], dev), cu(case["gamma"], dev), cu(case["beta"], dev)

    def fwd(self):
        case = self.case
        self.arena.reset()
        ab, save, y, code, rm, rv, _, _, _, ws = self.arena.views
        use_rs = case["rm"] is not None
        if use_rs:
            rm.copy_(cu(case["rm"], self.dev)); rv.copy_(cu(case["rv"], self.dev))
        nbt = None if case["nbt"] is None else torch.tensor([case["nbt"]], dtype=torch.int64, device=self.dev)
        rc = self.lib.alignq_bnq_pool_fwd(ptr(self.z), *self.shape, ptr(self.gamma), ptr(self.beta), ptr(rm) if use_rs else None,
                                          ptr(rv) if use_rs else None, ptr(nbt), float(O.MOMENTUM), float(O.BN_EPS), self.k, self.r,
                                          self.formula, ptr(ab), ptr(save), ptr(y), ptr(code), ptr(ws), self.L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, rc
        ab, save, y, code, rm, rv, dz, dgam, dbet, _ = self.arena.get()            # (asserts the guards)
        assert untouched(dz) and untouched(dgam) and untouched(dbet)
        return dict(ab=ab.reshape(1, 2, self.C), save=save.reshape(1, 2, self.C), y=y, code=code, rm=rm, rv=rv,
                    nbt=np.float32(-1 if nbt is None else nbt.item()))

    def bwd(self, g, fw, want_dgb=True):
        self.arena.reset()
        ab, save, _, code, _, _, dz, dgam, dbet, ws = self.arena.views
        ab.copy_(cu(fw["ab"].reshape(-1), self.dev)); save.copy_(cu(fw["save"].reshape(-1), self.dev)); code.copy_(cu(fw["code"], self.dev))
        rc = self.lib.alignq_bnq_pool_bwd(ptr(g), ptr(self.z), ptr(code), ptr(ab), ptr(save), *self.shape, self.r, ptr(dz),
                                          ptr(dgam) if want_dgb else None, ptr(dbet) if want_dgb else None, ptr(ws), self.L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, rc
        out = self.arena.get()
        return dict(dz=out[6], dgamma=out[7], dbeta=out[8])


def twice(run):
    out, again = run(), run()
    assert all(same(out[k_], again[k_]) for k_ in out), "a second launch gives other bits"
    return out


@pytest.mark.parametrize("i", range(len(ROWS)), ids=IDS)
def test_forward_and_backward(dev, i):
    row = ROWS[i]
    B, H, W, C, formula, k, r, nulls = row
    P = B * H * W
    case, tag = O.make_case(1, P, C, 0, nulls, i), IDS[i]
    site = Site(dev, case, row)
    fw = twice(site.fwd)
    # ---- statistics: bit for bit (dyadic inputs: the sums are exact in any order)
    want = O.case_stats(case)
    for name in ("ab", "save"):
        assert same(fw[name], want[name]), f"{tag}: {name} differs from the restatement"
    if nulls:
        assert untouched(fw["rm"]) and untouched(fw["rv"])
    else:
        assert same(fw["rm"], want["rm"]) and same(fw["rv"], want["rv"]) and int(fw["nbt"]) == want["nbt"], f"{tag}: running statistics"
    # ---- y and the code: bit for bit from the device's own (a, b); np.argmax returns the FIRST maximum
    u = windows(O.fwd_ref(case["z"], fw["ab"], formula, 1, k, r)[0], B, H, W)
    sel = u.argmax(axis=1)
    y_ref = np.take_along_axis(u, sel[:, None, :], axis=1)[:, 0, :]
    nd = int((bits(fw["y"]) != bits(y_ref).reshape(-1)).sum())
    assert nd == 0, f"{tag}: y differs in {nd} of {y_ref.size} elements"
    code = fw["code"].view(np.uint8)
    assert untouched(code[site.code_bytes:].view(np.float32))
    code = code[:site.code_bytes].reshape(P // 4, C)                   # the header's layout: one byte per element of y
    print(f"[bnq-pool] {tag}: {float((np.ptp(np.sort(u, axis=1)[:, 2:, :], axis=1) == 0).mean()):.2f} of the windows tie for the maximum")
    assert np.array_equal(code & 3, sel), f"{tag}: not the first row-major maximum"
    assert np.array_equal(code >> 2, (y_ref > 0).astype(np.uint8)), f"{tag}: pass bit is not y > 0 (bits 3-7 zero)"
    # ---- backward in float64: the pooled gradient scattered to the selected positions, pos from the pass bits
    gp = np.ascontiguousarray(windows(O.make_g(case["z"], fw["save"], i), B, H, W)[:, 0, :])
    g_full = scatter(gp, sel, B, H, W)
    pos = scatter((code >> 2).astype(bool), sel, B, H, W)
    x, zhat, a = O.ref_inputs(case["z"], fw["ab"], fw["save"])
    ref = O.bwd_ref(g_full, x, zhat, a, pos, r)
    gd = cu(gp, dev)
    out = twice(lambda: site.bwd(gd, fw))
    w = {n: O.worst(out[n], ref[n], ref["bar_" + n]) for n in ("dz", "dgamma", "dbeta")}
    print(f"[bnq-pool] {tag}: worst error / bar  dz {w['dz']:.3f}  dgamma {w['dgamma']:.3f}  dbeta {w['dbeta']:.3f}")
    assert max(w.values()) <= 1.0, (tag, w)
    lean = site.bwd(gd, fw, want_dgb=False)
    assert same(lean["dz"], out["dz"]) and untouched(lean["dgamma"]) and untouched(lean["dbeta"]), "dgamma / dbeta NULL"

