"""The folded batch-norm + quantiser kernels (csrc/bnq_kernels.hip, alignq_bnq_*) through the C ABI against tests/bnq_oracle.py, one
row per launch form: the statistics (ab, save, running statistics, num_batches_tracked) bit for bit from inputs that make them exact;
y, the one-bit mask and the int16 level indices bit for bit from the (a, b) the device itself left (no tie band); the backward
against float64 at the oracle's derived bars, every check printing its worst error / bar first.  Every output is written into a
NaN-filled window between sentinel guards (the workspace with its partials and ktot included, the mask pre-filled with 0xAA), every
launch runs twice and must give the same bits.  Then the partials handed in by a convolution, alignq_bnq_affine,
alignq_bnq_bwd_dx, the refusals, and the fast exponential on which the backward bars' c_exp rests.

Not run: the 16384-workgroup cap of tiles() (64 M elements) and parts_for's `cap < 64` arm (C > 4096 is refused).

Measured on an MI355X (worst error / bar of dz, dgamma, dbeta; the larger of the ReLU forms and the form without ReLU; the y-form and
the mask-form are bit-equal).  Every statistic and every forward output was bit-equal to the restatement.
    in-kernel   1x2x4 k1 .064 .221 .071 | 1x2x4 k32 .073 .070 .105 | 1x75x4 k4 .290 .074 .167 | 1x75x4 k8 .249 .043 .097
                1x105x16 k16 .282 .088 .120 | 1x105x16 k2 .327 .179 .161 | 1x4100x64 .469 .198 .208 | 1x70000x4 .417 .127 .113
                1x40000x64 .516 .191 .210 | 1x65536x64 .540 .182 .202
    general     2x54x4 k4 .356 .100 .141 | 2x54x4 k32 .338 .120 .152 | 1x33x128 k16 .446 .265 .226 | 1x33x128 k8 .344 .161 .214
                3x130x256 k2 .486 .171 .199 | 3x130x256 k8 .366 .134 .163 | 8x9x32 k1 .336 .194 .235 | 8x9x32 k4 .312 .140 .214
                1x70000x64 .532 .179 .173 | 1x9000x512 .561 .199 .216 | 2x3000x1024 .539 .188 .228
    512 threads 1x2x2048 k1 .134 .573 .595 | k2 .152 .507 .571 | k4 .190 .534 .616 | k8 .124 .399 .445 | k16 .136 .435 .608
                k32 .144 .375 .494 | 2x700x2048 .511 .223 .233
    bwd_dx      1x5000x4 .737 .202 .656 | 1x130x256 .783 .304 .985 | 1x33x2048 .658 .421 .957 | 2x5000x4 .609 .260 .754
                2x130x256 .697 .299 .986 | 2x33x2048 .699 .350 .986 | 3x5000x4 .677 .178 .436 | 3x130x256 .745 .208 .756
                3x33x2048 .707 .335 .965      (bar_dbeta is there the final rounding to float alone: at most 1 by construction)
    act_jac     1.946 (x^2/2 + 1) eps at x = 0.838 (act_range 2), 1.820 at x = -5.697 (act_range 10)
A library with three defects planted (fin_totals skipping the last partial, the second slice of a pair given the first's k1, the
mask's tail chunk not written) failed 41 of the 63 cases here: every in-kernel row, every row with two or more slices and every
row whose float4 count is no multiple of 64."""
import numpy as np
import pytest
import torch

from tests import bnq_oracle as B
from tests.test_gpu_dwconv import SENTINEL, Arena

pytestmark = pytest.mark.gpu
ROW_IDS = [B.row_id(r) for r in B.ROWS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def ptr(t):
    return None if t is None else t.data_ptr()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def untouched(a):
    return bool((bits(a) == SENTINEL).all())


def floats(nbytes):
    return max((nbytes + 3) // 4, 4)


class Fwd:
    """alignq_bnq_fwd / alignq_bnq_fwd_parts on one case; windows: ab, save, y, mask, bins, running_mean, running_var, ws"""

    def __init__(self, dev, case, formula, relu, k, r, mask, bins, conv_part=None, conv_parts=0):
        from alignq_amd import _lib as L
        self.L, self.lib, self.dev, self.case = L, L.load(), dev, case
        self.groups, self.P, self.C = case["groups"], case["P"], case["C"]
        self.formula, self.relu, self.k, self.r, self.mask, self.bins = formula, relu, k, r, mask, bins
        n, gc = self.groups * self.P * self.C, self.groups * 2 * self.C
        self.n = n
        self.mask_bytes = int(self.lib.alignq_bnq_mask_bytes(self.P, self.C, self.groups))
        assert self.mask_bytes == 8 * self.groups * B.mask_words(self.P * self.C // 4)
        ws_bytes = int(self.lib.alignq_bnq_ws_bytes(self.C, self.groups))
        assert ws_bytes == B.ws_bytes(self.C, self.groups)
        self.arena = Arena(dev, [gc, gc, n, floats(self.mask_bytes), floats(2 * n), self.C, self.C, floats(ws_bytes)])
        self.z, self.res = cu(case["z"], dev), cu(case["res"], dev)
        self.gamma, self.beta = cu(case["gamma"], dev), cu(case["beta"], dev)
        self.conv_part, self.conv_parts = conv_part, conv_parts

    def run(self, entry="fwd"):
        """entry: 'fwd' | 'fwd_parts' | 'stats' | 'stats_parts'; returns a dict of host arrays"""
        L, lib, case = self.L, self.lib, self.case
        self.arena.reset()
        ab, save, y, mask, bins, rm, rv, ws = self.arena.views
        mask.view(torch.int32).fill_(-0x55555556)                          # 0xAAAAAAAA
        use_rs = case["rm"] is not None
        if use_rs:
            rm.copy_(cu(case["rm"], self.dev)); rv.copy_(cu(case["rv"], self.dev))
        nbt = None if case["nbt"] is None else torch.tensor([case["nbt"]], dtype=torch.int64, device=self.dev)
        head = (self.P, self.C, self.groups, ptr(self.gamma), ptr(self.beta), ptr(rm) if use_rs else None, ptr(rv) if use_rs else None,
                ptr(nbt), float(B.MOMENTUM), float(B.BN_EPS))
        want_y = self.bins != "noy"
        tail = (self.k, self.r, self.formula, self.relu, ptr(self.res), ptr(ab), ptr(save), ptr(y) if want_y else None,
                ptr(mask) if self.mask else None, ptr(ws))
        if entry == "fwd":
            assert not self.bins
            rc = lib.alignq_bnq_fwd(ptr(self.z), *head, *tail, L.stream_ptr())
        elif entry == "fwd_parts":
            rc = lib.alignq_bnq_fwd_parts(ptr(self.z), *head, *tail, ptr(self.conv_part), self.conv_parts,
                                          ptr(bins) if self.bins else None, L.stream_ptr())
        elif entry == "stats":
            rc = lib.alignq_bnq_stats(ptr(self.z), *head, ptr(ab), ptr(save), ptr(ws), L.stream_ptr())
        else:
            rc = lib.alignq_bnq_stats_parts(None, *head, ptr(ab), ptr(save), None, ptr(self.conv_part), self.conv_parts, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, rc
        ab, save, y, mask, bins, rm, rv, ws = self.arena.get()               # (asserts the guards)
        gshape = (self.groups, 2, self.C)
        return dict(ab=ab.reshape(gshape), save=save.reshape(gshape), y=y.reshape(self.groups, self.P, self.C),
                    mask=mask[:self.mask_bytes // 4].view(np.uint64).reshape(self.groups, -1), mask_raw=mask,
                    bins=bins.view(np.int16)[:self.n].reshape(self.groups, self.P, self.C), bins_raw=bins, rm=rm, rv=rv,
                    nbt=None if nbt is None else int(nbt.item()))


def check_stats(tag, out, want, case):
    """section 1: bit for bit"""
    for name in ("ab", "save"):
        nd = int((bits(out[name]) != bits(want[name])).sum())
        assert nd == 0, f"{tag}: {name} differs from the restatement in {nd} values"
    if case["rm"] is None:
        assert untouched(out["rm"]) and untouched(out["rv"]) and out["nbt"] is None
    else:
        assert same(out["rm"], want["rm"]), f"{tag}: running_mean"
        assert same(out["rv"], want["rv"]), f"{tag}: running_var"
        assert out["nbt"] == want["nbt"], f"{tag}: num_batches_tracked {out['nbt']} != {want['nbt']}"


def check_outputs(tag, fw, out):
    """section 2: y, mask, bins bit for bit from the device's own (a, b)"""
    case = fw.case
    y_ref, bins_ref, _ = B.fwd_ref(case["z"], out["ab"], fw.formula, fw.relu, fw.k, fw.r, case["res"])
    if fw.bins == "noy":
        assert untouched(out["y"]), f"{tag}: y == NULL but its window was written"
    else:
        nd = int((bits(out["y"]) != bits(y_ref)).sum())
        assert nd == 0, f"{tag}: y differs in {nd} of {y_ref.size} elements"
    if fw.mask:
        stored = y_ref                                                     # (== the stored y, just asserted, or what it would be)
        assert np.array_equal(out["mask"], B.mask_ref(stored)), f"{tag}: mask bits"
        assert (out["mask_raw"].view(np.uint32)[fw.mask_bytes // 4:] == 0xAAAAAAAA).all()
    else:
        assert (out["mask_raw"].view(np.uint32) == 0xAAAAAAAA).all(), f"{tag}: mask == NULL but its window was written"
    if fw.bins:
        assert np.array_equal(out["bins"].astype(np.int32), bins_ref), f"{tag}: bins_out"
    else:
        assert untouched(out["bins_raw"])
    return y_ref


FWD_KEYS = ("ab", "save", "y", "mask_raw", "bins_raw", "rm", "rv")


def twice(fw, entry):
    out, again = fw.run(entry), fw.run(entry)
    for key in FWD_KEYS:
        assert same(out[key], again[key]), f"second run differs in {key}"
    assert out["nbt"] == again["nbt"]
    return out


class Bwd:
    """alignq_bnq_bwd / alignq_bnq_bwd_dx; windows: dz, dres, dgamma, dbeta, ws (partials and ktot)"""

    def __init__(self, dev, z, g, ab, save):
        from alignq_amd import _lib as L
        self.L, self.lib, self.dev = L, L.load(), dev
        self.groups, self.P, self.C = z.shape
        n = z.size
        self.arena = Arena(dev, [n, n, self.C, self.C, floats(int(self.lib.alignq_bnq_ws_bytes(self.C, self.groups)))])
        self.z, self.g, self.ab, self.save = cu(z, dev), cu(g, dev), cu(ab, dev), cu(save, dev)

    def run(self, r, relu, y=None, mask=None, want_dres=True, want_dgb=True, dx_form=False, in_place=False):
        L, lib = self.L, self.lib
        self.arena.reset()
        dz, dres, dgam, dbet, ws = self.arena.views
        dgb = (ptr(dgam), ptr(dbet)) if want_dgb else (None, None)
        if dx_form:
            src = self.g
            if in_place:
                dz.copy_(self.g.reshape(-1))
                src = dz
            rc = lib.alignq_bnq_bwd_dx(ptr(src), ptr(self.z), ptr(self.ab), ptr(self.save), self.P, self.C, self.groups, ptr(dz), *dgb,
                                       ptr(ws), L.stream_ptr())
        else:
            rc = lib.alignq_bnq_bwd(ptr(self.g), ptr(self.z), ptr(y), ptr(mask), ptr(self.ab), ptr(self.save), self.P, self.C,
                                    self.groups, r, relu, ptr(dz), ptr(dres) if want_dres else None, *dgb, ptr(ws), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, rc
        dz, dres, dgam, dbet, _ = self.arena.get()
        if not want_dres:
            assert untouched(dres)
        if not want_dgb:
            assert untouched(dgam) and untouched(dbet)
        shape = (self.groups, self.P, self.C)
        return dict(dz=dz.reshape(shape), dres=dres.reshape(shape), dgamma=dgam, dbeta=dbet)

    def twice(self, *a, **kw):
        out, again = self.run(*a, **kw), self.run(*a, **kw)
        assert all(same(out[k_], again[k_]) for k_ in out), "second run differs"
        return out


def check_bwd(tag, out, ref, dres=True):
    w = {n: B.worst(out[n], ref[n], ref["bar_" + n]) for n in ("dz", "dgamma", "dbeta")}
    print(f"[bnq-forms] {tag}: worst error / bar  dz {w['dz']:.3f}  dgamma {w['dgamma']:.3f}  dbeta {w['dbeta']:.3f}")
    assert max(w.values()) <= 1.0, (tag, w)
    if dres:
        assert same(out["dres"], ref["dres"].astype(np.float32)), f"{tag}: dres is not g * [y > 0]"


@pytest.mark.parametrize("i", range(len(B.ROWS)), ids=ROW_IDS)
def test_forward_and_backward_forms(dev, i):
    """alignq_bnq_fwd (alignq_bnq_fwd_parts with conv_part == NULL where bins_out is asked for), then alignq_bnq_bwd in its y-form,
    its mask-form, without the ReLU (y and mask NULL), with and without dres / dgamma / dbeta."""
    row = B.ROWS[i]
    d, case, tag = B.row_dict(row), B.case_of(row, i), ROW_IDS[i]
    fw = Fwd(dev, case, d["formula"], d["relu"], d["k"], d["r"], d["mask"], d["bins"])
    out = twice(fw, "fwd_parts" if d["bins"] else "fwd")
    check_stats(tag, out, B.case_stats(case), case)
    y_ref = check_outputs(tag, fw, out)
    # ---- backward, from what the forward left
    z, ab, save = case["z"], out["ab"], out["save"]
    g = B.make_g(z, save, i)
    x, zhat, a = B.ref_inputs(z, ab, save)
    bw = Bwd(dev, z, g, ab, save)
    if d["relu"]:
        pos = y_ref > 0
        zeros = 1.0 - pos.mean()
        ref = B.bwd_ref(g, x, zhat, a, pos, d["r"])
        first = None
        if d["bins"] != "noy":
            first = bw.twice(d["r"], 1, y=cu(out["y"], dev))
            check_bwd(f"{tag} y-form ({100 * zeros:.0f} % masked)", first, ref)
        if d["mask"]:
            mk = cu(out["mask_raw"], dev)
            got = bw.twice(d["r"], 1, mask=mk)
            check_bwd(f"{tag} mask-form", got, ref)
            if first is not None:
                assert all(same(first[k_], got[k_]) for k_ in got), "y-form and mask-form differ"
            first = got
            lean = bw.run(d["r"], 1, mask=mk, want_dres=False, want_dgb=False)
            assert same(lean["dz"], first["dz"]), "dz changes with dgamma / dbeta / dres NULL"
        if case["gamma"] is not None:
            ch0 = first["dz"][:, :, case["ch"]["gamma0"]]
            assert not np.isnan(ch0).any() and not ch0.any(), "gamma == 0: dz must be +0 or -0"
    ref0 = B.bwd_ref(g, x, zhat, a, None, d["r"])
    plain = bw.twice(d["r"], 0)
    check_bwd(f"{tag} relu = 0, y and mask NULL", plain, ref0)
    lean = bw.run(d["r"], 0, want_dres=False, want_dgb=False)
    assert same(lean["dz"], plain["dz"]), "dz changes with dgamma / dbeta / dres NULL"


@pytest.mark.parametrize("groups,cp", B.PARTS_ROWS, ids=[f"{g}x{B.PARTS_P}x{B.PARTS_C}-parts{cp}" for g, cp in B.PARTS_ROWS])
def test_partials_handed_in(dev, groups, cp):
    """alignq_bnq_stats_parts with z == NULL and alignq_bnq_fwd_parts: the statistics come from the given partials ALONE - they are
    those of ANOTHER tensor than z, so a launch that summed z itself (the in-kernel path of this shape at groups == 1) is seen -
    and the apply pass runs on z.  The partials lie between NaN doubles."""
    P, C = B.PARTS_P, B.PARTS_C
    odd = cp % 2
    case = dict(B.make_case(groups, P, C, odd, 0, 40 + groups))
    other = B.make_z(groups, P, C, 9000 + cp)
    part = B.random_partials(other, cp, cp + groups)
    pad = 64
    buf = torch.full((part.size + 2 * pad,), float("nan"), dtype=torch.float64, device=dev)
    buf[pad:pad + part.size] = cu(part.reshape(-1), dev)
    conv_part = buf[pad:pad + part.size]
    assert conv_part.data_ptr() % 16 == 0
    want = B.case_stats(case, (part[..., 0].sum(axis=1), part[..., 1].sum(axis=1)))
    assert np.array_equal(part[..., 0].sum(axis=1), B.totals(other)[0])
    tag = f"parts {groups}x{P}x{C} conv_parts={cp}"
    fw = Fwd(dev, case, odd, 1, 4 if odd else 8, 2.0, 1, "" if odd else "y", conv_part, cp)
    st = twice(fw, "stats_parts")
    check_stats(tag + " stats_parts", st, want, case)
    assert untouched(st["y"])
    out = twice(fw, "fwd_parts")
    check_stats(tag + " fwd_parts", out, want, case)
    check_outputs(tag, fw, out)
    host = buf.cpu().numpy()
    assert np.isnan(host[:pad]).all() and np.isnan(host[-pad:]).all() and np.array_equal(host[pad:-pad], part.reshape(-1))


def test_stats_alone_equals_the_restatement(dev):
    """alignq_bnq_stats (never the in-kernel form) at an in-kernel shape, a lone tail slice and the 512-thread form"""
    for seed, (groups, P, C) in enumerate([(1, 4100, 64), (3, 130, 256), (2, 33, 2048)]):
        case = B.make_case(groups, P, C, 0, 0, 60 + seed)
        fw = Fwd(dev, case, 0, 0, 8, 2.0, 0, "")
        out = twice(fw, "stats")
        check_stats(f"stats {groups}x{P}x{C}", out, B.case_stats(case), case)
        assert untouched(out["y"]) and untouched(out["bins_raw"])


@pytest.mark.parametrize("groups,P,C", B.AFFINE_ROWS, ids=[f"{g}x{P}x{C}" for g, P, C in B.AFFINE_ROWS])
def test_affine_is_one_fma(dev, groups, P, C):
    from alignq_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(P + C)
    z = rng.standard_normal((groups, P, C)).astype(np.float32)
    ab = (rng.standard_normal((groups, 2, C)) * 1.5).astype(np.float32)
    zd, abd = cu(z, dev), cu(ab, dev)
    arena = Arena(dev, [z.size])
    outs = []
    for _ in range(2):
        arena.reset()
        assert lib.alignq_bnq_affine(ptr(zd), ptr(abd), P, C, groups, ptr(arena.views[0]), L.stream_ptr()) == 0
        torch.cuda.synchronize()
        outs.append(arena.get()[0])
    assert not np.isnan(outs[0]).any()
    assert same(outs[0], B.bn_x(z, ab).reshape(-1)), "y is not fma(a, z, b)"
    assert same(outs[0], outs[1]), "second run differs"


@pytest.mark.parametrize("groups,P,C", B.BWD_DX_ROWS, ids=[f"{g}x{P}x{C}" for g, P, C in B.BWD_DX_ROWS])
def test_backward_from_a_given_dx(dev, groups, P, C):
    """alignq_bnq_bwd_dx: e_dx = 0 in the bars; in place (dz == dx) against out of place, dgamma / dbeta NULL against given"""
    case = B.make_case(groups, P, C, 0, 0, 80 + groups)
    st = B.case_stats(case)
    z, ab, save = case["z"], st["ab"], st["save"]
    g = B.make_g(z, save, P + C)
    x, zhat, a = B.ref_inputs(z, ab, save)
    ref = B.bwd_ref(g, x, zhat, a, None, 0.0, from_dx=True)
    bw = Bwd(dev, z, g, ab, save)
    out = bw.twice(0.0, 0, dx_form=True, want_dres=False)
    check_bwd(f"bwd_dx {groups}x{P}x{C}", out, ref, dres=False)
    inp = bw.twice(0.0, 0, dx_form=True, want_dres=False, in_place=True)
    assert all(same(out[k_], inp[k_]) for k_ in ("dz", "dgamma", "dbeta")), "in place differs from out of place"
    lean = bw.run(0.0, 0, dx_form=True, want_dres=False, want_dgb=False)
    assert same(lean["dz"], out["dz"])
    ch0 = out["dz"][:, :, case["ch"]["gamma0"]]
    assert not np.isnan(ch0).any() and not ch0.any()


# ------------------------------------------------------------------------------------------------ refusals
class _Refuse:
    """valid arguments of every entry point at (groups 2, P 6, C 8), every buffer a window of ONE arena (inputs included: nothing
    may be written on a refusal); call(entry, **changes) returns the code"""
    NAMES = ("z", "g", "y", "res", "ab", "save", "dz", "dres", "mask", "bins", "gamma", "beta", "rm", "rv", "dgamma", "dbeta", "ws")

    def __init__(self, dev):
        from alignq_amd import _lib as L
        self.L, self.lib = L, L.load()
        # room for every shape tried below, so that a call that fails to refuse still stays inside its windows and is seen there
        big = 2 * 9 * 4096
        sizes = dict(z=big, g=big, y=big, res=big, dz=big, dres=big, ab=big, save=big, mask=big, bins=big, gamma=4096, beta=4096, rm=4096,
                     rv=4096, dgamma=4096, dbeta=4096, ws=floats(max(B.ws_bytes(4096, 1), B.ws_bytes(8, 9))))
        self.arena = Arena(dev, [sizes[n] for n in self.NAMES])
        self.p = {n: v.data_ptr() for n, v in zip(self.NAMES, self.arena.views)}
        self.nbt = torch.zeros(1, dtype=torch.int64, device=dev)

    def call(self, entry, off=None, **ch):
        a = dict(P=6, C=8, groups=2, k=8, r=2.0, formula=0, relu=1, res=None, mask=self.p["mask"], bins=None, y=self.p["y"])
        a.update(ch)
        p = dict(self.p)
        if off:
            p[off] += 4
            for key in ("mask", "y", "res", "bins"):
                if off == key:
                    a[key] = p[key]
        lib, st = self.lib, self.L.stream_ptr()
        head = (a["P"], a["C"], a["groups"], p["gamma"], p["beta"], p["rm"], p["rv"], ptr(self.nbt), 0.1, 1e-5)
        if entry == "fwd":
            rc = lib.alignq_bnq_fwd_parts(p["z"], *head, a["k"], a["r"], a["formula"], a["relu"], a["res"], p["ab"], p["save"], a["y"],
                                          a["mask"], p["ws"], None, 0, a["bins"], st)
        elif entry == "bwd":
            rc = lib.alignq_bnq_bwd(p["g"], p["z"], a["y"], a["mask"], p["ab"], p["save"], a["P"], a["C"], a["groups"], a["r"], a["relu"],
                                    p["dz"], p["dres"], p["dgamma"], p["dbeta"], p["ws"], st)
        elif entry == "stats":
            rc = lib.alignq_bnq_stats_parts(p["z"], *head, p["ab"], p["save"], p["ws"], None, 0, st)
        elif entry == "affine":
            rc = lib.alignq_bnq_affine(p["z"], p["ab"], a["P"], a["C"], a["groups"], a["y"], st)
        else:
            rc = lib.alignq_bnq_bwd_dx(p["g"], p["z"], p["ab"], p["save"], a["P"], a["C"], a["groups"], p["dz"], p["dgamma"], p["dbeta"],
                                       p["ws"], st)
        torch.cuda.synchronize()
        return rc


ENTRIES = ("fwd", "bwd", "stats", "affine", "bwd_dx")


def test_refusals_leave_every_window_untouched(dev):
    """return codes as bnq_kernels.hip:618-631, :672-679, :712-715, :731-733, :742-744 state"""
    from alignq_amd import _lib as L
    R = _Refuse(dev)
    seen = []

    def expect(code, entry, **kw):
        rc = R.call(entry, **kw)
        seen.append((entry, kw, rc))
        assert rc == code, (entry, kw, rc, code)

    for C in (0, 2, 6, 12, 4096):
        for e in ENTRIES:
            expect(L.EUNSUPPORTED, e, C=C, P=2, groups=1)
    for e in ENTRIES:
        expect(L.EINVAL, e, P=0 if e == "affine" else 1)
        for groups in (0, 9):
            expect(L.EINVAL, e, groups=groups)
    for e, names in (("fwd", ("z", "y", "mask", "res", "bins")), ("bwd", ("z", "y", "g", "dz", "mask", "dres")), ("stats", ("z",)),
                     ("affine", ("z", "y")), ("bwd_dx", ("z", "g", "dz"))):
        for name in names:
            kw = {}
            if name == "res":
                kw["res"] = R.p["res"]
            if name == "bins":
                kw["bins"] = R.p["bins"]
            if name == "y" and e == "bwd":
                kw["mask"] = None                         # (the bits, when given, replace y: its alignment then does not matter)
            expect(L.EINVAL, e, off=name, **kw)
    for k in (0, 17):
        expect(L.EINVAL, "fwd", k=k)
    expect(L.EINVAL, "fwd", formula=2)
    expect(L.EINVAL, "fwd", bins=R.p["bins"], formula=1)
    expect(L.EINVAL, "fwd", bins=R.p["bins"], res=R.p["res"])
    expect(L.EINVAL, "fwd", bins=R.p["bins"], k=15)
    expect(L.EINVAL, "bwd", y=None, mask=None)            # relu without a source for the mask
    assert (R.arena.raw() == SENTINEL).all(), "a refused call wrote something"
    assert int(R.nbt.item()) == 0
    assert len(seen) > 60


# ------------------------------------------------------------------------------------------------ the bars' c_exp
def test_fast_exponential_within_c_exp(dev):
    """act_jac alone (alignq_act_quant_bwd with g = 1) against float64 on [-6, 6]: the figure behind bnq_oracle.C_EXP"""
    from alignq_amd import _lib as L
    lib = L.load()
    grid = np.linspace(-6.0, 6.0, 1 << 20).astype(np.float32)
    rng = np.random.default_rng(0)
    x = np.concatenate([grid, np.nextafter(grid, np.float32(9)), np.nextafter(grid, np.float32(-9)),
                        rng.uniform(-6, 6, 1 << 20).astype(np.float32)])
    xd = cu(x, dev)
    worst = 0.0
    for r in (2.0, 10.0):
        dx = torch.full_like(xd, float("nan"))
        assert lib.alignq_act_quant_bwd(ptr(torch.ones_like(xd)), ptr(xd), ptr(dx), x.size, r, L.stream_ptr()) == 0
        torch.cuda.synchronize()
        u = B.exp_units(x, dx.cpu().numpy(), r)
        j = int(u.argmax())
        print(f"[bnq-forms] act_jac, r = {r}: worst relative error {u[j]:.3f} (x^2/2 + 1) eps at x = {x[j]!r}; "
              f"worst in units of eps alone {float((u * (0.5 * x.astype(np.float64) ** 2 + 1)).max()):.2f}")
        worst = max(worst, float(u[j]))
    assert worst <= B.MEASURED_EXP_UNITS * 1.001 + 0.005, "the recorded figure is no longer the worst: measure again"
    assert B.C_EXP >= 2 * worst and B.C_EXP == int(np.ceil(2 * B.MEASURED_EXP_UNITS))
