"""The classifier head (csrc/head_body.h: alignq_head_ce_fwd / _bwd, and its two roles alignq_head_ce_bwd_site_prep and
alignq_site_reduce_loss_multi_head) through the C ABI against tests/head_oracle.py, one row per launch form.  Every output lies in a
NaN-filled window between sentinel guards, every launch runs twice and must give the same bits, the three forms of the forward (loss
only; ce_mean + counter; + site_scal / trans_total at n_sites 1, 21, 65) must agree bit for bit in pooled / logits / probs / loss and
leave the counter at 0; the backward runs with g in {1.0, 0.37} from device memory, with and without dbias.  Bars: head_oracle's
docstring (gamma_n from operation counts; the project's own 2e-6 bars behind expf / logf); pooled and logits bit for bit on the
exact rows.  Rows whose targets lie outside [0, K): loss 0, dl = 0 (exactly zero dfeat rows, dW / dbias without them), on the staged
and the unstaged path.  Then the two roles against the launches they replace, bit for bit, and a captured forward -> backward chain.

Measured on an MI355X (worst error / bar: pooled logits | loss probs ce_mean | dfeat dW dbias; the worse of g = 1.0 and 0.37):
    128x64x64x10           .027 .031 | .088 .040 .005 | .259 .011 .014   trans_total .704
    80x64x64x10            .026 .029 | .078 .036 .039 | .211 .020 .023   trans_total .244
    1x1x1x1                .000 .296 | .000 .000 .000 | .000 .000 .000   trans_total .865
    3x5x3x2                .121 .215 | .018 .016 .004 | .263 .119 .106   trans_total .525
    7x49x100x31            .035 .017 | .050 .010 .006 | .162 .269 .218   trans_total .783
    5x200x256x64           .034 .006 | .090 .018 .029 | .099 .302 .247   trans_total .736
    2x1x256x64             .000 .010 | .058 .038 .042 | .106 .326 .208   trans_total .424
    130x16x8x5             .163 .222 | .067 .045 .007 | .266 .013 .019   trans_total .352
    1025x1x4x3             .000 .385 | .100 .096 .012 | .422 .001 .001   trans_total .716
    128x64x32x10-exact     .000 .000 | .091 .054 .017 | .222 .011 .021   trans_total .834
    16x32x256x64-exact     .000 .000 | .048 .068 .003 | .161 .301 .138   trans_total .398
    3x5x3x2-nobias         .124 .339 | .046 .026 .009 | .150 .170 .136   trans_total .525
    7x49x100x31-nobias     .040 .015 | .058 .013 .004 | .143 .238 .215   trans_total .783
    80x64x64x10-oor        .026 .039 | .070 .036 .014 | .274 .028 .018   trans_total .244
    1025x1x4x3-oor         .000 .366 | .107 .070 .024 | .323 .002 .002   trans_total .716
pooled and logits were bit-equal to the float64 result on both exact rows; every role and the captured chain were bit-equal to the
launches they replace.  Against the library before the out-of-range rule (dl = g / B * probs for such rows) the four cases with
out-of-range targets fail (80x64x64x10-oor, 1025x1x4x3-oor, and the role at 1025x1x4x3-oor with 1 and 33 sites).  Libraries with one
planted defect each: the pooling's tail loop dropped failed 9 of the 25 cases here, the dW role's tail loop dropped failed 11.
"""
import numpy as np
import pytest
import torch

from tests import head_oracle as H
from tests.test_gpu_dwconv import SENTINEL, Arena

pytestmark = pytest.mark.gpu

NAMES = ("pooled", "logits", "probs", "loss", "ce", "trans", "dfeat", "dW", "dbias")
# (row, exact, bias, out-of-range targets)
CASES = ([(s, False, True, False) for s, _ in H.ROWS] + [(s, True, True, False) for s, _ in H.EXACT_ROWS]
         + [((3, 5, 3, 2), False, False, False), ((7, 49, 100, 31), False, False, False)]
         + [((80, 64, 64, 10), False, True, True), ((1025, 1, 4, 3), False, True, True)])
CASE_IDS = [H.row_id(s) + ("-exact" if e else "") + ("" if b else "-nobias") + ("-oor" if o else "") for s, e, b, o in CASES]


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


def written(a):
    return bool((bits(a) != SENTINEL).all())


class Head:
    """the head's launches on one case; windows: pooled, logits, probs, loss, ce_mean, trans_total, dfeat, dW, dbias"""

    def __init__(self, dev, case):
        from alignq_amd import _lib as L
        self.L, self.lib, self.dev, self.case = L, L.load(), dev, case
        self.B, self.HW, self.C, self.K = B, HW, C, K = case["shape"]
        self.arena = Arena(dev, [B * C, B * K, B * K, B, 1, 1, B * HW * C, K * C, K])
        self.feat, self.W, self.bias, self.target = (cu(case[n], dev) for n in ("feat", "W", "bias", "target"))
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        rng = np.random.default_rng(B + C)
        self.scal_host = rng.random((65, 4)).astype(np.float32)
        self.scal = cu(self.scal_host, dev)

    def views(self):
        return dict(zip(NAMES, self.arena.views))

    def shapes(self, out):
        B, HW, C, K = self.case["shape"]
        sh = dict(pooled=(B, C), logits=(B, K), probs=(B, K), loss=(B,), ce=(1,), trans=(1,), dfeat=(B, HW, C), dW=(K, C), dbias=(K,))
        return {n: out[n].reshape(sh[n]) for n in NAMES}

    def launch_fwd(self, form, n_sites=0):
        v = self.views()
        ce = ptr(v["ce"]) if form != "loss" else None
        counter = ptr(self.counter) if form != "loss" else None
        scal, trans = (ptr(self.scal), ptr(v["trans"])) if form == "trans" else (None, None)
        return self.lib.alignq_head_ce_fwd(ptr(self.feat), ptr(self.W), ptr(self.bias), ptr(self.target), self.B, self.HW, self.C, self.K,
                                           ptr(v["pooled"]), ptr(v["logits"]), ptr(v["probs"]), ptr(v["loss"]), ce, counter, scal,
                                           n_sites if form == "trans" else 0, trans, self.L.stream_ptr())

    def fwd(self, form, n_sites=0):
        """form: 'loss' (ce_mean, counter, site_scal NULL) | 'ce' (ce_mean + counter) | 'trans' (+ site_scal / trans_total)"""
        self.arena.reset()
        rc = self.launch_fwd(form, n_sites)
        torch.cuda.synchronize()
        assert rc == 0, rc
        out = self.shapes(dict(zip(NAMES, self.arena.get())))                  # (asserts the guards)
        assert int(self.counter.item()) == 0, "the ticket was not re-armed"
        for n in ("pooled", "logits", "probs", "loss"):
            assert written(out[n]), f"{form}: {n} has unwritten elements"
        assert written(out["ce"]) == (form != "loss") and untouched(out["ce"]) == (form == "loss")
        assert written(out["trans"]) == (form == "trans") and untouched(out["trans"]) == (form != "trans")
        assert untouched(out["dfeat"]) and untouched(out["dW"]) and untouched(out["dbias"])
        return out

    def launch_bwd(self, g, probs, pooled, want_dbias=True):
        v = self.views()
        return self.lib.alignq_head_ce_bwd(ptr(g), ptr(probs), ptr(self.target), ptr(pooled), ptr(self.W), self.B, self.HW, self.C, self.K,
                                           ptr(v["dfeat"]), ptr(v["dW"]), ptr(v["dbias"]) if want_dbias else None, self.L.stream_ptr())

    def bwd(self, g, probs, pooled, want_dbias=True):
        self.arena.reset()
        rc = self.launch_bwd(g, probs, pooled, want_dbias)
        torch.cuda.synchronize()
        assert rc == 0, rc
        out = self.shapes(dict(zip(NAMES, self.arena.get())))
        assert written(out["dfeat"]) and written(out["dW"]), "dfeat / dW have unwritten elements"
        assert written(out["dbias"]) if want_dbias else untouched(out["dbias"])
        for n in NAMES[:6]:
            assert untouched(out[n])
        return out


def twice(run, *a, **kw):
    out, again = run(*a, **kw), run(*a, **kw)
    for n in NAMES:
        assert same(out[n], again[n]), f"second launch differs in {n}"
    return out


def check_forward(head, out):
    """worst error / bar of (pooled, logits, loss, probs); asserts nothing but the exact rows' bit equality"""
    case = head.case
    w = {}
    w["pooled"] = H.worst(out["pooled"], *H.pooled_ref(case["feat"]))
    w["logits"] = H.worst(out["logits"], *H.logits_ref(out["pooled"], case["W"], case["bias"]))
    loss, probs, ce = H.softmax_ref(out["logits"], case["target"])
    w["loss"] = H.worst(out["loss"], loss, 2e-6 * np.maximum(1.0, np.abs(loss)))
    w["probs"] = H.worst(out["probs"], probs, 2e-6)
    return w, ce


def check_ce(out, ce_ref):
    got = float(out["ce"][0])
    w = abs(got - ce_ref) / (2e-6 * max(1.0, abs(ce_ref)))
    assert abs(got - float(out["loss"].astype(np.float64).mean())) <= 1e-6, "ce_mean is not the mean of the stored losses"
    return w


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_forward_and_backward_forms(dev, i):
    shape, exact, with_bias, oor = CASES[i]
    B, HW, C, K = shape
    case = H.make_case(shape, i, exact=exact, bias=with_bias, oor=oor)
    head = Head(dev, case)
    # ---- forward: three forms
    a = twice(head.fwd, "loss")
    b = twice(head.fwd, "ce")                                     # (the same counter word serves both launches)
    w, ce_ref = check_forward(head, a)
    w["ce"] = check_ce(b, ce_ref)
    w["trans"] = 0.0
    for n_sites in (1, 21, 65):
        c = twice(head.fwd, "trans", n_sites)
        for n in ("pooled", "logits", "probs", "loss", "ce"):
            assert same(b[n], c[n]), f"n_sites {n_sites}: {n} differs from the ce_mean form"
        w["trans"] = max(w["trans"], H.worst(c["trans"], *H.trans_ref(head.scal_host, n_sites)))
    for n in ("pooled", "logits", "probs", "loss"):
        assert same(a[n], b[n]), f"{n} differs between the loss-only and the ce_mean form"
    # ---- backward from the device's own probs and pooled
    probs_d, pooled_d = cu(a["probs"], dev), cu(a["pooled"], dev)
    wb = dict(dfeat=0.0, dW=0.0, dbias=0.0)
    outs = {}
    for g in (1.0, 0.37):
        gd = torch.tensor([g], dtype=torch.float32, device=dev)
        full = twice(head.bwd, gd, probs_d, pooled_d, True)
        lean = twice(head.bwd, gd, probs_d, pooled_d, False)
        assert same(full["dfeat"], lean["dfeat"]) and same(full["dW"], lean["dW"]), "dfeat / dW change with dbias == NULL"
        ref = H.backward(g, a["probs"], a["pooled"], case["W"], case["target"], HW)
        wb["dfeat"] = max(wb["dfeat"], H.worst(full["dfeat"], ref["dfeat"][:, None, :], ref["bar_dfeat"][:, None, :]))
        wb["dW"] = max(wb["dW"], H.worst(full["dW"], ref["dW"], ref["bar_dW"]))
        wb["dbias"] = max(wb["dbias"], H.worst(full["dbias"], ref["dbias"], ref["bar_dbias"]))
        outs[g] = full
    print(f"[head-forms] {CASE_IDS[i]}: worst error / bar  pooled {w['pooled']:.3f} logits {w['logits']:.3f} | loss {w['loss']:.3f} "
          f"probs {w['probs']:.3f} ce_mean {w['ce']:.3f} trans {w['trans']:.3f} | dfeat {wb['dfeat']:.3f} dW {wb['dW']:.3f} "
          f"dbias {wb['dbias']:.3f}")
    if exact:
        fw = H.forward(case)
        assert same(a["pooled"], fw["pooled"].astype(np.float32)), "exact row: pooled is not the float64 result rounded to fp32"
        assert same(a["logits"], fw["logits"].astype(np.float32)), "exact row: logits are not the float64 result rounded to fp32"
    assert max(w.values()) <= 1.0, w
    if oor:
        rows = list(H.oor_rows(B))
        assert (~H.valid_rows(case["target"], K)).sum() == 3
        assert not a["loss"][rows].any() and not np.isnan(a["loss"][rows]).any(), "out-of-range target: loss must be 0"
        for g, full in outs.items():
            z = full["dfeat"][rows]
            assert not np.isnan(z).any() and not z.any(), f"g = {g}: out-of-range target: dfeat rows must be exactly zero"
    assert max(wb.values()) <= 1.0, wb


# ------------------------------------------------------------------------------------------------ the roles
def _sites(dev, S, seed, B=128, dim=128):
    g = torch.Generator(device="cpu").manual_seed(seed)
    D = [torch.randn(B, B, generator=g).to(dev) * 0.05 for _ in range(S)]
    A = [torch.randn(dim, dim, generator=g).to(dev) * 0.05 for _ in range(S)]
    Gm = [torch.rand(dim, dim, generator=g).to(dev) * 0.01 for _ in range(S)]
    scal = [torch.rand(4, generator=g).to(dev) for _ in range(S)]
    Fs = [(16384, 8192, 4096)[s % 3] for s in range(S)]
    return D, A, Gm, scal, Fs


@pytest.mark.parametrize("S", [1, 33])
@pytest.mark.parametrize("shape,oor", [((128, 64, 64, 10), False), ((7, 49, 100, 31), False), ((1025, 1, 4, 3), True)],
                         ids=["128x64x64x10", "7x49x100x31", "1025x1x4x3-oor"])
def test_backward_as_a_role_of_the_site_preparation(dev, shape, oor, S):
    """alignq_head_ce_bwd_site_prep == alignq_head_ce_bwd + alignq_site_prep_fused_multi, bit for bit; 33 sites cross the 32 that
    ride with the head"""
    from alignq_amd import _lib as L
    lib = L.load()
    B, dim = 128, 128
    case = H.make_case(shape, 40 + S, oor=oor)
    head = Head(dev, case)
    fw = head.fwd("loss")
    probs_d, pooled_d = cu(fw["probs"], dev), cu(fw["pooled"], dev)
    gce = torch.tensor([0.37], dtype=torch.float32, device=dev)
    gtr = torch.tensor([0.7], dtype=torch.float32, device=dev)
    alone = head.bwd(gce, probs_d, pooled_d, True)
    D, A, Gm, scal, Fs = _sites(dev, S, 7 * S + shape[0])
    nS = lib.alignq_site_bwd_ws_bytes(B) // 4
    f32 = dict(dtype=torch.float32, device=dev)

    def outs():
        return ([torch.zeros(nS, **f32) for _ in range(S)], [torch.zeros(dim, dim, **f32) for _ in range(S)],
                [torch.zeros(dim, dim, **f32) for _ in range(S)])

    def site(o):
        return (S, L.ptr_array(D), L.ptr_array(A), L.ptr_array(Gm), L.ptr_array(scal), ptr(gtr), L.i64_array(Fs), B, dim, 0.01,
                L.ptr_array(o[0]), L.ptr_array(o[1]), L.ptr_array(o[2]), L.stream_ptr())

    o1, o2 = outs(), outs()
    assert lib.alignq_site_prep_fused_multi(*site(o1)) == 0
    head.arena.reset()
    v = head.views()
    rc = lib.alignq_head_ce_bwd_site_prep(ptr(gce), ptr(probs_d), ptr(head.target), ptr(pooled_d), ptr(head.W), head.B, head.HW, head.C,
                                          head.K, ptr(v["dfeat"]), ptr(v["dW"]), ptr(v["dbias"]), *site(o2))
    torch.cuda.synchronize()
    assert rc == 0, rc
    merged = head.shapes(dict(zip(NAMES, head.arena.get())))
    for n in NAMES:
        assert same(alone[n], merged[n]), f"{n} differs between the role and the stand-alone launch"
    assert written(merged["dfeat"]) and written(merged["dW"]) and written(merged["dbias"])
    for s in range(S):
        for x, y, what in zip((o1[0][s], o1[1][s], o1[2][s]), (o2[0][s], o2[1][s], o2[2][s]), ("S", "dalterD", "dgamma")):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"site {s}: {what}"
        assert o2[0][s].abs().sum().item() > 0
    if oor:
        z = merged["dfeat"][list(H.oor_rows(shape[0]))]
        assert not np.isnan(z).any() and not z.any()


@pytest.mark.parametrize("HB", [1, 80, 128])
def test_forward_as_a_role_of_the_closing_reduction(dev, HB):
    """alignq_site_reduce_loss_multi_head == alignq_site_reduce_loss_multi + alignq_head_ce_fwd, bit for bit: the head's outputs, each
    site's D / scal and trans_total; two sites of [128, 64] whose workspaces alignq_site_partials filled, each path on its own copy"""
    from alignq_amd import _lib as L
    lib = L.load()
    B, F, S, dim = 128, 64, 2, 128
    st = L.stream_ptr()
    f32 = dict(dtype=torch.float32, device=dev)
    rng = np.random.default_rng(HB)
    ws_bytes = int(lib.alignq_site_ws_bytes(B, F))
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    ws = []
    for s in range(S):
        x = cu((rng.standard_normal((B, F)) * 1.2).astype(np.float32), dev)
        xq, stats = torch.empty_like(x), torch.empty(4, F, **f32)
        w = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
        assert lib.alignq_site_partials(ptr(x), B, F, 8, 2.0, 0.0, ptr(xq), ptr(stats), ptr(w), st) == 0
        ws.append(w)
    torch.cuda.synchronize()
    A = [cu((rng.standard_normal((dim, dim)) * 0.05).astype(np.float32), dev) for _ in range(S)]
    Gm = [cu((rng.standard_normal((dim, dim)) * 0.05).astype(np.float32), dev) for _ in range(S)]
    Fs = L.i64_array([F] * S)
    case = H.make_case((HB, 64, 64, 10), 60 + HB)
    results = []
    for role in (False, True):
        head = Head(dev, case)
        my_ws = [w.clone() for w in ws]
        D = [torch.zeros(B, B, **f32) for _ in range(S)]
        scal_all = torch.full((S, 4), -1.0, **f32)
        scal = [scal_all[s] for s in range(S)]
        counters = torch.zeros(2, dtype=torch.int32, device=dev)
        v = head.views()
        sites = (S, L.ptr_array(my_ws), L.ptr_array(D), L.ptr_array(A), L.ptr_array(Gm), L.ptr_array(scal), Fs, B, dim, 0.2, 0.3)
        hd = (ptr(head.feat), ptr(head.W), ptr(head.bias), ptr(head.target), HB, 64, 64, 10, ptr(v["pooled"]), ptr(v["logits"]),
              ptr(v["probs"]), ptr(v["loss"]), ptr(v["ce"]), ptr(counters))
        if role:
            rc = lib.alignq_site_reduce_loss_multi_head(*sites, *hd, ptr(scal_all), S, ptr(v["trans"]), ptr(counters[1:]), st)
        else:
            rc = lib.alignq_site_reduce_loss_multi(*sites, st)
            assert rc == 0, rc
            rc = lib.alignq_head_ce_fwd(*hd[:4], HB, 64, 64, 10, *hd[8:], ptr(scal_all), S, ptr(v["trans"]), st)
        torch.cuda.synchronize()
        assert rc == 0, rc
        assert counters.cpu().tolist() == [0, 0], "a ticket was not re-armed"
        out = head.shapes(dict(zip(NAMES, head.arena.get())))
        for n in NAMES[:6]:
            assert written(out[n]), n
        results.append((out, [d.cpu().numpy() for d in D], scal_all.cpu().numpy()))
    (o1, D1, s1), (o2, D2, s2) = results
    for n in NAMES:
        assert same(o1[n], o2[n]), f"{n} differs between the role and the stand-alone launch"
    for s in range(S):
        assert same(D1[s], D2[s]) and np.abs(D1[s]).sum() > 0, f"site {s}: D"
    assert same(s1, s2) and (s1 != -1.0).all()
    assert H.worst(o2["trans"], *H.trans_ref(s2, S)) <= 1.0
    w, ce_ref = check_forward(Head(dev, case), o2)
    assert max(w.values()) <= 1.0 and check_ce(o2, ce_ref) <= 1.0, w


# ------------------------------------------------------------------------------------------------ captured replay
def test_captured_chain_replays_to_the_eager_bits(dev):
    """forward in the ce_mean form, then the backward from the probs / pooled it left: one stream, a chain"""
    case = H.make_case((7, 49, 100, 31), 90)
    head = Head(dev, case)                                  # arena, counter and scalars exist before the capture
    gd = torch.tensor([0.37], dtype=torch.float32, device=dev)

    def chain():
        v = head.views()
        return [head.launch_fwd("ce"), head.launch_bwd(gd, v["probs"], v["pooled"], True)]

    head.arena.reset()
    assert chain() == [0, 0]
    torch.cuda.synchronize()
    eager = head.arena.get()
    assert all(written(eager[NAMES.index(n)]) for n in NAMES if n != "trans")
    head.arena.reset()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert head.L.stream_ptr() == side.cuda_stream
        rcs = chain()
    assert rcs == [0, 0]
    for _ in range(2):
        head.arena.reset()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(head.arena.get(), eager):
            assert same(got, want)
        assert int(head.counter.item()) == 0
