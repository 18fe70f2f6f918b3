"""Packed k-bit weight checkpoints on the GPU (csrc/pack_kernels.hip, alignq_amd/export.py, EvalStep(weights=)).

The codes alignq_weight_pack_multi writes are compared bit for bit with the NumPy statement of the format (tests/packed_oracle.py)
applied to the quantiser's own W_q; what alignq_weight_unpack_multi writes is compared bit for bit with W_q + 0.0 (a code has no sign
of zero), with alignq_qconv_pack_weights' bins of that W_q, and with the filter-image layout of tests/filter_image_oracle.py; an
evaluation from a saved and re-loaded PackedModel on a skeleton whose filters are NaN equals the evaluation of the trained model.

Every buffer a launch writes is a window of one byte arena: 0xFF inside (an unwritten fp32 element stays a NaN no kernel here makes),
0xA5 in the 256 bytes around it."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import filter_image_oracle as FO
from tests import packed_oracle as PO

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE, PREFILL = 256, 0xA5, 0xFF
SIZES = [1, 31, 32, 33, 432, 2304, 36869]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from alignq_amd import _lib
    _lib.load()
    return _lib


class Windows:
    """windows of the given byte sizes in one arena, each 16-byte aligned, between guards"""

    def __init__(self, dev, nbytes):
        self.offs, off = [], 0
        for n in nbytes:
            off = (off + GUARD + 15) // 16 * 16
            self.offs.append(off)
            off += n
        self.nbytes, self.total = list(nbytes), off + GUARD
        host = np.full(self.total, GUARD_BYTE, dtype=np.uint8)
        for o, n in zip(self.offs, self.nbytes):
            host[o:o + n] = PREFILL
        self.buf = torch.from_numpy(host.copy()).to(dev)
        assert self.buf.data_ptr() % 16 == 0

    def view(self, i, dtype):
        return self.buf[self.offs[i]:self.offs[i] + self.nbytes[i]].view(dtype)

    def views(self, dtype):
        return [self.view(i, dtype) for i in range(len(self.offs))]

    def get(self, dtype):
        """the windows' contents as `dtype`; asserts that every guard byte is intact"""
        host = self.buf.cpu().numpy()
        inside = np.zeros(self.total, bool)
        for o, n in zip(self.offs, self.nbytes):
            inside[o:o + n] = True
        assert np.all(host[~inside] == GUARD_BYTE), "a kernel wrote outside its buffer"
        return [host[o:o + n].copy().view(dtype) for o, n in zip(self.offs, self.nbytes)]


def _quantise(L, dev, sizes, k, formula, seed):
    """W_q (flat CUDA fp32 tensors of the given sizes) from ONE alignq_weight_quant_fwd_multi call on randn * 0.05.  The quantiser
    takes no tensor of fewer than two elements (its standard deviation divides by n - 1): a size of 1 is the first element of a
    two-element tensor's W_q."""
    lib = L.load()
    g = torch.Generator().manual_seed(seed)
    ws = [(torch.randn(max(n, 2), generator=g) * 0.05).to(dev) for n in sizes]
    qs = [torch.full_like(w, float("nan")) for w in ws]
    T = len(ws)
    ms = torch.empty(T, 2, device=dev)
    scratch = torch.empty(lib.alignq_weight_multi_ws_bytes(T), dtype=torch.uint8, device=dev)
    L.check(lib.alignq_weight_quant_fwd_multi(T, L.ptr_array(ws), L.ptr_array(qs), None, None, L.i64_array([w.numel() for w in ws]),
                                              L.ptr(ms), k, formula, L.ptr(scratch), L.stream_ptr()), "fwd_multi")
    torch.cuda.synchronize()
    return [q[:n] for q, n in zip(qs, sizes)]


def _pack(L, dev, qs, k, formula):
    """(code words per tensor as uint32 arrays, bad) of one alignq_weight_pack_multi call into guarded windows"""
    lib = L.load()
    bits = lib.alignq_weight_code_bits(k, formula)
    sizes = [lib.alignq_packed_bytes(q.numel(), bits) for q in qs]
    assert sizes == [4 * PO.packed_words(q.numel(), bits) for q in qs]
    win = Windows(dev, sizes)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(lib.alignq_weight_pack_multi(len(qs), L.ptr_array(qs), L.i64_array([q.numel() for q in qs]), k, formula,
                                         L.ptr_array(win.views(torch.int32)), L.ptr(bad), L.stream_ptr()), "pack")
    torch.cuda.synchronize()
    return win.get(np.uint32), int(bad.item()), win


def _unpack_q(L, dev, code_tensors, numels, k, formula):
    win = Windows(dev, [4 * n for n in numels])
    L.check(L.load().alignq_weight_unpack_multi(len(numels), L.ptr_array(code_tensors), L.i64_array(numels), k, formula,
                                                L.ptr_array(win.views(torch.float32)), None, None, None, None, L.stream_ptr()), "unpack")
    torch.cuda.synchronize()
    return win.get(np.float32)


def _plus_zero_bits(q):
    return (q + np.float32(0)).view(np.uint32)


# --------------------------------------------------------------------------------------------------------------------- 1. pack
@pytest.mark.parametrize("k", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("formula", [0, 1])
@pytest.mark.parametrize("form", ["T7", "T65"])
def test_pack_equals_the_oracle_bit_for_bit(L, dev, k, formula, form):
    """T7: the seven sizes in one call (a single element, one group less / exactly / more than one element, several workgroups, a
    size that is no multiple of 4 or 32 with several passes per workgroup).  T65: tiny tensors, the call crosses the 64-tensor chunk."""
    sizes = SIZES if form == "T7" else [1 + (7 * i) % 67 for i in range(65)]
    qs = _quantise(L, dev, sizes, k, formula, 31 * k + formula)
    bits = PO.code_bits(k, formula)
    words, bad, win = _pack(L, dev, qs, k, formula)
    assert bad == 0
    for q, got in zip(qs, words):
        qh = q.cpu().numpy()
        assert np.isfinite(qh).all()
        c = PO.codes(qh, k, formula)
        want = PO.pack(c, bits)
        assert got.shape == want.shape
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, (qh.size, diff[:8], got[diff[:8]], want[diff[:8]])
        assert np.array_equal(PO.dequant(c, k, formula).view(np.uint32), _plus_zero_bits(qh))      # the oracle's codes are W_q's
    # and back: W_q + 0.0, bit for bit, from the launch's own words
    back = _unpack_q(L, dev, win.views(torch.int32), sizes, k, formula)
    for q, b in zip(qs, back):
        assert np.array_equal(b.view(np.uint32), _plus_zero_bits(q.cpu().numpy()))


def test_pack_counts_values_without_a_code(L, dev):
    """one NaN and one off-grid value (0.3 at k = 2, ADMM tree: levels are thirds): bad == 2, their codes 0, every other code unchanged"""
    k, formula, n = 2, 0, 432
    q = _quantise(L, dev, [n], k, formula, 77)[0].clone()
    clean = PO.codes(q.cpu().numpy(), k, formula)
    q[5] = float("nan")
    q[100] = 0.3
    words, bad, _ = _pack(L, dev, [q], k, formula)
    assert bad == 2
    clean[5] = clean[100] = 0
    assert np.array_equal(words[0], PO.pack(clean, PO.code_bits(k, formula)))
    for v in (float("inf"), -float("inf"), 1.0 + 1.0 / 3.0, -2.0):        # non-finite and out of range
        q2 = q.clone()
        q2[7] = v
        assert _pack(L, dev, [q2], k, formula)[1] == 3


# --------------------------------------------------------------------------------------------------------------------- 2. unpack
def _flip(CO, KK, CI):
    return 1 if (KK == 9 and CO == CI) else 0


def _quantise_img(L, dev, k, formula, seed):
    """the seven image geometries (and an 1001-element tensor without image) through alignq_weight_quant_fwd_multi_img:
    (W_q list, geometries, the launch's own image buffers as uint16 arrays)"""
    lib = L.load()
    g = torch.Generator().manual_seed(seed)
    geos = [(CO, KK, CI, _flip(CO, KK, CI)) for CO, KK, CI in FO.GEOMETRIES] + [None]
    ws = [(torch.randn(1001 if ge is None else ge[0] * ge[1] * ge[2], generator=g) * 0.05).to(dev) for ge in geos]
    qs = [torch.full_like(w, float("nan")) for w in ws]
    T = len(ws)
    ms = torch.empty(T, 2, device=dev)
    scratch = torch.empty(lib.alignq_weight_multi_ws_bytes(T), dtype=torch.uint8, device=dev)
    imgs = [None if ge is None else torch.empty(lib.alignq_filter_image_bytes(*ge[:3]), dtype=torch.uint8, device=dev) for ge in geos]
    geom = []
    for ge in geos:
        geom += list(ge) if ge is not None else [0, 0, 0, 0]
    L.check(lib.alignq_weight_quant_fwd_multi_img(T, L.ptr_array(ws), L.ptr_array(qs), None, None, L.i64_array([w.numel() for w in ws]),
                                                  L.ptr(ms), k, formula, L.ptr(scratch), L.ptr_array(imgs),
                                                  (ctypes.c_int32 * len(geom))(*geom), L.stream_ptr()), "fwd_multi_img")
    torch.cuda.synchronize()
    return qs, geos, [None if im is None else im.cpu().numpy().view(np.uint16) for im in imgs]


def _geom_array(geos):
    flat = []
    for ge in geos:
        flat += list(ge) if ge is not None else [0, 0, 0, 0]
    return (ctypes.c_int32 * len(flat))(*flat)


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("formula", [0, 1])
def test_unpack_writes_wq_bins_and_images(L, dev, k, formula):
    lib = L.load()
    from alignq_amd import export
    qs, geos, own_imgs = _quantise_img(L, dev, k, formula, 13 * k + formula)
    T = len(qs)
    numels = [q.numel() for q in qs]
    codes, bad = export.pack_codes(qs, k, formula)
    assert bad == 0
    q0 = [q + 0.0 for q in qs]                                                     # -0 -> +0: what the codes can say
    qh = [q.cpu().numpy() for q in q0]
    # the bins alignq_qconv_pack_weights writes from W_q + 0.0 (it takes sizes that are multiples of 4: all but the last tensor)
    bf_ref = [torch.empty(n, dtype=torch.int16, device=dev) for n in numels[:-1]]
    hf_ref = [torch.empty(n, dtype=torch.int16, device=dev) for n in numels[:-1]]
    L.check(lib.alignq_qconv_pack_weights(T - 1, L.ptr_array(q0[:-1]), L.i64_array(numels[:-1]), k, L.ptr_array(bf_ref),
                                          L.ptr_array(hf_ref), L.stream_ptr()), "pack_weights")
    img_bytes = [0 if ge is None else lib.alignq_filter_image_bytes(*ge[:3]) for ge in geos]

    def run(q_on, bf_on, hf_on, img_on):
        """one unpack call; *_on: per tensor whether the entry is given (None: the whole table is NULL)"""
        wq, wb, wh = Windows(dev, [4 * n for n in numels]), Windows(dev, [2 * n for n in numels]), Windows(dev, [2 * n for n in numels])
        wi = Windows(dev, [max(b, 16) for b in img_bytes])

        def tab(win, on, dtype):
            return None if on is None else L.ptr_array([v if o else None for v, o in zip(win.views(dtype), on)])
        L.check(lib.alignq_weight_unpack_multi(T, L.ptr_array(codes), L.i64_array(numels), k, formula, tab(wq, q_on, torch.float32),
                                               tab(wb, bf_on, torch.int16), tab(wh, hf_on, torch.int16), tab(wi, img_on, torch.int16),
                                               _geom_array(geos), L.stream_ptr()), "unpack")
        torch.cuda.synchronize()
        return wq.get(np.uint32), wb.get(np.uint16), wh.get(np.uint16), wi.get(np.uint16)

    has_img = [ge is not None for ge in geos]
    all_on = [True] * T
    got_q, got_bf, got_hf, got_img = run(all_on, all_on, all_on, has_img)
    nlev = np.float32(2 ** k - 1)
    for t in range(T):
        assert np.array_equal(got_q[t], qh[t].view(np.uint32)), t
        if t < T - 1:
            assert np.array_equal(got_bf[t], bf_ref[t].cpu().numpy().view(np.uint16)), t
            assert np.array_equal(got_hf[t], hf_ref[t].cpu().numpy().view(np.uint16)), t
        else:       # n = 1001: a last thread with one element; the bins from their definition rint(W_q * n) as bf16 / f16 patterns
            b = np.rint(qh[t] * nlev)
            assert np.array_equal(got_bf[t], FO.bf16_bits(b)) and np.array_equal(got_hf[t], b.astype(np.float16).view(np.uint16))
        if geos[t] is not None:
            want = FO.images(qh[t], *geos[t], k)
            assert got_img[t].shape == want.shape
            diff = np.flatnonzero(got_img[t] != want)
            assert diff.size == 0, (geos[t], diff[:8])
            if formula == 1:                                   # no -0 in the CDF tree: the quantiser launch's own images
                assert np.array_equal(got_img[t], own_imgs[t])
    # NULL entries and NULL tables: nothing is written there, everything else as before
    q_on = [t != 0 for t in range(T)]
    bf_on = [t != 2 for t in range(T)]
    img_on = [h and t != 1 for t, h in enumerate(has_img)]
    part_q, part_bf, part_hf, part_img = run(q_on, bf_on, None, img_on)
    for t in range(T):
        assert np.array_equal(part_q[t], got_q[t]) if q_on[t] else np.all(part_q[t] == 0xFFFFFFFF)
        assert np.array_equal(part_bf[t], got_bf[t]) if bf_on[t] else np.all(part_bf[t] == 0xFFFF)
        assert np.all(part_hf[t] == 0xFFFF)
        assert np.array_equal(part_img[t], got_img[t]) if img_on[t] else np.all(part_img[t] == 0xFFFF)


def test_unpack_argument_checks(L, dev):
    lib = L.load()
    n = 16 * 9 * 16
    codes16 = torch.zeros(lib.alignq_packed_bytes(n, 17) // 4, dtype=torch.int32, device=dev)
    q = torch.empty(n, device=dev)
    half = torch.empty(n, dtype=torch.int16, device=dev)
    img = torch.empty(lib.alignq_filter_image_bytes(16, 9, 16), dtype=torch.uint8, device=dev)
    st = L.stream_ptr()

    def call(k, q_=None, bf=None, hf=None, im=None, geo=(16, 9, 16, 1)):
        one = lambda t: None if t is None else L.ptr_array([t])
        return lib.alignq_weight_unpack_multi(1, L.ptr_array([codes16]), L.i64_array([n]), k, 0, one(q_), one(bf), one(hf), one(im),
                                              (ctypes.c_int32 * 4)(*geo), st)
    assert call(16, q_=q) == 0
    assert call(16, q_=q, im=img) == L.EINVAL                       # bins beyond bf16's 8 significant bits
    assert call(9, q_=q, bf=half) == L.EINVAL and call(9, q_=q, hf=half) == L.EINVAL
    assert call(8, q_=q, im=img, geo=(16, 9, 32, 1)) == L.EINVAL    # the geometry does not match n
    assert call(8, q_=q, im=img, geo=(24, 6, 16, 0)) == L.EINVAL    # a geometry without images
    assert call(8) == L.EINVAL and call(17, q_=q) == L.EINVAL and call(0, q_=q) == L.EINVAL
    assert call(8, q_=q, bf=half, hf=half, im=img) == 0
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    assert lib.alignq_weight_pack_multi(1, L.ptr_array([q]), L.i64_array([n]), 17, 0, L.ptr_array([codes16]), L.ptr(bad), st) == L.EINVAL
    assert lib.alignq_weight_pack_multi(1, L.ptr_array([q]), L.i64_array([0]), 8, 0, L.ptr_array([codes16]), L.ptr(bad), st) == L.EINVAL
    assert lib.alignq_weight_pack_multi(1, L.ptr_array([q]), L.i64_array([n]), 8, 0, L.ptr_array([codes16]), None, st) == L.EINVAL
    torch.cuda.synchronize()


def test_unpack_replays_in_a_graph_and_follows_the_codes(L, dev):
    from alignq_amd import export
    k, formula = 4, 0
    geo = (32, 9, 32, 1)
    n = 32 * 9 * 32
    qa, qb = _quantise(L, dev, [n, n], k, formula, 5)
    (ca, cb), bad = export.pack_codes([qa, qb], k, formula)
    assert bad == 0 and not torch.equal(ca, cb)
    live = ca.clone()
    q = torch.full((n,), float("nan"), device=dev)
    bf, hf = (torch.full((n,), -1, dtype=torch.int16, device=dev) for _ in range(2))
    img = torch.full((L.load().alignq_filter_image_bytes(*geo[:3]),), 255, dtype=torch.uint8, device=dev)

    def launch():
        export.unpack_filters([live], [n], k, formula, qs=[q], bins_bf16=[bf], bins_f16=[hf], images=[img], geoms=[geo])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = [t.clone() for t in (q, bf, hf, img)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for t in (q, bf, hf, img):
        t.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, (q, bf, hf, img)))
    assert np.array_equal(q.cpu().numpy().view(np.uint32), _plus_zero_bits(qa.cpu().numpy()))
    live.copy_(cb)
    graph.replay()
    torch.cuda.synchronize()
    hb = (qb + 0.0).cpu().numpy()
    assert np.array_equal(q.cpu().numpy().view(np.uint32), hb.view(np.uint32))
    assert np.array_equal(bf.cpu().numpy().view(np.uint16), FO.bf16_bits(np.rint(hb * np.float32(15))))
    assert np.array_equal(img.cpu().numpy().view(np.uint16), FO.images(hb, *geo, k))


# --------------------------------------------------------------------------------------------------------------------- 3. models
def _randomise_bn(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)


def _packed_eval_equals_dense(dev, monkeypatch, tmp_path, make, x, y, want_bins, want_images):
    """EvalStep(skeleton, weights=packed file) against EvalStep(trained net): logits, counts, captured replay, launch counts"""
    from alignq_amd import export, fused
    from alignq_amd.eval_step import EvalStep
    torch.manual_seed(1)
    net = make().to(dev)
    _randomise_bn(net, 2)
    with EvalStep(net) as ev0:
        want = ev0(x, y).clone()
        want_counts = ev0.counts()
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and want_counts[3] == x.shape[0]

    path = os.path.join(tmp_path, "net.alignq")
    pk = export.pack_model(net)
    admm = {k for k in net.state_dict() if k.endswith((".alterD", ".gamma"))}
    assert not (admm & set(pk.rest)) and set(pk.rest) | set(pk.filters) | admm == set(net.state_dict())
    assert admm <= set(export.pack_model(net, keep_admm=True).rest)
    pk.save(path)
    dense = os.path.join(tmp_path, "dense.pt")
    torch.save(net.state_dict(), dense)
    print("file sizes: packed %d B, dense state_dict %d B; nbytes %d, dense_nbytes %d"
          % (os.path.getsize(path), os.path.getsize(dense), pk.nbytes(), pk.dense_nbytes()))
    assert os.path.getsize(path) < os.path.getsize(dense) and pk.nbytes() < pk.dense_nbytes()
    pk = export.PackedModel.load(path)
    assert all(not f["codes"].is_cuda for f in pk.filters.values())

    torch.manual_seed(3)
    skeleton = make().to(dev)
    pk.apply(skeleton)
    named = export.quantised_convs(skeleton)
    assert named and set(n for n, _ in named) == set(pk.filters)
    with torch.no_grad():
        for _, c in named:
            c.weight.fill_(float("nan"))                  # whoever reads an fp32 filter value poisons the logits

    # one dequantised filter: logical shape, channels-last memory, the quantiser's values
    name, conv = export.quantised_convs(net)[1]
    fused.prequantize_weights([conv])
    wq = conv.quantize_fn.parked.q.detach() + 0.0
    conv.quantize_fn.unpark()
    deq = pk.dequantize(name)
    assert deq.shape == conv.weight.shape and deq.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(deq.view(torch.int32), wq.view(torch.int32))

    calls = {"prequantize": 0, "unpack": 0, "bins": 0, "images": 0}
    real_pre, real_unpack = fused.prequantize_weights, export.unpack_filters
    monkeypatch.setattr(fused, "prequantize_weights", lambda *a, **kw: (calls.__setitem__("prequantize", calls["prequantize"] + 1),
                                                                        real_pre(*a, **kw))[1])
    monkeypatch.setattr(export, "unpack_filters", lambda *a, **kw: (calls.__setitem__("unpack", calls["unpack"] + 1),
                                                                    real_unpack(*a, **kw))[1])
    qcls = type(named[0][1].quantize_fn)
    real_filter_of = qcls.filter_of

    def counting(self, wq_):
        rec = real_filter_of(self, wq_)
        calls["bins"] += rec.bins is not None
        calls["images"] += rec.image is not None
        return rec
    monkeypatch.setattr(qcls, "filter_of", counting)

    ev = EvalStep(skeleton, weights=pk)
    with ev:
        assert calls["unpack"] == 1 and calls["prequantize"] == 0
        got = ev(x, y).clone()
        assert ev.counts() == want_counts
        ev.capture(x, y)
        graph = ev._graph
        assert graph is not None
        replayed = ev(x, y).clone()
        torch.cuda.synchronize()
        parked = [c.quantize_fn.parked.q for _, c in named]
    assert torch.equal(got, want)
    assert torch.equal(replayed, want)
    if want_bins:
        assert calls["bins"] >= 1
    if want_images:
        assert calls["images"] >= 1
    # a second evaluation: the same tensors refreshed (they are spoiled in between), the same graph replayed
    for t in parked:
        t.fill_(float("nan"))
    with ev:
        assert calls["unpack"] == 2 and calls["prequantize"] == 0
        assert ev._graph is graph
        assert all(c.quantize_fn.parked.q is t for (_, c), t in zip(named, parked))
        again = ev(x, y).clone()
        assert ev.counts() == want_counts
    assert torch.equal(again, want)
    with torch.no_grad():
        assert all(bool(torch.isnan(c.weight).all()) for _, c in named)          # apply() and the step left the filters alone


@pytest.mark.parametrize("bits", [8, 2])
@pytest.mark.parametrize("tree", ["admm", "cdf"])
def test_cifar_model_evaluates_from_the_packed_file(dev, monkeypatch, tmp_path, tree, bits):
    from alignq_amd import config
    from alignq_amd.resnet import PreActBlock_conv_Q, PreActResNet
    old = (config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size)
    config.args.bitW = config.args.abitW = bits
    config.args.train_batch_size = config.args.eval_batch_size = 16
    try:
        g = torch.Generator().manual_seed(40 + bits)
        x = torch.randn(16, 3, 32, 32, generator=g).to(dev)
        y = torch.randint(0, 10, (16,), generator=g).to(dev)
        _packed_eval_equals_dense(dev, monkeypatch, tmp_path,
                                  lambda: PreActResNet(PreActBlock_conv_Q, [1, 1, 1], bits, bits, "second", 10, tree=tree), x, y,
                                  want_bins=False, want_images=True)
    finally:
        config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size = old


def test_office_model_evaluates_from_the_packed_file(dev, monkeypatch, tmp_path):
    """DANN on a one-block-per-stage bottleneck ResNet at the default width (channels 64..2048): the GEMM convolutions and their
    pre-packed bins are really used"""
    from alignq_amd import config
    from alignq_amd.resnet_office import DANN, Bottleneck, ResNet
    old = (config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size)
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = config.args.eval_batch_size = 8
    try:
        g = torch.Generator().manual_seed(50)
        x = torch.randn(8, 3, 224, 224, generator=g).to(dev)
        y = torch.randint(0, 31, (8,), generator=g).to(dev)
        _packed_eval_equals_dense(dev, monkeypatch, tmp_path,
                                  lambda: DANN(lambda w, a, s: ResNet(w, a, s, Bottleneck, [1, 1, 1, 1]), 8, 8, "aligned"), x, y,
                                  want_bins=True, want_images=False)
    finally:
        config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size = old


def test_eval_step_refuses_weights_that_do_not_fit(dev, tmp_path):
    from alignq_amd import config, export
    from alignq_amd.eval_step import EvalStep
    from alignq_amd.resnet import PreActBlock_conv_Q, PreActResNet
    old = config.args.train_batch_size
    config.args.train_batch_size = 16
    try:
        def make(wbit=8, tree="admm"):
            return PreActResNet(PreActBlock_conv_Q, [1, 1, 1], wbit, 8, "second", 10, tree=tree).to(dev)
        pk = export.pack_model(make())
        with pytest.raises(ValueError, match="channels_last"):
            EvalStep(make(), channels_last=False, weights=pk)
        with pytest.raises(ValueError, match="layers.0.conv0.weight"):
            EvalStep(make(wbit=4), weights=pk)                                    # a wrong w_bit
        fewer = export.PackedModel(pk.meta, {k: v for k, v in pk.filters.items() if k != "layers.2.skip_conv.weight"}, pk.rest)
        with pytest.raises(ValueError, match="no packed filter for layers.2.skip_conv.weight"):
            EvalStep(make(), weights=fewer)
        with pytest.raises(ValueError, match="formula"):
            EvalStep(make(tree="cdf"), weights=pk)
        bad = make()
        with torch.no_grad():
            bad.layers[1].conv1.weight[3, 2, 1, 1] = float("nan")
        with pytest.raises(ValueError, match="layers.1.conv1.weight"):
            export.pack_model(bad)
        torch.cuda.synchronize()
    finally:
        config.args.train_batch_size = old
