"""DenseNet's training without concatenations (include/alignq_dense_train.h, fused.DenseBlockFn, `fuse_dense_train`): each of the five
operations bit for bit against the launch it replaces run on contiguous copies, the model against a twin under `train_sites=True`, and
the block against a float64 CPU twin."""
import pytest
import torch

from tests.test_gpu_dwconv import _count, dev  # noqa: F401  (dev: the fixture)
from tests.test_gpu_train_sites import dense_block, float64_twin

pytestmark = pytest.mark.gpu
B, H, W = 2, 9, 10          # partial 8 x 8 tiles on both axes, partial 4 x 8 filter-gradient tiles
P = B * H * W
SENTINEL = -777.25
# (CIN, COUT, spare channels behind the layer's, formula, a_bit): CIN = one partial chunk, one chunk + a tail, two chunks + a tail
# (the statistics' L = 1, 9, 17); pitch CIN + COUT and a wider one; both formulas at 4 bits, one 8-bit case
CASES = [(cin, cout, spare, "CDF", 4) for cin in (4, 36, 68) for cout in (12, 40) for spare in (0, 8)]
CASES += [(36, 12, 0, "ADMM", 4), (68, 40, 8, "ADMM", 4), (36, 12, 8, "CDF", 8)]


@pytest.mark.parametrize("cin,cout,spare,formula,k", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_each_operation_has_the_bits_of_the_launch_it_replaces(dev, cin, cout, spare, formula, k):
    from alignq_amd import _lib as L
    from alignq_amd import ops
    lib, st = L.load(), L.stream_ptr()
    formula = getattr(L, "FORMULA_" + formula)
    ld, r, w_bit, relu = cin + cout + spare, 2.0, 4, L.CLAMP_RELU
    g = torch.Generator(device=dev).manual_seed(1000 * cin + 10 * cout + spare + k)
    f32 = dict(dtype=torch.float32, device=dev)
    rnd = lambda *s: torch.randn(*s, generator=g, **f32)      # noqa: E731
    call = lambda name, *a: L.check(getattr(lib, name)(*a, st), name)      # noqa: E731

    def byt(n):
        return torch.empty(n, dtype=torch.uint8, device=dev)

    buf = torch.full((P, ld), SENTINEL, **f32)
    buf[:, :cin] = rnd(P, cin) * 1.5 + 0.3
    buf0, zc = buf.clone(), buf[:, :cin].contiguous()
    gamma, beta = torch.rand(cin, generator=g, **f32) + 0.5, rnd(cin) * 0.2
    n = 2 ** w_bit - 1
    wq = (torch.randint(-n, n + 1, (cout, cin, 3, 3), generator=g, device=dev).float() / n).contiguous(memory_format=torch.channels_last)
    bins = ops.pack_filter_bins([wq], w_bit)[0][0]
    stats = lambda: [torch.zeros(cin, **f32), torch.ones(cin, **f32), torch.zeros((), dtype=torch.int64, device=dev)]      # noqa: E731
    new4 = lambda: [torch.empty(2, cin, **f32) for _ in range(2)]      # noqa: E731

    # the launches replaced, on contiguous copies
    (ab, save), run, y = new4(), stats(), torch.empty(P, cin, **f32)
    mask, ws = byt(lib.alignq_bnq_any_mask_bytes(P, cin)), byt(lib.alignq_bnq_any_ws_bytes(P, cin))
    call("alignq_bnq_any_fwd", zc.data_ptr(), P, cin, gamma.data_ptr(), beta.data_ptr(), *(t.data_ptr() for t in run), 0.1, 1e-5, k, r,
         formula, relu, ab.data_ptr(), save.data_ptr(), y.data_ptr(), mask.data_ptr(), ws.data_ptr())
    out = torch.empty(P, cout, **f32)
    call("alignq_k3conv_fwd", y.data_ptr(), bins.data_ptr(), out.data_ptr(), B, H, W, cin, cout, w_bit)
    G = rnd(P, ld)
    G0, dy = G.clone(), G[:, cin:cin + cout].contiguous()
    gy, dw = torch.empty(P, cin, **f32), torch.empty_like(wq)
    call("alignq_k3conv_dgrad", dy.data_ptr(), bins.data_ptr(), gy.data_ptr(), B, H, W, cin, cout, w_bit)
    wws = byt(lib.alignq_k3conv_wgrad_ws_bytes(B, H, W, cin, cout))
    call("alignq_k3conv_wgrad", y.data_ptr(), dy.data_ptr(), dw.data_ptr(), wws.data_ptr(), B, H, W, cin, cout, None)
    dz, dgamma, dbeta = torch.empty(P, cin, **f32), torch.empty(cin, **f32), torch.empty(cin, **f32)
    call("alignq_bnq_any_bwd", gy.data_ptr(), zc.data_ptr(), mask.data_ptr(), ab.data_ptr(), save.data_ptr(), P, cin, r, relu,
         dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr())

    # (1) statistics at a pitch
    (ab2, save2), run2 = new4(), stats()
    ws2 = byt(lib.alignq_dense_train_site_ws_bytes(P, cin))
    call("alignq_dense_train_stats", buf.data_ptr(), ld, P, cin, gamma.data_ptr(), beta.data_ptr(), *(t.data_ptr() for t in run2), 0.1,
         1e-5, ab2.data_ptr(), save2.data_ptr(), ws2.data_ptr())
    assert torch.equal(ab2, ab) and torch.equal(save2, save) and all(torch.equal(a, b) for a, b in zip(run2, run)) and int(run2[2]) == 1
    # (2) the layer in place: its channels written, every other one as it was
    call("alignq_dense_train_layer_fwd", buf.data_ptr(), ld, buf.data_ptr() + 4 * cin, ld, ab2.data_ptr(), bins.data_ptr(), B, H, W, cin,
         cout, w_bit, k, r, formula)
    assert torch.equal(buf[:, cin:cin + cout], out), "forward"
    assert torch.equal(buf[:, :cin], zc) and torch.equal(buf[:, cin + cout:], buf0[:, cin + cout:]), "forward wrote outside its channels"
    # (3) data gradient with dy at a pitch
    gy2 = torch.empty(P, cin, **f32)
    call("alignq_dense_train_dgrad", G.data_ptr() + 4 * cin, ld, bins.data_ptr(), gy2.data_ptr(), B, H, W, cin, cout, w_bit)
    assert torch.equal(gy2, gy), "data gradient"
    # (4) filter gradient with the activation formed again
    dw2 = torch.empty_like(wq)
    call("alignq_dense_train_wgrad", buf.data_ptr(), ld, ab2.data_ptr(), G.data_ptr() + 4 * cin, ld, dw2.data_ptr(), wws.data_ptr(), B, H,
         W, cin, cout, k, r, formula, None)
    assert torch.equal(dw2, dw), "filter gradient"
    # (5) site backward, accumulating into G's first CIN channels
    dgamma2, dbeta2 = torch.empty(cin, **f32), torch.empty(cin, **f32)
    call("alignq_dense_train_site_bwd", gy2.data_ptr(), buf.data_ptr(), ld, ab2.data_ptr(), save2.data_ptr(), G.data_ptr(), ld, P, cin, k,
         r, formula, dgamma2.data_ptr(), dbeta2.data_ptr(), ws2.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(dgamma2, dgamma) and torch.equal(dbeta2, dbeta), "dgamma / dbeta"
    assert torch.equal(G[:, :cin], G0[:, :cin] + dz), "G + dz"
    assert torch.equal(G[:, cin:], G0[:, cin:]), "site backward wrote outside its channels"
    assert float(dz.abs().max()) > 0 and float(dw.abs().max()) > 0 and float((y > 0).float().mean()) > 0.05


def model_state(dev, **kw):
    from alignq_amd import densenet as D
    torch.manual_seed(3)
    # (stem=True in both runs: every convolution of the model then has an order of sums this repository fixes)
    net = D.use_hip_convs(D.DenseNet(4, 4, "second", depth=10, compressionRate=1).to(dev).train(), stem=True, **kw)
    torch.manual_seed(4)
    # (32 x 32: the head's AvgPool2d(8) takes the 8 x 8 map two transitions leave; a 16 x 16 image leaves 4 x 4, which it refuses)
    x = torch.randn(4, 3, 32, 32, device=dev).contiguous(memory_format=torch.channels_last)
    logits = net(x)
    torch.nn.functional.cross_entropy(logits, torch.tensor([1, 7, 0, 3], device=dev)).backward()
    torch.cuda.synchronize()
    return [("logits", logits.detach())] + [(n + ".grad", p.grad) for n, p in net.named_parameters()] + list(net.named_buffers())


def test_the_model_has_the_bits_of_train_sites_and_the_flag_off_calls_nothing_new(dev, monkeypatch):
    from alignq_amd import _lib as L
    calls = _count(monkeypatch, L.load(), tuple(L.DENSETRAIN_SIGNATURES))
    want = model_state(dev, train_sites=True)
    assert not any(calls.values()), calls
    got = model_state(dev, dense_train=True)
    assert calls["alignq_dense_train_layer_fwd"] == 6 and calls["alignq_dense_train_site_bwd"] == 6, calls
    assert [n for n, _ in got] == [n for n, _ in want] and len(got) > 40
    bad = [n for (n, a), (_, b) in zip(got, want) if a is None or b is None or not torch.equal(a, b)]
    assert not bad, bad
    assert all(int(t) == 1 for n, t in got if n.endswith("num_batches_tracked"))


def test_the_block_stays_as_close_to_float64_as_train_sites(dev):
    """Against the float64 CPU twin of tests/test_gpu_train_sites.py (three layers at 24 channels, batch 8, 8 x 8): the largest
    |got - twin| / max |twin| over the loss (the block's output against a random weight) and the nine parameter gradients with
    `fuse_dense_train` stays within twice that of the `fuse_train_sites` path on the same inputs (the existing test's margin for
    quantiser level flips)."""
    from alignq_amd import config, fused, paths
    block = dense_block(dev)
    paths.apply(block, fuse_train_sites=True)
    x0 = torch.randn(8, 24, 8, 8, device=dev).contiguous(memory_format=torch.channels_last)
    w = torch.randn(8, 60, 8, 8, device=dev).contiguous(memory_format=torch.channels_last)
    loss64, grads64, _ = float64_twin(block, x0, w, float(config.args.act_range))

    def deviation(forward):
        block.zero_grad(set_to_none=True)
        loss = (forward(x0.clone(memory_format=torch.channels_last)) * w).sum()
        loss.backward()
        rel = [abs(float(loss.detach()) - loss64) / abs(loss64)]
        return max(rel + [float((p.grad.cpu().double() - g).abs().max() / g.abs().max()) for p, g in zip(block.parameters(), grads64)])

    sites, dense = deviation(block), deviation(lambda x: fused.dense_block_train(block, x))
    print(f"[dense-train] deviation from float64: train_sites {sites:.3e}, dense_train {dense:.3e}")
    assert dense <= 2 * sites
