"""`fuse_train_sites` on a three-layer dense block at 24 channels (batch 8, 8 x 8): with the flag on, every bn -> act_q0 -> ReLU site is one
fused.BNQuantAnyFn node - bit-equal to the same chain written out by hand, one alignq_bnq_any_fwd / _bwd call per site and no batch-norm
call; with the flag off, the launches are the composition's and no alignq_bnq_any_* entry is called."""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_dwconv import _count, dev  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu
ANY = ("alignq_bnq_any_fwd", "alignq_bnq_any_bwd")


def dense_block(dev):
    from alignq_amd import densenet as D
    torch.manual_seed(11)
    layers = [D.DenseBasicBlock("second", 4, 4, inplanes=c, filters=c, index=None) for c in (24, 36, 48)]
    for m in layers:                                   # batch-norms away from (1, 0), so that dgamma and dbeta differ per channel
        m.bn1.weight.data.uniform_(0.5, 1.5)
        m.bn1.bias.data.normal_(0, 0.2)
    return D.use_hip_convs(torch.nn.Sequential(*layers).to(dev).train())


def by_hand(block, x):
    """the flag-on forward written out: BNQuantAnyFn with the ReLU clamp, the layer's convolution, the concatenation"""
    from alignq_amd import config, fused
    for m in block:
        bn, act = m.bn1, m.act_q0
        y = fused.BNQuantAnyFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps,
                                     act.a_bit, config.args.act_range, act._formula, fused.CLAMP_RELU)
        x = torch.cat((x, m.conv1(y)), 1)
    return x


def run(block, forward, x0, w):
    x = x0.clone(memory_format=torch.channels_last).requires_grad_(True)
    block.zero_grad(set_to_none=True)
    out = forward(x)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    state = [out.detach(), x.grad] + [p.grad for p in block.parameters()]
    state += [b for m in block for b in (m.bn1.running_mean, m.bn1.running_var, m.bn1.num_batches_tracked)]
    return [t.clone() for t in state]


def test_flag_on_is_the_hand_written_chain_and_flag_off_is_the_composition(dev, monkeypatch):
    from alignq_amd import _lib as L
    from alignq_amd import paths
    block = dense_block(dev)
    twin = copy.deepcopy(block)
    x0 = torch.randn(8, 24, 8, 8, device=dev).contiguous(memory_format=torch.channels_last)
    w = torch.randn(8, 60, 8, 8, device=dev).contiguous(memory_format=torch.channels_last)
    lib = L.load()
    others = [n for table in ("SIGNATURES", "POINTWISE_SIGNATURES", "K3CONV_SIGNATURES") for n in getattr(L, table)
              if n.endswith(("_fwd", "_bwd", "_dgrad", "_wgrad", "_multi"))]
    calls = _count(monkeypatch, lib, ANY + tuple(others))
    bn_calls = []
    real_bn = F.batch_norm
    monkeypatch.setattr(F, "batch_norm", lambda *a, **kw: bn_calls.append(1) or real_bn(*a, **kw))

    def counted(model, forward):
        for k in calls:
            calls[k] = 0
        del bn_calls[:]
        state = run(model, forward, x0, w)
        return state, {k: v for k, v in calls.items() if v}, len(bn_calls)

    # flag off (the class default): the composition, as before
    plain = copy.deepcopy(block)
    _, off_calls, off_bn = counted(plain, plain)
    assert off_bn == 3 and not any(n in off_calls for n in ANY), off_calls
    # flag on: one any-width node per site each way, no batch-norm call, every other launch as with the flag off
    rec = paths.apply(block, fuse_train_sites=True)
    assert len(rec) == 3
    on, on_calls, on_bn = counted(block, block)
    assert on_bn == 0 and on_calls["alignq_bnq_any_fwd"] == 3 and on_calls["alignq_bnq_any_bwd"] == 3, on_calls
    site = lambda c: {k: v for k, v in c.items() if "act_quant" not in k and k not in ANY}      # noqa: E731
    assert site(on_calls) == site(off_calls), (on_calls, off_calls)
    hand, hand_calls, _ = counted(twin, lambda x: by_hand(twin, x))
    assert hand_calls == on_calls
    for i, (a, b) in enumerate(zip(on, hand)):
        assert torch.equal(a, b) and a.stride() == b.stride(), f"tensor {i} of the flag-on run differs from the hand-written chain"
    assert all(int(m.bn1.num_batches_tracked) == 1 for m in block)


def float64_twin(block, x0, w, act_range):
    """the same block in torch double on the CPU (oracle/torch_ref.py's quantisers, CDF tree): loss, parameter gradients in
    block.parameters() order, and every site's output"""
    from oracle import torch_ref as R
    cfg = R.Config(tree="cdf", act_range=act_range)
    x = x0.detach().cpu().double()
    params, sites = [], []
    for m in block:
        gam, bet, wt = (p.detach().cpu().double().requires_grad_(True) for p in (m.bn1.weight, m.bn1.bias, m.conv1.weight))
        params += [gam, bet, wt]                       # (the module's own order: bn1 before conv1)
        y = torch.relu(R.act_quant(F.batch_norm(x, None, None, gam, bet, True, 0.1, m.bn1.eps), m.act_q0.a_bit, "second", cfg)[0])
        sites.append(y.detach())
        x = torch.cat((x, F.conv2d(y, R.weight_quant(wt, 4, cfg)[0], None, 1, 1)), 1)
    loss = (x * w.detach().cpu().double()).sum()
    loss.backward()
    return float(loss.detach()), [p.grad for p in params], sites


def deviation(block, x0, w, twin):
    """(the largest |got - twin| / max |twin| over the loss and the parameter gradients, the largest site-output difference)"""
    loss64, grads64, sites64 = twin
    seen = []
    hooks = [m.conv1.register_forward_pre_hook(lambda mod, inp: seen.append(inp[0].detach().cpu().double())) for m in block]
    x = x0.clone(memory_format=torch.channels_last)
    block.zero_grad(set_to_none=True)
    loss = (block(x) * w).sum()
    loss.backward()
    loss = loss.detach()
    for h in hooks:
        h.remove()
    assert [n for n, _ in block.named_parameters()] == [f"{i}.{n}" for i in range(3) for n in ("bn1.weight", "bn1.bias", "conv1.weight")]
    rel = [abs(float(loss) - loss64) / abs(loss64)]
    rel += [float((p.grad.cpu().double() - g).abs().max() / g.abs().max()) for p, g in zip(block.parameters(), grads64)]
    return max(rel), max(float((a - b).abs().max()) for a, b in zip(seen, sites64))


def test_flag_on_stays_as_close_to_float64_as_the_composition(dev):
    """Against a CPU float64 twin of the block: the deviation (largest |got - twin| / max |twin| over the loss and the nine parameter
    gradients) with the flag on stays within twice the flag-off model's own (a folded site rounds its statistics differently from
    MIOpen's batch-norm, so each run puts a handful of elements on the neighbouring level, and two runs' flips can add), and no site
    output differs from the twin's by more than one quantiser level, 2 r / 15, in either run.
    Measured on an MI355X at this seed: deviation 5.943e-06 with the flag off and 5.943e-06 with it on; no site output off its level in
    either run (largest difference 0.0000 levels)."""
    from alignq_amd import config, paths
    block = dense_block(dev)
    x0 = torch.randn(8, 24, 8, 8, device=dev).contiguous(memory_format=torch.channels_last)
    w = torch.randn(8, 60, 8, 8, device=dev).contiguous(memory_format=torch.channels_last)
    twin = float64_twin(block, x0, w, float(config.args.act_range))
    level = 2.0 * float(config.args.act_range) / 15.0
    off, off_site = deviation(copy.deepcopy(block), x0, w, twin)
    paths.apply(block, fuse_train_sites=True)
    on, on_site = deviation(block, x0, w, twin)
    print(f"[train-sites] deviation from float64: flag off {off:.3e}, flag on {on:.3e}; site outputs: off {off_site / level:.4f}, "
          f"on {on_site / level:.4f} levels")
    assert off_site <= level * (1 + 1e-6) and on_site <= level * (1 + 1e-6)
    assert on <= 2 * off
