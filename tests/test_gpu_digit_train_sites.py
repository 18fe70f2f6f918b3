"""`fuse_train_sites` on the digit DANN (alignq_amd/digit.py) at 4W/4A, 6 source + 6 target images, training mode, one seed per run: with
the flag on each half of `feature` is conv -> fused.BNQuantPoolFn [-> Dropout2d on the pooled tensor]; with it off, `forward` is
`feature` module by module."""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests.golden.digit_init import digit_init_
from tests.test_gpu_digit import bits4, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ALPHA, SEED = 0.3, 17
ZERO_GRAD = ("feature.0.bias", "feature.5.bias", "classifier.0.bias", "classifier.3.bias", "discriminator.0.bias")


def setup(dev):
    from alignq_amd import digit
    net = digit.use_hip_convs(digit_init_(digit.MNISTmodel_quant("second", 4, 4)).to(dev).train())
    g = torch.Generator().manual_seed(6)
    src, tgt = torch.randn(6, 1, 28, 28, generator=g).to(dev), torch.randn(6, 3, 28, 28, generator=g).to(dev)
    return net, src, tgt, torch.randint(0, 10, (6,), generator=g).to(dev)


def heads(net, feat):
    from alignq_amd.resnet_office import ReverseLayerF
    return net.classifier(feat), net.discriminator(ReverseLayerF.apply(feat, ALPHA))


def by_hand(net, x):
    """the flag-on forward written out on the un-pooled fold: k5conv -> BNQuantAnyFn(CLAMP_RELU) -> F.max_pool2d [-> Dropout2d]"""
    from alignq_amd import config, fused
    x = x.expand(x.shape[0], 3, 28, 28).contiguous(memory_format=torch.channels_last)
    f = net.feature
    for i in (0, 5):
        bn, act = f[i + 1], f[i + 2]
        y = fused.BNQuantAnyFn.apply(f[i](x), bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum,
                                     bn.eps, act.a_bit, config.args.act_range, act._formula, fused.CLAMP_RELU)
        x = F.max_pool2d(y, 2)
        x = f[8](x) if i == 5 else x
    return heads(net, x.reshape(-1, 768))


def run(net, forward, src, tgt, labels):
    """one forward + backward of digit.train_iteration's loss: (logits and buffers, parameter gradients, the Dropout2d masks)"""
    masks = []
    hook = net.feature[8].register_forward_hook(lambda m, i, o: masks.append((o.detach().abs().amax((2, 3)) > 0).double().cpu() * 2))
    torch.manual_seed(SEED)
    net.zero_grad(set_to_none=True)
    (sc, sd), (_, td) = forward(src), forward(tgt)
    dom = lambda n: torch.full((6,), n, dtype=torch.long, device=src.device)      # noqa: E731
    (F.cross_entropy(sc, labels) + F.cross_entropy(sd, dom(0)) + F.cross_entropy(td, dom(1))).backward()
    torch.cuda.synchronize()
    hook.remove()
    return [t.detach().clone() for t in [sc, sd, td] + list(net.buffers())], [p.grad.clone() for p in net.parameters()], masks


def float64_twin(net, src, tgt, labels, masks):
    """the same loss in torch double on the CPU (oracle/torch_ref.py's quantisers, CDF tree), the Dropout2d masks given: the
    parameter gradients in net.parameters() order"""
    from alignq_amd.resnet_office import ReverseLayerF
    from oracle import torch_ref as R
    cfg = R.Config(tree="cdf", act_range=2.0)
    P = {n: p.detach().cpu().double().requires_grad_(True) for n, p in net.named_parameters()}

    def seq(name, x):
        for j, m in enumerate(getattr(net, name)):
            w, b = P.get(f"{name}.{j}.weight"), P.get(f"{name}.{j}.bias")
            x = F.linear(x, w, b) if isinstance(m, torch.nn.Linear) else torch.relu(x) if w is None else \
                F.batch_norm(x, None, None, w, b, True, 0.1, m.eps)
        return x

    def forward(x, mask):
        x = x.cpu().double().expand(6, 3, 28, 28)
        for i in (0, 5):
            z = F.conv2d(x, R.weight_quant(P[f"feature.{i}.weight"], 4, cfg)[0], P[f"feature.{i}.bias"])
            z = F.batch_norm(z, None, None, P[f"feature.{i + 1}.weight"], P[f"feature.{i + 1}.bias"], True, 0.1, net.feature[i + 1].eps)
            v = R.act_quant(z, 4, "second", cfg)[0]
            x = F.max_pool2d(torch.relu(v * mask[:, :, None, None] if i == 5 else v), 2)
        feat = x.reshape(-1, 768)
        return seq("classifier", feat), seq("discriminator", ReverseLayerF.apply(feat, ALPHA))
    (sc, sd), (_, td) = forward(src, masks[0]), forward(tgt, masks[1])
    dom = lambda n: torch.full((6,), n, dtype=torch.long)      # noqa: E731
    (F.cross_entropy(sc, labels.cpu()) + F.cross_entropy(sd, dom(0)) + F.cross_entropy(td, dom(1))).backward()
    return [P[n].grad for n, _ in net.named_parameters()]


def deviation(net, grads, grads64):
    """largest |got - twin| / max |twin| over the parameter gradients.  The five biases that a training batch-norm follows directly are
    left out: a constant added in front of it has the exact gradient 0 (the twin's is 1e-17), so there is no scale to measure against."""
    return max(float((g.cpu().double() - w).abs().max() / w.abs().max())
               for (n, _), g, w in zip(net.named_parameters(), grads, grads64) if n not in ZERO_GRAD)


def test_flag_on_is_the_hand_written_chain_and_as_close_to_float64_as_the_composition(dev, bits4):
    """Flag on against the same chain on the un-pooled fold (BNQuantAnyFn -> F.max_pool2d -> Dropout2d) on a deep copy: the three logits
    and every buffer torch.equal; the parameter gradients differ only through the order of the backward sums, so their deviation from a
    CPU float64 twin (largest |got - twin| / max |twin| over the parameter gradients) may be at most twice the flag-off model's own -
    the criterion and the reason of tests/test_gpu_train_sites.py.
    Measured on an MI355X at this seed: deviation 2.074e-06 with the flag off, 2.074e-06 with it on, 2.074e-06 for the hand-written chain."""
    from alignq_amd import paths
    net, src, tgt, labels = setup(dev)
    off_net, hand_net = copy.deepcopy(net), copy.deepcopy(net)
    assert len(paths.apply(net, fuse_train_sites=True)) == 1
    off_out, off_grads, masks = run(off_net, lambda x: off_net(x, ALPHA), src, tgt, labels)
    on_out, on_grads, on_masks = run(net, lambda x: net(x, ALPHA), src, tgt, labels)
    hand_out, hand_grads, _ = run(hand_net, lambda x: by_hand(hand_net, x), src, tgt, labels)
    for i, (a, b) in enumerate(zip(on_out, hand_out)):
        assert torch.equal(a, b), f"tensor {i} (logits, then buffers) of the flag-on run differs from the hand-written chain"
    assert all(int(net.feature[i].num_batches_tracked) == 2 for i in (1, 6))
    # Dropout2d behind the pool drew the channels it draws in front of it (where a pooled channel is all zero the mask cannot be read)
    assert all(bool(((a == b) | (a == 0)).all()) for a, b in zip(on_masks, masks))
    grads64 = float64_twin(off_net, src, tgt, labels, masks)
    off, on, hand = (deviation(net, g, grads64) for g in (off_grads, on_grads, hand_grads))
    print(f"[digit-train-sites] deviation of the parameter gradients from float64: flag off {off:.3e}, flag on {on:.3e}, "
          f"hand-written chain {hand:.3e}")
    assert on <= 2 * off


def test_flag_off_is_feature_module_by_module(dev, bits4):
    net, src, tgt, labels = setup(dev)
    assert getattr(net, "fuse_train_sites", False) is False

    def modules(x):
        x = x.expand(x.shape[0], 3, 28, 28).contiguous(memory_format=torch.channels_last)
        for m in net.feature:
            x = m(x)
        return heads(net, x.reshape(-1, 768))
    out, grads, _ = run(net, lambda x: net(x, ALPHA), src, tgt, labels)
    want, wgrads, _ = run(net, modules, src, tgt, labels)       # (training-mode outputs do not depend on the running statistics)
    assert all(torch.equal(a, b) for a, b in zip(out[:3], want[:3])) and all(torch.equal(a, b) for a, b in zip(grads, wgrads))
