#!/usr/bin/env python3
"""Golden-vector generator for DSAN (cdf_alignment_admm/dsan_office): imports the reference's own utils/mmd.py,
utils/Weight.py, model/resnet.py and optimizers on CPU (the recipe of gen_goldens.py, whose helpers it uses; `mmd.device` is
overwritten with cpu like `q.device`) and writes

  G15 g15_lmmd.npz              mmd.lmmd: loss, d_source, d_target for the cases below;
  G16 g16_office_tiny_dsan.npz  two DSAN iterations of main.py:386-478 on the tiny ResNet of G10.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_goldens_dsan.py            # both
    python tests/golden/gen_goldens_dsan.py --variant lmmd                      # one (child process)
"""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_goldens as G  # noqa: E402

G.VARIANTS["dsan"] = ("cdf_alignment_admm/dsan_office", "utils.options_office")
C = 31          # utils/Weight.py: class_num is fixed at 31


def _mmd():
    import importlib
    import torch
    q, args = G._enter("dsan", ["--bitW", "4", "--abitW", "4", "--train_batch_size", "6"])
    mmd = importlib.import_module("utils.mmd")
    mmd.device = torch.device("cpu")
    return q, args, mmd


# G15 cases: (name, B, D, source-label recipe, target recipe, kernel_mul, kernel_num, fix_sigma)
LMMD_CASES = [
    ("b32", 32, 256, "random", "random", 2.0, 5, None),
    ("b28", 28, 256, "random", "random", 2.0, 5, None),
    ("d2048", 8, 2048, "random", "random", 2.0, 5, None),
    ("mul_num", 24, 256, "random", "random", 1.5, 3, None),
    ("fix_sigma", 16, 256, "random", "random", 2.0, 7, 300.0),
    ("no_common", 20, 256, "low", "high", 2.0, 5, None),
    ("identical", 12, 256, "random", "random", 2.0, 5, None),
    ("one_class", 16, 256, "single", "random", 2.0, 5, None),
]


def gen_lmmd():
    import torch
    _, _, mmd = _mmd()
    out = {"names": np.array([c[0] for c in LMMD_CASES])}
    g = torch.Generator().manual_seed(1505)
    for ci, (name, B, D, srec, trec, mul, num, fix) in enumerate(LMMD_CASES):
        xs = torch.randn(B, D, generator=g) * 0.8 + 0.1
        xt = torch.randn(B, D, generator=g) * 1.1 - 0.2
        if name == "identical":            # every row the same: bandwidth 0, the kernel matrix is NaN (mmd.py:33-35)
            xs = xt = torch.randn(1, D, generator=g).expand(B, D).contiguous()
            xt = xt.clone()
        ys = {"random": torch.randint(0, C, (B,), generator=g), "low": torch.randint(0, 10, (B,), generator=g),
              "single": torch.full((B,), 7, dtype=torch.long)}[srec]
        logits = torch.randn(B, C, generator=g) * 2.0
        if trec == "high":                 # target argmax only in classes >= 10: no class in common with the source
            logits[:, 10:] += 20.0
        if srec == "single":
            logits[0, 7] += 20.0           # the class is present among the target argmax too
        p = torch.softmax(logits, dim=1)
        s, t = xs.clone().requires_grad_(True), xt.clone().requires_grad_(True)
        loss = mmd.lmmd(s, t, ys, p, kernel_mul=mul, kernel_num=num, fix_sigma=fix)
        if loss.requires_grad:
            loss.backward()
        ds = s.grad if s.grad is not None else torch.zeros_like(s)
        dt = t.grad if t.grad is not None else torch.zeros_like(t)
        if name in ("no_common", "identical"):
            assert float(loss) == 0.0, (name, float(loss))
        else:
            assert float(loss) != 0.0, name
        out.update({f"xs_{ci}": G._np(xs), f"xt_{ci}": G._np(xt), f"ys_{ci}": G._np(ys), f"p_{ci}": G._np(p),
                    f"kernel_mul_{ci}": np.array(mul), f"kernel_num_{ci}": np.array(num),
                    f"fix_sigma_{ci}": np.array(0.0 if fix is None else fix), f"loss_{ci}": G._np(loss),
                    f"ds_{ci}": G._np(ds), f"dt_{ci}": G._np(dt)})
    G._save("g15_lmmd", **out)


def _common_classes(ys, p):
    return len(set(ys.tolist()) & set(p.argmax(1).tolist()))


def gen_office_tiny_dsan():
    """G16: G10's recipe for DSAN - ResNet(Bottleneck, [1,1,1,1], width_per_group=8) with the DSAN head (bottle 2048 -> 256,
    cls_fc 256 -> 31), 4W/4A, batch 6, G10's 64x64 inputs (not stored again), det_init parameters - through TWO iterations of
    main.py:386-478 with the per-epoch SGD re-creation of main.py:316-329 between them.  The forward is the reference's DSAN.forward with the LMMD over
    the BOTTLENECKED target features (cdf_alignment/dsan_office/model/resnet.py:346-358; the ADMM tree's resnet.py:378 passes
    the 2048-wide features and fails), built from the reference's own modules.  The source labels are drawn until both
    iterations have a class in common with the target argmax (otherwise the LMMD term would be 0 and test nothing)."""
    import importlib
    import math
    import torch
    from det_init import det_init_, sample
    q, args, mmd = _mmd()
    r = importlib.import_module("model.resnet")
    r.device = torch.device("cpu")
    r.mmd.device = torch.device("cpu")
    from utils.optimizer import SGD, ADMM_OPT
    B, lr, num_epochs, param = 6, 0.004, 10, float(args.param)
    assert args.bottle_neck and args.train_batch_size == B
    lambds = [2. / (1. + np.exp(-10 * p) + 1e-6) - 1 for p in (0.05, 0.3)]          # main.py:381-382 at two points of the ramp

    def run(label_seed):
        torch.manual_seed(0)
        net = r.DSAN(lambda w, a, s: r.ResNet(w, a, s, r.Bottleneck, [1, 1, 1, 1], width_per_group=8), 4, 4, args.stage)
        net.train()
        det_init_(net)
        g = torch.Generator().manual_seed(31)
        xs = torch.randn(2, B, 3, 64, 64, generator=g)
        xt = torch.randn(2, B, 3, 64, 64, generator=g) * 1.2 + 0.1
        ys = torch.randint(0, C, (2, B), generator=torch.Generator().manual_seed(label_seed))
        # the inputs are G10's (same generator stream); stored once, in g10_office_tiny_dann.npz (size limit per fixture)
        g10 = np.load(os.path.join(HERE, "g10_office_tiny_dann.npz"))
        assert np.array_equal(g10["xs"], G._np(xs)) and np.array_equal(g10["xt"], G._np(xt))
        out = dict(inputs=np.array("g10_office_tiny_dann"), ys=G._np(ys), stage=np.array(str(args.stage)), lr=np.array(lr),
                   num_epochs=np.array(num_epochs), param=np.array(param), lambd=np.array(lambds),
                   names=np.array([n for n, _ in net.named_parameters()]))
        named = list(net.named_parameters())
        param_admm = [(n, p) for n, p in named if "alterD" in n or "gamma" in n]
        opt_a = ADMM_OPT([p for _, p in param_admm])
        ce = torch.nn.CrossEntropyLoss()
        f = net.feature_layers
        blocks = [b for layer in (f.layer1, f.layer2, f.layer3, f.layer4) for b in layer]
        for it, epoch in enumerate((1, 2)):
            rate = lr / math.pow(1 + 10 * (epoch - 1) / num_epochs, 0.75)                 # main.py:316
            opt_t = SGD([{"params": net.feature_layers.parameters()},                      # main.py:318-322 (new every epoch)
                         {"params": net.bottle.parameters(), "lr": rate},
                         {"params": net.cls_fc.parameters(), "lr": rate}],
                        lr=rate / 10, momentum=0.9, weight_decay=5e-4)
            opt_t.zero_grad()
            opt_a.zero_grad()
            # DSAN.forward (resnet.py:368-382) with the bottlenecked target in the LMMD
            src, trans_loss = net.feature_layers(xs[it])
            src = net.bottle(src)
            s_pred = net.cls_fc(src)
            tgt, tgt_trans_loss = net.feature_layers(xt[it])
            tgt = net.bottle(tgt)
            p = torch.nn.functional.softmax(net.cls_fc(tgt), dim=1)
            m = _common_classes(ys[it], p)
            if m < 1:
                return None
            lm = mmd.lmmd(src, tgt, ys[it], p)
            trans_loss = trans_loss + tgt_trans_loss
            loss_mmd = lm + trans_loss / (args.train_batch_size ** 2)
            loss_cls = ce(s_pred, ys[it])
            loss = loss_cls + args.param * lambds[it] * loss_mmd                            # main.py:404-410
            loss.backward()
            idx = [j for j, (n, _) in enumerate(named) if ("conv" in n or "downsample.0" in n) and "weight" in n][1:]
            w_cdf, w_pdf = [], []
            for b in blocks:
                for k, conv in enumerate([b.conv1, b.conv2, b.conv3, b.downsample]):
                    if conv is not None:
                        conv = conv[0] if k == 3 else conv
                        w_cdf.append(conv.quantize_fn.weight_cdf)
                        w_pdf.append(conv.quantize_fn.weight_pdf)
            a_idx = [j for j, (n, _) in enumerate(param_admm) if "alterD" in n]
            g_idx = [j for j, (n, _) in enumerate(param_admm) if "gamma" in n]
            out[f"s_pred_{it}"], out[f"p_{it}"], out[f"m_{it}"] = G._np(s_pred), G._np(p), np.array(m)
            out[f"lmmd_{it}"], out[f"trans_{it}"] = G._np(lm), G._np(trans_loss)
            out[f"loss_mmd_{it}"], out[f"loss_{it}"] = G._np(loss_mmd), G._np(loss)
            for bi, b in enumerate(blocks):
                out[f"D_{it}_{bi}"] = G._np(b.admm0.D)                                      # the TARGET pass's D
            for j, (n, p_) in enumerate(named):
                if p_.grad is not None:                 # feature_layers.fc is never used
                    out[f"grad_{it}/{j}"] = G._np(sample(p_.grad))
            opt_t.step(idx, w_cdf, w_pdf, float(args.lam), float(args.lam2))
            opt_a.step(a_idx, g_idx, [b.admm0.D for b in blocks], [b.admm0.alterD for b in blocks],
                       [b.admm0.gamma for b in blocks], [b.admm0.mu for b in blocks], [b.admm0.rho for b in blocks])
            for j, (n, p_) in enumerate(named):
                out[f"after_{it}/{j}"] = G._np(sample(p_))
                st = opt_t.state.get(p_, {})
                if "momentum_buffer" in st:
                    out[f"buf_{it}/{j}"] = G._np(sample(st["momentum_buffer"]))
            out[f"rate_{it}"] = np.array(rate)
        return out

    for seed in range(100, 200):
        out = run(seed)
        if out is not None:
            break
    assert out is not None and int(out["m_0"]) >= 1 and int(out["m_1"]) >= 1, "no label draw with a common class"
    out["label_seed"] = np.array(seed)
    # the full-size model's parameter names (drop-in check); resnet50_quant without its pretrained=True download
    r50 = r.DSAN(lambda w, a, s: r.resnet50_quant(w, a, s, pretrained=False), 4, 4, args.stage)
    out["names_r50"] = np.array([n for n, _ in r50.named_parameters()])
    G._save("g16_office_tiny_dsan", **out)


GEN = {"lmmd": gen_lmmd, "office_tiny_dsan": gen_office_tiny_dsan}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=sorted(GEN), default=None)
    a = ap.parse_args()
    if a.variant is None:
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        for v in GEN:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", v], check=True, env=env)
        return
    GEN[a.variant]()


if __name__ == "__main__":
    main()
