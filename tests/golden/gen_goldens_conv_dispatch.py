"""Which kernel family every Conv2d_Q convolution gets, as a record: tests/golden/g23_conv_dispatch.json.

Run once on the MI355X at the commit whose choice is to be kept (`python -m tests.golden.gen_goldens_conv_dispatch`); it uses only names
that exist before and after the choice was moved into one function.  tests/test_gpu_conv_dispatch.py imports the cases from here,
recomputes every row and compares it with the file.  The file holds names and shapes, no values.

A single-convolution case is a Conv2d_Q (cdf_alignment_admm.conv2d_Q_fn) or Conv2d_Q3 (densenet.conv2d_Q3_fn), its flags, an input and
the method called.  Its row: the type name of the output's grad_fn, of that node's first input edge (`from`: a materialised packed
handle shows here), which by-product record the output carries, the output's shape, and for forward_with_shortcut the second output's
grad_fn and whether it shares the input's storage; or the type name of the exception the call raised.

A perturbation names its base case; the generator asserts that its row takes another path than the base's (grad_fn, from, record or
exception), or that it is listed in SAME_AS_BASE with the reason.  Whole models: the multiset of autograd node type names reachable
from the roots of one training iteration's backward, and the multiset of autograd-function forwards (and torch convolutions) one
evaluation batch calls inside fused.eval_scope (no graph exists there: EvalStep runs without gradients)."""
import collections
import json
import os

import torch

CL = torch.channels_last
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g23_conv_dispatch.json")
NODES = ("QConv3x3Fn", "QConvGenFn", "QTransitionFn", "QConvStemFn", "QConvStem7Fn", "QConvGemmFn", "QConvDwFn", "QConvPwFn",
         "QConvK3Fn", "Convolution")


def gen_height():
    """the smallest height the transition kernels leave partials for (as tests/test_gpu_conv_records.py finds it)"""
    from alignq_amd import _lib as L
    lib = L.load()
    return next(h for h in range(2, 34, 2) if all(lib.alignq_conv_gen_bn_parts(2, h, 32, 16, 32, ks, 2) > 0 for ks in (3, 1)))


def _case(name, conv, x, base=None, kind="Q", w_bit=4, flags=("use_qconv",), x_grad=True, layout="cl", dtype="float32", w_layout="cl",
          call="forward", packed=None):
    """conv: (C_in, C_out, kernel, stride, padding[, dilation, groups, bias]); x: the input's shape; packed: (index dtype, a_bit, tag)"""
    return dict(name=name, conv=tuple(conv) + (1, 1, False)[len(conv) - 5:], x=tuple(x), base=base, kind=kind, w_bit=w_bit,
                flags=tuple(flags), x_grad=x_grad, layout=layout, dtype=dtype, w_layout=w_layout, call=call, packed=packed)


def _perturbed(base, suffix, **changes):
    """`base` with fields replaced; `conv_` / `x_` prefixed keys replace one position of the conv / x tuples"""
    c = dict(base, name=base["name"] + ":" + suffix, base=base["name"])
    for key, value in changes.items():
        if key[:-1] in ("conv", "x") and key[-1].isdigit():
            t = list(c[key[:-1]])
            t[int(key[-1])] = value
            c[key[:-1]] = tuple(t)
        else:
            c[key] = value
    return c


# perturbations whose row equals the base's, and why
SAME_AS_BASE = {
    "dw:w_bit32": "the depthwise kernels read the fp32 W_q whatever produced it: qconv_dw_supported states no w_bit condition",
    "dw:w_bit9": "as dw:w_bit32",
    "body:emit": "emit_bn_stats changes only the GEMM and 7x7 stem rungs",
    "gemm1:h9": "alignq_qconv_supported takes any height",
    "gemm1:w9": "alignq_qconv_supported takes any width",
    "pw:h9": "alignq_pwconv_supported takes any row count",
    "k3:h9": "alignq_k3conv_supported takes any height",
    "k3:w9": "alignq_k3conv_supported takes any width",
    "dw:h9": "alignq_dwconv3x3_supported takes any height",
    "dw:w9": "alignq_dwconv3x3_supported takes any width",
    "stem7:h9": "alignq_qconv_stem7_fwd takes any height from 8",
    "gemm1:plainw": "a 1x1 filter is plain-contiguous and channels-last at once; the GEMM family asks the layout of 3x3 filters only",
    "pw:plainw": "a 1x1 filter is plain-contiguous and channels-last at once, and the pointwise family takes either",
    "dw:plainw": "a (C, 1, 3, 3) filter is plain-contiguous and channels-last at once",
    "gen1:plainw": "a 1x1 filter is plain-contiguous and channels-last at once, and the transition family takes either for 1x1",
    "gemm1:pw_on": "the GEMM rung stands before the pointwise one: a 64 -> 64 1x1 convolution stays on QConvGemmFn",
    "body64:q3": "a Conv2d_Q3 with use_qconv_k3 off is a Conv2d_Q",
    "pw:w9": "alignq_pwconv_supported takes any row count",
    "dw:stride2": "the depthwise family takes stride 1 and stride 2",
    "body64:emit": "as body:emit",
    "body:packed_int8": "the body family's packed rung reads the indices: the same node on the handle itself (`from` is not a MaterializeFn)",
    "body:packed_int8_tag": "as body:packed_int8; the body family does not read the level tag",
    "body:packed_int16": "as body:packed_int8",
    "body:packed_int16_tag": "as body:packed_int8_tag",
    "gemm1:packed_int16_tag": "the GEMM family's packed rung reads tagged int16 indices: the same node on the handle itself",
}


def single_cases(Hg=None):
    """Hg: the transitions' height (default: asked of the library)"""
    Hg = gen_height() if Hg is None else Hg
    P = _perturbed
    out = []

    def family(base, shared=(), **own):
        """base, then the perturbations every predicate states (minus `shared` exclusions), then the family's own"""
        out.append(base)
        common = dict(bias=dict(conv7=True), groups2=dict(conv6=2), dil2=dict(conv5=2), w_bit9=dict(w_bit=9), w_bit32=dict(w_bit=32),
                      nchw=dict(layout="nchw"), half=dict(dtype="float16"), plainw=dict(w_layout="plain"),
                      h9=dict(x2=base["x"][2] + 1), w9=dict(x3=base["x"][3] + 1), off=dict(flags=()))
        for suffix, ch in common.items():
            if suffix not in shared:
                out.append(P(base, suffix, **ch))
        for suffix, ch in own.items():
            out.append(P(base, suffix, **ch))
        return base

    # ---- the ResNet-20 body: 3x3 / stride 1, C in {16, 32, 64} at width 32 / 16 / 8
    body = family(_case("body", (16, 16, 3, 1, 1), (2, 16, 8, 32)), c8=dict(conv0=8, conv1=8, x1=8), stride2=dict(conv3=2),
                  pad0=dict(conv4=0), emit=dict(flags=("use_qconv", "emit_bn_stats")), nograd=dict(x_grad=False))
    for suffix, ch in dict(tap=dict(), tap_nograd=dict(x_grad=False), tap_off=dict(flags=()), tap_nchw=dict(layout="nchw")).items():
        out.append(P(body, suffix, call="shortcut", **ch))
    # ---- the transitions: stride 2, 3x3 or 1x1, (16, 32) at width 32
    gen3 = family(_case("gen3", (16, 32, 3, 2, 1), (2, 16, Hg, 32)), c48=dict(conv1=48), stride1=dict(conv3=1))
    family(_case("gen1", (16, 32, 1, 2, 0), (2, 16, Hg, 32)), c48=dict(conv1=48), pad1=dict(conv4=1))
    for suffix, ch in dict(tap=dict(), tap_nograd=dict(x_grad=False), tap_off=dict(flags=())).items():
        out.append(P(gen3, suffix, call="shortcut", **ch))
    # ---- the two stems (their image needs no gradient); 3 channels cannot be split into 2 groups
    family(_case("stem", (3, 16, 3, 1, 1), (2, 3, 8, 32), x_grad=False), shared=("groups2",), grad=dict(x_grad=True), c8=dict(conv1=8),
           stride2=dict(conv3=2))
    stem7 = family(_case("stem7", (3, 64, 7, 2, 3), (2, 3, 8, 8), x_grad=False), shared=("groups2", "w9"), grad=dict(x_grad=True),
                   c32=dict(conv1=32), h7=dict(x2=7), w7=dict(x3=7), pad2=dict(conv4=2), stride1=dict(conv3=1),
                   emit=dict(flags=("use_qconv", "emit_bn_stats")))
    out.append(P(stem7, "emit_off", flags=("emit_bn_stats",)))
    # ---- the GEMM family: channel counts multiples of 64, 1x1 or 3x3, stride 1 or 2
    gemm1 = family(_case("gemm1", (64, 64, 1, 1, 0), (2, 64, 8, 8)), c32=dict(conv0=32, x1=32), stride3=dict(conv3=3), pad1=dict(conv4=1),
                   emit=dict(flags=("use_qconv", "emit_bn_stats")), pw_on=dict(flags=("use_qconv", "use_qconv_pw")),
                   tap=dict(call="shortcut"))
    family(_case("gemm3s2", (64, 128, 3, 2, 1), (2, 64, 8, 8)), shared=("h9", "w9"), emit=dict(flags=("use_qconv", "emit_bn_stats")),
           k5=dict(conv2=5, conv4=2))
    # ---- depthwise 3x3
    family(_case("dw", (16, 16, 3, 1, 1, 1, 16), (2, 16, 8, 8)), shared=("groups2",), groups8=dict(conv6=8), c18=dict(conv0=18, conv1=18,
           conv6=18, x1=18), stride3=dict(conv3=3), pad0=dict(conv4=0), stride2=dict(conv3=2))
    # ---- pointwise 1x1 at multiples of 8 (use_qconv_pw)
    family(_case("pw", (8, 24, 1, 1, 0), (2, 8, 8, 8), flags=("use_qconv", "use_qconv_pw")), pw_off=dict(flags=("use_qconv",)),
           pw_only=dict(flags=("use_qconv_pw",)), c12=dict(conv0=12, x1=12), stride2=dict(conv3=2), pad1=dict(conv4=1))
    # ---- 3x3 at multiples of 4 (Conv2d_Q3, use_qconv_k3)
    k3 = family(_case("k3", (24, 12, 3, 1, 1), (2, 24, 8, 8), kind="Q3", flags=("use_qconv", "use_qconv_k3")),
                k3_off=dict(flags=("use_qconv",)), k3_only=dict(flags=("use_qconv_k3",)), c26=dict(conv0=26, x1=26), stride2=dict(conv3=2),
                pad0=dict(conv4=0), q=dict(kind="Q", flags=("use_qconv",)), tap=dict(call="shortcut"))
    out.append(P(k3, "packed", packed=("int8", 4, False)))
    # ---- shapes more than one family takes: the order decides
    b64 = _case("body64", (64, 64, 3, 1, 1), (2, 64, 8, 8))                      # body, GEMM and k3 all take it
    out += [b64, P(b64, "q3", kind="Q3"), P(b64, "q3_k3", kind="Q3", flags=("use_qconv", "use_qconv_k3")),
            P(b64, "emit", flags=("use_qconv", "emit_bn_stats")), P(b64, "tap", call="shortcut")]
    w32 = _case("k3w32", (16, 16, 3, 1, 1), (2, 16, 8, 32), kind="Q3", flags=("use_qconv", "use_qconv_k3"))
    out += [w32, P(w32, "k3_off", flags=("use_qconv",)), P(w32, "q", kind="Q", flags=("use_qconv",)), P(w32, "tap", call="shortcut")]
    g1pw = _case("gemm1_pw", (64, 64, 1, 1, 0), (2, 64, 8, 8), flags=("use_qconv", "use_qconv_pw"))
    out += [g1pw, P(g1pw, "c72", conv1=72)]
    # ---- packed handles: int8 / int16 level indices, with and without the level tag
    for idx, a_bit in (("int8", 4), ("int16", 8)):
        for tag in (False, True):
            sfx = f"{idx}{'_tag' if tag else ''}"
            out.append(P(body, "packed_" + sfx, packed=(idx, a_bit, tag)))
            out.append(P(gemm1, "packed_" + sfx, packed=(idx, a_bit, tag)))
            out.append(P(gemm1, "packed_emit_" + sfx, packed=(idx, a_bit, tag), flags=("use_qconv", "emit_bn_stats")))
    out += [P(body, "packed_off", packed=("int8", 4, False), flags=()), P(body, "packed_tap", packed=("int8", 4, False), call="shortcut"),
            P(gen3, "packed", packed=("int8", 4, False)), P(body, "packed_h9", packed=("int8", 4, False), x2=9)]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return out


def _name(node):
    return None if node is None else type(node).__name__


def _input(case, dev):
    from alignq_amd import fused
    shape = case["x"]
    if case["packed"] is not None:
        idx, a_bit, tag = case["packed"]
        g = torch.Generator().manual_seed(3)
        bins = torch.randint(0, 2 ** a_bit, shape, generator=g).to(getattr(torch, idx)).to(dev).contiguous(memory_format=CL)
        x = fused.packed_handle(shape, dev).requires_grad_(case["x_grad"])
        x._alignq_bins = (bins, a_bit)
        if tag:
            x._alignq_levels = float(2 ** a_bit - 1)
        return x
    x = torch.randn(shape, generator=torch.Generator().manual_seed(4)).to(dev).to(getattr(torch, case["dtype"]))
    if case["layout"] == "cl":
        x = x.contiguous(memory_format=CL)
    return x.requires_grad_(case["x_grad"])


def _module(case, dev, conv=None):
    import alignq_amd.cdf_alignment_admm as A
    from alignq_amd import densenet
    cin, cout, ks, stride, pad, dil, groups, bias = conv or case["conv"]
    make = densenet.conv2d_Q3_fn if case["kind"] == "Q3" else A.conv2d_Q_fn
    m = make(w_bit=case["w_bit"], stage="second")(cin, cout, ks, stride, pad, dil, groups, bias).to(dev)
    if case["w_layout"] == "cl":
        m = m.to(memory_format=CL)
    for flag in case["flags"]:
        setattr(m, flag, True)
    return m


def _parts(y):
    return [a for a in ("_alignq_bn_part", "_alignq_bnq_part") if hasattr(y, a)]


def run_single(case, dev):
    try:
        m, x = _module(case, dev), _input(case, dev)
        out = m.forward_with_shortcut(x) if case["call"] == "shortcut" else m(x)
        y = out[0] if case["call"] == "shortcut" else out
        row = dict(grad_fn=_name(y.grad_fn), parts=_parts(y), shape=list(y.shape),
                   **{"from": _name(y.grad_fn.next_functions[0][0]) if y.grad_fn is not None and y.grad_fn.next_functions else None})
        if case["call"] == "shortcut":
            alias = out[1]
            row.update(tap_fn=_name(alias.grad_fn), tap_shares_storage=alias.untyped_storage().data_ptr() == x.untyped_storage().data_ptr())
        torch.cuda.synchronize()
        return row
    except (RuntimeError, TypeError, ValueError) as e:
        # (the `half` perturbations end here: every predicate refuses the dtype, and torch's convolution then raises on a half input
        # with an fp32 filter.  A dropped dtype check shows as a row that no longer raises - indirectly, but it shows)
        return dict(raises=type(e).__name__)


def transition_cases():
    """What ops.transition_supported states itself: the two flags, equal w_bit, a gradient for x.  Its other conditions are not crossed
    here: the filters' requires_grad (a module's parameter always has it), and the kernel-shape checks, which are qconv_gen_supported's
    and are crossed by the gen3 / gen1 perturbations of single_cases; nchw and h stand for them once."""
    Hg = gen_height()
    base = dict(name="transition", x=(2, 16, Hg, 32), x_grad=True, flags3=("use_qconv",), flags1=("use_qconv",), w_bit1=4, layout="cl", base=None)
    P = _perturbed
    return [base, P(base, "nograd", x_grad=False), P(base, "off3", flags3=()), P(base, "off1", flags1=()), P(base, "w_bit", w_bit1=8),
            P(base, "nchw", layout="nchw"), P(base, "h", x2=Hg + 1)]


def run_transition(case, dev):
    from alignq_amd import resnet
    c = dict(kind="Q", w_bit=4, w_layout="cl", packed=None, dtype="float32", **{k: case[k] for k in ("x", "x_grad", "layout")})
    conv3 = _module(dict(c, flags=case["flags3"]), dev, (16, 32, 3, 2, 1, 1, 1, False))
    conv1 = _module(dict(c, flags=case["flags1"], w_bit=case["w_bit1"]), dev, (16, 32, 1, 2, 0, 1, 1, False))
    pair = resnet._transition_pair(conv3, conv1, _input(c, dev))
    torch.cuda.synchronize()
    if pair is None:
        return dict(grad_fn=None, parts=[], shape=None)
    return dict(grad_fn=[_name(y.grad_fn) for y in pair], parts=[_parts(y) for y in pair], shape=[list(y.shape) for y in pair])


def path_of(row):
    return {k: v for k, v in row.items() if k != "shape"}


# ------------------------------------------------------------------------------------------------ whole models
def graph_names(roots):
    seen, names = set(), collections.Counter()
    stack = [r.grad_fn for r in roots if torch.is_tensor(r) and r.grad_fn is not None]
    while stack:
        n = stack.pop()
        if n in seen:
            continue
        seen.add(n)
        names[type(n).__name__] += 1
        stack += [f for f, _ in n.next_functions if f is not None]
    return dict(sorted(names.items()))


class forward_calls:
    """counts, while active, the forwards of every autograd function of ops and fused and torch's conv2d"""

    def __enter__(self):
        from alignq_amd import fused, ops
        self.counts, self.saved = collections.Counter(), []
        for mod in (ops, fused):
            for name, cls in sorted(vars(mod).items()):
                if isinstance(cls, type) and issubclass(cls, torch.autograd.Function) and cls.__module__ == mod.__name__:
                    if "forward" not in cls.__dict__:
                        continue
                    self.saved.append((cls, "forward", cls.__dict__["forward"]))
                    cls.forward = staticmethod(self._counted(name, cls.forward))
        self.saved.append((torch.nn.functional, "conv2d", torch.nn.functional.conv2d))
        torch.nn.functional.conv2d = self._counted("torch.conv2d", torch.nn.functional.conv2d)
        return self.counts

    def _counted(self, name, fn):
        def call(*a, **k):
            self.counts[name] += 1
            return fn(*a, **k)
        return call

    def __exit__(self, *exc):
        for owner, attr, value in self.saved:
            setattr(owner, attr, value)
        return False


def _train_roots(step, *inputs):
    """one iteration of a captured-step object, eager; the roots its backward starts from"""
    held, real = [], step._backward

    def spy(roots, *a, **k):
        held.append(graph_names(roots))
        return real(roots, *a, **k)
    step._backward = spy
    try:
        step(*inputs)
    finally:
        del step._backward
    torch.cuda.synchronize()
    return held[0]


def _eval_calls(net, x, y):
    from alignq_amd.eval_step import EvalStep
    with EvalStep(net, channels_last=True, qconv=True) as ev, forward_calls() as counts:
        ev(x, y)
    torch.cuda.synchronize()
    return dict(sorted(counts.items()))


def model_records(dev):
    import torch.nn.functional as F
    from alignq_amd import config, densenet, mobilenet
    from alignq_amd.resnet import resnet20_quant
    from alignq_amd.resnet_office import resnet50_dann
    from alignq_amd.train_step import OfficeTrainStep, TrainStep
    a = config.args
    old = (a.bitW, a.abitW, a.train_batch_size, a.eval_batch_size)
    a.bitW = a.abitW = 4
    a.train_batch_size = a.eval_batch_size = 2
    rec = {}
    try:
        g = torch.Generator().manual_seed(7)
        x32 = torch.randn(2, 3, 32, 32, generator=g).to(dev)
        y = torch.randint(0, 10, (2,), generator=g).to(dev)
        for tree in ("admm", "cdf"):
            torch.manual_seed(0)
            net = resnet20_quant(4, 4, tree=tree).to(dev).train()
            rec[f"resnet20_{tree}:train"] = _train_roots(TrainStep(net, channels_last=True, qconv=True), x32, y)
            rec[f"resnet20_{tree}:eval"] = _eval_calls(net, x32, y)
        torch.manual_seed(0)
        net = resnet50_dann(4, 4).to(dev).train()
        xs, xt = (torch.randn(2, 3, 64, 64, generator=g).to(dev) for _ in range(2))
        ys = torch.randint(0, 31, (2,), generator=g).to(dev)
        rec["office_resnet50:train"] = _train_roots(OfficeTrainStep(net, lr=0.004, channels_last=True), xs, ys, xt)
        rec["office_resnet50:eval"] = _eval_calls(net, xs, ys)
        xcl = x32.contiguous(memory_format=CL)
        for name, make in (("mobilenet_v2", lambda: mobilenet.use_hip_convs(mobilenet.mobile_v2(4, 4, "no_align").to(dev))),
                           ("mobilenet_v2_pw", lambda: mobilenet.use_hip_convs(mobilenet.mobile_v2(4, 4, "no_align").to(dev), pointwise=True)),
                           ("densenet40_d16", lambda: densenet.use_hip_convs(
                               densenet.DenseNet(4, 4, "no_align", depth=16, compressionRate=1).to(dev))),
                           ("densenet40_d16_dense_eval", lambda: densenet.use_hip_convs(
                               densenet.DenseNet(4, 4, "no_align", depth=16, compressionRate=1).to(dev), dense_eval=True))):
            torch.manual_seed(0)
            net = make().train()
            rec[name + ":train"] = graph_names([F.cross_entropy(net(xcl), y)])
            rec[name + ":eval"] = _eval_calls(net, xcl, y)
    finally:
        a.bitW, a.abitW, a.train_batch_size, a.eval_batch_size = old
    return rec


def compute(dev):
    return dict(single={c["name"]: run_single(c, dev) for c in single_cases()},
                transition={c["name"]: run_transition(c, dev) for c in transition_cases()},
                models=model_records(dev))


def problems(got):
    """what would let the record pass by testing nothing: a family no case reaches, a base case that raises, a perturbation that takes
    its base's path without a stated reason (or has a reason and does not)"""
    single, out = got["single"], []
    seen = [str(r.get("grad_fn")) for r in list(single.values()) + list(got["transition"].values())]
    out += [f"no case reaches {node}" for node in NODES if not any(node in s for s in seen)]
    for case in single_cases() + transition_cases():
        rows = got["transition"] if case["name"].startswith("transition") else single
        row = rows[case["name"]]
        if case["base"] is None:
            if "raises" in row:
                out.append(f"{case['name']}: a base case raises {row}")
        elif (path_of(row) == path_of(rows[case["base"]])) != (case["name"] in SAME_AS_BASE):
            out.append(f"{case['name']}: {row} against its base's {rows[case['base']]}")
    return out + [f"{name}: nothing counted" for name, counts in got["models"].items() if not counts]


def main(path=PATH):
    assert torch.cuda.is_available(), "the record is made on the MI355X"
    got = json.loads(json.dumps(compute(torch.device("cuda:0"))))
    bad = problems(got)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path + (".rejected" if bad else ""), "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    assert not bad, "\n".join(bad)
    print("wrote", path, len(got["single"]), "single rows,", len(got["transition"]), "transition rows,", len(got["models"]), "model rows")


if __name__ == "__main__":
    import sys
    main(*sys.argv[1:2])
