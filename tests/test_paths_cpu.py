"""alignq_amd.paths: the kernel-path flags are declared by the module classes that read them, assigned by `apply` on exactly those
classes and put back exactly by `restore`; the three training steps leave the flags their arguments ask for, also on a model that an
earlier step has used; dp.attach(global_corr=True) / dp.detach leave them as they were.  No GPU: only constructors run."""
import itertools

import pytest
import torch

from alignq_amd import paths

# class -> the flags it declares ("Kernel-path flags"); a class that is not listed declares none
CONV = {"use_qconv", "use_qconv_pw", "emit_bn_stats"}
DECLARED = {
    "cifar": {"Conv2d_Q": CONV, "PreActBlock_conv_Q": {"fuse_bn", "pack_bins"}, "PreActResNet": {"fuse_bn"}},
    "office": {"Conv2d_Q": CONV, "Bottleneck": {"fuse_bn", "fuse_relu", "pack_bins"}, "ResNet": {"fuse_bn", "fuse_relu", "_wq_stage"}},
    "mobile": {"Conv2d_Q": CONV},
}
MODELS = [("cifar_admm", "cifar"), ("cifar_cdf", "cifar"), ("dann", "office"), ("dsan", "office"), ("mobile", "mobile")]


def cifar(tree="admm"):
    from alignq_amd.resnet import PreActBlock_conv_Q, PreActResNet
    return PreActResNet(PreActBlock_conv_Q, [1, 1, 1], 8, 8, "second", 10, tree=tree)


def office(cls):
    from alignq_amd.resnet_office import Bottleneck, ResNet
    return cls(lambda w, a, s: ResNet(w, a, s, Bottleneck, [1, 1, 1, 1], width_per_group=8), 4, 4, "aligned")


def build(name):
    from alignq_amd import mobilenet, resnet_office
    torch.manual_seed(0)
    if name.startswith("cifar"):
        return cifar(name[len("cifar_"):])
    if name == "mobile":
        return mobilenet.mobile_v2(4, 4, "second")
    return office(resnet_office.DANN if name == "dann" else resnet_office.DSAN)


def own(model):
    """Every module's instance __dict__: its keys and the identity of each value."""
    return {n: {k: id(v) for k, v in m.__dict__.items()} for n, m in model.named_modules()}


def effective(model):
    """{class name: the set of (flag, value) over its modules}, every flag read as a plain attribute; classes without flags left out."""
    out = {}
    for m in model.modules():
        for f in paths.FLAGS + ("_features_only",):
            if hasattr(type(m), f):
                out.setdefault(type(m).__name__, set()).add((f, getattr(m, f)))
    return out


def expect(**per_class):
    return {cls: set(flags.items()) for cls, flags in per_class.items()}


# ------------------------------------------------------------------------------------------------------------ 1. apply
@pytest.mark.parametrize("name,kind", MODELS, ids=[m[0] for m in MODELS])
def test_apply_assigns_on_exactly_the_declaring_classes(name, kind):
    model, declared = build(name), DECLARED[kind]
    assert set(declared) <= {type(m).__name__ for m in model.modules()}          # every listed class is in the model
    for m in model.modules():                                                    # the declarations are the table, with their off values
        for f in paths.FLAGS:
            if f in declared.get(type(m).__name__, ()):
                assert getattr(m, f) is (None if f == "_wq_stage" else False) and f not in m.__dict__
            else:
                assert not hasattr(m, f)
    for f in paths.FLAGS:
        value = object()
        rec = paths.apply(model, **{f: value})
        for m in model.modules():
            if f in declared.get(type(m).__name__, ()):
                assert m.__dict__[f] is value
            else:
                assert not hasattr(m, f)
        assert len(rec) == sum(f in declared.get(type(m).__name__, ()) for m in model.modules())
        paths.restore(rec)


@pytest.mark.parametrize("name,kind", MODELS, ids=[m[0] for m in MODELS])
def test_an_unknown_name_is_a_type_error_and_changes_nothing(name, kind):
    model = build(name)
    before = own(model)
    for bad in ({"fuse_bnn": True}, {"use_qconv": True, "_features_only": True}, {"global_corr": True, "fuse_bn": True}):
        with pytest.raises(TypeError, match="no such flag"):
            paths.apply(model, **bad)
        assert own(model) == before


# ---------------------------------------------------------------------------------------------------------- 2. restore
@pytest.mark.parametrize("name,kind", MODELS, ids=[m[0] for m in MODELS])
def test_restore_puts_every_instance_dict_back(name, kind):
    model = build(name)
    every = dict(use_qconv=True, use_qconv_pw=True, emit_bn_stats=True, fuse_bn=True, fuse_relu=True, pack_bins=True,
                 _wq_stage=lambda i: None)
    # nothing set: a flag that was only the class default is absent again
    before = own(model)
    rec = paths.apply(model, **every)
    assert own(model) != before
    paths.restore(rec)
    assert own(model) == before and not any(f in m.__dict__ for m in model.modules() for f in paths.FLAGS)
    # some flags set by hand beforehand, on some of the modules
    declaring = [m for m in model.modules() if any(hasattr(type(m), f) for f in paths.FLAGS)]
    for i, m in enumerate(declaring):
        flags = [f for f in paths.FLAGS if hasattr(type(m), f)]
        if i % 2 == 0:
            setattr(m, flags[0], True)
        if i % 3 == 0:
            setattr(m, flags[-1], False)         # (an explicit off is kept as an explicit off)
    by_hand = own(model)
    assert by_hand != before
    rec = paths.apply(model, **every)
    paths.restore(rec)
    assert own(model) == by_hand
    # two nested applies, restored in reverse order
    outer = paths.apply(model, use_qconv=True, fuse_bn=True, pack_bins=False)
    mid = own(model)
    inner = paths.apply(model, use_qconv=False, fuse_bn=False, fuse_relu=True, _wq_stage=None)
    paths.restore(inner)
    assert own(model) == mid
    paths.restore(outer)
    assert own(model) == by_hand


# --------------------------------------------------------------------------------------------------- 3. the constructors
@pytest.mark.parametrize("tree", ["admm", "cdf"])
@pytest.mark.parametrize("channels_last,qconv,fuse_bn,pack_bins", list(itertools.product([False, True], repeat=4)))
def test_train_step_leaves_the_flags_its_arguments_ask_for(tree, channels_last, qconv, fuse_bn, pack_bins):
    from alignq_amd.train_step import TrainStep
    net = cifar(tree)
    step = TrainStep(net, channels_last=channels_last, qconv=qconv, fuse_bn=fuse_bn, pack_bins=pack_bins)
    q = channels_last and qconv
    assert step.qconv is q
    assert effective(net) == expect(
        Conv2d_Q=dict(use_qconv=q, use_qconv_pw=False, emit_bn_stats=False),
        PreActBlock_conv_Q=dict(fuse_bn=fuse_bn, pack_bins=q and fuse_bn and pack_bins),
        PreActResNet=dict(fuse_bn=fuse_bn, _features_only=False))


@pytest.mark.parametrize("kw", [{}, {"channels_last": True}, {"fuse_relu": False}], ids=["defaults", "channels_last", "no_fuse_relu"])
@pytest.mark.parametrize("tree", ["dann", "dsan"])
def test_office_steps_leave_the_flags_their_arguments_ask_for(tree, kw):
    from alignq_amd import resnet_office
    from alignq_amd.train_step import DSANTrainStep, OfficeTrainStep
    torch.manual_seed(0)
    net = office(resnet_office.DANN if tree == "dann" else resnet_office.DSAN)
    step = (OfficeTrainStep if tree == "dann" else DSANTrainStep)(net, lr=0.004, **kw)
    channels_last, fuse_relu = kw.get("channels_last", False), kw.get("fuse_relu", True)      # fuse_bn, qconv, pack_bins: on
    q = channels_last and torch.cuda.is_available()
    fold = fuse_relu and channels_last
    assert step.qconv is q and step.dual is fold
    assert effective(net) == expect(
        Conv2d_Q=dict(use_qconv=q, use_qconv_pw=False, emit_bn_stats=q and fuse_relu),
        Bottleneck=dict(fuse_bn=fold, fuse_relu=fuse_relu, pack_bins=q and fuse_relu),
        ResNet=dict(fuse_bn=fold, fuse_relu=fuse_relu, _wq_stage=None))


# ------------------------------------------------------------------------------------------------ 4. a model used twice
def test_a_second_train_step_on_the_same_model_lowers_what_the_first_raised():
    from alignq_amd.train_step import TrainStep
    net = cifar()
    TrainStep(net, channels_last=True, qconv=True)
    names = ("use_qconv", "fuse_bn", "pack_bins")
    assert {f for m in net.modules() for f in names if getattr(m, f, False)} == set(names)        # the first step raised all three
    TrainStep(net, channels_last=False, qconv=False, fuse_bn=False, pack_bins=False)
    left = sorted((n, f) for n, m in net.named_modules() for f in names if getattr(m, f, False))
    assert left == [], f"{len(left)} flags of the first step are still on, e.g. {left[:3]}"


# ---------------------------------------------------------------------------------------------- 5. dp.attach / dp.detach
def test_attach_global_corr_then_detach_leaves_the_flags_as_before(tmp_path):
    import torch.distributed as dist
    from alignq_amd import dp
    from alignq_amd.train_step import TrainStep
    net = cifar()
    step = TrainStep(net, lr=0.01)
    net.layers[0].fuse_bn = False                                   # one module differs by hand: it must come back as it was
    before, flags = own(net), effective(net)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/store", rank=0, world_size=1)
    try:
        dp.attach(step, global_corr=True)
        assert not any(m.fuse_bn for m in net.modules() if hasattr(type(m), "fuse_bn"))
        dp.detach(step)
    finally:
        dist.destroy_process_group()
    assert effective(net) == flags
    sites = {n for n, m in net.named_modules() if hasattr(m, "a_bit") and hasattr(m, "opt")}
    after = own(net)
    for n in sites:                                                 # (detach leaves the sites' global_corr = None behind: not a flag)
        assert after[n].pop("global_corr") == id(None)
    assert after == before
