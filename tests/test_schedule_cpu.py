"""alignq_amd/schedule.py on the CPU: the table builders against torch's MultiStepLR and against literal restatements of the
reference's lines (cdf_alignment_admm/resnet-20-cifar-10/main.py:97,126; dann_office/main.py:321-328,345-348; dsan_office/
main.py:316-329,345-347,381-382,410), pinned to the rates and ramp values fixtures G10 and G16 recorded from the reference; the
HyperBlock's staging on a host "device"; the three exports and their argument checks, which need no device."""
import math
import warnings

import numpy as np
import pytest
import torch

from tests.conftest import load_golden


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def f32(x):
    return np.float32(x)


@pytest.mark.parametrize("lr,milestones,gamma,epochs", [(0.04, [80, 150], 0.1, 200),      # utils/options.py:62,70-76 (ResNet-20)
                                                        (0.04, [80, 120], 0.1, 200),      # the ResNet-56 tree's
                                                        (0.037, [3, 7, 8, 19], 0.3, 23)])
def test_multistep_rows_are_float32_of_torch_multisteplr(lr, milestones, gamma, epochs):
    """the scheduler driven as main.py:125-127 drives it (`step(epoch)` in front of every epoch) and in torch's chained form"""
    from alignq_amd.schedule import multistep
    iters = 3
    t = multistep(lr, milestones, gamma, epochs, iters).numpy()
    assert t.shape == (epochs * iters, 4) and t.dtype == np.float32
    for chained in (False, True):
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
        sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones, gamma=gamma)
        for epoch in range(epochs):
            if not chained:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    sch.step(epoch)
            want = f32(opt.param_groups[0]["lr"])
            for i in range(iters):
                assert bits(t[epoch * iters + i, 0]) == bits(want), (chained, epoch, i)
            if chained:
                opt.step()
                sch.step()
    assert not t[:, 1:3].any()
    assert t[0, 3] == 1.0 and not t[1:, 3].any()           # the run starts with a new optimizer, nothing else does


def test_office_dann_rows_restate_the_reference():
    from alignq_amd.schedule import office_dann
    from alignq_amd.train_step import dann_alpha
    g = load_golden("g10_office_tiny_dann")
    lr, num_epochs, num_iterations = float(g["lr"]), int(g["num_epochs"]), 7
    t = office_dann(lr, num_epochs, num_iterations, start_epoch=1).numpy()
    assert t.shape == ((num_epochs - 1) * num_iterations, 6)
    r = 0
    for epoch in range(1, num_epochs):
        LEARNING_RATE = lr / math.pow((1 + 10 * (epoch - 1) / num_epochs), 0.75)                       # main.py:321
        for i in range(1, num_iterations + 1):                                                       # :341-343
            num_iters = num_iterations * epoch + i                                                   # :345
            p = float(num_iters) / num_epochs / num_iterations                                       # :347
            alpha = 2. / (1. + np.exp(-10 * p) + 1e-6) - 1                                           # :348
            want = [LEARNING_RATE / 10, LEARNING_RATE, LEARNING_RATE, alpha, 0.0, 1.0 if i == 1 else 0.0]
            assert np.array_equal(bits(t[r]), bits(want)), (epoch, i)
            assert dann_alpha(num_iters, num_epochs, num_iterations) == alpha
            r += 1
    fresh = t[:, 5]
    assert np.array_equal(np.nonzero(fresh)[0], np.arange(num_epochs - 1) * num_iterations) and set(fresh) == {0.0, 1.0}
    # the reference's own rates (fixture G10 ran epochs 1 and 2)
    for it in (0, 1):
        row = t[it * num_iterations]
        assert bits(row[1]) == bits(f32(g[f"rate_{it}"])) and bits(row[2]) == bits(row[1])
        assert bits(row[0]) == bits(f32(float(g[f"rate_{it}"]) / 10))


@pytest.mark.parametrize("bottle_neck", [True, False])
def test_office_dsan_rows_restate_the_reference(bottle_neck):
    from alignq_amd.schedule import office_dsan
    g = load_golden("g16_office_tiny_dsan")
    lr, num_epochs, num_iterations, param = float(g["lr"]), int(g["num_epochs"]), 10, float(g["param"])
    t = office_dsan(lr, num_epochs, num_iterations, param=param, start_epoch=1, bottle_neck=bottle_neck).numpy()
    G = 3 if bottle_neck else 2
    assert t.shape == ((num_epochs - 1) * num_iterations, G + 3)
    r = 0
    for epoch in range(1, num_epochs):
        LEARNING_RATE = lr / math.pow((1 + 10 * (epoch - 1) / num_epochs), 0.75)                       # main.py:316
        for i in range(num_iterations):                                                              # :345
            num_iters = num_iterations * epoch + i                                                   # :347
            p = float(num_iters) / num_epochs / num_iterations                                       # :381
            lambd = 2. / (1. + np.exp(-10 * p) + 1e-6) - 1                                           # :382
            want = [LEARNING_RATE / 10] + [LEARNING_RATE] * (G - 1) + [0.0, param * lambd, 1.0 if i == 0 else 0.0]
            assert np.array_equal(bits(t[r]), bits(want)), (epoch, i)
            r += 1
    assert np.array_equal(np.nonzero(t[:, G + 2])[0], np.arange(num_epochs - 1) * num_iterations)
    for it in (0, 1):
        row = t[it * num_iterations]
        assert bits(row[0]) == bits(f32(float(g[f"rate_{it}"]) / 10))
        assert all(bits(row[j]) == bits(f32(g[f"rate_{it}"])) for j in range(1, G))
    # G16's second lambd is the ramp at p = 0.3: epoch 3, i = 0 of this run (tests/test_dsan_cpu.py: dsan_lambd(30, 10, 10));
    # its first, p = 0.05, lies in epoch 0, which a run of 10 epochs cannot start with (the rate of main.py:316 divides by zero)
    assert bits(t[(3 - 1) * num_iterations, G + 1]) == bits(f32(float(g["lambd"][1]) * param))
    with pytest.raises(ZeroDivisionError):
        office_dsan(lr, num_epochs, num_iterations, param=param)
    t0 = office_dsan(lr, 20, 10, param=param, bottle_neck=bottle_neck).numpy()          # 20 epochs: num_iters 10 is p = 0.05, G16's first lambd
    assert bits(t0[10, G + 1]) == bits(f32(float(g["lambd"][0]) * param))


def test_hyper_block_stages_only_changes():
    from alignq_amd.schedule import HyperBlock
    b = HyperBlock("cpu", 3)
    assert b.cols == 6 and b.row.dtype == torch.float32
    b.set(lr=[0.1, 0.2, 0.3], alpha=0.5, fresh=1)
    assert b.copies == 1
    assert np.array_equal(bits(b.row.numpy()), bits([0.1, 0.2, 0.3, 0.5, 0.0, 1.0]))
    b.set(alpha=0.5)
    b.set(lr=[0.1, 0.2, 0.3])
    assert b.copies == 1                                      # nothing changed: nothing staged
    b.set(fresh=0)
    assert b.copies == 2 and float(b.fresh) == 0.0 and float(b.alpha) == 0.5
    b.set(lr=0.7, coef=0.25)
    assert [float(b.lr(i)) for i in range(3)] == [float(f32(0.7))] * 3 and float(b.coef) == 0.25
    assert b.lr(1).data_ptr() == b.row.data_ptr() + 4 and b.fresh.data_ptr() == b.row.data_ptr() + 20     # views, fixed addresses
    assert b.values() == b.read()
    with pytest.raises(ValueError):
        b.set(lr=[0.1, 0.2])
    b.invalidate()                                            # someone else wrote the row: the same values are staged again
    b.set(fresh=0)
    assert b.copies == 4


def test_new_exports_resolve_and_check_their_arguments_without_a_device():
    from alignq_amd import _lib as L
    lib = L.load()
    for name in ("alignq_sgd_step_multi_dev", "alignq_sgd_admm_step_multi_dev", "alignq_hyper_advance"):
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.alignq_abi_version() == L.ABI_VERSION == 23            # exports were added, the version was not bumped
    one = L.ptr_array([None])
    host = np.zeros(8, np.float32)
    ptr = host.ctypes.data                                             # non-NULL; never dereferenced by the checks below
    n = L.i64_array([8])
    arr = (L._c.c_void_p * 1)(ptr)
    sgd = (1, arr, arr, arr, n, one, one, L.i32_array([0]))
    tail = (0.9, 0.0, 1e-4, 0, 8, 1.0, 4.0)
    assert lib.alignq_sgd_step_multi_dev(*sgd, None, None, *tail, None) == L.EINVAL                      # NULL lr_dev
    assert lib.alignq_sgd_admm_step_multi_dev(*sgd, None, None, *tail, 1, arr, arr, arr, 2, 2, 0.2, 0.3, None) == L.EINVAL
    assert lib.alignq_sgd_step_multi_dev(0, arr, arr, arr, n, one, one, L.i32_array([0]), ptr, None, *tail, None) == L.EINVAL
    assert lib.alignq_hyper_advance(None, 5, 7, ptr, ptr, None) == L.EINVAL                              # NULL table
    assert lib.alignq_hyper_advance(ptr, 0, 7, ptr, ptr, None) == L.EINVAL                               # rows = 0
    assert lib.alignq_hyper_advance(ptr, 5, 7, None, ptr, None) == L.EINVAL
    assert lib.alignq_hyper_advance(ptr, 5, 7, ptr, None, None) == L.EINVAL
    assert lib.alignq_hyper_advance(ptr, 5, 65, ptr, ptr, None) == L.EINVAL                              # cols <= 64


def test_device_hyper_with_a_grad_hook_is_refused():
    from alignq_amd.resnet import PreActBlock_conv_Q, PreActResNet
    from alignq_amd.train_step import TrainStep
    net = PreActResNet(PreActBlock_conv_Q, [1, 1, 1], 8, 8, "second", 10)
    with pytest.raises(NotImplementedError):
        TrainStep(net, grad_hook=lambda step: None, device_hyper=True)


def tiny_office(cls):
    from alignq_amd.resnet_office import Bottleneck, ResNet
    return cls(lambda w, a, s: ResNet(w, a, s, Bottleneck, [1, 1, 1, 1], width_per_group=8), 4, 4, "aligned")


def test_device_hyper_refuses_the_data_parallel_route_of_dp_attach():
    """dp.attach / dp.attach_office install their hook by assignment after the step was built: refused there too, before
    anything is broadcast or changed (no process group is needed to see it); a hook assigned by hand is refused by capture and
    by the next iteration, before they touch the model."""
    from alignq_amd import dp
    from alignq_amd.resnet import PreActBlock_conv_Q, PreActResNet
    from alignq_amd.resnet_office import DANN
    from alignq_amd.train_step import OfficeTrainStep, TrainStep
    step = TrainStep(PreActResNet(PreActBlock_conv_Q, [1, 1, 1], 8, 8, "second", 10), device_hyper=True)
    fuse = [m.fuse_bn for m in step.model.modules() if hasattr(m, "fuse_bn")]
    for kw in ({}, {"global_corr": True}):
        with pytest.raises(NotImplementedError, match="device_hyper"):
            dp.attach(step, **kw)
    assert step.grad_hook is None and getattr(step, "_global_corr_undo", None) is None
    assert fuse == [m.fuse_bn for m in step.model.modules() if hasattr(m, "fuse_bn")]
    step.grad_hook = lambda s: None
    before = [p.detach().clone() for p in step.model.parameters()]
    x, y = torch.zeros(4, 3, 32, 32), torch.zeros(4, dtype=torch.long)
    for use in (lambda: step(x, y), lambda: step.capture(x, y, warmup=1), step._replay):
        with pytest.raises(NotImplementedError, match="device_hyper"):
            use()
    assert all(torch.equal(a, b) for a, b in zip(before, step.model.parameters()))
    step.grad_hook = None
    ostep = OfficeTrainStep(tiny_office(DANN), lr=0.004, device_hyper=True)
    with pytest.raises(NotImplementedError, match="device_hyper"):
        dp.attach_office(ostep)
    assert ostep.grad_hook is None and not ostep._staged
    # without device_hyper the hook is assigned as before
    plain = TrainStep(PreActResNet(PreActBlock_conv_Q, [1, 1, 1], 8, 8, "second", 10))
    hook = lambda s: None                                          # noqa: E731
    plain.grad_hook = hook
    assert plain.grad_hook is hook


def test_a_table_is_not_detached_and_lambd_is_only_optional_with_one():
    from alignq_amd.resnet_office import DSAN
    from alignq_amd.schedule import office_dsan
    from alignq_amd.train_step import DSANTrainStep
    for device_hyper in (False, True):
        step = DSANTrainStep(tiny_office(DSAN), lr=0.004, device_hyper=device_hyper)
        with pytest.raises(TypeError, match="lambd"):
            step(None, None, None)                                 # a forgotten lambd is an error, as it always was
    with pytest.raises(ValueError):
        step.set_schedule(None)
    step.set_schedule(office_dsan(0.004, 20, 5, param=0.3))
    with pytest.raises(ValueError):
        step.set_schedule(None)
    with pytest.raises(RuntimeError, match="table"):
        step.set_lambd(0.5)
