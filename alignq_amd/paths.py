"""The kernel-path flags of a model, set in one place.

A module class that reads a flag declares it as a class attribute holding its off value (quantization.Conv2d_Q, resnet.PreActBlock_conv_Q
/ PreActResNet, resnet_office.Bottleneck / ResNet, densenet.Conv2d_Q3 / DenseNet; the table is in DESIGN.md).  `apply` assigns a flag on every module of a model whose
class declares it and on no other; `restore` puts back what `apply` found.  The flags stay plain attributes: `m.use_qconv = False` on
one module works as before."""
from __future__ import annotations

FLAGS = ("use_qconv", "use_qconv_pw", "emit_bn_stats", "fuse_bn", "fuse_relu", "pack_bins", "_wq_stage", "use_qconv_k3",
         "fuse_dense_eval")
_ABSENT = object()


def apply(model, **flags):
    """Assign every given flag on the modules of `model` whose class declares it (none: not an error, e.g. pack_bins on MobileNet-V2).
    Returns the record `restore` takes: what each touched module's own __dict__ held before, absence included."""
    unknown = sorted(set(flags) - set(FLAGS))
    if unknown:
        raise TypeError(f"paths.apply: no such flag: {', '.join(unknown)} (the flags are {', '.join(FLAGS)})")
    record = []
    for m in model.modules():
        for name, value in flags.items():
            if hasattr(type(m), name):
                record.append((m, name, m.__dict__.get(name, _ABSENT)))
                setattr(m, name, value)
    return record


def restore(record):
    """Undo one `apply`: every instance __dict__ as it was (a flag that was only the class default is removed again).  Nested
    applies are restored in reverse order."""
    for m, name, old in reversed(record):
        if old is _ABSENT:
            m.__dict__.pop(name, None)
        else:
            m.__dict__[name] = old
