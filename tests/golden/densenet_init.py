"""Deterministic parameters of the DenseNet fixtures (G21), shared by the generator (reference side) and the tests (this
repository's model): det_init.det_init_ as it stands - every batch-norm of the model has `bn` in its name (`dense1.0.bn1`, `trans1.bn1`,
`bn`), so every gain is drawn around 1 - and the reduced geometry both sides build."""
try:
    from .det_init import det_init_          # imported as tests.golden.densenet_init (the tests)
except ImportError:
    from det_init import det_init_           # imported from the generator's own directory

REDUCED = dict(depth=10, compressionRate=1)      # 3x3: 24, 36 | 48, 60 | 72, 84 -> 12; transitions 48 -> 48 and 72 -> 72
TF_LAYERS = (("dense1", 0), ("dense2", 0), ("dense2", 1), ("dense3", 1))      # the teacher-forced dense layers of G21 (b)


def densenet_init_(module, seed=2100):
    return det_init_(module, seed)
