"""ctypes binding of libalignq_hip.so, derived from include/alignq.h at import (_header.py reads the prototypes, the two
argument records and the constants).  The product path has NO fallback: if the HIP library is missing or a tensor is not a CUDA
fp32 tensor, the call raises."""
from __future__ import annotations

import ctypes
import os

import torch

from . import _header
from ._header import AlignQLibraryError      # raised by load() and by the header reader

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("ALIGNQ_SO") or os.path.join(_HERE, "lib", "libalignq_hip.so")   # ALIGNQ_SO: A/B builds of tools/

_c = ctypes
# SIGNATURES: name -> (restype, argtypes), every prototype of the header (the path csrc/ includes it from)
SIGNATURES, _STRUCTS, _CONSTANTS = _header.read(os.path.join(_HERE, "..", "include", "alignq.h"))

FORMULA_ADMM, FORMULA_CDF = _CONSTANTS["ALIGNQ_FORMULA_ADMM"], _CONSTANTS["ALIGNQ_FORMULA_CDF"]
MAX_BATCH = _CONSTANTS["ALIGNQ_MAX_BATCH"]                 # rows the FUSED site kernels hold on chip
MAX_CORR_BATCH = _CONSTANTS["ALIGNQ_MAX_CORR_BATCH"]       # rows alignq_corr_fwd / _bwd take (blocked Gram above 128)
ABI_VERSION = _CONSTANTS["ALIGNQ_ABI_VERSION"]
EINVAL, EUNSUPPORTED = _CONSTANTS["ALIGNQ_EINVAL"], _CONSTANTS["ALIGNQ_EUNSUPPORTED"]

# MOBILE_SIGNATURES: the entry points of include/alignq_mobile.h (MobileNet-V2's folded evaluation sites), a table of its own:
# alignq.h's set of entry points and its ABI version are fixed, so an extension is declared next to it and never merged into SIGNATURES
MOBILE_SIGNATURES, _MOBILE_STRUCTS, _MOBILE_CONSTANTS = _header.read(os.path.join(_HERE, "..", "include", "alignq_mobile.h"))
CLAMP_NONE, CLAMP_RELU, CLAMP_RELU6 = (_MOBILE_CONSTANTS[n] for n in ("ALIGNQ_CLAMP_NONE", "ALIGNQ_CLAMP_RELU", "ALIGNQ_CLAMP_RELU6"))

# POINTWISE_SIGNATURES: the entry points of include/alignq_pointwise.h (the 1x1 Conv2d_Q convolutions at channel counts that are
# multiples of 8), a third table for the same reason: neither of the two sets above moves
POINTWISE_SIGNATURES, _POINTWISE_STRUCTS, _POINTWISE_CONSTANTS = _header.read(os.path.join(_HERE, "..", "include", "alignq_pointwise.h"))
PW_FWD, PW_DGRAD, PW_WGRAD = (_POINTWISE_CONSTANTS[n] for n in ("ALIGNQ_PW_FWD", "ALIGNQ_PW_DGRAD", "ALIGNQ_PW_WGRAD"))

# K3CONV_SIGNATURES: the entry points of include/alignq_k3conv.h (the 3x3 / stride 1 Conv2d_Q convolutions at channel counts that
# are multiples of 4), a fourth table, bound after the three above
K3CONV_SIGNATURES, _K3CONV_STRUCTS, _K3CONV_CONSTANTS = _header.read(os.path.join(_HERE, "..", "include", "alignq_k3conv.h"))
K3_FWD, K3_DGRAD, K3_WGRAD = (_K3CONV_CONSTANTS[n] for n in ("ALIGNQ_K3_FWD", "ALIGNQ_K3_DGRAD", "ALIGNQ_K3_WGRAD"))

# DENSE_SIGNATURES: the entry points of include/alignq_dense.h (DenseNet's evaluation without concatenations: a dense layer's site
# inside its 3x3 convolution, the transition's pool written at a pitch), a fifth table, bound last
DENSE_SIGNATURES, _DENSE_STRUCTS, _DENSE_CONSTANTS = _header.read(os.path.join(_HERE, "..", "include", "alignq_dense.h"))


class SiteBnArgs(ctypes.Structure):
    """include/alignq.h: alignq_site_bn_args (one site of alignq_site_partials_bn_twin; the arguments of alignq_site_partials_bn)"""
    _fields_ = _STRUCTS["alignq_site_bn_args"]


class SiteBwdBnArgs(ctypes.Structure):
    """include/alignq.h: alignq_site_bwd_bn_args (one site of alignq_site_bwd_apply_bn_twin; alignq_site_bwd_apply_bn's arguments)"""
    _fields_ = _STRUCTS["alignq_site_bwd_bn_args"]


class EvalSite(ctypes.Structure):
    """include/alignq_mobile.h: alignq_eval_site (one eval-mode batch-norm + quantiser + clamp)"""
    _fields_ = _MOBILE_STRUCTS["alignq_eval_site"]


class DenseSite(ctypes.Structure):
    """include/alignq_dense.h: alignq_dense_site (the eval-mode batch-norm + quantiser + clamp in front of a dense layer's convolution)"""
    _fields_ = _DENSE_STRUCTS["alignq_dense_site"]


_lib = None


def load():
    """Load the shared library (once).  Raises AlignQLibraryError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise AlignQLibraryError(
            f"{SO_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C alignq_amd/csrc` (hipcc --offload-arch=gfx950). alignq_amd has no CPU fallback.")
    lib = ctypes.CDLL(SO_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)       # AttributeError if the .so does not export what alignq.h declares
        fn.restype, fn.argtypes = res, args
    if lib.alignq_abi_version() != ABI_VERSION:
        raise AlignQLibraryError("libalignq_hip.so ABI version mismatch; rebuild")
    # the extension tables, in the order they were added (read from the module's globals now: a test models an older library by
    # emptying one)
    for table, header, source in (("MOBILE_SIGNATURES", "alignq_mobile.h", "mobile_eval_kernels.hip"),
                                  ("POINTWISE_SIGNATURES", "alignq_pointwise.h", "pointwise_kernels.hip"),
                                  ("K3CONV_SIGNATURES", "alignq_k3conv.h", "k3conv_kernels.hip"),
                                  ("DENSE_SIGNATURES", "alignq_dense.h", "dense_eval_kernels.hip")):
        for name, (res, args) in globals()[table].items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise AlignQLibraryError(f"{SO_PATH} does not export {name} (include/{header}): it was built before "
                                         f"csrc/{source} existed; rebuild it with `make -C alignq_amd/csrc`") from None
            fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().alignq_strerror(rc).decode()
        raise RuntimeError(f"{what}: {msg} (code {rc})")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def ptr_array(tensors):
    """HOST array of device pointers (NULL for None) for the multi-tensor entry points."""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def i64_array(values):
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def i32_array(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def _cuda_f32(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"alignq_amd: {name} is on {t.device}; the HIP kernels need a CUDA/ROCm tensor "
                           "(there is no CPU fallback in the product path)")
    if t.dtype != torch.float32:
        raise TypeError(f"alignq_amd: {name} must be float32, got {t.dtype}")


def dev_f32(t: torch.Tensor, name: str = "tensor") -> torch.Tensor:
    """Validate (CUDA, fp32) and return a contiguous view/copy.  No silent CPU path."""
    _cuda_f32(t, name)
    return t if t.is_contiguous() else t.contiguous()


def dense_f32(t: torch.Tensor, name: str = "tensor") -> torch.Tensor:
    """Like dev_f32 but also accepts channels-last (NHWC-strided) 4-D tensors without copying: the elementwise and
    per-site kernels only need ONE dense [B, F] row-major image of the storage (any fixed permutation of the feature
    axis leaves statistics, Gram matrices and elementwise results unchanged), so the storage is used as it lies."""
    _cuda_f32(t, name)
    if t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)):
        return t
    return t.contiguous()


def like_layout(g: torch.Tensor, ref: torch.Tensor, name: str = "grad") -> torch.Tensor:
    """Return g (CUDA fp32) laid out in memory exactly like ref (same strides), copying only if it is not."""
    if not g.is_cuda or g.dtype != torch.float32:
        raise TypeError(f"alignq_amd: {name} must be a CUDA float32 tensor")
    if g.stride() == ref.stride():
        return g
    out = torch.empty_like(ref)
    out.copy_(g)
    return out
