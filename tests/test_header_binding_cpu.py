"""The ctypes binding is read from include/alignq.h (alignq_amd/_header.py): the reader on synthetic headers, signatures of
the real header written out by hand (the independent statement of the type map), and the two argument records' layout against
the C compiler's."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

vp, i32, i64, f32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
u32, u64, sz = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t

SYNTHETIC = """\
/* demo.h: int alignq_in_comment(ws); the second launch of alignq_site_prep_fused[_multi], or
 * alignq_qconv_dgrad(ws); spread over lines */
#ifndef DEMO_H
#define DEMO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define ALIGNQ_ABI_VERSION 7
#define ALIGNQ_EINVAL (-1)   /* bad argument: int alignq_not_this(int); */
#define ALIGNQ_WIDE ( 12 )   // int alignq_line_comment(int x);
const char* alignq_name(int code);
size_t alignq_bytes(int64_t n, uint64_t seed);   /* see alignq_qconv_dgrad(ws) */
int64_t alignq_big(void);
int alignq_mix(const float* x, void* const* tab, int32_t k, unsigned flags, uint32_t v,
               float a, double b, const uint8_t* img, void* stream);
typedef struct alignq_rec {
  const float* z; float momentum, bn_eps; int C, HW, B; int64_t F;
  void* ws;   /* int alignq_hidden(int); */
} alignq_rec;
int alignq_take(const alignq_rec* a, unsigned* counter);
#ifdef __cplusplus
}
#endif
#endif /* DEMO_H */
"""


def _same(got, want):
    """restype and every argtype are the SAME ctypes objects, not merely equal-sized ones"""
    return got[0] is want[0] and len(got[1]) == len(want[1]) and all(a is b for a, b in zip(got[1], want[1]))


def test_reader_on_synthetic_text():
    from alignq_amd import _header
    functions, structs, constants = _header.parse(SYNTHETIC)
    want = {"alignq_name": (ctypes.c_char_p, [i32]),
            "alignq_bytes": (sz, [i64, u64]),
            "alignq_big": (i64, []),
            "alignq_mix": (i32, [vp, vp, i32, u32, u32, f32, f64, vp, vp]),
            "alignq_take": (i32, [vp, vp])}
    assert list(functions) == list(want)
    for name in want:
        assert _same(functions[name], want[name]), name
    assert structs == {"alignq_rec": [("z", vp), ("momentum", f32), ("bn_eps", f32), ("C", i32), ("HW", i32), ("B", i32),
                                      ("F", i64), ("ws", vp)]}
    assert constants == {"ALIGNQ_ABI_VERSION": 7, "ALIGNQ_EINVAL": -1, "ALIGNQ_WIDE": 12}


@pytest.mark.parametrize("header, offending", [
    ("int alignq_bad(const float* x, long n);", "long n"),                                         # unknown scalar type
    ("typedef struct { int a; } alignq_rec;\nint alignq_bad(alignq_rec r, void* stream);", "alignq_rec r"),   # struct by value
    ("int alignq_bad(void (*cb)(int), void* stream);", "void (*cb)(int)"),                         # function pointer
])
def test_reader_refuses_what_it_does_not_know(header, offending):
    from alignq_amd import _header
    with pytest.raises(_header.AlignQLibraryError) as e:
        _header.parse(header)
    assert offending in str(e.value)


def test_pinned_real_signatures_and_constants():
    from alignq_amd import _lib
    S = _lib.SIGNATURES
    assert len(S) == 149
    want = {
        "alignq_strerror": (ctypes.c_char_p, [i32]),
        "alignq_site_ws_bytes": (sz, [i32, i64]),
        "alignq_dwconv3x3_wgrad_ws_bytes": (i64, [i32] * 5),
        "alignq_lmmd_fwd": (i32, [vp, vp, vp, vp, i32, i64, i32, f64, i32, f64, vp, vp, vp]),
        "alignq_data_batch": (i32, [vp, vp, vp, vp, i32, vp, i64, i32, i32, i32, u64, i32, i32, vp, i32, vp, vp]),
        "alignq_dp_stream_wait_ge": (i32, [vp, vp, u32]),
        "alignq_site_partials_bn_twin": (i32, [vp, vp, vp]),
        "alignq_hyper_advance": (i32, [vp, i32, i32, vp, vp, vp]),
        "alignq_conv3x3_nhwc_bwd_fill_img": (i32, [vp] * 6 + [i32] * 5 + [vp] * 10 + [i32] * 3 + [vp] * 5),
        "alignq_site_partials_bn_fill": (i32, [vp] * 7 + [f32, f32, vp, vp, i32, i32, i32, i64, i32, f32, f32, i32, vp, i32, i32]
                                         + [vp] * 4 + [i32] + [vp] * 6 + [i32, f32, f32, vp]),
    }
    assert len(want["alignq_conv3x3_nhwc_bwd_fill_img"][1]) == 29 and len(want["alignq_site_partials_bn_fill"][1]) == 37
    for name in want:
        assert _same(S[name], want[name]), (name, S[name])
    assert (_lib.ABI_VERSION, _lib.MAX_BATCH, _lib.MAX_CORR_BATCH) == (23, 128, 1024)
    assert (_lib.EINVAL, _lib.EUNSUPPORTED, _lib.FORMULA_ADMM, _lib.FORMULA_CDF) == (-1, -2, 0, 1)


def test_record_layout_against_the_c_compiler(tmp_path):
    from alignq_amd import _lib
    cc = shutil.which("cc") or (os.path.exists("/opt/rocm/llvm/bin/clang") and "/opt/rocm/llvm/bin/clang")
    if not cc:
        pytest.skip("no C compiler: neither cc on PATH nor /opt/rocm/llvm/bin/clang")
    records = {"alignq_site_bn_args": _lib.SiteBnArgs, "alignq_site_bwd_bn_args": _lib.SiteBwdBnArgs}
    assert (len(_lib.SiteBnArgs._fields_), len(_lib.SiteBwdBnArgs._fields_)) == (26, 19)
    lines = ['#include <stdio.h>', '#include "alignq.h"', 'int main(void) {']
    for cname, cls in records.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {}
    for cname, cls in records.items():
        want[cname] = str(ctypes.sizeof(cls))
        want.update({f"{cname}.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert got == want
    assert (got["alignq_site_bn_args"], got["alignq_site_bwd_bn_args"]) == ("168", "136")
    assert (got["alignq_site_bn_args.F"], got["alignq_site_bwd_bn_args.dx_part"]) == ("96", "128")
