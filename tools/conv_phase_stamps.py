"""Phase stamps of the body convolutions (diagnostic build `make -C alignq_amd/csrc stamps`, or ALIGNQ_SO = another library
built with -DALIGNQ_STAMPS; see tools/README.md): at batch 128 and C = 16 / 32 / 64, the forward launch (workgroup 0) and the
one-launch backward in the lazy batch-norm form with int16 index operands, as the captured step runs them (one stamped workgroup
per role, and every workgroup's entry / exit).  Times in us from the launch's first workgroup entry (backward) or from the
stamped workgroup's entry (forward).
    python tools/conv_phase_stamps.py [--images]
--images: the filter comes from the weight quantiser's launch together with its pre-packed bf16 images, and the convolutions read the
images (alignq_conv3x3_nhwc_img / alignq_conv3x3_nhwc_bwd_fill_img)."""
import ctypes, os, sys, numpy as np, torch
sys.path.insert(0, '.')
from alignq_amd import _lib as L
if not os.environ.get("ALIGNQ_SO"):
    L.SO_PATH = 'tools/lib/libalignq_stamps.so'
lib = L.load()
lib.alignq_debug_read_conv_stamps.argtypes = [ctypes.c_void_p]
lib.alignq_debug_read_conv_block_stamps.argtypes = [ctypes.c_void_p]
dev = torch.device('cuda:0')
IMAGES = "--images" in sys.argv[1:]
B, k = 128, 8
p = L.ptr


def stamps():
    buf = (ctypes.c_ulonglong * 64)()
    lib.alignq_debug_read_conv_stamps(buf)
    return np.array(buf, dtype=np.int64) * 0.01          # 100 MHz -> us


def blocks(n):
    buf = (ctypes.c_ulonglong * (2 * 4096))()
    lib.alignq_debug_read_conv_block_stamps(buf)
    return np.array(buf, dtype=np.int64).reshape(2, 4096)[:, :n] * 0.01


def fmt(names, t, t0):
    return " | ".join(f"{n} {v - t0:.2f}" for n, v in zip(names, t))


print("library", os.path.basename(L.SO_PATH), "| filter images" if IMAGES else "| fp32 filter")
torch.manual_seed(0)
for (C, H) in ((16, 32), (32, 16), (64, 8)):
    n = 2 ** k - 1
    cl = torch.channels_last
    x = torch.randn(B, C, H, H, device=dev).contiguous(memory_format=cl)
    xi = torch.randint(0, 256, (B, H, H, C), device=dev, dtype=torch.int16)
    w = (torch.round(torch.tanh(torch.randn(C, C, 3, 3)) * n) / n).to(dev).contiguous(memory_format=cl)
    img = None
    if IMAGES:       # W_q and its images from one quantiser launch
        raw = (torch.randn(C, C, 3, 3) * 0.05).to(dev).contiguous(memory_format=cl)
        w, wc, wp = torch.empty_like(raw), torch.empty_like(raw), torch.empty_like(raw)
        img = torch.empty(lib.alignq_filter_image_bytes(C, 9, C), dtype=torch.uint8, device=dev)
        wms = torch.empty(1, 2, device=dev)
        wws = torch.empty(lib.alignq_weight_multi_ws_bytes(1), dtype=torch.uint8, device=dev)
        L.check(lib.alignq_weight_quant_fwd_multi_img(1, L.ptr_array([raw]), L.ptr_array([w]), L.ptr_array([wc]), L.ptr_array([wp]),
                                                      L.i64_array([raw.numel()]), p(wms), k, 0, p(wws), L.ptr_array([img]),
                                                      (ctypes.c_int32 * 4)(C, 9, C, 1), L.stream_ptr()), "weight quantiser")
    y, dx = torch.empty_like(x), torch.empty_like(x)
    g, z = torch.randn_like(x) * 0.01, torch.randn_like(x)
    add = torch.randn_like(x)
    ab, save = torch.rand(2, C, device=dev) + 0.5, torch.rand(2, C, device=dev) + 0.5
    part = torch.randn(2 * C * H * H, device=dev) * 0.01          # at least [n_tiles][min(C, tile_f)][2]
    dgam, dbet = torch.empty(C, device=dev), torch.empty(C, device=dev)
    n_parts = lib.alignq_conv3x3_bn_parts(B, H, H, C)
    bnp = torch.empty(C, n_parts, 2, device=dev)
    ws = torch.empty(lib.alignq_conv3x3_wgrad_ws_bytes(C), dtype=torch.uint8, device=dev)
    ns = ctypes.c_int(0)
    st = L.stream_ptr()
    for xb, name in ((0, "fp32"), (2, "int16")):
        for it in range(3):
            tail = (p(y), B, H, H, C, k, 0, None, p(bnp), p(xi) if xb else None, xb, k if xb else 0, st)
            if IMAGES:
                L.check(lib.alignq_conv3x3_nhwc_img(None if xb else p(x), p(w), p(img), *tail), "fwd")
            else:
                L.check(lib.alignq_conv3x3_nhwc(None if xb else p(x), p(w), *tail), "fwd")
            torch.cuda.synchronize()
        a = stamps()
        print(f"C={C} forward {name:5s} wg 0: " + fmt(("loads issued", "filter ready", "tile staged", "MFMA done", "stored"),
                                                         a[[1, 3, 2, 4, 5]], a[0]))
        for it in range(3):
            tail = (p(dx), p(ws), B, H, H, C, k, ctypes.byref(ns), p(add), p(z), p(ab), p(save), None, p(part), p(dgam), p(dbet),
                    p(xi) if xb else None, xb, k if xb else 0)
            if IMAGES:
                L.check(lib.alignq_conv3x3_nhwc_bwd_fill_img(None if xb else p(x), p(g), p(w), p(img), *tail, 0, None, None, None, None,
                                                             st), "bwd")
            else:
                L.check(lib.alignq_conv3x3_nhwc_bwd(None if xb else p(x), p(g), p(w), *tail, st), "bwd")
            torch.cuda.synchronize()
        a = stamps()
        NB = (C // 32) ** 2 if C >= 32 else 1
        n_w = ns.value * NB
        n_d = B * H // ((256 if C == 16 else 128 if C == 32 else 32) // H)
        e = blocks(n_w + n_d)
        t0 = e[0].min()
        ent, ext = e[0] - t0, e[1] - t0
        per = (a[18:50:2] > a[16]).sum()                 # tiles of the stamped filter-gradient workgroup (this launch's stamps)
        print(f"C={C} backward {name:5s} grid {n_w} filter-gradient + {n_d} data-gradient workgroups")
        for role, sl in (("filter-gradient", slice(0, n_w)), ("data-gradient  ", slice(n_w, n_w + n_d))):
            d = ext[sl] - ent[sl]
            print(f"   {role}: entry p50 {np.median(ent[sl]):.2f} max {ent[sl].max():.2f} | residency min {d.min():.2f} p50 "
                  f"{np.median(d):.2f} max {d.max():.2f} | last exit {ext[sl].max():.2f}")
        last = np.sort(ent)[-256:]
        print(f"   last 256 workgroups enter at {last.min():.2f} .. {last.max():.2f}; launch span (first entry -> last exit) {ext.max():.2f}")
        print("   data-gradient tile 0:  " + fmt(("entry", "loads issued", "filter ready", "tile staged", "MFMA done", "stored"),
                                                  a[[8, 9, 11, 10, 12, 13]], t0))
        tl = " | ".join(f"t{i} staged {a[18 + 2 * i] - t0:.2f} mfma {a[19 + 2 * i] - t0:.2f}" for i in range(int(per)))
        print(f"   filter-gradient wg 0:  entry {a[16] - t0:.2f} | prologue {a[17] - t0:.2f} | {tl} | acc final {a[50] - t0:.2f} | "
              f"stored {a[51] - t0:.2f}")
