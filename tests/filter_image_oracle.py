"""Plain-NumPy statement of the two pre-packed bf16 filter images that alignq_weight_quant_fwd_multi_img writes for a channels-last
filter W_q [CO][KK][CI] (include/alignq.h, DESIGN.md "Filter images"):

    b(co, t, ci) = bf16(rint(W_q[co][t][ci] * (2^k - 1)))                       (bit pattern, uint16)
    F[CO/16][NSF][64][8], NSF = ceil(KK*CI/32):  F[g][s][16 qq + m][j] = b(16 g + m, t, c),   kk = 32 s + 8 qq + j, t = kk // CI, c = kk % CI
    D[CI/16][NSD][64][8], NSD = ceil(KK*CO/32):  D[g][s][16 qq + m][j] = b(co, ts, 16 g + m), kk = 32 s + 8 qq + j, t' = kk // CO,
                                                 co = kk % CO, ts = KK - 1 - t' if flip else t'
    +0 where t (t') >= KK.

Written slot by slot from the definition (loops over the DESTINATION), so that it shares nothing with the kernel's scatter over
the source elements."""
import numpy as np

GEOMETRIES = [(16, 9, 16), (32, 9, 32), (64, 9, 64), (32, 9, 16), (32, 1, 16), (64, 9, 32), (64, 1, 32)]      # (CO, KK, CI)


def image_elems(CO, KK, CI):
    """(elements of F, elements of D)"""
    nsf, nsd = (KK * CI + 31) // 32, (KK * CO + 31) // 32
    return (CO // 16) * nsf * 512, (CI // 16) * nsd * 512


def slot_sources(CO, KK, CI, flip):
    """Per image, an int64 array with one entry per slot: the flat index (co * KK + t) * CI + ci of the filter element the slot
    holds, or -1 for a padding slot."""
    out = []
    for rows, cols, fwd in ((CO, CI, True), (CI, CO, False)):
        ns = (KK * cols + 31) // 32
        src = np.full((rows // 16, ns, 64, 8), -1, dtype=np.int64)
        for g in range(rows // 16):
            for s in range(ns):
                for lane in range(64):
                    qq, m = lane >> 4, lane & 15
                    for j in range(8):
                        kk = 32 * s + 8 * qq + j
                        t, c = kk // cols, kk % cols
                        if t >= KK:
                            continue
                        if fwd:
                            co, tt, ci = 16 * g + m, t, c
                        else:
                            co, tt, ci = c, (KK - 1 - t if flip else t), 16 * g + m
                        src[g, s, lane, j] = (co * KK + tt) * CI + ci
        out.append(src.reshape(-1))
    return out


def bf16_bits(v):
    """bit patterns (uint16) of float32 values that are exactly representable in bf16 (integers of magnitude <= 255 are)"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any(), "not exact in bf16"
    return (u >> 16).astype(np.uint16)


def images(q, CO, KK, CI, flip, k):
    """q: the quantiser's output in storage order ([CO][KK][CI], any shape with CO*KK*CI float32 elements).
    Returns the whole buffer (F then D) as uint16."""
    q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1)
    assert q.size == CO * KK * CI
    b = bf16_bits(np.rint(q * np.float32(2 ** k - 1)))        # one IEEE fp32 product, round to nearest even: rintf(q * n)
    parts = []
    for src in slot_sources(CO, KK, CI, flip):
        img = np.zeros(src.size, dtype=np.uint16)
        live = src >= 0
        img[live] = b[src[live]]
        parts.append(img)
    return np.concatenate(parts)
