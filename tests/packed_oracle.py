"""Plain-NumPy statement of the packed k-bit weight format (include/alignq.h, DESIGN.md "Packed weights").

    k = w_bit in 1..16, n = 2^k - 1, b = rint(W_q * n)
    ADMM tree (formula 0, levels -n..n):   code = b + n          bits = k + 1
    CDF tree  (formula 1, W_q = 2 i/n - 1): code = i = (b + n)/2  bits = k
    dequant: one IEEE fp32 division, (code - n)/n, or (code/n)*2 - 1
    stream:  groups of 32 elements; group g = the uint32 words [g*bits, g*bits + bits) read as one little-endian integer of
             32*bits bits; element e of the group = its bits [e*bits, (e+1)*bits); the last group zero-padded

`pack` loops over the DESTINATION words (each word gathers the bits of the elements that overlap it), so it shares nothing with the
kernel's scatter from the source elements."""
import numpy as np


def code_bits(k, formula):
    return k + 1 if formula == 0 else k


def packed_words(n, bits):
    return (n + 31) // 32 * bits


def codes(wq, k, formula):
    """uint32 codes of quantiser outputs (any shape, float32), flattened in storage order"""
    wq = np.ascontiguousarray(wq, dtype=np.float32).reshape(-1)
    n = 2 ** k - 1
    b = np.rint(wq * np.float32(n)).astype(np.int64)            # one IEEE fp32 product, round to nearest even: rintf(W_q * n)
    s = b + n
    assert s.min() >= 0 and s.max() <= 2 * n
    if formula == 0:
        return s.astype(np.uint32)
    assert not (s & 1).any()
    return (s >> 1).astype(np.uint32)


def dequant(c, k, formula):
    c = np.asarray(c, dtype=np.uint32)
    n = 2 ** k - 1
    if formula == 0:
        return ((c.astype(np.int64) - n).astype(np.float32) / np.float32(n)).astype(np.float32)
    return ((c.astype(np.float32) / np.float32(n)) * np.float32(2) - np.float32(1)).astype(np.float32)


def pack(c, bits):
    """uint32 words of the stream of the codes c (1-D, every code < 2^bits)"""
    c = np.asarray(c, dtype=np.uint32).reshape(-1)
    assert 1 <= bits <= 17 and (c.size == 0 or int(c.max()) < 2 ** bits)
    n = c.size
    groups = (n + 31) // 32
    padded = np.zeros(groups * 32, dtype=np.uint64)
    padded[:n] = c
    padded = padded.reshape(groups, 32)
    words = np.zeros((groups, bits), dtype=np.uint32)
    for w in range(bits):                                   # destination word w of every group: bits [32 w, 32 w + 32)
        acc = np.zeros(groups, dtype=np.uint64)
        for e in range(32):
            lo = e * bits                                   # the element's first bit in the group
            if lo + bits <= 32 * w or lo >= 32 * w + 32:
                continue
            sh = lo - 32 * w
            part = padded[:, e] << np.uint64(sh) if sh >= 0 else padded[:, e] >> np.uint64(-sh)
            acc |= part & np.uint64(0xFFFFFFFF)
        words[:, w] = acc.astype(np.uint32)
    return words.reshape(-1)


def unpack(words, n, bits):
    """the n codes of a stream"""
    words = np.asarray(words, dtype=np.uint32).reshape(-1)
    groups = (n + 31) // 32
    assert words.size == groups * bits
    out = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        g, e = divmod(i, 32)
        big = 0
        for w in range(bits):
            big |= int(words[g * bits + w]) << (32 * w)
        out[i] = (big >> (e * bits)) & (2 ** bits - 1)
    return out


def unpack_fast(words, n, bits):
    """unpack for large tensors (vectorised over the groups; same definition)"""
    words = np.asarray(words, dtype=np.uint32).reshape(-1, bits).astype(np.uint64)
    out = np.zeros((words.shape[0], 32), dtype=np.uint32)
    for e in range(32):
        lo = e * bits
        w, sh = divmod(lo, 32)
        v = words[:, w] >> np.uint64(sh)
        if sh + bits > 32:
            v = v | (words[:, w + 1] << np.uint64(32 - sh))
        out[:, e] = (v & np.uint64(2 ** bits - 1)).astype(np.uint32)
    return out.reshape(-1)[:n]
