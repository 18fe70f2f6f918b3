"""The NumPy statement of the filter-image layouts (tests/filter_image_oracle.py) is itself consistent: on every geometry each
filter element appears in exactly one slot of each image, the remaining slots are padding and hold +0, and the values agree with
what the convolution kernels' fp32 branches form for lane (qq, m), k step s, element j."""
import numpy as np
import pytest

from tests import filter_image_oracle as FO


@pytest.mark.parametrize("CO,KK,CI", FO.GEOMETRIES)
@pytest.mark.parametrize("flip", [0, 1])
def test_each_live_slot_is_hit_exactly_once_and_padding_is_zero(CO, KK, CI, flip):
    nF, nD = FO.image_elems(CO, KK, CI)
    srcF, srcD = FO.slot_sources(CO, KK, CI, flip)
    assert srcF.size == nF and srcD.size == nD
    n = CO * KK * CI
    for src in (srcF, srcD):
        live = src[src >= 0]
        assert live.size == n
        assert np.array_equal(np.sort(live), np.arange(n))          # a permutation of the filter: every element exactly once
        assert src.size - live.size == src.size - n and src.size % 512 == 0
    # padding slots carry the bit pattern of +0 whatever the filter holds
    rng = np.random.default_rng(CO + KK + CI + flip)
    k = 8
    q = rng.integers(-255, 256, n).astype(np.float32) / np.float32(255)
    q[q == 0] = np.float32(1) / np.float32(255)                   # no zero bins: a zero slot then is a padding slot
    img = FO.images(q, CO, KK, CI, flip, k)
    assert img.size == nF + nD
    assert np.array_equal(img[:nF] == 0, srcF < 0) and np.array_equal(img[nF:] == 0, srcD < 0)


@pytest.mark.parametrize("CO,KK,CI", FO.GEOMETRIES)
def test_slots_are_the_fragments_the_fp32_branches_form(CO, KK, CI):
    """The kernels' own index arithmetic (csrc/conv_kernels.hip), written out: forward A[m = co][k = (tap, ci)] = W[co][tap][ci];
    body data gradient A[m = ci][k = (tap', co)] = W[co][KK - 1 - tap'][ci] (flip = 1), transition data gradient
    W[co][tap'][ci] (flip = 0)."""
    for flip in (0, 1):
        srcF, srcD = FO.slot_sources(CO, KK, CI, flip)
        nsf, nsd = (KK * CI + 31) // 32, (KK * CO + 31) // 32
        F = srcF.reshape(CO // 16, nsf, 64, 8)
        D = srcD.reshape(CI // 16, nsd, 64, 8)
        for g in range(CO // 16):
            for s in range(nsf):
                for lane in (0, 17, 38, 63):
                    q, m = lane >> 4, lane & 15
                    k0 = 32 * s + 8 * q
                    tap, c0 = k0 // CI, k0 % CI
                    for j in range(8):
                        want = ((16 * g + m) * KK + tap) * CI + c0 + j if tap < KK else -1
                        assert F[g, s, lane, j] == want
        for g in range(CI // 16):
            for s in range(nsd):
                for lane in (0, 17, 38, 63):
                    q, m = lane >> 4, lane & 15
                    k0 = 32 * s + 8 * q
                    tap, c0 = k0 // CO, k0 % CO
                    for j in range(8):
                        ts = KK - 1 - tap if flip else tap
                        want = ((c0 + j) * KK + ts) * CI + 16 * g + m if tap < KK else -1
                        assert D[g, s, lane, j] == want


def test_rounding_matches_rintf():
    """rint of one fp32 product, ties to even, as the kernels' rintf(q * n)"""
    q = np.array([0.5 / 3, 1.5 / 3, 2.5 / 3, -0.5 / 3, 1.0, -1.0, 0.0], dtype=np.float32)
    img = FO.images(np.resize(q, 16 * 9 * 16), 16, 9, 16, 1, 2)
    vals = set(np.unique(img).tolist())
    assert vals <= {0x0000, 0x8000, 0x3F80, 0xBF80, 0x4000, 0xC000, 0x4040, 0xC040}, [hex(v) for v in vals]
