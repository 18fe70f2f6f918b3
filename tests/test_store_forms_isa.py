"""The large outputs the batch-128 site kernels and the CIFAR convolutions leave to the next launch are stored WRITE-THROUGH
(csrc/store_forms.h: 16-byte stores carrying the sc1 cache bit), and -DALIGNQ_PLAIN_STORES restores plain stores in exactly
those kernels.  Asserted on the gfx950 assembly of both builds (cross-compiled: no GPU needed): the cache bit is an ISA property
no numerical test can see - the values and addresses are the same either way."""
import concurrent.futures
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mangled-name patterns of the converted instantiations, per file
CONVERTED = {
    "site4_kernels.hip": [
        # site_fwd4_kernel<TF, PAIR, SINGLE = true, 1024, FULLP>: every one-tile form (slab epilogue; FULLP: x_q / y as well)
        r"site_fwd4_kernelILi(64|32)ELb[01]ELb1ELi1024ELb[01]E",
        # site_bwd4_kernel<TF, PAIR, BN, VEC = true, LOOP = false, FULLP>: the vectorised one-tile forms (dres, dx)
        r"site_bwd4_kernelILi(64|32)ELb[01]ELb[01]ELb1ELb0ELb[01]E",
    ],
    "conv_kernels.hip": [
        r"conv3x3_nhwc_kernelI", r"conv3x3_bwd_kernelI", r"convgen_fwd_kernelI", r"dgrad_s2_kernelI", r"transition_fwd_kernelI",
        r"transition_bwd_kernelI", r"stem_fwd_kernelE",
    ],
}
# forms that keep plain stores in BOTH builds: the multi-tile forward, the looped backward, the dword backward
PLAIN_FORMS = {
    "site4_kernels.hip": [r"site_fwd4_kernelILi64ELb[01]ELb0ELi(1024|512)ELb0E", r"site_bwd4_kernelILi(64|32)ELb[01]ELb0ELb1ELb1ELb0E",
                          r"site_bwd4_kernelILi(64|32)ELb[01]ELb[01]ELb0ELb0ELb0E"],
    "conv_kernels.hip": [],
}
WT16 = re.compile(r"^(global|buffer)_store_dwordx4 .*\bsc1\b")


def _isa(args):
    src, flags = args
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT}/include",
           f"-I{ROOT}/alignq_amd/csrc", "--cuda-device-only", "-S", os.path.join(ROOT, "alignq_amd", "csrc", src), "-o", "-"] + flags
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out, name = {}, None
    for line in res.stdout.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                name = None
            else:
                out[name].append(line.strip())
    return out


@pytest.fixture(scope="module")
def isa():
    jobs = [(src, flags) for src in CONVERTED for flags in ([], ["-DALIGNQ_PLAIN_STORES"])]
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:
        res = list(pool.map(_isa, jobs))
    return {(src, bool(flags)): r for (src, flags), r in zip(jobs, res)}


def _count(body):
    return sum(1 for ln in body if WT16.match(ln))


@pytest.mark.parametrize("src", sorted(CONVERTED))
def test_converted_kernels_write_through_and_the_plain_build_does_not(isa, src):
    new, plain = isa[(src, False)], isa[(src, True)]
    assert set(new) == set(plain)
    for pat in CONVERTED[src]:
        names = [k for k in new if re.search(pat, k)]
        assert names, (src, pat)
        for k in names:
            assert _count(new[k]) >= 1, ("no 16-byte sc1 store", k)
            assert _count(plain[k]) == 0, ("the plain build stores write-through", k)


@pytest.mark.parametrize("src", sorted(CONVERTED))
def test_unconverted_forms_and_hand_offs_are_the_same_code_in_both_builds(isa, src):
    new, plain = isa[(src, False)], isa[(src, True)]
    for pat in PLAIN_FORMS[src]:
        names = [k for k in new if re.search(pat, k)]
        assert names, (src, pat)
        for k in names:
            assert _count(new[k]) == 0, k
    converted = [k for k in new if any(re.search(p, k) for p in CONVERTED[src])]
    assert 8 <= len(converted) < len(new)
    strip = lambda body: [ln for ln in body if ln and not ln.startswith((";", "."))]      # instructions only
    for k in new:
        if "s_endpgm" not in new[k]:
            continue                                     # (a data symbol, not a kernel)
        if k not in converted and "wgrad" not in k:      # (the filter-gradient slabs: 4-byte write-through stores)
            assert strip(new[k]) == strip(plain[k]), k      # the ticket hand-offs (slab_reduce*, the head role) among them
