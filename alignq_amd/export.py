"""Packed k-bit weight checkpoints (DESIGN.md "Packed weights"; include/alignq.h: alignq_weight_pack_multi / _unpack_multi).

A trained model leaves as the level indices of its quantised filters, bit-packed, plus everything else of its state_dict (batch-norm
parameters and buffers, biases, nn.Linear heads, filters with w_bit == 32) as it is; the ADMM alterD / gamma matrices, which only
training reads, are dropped unless asked for.  What is packed is weight_quantize_fn.forward's weight_q (the reference's
model/quantization.py:71-85 / :62-78): dequantising a packed filter gives exactly those values (-0 of the ADMM tree as +0).

    pk = pack_model(net)                      # on the GPU: quantise (fused.prequantize_weights), pack
    pk.save("net.alignq")                     # one torch.save of plain dicts of tensors and scalars
    pk = PackedModel.load("net.alignq")       # weights_only=True; works without a GPU
    skeleton = make_net(); pk.apply(skeleton) # batch-norm, head, ... ; the packed filters' .weight stay as they are
    with EvalStep(skeleton.cuda(), weights=pk) as ev:     # evaluates from the codes; the fp32 filters are never read
        ...
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .admm import ADMM

FORMAT, FORMAT_VERSION = "alignq-packed-weights", 1
_NO_CPU = "(there is no CPU fallback in the product path)"


def code_bits(w_bit, formula):
    """bits per code (alignq_weight_code_bits); 0: this w_bit has no packed form"""
    if not 1 <= int(w_bit) <= 16:
        return 0
    return int(w_bit) + 1 if formula == L.FORMULA_ADMM else int(w_bit)


def packed_bytes(n, bits):
    """alignq_packed_bytes: ceil(n / 32) * bits * 4"""
    return (int(n) + 31) // 32 * int(bits) * 4


def _stream_fits(f):
    """whether a filter entry's code tensor is the int32 stream its shape, w_bit and formula call for (the kernels trust the size)"""
    bits = code_bits(f["w_bit"], f["formula"])
    return (bits != 0 and int(f["bits"]) == bits and f["codes"].dtype == torch.int32 and f["codes"].dim() == 1
            and f["codes"].numel() * 4 == packed_bytes(PackedModel._numel(f), bits))


def quantised_convs(model):
    """[(state_dict key of the filter, module)] of the Conv2d_Q modules whose filters are quantised (w_bit < 32) by a quantiser that
    takes parked filters (weight_quantize_fn.parks_filters), in module order"""
    return [(name + ".weight", m) for name, m in model.named_modules()
            if hasattr(m, "quantize_fn") and getattr(m.quantize_fn, "w_bit", 32) != 32 and getattr(m.quantize_fn, "parks_filters", False)]


def admm_keys(model):
    """state_dict keys of the ADMM matrices (alterD, gamma): training state, not part of the evaluated function"""
    # (under every name a module has: an activation quantiser holds its site's ADMM module as `opt`, the block holds it too)
    return {f"{name}.{p}" for name, m in model.named_modules(remove_duplicate=False) if isinstance(m, ADMM)
            for p in ("alterD", "gamma")}


def pack_codes(qs, w_bit, formula):
    """(codes, bad): int32 code streams of the quantiser outputs `qs` (CUDA fp32 tensors, taken in storage order) from one
    alignq_weight_pack_multi call, and the number of elements no code dequantises to."""
    lib = L.load()
    bits = lib.alignq_weight_code_bits(int(w_bit), int(formula))
    if not bits:
        raise ValueError(f"alignq_amd: w_bit={w_bit} has no packed form (1..16)")
    qs = [L.dense_f32(q, "quantised filter") for q in qs]
    dev = qs[0].device
    codes = [torch.empty(lib.alignq_packed_bytes(q.numel(), bits) // 4, dtype=torch.int32, device=dev) for q in qs]
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(lib.alignq_weight_pack_multi(len(qs), L.ptr_array(qs), L.i64_array([q.numel() for q in qs]), int(w_bit), int(formula),
                                         L.ptr_array(codes), L.ptr(bad), L.stream_ptr()), "alignq_weight_pack_multi")
    return codes, int(bad.item())


def unpack_filters(codes, numels, w_bit, formula, qs=None, bins_bf16=None, bins_f16=None, images=None, geoms=None):
    """One alignq_weight_unpack_multi call (one launch per 64 tensors): from the code streams, fp32 W_q into qs, the GEMM
    convolutions' bins and the filter images (lists with None for a tensor that gets none; geoms: (CO, KK, CI, flip) per image)."""
    geom = None
    if images is not None and any(im is not None for im in images):
        flat = []
        for im, g in zip(images, geoms):
            flat += list(g) if im is not None else [0, 0, 0, 0]
        geom = (ctypes.c_int32 * len(flat))(*flat)

    def tab(ts):
        return None if ts is None or all(t is None for t in ts) else L.ptr_array(list(ts))
    L.check(L.load().alignq_weight_unpack_multi(len(codes), L.ptr_array(list(codes)), L.i64_array(numels), int(w_bit), int(formula),
                                                tab(qs), tab(bins_bf16), tab(bins_f16), tab(images) if geom is not None else None,
                                                geom, L.stream_ptr()), "alignq_weight_unpack_multi")


class PackedModel:
    """meta: {"format", "version", "act_range"}; filters: {"<module>.weight": {"codes": int32 tensor, "shape": [CO, CI, KH, KW],
    "w_bit", "formula", "bits"}} (codes of the channels-last storage [CO][KH][KW][CI]); rest: every other state_dict entry.  A plain
    container: CPU tensors work for everything but dequantize()."""

    def __init__(self, meta, filters, rest):
        self.meta, self.filters, self.rest = dict(meta), dict(filters), dict(rest)

    # ------------------------------------------------------------------------------------------------ file
    def save(self, path):
        torch.save({"meta": self.meta,
                    "filters": {k: dict(f, codes=f["codes"].detach().cpu()) for k, f in self.filters.items()},
                    "rest": {k: v.detach().cpu() for k, v in self.rest.items()}}, path)

    @classmethod
    def load(cls, path, map_location=None):
        blob = torch.load(path, map_location=map_location, weights_only=True)
        meta = blob.get("meta", {}) if isinstance(blob, dict) else {}
        if meta.get("format") != FORMAT or meta.get("version") != FORMAT_VERSION:
            raise ValueError(f"{path}: not a packed alignq_amd model of format version {FORMAT_VERSION} (meta = {meta})")
        return cls(meta, blob["filters"], blob["rest"])

    # ------------------------------------------------------------------------------------------------ sizes
    @staticmethod
    def _numel(f):
        n = 1
        for s in f["shape"]:
            n *= int(s)
        return n

    def nbytes(self):
        """bytes of the packed code streams plus the rest's tensors (exact; the file adds torch.save's framing)"""
        return (sum(packed_bytes(self._numel(f), f["bits"]) for f in self.filters.values())
                + sum(v.numel() * v.element_size() for v in self.rest.values()))

    def dense_nbytes(self):
        """the same tensors with every packed filter as fp32"""
        return (sum(4 * self._numel(f) for f in self.filters.values())
                + sum(v.numel() * v.element_size() for v in self.rest.values()))

    # ------------------------------------------------------------------------------------------------ use
    def apply(self, model):
        """Load `rest` into a model of the same architecture.  Strict about every key held here; the model may have, beyond them, only
        the packed filters (left alone) and the ADMM matrices."""
        sd = model.state_dict()
        problems = []
        for k, v in self.rest.items():
            if k not in sd:
                problems.append(f"unexpected key {k}")
            elif tuple(sd[k].shape) != tuple(v.shape):
                problems.append(f"shape of {k}: model {tuple(sd[k].shape)}, packed {tuple(v.shape)}")
        for k, f in self.filters.items():
            if k not in sd:
                problems.append(f"unexpected packed filter {k}")
            elif tuple(sd[k].shape) != tuple(f["shape"]):
                problems.append(f"shape of {k}: model {tuple(sd[k].shape)}, packed {tuple(f['shape'])}")
        tolerated = set(self.filters) | admm_keys(model)
        problems += [f"missing key {k}" for k in sd if k not in self.rest and k not in tolerated]
        if problems:
            raise ValueError("PackedModel.apply: " + "; ".join(problems))
        with torch.no_grad():
            for k, v in self.rest.items():
                sd[k].copy_(v)
        return model

    def dequantize(self, name):
        """fp32 W_q of the packed filter `name`: its logical shape [CO, CI, KH, KW] in channels-last memory, on the GPU"""
        f = self.filters[name]
        if not _stream_fits(f):
            raise ValueError(f"PackedModel.dequantize: the code stream of {name} does not have the size of its shape and bits")
        codes = f["codes"]
        if not codes.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError(f"alignq_amd: PackedModel.dequantize needs a CUDA/ROCm device {_NO_CPU}")
            codes = codes.cuda()
        shape = [int(s) for s in f["shape"]]
        q = torch.empty(shape, dtype=torch.float32, device=codes.device,
                        memory_format=torch.channels_last if len(shape) == 4 else torch.contiguous_format)
        unpack_filters([codes.contiguous()], [q.numel()], f["w_bit"], f["formula"], qs=[q])
        return q


def pack_model(model, keep_admm=False):
    """PackedModel of a trained model (on the GPU).  The filters are converted to channels-last as EvalStep does, quantised by
    fused.prequantize_weights and packed with one launch per (w_bit, formula) group.  ValueError naming the filter if a quantiser
    output has no code (NaN weights)."""
    from . import config, fused
    first = next(model.parameters(), None)
    if first is None or not first.is_cuda:
        raise RuntimeError(f"alignq_amd: pack_model needs the model on a CUDA/ROCm device {_NO_CPU}")
    model = model.to(memory_format=torch.channels_last)
    named = quantised_convs(model)
    convs = [c for _, c in named]
    groups = {}
    for name, c in named:
        k, formula = c.quantize_fn.w_bit, c.quantize_fn._formula
        if not code_bits(k, formula):
            raise ValueError(f"pack_model: {name} has w_bit={k}; only 1..16 (or 32: kept as fp32) can be packed")
        groups.setdefault((k, formula), []).append((name, c))
    filters = {}
    with torch.no_grad():
        fused.prequantize_weights(convs)
        try:
            for (k, formula), members in groups.items():
                qs = [c.quantize_fn.parked.q.detach() for _, c in members]
                codes, bad = pack_codes(qs, k, formula)
                if bad:
                    culprits = []
                    for (name, _), q, cd in zip(members, qs, codes):
                        back = torch.empty_like(q)
                        unpack_filters([cd], [q.numel()], k, formula, qs=[back])
                        if bool((back != q).any()):
                            culprits.append(name)
                    raise ValueError(f"pack_model: {bad} quantised value(s) without a code (non-finite weights?) in " + ", ".join(culprits))
                for (name, c), cd in zip(members, codes):
                    filters[name] = {"codes": cd, "shape": [int(s) for s in c.weight.shape], "w_bit": int(k), "formula": int(formula),
                                     "bits": code_bits(k, formula)}
        finally:
            for c in convs:
                c.quantize_fn.unpark()
    drop = set(filters) | (set() if keep_admm else admm_keys(model))
    rest = {k: v.detach().clone() for k, v in model.state_dict().items() if k not in drop}
    meta = {"format": FORMAT, "version": FORMAT_VERSION, "act_range": float(config.args.act_range)}
    return PackedModel(meta, filters, rest)


class PackedFilters:
    """EvalStep's side of `weights=`: checks a PackedModel against the model's quantised convolutions, holds the codes on the model's
    device and the tensors every begin() refreshes."""

    def __init__(self, pk, model):
        self.named = quantised_convs(model)
        problems = []
        for name, c in self.named:
            f = pk.filters.get(name)
            if f is None:
                problems.append(f"no packed filter for {name}")
                continue
            want = (tuple(c.weight.shape), int(c.quantize_fn.w_bit), int(c.quantize_fn._formula))
            have = (tuple(int(s) for s in f["shape"]), int(f["w_bit"]), int(f["formula"]))
            if want != have:
                problems.append(f"{name}: model (shape, w_bit, formula) = {want}, packed {have}")
            elif not _stream_fits(f):
                problems.append(f"{name}: the code stream does not have the size of its shape and bits")
        if problems:
            raise ValueError("EvalStep(weights=): " + "; ".join(problems))
        self.pk = pk
        self.codes = None        # per conv, on the device
        self.out = None          # id(conv) -> (q, bins or None, (image, its geometry) or None)

    def refresh(self, pack, images):
        """Unpack every filter (one call per (w_bit, formula) group) into tensors that stay the same across calls; returns
        {id(conv): fused.QuantizedFilter(conv.weight, q, bins=, image=)} (no cdf, no pdf)."""
        from . import fused
        lib = L.load()
        dev = self.named[0][1].weight.device if self.named else None
        if self.out is None or any(o[0].device != dev for o in self.out.values()):
            self.codes = {name: self.pk.filters[name]["codes"].to(dev).contiguous() for name, _ in self.named}
            self.out = {}
            for name, c in self.named:
                k = c.quantize_fn.w_bit
                q = torch.empty_like(c.weight)
                bins = image = None
                if pack and 1 <= k <= 8 and q.numel() % 4 == 0:
                    bins = (torch.empty_like(q, dtype=torch.int16), torch.empty_like(q, dtype=torch.int16))
                if images and 1 <= k <= 8 and c.use_qconv:
                    geo = fused.filter_image_geometry(c.weight)
                    if geo is not None:
                        image = (torch.empty(lib.alignq_filter_image_bytes(*geo[:3]), dtype=torch.uint8, device=dev), geo)
                self.out[id(c)] = (q, bins, image)
        groups = {}
        for name, c in self.named:
            groups.setdefault((c.quantize_fn.w_bit, c.quantize_fn._formula), []).append((name, c))
        for (k, formula), members in groups.items():
            outs = [self.out[id(c)] for _, c in members]
            unpack_filters([self.codes[name] for name, _ in members], [o[0].numel() for o in outs], k, formula,
                           qs=[o[0] for o in outs],
                           bins_bf16=[o[1][0] if o[1] else None for o in outs], bins_f16=[o[1][1] if o[1] else None for o in outs],
                           images=[o[2][0] if o[2] else None for o in outs], geoms=[o[2][1] if o[2] else None for o in outs])
        recs = {}
        for _, c in self.named:
            q, bins, image = self.out[id(c)]
            recs[id(c)] = fused.QuantizedFilter(c.weight, q, bins=bins, image=image[0] if image else None)
        return recs
