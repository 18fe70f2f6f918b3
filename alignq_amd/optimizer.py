"""SGD and ADMM_OPT — drop-ins for the reference's utils/optimizer.py (ADMM_OPT :15-135, SGD :138-262),
same constructor and step() signatures, both torch.optim.Optimizer subclasses (state_dict keeps the
`momentum_buffer` key, main.py:142-143).  The arithmetic runs in HIP kernels (alignq_sgd_step,
alignq_sgd_grad_approx, alignq_admm_update); parameters are updated IN PLACE at fixed addresses so the
whole step is HIP-graph capturable (the reference rebinds `p.data` to fresh tensors).

Reference quirks kept:
  * SGD: for tensors in `idx` the update still uses the un-approximated direction; only the value left
    in p.grad is `dir * sigmoid_d(transform(w_cdf)) * w_pdf`;
  * ADMM_OPT: parameters whose grad is None are skipped; the dual update uses the padded D and the NEW
    alterD of the alterD parameter that precedes it in the parameter list.
"""
from __future__ import annotations

import torch
from torch.optim.optimizer import Optimizer

from . import _lib as L
from . import config


class SGD(Optimizer):
    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: {}".format(momentum))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov))
        self._hyper = None

    def attach_hyper(self, block):
        """Read the learning rates (and the `fresh` flag) from `block` (alignq_amd.schedule.HyperBlock: one rate slot per parameter
        group, in order) instead of passing group["lr"] by value: the launches go to the `_dev` entry points, so a captured step
        follows whatever the block holds at replay time.  Every momentum buffer is created here (zeros): a buffer is then never
        born inside a capture, and "this step starts the momentum afresh" (a new SGD in the reference, utils/optimizer.py:222-224)
        is the block's `fresh` slot, under which the kernel does not read the buffer."""
        if block.n_groups != len(self.param_groups):
            raise ValueError(f"SGD.attach_hyper: the block has {block.n_groups} rate slots, the optimizer {len(self.param_groups)} "
                             "parameter groups")
        for group in self.param_groups:
            if group["momentum"] != 0:
                for p in group["params"]:
                    if "momentum_buffer" not in self.state[p]:
                        self.state[p]["momentum_buffer"] = torch.zeros_like(p)
        self._hyper = block
        return self

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("nesterov", False)
        self.__dict__.setdefault("_hyper", None)

    def _gather(self, idx, w_cdf, w_pdf):
        """Per parameter group: (hyper-parameters, tensors of the multi-tensor launch); creates missing momentum buffers."""
        bitW = int(config.args.bitW)
        out = []
        for gi, group in enumerate(self.param_groups):
            wd, mom, damp, nest, lr = (group["weight_decay"], group["momentum"], group["dampening"],
                                       group["nesterov"], group["lr"])
            ps, gs, bufs, firsts, cdfs, pdfs = [], [], [], [], [], []
            for i, p in enumerate(group["params"]):
                if p.grad is None:
                    continue
                if L.dense_f32(p, "parameter") is not p:
                    raise RuntimeError("alignq_amd.SGD needs dense (contiguous or channels-last) parameters")
                g = p.grad
                if g.stride() != p.stride():
                    g = p.grad = L.like_layout(g, p)
                first, buf = 0, None
                if mom != 0:
                    state = self.state[p]
                    if "momentum_buffer" not in state:
                        state["momentum_buffer"] = torch.empty_like(p)
                        first = 1
                    buf = state["momentum_buffer"]
                c = pdf = None
                if bitW < 32 and i in idx:
                    j = idx.index(i)
                    c, pdf = L.like_layout(w_cdf[j].detach(), p, "w_cdf"), L.like_layout(w_pdf[j].detach(), p, "w_pdf")
                ps.append(p); gs.append(g); bufs.append(buf); firsts.append(first); cdfs.append(c); pdfs.append(pdf)
            if ps:
                out.append(((float(lr), float(mom), float(damp), float(wd), int(bool(nest))), ps, gs, bufs, firsts, cdfs, pdfs, gi))
        return out

    @staticmethod
    def _c_args(item, hyper=None):
        """The argument prefix alignq_sgd_step_multi and alignq_sgd_admm_step_multi share; with `hyper` (a HyperBlock) that of
        their `_dev` forms: the group's rate slot and the `fresh` slot as device pointers in place of the rate."""
        (lr, mom, damp, wd, nest), ps, gs, bufs, firsts, cdfs, pdfs, gi = item
        rate = (lr,) if hyper is None else (L.ptr(hyper.lr(gi)), L.ptr(hyper.fresh))
        return (len(ps), L.ptr_array(ps), L.ptr_array(gs), L.ptr_array(bufs) if mom != 0 else None,
                L.i64_array([p.numel() for p in ps]), L.ptr_array(cdfs), L.ptr_array(pdfs), L.i32_array(firsts)) + rate + \
            (mom, damp, wd, nest, min(int(config.args.bitW), 30))

    @torch.no_grad()
    def step(self, idx, w_cdf, w_pdf, lam, lam2, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._launch(self._gather(idx, w_cdf, w_pdf), lam, lam2)
        return loss

    def _launch(self, items, lam, lam2):
        """Run gathered groups.  `items` carries the `first` flags of momentum buffers `_gather` has just created (uninitialised
        memory the kernel must overwrite, not read): whoever gathers must launch THESE items, never gather again."""
        lib = L.load()
        st = L.stream_ptr()
        hyper = self._hyper
        for item in items:
            # one multi-tensor launch (per <=72 tensors) for the whole group: step + p.grad rewrite for idx members
            if hyper is not None:
                L.check(lib.alignq_sgd_step_multi_dev(*self._c_args(item, hyper), float(lam), float(lam2), st),
                        "alignq_sgd_step_multi_dev")
                continue
            L.check(lib.alignq_sgd_step_multi(*self._c_args(item), float(lam), float(lam2), st), "alignq_sgd_step_multi")


class ADMM_OPT(Optimizer):
    def __init__(self, params):
        super().__init__(params, dict())

    @torch.no_grad()
    def step(self, alterD_idx, gamma_idx, Ds, alterDs, gammas, mus, rhos, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if int(config.args.bitW) >= 32:
            raise KeyError("lr")   # the reference's non-quantised branch reads group['lr'], which ADMM_OPT never defines
        for (mu, rho, b, dim), sites in self._gather(alterD_idx, gamma_idx, Ds, gammas, mus, rhos).items():
            lib = L.load()
            # above dim = 128 (the exact-global correlation's ADMM(dim = B_g)): 64 workgroups per site through a workspace
            ws = (torch.empty(lib.alignq_admm_update_ws_bytes(len(sites), dim), dtype=torch.uint8, device=sites[0][1].device)
                  if dim > 128 else None)
            L.check(lib.alignq_admm_update_ws(L.ptr_array([s_[0] for s_ in sites]), L.ptr_array([s_[1] for s_ in sites]),
                                              L.ptr_array([s_[2] for s_ in sites]), len(sites), b, dim, mu, rho, L.ptr(ws),
                                              L.stream_ptr()), "alignq_admm_update_ws")
        return loss

    def _gather(self, alterD_idx, gamma_idx, Ds, gammas, mus, rhos):
        """{(mu, rho, b, dim): [(D, alterD, gamma)]}: walks the parameter list like utils/optimizer.py:76-124."""
        groups = {}
        for group in self.param_groups:
            params = group["params"]
            pending = None            # (j, alterD param) waiting for its dual
            for i, p in enumerate(params):
                if p.grad is None:
                    continue
                if i in alterD_idx:
                    if pending is not None:
                        raise NotImplementedError("alterD parameter without its gamma right after it")
                    pending = (alterD_idx.index(i), p)
                elif i in gamma_idx:
                    if pending is None:
                        raise NotImplementedError("gamma parameter whose alterD was skipped (grad None)")
                    j, pa = pending
                    if gammas[j] is not p:
                        raise NotImplementedError("gamma parameter order does not pair with its alterD")
                    pending = None
                    D = L.dev_f32(Ds[j].detach(), "D")
                    L.dev_f32(pa, "alterD")
                    L.dev_f32(p, "gamma")
                    b, dim = D.shape[0], pa.shape[0]
                    groups.setdefault((float(mus[j]), float(rhos[j]), b, dim), []).append((D, pa, p))
                else:
                    raise KeyError("lr")
            if pending is not None:
                # alterD updated, dual skipped: do the primal only by pairing with a scratch dual
                raise NotImplementedError("alterD parameter without a following gamma parameter")
        return groups


@torch.no_grad()
def sgd_admm_step(sgd, sgd_args, admm, admm_args):
    """`sgd.step(*sgd_args)` then `admm.step(*admm_args)` (main.py:330-340) with ONE kernel launch when the two optimizers
    hold disjoint parameters (the CIFAR drivers split alterD / gamma off by name), there is one SGD group and all sites share
    (mu, rho, b, dim); anything else runs the two steps as they are.  Same results either way."""
    idx, w_cdf, w_pdf, lam, lam2 = sgd_args
    alterD_idx, gamma_idx, Ds, alterDs, gammas, mus, rhos = admm_args
    if int(config.args.bitW) < 32:
        mine = {id(p) for g in sgd.param_groups for p in g["params"]}
        disjoint = not any(id(p) in mine for g in admm.param_groups for p in g["params"])
        # eligibility is decided BEFORE any optimizer state is created: _gather makes the missing momentum buffers and reports
        # them only in the items it returns (round-3 advisor finding: items gathered here and dropped left buffers that a second
        # gather took for initialised ones)
        one_group = sum(1 for g in sgd.param_groups if any(p.grad is not None for p in g["params"])) == 1
        groups = admm._gather(alterD_idx, gamma_idx, Ds, gammas, mus, rhos) if disjoint and one_group else None
        # (above dim = 128 the ADMM role of the one-launch form would walk dim^2 elements with one workgroup per site: 1 ms at
        #  dim = 1024; the separate steps take the many-workgroup update)
        if groups is not None and len(groups) == 1 and next(iter(groups))[3] <= 128:
            items = sgd._gather(idx, w_cdf, w_pdf)
            assert len(items) == 1
            ((mu, rho, b, dim), sites), = groups.items()
            hyper = sgd._hyper
            name = "alignq_sgd_admm_step_multi" if hyper is None else "alignq_sgd_admm_step_multi_dev"
            L.check(getattr(L.load(), name)(
                *SGD._c_args(items[0], hyper), float(lam), float(lam2), len(sites), L.ptr_array([s_[0] for s_ in sites]),
                L.ptr_array([s_[1] for s_ in sites]), L.ptr_array([s_[2] for s_ in sites]), b, dim, mu, rho, L.stream_ptr()),
                name)
            return
    sgd.step(idx, w_cdf, w_pdf, lam, lam2)
    admm.step(alterD_idx, gamma_idx, Ds, alterDs, gammas, mus, rhos)
