"""idg_adam_step_f32: the dense Adam step and the optimizer around it."""
import torch

from ..native import check, lib
from ._base import _ptr, _require_device, _stream


def adam_step_raw(param, grad, exp_avg, exp_avg_sq, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    _require_device(param, grad, exp_avg, exp_avg_sq)
    for t in (param, grad, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("adam_step_raw needs contiguous float32 tensors")
    check(lib.idg_adam_step_f32(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), float(lr),
                                float(beta1), float(beta2), float(eps), int(step), _stream()), "idg_adam_step_f32")


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's default algorithm (utility/utility_train/trainer.py:11) as one HIP
    kernel per parameter tensor.  Same constructor signature for the arguments the reference
    uses; weight decay / amsgrad are not part of the reference path and are rejected."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if weight_decay != 0 or amsgrad:
            raise NotImplementedError("idgrec_amd.Adam implements the reference's plain Adam only")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                adam_step_raw(p.data, g, st["exp_avg"], st["exp_avg_sq"], group["lr"], st["step"], b1, b2, group["eps"])
        return loss
