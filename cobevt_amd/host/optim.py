"""FusedAdam / FusedAdamW: torch.optim.Adam / AdamW on the package's multi-tensor kernels (ops.multi_adam, csrc/train_glue.hip).

One prepare launch per param group (the step counters and the four per-tensor coefficients) and one update launch per 64 tensors,
instead of the dozen multi-tensor passes of torch's foreach implementation.  The tensors' addresses travel in the kernel arguments,
and everything that changes between steps is read from device memory, so `step()` can be captured into a HIP graph without
`capturable=True` - and, unlike torch's captured step, follows a learning-rate schedule:

  * `param_group["lr"]` stays the user-facing Python float (torch's schedulers and host.lr_scheduler.CosineLRScheduler write it);
  * an eager step passes that float by value;
  * a step issued while the stream is capturing reads the group's device word instead, and `sync_hyperparameters()` uploads every
    group's current float to its word (host.CapturedTrainStep.step calls it before each replay);
  * betas, eps and weight_decay are baked into the graph at capture, as in torch.

State per parameter is torch's: `step` (a 0-dim fp32 device tensor), `exp_avg`, `exp_avg_sq` - a state_dict() loads into
torch.optim.AdamW and a torch checkpoint loads into these classes.  torch.amp.GradScaler hands its scale and found_inf words over
as attributes (`_step_supports_amp_scaling`); the kernels unscale the gradients and skip the whole step on an overflow.

fp32 contiguous parameters only; amsgrad, maximize, differentiable, sparse gradients raise CobevtHipError.
"""
import torch

from .. import ops
from ..lib import CobevtHipError


class _FusedAdamBase(torch.optim.Optimizer):
    _ADAMW = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=None):
        name = type(self).__name__
        if amsgrad or maximize or differentiable:
            raise CobevtHipError("%s: amsgrad, maximize and differentiable are not supported (use torch.optim for them)" % name)
        if decoupled_weight_decay is not None and bool(decoupled_weight_decay) != self._ADAMW:
            raise CobevtHipError("%s: decoupled_weight_decay is fixed by the class (FusedAdamW: True, FusedAdam: False)" % name)
        if torch.is_tensor(lr) and lr.numel() != 1:
            raise CobevtHipError("%s: a tensor lr must have one element" % name)
        if not 0.0 <= float(lr):
            raise CobevtHipError("%s: invalid learning rate %r" % (name, lr))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise CobevtHipError("%s: invalid betas %r" % (name, betas))
        if not 0.0 <= eps or not 0.0 <= weight_decay:
            raise CobevtHipError("%s: eps and weight_decay must be >= 0, got %r, %r" % (name, eps, weight_decay))
        # foreach / fused / capturable choose between torch's implementations; there is one here, and it is capturable as it stands
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=self._ADAMW)
        super().__init__(params, defaults)
        self._step_supports_amp_scaling = True      # torch/amp/grad_scaler.py: step() then finds grad_scale / found_inf as attributes
        self._lr_words = {}         # index of the param group -> its fp64 device word
        self._coef = {}             # index of the param group -> fp32 (params of the group, 4) device scratch

    # ------------------------------------------------------------------------------------------------------------------
    def _group_buffers(self, gi, group, device, capturing):
        word = self._lr_words.get(gi)
        if capturing and (word is None or word.device != device or gi not in self._coef
                          or self._coef[gi].shape[0] < len(group["params"])):
            # created inside the capture, the word's first fill would be a node of the graph and undo every later upload
            raise CobevtHipError("%s: take one eager step before capturing step() - the optimizer state, the coefficient scratch and "
                                 "the learning-rate word must exist before the capture" % type(self).__name__)
        if word is None or word.device != device:
            word = self._lr_words[gi] = torch.full((), float(group["lr"]), dtype=torch.float64, device=device)
        coef = self._coef.get(gi)
        if coef is None or coef.device != device or coef.shape[0] < len(group["params"]):
            coef = self._coef[gi] = torch.zeros((len(group["params"]), 4), dtype=torch.float32, device=device)
        return word, coef

    def lr_words(self):
        """the groups' device learning-rate words (fp64), in group order; a group that has not stepped yet has none (None)"""
        return [self._lr_words.get(gi) for gi in range(len(self.param_groups))]

    def sync_hyperparameters(self):
        """Upload every group's current `lr` to its device word: call it before replaying a captured step.  (A fill launch with the
        value in its arguments: no host -> device copy, no synchronisation.)"""
        for gi, group in enumerate(self.param_groups):
            word = self._lr_words.get(gi)
            if word is None:
                continue
            lr = group["lr"]
            if torch.is_tensor(lr):
                word.copy_(lr.reshape(()), non_blocking=True)
            else:
                word.fill_(float(lr))

    def _init_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        elif not torch.is_tensor(st["step"]) or st["step"].device != p.device or st["step"].dtype != torch.float32:
            # a checkpoint of a non-capturable torch optimizer keeps `step` as a CPU tensor (or a number)
            st["step"] = torch.as_tensor(float(st["step"]), dtype=torch.float32).to(p.device)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale = getattr(self, "grad_scale", None)
        found_inf = getattr(self, "found_inf", None)
        name = type(self).__name__
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize") or group.get("differentiable"):
                raise CobevtHipError("%s: amsgrad, maximize and differentiable are not supported" % name)
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            for p in params:
                if p.grad.is_sparse:
                    raise CobevtHipError("%s does not support sparse gradients" % name)
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise CobevtHipError("%s: parameters must be contiguous fp32 tensors, got %s with strides %s"
                                         % (name, p.dtype, p.stride()))
            device = params[0].device
            capturing = device.type == "cuda" and torch.cuda.is_current_stream_capturing()
            if capturing and any(len(self.state[p]) == 0 for p in params):
                self._group_buffers(-1, group, device, True)         # (raises: zero fills inside the graph would reset the state on every replay)
            states = [self._init_state(p) for p in params]
            word, coef = self._group_buffers(gi, group, device, capturing)
            lr = group["lr"]
            if torch.is_tensor(lr) and not capturing:
                lr = float(lr)
            beta1, beta2 = group["betas"]
            ops.multi_adam(params, [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in params],
                           [s["exp_avg"] for s in states], [s["exp_avg_sq"] for s in states], [s["step"] for s in states], coef,
                           lr=0.0 if capturing else lr, beta1=beta1, beta2=beta2, eps=group["eps"], weight_decay=group["weight_decay"],
                           adamw=self._ADAMW, lr_dev=word if capturing else None,
                           grad_scale=None if grad_scale is None else grad_scale.to(device).reshape(()),
                           found_inf=None if found_inf is None else found_inf.to(device).reshape(()))
        return loss


class FusedAdamW(_FusedAdamBase):
    """torch.optim.AdamW (decoupled weight decay) on ops.multi_adam."""
    _ADAMW = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, **kwargs):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kwargs)


class FusedAdam(_FusedAdamBase):
    """torch.optim.Adam (weight decay as an L2 term of the gradient) on ops.multi_adam."""
    _ADAMW = False
