"""Training-loop helpers - mirrors of opv2v/opencood/tools/train_utils.py: `setup_optimizer` (:174-199), `setup_lr_schedular` (:202-260,
the reference's spelling) and `to_device` (:263-272) with the reference's signatures and yaml keys, and checkpoint loading — mirror of opv2v/opencood/tools/train_utils.py:24-65 (`load_saved_model`): the newest
`net_epoch<N>.pth` of a run directory is a plain state_dict with the reference's key names, which the HIP modules accept
unchanged (tests/golden/gv0_state_dict_schema.npz pins the key / shape schema)."""
import glob
import os
import re

import torch

from .lr_scheduler import CosineLRScheduler
from .optim import FusedAdam, FusedAdamW


def find_last_checkpoint(save_dir):
    """highest N among <save_dir>/*epoch<N>.pth, 0 when there is none (:42-52)"""
    best = 0
    for path in glob.glob(os.path.join(save_dir, "*epoch*.pth")):
        found = re.findall(".*epoch(.*).pth.*", path)
        best = max(best, int(found[0]))
    return best


def load_saved_model(saved_path, model):
    """-> (epoch, model); non-strict load as in the reference (:54-63), on the CPU first; cached kernel plans of the
    model are rebuilt on the next forward because the parameters' versions change."""
    assert os.path.exists(saved_path), "{} not found".format(saved_path)
    initial_epoch = find_last_checkpoint(saved_path)
    if initial_epoch > 0:
        print("resuming by loading epoch %d" % initial_epoch)
        checkpoint = torch.load(os.path.join(saved_path, "net_epoch%d.pth" % initial_epoch), map_location="cpu")
        model.load_state_dict(checkpoint, strict=False)
        del checkpoint
    return initial_epoch, model


_FUSED = {"AdamW": FusedAdamW, "Adam": FusedAdam}
_FUSED_ARGS = ("betas", "eps", "weight_decay")         # with anything else in `args` the torch class is built, as in the reference


def setup_optimizer(hypes, model):
    """hypes['optimizer'] = {core_method, lr, args (optional)} -> the optimizer over the model's trainable parameters (:174-199).
    AdamW / Adam on a ROCm model with fp32 parameters and no arguments beyond betas / eps / weight_decay are the package's
    FusedAdamW / FusedAdam; every other name of torch.optim (and every other argument) builds torch's class as the reference does."""
    method_dict = hypes["optimizer"]
    name = method_dict["core_method"]
    optimizer_method = getattr(torch.optim, name, None)
    if not optimizer_method:
        raise ValueError("{} is not supported".format(name))
    params = [p for p in model.parameters() if p.requires_grad]
    args = dict(method_dict.get("args") or {})
    if name in _FUSED and all(k in _FUSED_ARGS for k in args) and params \
            and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in params):
        optimizer_method = _FUSED[name]
    return optimizer_method(params, lr=method_dict["lr"], **args)


def setup_lr_schedular(hypes, optimizer, n_iter_per_epoch):
    """hypes['lr_scheduler'] -> the scheduler (:202-260): 'step', 'multistep' and 'exponential' are torch's classes, stepped once an
    epoch; 'cosineannealwarm' is host.lr_scheduler.CosineLRScheduler, whose step_update(iteration) runs after every step."""
    config = hypes["lr_scheduler"]
    method = config["core_method"]
    if method == "step":
        return torch.optim.lr_scheduler.StepLR(optimizer, step_size=config["step_size"], gamma=config["gamma"])
    if method == "multistep":
        return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=config["step_size"], gamma=config["gamma"])
    if method == "exponential":
        return torch.optim.lr_scheduler.ExponentialLR(optimizer, config["gamma"])
    if method == "cosineannealwarm":
        return CosineLRScheduler(optimizer, t_initial=config["epoches"] * n_iter_per_epoch, lr_min=config["lr_min"],
                                 warmup_lr_init=config["warmup_lr"], warmup_t=config["warmup_epoches"] * n_iter_per_epoch,
                                 cycle_limit=1, t_in_epochs=False)
    raise ValueError("Unidentified scheduler {!r}".format(method))


def to_device(inputs, device):
    """lists and dicts entry by entry, numbers and strings as they are, everything else .to(device) (:263-272)"""
    if isinstance(inputs, list):
        return [to_device(x, device) for x in inputs]
    if isinstance(inputs, dict):
        return {k: to_device(v, device) for k, v in inputs.items()}
    if isinstance(inputs, (int, float, str)):
        return inputs
    return inputs.to(device)
