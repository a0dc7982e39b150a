"""CosineLRScheduler: the `cosineannealwarm` schedule of the reference's yaml files (train_utils.py:239-255 builds timm's
CosineLRScheduler with t_initial, lr_min, warmup_lr_init, warmup_t, cycle_limit=1, t_in_epochs=False and train_camera.py calls
`scheduler.step_update(epoch * n_iter_per_epoch + i)` after every iteration and `scheduler.step(epoch)` after every epoch).

timm is a third-party package that is not a dependency here; this file restates its published scheduler for exactly those arguments
(one cycle, no cycle decay, no noise, warm-up without a prefix shift).  Parity with timm itself is unpinned: no test compares the
two.
"""
import math


class CosineLRScheduler(object):
    def __init__(self, optimizer, t_initial, lr_min=0.0, warmup_t=0, warmup_lr_init=0.0, cycle_limit=1, t_in_epochs=True):
        if t_initial < 1 or warmup_t < 0:
            raise ValueError("CosineLRScheduler: t_initial >= 1 and warmup_t >= 0, got %r, %r" % (t_initial, warmup_t))
        if cycle_limit != 1:
            raise ValueError("CosineLRScheduler: only cycle_limit=1 (the reference's setting) is restated here")
        self.optimizer = optimizer
        self.t_initial, self.lr_min, self.warmup_t, self.warmup_lr_init = t_initial, lr_min, warmup_t, warmup_lr_init
        self.t_in_epochs = t_in_epochs
        for group in optimizer.param_groups:
            group.setdefault("initial_lr", group["lr"])
        self.base_values = [float(group["initial_lr"]) for group in optimizer.param_groups]
        self.warmup_steps = [(v - warmup_lr_init) / warmup_t for v in self.base_values] if warmup_t else [1.0] * len(self.base_values)
        if warmup_t:
            self._set([warmup_lr_init] * len(self.base_values))

    def _get_lr(self, t):
        if t < self.warmup_t:
            return [self.warmup_lr_init + t * s for s in self.warmup_steps]
        if t < self.t_initial:
            return [self.lr_min + 0.5 * (v - self.lr_min) * (1.0 + math.cos(math.pi * t / self.t_initial)) for v in self.base_values]
        return [self.lr_min] * len(self.base_values)

    def _set(self, values):
        for group, v in zip(self.optimizer.param_groups, values):
            group["lr"] = v

    def step(self, epoch, metric=None):
        """per-epoch hook: inert with t_in_epochs=False (the reference's setting)"""
        if self.t_in_epochs:
            self._set(self._get_lr(epoch))

    def step_update(self, num_updates, metric=None):
        """per-iteration hook: sets every group's lr for update number `num_updates`"""
        if not self.t_in_epochs:
            self._set(self._get_lr(num_updates))

    def state_dict(self):
        return {k: v for k, v in self.__dict__.items() if k != "optimizer"}

    def load_state_dict(self, state_dict):
        self.__dict__.update(state_dict)
