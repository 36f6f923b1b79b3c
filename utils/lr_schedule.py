"""Learning-rate schedules of the training entry points (--lr_schedule, --warmup_steps, --lr_min), computed on the host.

The fused optimizer step takes ``lr`` by value on every launch, so a schedule is nothing but a number written into
``optimizer.param_groups[0]["lr"]`` before the step.  Every value is a pure function of the step index and of the
validation losses handed to ``epoch_end`` -- data-parallel ranks that feed the same (broadcast) losses compute the same values.

  constant   base_lr
  cosine     per optimizer step over the planned total T:  lr_min + (base_lr - lr_min) (1 + cos(pi (s - W) / (T - W))) / 2
             for step index s >= W (s counts from 0, W = warmup_steps); s >= T stays at lr_min
  plateau    torch.optim.lr_scheduler.ReduceLROnPlateau(mode="min", factor=0.5, patience=5) stepped on the epoch's
             validation loss, the scheduler the reference declares (train_DC_focal.py:225) -- with its defaults: relative
             threshold 1e-4, no cooldown, a reduction smaller than 1e-8 is not applied; never below lr_min
All three start with a linear warm-up over the first W steps: the value of step s < W is scaled by (s + 1) / W.
"""
import math

KINDS = ("constant", "cosine", "plateau")


class LRSchedule:
    FACTOR, PATIENCE, THRESHOLD, EPS = 0.5, 5, 1e-4, 1e-8       # ReduceLROnPlateau's

    def __init__(self, kind, base_lr, total_steps=0, warmup_steps=0, lr_min=0.0):
        if kind not in KINDS:
            raise ValueError(f"lr schedule must be one of {', '.join(KINDS)}, not {kind!r}")
        if not base_lr >= 0.0 or not 0.0 <= lr_min <= base_lr:
            raise ValueError(f"need 0 <= lr_min <= lr, not lr {base_lr}, lr_min {lr_min}")
        if warmup_steps < 0:
            raise ValueError(f"warmup_steps must be >= 0, not {warmup_steps}")
        if kind == "cosine" and total_steps <= warmup_steps:
            raise ValueError(f"the cosine schedule needs more planned steps ({total_steps}) than warm-up steps ({warmup_steps})")
        self.kind, self.base_lr, self.total_steps = kind, float(base_lr), int(total_steps)
        self.warmup_steps, self.lr_min = int(warmup_steps), float(lr_min)
        self.plateau_lr, self.best, self.num_bad = float(base_lr), math.inf, 0

    def lr_at(self, step):
        """The learning rate of the optimizer step with index `step` (from 0)."""
        if self.kind == "cosine":
            q = min(max((step - self.warmup_steps) / (self.total_steps - self.warmup_steps), 0.0), 1.0)
            lr = self.lr_min + (self.base_lr - self.lr_min) * 0.5 * (1.0 + math.cos(math.pi * q))
        elif self.kind == "plateau":
            lr = self.plateau_lr
        else:
            lr = self.base_lr
        if step < self.warmup_steps:
            lr *= (step + 1) / self.warmup_steps
        return lr

    def epoch_end(self, val_loss):
        """plateau: one ReduceLROnPlateau.step(val_loss); the other kinds ignore it.  Returns the rate after it."""
        if self.kind != "plateau":
            return None
        val_loss = float(val_loss)
        if val_loss < self.best * (1.0 - self.THRESHOLD):
            self.best, self.num_bad = val_loss, 0
        else:
            self.num_bad += 1
        if self.num_bad > self.PATIENCE:
            new = max(self.plateau_lr * self.FACTOR, self.lr_min)
            if self.plateau_lr - new > self.EPS:
                self.plateau_lr = new
            self.num_bad = 0
        return self.plateau_lr
