"""Learning-rate schedules for fit(lrs_mode='poly'): stepped once per update, they drive every parameter group's `lr`."""
import torch


class WarmupPolyLR(torch.optim.lr_scheduler.LRScheduler):
    """Warm-up followed by polynomial decay towards `target_lr`, the schedule of the DB paper's recipe.  At iteration t (the number of
    step() calls so far), for every group with base rate b:

        lr = target_lr + (b - target_lr) f(t)
        t <  warmup_iters:  f = warmup_factor                          ('constant')
                            f = warmup_factor (1 - a) + a,  a = t / warmup_iters     ('linear': from warmup_factor up to 1)
        t >= warmup_iters:  f = (1 - T / N)^power,   T = t - warmup_iters,  N = max_iters - warmup_iters

    `max_iters` defaults to 0, and the reference driver passes `warmup_iters` only.  It therefore trains with N = -warmup_iters:
    past the warm-up the factor is (1 + T / warmup_iters)^0.9 and the rate RISES without bound (twice the base rate at
    t = 2.16 warmup_iters).  That is reproduced here value for value, because it is what the reference's results were obtained with;
    pass the true `max_iters` for the schedule the paper describes, which reaches target_lr at t = max_iters.  Beyond max_iters the
    base 1 - T / N is negative and its fractional power is no real number: the factor stays 0 there (lr = target_lr)."""

    def __init__(self, optimizer, target_lr=0, max_iters=0, power=0.9, warmup_factor=1.0 / 3, warmup_iters=500, warmup_method='linear',
                 last_epoch=-1):
        if warmup_method not in ('constant', 'linear'):
            raise ValueError("warmup_method must be 'constant' or 'linear', got %r" % (warmup_method, ))
        if max_iters == warmup_iters:
            raise ValueError('max_iters == warmup_iters leaves no iterations to decay over')
        self.target_lr, self.max_iters, self.power = target_lr, max_iters, power
        self.warmup_factor, self.warmup_iters, self.warmup_method = warmup_factor, warmup_iters, warmup_method
        super().__init__(optimizer, last_epoch)

    def factor(self, t):
        if t < self.warmup_iters:
            if self.warmup_method == 'constant':
                return self.warmup_factor
            a = float(t) / self.warmup_iters
            return self.warmup_factor * (1 - a) + a
        base = 1 - (t - self.warmup_iters) / (self.max_iters - self.warmup_iters)
        return base**self.power if base > 0 else 0.0

    def get_lr(self):
        f = self.factor(self.last_epoch)
        return [self.target_lr + (b - self.target_lr) * f for b in self.base_lrs]
