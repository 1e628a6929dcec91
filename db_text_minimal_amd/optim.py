"""Fused flat Adam — the optimizer of /root/reference/src/train.py:114-117
(`torch.optim.Adam(lr=.005, betas=(.9,.999), eps=1e-8, weight_decay=0,
amsgrad=False)`) as ONE HIP launch over the model's flat parameter buffer
(dbn_adam_step: reads p,g,m,v, writes p,m,v = 28 B/param).

It subclasses `torch.optim.Optimizer` only for interface compatibility (so the
reference's `ReduceLROnPlateau` / `WarmupPolyLR` schedulers, train.py:119-139, accept it and drive
`param_groups[0]['lr']`); no torch optimizer arithmetic is used.

Three options beyond the reference configuration, all on the device and all off by default (`FusedAdam(model)` launches
adam_kernel through dbn_adam_step exactly as before; csrc/optim.hip):

  amsgrad=True            the reference driver's `cfg.optimizer.amsgrad`: a third moment buffer `max_exp_avg_sq`, the running maximum
                          of exp_avg_sq, under the square root (dbn_adam_step_ex, 36 B/param).
  max_grad_norm=c         torch.nn.utils.clip_grad_norm_(parameters, c) over the whole flat gradient: the squared norm is summed in
                          float64 by dbn_grad_sqnorm (4 B/param, the same bits on every run), stays in device memory, and every thread
                          of the Adam launch forms min(1, c / (norm + 1e-6)) from it — no host synchronisation.  `last_grad_norm` is
                          the pre-clip norm as a 0-dim device tensor, for logging.  A non-finite norm behaves as torch with
                          error_if_nonfinite=False: the coefficient is NaN and propagates (no step is skipped: the host owns the
                          step count).
  accumulation_steps=k    one update from the SUM of k backward passes: after each pass `accumulate()` folds the engine's flat
                          gradient into an fp32 accumulator (dbn_grad_accumulate, in pass order), and `step()` consumes the
                          accumulator once exactly k passes are folded — any other count raises, nothing is dropped silently.
                          DBTrainer drives this (train.py) and passes grad_scale = 1 / (world k), the mean over ranks and passes.

`weight_decay` stays refused by the constructor: dbn_adam_step_ex takes it (torch's L2 form, g + weight_decay p after the clip, tested
against float64), but an existing test pins the constructor's NotImplementedError, so exposing it is left to a later change.
"""
import torch

from . import _lib
from ._lib import check

# the hyper-parameters a checkpoint written before these options existed does not hold, and what it was trained with
NEW_HYPER_DEFAULTS = {'amsgrad': False, 'max_grad_norm': None, 'accumulation_steps': 1}


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, model, lr=0.005, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, max_grad_norm=None,
                 accumulation_steps=1):
        if weight_decay != 0:
            raise NotImplementedError('weight_decay=0 only (the reference configuration, example_config.yaml:68-77): the C entry point '
                                      'dbn_adam_step_ex takes a weight decay, but tests/test_host_cpu.py pins this refusal')
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError('max_grad_norm must be positive or None, got %r' % (max_grad_norm, ))
        if int(accumulation_steps) != accumulation_steps or accumulation_steps < 1:
            raise ValueError('accumulation_steps must be a positive integer, got %r' % (accumulation_steps, ))
        self.model = model
        self.engine = model.engine
        params = [p for _, p in self.engine.live_params]
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=bool(amsgrad),
                                      max_grad_norm=None if max_grad_norm is None else float(max_grad_norm),
                                      accumulation_steps=int(accumulation_steps)))
        self.step_count = 0
        self.exp_avg = None
        self.exp_avg_sq = None
        self.max_exp_avg_sq = None  # amsgrad only
        self.grad_acc = None        # accumulation_steps > 1 only: the sum of the folded passes
        self.folded = 0             # passes folded into grad_acc since the last update
        self._sqnorm = None         # max_grad_norm only: the squared norm (one double) and the partial sums behind it
        self._sqnorm_ws = None
        self._norm_scale = None

    # the options live in param_groups[0], so that state_dict() carries them and load_state_dict() restores them
    @property
    def amsgrad(self):
        return bool(self.param_groups[0]['amsgrad'])

    @property
    def max_grad_norm(self):
        return self.param_groups[0]['max_grad_norm']

    @property
    def accumulation_steps(self):
        return int(self.param_groups[0]['accumulation_steps'])

    @property
    def last_grad_norm(self):
        """The gradient norm of the last step() BEFORE clipping (what clip_grad_norm_ returns), as a 0-dim float64 device tensor:
        reading it enqueues two tiny operations and never waits for the device.  None when clipping is off or no step has run."""
        if self.max_grad_norm is None or self._norm_scale is None:
            return None
        return self._sqnorm[0].sqrt() * self._norm_scale

    def zero_grad(self, set_to_none=True):
        """Every backward pass OVERWRITES the engine's flat gradient buffer completely, so there is nothing to clear there —
        and no accumulation either: `step()` consumes the gradients of ONE backward pass.  Gradient accumulation (a second
        backward pass without a zero_grad() / step() in between, which torch.optim.Adam would sum) is refused by step() with a
        RuntimeError instead of silently dropping the first pass; use torch.optim.Adam over `model.parameters()` for that.
        On the autograd surface the parameters' `.grad` views are dropped here so they do not keep accumulating across
        iterations.
        With accumulation_steps > 1 the passes are summed by accumulate(); zero_grad() leaves that accumulator alone (it is called
        before every backward pass of a cycle) — discard_accumulated() drops it."""
        for _, p in self.engine.live_params:
            p.grad = None
        self.engine.backwards_since_clear = 0
        return None

    def _ensure_state(self):
        eng = self.engine
        eng.ensure_flat()
        if self.exp_avg is None or self.exp_avg.shape != eng.flat.shape or self.exp_avg.device != eng.flat.device:
            self.exp_avg = torch.zeros_like(eng.flat)
            self.exp_avg_sq = torch.zeros_like(eng.flat)
            self.max_exp_avg_sq = self.grad_acc = self._sqnorm = None
            self.folded = 0
        if self.amsgrad and self.max_exp_avg_sq is None:
            self.max_exp_avg_sq = torch.zeros_like(eng.flat)
        if self.accumulation_steps > 1 and self.grad_acc is None:
            self.grad_acc = torch.zeros_like(eng.flat)
            self.folded = 0
        if self.max_grad_norm is not None and self._sqnorm is None:
            self._sqnorm = torch.zeros(1, device=eng.flat.device, dtype=torch.float64)
            self._sqnorm_ws = torch.empty(_lib.lib().dbn_grad_sqnorm_ws_doubles(eng.flat.numel()), device=eng.flat.device,
                                          dtype=torch.float64)
            self._norm_scale = None

    @torch.no_grad()
    def accumulate(self):
        """accumulation_steps > 1: fold the engine's flat gradient (ONE backward pass) into the accumulator on the engine's stream —
        the first fold of a cycle copies, the later ones add in fp32, in pass order."""
        k = self.accumulation_steps
        if k <= 1:
            raise RuntimeError('FusedAdam.accumulate() needs accumulation_steps > 1 (it is %d)' % k)
        self._ensure_state()
        eng = self.engine
        if eng.backwards_since_clear != 1:
            raise RuntimeError('FusedAdam.accumulate(): %d backward passes ran since the last zero_grad()/accumulate(); the flat '
                               'gradient buffer holds exactly one pass, and each pass is folded once' % eng.backwards_since_clear)
        check(_lib.lib().dbn_grad_accumulate(self.grad_acc.data_ptr(), eng.flat_grad.data_ptr(), eng.flat.numel(),
                                             1 if self.folded == 0 else 0, eng.stream), 'grad_accumulate')
        self.folded += 1
        eng.backwards_since_clear = 0

    def discard_accumulated(self):
        """Drop the passes folded so far (after a refused step(), or to abandon a cycle)."""
        self.folded = 0

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        """Consumes the engine's flat gradient buffer (filled by DBTrainer / engine.backward) — with accumulation_steps = k > 1 the
        accumulator of exactly k accumulate() calls instead."""
        if closure is not None:
            raise NotImplementedError('closures are not supported')
        self._ensure_state()
        eng = self.engine
        k = self.accumulation_steps
        if k > 1:
            if self.folded != k or eng.backwards_since_clear != 0:
                raise RuntimeError('FusedAdam.step(): %d of accumulation_steps=%d backward passes are folded into the accumulator and %d '
                                   'ran without accumulate(); an update takes exactly %d folded passes (nothing is dropped or applied '
                                   'early — discard_accumulated() abandons the cycle)' % (self.folded, k, eng.backwards_since_clear, k))
            grad = self.grad_acc
        else:
            if eng.backwards_since_clear > 1:
                raise RuntimeError('FusedAdam.step(): %d backward passes ran since the last zero_grad()/step(); the flat gradient buffer '
                                   'holds only the last one (no gradient accumulation on the fused path — use torch.optim.Adam over '
                                   'model.parameters())' % eng.backwards_since_clear)
            grad = eng.flat_grad
        eng.backwards_since_clear = 0
        self.folded = 0
        g = self.param_groups[0]
        self.step_count += 1
        L, n = _lib.lib(), eng.flat.numel()
        clip = self.max_grad_norm
        if not self.amsgrad and clip is None:  # the plain step, as ever
            check(L.dbn_adam_step(eng.flat.data_ptr(), grad.data_ptr(), self.exp_avg.data_ptr(),
                                  self.exp_avg_sq.data_ptr(), n, float(g['lr']), float(g['betas'][0]),
                                  float(g['betas'][1]), float(g['eps']), self.step_count, float(grad_scale), eng.stream),
                  'adam_step')
        else:
            if clip is not None:
                check(L.dbn_grad_sqnorm(grad.data_ptr(), n, self._sqnorm_ws.data_ptr(), self._sqnorm.data_ptr(), eng.stream), 'grad_sqnorm')
                self._norm_scale = abs(float(grad_scale))
            check(L.dbn_adam_step_ex(eng.flat.data_ptr(), grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                     self.max_exp_avg_sq.data_ptr() if self.amsgrad else None, n, float(g['lr']), float(g['betas'][0]),
                                     float(g['betas'][1]), float(g['eps']), 0.0, self.step_count, float(grad_scale),
                                     None if clip is None else self._sqnorm.data_ptr(), 0.0 if clip is None else float(clip), eng.stream),
                  'adam_step_ex')
        eng.mark_params_dirty()

    def state_dict(self):
        """`max_exp_avg_sq` is None without amsgrad; the three options travel in param_groups.  The gradient accumulator is NOT part of
        the state: a checkpoint is taken between updates (after the step() that ends a cycle), never inside one."""
        if self.engine.flat is not None or any(p.is_cuda for _, p in self.engine.live_params):
            self._ensure_state()  # moments exist (zeros) before the first step, so a fresh optimizer round-trips
        return {'step': self.step_count, 'exp_avg': self.exp_avg, 'exp_avg_sq': self.exp_avg_sq,
                'max_exp_avg_sq': self.max_exp_avg_sq if self.amsgrad else None,
                'param_groups': [{k: v for k, v in self.param_groups[0].items() if k != 'params'}]}

    def load_state_dict(self, sd):
        """A checkpoint written before the options existed loads: the hyper-parameters it lacks take their defaults (what it was trained
        with: no amsgrad, no clipping, no accumulation), a missing `max_exp_avg_sq` starts from zeros.  Passes folded so far are
        discarded (see state_dict())."""
        group = dict(NEW_HYPER_DEFAULTS)
        group.update(sd['param_groups'][0])
        self.param_groups[0].update(group)
        self._ensure_state()
        self.step_count = int(sd['step'])
        self.folded = 0
        for name in ('exp_avg', 'exp_avg_sq') + (('max_exp_avg_sq', ) if self.amsgrad else ()):
            if sd.get(name) is None:  # saved before any state existed
                getattr(self, name).zero_()
            else:
                getattr(self, name).copy_(sd[name])
