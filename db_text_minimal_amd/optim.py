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

`weight_decay` stays refused by FusedAdam's constructor (existing tests pin the NotImplementedError): weight decay, coupled as in
torch.optim.Adam(weight_decay) or decoupled as in torch.optim.AdamW, is `FusedAdamW` below.

The optimizer family (csrc/optim_groups.hip) stands on FlatOptimizer, which holds what DBTrainer uses of any of
them (step(grad_scale=), zero_grad, accumulate, discard_accumulated, accumulation_steps, folded, grad_acc, last_grad_norm):

  FusedSGD     torch.optim.SGD with clip_grad_norm_ in front: momentum, dampening, nesterov, L2 weight decay (dbn_sgd_step: 12 B/param
               without momentum, 20 with)
  FusedAdamW   Adam with weight decay, decoupled (torch.optim.AdamW, the default) or coupled (torch.optim.Adam(weight_decay), what the
               reference driver constructs), AMSGrad optional (dbn_adamw_step: 28 / 36 B/param)

Both take `param_groups` (torch-style dicts over the model's live parameters that may set `lr` and `weight_decay`; at most 8 groups,
the remainder included; split_decay() builds the usual two) and `ema_decay` (an exponential moving average of the weights written by the
update's own launch, +8 B/param: ema_weights(), ema_state_dict()).  The groups reach the kernel as a table of runs of quads
(build_runs), uploaded once; their learning rates and decays travel in the kernel arguments, so a scheduler drives every group's `lr`
without an upload.
"""
import contextlib
import ctypes

import torch

from . import _lib
from ._lib import check

# the hyper-parameters a checkpoint written before these options existed does not hold, and what it was trained with
NEW_HYPER_DEFAULTS = {'amsgrad': False, 'max_grad_norm': None, 'accumulation_steps': 1}

MAX_GROUPS = 8   # dbn_optim_max_groups(): the per-group coefficients travel in the kernel arguments
MAX_RUNS = 1024  # dbn_optim_max_runs(): the run table is staged in LDS


def _check_common_options(max_grad_norm, accumulation_steps):
    if max_grad_norm is not None and not float(max_grad_norm) > 0:
        raise ValueError('max_grad_norm must be positive or None, got %r' % (max_grad_norm, ))
    if int(accumulation_steps) != accumulation_steps or accumulation_steps < 1:
        raise ValueError('accumulation_steps must be a positive integer, got %r' % (accumulation_steps, ))


class FlatOptimizer(torch.optim.Optimizer):
    """What every optimizer over the engine's flat buffers shares: the bookkeeping of backward passes (one pass per update, or exactly
    accumulation_steps folded ones), the fold, the norm behind max_grad_norm.  The subclasses own their state and their launch."""
    TORCH_EQUIVALENT = 'torch.optim.Adam'  # named by the refusal of a second backward pass

    def __init__(self, model, params, defaults):
        self.model = model
        self.engine = model.engine
        super().__init__(params, defaults)
        self.step_count = 0
        self.grad_acc = None        # accumulation_steps > 1 only: the sum of the folded passes
        self.folded = 0             # passes folded into grad_acc since the last update
        self._sqnorm = None         # max_grad_norm only: the squared norm (one double) and the partial sums behind it
        self._sqnorm_ws = None
        self._norm_scale = None

    # the options live in param_groups[0], so that state_dict() carries them and load_state_dict() restores them
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

    def _ensure_workspaces(self):
        """the accumulator and the norm's workspace, for the options that need them (the flat buffers exist)"""
        eng = self.engine
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
        k, me = self.accumulation_steps, type(self).__name__
        if k <= 1:
            raise RuntimeError('%s.accumulate() needs accumulation_steps > 1 (it is %d)' % (me, k))
        self._ensure_state()
        eng = self.engine
        if eng.backwards_since_clear != 1:
            raise RuntimeError('%s.accumulate(): %d backward passes ran since the last zero_grad()/accumulate(); the flat '
                               'gradient buffer holds exactly one pass, and each pass is folded once' % (me, eng.backwards_since_clear))
        check(_lib.lib().dbn_grad_accumulate(self.grad_acc.data_ptr(), eng.flat_grad.data_ptr(), eng.flat.numel(),
                                             1 if self.folded == 0 else 0, eng.stream), 'grad_accumulate')
        self.folded += 1
        eng.backwards_since_clear = 0

    def discard_accumulated(self):
        """Drop the passes folded so far (after a refused step(), or to abandon a cycle)."""
        self.folded = 0

    def _take_gradient(self, closure):
        """The head of every step(): the refusals, then the buffer this update consumes (the flat gradient of one pass, or the
        accumulator of exactly accumulation_steps folds); the pass counters start over and step_count advances."""
        if closure is not None:
            raise NotImplementedError('closures are not supported')
        self._ensure_state()
        eng, me = self.engine, type(self).__name__
        k = self.accumulation_steps
        if k > 1:
            if self.folded != k or eng.backwards_since_clear != 0:
                raise RuntimeError('%s.step(): %d of accumulation_steps=%d backward passes are folded into the accumulator and %d '
                                   'ran without accumulate(); an update takes exactly %d folded passes (nothing is dropped or applied '
                                   'early — discard_accumulated() abandons the cycle)' % (me, self.folded, k, eng.backwards_since_clear, k))
            grad = self.grad_acc
        else:
            if eng.backwards_since_clear > 1:
                raise RuntimeError('%s.step(): %d backward passes ran since the last zero_grad()/step(); the flat gradient buffer '
                                   'holds only the last one (no gradient accumulation on the fused path — use %s over '
                                   'model.parameters())' % (me, eng.backwards_since_clear, self.TORCH_EQUIVALENT))
            grad = eng.flat_grad
        eng.backwards_since_clear = 0
        self.folded = 0
        self.step_count += 1
        return grad

    def _clip_args(self, grad, grad_scale):
        """max_grad_norm: launch the norm of `grad`; returns the (sqnorm pointer, max_norm) pair of the step entry points"""
        clip = self.max_grad_norm
        if clip is None:
            return None, 0.0
        eng = self.engine
        check(_lib.lib().dbn_grad_sqnorm(grad.data_ptr(), eng.flat.numel(), self._sqnorm_ws.data_ptr(), self._sqnorm.data_ptr(), eng.stream),
              'grad_sqnorm')
        self._norm_scale = abs(float(grad_scale))
        return self._sqnorm.data_ptr(), float(clip)

    def state_tensors(self):
        """the state buffers a data-parallel start broadcasts from rank 0, in a fixed order"""
        raise NotImplementedError


class FusedAdam(FlatOptimizer):
    def __init__(self, model, lr=0.005, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, max_grad_norm=None,
                 accumulation_steps=1):
        if weight_decay != 0:
            raise NotImplementedError('weight_decay=0 only (the reference configuration, example_config.yaml:68-77): the C entry point '
                                      'dbn_adam_step_ex takes a weight decay, but tests/test_host_cpu.py pins this refusal')
        _check_common_options(max_grad_norm, accumulation_steps)
        params = [p for _, p in model.engine.live_params]
        super().__init__(model, params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=bool(amsgrad),
                                             max_grad_norm=None if max_grad_norm is None else float(max_grad_norm),
                                             accumulation_steps=int(accumulation_steps)))
        self.exp_avg = None
        self.exp_avg_sq = None
        self.max_exp_avg_sq = None  # amsgrad only

    @property
    def amsgrad(self):
        return bool(self.param_groups[0]['amsgrad'])

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
        self._ensure_workspaces()

    def state_tensors(self):
        return [t for t in (self.exp_avg, self.exp_avg_sq, self.max_exp_avg_sq) if t is not None]

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        """Consumes the engine's flat gradient buffer (filled by DBTrainer / engine.backward) — with accumulation_steps = k > 1 the
        accumulator of exactly k accumulate() calls instead."""
        grad = self._take_gradient(closure)
        eng = self.engine
        g = self.param_groups[0]
        L, n = _lib.lib(), eng.flat.numel()
        if not self.amsgrad and self.max_grad_norm is None:  # the plain step, as ever
            check(L.dbn_adam_step(eng.flat.data_ptr(), grad.data_ptr(), self.exp_avg.data_ptr(),
                                  self.exp_avg_sq.data_ptr(), n, float(g['lr']), float(g['betas'][0]),
                                  float(g['betas'][1]), float(g['eps']), self.step_count, float(grad_scale), eng.stream),
                  'adam_step')
        else:
            sqnorm, clip = self._clip_args(grad, grad_scale)
            check(L.dbn_adam_step_ex(eng.flat.data_ptr(), grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                     self.max_exp_avg_sq.data_ptr() if self.amsgrad else None, n, float(g['lr']), float(g['betas'][0]),
                                     float(g['betas'][1]), float(g['eps']), 0.0, self.step_count, float(grad_scale), sqnorm, clip,
                                     eng.stream), 'adam_step_ex')
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


# ----------------------------------------------------------------------------------------------------------------------------------
# parameter groups
# ----------------------------------------------------------------------------------------------------------------------------------
def build_runs(offsets, numels, groups):
    """The run table of a group assignment (pure host function).  offsets / numels: the parameters as flat_layout (engine.py) places
    them, every offset a multiple of 4, so parameter i owns the quads [offsets[i] / 4, offsets[i] / 4 + ceil(numels[i] / 4)): its padding
    stays with it.  groups[i]: its group.  Returns (run_end, run_group): run r covers the quads [run_end[r - 1], run_end[r]) and belongs
    to run_group[r]; adjacent parameters of one group merge into one run."""
    if not (len(offsets) == len(numels) == len(groups)):
        raise ValueError('offsets, numels and groups differ in length')
    run_end, run_group, at = [], [], 0
    for off, n, g in zip(offsets, numels, groups):
        if off % 4 or off != 4 * at:
            raise ValueError('the parameters are not packed as flat_layout packs them (offset %d after quad %d)' % (off, at))
        if n == 0:
            continue
        at += (n + 3) // 4
        if run_group and run_group[-1] == g:
            run_end[-1] = at
        else:
            run_end.append(at)
            run_group.append(g)
    return run_end, run_group


def split_decay(model, weight_decay):
    """Two group dicts for `param_groups`: tensors with ndim >= 2 (convolution and transposed-convolution weights) take `weight_decay`,
    everything else (BatchNorm weights and biases, biases) takes 0."""
    live = [p for _, p in model.engine.live_params]
    return [{'params': [p for p in live if p.ndim >= 2], 'weight_decay': weight_decay},
            {'params': [p for p in live if p.ndim < 2], 'weight_decay': 0.0}]


def _group_dicts(live, param_groups, defaults):
    """The torch param_groups of a grouped optimizer: the user's dicts, then the live parameters nobody listed with the constructor's
    values.  Raises ValueError for what the kernel cannot honour."""
    if param_groups is None:
        return [{'params': list(live)}]
    ids = {id(p) for p in live}
    seen, out = set(), []
    for gi, group in enumerate(param_groups):
        if not isinstance(group, dict) or 'params' not in group:
            raise ValueError("param_groups[%d] is not a dict with 'params'" % gi)
        params = group['params']
        params = [params] if torch.is_tensor(params) else list(params)
        for p in params:
            if not torch.is_tensor(p) or id(p) not in ids:
                raise ValueError('param_groups[%d] holds a tensor that is not a live parameter of the model' % gi)
            if id(p) in seen:
                raise ValueError('param_groups[%d] lists a parameter a second time' % gi)
            seen.add(id(p))
        for key, value in group.items():
            if key not in ('params', 'lr', 'weight_decay') and (key not in defaults or value != defaults[key]):
                raise ValueError('param_groups[%d] sets %r: a group may differ from the optimizer in lr and weight_decay only' % (gi, key))
        if params:
            out.append(dict(group, params=params))
    rest = [p for p in live if id(p) not in seen]
    if rest:
        out.append({'params': rest})
    if len(out) > MAX_GROUPS:
        raise ValueError('%d parameter groups (the unlisted parameters included): at most %d' % (len(out), MAX_GROUPS))
    return out


def _floats(values):
    return (ctypes.c_float * len(values))(*values)


class GroupedFlatOptimizer(FlatOptimizer):
    """FusedSGD and FusedAdamW: parameter groups, the weight EMA and the state dictionary.  A subclass names its state buffers in
    STATE (attribute names; `_state_names()` narrows them to the ones in use) and implements _launch()."""
    STATE = ()

    def __init__(self, model, defaults, param_groups, max_grad_norm, accumulation_steps, ema_decay, ema_warmup):
        _check_common_options(max_grad_norm, accumulation_steps)
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError('ema_decay must lie in [0, 1) or be None, got %r' % (ema_decay, ))
        live = [p for _, p in model.engine.live_params]
        defaults = dict(defaults, max_grad_norm=None if max_grad_norm is None else float(max_grad_norm),
                        accumulation_steps=int(accumulation_steps), ema_decay=None if ema_decay is None else float(ema_decay),
                        ema_warmup=bool(ema_warmup))
        super().__init__(model, _group_dicts(live, param_groups, defaults), defaults)
        for name in self.STATE:
            setattr(self, name, None)
        self.ema = None           # ema_decay only: the shadow of the flat parameters
        self._runs = None         # more than one group: (run_end, run_group) on the device, and how many
        self._layout = None

    @property
    def ema_decay(self):
        return self.param_groups[0]['ema_decay']

    @property
    def ema_warmup(self):
        return bool(self.param_groups[0]['ema_warmup'])

    def _state_names(self):
        return self.STATE

    def state_tensors(self):
        names = list(self._state_names()) + (['ema'] if self.ema_decay is not None else [])
        return [getattr(self, n) for n in names]

    def group_of_params(self):
        """the group index of every live parameter, in flat-buffer order"""
        where = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g['params']}
        return [where[id(p)] for _, p in self.engine.live_params]

    def _ensure_state(self):
        eng = self.engine
        eng.ensure_flat()
        layout = (eng.flat.data_ptr(), eng.flat.numel(), eng.flat.device)
        if self._layout != layout:  # first use, or the parameters moved: everything starts over
            for name in self.STATE:
                setattr(self, name, None)
            self.ema = self.grad_acc = self._sqnorm = self._runs = None
            self.folded = 0
            self._layout = layout
        for name in self._state_names():
            if getattr(self, name) is None:
                setattr(self, name, torch.zeros_like(eng.flat))
        if self.ema_decay is not None and self.ema is None:
            self.ema = eng.flat.clone()  # before the first update: the shadow starts as the parameters
        if len(self.param_groups) > 1 and self._runs is None:
            ends, groups = build_runs(eng.offsets, [p.numel() for _, p in eng.live_params], self.group_of_params())
            if len(ends) > MAX_RUNS:
                raise ValueError('the parameter groups alternate %d times along the flat buffer: at most %d runs' % (len(ends), MAX_RUNS))
            self._runs = (torch.tensor([ends, groups], dtype=torch.int32).to(eng.flat.device), len(ends))
        self._ensure_workspaces()

    def _group_args(self):
        """(lr, weight_decay, ngroups, run_end, run_group, nruns) of the entry points: one group has no table"""
        groups = self.param_groups
        table, nruns = self._runs if self._runs is not None else (None, 0)
        lr, wd = _floats([float(g['lr']) for g in groups]), _floats([float(g['weight_decay']) for g in groups])
        return (lr, wd, len(groups), None if table is None else table[0].data_ptr(), None if table is None else table[1].data_ptr(), nruns)

    def ema_factors(self, t=None):
        """(d, 1 - d) as the two fp32 values update `t` (1-based; default: the last one) hands the kernel: with ema_warmup
        d_t = min(d, (1 + t) / (10 + t)), formed in float64 and rounded once each."""
        t = self.step_count if t is None else t
        d = float(self.ema_decay)
        if self.ema_warmup:
            d = min(d, (1.0 + t) / (10.0 + t))
        return float(torch.tensor(d, dtype=torch.float32)), float(torch.tensor(1.0 - d, dtype=torch.float32))

    def _ema_args(self):
        if self.ema_decay is None:
            return None, 0.0, 0.0
        d, omd = self.ema_factors()
        return self.ema.data_ptr(), d, omd

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        """One update from the engine's flat gradient (or the accumulator of exactly accumulation_steps folds), as FusedAdam.step."""
        grad = self._take_gradient(closure)
        sqnorm, clip = self._clip_args(grad, grad_scale)
        self._launch(grad, float(grad_scale), sqnorm, clip)
        self.engine.mark_params_dirty()

    def _launch(self, grad, grad_scale, sqnorm, clip):
        raise NotImplementedError

    # ---- the averaged weights
    def _require_ema(self, what):
        if self.ema_decay is None:
            raise RuntimeError('%s.%s needs ema_decay' % (type(self).__name__, what))
        self._ensure_state()

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model holds the averaged weights (and the shadow the model's own): the flat parameters and the shadow
        are exchanged on the engine's stream on the way in and exchanged back on the way out, bit for bit."""
        self._require_ema('ema_weights()')
        self._swap_ema()
        try:
            yield self
        finally:
            self._swap_ema()

    @torch.no_grad()
    def _swap_ema(self):
        eng = self.engine
        held = eng.flat.clone()
        eng.flat.copy_(self.ema)
        self.ema.copy_(held)
        eng.mark_params_dirty()

    @torch.no_grad()
    def ema_state_dict(self):
        """model.state_dict() with the shadow's values for the live parameters; the BatchNorm buffers are the model's"""
        self._require_ema('ema_state_dict()')
        eng = self.engine
        sd = self.model.state_dict()
        for (name, p), off in zip(eng.live_params, eng.offsets):
            if name in sd:
                sd[name] = self.ema[off:off + p.numel()].view(p.shape).clone()
        return sd

    # ---- checkpoints
    def state_dict(self):
        """The state buffers by name (None for the ones the configuration does not use), `ema`, the update count and every group's
        hyper-parameters.  The gradient accumulator is not part of the state (see FusedAdam.state_dict)."""
        if self.engine.flat is not None or any(p.is_cuda for _, p in self.engine.live_params):
            self._ensure_state()
        used = set(self._state_names())
        sd = {name: (getattr(self, name) if name in used else None) for name in self.STATE}
        sd.update(step=self.step_count, ema=self.ema if self.ema_decay is not None else None,
                  param_groups=[{k: v for k, v in g.items() if k != 'params'} for g in self.param_groups])
        return sd

    def load_state_dict(self, sd):
        """Into an optimizer built with the same groups: every group takes the saved hyper-parameters; a buffer saved as None starts
        from zeros, a missing shadow from the parameters.  Passes folded so far are discarded."""
        if len(sd['param_groups']) != len(self.param_groups):
            raise ValueError('the checkpoint holds %d parameter groups, this optimizer %d' % (len(sd['param_groups']), len(self.param_groups)))
        for g, saved in zip(self.param_groups, sd['param_groups']):
            g.update({k: v for k, v in saved.items() if k != 'params'})
        self._ensure_state()
        self.step_count = int(sd['step'])
        self.folded = 0
        for name in self._state_names():
            if sd.get(name) is None:
                getattr(self, name).zero_()
            else:
                getattr(self, name).copy_(sd[name])
        if self.ema_decay is not None:
            self.ema.copy_(self.engine.flat if sd.get('ema') is None else sd['ema'])


class FusedSGD(GroupedFlatOptimizer):
    """torch.optim.SGD over the flat buffer in one launch (dbn_sgd_step), with clip_grad_norm_ in front when max_grad_norm is set:
        g = coef s acc + weight_decay_G p;  buf' = g on the first update, momentum buf + (1 - dampening) g afterwards
        p' = p - lr_G (g + momentum buf' | buf' | g)          (nesterov | momentum | momentum = 0: no buffer exists)"""
    TORCH_EQUIVALENT = 'torch.optim.SGD'
    STATE = ('momentum_buffer', )

    def __init__(self, model, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, max_grad_norm=None, accumulation_steps=1,
                 param_groups=None, ema_decay=None, ema_warmup=False):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError('lr, momentum and weight_decay must not be negative')
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        super().__init__(model, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov)),
                         param_groups, max_grad_norm, accumulation_steps, ema_decay, ema_warmup)

    def _state_names(self):
        return self.STATE if self.param_groups[0]['momentum'] != 0 else ()

    def _launch(self, grad, grad_scale, sqnorm, clip):
        eng, g = self.engine, self.param_groups[0]
        buf = self.momentum_buffer
        check(_lib.lib().dbn_sgd_step(eng.flat.data_ptr(), grad.data_ptr(), None if buf is None else buf.data_ptr(), eng.flat.numel(),
                                      *self._group_args(), float(g['momentum']), float(g['dampening']), int(bool(g['nesterov'])),
                                      int(self.step_count == 1), grad_scale, sqnorm, clip, *self._ema_args(), eng.stream), 'sgd_step')


class FusedAdamW(GroupedFlatOptimizer):
    """Adam with weight decay over the flat buffer in one launch (dbn_adamw_step).  decoupled=True is torch.optim.AdamW:
    p <- p (1 - lr_G weight_decay_G), then Adam's update with the undecayed gradient.  decoupled=False is
    torch.optim.Adam(weight_decay): g + weight_decay_G p after the clip, what the reference driver constructs."""
    TORCH_EQUIVALENT = 'torch.optim.AdamW'
    STATE = ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')

    def __init__(self, model, lr=0.005, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, decoupled=True, amsgrad=False,
                 max_grad_norm=None, accumulation_steps=1, param_groups=None, ema_decay=None, ema_warmup=False):
        if lr < 0 or weight_decay < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError('lr, eps and weight_decay must not be negative, the betas lie in [0, 1)')
        super().__init__(model, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, decoupled=bool(decoupled),
                                     amsgrad=bool(amsgrad)),
                         param_groups, max_grad_norm, accumulation_steps, ema_decay, ema_warmup)

    @property
    def amsgrad(self):
        return bool(self.param_groups[0]['amsgrad'])

    def _state_names(self):
        return self.STATE if self.amsgrad else self.STATE[:2]

    def _launch(self, grad, grad_scale, sqnorm, clip):
        eng, g = self.engine, self.param_groups[0]
        check(_lib.lib().dbn_adamw_step(eng.flat.data_ptr(), grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                        self.max_exp_avg_sq.data_ptr() if self.amsgrad else None, eng.flat.numel(), *self._group_args(),
                                        float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), int(bool(g['decoupled'])),
                                        self.step_count, grad_scale, sqnorm, clip, *self._ema_args(), eng.stream), 'adamw_step')
