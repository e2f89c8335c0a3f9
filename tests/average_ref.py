"""K43's rule restated: the tick (does this call blend, and with what weight) and the element rule, one rounding per operation
in numpy ``float32`` — what ``mbv_weight_average_update`` and ``arena.WeightAverage`` are held to bit for bit — and the same in
``float64`` for sanity checks.  Pure numpy; no product code."""
import numpy as np


class AverageRef:
    """``step(param, applied)`` mirrors one ``WeightAverage.update()`` after an optimizer step that was applied or skipped."""

    def __init__(self, param, mode='ema', decay=0.9999, warmup=True, every=1, dtype=np.float32):
        assert mode in ('ema', 'mean') and every >= 1
        self.t = dtype
        self.mode, self.warmup, self.every = mode, bool(warmup), int(every)
        self.decay = dtype(decay)              # the product takes the decay as an f32
        self.avg = np.array(param, dtype=dtype, copy=True)
        self.updates = self.calls = 0
        self.weight = dtype(0)

    def tick(self, applied=True):
        """The blend weight of this call (0: do nothing); advances the counters."""
        t = self.t
        w = t(0)
        if applied:
            self.calls += 1
            if self.calls % self.every == 0:
                u = self.updates
                if self.mode == 'mean':
                    w = t(1) / t(u + 1)
                else:
                    d = self.decay
                    if self.warmup:
                        d = min(d, t(1 + u) / t(10 + u))
                    w = t(1) - d
                self.updates += 1
        self.weight = w
        return w

    def step(self, param, applied=True):
        w = self.tick(applied)
        p = np.asarray(param, dtype=self.t)
        if w == 1:
            self.avg = p.copy()
        elif w != 0:
            d = p - self.avg                   # three roundings: subtract, multiply, add
            d = w * d
            self.avg = self.avg + d
        assert self.avg.dtype == self.t
        return self.avg


def run(init, snapshots, applied=None, **kw):
    """The averages after each of ``snapshots`` (parameter values after each optimizer step), starting from ``init``."""
    ref = AverageRef(init, **kw)
    applied = [True] * len(snapshots) if applied is None else applied
    return [ref.step(p, a).copy() for p, a in zip(snapshots, applied)], ref
