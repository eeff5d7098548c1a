"""Drop-in flow metrics over the fused statistics kernel (rmd.ops.flow_metrics, csrc/metrics.hip).

  Metric               registry / base            <- src/metrics/common.py:5-57
  EndPointError        'epe'                      <- src/metrics/epe.py:10-57
  FlAll                'fl-all'                   <- src/metrics/fl_all.py:7-48
  AverageAngularError  'aae'                      <- src/metrics/aae.py:7-48
  FlowMagnitude        'flow-magnitude'           <- src/metrics/flow.py:7-40
  Loss                 'loss'                     <- src/metrics/loss.py:7-34
  FlowMetrics          the list of a config       <- Metrics, src/cmd/eval.py:93-109

Same `type` strings, constructor arguments and defaults, from_config / get_config, result keys in the
same order, compute(model, optimizer, estimate, target, valid, loss) and reduce as the reference's.  A
compute is one launch and one readback where the reference reads back once per value; FlowMetrics
shares one launch and one readback among all its metrics (the loss rides along), and per_sample()
returns what the evaluator's per-sample loop (src/evaluation/evaluator.py:29-37) would collect, still
from that one launch.  The gradient, parameter and learning-rate metrics are not covered:
Metric.from_config raises the reference's KeyError for a type it does not know.

AverageAngularError deviates on purpose: the reference indexes the LAST axis of the
(..., 2, H, W) tensors it is handed; this class takes the flow components from the channel axis, over
all pixels, which is what the reference computes from channel-last views.
"""

from collections import OrderedDict

import numpy as np
import torch

from . import ops


def _values(host, sample=None, estimate=0):
    """Python floats of one estimate from a host-side FlowMetricsResult: the batch or one sample."""
    key = "lists/batch" if sample is None else "lists/per_sample"
    lists = host._derived.get(key)
    if lists is None:               # one tolist() per tensor and result, not one per sample
        d = host.batch() if sample is None else host.per_sample()
        lists = host._derived[key] = {k: v.tolist() for k, v in d.items()}
    pick = (lambda t: t[estimate]) if sample is None else (lambda t: t[estimate][sample])
    out = {k: pick(v) for k, v in lists.items() if k != "within"}
    out["within"] = dict(zip(host.distances, pick(lists["within"])))
    return out


class Metric:
    """src/metrics/common.py:5-57."""

    type = None

    @classmethod
    def _typecheck(cls, cfg):
        if cfg['type'] != cls.type:
            raise ValueError(f"invalid metric type '{cfg['type']}', expected '{cls.type}'")

    @classmethod
    def from_config(cls, cfg):
        types = [AverageAngularError, EndPointError, FlAll, FlowMagnitude, Loss]
        types = {cls.type: cls for cls in types}

        return types[cfg['type']].from_config(cfg)

    def __init__(self):
        pass

    def get_config(self):
        raise NotImplementedError

    # what this metric asks of the shared launch, and its result from that launch's values
    distances = ()
    ord = None

    def result(self, values, loss=None):
        raise NotImplementedError

    @torch.no_grad()
    def compute(self, model, optimizer, estimate, target, valid, loss):
        # Inputs are (c, h, w) for estimate and target and (h, w) for the valid mask, optionally with a
        # batch dimension in front: the metric is then computed over the whole batch.
        host = ops.flow_metrics(estimate, target, valid, distances=self.distances,
                                ord=2 if self.ord is None else self.ord).host()
        return self.result(_values(host))

    def __call__(self, model, optimizer, estimate, target, valid, loss):
        return self.compute(model, optimizer, estimate, target, valid, loss)

    @torch.no_grad()
    def reduce(self, values):
        return {k: np.mean(vs) for k, vs in values.items()}


class EndPointError(Metric):
    type = 'epe'

    @classmethod
    def from_config(cls, cfg):
        cls._typecheck(cfg)

        key = cfg.get('key', 'EndPointError/')
        dist = list(cfg.get('distances', [1, 3, 5]))

        return cls(dist, key)

    def __init__(self, distances=[1, 3, 5], key='EndPointError/'):
        super().__init__()

        self.distances = distances
        self.key = key

    def get_config(self):
        return {
            'type': self.type,
            'key': self.key,
            'distances': self.distances,
        }

    def result(self, values, loss=None):
        # note: these definitions are inverted (i.e. 1 - x) to the bad-pixel error as used in literature
        result = OrderedDict()
        result[f'{self.key}mean'] = values['epe']
        for d in self.distances:
            result[f'{self.key}{d}px'] = values['within'][float(d)]
        return result


class FlAll(Metric):
    type = 'fl-all'

    @classmethod
    def from_config(cls, cfg):
        cls._typecheck(cfg)

        key = cfg.get('key', 'Fl-all')

        return cls(key)

    def __init__(self, key='Fl-all'):
        super().__init__()

        self.key = key

    def get_config(self):
        return {
            'type': self.type,
            'key': self.key,
        }

    def result(self, values, loss=None):
        # outliers/bad pixels: epe > 3px and epe > 5% of the target (the kernel's defaults)
        return {self.key: values['fl_all']}


class AverageAngularError(Metric):
    type = 'aae'

    @classmethod
    def from_config(cls, cfg):
        cls._typecheck(cfg)

        key = cfg.get('key', 'AverageAngularError')

        return cls(key)

    def __init__(self, key='AverageAngularError'):
        super().__init__()

        self.key = key

    def get_config(self):
        return {
            'type': self.type,
            'key': self.key,
        }

    def result(self, values, loss=None):
        return {self.key: values['aae']}


class FlowMagnitude(Metric):
    type = 'flow-magnitude'

    @classmethod
    def from_config(cls, cfg):
        cls._typecheck(cfg)

        key = cfg.get('key', 'FlowMagnitude')
        ord = cfg.get('ord', 2)

        return cls(ord, key)

    def __init__(self, ord=2, key='FlowMagnitude'):
        super().__init__()

        self.ord = ord
        self.key = key

    def get_config(self):
        return {
            'type': self.type,
            'key': self.key,
            'ord': self.ord,
        }

    def result(self, values, loss=None):
        return {self.key: values['magnitude']}


class Loss(Metric):
    """The passthrough of src/metrics/loss.py: no launch; a tensor is read back, a number is taken as is."""

    type = 'loss'

    @classmethod
    def from_config(cls, cfg):
        cls._typecheck(cfg)

        key = cfg.get('key', 'Loss')
        return cls(key)

    def __init__(self, key='Loss'):
        super().__init__()

        self.key = key

    def get_config(self):
        return {
            'type': 'loss',
            'key': self.key,
        }

    def result(self, values, loss=None):
        return {self.key: loss.item() if isinstance(loss, torch.Tensor) else loss}

    @torch.no_grad()
    def compute(self, model, optimizer, estimate, target, valid, loss):
        return self.result(None, loss)


class FlowMetrics:
    """Metrics of src/cmd/eval.py:93-109 over one shared launch."""

    @classmethod
    def from_config(cls, cfg):
        return cls([Metric.from_config(c) for c in cfg])

    def __init__(self, metrics):
        self.metrics = metrics

    def _launch(self, estimate, target, valid, loss=None):
        """One launch for all metrics (one more per additional magnitude `ord`), one readback each."""
        distances = []
        for m in self.metrics:
            distances += [float(d) for d in m.distances if float(d) not in distances]
        ords = []
        for m in self.metrics:
            if m.ord is not None and float(m.ord) not in ords:
                ords.append(float(m.ord))
        extra = loss if isinstance(loss, torch.Tensor) else None
        first = ords[0] if ords else 2.0
        hosts = {first: ops.flow_metrics(estimate, target, valid, distances, ord=first, extra=extra).host()}
        for o in ords[1:]:
            hosts[o] = ops.flow_metrics(estimate, target, valid, (), ord=o).host()
        if extra is not None:
            loss = float(hosts[first].extra)
        return hosts, first, loss

    def _collect(self, hosts, first, loss, sample=None):
        values = {o: _values(h, sample) for o, h in hosts.items()}
        result = OrderedDict()
        for m in self.metrics:
            if isinstance(m, Loss) and loss is None:
                continue
            result.update(m.result(values[first if m.ord is None else float(m.ord)], loss))
        return result

    @torch.no_grad()
    def __call__(self, model, estimate, target, valid, loss):
        hosts, first, loss = self._launch(estimate, target, valid, loss)
        return self._collect(hosts, first, loss)

    @torch.no_grad()
    def per_sample(self, model, estimate, target, valid):
        """One dict per sample of the batch, as if every sample had been passed on its own."""
        hosts, first, _ = self._launch(estimate, target, valid)
        return [self._collect(hosts, first, None, b) for b in range(hosts[first].stats.shape[1])]
