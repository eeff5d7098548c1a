"""Drop-in loss classes over the fused sequence loss (rmd.ops.sequence_loss, csrc/loss.hip).

  SequenceLoss                      'raft/sequence'               <- src/models/impls/raft.py:596-644
  MultiLevelSequenceLoss            'raft+dicl/mlseq'             <- src/models/common/loss/mlseq.py:7-67
  RestrictedMultiLevelSequenceLoss  'raft+dicl/mlseq-restricted'  <- src/models/impls/raft_dicl_ctf_l3.py:401-473
  MultiscaleLoss                    'dicl/multiscale'             <- src/models/impls/dicl.py:416-472

Same `type` strings, from_config / get_config (same defaults), compute signatures and __call__ argument
merging as the reference's (src/models/model.py:65-83).  Each compute turns the reference's loop into one
weight per prediction and hands all predictions to one fused call; the masks of the restricted and the
multiscale loss are plain elementwise torch ops.  Nothing here reads a value back to the host.
"""

import torch

from . import cpu, ops


class Loss:
    """src/models/model.py:65-83."""

    type = None

    @classmethod
    def _typecheck(cls, cfg):
        if cfg['type'] != cls.type:
            raise ValueError(f"invalid loss type '{cfg['type']}', expected '{cls.type}'")

    @classmethod
    def from_config(cls, cfg):
        cls._typecheck(cfg)
        return cls(cfg.get('arguments', {}))

    def __init__(self, arguments={}):
        self.arguments = arguments

    def get_config(self):
        raise NotImplementedError

    def compute(self, model, result, target, valid, **kwargs):
        raise NotImplementedError

    def __call__(self, model, result, target, valid, **kwargs):
        return self.compute(model, result, target, valid, **(self.arguments | kwargs))


class SequenceLoss(Loss):
    type = 'raft/sequence'

    def get_config(self):
        default_args = {'ord': 1, 'gamma': 0.8, 'include_invalid': False}
        return {'type': self.type, 'arguments': default_args | self.arguments}

    def compute(self, model, result, target, valid, ord=1, gamma=0.8, include_invalid=False):
        n = len(result)
        weights = [gamma**(n - i - 1) for i in range(n)]                    # raft.py:622
        return ops.sequence_loss(result, target, valid, weights, ord=ord, include_invalid=include_invalid)


def _mlseq_weights(result, alpha, gamma):
    """alpha[level] * gamma**(n - i - 1) per prediction, levels flattened in order (mlseq.py:37-42)."""
    return [alpha[i_level] * gamma**(len(level) - i_seq - 1)
            for i_level, level in enumerate(result) for i_seq in range(len(level))]


class MultiLevelSequenceLoss(Loss):
    """Multi-level sequence loss"""

    type = 'raft+dicl/mlseq'

    def get_config(self):
        default_args = {'ord': 1, 'gamma': 0.8, 'alpha': (1.0, 0.5), 'scale': 1.0}
        return {'type': self.type, 'arguments': default_args | self.arguments}

    def compute(self, model, result, target, valid, ord=1, gamma=0.8, alpha=(0.4, 1.0), scale=1.0):
        flows = [flow for level in result for flow in level]
        return ops.sequence_loss(flows, target, valid, _mlseq_weights(result, alpha, gamma), ord=ord, scale=scale)


class RestrictedMultiLevelSequenceLoss(Loss):
    """Multi-level sequence loss"""

    type = 'raft+dicl/mlseq-restricted'

    def get_config(self):
        default_args = {'ord': 1, 'gamma': 0.85, 'alpha': (0.38, 0.6, 1.0), 'scale': 1.0,
                        'delta_range': (128, 64, 32), 'delta_mode': 'bilinear'}
        return {'type': self.type, 'arguments': default_args | self.arguments}

    def compute(self, model, result, target, valid, ord=1, gamma=0.8, alpha=(0.4, 1.0), scale=1.0,
                delta_range=(128, 64, 32), delta_mode='nearest'):
        flows, masks = [], []
        with torch.no_grad():
            for i_level, level in enumerate(result):
                for flow_prev, flow in level:
                    flow_prev = flow_prev.detach().float()
                    if flow_prev.shape != target.shape:                     # raft_dicl_ctf_l3.py:445-446
                        flow_prev = cpu.loss_upsample(flow_prev, target.shape, delta_mode)
                    # restrict loss to displacements in range (raft_dicl_ctf_l3.py:449-451)
                    delta = (target - flow_prev).abs()
                    valid_lvl = (delta[:, 0] <= delta_range[i_level]) & (delta[:, 1] <= delta_range[i_level])
                    masks.append(valid_lvl & valid.bool())
                    flows.append(flow)
        # a level without any pixel in range is skipped (raft_dicl_ctf_l3.py:453): decided on the device
        return ops.sequence_loss(flows, target, valid, _mlseq_weights(result, alpha, gamma), ord=ord, masks=masks,
                                 skip_empty=True, scale=scale)


class MultiscaleLoss(Loss):
    type = 'dicl/multiscale'

    def get_config(self):
        default_args = {'ord': 2, 'mode': 'bilinear'}
        return {'type': self.type, 'arguments': default_args | self.arguments}

    def compute(self, model, result, target, valid, weights, ord=2, mode='bilinear', valid_range=None):
        masks = None
        if valid_range is not None:                                         # dicl.py:443-447
            with torch.no_grad():
                masks = [valid.bool() & (target[..., 0, :, :].abs() < valid_range[i][0])
                         & (target[..., 1, :, :].abs() < valid_range[i][1]) for i in range(len(result))]
        if ord != 'robust':
            ord = float(ord)                                                # dicl.py:453
        # normalize for our convenience (dicl.py:462)
        w = [weights[i] / len(result) for i in range(len(result))]
        return ops.sequence_loss(result, target, valid, w, ord=ord, masks=masks, mode=mode)
