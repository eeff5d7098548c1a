"""Shared helpers of test_loss.py / test_gpu_loss.py: the loss fixtures of tests/golden/gen_golden_loss.py
(loaded once per process and never modified) and a runner of the rmd.loss classes on them."""

import functools
import json

import numpy as np
import torch

from conftest import load_golden

# fixture file -> variant tags (tests/golden/gen_golden_loss.py)
FILES = {
    "loss_seq": ["ord1", "ord2", "absmean", "invalid"],
    "loss_mlseq": ["ord1", "ord2"],
    "loss_mlseq_ragged": ["ord1", "ord2"],
    "loss_empty_all": ["ord1"],
    "loss_empty_one": ["ord1"],
    "loss_restricted": ["bilinear", "nearest"],
    "loss_multiscale": ["ord2_range", "ord2_norange", "ordrobust_range", "ordrobust_norange"],
    "loss_many": ["ord1"],
}
CASES = [(f, tag) for f, tags in FILES.items() for tag in tags]


class Case:
    def __init__(self, name, tag):
        g = _file(name)
        assert tag in json.loads(str(g["variants"]))
        self.name, self.tag = name, tag
        self.type = str(g["type"])
        self.arguments = json.loads(str(g[f"{tag}/arguments"]))
        self.config = json.loads(str(g[f"{tag}/config"]))
        self.structure = json.loads(str(g["structure"]))
        self.target = g["target"].astype(np.float32)
        self.valid = g["valid"]
        n = sum(1 for k in g if k.startswith("flow_"))
        self.flows = [g[f"flow_{i}"].astype(np.float32) for i in range(n)]
        self.prevs = [g[f"prev_{i}"].astype(np.float32) for i in range(n)] if self.structure["pairs"] else None
        self.loss = float(g[f"{tag}/loss"])
        self.grads = [g[f"{tag}/grad_{i}"] for i in range(n)]

    def result(self, flows, prevs=None):
        """The reference's result structure over the given flow tensors."""
        levels = self.structure["levels"]
        if levels is None:
            return list(flows)
        out, at = [], 0
        for n in levels:
            if self.structure["pairs"]:
                out.append([(prevs[i], flows[i]) for i in range(at, at + n)])
            else:
                out.append(list(flows[at:at + n]))
            at += n
        return out


@functools.lru_cache(maxsize=None)
def _file(name):
    return load_golden(name)


@functools.lru_cache(maxsize=None)
def case(name, tag):
    return Case(name, tag)


def loss_class(type_name):
    import rmd.loss
    for cls in (rmd.loss.SequenceLoss, rmd.loss.MultiLevelSequenceLoss, rmd.loss.RestrictedMultiLevelSequenceLoss,
                rmd.loss.MultiscaleLoss):
        if cls.type == type_name:
            return cls
    raise KeyError(type_name)


def run(c, device, requires_grad=None):
    """The rmd.loss class of case c on `device` -> (loss object, loss tensor, flow tensors after backward)."""
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    flows = [t(f).requires_grad_(True if requires_grad is None else requires_grad[i])
             for i, f in enumerate(c.flows)]
    prevs = [t(p) for p in c.prevs] if c.prevs is not None else None
    obj = loss_class(c.type).from_config({"type": c.type, "arguments": c.arguments})
    loss = obj(None, c.result(flows, prevs), t(c.target), t(c.valid))
    loss.backward()
    return obj, loss, flows


def check_against_fixture(c, loss, flows, loss_rtol):
    from conftest import assert_fp32_gate
    got = float(loss.detach().cpu())
    print(f"{c.name}/{c.tag}: loss {got!r} ref {c.loss!r} rel {abs(got - c.loss) / max(abs(c.loss), 1e-30):.3e}")
    assert np.isnan(got) == np.isnan(c.loss)
    if not np.isnan(c.loss):
        assert abs(got - c.loss) <= loss_rtol * abs(c.loss), (got, c.loss)
    for f, ref in zip(flows, c.grads):
        # a prediction the loss skips (no pixel in range) is not in the reference's graph: no gradient == zeros
        g = np.zeros_like(ref) if f.grad is None else f.grad.detach().cpu().numpy()
        assert g.dtype == np.float32 and g.shape == ref.shape
        assert np.array_equal(g == 0, ref == 0), "zero pattern differs"
        assert_fp32_gate(g, ref)
