"""rmd — MI355X-native (gfx950) cost-volume backend for qzed/raft-meets-dicl.

Drop-in host mirror of the reference's hot-path modules; every compute call on GPU tensors goes
through the C ABI of librmd.so (include/rmd.h) on the current HIP stream and raises if the library
is missing.  CPU tensors dispatch to the operators' CPU kernels (rmd/cpu.py: the reference's ATen
algorithm), so the modules also run on device='cpu' as the reference's do.

  rmd.raft.CorrBlock                    <- src/models/impls/raft.py:15-95
  rmd.raft_fs.CorrBlock                 <- src/models/impls/raft_fs.py:13-87
  rmd.corr.make_cmod / CorrelationModule <- src/models/common/corr/{dicl,dicl_1x1,dicl_emb,dot}.py
  rmd.raft_dicl_ml.CorrelationModule    <- src/models/impls/raft_dicl_ml.py:235-343
  rmd.blocks.dicl                       <- src/models/common/blocks/dicl.py:93-150
  rmd.blocks.raft.ResidualBlock         <- src/models/common/blocks/raft.py:13-46
  rmd.encoders.FeatureEncoder / make_encoder_s3
                                        <- src/models/common/encoders/raft/s3.py:8-72, encoders/__init__.py:52-60
                                           (one fused forward, rmd.ops.feature_encoder)
  rmd.dicl.compute_cost                 <- src/models/impls/dicl.py:171-241 (+ fused warp)
  rmd.dicl.FlowRegression / FlowEntropy / FlowLevelMixin
                                        <- src/models/impls/dicl.py:31-85, 186-210 (one fused head pass,
                                           rmd.ops.dicl_flow_head)
  rmd.hsup.HUpNone / HUpBilinear / HUpCrossAttn / make_hidden_state_upsampler
                                        <- src/models/common/hsup.py:8-108 (one fused local cross-attention
                                           pass, rmd.ops.local_cross_attn)
  rmd.warp.warp_backwards               <- src/models/common/warp.py:5-33
  rmd.raft.Up8Network / SoftArgMax*     <- src/models/impls/raft.py:98-190,299-331 (rmd.heads)
  rmd.input.InputSpec / ModuloPadding   <- src/models/input.py:32-313 (frame pair + flow target format)
  rmd.loss.SequenceLoss / MultiLevelSequenceLoss / RestrictedMultiLevelSequenceLoss / MultiscaleLoss
                                        <- raft.py:596-644, common/loss/mlseq.py, raft_dicl_ctf_l3.py:401-473,
                                           dicl.py:416-472 (one fused forward + backward, rmd.ops.sequence_loss)
  rmd.metrics.EndPointError / FlAll / AverageAngularError / FlowMagnitude / Loss / FlowMetrics
                                        <- src/metrics/{epe,fl_all,aae,flow,loss}.py, src/cmd/eval.py:93-109
                                           (one fused statistics pass, rmd.ops.flow_metrics)
"""

from . import blocks, config, corr, cpu, dicl, encoders, heads, hsup, input, loss, metrics, ops, raft, raft_dicl_ml, raft_fs, warp  # noqa: F401
from .hsup import HUpBilinear, HUpCrossAttn, HUpNone, make_hidden_state_upsampler  # noqa: F401
from .loss import MultiLevelSequenceLoss, MultiscaleLoss, RestrictedMultiLevelSequenceLoss, SequenceLoss  # noqa: F401
from .metrics import FlowMetrics  # noqa: F401
from .ops import set_default_precision, get_default_precision  # noqa: F401

__version__ = "0.1"
