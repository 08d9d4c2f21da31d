"""``model.ts2vec.losses`` of the reference: the three names and signatures, computed by the fused HIP kernels
(arcweld.ts2vec, csrc/ts2vec_loss.hip).  f32 device tensors; there is no CPU path."""
from arcweld import ts2vec as _ts

__all__ = ["hierarchical_contrastive_loss", "instance_contrastive_loss", "temporal_contrastive_loss"]


def hierarchical_contrastive_loss(z1, z2, alpha=0.5, temporal_unit=0):
    return _ts.hierarchical_contrastive_loss(z1, z2, alpha=alpha, temporal_unit=temporal_unit)


def instance_contrastive_loss(z1, z2):
    return _ts.instance_contrastive_loss(z1, z2)


def temporal_contrastive_loss(z1, z2):
    return _ts.temporal_contrastive_loss(z1, z2)
