"""``model.ts2vec.encoder.TSEncoder`` of the reference, computed by arcweld.ts2vec (csrc/ts2vec.hip)."""
from arcweld.ts2vec import TSEncoder

__all__ = ["TSEncoder"]
