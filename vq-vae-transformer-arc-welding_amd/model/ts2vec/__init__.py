"""Drop-in surface of the reference's ``model/ts2vec`` package: the TS2Vec baseline whose pooled representations the
evaluation protocols score.  Inference only: ``TS2Vec.encode`` runs arcweld.ts2vec.TSEncoder on the HIP kernels."""
from .encoder import TSEncoder
from .ts2vec import TS2Vec

__all__ = ["TS2Vec", "TSEncoder"]
