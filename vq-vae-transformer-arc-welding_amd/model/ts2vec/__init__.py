"""Drop-in surface of the reference's ``model/ts2vec`` package: the TS2Vec baseline whose pooled representations the
evaluation protocols score.  ``TS2Vec.encode`` runs arcweld.ts2vec.TSEncoder on the HIP kernels; ``TS2Vec.fit`` trains
it with the fused contrastive loss of csrc/ts2vec_loss.hip (``model.ts2vec.losses``)."""
from .encoder import TSEncoder
from .ts2vec import TS2Vec

__all__ = ["TS2Vec", "TSEncoder"]
