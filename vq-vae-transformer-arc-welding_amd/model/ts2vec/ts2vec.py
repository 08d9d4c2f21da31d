"""``model.ts2vec.ts2vec.TS2Vec`` of the reference: constructor, ``encode``, ``save`` and ``load`` -- the files
interoperate with the reference's in both directions.  ``fit`` is not built (arcweld/ts2vec.py): train with the
reference, load the checkpoint here.  Unlike the reference this module needs neither tqdm, wandb nor scikit-learn."""
import torch

from arcweld.ts2vec import TSEncoder, averaged_state_dict, strip_averaged


class TS2Vec:
    '''The TS2Vec model (https://github.com/yuezhihan/ts2vec), inference side.'''

    def __init__(
        self,
        input_dims,
        output_dims=320,
        hidden_dims=64,
        depth=10,
        device='cuda',
        lr=0.001,
        batch_size=16,
        max_train_length=None,
        temporal_unit=0,
        after_iter_callback=None,
        after_epoch_callback=None
    ):
        self.device = device
        self.lr = lr
        self.batch_size = batch_size
        self.max_train_length = max_train_length
        self.temporal_unit = temporal_unit
        # the reference keeps the trained net (_net) and its SWA average (net) and evaluates the average; without
        # training there is one set of weights, the averaged one a checkpoint holds
        self.net = TSEncoder(input_dims=input_dims, output_dims=output_dims, hidden_dims=hidden_dims,
                             depth=depth).to(self.device).eval()
        self._net = self.net
        self.n_averaged = 1
        self.after_iter_callback = after_iter_callback
        self.after_epoch_callback = after_epoch_callback
        self.n_epochs = 0
        self.n_iters = 0

    def fit(self, train_data, n_epochs=None, n_iters=None, verbose=False):
        raise NotImplementedError("TS2Vec.fit is not built: the hierarchical contrastive loss, the random crops and "
                                  "masks, AdamW and the SWA average are the follow-up to the inference path "
                                  "(DESIGN.md section 7).  Train with the reference and `load` its checkpoint.")

    def encode(self, data, mask=None, encoding_window=None, causal=False, sliding_length=None, sliding_padding=0,
               batch_size=None):
        '''Representations of data (n_instance, n_timestamps, n_features), NaN = missing, as a numpy array:
        (n_instance, n_timestamps, output_dims), or (n_instance, output_dims) with encoding_window='full_series'.
        batch_size None: this model's batch_size, as in the reference.  What arcweld.ts2vec.TSEncoder.encode does
        not build (random masks, integer / 'multiscale' windows, sliding_length, causal) is a ValueError.'''
        assert self.net is not None, 'please train or load a net first'
        assert data.ndim == 3
        if batch_size is None:
            batch_size = self.batch_size
        out = self.net.encode(data, mask=mask, encoding_window=encoding_window, batch_size=batch_size, causal=causal,
                              sliding_length=sliding_length, sliding_padding=sliding_padding)
        return out.cpu().numpy()

    def save(self, fn):
        '''Save the model to a file the reference's TS2Vec.load reads (an AveragedModel state dict).'''
        torch.save(averaged_state_dict(self.net, self.n_averaged), fn)

    def load(self, fn):
        '''Load a file written by this class's or the reference's TS2Vec.save.'''
        state_dict = torch.load(fn, map_location=self.device)
        plain, n_averaged = strip_averaged(state_dict)
        self.net.load_state_dict(plain)
        self.n_averaged = n_averaged if n_averaged is not None else 1
