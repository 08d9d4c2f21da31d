"""``model.ts2vec.ts2vec.TS2Vec`` of the reference: constructor, ``fit``, ``encode``, ``save`` and ``load`` -- the files
interoperate with the reference's in both directions.  ``fit`` trains with the fused contrastive loss of
csrc/ts2vec_loss.hip; the encoder's training forward and backward run on torch ops (arcweld/ts2vec.py).  Unlike the
reference this module needs neither tqdm, wandb nor scikit-learn."""
import copy

import numpy as np
import torch
from torch.utils.data import DataLoader, TensorDataset

from arcweld.ts2vec import (TSEncoder, averaged_state_dict, centerize_vary_length_series, draw_crops,
                            hierarchical_contrastive_loss, split_with_nan, strip_averaged, swa_update, take_per_row)


class TS2Vec:
    '''The TS2Vec model (https://github.com/yuezhihan/ts2vec).'''

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
        # the reference keeps the trained net (_net) and its SWA average (net) and evaluates the average.  Until the
        # first fit there is one set of weights: _net becomes a training copy of net then (for a fresh model exactly
        # the reference's state, whose average starts as a copy of _net; after `load`, training resumes from the
        # loaded average, where the reference would train its still random _net)
        self.net = TSEncoder(input_dims=input_dims, output_dims=output_dims, hidden_dims=hidden_dims,
                             depth=depth).to(self.device).eval()
        self._net = self.net
        self.n_averaged = 1
        self.after_iter_callback = after_iter_callback
        self.after_epoch_callback = after_epoch_callback
        self.n_epochs = 0
        self.n_iters = 0

    def fit(self, train_data, n_epochs=None, n_iters=None, verbose=False):
        '''Train on train_data (n_instance, n_timestamps, n_features), NaN = missing, until n_epochs epochs or n_iters
        iterations have run in this model's lifetime (neither given: 200 iterations, 600 for more than 100000
        values).  Returns the mean loss of every completed epoch.  The crops and masks come from np.random and the
        batches from torch's generator in the reference's order: a seeded run is replayable.'''
        assert train_data.ndim == 3
        if torch.device(self.device).type != 'cuda':
            raise NotImplementedError("TS2Vec.fit on a CPU device is not built: training has no CPU path (the "
                                      "contrastive loss runs on the HIP kernels); construct the model on the GPU")
        if n_iters is None and n_epochs is None:
            n_iters = 200 if train_data.size <= 100000 else 600

        if self.max_train_length is not None:
            sections = train_data.shape[1] // self.max_train_length
            if sections >= 2:
                train_data = np.concatenate(split_with_nan(train_data, sections, axis=1), axis=0)
        missing_step = np.isnan(train_data).all(axis=-1).any(axis=0)
        if missing_step[0] or missing_step[-1]:
            train_data = centerize_vary_length_series(train_data)
        train_data = train_data[~np.isnan(train_data).all(axis=2).all(axis=1)]

        dataset = TensorDataset(torch.from_numpy(train_data).to(torch.float))
        loader = DataLoader(dataset, batch_size=min(self.batch_size, len(dataset)), shuffle=True, drop_last=True)

        if self._net is self.net:
            self._net = copy.deepcopy(self.net).train()
        optimizer = torch.optim.AdamW(self._net.parameters(), lr=self.lr)
        loss_log = []
        while True:
            if n_epochs is not None and self.n_epochs >= n_epochs:
                break
            cum_loss, n_epoch_iters, interrupted = 0, 0, False
            for (x,) in loader:
                if n_iters is not None and self.n_iters >= n_iters:
                    interrupted = True
                    break
                if self.max_train_length is not None and x.size(1) > self.max_train_length:
                    window = np.random.randint(x.size(1) - self.max_train_length + 1)
                    x = x[:, window:window + self.max_train_length]
                x = x.to(self.device)
                c = draw_crops(x.size(1), x.size(0), self.temporal_unit)

                optimizer.zero_grad()
                out1 = self._net.train_forward(take_per_row(x, c["offset"] + c["eleft"], c["right"] - c["eleft"]))
                out2 = self._net.train_forward(take_per_row(x, c["offset"] + c["left"], c["eright"] - c["left"]))
                loss = hierarchical_contrastive_loss(out1[:, -c["crop_l"]:], out2[:, :c["crop_l"]],
                                                     temporal_unit=self.temporal_unit)
                loss.backward()
                optimizer.step()
                self.n_averaged = swa_update(self.net, self._net, self.n_averaged)

                loss_value = loss.item()
                cum_loss += loss_value
                n_epoch_iters += 1
                self.n_iters += 1
                if self.after_iter_callback is not None:
                    self.after_iter_callback(self, loss_value)
            if interrupted:
                break
            cum_loss /= n_epoch_iters
            loss_log.append(cum_loss)
            if verbose:
                print(f"Epoch #{self.n_epochs}: loss={cum_loss}")
            self.n_epochs += 1
            if self.after_epoch_callback is not None:
                self.after_epoch_callback(self, cum_loss)
        return loss_log

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
        self._net = self.net            # the next fit trains a copy of what was loaded
