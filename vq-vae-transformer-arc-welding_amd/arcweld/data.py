"""HBM-resident data plumbing for the two training stages.

The reference feeds host DataLoaders (ASIMoWDataModule for reconstruction, dataloader/asimow_dataloader.py; and
LatentPredDataModule over tokenized sequences, dataloader/latentspace_dataloader.py) and, under DDP, a
DistributedSampler per rank.  Here a whole split is resident in HBM (1024 windows x 200 x 2 f32 = 1.6 MB; a
288 GB device holds the full ASIMoW set many times over) and a batch is an index-gather on the device:

* DeviceBatches -- DataLoader(shuffle, drop_last=False) x DistributedSampler(rank, world) semantics: per-epoch
  permutation seeded by (seed + epoch), padded to a multiple of world, rank r takes positions r, r+world, ...
* synthetic_windows -- N(0, 1) 200x2 windows (the StandardScaler'd ASIMoW distribution); the real
  dataset is not available offline.
* ReconstructionDataModule / LatentPredDataModule / ClassificationDataModule -- the datamodule surface the entry
  scripts use.
* WeightedBatches -- DataLoader(sampler=WeightedRandomSampler(weights, n)) semantics for the classifier's training
  split: n draws with replacement per epoch.
"""
from __future__ import annotations

import math

import torch

from . import tokenize


def _rank_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


class DeviceBatches:
    def __init__(self, tensors, batch_size, shuffle=True, seed=0, rank=None, world=None, drop_last=False):
        self.tensors = tensors if isinstance(tensors, (list, tuple)) else (tensors,)
        self.single = not isinstance(tensors, (list, tuple))
        self.n = len(self.tensors[0])
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        self.seed = seed
        r, w = _rank_world()
        self.rank = r if rank is None else rank
        self.world = w if world is None else world
        self.drop_last = drop_last
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def indices(self):
        """This rank's sample indices for the current epoch (torch DistributedSampler arithmetic)."""
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            order = torch.randperm(self.n, generator=g)
        else:
            order = torch.arange(self.n)
        per_rank = math.ceil(self.n / self.world)
        total = per_rank * self.world
        if total > self.n:
            order = torch.cat([order, order[:total - self.n]])
        return order[self.rank:total:self.world]

    def __len__(self):
        per_rank = math.ceil(self.n / self.world)
        return per_rank // self.batch_size if self.drop_last else math.ceil(per_rank / self.batch_size)

    def __iter__(self):
        idx = self.indices().to(self.tensors[0].device)
        for b in range(len(self)):
            sel = idx[b * self.batch_size:(b + 1) * self.batch_size]
            out = tuple(t.index_select(0, sel) for t in self.tensors)
            yield out[0] if self.single else out


def synthetic_windows(n, n_cycles=1, seed=0, device="cuda", window=200, channels=2):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return torch.randn(n, window * n_cycles, channels, device=device, generator=g)


def synthetic_labels(n, seed=0, device="cuda"):
    g = torch.Generator(device=device)
    g.manual_seed(seed + 7)
    return torch.randint(0, 2, (n,), device=device, generator=g)


class ReconstructionDataModule:
    """ASIMoWDataModule(task="reconstruction", n_cycles=1) surface over synthetic windows (or given tensors)."""

    def __init__(self, batch_size=1024, n_train=8192, n_val=1024, n_test=1024, seed=0, device="cuda", data=None):
        self.batch_size, self.seed, self.device = batch_size, seed, device
        self.sizes = (n_train, n_val, n_test)
        self.data = data
        self.train_ds = self.val_ds = self.test_ds = None

    def setup(self, stage=None):
        if self.train_ds is not None:
            return
        if self.data is not None:
            self.train_ds, self.val_ds, self.test_ds = self.data
        else:
            self.train_ds, self.val_ds, self.test_ds = (synthetic_windows(n, 1, self.seed + 101 * i, self.device)
                                                        for i, n in enumerate(self.sizes))

    def train_dataloader(self):
        return DeviceBatches(self.train_ds, self.batch_size, shuffle=True, seed=self.seed)

    def val_dataloader(self):
        return DeviceBatches(self.val_ds, self.batch_size, shuffle=False)

    def test_dataloader(self):
        return DeviceBatches(self.test_ds, self.batch_size, shuffle=False, rank=0, world=1)


class LatentPredDataModule:
    """Tokenized sequences for the Transformer (latentspace_dataloader.py:23-135, task "autoregressive_ids" /
    "autoregressive_ids_classification"): every split's windows (n, n_cycles*200, 2) are encoded by the frozen
    VQ-VAE in one fused pass and wrapped in MyLatentAutoregressiveDataset (start/end tokens)."""

    def __init__(self, vqvae, splits, batch_size=16, task="autoregressive_ids", seed=0, encode_dtype=torch.float32,
                 tokenized=None):
        self.vqvae, self.splits, self.batch_size, self.task, self.seed = vqvae, splits, batch_size, task, seed
        self.encode_dtype = encode_dtype
        self.tokenized = tokenized          # optional [(ids, labels)] per split, shared between the two tasks
        self.ds = None

    def tokenize(self):
        if self.tokenized is None:
            self.tokenized = [(tokenize.encode_ids(self.vqvae, x, dtype=self.encode_dtype), y)
                              for x, y in self.splits]
        return self.tokenized

    def setup(self, stage=None):
        if self.ds is not None:
            return
        self.ds = []
        for ids, y in self.tokenize():
            labels = None if self.task == "autoregressive_ids" else y
            self.ds.append(tokenize.MyLatentAutoregressiveDataset(ids, labels))
        self.train_ds, self.val_ds, self.test_ds = self.ds

    def _batches(self, ds, shuffle, **kw):
        cond = ds.labels if ds.labels is not None else torch.zeros(len(ds), 1, dtype=torch.long,
                                                                   device=ds.data.device)
        return DeviceBatches((ds.data, cond, ds.data_shifted), self.batch_size, shuffle=shuffle, seed=self.seed, **kw)

    def train_dataloader(self):
        return self._batches(self.train_ds, True)

    def val_dataloader(self):
        return self._batches(self.val_ds, False)

    def test_dataloader(self):
        return self._batches(self.test_ds, False, rank=0, world=1)


class WeightedBatches:
    """DataLoader(batch_size, sampler=WeightedRandomSampler(weights, len(weights))) over device tensors: every epoch
    draws n indices with replacement, probability proportional to ``weights`` (asimow_dataloader.py:123-131)."""

    def __init__(self, tensors, weights, batch_size, seed=0):
        self.tensors = tuple(tensors)
        self.weights = torch.as_tensor(weights, dtype=torch.float64).cpu()
        self.n = len(self.tensors[0])
        if len(self.weights) != self.n:
            raise ValueError(f"{len(self.weights)} sampling weights for {self.n} samples")
        self.batch_size, self.seed, self.epoch = int(batch_size), seed, 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def indices(self):
        g = torch.Generator()
        g.manual_seed(self.seed + self.epoch)
        return torch.multinomial(self.weights, self.n, replacement=True, generator=g)

    def __len__(self):
        return math.ceil(self.n / self.batch_size)

    def __iter__(self):
        idx = self.indices().to(self.tensors[0].device)
        for b in range(len(self)):
            sel = idx[b * self.batch_size:(b + 1) * self.batch_size]
            yield tuple(t.index_select(0, sel) for t in self.tensors)


def class_sampling_weights(labels):
    """1 - ratio for label 0 and ratio for label 1, ratio = mean(labels == 0) (get_sampling_weights,
    asimow_dataloader.py:107-121; arcweld.asimow.sampling_weights on host arrays)."""
    from .asimow import sampling_weights
    return torch.as_tensor(sampling_weights(labels.detach().cpu().numpy()))


@torch.no_grad()
def latent_vectors(vqvae, x, n_cycles, window=200, chunk=4096):
    """x (n, n_cycles*window, C) -> (n, n_cycles, embedding_dim*enc_out_len): window i of every sequence through the
    frozen VQ-VAE's patch_embed -> encoder -> vector_quantization, its z_q (B, embedding_dim, enc_out_len) flattened
    by reshape(B, -1) (create_latent_space_dataset_VQ_VAE, latentspace_dataloader.py:144-203)."""
    n, LT, C = x.shape
    if LT != n_cycles * window:
        raise ValueError(f"sequence length {LT} is not n_cycles * window = {n_cycles} * {window}")
    rows = x.reshape(n * n_cycles, window, C)
    out = []
    for o in range(0, len(rows), chunk):
        z_e = vqvae.encoder(vqvae.patch_embed(rows[o:o + chunk]))
        z_q = vqvae.vector_quantization(z_e)[1]
        out.append(z_q.reshape(z_q.shape[0], -1).float())
    return torch.cat(out).view(n, n_cycles, -1)


class ClassificationDataModule:
    """The classification surface of ASIMoWDataModule(task="classification") / LatentPredDataModule(task=
    "classification") (train_classification_model.py:84-101): ``splits`` = [(x (n, n_cycles*200, 2), labels (n,))]
    for train / val / test.  dataset "asimow" feeds the windows as they are (the GRU reshapes them to
    (B, n_cycles, 400)); "latent_vq_vae" feeds the frozen VQ-VAE's latent vectors (n, n_cycles, in_dim).  The training
    loader samples with replacement by class weight; validation and test are sequential."""

    def __init__(self, splits, batch_size=512, n_cycles=5, dataset="asimow", vqvae=None, seed=0, window=200):
        if dataset not in ("asimow", "latent_vq_vae"):
            raise ValueError(f"Invalid dataset name. {dataset} not supported")
        if dataset == "latent_vq_vae" and vqvae is None:
            raise ValueError("dataset latent_vq_vae needs the frozen VQ-VAE")
        self.splits, self.batch_size, self.n_cycles, self.dataset = splits, batch_size, n_cycles, dataset
        self.vqvae, self.seed, self.window = vqvae, seed, window
        self.ds = None

    @property
    def in_dim(self):
        """Width of one GRU time step: 200*2 raw samples, or embedding_dim * enc_out_len (utils.py:40)."""
        if self.dataset == "asimow":
            return self.window * 2
        return int(self.vqvae.embedding_dim * self.vqvae.enc_out_len)

    def setup(self, stage=None):
        if self.ds is not None:
            return
        self.ds = []
        for x, y in self.splits:
            if self.dataset == "latent_vq_vae":
                x = latent_vectors(self.vqvae, x, self.n_cycles, self.window)
            self.ds.append((x.float(), y.long()))
        self.train_ds, self.val_ds, self.test_ds = self.ds

    def train_dataloader(self):
        return WeightedBatches(self.train_ds, class_sampling_weights(self.train_ds[1]), self.batch_size, self.seed)

    def val_dataloader(self):
        return DeviceBatches(self.val_ds, self.batch_size, shuffle=False, rank=0, world=1)

    def test_dataloader(self):
        return DeviceBatches(self.test_ds, self.batch_size, shuffle=False, rank=0, world=1)
