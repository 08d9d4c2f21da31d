"""Generate tests/golden/ts2vec_loss.npz by importing the REFERENCE model/ts2vec/losses.py and utils.py (they need only
torch and numpy; run only where the reference checkout is present, see make_golden.py):

    python tests/golden/make_golden_ts2vec_loss.py

Loss cases 'L<i>', (B, T, C, alpha, temporal_unit) of CASES, seeded f32 inputs on the CPU: 'L<i>/z1', 'L<i>/z2',
'L<i>/cfg' (alpha, temporal_unit), 'L<i>/loss' and the input gradients 'L<i>/dz1', 'L<i>/dz2' of the reference's
hierarchical_contrastive_loss.
Helper cases: 'take/A', 'take/idx', 'take/n', 'take/out';  'split/x', 'split/sections', 'split/out<j>';
'center/x', 'center/out' (series with NaN padding at the left, the right, both ends and none).
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from make_golden import REF, save

CASES = [(3, 7, 16, .5, 0), (2, 70, 16, .5, 0), (1, 5, 16, .5, 0), (2, 1, 16, .5, 0), (3, 33, 16, .3, 2),
         (3, 9, 32, 1, 0), (3, 9, 32, 0, 0)]


def main():
    sys.path.insert(0, REF)
    from model.ts2vec.losses import hierarchical_contrastive_loss
    from model.ts2vec.utils import centerize_vary_length_series, split_with_nan, take_per_row
    arrays = {}
    for i, (B, T, C, alpha, tu) in enumerate(CASES):
        g = torch.Generator().manual_seed(5100 + i)
        scale = 0.5          # similarities of a few units: the reference's own f32 gradients hold 1e-6 of their maximum
        z1 = (torch.randn((B, T, C), generator=g) * scale).requires_grad_(True)
        # a second view that is related to the first but not so close that the softmax saturates (the reference's f32
        # gradients then cancel to a few digits, which is its rounding and no yardstick)
        z2 = (0.5 * z1.detach() + torch.randn((B, T, C), generator=g) * scale).requires_grad_(True)
        loss = hierarchical_contrastive_loss(z1, z2, alpha=alpha, temporal_unit=tu)
        if loss.requires_grad:
            loss.backward()
        zero = torch.zeros((B, T, C))
        arrays[f"L{i}/z1"], arrays[f"L{i}/z2"] = z1.detach().numpy(), z2.detach().numpy()
        arrays[f"L{i}/cfg"] = np.array([alpha, tu], dtype=np.float32)
        arrays[f"L{i}/loss"] = np.float32(loss.item())
        arrays[f"L{i}/dz1"] = (z1.grad if z1.grad is not None else zero).numpy()
        arrays[f"L{i}/dz2"] = (z2.grad if z2.grad is not None else zero).numpy()

    rng = np.random.RandomState(5200)
    A = torch.tensor(rng.randn(4, 12, 2).astype(np.float32))
    idx = np.array([0, 3, 5, 1])
    arrays["take/A"], arrays["take/idx"], arrays["take/n"] = A.numpy(), idx, np.int64(6)
    arrays["take/out"] = take_per_row(A, idx, 6).numpy()

    x = rng.randn(2, 11, 2).astype(np.float32)
    arrays["split/x"], arrays["split/sections"] = x, np.int64(3)
    for j, part in enumerate(split_with_nan(x, 3, axis=1)):
        arrays[f"split/out{j}"] = part

    c = rng.randn(4, 10, 2).astype(np.float32)
    c[0, :3] = np.nan
    c[1, 6:] = np.nan
    c[2, :1] = np.nan
    c[2, 6:] = np.nan
    arrays["center/x"] = c
    arrays["center/out"] = centerize_vary_length_series(c)
    save("ts2vec_loss.npz", **arrays)


if __name__ == "__main__":
    main()
