"""Generate tests/golden/gru_small.npz by importing the REFERENCE model/gru.py (see make_golden.py for the stub
packages and the rules; run only where the reference checkout is present):

    python tests/golden/make_golden_gru.py

GRU(input_size=3, in_dim=12, hidden_sizes=20, n_hidden_layers=2, output_size=2, dropout_p=0) with the deterministic
state of oracle/gen.py (base WSEED), B = 6 inputs (6, 3, 12) ~ N(0, 1) and labels from oracle/gen.py: forward, cross
entropy, backward, on CPU in fp32.  Stored: logits, loss, every parameter gradient under ``grad/<state-dict name>``,
and the sorted state-dict keys with their shapes (1-D shapes padded with 0).  Inputs are regenerated from the seeds,
so only outputs are stored.
"""
from __future__ import annotations

import numpy as np
import torch

from make_golden import grads_of, install_shim, load_det_state, save
from oracle import gen

WSEED, XSEED, YSEED = 31, 32, 33
CFG = dict(input_size=3, in_dim=12, hidden_sizes=20, n_hidden_layers=2, output_size=2, dropout_p=0.0)
B = 6


def inputs():
    x = gen.normal(XSEED, (B, CFG["input_size"], CFG["in_dim"]), 1.0)
    y = gen.randint(YSEED, (B,), 0, 2)
    return x, y


def main():
    install_shim()
    from model.gru import GRU
    torch.manual_seed(0)
    torch.use_deterministic_algorithms(True)
    m = GRU(**CFG).train()
    load_det_state(m, WSEED)
    x, y = inputs()
    logits = m(torch.from_numpy(x))
    loss = m.loss(logits, torch.from_numpy(y))
    loss.backward()
    sd = m.state_dict()
    keys = sorted(sd)
    shapes = np.zeros((len(keys), 2), dtype=np.int64)
    for i, k in enumerate(keys):
        shapes[i, :sd[k].dim()] = tuple(sd[k].shape)
    save("gru_small.npz", logits=logits.detach().numpy(), loss=loss.detach().numpy(), state_keys=np.array(keys),
         state_shapes=shapes, **grads_of(m))


if __name__ == "__main__":
    main()
