"""Generate tests/golden/ts2vec_{a,b,c}.npz and ts2vec_saved.pt by importing the REFERENCE model/ts2vec/encoder.py
(it needs only torch and numpy; run only where the reference checkout is present, see make_golden.py):

    python tests/golden/make_golden_ts2vec.py

Seeded cases, the reference TSEncoder in eval mode on CPU in fp32:
  a  input_dims 2, hidden 16, output 32, depth 3, T 37, B 3; one all-NaN step and one step with a single NaN channel
  b  input_dims 1, hidden 16, output 16, depth 6, T 20, B 2: the dilations 32 and 64 exceed T
  c  input_dims 3, hidden 32, output 48, depth 2, inputs of T 1 and of T 2 (B 2 each)
Stored per file: the weights under the key names TS2Vec.save writes ('w/module.<name>', 'w/n_averaged'); per input j
'x<j>', 'mask<j>' (the explicit (B, T) mask) and, for each mask of all_true / mask_last / all_false / explicit,
'y<j>/<mask>' (B, T, C_out) and 'pool<j>/<mask>' (B, C_out): the full_series pooling by the expression of the
reference's TS2Vec._eval_with_pooling.  ts2vec_saved.pt is case c's encoder written exactly as TS2Vec.save writes it:
torch.save of the state dict of torch.optim.swa_utils.AveragedModel(net) after one update_parameters.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from make_golden import HERE, REF, save

CASES = {
    "a": dict(cfg=dict(input_dims=2, hidden_dims=16, output_dims=32, depth=3), B=3, Ts=(37,), seed=4101),
    "b": dict(cfg=dict(input_dims=1, hidden_dims=16, output_dims=16, depth=6), B=2, Ts=(20,), seed=4102),
    "c": dict(cfg=dict(input_dims=3, hidden_dims=32, output_dims=48, depth=2), B=2, Ts=(1, 2), seed=4103),
}
MASKS = ("all_true", "mask_last", "all_false", "explicit")


def main():
    sys.path.insert(0, REF)
    from model.ts2vec.encoder import TSEncoder
    for name, case in CASES.items():
        torch.manual_seed(case["seed"])
        net = TSEncoder(**case["cfg"]).eval()
        avg = torch.optim.swa_utils.AveragedModel(net)
        avg.update_parameters(net)
        arrays = {"w/" + k: v.numpy() for k, v in avg.state_dict().items()}
        g = torch.Generator().manual_seed(case["seed"] + 1)
        for j, T in enumerate(case["Ts"]):
            x = torch.randn((case["B"], T, case["cfg"]["input_dims"]), generator=g)
            if name == "a":
                x[0, 5, :] = float("nan")
                x[1, 10, 1] = float("nan")
            explicit = torch.rand((case["B"], T), generator=g) > 0.3
            arrays[f"x{j}"], arrays[f"mask{j}"] = x.numpy().copy(), explicit.numpy().copy()
            for mk in MASKS:
                with torch.no_grad():       # the reference's forward writes into x and into a mask tensor: copies
                    out = avg(x.clone(), explicit.clone() if mk == "explicit" else mk)
                    pool = F.max_pool1d(out.transpose(1, 2), kernel_size=out.size(1)).transpose(1, 2).squeeze(1)
                arrays[f"y{j}/{mk}"], arrays[f"pool{j}/{mk}"] = out.numpy(), pool.numpy()
        save(f"ts2vec_{name}.npz", **arrays)
        if name == "c":
            path = os.path.join(HERE, "ts2vec_saved.pt")
            torch.save(avg.state_dict(), path)
            print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
