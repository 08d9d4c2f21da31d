"""A restatement of the TS2Vec encoder's eval forward in torch CPU ops, parameterised by dtype: what the HIP kernels
of csrc/ts2vec.hip are held to (float64), and the yardstick of the reference arithmetic's own rounding (float32
against float64).  Written from the semantics stated in include/arcweld_amd.h, not from the kernels:

  a step with a NaN in any channel, or one the mask hides, is zero before and after input_fc (bias included);
  depth + 1 blocks  y = conv2(gelu(conv1(gelu(x)))) + (projector(x) if the block has one else x), exact erf GELU,
  kernel 3, dilation 2^i, zero padding 2^i on both sides; pooled = the max over time.

state dicts carry the reference's key names; `plain` strips the AveragedModel prefix of a saved file.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

MASKS = ("all_true", "mask_last", "all_false", "explicit")


def plain(sd):
    """module.<name> -> <name>, n_averaged dropped; values as torch tensors."""
    out = {}
    for k, v in sd.items():
        if k == "n_averaged":
            continue
        out[k[len("module."):] if k.startswith("module.") else k] = torch.as_tensor(np.asarray(v))
    return out


def n_blocks(sd):
    return 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("feature_extractor.net."))


def mask_of(name, n, T, explicit=None):
    """The (n, T) bool mask of a named mode (True = keep)."""
    m = torch.ones((n, T), dtype=torch.bool)
    if name == "all_false":
        m[:] = False
    elif name == "mask_last":
        m[:, -1] = False
    elif name == "explicit":
        m = torch.as_tensor(np.asarray(explicit)).bool().clone()
    elif name not in (None, "all_true"):
        raise ValueError(name)
    return m


@torch.no_grad()
def encode_ref(sd, x, mask=None, dtype=torch.float64, pooled=False):
    """sd: plain state dict; x (n, T, C) with NaN for missing samples; mask: None or (n, T) bool.
    (n, T, C_out), or (n, C_out) with pooled."""
    p = {k: v.to(dtype) for k, v in plain(sd).items()}
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    keep = ~torch.isnan(x).any(-1)
    if mask is not None:
        keep = keep & torch.as_tensor(np.asarray(mask)).bool()
    x = torch.where(keep[..., None], x, torch.zeros((), dtype=dtype))
    h = x @ p["input_fc.weight"].t() + p["input_fc.bias"]
    h = torch.where(keep[..., None], h, torch.zeros((), dtype=dtype))
    h = h.transpose(1, 2)                                             # (n, C, T)
    for i in range(n_blocks(p)):
        pre, d = f"feature_extractor.net.{i}.", 2 ** i
        res = h
        if pre + "projector.weight" in p:
            res = F.conv1d(h, p[pre + "projector.weight"], p[pre + "projector.bias"])
        u = F.conv1d(F.gelu(h), p[pre + "conv1.conv.weight"], p[pre + "conv1.conv.bias"], padding=d, dilation=d)
        u = F.conv1d(F.gelu(u), p[pre + "conv2.conv.weight"], p[pre + "conv2.conv.bias"], padding=d, dilation=d)
        h = u + res
    out = h.transpose(1, 2).contiguous()
    return out.amax(1) if pooled else out


def seeded_state(input_dims, output_dims, hidden_dims, depth, seed, scale=1.0):
    """A plain state dict with the reference's key names and nn.Linear / nn.Conv1d-like uniform(+-1/sqrt(fan_in))
    values from a seeded generator; the last block (and any block that changes width) has the projector."""
    g = torch.Generator().manual_seed(seed)

    def u(shape, fan_in):
        b = scale / fan_in ** 0.5
        return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1).mul(b).float()

    sd = {"input_fc.weight": u((hidden_dims, input_dims), input_dims), "input_fc.bias": u((hidden_dims,), input_dims)}
    widths = [hidden_dims] * depth + [output_dims]
    cin = hidden_dims
    for i, c in enumerate(widths):
        pre = f"feature_extractor.net.{i}."
        sd[pre + "conv1.conv.weight"], sd[pre + "conv1.conv.bias"] = u((c, cin, 3), 3 * cin), u((c,), 3 * cin)
        sd[pre + "conv2.conv.weight"], sd[pre + "conv2.conv.bias"] = u((c, c, 3), 3 * c), u((c,), 3 * c)
        if cin != c or i == len(widths) - 1:
            sd[pre + "projector.weight"], sd[pre + "projector.bias"] = u((c, cin, 1), cin), u((c,), cin)
        cin = c
    return sd


def error_ratio(got, sd, x, mask=None, pooled=False):
    """(err, e_ref): max |got - restatement_f64| and max |restatement_f32 - restatement_f64| -- the reference
    arithmetic's own rounding on this input, never the kernel's."""
    r64 = encode_ref(sd, x, mask, torch.float64, pooled)
    r32 = encode_ref(sd, x, mask, torch.float32, pooled).double()
    got = torch.as_tensor(np.asarray(got)).double()
    return float((got - r64).abs().max()), float((r32 - r64).abs().max())
