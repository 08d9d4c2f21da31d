"""The TS2Vec baseline's encoder, eval forward on the device (csrc/ts2vec.hip).

The reference scores its evaluation protocols (fit_knn / fit_lr / fit_svm, here arcweld.retrieve's three probes) on
``TS2Vec.encode(x, encoding_window='full_series')``: the max over time of a dilated-convolution encoder's output
(model/ts2vec/encoder.py, dilated_conv.py of the reference).  This module is that encoder's inference path:

  TSEncoder            an nn.Module with the reference's constructor and parameter names (a reference TSEncoder state
                       dict loads as is); ``encode`` runs the forward on the HIP kernels, f32 throughout
  strip_averaged       the dict ``TS2Vec.save`` writes (an AveragedModel's: 'module.' keys plus 'n_averaged') -> the
                       encoder's own keys;  averaged_state_dict: the way back
  encoder_from_state_dict / load_checkpoint   an encoder whose widths and depth are read from the weights' shapes

The forward, per sequence (B, T, C_in):
  x = input_fc(x) with every row that holds a NaN, or that the mask excludes, zeroed (bias included);
  depth + 1 blocks  y = conv2(gelu(conv1(gelu(x)))) + (projector(x) or x), kernel 3, dilation 2^i, zero padding;
  the last block widens hidden -> output and has the 1x1 projector; dropout is the identity in eval.
Each convolution is one launch over the batch chunk (arcweld.kernels.ts_conv); GELU is applied once per element in the
producing epilogue, the last convolution reduces over time itself for encoding_window='full_series'.

Training (``fit``: the hierarchical contrastive loss, random crops and masks, AdamW, the SWA average) is not built: a
checkpoint written by the reference is the input.  There is no CPU path.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from . import _native as nat

__all__ = ["TSEncoder", "strip_averaged", "averaged_state_dict", "encoder_from_state_dict", "load_checkpoint",
           "MAX_T", "MAX_WIDTH", "MAX_INPUT_DIMS", "MAX_DEPTH", "WORKSPACE_BYTES"]

MAX_T, MAX_WIDTH, MAX_INPUT_DIMS = nat.AW_TS_MAX_T, nat.AW_TS_MAX_WIDTH, nat.AW_TS_MAX_CIN
MAX_DEPTH = nat.AW_TS_MAX_DILATION.bit_length() - 1          # the last block's dilation is 2^depth
WORKSPACE_BYTES = nat.AW_TS_WORKSPACE_BYTES
_MAX_BATCH = nat.AW_TS_MAX_BATCH
_TILE_T, _WG_PER_CU = 128, 2        # csrc/ts2vec.hip: time steps per workgroup (aw_ts_describe), workgroups per CU
_RANDOM_MASKS = ("binomial", "continuous")
_MASKS = ("all_true", "all_false", "mask_last")


class _SamePadConv(nn.Module):
    """A k = 3 convolution with zero padding `dilation` on both sides: the output is as long as the input."""

    def __init__(self, cin, cout, dilation):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, 3, padding=dilation, dilation=dilation)


class _ConvBlock(nn.Module):
    def __init__(self, cin, cout, dilation, final):
        super().__init__()
        self.conv1 = _SamePadConv(cin, cout, dilation)
        self.conv2 = _SamePadConv(cout, cout, dilation)
        self.projector = nn.Conv1d(cin, cout, 1) if cin != cout or final else None


class _DilatedConvEncoder(nn.Module):
    def __init__(self, cin, channels):
        super().__init__()
        self.net = nn.Sequential(*[_ConvBlock(channels[i - 1] if i else cin, c, 2 ** i, i == len(channels) - 1)
                                   for i, c in enumerate(channels)])


def _check_int(v, name, lo):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
        raise ValueError(f"{name}: expected an int >= {lo}, got {v!r}")
    return int(v)


class TSEncoder(nn.Module):
    """The dilated-convolution encoder of TS2Vec: ``TSEncoder(input_dims, output_dims, hidden_dims=64, depth=10)``.

    Parameters carry the reference's names (input_fc.*, feature_extractor.net.<i>.conv1.conv.*, .conv2.conv.*,
    .projector.*), so state dicts move both ways.  What ``encode`` can run: input_dims 1..8, hidden_dims and
    output_dims multiples of 16 up to 512, depth 0..30, T 1..4096 (include/arcweld_amd.h); anything else is a
    ValueError at ``encode``, before any launch."""

    def __init__(self, input_dims, output_dims, hidden_dims=64, depth=10):
        super().__init__()
        self.input_dims = _check_int(input_dims, "input_dims", 1)
        self.output_dims = _check_int(output_dims, "output_dims", 1)
        self.hidden_dims = _check_int(hidden_dims, "hidden_dims", 1)
        self.depth = _check_int(depth, "depth", 0)
        self.input_fc = nn.Linear(self.input_dims, self.hidden_dims)
        self.feature_extractor = _DilatedConvEncoder(self.hidden_dims,
                                                     [self.hidden_dims] * self.depth + [self.output_dims])
        self.repr_dropout = nn.Dropout(p=0.1)                 # the identity in eval; no parameters
        self.workspace_bytes = WORKSPACE_BYTES                # bound of the activation buffers of one batch chunk
        self._pack, self._pack_key = None, None
        self.n_relayouts = 0

    # -------------------------------------------------------------------------------------------- weights
    def _packed(self):
        """The weights as the kernels read them -- every convolution (cout, cin, taps) -> (taps, cout, cin) f32 --,
        re-laid-out when the parameters change (a load, a move to another device), not per call."""
        key = tuple((p.data_ptr(), p._version, str(p.device), p.dtype) for p in self.parameters())
        if self._pack is None or self._pack_key != key:
            def conv(c):
                return (c.weight.detach().float().permute(2, 0, 1).contiguous(), c.bias.detach().float().contiguous())
            blocks = [(conv(b.conv1.conv), conv(b.conv2.conv), conv(b.projector) if b.projector is not None else None)
                      for b in self.feature_extractor.net]
            fc = (self.input_fc.weight.detach().float().contiguous(), self.input_fc.bias.detach().float().contiguous())
            self._pack, self._pack_key = (fc, blocks), key
            self.n_relayouts += 1
        return self._pack

    # -------------------------------------------------------------------------------------------- arguments
    def _check_limits(self, T):
        if not 1 <= self.input_dims <= MAX_INPUT_DIMS:
            raise ValueError(f"input_dims: {self.input_dims} outside 1..{MAX_INPUT_DIMS}, what the encoder kernels hold")
        for nm, v in (("hidden_dims", self.hidden_dims), ("output_dims", self.output_dims)):
            if v % 16 or not 16 <= v <= MAX_WIDTH:
                raise ValueError(f"{nm}: {v} is not a multiple of 16 in 16..{MAX_WIDTH}, what the encoder kernels hold")
        if self.depth > MAX_DEPTH:
            raise ValueError(f"depth: {self.depth} above {MAX_DEPTH} (the last dilation is 2^depth)")
        if not 1 <= T <= MAX_T:
            raise ValueError(f"data: sequence length {T} outside 1..{MAX_T}")

    def _check_mask(self, mask, n, T):
        if mask is None or (isinstance(mask, str) and mask == "all_true"):
            return None
        if isinstance(mask, str):
            if mask in _RANDOM_MASKS:
                raise ValueError(f"mask: the random masks {_RANDOM_MASKS} belong to training and are not built; "
                                 f"expected None, one of {_MASKS} or an (n, T) bool tensor, got {mask!r}")
            if mask not in _MASKS:
                raise ValueError(f"mask: expected None, one of {_MASKS} or an (n, T) bool tensor, got {mask!r}")
            return mask
        m = torch.as_tensor(mask)
        if m.dtype != torch.bool or tuple(m.shape) != (n, T):
            raise ValueError(f"mask: expected None, one of {_MASKS} or a bool tensor of shape {(n, T)}, got {m.dtype} "
                             f"of shape {tuple(m.shape)}")
        return m

    # -------------------------------------------------------------------------------------------- forward
    def _bytes_per_sequence(self, T):
        return 4 * T * (5 * self.hidden_dims + 2 * self.output_dims)

    @torch.no_grad()
    def encode(self, data, mask=None, encoding_window=None, batch_size=None, causal=False, sliding_length=None,
               sliding_padding=0):
        """Representations of ``data`` (n, T, input_dims), a tensor or an array; NaN marks missing samples (a step with
        a NaN in any channel counts as missing).  ``data`` is only read.

        mask: None / 'all_true', 'all_false', 'mask_last', or an (n, T) bool tensor (False = hide the step).
        encoding_window: None -> (n, T, output_dims); 'full_series' -> (n, output_dims), the max over time.
        batch_size: sequences per pass (None: as many as the workspace bound allows); a sequence's result does not
        depend on it.  Returns an f32 tensor on the encoder's device.
        Not built, each a ValueError naming the argument: the random masks, integer and 'multiscale' windows,
        sliding_length (with sliding_padding) and causal."""
        if causal:
            raise ValueError("causal: causal inference belongs to the sliding window and is not built")
        if sliding_length is not None or sliding_padding:
            raise ValueError("sliding_length: sliding-window inference (sliding_length, sliding_padding) is not built")
        if encoding_window is not None and not (isinstance(encoding_window, str) and encoding_window == "full_series"):
            raise ValueError(f"encoding_window: expected None or 'full_series'; integer and 'multiscale' windows are "
                             f"not built, got {encoding_window!r}")
        if batch_size is not None:
            batch_size = _check_int(batch_size, "batch_size", 1)
        if isinstance(data, np.ndarray):
            data = torch.from_numpy(data)
        if not isinstance(data, torch.Tensor) or data.dim() != 3 or not data.is_floating_point():
            raise ValueError(f"data: expected a floating-point (n, T, {self.input_dims}) tensor or array, got "
                             f"{tuple(data.shape) if isinstance(data, torch.Tensor) else type(data).__name__}")
        n, T, C = data.shape
        if C != self.input_dims:
            raise ValueError(f"data: {C} channels, the encoder has input_dims = {self.input_dims}")
        self._check_limits(T)
        mask = self._check_mask(mask, n, T)
        per_seq = self._bytes_per_sequence(T)
        nb = min(int(self.workspace_bytes) // per_seq, _MAX_BATCH, batch_size if batch_size is not None else n)
        if nb < 1 and n:
            raise ValueError(f"data: one sequence of length {T} needs {per_seq} bytes of activations, the workspace "
                             f"bound is {self.workspace_bytes}")

        dev = self.input_fc.weight.device
        if dev.type != "cuda":
            raise nat.NativeError("TSEncoder.encode runs on the HIP kernels: move the encoder to the device "
                                  "(there is no CPU path)")
        # whole rounds of workgroups: a chunk whose hidden-width grid (time tiles x sequences) is a little more than
        # what the device holds at once leaves it nearly empty for the last round, so the chunk shrinks to a multiple
        # of one round (two workgroups per CU: the convolution's launch bounds and LDS).  Results do not depend on it.
        tiles = -(-T // _TILE_T)
        per_round = _WG_PER_CU * torch.cuda.get_device_properties(dev).multi_processor_count
        if nb * tiles > per_round:
            nb = max((nb * tiles // per_round) * per_round // tiles, 1)
        pooled = encoding_window == "full_series"
        Co, H = self.output_dims, self.hidden_dims
        result = torch.empty((n, Co) if pooled else (n, T, Co), dtype=torch.float32, device=dev)
        if n == 0:
            return result
        pack = self._packed()
        ws = torch.empty(nb * per_seq // 4, dtype=torch.float32, device=dev)
        for o in range(0, n, nb):
            m = min(nb, n - o)
            x = data[o:o + m].to(dev, torch.float32).contiguous()
            if isinstance(mask, str):
                mk = torch.ones((m, T), dtype=torch.bool, device=dev)
                if mask == "all_false":
                    mk.zero_()
                else:
                    mk[:, -1] = False
            elif mask is not None:
                mk = mask[o:o + m].to(dev).contiguous()
            else:
                mk = None
            self._forward_chunk(x.view(m * T, C), None if mk is None else mk.view(m * T), m, T, pack, ws,
                                result[o:o + m], pooled)
        return result

    def forward(self, x, mask=None):
        """(B, T, input_dims) -> (B, T, output_dims): ``encode`` with encoding_window None (the eval forward)."""
        return self.encode(x, mask=mask)

    def _forward_chunk(self, x, mask, m, T, pack, ws, result, pooled):
        from . import kernels as k
        (fc_w, fc_b), blocks = pack
        rows, H, Co = m * T, self.hidden_dims, self.output_dims
        hid = [ws[i * rows * H:(i + 1) * rows * H].view(rows, H) for i in range(5)]
        wide = [ws[5 * rows * H + i * rows * Co:5 * rows * H + (i + 1) * rows * Co].view(rows, Co) for i in range(2)]
        X, GX, Hb, Y, GY = hid
        k.ts_input_fc(x, fc_w, fc_b, mask=mask, out=X, out_gelu=GX)
        for i, ((w1, b1), (w2, b2), proj) in enumerate(blocks):
            d, last = 2 ** i, i == len(blocks) - 1
            if not last:
                k.ts_conv(GX, w1, b1, m, T, d, out_gelu=Hb)
                k.ts_conv(Hb, w2, b2, m, T, d, resid=X, out=Y, out_gelu=GY)
                X, Y, GX, GY = Y, X, GY, GX
                continue
            R, H2 = wide
            k.ts_conv(X, proj[0], proj[1], m, T, 1, out=R)                       # the 1x1 projector: one tap
            k.ts_conv(GX, w1, b1, m, T, d, out_gelu=H2)
            if pooled:
                k.ts_conv(H2, w2, b2, m, T, d, resid=R, pool=result)
            else:
                k.ts_conv(H2, w2, b2, m, T, d, resid=R, out=result.view(rows, Co))


# ------------------------------------------------------------------------------------------------ checkpoints
def strip_averaged(state_dict):
    """(encoder state dict, n_averaged) of the dict ``TS2Vec.save`` writes -- torch's AveragedModel: every key prefixed
    'module.', plus 'n_averaged' --; a plain TSEncoder state dict passes through with n_averaged None."""
    n_avg = state_dict.get("n_averaged")
    plain = OrderedDict()
    for key, v in state_dict.items():
        if key == "n_averaged":
            continue
        if n_avg is not None and not key.startswith("module."):
            raise ValueError(f"state_dict: the key {key!r} beside 'n_averaged' lacks the 'module.' prefix")
        plain[key[len("module."):] if key.startswith("module.") else key] = v
    return plain, (int(n_avg) if n_avg is not None else None)


def averaged_state_dict(encoder, n_averaged=1):
    """The encoder's weights under the key names ``TS2Vec.save`` writes: 'n_averaged', then 'module.<name>'."""
    out = OrderedDict(n_averaged=torch.tensor(int(n_averaged), dtype=torch.long))
    for key, v in encoder.state_dict().items():
        out["module." + key] = v
    return out


def encoder_from_state_dict(state_dict, device=None):
    """A TSEncoder built for, and loaded with, a reference state dict (plain or ``TS2Vec.save``'s): input_dims,
    hidden_dims, output_dims and depth are read from the shapes."""
    plain, _ = strip_averaged(state_dict)
    plain = OrderedDict((k, v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v)))
                        for k, v in plain.items())                  # arrays (an .npz of weights) load too
    try:
        hidden, cin = plain["input_fc.weight"].shape
        idx = sorted({int(key.split(".")[2]) for key in plain if key.startswith("feature_extractor.net.")})
        if idx != list(range(len(idx))) or not idx:
            raise KeyError("feature_extractor.net.<i>")
        out = plain[f"feature_extractor.net.{idx[-1]}.conv2.conv.weight"].shape[0]
    except (KeyError, ValueError, IndexError, AttributeError) as e:
        raise ValueError(f"state_dict: not a TS2Vec encoder's ({e})") from None
    enc = TSEncoder(int(cin), int(out), hidden_dims=int(hidden), depth=len(idx) - 1)
    enc.load_state_dict(plain)
    return enc.to(device).eval() if device is not None else enc.eval()


def load_checkpoint(path, device=None):
    """encoder_from_state_dict of the file ``TS2Vec.save`` wrote."""
    return encoder_from_state_dict(torch.load(path, map_location="cpu", weights_only=True), device=device)
