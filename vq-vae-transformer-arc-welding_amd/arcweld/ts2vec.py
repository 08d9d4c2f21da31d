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

Training (model.ts2vec.TS2Vec.fit) stands on this module too:

  hierarchical_contrastive_loss, instance_contrastive_loss, temporal_contrastive_loss
                       the reference's losses.py as autograd functions over f32 device tensors, on the fused kernels
                       of csrc/ts2vec_loss.hip: no (2T, 2T) similarity is ever written, the extra memory is O(B T C)
  TSEncoder.train_forward   the differentiable forward on torch ops (F.linear / F.gelu / F.conv1d, autograd) with the
                       random masks; the convolutions' backward on HIP is the follow-up
  take_per_row, split_with_nan, centerize_vary_length_series, draw_crops, swa_update   what ``fit`` is made of
There is no CPU path for ``encode`` or the loss.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _native as nat

__all__ = ["TSEncoder", "strip_averaged", "averaged_state_dict", "encoder_from_state_dict", "load_checkpoint",
           "MAX_T", "MAX_WIDTH", "MAX_INPUT_DIMS", "MAX_DEPTH", "WORKSPACE_BYTES",
           "hierarchical_contrastive_loss", "instance_contrastive_loss", "temporal_contrastive_loss",
           "take_per_row", "split_with_nan", "centerize_vary_length_series", "draw_crops", "swa_update",
           "binomial_mask", "continuous_mask"]

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

    # -------------------------------------------------------------------------------------------- training forward
    def train_forward(self, x, mask="binomial"):
        """The differentiable forward of training, (B, T, input_dims) -> (B, T, output_dims), on torch ops over this
        module's own parameters (any device; autograd gives the backward).  ``x`` is only read.  A step with a NaN in
        any channel, and a step the mask hides, is zero before and after input_fc.  mask: 'binomial' (each step kept
        with probability 1/2, drawn as np.random.binomial(1, 0.5, (B, T))), 'continuous' (5 hidden runs of T // 10
        steps per sequence, starts from np.random.randint), 'all_true', 'all_false', 'mask_last', or a (B, T) bool
        tensor (False = hide); None is 'binomial'.  GELU is the exact erf form; the output passes
        F.dropout(p = self.repr_dropout.p)."""
        w = self.input_fc.weight
        x = torch.as_tensor(x)
        if x.dim() != 3 or x.shape[2] != self.input_dims or not x.is_floating_point():
            raise ValueError(f"x: expected a floating-point (B, T, {self.input_dims}) tensor, got {tuple(x.shape)}")
        x = x.to(w.device, w.dtype)
        B, T = x.shape[:2]
        if mask is None:
            mask = "binomial"
        if isinstance(mask, str):
            if mask == "binomial":
                mk = binomial_mask(B, T)
            elif mask == "continuous":
                mk = continuous_mask(B, T)
            elif mask in _MASKS:
                mk = torch.ones((B, T), dtype=torch.bool)
                if mask == "all_false":
                    mk.zero_()
                elif mask == "mask_last":
                    mk[:, -1] = False
            else:
                raise ValueError(f"mask: expected one of {_RANDOM_MASKS + _MASKS} or a (B, T) bool tensor, got {mask!r}")
        else:
            mk = torch.as_tensor(mask)
            if mk.dtype != torch.bool or tuple(mk.shape) != (B, T):
                raise ValueError(f"mask: expected a bool tensor of shape {(B, T)}, got {mk.dtype} {tuple(mk.shape)}")
        keep = (mk.to(w.device) & ~torch.isnan(x).any(-1)).unsqueeze(-1)
        zero = torch.zeros((), dtype=w.dtype, device=w.device)
        h = F.linear(torch.where(keep, x, zero), w, self.input_fc.bias)
        h = torch.where(keep, h, zero).transpose(1, 2)                       # (B, hidden, T)
        for blk in self.feature_extractor.net:
            d = blk.conv1.conv.dilation[0]
            res = h if blk.projector is None else F.conv1d(h, blk.projector.weight, blk.projector.bias)
            u = F.conv1d(F.gelu(h), blk.conv1.conv.weight, blk.conv1.conv.bias, padding=d, dilation=d)
            u = F.conv1d(F.gelu(u), blk.conv2.conv.weight, blk.conv2.conv.bias, padding=d, dilation=d)
            h = u + res
        return F.dropout(h, p=self.repr_dropout.p, training=True).transpose(1, 2)

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


# ------------------------------------------------------------------------------------------------ training: the loss
class _PairedNCE(torch.autograd.Function):
    """The hierarchy of paired InfoNCE terms (csrc/ts2vec_loss.hip).  ``plan``: 'hierarchy', or the single level-0
    term 'instance' / 'temporal'.  The forward keeps the pooled levels and one lse per row and term; the backward
    recomputes the similarities tile by tile, deepest level first, and every level's gradient is written in one fixed
    launch order (instance, temporal, then the un-pooled deeper gradient): the same bits every run."""

    @staticmethod
    def forward(ctx, z1, z2, alpha, temporal_unit, plan):
        from . import kernels as k
        a, b = z1.detach().contiguous(), z2.detach().contiguous()
        levels, terms, d = [(a, b)], [], 0
        total = torch.zeros((), dtype=torch.float64, device=a.device)

        def term(level, layout, weight):
            u, v = levels[level]
            if weight == 0 or (u.shape[0] if layout == "instance" else u.shape[1]) == 1:
                return                                   # a pair alone in its group: the term is exactly 0
            lse, row_loss = k.nce_rows_fwd(u, v, layout)
            terms.append((level, layout, weight, lse))
            total.add_(row_loss.double().sum(), alpha=weight / row_loss.numel())

        if plan != "hierarchy":
            term(0, plan, 1.0)
            d = 1
        else:
            while levels[-1][0].shape[1] > 1:
                term(len(levels) - 1, "instance", alpha)
                if d >= temporal_unit:
                    term(len(levels) - 1, "temporal", 1 - alpha)
                d += 1
                levels.append(tuple(k.ts_pool2_fwd(t) for t in levels[-1]))
            term(len(levels) - 1, "instance", alpha)
            d += 1
        ctx.levels, ctx.terms, ctx.depth = levels, terms, d
        return (total / d).float()

    @staticmethod
    def backward(ctx, gout):
        from . import kernels as k
        levels, g = ctx.levels, float(gout)
        deeper = None
        for level in range(len(levels) - 1, -1, -1):
            u, v = levels[level]
            du, dv = torch.empty_like(u), torch.empty_like(v)
            written = False
            for lv, layout, weight, lse in ctx.terms:
                if lv == level:
                    k.nce_rows_bwd(u, v, layout, lse, g * weight / (ctx.depth * lse.numel()), du, dv,
                                   accumulate=written)
                    written = True
            if not written:
                du.zero_(), dv.zero_()
            if deeper is not None:
                k.ts_pool2_bwd(u, deeper[0], du)
                k.ts_pool2_bwd(v, deeper[1], dv)
            deeper = (du, dv)
        return deeper[0], deeper[1], None, None, None


def _loss_args(z1, z2, temporal_unit, instance, temporal, who):
    """Everything the kernels would refuse, as a ValueError before the device is looked at or anything is launched."""
    from . import kernels as k
    for nm, z in (("z1", z1), ("z2", z2)):
        if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.dtype != torch.float32:
            raise ValueError(f"{who}: {nm} must be a (B, T, C) float32 tensor, got "
                             f"{(z.dtype, tuple(z.shape)) if isinstance(z, torch.Tensor) else type(z).__name__}")
    if z1.shape != z2.shape:
        raise ValueError(f"{who}: z1 {tuple(z1.shape)} and z2 {tuple(z2.shape)} differ in shape")
    B, T, C = z1.shape
    if B < 1 or T < 1:
        raise ValueError(f"{who}: empty input {tuple(z1.shape)}")
    if C % 16 or not 16 <= C <= k.NCE_MAX_WIDTH:
        raise ValueError(f"{who}: C = {C} is not a multiple of 16 in 16..{k.NCE_MAX_WIDTH}")
    if T * C >= 1 << 22:
        raise ValueError(f"{who}: T * C = {T * C} must stay below 2^22")
    if instance and 2 * B > k.NCE_MAX_ROWS:
        raise ValueError(f"{who}: the instance term has 2 B = {2 * B} rows per group, above {k.NCE_MAX_ROWS}")
    if temporal and 2 * (T >> temporal_unit) > k.NCE_MAX_ROWS:
        raise ValueError(f"{who}: the temporal term has 2 T = {2 * (T >> temporal_unit)} rows per group at its "
                         f"first level, above {k.NCE_MAX_ROWS}")
    if not z1.is_cuda or not z2.is_cuda:
        raise nat.NativeError(f"{who} runs on the HIP kernels: pass device tensors (there is no CPU path)")
    if z1.device != z2.device:
        raise ValueError(f"{who}: z1 and z2 are on different devices")


def hierarchical_contrastive_loss(z1, z2, alpha=0.5, temporal_unit=0):
    """The reference's hierarchical contrastive loss of two views (B, T, C), f32 on the device, differentiable in both:
    at every level of a max-pool pyramid over time (kernel 2, an odd last step dropped) alpha times the instance term
    (across the batch, per step) plus, from level ``temporal_unit`` on, (1 - alpha) times the temporal term (across
    time, per sequence); one more instance term at length 1; the sum divided by the number of levels.  A term whose
    weight is 0 is skipped.  Non-contiguous views are copied.  The sum is accumulated in f64 in a fixed order."""
    alpha, temporal_unit = float(alpha), int(temporal_unit)
    if temporal_unit < 0:
        raise ValueError(f"temporal_unit: expected an int >= 0, got {temporal_unit}")
    _loss_args(z1, z2, temporal_unit, alpha != 0, 1 - alpha != 0, "hierarchical_contrastive_loss")
    return _PairedNCE.apply(z1, z2, alpha, temporal_unit, "hierarchy")


def instance_contrastive_loss(z1, z2):
    """The instance term alone: per time step, each of the 2 B rows against the others, its pair the positive."""
    _loss_args(z1, z2, 0, True, False, "instance_contrastive_loss")
    return _PairedNCE.apply(z1, z2, 1.0, 0, "instance")


def temporal_contrastive_loss(z1, z2):
    """The temporal term alone: per sequence, each of the 2 T rows against the others, its pair the positive."""
    _loss_args(z1, z2, 0, False, True, "temporal_contrastive_loss")
    return _PairedNCE.apply(z1, z2, 1.0, 0, "temporal")


# ------------------------------------------------------------------------------------------------ training: data
def binomial_mask(B, T, p=0.5):
    """(B, T) bool, True = keep, one np.random.binomial draw of the whole array."""
    return torch.from_numpy(np.random.binomial(1, p, size=(B, T))).to(torch.bool)


def continuous_mask(B, T, n=5, l=0.1):
    """(B, T) bool with n runs of l hidden steps per sequence (a float counts in fractions of T); the starts come
    from np.random.randint, sequence by sequence."""
    n = int(n * T) if isinstance(n, float) else n
    l = int(l * T) if isinstance(l, float) else l
    n, l = max(min(n, T // 2), 1), max(l, 1)
    keep = torch.ones((B, T), dtype=torch.bool)
    for i in range(B):
        for _ in range(n):
            t0 = np.random.randint(T - l + 1)
            keep[i, t0:t0 + l] = False
    return keep


def take_per_row(A, indx, num_elem):
    """out[i] = A[i, indx[i] : indx[i] + num_elem]: a window per row, all of one length."""
    cols = torch.as_tensor(np.asarray(indx)).reshape(-1, 1) + torch.arange(num_elem)
    return A[torch.arange(cols.shape[0]).unsqueeze(1), cols]


def split_with_nan(x, sections, axis=0):
    """np.array_split into ``sections`` along ``axis``, the shorter pieces padded at the end with NaN to the length of
    the first."""
    if x.dtype not in (np.float16, np.float32, np.float64):
        raise ValueError(f"split_with_nan: a floating-point array is needed to hold NaN, got {x.dtype}")
    parts = np.array_split(x, sections, axis=axis)
    full = parts[0].shape[axis]
    out = []
    for part in parts:
        pad = [(0, 0)] * x.ndim
        pad[axis] = (0, full - part.shape[axis])
        out.append(np.pad(part, pad, mode="constant", constant_values=np.nan) if pad[axis][1] > 0 else part)
    return out


def centerize_vary_length_series(x):
    """(n, T, C) series padded with all-NaN steps at either end, each rotated so that its valid span is centred."""
    valid = ~np.isnan(x).all(axis=-1)
    lead, trail = np.argmax(valid, axis=1), np.argmax(valid[:, ::-1], axis=1)
    shift = (lead + trail) // 2 - lead
    T = x.shape[1]
    src = (np.arange(T)[None, :] - shift[:, None]) % T
    return np.take_along_axis(x, src[:, :, None], axis=1)


def draw_crops(ts_l, batch, temporal_unit=0):
    """One iteration's crops from np.random in the reference's order -- crop_l, crop_left, crop_eleft, crop_eright,
    then the per-row offsets -- so that a seeded run is replayable.  Returns a dict; view 1 is
    take_per_row(x, offset + eleft, right - eleft)'s last crop_l steps, view 2 take_per_row(x, offset + left,
    eright - left)'s first crop_l: the same crop_l steps of every row."""
    crop_l = int(np.random.randint(low=2 ** (temporal_unit + 1), high=ts_l + 1))
    left = int(np.random.randint(ts_l - crop_l + 1))
    right = left + crop_l
    eleft = int(np.random.randint(left + 1))
    eright = int(np.random.randint(low=right, high=ts_l + 1))
    offset = np.random.randint(low=-eleft, high=ts_l - eright + 1, size=batch)
    return dict(crop_l=crop_l, left=left, right=right, eleft=eleft, eright=eright, offset=offset)


@torch.no_grad()
def swa_update(averaged, current, n_averaged):
    """The running mean of torch's AveragedModel over parameters: avg += (p - avg) / (n_averaged + 1), a copy when
    n_averaged is 0.  Returns n_averaged + 1."""
    for avg, p in zip(averaged.parameters(), current.parameters()):
        if n_averaged == 0:
            avg.copy_(p)
        else:
            avg.add_((p.detach().to(avg.device) - avg) / (n_averaged + 1))
    return n_averaged + 1
