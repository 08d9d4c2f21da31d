"""Latent-token Transformer decoder -- drop-in for model/transformer_decoder.py:13-230 of the reference.

Same constructor, module tree / state_dict keys, initialisation, optimizer groups, task switching, step methods
and log keys.  One opt-in extension: ``pe_len`` (default 512, the reference's hard-coded positional table,
:22-23) sizes the sinusoidal table from its closed form (model/embedding.py:10-18) so that sequences longer than
512 tokens -- the stress configuration's T = 1025 -- can run; at the default the state_dict is the reference's.  forward() runs the fused HIP engine (arcweld.decoder): embedding, the pre-LN blocks (flash-style
causal attention, GEMM epilogues carrying bias/GELU/dropout/residual), ln_f and the task head; the losses are the
HIP cross-entropy kernels.
"""
import math

import torch
from torch import nn

from arcweld import decoder as engine
from arcweld import kernels as K
from arcweld.lightning import LightningModule
from arcweld.optim import RAdam
from model.embedding import LatentEmbedding
from model.transformer_block import Block


def _binary_scores(preds, y):
    """accuracy (multiclass, 2 classes, micro) and binary F1 of predicted labels (torchmetrics semantics)."""
    acc = (preds == y).float().mean()
    tp = ((preds == 1) & (y == 1)).sum().float()
    fp = ((preds == 1) & (y == 0)).sum().float()
    fn = ((preds == 0) & (y == 1)).sum().float()
    den = 2 * tp + fp + fn
    f1 = torch.where(den > 0, 2 * tp / den.clamp_min(1), torch.zeros_like(den))
    return acc, f1


class MyTransformerDecoder(LightningModule):

    def __init__(self, d_model: int = 64, n_classes: int = 131, seq_len: int = 100, n_blocks: int = 2,
                 n_head: int = 6, res_dropout=0.1, att_dropout=0.0, learning_rate: float = 1e-3,
                 class_h_bias: bool = False, class_h_dropout: bool = False, pe_len: int = 512):
        super().__init__()
        self.task = "generate"
        self.learning_rate = learning_rate
        self.betas = (0.9, 0.95)
        self.weight_decay = 0.1
        self.seq_len = seq_len
        self.d_model = d_model
        self.n_head = n_head
        self.n_classes = n_classes
        self.res_dropout = res_dropout
        self.embedding = LatentEmbedding(input_size=n_classes, d_model=d_model, seq_len=int(pe_len))
        self.transformer = nn.ModuleDict(dict(
            drop=nn.Dropout(res_dropout),
            h=nn.ModuleList([Block(d_model=d_model, seq_len=seq_len, n_head=n_head, res_dropout=res_dropout,
                                   att_dropout=att_dropout) for _ in range(n_blocks)]),
            ln_f=nn.LayerNorm(d_model),
        ))
        self.lm_head = nn.Linear(d_model, n_classes, bias=False)
        head = dict(linear_1=nn.Linear(d_model, 1, bias=class_h_bias), activation=nn.GELU(),
                    linear_2=nn.Linear(seq_len, 2, bias=class_h_bias))
        if class_h_dropout:
            head['dropout'] = nn.Dropout(p=0.1)      # registered but never applied (reference :38-39, :127-129)
        self.class_head = nn.ModuleDict(head)
        self.apply(self._init_weights)
        for pn, p in self.named_parameters():
            if pn.endswith('c_proj.weight'):
                torch.nn.init.normal_(p, mean=0.0, std=0.02 / math.sqrt(2 * n_blocks))
        n_params = sum(p.numel() for p in self.transformer.parameters())
        print("number of parameters: %.4fM" % (n_params / 1e6,))
        self.save_hyperparameters()

    def _init_weights(self, module):
        if isinstance(module, nn.Linear):
            torch.nn.init.normal_(module.weight, mean=0.0, std=0.02)
            if module.bias is not None:
                torch.nn.init.zeros_(module.bias)
        elif isinstance(module, nn.Embedding):
            torch.nn.init.normal_(module.weight, mean=0.0, std=0.02)
        elif isinstance(module, nn.LayerNorm):
            torch.nn.init.zeros_(module.bias)
            torch.nn.init.ones_(module.weight)

    def configure_optimizers(self):
        """Two RAdam groups: Linear weights decayed (0.1, L2 as torch.optim.RAdam), everything else not
        (reference :64-114)."""
        decay, no_decay = set(), set()
        for mn, m in self.named_modules():
            for pn, p in m.named_parameters():
                fpn = '%s.%s' % (mn, pn) if mn else pn
                if pn.endswith('bias'):
                    no_decay.add(fpn)
                elif pn.endswith('weight') and isinstance(m, nn.Linear):
                    decay.add(fpn)
                elif pn.endswith('weight') and isinstance(m, (nn.LayerNorm, nn.Embedding)):
                    no_decay.add(fpn)
        param_dict = dict(self.named_parameters())
        assert not (decay & no_decay), "parameters %s made it into both decay/no_decay sets!" % (decay & no_decay,)
        missing = param_dict.keys() - (decay | no_decay)
        assert not missing, "parameters %s were not separated into either decay/no_decay set!" % (missing,)
        groups = [
            {"params": [param_dict[pn] for pn in sorted(decay)], "weight_decay": self.weight_decay},
            {"params": [param_dict[pn] for pn in sorted(no_decay)], "weight_decay": 0.0},
        ]
        return RAdam(groups, lr=self.learning_rate, betas=self.betas)

    def _task_params(self, generate):
        ps = [self.embedding.latent_embedding.weight]
        for mod in list(self.transformer.h) + [self.transformer.ln_f]:
            ps += list(mod.parameters())
        if generate:
            ps.append(self.lm_head.weight)
        else:
            ps += list(self.class_head.parameters())
        return ps

    def active_parameters(self):
        """Parameters that receive a gradient in the current task (the other head is unused: its grad stays None
        under DDP(find_unused_parameters=True), train_transformer_mtasks.py:30)."""
        return self._task_params(self.task == "generate")

    def _next_seed(self):
        """Host part of the dropout seed: fixed per (torch seed, rank).  The per-call variation comes from the
        module's device-side counter (arcweld.vqvae.rng_snapshot), so eager calls and replays of a captured step
        graph draw the same sequence of masks."""
        rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
        return (torch.initial_seed() * 1000003 + 7919 + (rank << 40)) & 0x7FFFFFFFFFFFFFFF

    def forward(self, x, generate: bool = True):
        """ids (B, T) -> logits (B, T, n_classes) [generate] or (B, 2) [classification] (reference :116-131)."""
        B, T = x.size()
        mask_len = self.transformer.h[0].attn.bias.shape[-1] if len(self.transformer.h) else T
        if T > mask_len:
            raise RuntimeError(f"The size of tensor a ({mask_len}) must match the size of tensor b ({T}) at "
                               "non-singleton dimension 3 (causal mask has seq_len rows, transformer_block.py:53)")
        params = tuple(self._task_params(generate))
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return engine.DecoderFunction.apply(self, x, generate, self._next_seed(), *params)
        out, _ = engine.forward(self, x, generate, self.training, need_backward=False, seed=self._next_seed())
        return out

    def _loss_scale_tensor(self, scale, dev):
        """Persistent device scalar holding the loss scale, one per (scale, device) and never freed: the step graphs
        make it before their capture (the captured step has no fill launch for it) and keep reading its address, so a
        later call with another scale gets a tensor of its own instead of replacing one a graph still holds."""
        cache = self.__dict__.setdefault("_gscale", {})
        key = (float(scale), str(dev))
        if key not in cache:
            cache[key] = torch.full((1,), scale, device=dev)
        return cache[key]

    # the captured step may run a whole accumulation group as one batch (fused_train_step(groups=G),
    # arcweld.graphs.StepGraphs)
    grouped_accumulation = True

    @torch.no_grad()
    def fused_train_step(self, batch, scale, mid_hook=None, groups=1):
        """One training micro-step on the kernels without autograd: training_step followed by
        ``(loss * scale).backward()``.  Gradients accumulate into each parameter's ``.grad`` (the flat optimizer
        views when a Trainer installed ``_grad_sink``); ``mid_hook`` runs once backward_late_parameters() are final
        (arcweld.decoder.backward).  groups = G: `batch` is the G micro-batches of an accumulation group concatenated
        along the sequences, each with its own loss mean (arcweld.decoder.fused_step).  Returns the loss."""
        sink = getattr(self, "_grad_sink", None)

        def slot(p):
            if sink is not None and p in sink:
                return sink[p]
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            return p.grad

        loss, logits = engine.fused_step(self, batch, scale, slot, mid_hook=mid_hook, groups=groups)
        if self.task == "generate":
            self.log('train/loss', loss, prog_bar=True)
        else:
            self.log_classification_results(loss, logits, batch[1], "train")
        return loss

    def operand_set(self):
        """The persistent GEMM operand copies of the training step (arcweld.operands), for the optimizer to keep
        current (arcweld.optim.RAdam.attach_operands)."""
        return engine.operand_set(self)

    def backward_late_parameters(self):
        """Parameters whose gradients are final at fused_train_step's mid_hook (the task head, ln_f, the later half
        of the blocks): a data-parallel step all-reduces them while the earlier blocks' backward runs."""
        return engine.late_parameters(self, self.task == "generate")

    def switch_to_generate(self):
        self.task = "generate"

    def switch_to_classification(self):
        self.task = "classification"

    def _step(self, batch):
        if self.task == "generate":
            return self.step_task_gen(batch)
        elif self.task == "classification":
            return self.step_task_class(batch)

    def step_task_gen(self, batch):
        x, _, y = batch
        logits = self(x, generate=True)
        loss = self.loss_gen(logits, y)
        return loss, logits, y

    def step_task_class(self, batch):
        x, cond, _ = batch
        logits = self(x, generate=False)
        loss = self.loss_class(logits, cond)
        return loss, logits, cond

    def log_classification_results(self, loss, logits, y, ds_type):
        preds = logits.argmax(dim=1)         # argmax(log_softmax) == argmax(logits)
        acc, f1score = _binary_scores(preds, y)
        sync_dist = on_epoch = ds_type in ("val", "test")
        self.log(f'{ds_type}/cl/loss', loss, sync_dist=sync_dist, on_epoch=on_epoch)
        self.log(f'{ds_type}/cl/acc', acc, prog_bar=False, sync_dist=sync_dist, on_epoch=on_epoch)
        self.log(f'{ds_type}/cl/f1_score', f1score, prog_bar=True, sync_dist=sync_dist, on_epoch=on_epoch)

    def training_step(self, batch, batch_idx):
        loss, logits, labels = self._step(batch)
        if self.task == "generate":
            self.log('train/loss', loss, prog_bar=True)
        else:
            self.log_classification_results(loss, logits, labels, "train")
        return loss

    def validation_step(self, batch, batch_idx):
        loss, logits, labels = self._step(batch)
        if self.task == "generate":
            self.log('val/loss', loss, prog_bar=True, sync_dist=True)
        else:
            self.log_classification_results(loss, logits, labels, "val")
        return loss

    def test_step(self, batch, batch_idx):
        loss, logits, labels = self._step(batch)
        if self.task == "generate":
            self.log('test/loss', loss, prog_bar=True)
        else:
            self.log_classification_results(loss, logits, labels, "test")
        return loss

    def generate(self, x, do_sample=False, top_k=None, use_cache=True):
        """Autoregressive continuation by seq_len tokens (reference :203-224): greedy (top-1) or multinomial
        sampling, context cropped to the last seq_len tokens.

        use_cache (default): the prompt is prefilled once and each new token is one cached decode step
        (arcweld.decoder.forward_cached, aw_attn_decode); once the context is cropped every position moves, so
        those steps re-prefill the window -- what the reference computes at every step.  use_cache=False runs
        the reference's full recompute through forward()."""
        if use_cache:
            return self._generate_cached(x, do_sample, top_k)
        with torch.no_grad():
            for _ in range(self.seq_len):
                x_cond = x if x.size(1) <= self.seq_len else x[:, -self.seq_len:]
                logits = self(x_cond)
                if top_k is not None:
                    logits = logits.clone()
                    v, _ = torch.topk(logits, top_k)
                    logits[logits < v[:, [-1]]] = -float('Inf')
                probs = torch.softmax(logits, dim=-1)[:, -1]
                if do_sample:
                    idx_next = torch.multinomial(probs, num_samples=1)
                else:
                    _, idx_next = torch.topk(probs, k=1, dim=-1)
                x = torch.cat([x, idx_next], dim=-1)
        return x

    @torch.no_grad()
    def _generate_cached(self, x, do_sample, top_k):
        cache = engine.KVCache(self, x.size(0), self.seq_len)
        filled = 0                      # positions of x[:, :filled] are in the cache
        for _ in range(self.seq_len):
            L = x.size(1)
            if L > self.seq_len:        # cropped window: every position shifted, prefill it again
                logits = engine.forward_cached(self, x[:, -self.seq_len:], cache, 0)
                filled = 0
            elif filled == 0:
                logits = engine.forward_cached(self, x, cache, 0)
                filled = L
            else:
                logits = engine.forward_cached(self, x[:, filled:], cache, filled)
                filled = L
            if top_k is not None:
                v, _ = torch.topk(logits, top_k)
                logits = logits.masked_fill(logits < v[:, [-1]], -float('Inf'))
            probs = torch.softmax(logits, dim=-1)
            if do_sample:
                idx_next = torch.multinomial(probs, num_samples=1)
            else:
                _, idx_next = torch.topk(probs, k=1, dim=-1)
            x = torch.cat([x, idx_next], dim=-1)
        return x

    @torch.no_grad()
    def generate_ids(self, x, n_new, do_sample=False, top_k=None, temperature=1.0, valid_ids=None, seed=0, top_p=None,
                     min_p=None, return_logp=False):
        """ids (B, L0) -> (B, L0 + n_new) int64: n_new tokens appended by one prefill and one cached decode step per
        token, each followed by ONE launch that picks the token (aw_sample_next: column mask, temperature, top-k
        filter, softmax, greedy or multinomial pick) and writes it into the preallocated result -- no torch op per
        token beyond what ``forward_cached`` does.

        valid_ids: only ids < valid_ids can be produced (None: the whole vocabulary); ``valid_ids = n_classes - 2``
        keeps the start and end tokens out, so that every generated id has a codebook row.  temperature divides the
        logits.  do_sample draws from the counter hash of (seed, step, row): the same seed gives the same ids.
        Needs L0 + n_new <= seq_len (the cropped-window re-prefill of ``generate`` is not carried over).  A row
        whose logits hold a NaN or no finite value raises RuntimeError at the end.

        top_p in (0, 1] (nucleus: the fewest most probable ids whose mass reaches top_p) and min_p in [0, 1) (ids with
        at least min_p times the probability of the most likely one) cut the sampled distribution after top_k, in the
        order top_k, min_p, top_p; None is off.  return_logp: returns (ids, {"logp", "logq"}), both (B, n_new) f32:
        logp is each generated id's log-probability under the model over the allowed ids -- no temperature, no
        filter: what ``score_ids(ids, valid_ids)`` gives for it --, logq its log-probability under the distribution it
        was drawn from (0 for greedy).  Any of the three switches the token launch to aw_sample_next_ex, which writes
        straight into those two buffers; without them the call is aw_sample_next's as before."""
        if x.dim() != 2 or x.dtype != torch.int64:
            raise ValueError("generate_ids expects int64 ids of shape (B, L0)")
        B, L0 = x.shape
        n_new = int(n_new)
        if L0 < 1 or n_new < 0 or L0 + n_new > self.seq_len:
            raise ValueError(f"generate_ids: prompt length {L0} + n_new {n_new} must lie in 1..seq_len = {self.seq_len}")
        V = self.n_classes
        n_valid = V if valid_ids is None else int(valid_ids)
        if not 1 <= n_valid <= V:
            raise ValueError(f"generate_ids: valid_ids = {valid_ids} outside 1..n_classes = {V}")
        k = 0 if top_k is None else int(top_k)
        if top_k is not None and not 1 <= k <= n_valid:
            raise ValueError(f"generate_ids: top_k = {top_k} outside 1..{n_valid} allowed ids")
        if not (temperature > 0 and math.isfinite(temperature)):
            raise ValueError(f"generate_ids: temperature must be positive and finite, got {temperature}")
        if top_p is not None and not 0.0 < top_p <= 1.0:
            raise ValueError(f"generate_ids: top_p must lie in (0, 1], got {top_p}")
        if min_p is not None and not 0.0 <= min_p < 1.0:
            raise ValueError(f"generate_ids: min_p must lie in [0, 1), got {min_p}")
        ex = top_p is not None or min_p is not None or return_logp
        out = torch.empty(B, L0 + n_new, dtype=torch.int64, device=x.device)
        out[:, :L0] = x
        lp = {k: torch.empty(B, n_new, device=x.device) for k in ("logp", "logq")} if return_logp else None
        if n_new == 0:
            return (out, lp) if return_logp else out
        bad = torch.zeros(1, dtype=torch.int32, device=x.device)
        cache = engine.KVCache(self, B, self.seq_len)     # as generate(): the same decode launches, the same logits
        for i in range(n_new):
            pos = L0 + i                # the column this step fills
            logits = engine.forward_cached(self, out[:, :L0], cache, 0) if i == 0 else \
                engine.forward_cached(self, out[:, pos - 1:pos], cache, pos - 1)
            if ex:
                K.sample_next_ex(logits, out, pos, bad, n_valid=n_valid, top_k=k,
                                 top_p=1.0 if top_p is None else top_p, min_p=0.0 if min_p is None else min_p,
                                 inv_temperature=1.0 / temperature, do_sample=do_sample, seed=seed, step=i,
                                 logp_out=lp and lp["logp"], logq_out=lp and lp["logq"], col_lp=i)
            else:
                K.sample_next(logits, out, pos, bad, n_valid=n_valid, top_k=k, inv_temperature=1.0 / temperature,
                              do_sample=do_sample, seed=seed, step=i)
        nbad = int(bad.item())
        if nbad:
            raise RuntimeError(f"generate_ids: {nbad} sampling steps met logits with a NaN or no finite value")
        return (out, lp) if return_logp else out

    @torch.no_grad()
    def sample_ids(self, x, n_new, num_samples, top_k=None, temperature=1.0, valid_ids=None, seed=0, top_p=None,
                   min_p=None, return_logp=False):
        """An ensemble of continuations: ids (B, L0) int64 -> (B, N, L0 + n_new) int64, N = num_samples independent
        draws of n_new tokens per prompt; with return_logp also {"logp", "logq"}, each (B, N, n_new) f32, as
        ``generate_ids`` defines them.  Always samples (greedy is ``generate_ids``).  num_samples in 1..32, the fan-out
        limit of aw_beam_gather; every other argument and the length rule L0 + n_new <= seq_len are ``generate_ids``'.

        Sample j of prompt b is row b * N + j of the B * N rows the token launches see, so
        ``sample_ids(x, n_new, N, seed=s, ...)[b, j]`` equals ``generate_ids(x.repeat_interleave(N, 0), n_new,
        do_sample=True, seed=s, ...)[b * N + j]``: the same draw counter step * (B * N) + row.

        ONE prefill on the B prompt rows (not B * N); its logits rows are repeated to B * N once and ONE aw_beam_gather
        launch (W_in = 1, a zero parent table) spreads the prompt's cache of every block over B * N rows of a second
        cache set that shares the operand copies of the weights.  Then per token one cached decode step on B * N rows
        and one aw_sample_next / aw_sample_next_ex launch, both writing into the preallocated result viewed as
        (B * N, ...).  Logits with a NaN or no finite value raise RuntimeError at the end."""
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.int64:
            raise ValueError("sample_ids expects int64 ids of shape (B, L0)")
        B, L0 = x.shape
        n_new = int(n_new)
        if L0 < 1 or n_new < 0 or L0 + n_new > self.seq_len:
            raise ValueError(f"sample_ids: prompt length {L0} + n_new {n_new} must lie in 1..seq_len = {self.seq_len}")
        N = int(num_samples)
        if not 1 <= N <= K.nat.AW_BEAM_MAX_W:
            raise ValueError(f"sample_ids: num_samples = {num_samples} outside 1..{K.nat.AW_BEAM_MAX_W}")
        n_valid = self._n_valid(valid_ids, "sample_ids")
        k = 0 if top_k is None else int(top_k)
        if top_k is not None and not 1 <= k <= n_valid:
            raise ValueError(f"sample_ids: top_k = {top_k} outside 1..{n_valid} allowed ids")
        if not (temperature > 0 and math.isfinite(temperature)):
            raise ValueError(f"sample_ids: temperature must be positive and finite, got {temperature}")
        if top_p is not None and not 0.0 < top_p <= 1.0:
            raise ValueError(f"sample_ids: top_p must lie in (0, 1], got {top_p}")
        if min_p is not None and not 0.0 <= min_p < 1.0:
            raise ValueError(f"sample_ids: min_p must lie in [0, 1), got {min_p}")
        ex = top_p is not None or min_p is not None or return_logp
        dev = x.device
        out = torch.empty(B, N, L0 + n_new, dtype=torch.int64, device=dev)
        out[:, :, :L0] = x[:, None, :]
        lp = {nm: torch.empty(B, N, n_new, device=dev) for nm in ("logp", "logq")} if return_logp else None
        if n_new == 0:
            return (out, lp) if return_logp else out
        rows = out.view(B * N, L0 + n_new)
        lp_rows = {nm: t.view(B * N, n_new) for nm, t in lp.items()} if lp else None
        bad = torch.zeros(1, dtype=torch.int32, device=dev)

        def pick(i, logits):
            if ex:
                K.sample_next_ex(logits, rows, L0 + i, bad, n_valid=n_valid, top_k=k,
                                 top_p=1.0 if top_p is None else top_p, min_p=0.0 if min_p is None else min_p,
                                 inv_temperature=1.0 / temperature, do_sample=True, seed=seed, step=i,
                                 logp_out=lp_rows and lp_rows["logp"], logq_out=lp_rows and lp_rows["logq"], col_lp=i)
            else:
                K.sample_next(logits, rows, L0 + i, bad, n_valid=n_valid, top_k=k, inv_temperature=1.0 / temperature,
                              do_sample=True, seed=seed, step=i)

        prompt = engine.KVCache(self, B, self.seq_len)       # as generate_ids: the same prefill, the same logits
        pick(0, engine.forward_cached(self, x, prompt, 0).repeat_interleave(N, dim=0))
        if n_new > 1:
            cur = engine.KVCache(self, B * N, self.seq_len, share=prompt)
            tab = K.beam_cache_table([prompt.kv, cur.kv])
            K.beam_gather(tab[0], tab[1], B, 1, torch.zeros(B, N, dtype=torch.int32, device=dev), self.seq_len, L0,
                          2 * self.d_model, prompt.T_, bad)
            for i in range(1, n_new):
                pos = L0 + i                                 # the column this step fills
                pick(i, engine.forward_cached(self, rows[:, pos - 1:pos], cur, pos - 1))
        nbad = int(bad.item())
        if nbad:
            raise RuntimeError(f"sample_ids: {nbad} sampling steps met logits with a NaN or no finite value")
        return (out, lp) if return_logp else out

    @torch.no_grad()
    def beam_search_ids(self, x, n_new, num_beams, valid_ids=None, num_return=1):
        """Fixed-length beam search: ids (B, L0) int64 -> {"ids": (B, num_return, L0 + n_new) int64, "scores":
        (B, num_return) f32, "logp": (B, num_return, n_new) f32}, the num_return most probable continuations the search
        found, best first.  logp holds each generated id's log-probability under the model over the allowed ids -- the
        scale of ``score_ids(ids, valid_ids)`` and of ``generate_ids(return_logp=True)`` --, scores its running sum as
        the search accumulated it (the sum of logp up to f32 rounding).

        num_beams in 1..32 beams are kept per sequence, and num_beams * (the number of allowed ids) may not exceed 16384
        (a sequence's candidates are ranked in one workgroup's LDS); 1 <= num_return <= num_beams.  valid_ids and the
        length rule L0 + n_new <= seq_len are those of ``generate_ids``.  Every hypothesis has exactly n_new new ids:
        with ``valid_ids = n_classes - 2`` no end token can be produced, so there is no length penalty and no early
        finish.  Candidates are ranked by score descending, equal scores by the lower (beam, id) pair, so the result is
        the same on every call.  num_beams = 1 returns the ids of greedy ``generate_ids``.  n_new = 0 returns the prompt
        repeated, zero scores and an empty logp.  When fewer than num_return different continuations exist
        (n_valid ** n_new < num_return) the tail carries score -inf (and ids that repeat other rows' prefixes).

        One prefill on B rows, then per token one cached decode step on B * num_beams rows, ONE aw_beam_step launch
        (log-softmax, add the beam scores, keep the best num_beams of num_beams * n_valid candidates, written into
        per-step slabs) and ONE aw_beam_gather launch that reorders all blocks' KV caches by the survivors' parents
        into a second cache set (the two sets swap; the operand copies of the weights are made once and shared); one
        aw_beam_backtrack launch at the end turns the slabs into hypotheses.  No torch op per token beyond
        ``forward_cached``'s own.  Logits with a NaN or no finite value raise RuntimeError at the end."""
        if x.dim() != 2 or x.dtype != torch.int64:
            raise ValueError("beam_search_ids expects int64 ids of shape (B, L0)")
        B, L0 = x.shape
        n_new = int(n_new)
        if L0 < 1 or n_new < 0 or L0 + n_new > self.seq_len:
            raise ValueError(f"beam_search_ids: prompt length {L0} + n_new {n_new} must lie in 1..seq_len = "
                             f"{self.seq_len}")
        n_valid = self._n_valid(valid_ids, "beam_search_ids")
        W, R = int(num_beams), int(num_return)
        if not 1 <= W <= K.nat.AW_BEAM_MAX_W:
            raise ValueError(f"beam_search_ids: num_beams = {num_beams} outside 1..{K.nat.AW_BEAM_MAX_W}")
        if not 1 <= R <= W:
            raise ValueError(f"beam_search_ids: num_return = {num_return} outside 1..num_beams = {W}")
        if W * n_valid > K.nat.AW_SAMPLE_MAX_V:
            raise ValueError(f"beam_search_ids: num_beams * allowed ids = {W} * {n_valid} exceeds the "
                             f"{K.nat.AW_SAMPLE_MAX_V} candidates one workgroup ranks")
        dev = x.device
        ids = x[:, None, :].expand(B, R, L0)
        if n_new == 0:
            return {"ids": ids.contiguous(), "scores": torch.zeros(B, R, device=dev),
                    "logp": torch.empty(B, R, 0, device=dev)}
        out = torch.empty(B, R, L0 + n_new, dtype=torch.int64, device=dev)
        out[:, :, :L0] = ids
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        score = torch.empty(n_new, B, W, device=dev)
        logp = torch.empty(n_new, B, W, device=dev)
        parent = torch.empty(n_new, B, W, dtype=torch.int32, device=dev)
        token = torch.empty(n_new, B, W, dtype=torch.int64, device=dev)
        prompt = engine.KVCache(self, B, self.seq_len)       # as generate_ids: the same prefill, the same logits
        width = 2 * self.d_model

        def step(i, logits, scores_in):
            K.beam_step(logits, scores_in, score[i], parent[i], token[i], logp[i], bad, n_valid=n_valid)

        step(0, engine.forward_cached(self, x, prompt, 0), torch.zeros(B, 1, device=dev))
        if n_new > 1:
            cur, nxt = (engine.KVCache(self, B * W, self.seq_len, share=prompt) for _ in range(2))
            tab = list(K.beam_cache_table([prompt.kv, cur.kv, nxt.kv]))      # built once: three rows of pointers
            K.beam_gather(tab[0], tab[1], B, 1, parent[0], self.seq_len, L0, width, prompt.T_, bad)
            src, dst = 1, 2
            for i in range(1, n_new):
                pos = L0 + i                                 # the column this step fills
                step(i, engine.forward_cached(self, token[i - 1].view(B * W, 1), cur, pos - 1), score[i - 1])
                if i < n_new - 1:
                    K.beam_gather(tab[src], tab[dst], B, W, parent[i], self.seq_len, pos, width, prompt.T_, bad)
                    cur, nxt, src, dst = nxt, cur, dst, src
        lp = torch.empty(B, R, n_new, device=dev)
        K.beam_backtrack(parent, token, logp, out, L0, lp, bad)
        nbad = int(bad.item())
        if nbad:
            raise RuntimeError(f"beam_search_ids: {nbad} steps met logits with a NaN or no finite value")
        return {"ids": out, "scores": score[n_new - 1, :, :R].contiguous(), "logp": lp}

    def _check_scoring(self, x, who):
        """The argument checks of score_ids / score_groups, before any launch."""
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.int64:
            raise ValueError(f"{who} expects int64 ids of shape (B, T)")
        if not 2 <= x.shape[1] <= self.seq_len:
            raise ValueError(f"{who}: sequence length {x.shape[1]} must lie in 2..seq_len = {self.seq_len}")

    def _n_valid(self, valid_ids, who):
        n_valid = self.n_classes if valid_ids is None else int(valid_ids)
        if not 1 <= n_valid <= self.n_classes:
            raise ValueError(f"{who}: valid_ids = {valid_ids} outside 1..n_classes = {self.n_classes}")
        return n_valid

    @torch.no_grad()
    def score_groups(self, x, groups, group_rows, valid_ids=None, who="score_groups"):
        """Teacher-forced scores of ids x (B, T) int64 with groups * group_rows == T - 1: position t predicts
        x[:, t + 1].  One eval forward (its logits stay in the padded buffer, scored in place) and ONE aw_score_rows
        launch; returns {"logp", "entropy" (B, T-1) f32, "rank" (B, T-1) int32, "group_nll" (B, groups) f32}, the last
        the negative log-likelihood summed over each run of group_rows targets.  Raises RuntimeError at the end when a
        row's logits hold a NaN or no finite value, or a target lies outside the allowed ids."""
        self._check_scoring(x, who)
        n_valid = self._n_valid(valid_ids, who)
        B, T = x.shape
        groups, group_rows = int(groups), int(group_rows)
        if groups < 1 or group_rows < 1 or groups * group_rows != T - 1:
            raise ValueError(f"{who}: {groups} groups of {group_rows} targets do not make the T - 1 = {T - 1} targets")
        x = x.contiguous()
        out, _ = engine.forward(self, x, True, False, need_backward=False)
        logits = out.view(B * T, self.n_classes)          # rows of the padded buffer: stride(0) is its ldl
        dev = x.device
        targets = x[:, 1:].contiguous()
        logp, entropy = torch.empty(B, T - 1, device=dev), torch.empty(B, T - 1, device=dev)
        rank = torch.empty(B, T - 1, device=dev, dtype=torch.int32)
        nll = torch.empty(B, groups, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        K.score_rows(logits, targets, T, groups, group_rows, logp, rank, entropy, nll, bad, n_valid=n_valid)
        nbad = int(bad.item())
        if nbad:
            raise RuntimeError(f"{who}: {nbad} positions met logits with a NaN or no finite value, or a target "
                               f"outside the {n_valid} allowed ids")
        return {"logp": logp, "rank": rank, "entropy": entropy, "group_nll": nll}

    @torch.no_grad()
    def score_ids(self, x, valid_ids=None):
        """How well the model explains measured ids: x (B, T) int64, 2 <= T <= seq_len -> {"logp", "entropy" (B, T-1)
        f32, "rank" (B, T-1) int32} of the targets x[:, 1:] (position t predicts x[:, t + 1]).

        logp is the log-probability of the target, entropy that of the predicted distribution, rank the number of
        ids the model prefers to the target (0: greedy ``generate_ids`` would have produced it; ties break low).
        valid_ids: the softmax is renormalised over ids < valid_ids, as ``generate_ids`` restricts its choice (None:
        the whole vocabulary).  One eval forward and one aw_score_rows launch."""
        self._check_scoring(x, "score_ids")
        out = self.score_groups(x, 1, x.shape[1] - 1, valid_ids=valid_ids, who="score_ids")
        del out["group_nll"]
        return out

    def loss_gen(self, logits, labels):
        return engine.cross_entropy(logits.view(-1, logits.size(-1)), labels.view(-1), ignore_index=-1)

    def loss_class(self, logits, labels):
        return engine.cross_entropy(logits, labels)
