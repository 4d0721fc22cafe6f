"""Drop-in call surface of the reference's OCRModel / VisionEncoder / AutoRegressiveDecoder for the
``generate()`` hot path, backed by the HIP engine behind the C ABI (include/texocr.h) through the
``torch.ops.texocr.*`` custom operators (texocr_amd/ops.py).

Mirrors (reference file:line):
  OCRModel(encoder, decoder, bos_token, eos_token, trg_pad_idx, device)   model/ocr_model.py:16-32   (an nn.Module)
  OCRModel.generate(src, max_len, temp=0.3)                               model/ocr_model.py:46-66
  model.encoder(src) -> (B, N, D)                                         model/encoder.py:128-152
  model.decoder.generate(start_tokens, eos_tok, max_len, temp, enc=)      model/decoder.py:77-122
  model.decoder.net(x, mask=, enc=) -> (B, t, V)                          model/decoder.py:41-67
  model.decoder.net(x, mask=, enc=, return_attn=True) -> (logits, maps)   model/decoder.py:62-65, model/attention.py:166-178
  create_model(config)                                                    model/ocr_model.py:113-130
  model.state_dict() / model.load_state_dict(reference_state_dict)        key layout: SURVEY.md 8a

The classes are nn.Modules whose parameters carry the reference's names -- including the aliases: ONE LayerNorm
parameter pair is registered under ``layers.{s}.0`` for every sub-layer s of a stack (attention.py:200,221), so
``state_dict()`` has the reference's keys (144 for the default dims) while ``parameters()`` counts each tensor once.
The parameters are the host-visible master copy; the engine keeps its own re-laid-out copy (bf16 or fp32), refreshed
lazily after ``load_state_dict`` (or ``model.sync_weights()`` after editing parameters in place).

Differences that are deliberate and documented:
  * decoding is greedy by default (``decode='greedy'``: argmax; the reference samples with top-k /
    temperature / multinomial -- available as ``decode='sample'``);
  * the decoder is KV-cached; once the output outgrows ``decoder.max_len`` the reference slides its window
    (decoder.py:99-100) and so does this build, by re-running the window through the cached path for every further
    token (exact, slow: window-length engine steps per token);
  * errors are ValueError / RuntimeError, never ``assert``.
There is no CPU path: tensors must live on the GPU and the HIP library must be built.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
import re
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib, guard, ops
from .config import Dims
from .synth import state_dict_layout

_DTYPES = {"fp32": _lib.TXO_F32, "f32": _lib.TXO_F32, "float32": _lib.TXO_F32,
           "bf16": _lib.TXO_BF16, "bfloat16": _lib.TXO_BF16}

_LN_ALIAS = re.compile(r"\.layers\.(\d+)\.0\.(weight|bias)$")


def _is_ln_alias(key: str) -> bool:
    m = _LN_ALIAS.search(key)
    return bool(m) and int(m.group(1)) > 0


def _check_modes(stop: str, decode: str = "greedy") -> None:
    if stop not in ("global", "row"):
        raise ValueError("stop must be 'global' or 'row'")
    if decode not in ("greedy", "sample"):
        raise ValueError("decode must be 'greedy' or 'sample'")


class HipEngine:
    """Owns one txo_engine handle (weights copy, KV caches, workspace) on the current device."""

    def __init__(self, dims: Dims, dtype: str = "fp32", max_batch: int = 64, max_tokens: int = 0):
        if dtype not in _DTYPES:
            raise ValueError(f"dtype must be one of {sorted(_DTYPES)}")
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the texocr_amd engine runs only on an MI355X (no CPU fallback)")
        self.dims, self.dtype = dims, dtype
        # the engine's memory and streams belong to the device that is current NOW; every later call checks its
        # tensors against it and runs with that device current
        self.device = torch.cuda.current_device()
        self.max_batch, self.max_tokens = max_batch, max_tokens or dims.n_pos
        self.handle = None
        self.loaded = False
        self._provider = None            # callable -> reference-layout state dict (set by OCRModel)
        self._stale = False              # the provider's weights are newer than the engine's copy
        self._create()
        self.id = ops.register_engine(self)

    def _create(self) -> None:
        d = self.dims
        ch, cw = d.canvas_hw
        cfg = _lib.TxoConfig(
            canvas_h=ch, canvas_w=cw, embed=1 if d.embed == "hybrid" else 0,
            in_channels=d.in_channels, embed_dim=d.embed_dim,
            enc_heads=d.enc_heads, enc_layers=d.enc_layers, dec_heads=d.dec_heads,
            dec_layers=d.dec_layers, enc_exp=d.enc_exp, dec_exp=d.dec_exp, vocab=d.vocab,
            max_len=d.max_len, bos=d.bos, eos=d.eos, pad=d.pad, dtype=_DTYPES[self.dtype],
            max_batch=self.max_batch, max_tokens=self.max_tokens)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.txo_engine_create(C.byref(cfg), C.byref(h)))
        self.handle = h
        self.loaded = False
        self.token_rules = None                      # (a new handle has no token rules: a set installed by hand goes with the old one)
        self.repeat_guard = None                     # (... and no repeat guard)
        self.alts = 0                                # (... and keeps no alternatives)
        if getattr(self, "_ragged_hybrid", False):   # (a reload of the weights makes a new handle: the switch follows the engine object)
            _lib.check(self.lib.txo_set_ragged_hybrid(h, 1))
        if getattr(self, "_rules_beam", False):
            _lib.check(self.lib.txo_set_rules_beam(h, 1))
        if getattr(self, "_guard_beam", False):
            _lib.check(self.lib.txo_set_guard_beam(h, 1))
        self._env_seen = self._txo_env()             # what the engine saw when it read its knobs

    @staticmethod
    def _txo_env():
        return tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("TXO_")))

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self.lib.txo_engine_destroy(h)
            self.handle = None
        i = getattr(self, "id", None)
        if i is not None:
            ops.unregister_engine(i)

    # ---- weights -------------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, "torch.Tensor | np.ndarray"], strict: bool = True) -> None:
        """Upload a reference-layout state dict (aliased shared-LN keys included; aliases for s > 0 may be omitted).
        Loading again replaces the engine (a handle's weights are immutable once finalized)."""
        want = {k: tuple(s) for k, s, _ in state_dict_layout(self.dims)}
        missing = [k for k in want if k not in sd and not _is_ln_alias(k)]
        unexpected = [k for k in sd if k not in want]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing keys {sorted(set(missing))[:6]}, unexpected keys {unexpected[:6]}")
        arrays = {}
        for k, v in sd.items():
            if k not in want:
                continue
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            a = np.ascontiguousarray(a, dtype=np.float32)
            if tuple(a.shape) != want[k]:
                raise RuntimeError(f"load_state_dict: size mismatch for {k}: got {tuple(a.shape)}, expected {want[k]}")
            arrays[k] = a
        if self.loaded:
            self.lib.txo_engine_destroy(self.handle)
            self.handle = None
            self._create()
        with torch.cuda.device(self.device):
            for k, a in arrays.items():
                shape = (C.c_int64 * a.ndim)(*a.shape)
                _lib.check(self.lib.txo_engine_set_weight(self.handle, k.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))
            _lib.check(self.lib.txo_engine_finalize_weights(self.handle))
        self.loaded = True
        self._stale = False

    def _ensure(self) -> None:
        if (self._stale or not self.loaded) and self._provider is not None:
            self.load_state_dict(self._provider())
        # the engine reads its TXO_* development knobs once, at creation; if the environment changed since the last call (tests
        # flip TXO_PERSIST / TXO_LANES on a live engine) it is told to read them again
        env = self._txo_env()
        if env != self._env_seen and self.handle:
            self.query(_lib.Q_RELOAD_KNOBS)
            self._env_seen = env

    # ---- path (every call goes through a torch.ops.texocr operator) -------------------------------------------------
    def encode(self, img: torch.Tensor) -> torch.Tensor:
        self._ensure()
        return torch.ops.texocr.encode(img, self.id)

    def decode_begin(self, enc: torch.Tensor) -> None:
        self._ensure()
        torch.ops.texocr.decode_begin(enc, self.id)

    def set_key_mask(self, mask: Optional[torch.Tensor]) -> None:
        """Padding mask (B, cols) bool over the positions of the current decode_step session (False = padding); None clears."""
        torch.ops.texocr.decode_set_key_mask(mask, self.id)

    def decode_prefill(self, tokens: torch.Tensor, want_logits: bool = True) -> Optional[torch.Tensor]:
        """All positions of a prefix in one pass (txo_decode_prefill); the K/V cache then holds rows 0..t-1."""
        logits = torch.ops.texocr.decode_prefill(tokens, self.id, bool(want_logits))
        return logits if want_logits else None

    def decode_score(self, tokens: torch.Tensor):
        """Teacher-forced scores of the current session (txo_decode_score): tokens (B, L) -> (logp, top1, top1_logp), each (B, L-1)."""
        return torch.ops.texocr.decode_score(tokens, self.id)

    def decode_attn(self, tokens: torch.Tensor, want_logits: bool = True, want_self: bool = True, want_cross: bool = True,
                    want_mean: bool = False):
        """decode_prefill plus the attention probabilities of every decoder layer (txo_decode_attn) -> (logits (B, t, V), self
        (Ld, B, heads, t, t), cross (Ld, B, heads, t, N), mean (Ld, B, t, N) = cross averaged over the heads); None for a part that
        was not asked for (it is never allocated)."""
        out = torch.ops.texocr.decode_attn(tokens, self.id, bool(want_logits), bool(want_self), bool(want_cross), bool(want_mean))
        return tuple(o if w else None for o, w in zip(out, (want_logits, want_self, want_cross, want_mean)))

    def decode_step(self, t: int, tok_in: Optional[torch.Tensor] = None, want_logits: bool = True):
        batch = ops.session(self, "decode_step").rows
        logits, nxt = torch.ops.texocr.decode_step(tok_in, self.id, int(t), batch, bool(want_logits))
        return (logits if want_logits else None), nxt

    def generate(self, img: Optional[torch.Tensor], max_len: int, eos: Optional[int], enc: Optional[torch.Tensor] = None,
                 return_logits: bool = False, return_logp: bool = False):
        """-> tokens (B, n); with return_logits (tokens, logits); with return_logp (tokens, logp) -- logp (B, n) float32, the
        log-probability of every token under softmax(logits) at temperature 1 over the whole vocabulary, from the token selection
        itself (txo_generate_logp); with both (tokens, logits, logp)."""
        if (img is None) == (enc is None):
            raise ValueError("pass exactly one of img / enc")
        self._ensure()
        o = self._generate_op("" if enc is None else "_from_enc", img if enc is None else enc, max_len, eos, logits=return_logits, logp=return_logp)
        out = (o["toks"],) + ((o["logits"],) if return_logits else ()) + ((o["logp"],) if return_logp else ())
        return out if len(out) > 1 else out[0]

    def _generate_op(self, kind: str, src, max_len: int, eos: Optional[int], *, logits: bool = False, logp: bool = False, prefix=None,
                     prefix_len=None) -> dict:
        """The one place that picks among the nine texocr::generate* ops: by the source (kind "": a (B, C, H, W) tensor; "_from_enc": encoder
        rows; "_ragged": images of different sizes), the prefix and the flags.  -> the op's outputs by name, cut to its n valid columns."""
        head = ops.pack_ragged(src) if kind == "_ragged" else (src,)
        tail = (self.id, int(max_len), -1 if eos is None else int(eos))
        if prefix is not None:
            names, name, args = ("toks", "n", "logp", "plogp"), "generate_prefix" + kind, (*head, prefix, prefix_len, *tail, bool(logp))
        elif kind == "_ragged":
            names, name, args = ("toks", "n", "logp"), "generate_ragged" + ("_logp" if logp else ""), (*head, *tail)
        else:
            names = ("toks", "n", "logp", "logits") if logp else ("toks", "n", "logits")
            name, args = "generate" + kind + ("_logp" if logp else ""), (*head, *tail, bool(logits))
        o = dict(zip(names, getattr(torch.ops.texocr, name)(*args)))
        n = int(o.pop("n").item())
        return {k: v if k == "plogp" else v[:, :n] for k, v in o.items()}

    def generate_prefix(self, src, prefix: torch.Tensor, max_len: int, eos: Optional[int], prefix_len=None,
                        enc: Optional[torch.Tensor] = None, return_logp: bool = False):
        """Prompted decode (txo_generate_prefix / _ragged / _from_enc): the engine's loop continued behind prefix (B, P) int64 -- src a
        (B, C, H, W) tensor or a sequence of (C, H_b, W_b) images, or enc -- with prefix_len (B,) (None: every row has length P).
        -> tokens (B, n), column j of row b the j-th token behind row b's own prefix; with return_logp (tokens, logp (B, n),
        prefix_logp (B, P): the log-probabilities of the forced tokens, 0.0 where the loop forced none)."""
        if (src is None) == (enc is None):
            raise ValueError("pass exactly one of src / enc")
        if prefix_len is not None:
            prefix_len = torch.as_tensor(prefix_len).to(device="cpu", dtype=torch.int32).reshape(-1).contiguous()
        ops.check_prefix(tuple(prefix.shape), prefix_len, max_len, self.dims.max_len, self.max_batch * self.max_tokens)   # before anything changes
        self._ensure()
        kind = "_from_enc" if enc is not None else "" if isinstance(src, torch.Tensor) else "_ragged"
        o = self._generate_op(kind, src if enc is None else enc, max_len, eos, logp=return_logp, prefix=prefix, prefix_len=prefix_len)
        return (o["toks"], o["logp"], o["plogp"]) if return_logp else o["toks"]

    # ---- ragged batches (build extension): images of different sizes in one call; `images` is a sequence of (C, H_b, W_b) tensors, or a
    # container that already exists (ops.PackedImages: what ingest returns) ----
    def ingest(self, images, fit: bool = False, trim=False, regions=None) -> "ops.PackedImages":
        """Device-side image ingest (txo_ingest_u8): raw uint8 images (PIL, numpy, uint8 tensors on the CPU or this device; L, RGB, RGBA) ->
        the container of a ragged batch, in one copy of the pixel bytes and one launch.  Needs no weights.  fit=True (txo_ingest_u8_fit): an
        image beyond the canvas is downscaled on the device to fit it.  trim=(level, margin) (True: the defaults) / regions=(B, 4): a
        rectangle of every image -- its ink and a margin, or the caller's -- takes the image's place first (txo_ingest_u8_view)."""
        if trim is True:
            trim = (ops.TRIM_LEVEL, ops.TRIM_MARGIN)
        return ops.pack_u8(images, self.dims.in_channels, torch.device("cuda", self.device), engine=self.id,
                           fit=self.dims.canvas_hw if fit else None, trim=trim or None, regions=regions)

    def encode_ragged(self, images):
        """-> (enc (B, Ns, D) with zero rows behind each image's own token count, n_tokens (B,) int32 CPU)"""
        self._ensure()
        box, sizes = ops.pack_ragged(images)
        return torch.ops.texocr.encode_ragged(box, sizes, self.id), ops.ragged_tokens(sizes)

    def decode_begin_ragged(self, enc: torch.Tensor, n_tokens: torch.Tensor) -> None:
        self._ensure()
        torch.ops.texocr.decode_begin_ragged(enc, n_tokens, self.id)

    def score_ragged(self, images, tokens: torch.Tensor, mask: Optional[torch.Tensor] = None):
        """txo_score_ragged: images of different sizes, tokens (B, L), mask (B, L) or None -> (logp, top1, top1_logp), each (B, L-1)"""
        self._ensure()
        box, sizes = ops.pack_ragged(images)
        return torch.ops.texocr.score_ragged(box, sizes, tokens, mask, self.id)

    def generate_ragged(self, images, max_len: int, eos: Optional[int], return_logp: bool = False):
        self._ensure()
        # beyond the positional table the window slides through the ragged multi-position forward
        with self.ragged_forward() if int(max_len) > self.dims.max_len else contextlib.nullcontext():
            o = self._generate_op("_ragged", images, max_len, eos, logp=return_logp)
        return (o["toks"], o["logp"]) if return_logp else o["toks"]

    def generate_beam(self, img: torch.Tensor, beams: int, max_len: int, eos: Optional[int], return_beams: bool = False):
        """Beam search (build extension; the reference has none).  Returns the best beam's tokens (B, n), or with
        return_beams=True (tokens (B, beams, n), scores (B, beams)) sorted best first."""
        self._ensure()
        toks, scores, allt, n = torch.ops.texocr.generate_beam(img, self.id, int(beams), int(max_len),
                                                              -1 if eos is None else int(eos), bool(return_beams))
        n = int(n.item())
        if return_beams:
            return allt[:, :n].reshape(img.shape[0], beams, n), scores
        return toks[:, :n]

    def beam_search(self, src, beams: int, max_len: int, eos: Optional[int], return_logp: bool = False, length_alpha: float = 0.0):
        """txo_beam_search (src a (B, C, H, W) tensor) / txo_beam_search_ragged (src a sequence of (C, H_b, W_b) tensors) ->
        (tokens (B, beams, n), scores (B, beams), lengths (B, beams) int32, logp (B, beams, n) or None), best first per image."""
        self._ensure()
        args = (self.id, int(beams), int(max_len), -1 if eos is None else int(eos), bool(return_logp), float(length_alpha))
        if isinstance(src, torch.Tensor):
            B = src.shape[0]
            toks, scores, lengths, logp, n = torch.ops.texocr.beam_search(src, *args)
        else:
            B = len(src)
            box, sizes = ops.pack_ragged(src)
            toks, scores, lengths, logp, n = torch.ops.texocr.beam_search_ragged(box, sizes, *args)
        n = int(n.item())
        return (toks[:, :n].reshape(B, beams, n), scores.reshape(B, beams), lengths.reshape(B, beams),
                logp[:, :n].reshape(B, beams, n) if return_logp else None)

    def set_sampling(self, on: bool, temp: float = 1.0, seed: int = 0, threshold: float = 0.9) -> None:
        """on=True: the reference sampler (top-k with k = int((1 - threshold) * vocab), utils.py:85-91 -- 99 for
        vocab 1000 because of float rounding -- then softmax(/temp) and one multinomial draw, decoder.py:104-108)."""
        self._ensure()
        k = int((1 - threshold) * self.dims.vocab)
        _lib.check(self.lib.txo_set_sampling(self.handle, 1 if on else 0, max(k, 1), float(temp), int(seed) & (2**64 - 1)))

    def set_stop_mode(self, stop: str) -> None:
        """'global': the reference's loop (decoder.py:115-116: rows keep producing tokens after their eos, one break when every row
        contains it).  'row' (build extension): a row is finished at its first eos -- later tokens are the pad id -- and finished rows
        stop costing work on the launch path (txo_set_stop_mode)."""
        _check_modes(stop)
        self._ensure()
        _lib.check(self.lib.txo_set_stop_mode(self.handle, 1 if stop == "row" else 0))

    def set_token_rules(self, rules) -> None:
        """txo_set_token_rules: a texocr_amd.rules.TokenRules (checked on the host first: the same refusals, before the engine is touched), or
        None = off.  While set, every generate from BOS or a prefix picks under the rules, on the launch path; beam search raises unless
        rules_beam is on."""
        self._ensure()
        if rules is None:
            torch.ops.texocr.set_token_rules(None, self.id, 0)
            return
        rules.validate(self.dims.vocab)
        torch.ops.texocr.set_token_rules(torch.from_numpy(rules.table), self.id, rules.depth_max)

    def last_rule_state(self, tokens: torch.Tensor) -> torch.Tensor:
        """(B, 2) int32: the (state, depth) of every row behind the last constrained generate, beside its tokens (B, n)"""
        return torch.ops.texocr.last_rule_state(tokens if tokens.ndim == 2 else tokens[None, :], self.id)

    def set_alternatives(self, k: int) -> None:
        """txo_set_alternatives: k in [1, 8] (checked on the host first, ops.check_alts: the same refusals), or 0 = off.  While set, every
        generate from BOS or a prefix keeps the k best ids / log-probabilities of every row it picks from, on the launch path; beam search raises."""
        self._ensure()
        torch.ops.texocr.set_alternatives(self.id, ops.check_alts(k, self.dims.vocab) if k else 0)

    def last_alternatives(self, tokens: torch.Tensor) -> "Alts":
        """Alts (B, n, k) of the last generate, beside its tokens (B, n)"""
        return Alts(*torch.ops.texocr.last_alternatives(tokens if tokens.ndim == 2 else tokens[None, :], self.id, int(getattr(self, "alts", 0))))

    def decode_score_alts(self, tokens: torch.Tensor, k: int):
        return torch.ops.texocr.decode_score_alts(tokens, self.id, int(k))

    def set_repeat_guard(self, repeat_guard) -> None:
        """txo_set_repeat_guard: (max_period, max_repeats) (checked on the host first, texocr_amd.guard.check: the same refusals), or None =
        off.  While set, every generate from BOS or a prefix picks under the guard, on the launch path; close=True raises there, and beam search raises unless guard_beam is on."""
        self._ensure()
        g = guard.check(repeat_guard, self.dims.vocab)
        torch.ops.texocr.set_repeat_guard(self.id, *(g or (0, 0)))

    @contextlib.contextmanager
    def modes(self, sample: Optional[Tuple[float, Optional[int]]] = None, stop: str = "global", decode: Optional[str] = None, rules=None,
              close: bool = False, repeat_guard=None, alts: int = 0):
        """The engine's global switches around the calls of one generate: sampling with sample = (temp, seed) -- a seed of None is
        drawn from torch's generator; decode='greedy' overrides it --, per-row stop, and token rules (rules=: a TokenRules installed for the
        scope; the set that was installed before, or none, is back behind every exit).  Nothing else in this module turns sampling or the
        per-row stop on, and both are off again behind every exit.  Yields (temp, seed) as set, or None.
        close=True (only with rules=, ValueError otherwise): the closing decode (txo_set_rules_close) for the scope, off again behind it.
        repeat_guard=(max_period, max_repeats): the repeat guard (txo_set_repeat_guard) for the scope; the one set before, or none, is back
        behind every exit.
        alts=k: alternatives per token (txo_set_alternatives) for the scope; the k set before, or 0, is back behind every exit."""
        _check_modes(stop, decode or "greedy")
        if close not in (False, True, 0, 1):
            raise ValueError("close must be False or True")
        if close and rules is None:
            raise ValueError("close=True needs rules=: the closing decode is a budget on top of a rule set")
        if decode == "greedy":
            sample = None
        if sample is not None and sample[1] is None:
            sample = (sample[0], int(torch.randint(0, 2**62, (1,)).item()))
        before = getattr(self, "token_rules", None)                # what ops.set_token_rules recorded: (table, depth_max) or None
        guard_before = getattr(self, "repeat_guard", None)         # what ops.set_repeat_guard recorded: (P, R) or None
        alts_before = getattr(self, "alts", 0)                     # what ops.set_alternatives recorded
        try:
            if alts:
                self.set_alternatives(alts)
            if repeat_guard is not None:
                self.set_repeat_guard(repeat_guard)
            if rules is not None:
                self.set_token_rules(rules)
            if close:                                              # (behind the rules: the engine computes its table here, or refuses)
                torch.ops.texocr.set_rules_close(self.id, True)
            if sample is not None:
                self.set_sampling(True, temp=sample[0], seed=sample[1])
            if stop == "row":
                self.set_stop_mode("row")
            yield sample
        finally:
            if alts:
                torch.ops.texocr.set_alternatives(self.id, alts_before)
            if repeat_guard is not None:
                torch.ops.texocr.set_repeat_guard(self.id, *(guard_before or (0, 0)))
            if sample is not None:
                self.set_sampling(False)
            if stop == "row":
                self.set_stop_mode("global")
            if close:
                torch.ops.texocr.set_rules_close(self.id, False)
            if rules is not None:
                if before is None:
                    torch.ops.texocr.set_token_rules(None, self.id, 0)
                else:
                    torch.ops.texocr.set_token_rules(before[0], self.id, before[1])

    @property
    def ragged_hybrid(self) -> bool:
        """txo_set_ragged_hybrid: ragged batches on the hybrid ResNetV2 front end.  False (the default): every ragged call of a hybrid
        engine raises ValueError naming ragged batches and the hybrid front end, as before the backbone had a ragged form.  True: they run,
        each image's convolutions and GroupNorm statistics bounded by its own extent.  No effect on the patch front end."""
        return getattr(self, "_ragged_hybrid", False)

    @ragged_hybrid.setter
    def ragged_hybrid(self, on) -> None:
        if on not in (False, True, 0, 1):
            raise ValueError("ragged_hybrid must be False or True")
        _lib.check(self.lib.txo_set_ragged_hybrid(self.handle, 1 if on else 0))
        self._ragged_hybrid = bool(on)

    @property
    def rules_beam(self) -> bool:
        """txo_set_rules_beam: beam search under token rules.  False (the default): every beam call raises ValueError while token rules are
        set, as before the search had a constrained form.  True: it runs with the rules inside the beam selection (csrc/beam_rules.h).
        No effect on a beam search without rules."""
        return getattr(self, "_rules_beam", False)

    @rules_beam.setter
    def rules_beam(self, on) -> None:
        if on not in (False, True, 0, 1):
            raise ValueError("rules_beam must be False or True")
        torch.ops.texocr.set_rules_beam(self.id, bool(on))
        self._rules_beam = bool(on)

    @property
    def guard_beam(self) -> bool:
        """txo_set_guard_beam: beam search under a repeat guard.  False (the default): every beam call raises ValueError while a guard is
        set, as before the search had a guarded form.  True: it runs with the ban inside the beam selection (csrc/beam_guard.h).
        No effect on a beam search without a guard."""
        return getattr(self, "_guard_beam", False)

    @guard_beam.setter
    def guard_beam(self, on) -> None:
        if on not in (False, True, 0, 1):
            raise ValueError("guard_beam must be False or True")
        torch.ops.texocr.set_guard_beam(self.id, bool(on))
        self._guard_beam = bool(on)

    def last_beam_rule_state(self, tokens: torch.Tensor) -> torch.Tensor:
        """(B, beams, 2) int32: the (state, depth) of every beam of the last constrained beam search, beside its tokens (B, beams, n)"""
        return torch.ops.texocr.last_beam_rule_state(tokens, self.id)

    def rules_close_dist(self, rules) -> torch.Tensor:
        """txo_rules_close_dist: the closing decode's distance table as the ENGINE computes it for `rules` (installed with the switch on for
        the length of this call) -> (S, depth_max + 1) int32 on the CPU; rules.close_dist(dims.eos) is the host's restatement"""
        with self.modes(rules=rules, close=True):
            return ops.rules_close_dist(self.id, rules.n_states, rules.depth_max)

    @contextlib.contextmanager
    def ragged_forward(self):
        """txo_set_ragged_forward(1) around calls that run the multi-position forward on a ragged session (decode_prefill / decode_score /
        decode_attn / set_key_mask behind decode_begin_ragged) or slide the window of a ragged generate; put back behind every exit.  Outside
        it those calls are refused with a message naming ragged batches, as before the forward had a ragged form."""
        self._ensure()                                             # (a reload of the weights makes a new handle: before the switch, not after)
        before = getattr(self, "_ragged_forward", False)
        _lib.check(self.lib.txo_set_ragged_forward(self.handle, 1))
        self._ragged_forward = True
        try:
            yield
        finally:
            self._ragged_forward = before
            if self.handle:
                _lib.check(self.lib.txo_set_ragged_forward(self.handle, 1 if before else 0))

    @contextlib.contextmanager
    def key_mask(self, mask: Optional[torch.Tensor]):
        """set_key_mask(mask) around the steps of the current session, cleared behind every exit; None or no padding at all: nothing.
        Yields whether a mask was set."""
        on = mask is not None and not bool(mask.all())
        if on:
            self.set_key_mask(mask)
        try:
            yield on
        finally:
            if on:
                self.set_key_mask(None)

    def query(self, what: int) -> int:
        """txo_engine_query, `what` one of _lib.Q_*: LAST_PERSISTENT = the last generate() ran as one persistent launch,
        PERSIST_FALLBACKS = persistent launches that fell back, LAST_ROW_RANGES = row ranges (streams) of the last launch-path decode,
        LAST_LATENT = the last decode's cross attention ran in latent form, RELOAD_KNOBS = (not a question) re-read the TXO_*
        development knobs of generate() from the environment, LAST_COMPACTIONS = live-row compactions of the last generate (stop='row'
        on the launch path), SAMPLE_VOCAB_MAX = the largest vocabulary decode='sample' accepts on this device (set_sampling raises
        ValueError beyond it), LAST_RAGGED = the last generate decoded a ragged batch."""
        out = C.c_int64(0)
        _lib.check(self.lib.txo_engine_query(self.handle, int(what), C.byref(out)))
        return out.value

    # profiling hooks used by bench.py
    def profile(self, on) -> None:
        """0/False off, 1/True full (markers around every encode and step), 2 cross-attention dispatch events only."""
        self._ensure()
        _lib.check(self.lib.txo_profile_enable(self.handle, int(on)))

    def profile_read(self, kind: int):
        ms, n = C.c_double(0), C.c_int64(0)
        _lib.check(self.lib.txo_profile_read(self.handle, kind, C.byref(ms), C.byref(n)))
        return ms.value, n.value


# --------------------------------------------------------------------------------------------------
# parameters in the reference's module tree
# --------------------------------------------------------------------------------------------------
class _Node(nn.Module):
    """A name-only container: the reference's module tree is mirrored for its parameter NAMES."""


def _attach(root: nn.Module, dotted: str, p: nn.Parameter) -> None:
    parts = dotted.split(".")
    m = root
    for name in parts[:-1]:
        if name not in m._modules:
            m.add_module(name, _Node())
        m = m._modules[name]
    m.register_parameter(parts[-1], p)


_NORM_KEY = re.compile(r"(layers\.\d+\.0|\.norm|stem\.1|\.block(_list)?\.[135])\.(weight|bias)$")


def _default_init(key: str, shape, fan_in_of: Dict[str, int], gen: torch.Generator) -> torch.Tensor:
    """torch's default initialisers of the reference's layers (values only matter until load_state_dict)."""
    leaf = key.rsplit(".", 1)[-1]
    if key.endswith(("cls_token", "pos_embed")):
        return torch.zeros(shape)                                            # encoder.py:106-107 (never initialised there)
    if "embedding" in key:
        return torch.randn(shape, generator=gen)                             # nn.Embedding
    if _NORM_KEY.search(key):
        return torch.ones(shape) if leaf == "weight" else torch.zeros(shape)
    fan_in = fan_in_of.get(key[: -len(leaf)] + "weight", 1)
    bound = 1.0 / math.sqrt(max(fan_in, 1))                                  # kaiming_uniform(a=sqrt(5)) and the bias bound
    return (torch.rand(shape, generator=gen) * 2 - 1) * bound


def _build_params(root: nn.Module, dims: Dims, prefix: str, shared: Dict[str, nn.Parameter], device) -> None:
    layout = state_dict_layout(dims)
    fan_in = {k: int(np.prod(s[1:])) for k, s, _ in layout if len(s) > 1}
    gen = torch.Generator().manual_seed(0)
    for key, shape, canon in layout:
        if not key.startswith(prefix):
            continue
        if canon not in shared:
            shared[canon] = nn.Parameter(_default_init(canon, shape, fan_in, gen).to(device), requires_grad=False)
        _attach(root, key[len(prefix):], shared[canon])


# --------------------------------------------------------------------------------------------------
# reference-shaped facades
# --------------------------------------------------------------------------------------------------
class VisionEncoder(nn.Module):
    """model.encoder: callable (B,C,H,W) -> (B, N, D); CLS token at index 0 (encoder.py:128-152)."""

    def __init__(self, engine: HipEngine, _shared: Optional[dict] = None):
        super().__init__()
        self._engine = engine
        d = engine.dims
        self.height, self.width = d.canvas_hw
        self.patch_size = d.patch
        _build_params(self, d, "encoder.", _shared if _shared is not None else {}, torch.device("cuda", engine.device))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._engine.encode(x)

    def forward_ragged(self, images):
        """Build extension: a sequence of (C, H_b, W_b) images of different sizes -> (enc (B, Ns, D), n_tokens (B,) int32 CPU).
        enc[b, :n_tokens[b]] is forward(images[b][None])[0]; the rows behind it are zeros."""
        return self._engine.encode_ragged(images)


def _need_enc(enc) -> None:
    if enc is None:
        raise ValueError("Must provide enc (cross-attending decoder)")       # attention.py:232-233


def _check_x(x: torch.Tensor, shape: str) -> None:
    if x.ndim != 2 or x.dtype != torch.int64 or not x.is_cuda:
        raise ValueError(f"x must be an int64 GPU tensor of shape {shape}")


def _check_token_ids(tokens: torch.Tensor, vocab: int) -> None:
    """The reference's nn.Embedding raises IndexError for an id outside the table (decoder.py:51); so does this facade (the C ABI
    forces such ids into the table instead: it cannot raise from the device)."""
    if tokens.numel() and (int(tokens.min()) < 0 or int(tokens.max()) >= vocab):
        raise IndexError(f"token id outside the vocabulary [0, {vocab})")


def _check_n_tokens(n_tokens, enc: torch.Tensor) -> torch.Tensor:
    """n_tokens of a ragged encoder output enc (B, Ns, D), as VisionEncoder.forward_ragged returns it -> (B,) int32 on the host"""
    n = torch.as_tensor(n_tokens).to(device="cpu", dtype=torch.int32)
    if n.ndim != 1 or n.shape[0] != enc.shape[0]:
        raise ValueError(f"n_tokens must have one entry per row of enc ({enc.shape[0]}), got shape {tuple(n.shape)}")
    if int(n.min()) < 1 or int(n.max()) > enc.shape[1]:
        raise ValueError(f"n_tokens must be in [1, {enc.shape[1]}] (the rows of a slot of enc)")
    return n.contiguous()


@contextlib.contextmanager
def _session(eng, enc: torch.Tensor, n_tokens: Optional[torch.Tensor]):
    """the session on enc around a facade's multi-position calls: fixed shape, or (n_tokens, checked by _check_n_tokens) ragged, with the
    engine's ragged forward switched on for the length of the block"""
    if n_tokens is None:
        eng.decode_begin(enc)
        yield
    else:
        with eng.ragged_forward():
            eng.decode_begin_ragged(enc, n_tokens)
            yield


class Alts(NamedTuple):
    """Alternatives per token (build extension): ids (B, n, k) int32 and logp (B, n, k) float32.  ids[b, t] are the k largest entries of the
    logits row token t of row b was picked from, in descending value, the lower id first among equals (a stable descending sort: ids[..., 0]
    is the greedy pick); logp = log_softmax(row)[ids], temperature 1 over the whole vocabulary.  Always the RAW model's row: not the
    sampler's top-k / temperature distribution, not masked by rules=, close=True or repeat_guard= -- under a sampled, constrained or guarded
    decode the committed token may be missing from its own alternatives, which is how a caller sees that a rule forced it.  Where tokens /
    logp hold pad / 0.0 (behind a row's eos under stop='row', columns a longer-prefix row never reached) so do ids / logp."""
    ids: torch.Tensor
    logp: torch.Tensor


def _squeeze0(o):
    return Alts(o.ids.squeeze(0), o.logp.squeeze(0)) if isinstance(o, Alts) else o.squeeze(0)


def _append_alts(eng, out, k: int):
    """a generate's result with the Alts of the call behind it (k = 0: the result as it is)"""
    if not k:
        return out
    out = out if isinstance(out, tuple) else (out,)
    return (*out, eng.last_alternatives(out[0]))


class Score(NamedTuple):
    """What AutoRegressiveDecoder.score / OCRModel.score return (position p of row b scores the target trg[b, p + 1]):
    logp (B, L-1) log-probability of the target; top1 (B, L-1) arg-max of the logits; top1_logp (B, L-1) its log-probability;
    valid (B, L-1) bool, both the fed token and its target are not padding; nll (B,) -sum of logp over valid; loss (0-dim) sum of
    nll / number of valid positions; token_acc (0-dim) share of valid positions whose top1 is the target.  Values of logp / top1 /
    top1_logp outside `valid` are unspecified."""
    logp: torch.Tensor
    top1: torch.Tensor
    top1_logp: torch.Tensor
    valid: torch.Tensor
    nll: torch.Tensor
    loss: torch.Tensor
    token_acc: torch.Tensor


def score_summary(logp: torch.Tensor, top1: torch.Tensor, top1_logp: torch.Tensor, trg: torch.Tensor, mask: torch.Tensor) -> Score:
    """The arithmetic on top of the engine's three arrays (plain torch, any device): trg (B, L) tokens, mask (B, L) bool (False =
    padding).  Sums run in float64 and come back as float32; with no valid position loss and token_acc are nan."""
    mask = mask.to(device=logp.device, dtype=torch.bool)
    valid = mask[:, :-1] & mask[:, 1:]
    n = valid.sum()
    nll64 = -(torch.where(valid, logp, torch.zeros_like(logp)).double().sum(dim=1))
    hit = (top1 == trg[:, 1:].to(top1.device)) & valid
    return Score(logp, top1, top1_logp, valid, nll64.float(), (nll64.sum() / n).float(), (hit.sum().double() / n).float())


class _BeamFields(NamedTuple):
    tokens: torch.Tensor
    scores: torch.Tensor
    lengths: torch.Tensor
    logp: Optional[torch.Tensor]


class Beams(_BeamFields):
    """What OCRModel.beam_search returns, the beams of every image best first: tokens (B, beams, n) int64; scores (B, beams) the sum of a
    beam's log-probabilities; lengths (B, beams) int32, the index of the beam's first eos + 1, or n without one; logp (B, beams, n)
    float32 or None, the log-probability of every token at the beam's own prefix -- the floats the search summed, left to right, into
    scores.  Behind a beam's length tokens hold eos and logp holds 0.
    rule_state, the last field: (B, beams, 2) int32 under rules= (with OCRModel.rules_beam on), every beam's (state, depth) behind its last
    token that counts -- its first eos, or n --, and None without rules.  It is read by name: as a tuple a Beams stays the four fields
    above, so code that unpacks or iterates one keeps working.
    Under rules= an image may have fewer than `beams` allowed sequences: the surplus beams are DEAD -- score -inf -- and outside every
    guarantee: their tokens, lengths and rule_state are unspecified.  Look at scores before anything else of a beam."""
    rule_state: Optional[torch.Tensor] = None

    def __new__(cls, tokens, scores, lengths, logp, rule_state=None):
        self = super().__new__(cls, tokens, scores, lengths, logp)
        self.rule_state = rule_state
        return self


def check_beam_args(beams, max_len, length_alpha, n_images: int, table: int, max_batch: int) -> None:
    """OCRModel.beam_search's refusals, before the engine is touched (ValueError): beams in [1, 8], max_len inside the positional table,
    a finite length_alpha >= 0, images * beams within the engine's max_batch"""
    if isinstance(beams, bool) or not isinstance(beams, int) or not 1 <= beams <= 8:
        raise ValueError(f"beam search needs beams in [1, 8], got {beams!r}")
    if isinstance(max_len, bool) or not isinstance(max_len, int) or max_len < 1:
        raise ValueError(f"beam search needs max_len >= 1, got {max_len!r}")
    if max_len > table:
        raise ValueError(f"beam search needs max_len <= decoder.max_len ({table})")
    if table > 1024:
        raise ValueError(f"beam search needs decoder.max_len <= 1024, this decoder has {table}")
    if isinstance(length_alpha, bool) or not isinstance(length_alpha, (int, float)) or not math.isfinite(length_alpha) or length_alpha < 0:
        raise ValueError(f"beam search needs a finite length_alpha >= 0, got {length_alpha!r}")
    if n_images < 1:
        raise ValueError("beam search needs at least one image")
    if n_images * beams > max_batch or n_images * beams > 32767:
        raise ValueError(f"beam search needs images * beams <= the engine's max_batch ({min(max_batch, 32767)}), got {n_images} * {beams}")


class Alignment(NamedTuple):
    """What OCRModel.align / AutoRegressiveDecoder.align return -- where in the image every fed position looked (position p of row b is
    the one that predicts trg[b, p + 1]): maps, the head-mean cross attention on the encoder's patch rows, (B, L-1, H/16, W/16) from
    OCRModel.align and (B, L-1, N-1) from the decoder's; cls (B, L-1) the mass on the CLS row; peak (B, L-1, 2) the arg-max patch as
    (row, col) -- (B, L-1) flat patch indices from the decoder's.  maps[b, p].sum() + cls[b, p] is 1.  Rows of padded positions are
    unspecified."""
    maps: torch.Tensor
    cls: torch.Tensor
    peak: torch.Tensor


def alignment(cross_mean: torch.Tensor, layer: Optional[int] = -1, grid: Optional[Tuple[int, int]] = None) -> Alignment:
    """The arithmetic on top of the engine's head-mean maps (plain torch, any device): cross_mean (Ld, B, t, N) with the CLS row at key 0;
    layer: which decoder layer, None = the mean over the layers; grid = (rows, cols) of the patch grid, None leaves the patches flat."""
    m = cross_mean.mean(dim=0) if layer is None else cross_mean[layer]
    cls, maps = m[..., 0], m[..., 1:]
    peak = maps.argmax(dim=-1)
    if grid is not None:
        maps = maps.reshape(*maps.shape[:2], *grid)
        peak = torch.stack((peak // grid[1], peak % grid[1]), dim=-1)
    return Alignment(maps, cls, peak)


def alignment_ragged(cross_mean: torch.Tensor, n_tokens: Sequence[int], layer: Optional[int] = -1,
                     grids: Optional[Sequence[Tuple[int, int]]] = None) -> List[Alignment]:
    """alignment() per image of a ragged session: cross_mean (Ld, B, t, Ns), image b owns the keys 0 .. n_tokens[b]-1 of row b (the engine
    writes zeros behind them; they are cut off, not looked at) -> B Alignments with a leading dimension of 1, element b over image b's own
    n_b - 1 patches, on the grid grids[b] = (h_b, w_b) if given."""
    n = [int(v) for v in n_tokens]
    if len(n) != cross_mean.shape[1] or (grids is not None and len(grids) != len(n)):
        raise ValueError("n_tokens / grids must have one entry per image")
    for b, nb in enumerate(n):
        if grids is not None and 1 + int(grids[b][0]) * int(grids[b][1]) != nb:
            raise ValueError(f"grids[{b}] = {tuple(grids[b])} does not hold the {nb - 1} patches of image {b}")
    return [alignment(cross_mean[:, b:b + 1, :, :nb], layer, None if grids is None else (int(grids[b][0]), int(grids[b][1])))
            for b, nb in enumerate(n)]


class Transformer(nn.Module):
    """model.decoder.net: (B,t) int64 tokens -> (B,t,V) logits over the whole prefix (decoder.py:41-67): ONE causal
    multi-position pass (txo_decode_prefill), which also leaves the K/V cache filled for the positions given."""

    def __init__(self, engine: HipEngine, _shared: Optional[dict] = None):
        super().__init__()
        self._engine = engine
        self.max_len = engine.dims.max_len
        _build_params(self, engine.dims, "decoder.net.", _shared if _shared is not None else {}, torch.device("cuda", engine.device))

    def forward(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None, enc: Optional[torch.Tensor] = None, **kw):
        """return_attn=True: (logits, attn_maps) as the reference returns them (decoder.py:62-65): the post-softmax attention of every
        block in stack order -- self 0, cross 0, self 1, cross 1, ... -- each (B, heads, t, keys), views into two buffers.
        n_tokens= (build extension): enc is a ragged encoder output (B, Ns, D) and n_tokens its valid rows per image, both as
        VisionEncoder.forward_ragged returns them; row b is what the call gives on enc[b:b+1, :n_tokens[b]], and the cross maps are
        (B, heads, t, Ns) with exact zeros behind an image's own keys."""
        return_attn = bool(kw.pop("return_attn", False))
        n_tokens = kw.pop("n_tokens", None)
        if kw:
            raise ValueError(f"unsupported arguments for the inference path: {sorted(kw)}")
        _need_enc(enc)
        if n_tokens is not None:
            n_tokens = _check_n_tokens(n_tokens, enc)
        padded = mask is not None and not bool(mask.all())
        if padded and tuple(mask.shape) != tuple(x.shape):
            raise ValueError("mask must have the shape of x")
        _check_x(x, "(B, t)")
        if x.shape[1] > self.max_len:
            raise ValueError("prefix longer than decoder.max_len")
        eng = self._engine
        _check_token_ids(x, eng.dims.vocab)
        # the one-pass prefill (csrc/prefill.h, with or without a key mask) needs a vocabulary that is a multiple of 8 and a prefix that
        # fits the engine's workspace (max_batch * max_tokens rows); anything else takes the single-position steps
        one_pass = eng.dims.vocab % 8 == 0 and x.shape[1] <= eng.max_batch * eng.max_tokens and os.environ.get("TXO_NET_STEPWISE") is None
        # attention.py:130-155: a padded position is never attended by a query that is not padding.  Logits AT padded positions are
        # unspecified here (the reference softmaxes such a row uniformly over all keys, future ones included; nothing reads it)
        with _session(eng, enc, n_tokens), eng.key_mask(mask.to(x.device) if padded else None):
            if not return_attn:
                return eng.decode_prefill(x) if one_pass else self._net_stepwise(x)
            # (the maps need no logits: a vocabulary the one-pass logits cannot take gets them from the stepwise route behind)
            logits, self_p, cross_p, _ = eng.decode_attn(x, want_logits=one_pass)
            if not one_pass:
                logits = self._net_stepwise(x)
        return logits, [m[l] for l in range(self_p.shape[0]) for m in (self_p, cross_p)]

    def _net_stepwise(self, x: torch.Tensor) -> torch.Tensor:
        """fallback (odd vocabulary sizes; tests): one cached step per position"""
        eng = self._engine
        out = torch.empty((x.shape[0], x.shape[1], eng.dims.vocab), device=x.device, dtype=torch.float32)
        xt = x.t().contiguous()
        for t in range(x.shape[1]):
            out[:, t] = eng.decode_step(t, xt[t])[0]
        return out


class AutoRegressiveDecoder(nn.Module):
    """model.decoder (decoder.py:70-122)."""

    def __init__(self, engine: HipEngine, _shared: Optional[dict] = None):
        super().__init__()
        self._engine = engine
        self.net = Transformer(engine, _shared)
        self.max_len = self.net.max_len

    def forward(self, *a, **k):
        raise NotImplementedError("AutoRegressiveDecoder.forward is the training loss (decoder.py:124-145); this engine "
                                  "implements the generate() inference path only")

    @torch.no_grad()
    def score(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None, enc: Optional[torch.Tensor] = None,
              n_tokens: Optional[torch.Tensor] = None, alts: int = 0):
        """alts=k (build extension, 1..8): -> (Score, Alts), the k best ids / log-probabilities of every scored row (B, L-1, k) from the same
        fused kernel (the logits are still never stored); Alts.ids[..., 0] is Score.top1 and Alts.logp[..., 0] Score.top1_logp bit for bit, and
        every Score field is bit for bit what the call without alts= returns.  Not with n_tokens= (ValueError).
        The quantity forward() trains on, for inference (decoder.py:124-145 without autograd): x (B, L) int64 target sequences
        (bos first), x[:, :-1] is fed in one causal pass and x[:, 1:] are the targets.  mask (B, L) bool, False = padding (None: no
        padding).  The logits are never materialised (csrc/score.h).  Unlike the reference's loss, `loss` averages over the valid
        positions only (F.cross_entropy there has no ignore_index); without padding the two are the same number.
        n_tokens= (build extension): enc / n_tokens as VisionEncoder.forward_ragged returns them; row b scores against image b's own rows."""
        _need_enc(enc)
        if alts:
            ops.check_alts(alts, self._engine.dims.vocab)
            if n_tokens is not None:
                raise ValueError("alts= is not available with n_tokens= (alternatives are not kept on a ragged scoring pass)")
        if n_tokens is not None:
            n_tokens = _check_n_tokens(n_tokens, enc)
        _check_x(x, "(B, L)")
        if x.shape[1] < 2:
            raise ValueError("x needs at least two columns (one fed token and its target)")
        if x.shape[1] - 1 > self.max_len:
            raise ValueError("sequence longer than decoder.max_len + 1")
        if mask is not None and tuple(mask.shape) != tuple(x.shape):
            raise ValueError("mask must have the shape of x")
        eng = self._engine
        _check_token_ids(x, eng.dims.vocab)
        m = torch.ones_like(x, dtype=torch.bool) if mask is None else mask.to(device=x.device, dtype=torch.bool)
        with _session(eng, enc, n_tokens), eng.key_mask(m[:, :-1]):   # (the last column is a target only, never a key)
            if alts:
                logp, top1, top1_logp, ids, alp = eng.decode_score_alts(x, alts)
                return score_summary(logp, top1, top1_logp, x, m), Alts(ids, alp)
            logp, top1, top1_logp = eng.decode_score(x)
        return score_summary(logp, top1, top1_logp, x, m)

    @torch.no_grad()
    def align(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None, enc: Optional[torch.Tensor] = None, layer: Optional[int] = -1,
              grid: Optional[Tuple[int, int]] = None, n_tokens: Optional[torch.Tensor] = None,
              grids: Optional[Sequence[Tuple[int, int]]] = None):
        """Build extension: where every position of a teacher-forced pass looked.  x (B, L) and mask as score() takes them; x[:, :-1] is
        fed in one causal pass that returns only the head mean of the cross-attention maps (the per-head tensors are never made).
        layer: the decoder layer (-1 = the last), None = the mean over the layers.  -> Alignment over the N - 1 patch rows of enc.
        n_tokens= (build extension): enc / n_tokens as VisionEncoder.forward_ragged returns them -> a list of B Alignments (leading
        dimension 1), element b over image b's own n_b - 1 patches, on grids[b] = (h_b, w_b) if grids is given (alignment_ragged)."""
        _need_enc(enc)
        if n_tokens is not None:
            n_tokens = _check_n_tokens(n_tokens, enc)
            if grids is not None and len(grids) != n_tokens.shape[0]:
                raise ValueError("grids must have one (rows, cols) per image")
        elif grids is not None:
            raise ValueError("grids belongs to a ragged encoder output (pass n_tokens); a fixed-shape call takes grid")
        _check_x(x, "(B, L)")
        if x.shape[1] < 2:
            raise ValueError("x needs at least two columns (one fed token and its target)")
        if x.shape[1] - 1 > self.max_len:
            raise ValueError("sequence longer than decoder.max_len + 1")
        if mask is not None and tuple(mask.shape) != tuple(x.shape):
            raise ValueError("mask must have the shape of x")
        eng = self._engine
        if layer is not None and not -eng.dims.dec_layers <= layer < eng.dims.dec_layers:
            raise ValueError(f"layer must be None or in [{-eng.dims.dec_layers}, {eng.dims.dec_layers})")
        _check_token_ids(x, eng.dims.vocab)
        with _session(eng, enc, n_tokens), eng.key_mask(None if mask is None else mask.to(device=x.device, dtype=torch.bool)[:, :-1]):
            mean = eng.decode_attn(x[:, :-1].contiguous(), want_logits=False, want_self=False, want_cross=False, want_mean=True)[3]
        if n_tokens is not None:
            return alignment_ragged(mean, n_tokens.tolist(), layer, grids)
        return alignment(mean, layer, grid)

    @torch.no_grad()
    def generate(self, start_tokens: torch.Tensor, eos_tok: Optional[int], max_len: int, temp: float = 1.0,
                 decode: str = "greedy", generator: Optional[torch.Generator] = None, seed: Optional[int] = None,
                 **kwargs) -> torch.Tensor:
        enc = kwargs.pop("enc", None)
        mask = kwargs.pop("mask", None)
        return_logits = bool(kwargs.pop("return_logits", False))   # build extension: also the logits every token was picked from
        # build extension: also logp (B, n) float32 = log_softmax(logits)[token] of every position, temperature 1 over the whole vocabulary in
        # greedy and sampled decode alike, 0 behind a row's first eos with stop='row'; with return_logits: (tokens, logits, logp)
        return_logp = bool(kwargs.pop("return_logp", False))
        stop = kwargs.pop("stop", "global")                        # build extension: 'row' = per-row stop, pad behind a row's first eos
        pad = kwargs.pop("pad", None)
        # build extension: (B,) lengths of the rows of start_tokens (columns at and behind a row's length are never read); the result's
        # column j of row b is then the j-th token behind row b's own start.  Needs the engine's prompted loop (see below).
        prefix_len = kwargs.pop("prefix_len", None)
        # build extension: a texocr_amd.rules.TokenRules the loop picks under (installed for this call); the result gains rule_state (B, 2)
        # int32 as its last element.  Needs the engine's own loop: a BOS start or the prompted route, not the stepwise one.
        rules = kwargs.pop("rules", None)
        close = kwargs.pop("close", False)                         # build extension, with rules=: the closing decode (OCRModel.generate)
        # build extension: (max_period, max_repeats), the repeat guard (OCRModel.generate).  Needs the engine's own loop, like rules=
        repeat_guard = kwargs.pop("repeat_guard", None)
        # build extension: k in [1, 8], an Alts (B, n, k) of the k best ids / log-probabilities behind every token, appended to the result directly
        # before rule_state where there is one and last otherwise.  Needs the engine's own loop inside the positional table, like rules=
        return_alts = kwargs.pop("return_alts", 0)
        rstate = alts = None
        if kwargs:
            raise ValueError(f"unsupported arguments: {sorted(kwargs)}")
        _need_enc(enc)
        if return_alts:
            ops.check_alts(return_alts, self._engine.dims.vocab)
        if mask is not None and mask.ndim == 1:
            mask = mask[None, :]
        padded = mask is not None and not bool(mask.all())
        if padded and tuple(mask.shape) != tuple(start_tokens.shape if start_tokens.ndim == 2 else start_tokens[None, :].shape):
            raise ValueError("mask must have the shape of start_tokens")
        squeeze = start_tokens.ndim == 1
        st = start_tokens[None, :] if squeeze else start_tokens                  # decoder.py:88
        B, T0 = st.shape
        eng = self._engine
        if prefix_len is not None:                                 # (columns at and behind a row's length are never read: nor checked)
            if padded:
                raise ValueError("prefix_len is not available with a padding mask")
            prefix_len = torch.as_tensor(prefix_len).to(device="cpu", dtype=torch.int32).reshape(-1)
            ops.check_prefix(tuple(st.shape), prefix_len, max_len, self.max_len, eng.max_batch * eng.max_tokens)
        _check_token_ids(_inside_lengths(st, prefix_len, 0), eng.dims.vocab)
        if seed is None and generator is not None:
            seed = generator.initial_seed()
        # A start that is not the single BOS column continues in the ENGINE's loop (txo_generate_prefix_from_enc: one multi-position pass
        # over the start, then the loop with everything generate() has -- and return_logp) where the loop can take it: no padding mask,
        # (T0 - 1) + max_len inside the positional table, T0 - 1 rows inside the multi-position pass's workspace.  Otherwise the stepwise
        # loop below, as before.  return_logp=True on this route: (tokens, logp, prefix_logp).
        bos_start = T0 == 1 and prefix_len is None and bool((st == eng.dims.bos).all())
        prompted = (not padded and not bos_start and not return_logits and T0 - 1 + max_len <= self.max_len
                    and T0 - 1 <= eng.max_batch * eng.max_tokens)
        if prefix_len is not None:
            prompted = True
            if return_logits:
                raise ValueError("return_logits is not available with prefix_len (a prompted decode keeps no logits)")
        with eng.modes(sample=(temp, seed), stop=stop, decode=decode, rules=rules, close=close, repeat_guard=repeat_guard, alts=return_alts) as sample:
            if prompted:
                out = eng.generate_prefix(None, st.to(enc.device), max_len, eos_tok, prefix_len=prefix_len, enc=enc, return_logp=return_logp)
                if return_alts:
                    alts = eng.last_alternatives(out[0] if return_logp else out)
                if rules is not None:
                    rstate = eng.last_rule_state(out[0] if return_logp else out)
                # stop='row': the engine has padded with its own pad id, by each row's own prefix; a caller's pad= is put in its place -- every
                # column the engine padded lies behind the row's first eos (the loop breaks only once every row holds one)
                if stop == "row" and eos_tok is not None and pad is not None and int(pad) != eng.dims.pad:
                    toks = out[0] if return_logp else out
                    toks = _pad_after_eos(toks, _inside_lengths(st, prefix_len, -1).to(toks.device), eos_tok, int(pad))
                    out = (toks, *out[1:]) if return_logp else toks
                if return_alts:
                    out = (*out, alts) if return_logp else (out, alts)
                if rules is not None:
                    out = (*out, rstate) if (return_logp or return_alts) else (out, rstate)
                if return_logp or return_alts or rules is not None:
                    return tuple(_squeeze0(o) for o in out) if squeeze else out
                return out.squeeze(0) if squeeze else out
            # beyond the positional table the engine slides the window with its multi-position forward, which needs a vocabulary
            # that is a multiple of 8 and a table that fits its workspace -- else the general stepwise loop below
            window_ok = max_len <= self.max_len or (eng.dims.vocab % 8 == 0 and self.max_len <= eng.max_batch * eng.max_tokens)
            engine_loop = not padded and T0 == 1 and bool((st == eng.dims.bos).all()) and (window_ok or return_logits)
            if rules is not None and not engine_loop:
                raise ValueError("rules= needs the engine's own loop: a start the prompted decode or a BOS start can take (no padding mask; beyond "
                                 "decoder.max_len a vocabulary that is a multiple of 8 and max_length <= max_batch * max_tokens)")
            if repeat_guard is not None and not engine_loop:
                raise ValueError("repeat_guard= needs the engine's own loop: a start the prompted decode or a BOS start can take (no padding mask; "
                                 "beyond decoder.max_len a vocabulary that is a multiple of 8 and max_length <= max_batch * max_tokens)")
            if return_alts and not engine_loop:
                raise ValueError("return_alts= needs the engine's own loop: a start the prompted decode or a BOS start can take (no padding mask)")
            if padded:
                if return_logits or return_logp:
                    raise ValueError("return_logits / return_logp are not available with a padding mask")
                out = self._generate_stepwise(st, eos_tok, max_len, enc, sample, mask=mask)
            elif T0 == 1 and bool((st == eng.dims.bos).all()) and (window_ok or return_logits):
                out = eng.generate(None, max_len, eos_tok, enc=enc, return_logits=return_logits, return_logp=return_logp)
                if return_alts:
                    alts = eng.last_alternatives(out[0] if (return_logits or return_logp) else out)
                if rules is not None:
                    rstate = eng.last_rule_state(out[0] if (return_logits or return_logp) else out)
            elif return_logits:
                raise ValueError("return_logits needs a BOS start inside the positional table (max_len <= decoder.max_len)")
            elif return_logp:
                raise ValueError("return_logp needs a BOS start and the engine's own loop (beyond decoder.max_len: a vocabulary that is a "
                                 "multiple of 8 and max_length <= max_batch * max_tokens)")
            else:
                out = self._generate_stepwise(st, eos_tok, max_len, enc, sample)
        if stop == "row" and eos_tok is not None:
            # (the engine's own generate has padded already; the stepwise loop -- arbitrary start prefix, padding mask -- and the
            # return_logits form are padded here: the same rule, tokens behind a row's first eos, start tokens included in the test as
            # decoder.py:115 does.  Logits behind a row's eos are what the finished row kept producing: unspecified.)
            p_id = eng.dims.pad if pad is None else int(pad)
            if return_logits or return_logp:                       # (logp behind a row's eos: the engine has written 0 there)
                out = (_pad_after_eos(out[0], st.to(out[0].device), eos_tok, p_id), *out[1:])
            else:
                out = _pad_after_eos(out, st.to(out.device), eos_tok, p_id)
        if return_alts:
            out = (*out, alts) if (return_logits or return_logp) else (out, alts)
        if rules is not None:
            out = (*out, rstate) if (return_logits or return_logp or return_alts) else (out, rstate)
        if return_logits or return_logp or return_alts or rules is not None:
            return tuple(_squeeze0(o) for o in out) if squeeze else out
        return out.squeeze(0) if squeeze else out

    def _generate_stepwise(self, st, eos_tok, max_len, enc, sample, mask=None):
        """General form (arbitrary start prefix, any max_len): one engine step per position with the reference's per-step
        host-side eos check (decoder.py:115-116); the engine picks the token (argmax or its sampler).

        While the output fits the positional table the KV cache is extended by one position per token.  Beyond it the
        reference feeds ``output[:, -max_len:]`` through the whole decoder with positions re-indexed from 0
        (decoder.py:99-100): no cached key survives that shift, so every further token re-runs its window through the
        cached path (max_len engine steps per token).  Exact and slow -- the reference is as slow there."""
        eng = self._engine
        st = st.to(enc.device)
        B, T0 = st.shape
        L = self.max_len
        eng.decode_begin(enc)
        output = st
        # decoder.py:95-101,112: the mask covers the start tokens, every generated token extends it with True, and it slides with the window
        m = None if mask is None else mask.to(device=enc.device, dtype=torch.bool)
        valid = 0                                                  # positions of the CURRENT window held by the cache
        with eng.key_mask(None if m is None else m[:, -L:]) as masked:
            for i in range(max_len):
                window = output[:, -L:]                            # decoder.py:99-100
                n = window.shape[1]
                if output.shape[1] > L:
                    valid = 0                                      # every position shifted: nothing cached is reusable
                    if masked:
                        eng.set_key_mask(m[:, -L:])
                wt = window.t().contiguous()
                if n - 1 - valid > 1 and eng.dims.vocab % 8 == 0 and n - 1 <= eng.max_batch * eng.max_tokens:   # (with or without a padding mask)
                    eng.decode_prefill(window[:, :n - 1].contiguous(), want_logits=False)   # positions 0..n-2 in one pass
                else:
                    for p in range(valid, n - 1):
                        eng.decode_step(p, wt[p], want_logits=False)
                if sample is not None and output.shape[1] > L:
                    # the device sampler draws from a counter RNG keyed by (seed, row, position); once the window slides the
                    # position stays at L - 1, so the seed advances with the token index instead (inside the caller's modes() scope)
                    eng.set_sampling(True, temp=sample[0], seed=sample[1] + i)
                _, tok = eng.decode_step(n - 1, wt[n - 1], want_logits=False)
                valid = n
                output = torch.cat((output, tok[:, None]), dim=-1)
                if masked:
                    m = torch.nn.functional.pad(m, (0, 1), value=True)
                if eos_tok is not None and bool((output == eos_tok).any(dim=1).all()):
                    break
        return output[:, T0:]


def _inside_lengths(tokens: torch.Tensor, lens, fill: int) -> torch.Tensor:
    """tokens (B, P) with every column at and behind its row's length lens[b] replaced by `fill` (lens None: as they are)"""
    if lens is None:
        return tokens
    cols = torch.arange(tokens.shape[1], device=tokens.device)[None, :]
    keep = cols < torch.as_tensor(lens).to(device=tokens.device, dtype=torch.int64).reshape(-1, 1)
    return torch.where(keep, tokens, torch.full_like(tokens, fill))


def _pad_after_eos(tokens: torch.Tensor, start: torch.Tensor, eos: int, pad: int) -> torch.Tensor:
    """stop='row': every token behind a row's first eos (looked for in start tokens + output, decoder.py:115) becomes `pad`."""
    if tokens.numel() == 0:
        return tokens
    seen_before = (start == eos).any(dim=1, keepdim=True)
    is_eos = tokens == eos
    prior = (torch.cumsum(is_eos.to(torch.int32), dim=1) - is_eos.to(torch.int32)) > 0     # an eos strictly before this column
    return torch.where(prior | seen_before, torch.full_like(tokens, pad), tokens)


class OCRModel(nn.Module):
    """TeXOCR model for image-to-LaTeX conversion -- inference surface (ocr_model.py:14-66)."""

    def __init__(self, encoder: VisionEncoder, decoder: AutoRegressiveDecoder, bos_token: int, eos_token: int,
                 trg_pad_idx: int, device: torch.device):
        super().__init__()
        if encoder._engine is not decoder._engine:
            raise ValueError("encoder and decoder must share one engine")
        self.encoder, self.decoder = encoder, decoder
        self.bos_token, self.eos_token, self.trg_pad_idx = bos_token, eos_token, trg_pad_idx
        self.device = device
        self._engine = encoder._engine
        self._engine._provider = self._export_weights
        self._engine._stale = True
        self.eval()

    @property
    def ragged_hybrid(self) -> bool:
        """Build extension: accept ragged batches (forward_ragged, generate_ragged, score_ragged, align_ragged) on the hybrid front end
        (HipEngine.ragged_hybrid); off by default."""
        return self._engine.ragged_hybrid

    @ragged_hybrid.setter
    def ragged_hybrid(self, on) -> None:
        self._engine.ragged_hybrid = on

    @property
    def rules_beam(self) -> bool:
        """Build extension: accept rules= in beam_search and generate(beam=k) (HipEngine.rules_beam); off by default."""
        return self._engine.rules_beam

    @rules_beam.setter
    def rules_beam(self, on) -> None:
        self._engine.rules_beam = on

    @property
    def guard_beam(self) -> bool:
        """Build extension: accept repeat_guard= in beam_search and generate(beam=k) (HipEngine.guard_beam); off by default."""
        return self._engine.guard_beam

    @guard_beam.setter
    def guard_beam(self, on) -> None:
        self._engine.guard_beam = on

    # ---- weights: the reference's state_dict layout, aliases included ----
    def _export_weights(self) -> Dict[str, torch.Tensor]:
        return dict(self.state_dict())

    def sync_weights(self) -> "OCRModel":
        """Re-upload the parameters to the engine at the next call (after editing them in place)."""
        self._engine._stale = True
        return self

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """nn.Module.load_state_dict for the reference's key layout.  Accepts tensors or numpy arrays; the aliased
        shared-LayerNorm keys layers.{s}.0.* (s > 0) may be omitted, and when given must equal layers.0.0.* -- the
        reference holds ONE LayerNorm per stack (attention.py:200,221)."""
        sd = {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))) for k, v in state_dict.items()}
        own = self.state_dict()
        for k in own:
            if _is_ln_alias(k):
                base = _LN_ALIAS.sub(lambda m: f".layers.0.0.{m.group(2)}", k)
                if k in sd and base in sd and not torch.equal(sd[k].float().cpu(), sd[base].float().cpu()):
                    raise ValueError(f"{k} differs from {base}: the reference shares ONE LayerNorm per stack")
                if k not in sd and base in sd:
                    sd[k] = sd[base]
        for k, v in sd.items():
            if k in own and tuple(v.shape) != tuple(own[k].shape):
                raise RuntimeError(f"load_state_dict: size mismatch for {k}: got {tuple(v.shape)}, expected {tuple(own[k].shape)}")
        res = super().load_state_dict(sd, strict=strict)
        self._engine._stale = True
        return res

    def to(self, *args, **kwargs):
        dev = kwargs.get("device", args[0] if args else None)
        if dev is not None and not isinstance(dev, torch.dtype) and torch.device(dev).type != "cuda":
            raise ValueError("this model only runs on the GPU")
        return self

    @torch.no_grad()
    def generate(self, src: torch.Tensor, max_len: int, temp: float = 0.3, *, decode: str = "greedy",
                 generator: Optional[torch.Generator] = None, seed: Optional[int] = None, return_logits: bool = False,
                 beam: int = 0, return_beams: bool = False, stop: str = "global", return_logp: bool = False,
                 prefix: Optional[torch.Tensor] = None, prefix_len=None, rules=None, close: bool = False, repeat_guard=None,
                 return_alts: int = 0):
        """return_alts=k (build extension; k in [1, 8]): which tokens the model would have taken instead.  An Alts (ids, logp), each (B, n, k),
        is appended to the result, directly before rule_state where there is one and last otherwise: the k best ids of the raw logits row
        behind every token and their log-probabilities (see Alts: raw, not the sampler's distribution, not masked by rules= / close= /
        repeat_guard=, so a forced token may be missing from its own alternatives).  In a greedy decode ids[..., 0] are the tokens and
        logp[..., 0] is return_logp's logp bit for bit.  With prefix=: the columns are the tokens' own.  The decode runs on the launch path.
        Refused (ValueError): k outside [1, 8] or beyond the vocabulary, with beam=, max_len > decoder.max_len.
        repeat_guard=(max_period, max_repeats) (build extension; both in [1, 16]): the repeat guard, for this call.  No row may end in
        max_repeats + 1 consecutive copies of a block of at most max_period tokens: the token that would complete such a run is masked in
        the selection like a rule-disallowed one (texocr_amd.guard.banned is the rule; the history is the prefix's tokens behind its start
        token, then the row's picks).  eos is never banned, a prefix token never masked; logp and logits stay those of the raw logits.  With
        rules=: a token must be allowed and unbanned, and where none is the ban is dropped for that pick.  The decode runs on the launch
        path.  Refused (ValueError): with close=True outside beam search, out-of-range values, a vocabulary of at most max_period + 1
        entries.  With beam=: the engine's refusal (ValueError) unless guard_beam is on; then every beam is held to the guard on its own
        history inside the beam selection, also beside close=True (see beam_search).
        close=True (build extension, only with rules=; ValueError otherwise): the closing decode, for this call.  A row may only pick a
        token from which its rules can still reach eos in the positions it has left (rules.TokenRules.allowed(remaining=) is the rule), so
        every row ends at an eos its rules allow -- under rules.brace_rules: balanced and finished inside max_len.  The one exception of a
        row is a forced prefix too deep to close in max_len: it closes as far as it gets and rule_state shows the rest.  Refused
        (ValueError) when the rules cannot reach eos from the start, or not within max_len.  With beam= (and rules_beam): every live beam
        ends finished; dead beams (score -inf) stay outside every guarantee.
        rules= (build extension): a texocr_amd.rules.TokenRules -- which tokens the loop may pick (vocabulary bans, brace balance:
        rules.ban / rules.brace_rules) -- installed for this call; the result gains rule_state (B, 2) int32 = every row's (state, depth)
        behind its last returned token as its LAST element.  The decode then runs on the launch path (not the persistent launch); logp and
        logits stay those of the raw logits.  No closure guarantee: a row that runs out of positions may end at depth > 0.  With beam=:
        the engine's refusal (ValueError) unless rules_beam is on; then the rules bind inside the beam selection (see beam_search) and
        rule_state (B, beam, 2), the state of every beam in the order of return_beams' tokens, is appended to the result.
        return_logp=True (build extension): (tokens, logp), both (B, n_steps) -- logp[b, t] = log_softmax(logits[b, t])[tokens[b, t]],
        what score(src, cat([bos], tokens)).logp reports, taken from the token selection itself: temperature 1 and the whole vocabulary
        also with decode='sample' (not the sampler's top-k / temperature distribution); stop='row': 0 behind a row's first eos, so
        logp.sum(1) is the sequence log-probability.  With return_logits: (tokens, logits, logp).
        prefix= (build extension): (B, P) int64 tokens the decode continues instead of starting at BOS (put BOS in column 0 yourself),
        prefix_len= (B,) their lengths per row (None: P) -> tokens (B, n), column j of row b the j-th token behind row b's own prefix;
        with return_logp (tokens, logp, prefix_logp (B, P)): prefix_logp[b, i] scores prefix[b, i] for min(prefix_len) <= i < prefix_len[b],
        0.0 elsewhere.  Needs (longest prefix - 1) + max_len <= decoder.max_len; not with beam= or return_logits."""
        _check_modes(stop)
        if prefix is not None:
            return self._generate_prefix(src, max_len, temp, decode, generator, seed, return_logits, beam, stop, return_logp, prefix, prefix_len, rules,
                                         close, repeat_guard, return_alts)
        if prefix_len is not None:
            raise ValueError("prefix_len needs prefix")
        if return_alts:
            ops.check_alts(return_alts, self._engine.dims.vocab)
            if beam:
                raise ValueError("return_alts is not available with beam search (beam=k): alternatives are kept by the greedy / sampled decode only")
        if beam and return_logp:
            raise ValueError("return_logp is not available with beam search (beam=k): it returns beam scores (return_beams=True)")
        if beam:                                           # build extension (BASELINE config 5); engine max_batch >= B * beam
            if max_len > self.decoder.max_len:
                raise ValueError(f"beam search needs max_len <= decoder.max_len ({self.decoder.max_len})")
            with self._engine.modes(rules=rules, close=close, repeat_guard=repeat_guard):   # (with rules the engine refuses unless rules_beam is on; with a guard, unless guard_beam is)
                if rules is None:
                    return self._engine.generate_beam(src, beam, max_len, self.eos_token, return_beams=return_beams)
                toks, scores = self._engine.generate_beam(src, beam, max_len, self.eos_token, return_beams=True)
                state = self._engine.last_beam_rule_state(toks)
            return (toks, scores, state) if return_beams else (toks[:, 0], state)
        if decode == "greedy" and self.bos_token == self._engine.dims.bos:
            # (max_len > decoder.max_len: txo_generate slides the window like the reference, decoder.py:99-100)
            # (stop='row' with return_logits: the engine does not compact -- a finished row's logits would be missing -- and only pads)
            with self._engine.modes(stop=stop, rules=rules, close=close, repeat_guard=repeat_guard, alts=return_alts):
                out = self._engine.generate(src, max_len, self.eos_token, return_logits=return_logits, return_logp=return_logp)
                out = _append_alts(self._engine, out, return_alts)
                if rules is None:
                    return out
                out = out if isinstance(out, tuple) else (out,)
                return (*out, self._engine.last_rule_state(out[0]))
        enc = self.encoder(src)
        start = torch.full((src.shape[0], 1), self.bos_token, dtype=torch.int64, device=src.device)   # ocr_model.py:57
        return self.decoder.generate(start_tokens=start, eos_tok=self.eos_token, max_len=max_len, temp=temp,
                                     decode=decode, generator=generator, seed=seed, enc=enc, return_logits=return_logits,
                                     stop=stop, pad=self.trg_pad_idx, return_logp=return_logp,
                                     **({} if rules is None and not close else {"rules": rules, "close": close}),
                                     **({} if repeat_guard is None else {"repeat_guard": repeat_guard}),
                                     **({} if not return_alts else {"return_alts": return_alts}))

    def _generate_prefix(self, src, max_len, temp, decode, generator, seed, return_logits, beam, stop, return_logp, prefix, prefix_len, rules=None,
                         close=False, repeat_guard=None, return_alts=0):
        """generate(prefix=) / generate_ragged(prefix=): src a (B, C, H, W) tensor or a sequence of images.  Every refusal comes before
        the engine is touched."""
        if return_alts:
            ops.check_alts(return_alts, self._engine.dims.vocab)
            if beam:
                raise ValueError("return_alts is not available with beam search (beam=k): alternatives are kept by the greedy / sampled decode only")
        if beam:
            raise ValueError("prefix= is not available with beam search (beam=k)")
        if return_logits:
            raise ValueError("prefix= is not available with return_logits (a prompted decode keeps no logits)")
        _check_modes(stop, decode)
        B = src.shape[0] if isinstance(src, torch.Tensor) else len(src)
        if not isinstance(prefix, torch.Tensor) or prefix.ndim != 2 or prefix.dtype != torch.int64 or prefix.shape[0] != B:
            raise ValueError(f"prefix must be an int64 tensor of shape (B, P) with one row per image ({B})")
        eng = self._engine
        if prefix_len is not None:
            prefix_len = torch.as_tensor(prefix_len).to(device="cpu", dtype=torch.int32).reshape(-1)
        ops.check_prefix(tuple(prefix.shape), prefix_len, max_len, self.decoder.max_len, eng.max_batch * eng.max_tokens)
        _check_token_ids(_inside_lengths(prefix, prefix_len, 0), eng.dims.vocab)   # (columns at and behind a row's length are never read)
        if seed is None and generator is not None:
            seed = generator.initial_seed()
        dev = src[0].device if isinstance(src, (list, tuple)) else src.device           # (a tensor or a PackedImages says it itself)
        with eng.modes(sample=(temp, seed), stop=stop, decode=decode, rules=rules, close=close, repeat_guard=repeat_guard, alts=return_alts):
            out = eng.generate_prefix(src, prefix.to(dev), max_len, self.eos_token, prefix_len=prefix_len, return_logp=return_logp)
            out = _append_alts(eng, out, return_alts)
            if rules is None:
                return out
            out = out if isinstance(out, tuple) else (out,)
            return (*out, eng.last_rule_state(out[0]))

    @torch.no_grad()
    def ingest(self, images, fit: bool = False, trim=False, regions=None) -> "ops.PackedImages":
        """Build extension: device-side image ingest.  A list of raw uint8 images of any sizes -- PIL images, numpy arrays or uint8 tensors
        (on the CPU or the model's device) of shape (H, W), (H, W, 3) or (H, W, 4): L, RGB, RGBA with the alpha ignored -> PackedImages(box
        (B, in_channels, Hc, Wc) float32, sizes (B, 2) int32 CPU), from ONE copy of the pixel bytes and ONE launch (txo_ingest_u8).  box is
        bit for bit ops.pack_ragged of the images preprocessed on the host (wrapper.preprocess_image: ToTensor -> Grayscale -> Invert, zero
        pad to multiples of 16, expanded to in_channels).  Every *_ragged method, beam_search and generate_ragged(prefix=) take the result
        in place of a list of (C, H_b, W_b) tensors; if all images have one size, box is a valid (B, C, H, W) for generate / score / align /
        beam_search.  PIL modes other than L / RGB / RGBA are converted with convert('RGB') on the host first.
        fit=True (default False: an image beyond the canvas is refused by the call that takes the container, as ever): every image with a
        side beyond the canvas (dims.canvas_hw) is downscaled on the device to fit it, aspect ratio kept (ops.fit_size; never upscaled), bit
        for bit PIL's Image.resize(..., BILINEAR) of its L / RGB channels -- an RGBA image is fitted on its RGB channels, the alpha is not
        read -- and `sizes` holds the fitted sizes.  Still one copy of the raw bytes.  An axis that would shrink by more than 32 times is a
        ValueError naming the image.
        trim=(level, margin), or True for (127, 2) (default False): every image is first cut to its ink on the device -- a pixel is ink iff
        min(read channels) <= level; `margin` pixels are kept around the ink box, clamped to the image; an image without ink stays whole
        (ops.trim_view is the rule) -- and the view takes the image's place in front of the fit and the ingest: an image beyond the canvas
        whose ink fits is accepted without a fit.  regions=(B, 4) = (y0, x0, h, w): image b is cut to the caller's rectangle instead; pass
        a page once per region and its bytes go up (or, on the device, are used) once.  trim and regions together are a ValueError.  Either
        way the container is bit for bit that of contiguous copies of the views, the result's `views` (B, 4) int32 holds them in source
        pixels, and the trim costs the one wait of the path (the container's size depends on its answer)."""
        return self._engine.ingest(images, fit=fit, trim=trim, regions=regions)

    @torch.no_grad()
    def beam_search(self, src, beams: int, max_len: int, *, return_logp: bool = False, length_alpha: float = 0.0, rules=None,
                    close: bool = False, repeat_guard=None, return_alts: int = 0) -> Beams:
        """Build extension: the k = beams best sequences of every image, with score, length and (return_logp=True) the log-probability of
        every token -> Beams.  src is a (B, C, H, W) tensor, or a sequence of (C, H_b, W_b) tensors of different sizes: those go
        through ONE ragged encode and ONE decode, and the beams of image b are what beam_search(src[b][None]) returns, over the batch's n.
        The search is generate(beam=k)'s (same tokens and scores); eos is the model's eos_token.  length_alpha > 0 orders an image's beams
        by score / length ** length_alpha instead of by score -- the final order only, the set of beams does not depend on it.
        Needs beams in [1, 8], max_len <= decoder.max_len and images * beams <= the engine's max_batch (ValueError otherwise).
        rules= (build extension): a texocr_amd.rules.TokenRules installed for this call.  With rules_beam off (the default) the engine
        refuses (ValueError).  On: a candidate the rules disallow in its parent's state counts as -inf in the selection, so no disallowed
        hypothesis ever holds a slot; scores and logp stay sums of the RAW model's log-probabilities (nothing is renormalised), and
        Beams.rule_state holds every beam's state.  No closure guarantee: a beam that runs out of positions may end at depth > 0.
        close=True (only with rules=): the closing search, generate(close=True)'s budget inside the selection with R = max_len - position: a
        hypothesis that could no longer reach eos never holds a slot, so every LIVE beam ends finished (under brace_rules: balanced) and
        lengths <= max_len; dead beams stay outside every guarantee.
        repeat_guard=(max_period, max_repeats) (build extension): with guard_beam off (the default) the engine refuses (ValueError).  On: the
        repeat guard inside the selection.  Every beam's ban set is texocr_amd.guard.banned on the tokens ITS ancestry committed; a banned
        candidate counts as -inf like a rule-disallowed one, eos is never banned, scores and logp stay sums of the raw log-probabilities.
        Beside rules= (rules_beam on as well) a candidate must be allowed and unbanned; a beam that has no such token drops its ban at that
        pick (the yield rule), so with close=True every live beam still ends finished."""
        if return_alts:
            raise ValueError("return_alts is not available in beam_search: alternatives are kept by generate()'s greedy / sampled decode only")
        if isinstance(src, torch.Tensor):
            if src.ndim != 4:
                raise ValueError("beam search needs src of shape (B, C, H, W), or a sequence of (C, H_b, W_b) images")
            n_images = int(src.shape[0])
        elif isinstance(src, (list, tuple, ops.PackedImages)):
            n_images = len(src)
        else:
            raise ValueError("beam search needs src of shape (B, C, H, W), or a sequence of (C, H_b, W_b) images")
        check_beam_args(beams, max_len, length_alpha, n_images, self.decoder.max_len, self._engine.max_batch)
        with self._engine.modes(rules=rules, close=close, repeat_guard=repeat_guard):   # rules=: the engine refuses (ValueError) unless rules_beam is on
            out = self._engine.beam_search(src, beams, max_len, self.eos_token, return_logp=return_logp, length_alpha=length_alpha)
            return Beams(*out, self._engine.last_beam_rule_state(out[0]) if rules is not None else None)

    @torch.no_grad()
    def generate_ragged(self, images, max_len: int, temp: float = 0.3, *, decode: str = "greedy", seed: Optional[int] = None,
                        stop: str = "global", return_logp: bool = False, prefix: Optional[torch.Tensor] = None, prefix_len=None, rules=None,
                        close: bool = False, repeat_guard=None, return_alts: int = 0):
        """return_alts=k: as generate() takes it (an Alts appended, before rule_state); refused with max_len > decoder.max_len.
        Build extension: generate() over a sequence of (C, H_b, W_b) images of different sizes in ONE engine call -> (B, n_steps).
        Row b is what generate(images[b][None]) returns, over the batch's n_steps (the eos rules are generate()'s; a sampled draw
        is keyed by the row of the batch).  max_len may exceed decoder.max_len: the window slides as in generate(), under the engine's
        two preconditions (a vocabulary that is a multiple of 8, max_length <= max_batch * max_tokens; ValueError before anything is
        decoded otherwise).  return_logp=True: (tokens, logp) as generate() returns them.  prefix= / prefix_len= / rules= / close= /
        repeat_guard=: as generate() takes them (rules=: rule_state (B, 2) is the result's last element)."""
        if prefix is not None:
            return self._generate_prefix(images, max_len, temp, decode, None, seed, False, 0, stop, return_logp, prefix, prefix_len, rules, close,
                                         repeat_guard, return_alts)
        if prefix_len is not None:
            raise ValueError("prefix_len needs prefix")
        if return_alts:
            ops.check_alts(return_alts, self._engine.dims.vocab)
        with self._engine.modes(sample=(temp, seed), stop=stop, decode=decode, rules=rules, close=close, repeat_guard=repeat_guard, alts=return_alts):
            out = self._engine.generate_ragged(images, max_len, self.eos_token, return_logp=return_logp)
            out = _append_alts(self._engine, out, return_alts)
            if rules is None:
                return out
            out = out if isinstance(out, tuple) else (out,)
            return (*out, self._engine.last_rule_state(out[0]))

    @torch.no_grad()
    def score(self, src: torch.Tensor, trg: torch.Tensor, mask: Optional[torch.Tensor] = None, alts: int = 0):
        """Teacher-forced scoring of trg (B, L) against the images src -- what forward(src, trg) computes (ocr_model.py:38-44),
        without autograd and per token: see AutoRegressiveDecoder.score.  mask defaults to trg != trg_pad_idx (make_trg_mask).
        The confidence of a generate() result: score(src, cat([bos], tokens)).
        alts=k (build extension, 1..8): -> (Score, Alts), the k best ids / log-probabilities of every scored row (AutoRegressiveDecoder.score)."""
        if alts:
            ops.check_alts(alts, self._engine.dims.vocab)
        if mask is None:
            mask = trg != self.trg_pad_idx
        return self.decoder.score(trg, mask=mask, enc=self.encoder(src), **({"alts": alts} if alts else {}))

    def _ragged_trg(self, images, trg: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
        """the checks score_ragged / align_ragged share, before the engine is touched -> the mask (default trg != trg_pad_idx)"""
        if trg.ndim != 2 or trg.shape[0] != len(images):
            raise ValueError(f"trg must be (B, L) with one row per image ({len(images)}), got {tuple(trg.shape)}")
        if trg.shape[1] < 2:
            raise ValueError("trg needs at least two columns (one fed token and its target)")
        if trg.shape[1] - 1 > self.decoder.max_len:
            raise ValueError("sequence longer than decoder.max_len + 1")
        if mask is None:
            mask = trg != self.trg_pad_idx
        if tuple(mask.shape) != tuple(trg.shape):
            raise ValueError("mask must have the shape of trg")
        return mask

    @torch.no_grad()
    def score_ragged(self, images, trg: torch.Tensor, mask: Optional[torch.Tensor] = None, alts: int = 0) -> Score:
        """alts=: refused (ValueError) -- alternatives are not kept on a ragged scoring pass.
        Build extension: score() over a sequence of (C, H_b, W_b) images of different sizes in ONE engine call (txo_score_ragged): row b
        is what score(images[b][None], trg[b:b+1], mask[b:b+1]) returns; loss and token_acc run over the whole batch's valid positions."""
        if alts:
            raise ValueError("alts= is not available in score_ragged: alternatives are not kept on a ragged scoring pass (use score())")
        mask = self._ragged_trg(images, trg, mask)
        _check_x(trg, "(B, L)")
        _check_token_ids(trg, self._engine.dims.vocab)
        m = mask.to(device=trg.device, dtype=torch.bool)
        logp, top1, top1_logp = self._engine.score_ragged(images, trg, m)
        return score_summary(logp, top1, top1_logp, trg, m)

    @torch.no_grad()
    def align_ragged(self, images, trg: torch.Tensor, mask: Optional[torch.Tensor] = None, layer: Optional[int] = -1) -> List[Alignment]:
        """Build extension: align() over a sequence of (C, H_b, W_b) images of different sizes in one encode and one teacher-forced pass:
        a list of B Alignments, element b what align(images[b][None], trg[b:b+1], mask[b:b+1], layer) returns, on image b's own
        (H_b / 16, W_b / 16) patch grid."""
        mask = self._ragged_trg(images, trg, mask)
        ps = self.encoder.patch_size
        if isinstance(images, ops.PackedImages):
            grids = images.grids(ps)
        else:
            grids = [(int(im.shape[1]) // ps, int(im.shape[2]) // ps) for im in images]
        enc, ntok = self.encoder.forward_ragged(images)
        return self.decoder.align(trg, mask=mask, enc=enc, layer=layer, n_tokens=ntok, grids=grids)

    @torch.no_grad()
    def align(self, src: torch.Tensor, trg: torch.Tensor, mask: Optional[torch.Tensor] = None, layer: Optional[int] = -1) -> Alignment:
        """Build extension: where in the image every token of trg (B, L) came from -- the companion of score(): the head-mean cross
        attention of decoder layer `layer` (None: the mean over the layers) on the image's patch grid, from one teacher-forced pass
        over trg[:, :-1].  mask defaults to trg != trg_pad_idx.  See Alignment."""
        if mask is None:
            mask = trg != self.trg_pad_idx
        grid = (int(src.shape[2]) // self.encoder.patch_size, int(src.shape[3]) // self.encoder.patch_size)
        return self.decoder.align(trg, mask=mask, enc=self.encoder(src), layer=layer, grid=grid)

    def forward(self, *a, **k):
        raise NotImplementedError("OCRModel.forward is the training loss (ocr_model.py:38-44); this engine "
                                  "implements the generate() inference path only")


def _assemble(dims: Dims, dtype: str, max_batch: int, max_tokens: int, device: torch.device, ragged_hybrid: bool = False,
              rules_beam: bool = False, guard_beam: bool = False) -> OCRModel:
    eng = HipEngine(dims, dtype=dtype, max_batch=max_batch, max_tokens=max_tokens)
    if ragged_hybrid:
        eng.ragged_hybrid = True
    if rules_beam:
        eng.rules_beam = True
    if guard_beam:
        eng.guard_beam = True
    shared: Dict[str, nn.Parameter] = {}
    return OCRModel(VisionEncoder(eng, shared), AutoRegressiveDecoder(eng, shared), dims.bos, dims.eos, dims.pad, device)


def create_model(config: dict, dtype: str = "fp32", max_batch: int = 64, max_tokens: int = 0, ragged_hybrid: bool = False,
                 rules_beam: bool = False, guard_beam: bool = False) -> OCRModel:
    """create_model(config) (ocr_model.py:113-130).  As in the reference the model comes back with default-initialised
    parameters; load_state_dict replaces them.  ragged_hybrid=True (build extension): the model's ragged calls work on the hybrid
    front end (OCRModel.ragged_hybrid).  rules_beam=True (build extension): beam search accepts rules= (OCRModel.rules_beam).
    guard_beam=True (build extension): beam search accepts repeat_guard= (OCRModel.guard_beam)."""
    dims = Dims.from_config(config)
    device = torch.device(config.get("device", "cuda"))
    if device.type != "cuda":
        device = torch.device("cuda")
    return _assemble(dims, dtype, max_batch, max_tokens, device, ragged_hybrid, rules_beam, guard_beam)


def model_from_dims(dims: Dims, dtype: str = "fp32", max_batch: int = 64, max_tokens: int = 0) -> OCRModel:
    return _assemble(dims, dtype, max_batch, max_tokens, torch.device("cuda"))
