"""PyTorch custom operators over the C ABI (include/texocr.h): ``torch.ops.texocr.*``.

north_star: "driven from Python via PyTorch-ROCm custom ops through a thin C-ABI".  Each operator is a thin
shim: it checks its tensors, takes the current HIP stream from torch and calls ONE ``txo_*`` entry point of
``libtexocr_hip.so`` through ctypes.  Fake (meta) implementations give the output shapes, so the operators can be
traced (``torch.compile`` / ``FakeTensorMode``) without a GPU.  The reference callables they stand for
(file:line in the reference tree):

  texocr::encode            VisionEncoder.forward                     model/encoder.py:128-152
  texocr::decode_begin      the ``enc=`` hand-over of decoder.generate model/decoder.py:56,103 (+ attention.py:125-126 once)
  texocr::decode_step       Transformer.forward, one position         model/decoder.py:41-67
  texocr::decode_score      AutoRegressiveDecoder.forward, no autograd  model/decoder.py:124-145
  texocr::decode_attn       Transformer.forward(return_attn=True)     model/decoder.py:41-67 (+ attention.py:166-178: post_softmax_attn)
  texocr::generate          OCRModel.generate                         model/ocr_model.py:46-66
  texocr::generate_from_enc AutoRegressiveDecoder.generate            model/decoder.py:77-122
  texocr::generate_beam     (build extension, BASELINE config 5)
  texocr::beam_search / beam_search_ragged
                            (build extension) generate_beam's search returning every beam with its score, its length and the
                            log-probability of each token, on a fixed batch or a ragged container (txo_beam_out)
  texocr::generate_logp / generate_from_enc_logp / generate_ragged_logp
                            (build extension) generate / generate_from_enc / generate_ragged that also return the log-probability
                            of every produced token, taken from the token selection itself (no second pass, no (B, T, V) tensor)
  texocr::set_rules_beam / last_beam_rule_state
                            (build extension, opt-in) beam search under token rules (texocr::set_token_rules) and the beams' rule states
  texocr::set_guard_beam    (build extension, opt-in) the repeat guard inside the beam selection: the beam entries accept a guard
  texocr::set_repeat_guard  (build extension, opt-in) the repeat guard: a row of the generate family may not end in max_repeats + 1 copies of a
                            block of at most max_period tokens (texocr_amd/guard.py is the rule in numpy)
  texocr::set_alternatives / last_alternatives / decode_score_alts / score_alts
                            (build extension, opt-in) the k best ids and log-probabilities of every logits row: beside the tokens of the
                            generate family (csrc/step_alts.h), and beside the teacher-forced scores (csrc/score.h), no (B, T, V) tensor
  texocr::set_rules_close   (build extension, opt-in) the closing decode: a constrained decode or beam search only picks tokens from which
                            eos can still be reached in the positions left (``rules_close_dist`` reads the engine's distance table)
  texocr::encode_ragged / decode_begin_ragged / generate_ragged / score_ragged
                            (build extension) the same callables over a RAGGED batch: B images of different sizes in one
                            container, every image computed as if it had been passed on its own (``pack_ragged`` builds the container);
                            decode_prefill / decode_score / decode_attn / decode_set_key_mask run on a ragged session as on any other
  texocr::ingest_u8         (build extension) the raw uint8 pixels of B images of different sizes and channel counts -> that container, on
                            the device in one launch, bit for bit what the host preprocessing makes of them (``pack_u8`` is its front end)
  texocr::ingest_u8_fit     (build extension) the same with every image beyond a target size downscaled to fit it first, bit for bit PIL's
                            BILINEAR resize (``pack_u8(..., fit=(Fh, Fw))``)
  texocr::ingest_trim_views (build extension) the ink extents of every image, found on the device in one launch -> the views (y0, x0, h', w')
                            that keep the ink and a margin (``trim_view`` is the rule on the host; ``pack_u8(..., trim=(level, margin))``)
  texocr::ingest_u8_view    (build extension) ingest_u8 / ingest_u8_fit of a rectangle of every source image: the trimmed views, or the
                            caller's regions of a page that went up once (``pack_u8(..., regions=...)``)

An engine is named by an integer id (operators take tensors and scalars only); ``register_engine`` hands one out.
There is no CPU implementation: calling an operator on CPU tensors raises.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from dataclasses import dataclass
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch
from torch.library import custom_op

from . import _lib

_ENGINES: Dict[int, "weakref.ReferenceType"] = {}
_NEXT = [1]


def register_engine(obj) -> int:
    """obj: anything with ``.dims`` (fake implementations) and, for real calls, ``.handle`` / ``.lib`` / ``.device``
    (texocr_amd.model.HipEngine)."""
    i = _NEXT[0]
    _NEXT[0] += 1
    _ENGINES[i] = weakref.ref(obj)
    return i


def unregister_engine(i: int) -> None:
    _ENGINES.pop(i, None)


def _eng(i: int, ready: bool = False):
    r = _ENGINES.get(int(i))
    e = r() if r is not None else None
    if e is None:
        raise RuntimeError(f"texocr: no live engine with id {i}")
    if ready and hasattr(e, "_ensure"):
        e._ensure()                      # upload the owning module's parameters if they changed since the last call
    return e


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _f32_dev(t: torch.Tensor, name: str, eng) -> torch.Tensor:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA/HIP tensor (this engine has no CPU path)")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if t.device.index != eng.device:
        raise ValueError(f"{name} lives on cuda:{t.device.index} but the engine was created on cuda:{eng.device}")
    return t.contiguous()


def _i64_dev(t: torch.Tensor, name: str, eng, rows: int, ndim: int, shape: str) -> torch.Tensor:
    """token ids: `rows` rows, `ndim` dimensions; `shape` is how the message names them"""
    if t.dtype != torch.int64 or not t.is_cuda or t.ndim != ndim or t.shape[0] != rows:
        raise ValueError(f"{name} must be an int64 GPU tensor of shape {shape}")
    if t.device.index != eng.device:
        raise ValueError(f"{name} live{'' if name.endswith('s') else 's'} on cuda:{t.device.index} but the engine was created on cuda:{eng.device}")
    return t.contiguous()


def _img_arg(img: torch.Tensor, eng) -> torch.Tensor:
    if img.ndim != 4:
        raise ValueError("expected an image batch of shape (B, C, H, W)")
    img = _f32_dev(img, "src", eng)
    eng.dims.check_image(*img.shape[1:])
    return img


def _enc_arg(enc: torch.Tensor, eng, n: str = "N") -> torch.Tensor:
    enc = _f32_dev(enc, "enc", eng)
    if enc.ndim != 3 or enc.shape[2] != eng.dims.embed_dim:
        raise ValueError(f"enc must be (B, {n}, {eng.dims.embed_dim})")
    return enc


# ---- the decode session, as far as the binding has to know it ------------------------------------------------------------------
@dataclass
class Session:
    rows: int                               # rows of a decode_step / decode_prefill / decode_score / key mask
    src: torch.Tensor                       # what the session was opened on: kept alive while the engine may read it
    mask: Optional[torch.Tensor] = None     # the uint8 key mask handed to the engine, kept alive likewise
    keys: Optional[int] = None              # N of the session where `src` does not say it: the slot stride Ns behind score_ragged (src = the container)


def _open(e, rows: int, src: torch.Tensor, keys: Optional[int] = None) -> None:
    """The one writer of ``e.session``, behind every entry point that leaves the engine with an open session (_call).  Invariant: whenever the
    engine's session is open, the record's ``rows`` equals the engine's ``ses.rows`` -- the operators size their outputs by it and the
    engine writes ``ses.rows`` rows into them.  Not the converse: the engine also closes a session on its own (a stop='row' generate
    that compacted) while the record stays; it then refuses the next step (TXO_E_STATE) before it writes anything."""
    e.session = Session(int(rows), src, keys=keys)


def _close(e) -> None:
    """no session is known to be open: behind generate_ragged (the engine closes its own) and behind a failed call that would have changed it"""
    e.session = None


def session(e, op: str) -> Session:
    """The record of the open session, for the operators (and HipEngine.decode_step) that work on one."""
    s = getattr(e, "session", None)
    if s is None:
        raise RuntimeError(f"texocr::{op} needs a session started by texocr::decode_begin")
    return s


def _call(e, fn: str, *args, leaves: Optional[tuple] = None) -> None:
    """ONE entry point ``fn(handle, *args, stream)`` on the engine's device and torch's current stream; raises what _lib.check raises.
    leaves: the engine's session behind an entry point that opens, replaces or closes it -- (rows, src[, keys]): this one, open; (): none.
    If such a call fails the engine's state is not known here and the record stays closed: the engine will say what it holds."""
    if leaves is not None:
        _close(e)
    with torch.cuda.device(e.device):
        _lib.check(getattr(e.lib, fn)(e.handle, *args, _stream()))
    if leaves:
        _open(e, *leaves)


# ---------------------------------------------------------------------------------------------------------------
@custom_op("texocr::encode", mutates_args=())
def encode(img: torch.Tensor, engine: int) -> torch.Tensor:
    e = _eng(engine, ready=True)
    img = _img_arg(img, e)
    B, Cc, H, W = img.shape
    out = torch.empty((B, e.dims.n_tokens(H, W), e.dims.embed_dim), device=img.device, dtype=torch.float32)
    _call(e, "txo_encode", img.data_ptr(), B, Cc, H, W, out.data_ptr())
    return out


@encode.register_fake
def _(img, engine):
    d = _eng(engine).dims
    B, _, H, W = img.shape
    return img.new_empty((B, d.n_tokens(H, W), d.embed_dim), dtype=torch.float32)


@custom_op("texocr::decode_begin", mutates_args=())
def decode_begin(enc: torch.Tensor, engine: int) -> None:
    e = _eng(engine, ready=True)
    enc = _enc_arg(enc, e)
    _call(e, "txo_decode_begin", enc.data_ptr(), enc.shape[0], enc.shape[1], leaves=(enc.shape[0], enc))


@custom_op("texocr::decode_set_key_mask", mutates_args=())
def decode_set_key_mask(mask: Optional[torch.Tensor], engine: int) -> None:
    """The `mask` argument of decoder.generate / decoder.net (decoder.py:95-101; attention.py:130-155) for the decode_step calls of
    the current session: (B, cols) bool, False = padding (never attended by later queries); None clears it."""
    e = _eng(engine)
    ses = session(e, "decode_set_key_mask")
    if mask is None:
        _call(e, "txo_decode_set_key_mask", None, 0)
        return
    if mask.ndim != 2 or mask.shape[0] != ses.rows or not mask.is_cuda:
        raise ValueError("mask must be a GPU tensor of shape (B, cols) matching the session started by texocr::decode_begin")
    ses.mask = mask.to(torch.uint8).contiguous()
    _call(e, "txo_decode_set_key_mask", ses.mask.data_ptr(), int(ses.mask.shape[1]))


@custom_op("texocr::decode_step", mutates_args=())
def decode_step(tok_in: Optional[torch.Tensor], engine: int, t: int, batch: int, want_logits: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """One position: returns (logits (B, V) -- (0, V) when want_logits is false --, argmax token (B,))."""
    e = _eng(engine)
    if batch != session(e, "decode_step").rows:
        raise ValueError("batch does not match the decode session started by texocr::decode_begin")
    dev = torch.device("cuda", e.device)
    if tok_in is not None:
        tok_in = _i64_dev(tok_in, "tok_in", e, batch, 1, "(B,)")
    logits = torch.empty((batch if want_logits else 0, e.dims.vocab), device=dev, dtype=torch.float32)
    nxt = torch.empty((batch,), device=dev, dtype=torch.int64)
    _call(e, "txo_decode_step", None if tok_in is None else tok_in.data_ptr(), int(t), logits.data_ptr() if want_logits else None,
          nxt.data_ptr())
    return logits, nxt


@decode_step.register_fake
def _(tok_in, engine, t, batch, want_logits):
    d = _eng(engine).dims
    ref = tok_in if tok_in is not None else torch.empty(0)
    return (ref.new_empty((batch if want_logits else 0, d.vocab), dtype=torch.float32),
            ref.new_empty((batch,), dtype=torch.int64))


@custom_op("texocr::decode_prefill", mutates_args=())
def decode_prefill(tokens: torch.Tensor, engine: int, want_logits: bool) -> torch.Tensor:
    """Transformer.forward over a whole prefix in one pass (decoder.py:41-67): tokens (B, t) int64 at positions 0..t-1 ->
    logits (B, t, V) (or (0, t, V)); fills the self-attention K/V cache rows 0..t-1 of the session opened by decode_begin."""
    e = _eng(engine)
    B = session(e, "decode_prefill").rows
    tokens = _i64_dev(tokens, "tokens", e, B, 2, "(B, t) matching the session started by texocr::decode_begin")
    t = tokens.shape[1]
    logits = torch.empty((B if want_logits else 0, t, e.dims.vocab), device=tokens.device, dtype=torch.float32)
    _call(e, "txo_decode_prefill", tokens.data_ptr(), int(t), logits.data_ptr() if want_logits else None)
    return logits


@decode_prefill.register_fake
def _(tokens, engine, want_logits):
    d = _eng(engine).dims
    return tokens.new_empty((tokens.shape[0] if want_logits else 0, tokens.shape[1], d.vocab), dtype=torch.float32)


@custom_op("texocr::decode_score", mutates_args=())
def decode_score(tokens: torch.Tensor, engine: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Teacher-forced scores of the session opened by decode_begin (txo_decode_score): tokens (B, L) int64, columns 0..L-2 fed in one
    causal pass, column p+1 the target of position p -> (logp (B, L-1) = log_softmax(logits)[target], top1 (B, L-1) = argmax of the
    logits, top1_logp (B, L-1)).  No (B, L-1, V) tensor is made on the way; the K/V cache holds rows 0..L-2 afterwards."""
    e = _eng(engine)
    B = session(e, "decode_score").rows
    tokens = _i64_dev(tokens, "tokens", e, B, 2, "(B, L) matching the session started by texocr::decode_begin")
    L = int(tokens.shape[1])
    if L < 2 or L - 1 > e.dims.max_len:
        raise ValueError(f"tokens must have 2 <= L <= max_len + 1 = {e.dims.max_len + 1} columns, got {L}")
    logp = torch.empty((B, L - 1), device=tokens.device, dtype=torch.float32)
    top1 = torch.empty((B, L - 1), device=tokens.device, dtype=torch.int64)
    top1_logp = torch.empty((B, L - 1), device=tokens.device, dtype=torch.float32)
    _call(e, "txo_decode_score", tokens.data_ptr(), L, logp.data_ptr(), top1.data_ptr(), top1_logp.data_ptr())
    return logp, top1, top1_logp


@decode_score.register_fake
def _(tokens, engine):
    B, L = tokens.shape
    return (tokens.new_empty((B, L - 1), dtype=torch.float32), tokens.new_empty((B, L - 1), dtype=torch.int64),
            tokens.new_empty((B, L - 1), dtype=torch.float32))


ALTS_MAX = 8       # include/texocr.h: txo_set_alternatives


def check_alts(k, vocab: Optional[int] = None) -> int:
    """k of an alternatives request, as the engine checks it (the same refusals, before the engine is touched)"""
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"alternatives: k must be an int in [1, {ALTS_MAX}], got {k!r}")
    if k < 1 or k > ALTS_MAX:
        raise ValueError(f"alternatives: k is {k}; it must be in [1, {ALTS_MAX}]")
    if vocab is not None and k > vocab:
        raise ValueError(f"alternatives: k is {k} and the vocabulary has {vocab} entries")
    return k


@custom_op("texocr::decode_score_alts", mutates_args=())
def decode_score_alts(tokens: torch.Tensor, engine: int, k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """decode_score with the k best of every scored row (txo_decode_score_alts) -> (logp, top1, top1_logp, alt_ids (B, L-1, k) int32,
    alt_logp (B, L-1, k) float32): descending value, the lower id first among equals; alt_ids[..., 0] is top1 and alt_logp[..., 0] top1_logp,
    and the first three are bit for bit decode_score's."""
    e = _eng(engine)
    B = session(e, "decode_score_alts").rows
    tokens = _i64_dev(tokens, "tokens", e, B, 2, "(B, L) matching the session started by texocr::decode_begin")
    L = int(tokens.shape[1])
    if L < 2 or L - 1 > e.dims.max_len:
        raise ValueError(f"tokens must have 2 <= L <= max_len + 1 = {e.dims.max_len + 1} columns, got {L}")
    logp = torch.empty((B, L - 1), device=tokens.device, dtype=torch.float32)
    top1 = torch.empty((B, L - 1), device=tokens.device, dtype=torch.int64)
    top1_logp = torch.empty((B, L - 1), device=tokens.device, dtype=torch.float32)
    ids = torch.empty((B, L - 1, max(int(k), 0)), device=tokens.device, dtype=torch.int32)
    alp = torch.empty((B, L - 1, max(int(k), 0)), device=tokens.device, dtype=torch.float32)
    _call(e, "txo_decode_score_alts", tokens.data_ptr(), L, logp.data_ptr(), top1.data_ptr(), top1_logp.data_ptr(), int(k), ids.data_ptr(), alp.data_ptr())
    return logp, top1, top1_logp, ids, alp


@decode_score_alts.register_fake
def _(tokens, engine, k):
    B, L = tokens.shape
    return (tokens.new_empty((B, L - 1), dtype=torch.float32), tokens.new_empty((B, L - 1), dtype=torch.int64),
            tokens.new_empty((B, L - 1), dtype=torch.float32), tokens.new_empty((B, L - 1, k), dtype=torch.int32),
            tokens.new_empty((B, L - 1, k), dtype=torch.float32))


@custom_op("texocr::score_alts", mutates_args=())
def score_alts(img: torch.Tensor, tokens: torch.Tensor, mask: Optional[torch.Tensor], engine: int, k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """txo_score_alts: images (B, C, H, W), tokens (B, L) int64, mask (B, L) bool / uint8 (False = padding) or None: encode, open the session
    and score in one call -> decode_score_alts's five tensors.  The session stays open on the engine's own encoder rows."""
    e = _eng(engine, ready=True)
    img = _img_arg(img, e)
    B = int(img.shape[0])
    tokens = _i64_dev(tokens, "tokens", e, B, 2, "(B, L), one row per image")
    L = int(tokens.shape[1])
    if L < 2 or L - 1 > e.dims.max_len:
        raise ValueError(f"tokens must have 2 <= L <= max_len + 1 = {e.dims.max_len + 1} columns, got {L}")
    m8 = None
    if mask is not None:
        if tuple(mask.shape) != (B, L):
            raise ValueError("mask must have the shape of tokens")
        m8 = mask.to(device=tokens.device, dtype=torch.uint8).contiguous()
    logp = torch.empty((B, L - 1), device=tokens.device, dtype=torch.float32)
    top1 = torch.empty((B, L - 1), device=tokens.device, dtype=torch.int64)
    top1_logp = torch.empty((B, L - 1), device=tokens.device, dtype=torch.float32)
    ids = torch.empty((B, L - 1, max(int(k), 0)), device=tokens.device, dtype=torch.int32)
    alp = torch.empty((B, L - 1, max(int(k), 0)), device=tokens.device, dtype=torch.float32)
    _call(e, "txo_score_alts", img.data_ptr(), B, int(img.shape[1]), int(img.shape[2]), int(img.shape[3]), tokens.data_ptr(),
          None if m8 is None else m8.data_ptr(), L, logp.data_ptr(), top1.data_ptr(), top1_logp.data_ptr(), int(k), ids.data_ptr(), alp.data_ptr(),
          leaves=(B, img, 1 + (int(img.shape[2]) // 16) * (int(img.shape[3]) // 16)))
    return logp, top1, top1_logp, ids, alp


@score_alts.register_fake
def _(img, tokens, mask, engine, k):
    B, L = tokens.shape
    return (tokens.new_empty((B, L - 1), dtype=torch.float32), tokens.new_empty((B, L - 1), dtype=torch.int64),
            tokens.new_empty((B, L - 1), dtype=torch.float32), tokens.new_empty((B, L - 1, k), dtype=torch.int32),
            tokens.new_empty((B, L - 1, k), dtype=torch.float32))


def _session_keys(e, ses: Session) -> int:
    """N of the open session: the encoder rows it was opened on (a ragged session: the slot stride Ns), or those of the images a generate
    call encoded itself"""
    if ses.keys is not None:
        return ses.keys
    src = ses.src
    return int(src.shape[1]) if src.ndim == 3 else e.dims.n_tokens(int(src.shape[2]), int(src.shape[3]))


def _attn_shapes(d, B: int, t: int, N: int, want_logits: bool, want_self: bool, want_cross: bool, want_mean: bool):
    """(logits, self, cross, mean) of decode_attn; a part not asked for keeps its trailing dimensions and has no rows"""
    Ld, H = d.dec_layers, d.dec_heads
    return ((B if want_logits else 0, t, d.vocab), (Ld if want_self else 0, B, H, t, t), (Ld if want_cross else 0, B, H, t, N),
            (Ld if want_mean else 0, B, t, N))


@custom_op("texocr::decode_attn", mutates_args=())
def decode_attn(tokens: torch.Tensor, engine: int, want_logits: bool, want_self: bool, want_cross: bool,
                want_mean: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """decode_prefill that also returns the attention probabilities of every decoder layer (txo_decode_attn): tokens (B, t) int64 ->
    (logits (B, t, V), self (Ld, B, heads, t, t), cross (Ld, B, heads, t, N), mean (Ld, B, t, N) = the cross maps averaged over the
    heads); a part that was not asked for comes back with no rows.  N counts the CLS row 0.  The session record is left as it is."""
    e = _eng(engine)
    ses = session(e, "decode_attn")
    B = ses.rows
    tokens = _i64_dev(tokens, "tokens", e, B, 2, "(B, t) matching the session started by texocr::decode_begin")
    if not (want_self or want_cross or want_mean):
        raise ValueError("texocr::decode_attn: ask for at least one of the self, cross and head-mean maps")
    shapes = _attn_shapes(e.dims, B, int(tokens.shape[1]), _session_keys(e, ses), want_logits, want_self, want_cross, want_mean)
    outs = [torch.empty(sh, device=tokens.device, dtype=torch.float32) for sh in shapes]
    _call(e, "txo_decode_attn", tokens.data_ptr(), int(tokens.shape[1]), *[o.data_ptr() if o.shape[0] else None for o in outs])
    return outs[0], outs[1], outs[2], outs[3]


@decode_attn.register_fake
def _(tokens, engine, want_logits, want_self, want_cross, want_mean):
    e = _eng(engine)
    shapes = _attn_shapes(e.dims, tokens.shape[0], tokens.shape[1], _session_keys(e, session(e, "decode_attn")), want_logits, want_self,
                          want_cross, want_mean)
    return tuple(tokens.new_empty(sh, dtype=torch.float32) for sh in shapes)


class _Gen(NamedTuple):
    """what a token decode returns; an output that was not asked for has no rows"""
    toks: torch.Tensor          # (B, max_len) int64, of which the first n columns are valid
    n: torch.Tensor             # int64 CPU tensor of shape (1,)
    logp: torch.Tensor          # (B, max_len) float32
    logits: torch.Tensor        # (B, max_len, V) float32
    plogp: torch.Tensor         # (B, P) float32: the forced tokens of a prompted decode


def _gen_shapes(src, vocab: int, max_len: int, want_logits: bool, want_logp: bool, prefix) -> _Gen:
    """the outputs of every texocr::generate* op, real and fake alike (new_empty: on src's device, or meta)"""
    B = src.shape[0]
    return _Gen(src.new_empty((B, max_len), dtype=torch.int64), torch.empty((1,), dtype=torch.int64, device="cpu"),
                src.new_empty((B if want_logp else 0, max_len), dtype=torch.float32),
                src.new_empty((B if want_logits else 0, max_len, vocab), dtype=torch.float32),
                src.new_empty((B if want_logp and prefix is not None else 0, 0 if prefix is None else prefix.shape[1]), dtype=torch.float32))


def _gen_fake(src, engine, max_len, want_logits=False, want_logp=False, prefix=None) -> _Gen:
    return _gen_shapes(src, _eng(engine).dims.vocab, max_len, want_logits, want_logp, prefix)


def _generate(src: torch.Tensor, engine: int, max_len: int, eos: int, *, kind: str = "", sizes=None, want_logits: bool = False,
              want_logp: bool = False, prefix=None, prefix_len=None) -> _Gen:
    """The body of the nine texocr::generate* ops: checks the source (kind "": images (B, C, H, W); "_from_enc": encoder rows (B, N, D);
    "_ragged": a container + sizes) and the prefix, allocates the outputs, and makes the one call txo_generate[_prefix]<kind>[_logp]."""
    e = _eng(engine, ready=True)
    if kind == "_from_enc":
        src = _enc_arg(src, e)
        head = (src.data_ptr(), src.shape[0], src.shape[1])
    else:
        src, sizes = _ragged_args(src, sizes, e) if kind else (_img_arg(src, e), None)
        head = (src.data_ptr(), *src.shape) + ((_i32p(sizes),) if kind else ())
    B = src.shape[0]
    if prefix is not None:
        prefix, prefix_len = _prefix_args(prefix, prefix_len, e, B, max_len)
    g = _gen_shapes(src, e.dims.vocab, max_len, want_logits, want_logp, prefix)
    if os.environ.get("TXO_DEBUG_POISON"):      # tests: a column the engine returns as valid but never wrote shows as -7, a log-probability as nan
        g.toks.fill_(-7)
        g.logp.fill_(float("nan"))
    n = C.c_int32(0)
    ptr = lambda t, want: t.data_ptr() if want else None
    if prefix is not None:
        fn = "txo_generate_prefix" + kind
        tail = (prefix.data_ptr(), int(prefix.shape[1]), None if prefix_len is None else _i32p(prefix_len), int(max_len), int(eos), g.toks.data_ptr(),
                C.byref(n), ptr(g.logp, want_logp), ptr(g.plogp, want_logp))
    else:
        fn = "txo_generate" + kind + ("_logp" if want_logp else "")
        tail = (int(max_len), int(eos), g.toks.data_ptr(), C.byref(n)) + (() if kind == "_ragged" else (ptr(g.logits, want_logits),)) \
            + ((g.logp.data_ptr(),) if want_logp else ())
    _call(e, fn, *head, *tail, leaves=() if kind == "_ragged" else (B, src))   # nothing ragged outlives the call (engine.hip: generate_common)
    return g._replace(n=torch.tensor([n.value], dtype=torch.int64))


@custom_op("texocr::generate", mutates_args=())
def generate(img: torch.Tensor, engine: int, max_len: int, eos: int, want_logits: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Greedy OCRModel.generate: (tokens (B, max_len) of which the first n are valid, n as an int64 CPU tensor of shape (1,),
    logits (B, max_len, V) or (0, max_len, V)).  eos < 0: no eos test (eos_tok=None)."""
    g = _generate(img, engine, max_len, eos, want_logits=want_logits)
    return g.toks, g.n, g.logits


@custom_op("texocr::generate_from_enc", mutates_args=())
def generate_from_enc(enc: torch.Tensor, engine: int, max_len: int, eos: int, want_logits: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    g = _generate(enc, engine, max_len, eos, kind="_from_enc", want_logits=want_logits)
    return g.toks, g.n, g.logits


@generate.register_fake
@generate_from_enc.register_fake
def _(src, engine, max_len, eos, want_logits):
    g = _gen_fake(src, engine, max_len, want_logits)
    return g.toks, g.n, g.logits


def _logp_output(toks: torch.Tensor) -> torch.Tensor:
    logp = torch.empty(toks.shape, device=toks.device, dtype=torch.float32)
    if os.environ.get("TXO_DEBUG_POISON"):      # tests: a returned position the engine never wrote shows as nan
        logp.fill_(float("nan"))
    return logp


@custom_op("texocr::generate_logp", mutates_args=())
def generate_logp(img: torch.Tensor, engine: int, max_len: int, eos: int, want_logits: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """texocr::generate plus logp (B, max_len) float32: log_softmax(logits)[token] of every valid position, at temperature 1 over the
    whole vocabulary whatever the token selection (txo_generate_logp) -> (tokens, n, logp, logits (B, max_len, V) or (0, max_len, V))."""
    g = _generate(img, engine, max_len, eos, want_logits=want_logits, want_logp=True)
    return g.toks, g.n, g.logp, g.logits


@custom_op("texocr::generate_from_enc_logp", mutates_args=())
def generate_from_enc_logp(enc: torch.Tensor, engine: int, max_len: int, eos: int, want_logits: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    g = _generate(enc, engine, max_len, eos, kind="_from_enc", want_logits=want_logits, want_logp=True)
    return g.toks, g.n, g.logp, g.logits


@generate_logp.register_fake
@generate_from_enc_logp.register_fake
def _(src, engine, max_len, eos, want_logits):
    g = _gen_fake(src, engine, max_len, want_logits, True)
    return g.toks, g.n, g.logp, g.logits


@custom_op("texocr::generate_beam", mutates_args=())
def generate_beam(img: torch.Tensor, engine: int, beams: int, max_len: int, eos: int, want_all: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Beam search (build extension): (best tokens (B, max_len), scores (B, beams), all beams (B*beams, max_len) or (0, max_len),
    n as an int64 CPU tensor)."""
    e = _eng(engine, ready=True)
    img = _img_arg(img, e)
    B, Cc, H, W = img.shape
    toks = torch.empty((B, max_len), device=img.device, dtype=torch.int64)
    scores = torch.empty((B, beams), device=img.device, dtype=torch.float32)
    allt = torch.empty((B * beams if want_all else 0, max_len), device=img.device, dtype=torch.int64)
    n = C.c_int32(0)
    _call(e, "txo_generate_beam", img.data_ptr(), B, Cc, H, W, int(beams), int(max_len), int(eos), toks.data_ptr(), scores.data_ptr(),
          allt.data_ptr() if want_all else None, C.byref(n), leaves=(B, img))   # one row per IMAGE (engine.hip: struct Rows in generate_beam)
    return toks, scores, allt, torch.tensor([n.value], dtype=torch.int64)


@generate_beam.register_fake
def _(img, engine, beams, max_len, eos, want_all):
    B = img.shape[0]
    return (img.new_empty((B, max_len), dtype=torch.int64), img.new_empty((B, beams), dtype=torch.float32),
            img.new_empty((B * beams if want_all else 0, max_len), dtype=torch.int64), torch.empty((1,), dtype=torch.int64, device="cpu"))


# ---- ragged batches (build extension): images of different sizes in one call ---------------------------------------------------
@dataclass(frozen=True)
class PackedImages:
    """A ragged batch that is already in its container -- what pack_u8 / OCRModel.ingest return, and what every *_ragged method takes in
    place of a sequence of (C, H_b, W_b) tensors: box (B, C, Hc, Wc) float32 on the device, image b in the top-left corner of slot b and
    zeros around it; sizes (B, 2) int32 CPU = (H_b, W_b), multiples of 16.  len() is the number of images.
    views (pack_u8 with trim= / regions=; else None): (B, 4) int32 CPU = (y0, x0, h', w'), the rectangle of source image b that slot b holds, in
    SOURCE pixels and before the fit: what maps a return_align map or a peak patch back to the source."""
    box: torch.Tensor
    sizes: torch.Tensor
    views: Optional[torch.Tensor] = None

    def __len__(self) -> int:
        return int(self.box.shape[0])

    @property
    def device(self) -> torch.device:
        return self.box.device

    def grids(self, patch: int = 16):
        """the patch grid (H_b / patch, W_b / patch) of every image"""
        return [(int(h) // patch, int(w) // patch) for h, w in self.sizes.tolist()]


def pack_ragged(images: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """B images (C, H_b, W_b) -> (container (B, C, Hc, Wc) float32, sizes (B, 2) int32 CPU = (H_b, W_b)).  Image b sits in the
    top-left corner of its slot; Hc / Wc are the largest height / width; the rest of the container is zero (the engine never reads
    it).  Every side must be a positive multiple of 16; all images share C, the device and float32.  A PackedImages is passed through
    untouched: (its box, its sizes)."""
    if isinstance(images, PackedImages):         # already a container (pack_u8): handed on as it is
        return images.box, images.sizes
    if len(images) == 0:
        raise ValueError("pack_ragged: no images")
    first = images[0]
    if first.ndim != 3:
        raise ValueError("pack_ragged: every image must be (C, H, W)")
    Cc = first.shape[0]
    for i, im in enumerate(images):
        if im.ndim != 3 or im.shape[0] != Cc:
            raise ValueError(f"pack_ragged: image {i} must be ({Cc}, H, W), got {tuple(im.shape)}")
        if im.dtype != torch.float32:
            raise ValueError(f"pack_ragged: image {i} must be float32, got {im.dtype}")
        if im.device != first.device:
            raise ValueError(f"pack_ragged: image {i} lives on {im.device}, image 0 on {first.device}")
        h, w = int(im.shape[1]), int(im.shape[2])
        if h <= 0 or w <= 0 or h % 16 or w % 16:
            raise ValueError(f"pack_ragged: image {i} is {h}x{w}; sides must be positive multiples of 16")
    Hc, Wc = max(int(im.shape[1]) for im in images), max(int(im.shape[2]) for im in images)
    box = torch.zeros((len(images), Cc, Hc, Wc), dtype=torch.float32, device=first.device)
    for b, im in enumerate(images):
        box[b, :, :im.shape[1], :im.shape[2]] = im
    sizes = torch.tensor([[int(im.shape[1]), int(im.shape[2])] for im in images], dtype=torch.int32)
    return box, sizes


def _ragged_args(img: torch.Tensor, sizes: torch.Tensor, e):
    if img.ndim != 4:
        raise ValueError("expected a container of shape (B, C, Hc, Wc)")
    img = _f32_dev(img, "container", e)
    if sizes.is_cuda or sizes.dtype != torch.int32 or sizes.ndim != 2 or tuple(sizes.shape) != (img.shape[0], 2):
        raise ValueError("sizes must be an int32 CPU tensor of shape (B, 2) = (H_b, W_b): launch geometry depends on them")
    return img, sizes.contiguous()


def _i32p(t: torch.Tensor):
    return C.cast(t.data_ptr(), C.POINTER(C.c_int32))


def ragged_tokens(sizes: torch.Tensor) -> torch.Tensor:
    """(B, 2) image sizes -> (B,) int32 encoder tokens per image, 1 + (H_b / 16)(W_b / 16)"""
    return (1 + (sizes[:, 0] // 16) * (sizes[:, 1] // 16)).to(torch.int32)


@custom_op("texocr::encode_ragged", mutates_args=())
def encode_ragged(img: torch.Tensor, sizes: torch.Tensor, engine: int) -> torch.Tensor:
    """txo_encode_ragged: container (B, C, Hc, Wc) + sizes (B, 2) int32 CPU -> enc (B, Ns, D), Ns = the largest token count; rows
    behind an image's own count are zeros."""
    e = _eng(engine, ready=True)
    img, sizes = _ragged_args(img, sizes, e)
    B, Cc, Hc, Wc = img.shape
    ns = int(ragged_tokens(sizes).max()) if B else 1
    out = torch.empty((B, max(ns, 1), e.dims.embed_dim), device=img.device, dtype=torch.float32)
    n = C.c_int32(0)
    _call(e, "txo_encode_ragged", img.data_ptr(), B, Cc, Hc, Wc, _i32p(sizes), out.data_ptr(), C.byref(n))
    if n.value != out.shape[1]:
        raise RuntimeError(f"texocr::encode_ragged: the engine's slot stride {n.value} is not the binding's {out.shape[1]}")
    return out


@encode_ragged.register_fake
def _(img, sizes, engine):
    d = _eng(engine).dims
    ns = int(ragged_tokens(sizes).max())
    return img.new_empty((img.shape[0], ns, d.embed_dim), dtype=torch.float32)


@custom_op("texocr::decode_begin_ragged", mutates_args=())
def decode_begin_ragged(enc: torch.Tensor, n_tokens: torch.Tensor, engine: int) -> None:
    """txo_decode_begin_ragged: enc (B, Ns, D) as encode_ragged returns it, n_tokens (B,) int32 CPU = valid rows per image."""
    e = _eng(engine, ready=True)
    enc = _enc_arg(enc, e, "Ns")
    if n_tokens.is_cuda or n_tokens.dtype != torch.int32 or tuple(n_tokens.shape) != (enc.shape[0],):
        raise ValueError("n_tokens must be an int32 CPU tensor of shape (B,)")
    n_tokens = n_tokens.contiguous()
    _call(e, "txo_decode_begin_ragged", enc.data_ptr(), enc.shape[0], enc.shape[1], _i32p(n_tokens), leaves=(enc.shape[0], enc))


@custom_op("texocr::score_ragged", mutates_args=())
def score_ragged(img: torch.Tensor, sizes: torch.Tensor, tokens: torch.Tensor, mask: Optional[torch.Tensor], engine: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """txo_score_ragged: container (B, C, Hc, Wc) + sizes (B, 2) int32 CPU, tokens (B, L) int64, mask (B, L) bool / uint8 (False = padding) or
    None -> (logp, top1, top1_logp), each (B, L-1), row b what the fixed-shape pipeline gives image b on its own.  The ragged session stays open."""
    e = _eng(engine, ready=True)
    img, sizes = _ragged_args(img, sizes, e)
    B, Cc, Hc, Wc = img.shape
    tokens = _i64_dev(tokens, "tokens", e, B, 2, "(B, L) with one row per image")
    L = int(tokens.shape[1])
    if L < 2 or L - 1 > e.dims.max_len:
        raise ValueError(f"tokens must have 2 <= L <= max_len + 1 = {e.dims.max_len + 1} columns, got {L}")
    m8 = None
    if mask is not None:
        if tuple(mask.shape) != (B, L) or not mask.is_cuda:
            raise ValueError("mask must be a GPU tensor of the shape of tokens")
        m8 = mask.to(torch.uint8).contiguous()
    logp = torch.empty((B, L - 1), device=tokens.device, dtype=torch.float32)
    top1 = torch.empty((B, L - 1), device=tokens.device, dtype=torch.int64)
    top1_logp = torch.empty((B, L - 1), device=tokens.device, dtype=torch.float32)
    _call(e, "txo_score_ragged", img.data_ptr(), B, Cc, Hc, Wc, _i32p(sizes), tokens.data_ptr(), None if m8 is None else m8.data_ptr(), L,
          logp.data_ptr(), top1.data_ptr(), top1_logp.data_ptr(), leaves=(B, img, int(ragged_tokens(sizes).max())))
    return logp, top1, top1_logp


@score_ragged.register_fake
def _(img, sizes, tokens, mask, engine):
    B, L = tokens.shape
    return (tokens.new_empty((B, L - 1), dtype=torch.float32), tokens.new_empty((B, L - 1), dtype=torch.int64),
            tokens.new_empty((B, L - 1), dtype=torch.float32))


@decode_begin.register_fake
@decode_begin_ragged.register_fake
@decode_set_key_mask.register_fake
def _(*args):
    return None


@custom_op("texocr::generate_ragged", mutates_args=())
def generate_ragged(img: torch.Tensor, sizes: torch.Tensor, engine: int, max_len: int, eos: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """txo_generate_ragged: (tokens (B, max_len) of which the first n are valid, n as an int64 CPU tensor of shape (1,))."""
    g = _generate(img, engine, max_len, eos, kind="_ragged", sizes=sizes)
    return g.toks, g.n


@generate_ragged.register_fake
def _(img, sizes, engine, max_len, eos):
    return _gen_fake(img, engine, max_len)[:2]


def _beam_outputs(img: torch.Tensor, beams: int, max_len: int, want_logp: bool, length_alpha: float):
    """the four outputs of a beam search over img.shape[0] images and the txo_beam_out that names them"""
    rows = img.shape[0] * int(beams)
    toks = torch.empty((rows, max_len), device=img.device, dtype=torch.int64)
    if os.environ.get("TXO_DEBUG_POISON"):      # tests: a column the engine returns as valid but never wrote shows as -7
        toks.fill_(-7)
    scores = torch.empty((rows,), device=img.device, dtype=torch.float32)
    lengths = torch.empty((rows,), device=img.device, dtype=torch.int32)
    logp = _logp_output(toks) if want_logp else torch.empty((0, max_len), device=img.device, dtype=torch.float32)
    out = _lib.TxoBeamOut(toks.data_ptr(), scores.data_ptr(), logp.data_ptr() if want_logp else None, lengths.data_ptr(), float(length_alpha))
    return toks, scores, lengths, logp, out


@custom_op("texocr::beam_search", mutates_args=())
def beam_search(img: torch.Tensor, engine: int, beams: int, max_len: int, eos: int, want_logp: bool,
                length_alpha: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """txo_beam_search: (tokens (B*beams, max_len) of which the first n columns are valid, scores (B*beams,), lengths (B*beams,) int32,
    logp (B*beams, max_len) or (0, max_len), n as an int64 CPU tensor of shape (1,)); row b * beams + i is the i-th best beam of image b."""
    e = _eng(engine, ready=True)
    img = _img_arg(img, e)
    B, Cc, H, W = img.shape
    toks, scores, lengths, logp, out = _beam_outputs(img, beams, max_len, want_logp, length_alpha)
    n = C.c_int32(0)
    _call(e, "txo_beam_search", img.data_ptr(), B, Cc, H, W, int(beams), int(max_len), int(eos), C.byref(out), C.byref(n),
          leaves=(B, img))                      # one row per IMAGE, as behind txo_generate_beam
    return toks, scores, lengths, logp, torch.tensor([n.value], dtype=torch.int64)


@custom_op("texocr::beam_search_ragged", mutates_args=())
def beam_search_ragged(img: torch.Tensor, sizes: torch.Tensor, engine: int, beams: int, max_len: int, eos: int, want_logp: bool,
                       length_alpha: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """txo_beam_search_ragged: texocr::beam_search over a container (B, C, Hc, Wc) + sizes (B, 2) int32 CPU."""
    e = _eng(engine, ready=True)
    img, sizes = _ragged_args(img, sizes, e)
    B, Cc, Hc, Wc = img.shape
    toks, scores, lengths, logp, out = _beam_outputs(img, beams, max_len, want_logp, length_alpha)
    n = C.c_int32(0)
    _call(e, "txo_beam_search_ragged", img.data_ptr(), B, Cc, Hc, Wc, _i32p(sizes), int(beams), int(max_len), int(eos), C.byref(out),
          C.byref(n), leaves=())                # nothing ragged outlives the call (engine.hip: beam_common)
    return toks, scores, lengths, logp, torch.tensor([n.value], dtype=torch.int64)


def _beam_fake(img, beams, max_len, want_logp):
    rows = img.shape[0] * beams
    return (img.new_empty((rows, max_len), dtype=torch.int64), img.new_empty((rows,), dtype=torch.float32),
            img.new_empty((rows,), dtype=torch.int32), img.new_empty((rows if want_logp else 0, max_len), dtype=torch.float32),
            torch.empty((1,), dtype=torch.int64, device="cpu"))


@beam_search.register_fake
def _(img, engine, beams, max_len, eos, want_logp, length_alpha):
    return _beam_fake(img, beams, max_len, want_logp)


@beam_search_ragged.register_fake
def _(img, sizes, engine, beams, max_len, eos, want_logp, length_alpha):
    return _beam_fake(img, beams, max_len, want_logp)


# ---- prompted decode (txo_generate_prefix*): generate()'s loop continued behind a caller's token prefix -------------------------------
def check_prefix(prefix_shape, prefix_len, max_len: int, table: int, workspace: Optional[int] = None) -> Tuple[int, int]:
    """The refusals of a prompted decode that need no device (ValueError, every message names the prefix), shared by the operators and
    the facades so that they fire before the engine's session changes: prefix (B, P) with P >= 1; prefix_len None or B lengths in
    [1, P]; (longest - 1) + max_len inside the positional table (a prompted decode does not slide the window); (shortest - 1) rows
    inside the multi-position pass's workspace.  -> (shortest, longest)"""
    if len(prefix_shape) != 2 or prefix_shape[1] < 1:
        raise ValueError("prefix must be (B, P) with at least one column")
    B, P = int(prefix_shape[0]), int(prefix_shape[1])
    if int(max_len) < 1:
        raise ValueError("prefix decode: max_len must be >= 1")
    m = M = P
    if prefix_len is not None:
        lens = [int(v) for v in (prefix_len.tolist() if hasattr(prefix_len, "tolist") else prefix_len)]
        if len(lens) != B:
            raise ValueError(f"prefix_len must have one entry per row of prefix ({B}), got {len(lens)}")
        if lens and (min(lens) < 1 or max(lens) > P):
            raise ValueError(f"prefix_len must be in [1, {P}] (the columns of prefix)")
        if lens:
            m, M = min(lens), max(lens)
    if M - 1 + int(max_len) > table:
        raise ValueError(f"prefix decode: the longest prefix ({M}) - 1 + max_len ({int(max_len)}) exceeds decoder.max_len ({table}); a prompted "
                         "decode does not slide the window")
    if workspace is not None and m - 1 > workspace:
        raise ValueError(f"prefix decode: the shortest prefix ({m}) does not fit the multi-position pass's workspace (max_batch * max_tokens = {workspace} rows)")
    return m, M


def _prefix_args(prefix: torch.Tensor, prefix_len: Optional[torch.Tensor], e, B: int, max_len: int):
    prefix = _i64_dev(prefix, "prefix", e, B, 2, "(B, P) with one row per image")
    if prefix_len is not None:
        if prefix_len.is_cuda or prefix_len.dtype != torch.int32 or tuple(prefix_len.shape) != (B,):
            raise ValueError("prefix_len must be an int32 CPU tensor of shape (B,): the loop's start and length depend on it")
        prefix_len = prefix_len.contiguous()
    ws = e.max_batch * e.max_tokens if hasattr(e, "max_batch") else None
    check_prefix(tuple(prefix.shape), prefix_len, max_len, e.dims.max_len, ws)
    return prefix, prefix_len


@custom_op("texocr::generate_prefix", mutates_args=())
def generate_prefix(img: torch.Tensor, prefix: torch.Tensor, prefix_len: Optional[torch.Tensor], engine: int, max_len: int, eos: int,
                    want_logp: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """txo_generate_prefix: prefix (B, P) int64 on the GPU, prefix_len (B,) int32 CPU or None (every row has length P) -> (tokens (B, max_len)
    of which the first n are valid -- column j of row b is the j-th token behind row b's own prefix --, n as an int64 CPU tensor of shape
    (1,), logp (B, max_len) or (0, max_len), prefix_logp (B, P) or (0, P): the log-probabilities of the forced tokens)."""
    g = _generate(img, engine, max_len, eos, want_logp=want_logp, prefix=prefix, prefix_len=prefix_len)
    return g.toks, g.n, g.logp, g.plogp


@custom_op("texocr::generate_prefix_from_enc", mutates_args=())
def generate_prefix_from_enc(enc: torch.Tensor, prefix: torch.Tensor, prefix_len: Optional[torch.Tensor], engine: int, max_len: int, eos: int,
                             want_logp: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    g = _generate(enc, engine, max_len, eos, kind="_from_enc", want_logp=want_logp, prefix=prefix, prefix_len=prefix_len)
    return g.toks, g.n, g.logp, g.plogp


@custom_op("texocr::generate_prefix_ragged", mutates_args=())
def generate_prefix_ragged(img: torch.Tensor, sizes: torch.Tensor, prefix: torch.Tensor, prefix_len: Optional[torch.Tensor], engine: int,
                           max_len: int, eos: int, want_logp: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """txo_generate_prefix_ragged: texocr::generate_prefix over a container (B, C, Hc, Wc) + sizes (B, 2) int32 CPU."""
    g = _generate(img, engine, max_len, eos, kind="_ragged", sizes=sizes, want_logp=want_logp, prefix=prefix, prefix_len=prefix_len)
    return g.toks, g.n, g.logp, g.plogp


def _prefix_fake(src, prefix, engine, max_len, want_logp):
    g = _gen_fake(src, engine, max_len, False, want_logp, prefix)
    return g.toks, g.n, g.logp, g.plogp


@generate_prefix.register_fake
@generate_prefix_from_enc.register_fake
def _(src, prefix, prefix_len, engine, max_len, eos, want_logp):
    return _prefix_fake(src, prefix, engine, max_len, want_logp)


@generate_prefix_ragged.register_fake
def _(img, sizes, prefix, prefix_len, engine, max_len, eos, want_logp):
    return _prefix_fake(img, prefix, engine, max_len, want_logp)


@custom_op("texocr::generate_ragged_logp", mutates_args=())
def generate_ragged_logp(img: torch.Tensor, sizes: torch.Tensor, engine: int, max_len: int, eos: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """txo_generate_ragged_logp: texocr::generate_ragged plus logp (B, max_len) float32 -> (tokens, n, logp)."""
    g = _generate(img, engine, max_len, eos, kind="_ragged", sizes=sizes, want_logp=True)
    return g.toks, g.n, g.logp


@generate_ragged_logp.register_fake
def _(img, sizes, engine, max_len, eos):
    return _gen_fake(img, engine, max_len, False, True)[:3]


# ---- constrained decode (txo_set_token_rules): which tokens the loop of the generate family may pick (texocr_amd/rules.py builds the tables) ----
@custom_op("texocr::set_token_rules", mutates_args=())
def set_token_rules(table: Optional[torch.Tensor], engine: int, depth_max: int) -> None:
    """txo_set_token_rules: table (S, V) int32 on the CPU, packed as texocr_amd.rules.pack packs an entry, and its depth cap; None: off (the
    default).  The engine checks the table and names what it refuses (ValueError).  ``engine.token_rules`` records what is installed."""
    e = _eng(engine, ready=True)
    if table is None:
        with torch.cuda.device(e.device):
            _lib.check(e.lib.txo_set_token_rules(e.handle, None, 0, 0, 0))
        e.token_rules = None
        return
    if table.is_cuda or table.dtype != torch.int32 or table.ndim != 2:
        raise ValueError("token rules: table must be an int32 CPU tensor of shape (S, V)")
    table = table.contiguous()
    with torch.cuda.device(e.device):
        _lib.check(e.lib.txo_set_token_rules(e.handle, table.data_ptr(), int(table.shape[0]), int(table.shape[1]), int(depth_max)))
    e.token_rules = (table, int(depth_max))


@custom_op("texocr::last_rule_state", mutates_args=())
def last_rule_state(tokens: torch.Tensor, engine: int) -> torch.Tensor:
    """txo_last_rule_state: the (state, depth) of every row of the last constrained generate -> (B, 2) int32 beside its `tokens` (B, n)"""
    e = _eng(engine)
    if not tokens.is_cuda or tokens.ndim != 2 or tokens.device.index != e.device:
        raise ValueError("last_rule_state: tokens must be the (B, n) GPU tensor the constrained generate returned")
    out = torch.empty((tokens.shape[0], 2), device=tokens.device, dtype=torch.int32)
    _call(e, "txo_last_rule_state", out.data_ptr(), int(tokens.shape[0]))
    return out


@set_token_rules.register_fake
def _(table, engine, depth_max):
    return None


@last_rule_state.register_fake
def _(tokens, engine):
    return tokens.new_empty((tokens.shape[0], 2), dtype=torch.int32)


# ---- constrained beam search (txo_set_rules_beam): the opt-in that lets the beam entries run under token rules -----------------------------
@custom_op("texocr::set_rules_beam", mutates_args=())
def set_rules_beam(engine: int, on: bool) -> None:
    """txo_set_rules_beam: on=True, a beam search under token rules runs the constrained selection; False (the default), it is refused"""
    e = _eng(engine)
    with torch.cuda.device(e.device):
        _lib.check(e.lib.txo_set_rules_beam(e.handle, 1 if on else 0))


@custom_op("texocr::last_beam_rule_state", mutates_args=())
def last_beam_rule_state(tokens: torch.Tensor, engine: int) -> torch.Tensor:
    """txo_last_beam_rule_state: the (state, depth) of every beam of the last constrained beam search -> (B, beams, 2) int32 beside its
    `tokens` (B, beams, n), in their order"""
    e = _eng(engine)
    if not tokens.is_cuda or tokens.ndim != 3 or tokens.device.index != e.device:
        raise ValueError("last_beam_rule_state: tokens must be the (B, beams, n) GPU tensor the constrained beam search returned")
    out = torch.empty((tokens.shape[0], tokens.shape[1], 2), device=tokens.device, dtype=torch.int32)
    _call(e, "txo_last_beam_rule_state", out.data_ptr(), int(tokens.shape[0]), int(tokens.shape[1]))
    return out


@set_rules_beam.register_fake
def _(engine, on):
    return None


# ---- closing decode (txo_set_rules_close): the budget that ends every constrained row at an allowed eos inside the call's positions --------
@custom_op("texocr::set_rules_close", mutates_args=())
def set_rules_close(engine: int, on: bool) -> None:
    """txo_set_rules_close: on=True, a constrained decode / beam search only picks tokens from which eos can still be reached in the positions
    left; False (the default): the plain rules.  The engine refuses (ValueError) when rules are set and eos is unreachable from the start."""
    e = _eng(engine)
    with torch.cuda.device(e.device):
        _lib.check(e.lib.txo_set_rules_close(e.handle, 1 if on else 0))


@set_rules_close.register_fake
def _(engine, on):
    return None


# ---- repeat guard (txo_set_repeat_guard): no row of the generate family ends in max_repeats + 1 copies of a block of <= max_period tokens ----
@custom_op("texocr::set_repeat_guard", mutates_args=())
def set_repeat_guard(engine: int, max_period: int, max_repeats: int) -> None:
    """txo_set_repeat_guard: (max_period, max_repeats), both in [1, 16]; (0, 0): off (the default).  The engine names what it refuses
    (ValueError).  ``engine.repeat_guard`` records what is set."""
    e = _eng(engine)
    with torch.cuda.device(e.device):
        _lib.check(e.lib.txo_set_repeat_guard(e.handle, int(max_period), int(max_repeats)))
    e.repeat_guard = (int(max_period), int(max_repeats)) if max_period or max_repeats else None


@set_repeat_guard.register_fake
def _(engine, max_period, max_repeats):
    return None


# ---- alternatives per token (txo_set_alternatives): the k best ids / log-probabilities of every row the generate family picks from ----
@custom_op("texocr::set_alternatives", mutates_args=())
def set_alternatives(engine: int, k: int) -> None:
    """txo_set_alternatives: k in [1, 8], 0: off (the default).  The engine names what it refuses (ValueError).  ``engine.alts`` records k."""
    e = _eng(engine)
    with torch.cuda.device(e.device):
        _lib.check(e.lib.txo_set_alternatives(e.handle, int(k)))
    e.alts = int(k)


@set_alternatives.register_fake
def _(engine, k):
    return None


@custom_op("texocr::last_alternatives", mutates_args=())
def last_alternatives(tokens: torch.Tensor, engine: int, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """txo_last_alternatives: the alternatives of the last generate beside its `tokens` (B, n) -> (ids (B, n, k) int32, logp (B, n, k) float32);
    k is what that generate ran with (the engine refuses if it ran without)."""
    e = _eng(engine)
    if not tokens.is_cuda or tokens.ndim != 2 or tokens.device.index != e.device:
        raise ValueError("last_alternatives: tokens must be the (B, n) GPU tensor the generate returned")
    B, n = int(tokens.shape[0]), int(tokens.shape[1])
    ids = torch.empty((B, n, int(k)), device=tokens.device, dtype=torch.int32)
    lp = torch.empty((B, n, int(k)), device=tokens.device, dtype=torch.float32)
    with torch.cuda.device(e.device):
        out = C.c_int64(0)
        _lib.check(e.lib.txo_engine_query(e.handle, _lib.Q_LAST_ALTS, C.byref(out)))
    if out.value != int(k):
        raise ValueError(f"last_alternatives: the last generate kept {out.value} alternatives per token, not {int(k)}")
    _call(e, "txo_last_alternatives", ids.data_ptr(), lp.data_ptr(), B, n)
    return ids, lp


@last_alternatives.register_fake
def _(tokens, engine, k):
    return (tokens.new_empty((*tokens.shape, k), dtype=torch.int32), tokens.new_empty((*tokens.shape, k), dtype=torch.float32))


# ---- repeat guard inside beam search (txo_set_guard_beam): the opt-in that lets the beam entries run under a repeat guard --------------------
@custom_op("texocr::set_guard_beam", mutates_args=())
def set_guard_beam(engine: int, on: bool) -> None:
    """txo_set_guard_beam: on=True, a beam search under a repeat guard runs the guarded selection; False (the default), it is refused"""
    e = _eng(engine)
    with torch.cuda.device(e.device):
        _lib.check(e.lib.txo_set_guard_beam(e.handle, 1 if on else 0))


@set_guard_beam.register_fake
def _(engine, on):
    return None


def rules_close_dist(engine: int, n_states: int, depth_max: int) -> torch.Tensor:
    """txo_rules_close_dist: the distance table the engine computed for the installed rules -> (S, depth_max + 1) int32 on the CPU"""
    e = _eng(engine)
    out = torch.empty((int(n_states), int(depth_max) + 1), dtype=torch.int32)
    _lib.check(e.lib.txo_rules_close_dist(e.handle, out.data_ptr(), int(n_states), int(depth_max) + 1))
    return out


@last_beam_rule_state.register_fake
def _(tokens, engine):
    return tokens.new_empty((tokens.shape[0], tokens.shape[1], 2), dtype=torch.int32)


# ---- device-side image ingest (txo_ingest_u8): raw uint8 pixels -> the container of a ragged batch, one copy and one launch ----------
U8_ALIGN = 16        # byte alignment of every host image inside the staged buffer


def _u8_array(im, i: int):
    """one image of pack_u8's list -> a contiguous uint8 numpy array (host images) or a contiguous uint8 device tensor, of shape (H, W) or
    (H, W, ch).  PIL modes other than L / RGB / RGBA go through convert('RGB') first, as preprocess_image does with every mode."""
    import numpy as np
    if isinstance(im, torch.Tensor):
        if im.dtype != torch.uint8:
            raise ValueError(f"pack_u8: image {i} must be uint8, got {im.dtype}")
        a = im.contiguous() if im.is_cuda else np.ascontiguousarray(im.numpy())
    elif isinstance(im, np.ndarray):
        if im.dtype != np.uint8:
            raise ValueError(f"pack_u8: image {i} must be uint8, got {im.dtype}")
        a = np.ascontiguousarray(im)
    elif hasattr(im, "convert") and hasattr(im, "mode"):                       # a PIL image
        a = np.ascontiguousarray(np.asarray(im if im.mode in ("L", "RGB", "RGBA") else im.convert("RGB"), dtype=np.uint8))
    else:
        raise ValueError(f"pack_u8: image {i} must be a PIL image, a numpy array or a tensor, got {type(im).__name__}")
    if a.ndim not in (2, 3):
        raise ValueError(f"pack_u8: image {i} must be (H, W), (H, W, 3) or (H, W, 4), got {tuple(a.shape)}")
    return a


def plan_u8(images: Sequence):
    """The host side of pack_u8, no device needed: -> (staged, device_tensors, src, shapes).
    staged: uint8 CPU tensor (n,), every HOST image of the list (PIL, numpy, CPU tensor) copied in at an offset aligned to 16, in list order;
    device_tensors: the uint8 device tensors of the list, contiguous, used where they lie;
    src: int64 CPU (B, 2) = (k, byte offset): image b starts `offset` bytes into the staged buffer (k = 0) or into device_tensors[k - 1];
    shapes: int32 CPU (B, 3) = (h, w, ch), ch = 1 for an (H, W) image.  The channel count is the engine's to judge (txo_ingest_u8).
    An OBJECT that appears several times in the list (a page passed once per region: pack_u8(regions=)) is staged, or listed in
    device_tensors, once; its entries of src name the same bytes."""
    import numpy as np
    seen = {}                                    # id(object of the list) -> (its array, its src entry)
    arrs, src, shapes, dev, total = [], [], [], [], 0
    for i, im in enumerate(images):
        if id(im) not in seen:
            a = _u8_array(im, i)
            if isinstance(a, torch.Tensor):
                dev.append(a)
                seen[id(im)] = (a, [len(dev), 0])
            else:
                seen[id(im)] = (a, [0, total])
                arrs.append((total, a))
                total = (total + a.size + U8_ALIGN - 1) // U8_ALIGN * U8_ALIGN
        a, where = seen[id(im)]
        shapes.append([a.shape[0], a.shape[1], a.shape[2] if a.ndim == 3 else 1])
        src.append(list(where))
    staged = np.zeros((total,), dtype=np.uint8)
    for o, a in arrs:
        staged[o:o + a.size] = a.reshape(-1)
    return (torch.from_numpy(staged), dev, torch.tensor(src, dtype=torch.int64).reshape(-1, 2),
            torch.tensor(shapes, dtype=torch.int32).reshape(-1, 3))


def box_u8(shapes: torch.Tensor) -> Tuple[int, int]:
    """(Hc, Wc) of the smallest container that holds the list: the maxima of the heights / widths rounded up to 16 (txo_ingest_box's rule)"""
    if shapes.shape[0] == 0:
        return 0, 0
    r = (shapes[:, :2].to(torch.int64) + 15) // 16 * 16
    return int(r[:, 0].max()), int(r[:, 1].max())


@custom_op("texocr::ingest_u8", mutates_args=())
def ingest_u8(bufs: Sequence[torch.Tensor], src: torch.Tensor, shapes: torch.Tensor, engine: int, channels: int, Hc: int,
              Wc: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """txo_ingest_u8: bufs = uint8 device tensors that hold the pixels (contiguous), src (B, 2) int64 CPU = (index into bufs, byte offset),
    shapes (B, 3) int32 CPU = (h, w, ch) -> (box (B, channels, Hc, Wc) float32 with every element written, sizes (B, 2) int32 CPU = (h, w)
    rounded up to 16).  One launch; the refusals are the engine's (ValueError with its message)."""
    return _ingest_container("txo_ingest_u8", bufs, src, shapes, engine=engine, channels=channels, box=(Hc, Wc))


def _u8_source(bufs: Sequence[torch.Tensor], src: torch.Tensor, shapes: torch.Tensor, e):
    """the checks texocr::ingest_u8 and ingest_u8_fit share -> (base address, offsets (B,) int64 CPU from it, shapes contiguous)"""
    B = int(shapes.shape[0])
    if src.is_cuda or src.dtype != torch.int64 or tuple(src.shape) != (B, 2):
        raise ValueError("src must be an int64 CPU tensor of shape (B, 2) = (index into bufs, byte offset)")
    if shapes.is_cuda or shapes.dtype != torch.int32 or shapes.ndim != 2 or shapes.shape[1] != 3:
        raise ValueError("shapes must be an int32 CPU tensor of shape (B, 3) = (h, w, ch)")
    for k, t in enumerate(bufs):
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"bufs[{k}] must be a contiguous uint8 GPU tensor")
        if t.device.index != e.device:
            raise ValueError(f"bufs[{k}] lives on cuda:{t.device.index} but the engine was created on cuda:{e.device}")
    shapes = shapes.contiguous()
    first = []                                   # the address of every image's first byte
    for b, ((k, off), (h, w, ch)) in enumerate(zip(src.tolist(), shapes.tolist())):
        if not 0 <= k < len(bufs) or off < 0:
            raise ValueError(f"src[{b}] = ({k}, {off}) does not name a byte of bufs")
        if h >= 1 and w >= 1 and ch >= 1 and off + h * w * ch > bufs[k].numel():      # (anything else is the engine's to refuse)
            raise ValueError(f"image {b}: {h}x{w}x{ch} bytes from offset {off} reach beyond bufs[{k}] ({bufs[k].numel()} bytes)")
        first.append(bufs[k].data_ptr() + off)
    base = min(first) if first else 0
    return base, torch.tensor([p - base for p in first], dtype=torch.int64), shapes


def _ingest_container(entry: str, bufs, src, shapes, *, engine: int, channels: int, box: Tuple[int, int], views=None,
                      fit: Optional[Tuple[int, int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The one body of texocr::ingest_u8 / ingest_u8_fit / ingest_u8_view, each on its own C entry point `entry`: the source checks, the view
    check (views given), the scratch of the horizontal passes (fit given; txo_ingest_fit_scratch, a tensor of this call: nothing is
    allocated when no image is oversized), the outputs and the one call.  box = (Hc, Wc); a view op without a fit passes the target 0 x 0."""
    e = _eng(engine)
    base, offsets, shapes = _u8_source(bufs, src, shapes, e)      # (the bound check is on the full images)
    dev = torch.device("cuda", e.device)
    B, Hc, Wc = int(shapes.shape[0]), int(box[0]), int(box[1])
    Fh, Fw = (0, 0) if fit is None else (int(fit[0]), int(fit[1]))
    fitted = shapes if fit is not None else None                  # the list the fit is applied to
    if views is not None:
        if views.is_cuda or views.dtype != torch.int32 or tuple(views.shape) != (B, 4):
            raise ValueError("views must be an int32 CPU tensor of shape (B, 4) = (y0, x0, h, w)")
        views = views.contiguous()
        if fit is not None:                                       # (a view the engine is about to refuse asks for no scratch)
            fitted = view_shapes(shapes, views).contiguous() if _views_inside(shapes, views) else None
    need = C.c_int64(0)
    if fitted is not None:
        _lib.check(_lib.load().txo_ingest_fit_scratch(_i32p(fitted), B, Fh, Fw, C.byref(need)))
    scratch = torch.empty((need.value,), dtype=torch.uint8, device=dev) if need.value else None
    # (a view op sizes the container from its views: where they are about to be refused, the engine is still given the box as it came)
    out = torch.empty((B, int(channels)) + ((Hc, Wc) if views is None else (max(Hc, 0), max(Wc, 0))), device=dev, dtype=torch.float32)
    if os.environ.get("TXO_DEBUG_POISON"):      # tests: an element the kernel left unwritten shows as nan
        out.fill_(float("nan"))
    sizes = torch.zeros((B, 2), dtype=torch.int32)
    args = [base, C.cast(offsets.data_ptr(), C.POINTER(C.c_int64)), _i32p(shapes)] + ([] if views is None else [_i32p(views)]) + [B, int(channels)]
    args += [Hc, Wc, out.data_ptr(), _i32p(sizes)] if entry == "txo_ingest_u8" else \
            [Fh, Fw, Hc, Wc, out.data_ptr(), _i32p(sizes), scratch.data_ptr() if scratch is not None else None, need.value]
    _call(e, entry, *args)
    return out, sizes


def _ingest_container_fake(bufs, src, shapes, *rest):
    """the outputs of the three container ops, whose arguments end in channels, [Fh, Fw,] Hc, Wc"""
    B, channels, (Hc, Wc) = shapes.shape[0], rest[-3 if len(rest) == 4 else -5], rest[-2:]
    return bufs[0].new_empty((B, channels, Hc, Wc), dtype=torch.float32), torch.empty((B, 2), dtype=torch.int32, device="cpu")


# ---- fit-to-canvas ingest (txo_ingest_u8_fit): an oversized image is downscaled on the device, bit for bit PIL's BILINEAR resize ----------
FIT_MAX_SCALE = 32       # an axis that would shrink by more than this is refused (txo_ingest_fit)


def fit_size(h: int, w: int, Fh: int, Fw: int) -> Tuple[int, int]:
    """txo_ingest_fit's rule in Python integers: (h, w) -> the size it is given under the target (Fh, Fw).  An image that fits is unchanged
    (never upscaled); otherwise the binding side becomes the target's and the other keeps the aspect ratio, rounded down, at least 1."""
    h, w, Fh, Fw = int(h), int(w), int(Fh), int(Fw)
    if h <= Fh and w <= Fw:
        return h, w
    if w * Fh <= h * Fw:
        return Fh, max(1, (w * Fh) // h)
    return max(1, (h * Fw) // w), Fw


def fit_shapes(shapes: torch.Tensor, Fh: int, Fw: int) -> torch.Tensor:
    """shapes (B, 3) = (h, w, ch) -> the same with every (h, w) fitted to (Fh, Fw): what box_u8 sizes the container of a fitted list from"""
    out = shapes.clone()
    for b, (h, w, _) in enumerate(shapes.tolist()):
        if h >= 1 and w >= 1:                    # (anything else is the engine's to refuse)
            out[b, 0], out[b, 1] = fit_size(h, w, Fh, Fw)
    return out


@custom_op("texocr::ingest_u8_fit", mutates_args=())
def ingest_u8_fit(bufs: Sequence[torch.Tensor], src: torch.Tensor, shapes: torch.Tensor, engine: int, channels: int, Fh: int, Fw: int,
                  Hc: int, Wc: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """txo_ingest_u8_fit: texocr::ingest_u8 with every image that exceeds (Fh, Fw) downscaled to fit it first (fit_size; bit for bit PIL's
    BILINEAR resize of its L / RGB channels) -> (box (B, channels, Hc, Wc), sizes (B, 2) int32 CPU = the FITTED sizes rounded up to 16).
    The scratch of the horizontal passes (txo_ingest_fit_scratch) is a tensor of this call; nothing is allocated when no image is oversized."""
    return _ingest_container("txo_ingest_u8_fit", bufs, src, shapes, engine=engine, channels=channels, box=(Hc, Wc), fit=(Fh, Fw))


# ---- trim-to-ink and region ingest (txo_ingest_trim_views / txo_ingest_u8_view): a rectangle of the source takes the image's place ----------
TRIM_LEVEL, TRIM_MARGIN = 127, 2     # the defaults: the mid-grey convention; a rim that keeps anti-aliased pixels lighter than the level


def _trim_args(level, margin) -> Tuple[int, int]:
    """the refusals of txo_ingest_trim_views about the rule's two numbers, in its words"""
    level, margin = int(level), int(margin)
    if not 0 <= level <= 254:
        raise ValueError(f"ingest: the trim level is {level}; it must lie in [0, 254] (a pixel is ink where a channel is <= level)")
    if margin < 0:
        raise ValueError(f"ingest: the trim margin is {margin}; it must be >= 0")
    return level, margin


def trim_view(arr, level: int = TRIM_LEVEL, margin: int = TRIM_MARGIN) -> Tuple[int, int, int, int]:
    """The trim rule of texocr.h "Trim-to-ink ingest" in numpy, on the bytes the ingest reads: arr uint8 (H, W) or (H, W, ch) with ch = 1
    (L), 3 (RGB) or 4 (RGBA: the alpha is not read) -> the view (y0, x0, h', w').  A pixel is ink iff min(read channels) <= level; the ink
    box is widened by `margin` pixels on every side and clamped to the image; an image without ink keeps (0, 0, H, W).  Product code: the
    wrapper's host path crops with it, and the engine's kernel (texocr::ingest_trim_views) gives the same four numbers."""
    import numpy as np
    level, margin = _trim_args(level, margin)
    a = np.asarray(arr)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"trim_view: the image must be uint8 (H, W) or (H, W, ch) with H, W >= 1, got {a.dtype} {tuple(a.shape)}")
    ink = (a if a.ndim == 2 else a[..., :3].min(axis=2)) <= level
    h, w = ink.shape
    ys, xs = np.flatnonzero(ink.any(axis=1)), np.flatnonzero(ink.any(axis=0))
    if ys.size == 0:
        return 0, 0, h, w
    y0, y1 = max(0, int(ys[0]) - margin), min(h, int(ys[-1]) + 1 + margin)
    x0, x1 = max(0, int(xs[0]) - margin), min(w, int(xs[-1]) + 1 + margin)
    return y0, x0, y1 - y0, x1 - x0


@custom_op("texocr::ingest_trim_views", mutates_args=())
def ingest_trim_views(bufs: Sequence[torch.Tensor], src: torch.Tensor, shapes: torch.Tensor, engine: int, level: int, margin: int) -> torch.Tensor:
    """txo_ingest_trim_views: bufs / src / shapes as texocr::ingest_u8 takes them -> views (B, 4) int32 CPU = (y0, x0, h', w') by trim_view's
    rule, from ONE launch over the bytes on the device.  SYNCHRONOUS (the one wait of the ingest path: the container's size depends on it)."""
    e = _eng(engine)
    base, offsets, shapes = _u8_source(bufs, src, shapes, e)
    B = int(shapes.shape[0])
    views = torch.zeros((B, 4), dtype=torch.int32)
    _call(e, "txo_ingest_trim_views", base, C.cast(offsets.data_ptr(), C.POINTER(C.c_int64)), _i32p(shapes), B, int(level), int(margin), _i32p(views))
    return views


@ingest_trim_views.register_fake
def _(bufs, src, shapes, engine, level, margin):
    return torch.empty((shapes.shape[0], 4), dtype=torch.int32, device="cpu")


def view_shapes(shapes: torch.Tensor, views: torch.Tensor) -> torch.Tensor:
    """shapes (B, 3) = (h, w, ch), views (B, 4) = (y0, x0, h', w') -> (B, 3) = (h', w', ch): the list the container is sized from"""
    out = shapes.clone()
    out[:, :2] = views[:, 2:4]
    return out


def _views_inside(shapes: torch.Tensor, views: torch.Tensor) -> bool:
    v, s = views.to(torch.int64), shapes.to(torch.int64)
    return bool(((v[:, 2:] >= 1) & (v[:, :2] >= 0) & (v[:, :2] + v[:, 2:] <= s[:, :2])).all())


@custom_op("texocr::ingest_u8_view", mutates_args=())
def ingest_u8_view(bufs: Sequence[torch.Tensor], src: torch.Tensor, shapes: torch.Tensor, views: torch.Tensor, engine: int, channels: int, Fh: int,
                   Fw: int, Hc: int, Wc: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """txo_ingest_u8_view: texocr::ingest_u8 (Fh = Fw = 0) or texocr::ingest_u8_fit of the rectangle views[b] = (y0, x0, h', w') of every source
    image (bufs / src / shapes describe the FULL images; entries may share bytes and views may overlap) -> (box, sizes) of the views, bit for
    bit what contiguous copies of them give.  Asynchronous; the refusals are the engine's."""
    return _ingest_container("txo_ingest_u8_view", bufs, src, shapes, engine=engine, channels=channels, box=(Hc, Wc), views=views,
                             fit=(Fh, Fw) if Fh or Fw else None)


for _op in (ingest_u8, ingest_u8_fit, ingest_u8_view):
    _op.register_fake(_ingest_container_fake)


def pack_u8(images: Sequence, in_channels: int, device, *, engine: int, fit: Optional[Tuple[int, int]] = None,
            trim: Optional[Tuple[int, int]] = None, regions=None) -> PackedImages:
    """Raw uint8 pixels -> the container of a ragged batch, prepared on the DEVICE: the counterpart of
    pack_ragged([wrapper._tensor(im) for im in images]), bit for bit, with one host-to-device copy of the pixel BYTES and one launch
    (texocr::ingest_u8 on the engine `engine`) instead of a float32 conversion, a copy and a slice assignment per image.
    images: PIL images, numpy arrays or uint8 tensors (CPU or `device`) of shape (H, W), (H, W, 3) or (H, W, 4) -- L, RGB, RGBA (alpha is
    ignored); sizes need not be multiples of 16 (the pad is zero).  Host images are concatenated into one buffer (every offset aligned to
    16) and sent in one copy; device tensors are used where they lie if they are contiguous.
    fit=(Fh, Fw) (default None: today's path): an image with a side beyond it is downscaled on the device to fit_size(h, w, Fh, Fw) first
    (texocr::ingest_u8_fit), bit for bit PIL's resize(..., BILINEAR) of its L / RGB channels; the container is sized by the fitted list.
    trim=(level, margin) (default None): every image is first cut to its ink and a margin (trim_view's rule, found on the device by
    texocr::ingest_trim_views -- the one wait of this call); regions=(B, 4) = (y0, x0, h, w): image b is cut to regions[b] -- pass a page
    once per region, it is staged (or, on the device, used) once.  Either way the view takes the image's place in front of the fit and
    the ingest, the result is bit for bit pack_u8 of contiguous copies a[y0:y0 + h, x0:x0 + w], and PackedImages.views holds the views in
    source pixels.  trim and regions together are a ValueError."""
    if trim is not None and regions is not None:
        raise ValueError("pack_u8: trim and regions are two ways to name the views; pass one of them")
    staged, dev, src, shapes = plan_u8(images)
    bufs = [staged.to(torch.device(device))] + dev
    views = None
    if trim is not None:
        level, margin = _trim_args(*trim)
        views = torch.ops.texocr.ingest_trim_views(bufs, src, shapes, int(engine), level, margin)
    elif regions is not None:
        views = torch.as_tensor(regions).to(device="cpu", dtype=torch.int32).reshape(-1, 4).contiguous()
        if views.shape[0] != shapes.shape[0]:
            raise ValueError(f"pack_u8: regions needs one (y0, x0, h, w) per image ({shapes.shape[0]}), got {views.shape[0]}")
    Fh, Fw = (0, 0) if fit is None else (int(fit[0]), int(fit[1]))
    sized = shapes if views is None else view_shapes(shapes, views)          # what the container holds: the images or their views, fitted
    Hc, Wc = box_u8(sized if fit is None else fit_shapes(sized, Fh, Fw))
    if views is not None:
        box, sizes = torch.ops.texocr.ingest_u8_view(bufs, src, shapes, views, int(engine), int(in_channels), Fh, Fw, Hc, Wc)
    elif fit is not None:
        box, sizes = torch.ops.texocr.ingest_u8_fit(bufs, src, shapes, int(engine), int(in_channels), Fh, Fw, Hc, Wc)
    else:
        box, sizes = torch.ops.texocr.ingest_u8(bufs, src, shapes, int(engine), int(in_channels), Hc, Wc)
    return PackedImages(box, sizes, views)
