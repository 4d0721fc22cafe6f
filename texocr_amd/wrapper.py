"""Serving front end around the engine (reference ``TeXOCRWrapper``, model/ocr_model.py:69-110): tokenizer +
checkpoint load + PIL image -> LaTeX string.

Differences from the reference, all on the host side of the path:
  * preprocessing is the inference part of ``img_transform`` (data_wrangling/dataset.py:365-371: ToTensor ->
    Grayscale(1) -> Invert) WITHOUT the train-time ``RandomAffine``; torchvision is not needed;
  * images whose sides are not multiples of 16 are padded (bottom/right, background = 0 after inversion); the
    reference relies on the dataset renderer having padded them already (render_data.py:81-92);
  * ``decode`` selects the reference's sampler ('sample', its default, temp 0.3), greedy, or 'beam' (build extension: the best of
    ``beams`` beams, OCRModel.beam_search);
  * ``max_len`` is passed through unchanged (default 350, ocr_model.py:94): beyond the positional table the decoder
    slides its window as the reference does.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .config import Dims
from .model import OCRModel, create_model
from .tokenizer import RegExTokenizer, process_output


def preprocess_image(img, patch: int = 16) -> torch.Tensor:
    """PIL image (any mode) -> (1, H', W') float32 in [0,1], white background -> 0, sides padded to multiples of 16."""
    a = np.asarray(img.convert("RGB"), dtype=np.float32) / 255.0                    # ToTensor
    g = 0.2989 * a[..., 0] + 0.587 * a[..., 1] + 0.114 * a[..., 2]                  # Grayscale (ITU-R 601-2 luma)
    g = 1.0 - g                                                                      # Invert (dataset.py:65-76)
    h, w = g.shape
    ph, pw = (-h) % patch, (-w) % patch
    if ph or pw:
        g = np.pad(g, ((0, ph), (0, pw)), constant_values=0.0)
    return torch.from_numpy(np.ascontiguousarray(g))[None]


def cut_at_eos(row: List[int], eos: Optional[int]) -> List[int]:
    """a generated row up to and including its first eos (the whole row if it has none)"""
    return row[:row.index(eos) + 1] if eos is not None and eos in row else row


def beam_chunk(max_batch: int, beams: int) -> int:
    """images per beam-search call of batch(decode='beam'): every image takes `beams` of the engine's max_batch decode rows"""
    if isinstance(beams, bool) or not isinstance(beams, int) or not 1 <= beams <= 8:
        raise ValueError(f"decode='beam' needs beams in [1, 8], got {beams!r}")
    if max_batch < beams:
        raise ValueError(f"decode='beam' with beams={beams} needs a wrapper created with max_batch >= {beams} (it has {max_batch})")
    return max_batch // beams


def align_inputs(rows: Sequence[List[int]], bos: int, pad: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """What batch(return_align=True) hands to OCRModel.align_ragged: rows = every image's tokens, cut at its eos (the eos included) ->
    (trg (B, L) int64 = [bos] + row padded with `pad` to the longest, mask (B, L) bool, False behind a row's own length).  Position p of
    row b is the one that produced rows[b][p]."""
    L = 1 + max(len(r) for r in rows)
    trg = torch.full((len(rows), L), pad, dtype=torch.int64)
    mask = torch.zeros((len(rows), L), dtype=torch.bool)
    for b, r in enumerate(rows):
        trg[b, 0] = bos
        trg[b, 1:1 + len(r)] = torch.tensor(r, dtype=torch.int64)
        mask[b, :1 + len(r)] = True
    return trg, mask


def pair_alts(tokenizer, ids, logp, n: int) -> List[List[Tuple[str, float]]]:
    """One row's alternatives for the caller: ids / logp (n_cols, k) as lists -> one list per kept token (the first n) of k (piece, logp) pairs,
    piece the tokenizer's string for the id (tokenizer.decode_list)"""
    return [list(zip(tokenizer.decode_list(ids[t]), [float(v) for v in logp[t]])) for t in range(n)]


def _split_result(res, return_logp: bool, ruled: bool, return_alts: int):
    """a generate's result -> (tokens, logp or None, Alts or None): the rule states dropped, the alternatives taken off the end"""
    res = res if isinstance(res, tuple) else (res,)
    if ruled:
        res = res[:-1]
    alts = None
    if return_alts:
        alts, res = res[-1], res[:-1]
    return res[0], (res[1] if return_logp else None), alts


class TeXOCRWrapper:
    def __init__(self, config: dict, dtype: str = "fp32", max_batch: int = 1, ragged_hybrid: bool = False, balanced: bool = False,
                 rules_beam: bool = False, close: bool = False, repeat_guard=None, guard_beam: bool = False):
        """repeat_guard=(max_period, max_repeats) (build extension): every __call__ / batch decodes under the repeat guard unless the call says
        otherwise (see batch)
        guard_beam=True (build extension): decode='beam' accepts a repeat guard -- the ban inside the beam selection (OCRModel.guard_beam);
        off, the default, the two together are a ValueError
        ragged_hybrid=True (build extension): batch() also works when config builds the hybrid ResNetV2 front end (OCRModel.ragged_hybrid)
        balanced=True (build extension): every __call__ / batch decodes under the brace rule of this tokenizer unless the call says otherwise
        (see batch)
        rules_beam=True (build extension): decode='beam' accepts balanced=True -- the brace rule inside the beam selection
        (OCRModel.rules_beam); off, the default, the two together are a ValueError
        close=True (build extension; only together with balanced): balanced decodes are closing decodes unless the call says otherwise (see batch)"""
        self.balanced = bool(balanced)
        self.close = bool(close)
        from . import guard
        self.repeat_guard = guard.check(repeat_guard)
        self._brace_rules = None
        self.tokenizer = RegExTokenizer()
        self.tokenizer.load(config["tokenizer_path"])                                # ocr_model.py:74-75
        config = dict(config)
        config["vocab_size"] = self.tokenizer.vocab_size                             # :78
        sd = None
        if config.get("model_path"):
            sd = torch.load(config["model_path"], map_location="cpu", weights_only=True)
            if "model_state_dict" in sd:                                             # utils.save_checkpoint layout (:52-61)
                sd = sd["model_state_dict"]
            key = "decoder.net.pos_embedding.embedding.weight"
            if key in sd:                                                            # ocr_model.py:84-88: the checkpoint decides
                config["max_length"] = int(sd[key].shape[0])
        self.model: OCRModel = create_model(config, dtype=dtype, max_batch=max_batch, ragged_hybrid=ragged_hybrid, rules_beam=rules_beam,
                                             guard_beam=guard_beam)
        if sd is not None:
            self.model.load_state_dict(sd)
        self.dims: Dims = self.model._engine.dims

    def _rules(self, balanced: Optional[bool], decode: str):
        """the rules= of a call: rules.brace_rules of the wrapper's tokenizer (built once) where balanced, else None"""
        if not (self.balanced if balanced is None else balanced):
            return None
        if decode == "beam" and not self.model.rules_beam:
            raise ValueError("balanced=True is not available with decode='beam' (beam search has no constrained form)")
        if self._brace_rules is None:
            from .rules import brace_rules
            self._brace_rules = brace_rules(self.tokenizer, vocab=self.dims.vocab, eos=self.model.eos_token,
                                            ban=(self.model.bos_token, self.model.trg_pad_idx)).validate(self.dims.vocab)
        return self._brace_rules

    def _close(self, close: Optional[bool], rules) -> dict:
        """the close= of a call as keyword arguments: the call's own setting, else the wrapper's where the call is balanced"""
        on = bool(self.close and rules is not None) if close is None else bool(close)
        if on and rules is None:
            raise ValueError("close=True needs balanced=True: the closing decode is a budget on top of the brace rule")
        return {"close": True} if on else {}

    def _guard(self, repeat_guard, decode: str) -> dict:
        """the repeat_guard= of a call as keyword arguments: the call's own (False: none), else the wrapper's"""
        g = self.repeat_guard if repeat_guard is None else (repeat_guard or None)
        if g is None:
            return {}
        if decode == "beam" and not self.model.guard_beam:
            raise ValueError("repeat_guard is not available with decode='beam' (the repeat guard binds generate() only)")
        return {"repeat_guard": g}

    def _alts(self, return_alts, decode: str) -> dict:
        """the return_alts= of a call as keyword arguments"""
        if not return_alts:
            return {}
        if decode == "beam":
            raise ValueError("return_alts is not available with decode='beam' (alternatives are kept by the greedy / sampled decode only)")
        from . import ops
        return {"return_alts": ops.check_alts(return_alts)}

    def _tensor(self, img) -> torch.Tensor:
        x = preprocess_image(img, self.dims.patch)
        if self.dims.in_channels != 1:
            x = x.expand(self.dims.in_channels, -1, -1)
        return x.contiguous()

    def _fitted(self, img, i: int = 0):
        """fit='canvas' on the host path: a PIL image with a side beyond the canvas -> PIL's resize(ops.fit_size, BILINEAR) of it, an L image
        as it is and any other mode through convert('RGB') first (the channels the ingest reads; PIL's own RGBA resize premultiplies by
        alpha).  An image that fits is returned untouched: PIL is called for oversized images only.  i: the image's place in its list, which
        the refusal names in the engine's words (txo_ingest_u8_fit)."""
        from PIL import Image
        from . import ops
        (w, h), (Fh, Fw) = img.size, self.dims.canvas_hw
        fh, fw = ops.fit_size(h, w, Fh, Fw)
        if (fh, fw) == (h, w):
            return img
        if h > ops.FIT_MAX_SCALE * fh or w > ops.FIT_MAX_SCALE * fw:
            raise ValueError(f"ingest: image {i} is {h}x{w}, {fh}x{fw} fitted to {Fh}x{Fw}: an axis shrinks by more than {ops.FIT_MAX_SCALE} times")
        return (img if img.mode == "L" else img.convert("RGB")).resize((fw, fh), Image.BILINEAR)

    @staticmethod
    def _trim_rule(trim: str, level: int, margin: int):
        """trim= / trim_level= / trim_margin= of batch and __call__ -> None ('none') or the rule's (level, margin), refused in the engine's words"""
        from . import ops
        if trim not in ("none", "ink"):
            raise ValueError(f"trim must be 'none' or 'ink', got {trim!r}")
        return ops._trim_args(level, margin) if trim == "ink" else None

    @staticmethod
    def _trimmed(img, rule):
        """trim='ink' on the host path: a PIL image -> its crop to ops.trim_view of the bytes the ingest reads (L / RGB / RGBA as they are, any
        other mode through convert('RGB')); an image whose view is the whole of it is returned untouched"""
        from . import ops
        y0, x0, h, w = ops.trim_view(ops._u8_array(img, 0), *rule)
        return img if (w, h) == img.size else img.crop((x0, y0, x0 + w, y0 + h))

    def _images(self, imgs: Sequence, ingest: str, fit: str = "none", trim=None):
        """imgs as one ragged call takes them -- ingest='host': a list of (C, H_b, W_b) tensors on the device, every image preprocessed
        on the host and copied on its own (the path that has always been there); 'device': ONE OCRModel.ingest over the raw pixels (a
        PackedImages, bit for bit the container the host path ends in).  fit='canvas': oversized images are downscaled to the canvas first,
        by PIL on the host path and by the engine on the device path, to the same bytes.  trim=(level, margin) (_trim_rule): every image is
        cut to its ink first -- ops.trim_view and PIL's crop on the host path, OCRModel.ingest(trim=) on the device path."""
        if fit not in ("none", "canvas"):
            raise ValueError(f"fit must be 'none' or 'canvas', got {fit!r}")
        if ingest == "device":
            kw = {} if trim is None else dict(trim=trim)
            return self.model.ingest(imgs, fit=True, **kw) if fit == "canvas" else self.model.ingest(imgs, **kw)
        if ingest != "host":
            raise ValueError(f"ingest must be 'host' or 'device', got {ingest!r}")
        if trim is not None:
            imgs = [self._trimmed(im, trim) for im in imgs]
        if fit == "canvas":
            imgs = [self._fitted(im, i) for i, im in enumerate(imgs)]
        return [self._tensor(im).cuda() for im in imgs]

    def _best_beams(self, xs, beams: int, max_len: int, length_alpha: float, return_logp: bool, rules=None, close: bool = False,
                    repeat_guard=None):
        """decode='beam': one OCRModel.beam_search over the images xs (a (B, C, H, W) tensor or a list of (C, H_b, W_b)) -> per image
        (the best beam's tokens up to and including its eos, their log-probabilities or None)"""
        res = self.model.beam_search(xs, beams, max_len, return_logp=return_logp, length_alpha=length_alpha,
                                     **({} if rules is None else {"rules": rules, "close": close}),
                                     **({} if repeat_guard is None else {"repeat_guard": repeat_guard}))
        lengths = res.lengths[:, 0].tolist()
        rows = [res.tokens[b, 0, :n].tolist() for b, n in enumerate(lengths)]
        logp = [res.logp[b, 0, :n].tolist() for b, n in enumerate(lengths)] if return_logp else [None] * len(rows)
        return rows, logp

    def _prefix_rows(self, prefixes: Sequence, decode: str, return_align: bool, max_len: int):
        """prefix= of __call__ / batch: one LaTeX string or token list per image -> (prefix (B, P) int64 with BOS in front, padded with the
        pad id; lengths (B,); the token lists; max_len capped so that the longest prefix and the continuation stay inside the positional
        table -- a prompted decode does not slide the window)"""
        if decode == "beam" or return_align:
            raise ValueError("prefix= is not available with decode='beam' or return_align")
        rows = [self.tokenizer.encode(p) if isinstance(p, str) else [int(t) for t in p] for p in prefixes]
        lens = [1 + len(r) for r in rows]
        room = self.dims.max_len - (max(lens) - 1)
        if room < 1:
            raise ValueError(f"prefix of {max(lens) - 1} tokens leaves no room in the positional table ({self.dims.max_len})")
        pre = torch.full((len(rows), max(lens)), self.model.trg_pad_idx, dtype=torch.int64)
        for b, r in enumerate(rows):
            pre[b, 0] = self.model.bos_token
            pre[b, 1:1 + len(r)] = torch.tensor(r, dtype=torch.int64)
        return pre, torch.tensor(lens, dtype=torch.int32), rows, min(int(max_len), room)

    def batch(self, imgs: Sequence, max_len: int = 350, temp: float = 0.3, decode: str = "sample",
              seed: Optional[int] = None, return_logp: bool = False, return_align: bool = False, beams: int = 5,
              length_alpha: float = 0.0, prefix: Optional[Sequence] = None, ingest: str = "host", fit: str = "none",
              trim: str = "none", trim_level: int = 127, trim_margin: int = 2, balanced: Optional[bool] = None,
              close: Optional[bool] = None, repeat_guard=None, return_alts: int = 0) -> List[tuple]:
        """return_alts=k (build extension; k in [1, 8]; not with decode='beam'): the last element of every result is one list per kept token
        of k (piece, logp) pairs -- the k best tokens of the raw logits row behind that token as the tokenizer's strings, with their
        log-probabilities (OCRModel.generate(return_alts=); raw: a token a rule, the guard or the sampler committed may be missing from its
        own list), cut where the tokens are cut.
        Build extension: __call__ over a list of PIL images of any sizes -> [(tokens, latex)] in order.
        Every image is preprocessed as __call__ does; chunks of the model's max_batch go through ONE ragged generate each with the
        per-row stop, and every row is cut at its eos.  max_len is capped at the positional table (a ragged decode does not slide the
        window).  A sampled draw is keyed by (seed + chunk index, row of its chunk, position): with an explicit seed the result is
        reproducible and no two images of the list share a stream of draws.
        return_logp=True: [(tokens, latex, logp)], logp the log-probability of every kept token (OCRModel.generate), cut as the tokens are.
        return_align=True appends to every tuple the maps (len(tokens), H_b/16, W_b/16) __call__(return_align=True) returns for that image,
        from ONE OCRModel.align_ragged pass per chunk over [bos] + tokens (positions behind a row's eos are masked).
        decode='beam': every image's best beam of `beams` (OCRModel.beam_search, ranked with length_alpha), from ONE ragged beam search
        per chunk of max_batch // beams images; temp and seed play no part.  A max_batch below beams is a ValueError.
        prefix=[...]: one LaTeX string or token list per image that the decode continues (BOS is put in front; OCRModel.generate_ragged
        with prefix= / prefix_len=): `tokens` (and logp) is the continuation, `latex` is decoded from prefix + continuation.
        ingest='device' (build extension; default 'host'): every chunk's images go to the device as raw uint8 pixels in ONE copy and are
        preprocessed there by ONE launch (OCRModel.ingest) instead of one float32 conversion, copy and slice assignment per image.  imgs may
        then also hold uint8 numpy arrays or tensors (H, W), (H, W, 3) or (H, W, 4).  The container is bit for bit the host path's, so
        every result is identical.
        fit='canvas' (build extension; default 'none': an image with a side beyond the canvas is a ValueError, as ever): such an image is
        downscaled to fit the canvas, aspect ratio kept (ops.fit_size; small images are never upscaled), with PIL's
        resize(..., BILINEAR) -- by PIL itself with ingest='host', by the engine (OCRModel.ingest(fit=True)) with ingest='device', to the
        same bytes, so every result is identical by either ingest here too.  An RGBA image is fitted on its RGB channels (convert('RGB');
        the alpha is not read).  An axis that would shrink by more than 32 times is a ValueError.  return_align maps of a fitted image
        are on the FITTED grid: (len(tokens), h'/16, w'/16) with (h', w') the fitted size rounded up to 16.
        trim='ink' (build extension; default 'none'): every image is first cut to its ink -- a pixel is ink iff min(R, G, B) <= trim_level
        (L: the byte itself; the alpha is not read), trim_margin pixels are kept around the ink box, clamped to the image, and an image
        without ink stays whole (ops.trim_view) -- by numpy and PIL's crop with ingest='host', by the engine (OCRModel.ingest(trim=)) with
        ingest='device', to the same pixels, so every result is identical by either ingest.  The cut comes BEFORE the fit: with
        fit='none' an image beyond the canvas whose ink fits is accepted, and one whose ink does not fit is refused as ever, with the
        trimmed size in the message.  return_align maps are on the grid of the trimmed (then fitted) image.
        balanced=True (build extension; default: the wrapper's own setting): the decode picks under rules.brace_rules of the tokenizer
        (OCRModel.generate_ragged(rules=)): no token closes a group that is not open, eos comes only at depth 0, <BOS> / <PAD> never.  A
        row that runs out of positions may still end open; logp stays the raw model's.  With decode='beam' only on a wrapper built with
        rules_beam=True: the rule then binds inside the beam selection, and a best beam that finished is balanced by construction.
        close=True (build extension; with balanced=True only; default: the wrapper's own setting): the closing decode
        (OCRModel.generate_ragged(close=True)) -- a row only picks tokens from which it can still close its groups and reach eos inside
        max_len, so every row ends balanced and finished; with a prefix too deep to close in max_len it closes as far as it gets.
        repeat_guard=(max_period, max_repeats) (build extension; default: the wrapper's own setting; False: none): the repeat guard
        (OCRModel.generate_ragged(repeat_guard=)) -- no row ends in max_repeats + 1 consecutive copies of a block of at most max_period
        tokens; texocr_amd.guard.hits flags the rows of an unguarded decode that looped.  With decode='beam' only on a wrapper built with
        guard_beam=True: the ban then binds inside the beam selection (OCRModel.beam_search(repeat_guard=)), also beside close=True.  Not with
        close=True in the other decodes."""
        rules = self._rules(balanced, decode)
        ckw = {**self._close(close, rules), **self._guard(repeat_guard, decode), **self._alts(return_alts, decode)}
        rule = self._trim_rule(trim, trim_level, trim_margin)
        eng = self.model._engine
        max_len = min(int(max_len), self.dims.max_len)
        pre = plen = prows = None
        if prefix is not None:
            if len(prefix) != len(imgs):
                raise ValueError(f"prefix needs one entry per image ({len(imgs)}), got {len(prefix)}")
            pre, plen, prows, max_len = self._prefix_rows(prefix, decode, return_align, max_len)
        step = beam_chunk(eng.max_batch, beams) if decode == "beam" else eng.max_batch
        out: List[tuple] = []
        xs = self._images(imgs, ingest, fit, rule) if ingest != "device" else None
        for c0 in range(0, len(imgs), step):
            chunk = xs[c0:c0 + step] if xs is not None else self._images(imgs[c0:c0 + step], ingest, fit, rule)
            if decode == "beam":
                full, logp = self._best_beams(chunk, beams, max_len, length_alpha, return_logp, rules, **ckw)
            else:
                chunk_seed = None if seed is None else int(seed) + c0 // step
                kw = {} if pre is None else dict(prefix=pre[c0:c0 + step].cuda(), prefix_len=plen[c0:c0 + step])
                toks = self.model.generate_ragged(chunk, max_len, temp=temp, decode=decode, seed=chunk_seed, stop="row",
                                                  return_logp=return_logp, **kw, **({} if rules is None else {"rules": rules}), **ckw)
                toks, logp, alts = _split_result(toks, return_logp, rules is not None, return_alts)   # (without the rule states)
                full = [cut_at_eos(row, self.model.eos_token) for row in toks.tolist()]
                logp = logp.tolist() if return_logp else None
                if return_alts:
                    alts = (alts.ids.tolist(), alts.logp.tolist())
            maps = None
            if return_align:
                trg, mask = align_inputs(full, self.model.bos_token, self.model.trg_pad_idx)
                maps = [a.maps[0].cpu() for a in self.model.align_ragged(chunk, trg.cuda(), mask=mask.cuda())]
            for b, row in enumerate(full):
                row = row[:-1]                                                        # ocr_model.py:104 (drops the last token)
                latex = process_output(self.tokenizer.decode(row if prows is None else prows[c0 + b] + row))
                item = (row, latex, logp[b][:len(row)]) if return_logp else (row, latex)
                item = (*item, maps[b][:len(row)]) if return_align else item
                out.append((*item, pair_alts(self.tokenizer, alts[0][b], alts[1][b], len(row))) if return_alts else item)
        return out

    def __call__(self, img, max_len: int = 350, temp: float = 0.3, decode: str = "sample",
                 seed: Optional[int] = None, return_logp: bool = False, return_align: bool = False, beams: int = 5,
                 length_alpha: float = 0.0, prefix=None, ingest: str = "host", fit: str = "none", trim: str = "none", trim_level: int = 127,
                 trim_margin: int = 2, balanced: Optional[bool] = None, close: Optional[bool] = None, repeat_guard=None,
                 return_alts: int = 0) -> tuple:
        """return_alts=k: the last element of the result is one list per kept token of k (piece, logp) pairs (see batch); max_len is then
        capped at the positional table (the sliding window keeps no alternatives).
        -> (tokens, latex); return_logp=True: (tokens, latex, logp), logp[i] the log-probability of tokens[i] (OCRModel.generate);
        return_align=True appends maps (len(tokens), H/16, W/16) float32 on the host: maps[i] is where in the (padded) image tokens[i]
        came from -- the head-mean cross attention of the last decoder layer (OCRModel.align), from one teacher-forced pass over
        [bos] + tokens behind the generate.  Not available once the output outgrew the positional table (the window has slid).
        decode='beam' (build extension): the best of `beams` beams (OCRModel.beam_search, ranked with length_alpha), cut at its eos;
        max_len is capped at the positional table; temp and seed play no part.
        prefix= (a LaTeX string or a token list): the decode continues it (BOS is put in front; OCRModel.generate(prefix=)); `tokens` (and
        logp) is the continuation, `latex` is decoded from prefix + continuation; max_len is capped so that both fit the positional table.
        ingest='device': the image is preprocessed on the device (see batch); the result is identical.
        fit='canvas': an image beyond the canvas is downscaled to fit it first (see batch); the maps of return_align are then on the
        fitted grid.
        trim='ink': the image is cut to its ink and a margin first (see batch), before the fit; the maps are on the trimmed image's grid.
        balanced=True: the decode picks under the tokenizer's brace rule (see batch).  close=True: as a closing decode (see batch).
        repeat_guard=(max_period, max_repeats): under the repeat guard (see batch)."""
        rules = self._rules(balanced, decode)
        ckw = {**self._close(close, rules), **self._guard(repeat_guard, decode), **self._alts(return_alts, decode)}
        if return_alts:
            max_len = min(int(max_len), self.dims.max_len)
        x = self._images([img], ingest, fit, self._trim_rule(trim, trim_level, trim_margin))
        x = x.box if ingest == "device" else x[0][None]
        prow: List[int] = []
        gen_kw = {}
        if prefix is not None:
            pre, _, (prow,), max_len = self._prefix_rows([prefix], decode, return_align, max_len)
            gen_kw = dict(prefix=pre.cuda())
        if decode == "beam":
            beam_chunk(self.model._engine.max_batch, beams)
            rows, lps = self._best_beams(x, beams, min(int(max_len), self.dims.max_len), length_alpha, return_logp, rules, **ckw)
            toks = torch.tensor(rows, dtype=torch.int64, device=x.device)
            logp = torch.tensor(lps, dtype=torch.float32) if return_logp else None   # (every float32 is exact in the list's doubles)
        else:
            # max_len may exceed the positional table (the reference's default 350 does for short tables): the model then
            # slides its window exactly as the reference does (decoder.py:99-100), at window-length engine steps per token
            toks = self.model.generate(x, max_len=max_len, temp=temp, decode=decode, seed=seed, return_logp=return_logp, **gen_kw,
                                       **({} if rules is None else {"rules": rules}), **ckw)
            toks, logp, alts = _split_result(toks, return_logp, rules is not None, return_alts)   # (without the rule states)
        out_tokens = toks.squeeze(0).tolist()[:-1]                                   # ocr_model.py:104 (drops the EOS)
        latex = process_output(self.tokenizer.decode(prow + out_tokens))             # :105-108
        out = (out_tokens, latex, logp.squeeze(0)[:len(out_tokens)].tolist()) if return_logp else (out_tokens, latex)
        if return_align:
            if toks.shape[1] > self.dims.max_len:
                raise ValueError(f"return_align: {toks.shape[1]} tokens were generated, more than the positional table holds "
                                 f"({self.dims.max_len}): the window has slid and no single pass sees the whole sequence")
            bos = torch.full((1, 1), self.model.bos_token, dtype=torch.int64, device=toks.device)
            maps = self.model.align(x, torch.cat((bos, toks), dim=1), mask=torch.ones((1, toks.shape[1] + 1), dtype=torch.bool)).maps
            out = (*out, maps[0, :len(out_tokens)].cpu())
        if return_alts:
            out = (*out, pair_alts(self.tokenizer, alts.ids[0].tolist(), alts.logp[0].tolist(), len(out_tokens)))
        return out
