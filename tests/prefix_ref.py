"""Host restatement of the prompted decode (include/texocr.h: txo_generate_prefix), for tests/test_prefix_cpu.py and
tests/test_gpu_prefix.py.  Like ref64 / sampler_ref / beam_ref it holds no tests.

Rows of a decode are independent (decoder.py:115 is the only cross-row operation), so every row is decoded on its own by the oracle's
reference loop -- oracle.cpu_ref.generate_recompute(..., start_tokens=row's own prefix), without eos, in the dtype of the weights it is
given (float64 through ref64.sd64) -- and `combine` applies the column rule and the global break to the rows' results:

  m = min len_b.  The loop decodes positions t = m-1 .. max(len_b)+max_len-2.  At position t row b commits prefix[b, t+1] if t+1 < len_b,
  else its own j-th token, j = t+1-len_b (kept if j < max_len).  A row contains eos if prefix[b, :len_b] or anything it committed does;
  the loop breaks after the first position at which every row contains eos (t_last).  n = min(max_len, t_last+2-m) columns come back; a
  column a row did not reach holds pad / 0.0; stop='row': pad / 0.0 behind a row's first eos (every column if its prefix holds one).
  prefix_logp[b, i] = log_softmax(logits at position i-1)[prefix[b, i]] for m <= i < len_b and i <= t_last+1, else 0.0; stop='row': 0.0 in
  every column of a row whose prefix holds eos (finished from the start, nothing is scored for it)."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch

from oracle import cpu_ref


class PrefixRef(NamedTuple):
    tokens: torch.Tensor        # (B, n) int64
    logp: torch.Tensor          # (B, n), the weights' dtype
    prefix_logp: torch.Tensor   # (B, P)
    margin: torch.Tensor        # (B, n) top-1 minus top-2 logit at every column a row picked itself (inf where it holds pad)
    t_last: int


def combine(prefix: torch.Tensor, lens: Sequence[int], free: torch.Tensor, eos: Optional[int], max_len: int, pad: int, stop: str = "global"):
    """The column rule on integers alone.  free (B, max_len): row b's own continuation of prefix[b, :len_b], eos ignored.
    -> (tokens (B, n), reached (B, n) bool: the row wrote the column itself, t_last)"""
    B = prefix.shape[0]
    lens = [int(v) for v in lens]
    m, M = min(lens), max(lens)
    has = [eos is not None and bool((prefix[b, :lens[b]] == eos).any()) for b in range(B)]
    first = [0 if has[b] else None for b in range(B)]            # output column from which on a finished row is padded (stop='row')
    t_last = M + max_len - 2
    for t in range(m - 1, M + max_len - 1):
        for b in range(B):
            tok = int(prefix[b, t + 1]) if t + 1 < lens[b] else (int(free[b, t + 1 - lens[b]]) if t + 1 - lens[b] < max_len else None)
            if eos is not None and tok == eos and not has[b]:
                has[b] = True
                first[b] = max(t + 2 - lens[b], 0)
        if eos is not None and all(has):
            t_last = t
            break
    n = min(max_len, t_last + 2 - m)
    tokens = torch.full((B, n), pad, dtype=torch.int64)
    reached = torch.zeros((B, n), dtype=torch.bool)
    for b in range(B):
        upto = min(n, t_last + 2 - lens[b])                       # columns 0 .. t_last + 1 - len_b were decoded
        if stop == "row" and first[b] is not None:
            upto = min(upto, first[b])
        if upto > 0:
            tokens[b, :upto] = free[b, :upto]
            reached[b, :upto] = True
    return tokens, reached, t_last


@torch.no_grad()
def generate_prefix(sd, images, prefix: torch.Tensor, lens: Optional[Sequence[int]], eos: Optional[int], max_len: int, pad: int,
                    stop: str = "global", bos: int = 0) -> PrefixRef:
    """sd: torch state dict (float64 for a float64 reference); images: a (B, C, H, W) tensor or a sequence of (C, H_b, W_b) tensors, in
    the weights' dtype; prefix (B, P) int64 on the host."""
    B, P = prefix.shape
    lens = [P] * B if lens is None else [int(v) for v in lens]
    m = min(lens)
    free, flogits, plogp = [], [], torch.zeros((B, P), dtype=sd["decoder.net.to_logits.weight"].dtype)
    for b in range(B):
        img = images[b][None]
        start = prefix[b:b + 1, :lens[b]]
        t, lg = cpu_ref.generate_recompute(sd, img, bos, None, max_len, collect_logits=True, start_tokens=start)
        free.append(t[0])
        flogits.append(lg[0])
        if lens[b] > m:                                          # teacher-forced positions m-1 .. len_b-2 score prefix[b, m .. len_b-1]
            net = cpu_ref.decoder_net(sd, start[:, :-1], cpu_ref.encode(sd, img))[0]
            lsm = torch.log_softmax(net, dim=-1)
            for i in range(m, lens[b]):
                plogp[b, i] = lsm[i - 1, int(prefix[b, i])]
    free, flogits = torch.stack(free), torch.stack(flogits)
    tokens, reached, t_last = combine(prefix, lens, free, eos, max_len, pad, stop)
    n = tokens.shape[1]
    lp_all = torch.log_softmax(flogits, dim=-1).gather(2, free[..., None])[..., 0][:, :n]
    top2 = flogits.topk(2, dim=-1).values
    margin = (top2[..., 0] - top2[..., 1])[:, :n]
    logp = torch.where(reached, lp_all, torch.zeros_like(lp_all))
    margin = torch.where(reached, margin, torch.full_like(margin, float("inf")))
    for b in range(B):                                           # forced positions an eos break left undecoded
        plogp[b, t_last + 2:] = 0
        if stop == "row" and eos is not None and bool((prefix[b, :lens[b]] == eos).any()):
            plogp[b] = 0                                         # finished from the start: nothing is scored for the row
    return PrefixRef(tokens, logp, plogp, margin, t_last)
