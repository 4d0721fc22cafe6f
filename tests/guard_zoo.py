"""Scripted decoders and boundary histories for the repeat-guard kernels (csrc/step_guard.h, csrc/beam_guard.h), numpy only.  Holds no tests.

A model with random weights loops only by accident, with period 1 or 2, so the guard tests that decode one never scan further back than
14 tokens.  Here the LOGITS FOLLOW A SCRIPT: the positional table carries one of 63 orthogonal +-1 codes (rows of a Hadamard matrix; zero
mean, unit variance: LayerNorm with weight 1 and bias 0 leaves them as they are) per position, `to_logits` turns the code of a position
into a strict ranking of a few tokens (first choice GAP * n, second GAP * (n - 1), ..., every other token near 0), the attention and FFN
output projections are scaled down so that the script dominates, and a small token embedding and a tenth of the random `to_logits` matrix
stay, so that two beams holding the same tokens in another order do not score within an ulp of each other.  tests/test_guard_zoo_cpu.py
pins, on oracle/cpu_ref.py, that the free greedy decode is the script's first choices and that consecutive ranks lie >= 100 x the bf16
logit error apart; nothing about the logits' values is asserted on the GPU.

Behind the positional table (the sliding window) every pick reads the LAST slot's ranking: the window's last position is max_len - 1.

Histories: `boundary(p, R)` gives the prefixes around the threshold m_p = R * p - 1 of period p, `ruler` the sequence whose ban set under
(8, 1) has four tokens by four periods.  The case lists at the bottom choose alphabets so that bans fall on id 0, on the last ordinary
id, in a partial last map word, two in one 32-bit word and two in one 16-byte request; the CPU test asserts each placement."""
import dataclasses
from typing import NamedTuple, Tuple

import numpy as np

from texocr_amd import synth
from texocr_amd.config import Dims

GAP = 4.0                                                         # logit distance of consecutive ranks (the CPU test measures what is left of it)
AMP = 4.0                                                         # the positional code's amplitude over the token embedding's 0.05
TOKEN_SCALE, MIX_SCALE, NOISE_SCALE = 0.1, 0.02, 0.1
BF16_LOGIT_ERROR = 0.025                                          # tests/test_gpu_parity.py: test_bf16_mode_logits_error_bounded


def dims(vocab, max_len, low_specials=False):
    """test_gpu_guard._tiny's model; low_specials: eos / bos / pad at 7 / 8 / 9, so that the last ids of the vocabulary are ordinary tokens"""
    d = Dims(canvas=64, in_channels=3, embed_dim=64, enc_heads=2, enc_layers=2, dec_heads=2, dec_layers=2, vocab=vocab, max_len=max_len,
             bos=vocab - 2, eos=vocab - 3, pad=vocab - 1)
    return dataclasses.replace(d, eos=7, bos=8, pad=9) if low_specials else d


def specials(d):
    return {d.bos, d.eos, d.pad}


def hadamard(n):
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    assert h.shape[0] == n
    return h


def scripted_sd(d, script, seed=5):
    """state dict on `d` whose logits at position t rank script[t] (a list of distinct token ids, first choice first) ahead of every other
    token; len(script) == d.max_len, at most 63 different rankings"""
    assert len(script) == d.max_len and d.embed_dim == 64
    kinds = {}
    slot = [kinds.setdefault(tuple(int(v) for v in r), len(kinds)) for r in script]
    assert len(kinds) <= 63, len(kinds)
    code = hadamard(64)[1:]                                       # (the constant row is what LayerNorm removes)
    sd = dict(synth.synth_state_dict(d, seed))
    for key in list(sd):
        if key.startswith("decoder.net.attn_layers.layers.") and key.endswith((".0.weight", ".0.bias")) or key.startswith("decoder.net.norm."):
            sd[key] = np.full_like(sd[key], 1.0 if key.endswith("weight") else 0.0)
        elif key.startswith("decoder.net.attn_layers.layers.") and ".fc_out." in key:
            sd[key] = (sd[key] * np.float32(MIX_SCALE)).astype(np.float32)
    sd["decoder.net.token_embedding.weight"] = (sd["decoder.net.token_embedding.weight"] * np.float32(TOKEN_SCALE)).astype(np.float32)
    sd["decoder.net.pos_embedding.embedding.weight"] = (AMP * code[slot]).astype(np.float32)
    w = sd["decoder.net.to_logits.weight"].astype(np.float64) * NOISE_SCALE
    for ranking, k in kinds.items():
        assert len(set(ranking)) == len(ranking) and all(0 <= v < d.vocab for v in ranking), ranking
        for i, v in enumerate(ranking):
            w[v] += GAP * (len(ranking) - i) * code[k] / 64.0
    sd["decoder.net.to_logits.weight"] = w.astype(np.float32)
    sd["decoder.net.to_logits.bias"] = np.zeros_like(sd["decoder.net.to_logits.bias"])
    return sd


def loop_script(block, escapes, n, at=None):
    """the block for ever, the escape tokens ranked behind it; at = {position: ranking} replaces single slots"""
    s = [[block[t % len(block)]] + list(escapes) for t in range(n)]
    for t, r in (at or {}).items():
        s[t] = list(r)
    return s


def const_script(ranking, n):
    return [list(ranking) for _ in range(n)]


def first_choices(script, n):
    """the free greedy decode of n positions: the script's first choices, the last slot's beyond the table"""
    return [script[min(t, len(script) - 1)][0] for t in range(n)]


# ---- histories -------------------------------------------------------------------------------------------------------------------------
class Boundary(NamedTuple):
    under: Tuple[int, ...]        # (i)   purely periodic, m_p = R * p - 2: the block's first token is NOT banned
    at: Tuple[int, ...]           # (ii)  purely periodic, m_p = R * p - 1: banned
    broken: Tuple[int, ...]       # (iii) (ii) with a mismatch at the LAST compared pair (indices n - R * p + 1 and n - R * p + 1 - p): m_p = R * p - 2
    #                                     again, not banned; None where R * p - 1 == 0 (nothing is compared: (1, 1))
    twin: Tuple[int, ...]         #       one token longer, the mismatch one pair further back (n - R * p against n - R * p - p): banned


def periodic(block, length):
    """the last `length` tokens of block block block ...: the next token of the sequence is block[0]"""
    p = len(block)
    reps = list(block) * (length // p + 2)
    return tuple(reps[len(reps) - length:]) if length else ()


def boundary(block, R, odd):
    """the four prefixes of period p = len(block) (its tokens distinct) and max_repeats R; `odd`: the mismatching token, not in the block.
    The next scripted token is block[0] in each: it would complete the (R + 1)-th copy where m_p allows"""
    p = len(block)
    assert len(set(block)) == p and odd not in block
    need = R * p - 1
    at = periodic(block, need + p)
    return Boundary(periodic(block, need + p - 1), at, ((odd,) + at[1:]) if need > 0 else None, (odd,) + at)


def trailing_matches(h, p):
    """m_p of a history, uncapped"""
    m, n = 0, len(h)
    while n - 1 - m - p >= 0 and h[n - 1 - m] == h[n - 1 - m - p]:
        m += 1
    return m


def ruler(a, b, c, d):
    """a b a c a b a d a b a c a b a: under (8, 1) and (16, 1) the ban set is {a, b, c, d}, by periods 1, 2, 4 and 8"""
    half = [a, b, a, c, a, b, a]
    return tuple(half + [d] + half)


def window(P, R):
    """how far back any scan of guard (P, R) looks: csrc/beam_guard.h: beam_guard_window"""
    return (R + 1) * P - 1


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
PERIODS = (1, 2, 3, 5, 8, 15, 16)
REPEATS = (1, 2, 3, 16)
TABLE = 320                                                        # positional table of the long cases: 300 positions, and the longest prefix (273 columns) + 17 picks

# the boundary table's model: one ranking at every position; a block is (A, fillers ...), the mismatch is ODD
BOUNDARY_V = 64
BOUNDARY_RANKING = (0, 1, 60, 45, 46, 47, 50, 51)                                  # a > b > c > ...: id 0, its neighbour in the same 16-byte request, the last ordinary id
FILLERS = tuple(range(20, 35))                                     # 15 distinct ids behind A in a block
ODD = 40


def boundary_block(p):
    return (BOUNDARY_RANKING[0],) + FILLERS[:p - 1]


def boundary_rows(R):
    """[(p, kind, history)] of one max_repeats, every period of PERIODS"""
    rows = []
    for p in PERIODS:
        bd = boundary(boundary_block(p), R, ODD)
        rows += [(p, kind, h) for kind, h in zip(Boundary._fields, bd) if h is not None]
    return rows


class Ruler(NamedTuple):
    vocab: int
    low_specials: bool
    letters: Tuple[int, int, int, int]    # a, b, c, d: the ban set
    x: int                                # the fifth-ranked token: the pick
    stream: str                           # what the vocabulary reaches in the kernels


RULERS = (
    Ruler(64, False, (0, 1, 31, 60), 33, "16-byte stream; id 0, ids 0 and 1 in one request, 0 / 1 / 31 in one word, 60 the last ordinary id"),
    Ruler(67, True, (64, 66, 0, 35), 20, "scalar stream; 64 and 66 in the partial last word (3 bits), 66 = V - 1 (the specials sit at 7 .. 9)"),
    Ruler(1000, False, (996, 992, 993, 0), 300, "register sampler; 992 and 993 in one request and one word, 996 the last ordinary id"),
    Ruler(1030, False, (1026, 1025, 0, 1), 500, "LDS sampler; 1025 and 1026 in the partial last word (6 bits), 1026 the last ordinary id"),
)


class Loop(NamedTuple):
    period: int
    vocab: int
    block: Tuple[int, ...]
    escapes: Tuple[int, ...]


def loop(period, vocab=64):
    """the free-running scripts: a block of `period` distinct tokens from id 0 up in steps of 3 (0 and 3 share a 16-byte request, the
    first eleven a 32-bit word), escapes ranked behind it: the last ordinary id first"""
    block = tuple(3 * i for i in range(period))
    return Loop(period, vocab, block, (vocab - 4, 50, 53, 55))


LOOPS = {p: loop(p) for p in (5, 8, 16)}
LOOP_GUARDS = ((16, 3), (8, 16), (16, 16))


PLUMB_TABLE = 160


def staggered(L, B, eos=None):
    """a period-8 script and B prefixes that differ: row r holds the script's first r tokens and then a mismatch, so its first ban under
    (8, 3) falls at position r + 32 and rows never hold the same history.  eos given: the second rank is eos at every third position, so
    a row ends at the first ban that falls on one (within three bans), rows end at different positions, and the others go on behind the
    compaction"""
    at = {}
    if eos is not None:
        at = {t: [L.block[t % 8], eos, L.escapes[1]] for t in range(0, PLUMB_TABLE, 3)}
    script = loop_script(L.block, L.escapes, PLUMB_TABLE, at=at)
    hists = [tuple(first_choices(script, r)) + (ODD,) for r in range(B)]
    return script, hists


def ban_words(ban):
    return sorted(v >> 5 for v in ban)


def share_word(ban):
    w = ban_words(ban)
    return len(set(w)) < len(w)


def share_request(ban):
    return any(v + 1 in ban and (v >> 2) == ((v + 1) >> 2) for v in ban)


def in_partial_word(ban, vocab):
    return vocab % 32 != 0 and any(v >= (vocab // 32) * 32 for v in ban)
