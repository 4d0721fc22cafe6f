"""Host restatement of the engine's sampler (csrc/step.h: sample_row_regs / sample_row_lds; include/texocr.h: txo_set_sampling), numpy
only.  Sampling is deterministic, so every token the device draws can be predicted from the fp32 logits it read (generate(...,
return_logits=True) returns exactly those):

- u: Philox4x32-10 with counter (row of the batch, position, 0, 0) and key (seed low 32 bits, seed high 32 bits);
  u = ((c0 >> 8) + 0.5f) / 2^24 in float32 (above 2^23 the addition rounds to even, so u can be exactly 1);
- kept set: the k = max(int((1 - 0.9) * V), 1) largest logits, ties at the k-th value kept lowest index first (the order is the
  kernel's: float bits mapped to order-preserving unsigned keys, so -0.0 sits below +0.0);
- the token: the first kept entry, in index order, at which the running sum of exp((logit - max) / temp) reaches u * total.

The draw is computed here in float64; the device sums fp32 probabilities in another order, so a target u * total that lies within
a few float32 roundings of a CDF boundary may fall on either side of it: `draw` also returns that distance and the two kept tokens
around the nearest boundary."""
from typing import NamedTuple

import numpy as np

THRESHOLD = 0.9
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO32, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(ctr, key) -> np.ndarray:
    """ctr (..., 4) and key (..., 2) uint32 (broadcast against each other) -> (..., 4) uint32: ten rounds as in step.h: philox4x32"""
    ctr, key = np.asarray(ctr, dtype=np.uint32), np.asarray(key, dtype=np.uint32)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., i], shape).astype(np.uint64) for i in range(4)]
    k0, k1 = (np.broadcast_to(key[..., i], shape).astype(np.uint64) for i in range(2))
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _LO32, (p0 >> _S32) ^ c[3] ^ k1, p0 & _LO32]
        k0, k1 = (k0 + _W0) & _LO32, (k1 + _W1) & _LO32
    return np.stack(c, -1).astype(np.uint32)


def u_from_c0(c0) -> np.ndarray:
    """the first Philox word -> u in (0, 1], float32 arithmetic: (c0 >> 8) is exact in float32, + 0.5f rounds to nearest even"""
    hi = (np.asarray(c0, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return (hi + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def uniform(seed, rows, t) -> np.ndarray:
    """u of the draw at (row of the batch, position t) under `seed` (an int in [0, 2^64), or an array of them); broadcast"""
    s = np.asarray(seed, dtype=np.uint64)
    r, tt, s = np.broadcast_arrays(np.asarray(rows, dtype=np.uint32), np.asarray(t, dtype=np.uint32), s)
    z = np.zeros(r.shape, np.uint32)
    key = np.stack([(s & _LO32).astype(np.uint32), (s >> _S32).astype(np.uint32)], -1)
    return u_from_c0(philox4x32_10(np.stack([r, tt, z, z], -1), key)[..., 0])


def topk_of(V: int) -> int:
    """k of the reference's top-k filter, as model.py: set_sampling passes it (int((1 - 0.9) * V) is 99 at V = 1000)"""
    return max(int((1 - THRESHOLD) * V), 1)


def order_keys(logits) -> np.ndarray:
    """float32 bits -> order-preserving uint32 (step.h: fkey)"""
    b = np.ascontiguousarray(logits, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def kept_mask(logits, k: int) -> np.ndarray:
    """(n, V) bool: the k largest of every row, ties at the k-th value lowest index first"""
    key = order_keys(logits).astype(np.int64)
    order = np.argsort(-key, axis=1, kind="stable")
    kept = np.zeros(key.shape, dtype=bool)
    np.put_along_axis(kept, order[:, :k], True, axis=1)
    return kept


def kept_probs(logits, temp: float, k: int) -> np.ndarray:
    """(n, V) float64: exp((v - max) / temp) over the kept set, 0 elsewhere, normalised per row"""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    p = np.where(kept_mask(x.astype(np.float32), k), np.exp((x - x.max(1, keepdims=True)) / temp), 0.0)
    return p / p.sum(1, keepdims=True)


class Draws(NamedTuple):
    token: np.ndarray     # (n,) the token the rule gives in float64
    dist: np.ndarray      # (n,) |u * total - nearest interior CDF boundary| / total (inf with one kept entry)
    pair: np.ndarray      # (n, 2) the kept tokens just below and just above that boundary


def draw_u(logits, temp: float, u, topk: int = None) -> Draws:
    """the draw for explicit u (n,) from logits (n, V)"""
    lg = np.asarray(logits, dtype=np.float32)
    n, V = lg.shape
    k = topk_of(V) if topk is None else min(max(int(topk), 1), V)
    u = np.broadcast_to(np.asarray(u, dtype=np.float64), (n,))
    token, dist, pair = np.empty(n, np.int64), np.empty(n), np.empty((n, 2), np.int64)
    idx = np.arange(V)
    step = max(1, (1 << 22) // V)
    for a in range(0, n, step):
        x = lg[a:a + step].astype(np.float64)
        kept = kept_mask(lg[a:a + step], k)
        p = np.where(kept, np.exp((x - x.max(1, keepdims=True)) / temp), 0.0)
        cdf = np.cumsum(p, 1)
        total = cdf[:, -1:]
        target = u[a:a + step, None] * total
        token[a:a + step] = np.argmax(cdf >= target, 1)
        last = V - 1 - np.argmax(kept[:, ::-1], 1)                        # the last kept entry closes the CDF: not a boundary
        inner = kept & (idx[None, :] != last[:, None])
        gap = np.where(inner, np.abs(cdf - target), np.inf)
        jb = np.argmin(gap, 1)
        dist[a:a + step] = gap[np.arange(len(jb)), jb] / total[:, 0]
        nxt = np.where(kept & (idx[None, :] > jb[:, None]), idx[None, :], V).min(1)
        pair[a:a + step, 0], pair[a:a + step, 1] = jb, np.where(nxt < V, nxt, jb)
    return Draws(token, dist, pair)


def draw(logits, temp: float, seed, row, t, topk: int = None) -> Draws:
    """for every entry i: the token drawn from logits[i] (fp32, (n, V)) under the key (seed[i], row[i], t[i]) (broadcast)"""
    lg = np.asarray(logits, dtype=np.float32)
    u = np.broadcast_to(uniform(seed, row, t), (lg.shape[0],))
    return draw_u(lg, temp, u, topk)


def keys_for(path: str, T0: int, L: int, i: int, seed: int):
    """(seed, position) of output token i (0-based) for a decode of start length T0 with a positional table of L entries.
    'engine': generate() from BOS -- the KV-cache steps and generate_window beyond the table alike key token i by position i
    (engine.hip: generate_window sets the position to the token index).  'stepwise': decoder.generate's general loop
    (model.py: _generate_stepwise) decodes token i at position T0 - 1 + i while the output fits the table; once the window slides the
    position stays at L - 1 and the seed advances with the token index instead."""
    if path == "engine":
        return seed % 2 ** 64, i
    if path != "stepwise":
        raise ValueError(path)
    if T0 + i <= L:
        return seed % 2 ** 64, T0 - 1 + i
    return (seed + i) % 2 ** 64, L - 1
