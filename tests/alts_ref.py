"""Alternatives per token, the rule in numpy float64 (include/texocr.h: txo_set_alternatives), and the scripted rows the GPU tests put it on.

ids: the indices of the k largest entries of the f32 row in descending value, the lower index first among equals -- a stable argsort of the
negated row.  logp: x[ids] - logsumexp(x) on the f32 values widened to float64."""
import numpy as np

import logit_scripts as ls

KS = (1, 3, 8)
LANES = ls.LANES


def alts(x, k):
    """x (..., V) float32 -> (ids (..., k) int64, logp (..., k) float64)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    ids = np.argsort(-x, axis=-1, kind="stable")[..., :k]
    m = x.max(axis=-1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True))
    return ids, np.take_along_axis(x, ids, axis=-1) - lse


def lane_entries(V, lane):
    """the indices alts_step_kernel's lane `lane` streams, in its order (step.h's two loops: float4 j4 = lane + 64 i when V % 4 == 0, else
    lane + 64 i)"""
    if V % 4 == 0:
        return [4 * j4 + c for j4 in range(lane, V // 4, LANES) for c in range(4)]
    return list(range(lane, V, LANES))


def _raised(V, name, idx, values=None):
    """base_row(V) (distinct values in (-4, 4)) with the entries idx raised to 6.0, 5.75, ... (or `values`): exact in f32, 0.25 apart"""
    row = ls.base_row(V)
    vals = [6.0 - 0.25 * r for r in range(len(idx))] if values is None else values
    for i, v in zip(idx, vals):
        row[i] = np.float32(v)
    return name, row, list(idx)


def scripts(V):
    """[(name, row (V,) float32, raised ids in their expected order)]"""
    out = []
    L = next((ln for ln in (5, 0) if len(lane_entries(V, ln)) >= 2), 5)          # a lane that holds two entries where one does (V = 65: lane 0 only)
    out.append(_raised(V, "one_lane", lane_entries(V, L)[:8]))                   # the eight largest in ONE lane, descending in its stream order
    out.append(_raised(V, "one_lane_rev", lane_entries(V, L)[:8][::-1]))         # ... ascending: every push goes to the front
    first = [lane_entries(V, lane)[0] for lane in range(63, 55, -1) if lane_entries(V, lane)]
    out.append(_raised(V, "eight_lanes", first))                                 # eight lanes, in descending lane order
    seams = [V - 1]
    if V % 4 == 0:
        seams.append(4 * (V // 4 - 1))                                           # the last float4
    if V > 1024:
        seams.append(1024)                                                       # the first float4 of the second sweep
    for sidx in seams:
        out.append(_raised(V, f"seam{sidx}", [0, sidx]))
    mine = lane_entries(V, L)
    a, b = (mine[0], mine[1]) if len(mine) > 1 else (mine[0], mine[0] + 1)       # two in one lane (a lane of V = 63 holds one entry)
    c = next(lane_entries(V, ln)[0] for ln in range(40, -1, -1) if ln != L and lane_entries(V, ln) and lane_entries(V, ln)[0] not in (a, b))
    three = sorted([a, b, c])
    out.append(_raised(V, "three_equal", three + [V - 2], [6.0, 6.0, 6.0, 5.0]))
    out.append(("equal", np.full(V, 1.25, np.float32), list(range(8))))
    return out


# ---- score on random weights: the reference sums in another order, so ranks are compared where the float64 order is clear -------------------
MARGIN = 2e-5                         # gpu_harness.assert_tokens_exact_up_to_margin
SCORE_CASE = dict(vocab=1000, weight_seed=3, rows=5, image_hw=(32, 48), image_seed=9, L=6, trg_seed=17)


def ranked_places(x64, k, margin=MARGIN):
    """(ids, keep): the float64 order of x64 (..., V), and the (row, rank) places whose gap to BOTH ranked neighbours exceeds margin"""
    order = np.argsort(-x64, axis=-1, kind="stable")[..., :k + 1]
    v = np.take_along_axis(x64, order, axis=-1)
    gap = v[..., :-1] - v[..., 1:]                                               # gap[j]: rank j to rank j + 1
    up = np.concatenate([np.full(gap[..., :1].shape, np.inf), gap[..., :-1]], axis=-1)
    return order[..., :k], (gap > margin) & (up > margin)


def score_targets(bos, vocab):
    import torch
    c = SCORE_CASE
    g = torch.Generator().manual_seed(c["trg_seed"])
    return torch.cat([torch.full((c["rows"], 1), bos, dtype=torch.int64), torch.randint(0, vocab - 3, (c["rows"], c["L"] - 1), generator=g)], 1)
