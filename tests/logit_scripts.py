"""Scripted logits rows for the kernels that turn a row into a token or a score, and the arithmetic of those kernels restated -- numpy
only, no GPU, no tests (tests/test_logit_scripts_cpu.py proves the placements; tests/test_gpu_logit_scripts.py runs the scripts).

The decode head is logits = wlog . LNf(y) + blog: with wlog all zeros every row at every position is blog, bit for bit, so a test chooses
the row.  A script is a base row of small distinct values with a few entries raised: `top` names them in the order a greedy selection
has to take them as the entries before are masked (the arg-max, the runner-up, the third).  The runner-up and the third lie on the other
side of a seam of the walk from the arg-max (another lane, sweep or tile).  All values are finite and |v| <= 1e4."""
from typing import NamedTuple, Tuple

import numpy as np

import guard_ref
import sampler_ref as sr
from texocr_amd import rules as R

# ---- the walks, each beside the header line it follows ---------------------------------------------------------------------------------
LANES = 64
SWEEP4 = 256          # step.h: `for (int base = 0; base < n4; base += 256)`: float4 per sweep = 4 unroll slots x 64 lanes
UNROLL = 4            # step.h: `for (int u = 0; u < 4; ++u)`, j4 = base + u * 64 + lane
SR_PER = 16           # step.h: constexpr int SR_PER = 16
VPT = 4               # step.h: constexpr int VPT = 4 (beam_select_kernel: vocabularies up to 256 * VPT in registers)
BEAM_THREADS = 256    # step.h: __launch_bounds__(256) beam_select_kernel, entries tid + 256 i
SC_VT = 4             # score.h: constexpr int SC_VT = 4 (16-entry tiles per step: a walk of 64 entries)
SC_TILE = 16 * SC_VT


class GreedyPlace(NamedTuple):
    f4: bool          # step.h: `if ((a.V & 3) == 0)`: the float4 stream; else the scalar loop `for (j = lane; j < V; j += 64)`
    sweep: int        # f4: (j / 4) / 256; scalar: j / 64 (the loop's iteration)
    slot: int         # f4: the unroll slot u; scalar: 0
    lane: int
    comp: int         # f4: .x .y .z .w = 0 .. 3; scalar: 0


def n4(V):
    return V >> 2     # step.h: const int n4 = a.V >> 2


def greedy_place(V, j):
    assert 0 <= j < V
    if V & 3:
        return GreedyPlace(False, j // LANES, 0, j % LANES, 0)
    j4 = j >> 2
    return GreedyPlace(True, j4 // SWEEP4, (j4 % SWEEP4) // LANES, j4 % LANES, j & 3)


def greedy_sweeps(V):
    return (n4(V) + SWEEP4 - 1) // SWEEP4 if V % 4 == 0 else (V + LANES - 1) // LANES


def sampler_form(V):
    """step.h: sample_in_regs(V) = V <= 64 * SR_PER; sample_row_regs loads 16 bytes `if ((V & 3) == 0 && (per & 3) == 0)`
    (tests/test_gpu_sampler.py: _form)"""
    if V > LANES * SR_PER:
        return "lds"
    per = (V + 63) // 64
    return "regs16" if V % 4 == 0 and per % 4 == 0 else "regs1"


def sampler_per(V):
    return (V + 63) // 64                                     # step.h: const int per = (V + 63) / 64, j0 = lane * per


def sampler_nin(V, lane):
    return max(0, min(sampler_per(V), V - lane * sampler_per(V)))     # step.h: const int nin = max(0, min(per, V - j0))


def sampler_place(V, j):
    """(lane, slot) of entry j in the lane-contiguous chunks both sampler forms share"""
    return j // sampler_per(V), j % sampler_per(V)


class BeamPlace(NamedTuple):
    regs: bool        # step.h: `if (V <= 256 * VPT)`
    thread: int       # regs: v % 256 (entries tid + 256 i); general: flat index f % 256 (`for (f = tid; f < total; f += 256)`)
    reg: int          # regs: i = v / 256; general: f / 256 (the loop's iteration)
    wave: int


def beam_place(V, v, parent=0):
    if V <= BEAM_THREADS * VPT:
        return BeamPlace(True, v % BEAM_THREADS, v // BEAM_THREADS, (v % BEAM_THREADS) // LANES)
    f = parent * V + v
    return BeamPlace(False, f % BEAM_THREADS, f // BEAM_THREADS, (f % BEAM_THREADS) // LANES)


class ScorePlace(NamedTuple):
    tile: int         # score.h: `for (int v0 = 0; v0 < V; v0 += 16 * SC_VT)`
    j: int            # v = v0 + j * 16 + lg * 4 + r
    lg: int           # the lane group (lane >> 4) that holds the entry
    r: int


def score_place(V, v):
    assert 0 <= v < V
    w = v % SC_TILE
    return ScorePlace(v // SC_TILE, w // 16, (w % 16) // 4, w % 4)


def score_tiles(V):
    return (V + SC_TILE - 1) // SC_TILE


def score_clamped_rows(V):
    """rows of the last tile read from row V - 1 (score.h: min(v0 + j * 16 + lc, V - 1)) and masked"""
    return score_tiles(V) * SC_TILE - V


# ---- the vocabularies --------------------------------------------------------------------------------------------------------------
VOCABS = {
    63: "scalar greedy branch; per = 1; score tile one short",
    64: "score tile exact; per = 1 with every lane full",
    65: "scalar greedy branch; per = 2 with lanes 33-63 empty; score tile one over",
    128: "two score tiles",
    129: "two score tiles plus one entry",
    960: "V % 4 == 0 but per = 15: register sampler with one-logit loads",
    1024: "one full sweep; last register vocabulary of sampler and beam",
    1025: "LDS sampler, general beam path, scalar branch beyond one sweep",
    1027: "scalar branch, 3 beyond one sweep",
    1028: "second sweep holds one float4 in lane 0",
    2048: "two full sweeps",
    2052: "a third sweep holding one float4",
}
SCORE_VOCABS = (63, 64, 65, 128, 129, 1027)
SAMPLER_VOCABS = (65, 960, 1024, 1025)          # regs1 with empty lanes, regs1 at per = 15, regs16, lds
BEAM_VOCABS = (1024, 1025)
CLOSE_VOCABS = (1028, 1027)

TOP, SECOND, THIRD = np.float32(6.0), np.float32(5.0), np.float32(4.5)
SPREAD = 8.0


class Script(NamedTuple):
    name: str
    V: int
    kind: str                 # single | tie | equal | wide
    row: np.ndarray           # (V,) float32
    top: Tuple[int, ...]      # the first three picks as the entries before are masked; a tie: its two members first

    @property
    def id(self):
        return f"V{self.V}-{self.name}"


def base_row(V):
    """V distinct values in (-4, 4), 8 / V apart (>= 3.9e-3 at V = 2052), in an order fixed by V"""
    perm = np.random.default_rng(1000 + V).permutation(V)
    return (-SPREAD / 2 + SPREAD * (perm + 0.5) / V).astype(np.float32)


def _others(V, taken, first, n):
    """n further indices for the runner-up and the third: the mirror of `first` across its seam, then the seams of the walk"""
    mirror = {0: V - 1, 3: 4, 4: 3, 252: 256, 255: 256, 256: 255, 1020: 1024, 1023: 1024, 1024: 1023, 1027: 1023}
    mirror.update({V - 4: 0, V - 2: V - 1 if V & 3 else 0, V - 1: 0})      # (V % 4 == 0: V - 2 and V - 1 share a float4)
    out = []
    for c in (mirror.get(first), 255, 256, 1024, 0, V - 1, 3, 4, 64, 63):
        if c is not None and 0 <= c < V and c not in taken and c not in out:
            out.append(c)
    return out[:n]


def single(V, i):
    row = base_row(V)
    second, third = _others(V, {i}, i, 2)
    row[i], row[second], row[third] = TOP, SECOND, THIRD
    return Script(f"max{i}", V, "single", row, (i, second, third))


def tie(V, a, b):
    assert a < b
    row = base_row(V)
    third, = _others(V, {a, b}, b, 1)
    row[a] = row[b] = TOP
    row[third] = SECOND
    return Script(f"tie{a}_{b}", V, "tie", row, (a, b, third))


def equal(V):
    return Script("equal", V, "equal", np.full(V, 1.25, np.float32), (0, 1, 2))


def wide(V):
    """values over +-80 with the maximum in the second sweep: all but a few terms of the log-sum-exp underflow, and the running
    (max, sum) of a lane is rescaled by exp(-160) on the way"""
    assert greedy_sweeps(V) >= 2
    perm = np.random.default_rng(2000 + V).permutation(V)
    row = (-80.0 + 156.0 * (perm + 0.5) / V).astype(np.float32)          # (-80, 76)
    i = 1024 + (V - 1024) // 2
    second, third = 1023, 255                                            # the last slot of the first sweep, and lane 63's first float4
    row[i], row[second], row[third] = 80.0, 79.0, 78.5
    return Script(f"wide{i}", V, "wide", row, (i, second, third))


SINGLES = (0, 3, 4, 252, 255, 256, 1020, 1023, 1024, 1027)


def single_indices(V):
    return sorted({i for i in SINGLES + (V - 4, V - 2, V - 1) if 0 <= i < V})


def tie_pairs(V):
    per = sampler_per(V)
    pairs = [(255, 256), (1023, 1024), (0, V - 1), (V - 2, V - 1), (63 * per - 1, 63 * per)]
    out = []
    for a, b in pairs:
        if 0 <= a < b < V and (a, b) not in out:
            out.append((a, b))
    return out


def greedy_scripts(V):
    out = [single(V, i) for i in single_indices(V)] + [tie(V, a, b) for a, b in tie_pairs(V)] + [equal(V)]
    if V > 1024:
        out.append(wide(V))
    return out


def score_pairs(V):
    """ties for the merge of the four lane groups (score.h: take over xor16 / xor32): lane groups 0|1, 0|2, 1|2, 3|0 of the next 16, the
    tile seam 63|64, and the row's ends"""
    pairs = [(0, 4), (0, 8), (4, 8), (12, 16), (63, 64), (0, V - 1), (V - 2, V - 1)]
    return [(a, b) for a, b in pairs if 0 <= a < b < V]


def score_scripts(V):
    idx = sorted({i for i in (0, 63, 64, V - 1) if 0 <= i < V})
    return [single(V, i) for i in idx] + [tie(V, a, b) for a, b in score_pairs(V)] + [equal(V)]


def beam_scripts(V):
    """top entries at the thread seam 255 | 256, in thread 255's / thread 0's fourth register 767 | 768, and at 1023 | 1024 (V = 1024:
    1023 with 767, two registers of thread 255)"""
    last = (1023, 1024) if V > 1024 else (767, 1023)
    return [tie(V, 255, 256), tie(V, 767, 768), tie(V, *last), single(V, 1023), single(V, 768)]


# ---- float64 expectation -----------------------------------------------------------------------------------------------------------------
class Expect(NamedTuple):
    pick: int            # the arg-max, lowest index among equals
    lse: float           # logsumexp of the row in float64
    logp: np.ndarray     # (V,) float64: v - lse
    margin: float        # top-1 minus top-2 value in float64 (0 for a tie)


def expect(row):
    x = np.asarray(row, np.float32).astype(np.float64)
    m = x.max()
    lse = float(m + np.log(np.exp(x - m).sum()))
    srt = np.sort(x)
    return Expect(int(np.argmax(x)), lse, x - lse, float(srt[-1] - srt[-2]))


# ---- masks: a two-state ban table and the (1, 1) guard -----------------------------------------------------------------------------------
GUARD = (1, 1)           # max_period 1, max_repeats 1: the previous pick is banned


def ban_table(V, banned, eos=None):
    """state 0 allows every token, state 1 bans `banned`; every token leads to state 1.  eos given: ONLY_AT_ZERO in both states (the depth
    never leaves 0), so that the closing decode can end a row"""
    flags = np.zeros((2, V), np.int64)
    flags[1, list(banned)] = R.BAN
    if eos is not None:
        flags[:, eos] = R.ONLY_AT_ZERO
    return R.TokenRules(R.pack(flags=flags, next=1), 1).validate(V)


def replay(row, n, rules=None, guard=None, eos=None, close=False):
    """n greedy picks from the fixed row under the masks, by the host rules alone (rules.TokenRules.allowed, guard_ref.mask; close: the
    budget of max_len = n) -> (tokens, the masked rows the selection saw)"""
    row = np.asarray(row, np.float32)
    st = rules.start(1) if rules is not None else None
    dist = rules.close_dist(eos) if close else None
    hist, seen, ended = [], [], False
    for t in range(n):
        ok = None
        if rules is not None:
            ok = rules.allowed(st, remaining=n - t, ended=[ended], dist=dist)[0] if close else rules.allowed(st)[0]
        if guard is not None:
            masked = guard_ref.mask(row, hist, guard[0], guard[1], eos, ok)[0]
        else:
            masked = row if ok is None else np.where(ok, row, R.MASKED)
        tok = int(np.argmax(masked))
        seen.append(masked)
        hist.append(tok)
        if rules is not None:
            st = rules.step(st, [tok])[0]
        ended = ended or (eos is not None and tok == eos)
    return np.asarray(hist, np.int64), np.stack(seen)


# ---- sampler scripts: the k-th largest entry is a pair -------------------------------------------------------------------------------------
class SamplerScript(NamedTuple):
    name: str
    V: int
    row: np.ndarray
    pair: Tuple[int, int]     # the two entries at the k-th place
    kept: int                 # the member of the pair the rule keeps
    zeros: bool               # the pair is (-0.0, +0.0)

    @property
    def id(self):
        return f"V{self.V}-{self.name}"


def _kth_pair(V, a, b, zeros):
    k = sr.topk_of(V)
    row = base_row(V).astype(np.float64)
    rest = np.array([j for j in np.argsort(-row, kind="stable") if j not in (a, b)])
    level = 0.5 * (row[rest[k - 2]] + row[rest[k - 1]])           # k - 1 entries above, the pair at the k-th place
    row = np.where(row > level, level + 0.25 * (row - level), row)   # the kept entries within 0.2 of each other: the k-th is drawn often
    if zeros:
        row = row - level
        row[a], row[b] = -0.0, 0.0
    else:
        row[a] = row[b] = level
    row = row.astype(np.float32)
    assert int((row > row[b]).sum()) == k - 1
    return row


def sampler_scripts(V):
    per = sampler_per(V)
    pairs = [(per - 1, per)] + ([(1023, 1024)] if V == 1025 else [])
    out = [SamplerScript(f"kth{a}_{b}", V, _kth_pair(V, a, b, False), (a, b), a, False) for a, b in pairs]
    a, b = pairs[0]
    out.append(SamplerScript(f"zeros{a}_{b}", V, _kth_pair(V, a, b, True), (a, b), b, True))     # by the order of the bits +0.0 is the larger
    return out


# ---- beam search over one row: every beam sees the same logits ------------------------------------------------------------------------------
def beam_logp_of(row, rules=None, guard=None):
    """beam_ref.replay_pairs' logp_of: tokens (B, k, n) -> (B, k, V) float64 log-probabilities of the fixed row after every prefix, -inf
    where the prefix's rule state (rules.run) or the guard's ban set on the prefix forbids the token"""
    lp = expect(row).logp

    def logp_of(tokens):
        tokens = np.asarray(tokens, np.int64)
        B, k, _ = tokens.shape
        out = np.broadcast_to(lp, (B, k, lp.shape[0])).copy()
        for b in range(B):
            for j in range(k):
                pre = tokens[b, j].tolist()
                if rules is not None:
                    out[b, j][~rules.allowed(rules.run(pre)[0][None])[0]] = -np.inf
                if guard is not None:
                    out[b, j][sorted(guard_ref.banned(pre, guard[0], guard[1]))] = -np.inf
        return out
    return logp_of
