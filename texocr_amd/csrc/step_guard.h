// Repeat guard (texocr.h: txo_set_repeat_guard): the token selection of step.h / step_prefix.h / step_rules.h with a ban on the token that
// would make a row end in max_repeats + 1 consecutive copies of one block of at most max_period tokens.
//
// Two integers, P = max_period and R = max_repeats, both in 1 .. 16.  A row's history at a pick is h[0 .. n-1]: every token the row has
// committed behind its start token, forced prefix tokens first, then its own picks (n = the position).  For a period p in 1 .. P, p <= n,
// m_p counts the trailing positions i with i - p >= 0 and h[i] == h[i - p], back from n - 1 to the first mismatch, and token h[n - p] is
// BANNED at this pick iff m_p >= R * p - 1: committing it would end the row in R + 1 copies of a p-token block.  The eos token is never
// banned, a forced token is never masked.  A banned logit takes the selection's sentinel -3.4e38f, exactly as a rule-disallowed one:
// greedy is the arg-max of the masked row (ties -> lowest index), sampling feeds the masked row to step.h's unchanged samplers.  logp and
// logits_out stay the RAW row's, nothing is renormalised.
//
// With token rules (StepArgs::rules != null; null: every token allowed) a token must be rule-allowed AND unbanned; if no token is both, the
// ban is dropped for that pick and the rules alone decide (installation guarantees one allowed token per state, and the guard may ban just
// that one).  The automaton advances on the committed token as in step_rules.h.
//
// Nothing is kept between picks: the ban set is computed from the committed tokens at every pick, read through ONE helper (guard_hist) --
// the forced table for the columns a prefix covers, tokens_out behind it, with the prompted decode's per-row output shift, by row of the
// BATCH (out_row) -- so the position word, live-row compaction, row ranges, captured steps and the host's run-ahead need no bookkeeping.
//
// The ban set (at most P tokens) goes into a V-bit map in LDS and the streaming pass tests one bit per logit (one LDS word per 16-byte
// request: four consecutive ids share a word).  The alternative, the P banned ids in scalar registers and up to sixteen compares per
// logit, costs more vector instructions per logit than the log-sum-exp the pass already carries, at every P; the map costs V / 32 words
// cleared per pick and is the same code for every P.
//
// Kernels of their own, behind every other kernel of the library: with no guard set the steps run the kernels they ran before.  One wave
// per row, like them.  Dynamic LDS: the bit map (guard_map_bytes), behind the staged row in the LDS form of the sampler.
#pragma once
#include "step_rules.h"

namespace txo {

constexpr int GUARD_MAX = 16;                                      // the largest max_period and max_repeats
__host__ __device__ inline size_t guard_map_bytes(int V) { return (size_t)((V + 31) >> 5) * sizeof(unsigned); }

// h[i] of the row (i < t, the position): the i-th token committed behind the start token; -1 where the call keeps no such column (a pick
// of a prompted decode beyond the returned columns: committed, never written).  len: the row's prefix length (0: not prompted)
__device__ inline int guard_hist(const StepArgs& a, int orow, int len, int i) {
    if (a.forced) {
        if (i + 1 < len) return (int)a.forced[(size_t)orow * a.forced_stride + i + 1];
        const int j = i + 1 - len;                                             // the prompted decode's output shift
        return j < a.out_cols ? (int)a.tokens_out[(size_t)orow * a.out_stride + j] : -1;
    }
    return (int)a.tokens_out[(size_t)orow * a.out_stride + i];
}
// the token lane p - 1 bans at position t (history length n = t), or -1.  Lanes take periods; the scan back makes at most R * p - 1
// comparisons and stops at the first mismatch
__device__ inline int guard_ban(const StepArgs& a, int orow, int len, int t, int lane) {
    const int p = lane + 1, n = t;
    if (p > a.guard_p || p > n) return -1;
    const int need = a.guard_r * p - 1;
    int m = 0;
    while (m < need) {
        const int i = n - 1 - m;
        if (i - p < 0) break;
        const int x = guard_hist(a, orow, len, i);
        if (x < 0 || x != guard_hist(a, orow, len, i - p)) break;
        ++m;
    }
    if (m < need) return -1;
    const int tok = guard_hist(a, orow, len, n - p);
    return ((unsigned)tok < (unsigned)a.V && tok != a.eos) ? tok : -1;         // (a finished row's columns are not written: whatever they hold stays in range)
}
// the row's ban set into the map (one wave; words = (V + 31) / 32); returns whether any token is banned (wave-uniform)
__device__ inline bool guard_stage(unsigned* bm, const StepArgs& a, int orow, int len, int t, int lane) {
    const int words = (a.V + 31) >> 5;
    for (int w = lane; w < words; w += 64) bm[w] = 0u;
    __syncthreads();
    const int tok = guard_ban(a, orow, len, t, lane);
    if (tok >= 0) atomicOr(&bm[tok >> 5], 1u << (tok & 31));
    __syncthreads();
    return __ballot(tok >= 0) != 0ull;
}
__device__ inline bool guard_bit(const unsigned* bm, int j) { return (bm[j >> 5] >> (j & 31)) & 1u; }

// the rules of the row, or "every token allowed": entry 0 at depth 0 under cap 0 is allowed (need 0, delta 0, no flag)
struct GuardRules { const int* rl; int depth, dmax; };

// stream_row_rules's single pass (both branches, the same requests, the same log-sum-exp calls over the RAW values in the same order) with two
// arg-maxes: best / bi over the rows masked by rules AND guard, rbest / rbi over the row masked by the rules alone (what the pick yields to
// when nothing is both allowed and unbanned)
__device__ inline void stream_row_guard(const float* lg, const GuardRules& g, const unsigned* bm, int V, int lane, bool lp, float* lo,
                                        float& best, int& bi, float& rbest, int& rbi, float& lm, float& ls) {
    best = -3.4e38f; bi = 0x7fffffff; rbest = -3.4e38f; rbi = 0x7fffffff; lm = -3.4e38f; ls = 0.f;
    const int* rl = g.rl;
    if ((V & 3) == 0) {                        // rows of both tables are 16-byte aligned
        const int n4 = V >> 2;
        for (int base = 0; base < n4; base += 256) {
            float4 v[4]; int4 r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j4 = base + u * 64 + lane;
                v[u] = j4 < n4 ? reinterpret_cast<const float4*>(lg)[j4] : make_float4(-3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f);
                r[u] = (rl && j4 < n4) ? reinterpret_cast<const int4*>(rl)[j4] : make_int4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j4 = base + u * 64 + lane;
                if (j4 >= n4) continue;
                if (lo) reinterpret_cast<float4*>(lo)[j4] = v[u];
                if (lp) lse_push4(lm, ls, v[u]);
                const int j = j4 * 4;                          // ascending index: first maximum wins inside a lane
                const unsigned w = bm[j >> 5] >> (j & 31);     // four consecutive ids, one word
                const float rx = rule_mask(v[u].x, r[u].x, g.depth, g.dmax), ry = rule_mask(v[u].y, r[u].y, g.depth, g.dmax);
                const float rz = rule_mask(v[u].z, r[u].z, g.depth, g.dmax), rw = rule_mask(v[u].w, r[u].w, g.depth, g.dmax);
                if (rx > rbest) { rbest = rx; rbi = j; }
                if (ry > rbest) { rbest = ry; rbi = j + 1; }
                if (rz > rbest) { rbest = rz; rbi = j + 2; }
                if (rw > rbest) { rbest = rw; rbi = j + 3; }
                const float mx = (w & 1u) ? -3.4e38f : rx, my = (w & 2u) ? -3.4e38f : ry;
                const float mz = (w & 4u) ? -3.4e38f : rz, mw = (w & 8u) ? -3.4e38f : rw;
                if (mx > best) { best = mx; bi = j; }
                if (my > best) { best = my; bi = j + 1; }
                if (mz > best) { best = mz; bi = j + 2; }
                if (mw > best) { best = mw; bi = j + 3; }
            }
        }
    } else {
        for (int j = lane; j < V; j += 64) {
            const float v = lg[j];
            const int r = rl ? rl[j] : 0;
            if (lo) lo[j] = v;
            if (lp) lse_push(lm, ls, v);
            const float rm = rule_mask(v, r, g.depth, g.dmax);
            if (rm > rbest) { rbest = rm; rbi = j; }
            const float m = guard_bit(bm, j) ? -3.4e38f : rm;
            if (m > best) { best = m; bi = j; }
        }
    }
    wave_argmax(best, bi);
    wave_argmax(rbest, rbi);
}

// the commit of either kernel below: step_rules.h's under rules, step.h's / step_prefix.h's without
__device__ inline void commit_guard(const StepArgs& a, int row, int orow, int t, const RuleRow& rr, int tok, float logp, bool forced, int len) {
    if (a.rules) commit_rules(a, row, orow, t, rr, tok, logp, forced, len);
    else if (a.forced) commit_prompted(a, row, orow, t, tok, logp, forced, len);
    else commit_token(a, row, t, tok, logp);
}

__global__ __launch_bounds__(64) void argmax_guard_step_kernel(StepArgs a) {
    extern __shared__ unsigned guard_lds[];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int t = a.st->t;
    const int orow = out_row(a, row);
    int len = 0;
    const int ftok = a.forced ? forced_token(a, orow, t, len) : -1;
    const bool forced = ftok >= 0;
    const bool lp = forced ? a.prefix_logp != nullptr : a.logp_out != nullptr;
    const RuleRow rr = a.rules ? rule_row(a, orow) : RuleRow{nullptr, 0, 0};
    const GuardRules g{rr.rl, rr.depth, a.rules ? a.depth_max : 0};
    guard_stage(guard_lds, a, orow, len, t, lane);
    const float* lg = a.logits + (size_t)row * a.V;
    float* lo = (a.logits_out && !a.forced) ? a.logits_out + ((size_t)orow * a.out_stride + t) * a.V : nullptr;   // (the prompted entries keep no logits)
    float best, rbest, lm, ls; int bi, rbi;
    stream_row_guard(lg, g, guard_lds, a.V, lane, lp, lo, best, bi, rbest, rbi, lm, ls);
    // nothing both allowed and unbanned (the guarded arg-max found no entry): the rules alone decide.  A forced token is never masked
    const int tok = forced ? ftok : (bi == 0x7fffffff ? rbi : bi);
    float logp = 0.f;
    if (lp) logp = raw_logp(lg, a.V, tok, lm, ls);
    if (lane == 0) commit_guard(a, row, orow, t, rr, tok, logp, forced, len);
}

// the sampler's step.  It decides before it samples: no ban and no rules -- step.h's / step_prefix.h's own sampler call, log-probability
// included (the same bits); otherwise the samplers on masked loads, want_lp = false, and the log-probability (and the raw logits_out) from one
// more pass over the raw row, as step_rules.h.  Under rules, a ban that leaves no token both allowed and unbanned is dropped first (one pass
// over the rules row).  A forced position consumes no draw.  REGS as sample_step_kernel; row_lds: the staged row (LDS form), the map behind it.
template <bool REGS>
__global__ __launch_bounds__(64) void sample_guard_step_kernel(StepArgs a) {
    extern __shared__ float row_lds[];
    unsigned* bm = reinterpret_cast<unsigned*>(REGS ? row_lds : row_lds + a.V);
    const int row = blockIdx.x, lane = threadIdx.x, V = a.V;
    const int t = a.st->t;
    const float* lg = a.logits + (size_t)row * V;
    const int orow = out_row(a, row);
    int len = 0;
    const int ftok = a.forced ? forced_token(a, orow, t, len) : -1;
    const RuleRow rr = a.rules ? rule_row(a, orow) : RuleRow{nullptr, 0, 0};
    if (ftok >= 0) {                                                           // (wave-uniform: one row per wave)
        float logp = 0.f;
        if (a.prefix_logp) {
            float best, lm, ls, wv; int bi;
            stream_row(lg, V, lane, true, ftok, best, bi, lm, ls, wv);
            logp = forced_logp(best, lm, ls, wv);
        }
        if (lane == 0) commit_guard(a, row, orow, t, rr, ftok, logp, true, len);
        return;
    }
    const int* rl = rr.rl;
    const int depth = rr.depth, dmax = a.rules ? a.depth_max : 0;
    bool ban = guard_stage(bm, a, orow, len, t, lane);
    if (ban && rl) {                                                           // (wave-uniform) does the ban leave an allowed token?
        bool any = false;
        for (int j = lane; j < V; j += 64) any = any || (rule_allows(rl[j], depth, dmax) && !guard_bit(bm, j));
        ban = __ballot(any) != 0ull;
    }
    float* lo = (a.logits_out && !a.forced) ? a.logits_out + ((size_t)orow * a.out_stride + t) * V : nullptr;
    const bool lp = a.logp_out != nullptr;
    int pick; float logp = 0.f;
    if (!ban && !rl) {                                                         // (wave-uniform) nothing to mask: the plain sampler, its own logp
        if constexpr (REGS) pick = sample_row_regs([&](int j) { return lg[j]; }, [&](int j) { return ld16(lg + j); }, lo, V, lane, a.topk, a.inv_temp, a.seed,
                                                   (unsigned)(a.row0 + orow), (unsigned)t, lp, logp);
        else pick = sample_row_lds([&](int j) { return lg[j]; }, row_lds, lo, V, lane, a.topk, a.inv_temp, a.seed, (unsigned)(a.row0 + orow), (unsigned)t,
                                   lp, logp);
        if (lane == 0) commit_guard(a, row, orow, t, rr, pick, logp, false, len);
        return;
    }
    const unsigned NO = __float_as_uint(-3.4e38f);
    auto ok = [&](int r, int j) { return rule_allows(r, depth, dmax) && !(ban && guard_bit(bm, j)); };
    auto load = [&](int j) { return ok(rl ? rl[j] : 0, j) ? lg[j] : -3.4e38f; };
    float unused = 0.f;
    if constexpr (REGS) {
        auto load4 = [&](int j) {
            u32x4 w = ld16(lg + j);
            u32x4 r = {0u, 0u, 0u, 0u};
            if (rl) r = ld16(rl + j);
            w.x = ok((int)r.x, j) ? w.x : NO; w.y = ok((int)r.y, j + 1) ? w.y : NO;
            w.z = ok((int)r.z, j + 2) ? w.z : NO; w.w = ok((int)r.w, j + 3) ? w.w : NO;
            return w;
        };
        pick = sample_row_regs(load, load4, nullptr, V, lane, a.topk, a.inv_temp, a.seed, (unsigned)(a.row0 + orow), (unsigned)t, false, unused);
    } else {
        pick = sample_row_lds(load, row_lds, nullptr, V, lane, a.topk, a.inv_temp, a.seed, (unsigned)(a.row0 + orow), (unsigned)t, false, unused);
    }
    if (lp || lo) {                                                            // (wave-uniform) the raw row once more
        float lm = -3.4e38f, ls = 0.f;
        for (int j = lane; j < V; j += 64) {
            const float v = lg[j];
            if (lo) lo[j] = v;
            if (lp) lse_push(lm, ls, v);
        }
        if (lp) logp = raw_logp(lg, V, pick, lm, ls);
    }
    if (lane == 0) commit_guard(a, row, orow, t, rr, pick, logp, false, len);
}
inline void launch_guard_step(hipStream_t s, int rows, const StepArgs& sa, bool sample) {
    const size_t map = guard_map_bytes(sa.V);
    if (!sample) hipLaunchKernelGGL(argmax_guard_step_kernel, dim3(rows), dim3(64), map, s, sa);
    else if (sample_in_regs(sa.V)) hipLaunchKernelGGL(sample_guard_step_kernel<true>, dim3(rows), dim3(64), map, s, sa);
    else hipLaunchKernelGGL(sample_guard_step_kernel<false>, dim3(rows), dim3(64), (size_t)sa.V * sizeof(float) + map, s, sa);
}

}  // namespace txo
