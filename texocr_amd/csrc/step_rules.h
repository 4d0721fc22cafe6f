// Constrained decode (texocr.h: txo_set_token_rules): the token selection of step.h / step_prefix.h with a per-row automaton that says which
// tokens a row may pick.
//
// A rule set is a table rules[S][V] of packed int32 (1 <= S <= 8 states) and a scalar depth_max (1 .. 255).  An entry packs
//   bits 0-7  need  (unsigned)     bits 8-15  delta (signed)     bits 16-23  next     bit 24  BAN     bit 25  ONLY_AT_ZERO
// Every row of the batch carries (s, depth), (0, 0) at the start.  In (s, depth) token v with r = rules[s][v] is allowed iff
//   !BAN  &&  depth >= need  &&  depth + delta <= depth_max  &&  (!ONLY_AT_ZERO || depth == 0)
// and committing it -- picked or forced -- moves the row to (next, clamp(depth + delta, 0, depth_max)).  A disallowed logit takes the
// selection's sentinel -3.4e38f: greedy is the arg-max of the masked row (ties -> lowest index), sampling feeds the masked row to step.h's
// unchanged samplers (a masked entry inside the kept set has probability exactly 0, which their `> 0` tests never pick).  Installation
// (txo_set_token_rules) has checked that every state has a token that is allowed at every depth, so no row ever faces an empty allowed set.
//
// logp keeps step.h's meaning: log_softmax of the RAW row over the whole vocabulary at the committed token -- a token the rules forced on the
// row shows up with its low probability, nothing is renormalised.
//
// The state is indexed by row of the BATCH through out_row, like outputs and sampler keys: compaction and row ranges move nothing.  A row
// frozen by the per-row stop keeps its state.  rule_hist[row][t] keeps the state behind position t: the host enqueues a few positions ahead of
// its look at the eos break, and the state a call reports is the one behind its last RETURNED position (rules_settle_kernel).
//
// Kernels of their own, behind every other kernel of the library: with StepArgs::rules == null the steps run step.h's / step_prefix.h's
// kernels as they were.  One wave per row, like them.
#pragma once
#include "step_prefix.h"

namespace txo {

constexpr int RULE_BAN = 1 << 24, RULE_ONLY_AT_ZERO = 1 << 25;
constexpr int RULES_MAX_STATES = 8;

__host__ __device__ inline int rule_need(int r) { return r & 0xff; }
__host__ __device__ inline int rule_delta(int r) { return (int)(signed char)((r >> 8) & 0xff); }
__host__ __device__ inline int rule_next(int r) { return (r >> 16) & 0xff; }
__host__ __device__ inline bool rule_allows(int r, int depth, int depth_max) {
    return !(r & RULE_BAN) && depth >= rule_need(r) && depth + rule_delta(r) <= depth_max && (!(r & RULE_ONLY_AT_ZERO) || depth == 0);
}
__host__ __device__ inline int rule_depth_after(int r, int depth, int depth_max) {
    const int d = depth + rule_delta(r);
    return d < 0 ? 0 : (d > depth_max ? depth_max : d);
}
__device__ inline float rule_mask(float v, int r, int depth, int depth_max) { return rule_allows(r, depth, depth_max) ? v : -3.4e38f; }

// the row's state and its row of the table (lane-uniform)
struct RuleRow { const int* rl; int s, depth; };
__device__ inline RuleRow rule_row(const StepArgs& a, int orow) {
    const int2 sd = a.rule_state[orow];
    const int s = (unsigned)sd.x < (unsigned)a.n_states ? sd.x : 0;
    return {a.rules + (size_t)s * a.V, s, sd.y};
}
// behind a commit (lane 0 of a row; frozen: the per-row stop had finished the row BEFORE this token -- commit_token's own test, taken before it)
__device__ inline void rule_advance(const StepArgs& a, int orow, int t, const RuleRow& rr, int tok, bool frozen) {
    if (frozen) return;
    const int r = rr.rl[in_vocab(tok, a.V)];
    const int2 nx = make_int2(rule_next(r), rule_depth_after(r, rr.depth, a.depth_max));
    a.rule_state[orow] = nx;
    if (a.rule_hist && t < a.rule_hist_stride) a.rule_hist[(size_t)orow * a.rule_hist_stride + t] = nx;
}

// stream_row's single pass (step_prefix.h; both branches) with the matching requests on the rules row in flight beside the logits: the running
// log-sum-exp over the RAW values (the same lse_push / lse_push4 calls in the same order), best / bi over the MASKED values; lo: the raw row out
__device__ inline void stream_row_rules(const float* lg, const int* rl, int depth, int depth_max, int V, int lane, bool lp, float* lo,
                                        float& best, int& bi, float& lm, float& ls) {
    best = -3.4e38f; bi = 0x7fffffff; lm = -3.4e38f; ls = 0.f;
    if ((V & 3) == 0) {                        // rows of both tables are 16-byte aligned
        const int n4 = V >> 2;
        for (int base = 0; base < n4; base += 256) {
            float4 v[4]; int4 r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j4 = base + u * 64 + lane;
                v[u] = j4 < n4 ? reinterpret_cast<const float4*>(lg)[j4] : make_float4(-3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f);
                r[u] = j4 < n4 ? reinterpret_cast<const int4*>(rl)[j4] : make_int4(RULE_BAN, RULE_BAN, RULE_BAN, RULE_BAN);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j4 = base + u * 64 + lane;
                if (j4 >= n4) continue;
                if (lo) reinterpret_cast<float4*>(lo)[j4] = v[u];
                if (lp) lse_push4(lm, ls, v[u]);
                const int j = j4 * 4;                          // ascending index: first maximum wins inside a lane
                const float mx = rule_mask(v[u].x, r[u].x, depth, depth_max), my = rule_mask(v[u].y, r[u].y, depth, depth_max);
                const float mz = rule_mask(v[u].z, r[u].z, depth, depth_max), mw = rule_mask(v[u].w, r[u].w, depth, depth_max);
                if (mx > best) { best = mx; bi = j; }
                if (my > best) { best = my; bi = j + 1; }
                if (mz > best) { best = mz; bi = j + 2; }
                if (mw > best) { best = mw; bi = j + 3; }
            }
        }
    } else {
        for (int j = lane; j < V; j += 64) {
            const float v = lg[j];
            const int r = rl[j];
            if (lo) lo[j] = v;
            if (lp) lse_push(lm, ls, v);
            const float m = rule_mask(v, r, depth, depth_max);
            if (m > best) { best = m; bi = j; }
        }
    }
    wave_argmax(best, bi);
}
// log_softmax(raw row)[tok] from the lanes' running (max, sum): (lg[tok] - raw max) - log sum exp(v - raw max).  Where tok is the raw arg-max the
// first term is exactly 0 and the float is argmax_step_kernel's -lse_finish(...), bit for bit; for a forced token it is forced_logp's.
__device__ inline float raw_logp(const float* lg, int V, int tok, float lm, float ls) {
    const float rawmax = wave_max(lm);
    return (lg[in_vocab(tok, V)] - rawmax) - lse_finish(lm, ls, rawmax);
}

// the commit of either kernel below: step.h's / step_prefix.h's, then the row's next state
__device__ inline void commit_rules(const StepArgs& a, int row, int orow, int t, const RuleRow& rr, int tok, float logp, bool forced, int len) {
    const bool frozen = a.stop_rows && a.eos >= 0 && a.eos_seen[row];
    if (a.forced) commit_prompted(a, row, orow, t, tok, logp, forced, len);
    else commit_token(a, row, t, tok, logp);
    rule_advance(a, orow, t, rr, tok, frozen);
}

__global__ __launch_bounds__(64) void argmax_rules_step_kernel(StepArgs a) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const int t = a.st->t;
    const int orow = out_row(a, row);
    int len = 0;
    const int ftok = a.forced ? forced_token(a, orow, t, len) : -1;
    const bool forced = ftok >= 0;
    const bool lp = forced ? a.prefix_logp != nullptr : a.logp_out != nullptr;
    const RuleRow rr = rule_row(a, orow);
    const float* lg = a.logits + (size_t)row * a.V;
    float* lo = (a.logits_out && !a.forced) ? a.logits_out + ((size_t)orow * a.out_stride + t) * a.V : nullptr;   // (the prompted entries keep no logits)
    float best, lm, ls; int bi;
    stream_row_rules(lg, rr.rl, rr.depth, a.depth_max, a.V, lane, lp, lo, best, bi, lm, ls);
    const int tok = forced ? ftok : bi;                                        // a forced token is never masked
    float logp = 0.f;
    if (lp) logp = raw_logp(lg, a.V, tok, lm, ls);
    if (lane == 0) commit_rules(a, row, orow, t, rr, tok, logp, forced, len);
}

// the sampler's step: step.h's samplers on masked loads, want_lp = false; the log-probability (and the raw logits_out) from one more pass over
// the raw row.  A forced position consumes no draw.  REGS as sample_step_kernel.
template <bool REGS>
__global__ __launch_bounds__(64) void sample_rules_step_kernel(StepArgs a) {
    extern __shared__ float row_lds[];
    const int row = blockIdx.x, lane = threadIdx.x, V = a.V;
    const int t = a.st->t;
    const float* lg = a.logits + (size_t)row * V;
    const int orow = out_row(a, row);
    int len = 0;
    const int ftok = a.forced ? forced_token(a, orow, t, len) : -1;
    const RuleRow rr = rule_row(a, orow);
    if (ftok >= 0) {                                                           // (wave-uniform: one row per wave)
        float logp = 0.f;
        if (a.prefix_logp) {
            float best, lm, ls, wv; int bi;
            stream_row(lg, V, lane, true, ftok, best, bi, lm, ls, wv);
            logp = forced_logp(best, lm, ls, wv);
        }
        if (lane == 0) commit_rules(a, row, orow, t, rr, ftok, logp, true, len);
        return;
    }
    const int* rl = rr.rl;
    const int depth = rr.depth, dmax = a.depth_max;
    auto load = [&](int j) { return rule_mask(lg[j], rl[j], depth, dmax); };
    int pick; float unused = 0.f;
    if constexpr (REGS) {
        auto load4 = [&](int j) {
            u32x4 w = ld16(lg + j);
            const u32x4 r = ld16(rl + j);
            const unsigned NO = __float_as_uint(-3.4e38f);
            w.x = rule_allows((int)r.x, depth, dmax) ? w.x : NO; w.y = rule_allows((int)r.y, depth, dmax) ? w.y : NO;
            w.z = rule_allows((int)r.z, depth, dmax) ? w.z : NO; w.w = rule_allows((int)r.w, depth, dmax) ? w.w : NO;
            return w;
        };
        pick = sample_row_regs(load, load4, nullptr, V, lane, a.topk, a.inv_temp, a.seed, (unsigned)(a.row0 + orow), (unsigned)t, false, unused);
    } else {
        pick = sample_row_lds(load, row_lds, nullptr, V, lane, a.topk, a.inv_temp, a.seed, (unsigned)(a.row0 + orow), (unsigned)t, false, unused);
    }
    float* lo = (a.logits_out && !a.forced) ? a.logits_out + ((size_t)orow * a.out_stride + t) * V : nullptr;
    const bool lp = a.logp_out != nullptr;
    float logp = 0.f;
    if (lp || lo) {                                                            // (wave-uniform) the raw row once more
        float lm = -3.4e38f, ls = 0.f;
        for (int j = lane; j < V; j += 64) {
            const float v = lg[j];
            if (lo) lo[j] = v;
            if (lp) lse_push(lm, ls, v);
        }
        if (lp) logp = raw_logp(lg, V, pick, lm, ls);
    }
    if (lane == 0) commit_rules(a, row, orow, t, rr, pick, logp, false, len);
}
inline void launch_rules_step(hipStream_t s, int rows, const StepArgs& sa, bool sample) {
    if (!sample) hipLaunchKernelGGL(argmax_rules_step_kernel, dim3(rows), dim3(64), 0, s, sa);
    else if (sample_in_regs(sa.V)) hipLaunchKernelGGL(sample_rules_step_kernel<true>, dim3(rows), dim3(64), 0, s, sa);
    else hipLaunchKernelGGL(sample_rules_step_kernel<false>, dim3(rows), dim3(64), (size_t)sa.V * sizeof(float), s, sa);
}

// (re)start the automaton of every row of the BATCH, beside reset_state_kernel / prefix_start_kernel: (0, 0), and for a prompted decode (m > 0)
// run over prefix columns 1 .. m-1 -- the tokens the multi-position pass has consumed (column 0 is the start token, which nothing committed)
__global__ void rules_start_kernel(int2* state, int rows, const int* rules, int V, int n_states, int depth_max, const int64_t* table, int stride, int m) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    int s = 0, depth = 0;
    for (int c = 1; c < m; ++c) {
        const int r = rules[(size_t)s * V + in_vocab((int)table[(size_t)i * stride + c], V)];
        depth = rule_depth_after(r, depth, depth_max);
        s = rule_next(r) < n_states ? rule_next(r) : 0;
    }
    state[i] = make_int2(s, depth);
}
// the end of a decode whose rows all ran every position (no per-row stop): the state behind position `last`, the last one the call returns -- the
// loop may have run a few positions more before the host saw the eos break.  A prompted decode (len: the rows' prefix lengths, else null) returns
// n_cols columns, and row b wrote its last one at position len_b + n_cols - 2: rows with a shorter prefix stop counting there.
__global__ void rules_settle_kernel(int2* state, const int2* hist, int stride, int rows, int last, const int* len, int n_cols) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    if (len) last = min(last, len[i] + n_cols - 2);
    if (last >= 0) state[i] = hist[(size_t)i * stride + last];
}
// txo_last_rule_state: the states to the caller's int32 [B][2]
__global__ void rules_state_out_kernel(int* out, const int2* state, int rows) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) { out[2 * i] = state[i].x; out[2 * i + 1] = state[i].y; }
}

// ---- closing decode (texocr.h: txo_set_rules_close) -----------------------------------------------------------------------------------------
// The rules above with a budget: a row may only pick a token from which its automaton can still reach eos in the positions the call has left.
// dist[s][d] (rules_close.h, computed on the host at installation) is the least number of picks, the eos included, from (s, d) to a committed
// eos.  A row in (s, d) that has not committed an eos, with R picks left in what the call returns (this one included) and D = dist[s][d]
// finite, may pick v iff the rule allows it AND (v == eos OR dist[next][depth after v] <= max(R, D) - 1).  Some allowed token always leads to
// D - 1, so the set is never empty; D <= R at a row's first pick ends the row at an allowed eos inside its R picks; D > R (a forced prefix)
// takes distance-reducing tokens only and ends open.  A row that has committed its eos, or stands where D is infinite, runs the plain rule.
//
// R comes from device-side state: the position word every step reads and the row's end position rule_close[row].x (the position behind its
// last returned one: prefix length + max_len - 1, so R = end - t), written once per call by rules_close_start_kernel -- a captured step bakes
// neither.  rule_close[row].y: the row has committed an eos.  Both by row of the BATCH, like the state.
//
// While R - 1 >= slack no token can be budgeted away (every move lands within dist_max <= R - 1) and the wave runs the plain kernels' masking
// code: the picks are theirs bit for bit.  A table with an infinite entry has no such slack -- a token may lead to a node that cannot close at
// all -- and its rows are budgeted at every position (slack = INT_MAX).  The budgeted branch costs one more dependent look-up per vocabulary
// entry, at an index every lane computes from its own entry: not a scalar load.  The table (at most 8 * 256 nodes of 16 bits = 4 KB) is staged
// into LDS with 16-byte loads first -- one wave's 64 look-ups per instruction is what LDS serves, and only the last dist_max positions of a row
// pay the staging.
constexpr int CLOSE_NODES = RULES_MAX_STATES * 256;
constexpr int CLOSE_FAR = 0xffff;                                  // an entry without a path (CLOSE_INF of rules_close.h)
struct CloseTable {
    unsigned short dist[CLOSE_NODES];                              // [n_states][depth_max + 1], CLOSE_FAR behind it: whole 16-byte pieces are read
    int slack, dist_max, pad[2];
};
struct CloseRow { bool bind; int lim; };                           // (lane-uniform) budgeted: a non-eos token must land at a distance <= lim
__device__ inline CloseRow close_row(const CloseTable* ct, int2 ce, int t, int s, int depth, int depth_max) {
    const int R = ce.x - t;
    if (ce.y || R - 1 >= ct->slack) return {false, 0};
    const int D = ct->dist[(s * (depth_max + 1) + min(max(depth, 0), depth_max)) & (CLOSE_NODES - 1)];
    if (D == CLOSE_FAR) return {false, 0};
    return {true, min(max(R, D) - 1, CLOSE_FAR - 1)};
}
// the first `nodes` entries into LDS, in 16-byte pieces, by the workgroup's `threads` threads; a barrier behind it
__device__ inline void close_stage(unsigned short* cl, const CloseTable* ct, int nodes, int tid, int threads) {
    const int n16 = (nodes * 2 + 15) >> 4;
    for (int i = tid; i < n16; i += threads) reinterpret_cast<uint4*>(cl)[i] = reinterpret_cast<const uint4*>(ct->dist)[i];
    __syncthreads();
}
__device__ inline bool close_allows(const unsigned short* cl, int r, int v, int depth, int depth_max, int eos, int lim) {
    if (!rule_allows(r, depth, depth_max)) return false;
    return v == eos || (int)cl[(rule_next(r) * (depth_max + 1) + rule_depth_after(r, depth, depth_max)) & (CLOSE_NODES - 1)] <= lim;
}
__device__ inline float close_mask(const unsigned short* cl, float x, int r, int v, int depth, int depth_max, int eos, int lim) {
    return close_allows(cl, r, v, depth, depth_max, eos, lim) ? x : -3.4e38f;
}
// stream_row_rules with the budgeted mask: the same requests, the same log-sum-exp calls in the same order, best / bi over the budgeted row
__device__ inline void stream_row_close(const float* lg, const int* rl, const unsigned short* cl, int depth, int depth_max, int eos, int lim, int V,
                                        int lane, bool lp, float* lo, float& best, int& bi, float& lm, float& ls) {
    best = -3.4e38f; bi = 0x7fffffff; lm = -3.4e38f; ls = 0.f;
    if ((V & 3) == 0) {
        const int n4 = V >> 2;
        for (int base = 0; base < n4; base += 256) {
            float4 v[4]; int4 r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j4 = base + u * 64 + lane;
                v[u] = j4 < n4 ? reinterpret_cast<const float4*>(lg)[j4] : make_float4(-3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f);
                r[u] = j4 < n4 ? reinterpret_cast<const int4*>(rl)[j4] : make_int4(RULE_BAN, RULE_BAN, RULE_BAN, RULE_BAN);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j4 = base + u * 64 + lane;
                if (j4 >= n4) continue;
                if (lo) reinterpret_cast<float4*>(lo)[j4] = v[u];
                if (lp) lse_push4(lm, ls, v[u]);
                const int j = j4 * 4;
                const float mx = close_mask(cl, v[u].x, r[u].x, j, depth, depth_max, eos, lim), my = close_mask(cl, v[u].y, r[u].y, j + 1, depth, depth_max, eos, lim);
                const float mz = close_mask(cl, v[u].z, r[u].z, j + 2, depth, depth_max, eos, lim), mw = close_mask(cl, v[u].w, r[u].w, j + 3, depth, depth_max, eos, lim);
                if (mx > best) { best = mx; bi = j; }
                if (my > best) { best = my; bi = j + 1; }
                if (mz > best) { best = mz; bi = j + 2; }
                if (mw > best) { best = mw; bi = j + 3; }
            }
        }
    } else {
        for (int j = lane; j < V; j += 64) {
            const float v = lg[j];
            const int r = rl[j];
            if (lo) lo[j] = v;
            if (lp) lse_push(lm, ls, v);
            const float m = close_mask(cl, v, r, j, depth, depth_max, eos, lim);
            if (m > best) { best = m; bi = j; }
        }
    }
    wave_argmax(best, bi);
}
// commit_rules, then the row's "has committed eos" (picked or forced; a row the per-row stop froze committed one long ago)
__device__ inline void commit_close(const StepArgs& a, int row, int orow, int t, const RuleRow& rr, int tok, float logp, bool forced, int len) {
    commit_rules(a, row, orow, t, rr, tok, logp, forced, len);
    if (a.eos >= 0 && in_vocab(tok, a.V) == a.eos) a.rule_close[orow].y = 1;
}

__global__ __launch_bounds__(64) void argmax_rules_close_step_kernel(StepArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned short cl[CLOSE_NODES];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int t = a.st->t;
    const int orow = out_row(a, row);
    int len = 0;
    const int ftok = a.forced ? forced_token(a, orow, t, len) : -1;
    const bool forced = ftok >= 0;
    const bool lp = forced ? a.prefix_logp != nullptr : a.logp_out != nullptr;
    const RuleRow rr = rule_row(a, orow);
    const CloseTable* ct = static_cast<const CloseTable*>(a.close_tab);
    const CloseRow cr = forced ? CloseRow{false, 0} : close_row(ct, a.rule_close[orow], t, rr.s, rr.depth, a.depth_max);
    const float* lg = a.logits + (size_t)row * a.V;
    float* lo = (a.logits_out && !a.forced) ? a.logits_out + ((size_t)orow * a.out_stride + t) * a.V : nullptr;
    float best, lm, ls; int bi;
    if (!cr.bind) {                                                            // (wave-uniform) slack, an ended row, a forced token: the plain rule's code
        stream_row_rules(lg, rr.rl, rr.depth, a.depth_max, a.V, lane, lp, lo, best, bi, lm, ls);
    } else {
        close_stage(cl, ct, a.n_states * (a.depth_max + 1), lane, 64);
        stream_row_close(lg, rr.rl, cl, rr.depth, a.depth_max, a.eos, cr.lim, a.V, lane, lp, lo, best, bi, lm, ls);
    }
    const int tok = forced ? ftok : bi;
    float logp = 0.f;
    if (lp) logp = raw_logp(lg, a.V, tok, lm, ls);
    if (lane == 0) commit_close(a, row, orow, t, rr, tok, logp, forced, len);
}

template <bool REGS>
__global__ __launch_bounds__(64) void sample_rules_close_step_kernel(StepArgs a) {
    extern __shared__ float row_lds[];
    __shared__ __attribute__((aligned(16))) unsigned short cl[CLOSE_NODES];
    const int row = blockIdx.x, lane = threadIdx.x, V = a.V;
    const int t = a.st->t;
    const float* lg = a.logits + (size_t)row * V;
    const int orow = out_row(a, row);
    int len = 0;
    const int ftok = a.forced ? forced_token(a, orow, t, len) : -1;
    const RuleRow rr = rule_row(a, orow);
    if (ftok >= 0) {                                                           // (wave-uniform: one row per wave)
        float logp = 0.f;
        if (a.prefix_logp) {
            float best, lm, ls, wv; int bi;
            stream_row(lg, V, lane, true, ftok, best, bi, lm, ls, wv);
            logp = forced_logp(best, lm, ls, wv);
        }
        if (lane == 0) commit_close(a, row, orow, t, rr, ftok, logp, true, len);
        return;
    }
    const CloseTable* ct = static_cast<const CloseTable*>(a.close_tab);
    const CloseRow cr = close_row(ct, a.rule_close[orow], t, rr.s, rr.depth, a.depth_max);
    const int* rl = rr.rl;
    const int depth = rr.depth, dmax = a.depth_max, eos = a.eos, lim = cr.lim;
    const unsigned NO = __float_as_uint(-3.4e38f);
    int pick; float unused = 0.f;
    if (!cr.bind) {                                                            // (wave-uniform) the plain rule's loads
        auto load = [&](int j) { return rule_mask(lg[j], rl[j], depth, dmax); };
        if constexpr (REGS) {
            auto load4 = [&](int j) {
                u32x4 w = ld16(lg + j);
                const u32x4 r = ld16(rl + j);
                w.x = rule_allows((int)r.x, depth, dmax) ? w.x : NO; w.y = rule_allows((int)r.y, depth, dmax) ? w.y : NO;
                w.z = rule_allows((int)r.z, depth, dmax) ? w.z : NO; w.w = rule_allows((int)r.w, depth, dmax) ? w.w : NO;
                return w;
            };
            pick = sample_row_regs(load, load4, nullptr, V, lane, a.topk, a.inv_temp, a.seed, (unsigned)(a.row0 + orow), (unsigned)t, false, unused);
        } else {
            pick = sample_row_lds(load, row_lds, nullptr, V, lane, a.topk, a.inv_temp, a.seed, (unsigned)(a.row0 + orow), (unsigned)t, false, unused);
        }
    } else {
        close_stage(cl, ct, a.n_states * (dmax + 1), lane, 64);
        auto load = [&](int j) { return close_mask(cl, lg[j], rl[j], j, depth, dmax, eos, lim); };
        if constexpr (REGS) {
            auto load4 = [&](int j) {
                u32x4 w = ld16(lg + j);
                const u32x4 r = ld16(rl + j);
                w.x = close_allows(cl, (int)r.x, j, depth, dmax, eos, lim) ? w.x : NO; w.y = close_allows(cl, (int)r.y, j + 1, depth, dmax, eos, lim) ? w.y : NO;
                w.z = close_allows(cl, (int)r.z, j + 2, depth, dmax, eos, lim) ? w.z : NO; w.w = close_allows(cl, (int)r.w, j + 3, depth, dmax, eos, lim) ? w.w : NO;
                return w;
            };
            pick = sample_row_regs(load, load4, nullptr, V, lane, a.topk, a.inv_temp, a.seed, (unsigned)(a.row0 + orow), (unsigned)t, false, unused);
        } else {
            pick = sample_row_lds(load, row_lds, nullptr, V, lane, a.topk, a.inv_temp, a.seed, (unsigned)(a.row0 + orow), (unsigned)t, false, unused);
        }
    }
    float* lo = (a.logits_out && !a.forced) ? a.logits_out + ((size_t)orow * a.out_stride + t) * V : nullptr;
    const bool lp = a.logp_out != nullptr;
    float logp = 0.f;
    if (lp || lo) {                                                            // (wave-uniform) the raw row once more
        float lm = -3.4e38f, ls = 0.f;
        for (int j = lane; j < V; j += 64) {
            const float v = lg[j];
            if (lo) lo[j] = v;
            if (lp) lse_push(lm, ls, v);
        }
        if (lp) logp = raw_logp(lg, V, pick, lm, ls);
    }
    if (lane == 0) commit_close(a, row, orow, t, rr, pick, logp, false, len);
}
inline void launch_rules_close_step(hipStream_t s, int rows, const StepArgs& sa, bool sample) {
    if (!sample) hipLaunchKernelGGL(argmax_rules_close_step_kernel, dim3(rows), dim3(64), 0, s, sa);
    else if (sample_in_regs(sa.V)) hipLaunchKernelGGL(sample_rules_close_step_kernel<true>, dim3(rows), dim3(64), 0, s, sa);
    else hipLaunchKernelGGL(sample_rules_close_step_kernel<false>, dim3(rows), dim3(64), (size_t)sa.V * sizeof(float), s, sa);
}
// beside rules_start_kernel: every row's end position -- the position behind the last one the call returns for it, prefix length (len null: 1,
// the BOS column) + max_len - 1 -- and whether the prefix columns the multi-position pass consumed (1 .. m-1) hold an eos
__global__ void rules_close_start_kernel(int2* close, int rows, const int* len, int max_len, int eos, const int64_t* table, int stride, int m) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    int ended = 0;
    if (eos >= 0) for (int c = 1; c < m; ++c) ended |= table[(size_t)i * stride + c] == eos ? 1 : 0;
    close[i] = make_int2((len ? len[i] : 1) + max_len - 1, ended);
}

}  // namespace txo
