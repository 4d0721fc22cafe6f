// Prompted decode (texocr.h: txo_generate_prefix): the token selection of step.h with a caller's prefix forced into the loop.
//
// The caller gives prefix [B][P] and per-row lengths len_b; m = min len_b.  Positions 0 .. m-2 come from ONE multi-position pass (prefill),
// the loop starts at position m-1 (prefix_start_kernel) and at position t a row
//   * with t + 1 <  len_b commits prefix[b][t + 1]: no arg-max or draw decides, no output column is written, and the token's
//     log-probability goes to prefix_logp[b][t + 1];
//   * with t + 1 >= len_b commits its own pick (arg-max or the sampler's draw, exactly as step.h) into output column t + 1 - len_b.
// So column j of row b is always the j-th token behind row b's own prefix.  Everything is indexed by the row of the BATCH (out_row), like
// outputs and sampler keys: live-row compaction and row ranges move nothing of it.  The bookkeeping behind a committed token is step.h's
// (arrive_token): a forced eos finishes a row like a picked one.
//
// These are kernels of their own, behind every other kernel of the library: the plain steps (StepArgs::forced == null) run step.h's kernels
// as they were.  One wave per row, like them.
#pragma once
#include "step.h"

namespace txo {

// the token of row `row` at position t: forced (>= 0, in the vocabulary) or -1 where the row picks for itself; len = the row's prefix length
__device__ inline int forced_token(const StepArgs& a, int orow, int t, int& len) {
    len = a.forced_len[orow];
    return t + 1 < len ? in_vocab((int)a.forced[(size_t)orow * a.forced_stride + t + 1], a.V) : -1;
}
// commit_token with the prompted decode's output rule (lane 0 of a row)
__device__ inline void commit_prompted(const StepArgs& a, int row, int orow, int t, int tok, float logp, bool forced, int len) {
    tok = in_vocab(tok, a.V);
    a.cur_tok[row] = tok;
    // per-row stop: nothing more is written for a finished row -- a row whose prefix holds eos is finished from the start (prefix_start_kernel),
    // so none of its forced tokens is scored: its prefix_logp stays 0.0 (texocr.h)
    const bool frozen = a.stop_rows && a.eos >= 0 && a.eos_seen[row];
    if (forced) {
        if (a.prefix_logp && !frozen) a.prefix_logp[(size_t)orow * a.forced_stride + t + 1] = logp;
    } else {
        const int j = t + 1 - len;                                             // >= 0: the row is behind its prefix
        if (j < a.out_cols && !frozen) {
            if (a.tokens_out) a.tokens_out[(size_t)orow * a.out_stride + j] = tok;
            if (a.logp_out) a.logp_out[(size_t)orow * a.out_stride + j] = logp;
        }
    }
    arrive_token(a, row, t, tok);
}

// One pass over a logits row, argmax_step_kernel's loops (both branches: 16-byte requests when V % 4 == 0, scalar otherwise) with the same
// per-lane order of operations: the row's maximum and its index, the running log-sum-exp (lp), and the logit at index `want` (-3.4e38 in
// every lane but the one that streamed it; want < 0: none)
__device__ inline void stream_row(const float* lg, int V, int lane, bool lp, int want, float& best, int& bi, float& lm, float& ls, float& wv) {
    best = -3.4e38f; bi = 0x7fffffff; lm = -3.4e38f; ls = 0.f; wv = -3.4e38f;
    if ((V & 3) == 0) {
        const int n4 = V >> 2;
        for (int base = 0; base < n4; base += 256) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j4 = base + u * 64 + lane;
                v[u] = j4 < n4 ? reinterpret_cast<const float4*>(lg)[j4] : make_float4(-3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j4 = base + u * 64 + lane;
                if (j4 >= n4) continue;
                if (lp) lse_push4(lm, ls, v[u]);
                const int j = j4 * 4;
                if ((want >> 2) == j4) { const int c = want & 3; wv = c == 0 ? v[u].x : (c == 1 ? v[u].y : (c == 2 ? v[u].z : v[u].w)); }
                if (v[u].x > best) { best = v[u].x; bi = j; }
                if (v[u].y > best) { best = v[u].y; bi = j + 1; }
                if (v[u].z > best) { best = v[u].z; bi = j + 2; }
                if (v[u].w > best) { best = v[u].w; bi = j + 3; }
            }
        }
    } else {
        for (int j = lane; j < V; j += 64) {
            const float v = lg[j];
            if (lp) lse_push(lm, ls, v);
            if (j == want) wv = v;
            if (v > best) { best = v; bi = j; }
        }
    }
    wave_argmax(best, bi);
}
// log_softmax(row)[forced token] from what stream_row left: (lg[forced] - row max) - log sum exp(v - row max).  Where the forced token is the
// arg-max the first term is exactly 0 and the float is the one argmax_step_kernel writes, -lse_finish(...), bit for bit.
__device__ inline float forced_logp(float best, float lm, float ls, float wv) {
    return (wave_max(wv) - best) - lse_finish(lm, ls, best);
}

__global__ __launch_bounds__(64) void argmax_prefix_step_kernel(StepArgs a) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const int t = a.st->t;
    const int orow = out_row(a, row);
    int len;
    const int ftok = forced_token(a, orow, t, len);
    const bool forced = ftok >= 0;
    const bool lp = forced ? a.prefix_logp != nullptr : a.logp_out != nullptr;
    float best, lm, ls, wv; int bi;
    stream_row(a.logits + (size_t)row * a.V, a.V, lane, lp, ftok, best, bi, lm, ls, wv);
    float logp = 0.f;
    if (lp) logp = forced ? forced_logp(best, lm, ls, wv) : -lse_finish(lm, ls, best);
    if (lane == 0) commit_prompted(a, row, orow, t, forced ? ftok : bi, logp, forced, len);
}

// the sampler's step: a forced position consumes no draw (a draw is keyed by (seed; row of the batch, position), so the free positions' draws
// are what they would be anyway); REGS as sample_step_kernel
template <bool REGS>
__global__ __launch_bounds__(64) void sample_prefix_step_kernel(StepArgs a) {
    extern __shared__ float row_lds[];
    const int row = blockIdx.x, lane = threadIdx.x, V = a.V;
    const int t = a.st->t;
    const float* lg = a.logits + (size_t)row * V;
    const int orow = out_row(a, row);
    int len;
    const int ftok = forced_token(a, orow, t, len);
    if (ftok >= 0) {                                                           // (wave-uniform: one row per wave)
        float logp = 0.f;
        if (a.prefix_logp) {
            float best, lm, ls, wv; int bi;
            stream_row(lg, V, lane, true, ftok, best, bi, lm, ls, wv);
            logp = forced_logp(best, lm, ls, wv);
        }
        if (lane == 0) commit_prompted(a, row, orow, t, ftok, logp, true, len);
        return;
    }
    int pick; float logp = 0.f;
    const bool lp = a.logp_out != nullptr;
    if constexpr (REGS) pick = sample_row_regs([&](int j) { return lg[j]; }, [&](int j) { return ld16(lg + j); }, nullptr, V, lane, a.topk, a.inv_temp, a.seed,
                                               (unsigned)(a.row0 + orow), (unsigned)t, lp, logp);
    else pick = sample_row_lds([&](int j) { return lg[j]; }, row_lds, nullptr, V, lane, a.topk, a.inv_temp, a.seed, (unsigned)(a.row0 + orow), (unsigned)t,
                               lp, logp);
    if (lane == 0) commit_prompted(a, row, orow, t, pick, logp, false, len);
}
inline void launch_prefix_step(hipStream_t s, int rows, const StepArgs& sa, bool sample) {
    if (!sample) hipLaunchKernelGGL(argmax_prefix_step_kernel, dim3(rows), dim3(64), 0, s, sa);
    else if (sample_in_regs(sa.V)) hipLaunchKernelGGL(sample_prefix_step_kernel<true>, dim3(rows), dim3(64), 0, s, sa);
    else hipLaunchKernelGGL(sample_prefix_step_kernel<false>, dim3(rows), dim3(64), (size_t)sa.V * sizeof(float), s, sa);
}

// the caller's prefix [rows][P] into the engine's table [rows][stride]: columns 0 .. min(len_b, stride) - 1 with their ids forced into the
// vocabulary (copy_tokens_kernel's rule), 0 behind them -- columns at and behind len_b of the caller's row are never read
__global__ void prefix_table_kernel(int64_t* table, int stride, const int64_t* prefix, int P, const int* len, int rows, int V) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * stride) return;
    const int r = i / stride, c = i - r * stride;
    long long v = 0;
    if (c < len[r] && c < P) { v = prefix[(size_t)r * P + c]; v = v < 0 ? 0 : (v >= V ? V - 1 : v); }
    table[i] = v;
}

// (re)start a row range's decode in the middle of the table, beside reset_state_kernel: position m - 1, fed with the prefix's token there; a row
// counts as containing eos from the start if prefix[b][:len_b] holds one anywhere (decoder.py:115 tests the whole output), forced yet or not.
// *st was zeroed on the stream before the launch (rows_with_eos is counted here); table / len are the range's slices.
__global__ void prefix_start_kernel(StepState* st, int64_t* cur_tok, int* eos_seen, int* done_flag, int rows, int n_flags, int eos,
                                    const int64_t* table, int stride, const int* len, int m) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) {
        const int64_t* p = table + (size_t)i * stride;
        cur_tok[i] = p[m - 1];
        int seen = 0;
        if (eos >= 0) { const int n = len[i]; for (int c = 0; c < n; ++c) seen |= p[c] == eos ? 1 : 0; }
        eos_seen[i] = seen;
        if (seen) atomicAdd(&st->rows_with_eos, 1);
    }
    if (i < n_flags) done_flag[i] = 0;
    if (i == 0) st->t = m - 1;
}

// The end of a prompted decode, on the caller's rows: positions 0 .. steps-1 count as decoded (the loop may have run a few more before the host
// saw the eos break).  Row b reached output column steps - len_b: every column behind it up to n holds pad and 0.0, and so does every column
// behind the row's first eos under the per-row stop (row_stop; a prefix that holds eos finishes the row before column 0) -- pad_after_eos_kernel's
// rule with the prefix in place of the BOS column.  prefix_logp (the engine's [rows][stride]) goes to the caller's [rows][P]: 0.0 at columns
// the loop did not force (i < m, i >= len_b, i > steps) and, under the per-row stop, in every column of a row whose prefix holds eos.
__global__ void prefix_finish_kernel(int64_t* tokens, float* logp, int out_stride, int n, int rows, int steps, int eos, int pad, int row_stop,
                                     const int64_t* table, int stride, const int* len, int m, const float* plogp, float* plogp_out, int P) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int L = len[r];
    const int64_t* p = table + (size_t)r * stride;
    int64_t* row = tokens + (size_t)r * out_stride;
    float* lp = logp ? logp + (size_t)r * out_stride : nullptr;
    bool done = false;
    if (row_stop && eos >= 0) for (int c = 0; c < L; ++c) done = done || p[c] == eos;
    const bool unscored = done;                                   // per-row stop, the prefix holds eos: finished from the start, prefix_logp all 0.0
    const int reached = steps - L;                                // last column the row wrote (< 0: none)
    for (int j = 0; j < n; ++j) {
        if (done || j > reached) { row[j] = pad; if (lp) lp[j] = 0.f; }
        else if (row_stop && eos >= 0 && row[j] == eos) done = true;
    }
    if (plogp_out)
        for (int i = 0; i < P; ++i) plogp_out[(size_t)r * P + i] = (!unscored && i >= m && i < L && i <= steps && i < stride) ? plogp[(size_t)r * stride + i] : 0.f;
}

}  // namespace txo
