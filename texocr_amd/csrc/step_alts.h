// Alternatives per token (texocr.h: txo_set_alternatives): the k best ids of every logits row a pick is made from, and their log-probabilities.
//
// For the f32 row x[0 .. V-1] the selection reads and 1 <= k <= ALTS_MAX:
//   ids[0 .. k-1]  the indices of the k largest entries in descending value, LOWER INDEX FIRST among equals (a stable descending sort), so
//                  ids[0] is argmax_step_kernel's pick;
//   logp[j]        x[ids[j]] - logsumexp(x): natural log, temperature 1, the whole vocabulary -- StepArgs::logp_out's quantity.
// Always the RAW row: not the sampler's top-k / temperature distribution, not masked by token rules, the closing budget or the repeat guard.
// Under such a decode the committed token may be missing from its own alternatives: that is how a caller sees that a rule forced it.
//
// ONE kernel of its own, launched between the logits GEMM and whatever pick kernel follows, on the same stream: it reads the position, the
// rows' eos state, row_map and the prefix lengths as the pick is about to see them and changes none of them, so it serves every form of the
// launch path -- greedy, both sampler forms, prompted, rules, closing, guard; eager and captured steps, row ranges, the per-row stop with
// compaction, ragged sessions -- and no pick kernel has a variant for it.  It takes no part in the arrival word.
//
// One wave per row, the row streamed EXACTLY as argmax_step_kernel streams it (the float4 sweeps of 256 when V % 4 == 0, the scalar loop
// otherwise, lse_push4 / lse_push in the same order): in a greedy decode logp[0] is bit for bit the logp the pick writes.  Every lane keeps the
// ALTS_MAX best (value, index) of what it streams, sorted, in registers (kbest.h); k rounds of wave_argmax over the lanes' heads then pop the row's best.
#pragma once
#include "kbest.h"
#include "step.h"

namespace txo {

constexpr int ALTS_MAX = KBEST_MAX;

struct AltsArgs {
    int32_t* ids; float* logp;            // the range's slices of [rows][cols][k], indexed by row of the BATCH (out_row) like the pick's outputs
    int k, cols;                          // cols: columns of a row of both (the engine's Tmax)
};

__global__ __launch_bounds__(64) void alts_step_kernel(StepArgs a, AltsArgs o) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const int t = a.st->t;
    const int orow = out_row(a, row);
    // the pick's own output rule (commit_token / commit_prompted): nothing for a frozen row, a forced position, a column beyond the outputs
    if (a.stop_rows && a.eos >= 0 && a.eos_seen[row]) return;
    int col = t;
    if (a.forced) {
        const int len = a.forced_len[orow];
        if (t + 1 < len) return;
        col = t + 1 - len;
        if (col >= a.out_cols) return;
    }
    if (col >= o.cols) return;
    const float* lg = a.logits + (size_t)row * a.V;
    KBest q; q.clear(-3.4e38f);
    float lm = -3.4e38f, ls = 0.f;
    if ((a.V & 3) == 0) {
        const int n4 = a.V >> 2;
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
                lse_push4(lm, ls, v[u]);
                const int j = j4 * 4;
                q.push(v[u].x, j); q.push(v[u].y, j + 1); q.push(v[u].z, j + 2); q.push(v[u].w, j + 3);
            }
        }
    } else {
        for (int j = lane; j < a.V; j += 64) {
            const float v = lg[j];
            lse_push(lm, ls, v);
            q.push(v, j);
        }
    }
    int32_t* ids = o.ids + ((size_t)orow * o.cols + col) * o.k;
    float* lp = o.logp + ((size_t)orow * o.cols + col) * o.k;
    float top = 0.f, lse = 0.f;
    for (int r = 0; r < o.k; ++r) {
        float best = q.val[0]; int bi = q.idx[0];
        wave_argmax(best, bi);                                                 // ties -> lowest index
        if (r == 0) { top = best; lse = lse_finish(lm, ls, best); }
        if (bi == q.idx[0] && bi != 0x7fffffff) q.pop(-3.4e38f);                       // (one lane holds index bi)
        if (lane == 0) { ids[r] = in_vocab(bi, a.V); lp[r] = r == 0 ? -lse : (best - top) - lse; }
    }
}

// every entry of [rows][cols][k] to pad / 0.0: what a column holds that no step writes
__global__ void alts_fill_kernel(int32_t* ids, float* logp, size_t n, int pad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { ids[i] = pad; logp[i] = 0.f; }
}

// The end of an alternatives decode: pad / 0.0 wherever the call's tokens and logp hold pad / 0.0 (the loop may have run a few positions ahead
// of the break, and without compaction a finished row goes on writing).  tokens: the caller's rows [rows][out_stride], n returned columns.
//   from BOS, per-row stop (row_stop):  behind a row's first eos -- pad_after_eos_kernel's rule (the BOS column counts);
//   prompted (len != null):  behind column steps - len_b, and under the per-row stop behind the row's first eos, the prefix counting --
//                            prefix_finish_kernel's rule.
__global__ void alts_finish_kernel(int32_t* ids, float* logp, int k, int cols, const int64_t* tokens, int out_stride, int n, int rows, int steps,
                                   int eos, int bos, int pad, int row_stop, const int64_t* table, int stride, const int* len) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const bool stop = row_stop && eos >= 0;
    bool done = false; int reached = n;
    if (len) {
        const int L = len[r];
        if (stop) for (int c = 0; c < L; ++c) done = done || table[(size_t)r * stride + c] == eos;
        reached = steps - L;
    } else done = stop && bos == eos;
    const int64_t* row = tokens + (size_t)r * out_stride;
    for (int j = 0; j < n && j < cols; ++j) {
        if (done || j > reached) {
            for (int q = 0; q < k; ++q) { ids[((size_t)r * cols + j) * k + q] = pad; logp[((size_t)r * cols + j) * k + q] = 0.f; }
        } else if (stop && row[j] == eos) done = true;
    }
}

}  // namespace txo
