// Teacher-forced scoring: logits -> log-softmax -> target gather in ONE kernel, without a logits array.
//
// AutoRegressiveDecoder.forward (reference model/decoder.py:124-145) feeds trg[:, :-1] through the decoder and takes the cross
// entropy of the logits against trg[:, 1:].  Per row m = (image, position) of the final-LayerNorm output z [M][D] this kernel gives
//   logp      = logit[target] - logsumexp(logits)        (log_softmax(logits)[target])
//   top1      = argmax(logits), lowest index among equals (torch.argmax; the rule of step.h)
//   top1_logp = logit[top1] - logsumexp(logits)
// with logits = z wlog^T + blog formed tile by tile in registers and never stored: the attention kernels' online softmax with
// the vocabulary in the role of the keys.  The products are those of the logits GEMM (the same T operands on the same MFMA:
// v_mfma_f32_16x16x32_bf16 / exact-f32 16x16x4, f32 accumulation); only the order of the f32 sums differs.
//
// Shape: a wave owns 16 rows.  Their z rows sit in the wave's own LDS slice (16 x D of T, 16-byte pieces XOR-swizzled with the
// row: a fragment read is bank-conflict free); the wave walks wlog [V][D] in tiles of 64 vocabulary entries, W fragments straight
// from global memory (wlog is 0.5-1.5 MB: L2 resident).  S^T = W z^T, so a lane holds 4 x 4 logits of ONE row (column lane & 15)
// per tile and keeps that row's running max / sum of exp / arg-max / target logit in registers; the 4 lane groups that share a
// row are combined once at the end in a fixed order (no atomics: results are bit-reproducible), and lane group 0 writes.
// A workgroup is 1-4 such waves (as many as fit 64 KB of LDS: 4 up to width 256 in f32 / 512 in bf16, 1 at width 768 in f32).
// Any vocabulary size: rows of a tile beyond V are read from row V-1 (never out of bounds) and masked before the softmax.
// A target id outside [0, V) is clamped into the table exactly as embed_rows_kernel clamps the ids it feeds: the score returned
// is the clamped id's (the Python facade raises IndexError before it gets here).
// Bound: the W fragment stream from L2 (every wave reads all of wlog once per 16 rows), then MFMA.  Measured against the logits
// GEMM + torch.log_softmax + gather it replaces (probes/score_bench.py): 2-10 % slower per call, 1.9 MB instead of 500 MB of
// peak memory at 256 x 256 rows.  A wlog tile shared through LDS by the workgroup's waves would cut the stream fourfold.
#pragma once
#include "common.h"
#include "kbest.h"

namespace txo {

constexpr int SC_ROWS = 16;          // rows per wave
constexpr int SC_VT = 4;             // 16-entry vocabulary tiles per step
constexpr float SC_MASKED = -1e30f;  // a logit that does not exist (tail of the last tile)

template <typename T> inline int score_waves(int D) {
    const size_t per = (size_t)SC_ROWS * D * sizeof(T);
    return (int)std::max<size_t>(1, std::min<size_t>(4, 65536 / per));
}

// z [M][D]; W [V][D]; tokens [images][tok_stride], row m = (b, p) with b = m / t: its target is tokens[b][p + 1].
// Outputs are indexed by m; each may be null.
// ALTS (the k-best form, score_rows_alts_kernel below): every lane also keeps the KBEST_MAX best of the logits it owns (kbest.h; it meets them
// in increasing index), and the 4 lane groups of a row are merged in k rounds of the top-1 merge's own exchange -- the same order, the same
// tie rule, no atomics -- so alt_ids[..][0] is top1 and alt_logp[..][0] the float top1_logp holds; alt_logp[j] = logit - lse like it.
// alt_ids / alt_logp [M][k].  The <false> form reads none of the three and is the kernel as it was (profiles/alts_resource_usage.txt).
template <typename T, bool ALTS>
__device__ __forceinline__ void score_rows_body(const T* __restrict__ z, const T* __restrict__ W, const float* __restrict__ bias,
                                                const int64_t* __restrict__ tokens, int tok_stride, int t, int M, int D, int V,
                                                float* __restrict__ logp, int64_t* __restrict__ top1, float* __restrict__ top1_logp,
                                                int k, int32_t* __restrict__ alt_ids, float* __restrict__ alt_logp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sc_lds[];
    constexpr int PER16 = Elem<T>::PER16, KCHUNK = Elem<T>::KCHUNK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, lg = lane >> 4;
    const int r0 = (blockIdx.x * (blockDim.x >> 6) + wave) * SC_ROWS;
    const int P = D / PER16;                                  // 16-byte pieces per row (a multiple of 8: D is a multiple of 64)
    const int rowbytes = D * (int)sizeof(T);
    unsigned char* zs = sc_lds + (size_t)wave * SC_ROWS * rowbytes;
    if (r0 < M) {                                             // (wave-uniform; a wave beyond the rows only meets the barrier)
        for (int idx = lane; idx < SC_ROWS * P; idx += 64) {
            const int row = idx / P, piece = idx - row * P;
            const int m = min(r0 + row, M - 1);
            st16(zs + row * rowbytes + ((piece ^ (row & 7)) << 4), ld16(z + (size_t)m * D + piece * PER16));
        }
    }
    __syncthreads();
    if (r0 >= M) return;

    const int m_row = min(r0 + lc, M - 1);
    int tgt;
    {
        const int b = m_row / t, p = m_row - b * t;
        long long id = tokens[(size_t)b * tok_stride + p + 1];
        id = id < 0 ? 0 : (id >= V ? V - 1 : id);             // embed_rows_kernel's clamp, on the target side
        tgt = (int)id;
    }
    float m_run = SC_MASKED, l_run = 0.f, best = SC_MASKED, tl = 0.f;
    int bi = 0;
    KBest kb;
    if constexpr (ALTS) kb.clear(SC_MASKED);
    const int KC = D / KCHUNK;
    const unsigned char* zrow = zs + lc * rowbytes;
    for (int v0 = 0; v0 < V; v0 += 16 * SC_VT) {
        const T* wr[SC_VT];
#pragma unroll
        for (int j = 0; j < SC_VT; ++j) wr[j] = W + (size_t)min(v0 + j * 16 + lc, V - 1) * D + lg * PER16;
        f32x4 acc[SC_VT];
#pragma unroll
        for (int j = 0; j < SC_VT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kc = 0; kc < KC; ++kc) {
            const u32x4 zf = ld16(zrow + ((((kc << 2) + lg) ^ (lc & 7)) << 4));
            u32x4 wf[SC_VT];
#pragma unroll
            for (int j = 0; j < SC_VT; ++j) wf[j] = ld16(wr[j] + kc * KCHUNK);
#pragma unroll
            for (int j = 0; j < SC_VT; ++j) mma16<T>(acc[j], wf[j], zf);
        }
        // acc[j][r] = logit of entry v0 + 16 j + 4 lg + r for row lc (without the bias)
        float mx = SC_MASKED;
#pragma unroll
        for (int j = 0; j < SC_VT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int v = v0 + j * 16 + lg * 4 + r;
                float x = SC_MASKED;
                if (v < V) {
                    x = acc[j][r] + bias[v];
                    if (x > best) { best = x; bi = v; }       // entries in increasing order: the first of equals stays
                    if (v == tgt) tl = x;
                    if constexpr (ALTS) kb.push(x, v);
                }
                acc[j][r] = x;
                mx = fmaxf(mx, x);
            }
        const float m_new = fmaxf(m_run, mx);
        float ps = 0.f;
#pragma unroll
        for (int j = 0; j < SC_VT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) ps += acc[j][r] <= SC_MASKED ? 0.f : expf(acc[j][r] - m_new);
        l_run = l_run * expf(m_run - m_new) + ps;             // (both still SC_MASKED: 0 * exp(0) + 0)
        m_run = m_new;
    }
    // the 4 lane groups of a row (lanes l, l ^ 16, l ^ 32, l ^ 48), fixed order
    const float m_all = grp4_max(m_run);
    const float l_all = grp4_sum(l_run * expf(m_run - m_all));
    const float tl_all = grp4_sum(tl);                        // one group holds the target's logit, the others 0
    {
        auto take = [&](float ov, int oi) { if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; } };
        const float o16 = xor16(best); const int i16 = xor16(bi);
        take(o16, i16);
        const float o32 = xor32(best); const int i32 = xor32(bi);
        take(o32, i32);
    }
    if (lg == 0 && r0 + lc < M) {
        const float lse = m_all + logf(l_all);
        const size_t m = (size_t)(r0 + lc);
        if (logp) logp[m] = tl_all - lse;
        if (top1) top1[m] = bi;
        if (top1_logp) top1_logp[m] = best - lse;
    }
    if constexpr (ALTS) {
        const float lse = m_all + logf(l_all);
        for (int r = 0; r < k; ++r) {
            float b = kb.val[0]; int i = kb.idx[0];
            auto take = [&](float ov, int oi) { if (ov > b || (ov == b && oi < i)) { b = ov; i = oi; } };
            const float o16 = xor16(b); const int i16 = xor16(i);
            take(o16, i16);
            const float o32 = xor32(b); const int i32 = xor32(i);
            take(o32, i32);
            if (i == kb.idx[0] && i != 0x7fffffff) kb.pop(SC_MASKED);         // (one lane of the four holds entry i)
            if (lg == 0 && r0 + lc < M) {
                const size_t o = (size_t)(r0 + lc) * k + r;
                alt_ids[o] = (unsigned)i < (unsigned)V ? i : 0;               // (a non-finite row: unspecified, inside the vocabulary)
                alt_logp[o] = b - lse;
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void score_rows_kernel(const T* __restrict__ z, const T* __restrict__ W, const float* __restrict__ bias,
                                                         const int64_t* __restrict__ tokens, int tok_stride, int t, int M, int D, int V,
                                                         float* __restrict__ logp, int64_t* __restrict__ top1, float* __restrict__ top1_logp) {
    score_rows_body<T, false>(z, W, bias, tokens, tok_stride, t, M, D, V, logp, top1, top1_logp, 0, nullptr, nullptr);
}
template <typename T>
__global__ __launch_bounds__(256) void score_rows_alts_kernel(const T* __restrict__ z, const T* __restrict__ W, const float* __restrict__ bias,
                                                              const int64_t* __restrict__ tokens, int tok_stride, int t, int M, int D, int V,
                                                              float* __restrict__ logp, int64_t* __restrict__ top1, float* __restrict__ top1_logp,
                                                              int k, int32_t* __restrict__ alt_ids, float* __restrict__ alt_logp) {
    score_rows_body<T, true>(z, W, bias, tokens, tok_stride, t, M, D, V, logp, top1, top1_logp, k, alt_ids, alt_logp);
}

// kmask [rows][tmax] from a caller's mask [rows][stride] of which the first `cols` columns are positions (txo_score: stride L,
// cols L - 1); positions >= cols are not padding
__global__ void set_key_mask_strided_kernel(const unsigned char* __restrict__ mask, unsigned char* __restrict__ kmask, int rows, int stride,
                                            int cols, int tmax) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * tmax) return;
    const int r = i / tmax, j = i - r * tmax;
    kmask[i] = j < cols ? (mask[(size_t)r * stride + j] != 0 ? 1 : 0) : 1;
}

}  // namespace txo
