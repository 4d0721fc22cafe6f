// Attention PROBABILITIES of the multi-position decoder forward (prefill.h): what the reference returns as `post_softmax_attn`
// (model/attention.py:166-178) when Transformer.forward is called with return_attn=True (model/decoder.py:41-67).  attn_mq_kernel is a
// flash attention and never holds them; this kernel recomputes them from the same Q / K layouts under the same score rules:
//   Q scaled by ATTN_SCALE, S^T = K Q^T on the exact-f32 MFMA (TI widened on its way into LDS), CAUSAL: key j takes part for query i
//   iff j <= i + (nk - nq), KMASK: a padded key is never seen by a query that is not padding (a padded query's row ignores the mask and
//   stays finite), a masked entry is exactly 0.f (the `sc <= -1e30f ? 0 : expf(...)` rule, rows clamped beyond nq included).
// Two sweeps over the 64-key stages, K only (no V, no O accumulators):
//   sweep 1: per query the running (max, sum of exp), kept per (head, query) in LDS as (max, 1 / sum);
//   sweep 2: S again, p = exp(S - max) * (1 / sum), written stage by stage.  Nothing of size nq x nk is ever held.
// MEAN = false: grid (query block, image * head), P [image][head][nq][nk].
// MEAN = true:  grid (query block, image); the block walks the heads in index order: sweep 1 once per head, then per key stage the
//   sum over the heads of p / heads in registers, written once: M [image][nq][nk].  Fixed order, no atomics: the same bits every run,
//   and the per-head tensor need not exist.  The statistics take heads * 128 * 8 bytes of dynamic LDS (attn_probs_lds_bytes).
// Output rows are nk floats apart (589, 631, 7, ...: row starts are not 16-byte aligned), so a wave passes its 16 x 64 tile through its
// own LDS tile and every store instruction writes 64 consecutive floats of one row with 4-byte stores.
// Bound: MFMA f32 for the two QK^T sweeps; not a benchmark path (no generate() call reaches it).
#pragma once
#include "prefill.h"

namespace txo {

constexpr size_t attn_probs_lds_bytes(int heads_walked) { return (size_t)heads_walked * EA_QBLK * 2 * sizeof(float); }

// RAGGED (cross maps of a ragged batch session, never causal): image b has nk = lens[b] keys in K panels kv_rows apart, as in
//   attn_mq_kernel<.., RAGGED>; the output rows stay nk_arg (= the slot stride Ns) floats apart and columns lens[b] .. nk_arg-1 of every row
//   are written as exactly 0.f (the caller's buffer may be uninitialised): inside the image's last stage by the masked-score rule, behind it
//   by plain stores -- those stages are not walked.  RAGGED = false is the kernel without the parameter.
template <typename TI, bool CAUSAL, bool KMASK, bool MEAN, bool RAGGED = false>
__global__ __launch_bounds__(256) void attn_probs_kernel(const TI* __restrict__ Q, const TI* __restrict__ Kg, float* __restrict__ P, int nq, int nk_arg,
                                                         int kv_rows, int heads, const unsigned char* __restrict__ kmask = nullptr,
                                                         int kmask_stride = 0, const int* __restrict__ lens = nullptr) {
    static_assert(!(RAGGED && (CAUSAL || KMASK)), "per-image key counts exist for the cross attention only");
    __shared__ __attribute__((aligned(16))) unsigned char Ks[EA_KSTAGE * 256];   // one 64-key stage, f32 rows
    __shared__ __attribute__((aligned(16))) float tiles[4][16 * 64];             // per wave: 16 queries x 64 keys on their way out
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    float2* stats = reinterpret_cast<float2*>(dyn_lds);                          // [head walked][query of the block] = (max, 1 / sum)
    const int b = MEAN ? blockIdx.y : blockIdx.y / heads;
    const int h0 = MEAN ? 0 : blockIdx.y - b * heads, nh = MEAN ? heads : 1;
    const int nk = RAGGED ? lens[b] : nk_arg;                 // keys that take part
    const int prow = RAGGED ? nk_arg : nk;                    // floats between two output rows
    const int q0 = blockIdx.x * EA_QBLK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, lg = lane >> 4;
    const int off = nk - nq;

    [[maybe_unused]] bool q_valid[2] = {true, true};          // KMASK: this lane's query is not padding (query i sits at position i + off)
    if constexpr (KMASK) {
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
            q_valid[qt] = kmask[(size_t)b * kmask_stride + min(q0 + wave * 32 + qt * 16 + lc, nq - 1) + off] != 0;
    }

    u32x4 qf[2][4];
    auto load_q = [&](int head) {
        const TI* Qb = Q + ((size_t)b * heads + head) * nq * DH;
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const int qrow = min(q0 + wave * 32 + qt * 16 + lc, nq - 1);
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                float4 tq = __builtin_bit_cast(float4, ld4_f32<TI>(Qb + (size_t)qrow * DH + kc * 16 + lg * 4));
                tq.x *= ATTN_SCALE; tq.y *= ATTN_SCALE; tq.z *= ATTN_SCALE; tq.w *= ATTN_SCALE;   // exact (power of two)
                qf[qt][kc] = __builtin_bit_cast(u32x4, tq);
            }
        }
    };
    // stage s of one head's K rows into LDS (loads behind nk - 1 clamp); the barrier in front waits for the readers of the stage before
    auto stage_in = [&](int head, int s) {
        const TI* Kb = Kg + ((size_t)b * heads + head) * kv_rows * DH;
        u32x4 rk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, row = idx >> 4, piece = idx & 15;
            rk[i] = ld4_f32<TI>(Kb + (size_t)min(s * EA_KSTAGE + row, nk - 1) * DH + piece * 4);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, row = idx >> 4, piece = idx & 15;
            st16(&Ks[swz256(row, piece)], rk[i]);
        }
        __syncthreads();
    };
    // the masked scores of stage s: sc[qt][kt][r] = key s * 64 + kt * 16 + lg * 4 + r against query q0 + wave * 32 + qt * 16 + lc
    auto scores = [&](int s, f32x4 (&sc)[2][4]) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            u32x4 kf[4];
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) kf[kc] = ld16(Ks + swz256(kt * 16 + lc, kc * 4 + lg));
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kc = 0; kc < 4; ++kc) mma16<float>(a, kf[kc], qf[qt][kc]);
                sc[qt][kt] = a;
            }
        }
        const int kbase = s * EA_KSTAGE;
        if constexpr (KMASK) {                                // padded keys, for the queries that are not padding themselves
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const int k0 = kbase + kt * 16 + lg * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r) {                 // byte reads: a row of the mask need not be a multiple of 4 long
                    const bool pad = k0 + r < nk && kmask[(size_t)b * kmask_stride + k0 + r] == 0;
#pragma unroll
                    for (int qt = 0; qt < 2; ++qt) if (pad && q_valid[qt]) sc[qt][kt][r] = -1e30f;
                }
            }
        }
        if (CAUSAL || kbase + EA_KSTAGE > nk) {               // keys past nk and, causal, keys after the query
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                const int lim = CAUSAL ? min(nk - 1, q0 + wave * 32 + qt * 16 + lc + off) : nk - 1;   // last key this lane's query may see
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kbase + kt * 16 + lg * 4 + r > lim) sc[qt][kt][r] = -1e30f;
            }
        }
    };

    // ---- sweep 1: (max, 1 / sum of exp) per (head, query).  Causal: no key beyond the block's last query takes part (block-uniform).
    const int last_key = CAUSAL ? min(nk - 1, min(q0 + EA_QBLK - 1, nq - 1) + off) : nk - 1;
    const int nstage1 = last_key / EA_KSTAGE + 1, nstage = (nk - 1) / EA_KSTAGE + 1;
    for (int hh = 0; hh < nh; ++hh) {
        load_q(h0 + hh);
        float m_run[2] = {-1e30f, -1e30f}, l_run[2] = {0.f, 0.f};
        for (int s = 0; s < nstage1; ++s) {
            stage_in(h0 + hh, s);
            f32x4 sc[2][4];
            scores(s, sc);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                float mx = sc[qt][0][0];
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sc[qt][kt][r]);
                mx = grp4_max(mx);
                const float m_new = fmaxf(m_run[qt], mx);
                const float alpha = expf(m_run[qt] - m_new);
                m_run[qt] = m_new;
                float ps = 0.f;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ps += sc[qt][kt][r] <= -1e30f ? 0.f : expf(sc[qt][kt][r] - m_new);
                l_run[qt] = l_run[qt] * alpha + ps;
            }
        }
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            const float inv = 1.0f / grp4_sum(l_run[qt]);     // (every query sees at least its own key / key 0: the sum is >= 1)
            if (lg == 0) stats[hh * EA_QBLK + wave * 32 + qt * 16 + lc] = make_float2(m_run[qt], inv);
        }
    }

    // ---- sweep 2: S again, p = exp(S - max) / sum; per key stage the heads in index order, then one write of the stage's tile.
    // (the statistics are read behind the barriers of stage_in; every stage of the row is written: the ones sweep 1 skipped hold zeros)
    float* tile = tiles[wave];
    float* Pb = P + (MEAN ? (size_t)b : (size_t)b * heads + h0) * nq * prow;
    [[maybe_unused]] const float fheads = (float)heads;
    for (int s = 0; s < nstage; ++s) {
        f32x4 acc[2][4];
        for (int hh = 0; hh < nh; ++hh) {
            if constexpr (MEAN) load_q(h0 + hh);              // (one head: its queries are still in registers)
            stage_in(h0 + hh, s);
            f32x4 sc[2][4];
            scores(s, sc);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                const float2 st = stats[hh * EA_QBLK + wave * 32 + qt * 16 + lc];
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = sc[qt][kt][r] <= -1e30f ? 0.f : expf(sc[qt][kt][r] - st.x) * st.y;
                        if constexpr (MEAN) acc[qt][kt][r] = hh == 0 ? p / fheads : acc[qt][kt][r] + p / fheads;
                        else acc[qt][kt][r] = p;
                    }
            }
        }
        const int key = s * EA_KSTAGE + lane;
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)                    // (the swizzle moves whole groups of 4 floats: one 16-byte LDS write)
                *reinterpret_cast<f32x4*>(&tile[lc * 64 + ((kt * 16 + lg * 4) ^ ((lc & 7) << 2))]) = acc[qt][kt];
            // the tile is wave-private: no workgroup barrier, but the order of its writes and reads is stated for compiler and hardware
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int qq = 0; qq < 16; ++qq) {
                const int qrow = q0 + wave * 32 + qt * 16 + qq;
                const float v = tile[qq * 64 + (lane ^ ((qq & 7) << 2))];
                // (RAGGED: the stage's columns behind nk are written too; their scores were masked, so v is exactly 0.f there)
                if (qrow < nq && key < prow) Pb[(size_t)qrow * prow + key] = v;   // queries >= nq store nothing
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the tile has been read before the next 16 queries overwrite it
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    if constexpr (RAGGED) {                                   // the stages behind the image's last: zeros, without walking them
        for (int s = nstage; s * EA_KSTAGE < prow; ++s) {
            const int key = s * EA_KSTAGE + lane;
            for (int qq = 0; qq < 32; ++qq) {
                const int qrow = q0 + wave * 32 + qq;
                if (qrow < nq && key < prow) Pb[(size_t)qrow * prow + key] = 0.f;
            }
        }
    }
}

}  // namespace txo
