// Repeat guard inside the beam selection (texocr.h: txo_set_guard_beam): beam_rules.h's selection with step_guard.h's ban.
//
// Slot j of an image at position t has the history h[0 .. t-1] of the tokens its ancestry committed:
//   h[i]     = tok_hist[i][path_cur[j][i + 1]]   for i <= t - 2   (the slot that held position i + 1 is the slot that picked token i)
//   h[t - 1] = tok_hist[t - 1][j]
// and its ban set is step_guard.h's, from that history: for a period p <= min(P, t) whose trailing match count reaches R * p - 1, token
// h[t - p], unless it is eos.  For a LIVE, UNFINISHED parent j the candidate (j, v) is
//   score[j] + (logit[j][v] - lse[j])   iff v is allowed AND not banned for j,   -INFINITY otherwise
// "allowed": every token without rules (BeamRuleArgs::rules == null), rule_allows under rules, beam_select_close_kernel's budgeted predicate
// under a closing search (BeamCloseArgs::tab != null).  A parent with no token both allowed and unbanned drops its ban at this pick and the
// rules, or the budget, decide alone -- the pick kernels' yield rule; so the guard only ever shrinks a non-empty allowed set to a non-empty
// one and a closing search keeps its guarantee.  Everything else is beam_select_rules_kernel's: the log-sum-exp of the RAW row, a finished
// parent's eos at + 0, dead slots, tie order, back-pointers, path copies, the arrival word and the done flag.
//
// The bans of a parent go into a V-bit map in LDS (k maps), behind the k staged windows: every parent's last min(t, (R + 1) * P - 1) tokens,
// which is as far back as any scan looks.  Staging costs two dependent loads per token, spread over the workgroup; one thread per
// (parent, period) then scans its window in LDS.  Nothing is kept between picks.
//
// Kernels of their own, behind every other kernel of the library: without a guard -- or with the switch off -- a beam search runs the
// kernels it ran before.
#pragma once
#include "beam_rules.h"
#include "step_guard.h"

namespace txo {

struct BeamGuardArgs { int p, r; };                                // max_period, max_repeats (both 1 .. GUARD_MAX)

__host__ __device__ inline int beam_guard_window(int p, int r) { return (r + 1) * p - 1; }
// dynamic LDS of beam_select_guard_kernel: k windows, k maps
__host__ __device__ inline size_t beam_guard_lds_bytes(int k, int V, int p, int r) {
    return (size_t)k * ((size_t)beam_guard_window(p, r) * sizeof(int) + guard_map_bytes(V));
}
constexpr size_t BEAM_GUARD_LDS_MAX = 65536 - 8192;                // what the kernel's static LDS (the close table, the reductions) leaves of 64 KB

// One workgroup per image, 256 threads, like beam_select_kernel; LOGP as there.  ra.rules null: no rules (ra.state unused); ca.tab null: no budget.
template <bool LOGP>
__global__ __launch_bounds__(256) void beam_select_guard_kernel(BeamArgs a, BeamRuleArgs ra, BeamCloseArgs ca, BeamGuardArgs ga) {
    constexpr int KMAX = 8;
    extern __shared__ unsigned bguard_lds[];
    __shared__ float red[8], s_lse[KMAX], s_score[KMAX], selv[KMAX];
    __shared__ int redi[4], s_fin[KMAX], seli[KMAX];
    __shared__ int2 s_state[KMAX];
    __shared__ __attribute__((aligned(16))) unsigned short cl[CLOSE_NODES];
    __shared__ int s_lim[KMAX];
    __shared__ unsigned s_any;                                // bit j: parent j has a token that is both allowed and unbanned
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k, V = a.V, t = a.st->t;
    const float* lg = a.logits + (size_t)img * k * V;
    const bool ruled = ra.rules != nullptr;
    const int R = ca.positions - t;                           // (block-uniform) picks left, and whether the budget can bind at all
    const bool budget = ca.tab != nullptr && R - 1 < ca.tab->slack;
    if (budget) close_stage(cl, ca.tab, ra.n_states * (ra.depth_max + 1), tid, 256);
    // ---- the ban maps ----
    const int W = beam_guard_window(ga.p, ga.r), L = min(t, W), words = (V + 31) >> 5;
    int* win = reinterpret_cast<int*>(bguard_lds);            // [k][W]: parent j's h[t - L .. t - 1] in win[j * W .. j * W + L)
    unsigned* bm = bguard_lds + k * W;                        // [k][words]
    for (int q = tid; q < k * words; q += 256) bm[q] = 0u;
    if (tid == 0) s_any = 0u;
    for (int q = tid; q < k * L; q += 256) {
        const int j = q / L, o = q - j * L, i = t - L + o, own = img * k + j;
        int slot = own;
        if (i < t - 1) {
            slot = a.path_cur[(size_t)own * a.path_stride + i + 1];
            if ((unsigned)slot >= (unsigned)(a.images * k)) slot = own;          // (never: every slot's path is written at every step)
        }
        win[j * W + o] = a.tok_hist[(size_t)i * a.hist_stride + slot];
    }
    __syncthreads();
    if (tid < k * ga.p) {                                     // one thread per (parent, period): step_guard.h's guard_ban over the window
        const int j = tid / ga.p, p = tid - j * ga.p + 1;
        if (p <= t) {
            const int need = ga.r * p - 1;
            const int* w = win + j * W + L;                   // w[-1 - m] = h[t - 1 - m]
            int m = 0;
            while (m < need) {
                if (L - 1 - m - p < 0 || w[-1 - m] != w[-1 - m - p]) break;
                ++m;
            }
            if (m >= need) {
                const int tok = w[-p];
                if ((unsigned)tok < (unsigned)V && tok != a.eos) atomicOr(&bm[j * words + (tok >> 5)], 1u << (tok & 31));
            }
        }
    }
    __syncthreads();
    constexpr int VPT = 4;                                    // register path: vocabularies up to 256 * VPT entries
    if (V <= 256 * VPT) {
        // beam_select_rules_kernel's register path.  Two bits per candidate while the rows are read: `ok` (allowed) and `okb` (allowed and
        // unbanned); once the workgroup knows which parents keep a token under their ban, okb replaces ok for those
        __shared__ float rmx[KMAX][4], rse[KMAX][4], rbv[2][4];
        __shared__ int rbi[2][4];
        float x[KMAX][VPT], sc[KMAX]; int fn[KMAX]; int2 sd[KMAX];
        unsigned ok = 0u, okb = 0u;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            sc[j] = 0.f; fn[j] = 0; sd[j] = make_int2(0, 0);
            if (j < k) { sc[j] = a.score[img * k + j]; fn[j] = a.fin[img * k + j]; if (ruled) sd[j] = beam_rule_state(ra, img * k + j); }
            const int* rl = ra.rules + (size_t)sd[j].x * V;
            int lim = -1;
            if (budget && j < k && !fn[j]) lim = beam_close_lim(ca, ra, sd[j], R);
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int v = tid + 256 * i;
                const bool in = j < k && v < V;
                x[j][i] = in ? lg[(size_t)j * V + v] : 0.f;
                const int r = in ? (ruled ? rl[v] : 0) : RULE_BAN;
                bool al;
                if (lim >= 0) al = close_allows(cl, r, v, sd[j].y, ra.depth_max, a.eos, lim);
                else al = rule_allows(r, sd[j].y, ra.depth_max);
                const bool ub = al && !guard_bit(bm + (in ? j * words : 0), in ? v : 0);   // (no map behind the k-th)
                ok |= (al ? 1u : 0u) << (j * VPT + i);
                okb |= (ub ? 1u : 0u) << (j * VPT + i);
            }
        }
        {   // which parents keep a token: one OR over the workgroup, ready behind the two barriers of the log-sum-exp
            unsigned mine = 0u;
#pragma unroll
            for (int j = 0; j < KMAX; ++j) if (__ballot((okb >> (j * VPT)) & 0xfu) != 0ull) mine |= 1u << j;
            if (lane == 0) atomicOr(&s_any, mine);
        }
        float mx[KMAX], lse[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) if (j < k) {
            float m = -3.4e38f;
#pragma unroll
            for (int i = 0; i < VPT; ++i) if (tid + 256 * i < V) m = fmaxf(m, x[j][i]);
            m = wave_max(m);
            if (lane == 0) rmx[j][wave] = m;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KMAX; ++j) if (j < k) {
            mx[j] = fmaxf(fmaxf(rmx[j][0], rmx[j][1]), fmaxf(rmx[j][2], rmx[j][3]));
            float se = 0.f;
#pragma unroll
            for (int i = 0; i < VPT; ++i) if (tid + 256 * i < V) se += expf(x[j][i] - mx[j]);
            se = wave_sum(se);
            if (lane == 0) rse[j][wave] = se;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KMAX; ++j) if (j < k) lse[j] = mx[j] + logf((rse[j][0] + rse[j][1]) + (rse[j][2] + rse[j][3]));
        {   // the yield rule: a parent whose ban leaves nothing keeps its allowed bits
            const unsigned any = s_any;
            unsigned keep = 0u;
#pragma unroll
            for (int j = 0; j < KMAX; ++j) if ((any >> j) & 1u) keep |= 0xfu << (j * VPT);
            ok = (okb & keep) | (ok & ~keep);
        }
        // candidates in place of the logits: the raw row minus the raw log-sum-exp where allowed and unbanned
#pragma unroll
        for (int j = 0; j < KMAX; ++j) if (j < k) {
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int v = tid + 256 * i;
                if (fn[j]) x[j][i] = (v == a.eos) ? sc[j] : -INFINITY;
                else x[j][i] = ((ok >> (j * VPT + i)) & 1u) ? sc[j] + (x[j][i] - lse[j]) : -INFINITY;
            }
        }
        unsigned taken = 0u;                                  // bit j * VPT + i: this thread's candidate was selected in an earlier round
        float sv[KMAX]; int si[KMAX];
#pragma unroll
        for (int r = 0; r < KMAX; ++r) if (r < k) {
            float best = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < KMAX; ++j) if (j < k) {
#pragma unroll
                for (int i = 0; i < VPT; ++i) {
                    const int v = tid + 256 * i, f = j * V + v;
                    if (v >= V || ((taken >> (j * VPT + i)) & 1u)) continue;
                    const float c = x[j][i];
                    if (c > best || (c == best && f < bi)) { best = c; bi = f; }
                }
            }
            wave_argmax(best, bi);
            if (lane == 0) { rbv[r & 1][wave] = best; rbi[r & 1][wave] = bi; }
            __syncthreads();
            float b = rbv[r & 1][0]; int ix = rbi[r & 1][0];
#pragma unroll
            for (int w = 1; w < 4; ++w) { const float bw = rbv[r & 1][w]; const int iw = rbi[r & 1][w]; if (bw > b || (bw == b && iw < ix)) { b = bw; ix = iw; } }
            sv[r] = b; si[r] = ix;
            const int j = ix / V, v = ix - j * V;
            if ((v & 255) == tid) taken |= 1u << (j * VPT + (v >> 8));
        }
        // (every thread read the image's k states, and the windows, before the first selection barrier: the writes below are in place)
        int allfin = 1;
#pragma unroll
        for (int r = 0; r < KMAX; ++r) if (r < k) {
            const int sel = (unsigned)si[r] < (unsigned)(k * V) ? si[r] : 0;         // (nothing finite left, or non-finite logits: a dead slot, inside the image's candidates)
            const int j = sel / V, v = sel - j * V;
            int fj = 0; int2 sj = make_int2(0, 0);
#pragma unroll
            for (int q = 0; q < KMAX; ++q) if (q == j) { fj = fn[q]; sj = sd[q]; }
            const bool dead = !(sv[r] > -INFINITY);                                  // (a masked eos finishes nothing; a dead slot holds no search open)
            const int nf = fj | ((a.eos >= 0 && v == a.eos && !dead) ? 1 : 0);
            allfin &= nf | (dead ? 1 : 0);
            if (tid == r) {
                const int row = img * k + r;
                a.score[row] = sv[r]; a.fin[row] = nf; a.cur_tok[row] = v;
                a.tok_hist[(size_t)t * a.hist_stride + row] = v;
                a.parent_hist[(size_t)t * a.hist_stride + row] = (short)(a.row0 + img * k + j);
                if (ruled) ra.state[row] = beam_rule_next(ra, V, sj, v, fj);
                if constexpr (LOGP) {
                    float lj = 0.f;
#pragma unroll
                    for (int q = 0; q < KMAX; ++q) if (q == j) lj = lse[q];
                    a.logp_hist[(size_t)t * a.hist_stride + row] = fj ? 0.f : lg[(size_t)j * V + v] - lj;
                }
            }
            beam_copy_path(a, img, r, j, t, tid);
        }
        if (tid == 0) beam_arrive(a, t, allfin);
        return;
    }
    if (tid < k) {
        s_score[tid] = a.score[img * k + tid]; s_fin[tid] = a.fin[img * k + tid];
        s_state[tid] = ruled ? beam_rule_state(ra, img * k + tid) : make_int2(0, 0);
        s_lim[tid] = (budget && !s_fin[tid]) ? beam_close_lim(ca, ra, s_state[tid], R) : -1;
    }
    // log-sum-exp of every beam's RAW row
    for (int j = 0; j < k; ++j) {
        float mx = -3.4e38f;
        for (int v = tid; v < V; v += 256) mx = fmaxf(mx, lg[(size_t)j * V + v]);
        mx = wave_max(mx);
        if (lane == 0) red[wave] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        float se = 0.f;
        for (int v = tid; v < V; v += 256) se += expf(lg[(size_t)j * V + v] - mx);
        se = wave_sum(se);
        if (lane == 0) red[4 + wave] = se;
        __syncthreads();
        if (tid == 0) s_lse[j] = mx + logf((red[4] + red[5]) + (red[6] + red[7]));
        __syncthreads();
    }
    // allowed (j, v): the rules, or the budget, alone
    auto allowed = [&](int j, int v) -> bool {
        if (!ruled) return true;
        const int2 sj = s_state[j];
        const int r = ra.rules[(size_t)sj.x * V + v];
        if (s_lim[j] >= 0) return close_allows(cl, r, v, sj.y, ra.depth_max, a.eos, s_lim[j]);
        return rule_allows(r, sj.y, ra.depth_max);
    };
    const int total = k * V;
    // which parents keep a token under their ban.  Without rules every one does: a ban set has at most P tokens and the vocabulary more than P + 1
    if (ruled) {
        unsigned mine = 0u;
        for (int f = tid; f < total; f += 256) {
            const int j = f / V, v = f - j * V;
            if (!((mine >> j) & 1u) && allowed(j, v) && !guard_bit(bm + j * words, v)) mine |= 1u << j;
        }
        unsigned wave_any = 0u;                               // (the lane that found a parent's token need not be lane 0)
        for (int j = 0; j < k; ++j) if (__ballot((mine >> j) & 1u) != 0ull) wave_any |= 1u << j;
        if (lane == 0) atomicOr(&s_any, wave_any);
    } else if (tid == 0) s_any = 0xffu;
    __syncthreads();
    const unsigned any = s_any;
    // k rounds of block-wide arg max over the k*V candidates, excluding what was already taken; the mask inside the candidate loop
    for (int r = 0; r < k; ++r) {
        float best = -INFINITY; int bi = 0x7fffffff;
        for (int f = tid; f < total; f += 256) {
            bool taken = false;
            for (int q = 0; q < r; ++q) taken |= seli[q] == f;
            if (taken) continue;
            const int j = f / V, v = f - j * V;
            float c;
            if (s_fin[j]) c = (v == a.eos) ? s_score[j] : -INFINITY;
            else {
                const bool al = allowed(j, v) && !(((any >> j) & 1u) && guard_bit(bm + j * words, v));
                c = al ? s_score[j] + (lg[f] - s_lse[j]) : -INFINITY;
            }
            if (c > best || (c == best && f < bi)) { best = c; bi = f; }
        }
        wave_argmax(best, bi);
        if (lane == 0) { red[wave] = best; redi[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            float b = red[0]; int i = redi[0];
            for (int w = 1; w < 4; ++w) if (red[w] > b || (red[w] == b && redi[w] < i)) { b = red[w]; i = redi[w]; }
            selv[r] = b; seli[r] = i;
        }
        __syncthreads();
    }
    // new beams: slot r of this image continues beam seli[r] / V with token seli[r] % V (states and windows were read into LDS before the barriers above)
    int allfin = 1;
    for (int r = 0; r < k; ++r) {
        const int sel = (unsigned)seli[r] < (unsigned)(k * V) ? seli[r] : 0;         // (a dead slot: see above)
        const int j = sel / V, v = sel - j * V;
        const bool dead = !(selv[r] > -INFINITY);                                // (as on the register path)
        const int nf = s_fin[j] | ((a.eos >= 0 && v == a.eos && !dead) ? 1 : 0);
        allfin &= nf | (dead ? 1 : 0);
        if (tid == r) {
            const int row = img * k + r;
            a.score[row] = selv[r]; a.fin[row] = nf; a.cur_tok[row] = v;
            a.tok_hist[(size_t)t * a.hist_stride + row] = v;
            a.parent_hist[(size_t)t * a.hist_stride + row] = (short)(a.row0 + img * k + j);
            if (ruled) ra.state[row] = beam_rule_next(ra, V, s_state[j], v, s_fin[j]);
            if constexpr (LOGP) a.logp_hist[(size_t)t * a.hist_stride + row] = s_fin[j] ? 0.f : lg[sel] - s_lse[j];
        }
        beam_copy_path(a, img, r, j, t, tid);
    }
    if (tid == 0) beam_arrive(a, t, allfin);
}

// The one launch of a selection step, whatever its form (here: the first place where every form's kernel is declared): one workgroup per
// image of the range; a form reads the arguments its kernel takes and no others.
enum class BeamForm { plain, rules, close, guard };
inline void launch_beam_select(hipStream_t s, const BeamArgs& ba, const BeamRuleArgs& ra, const BeamCloseArgs& ca, const BeamGuardArgs& ga, BeamForm form, bool logp) {
    const dim3 grid(ba.images), block(256);
    switch (form) {
    case BeamForm::plain:
        if (logp) hipLaunchKernelGGL(beam_select_kernel<true>, grid, block, 0, s, ba);
        else hipLaunchKernelGGL(beam_select_kernel<false>, grid, block, 0, s, ba);
        break;
    case BeamForm::rules:
        if (logp) hipLaunchKernelGGL(beam_select_rules_kernel<true>, grid, block, 0, s, ba, ra);
        else hipLaunchKernelGGL(beam_select_rules_kernel<false>, grid, block, 0, s, ba, ra);
        break;
    case BeamForm::close:
        if (logp) hipLaunchKernelGGL(beam_select_close_kernel<true>, grid, block, 0, s, ba, ra, ca);
        else hipLaunchKernelGGL(beam_select_close_kernel<false>, grid, block, 0, s, ba, ra, ca);
        break;
    case BeamForm::guard: {
        const size_t lds = beam_guard_lds_bytes(ba.k, ba.V, ga.p, ga.r);
        if (logp) hipLaunchKernelGGL(beam_select_guard_kernel<true>, grid, block, lds, s, ba, ra, ca, ga);
        else hipLaunchKernelGGL(beam_select_guard_kernel<false>, grid, block, lds, s, ba, ra, ca, ga);
        break;
    }
    }
}

}  // namespace txo
