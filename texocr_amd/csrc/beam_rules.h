// Constrained beam search (texocr.h: txo_set_rules_beam): step.h's beam selection with step_rules.h's automaton inside it.
//
// Every (image, beam) slot carries (s, depth), (0, 0) at the start.  For a LIVE parent j in (s_j, d_j) the candidate (j, v) is
//   score[j] + (logit[j][v] - lse[j])   iff rules[s_j][v] allows v at d_j (rule_allows),   -INFINITY otherwise
// with lse[j] the log-sum-exp of the RAW row: nothing is renormalised, a beam's score stays the sum of the raw model's log-probabilities
// of its tokens.  The masked value is the beam code's own dead marker -INFINITY, not the -3.4e38f of the single-row pick: a masked
// candidate ranks with the candidates of dead beams, behind every finite one.  A FINISHED parent offers eos at + 0 and nothing else,
// unmasked, and its state is frozen.  Slot r takes its parent's state advanced by its token (rule_next, rule_depth_after): the eos that
// finishes a beam advances the state once, its later repeats do not.
//
// Ranking, tie order (lower parent * V + token), back-pointers, slot tables, done flags and the arrival word are beam_select_kernel's.
// Fewer than k finite candidates is a normal case (a state that allows two tokens with k = 5 at position 0): the surplus slots are dead
// (score -inf), as slots 1 .. k-1 are before position 0; a dead beam's tokens and state are unspecified (in range).  A dead slot is never
// finished by the masked eos it may have been handed, and it does not hold the search open: once every LIVE beam of every image is finished
// nothing can revive a dead one, and the done flag is raised.
//
// Kernels of their own, behind every other kernel of the library: without rules -- or with the switch off -- a beam search runs step.h's
// kernels as they were.  The log-sum-exp below is theirs operation for operation, so an allow-all table gives their bits.
#pragma once
#include "step_rules.h"

namespace txo {

struct BeamRuleArgs {
    const int* rules; int n_states, depth_max;   // the packed table [n_states][V] and its depth cap (step_rules.h)
    int2* state;                                 // [images*k] the RANGE's slice of the (state, depth) of every slot, updated in place
};

__device__ inline int2 beam_rule_state(const BeamRuleArgs& ra, int row) {
    int2 sd = ra.state[row];
    if ((unsigned)sd.x >= (unsigned)ra.n_states) sd.x = 0;
    return sd;
}
// the state of the slot that continues a parent in (s, depth) with token v; a finished parent's is frozen
__device__ inline int2 beam_rule_next(const BeamRuleArgs& ra, int V, int2 sd, int v, int parent_finished) {
    if (parent_finished) return sd;
    const int r = ra.rules[(size_t)sd.x * V + v];
    return make_int2(rule_next(r), rule_depth_after(r, sd.y, ra.depth_max));
}
// One workgroup per image, 256 threads, like beam_select_kernel; LOGP as there.
template <bool LOGP>
__global__ __launch_bounds__(256) void beam_select_rules_kernel(BeamArgs a, BeamRuleArgs ra) {
    constexpr int KMAX = 8;
    __shared__ float red[8], s_lse[KMAX], s_score[KMAX], selv[KMAX];
    __shared__ int redi[4], s_fin[KMAX], seli[KMAX];
    __shared__ int2 s_state[KMAX];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k, V = a.V, t = a.st->t;
    const float* lg = a.logits + (size_t)img * k * V;
    constexpr int VPT = 4;                                    // register path: vocabularies up to 256 * VPT entries
    if (V <= 256 * VPT) {
        // beam_select_kernel's register path; the k rule-row reads go out beside the logits reads and each is folded at once into one bit
        // of `ok` (bit j * VPT + i: the candidate is allowed) -- no rule word stays in a register
        __shared__ float rmx[KMAX][4], rse[KMAX][4], rbv[2][4];
        __shared__ int rbi[2][4];
        float x[KMAX][VPT], sc[KMAX]; int fn[KMAX]; int2 sd[KMAX];
        unsigned ok = 0u;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            sc[j] = 0.f; fn[j] = 0; sd[j] = make_int2(0, 0);
            if (j < k) { sc[j] = a.score[img * k + j]; fn[j] = a.fin[img * k + j]; sd[j] = beam_rule_state(ra, img * k + j); }
            const int* rl = ra.rules + (size_t)sd[j].x * V;
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int v = tid + 256 * i;
                const bool in = j < k && v < V;
                x[j][i] = in ? lg[(size_t)j * V + v] : 0.f;
                const int r = in ? rl[v] : RULE_BAN;
                ok |= (rule_allows(r, sd[j].y, ra.depth_max) ? 1u : 0u) << (j * VPT + i);
            }
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
        // candidates in place of the logits: the raw row minus the raw log-sum-exp where allowed
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
        // (every thread read the image's k states before the first selection barrier: the writes below are in place)
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
                ra.state[row] = beam_rule_next(ra, V, sj, v, fj);
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
    if (tid < k) { s_score[tid] = a.score[img * k + tid]; s_fin[tid] = a.fin[img * k + tid]; s_state[tid] = beam_rule_state(ra, img * k + tid); }
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
    // k rounds of block-wide arg max over the k*V candidates, excluding what was already taken; the mask inside the candidate loop
    const int total = k * V;
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
                const int2 sj = s_state[j];
                c = rule_allows(ra.rules[(size_t)sj.x * V + v], sj.y, ra.depth_max) ? s_score[j] + (lg[f] - s_lse[j]) : -INFINITY;
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
    // new beams: slot r of this image continues beam seli[r] / V with token seli[r] % V (the states were read into LDS before the barriers above)
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
            ra.state[row] = beam_rule_next(ra, V, s_state[j], v, s_fin[j]);
            if constexpr (LOGP) a.logp_hist[(size_t)t * a.hist_stride + row] = s_fin[j] ? 0.f : lg[sel] - s_lse[j];
        }
        beam_copy_path(a, img, r, j, t, tid);
    }
    if (tid == 0) beam_arrive(a, t, allfin);
}

// Closing search (texocr.h: txo_set_rules_close; step_rules.h has the rule): for a live unfinished parent j the candidate (j, v) is finite iff
// the budgeted rule holds with that parent's state and R = positions - t picks left.  Finished parents, dead slots, the arrival word and
// beam_finish_rules_kernel are untouched, so every live beam of a closing search ends finished.  positions is a launch scalar: a beam
// step is never captured.
struct BeamCloseArgs { const CloseTable* tab; int positions; };
// parent (s, depth)'s budget at R picks left: the largest distance a non-eos candidate may land at, -1 = unbudgeted (the plain rule)
__device__ inline int beam_close_lim(const BeamCloseArgs& ca, const BeamRuleArgs& ra, int2 sd, int R) {
    const CloseRow cr = close_row(ca.tab, make_int2(R, 0), 0, sd.x, sd.y, ra.depth_max);
    return cr.bind ? cr.lim : -1;
}

// beam_select_rules_kernel with the budget: the same two paths, operation for operation, and where the budget cannot bind (R - 1 >= slack, a
// finished parent, an infinite distance) the same predicate.  A kernel of its own, so that the plain constrained search keeps its code.
template <bool LOGP>
__global__ __launch_bounds__(256) void beam_select_close_kernel(BeamArgs a, BeamRuleArgs ra, BeamCloseArgs ca) {
    constexpr int KMAX = 8;
    __shared__ float red[8], s_lse[KMAX], s_score[KMAX], selv[KMAX];
    __shared__ int redi[4], s_fin[KMAX], seli[KMAX];
    __shared__ int2 s_state[KMAX];
    __shared__ __attribute__((aligned(16))) unsigned short cl[CLOSE_NODES];
    __shared__ int s_lim[KMAX];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k, V = a.V, t = a.st->t;
    const float* lg = a.logits + (size_t)img * k * V;
    const int R = ca.positions - t;                           // (block-uniform) picks left, and whether the budget can bind at all
    const bool budget = R - 1 < ca.tab->slack;
    if (budget) close_stage(cl, ca.tab, ra.n_states * (ra.depth_max + 1), tid, 256);
    constexpr int VPT = 4;                                    // register path: vocabularies up to 256 * VPT entries
    if (V <= 256 * VPT) {
        // beam_select_kernel's register path; the k rule-row reads go out beside the logits reads and each is folded at once into one bit
        // of `ok` (bit j * VPT + i: the candidate is allowed) -- no rule word stays in a register
        __shared__ float rmx[KMAX][4], rse[KMAX][4], rbv[2][4];
        __shared__ int rbi[2][4];
        float x[KMAX][VPT], sc[KMAX]; int fn[KMAX]; int2 sd[KMAX];
        unsigned ok = 0u;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            sc[j] = 0.f; fn[j] = 0; sd[j] = make_int2(0, 0);
            if (j < k) { sc[j] = a.score[img * k + j]; fn[j] = a.fin[img * k + j]; sd[j] = beam_rule_state(ra, img * k + j); }
            const int* rl = ra.rules + (size_t)sd[j].x * V;
            int lim = -1;
            if (budget && j < k && !fn[j]) lim = beam_close_lim(ca, ra, sd[j], R);
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int v = tid + 256 * i;
                const bool in = j < k && v < V;
                x[j][i] = in ? lg[(size_t)j * V + v] : 0.f;
                const int r = in ? rl[v] : RULE_BAN;
                bool al;
                if (lim >= 0) al = close_allows(cl, r, v, sd[j].y, ra.depth_max, a.eos, lim);
                else al = rule_allows(r, sd[j].y, ra.depth_max);
                ok |= (al ? 1u : 0u) << (j * VPT + i);
            }
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
        // candidates in place of the logits: the raw row minus the raw log-sum-exp where allowed
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
        // (every thread read the image's k states before the first selection barrier: the writes below are in place)
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
                ra.state[row] = beam_rule_next(ra, V, sj, v, fj);
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
        s_score[tid] = a.score[img * k + tid]; s_fin[tid] = a.fin[img * k + tid]; s_state[tid] = beam_rule_state(ra, img * k + tid);
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
    // k rounds of block-wide arg max over the k*V candidates, excluding what was already taken; the mask inside the candidate loop
    const int total = k * V;
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
                const int2 sj = s_state[j];
                const int r = ra.rules[(size_t)sj.x * V + v];
                bool al;
                if (s_lim[j] >= 0) al = close_allows(cl, r, v, sj.y, ra.depth_max, a.eos, s_lim[j]);
                else al = rule_allows(r, sj.y, ra.depth_max);
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
    // new beams: slot r of this image continues beam seli[r] / V with token seli[r] % V (the states were read into LDS before the barriers above)
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
            ra.state[row] = beam_rule_next(ra, V, s_state[j], v, s_fin[j]);
            if constexpr (LOGP) a.logp_hist[(size_t)t * a.hist_stride + row] = s_fin[j] ? 0.f : lg[sel] - s_lse[j];
        }
        beam_copy_path(a, img, r, j, t, tid);
    }
    if (tid == 0) beam_arrive(a, t, allfin);
}

// beam_finish_kernel with the states: the same lengths, the same final order, tokens and increments, and the k states of the image moved
// into that order in place (read before the barrier, written behind it: the workgroup owns the image's slots).
__global__ __launch_bounds__(64) void beam_finish_rules_kernel(BeamFinishArgs a, int2* state) {
    __shared__ float s_key[8];
    const int img = blockIdx.x, r = threadIdx.x, k = a.k, row = img * k + r;
    int len = a.n; float sc = 0.f; int2 sd = make_int2(0, 0);
    if (r < k) {
        int cur = row;
        for (int t = a.n - 1; t >= 0; --t) {
            const size_t h = (size_t)t * a.hist_stride + cur;
            if (a.eos >= 0 && a.tok_hist[h] == a.eos) len = t + 1;
            cur = a.parent_hist[h];
        }
        sc = a.score[row];
        sd = state[row];
        float key = a.alpha > 0.f ? sc / powf((float)len, a.alpha) : 0.f;
        if ((__float_as_uint(key) & 0x7fffffffu) > 0x7f800000u) key = -INFINITY;      // (a NaN would compare false both ways: two beams, one row)
        s_key[r] = key;
    }
    __syncthreads();
    if (r >= k) return;
    int dst = 0;
    for (int q = 0; q < k; ++q) dst += (s_key[q] > s_key[r] || (s_key[q] == s_key[r] && q < r)) ? 1 : 0;
    const int orow = img * k + dst;
    if (a.scores) a.scores[orow] = sc;
    if (a.lengths) a.lengths[orow] = len;
    state[orow] = sd;
    int64_t* tk = a.tokens + (size_t)orow * a.out_stride;
    float* lp = a.logp ? a.logp + (size_t)orow * a.out_stride : nullptr;
    int cur = row;
    for (int t = a.n - 1; t >= 0; --t) {
        const size_t h = (size_t)t * a.hist_stride + cur;
        tk[t] = a.tok_hist[h];
        if (lp) lp[t] = a.logp_hist[h];
        cur = a.parent_hist[h];
    }
}

// the tail of a beam call: with `state` (a constrained search) the slots' states follow their beams into the final order
inline void launch_beam_finish(hipStream_t s, int images, const BeamFinishArgs& fa, int2* state) {
    if (state) hipLaunchKernelGGL(beam_finish_rules_kernel, dim3(images), dim3(64), 0, s, fa, state);
    else hipLaunchKernelGGL(beam_finish_kernel, dim3(images), dim3(64), 0, s, fa);
}

}  // namespace txo
