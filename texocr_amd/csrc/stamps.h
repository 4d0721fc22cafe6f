// Launch-path and persistent-launch time stamps (diagnostics: TXO_STAMPS, TXO_PSTAMPS, TXO_STAMPS_RAW -- knobs.h).  Host code, included
// by engine.hip only.  The text format of both files is what probes/stamp_run.py and probes/pstamp_run.py read.
#pragma once
#include "persist.h"   // PS_* (the persistent launch's stamp layout)

namespace txo {

struct Stamps {
    // TXO_STAMPS=<file>: every decode launch of ONE position records per-block entry / mid / exit times into buf (device, engine-owned)
    static constexpr int BLOCKS = 2048, KERNELS = 64;
    unsigned long long* buf = nullptr; int slot = -1;   // slot >= 0: the position being stamped; its next launch takes this slot
    std::vector<std::string> names;
    unsigned long long* next(const char* name) {
        if (slot < 0 || slot >= KERNELS) return nullptr;
        names.push_back(name);
        return buf + (size_t)(slot++) * BLOCKS * 3;
    }
    int begin(hipStream_t s) { HIP_TRY(hipMemsetAsync(buf, 0, sizeof(unsigned long long) * KERNELS * BLOCKS * 3, s)); slot = 0; names.clear(); return 0; }
    // raw: also one line per block of the launches whose name contains it (which CU / tile is the slow one)
    void dump(const char* file, const std::string* raw, hipStream_t s) {
        const int nk = slot; slot = -1;
        std::vector<unsigned long long> h((size_t)nk * BLOCKS * 3);
        if (hipStreamSynchronize(s) != hipSuccess) return;
        if (hipMemcpy(h.data(), buf, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return;
        FILE* f = fopen(file, "w");
        if (!f) return;
        unsigned long long t0 = ~0ull;
        for (auto v : h) if (v && v < t0) t0 = v;
        for (int k2 = 0; k2 < nk; ++k2) {
            unsigned long long first = ~0ull, last_in = 0, mid_lo = ~0ull, mid_hi = 0, first_out = ~0ull, last = 0; int nb = 0;
            for (int b = 0; b < BLOCKS; ++b) {
                const unsigned long long* d = &h[((size_t)k2 * BLOCKS + b) * 3];
                if (!d[0]) continue;
                ++nb; first = std::min(first, d[0]); last_in = std::max(last_in, d[0]); mid_lo = std::min(mid_lo, d[1]); mid_hi = std::max(mid_hi, d[1]);
                first_out = std::min(first_out, d[2]); last = std::max(last, d[2]);
            }
            fprintf(f, "%-24s blocks %4d | first entry %7.2f us, last entry %7.2f | operands/panel done %7.2f .. %7.2f | first exit %7.2f, last exit %7.2f\n",
                    names[k2].c_str(), nb, (first - t0) / 100.0, (last_in - t0) / 100.0, (mid_lo - t0) / 100.0, (mid_hi - t0) / 100.0,
                    (first_out - t0) / 100.0, (last - t0) / 100.0);
        }
        if (raw) {
            for (int k2 = 0; k2 < nk; ++k2) {
                if (names[k2].find(*raw) == std::string::npos) continue;
                for (int b = 0; b < BLOCKS; ++b) {
                    const unsigned long long* d = &h[((size_t)k2 * BLOCKS + b) * 3];
                    if (d[0]) fprintf(f, "raw %d %-24s block %4d  %7.2f %7.2f %7.2f\n", k2, names[k2].c_str(), b, (d[0] - t0) / 100.0, (d[1] - t0) / 100.0, (d[2] - t0) / 100.0);
                }
            }
        }
        fclose(f);
    }
    // TXO_PSTAMPS=<file>: the persistent launch's per-stage stamps of one position (persist.h), dev = the launch's stamp buffer
    static void dump_persist(const char* file, const unsigned long long* dev, int nteams, int layers) {
        const int ns = 7 * layers + 2;
        std::vector<unsigned long long> h((size_t)PS_TEAMS * PS_STAMP_RANKS * PS_MAX_STAGES * PS_STAMP_WORDS);
        if (hipMemcpy(h.data(), dev, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return;
        FILE* f = fopen(file, "w");
        if (!f) return;
        static const char* names[7] = {"LN+qkv gemm", "self attention", "self out-proj+GLU+res", "cross attention (LN+q fused)",
                                       "cross out-proj+GLU+res", "LN+ffn-in+GeGLU", "ffn-out+res"};
        static const int ranks[PS_STAMP_RANKS] = {0, 10, 20, PS_TEAM_BLOCKS - 1};
        fprintf(f, "# persistent decode launch, ONE decode position, workgroups of rank 0 / 10 / 20 / 31 of every team.  Per stage, us:\n"
                   "#   poll  = polling the team counter for the previous stage's arrivals (weights / K panel already requested)\n"
                   "#   work  = barrier + read the previous stage's rows (sc1) + compute + issue the stores\n"
                   "#   drain = s_waitcnt vmcnt(0) of every wave + workgroup barrier\n"
                   "#   pub   = the arrival atomic, issued -> returned\n"
                   "#   end   = time of publication since the position's first stamp\n");
        for (int k = 0; k < nteams; ++k)
            for (int r = 0; r < PS_STAMP_RANKS; ++r) {
                const unsigned long long* d = &h[((size_t)k * PS_STAMP_RANKS + r) * PS_MAX_STAGES * PS_STAMP_WORDS];
                if (!d[2]) continue;
                const unsigned long long t0 = d[2];
                fprintf(f, "team %d rank %d: position span %.2f us\n", k, ranks[r], (d[(ns - 1) * PS_STAMP_WORDS + 4] - t0) / 100.0);
                if (k > 1) continue;                           // the per-stage table for two teams is enough
                for (int i = 0; i < ns; ++i) {
                    const unsigned long long* e = d + i * PS_STAMP_WORDS;
                    const char* nm = i < 7 * layers ? names[i % 7] : (i == 7 * layers ? "LNf+logits" : "argmax+append");
                    fprintf(f, "  L%-2d %-30s poll %5.2f  work %5.2f  drain %5.2f  pub %5.2f | end %7.2f", i < 7 * layers ? i / 7 : -1, nm,
                            e[0] ? (e[1] - e[0]) / 100.0 : 0.0, e[1] ? (e[2] - e[1]) / 100.0 : 0.0, (e[3] - e[2]) / 100.0, (e[4] - e[3]) / 100.0,
                            (e[4] - t0) / 100.0);
                    const bool attn = i < 7 * layers && (i % 7 == 1 || i % 7 == 3);
                    if (e[5] && e[1] && !attn)   // GEMM tile of the workgroup's first group: rows read + MFMAs | K reduction | epilogue
                        fprintf(f, " | tile: seen->mfma done %5.2f  reduce %5.2f  epilogue+stores %5.2f", (e[6] - e[1]) / 100.0, (e[7] - e[6]) / 100.0, (e[2] - e[7]) / 100.0);
                    if (e[5] && e[1] && attn)    // attention tile of the workgroup's first group: wait end -> last pass's scores and PV done | reductions + store
                        fprintf(f, " | tile: seen->panel consumed %5.2f  reduce+store %5.2f  (other group / barrier %5.2f)", ((long long)e[6] - (long long)e[1]) / 100.0,
                                (e[7] - e[6]) / 100.0, ((long long)e[2] - (long long)e[7]) / 100.0);
                    if (e[5] && e[0] && i > 0)   // before the poll: previous publication -> tile entry (stage set-up) -> poll begin (the tile's weight / bias / gamma requests)
                        fprintf(f, " | pre: setup %5.2f  requests %5.2f", ((long long)e[5] - (long long)(e - PS_STAMP_WORDS)[4]) / 100.0, ((long long)e[0] - (long long)e[5]) / 100.0);
                    fprintf(f, "\n");
                }
            }
        fclose(f);
    }
};

}  // namespace txo
