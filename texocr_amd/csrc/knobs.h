// Every TXO_* environment variable the library reads, in one table (INTEGRATION.md mirrors it).  Host code, included by engine.hip only.
// Each entry: the variable and its default (in the code), then when it is read and its kind -- product setting (a deployment may set it),
// test hook (tests drive a path with it), A/B switch (the other side of a bit-identity or speed comparison) or diagnostic -- and what it does.
#pragma once
#include "gemm_pp.h"   // PP_SB_MB

namespace txo {

inline bool env_set(const char* n) { return getenv(n) != nullptr; }
inline int env_int(const char* n, int unset) { const char* e = getenv(n); return e ? atoi(e) : unset; }
inline int env_bool(const char* n, int unset) { const char* e = getenv(n); return e ? (atoi(e) != 0) : unset; }
inline int env_min1(const char* n, int unset) { const char* e = getenv(n); return e ? std::max(1, atoi(e)) : unset; }
inline bool env_str(const char* n, std::string* v) { const char* e = getenv(n); if (e) *v = e; return e != nullptr; }

static const bool g_dbg = env_set("TXO_DEBUG_SYNC");            // library load; diagnostic -- synchronise + print the status after every decode launch

struct Knobs {
    // Re-read by txo_engine_query(TXO_Q_RELOAD_KNOBS): the Python binding sends it when the TXO_* environment changed between two calls
    // (tests flip TXO_PERSIST / TXO_LANES on a live engine).  Run{} reads them: every field's initialiser is its read.
    struct Run {
        int persist = env_bool("TXO_PERSIST", -1);              // creation + reload; test hook / A/B switch -- 0 / 1 forces the persistent launch; unset = by batch
        int graph = env_bool("TXO_GRAPH", -1);                  // creation + reload; A/B switch -- 0 / 1 forces graph replay; unset = for B <= 4
        int lanes = env_min1("TXO_LANES", 0);                   // creation + reload; test hook -- row ranges (>= 1) of a launch-path decode; unset = by shape
        std::string stamps_file; bool stamps = env_str("TXO_STAMPS", &stamps_file);        // creation + reload; diagnostic -- <file>: per-block times of one position's launches
        std::string pstamps_file; bool pstamps = env_str("TXO_PSTAMPS", &pstamps_file);    // creation + reload; diagnostic -- <file>: per-stage times of one persistent position
        bool has_stagger = env_set("TXO_PS_STAGGER_US");        // creation + reload; A/B switch -- <us>: persist.h's stagger of the teams (in 10 ns ticks)
        int stagger_ticks = has_stagger ? (int)(atof(getenv("TXO_PS_STAGGER_US")) * 100.0) : 0;
        bool has_inject = env_set("TXO_PERSIST_INJECT_FAIL");   // creation + reload; test hook -- <n>: the persistent launch gives up (its fall-back path)
        int inject_fail = env_int("TXO_PERSIST_INJECT_FAIL", 0);
        void read() { *this = Run{}; }
    } run;
    bool backbone_bf16 = env_set("TXO_BACKBONE_BF16");        // creation; product setting -- bf16 backbone in the bf16 engine (checkpoints that tolerate it); unset = fp32
    bool bk_exact = env_set("TXO_BACKBONE_EXACT");            // creation; A/B switch -- exact-f32 backbone GEMM in the bf16 engine; unset = split onto bf16 MFMA
    bool self_plain = !env_set("TXO_SELF_FUSED");             // creation; A/B switch -- set: self-attention projection fused into the attention launch
    bool dec_wide_off = env_set("TXO_DEC_WIDE_OFF");          // creation; A/B switch -- set: no multi-tile decode GEMM blocks (16-row blocks only)
    int lat_self_env = env_int("TXO_LATENT_SELF", 0);         // creation; product setting -- 1: self attention in latent form (z history)
    int lat_mode = env_int("TXO_LATENT", -1);                 // creation; product setting -- 0 / 1 pins the cross-attention form; unset = auto_latent
    int lat_g_env = env_int("TXO_LAT_G", 0);                  // creation; A/B switch -- heads per latent tile; 0 = by rows (latent_group)
    bool use_pp = !env_set("TXO_GEMM_OLD");                   // creation; A/B switch -- set: 128x128 register-staged GEMM instead of gemm_pp (bf16)
    int pp_tr = env_bool("TXO_PP_TR", -1);                    // creation; A/B switch -- gemm_pp epilogue 1 direct / 0 staged through LDS; unset = by epilogue
    int pp_ct = env_int("TXO_PP_CT", 0);                      // creation; A/B switch -- gemm_pp column tiles per band; 0 = by size
    int pp_sb_mb = env_int("TXO_PP_SB_MB", PP_SB_MB);         // creation; A/B switch -- MB of A per gemm_pp row super-block; 0 = none
    int tune_lanes = env_int("TXO_TUNE_LANES", 1);            // creation; A/B switch -- 0: no stream-pair tuning (range 0 on the caller's stream)
    bool tune_verbose = env_set("TXO_TUNE_LANES_VERBOSE");    // creation; diagnostic -- print the stream-pair tuning's timings
    bool stop_graph_on = env_bool("TXO_STOP_GRAPH", 1);       // creation; A/B switch -- 0: per-row stop with eager launches instead of replay
    int stop_every = env_min1("TXO_STOP_EVERY", 16);          // creation; A/B switch -- positions between two looks at the live-row counts
    int stop_gain = env_min1("TXO_STOP_GAIN", 16);            // creation; A/B switch -- rows a compaction must free
    int enc_chunk_env = env_int("TXO_ENC_CHUNK", -1);         // creation; A/B switch -- images per encoder chunk, 0 = whole batch; unset = whole batch
    int w_tiled_on = env_int("TXO_W_TILED", 1);               // creation; A/B switch -- 0: decode projections read the row-major weights
    int a_tiled_on = env_int("TXO_A_TILED", 1);               // creation; A/B switch -- 0: the latent core writes c row-major
    std::string stamps_raw; bool has_stamps_raw = env_str("TXO_STAMPS_RAW", &stamps_raw);  // creation; diagnostic -- <substring>: TXO_STAMPS also per block
};

}  // namespace txo
