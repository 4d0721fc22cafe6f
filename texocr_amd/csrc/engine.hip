// Engine + C ABI (include/texocr.h) for the MI355X-native OCRModel.generate() path.
// Host side only orchestrates: all arithmetic is in the HIP kernels of this directory.
#include "../../include/texocr.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

namespace txo {
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
}  // namespace txo
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return txo::fail(TXO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
    } while (0)

#include "common.h"
#include "conv.h"
#include "dec_attn.h"
#include "dec_gemm.h"
#include "enc_attn.h"
#include "gemm_big.h"
#include "gemm_pp.h"
#include "gemm_split.h"
#include "lat_attn.h"
#include "persist.h"
#include "prefill.h"
#include "attn_probs.h"
#include "score.h"
#include "rows.h"
#include "step.h"
#include "step_prefix.h"   // (behind every other kernel: the kernels above keep their places in the code object)
#include "ingest.h"        // (likewise: the newest kernel goes last)
#include "ingest_fit.h"    // (the fit-to-canvas passes in front of it; uses ingest.h's per-pixel pieces)
#include "ingest_trim.h"   // (the ink extents in front of both; reads ingest.h's descriptors)
#include "step_rules.h"    // (the constrained token selection: step.h / step_prefix.h with a per-row automaton; last again)
#include "step_guard.h"    // (the repeat guard's token selection: step_rules.h with a ban on the block a row has just repeated; last again)
#include "beam_rules.h"    // (the constrained beam selection: step.h's beam kernels with that automaton; last again)
#include "rules_close.h"   // (host only: the closing decode's distance table)
#include "beam_guard.h"    // (the repeat guard inside the beam selection: beam_rules.h with step_guard.h's ban; last again)
#include "step_alts.h"     // (the k best of every row in front of the pick: step.h's streaming with kbest.h's lists; last again)
#include "knobs.h"    // host helpers from here on (they use fail() / HIP_TRY)
#include "lanes.h"
#include "session.h"
#include "stamps.h"
#include "ingest_req.h"

namespace txo {

static void dbg(hipStream_t s, const char* what, int l = -1) {
    if (!g_dbg) return;
    hipError_t e = hipStreamSynchronize(s);
    fprintf(stderr, "[txo] %s %d -> %s\n", what, l, hipGetErrorString(e));
    fflush(stderr);
}

struct HostTensor { std::vector<int64_t> shape; std::vector<float> data; };

// -------------------------------------------------------------------------------------------------
struct EngineBase {
    txo_config cfg{};
    std::map<std::string, HostTensor> host;     // reference-keyed weights until finalize
    bool ready = false;
    virtual ~EngineBase() {}
    virtual int finalize() = 0;
    virtual int encode(const float* img, int B, int C, int H, int W, float* enc_out, hipStream_t s) = 0;
    virtual int decode_begin(const float* enc, int B, int N, int eos, hipStream_t s) = 0;
    virtual int encode_ragged(const float* img, int B, int C, int Hc, int Wc, const int32_t* sizes, float* enc_out, int32_t* n_slot, hipStream_t s) = 0;
    virtual int decode_begin_ragged(const float* enc, int B, int Ns, const int32_t* n_tokens, int eos, hipStream_t s) = 0;
    virtual int score_ragged(const float* img, int B, int C, int Hc, int Wc, const int32_t* sizes, const int64_t* tokens, const unsigned char* mask,
                             int L, float* logp_out, int64_t* top1_out, float* top1_logp_out, hipStream_t s) = 0;
    // every txo_generate* but _beam (session.h).  Its slot here, where the first entry into the decode loop always stood, decides when the loop's
    // template kernels are first used, and with it their order in the code object (see the kernel #include list)
    virtual int generate(const DecodeReq& q, hipStream_t s) = 0;
    virtual int decode_step(const int64_t* tok_in, int t, float* logits_out, int64_t* tok_out, hipStream_t s) = 0;
    virtual int decode_prefill(const int64_t* tokens, int t, float* logits_out, hipStream_t s) = 0;
    virtual int decode_score(const int64_t* tokens, int L, float* logp_out, int64_t* top1_out, float* top1_logp_out, hipStream_t s) = 0;
    virtual int decode_attn(const int64_t* tokens, int t, float* logits_out, float* self_attn_out, float* cross_attn_out, float* cross_mean_out,
                            hipStream_t s) = 0;
    virtual int score(const float* img, int B, int C, int H, int W, const int64_t* tokens, const unsigned char* mask, int L, float* logp_out,
                      int64_t* top1_out, float* top1_logp_out, hipStream_t s) = 0;
    virtual int decode_set_key_mask(const unsigned char* mask, int cols, hipStream_t s) = 0;
    // txo_generate_beam (sink.best) / txo_beam_search, txo_beam_search_ragged (sink.out)
    virtual int beam_search(const DecodeSrc& src, int beams, int max_len, int eos, const BeamSink& sink, int* n_steps, hipStream_t s) = 0;
    int sample_mode = 0, sample_topk = 0; float sample_temp = 1.f; unsigned long long sample_seed = 0;
    size_t sample_lds_max = 65536;              // dynamic LDS the LDS-form sampler may ask for (init: the device's per-workgroup limit)
    int stop_mode = 0;                          // txo_set_stop_mode: 0 = the reference's global eos break only, 1 = per-row stop (pad behind a row's first eos)
    bool rag_fwd = false;                       // txo_set_ragged_forward: the multi-position forward on ragged sessions and the ragged sliding window are accepted
    bool rag_hybrid = false;                    // txo_set_ragged_hybrid: ragged batches are accepted on the hybrid front end (conv.h: the RAGGED forms)
    // txo_set_token_rules (step_rules.h): every generate from BOS or a prefix decodes on the launch path with the *_rules_step kernels while on
    bool rules_on = false; int rules_S = 0, rules_dmax = 0;
    int rules_rows = 0;                         // rows of the last constrained generate (txo_last_rule_state), 0: none since the rules were set
    virtual int set_token_rules(const int32_t* table, int S, int depth_max) = 0;   // behind txo_set_token_rules's checks; table null: off
    virtual int last_rule_state(int32_t* out, int B, hipStream_t s) = 0;
    // txo_set_rules_beam (beam_rules.h): while on, a beam search under token rules runs the constrained selection instead of being refused
    bool rules_beam = false;
    // txo_set_guard_beam (beam_guard.h): while on, a beam search under a repeat guard runs the guarded selection instead of being refused
    bool guard_beam = false;
    int brule_B = 0, brule_k = 0;               // images / beams of the last constrained beam search (txo_last_beam_rule_state), 0: none since the rules were set
    virtual int last_beam_rule_state(int32_t* out, int B, int beams, hipStream_t s) = 0;
    // txo_set_rules_close (rules_close.h; the closing kernels of step_rules.h / beam_rules.h): while on, a constrained decode or beam search
    // picks under the budget that ends every row at an allowed eos.  close_dist [S][depth_max + 1]: the table while rules and switch are both set
    bool rules_close = false;
    std::vector<int32_t> close_dist; int close_dist_max = 0;
    bool closing() const { return rules_on && rules_close; }
    virtual int set_rules_close(bool on) = 0;
    // txo_set_repeat_guard (step_guard.h): while set (max_period > 0), every generate from BOS or a prefix decodes on the launch path with the
    // *_guard_step kernels; last_guarded: the last txo_generate* ran them (TXO_Q_LAST_GUARDED)
    int guard_p = 0, guard_r = 0; bool last_guarded = false;
    // txo_set_alternatives (step_alts.h): while set (k > 0), every generate from BOS or a prefix decodes on the launch path with
    // alts_step_kernel in front of its pick.  last_alts: the k of the last txo_generate* (TXO_Q_LAST_ALTS), alts_B x alts_cols what
    // txo_last_alternatives may read of it
    int alts_k = 0, last_alts = 0, alts_B = 0, alts_cols = 0;
    virtual int last_alternatives(int32_t* ids_out, float* logp_out, int B, int cols, hipStream_t s) = 0;
    virtual int decode_score_alts(const int64_t* tokens, int L, float* logp_out, int64_t* top1_out, float* top1_logp_out, int k, int32_t* alt_ids_out,
                                  float* alt_logp_out, hipStream_t s) = 0;
    virtual int score_alts(const float* img, int B, int C, int H, int W, const int64_t* tokens, const unsigned char* mask, int L, float* logp_out,
                           int64_t* top1_out, float* top1_logp_out, int k, int32_t* alt_ids_out, float* alt_logp_out, hipStream_t s) = 0;
    // txo_ingest_u8 / _fit / _view behind their checks (ingest_req.h: ingest_plan): descriptors up in one staged copy, then one launch -- or,
    // where an image is downscaled, the horizontal pass of those that need one and the fused vertical pass + ingest
    virtual int ingest(const IngestPlan& p, const IngestReq& q, hipStream_t s) = 0;
    // txo_ingest_trim_views behind its checks: the ink extents of every image (ingest_trim.h) -> views [B][4]; waits on s
    virtual int trim_views(const IngestList& l, int level, int margin, int32_t* views, hipStream_t s) = 0;
    virtual int query(int what, int64_t* out) = 0;
    virtual int profile_enable(int on) = 0;
    virtual int profile_read(int kind, double* avg_ms, int64_t* count) = 0;
};

// rows [2X][K] -> groups of 2G rows: G "value" rows (g*G..) followed by their G "gate" rows (X + g*G..).
// G = 16 for the encoder GEMM (value / gate in adjacent MFMA column tiles), 8 for the decode GEMMs (both halves inside one tile)
static std::vector<float> interleave(const std::vector<float>& w, int X, int K, int G) {
    std::vector<float> o((size_t)2 * X * K);
    for (int g = 0; g < X / G; ++g)
        for (int h = 0; h < 2; ++h)
            for (int r = 0; r < G; ++r)
                memcpy(&o[((size_t)g * 2 * G + h * G + r) * K], &w[((size_t)h * X + g * G + r) * K], sizeof(float) * K);
    return o;
}

struct EventPool {
    std::vector<hipEvent_t> ev; size_t used = 0;
    hipEvent_t next() {
        if (used == ev.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; ev.push_back(e); }
        return ev[used++];
    }
    ~EventPool() { for (auto e : ev) (void)hipEventDestroy(e); }
};

template <typename T>
struct Engine : EngineBase {
    Knobs knobs;                      // every TXO_* setting, read at creation (knobs.h)
    // ----- device weights -----
    std::vector<void*> allocs;
    struct AttnW { T* wqkv = nullptr; T* wq = nullptr; T* wo = nullptr; float* bo = nullptr;
                   T* wo16 = nullptr; float* bo16 = nullptr;    // decoder: second copy interleaved by 16 (prefill: the large-GEMM epilogues)
                   T* wkT = nullptr; T* wv = nullptr;   
                   T* wqp = nullptr; T* wo_f = nullptr; };      // ... folded where inner == 2 D: q' = z (0.125 Wk_h^T Wq_h)^T [heads*D][D]; Wo' = Wo blockdiag(Wv_h) [2D][heads*D], rows interleaved by 8        // decoder cross attention, latent form (lat_attn.h): Wk per head transposed [heads][D][64], Wv [inner][D]
    struct MlpW { T* w1 = nullptr; float* b1 = nullptr; T* w2 = nullptr; float* b2 = nullptr;
                  T* w1_16 = nullptr; float* b1_16 = nullptr; };   // decoder, wide rows: second copy interleaved by 16 (large-batch FFN-in)
    float *cls = nullptr, *pos = nullptr, *patch_b = nullptr; T* patch_w = nullptr;
    // hybrid ResNetV2 embedder: standardised conv weights as [oc][kh][kw][ic] of T, GroupNorm affine fp32
    struct GnW { float* g = nullptr; float* b = nullptr; };
    template <typename TB> struct BlockW { TB *c1 = nullptr, *c2 = nullptr, *c3 = nullptr, *ds = nullptr; GnW n1, n2, n3, nds; int cin, mid, cout, stride; bool has_ds; };
    // the backbone in storage type TB: weights, the four activation buffers, the 1x1 projection to the embedding width
    template <typename TB> struct Backbone { TB* stem_w = nullptr; GnW stem_gn; std::vector<BlockW<TB>> blocks; TB* act[4] = {nullptr, nullptr, nullptr, nullptr}; TB* proj_w = nullptr; };
    Backbone<T> bk; Backbone<float> bk32;
    float *gn_partial = nullptr, *gn_stats = nullptr;
    bool hybrid = false;
    // bf16 mode, hybrid embedder: the BACKBONE still stores and multiplies in fp32 (bk32; r06).  With the reference's 45 conv / GroupNorm
    // layers at random weights a perturbation of 2^-9 anywhere -- rounding the input pixels alone -- moves the backbone's output by 10-20 %
    // (tests/test_oracle_golden.py), so no choice of WHICH tensors are stored as bf16 gives a usable mode; fp32 here costs ~3 ms per 64
    // images and puts the bf16 engine's encoder output within 1-2 % of the fp32 reference.  TXO_BACKBONE_BF16=1: the bf16 backbone
    // (r02-r05; kernels checked against a CPU emulation of bf16 storage) for checkpoints known to tolerate it.
    bool bk_fp32 = sizeof(T) == 2 && !knobs.backbone_bf16;
    float *enc_g = nullptr, *enc_b = nullptr, *encn_g = nullptr, *encn_b = nullptr, *enc_gb = nullptr;   // enc_gb: gamma then beta (GEMM epilogues)
    std::vector<AttnW> enc_attn; std::vector<MlpW> enc_mlp;
    float *tok_emb = nullptr, *pos_emb = nullptr, *dec_g = nullptr, *dec_b = nullptr, *decn_g = nullptr, *decn_b = nullptr, *dec_gb = nullptr;
    T* wlog = nullptr; float* blog = nullptr; T* wckv = nullptr;
    std::vector<AttnW> dec_self, dec_cross; std::vector<MlpW> dec_mlp;
    // ----- workspace -----
    float *ex = nullptr, *ey = nullptr, *eqkv = nullptr, *eenc = nullptr, *estats = nullptr; T *ez = nullptr, *eao = nullptr, *ehid = nullptr;
    T* enc_t = nullptr;               // bf16 copy of the encoder output (A operand of the cross K/V GEMM)
    T *ckv = nullptr, *skv = nullptr;  // cross [Ld][2][B*h][N][64], self [Ld][2][B*h][Tmax][64]
    float *dx = nullptr, *dy = nullptr, *dq = nullptr, *dlogits = nullptr; T *dao = nullptr, *dhid = nullptr, *dz = nullptr;
    T* zc = nullptr;                  // self attention in latent form: history of normalised block inputs [Ld][B][Tmax][D] (lat_attn.h)
    T *dqt = nullptr, *dqp = nullptr, *dcl = nullptr;   // latent cross attention: q [B][inner], q' and c [B][heads*D] in the storage type
    int64_t* cur_tok = nullptr; int *eos_seen = nullptr, *done_flag = nullptr; StepState* st = nullptr;
    unsigned char* kmask = nullptr;   // padding mask over the decoded positions of a decode_step session (txo_decode_set_key_mask)
    // ----- decode session: 1..MAXL row ranges (lanes.h); a range's step is a fixed launch sequence, captured once and replayed -----
    static constexpr int MAXL = LaneSet::MAXL;
    LaneSet lanes;
    // narrow decoder, folded latent out-projection (K = heads * D): 32 x 16 blocks from wide_mid_rows rows of a range on, 16 x 16 blocks below.
    // The 32 x 32 form (from wide_min_rows on: never, decode rows are < 65536) is KEPT: without its instantiation every later kernel of the code
    // object moves, and the bf16 persistent launch (143 KB, over twice the instruction cache) measured 1.5 % slower in alternating runs.
    static constexpr int wide_min_rows = 100000;   // (257 until the tiled operands: at a beam search's 320 rows per range 32 x 16 is now ahead, 98.5 vs 100.5 ms)
    static constexpr int wide_mid_rows = 129;
    // cross attention in latent form (lat_attn.h): scores / values against the raw encoder rows instead of projected K/V panels.
    // latent_ok: the tile exists for this engine's width / storage type.  knobs.lat_mode (TXO_LATENT): 1 = every decode runs with
    // launches in latent form, 0 = never, unset = where it measured faster (auto_latent).  ses.latent: what the current session does.
    bool latent_ok = false;
    int n_cus = 256;                  // compute units of this engine's device (init): one latent tile per CU is the grouping target
    // ses.lat_self: this session's SELF attention also runs in latent form (the history is z, not k / v: a quarter of the bytes at config.yml
    // dims).  Only inside generate() / generate_beam() with launches in latent form: a session opened through txo_decode_begin may be
    // prefilled or masked, which work on the K/V history.  OPT-IN (TXO_LATENT_SELF=1): measured on MI355X it
    // ties the K/V history at batch 256 (76.5 vs 76.7 ms per generate: the core is 9.8 us against 14.8 for the K/V kernel, averaged over
    // the 256 positions, but the folded output projection's K = heads*D costs 9.1 us against 4.8) and loses in beam search (121 vs 115 ms
    // at 5 x 128); what it saves is history capacity (a quarter).  profiles/r05_latent_self.txt.
    bool lat_self_ok() const {
        // (the beam slot table of the tile covers 16 keys x its wave count x LA_PATH_TILES positions: the bf16 tile at width 256 runs on 4 waves)
        const int waves = (D <= 256 && !(lat_nw4 && D == 256)) ? 8 : 4;
        return knobs.lat_self_env != 0 && zc != nullptr && !dec_self.empty() && dec_self[0].wqp != nullptr && Tmax <= 16 * waves * LA_PATH_TILES;
    }
    // bf16, width 256: the latent tile on FOUR waves (r05).  Same one tile per CU, half the waves to
    // merge and twice the keys per wave: the whole-batch launch at 256 rows 19.3 -> 17.9 us (rocprofv3), generate +2-3 % at 130-192 rows,
    // beam search 5 x 128 +5 %.  (Two such tiles per CU, 512 tiles of 4 heads at 256 rows, were slower: 22.2 us -- every row's encoder
    // rows cross the CU's L2 port twice.)  The wave count changes the order in which a row's key tiles are merged: low bits differ from the
    // 8-wave tile's, within the same bound against the reference.
    static constexpr bool lat_nw4 = sizeof(T) == 2;
    // per-row stop (step.h): batch row held by every slot of a row range, scratch of the compaction, {live rows, moves} per range
    int *row_map = nullptr, *row_map2 = nullptr, *cmoves = nullptr, *cinfo = nullptr; int64_t* cur_tok2 = nullptr;
    int last_compactions = 0;         // compactions of the last generate (TXO_Q_LAST_COMPACTIONS)
    // ragged batches (texocr.h: txo_encode_ragged ...): per-image sizes in engine-owned buffers.  rag_hw [Bmax][2] patch rows / columns and
    // rag_ntok [Bmax] encoder tokens of the last ragged encode; slens [Bmax] cross-attention keys per decode SLOT of a ragged session
    // (permuted with the rows by compact_lane), slens2 its scratch.  rag_host: pinned staging of the caller's host arrays, rag_ev: its last copy.
    int *rag_hw = nullptr, *rag_ntok = nullptr, *slens = nullptr, *slens2 = nullptr;
    int32_t* rag_host = nullptr; hipEvent_t rag_ev = nullptr; bool rag_ev_pending = false;
    std::vector<int32_t> rag_stage;   // host scratch [3 Bmax] (sized at creation)
    bool last_ragged = false;         // TXO_Q_LAST_RAGGED
    // device-side image ingest (ingest.h): the descriptors [Bmax] of the list on the device, their pinned staging, its last copy
    IngestDesc *ing_desc = nullptr, *ing_host = nullptr; hipEvent_t ing_ev = nullptr; bool ing_ev_pending = false;
    // fit-to-canvas ingest (ingest_fit.h): FitDesc [Bmax] followed by the list int [Bmax] of the images that need a horizontal pass; staged like ing_host
    char *fit_dev = nullptr, *fit_host = nullptr;
    // trim-to-ink ingest (ingest_trim.h): the ink extents int [Bmax][4] on the device and where they are copied back to (pinned)
    int *trim_rec = nullptr, *trim_host = nullptr;
    size_t fit_bytes(int B) const { return (sizeof(FitDesc) + sizeof(int)) * (size_t)B; }
    int rag_box[2] = {0, 0};          // the smallest H x W (multiples of 16) that holds every image of the last ragged batch
    // rag_fwd off (the default): these calls answer as they did before the forward had a ragged form
    int refuse_ragged_forward(const std::string& call) const {
        return fail(TXO_E_INVALID, call + ": not available on a ragged batch session unless txo_set_ragged_forward(e, 1) is in effect");
    }
    Stamps stamps;                    // TXO_STAMPS / TXO_PSTAMPS diagnostics (stamps.h)
    int64_t* tok_buf = nullptr;            // [Bmax][Tmax] generated ids (engine-owned so graphs do not bake user pointers)
    float* logp_buf = nullptr;             // [Bmax][Tmax] their log-probabilities, for a captured step that carries them (generate_impl)
    // prompted decode (step_prefix.h): the caller's prefix [Bmax][Tmax] with ids forced into the vocabulary, its per-row lengths [Bmax], and the forced
    // tokens' log-probabilities [Bmax][Tmax] -- engine-owned, so that a captured step can carry them
    int64_t* ftab = nullptr; int* flen = nullptr; float* fplogp = nullptr;
    int prefix_cols = 0;                   // StepArgs::out_cols of the running prompted decode
    // alternatives (step_alts.h): [Bmax][Tmax][k] ids and log-probabilities of the running / last decode, k = ses.alts / last_alts (room for
    // ALTS_MAX) -- engine-owned, so that a captured step can carry them; allocated at the first use
    int32_t* alt_ids = nullptr; float* alt_logp = nullptr;
    // constrained decode (step_rules.h): the packed table [RULES_MAX_STATES][V], every row's (state, depth) [Bmax] and the state behind every
    // position [Bmax][Tmax] -- engine-owned, so that a captured step can carry them
    int* rules_dev = nullptr; int2* rule_state = nullptr; int2* rule_hist = nullptr;
    // closing decode (txo_set_rules_close): the host copy of the installed table (the switch may come after the rules), the distance table on
    // the device, and every row's (end position, has committed eos) [Bmax]
    std::vector<int32_t> rules_host; CloseTable* close_dev = nullptr; int2* rule_close = nullptr;
    Session ses;                           // the open decode session (session.h)
    // persistent decode launch (persist.h): control block (device + pinned host copy), per-stage stamps of one position
    PersistCtl* pctl = nullptr; PersistCtl* pctl_host = nullptr; unsigned long long* pstamps = nullptr;
    int persist_fallbacks = 0;                            // launches that gave up (placement / time-out) and were redone with launches
    int persist_strikes = 0, persist_cooldown = 0;        // two give-ups in a row switch the fast path off for 64 generates (then it is tried again)
    bool last_persist = false;                            // the last generate() ran as ONE persistent launch
    int last_ranges = 1;                                  // row ranges (streams) the last launch-path decode ran on
    // beam search state (rows = images * beams)
    float* bscore = nullptr; int* bfin = nullptr; short* bpath[2] = {nullptr, nullptr}; short* bparent = nullptr; int* btok = nullptr;
    float* blogp = nullptr;                // [Tmax][Bmax] beside btok: the selected candidates' increments (txo_beam_search with logp)
    int2* brule_state = nullptr;           // [Bmax] constrained beam search (beam_rules.h): the (state, depth) of every (image, beam) slot
    // logp: the step also records blogp; ruled: beam_rules.h's selection; closing: its closing form over `positions` positions
    struct BeamCtx { int k; const short* path_cur; short* path_nxt; bool logp = false; bool ruled = false; bool closing = false; int positions = 0; int guard_p = 0, guard_r = 0; };
    // ----- profiling -----
    bool prof = false;                // full: per-launch cross-attention events + markers around every encode and step
    bool prof_cross = false;          // light: only the cross-attention dispatches carry events (no extra packets)
    bool prof_persist = false;        // mode 3: HIP events bound to the persistent decode launch (texocr_amd/csrc/persist.h)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_persist;
    unsigned cross_seq = 0;
    EventPool pool;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_cross, ev_enc, ev_step, ev_ingest;

    int D, Ie, Id, Fe, Fd, V, Tmax, Nmax, Bmax;

    ~Engine() override {
        if (pctl_host) (void)hipHostFree(pctl_host);
        if (rag_host) (void)hipHostFree(rag_host);
        if (rag_ev) (void)hipEventDestroy(rag_ev);
        if (ing_host) (void)hipHostFree(ing_host);
        if (fit_host) (void)hipHostFree(fit_host);
        if (trim_host) (void)hipHostFree(trim_host);
        if (ing_ev) (void)hipEventDestroy(ing_ev);
        for (void* p : allocs) (void)hipFree(p);
    }

    // All device memory of the engine comes from two arenas (workspace at create, weights at finalize), one hipMalloc
    // each: a decode step touches ~40 small buffers and every launch starts with cold caches, so sharing large pages keeps
    // address-translation misses off the operand round trip each dependent launch already pays.
    struct Arena { char* base = nullptr; size_t cap = 0, off = 0; bool measuring = false; };
    Arena arena;
    template <typename U> int dalloc(U** p, size_t n) {
        const size_t bytes = (n * sizeof(U) + 511) & ~(size_t)255;
        if (arena.measuring) { arena.off += bytes; *p = nullptr; return 0; }
        if (arena.base && arena.off + bytes <= arena.cap) {
            *p = reinterpret_cast<U*>(arena.base + arena.off);
            arena.off += bytes;
            return 0;
        }
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, bytes));
        allocs.push_back(q);
        *p = reinterpret_cast<U*>(q);
        return 0;
    }
    int arena_begin(size_t bytes) {
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, bytes + (2u << 20)));
        allocs.push_back(q);
        arena = Arena{};
        arena.base = reinterpret_cast<char*>(((uintptr_t)q + (2u << 20) - 1) & ~(uintptr_t)((2u << 20) - 1));   // 2 MiB aligned
        arena.cap = bytes;
        return 0;
    }
    int upload_f32(float** dst, const std::vector<float>& v) {
        if (int r = dalloc(dst, v.size())) return r;
        HIP_TRY(hipMemcpy(*dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    }
    int upload_T(T** dst, const std::vector<float>& v) { return upload_as<T>(dst, v); }
    template <typename TB> int upload_as(TB** dst, const std::vector<float>& v) {
        if (int r = dalloc(dst, v.size())) return r;
        if constexpr (sizeof(TB) == 4) {
            HIP_TRY(hipMemcpy(*dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
        } else {
            std::vector<uint16_t> h(v.size());
            for (size_t i = 0; i < v.size(); ++i) {      // round-to-nearest-even f32 -> bf16 (inputs are finite)
                uint32_t u; memcpy(&u, &v[i], 4);
                h[i] = (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
            }
            HIP_TRY(hipMemcpy(*dst, h.data(), h.size() * 2, hipMemcpyHostToDevice));
        }
        return 0;
    }

    const HostTensor* get(const std::string& key, std::initializer_list<int64_t> shape) {
        auto it = host.find(key);
        if (it == host.end()) { g_err = "missing weight: " + key; return nullptr; }
        if (it->second.shape != std::vector<int64_t>(shape)) { g_err = "wrong shape for " + key; return nullptr; }
        return &it->second;
    }

    // shared LayerNorm of a stack: every alias layers.{s}.0.* that was provided must be identical
    int shared_ln(const std::string& prefix, int n_sub, float** g, float** b) {
        const HostTensor* g0 = get(prefix + ".layers.0.0.weight", {D});
        const HostTensor* b0 = get(prefix + ".layers.0.0.bias", {D});
        if (!g0 || !b0) return TXO_E_STATE;
        for (int s = 1; s < n_sub; ++s)
            for (const char* leaf : {"weight", "bias"}) {
                auto it = host.find(prefix + ".layers." + std::to_string(s) + ".0." + leaf);
                if (it == host.end()) continue;
                const HostTensor& ref = (leaf[0] == 'w') ? *g0 : *b0;
                if (it->second.data != ref.data)
                    return fail(TXO_E_INVALID, prefix + ".layers." + std::to_string(s) + ".0." + leaf +
                                " differs from layers.0.0: the reference shares ONE LayerNorm per stack");
            }
        if (int r = upload_f32(g, g0->data)) return r;
        return upload_f32(b, b0->data);
    }

    // inner == 2 D (config.yml dims: 8 heads of 64 at width 256): the latent form's two per-head projections fold into their neighbours at
    // load time (products in double, rounded once to the storage type) and an attention sub-layer is THREE launches instead of five:
    //   q'[h*D + d'] = sum_d z[d] * M[h*D + d'][d],   M = 0.125 Wk_h^T Wq_h            (in the LN-prologue GEMM, N = heads*D)
    //   y[n]         = sum_{h,d} c[h*D + d] * Wo'[n][h*D + d],  Wo' = Wo[:, h] Wv_h     (in the gated output projection, K = heads*D)
    // (attention.py:124-127,148,166,172-173: k and v are linear images of the SAME D-element row -- the raw encoder row in the cross
    // attention, the normalised block input in the self attention, attention.py:114-116)
    int fold_latent(const HostTensor* q, const HostTensor* k, const HostTensor* v, const HostTensor* wo, int inner, AttnW* w, int G) {
        const int H = inner / DH, HD = H * D;
        std::vector<float> M((size_t)HD * D), WoF((size_t)2 * D * HD);
        std::vector<double> acc(std::max(D, HD));
        for (int h = 0; h < H; ++h)
            for (int d1 = 0; d1 < D; ++d1) {
                std::fill(acc.begin(), acc.begin() + D, 0.0);
                for (int j = 0; j < DH; ++j) {
                    const double kk = (double)ATTN_SCALE * k->data[((size_t)h * DH + j) * D + d1];
                    const float* qr = &q->data[((size_t)h * DH + j) * D];
                    for (int d = 0; d < D; ++d) acc[d] += kk * qr[d];
                }
                for (int d = 0; d < D; ++d) M[((size_t)h * D + d1) * D + d] = (float)acc[d];
            }
        for (int n = 0; n < 2 * D; ++n) {
            std::fill(acc.begin(), acc.begin() + HD, 0.0);
            for (int f = 0; f < inner; ++f) {
                const double wn = wo->data[(size_t)n * inner + f];
                const float* vr = &v->data[(size_t)f * D];
                double* dst = &acc[(size_t)(f / DH) * D];
                for (int d = 0; d < D; ++d) dst[d] += wn * vr[d];
            }
            for (int c2 = 0; c2 < HD; ++c2) WoF[(size_t)n * HD + c2] = (float)acc[c2];
        }
        if (int r = upload_T(&w->wqp, M)) return r;
        return upload_T(&w->wo_f, interleave(WoF, D, HD, G));
    }

    int load_attn(const std::string& p, int inner, bool cross, AttnW* w, std::vector<float>* kv_concat, int G) {
        const HostTensor *q = get(p + ".q.weight", {inner, D}), *k = get(p + ".k.weight", {inner, D}),
                         *v = get(p + ".v.weight", {inner, D}), *wo = get(p + ".fc_out.0.weight", {2 * D, inner}),
                         *bo = get(p + ".fc_out.0.bias", {2 * D});
        if (!q || !k || !v || !wo || !bo) return TXO_E_STATE;
        if (cross) {
            if (int r = upload_T(&w->wq, q->data)) return r;
            kv_concat->insert(kv_concat->end(), k->data.begin(), k->data.end());
            kv_concat->insert(kv_concat->end(), v->data.begin(), v->data.end());
            // latent form: q'_h = 0.125 Wk_h^T q_h is a per-head GEMM whose weight rows are COLUMNS of Wk_h -> stored transposed per head, [heads][D][64]
            std::vector<float> kT((size_t)inner * D);
            for (int h = 0; h < inner / DH; ++h)
                for (int d = 0; d < D; ++d)
                    for (int j = 0; j < DH; ++j) kT[((size_t)h * D + d) * DH + j] = ATTN_SCALE * k->data[((size_t)h * DH + j) * D + d];   // (0.125: exact)
            if (int r = upload_T(&w->wkT, kT)) return r;
            if (int r = upload_T(&w->wv, v->data)) return r;
            if (latent_fold()) { if (int r = fold_latent(q, k, v, wo, inner, w, G)) return r; }
        } else {
            std::vector<float> cat(q->data);
            cat.insert(cat.end(), k->data.begin(), k->data.end());
            cat.insert(cat.end(), v->data.begin(), v->data.end());
            if (int r = upload_T(&w->wqkv, cat)) return r;
            // decoder self attention in latent form (r05): the same two folds, against the history of normalised block inputs
            // (opt-in, TXO_LATENT_SELF=1: without it neither the fold nor the z history exists)
            if (G == 8 && latent_fold() && knobs.lat_self_env != 0) { if (int r = fold_latent(q, k, v, wo, inner, w, G)) return r; }
        }
        if (int r = upload_T(&w->wo, interleave(wo->data, D, inner, G))) return r;
        if (G != 16) {                                        // decoder: the prefill runs these projections on the encoder-side GEMMs
            if (int r = upload_T(&w->wo16, interleave(wo->data, D, inner, 16))) return r;
            if (int r = upload_f32(&w->bo16, interleave(bo->data, D, 1, 16))) return r;
        }
        return upload_f32(&w->bo, interleave(bo->data, D, 1, G));
    }
    int load_mlp(const std::string& p, int F, MlpW* w, int G) {
        const HostTensor *w1 = get(p + ".fc_in.fc.weight", {2 * F, D}), *b1 = get(p + ".fc_in.fc.bias", {2 * F}),
                         *w2 = get(p + ".fc_out.weight", {D, F}), *b2 = get(p + ".fc_out.bias", {D});
        if (!w1 || !b1 || !w2 || !b2) return TXO_E_STATE;
        if (int r = upload_T(&w->w1, interleave(w1->data, F, D, G))) return r;
        if (int r = upload_f32(&w->b1, interleave(b1->data, F, 1, G))) return r;
        if (int r = upload_T(&w->w2, w2->data)) return r;
        if (G == 8) {       // decoder: the prefill's FFN-in; also enqueue_step: FFN-in of wide bf16 decoders at >= 128 rows goes through the large-GEMM kernel
            if (int r = upload_T(&w->w1_16, interleave(w1->data, F, D, 16))) return r;
            if (int r = upload_f32(&w->b1_16, interleave(b1->data, F, 1, 16))) return r;
        }
        return upload_f32(&w->b2, b2->data);
    }

    // StdConv2d weight standardisation (resnet.py:58-61): per output channel over (ic, kh, kw), biased variance,
    // eps 1e-6 inside the sqrt (F.batch_norm, training=True).  Input-independent, so folded at load time; the result
    // is stored [oc][kh][kw][ic] (K order of the implicit-GEMM loader).  kpad > 0 pads K with zeros (stem: 49 -> 64).
    template <typename TB> int upload_conv(TB** dst, const HostTensor& w, int kpad) {
        const int oc = (int)w.shape[0], ic = (int)w.shape[1], kh = (int)w.shape[2], kw = (int)w.shape[3];
        const int k = ic * kh * kw, kk = kpad > 0 ? kpad : k;
        std::vector<float> o((size_t)oc * kk, 0.f);
        for (int n = 0; n < oc; ++n) {
            const float* src = &w.data[(size_t)n * k];
            double m = 0, v = 0;
            for (int i = 0; i < k; ++i) m += src[i];
            m /= k;
            for (int i = 0; i < k; ++i) v += (src[i] - m) * (src[i] - m);
            const double rs = 1.0 / std::sqrt(v / k + 1e-6);
            for (int c2 = 0; c2 < ic; ++c2)
                for (int y = 0; y < kh; ++y)
                    for (int x = 0; x < kw; ++x)
                        o[(size_t)n * kk + ((size_t)y * kw + x) * ic + c2] = (float)((src[((size_t)c2 * kh + y) * kw + x] - m) * rs);
        }
        return upload_as<TB>(dst, o);
    }
    int load_gn(const std::string& p, int ch, GnW* g) {
        const HostTensor *w = get(p + ".weight", {ch}), *b = get(p + ".bias", {ch});
        if (!w || !b) return TXO_E_STATE;
        if (int r = upload_f32(&g->g, w->data)) return r;
        return upload_f32(&g->b, b->data);
    }
    template <typename TB> int load_backbone(const std::string& p, Backbone<TB>& k) {
        const HostTensor* t;
        if (!(t = get(p + ".stem.0.weight", {64, 1, 7, 7}))) return TXO_E_STATE;
        if (int r = upload_conv(&k.stem_w, *t, 64)) return r;
        if (int r = load_gn(p + ".stem.1", 64, &k.stem_gn)) return r;
        static const int depths[3] = {2, 4, 6}, chans[3] = {256, 512, 1024};
        int prev = 64;
        for (int st = 0; st < 3; ++st)
            for (int i = 0; i < depths[st]; ++i) {
                BlockW<TB> b{};
                b.cin = prev; b.cout = chans[st]; b.mid = chans[st] / 4; b.stride = (i == 0 && st > 0) ? 2 : 1; b.has_ds = i == 0;
                const std::string q = p + ".stages." + std::to_string(st) + ".stage_blocks." + std::to_string(i);
                // every layer is registered twice (block_list.N and block.N, resnet.py:132-141); if both are given they must agree
                for (int j = 0; j < 6; ++j)
                    for (const char* leaf : {".weight", ".bias"}) {
                        auto a = host.find(q + ".block_list." + std::to_string(j) + leaf), c2 = host.find(q + ".block." + std::to_string(j) + leaf);
                        if (a != host.end() && c2 != host.end() && a->second.data != c2->second.data)
                            return fail(TXO_E_INVALID, q + ".block." + std::to_string(j) + leaf + " differs from its block_list alias");
                    }
                if (b.has_ds) {
                    if (!(t = get(q + ".downsample.conv.weight", {b.cout, b.cin, 1, 1}))) return TXO_E_STATE;
                    if (int r = upload_conv(&b.ds, *t, 0)) return r;
                    if (int r = load_gn(q + ".downsample.norm", b.cout, &b.nds)) return r;
                }
                if (!(t = get(q + ".block_list.0.weight", {b.mid, b.cin, 1, 1}))) return TXO_E_STATE;
                if (int r = upload_conv(&b.c1, *t, 0)) return r;
                if (int r = load_gn(q + ".block_list.1", b.mid, &b.n1)) return r;
                if (!(t = get(q + ".block_list.2.weight", {b.mid, b.mid, 3, 3}))) return TXO_E_STATE;
                if (int r = upload_conv(&b.c2, *t, 0)) return r;
                if (int r = load_gn(q + ".block_list.3", b.mid, &b.n2)) return r;
                if (!(t = get(q + ".block_list.4.weight", {b.cout, b.mid, 1, 1}))) return TXO_E_STATE;
                if (int r = upload_conv(&b.c3, *t, 0)) return r;
                if (int r = load_gn(q + ".block_list.5", b.cout, &b.n3)) return r;
                k.blocks.push_back(b);
                prev = b.cout;
            }
        return 0;
    }

    int finalize() override {
        if (ready) return fail(TXO_E_STATE, "weights already finalized");
        const txo_config& c = cfg;
        // non-finite weights are refused: the library is built with -fno-honor-nans (build.py), and a NaN / inf in a weight would reach
        // every row of every batch.  (Non-finite PIXELS reach only their own image's rows: txo_encode's contract.)
        for (auto& kv : host)
            for (float v : kv.second.data)
                if (!std::isfinite(v)) return fail(TXO_E_INVALID, "non-finite value in weight " + kv.first);
        {   // weights arena: fp32 size of everything handed in is an upper bound for both storage types
            size_t bytes = 0;
            for (auto& kv : host) bytes += kv.second.data.size() * sizeof(float) + 512;
            // + the decoder's second (16-interleaved) copies of the gated projections for the prefill
            bytes += (size_t)cfg.dec_layers * ((size_t)2 * 2 * D * Id + (size_t)2 * Fd * D + 4 * D + 2 * Fd + 4096) * sizeof(float);
            // + the latent form's copies of the cross-attention Wk (transposed per head) and Wv, and the folded pair where inner == 2 D
            bytes += (size_t)cfg.dec_layers * ((size_t)2 * D * Id + 1024) * sizeof(float);
            if (latent_fold()) bytes += (size_t)cfg.dec_layers * ((size_t)3 * cfg.dec_heads * D * D + 1024) * sizeof(float);
            if (int r = arena_begin(bytes + (1u << 20))) return r;
        }
        const int npos = 1 + (c.canvas_h / 16) * (c.canvas_w / 16);
        const HostTensor *t;
        if (!(t = get("encoder.cls_token", {1, 1, D}))) return TXO_E_STATE;
        if (int r = upload_f32(&cls, t->data)) return r;
        if (!(t = get("encoder.pos_embed", {1, npos, D}))) return TXO_E_STATE;
        if (int r = upload_f32(&pos, t->data)) return r;
        if (!hybrid) {
            if (!(t = get("encoder.patch_embed.proj.weight", {D, c.in_channels, 16, 16}))) return TXO_E_STATE;
            if (int r = upload_T(&patch_w, t->data)) return r;
        } else {
            if (!(t = get("encoder.patch_embed.proj.weight", {D, 1024, 1, 1}))) return TXO_E_STATE;
            if (bk_fp32) {
                if (int r = load_backbone("encoder.patch_embed.backbone_net", bk32)) return r;
                if (int r = upload_as<float>(&bk32.proj_w, t->data)) return r;
            } else {
                if (int r = load_backbone("encoder.patch_embed.backbone_net", bk)) return r;
                if (int r = upload_T(&patch_w, t->data)) return r;
            }
        }
        if (!(t = get("encoder.patch_embed.proj.bias", {D}))) return TXO_E_STATE;
        if (int r = upload_f32(&patch_b, t->data)) return r;
        if (int r = shared_ln("encoder.attn_layers", 2 * c.enc_layers, &enc_g, &enc_b)) return r;
        {
            std::vector<float> gb(get("encoder.attn_layers.layers.0.0.weight", {D})->data);
            const std::vector<float>& bb = get("encoder.attn_layers.layers.0.0.bias", {D})->data;
            gb.insert(gb.end(), bb.begin(), bb.end());
            if (int r = upload_f32(&enc_gb, gb)) return r;
        }
        enc_attn.resize(c.enc_layers); enc_mlp.resize(c.enc_layers);
        for (int l = 0; l < c.enc_layers; ++l) {
            const std::string p = "encoder.attn_layers.layers.";
            if (int r = load_attn(p + std::to_string(2 * l) + ".1", Ie, false, &enc_attn[l], nullptr, 16)) return r;
            if (int r = load_mlp(p + std::to_string(2 * l + 1) + ".1", Fe, &enc_mlp[l], 16)) return r;
        }
        if (!(t = get("encoder.norm.weight", {D}))) return TXO_E_STATE;
        if (int r = upload_f32(&encn_g, t->data)) return r;
        if (!(t = get("encoder.norm.bias", {D}))) return TXO_E_STATE;
        if (int r = upload_f32(&encn_b, t->data)) return r;

        if (!(t = get("decoder.net.token_embedding.weight", {V, D}))) return TXO_E_STATE;
        if (int r = upload_f32(&tok_emb, t->data)) return r;
        if (!(t = get("decoder.net.pos_embedding.embedding.weight", {Tmax, D}))) return TXO_E_STATE;
        if (int r = upload_f32(&pos_emb, t->data)) return r;
        if (int r = shared_ln("decoder.net.attn_layers", 3 * c.dec_layers, &dec_g, &dec_b)) return r;
        {
            std::vector<float> gb(get("decoder.net.attn_layers.layers.0.0.weight", {D})->data);
            const std::vector<float>& bb = get("decoder.net.attn_layers.layers.0.0.bias", {D})->data;
            gb.insert(gb.end(), bb.begin(), bb.end());
            if (int r = upload_f32(&dec_gb, gb)) return r;
        }
        dec_self.resize(c.dec_layers); dec_cross.resize(c.dec_layers); dec_mlp.resize(c.dec_layers);
        std::vector<float> kv_concat;
        for (int l = 0; l < c.dec_layers; ++l) {
            const std::string p = "decoder.net.attn_layers.layers.";
            if (int r = load_attn(p + std::to_string(3 * l) + ".1", Id, false, &dec_self[l], nullptr, 8)) return r;
            if (int r = load_attn(p + std::to_string(3 * l + 1) + ".1", Id, true, &dec_cross[l], &kv_concat, 8)) return r;
            if (int r = load_mlp(p + std::to_string(3 * l + 2) + ".1", Fd, &dec_mlp[l], 8)) return r;
        }
        if (int r = upload_T(&wckv, kv_concat)) return r;
        if (!(t = get("decoder.net.norm.weight", {D}))) return TXO_E_STATE;
        if (int r = upload_f32(&decn_g, t->data)) return r;
        if (!(t = get("decoder.net.norm.bias", {D}))) return TXO_E_STATE;
        if (int r = upload_f32(&decn_b, t->data)) return r;
        if (!(t = get("decoder.net.to_logits.weight", {V, D}))) return TXO_E_STATE;
        if (int r = upload_T(&wlog, t->data)) return r;
        if (!(t = get("decoder.net.to_logits.bias", {V}))) return TXO_E_STATE;
        if (int r = upload_f32(&blog, t->data)) return r;
        host.clear();
        if (knobs.w_tiled_on) {    // tiled copies of every weight the decode-step projections read (dec_gemm.h: w_tiled)
            HIP_TRY(hipDeviceSynchronize());
            const int H = c.dec_heads;
            for (int l = 0; l < c.dec_layers; ++l) {
                want_tiled(dec_self[l].wqkv, 3 * Id, D); want_tiled(dec_self[l].wo, 2 * D, Id);
                want_tiled(dec_self[l].wqp, H * D, D); want_tiled(dec_self[l].wo_f, 2 * D, H * D);
                want_tiled(dec_cross[l].wq, Id, D); want_tiled(dec_cross[l].wo, 2 * D, Id);
                want_tiled(dec_cross[l].wqp, H * D, D); want_tiled(dec_cross[l].wo_f, 2 * D, H * D);
                want_tiled(dec_mlp[l].w1, 2 * Fd, D); want_tiled(dec_mlp[l].w2, D, Fd);
            }
            want_tiled(wlog, V, D);
            if (int r = make_tiled_all()) return r;
        }
        ready = true;
        return 0;
    }

    int init() {
        arena = Arena{}; arena.measuring = true;
        if (int r = init_buffers()) return r;                 // pass 1: sizes only
        if (int r = arena_begin(arena.off)) return r;
        if (int r = init_buffers()) return r;                 // pass 2: carve
        HIP_TRY(hipMemset(st, 0, sizeof(StepState) * MAXL));
        // the self-attention cache starts as zeros: clamped loads may touch rows no step has written yet (fused self-attention
        // at t = 0 multiplies such a row by p = 0, which must not meet NaN/Inf bit patterns of recycled memory)
        HIP_TRY(hipMemset(skv, 0, sizeof(T) * (size_t)cfg.dec_layers * 2 * Bmax * Id * Tmax));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&pctl_host), sizeof(PersistCtl), hipHostMallocDefault));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&rag_host), sizeof(int32_t) * 3 * (size_t)Bmax, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&rag_ev, hipEventDisableTiming));
        rag_stage.assign((size_t)3 * Bmax, 0);
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&ing_host), sizeof(IngestDesc) * (size_t)Bmax, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&ing_ev, hipEventDisableTiming));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&fit_host), fit_bytes(Bmax), hipHostMallocDefault));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&trim_host), sizeof(int) * 4 * (size_t)Bmax, hipHostMallocDefault));
        return lanes.init(Tmax);
    }
    int init_buffers() {
        const txo_config& c = cfg;
        D = c.embed_dim; Ie = c.enc_heads * DH; Id = c.dec_heads * DH; Fe = c.enc_exp * D; Fd = c.dec_exp * D;
        V = c.vocab; Tmax = c.max_len; Bmax = c.max_batch;
        hybrid = c.embed == TXO_EMBED_HYBRID;
        {
            int dev = 0; hipDeviceProp_t prop;
            if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) {
                if (prop.multiProcessorCount > 0) n_cus = prop.multiProcessorCount;
                if (prop.sharedMemPerBlock > 0) sample_lds_max = prop.sharedMemPerBlock;
            }
            // the LDS-form sampler (step.h: sample_step_kernel<false>) stages a whole row, V * 4 bytes: beyond 64 KB it needs the opt-in,
            // and a refusal leaves it at 64 KB.  A larger vocabulary is refused by txo_set_sampling, never a failed launch mid-decode
            if (sample_lds_max > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_step_kernel<false>),
                                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)sample_lds_max) != hipSuccess) {
                (void)hipGetLastError(); sample_lds_max = 65536;
            }
            if (sample_lds_max > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_prefix_step_kernel<false>),   // (its prompted form)
                                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)sample_lds_max) != hipSuccess) {
                (void)hipGetLastError(); sample_lds_max = 65536;
            }
        }
        {
            bool exists = (D == 64 && la_supported<T, 64>()) || (D == 256 && la_supported<T, 256>()) || (D == 768 && la_supported<T, 768>());
            // the tile needs up to 145 KB of dynamic LDS: the opt-in is asked for HERE, and a refusal switches the latent form off for this
            // engine (every decode then takes the K/V form) instead of surfacing as a failed launch in the middle of a generate
            auto opt_in = [&](const void* kern, size_t lds) {
                if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { (void)hipGetLastError(); exists = false; }
            };
            if (exists) {
                if constexpr (la_supported<T, 64>()) { if (D == 64) opt_in(reinterpret_cast<const void*>(&lat_core_kernel<T, 64>), la_lds_bytes<T, 64>()); }
                if constexpr (la_supported<T, 256>()) { if (D == 256) opt_in(reinterpret_cast<const void*>(&lat_core_kernel<T, 256>), la_lds_bytes<T, 256>()); }
                if constexpr (la_supported<T, 256>() && sizeof(T) == 2) { if (D == 256) opt_in(reinterpret_cast<const void*>(&lat_core_kernel<T, 256, 4>), la_lds_bytes<T, 256, 4>()); }
                if constexpr (la_supported<T, 768>()) { if (D == 768) opt_in(reinterpret_cast<const void*>(&lat_core_kernel<T, 768>), la_lds_bytes<T, 768>()); }
            }
            latent_ok = exists;
        }
        Nmax = c.max_tokens > 0 ? c.max_tokens : 1 + (c.canvas_h / 16) * (c.canvas_w / 16);
        const size_t M = (size_t)Bmax * Nmax;
        const int Imax = Ie > Id ? Ie : Id, Fmax = Fe > Fd ? Fe : Fd;
        if (hybrid) {
            // largest NHWC activation per image: stem output (H/2 x W/2 x 64) = stage-0 output (H/4 x W/4 x 256) = 4096 per token
            const size_t E = (size_t)Bmax * (Nmax - 1) * 4096;
            if (bk_fp32) {
                for (auto& a : bk32.act) if (int r = dalloc(&a, E)) return r;
                // GroupNorm partial sums per 128-row output tile of the split convolutions: the stem's output is the largest (H/2 x W/2 pixels)
                const size_t rows = (size_t)Bmax * ((c.canvas_h + 1) / 2) * ((c.canvas_w + 1) / 2);
                if (int r = dalloc(&gn_tiles, (rows / GB_BM + 2) * 2 * 2 * 32 * 2)) return r;
            }
            else { for (auto& a : bk.act) if (int r = dalloc(&a, E)) return r; }
            if (int r = dalloc(&gn_partial, (size_t)Bmax * 64 * 64)) return r;
            if (int r = dalloc(&gn_stats, (size_t)Bmax * 64)) return r;
        }
        if (int r = dalloc(&ex, M * D)) return r;
        if (int r = dalloc(&estats, M * 2)) return r;
        if (int r = dalloc(&ey, M * D)) return r;
        if (int r = dalloc(&ez, M * D)) return r;
        if (int r = dalloc(&eenc, M * D)) return r;
        if (int r = dalloc(&enc_t, M * D)) return r;
        // (the prefill of the decoder runs in the encoder's workspace: sized for the wider of the two stacks)
        if (int r = dalloc(&eqkv, 3 * M * Imax)) return r;
        if (int r = dalloc(&eao, M * Imax)) return r;
        if (int r = dalloc(&ehid, M * Fmax)) return r;
        if (int r = dalloc(&ckv, (size_t)c.dec_layers * 2 * M * Id)) return r;
        if (int r = dalloc(&skv, (size_t)c.dec_layers * 2 * Bmax * Id * Tmax)) return r;
        if (int r = dalloc(&dx, (size_t)Bmax * D)) return r;
        if (int r = dalloc(&dy, (size_t)Bmax * D)) return r;
        if (int r = dalloc(&dq, (size_t)Bmax * Imax)) return r;
        if (int r = dalloc(&dao, (size_t)Bmax * Imax)) return r;
        if (int r = dalloc(&dhid, (size_t)Bmax * Fmax)) return r;
        if (int r = dalloc(&dz, (size_t)Bmax * D)) return r;
        if (int r = dalloc(&dqt, (size_t)Bmax * Imax)) return r;
        if (knobs.lat_self_env != 0) { if (int r = dalloc(&zc, (size_t)c.dec_layers * Bmax * Tmax * D)) return r; }   // z history of the opt-in latent self attention
        if (int r = dalloc(&dqp, (size_t)Bmax * c.dec_heads * D)) return r;
        // (+ tile alignment of the row ranges' regions: range li starts at ceil16(b0) + 16 li and spans ceil16(nb) rows -- beam ranges are not
        // multiples of 16 -- so the last of MAXL ranges can end at Bmax + 30 + 16 (MAXL - 1))
        if (int r = dalloc(&dcl, ((size_t)Bmax + 16 * MAXL + 32) * c.dec_heads * D)) return r;
        if (int r = dalloc(&dlogits, (size_t)Bmax * V)) return r;
        if (int r = dalloc(&cur_tok, (size_t)Bmax)) return r;
        if (int r = dalloc(&eos_seen, (size_t)Bmax)) return r;
        if (int r = dalloc(&row_map, (size_t)Bmax)) return r;
        if (int r = dalloc(&row_map2, (size_t)Bmax)) return r;
        if (int r = dalloc(&cur_tok2, (size_t)Bmax)) return r;
        if (int r = dalloc(&rag_hw, (size_t)2 * Bmax)) return r;
        if (int r = dalloc(&rag_ntok, (size_t)Bmax)) return r;
        if (int r = dalloc(&slens, (size_t)Bmax)) return r;
        if (int r = dalloc(&slens2, (size_t)Bmax)) return r;
        if (int r = dalloc(&cmoves, (size_t)2 * Bmax)) return r;
        if (int r = dalloc(&cinfo, (size_t)2 * MAXL)) return r;
        if (int r = dalloc(&kmask, (size_t)Bmax * Tmax)) return r;
        if (int r = dalloc(&done_flag, (size_t)Tmax * MAXL)) return r;
        if (int r = dalloc(&st, MAXL)) return r;
        if (int r = dalloc(&tok_buf, (size_t)Bmax * Tmax)) return r;
        if (int r = dalloc(&logp_buf, (size_t)Bmax * Tmax)) return r;
        if (int r = dalloc(&ftab, (size_t)Bmax * Tmax)) return r;
        if (int r = dalloc(&flen, (size_t)Bmax)) return r;
        if (int r = dalloc(&fplogp, (size_t)Bmax * Tmax)) return r;
        if (int r = dalloc(&bscore, (size_t)Bmax)) return r;
        if (int r = dalloc(&bfin, (size_t)Bmax)) return r;
        if (int r = dalloc(&bpath[0], (size_t)Bmax * Tmax)) return r;
        if (int r = dalloc(&bpath[1], (size_t)Bmax * Tmax)) return r;
        if (int r = dalloc(&bparent, (size_t)Bmax * Tmax)) return r;
        if (int r = dalloc(&btok, (size_t)Bmax * Tmax)) return r;
        if (int r = dalloc(&blogp, (size_t)Bmax * Tmax)) return r;
        if (int r = dalloc(&pctl, 1)) return r;
        if (int r = dalloc(&pstamps, (size_t)PS_TEAMS * PS_STAMP_RANKS * PS_MAX_STAGES * PS_STAMP_WORDS)) return r;
        if (int r = dalloc(&ing_desc, (size_t)Bmax)) return r;   // (last: no earlier buffer moves)
        if (int r = dalloc(&fit_dev, fit_bytes(Bmax))) return r;
        if (int r = dalloc(&trim_rec, (size_t)4 * Bmax)) return r;
        if (int r = dalloc(&rules_dev, (size_t)RULES_MAX_STATES * V)) return r;
        if (int r = dalloc(&rule_state, (size_t)Bmax)) return r;
        if (int r = dalloc(&rule_hist, (size_t)Bmax * Tmax)) return r;
        if (int r = dalloc(&brule_state, (size_t)Bmax)) return r;
        if (int r = dalloc(&close_dev, (size_t)1)) return r;
        if (int r = dalloc(&rule_close, (size_t)Bmax)) return r;
        return 0;
    }

    // ------------------------------------------------------------------------------------------
    template <int MODE, typename TZ>
    void launch_ln(hipStream_t s, const float* in, float* x_out, TZ* z_out, const float* g, const float* b, int rows, int rev = 0) {
        const dim3 grid((rows + 3) / 4), blk(256);
        if (D == 256) hipLaunchKernelGGL((ln_rows_kernel<TZ, 1, MODE>), grid, blk, 0, s, in, x_out, z_out, g, b, rows, rev);
        else if (D == 512) hipLaunchKernelGGL((ln_rows_kernel<TZ, 2, MODE>), grid, blk, 0, s, in, x_out, z_out, g, b, rows, rev);
        else if (D == 768) hipLaunchKernelGGL((ln_rows_kernel<TZ, 3, MODE>), grid, blk, 0, s, in, x_out, z_out, g, b, rows, rev);
        else hipLaunchKernelGGL((ln_rows_generic_kernel<TZ, MODE>), grid, blk, 0, s, in, x_out, z_out, g, b, rows, D);
    }

    // C = A * W^T with A plain row-major [M][K]: the 256x256 LDS-DMA kernel (gemm_pp.h) for bf16 shapes it fits, else the
    // 128x128 register-staged kernel.  TXO_GEMM_OLD=1 forces the latter (tests compare the two bit for bit).
    template <class Epi>
    void gemm_plain(hipStream_t s, const T* A, const T* W, int M, int N, int K, Epi epi, int rev = 0) {
        if constexpr (sizeof(T) == 2) {
            if (knobs.use_pp && gemm_pp_fits(M, N, K)) { launch_gemm_pp(s, A, W, M, N, K, epi, knobs.pp_tr, rev, knobs.pp_sb_mb, knobs.pp_ct); return; }
        }
        launch_gemm_big<T>(s, LoadPlain<T>{A, K}, W, M, N, K, epi);
    }

    // ---- hybrid embedder: ResNetV2 [2,4,6] on NHWC activations (conv.h) -----------------------------------------
    static void same_pad(int in, int k, int stride, int* out, int* pad_lo) {   // utils.py:97-99,112-123 (TF "SAME")
        *out = (in + stride - 1) / stride;
        const int pad = std::max((*out - 1) * stride + (k - 1) + 1 - in, 0);
        *pad_lo = pad / 2;
    }
    // A ragged batch on the backbone (conv.h: the RAGGED forms): hw = the images' patch grids (rag_hw of the chunk), mul = 16 / s at the
    // resolution of the tensor in hand; H x W below is then the CONTAINER's grid at that resolution.  hw null: a fixed-shape batch.
    struct RagExt { const int* hw = nullptr; int mul = 0; };
    template <typename TB>
    void conv(hipStream_t s, const TB* in, const TB* w, TB* out, int B, int H, int W, int C, int OC, int k, int stride, RagExt rg = {}) {
        int OH, OW, pt, pl;
        same_pad(H, k, stride, &OH, &pt); same_pad(W, k, stride, &OW, &pl);
        // (ragged: the container's sides are multiples of 16 like every image's, so pt / pl are each image's own; gn_hw = 0 -- see bk_gemm)
        const int gn_in = rg.hw ? 0 : H * W, gn_out = rg.hw ? 0 : OH * OW;
        // a 1x1 stride-1 convolution on NHWC activations IS a plain row-major GEMM: [B*H*W][C] x [OC][C]^T -> (bf16 backbone) the 256x256
        // LDS-DMA kernel where the shape fits it (the bottlenecks' expanding convolutions, 256 / 512 / 1024 output channels)
        if (k == 1 && stride == 1) {
            if constexpr (std::is_same<TB, T>::value) gemm_plain(s, in, w, B * H * W, OC, C, EpiStore<T>{out, OC, nullptr});
            else bk_gemm(s, LoadPlain<TB>{in, C}, w, B * H * W, OC, C, EpiStore<TB>{out, OC, nullptr}, gn_in);
            return;
        }
        if (rg.hw) {
            LoadConv<TB, true> ld{in, rg.hw, rg.mul, H, W, C, stride, pt, pl, FastDiv(OH * OW), FastDiv(OW), FastDiv(C), FastDiv(k)};
            bk_gemm(s, ld, w, B * OH * OW, OC, k * k * C, EpiStore<TB>{out, OC, nullptr}, gn_out);
            return;
        }
        LoadConv<TB> ld{in, H, W, C, stride, pt, pl, FastDiv(OH * OW), FastDiv(OW), FastDiv(C), FastDiv(k)};
        bk_gemm(s, ld, w, B * OH * OW, OC, k * k * C, EpiStore<TB>{out, OC, nullptr}, gn_out);
    }
    // a backbone GEMM in storage type TB.  fp32 backbone INSIDE the bf16 engine: fp32 operands split onto the bf16 matrix pipe
    // (gemm_split.h: ~2^-16 per product, 5x less matrix time than exact-f32 MFMA); everything else -- the fp32 parity engine first of all --
    // the exact kernel.  TXO_BACKBONE_EXACT=1 keeps the exact-f32 kernel in the bf16 engine too (A/B, tests).
    // gn_hw > 0: the output is the input of a GroupNorm over images of gn_hw pixels -- the split kernel then leaves the norm's partial sums
    // behind (gemm_split.h: GnPart) and group_norm() skips its own pass over the tensor (gn_fused).  A RAGGED encode never asks for them
    // (gn_hw = 0 from every caller): GnPart / gn_finish_tiles_kernel assume one HW for the whole batch and at most two images per row tile,
    // and a container row tile mixes pixels inside and outside an extent.  Its statistics are the unfused, per-image ones of conv.h.
    bool gn_fused = false;
    float* gn_tiles = nullptr;        // [row tiles][2 halves][2 images][32 groups][2]
    template <typename TB, class ALoad, class Epi>
    void bk_gemm(hipStream_t s, ALoad ld, const TB* w, int M, int N, int K, Epi epi, int gn_hw = 0) {
        gn_fused = false;
        if constexpr (sizeof(TB) == 4 && sizeof(T) == 2) {
            if (!knobs.bk_exact && gemm_split_fits(K)) {
                GnPart gp{nullptr, 1, 1};
                if (gn_hw > 0 && gn_tiles && gn_fusable(gn_hw, N)) { gp = GnPart{gn_tiles, gn_hw, N / 32}; gn_fused = true; }
                launch_gemm_split(s, ld, w, M, N, K, epi, gp);
                return;
            }
        }
        launch_gemm_big<TB>(s, ld, w, M, N, K, epi);
    }
    template <bool RELU, bool RES, typename TB>
    void group_norm(hipStream_t s, const TB* x, const TB* res, TB* y, const GnW& g, int B, int HW, int C, RagExt rg = {}, int Wc = 0) {
        if (rg.hw) {                                         // HW = the container's pixels per slot, Wc its width; sizes per image on the device
            const int chunk_px = std::max(256, (HW + 63) / 64), nchunk = (HW + chunk_px - 1) / chunk_px;   // (the grid: no image has more chunks)
            hipLaunchKernelGGL((gn_partial_kernel<TB, true>), dim3(nchunk, B), dim3(256), 0, s, x, gn_partial, HW, C, 0, rg.hw, rg.mul, Wc);
            hipLaunchKernelGGL(gn_finish_kernel<true>, dim3(B), dim3(32), 0, s, gn_partial, gn_stats, nchunk, (double)(C / 32), rg.hw, rg.mul);
            const size_t nvec = (size_t)B * HW * C / Elem<TB>::PER16;
            hipLaunchKernelGGL((gn_apply_kernel<TB, RELU, RES, true>), dim3((nvec + 255) / 256), dim3(256), 0, s, x, res, y, gn_stats, g.g,
                               g.b, HW, C, nvec, rg.hw, rg.mul, Wc);
            return;
        }
        if (gn_fused) {                                      // the convolution that wrote x left the partial sums per output tile (bk_gemm)
            gn_fused = false;
            hipLaunchKernelGGL(gn_finish_tiles_kernel, dim3(B), dim3(32), 0, s, gn_tiles, gn_stats, HW, (double)HW * (C / 32));
        } else {
            const int chunk_px = std::max(256, (HW + 63) / 64), nchunk = (HW + chunk_px - 1) / chunk_px;
            hipLaunchKernelGGL((gn_partial_kernel<TB>), dim3(nchunk, B), dim3(256), 0, s, x, gn_partial, HW, C, chunk_px, nullptr, 0, 0);
            hipLaunchKernelGGL(gn_finish_kernel<false>, dim3(B), dim3(32), 0, s, gn_partial, gn_stats, nchunk, (double)HW * (C / 32), nullptr, 0);
        }
        const size_t nvec = (size_t)B * HW * C / Elem<TB>::PER16;
        hipLaunchKernelGGL((gn_apply_kernel<TB, RELU, RES>), dim3((nvec + 255) / 256), dim3(256), 0, s, x, res, y, gn_stats, g.g,
                           g.b, HW, C, nvec, nullptr, 0, 0);
    }
    // H x W: the images' size; a ragged batch (hw = the chunk's patch grids): the size of the ACTIVATION container -- the smallest multiples of
    // 16 that hold every image of the batch (ragged_batch: rag_box), never more than the canvas the workspaces are sized for -- while the
    // image array itself is [B][1][Hi][Wi], the caller's container
    template <typename TB>
    int backbone(Backbone<TB>& k, const float* img, int B, int H, int W, const TB** feat, hipStream_t s, const int* hw = nullptr, int Hi = 0, int Wi = 0) {
        TB* const* act = k.act;
        int h1, w1, pt, pl;
        same_pad(H, 7, 2, &h1, &pt); same_pad(W, 7, 2, &w1, &pl);
        if (hw) bk_gemm(s, LoadStem<TB, true>{img, hw, Hi, Wi, pt, pl, FastDiv(h1 * w1), FastDiv(w1)}, k.stem_w, B * h1 * w1, 64, 64, EpiStore<TB>{act[1], 64, nullptr});
        else bk_gemm(s, LoadStem<TB>{img, H, W, pt, pl, FastDiv(h1 * w1), FastDiv(w1)}, k.stem_w, B * h1 * w1, 64, 64, EpiStore<TB>{act[1], 64, nullptr}, h1 * w1);
        group_norm<true, false>(s, (const TB*)act[1], (const TB*)nullptr, act[1], k.stem_gn, B, h1 * w1, 64, RagExt{hw, 8}, w1);
        int hc, wc, ppt, ppl;
        same_pad(h1, 3, 2, &hc, &ppt); same_pad(w1, 3, 2, &wc, &ppl);
        {
            const size_t nvec = (size_t)B * hc * wc * 64 / Elem<TB>::PER16;
            auto pool = hw ? maxpool3x3s2_kernel<TB, true> : maxpool3x3s2_kernel<TB, false>;
            hipLaunchKernelGGL(pool, dim3((nvec + 255) / 256), dim3(256), 0, s, act[1], act[0], h1, w1, 64, hc, wc, ppt, ppl, nvec, hw, 8);
        }
        TB* cur = act[0];
        int mul = 4;                                          // 16 / stride of `cur` against the image (ragged extents)
        for (const BlockW<TB>& b : k.blocks) {                // Bottleneck.forward (resnet.py:143-149)
            const int ho = (hc + b.stride - 1) / b.stride, wo = (wc + b.stride - 1) / b.stride;
            const RagExt ri{hw, mul}, ro{hw, mul / b.stride};
            const TB* res = cur;
            if (b.has_ds) {                                   // DownSample: 1x1 stride-s StdConv + GroupNorm (no act)
                conv<TB>(s, cur, b.ds, act[1], B, hc, wc, b.cin, b.cout, 1, b.stride, ri);
                group_norm<false, false>(s, (const TB*)act[1], (const TB*)nullptr, act[1], b.nds, B, ho * wo, b.cout, ro, wo);
                res = act[1];
            }
            conv<TB>(s, cur, b.c1, act[2], B, hc, wc, b.cin, b.mid, 1, 1, ri);
            group_norm<true, false>(s, (const TB*)act[2], (const TB*)nullptr, act[2], b.n1, B, hc * wc, b.mid, ri, wc);
            conv<TB>(s, act[2], b.c2, act[3], B, hc, wc, b.mid, b.mid, 3, b.stride, ri);
            group_norm<true, false>(s, (const TB*)act[3], (const TB*)nullptr, act[3], b.n2, B, ho * wo, b.mid, ro, wo);
            conv<TB>(s, act[3], b.c3, act[2], B, ho, wo, b.mid, b.cout, 1, 1, ro);
            group_norm<true, true>(s, (const TB*)act[2], res, act[0], b.n3, B, ho * wo, b.cout, ro, wo);   // relu(norm(x) + res)
            cur = act[0]; hc = ho; wc = wo; mul /= b.stride;
        }
        if (hc != H / 16 || wc != W / 16) return fail(TXO_E_INVALID, "backbone output grid does not match H/16 x W/16");
        *feat = cur;
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // ---- what an encode is given (session.h: ImageBatch), checked.  The size checks of one image inside its Hc x Wc container: `who` names it
    int check_image_size(const std::string& who, const char* is, int H, int W, int Hc, int Wc) {
        if (H <= 0 || W <= 0 || H % 16 || W % 16) return fail(TXO_E_INVALID, who + " height/width must be positive multiples of 16");
        if (H > Hc || W > Wc) return fail(TXO_E_INVALID, who + is + "larger than the container");
        if (H > cfg.canvas_h || W > cfg.canvas_w) return fail(TXO_E_INVALID, who + is + "larger than the position-embedding canvas");
        return 0;
    }
    int fixed_batch(int B, int C, int H, int W, ImageBatch* ib) {
        if (!ready) return fail(TXO_E_STATE, "weights not finalized");
        if (C != cfg.in_channels) return fail(TXO_E_INVALID, "image channel count does not match in_channels");
        if (int r = check_image_size("image", " ", H, W, H, W)) return r;
        const int N = 1 + (H / 16) * (W / 16);
        if (B < 1 || B > Bmax) return fail(TXO_E_INVALID, "batch exceeds engine max_batch");
        if (N > Nmax) return fail(TXO_E_INVALID, "token count exceeds engine max_tokens");
        *ib = ImageBatch{B, C, H, W, N};
        return 0;
    }
    int encode(const float* img, int B, int C, int H, int W, float* enc_out, hipStream_t s) override {
        ImageBatch ib;
        if (int r = fixed_batch(B, C, H, W, &ib)) return r;
        return encode_batch(ib, img, enc_out, s);
    }
    int encode_batch(const ImageBatch& ib, const float* img, float* enc_out, hipStream_t s) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (prof) { e0 = pool.next(); e1 = pool.next(); (void)hipEventRecord(e0, s); }
        // Image chunks (enc_chunk_images): every row of the stack belongs to ONE image, so the stack may run over a few images at a time
        // through the SAME workspace rows -- a chunk whose intermediates (stream, z, q/k/v, attention output, FFN hidden) fit the 256 MB
        // Infinity Cache keeps every producer -> consumer hand-over on the die instead of through HBM.  Same bits as the whole batch.
        const int bc = enc_chunk_images(ib.B);
        for (int b0 = 0; b0 < ib.B; b0 += bc) {
            const int nb = std::min(bc, ib.B - b0);
            if (int r = encode_images(ib.chunk(b0, nb), img + b0 * ib.pixels(), enc_out + (size_t)b0 * ib.N * D, s)) return r;
        }
        if (prof) { (void)hipEventRecord(e1, s); ev_enc.push_back({e0, e1}); }
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // images per encoder chunk: TXO_ENC_CHUNK=n forces n (0 = whole batch); default the whole batch (profiles/r06_encoder_chunk_sweep.txt)
    int enc_chunk_images(int B) const { return knobs.enc_chunk_env > 0 ? std::min(B, knobs.enc_chunk_env) : B; }
    // the RAGGED pairs of the encoder: the descriptor picks the instantiation, the arguments are spelled once
    void launch_patch_embed(hipStream_t s, const ImageBatch& ib, const float* img) {
        const int hw = ib.N - 1, w = ib.W / 16, G = cfg.canvas_w / 16;
        const int* rhw = rag_hw + 2 * ib.first;
        auto go = [&](auto load, auto epi) { launch_gemm_big<T>(s, load, patch_w, ib.B * hw, D, ib.C * 256, epi); };
        if (ib.ragged) go(LoadPatchRagged<T>{img, rhw, ib.C, ib.H, ib.W, hw}, EpiPatchRagged{ex, patch_b, pos, rhw, D, hw, G});
        else go(LoadPatch<T>{img, ib.C, ib.H, ib.W, hw, w}, EpiPatch{ex, patch_b, pos, D, hw, w, G});
    }
    const int* ragged_tokens(const ImageBatch& ib) const { return ib.ragged ? rag_ntok + ib.first : nullptr; }
    void launch_enc_attn_f32(hipStream_t s, const ImageBatch& ib, dim3 grid, size_t hs) {
        auto kern = ib.ragged ? enc_attn_kernel<T, true> : enc_attn_kernel<T, false>;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, eqkv, eqkv + hs, eqkv + 2 * hs, eao, ib.N, cfg.enc_heads, ib.B * cfg.enc_heads, ragged_tokens(ib));
    }
    void launch_enc_attn_bf16(hipStream_t s, const ImageBatch& ib, dim3 grid, size_t hs, int rev) {
        const bf16* qb = reinterpret_cast<const bf16*>(eqkv);
        auto kern = ib.ragged ? enc_attn_bf16_v2_kernel<T, true> : enc_attn_bf16_v2_kernel<T, false>;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, qb, qb + hs, qb + 2 * hs, eao, ib.N, cfg.enc_heads, ib.B * cfg.enc_heads, rev, ragged_tokens(ib));
    }
    int encode_images(const ImageBatch& ib, const float* img, float* enc_out, hipStream_t s) {
        const int B = ib.B, H = ib.H, W = ib.W, N = ib.N, hw = N - 1, w = W / 16;
        const int M = B * N, G = cfg.canvas_w / 16;

        hipLaunchKernelGGL(cls_rows_kernel, dim3((B * D + 255) / 256), dim3(256), 0, s, ex, cls, pos, B, N, D);
        if (!hybrid) launch_patch_embed(s, ib, img);
        else if (ib.ragged) {
            // (txo_set_ragged_hybrid.)  The backbone runs in container layout over the batch's bounding box (rag_box) and the projection packs
            // image b's own grid into rows 1 .. n_b-1 of slot b; the container grid does not map onto a slot's padding rows, so those are zeroed here
            const int* rhw = rag_hw + 2 * ib.first;
            const int Hb = rag_box[0], Wb = rag_box[1], hwC = (Hb / 16) * (Wb / 16);
            const size_t n4 = (size_t)M * (D / 4);
            hipLaunchKernelGGL(zero_pad_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, ex, ragged_tokens(ib), B, N, D / 4);
            const EpiTokensRagged epi{ex, patch_b, pos, rhw, D, hwC, Wb / 16, N, G};
            if (bk_fp32) {
                const float* feat = nullptr;
                if (int r = backbone<float>(bk32, img, B, Hb, Wb, &feat, s, rhw, H, W)) return r;
                bk_gemm(s, LoadPlain<float>{feat, 1024}, (const float*)bk32.proj_w, B * hwC, D, 1024, epi);
            } else {
                const T* feat = nullptr;
                if (int r = backbone<T>(bk, img, B, Hb, Wb, &feat, s, rhw, H, W)) return r;
                gemm_plain(s, feat, patch_w, B * hwC, D, 1024, epi);
            }
        } else {
            if (bk_fp32) {
                const float* feat = nullptr;
                if (int r = backbone<float>(bk32, img, B, H, W, &feat, s)) return r;
                bk_gemm(s, LoadPlain<float>{feat, 1024}, (const float*)bk32.proj_w, B * hw, D, 1024, EpiTokens{ex, patch_b, pos, D, hw, w, G});
            } else {
                const T* feat = nullptr;
                if (int r = backbone<T>(bk, img, B, H, W, &feat, s)) return r;
                gemm_plain(s, feat, patch_w, B * hw, D, 1024, EpiTokens{ex, patch_b, pos, D, hw, w, G});
            }
        }
        const size_t hs = (size_t)M * Ie;      // one of q/k/v, head-major [B*heads][N][64]
        // Walk direction (perf mode): successive kernels of the stack walk the rows alternately upwards and downwards, so that each
        // starts on the rows its producer wrote LAST -- still in the 256 MB Infinity Cache -- instead of on the ones it wrote first
        // (every intermediate here is 0.2-0.9 GB at batch 256: with all kernels walking upwards a consumer's first reads are the
        // producer's oldest lines).  Results do not depend on it (every kernel's rows are independent).
        bool down = false;                                    // direction of the NEXT kernel
        auto dir = [&]() -> int { if (sizeof(T) != 2) return 0; const bool d = down; down = !down; return d ? 1 : 0; };
        for (int l = 0; l < cfg.enc_layers; ++l) {
            // The stream between two sub-layers is x = LN(y) (the residual) and z = LN(x) (the block input), attention.py:242-259.
            // x is never written: the row kernel leaves {mean, rstd} of LN(y) per row (rows.h MODE 3) and the next GEMM epilogue
            // rebuilds its residual from y -- in place, ey is both its residual source and its output -- with the same expression.
            const ResidLN res_x{ey, estats, enc_gb, D}, res_first{ex, nullptr, nullptr, D};
            // (the epilogues store plainly: non-temporal stores, +22 % for a bare 256x256 store epilogue at K = 768 in probes/pp_store_policy.hip,
            // run these epilogues the same -- 45.84 vs 45.77 ms per ViT-Base encode, probes/enc_nt.py)
            if (l == 0) launch_ln<0, T>(s, ex, nullptr, ez, enc_g, enc_b, M, dir());
            else launch_ln<3, T>(s, ey, estats, ez, enc_g, enc_b, M, dir());
            const dim3 agrid = ea_grid((N + EA_QBLK - 1) / EA_QBLK, B * cfg.enc_heads);   // XCD-aware block order (enc_attn.h: ea_block)
            if constexpr (sizeof(T) == 4) {
                gemm_plain(s, ez, enc_attn[l].wqkv, M, 3 * Ie, D, EpiHeads<float>{eqkv, hs, Ie, cfg.enc_heads, N});
                launch_enc_attn_f32(s, ib, agrid, hs);
            } else {                                              // perf mode: bf16 q/k/v, bf16 MFMA attention
                gemm_plain(s, ez, enc_attn[l].wqkv, M, 3 * Ie, D, EpiHeads<bf16>{reinterpret_cast<bf16*>(eqkv), hs, Ie, cfg.enc_heads, N}, dir());
                launch_enc_attn_bf16(s, ib, agrid, hs, dir());
            }
            gemm_plain(s, eao, enc_attn[l].wo, M, 2 * D, Ie,
                               EpiGluRes<sizeof(T) == 2>{ey, l == 0 ? res_first : res_x, enc_attn[l].bo}, dir());
            launch_ln<3, T>(s, ey, estats, ez, enc_g, enc_b, M, dir());
            gemm_plain(s, ez, enc_mlp[l].w1, M, 2 * Fe, D, EpiGeglu<T>{ehid, enc_mlp[l].b1, Fe}, dir());
            gemm_plain(s, ehid, enc_mlp[l].w2, M, D, Fe, EpiBiasRes{ey, res_x, enc_mlp[l].b2}, dir());
        }
        launch_ln<2, float>(s, ey, nullptr, enc_out, encn_g, encn_b, M, dir());
        if (ib.ragged) {                                      // the padding rows of every slot are returned as zeros
            const size_t n4 = (size_t)M * (D / 4);
            hipLaunchKernelGGL(zero_pad_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, enc_out, ragged_tokens(ib), B, N, D / 4);
        }
        return 0;
    }

    // ---- ragged batches (texocr.h) ------------------------------------------------------------------------------------------------
    // host array -> engine-owned device buffer through the pinned staging area (its previous copy has left it first); no allocation
    // (up to two destinations: the first n0 values go to dst0, the rest to dst1)
    int upload_i32(const int32_t* src, int* dst0, int n0, int* dst1, int n1, hipStream_t s) {
        if (rag_ev_pending) { HIP_TRY(hipEventSynchronize(rag_ev)); rag_ev_pending = false; }
        memcpy(rag_host, src, sizeof(int32_t) * (n0 + n1));
        HIP_TRY(hipMemcpyAsync(dst0, rag_host, sizeof(int32_t) * n0, hipMemcpyHostToDevice, s));
        if (n1 > 0) HIP_TRY(hipMemcpyAsync(dst1, rag_host + n0, sizeof(int32_t) * n1, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(rag_ev, s));
        rag_ev_pending = true;
        return 0;
    }
    // ---- device-side image ingest (ingest.h, ingest_fit.h, ingest_trim.h); works before the weights are finalized (it reads none) -----------
    // What the three calls below share: the staging is free once its last copy has left it; `fill` then writes the descriptors of the B images
    // into it (non-zero: its refusal), and they go up as ONE staged copy, the way ragged_batch uploads its grids; no allocation.
    // pending: the copy's event is left for the next call to wait on (trim_views waits on the stream itself instead)
    struct Staging { void* dev; const void* host; size_t bytes; };
    template <typename Fill> int ingest_stage(int B, Staging st, hipStream_t s, bool pending, Fill fill) {
        if (B > Bmax) return fail(TXO_E_INVALID, "ingest: batch exceeds engine max_batch (the descriptor staging holds max_batch images)");
        if (ing_ev_pending) { HIP_TRY(hipEventSynchronize(ing_ev)); ing_ev_pending = false; }
        if (int r = fill()) return r;
        HIP_TRY(hipMemcpyAsync(st.dev, st.host, st.bytes, hipMemcpyHostToDevice, s));
        if (pending) { HIP_TRY(hipEventRecord(ing_ev, s)); ing_ev_pending = true; }
        return 0;
    }
    // one dispatch of an ingest kernel; profiling on (txo_profile_read kind 4): with a pair of pooled events bound to the dispatch itself
    template <typename... P> int ingest_launch(void (*kern)(P...), dim3 grid, dim3 blk, hipStream_t s, typename std::common_type<P>::type... args) {
        if (!prof) { hipLaunchKernelGGL(kern, grid, blk, 0, s, args...); return 0; }
        hipEvent_t e0 = pool.next(), e1 = pool.next();
        if (!e0 || !e1) return fail(TXO_E_HIP, "hipEventCreate failed");
        hipExtLaunchKernelGGL(kern, grid, blk, 0, s, e0, e1, 0, args...);
        ev_ingest.push_back({e0, e1});
        return 0;
    }
    int ingest(const IngestPlan& p, const IngestReq& q, hipStream_t s) override {
        const int B = q.src.B;
        const unsigned char* pix = q.src.pix;
        const dim3 grid((unsigned)((q.Wc + IG_BLOCK_W - 1) / IG_BLOCK_W), (unsigned)((q.Hc + IG_ROWS - 1) / IG_ROWS), (unsigned)B), blk(IG_LANES_X * IG_ROWS);
        if (!p.oversized) {                                   // nothing to downscale: txo_ingest_u8's own launch, its container bit for bit
            if (int r = ingest_stage(B, {ing_desc, ing_host, sizeof(IngestDesc) * B}, s, true, [&] {
                    for (int b = 0; b < B; ++b)
                        ing_host[b] = IngestDesc{(long long)p.off[b], p.shapes[3 * b], p.shapes[3 * b + 1], p.shapes[3 * b + 2], p.pitch ? p.pitch[b] : 0};
                    return 0;
                })) return r;
            if (int r = ingest_launch(p.pitch ? ingest_u8_kernel<true> : ingest_u8_kernel<false>, grid, blk, s, pix, ing_desc, q.box, q.C, q.Hc, q.Wc)) return r;
            HIP_TRY(hipGetLastError());
            return 0;
        }
        // Fit-to-canvas (ingest_fit.h): the descriptors and the list of the images with a horizontal pass in one staged copy, then that pass (if
        // any image has one) and the fused vertical pass + ingest
        int nh = 0, hmax = 0, wmax = 0;
        if (int r = ingest_stage(B, {fit_dev, fit_host, fit_bytes(B)}, s, true, [&] {
                FitDesc* fd = reinterpret_cast<FitDesc*>(fit_host);
                int* hl = reinterpret_cast<int*>(fit_host + sizeof(FitDesc) * (size_t)B);
                long long mid = 0;
                for (int b = 0; b < B; ++b) {
                    const int h = p.shapes[3 * b], w = p.shapes[3 * b + 1], ch = p.shapes[3 * b + 2], fh = p.fitted[2 * b], fw = p.fitted[2 * b + 1];
                    fd[b] = FitDesc{(long long)p.off[b], -1, h, w, ch, fh, fw, p.pitch ? p.pitch[b] : 0};
                    if (fw != w) {
                        fd[b].mid = mid;
                        mid += ingest_fit_mid_bytes(h, fw, ch);
                        hl[nh++] = b;
                        hmax = std::max(hmax, h); wmax = std::max(wmax, fw);
                    }
                }
                return 0;
            })) return r;
        const FitDesc* dd = reinterpret_cast<const FitDesc*>(fit_dev);
        const int* dl = reinterpret_cast<const int*>(fit_dev + sizeof(FitDesc) * (size_t)B);
        unsigned char* scratch = static_cast<unsigned char*>(q.scratch);
        const dim3 hgrid((unsigned)((wmax + FR_COLS - 1) / FR_COLS), (unsigned)((hmax + FR_ROWS - 1) / FR_ROWS), (unsigned)nh), hblk(FR_COLS * FR_LANES_Y);
        const auto rows = p.pitch ? fit_rows_kernel<true> : fit_rows_kernel<false>;
        const auto kern = p.pitch ? ingest_fit_kernel<true> : ingest_fit_kernel<false>;
        if (nh) if (int r = ingest_launch(rows, hgrid, hblk, s, pix, dd, dl, scratch)) return r;
        if (int r = ingest_launch(kern, grid, blk, s, pix, scratch, dd, q.box, q.C, q.Hc, q.Wc)) return r;
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // Trim-to-ink ingest (ingest_trim.h).  The list, level and margin have passed txo_ingest_trim_views' checks.  The descriptors go up as in
    // ingest; a fill of the records, the one launch over every byte, 16 B bytes back and a wait on s: the container's size depends on them.
    int trim_views(const IngestList& l, int level, int margin, int32_t* views, hipStream_t s) override {
        const int B = l.B;
        long long tiles = 0;
        if (int r = ingest_stage(B, {ing_desc, ing_host, sizeof(IngestDesc) * B}, s, false, [&] {
                long long pieces = 1;                         // of the largest image, whatever its first byte's alignment
                for (int b = 0; b < B; ++b) {
                    ing_host[b] = IngestDesc{(long long)l.offsets[b], l.shapes[3 * b], l.shapes[3 * b + 1], l.shapes[3 * b + 2], 0};
                    pieces = std::max(pieces, ((long long)l.shapes[3 * b] * l.shapes[3 * b + 1] * l.shapes[3 * b + 2] + 30) / 16);
                }
                tiles = (pieces + TB_TILE - 1) / TB_TILE;
                return tiles > 2147483647LL ? fail(TXO_E_INVALID, "ingest: an image exceeds the launch grid of the ink search") : 0;
            })) return r;
        hipLaunchKernelGGL(trim_fill_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, trim_rec, B);
        if (int r = ingest_launch(trim_bbox_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(TB_THREADS), s, l.pix, ing_desc, trim_rec, level)) return r;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(trim_host, trim_rec, sizeof(int) * 4 * (size_t)B, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));                     // (the staging is free again too: no event is left pending)
        for (int b = 0; b < B; ++b) trim_view_of(trim_host + 4 * b, l.shapes[3 * b], l.shapes[3 * b + 1], margin, views + 4 * b);
        return 0;
    }
    int ragged_refusals() {
        if (!ready) return fail(TXO_E_STATE, "weights not finalized");
        if (hybrid && !rag_hybrid)
            return fail(TXO_E_INVALID, "ragged batches: the hybrid front end is not supported (GroupNorm statistics and SAME padding are per image extent) "
                                       "unless txo_set_ragged_hybrid(e, 1) is in effect");
        if (latent_ok && knobs.lat_mode == 1)
            return fail(TXO_E_INVALID, "ragged batches: the latent cross-attention form (TXO_LATENT=1) is not supported; a ragged decode runs in the K/V form");
        return 0;
    }
    // the checked descriptor of a ragged batch; leaves {h_b, w_b} in rag_hw and n_b in rag_ntok
    int ragged_batch(int B, int C, int Hc, int Wc, const int32_t* sizes, hipStream_t s, ImageBatch* ib) {
        if (int r = ragged_refusals()) return r;
        if (!sizes) return fail(TXO_E_INVALID, "ragged batches: null sizes");
        if (C != cfg.in_channels) return fail(TXO_E_INVALID, "image channel count does not match in_channels");
        if (B < 1 || B > Bmax) return fail(TXO_E_INVALID, "ragged batches: batch exceeds engine max_batch");
        if (Hc <= 0 || Wc <= 0) return fail(TXO_E_INVALID, "ragged batches: the container's height/width must be positive");
        if (Wc % 4) return fail(TXO_E_INVALID, "ragged batches: the container's width must be a multiple of 4 (rows are read in 16-byte pieces)");
        int Ns = 0;
        std::vector<int32_t>& st = rag_stage;
        rag_box[0] = rag_box[1] = 0;
        for (int b = 0; b < B; ++b) {
            const int H = sizes[2 * b], W = sizes[2 * b + 1];
            if (int r = check_image_size("ragged batches: image " + std::to_string(b), " is ", H, W, Hc, Wc)) return r;
            rag_box[0] = std::max(rag_box[0], H); rag_box[1] = std::max(rag_box[1], W);
            st[2 * b] = H / 16; st[2 * b + 1] = W / 16; st[2 * Bmax + b] = 1 + (H / 16) * (W / 16);
            Ns = std::max(Ns, st[2 * Bmax + b]);
        }
        if (Ns > Nmax) return fail(TXO_E_INVALID, "ragged batches: token count of the largest image exceeds engine max_tokens");
        // (the backbone's workspaces hold max_tokens - 1 patches per image, and its container is the batch's bounding box)
        if (hybrid && (rag_box[0] / 16) * (rag_box[1] / 16) > Nmax - 1)
            return fail(TXO_E_INVALID, "ragged batches: the hybrid front end works on the smallest box that holds every image of the batch, and its "
                                       "patch count exceeds engine max_tokens - 1");
        // one staged copy: [2 B] patch grids followed by [B] token counts
        for (int b = 0; b < B; ++b) st[2 * B + b] = st[2 * Bmax + b];
        if (int r = upload_i32(st.data(), rag_hw, 2 * B, rag_ntok, B, s)) return r;
        *ib = ImageBatch{B, C, Hc, Wc, Ns, true};
        return 0;
    }
    int encode_ragged(const float* img, int B, int C, int Hc, int Wc, const int32_t* sizes, float* enc_out, int32_t* n_slot, hipStream_t s) override {
        ImageBatch ib;
        if (int r = ragged_batch(B, C, Hc, Wc, sizes, s, &ib)) return r;
        if (n_slot) *n_slot = ib.N;
        return encode_batch(ib, img, enc_out, s);
    }
    int decode_begin_ragged(const float* enc, int B, int Ns, const int32_t* n_tokens, int eos, hipStream_t s) override {
        if (int r = ragged_refusals()) return r;
        if (!n_tokens) return fail(TXO_E_INVALID, "ragged batches: null n_tokens");
        if (B < 1 || B > Bmax) return fail(TXO_E_INVALID, "ragged batches: batch exceeds engine max_batch");
        if (Ns < 1 || Ns > Nmax) return fail(TXO_E_INVALID, "ragged batches: slot stride exceeds engine max_tokens");
        for (int b = 0; b < B; ++b)
            if (n_tokens[b] < 1 || n_tokens[b] > Ns)
                return fail(TXO_E_INVALID, "ragged batches: n_tokens[" + std::to_string(b) + "] must be in [1, Ns]");
        return begin_session(enc, B, Ns, eos, s, true, KeyCounts{nullptr, n_tokens});
    }
    // what a decode reads, checked: a fixed or ragged batch of images, or the caller's encoder rows as they are (begin_session checks those)
    int resolve_source(const DecodeSrc& q, hipStream_t s, Source* src) {
        ImageBatch ib;
        if (q.img) { if (int r = q.sizes ? ragged_batch(q.B, q.C, q.H, q.W, q.sizes, s, &ib) : fixed_batch(q.B, q.C, q.H, q.W, &ib)) return r; }
        *src = Source{ib, q.img != nullptr, q.img ? q.img : q.enc, q.B, q.img ? ib.N : q.N};
        return 0;
    }
    // Every txo_generate* entry but txo_generate_beam (session.h: DecodeReq): from images, a ragged batch or encoder rows, with or without
    // log-probabilities, from BOS or behind a caller's prefix (a prompted decode, texocr.h).  Everything is refused before anything is
    // encoded, each family of entries in the order it always checked in.
    // Per-row stop (stop_mode 1, a build extension: the reference has only the global break,
    // decoder.py:115-116): the decode below is the same loop with the same break -- rows are independent, so every row's tokens up to its first eos
    // are what the global-break run gives -- and every token BEHIND a row's first eos becomes cfg.pad (pad_after_eos_kernel); on the launch
    // path the finished rows also stop costing work (compact_lane).
    int generate(const DecodeReq& q, hipStream_t s) override {
        const bool ragged = q.src.sizes != nullptr;
        // results of THIS call, also when it is refused (txo_generate_ragged / _logp: only once the batch is accepted, generate_common)
        if (q.prefix || !ragged) { last_compactions = 0; last_ragged = false; }
        last_guarded = false;
        last_alts = 0; alts_B = alts_cols = 0;
        if (ragged) { if (int r = ragged_refusals()) return r; }
        Decode d{q};
        if (int r = q.prefix ? check_prefix(q, &d.m, &d.M) : check_length(q.max_len, ragged)) return r;
        if (int r = resolve_source(q.src, s, &d.src)) return r;
        if (int r = close_refusals("generate", q.eos, q.max_len, !q.prefix)) return r;   // (behind every other refusal of the entry)
        if (guard_p > 0) {                                         // ... and the repeat guard's behind those
            if (closing())
                return fail(TXO_E_INVALID, "repeat guard: not available with a closing decode (txo_set_rules_close): the budget's guarantee and the guard's ban can "
                                           "conflict (txo_set_repeat_guard(e, 0, 0) switches the guard off)");
            if (sample_mode && !sample_in_regs(V) && (size_t)V * sizeof(float) + guard_map_bytes(V) > 65536)
                return fail(TXO_E_INVALID, "repeat guard: the vocabulary does not fit the guarded sampler's LDS (vocab * 4 bytes + vocab / 8 bytes per workgroup, 64 KB)");
        }
        if (alts_k > 0) {                                          // ... and the alternatives' last
            if (q.max_len > Tmax)
                return fail(TXO_E_INVALID, "alternatives: max_len exceeds the decoder's max_length (the sliding window's tail does not run the loop that keeps "
                                           "them; txo_set_alternatives(e, 0) switches them off)");
            if (!alt_ids) {
                if (int r = dalloc(&alt_ids, (size_t)Bmax * Tmax * ALTS_MAX)) return r;
                if (int r = dalloc(&alt_logp, (size_t)Bmax * Tmax * ALTS_MAX)) return r;
            }
        }
        if (q.prefix) {   // the lengths to the device, through the pinned staging of the ragged sizes (behind ragged_batch's own copy)
            std::vector<int32_t> len((size_t)q.src.B, q.P);
            if (q.prefix_len) len.assign(q.prefix_len, q.prefix_len + q.src.B);
            if (int r = upload_i32(len.data(), flen, q.src.B, nullptr, 0, s)) return r;
        }
        return generate_common(d, s);
    }
    // max_len of a decode from BOS.  Beyond the positional table the window slides (generate_window), and its multi-position forward has two
    // preconditions: refused BEFORE anything is decoded.  A ragged batch also needs the ragged forward for it, and says that first.
    int check_length(int max_len, bool ragged) {
        if (max_len < 1) return fail(TXO_E_INVALID, "max_len must be >= 1");
        if (max_len <= Tmax) return 0;
        if (ragged && !rag_fwd)
            return fail(TXO_E_INVALID, "ragged batches: max_len exceeds the decoder's max_length (the sliding window of a ragged batch needs txo_set_ragged_forward(e, 1))");
        if (V % 8 == 0 && (size_t)Tmax <= (size_t)Bmax * Nmax) return 0;
        return fail(TXO_E_INVALID, ragged ? "ragged batches: max_len exceeds the decoder's max_length and the sliding window's multi-position forward needs a "
                                            "vocabulary size that is a multiple of 8 and max_length <= max_batch * max_tokens"
                                          : "max_len exceeds the decoder's max_length and the sliding window's multi-position forward needs a vocabulary "
                                            "size that is a multiple of 8 and max_length <= max_batch * max_tokens (use decoder.generate's stepwise loop)");
    }
    // a prompted decode's bounds; *m / *M: the shortest / longest prefix length
    int check_prefix(const DecodeReq& q, int* m, int* M) {
        const int B = q.src.B, P = q.P;
        if (q.max_len < 1) return fail(TXO_E_INVALID, "prefix decode: max_len must be >= 1");
        if (B < 1 || B > Bmax) return fail(TXO_E_INVALID, "prefix decode: batch exceeds engine max_batch");
        if (P < 1) return fail(TXO_E_INVALID, "prefix decode: the prefix needs at least one column");
        *m = *M = P;
        if (q.prefix_len) {
            *M = 1;
            for (int b = 0; b < B; ++b) {
                if (q.prefix_len[b] < 1 || q.prefix_len[b] > P)
                    return fail(TXO_E_INVALID, "prefix decode: prefix_len[" + std::to_string(b) + "] must be in [1, P]");
                *m = std::min(*m, (int)q.prefix_len[b]); *M = std::max(*M, (int)q.prefix_len[b]);
            }
        }
        if ((long long)*M - 1 + q.max_len > Tmax)
            return fail(TXO_E_INVALID, "prefix decode: the longest prefix - 1 + max_len exceeds the decoder's max_length (a prompted decode does not slide the window)");
        if ((size_t)(*m - 1) > (size_t)Bmax * Nmax)
            return fail(TXO_E_INVALID, "prefix decode: the shortest prefix does not fit the multi-position pass's workspace (max_batch * max_tokens rows)");
        return 0;
    }

    // Opens the decode session on enc [B][N][D] (session.h), complete: no caller patches a field in behind this call.  kc: a ragged session's
    // key counts.  beams: decode rows per image.  project_kv: a session opened through txo_decode_begin or txo_score may be prefilled, and the
    // multi-position forward works on the projected K/V panels: such a session steps in the K/V form too (one-pass and stepwise logits of
    // decoder.net() then come from the same weights), unless TXO_LATENT=1 pins the latent form.  false: generate() / generate_beam() choose it.
    int decode_begin(const float* enc, int B, int N, int eos, hipStream_t s) override { return begin_session(enc, B, N, eos, s, true); }
    int begin_session(const float* enc, int B, int N, int eos, hipStream_t s, bool project_kv, KeyCounts kc = {}, int beams = 1) {
        if (!ready) return fail(TXO_E_STATE, "weights not finalized");
        if (B < 1 || B > Bmax) return fail(TXO_E_INVALID, "batch exceeds engine max_batch");
        if (N < 1 || N > Nmax) return fail(TXO_E_INVALID, "token count exceeds engine max_tokens");
        if (kc.host) { if (int r = upload_i32(kc.host, slens, B, nullptr, 0, s)) return r; }
        if (kc.dev) HIP_TRY(hipMemcpyAsync(slens, kc.dev, sizeof(int) * B, hipMemcpyDeviceToDevice, s));
        {   // the session's copy of the encoder rows in the storage type: A operand of the K/V projection; in the latent form what
            // every cross-attention tile of every layer reads (the caller's buffer is not referenced after this call)
            const size_t n4 = (size_t)B * N * D / 4;
            hipLaunchKernelGGL((cast_rows_kernel<T>), dim3((n4 + 255) / 256), dim3(256), 0, s, enc, enc_t, n4);
        }
        ses = Session{B * beams, N, B, true, kc.dev || kc.host, project_kv && latent_ok && knobs.lat_mode == 1};
        if (!ses.latent && project_kv) ensure_ckv(s);
        lanes.split(ses.rows, 1, s);
        reset_lanes(s, eos);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // The form of a launch-path decode, chosen by generate() / generate_beam() once the decode path is known.
    void choose_form(bool row_stop, hipStream_t s) {
        ses.latent = !ses.ragged && latent_ok && (knobs.lat_mode == 1 || (knobs.lat_mode < 0 && auto_latent(ses.rows)));   // (ragged: K/V form)
        ses.row_stop = row_stop;
        ses.lat_self = ses.latent && lat_self_ok() && !row_stop;      // (the z history is not moved by compact_lane)
        if (!ses.latent) ensure_ckv(s);                               // cross K/V of the session's images
    }

    // K/V of every decoder layer's cross attention in one GEMM: W = [Ld][k|v][Id][D] (attention.py:125-126).  The K/V form's decode
    // steps and the multi-position prefill read these panels; a latent-form session projects them only if a prefill asks.
    void ensure_ckv(hipStream_t s) {
        if (ses.ckv_valid) return;
        const int M = ses.images * ses.keys;
        gemm_plain(s, enc_t, wckv, M, cfg.dec_layers * 2 * Id, D, EpiHeads<T>{ckv, (size_t)M * Id, Id, cfg.dec_heads, ses.keys});
        ses.ckv_valid = true;
    }

    int abandon_lanes(hipStream_t s, int rc) { stamps.slot = -1; return lanes.abandon(s, ses.images, rc); }
    // start_m > 0: a prompted decode -- every range starts at position start_m - 1, fed from the prefix table (step_prefix.h)
    void reset_lanes(hipStream_t s, int eos, int start_m = 0) {
        for (int i = 0; i < lanes.n; ++i) {
            const LaneSet::Lane& ln = lanes[i];
            const int n = ln.nb > Tmax ? ln.nb : Tmax;
            if (start_m > 0) {
                (void)hipMemsetAsync(st + i, 0, sizeof(StepState), s);
                hipLaunchKernelGGL(prefix_start_kernel, dim3((n + 255) / 256), dim3(256), 0, s, st + i, cur_tok + ln.b0, eos_seen + ln.b0,
                                   done_flag + (size_t)i * Tmax, ln.nb, Tmax, eos, ftab + (size_t)ln.b0 * Tmax, Tmax, flen + ln.b0, start_m);
            } else
            hipLaunchKernelGGL(reset_state_kernel, dim3((n + 255) / 256), dim3(256), 0, s, st + i, cur_tok + ln.b0,
                               eos_seen + ln.b0, done_flag + (size_t)i * Tmax, ln.nb, Tmax, cfg.bos, eos);
            if (ses.row_stop) hipLaunchKernelGGL(iota_kernel, dim3((ln.nb + 255) / 256), dim3(256), 0, s, row_map + ln.b0, ln.nb, ln.b0);
        }
    }

    // tiled copies of the decode projections' weights for the launch path (dec_gemm.h: w_tiled), keyed by the row-major buffer
    std::map<const void*, T*> wtiled;
    // one allocation for all of them (the arenas' reason: few large mappings); `want` collects (buffer, N, K), make_tiled_all() builds
    struct TileReq { const T* w; int N, K; };
    std::vector<TileReq> tile_reqs;
    void want_tiled(const T* w, int N, int K) {
        if (!knobs.w_tiled_on || !w || K % Elem<T>::KCHUNK) return;
        for (auto& r : tile_reqs) if (r.w == w) return;
        tile_reqs.push_back({w, N, K});
    }
    int make_tiled_all() {
        if (tile_reqs.empty()) return 0;
        auto pieces = [](const TileReq& r) { return (size_t)((r.N + 15) / 16) * (r.K / Elem<T>::KCHUNK) * 64; };   // 16-byte pieces
        size_t total = 0;
        for (auto& r : tile_reqs) total += (pieces(r) * 16 + 255) & ~(size_t)255;
        unsigned char* base = nullptr;
        HIP_TRY(hipMalloc(&base, total));
        allocs.push_back(base);
        size_t off = 0;
        for (auto& r : tile_reqs) {
            T* d = reinterpret_cast<T*>(base + off);
            hipLaunchKernelGGL((tile_weights_kernel<T>), dim3((unsigned)((pieces(r) + 255) / 256)), dim3(256), 0, 0, r.w, d, r.N, r.K);
            wtiled[r.w] = d;
            off += (pieces(r) * 16 + 255) & ~(size_t)255;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        tile_reqs.clear();
        return 0;
    }
    void use_tiled(DecGemmArgs<T>& a) const {
        a.w_tiled = 0;
        if (!knobs.w_tiled_on) return;
        auto it = wtiled.find(a.W);
        if (it != wtiled.end()) { a.W = it->second; a.w_tiled = 1; }
    }

    template <int PRO, int EPI>
    int launch_dec_gemm(hipStream_t s, DecGemmArgs<T> a) {
        use_tiled(a);
        constexpr bool has_pro = PRO != PRO_NONE;
        // 16-column tiles (half the cold weight bytes per block, twice the blocks) where the block's traffic is its weight
        // slice: the out-projections and FFN-out (K >= 1024).  Launches with an LN prologue keep 32 columns: every block also
        // fetches the 16 rows of y, so more blocks only multiply that traffic (measured: FFN-in 3.9 -> 7 us at 16 columns).
        constexpr bool paired = EPI == EPI_GLU_RES || EPI == EPI_GEGLU;
        const bool half = (paired && !has_pro) || (EPI == EPI_BIAS_RES && a.K >= 1024);
        const int bn = half ? 16 : DG_BN;
        const dim3 grid((a.N + bn - 1) / bn, (a.rows + DG_BM - 1) / DG_BM), blk(256);
        const size_t lds = dec_gemm_lds_bytes<T>(a.K, has_pro);
        a.stamps = (grid.x * grid.y <= (unsigned)Stamps::BLOCKS) ? stamps.next(PRO == PRO_NONE ? (EPI == EPI_GLU_RES ? "gemm out-proj+GLU+res" : "gemm ffn-out+res") : (EPI == EPI_QKV ? "gemm LN+qkv" : (EPI == EPI_GEGLU ? "gemm LN+ffn-in+GeGLU" : (EPI == EPI_STORE_T ? "gemm LN+q' (latent)" : "gemm LN+logits")))) : nullptr;
        // K known at compile time for the shapes of the reference configurations (straight-line code, exact register
        // arrays); any other K takes the run-time form (KW = 0)
        constexpr int KCH = Elem<T>::KCHUNK;
        const int kw = (a.K % (4 * KCH) == 0) ? a.K / (4 * KCH) : 0;
#define TXO_DG(KW_, BN_) hipLaunchKernelGGL((dec_gemm_kernel<T, PRO, EPI, KW_, BN_>), grid, blk, lds, s, a)
        if constexpr ((paired && !has_pro) || EPI == EPI_BIAS_RES) {
            if (half) {
                switch (kw) {
                    case 4: TXO_DG(4, 16); break;    case 6: TXO_DG(6, 16); break;    case 8: TXO_DG(8, 16); break;
                    case 12: TXO_DG(12, 16); break;  case 16: TXO_DG(16, 16); break;
                    case 24:                                 // K = 3072 (FFN-out of a 768-wide decoder): every fragment requested up front, one round trip instead of three
                        if constexpr (EPI == EPI_BIAS_RES && sizeof(T) == 2) { TXO_DG(24, 16); break; }
                        TXO_DG(0, 16); break;
                    default: TXO_DG(0, 16);
                }
            } else {
                TXO_DG(0, 32);
            }
        } else {
            switch (kw) {
                case 2: TXO_DG(2, 32); break;  case 4: TXO_DG(4, 32); break;  case 6: TXO_DG(6, 32); break;
                default: TXO_DG(0, 32);
            }
        }
#undef TXO_DG
        return 0;
    }

    // >= 128 rows of a wide (>= 512) bf16 decoder: the projections without a LayerNorm prologue on blocks of RT x 16 rows that share
    // their weight fragments (dec_gemm.h: RT).  Returns false when the shape has no such instantiation (the caller launches the
    // 16-row kernel).  A row's bits do not depend on RT (same K split over the waves, same reduction order).
    template <int EPI>
    bool launch_dec_gemm_wide(hipStream_t s, DecGemmArgs<T> a) {
        if constexpr (sizeof(T) != 2) { (void)s; (void)a; return false; }
        else {
            if (a.rows < 128 || knobs.dec_wide_off) return false;
            use_tiled(a);
            constexpr int KCH = Elem<T>::KCHUNK;
            const int kw = (a.K % (4 * KCH) == 0) ? a.K / (4 * KCH) : 0;
            // narrow decoder: only the folded latent output projection (K = heads * D = 2048) of a beam search's many rows -- 640 rows are
            // 1280 16-row blocks of 128 KB each (19.6 us on one range; on two ranges of 320 rows the 32-row blocks give 1066 -> 1130 img/s).
            // Up to 256 rows per range they change nothing (batch 256: 76.1 vs 76.4 ms on two ranges, 82.0 vs 81.5 on one).  r05: 32 x 16 blocks
            // for 129 .. 256 rows of ONE range (192 rows: 384 blocks of 16 x 16 are one and a half rounds of the CUs, 192 of 32 x 16 one):
            // generate 60.3 -> 59.6 ms at 130 images, 64.7 -> 62.9 at 160, 68.6 -> 66.6 at 192; two ranges of <= 128 rows keep 16 x 16
            // (75.5 ms at 256 against 79.0), profiles/r05_folded_projection_blocks.txt.  A row's bits do not depend on the block.
            if (D < 512 && !(kw == 16 && a.rows >= std::min(wide_min_rows, wide_mid_rows) && EPI == EPI_GLU_RES)) return false;
            a.stamps = nullptr;
#define TXO_DGW(KW_, BN_, RT_)                                                                                              \
            do {                                                                                                            \
                const dim3 grid((a.N + BN_ - 1) / BN_, (a.rows + DG_BM * RT_ - 1) / (DG_BM * RT_)), blk(256);                 \
                hipLaunchKernelGGL((dec_gemm_wide_kernel<T, EPI, KW_, BN_, RT_>), grid, blk, (size_t)RT_ * 8192, s, a); \
                return true;                                                                                                \
            } while (0)
            if (kw == 6) TXO_DGW(6, 32, 4);                  // K = 768: the gated out-projections, FFN-in behind its LayerNorm launch
            if constexpr (EPI == EPI_GLU_RES) {
                if (kw == 16) { if (a.rows < wide_min_rows) TXO_DGW(16, 16, 2); TXO_DGW(16, 32, 2); }   // (at the beam shape, 320 rows per range: 16 columns and / or 64 rows per block 1080-1084 against 1134 img/s)
            }
#undef TXO_DGW
            return false;
        }
    }

    // attention front half: (optional) row prologue + q / qkv projection + cached single-query attention
    struct AttnOpt {
        bool cross = false; int apro = APRO_LN2;
        const T* W = nullptr; T* K = nullptr; T* V = nullptr; int lmax = 0, len = 0;
        float* x_out = nullptr;
        int kv_div = 1; const short* path = nullptr; int t_host = -1;   // beam search: shared cross K/V, scattered self history;  t_host: the position when the host knows it (enqueue_step)
    };
    void launch_dec_attn(hipStream_t s, int li, const AttnOpt& o) {
        const auto& ln = lanes[li];
        const size_t r0 = ln.b0;
        DecAttnArgs<T> a{};
        a.y = dy + r0 * D; a.tok = cur_tok + r0; a.tok_emb = tok_emb; a.pos_emb = pos_emb; a.x_out = o.x_out;
        a.gamma = dec_g; a.beta = dec_b; a.D = D; a.W = o.W;
        const size_t kr0 = o.cross ? r0 / o.kv_div : r0;      // cross panels are per IMAGE (kv_div beams share one)
        a.K = o.K + kr0 * cfg.dec_heads * o.lmax * DH; a.V = o.V + kr0 * cfg.dec_heads * o.lmax * DH;
        a.out = dao + r0 * Id; a.heads = cfg.dec_heads; a.lmax = o.lmax; a.len = o.len; a.t_ptr = &st[li].t; a.t_host = o.t_host;
        a.qin = dq + r0 * Id; a.kv_div = o.kv_div; a.path = o.path ? o.path + r0 * Tmax : nullptr; a.path_stride = Tmax;   // slots are range-local
        a.kmask = kmask + r0 * Tmax; a.kmask_stride = Tmax;
        a.stamps = (ln.nb * cfg.dec_heads <= Stamps::BLOCKS) ? stamps.next(o.cross ? "attn cross" : "attn self") : nullptr;
        const dim3 grid(ln.nb * cfg.dec_heads), blk(256);
        constexpr int NLS = sizeof(T) == 2 ? 8 : 16;       // self: 256 cached keys per pass
        constexpr int WBS = sizeof(T) == 2 ? 3 : 1;        // self: q,k,v weight rows requested together (bf16) or one by one
        // profiling: hipExtLaunchKernelGGL binds the start/stop events to the dispatch itself (the kernel's own begin /
        // end timestamps, what rocprofv3 reports), not to marker commands around it
        hipEvent_t e0 = nullptr, e1 = nullptr;
        // light mode never creates events inside a timed region: it records until the pre-created pool is used up
        // and instruments every fourth cross-attention launch (an event-carrying launch costs ~2 us of wall time)
        const bool timed = o.cross && (prof || (prof_cross && (cross_seq++ & 3) == 0 && pool.used + 2 <= pool.ev.size()));
        if (timed) { e0 = pool.next(); e1 = pool.next(); }
        const bool narrow = (D & 255) != 0;
#define TXO_DA1(MODE, APRO, NLV, WBV, NARROW)                                                                         \
        do {                                                                                                          \
            if (timed) hipExtLaunchKernelGGL((dec_attn_kernel<T, MODE, APRO, NLV, WBV, NARROW>), grid, blk, 0, s, e0, e1, 0, a); \
            else hipLaunchKernelGGL((dec_attn_kernel<T, MODE, APRO, NLV, WBV, NARROW>), grid, blk, 0, s, a);           \
        } while (0)
#define TXO_DA(MODE, APRO, NLV, WBV)                                                                          \
        do { if (narrow) TXO_DA1(MODE, APRO, NLV, WBV, true); else TXO_DA1(MODE, APRO, NLV, WBV, false); } while (0)
#define TXO_DAR(NARROW)                                                                                             \
        do {                                                                                                        \
            if (timed) hipExtLaunchKernelGGL((dec_attn_ragged_kernel<T, DA_NL_CROSS, NARROW>), grid, blk, 0, s, e0, e1, 0, a); \
            else hipLaunchKernelGGL((dec_attn_ragged_kernel<T, DA_NL_CROSS, NARROW>), grid, blk, 0, s, a);           \
        } while (0)
        if (o.cross && ses.ragged) {                                     // per-slot key counts (dec_attn.h: RAGGED)
            a.lens = slens + kr0;
            if (narrow) TXO_DAR(true); else TXO_DAR(false);
        }
        else if (o.cross) TXO_DA(ATT_CROSS, APRO_LN2, DA_NL_CROSS, 1);
        else if (o.apro == APRO_NONE && o.path) {
            if (narrow) hipLaunchKernelGGL((dec_attn_kernel<T, ATT_SELF, APRO_NONE, NLS, 1, true, true>), grid, blk, 0, s, a);
            else hipLaunchKernelGGL((dec_attn_kernel<T, ATT_SELF, APRO_NONE, NLS, 1, false, true>), grid, blk, 0, s, a);
        }
        else if (o.apro == APRO_NONE && ses.kmask_on) {               // padding mask over the decoded positions (txo_decode_set_key_mask)
            if (narrow) hipLaunchKernelGGL((dec_attn_kernel<T, ATT_SELF, APRO_NONE, NLS, 1, true, false, true>), grid, blk, 0, s, a);
            else hipLaunchKernelGGL((dec_attn_kernel<T, ATT_SELF, APRO_NONE, NLS, 1, false, false, true>), grid, blk, 0, s, a);
        }
        else if (o.apro == APRO_NONE) TXO_DA(ATT_SELF, APRO_NONE, NLS, 1);
        else if (o.apro == APRO_EMBED) TXO_DA(ATT_SELF, APRO_EMBED, NLS, WBS);
        else TXO_DA(ATT_SELF, APRO_LN2, NLS, WBS);
#undef TXO_DAR
#undef TXO_DA
#undef TXO_DA1
        if (timed) ev_cross.push_back({e0, e1});
    }

    // Where the latent form measured faster on MI355X with launches (config.yml dims, 224x672, bf16): from 129 rows on (batch 256:
    // cross-attention launch 49 -> 32 us, 2700 -> 3290 images/s).  Up to 128 rows the persistent kernel decodes (K/V form: at one
    // (row, head group) tile per CU the latent tile moves 493 KB per CU against 300 KB and is slower, 19 vs 16 us per launch at batch
    // 64); wide decoders (768: the in-tile projections' weights are 3.4 MB per row) and the fp32 parity mode keep the K/V form.
    // the latent form's two per-head projections fold into their neighbouring GEMMs (load_attn) where the folded weights stay small
    bool latent_fold() const { return latent_ok && cfg.dec_heads * DH == 2 * D; }
    bool auto_latent(int rows) const { return sizeof(T) == 2 && D == 256 && rows > PERSIST_MAX_BF16_GREEDY; }
    // heads per latent tile: the smallest group that leaves at most one tile per CU for `rows` rows (fewer tiles = fewer
    // re-reads of an image's encoder rows; more tiles = more CUs pulling).  A head's bits do not depend on it.
    int latent_group(int rows, int slots) const {
        const int H = cfg.dec_heads;
        if (knobs.lat_g_env > 0) return std::min(std::min(H, LA_GMAX), knobs.lat_g_env);
        for (int g = 2; g < std::min(H, LA_GMAX); g *= 2)
            if (rows * ((H + g - 1) / g) <= slots) return g;
        const int n = (H + LA_GMAX - 1) / LA_GMAX;            // as few tiles per row as the tile allows, evenly filled (12 heads: one tile of 12; 24: 12 + 12)
        return (H + n - 1) / n;
    }
    // cross attention of layer l in latent form (lat_attn.h): [LN sandwich + q] -> [q' per head] -> [scores / values against the raw
    // encoder rows] -> [Wv per head]; the gated output projection follows in enqueue_step as in the K/V form
    template <int KG>
    void launch_grp_gemm(hipStream_t s, const T* A, int lda, const T* W, T* out, int ldo, int rows, int N, int NG) {
        GrpGemmArgs<T> g{A, lda, W, out, ldo, rows, N, NG};
        hipLaunchKernelGGL((grp_gemm_kernel<T, KG>), dim3((N + 63) / 64, (rows + 15) / 16), dim3(256), 0, s, g);
    }
    // the latent core over lane li's rows: q' in dqp, c to dcl.  Cross attention: enc = the session's encoder rows of the lane's first image,
    // len = ses.keys, every beam of an image reads the same rows (kv_div).  Self attention: enc = the lane's rows of the z history of one layer,
    // enc_rows = Tmax, len = position + 1 (host value or *t_ptr), kv_div = 1, path = the beams' slot tables (or null).
    // The latent core's output c feeds the folded output projection as its A operand: written in that GEMM's tiled layout (dec_gemm.h: a_tiled)
    // when the core serves the CROSS attention with folded weights.  A lane's region starts on a 16-row tile boundary and lanes do not overlap.
    size_t c_base_row(int li) const { return ((lanes.lane[li].b0 + 15) / 16) * 16 + (size_t)16 * li; }
    bool c_tiled(int l, bool cross) const { return knobs.a_tiled_on && knobs.w_tiled_on && cross && dec_cross[l].wqp != nullptr && (D * (int)sizeof(T)) % 64 == 0; }
    void launch_lat_core(hipStream_t s, int li, int kv_div, const T* enc, int len, int enc_rows, const int* t_ptr, const short* path,
                         const char* stamp_name, bool cross, int layer = 0) {
        const auto& ln = lanes[li];
        const size_t r0 = ln.b0;
        const int H = cfg.dec_heads, HD = H * D;
        LatCoreArgs<T> a{};
        a.qp = dqp + r0 * HD; a.c = dcl + r0 * HD; a.enc = enc;
        if (c_tiled(layer, cross)) { a.c = dcl + c_base_row(li) * HD; a.c_hpr = H; }
        a.rows = ln.nb; a.heads = H; a.G = latent_group(ses.rows, n_cus); a.ngrp = (H + a.G - 1) / a.G; a.len = len; a.kv_div = kv_div;
        a.enc_rows = enc_rows; a.t_ptr = t_ptr; a.path = path; a.path_stride = Tmax;
        int nimg = (ln.nb + kv_div - 1) / kv_div;
        if (cross && kv_div > 1 && ln.nb % kv_div == 0 && knobs.lat_g_env == 0) {
            // beam search: the k beams of an image read the SAME encoder rows, and their q' / c rows are contiguous ([rows][heads * D]) --
            // one image = ONE row of k * heads heads, LA_GMAX of them per tile (the MFMA tile has 16 head columns whether 8 or 16 are
            // used): 640 tiles of 8 heads become 384 of up to 16.  A head's bits do not depend on the grouping.
            a.rows = nimg; a.heads = H * kv_div; a.G = LA_GMAX; a.ngrp = (a.heads + LA_GMAX - 1) / LA_GMAX; a.kv_div = 1;
        }
        const int nblk = ((nimg + 7) / 8) * 8 * a.kv_div * a.ngrp;   // XCD-aware tile order (lat_core_kernel)
        a.stamps = (nblk <= Stamps::BLOCKS) ? stamps.next(stamp_name) : nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        const bool timed = cross && (prof || (prof_cross && (cross_seq++ & 3) == 0 && pool.used + 2 <= pool.ev.size()));
        if (timed) { e0 = pool.next(); e1 = pool.next(); }
#define TXO_LA(D_)                                                                                                           \
        do {                                                                                                                 \
            if constexpr (la_supported<T, D_>()) {                                                                           \
                auto kern = lat_core_kernel<T, D_>;                                                                          \
                const size_t lds = la_lds_bytes<T, D_>();                                                                    \
                if (timed) hipExtLaunchKernelGGL(kern, dim3(nblk), dim3(la_waves<D_>() * 64), lds, s, e0, e1, 0, a);       \
                else hipLaunchKernelGGL(kern, dim3(nblk), dim3(la_waves<D_>() * 64), lds, s, a);                            \
            }                                                                                                                \
        } while (0)
        if (D == 256 && lat_nw4) {                                // two 4-wave tiles per CU (lat_attn.h: NW_)
            if constexpr (la_supported<T, 256>() && sizeof(T) == 2) {
                auto kern = lat_core_kernel<T, 256, 4>;
                const size_t lds = la_lds_bytes<T, 256, 4>();
                if (timed) hipExtLaunchKernelGGL(kern, dim3(nblk), dim3(256), lds, s, e0, e1, 0, a);
                else hipLaunchKernelGGL(kern, dim3(nblk), dim3(256), lds, s, a);
            }
        } else if (D == 64) TXO_LA(64); else if (D == 256) TXO_LA(256); else TXO_LA(768);
#undef TXO_LA
        if (timed) ev_cross.push_back({e0, e1});
    }
    // self attention of layer l in latent form (folded weights): [embedding / LN sandwich + q' = z M^T, z appended to the history] ->
    // [scores / values against the history of z]; the gated output projection (Wo' folded) follows in enqueue_step
    int launch_lat_self(hipStream_t s, int li, int l, const BeamCtx* bm, const DecGemmArgs<T>& base, int t_host) {
        const auto& ln = lanes[li];
        const size_t r0 = ln.b0;
        const int HD = cfg.dec_heads * D;
        T* zl = zc + ((size_t)l * ses.rows + r0) * Tmax * D;           // this lane's rows of layer l's history
        DecGemmArgs<T> a = base; a.N = HD; a.K = D; a.W = dec_self[l].wqp; a.y = dy + r0 * D; a.x_out = dx + r0 * D;
        a.tok = cur_tok + r0; a.tok_emb = tok_emb; a.pos_emb = pos_emb;
        a.h_out = dqp + r0 * HD; a.F = HD; a.z_cache = zl;
        if (int r = (l == 0 ? launch_dec_gemm<PRO_EMBED, EPI_STORE_T>(s, a) : launch_dec_gemm<PRO_LN2, EPI_STORE_T>(s, a))) return r;
        launch_lat_core(s, li, 1, zl, t_host + 1, Tmax, t_host >= 0 ? nullptr : &st[li].t, bm ? bm->path_cur + r0 * Tmax : nullptr,
                        "attn self (latent core)", false);
        return 0;
    }
    int launch_lat_cross(hipStream_t s, int li, int l, int kv_div, const DecGemmArgs<T>& base) {
        const auto& ln = lanes[li];
        const size_t r0 = ln.b0;
        const int H = cfg.dec_heads, HD = H * D;
        const bool fold = dec_cross[l].wqp != nullptr;
        if (fold) {   // 1+2. x = LN(y) (residual), z = LN(x), q' = z M^T  (M = 0.125 Wk_h^T Wq_h folded at load)
            DecGemmArgs<T> a = base; a.N = HD; a.K = D; a.W = dec_cross[l].wqp; a.y = dy + r0 * D; a.x_out = dx + r0 * D;
            a.h_out = dqp + r0 * HD; a.F = HD;
            if (int r = launch_dec_gemm<PRO_LN2, EPI_STORE_T>(s, a)) return r;
        } else {
            {   // 1. x = LN(y) (residual), z = LN(x), q = z Wq^T
                DecGemmArgs<T> a = base; a.N = Id; a.K = D; a.W = dec_cross[l].wq; a.y = dy + r0 * D; a.x_out = dx + r0 * D;
                a.h_out = dqt + r0 * Id; a.F = Id;
                if (int r = launch_dec_gemm<PRO_LN2, EPI_STORE_T>(s, a)) return r;
            }
            // 2. q'_h = q_h (0.125 Wk_h)
            launch_grp_gemm<DH>(s, dqt + r0 * Id, Id, dec_cross[l].wkT, dqp + r0 * HD, HD, ln.nb, HD, D);
        }
        // 3. c_h = softmax_n(q'_h . enc[n]) enc
        launch_lat_core(s, li, kv_div, enc_t + (r0 / kv_div) * (size_t)ses.keys * D, ses.keys, 0, nullptr, nullptr, "attn cross (latent core)", true, l);
        if (fold) return 0;                                       // 4+5: the gated output projection takes c directly (K = heads*D, Wo' folded at load)
        // 4. o_h = c_h Wv_h^T ; 'b h n d -> b n (h d)'
        if (D == 64) launch_grp_gemm<64>(s, dcl + r0 * HD, HD, dec_cross[l].wv, dao + r0 * Id, Id, ln.nb, Id, DH);
        else if (D == 256) launch_grp_gemm<256>(s, dcl + r0 * HD, HD, dec_cross[l].wv, dao + r0 * Id, Id, ln.nb, Id, DH);
        else launch_grp_gemm<768>(s, dcl + r0 * HD, HD, dec_cross[l].wv, dao + r0 * Id, Id, ln.nb, Id, DH);
        return 0;
    }

    // one decode position of lane `li` on stream s; tokens_out/logits_out are GLOBAL-batch base pointers
    // host_t: the decode position when the caller knows it (every eager loop does); -1 makes the kernels read the
    // device-side counter instead, which is what lets ONE captured graph serve every step
    // logp_out: [rows][out_stride] like tokens_out, or null (step.h: StepArgs::logp_out)
    int enqueue_step(hipStream_t s, int li, int64_t* tokens_out, int out_stride, float* logits_out, float* logp_out, int eos,
                     const BeamCtx* bm = nullptr, int host_t = -1) {
        const auto& ln = lanes[li];
        const int B = ses.rows, N = ses.keys, nb = ln.nb;
        const size_t r0 = ln.b0;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (prof) { e0 = pool.next(); e1 = pool.next(); (void)hipEventRecord(e0, s); }
        DecGemmArgs<T> base{};
        base.rows = nb; base.gamma = dec_g; base.beta = dec_b; base.t_ptr = &st[li].t; base.t_host = host_t; base.D = D;
        base.inner = Id; base.heads = cfg.dec_heads; base.tmax = Tmax;
        float* lx = dx + r0 * D; float* ly = dy + r0 * D; T* lao = dao + r0 * Id; T* lhid = dhid + r0 * Fd;
        float* llog = dlogits + r0 * V;
        const size_t self_stride = (size_t)B * Id * Tmax, cross_stride = (size_t)ses.images * N * Id;
        for (int l = 0; l < cfg.dec_layers; ++l) {
            T* kc = skv + (size_t)(2 * l) * self_stride; T* vc = skv + (size_t)(2 * l + 1) * self_stride;
            if (ses.lat_self) {   // causal self attention against the history of normalised block inputs (lat_attn.h)
                if (int r = launch_lat_self(s, li, l, bm, base, host_t)) return r;
                dbg(s, "self attn (latent)", l);
                DecGemmArgs<T> g = base; g.N = 2 * D; g.K = cfg.dec_heads * D; g.W = dec_self[l].wo_f; g.bias = dec_self[l].bo;
                g.A = dcl + r0 * cfg.dec_heads * D; g.resid = lx; g.y_out = ly;
                if (!launch_dec_gemm_wide<EPI_GLU_RES>(s, g)) { if (int r = launch_dec_gemm<PRO_NONE, EPI_GLU_RES>(s, g)) return r; }
                dbg(s, "self out", l);
            } else {   // causal self attention
                AttnOpt o; o.W = dec_self[l].wqkv; o.K = kc; o.V = vc; o.lmax = Tmax; o.x_out = lx; o.t_host = host_t;
                if (bm) o.path = bm->path_cur;
                if (knobs.self_plain || bm || ses.kmask_on) {
                    // default: LN sandwich + QKV GEMM (weights read once per 16 rows; k/v appended to the cache by
                    // its epilogue), then the plain cached attention.  TXO_SELF_FUSED=1 folds the projection into
                    // the attention launch instead (same wall time at B=64; re-reads 96 KB of weights per image).
                    DecGemmArgs<T> a = base; a.N = 3 * Id; a.K = D; a.W = dec_self[l].wqkv; a.y = ly; a.x_out = lx;
                    a.tok = cur_tok + r0; a.tok_emb = tok_emb; a.pos_emb = pos_emb;
                    a.q_out = dq + r0 * Id;
                    a.k_cache = kc + r0 * cfg.dec_heads * Tmax * DH; a.v_cache = vc + r0 * cfg.dec_heads * Tmax * DH;
                    // (one LayerNorm launch + the projection on 64-row blocks, as the out-projections and FFN-in below do at >= 128
                    // rows of a wide decoder, measured the same 17.7 us as this fused launch at 256 x 768: not used here)
                    if (int r = (l == 0 ? launch_dec_gemm<PRO_EMBED, EPI_QKV>(s, a) : launch_dec_gemm<PRO_LN2, EPI_QKV>(s, a))) return r;
                    o.apro = APRO_NONE;
                } else {
                    o.apro = l == 0 ? APRO_EMBED : APRO_LN2;
                }
                launch_dec_attn(s, li, o);
                dbg(s, "self attn", l);
                DecGemmArgs<T> g = base; g.N = 2 * D; g.K = Id; g.W = dec_self[l].wo; g.bias = dec_self[l].bo; g.A = lao;
                g.resid = lx; g.y_out = ly;
                if (!launch_dec_gemm_wide<EPI_GLU_RES>(s, g)) { if (int r = launch_dec_gemm<PRO_NONE, EPI_GLU_RES>(s, g)) return r; }
                dbg(s, "self out", l);
            }
            {   // cross attention (LN sandwich + q projection fused in): against the raw encoder rows (latent form) or over the cached projections
                const bool fold = ses.latent && dec_cross[l].wqp != nullptr;
                if (ses.latent) { if (int r = launch_lat_cross(s, li, l, bm ? bm->k : 1, base)) return r; }
                else {
                AttnOpt o; o.cross = true; o.W = dec_cross[l].wq; o.K = ckv + (size_t)(2 * l) * cross_stride;
                o.V = ckv + (size_t)(2 * l + 1) * cross_stride; o.lmax = N; o.len = N; o.x_out = lx; o.t_host = host_t;
                if (bm) o.kv_div = bm->k;
                launch_dec_attn(s, li, o);
                }
                dbg(s, "cross attn", l);
                DecGemmArgs<T> g = base; g.N = 2 * D; g.K = Id; g.W = dec_cross[l].wo; g.bias = dec_cross[l].bo; g.A = lao;
                g.resid = lx; g.y_out = ly;
                if (fold) {
                    g.K = cfg.dec_heads * D; g.W = dec_cross[l].wo_f; g.A = dcl + r0 * cfg.dec_heads * D;
                    if (c_tiled(l, true)) { g.A = dcl + c_base_row(li) * cfg.dec_heads * D; g.a_tiled = 1; }
                }
                if (!launch_dec_gemm_wide<EPI_GLU_RES>(s, g)) { if (int r = launch_dec_gemm<PRO_NONE, EPI_GLU_RES>(s, g)) return r; }
                dbg(s, "cross out", l);
            }
            {   // GeGLU feed-forward
                if (sizeof(T) == 2 && D >= 512 && nb >= 128 && dec_mlp[l].w1_16) {
                    // perf mode, wide rows (ViT-Base decoder: 768), >= 128 rows: the 16-row launch would be 3072 blocks that each
                    // redo the LayerNorm sandwich of their rows (39 us); one LayerNorm launch + the 128x128 GEMM takes ~15 us.
                    // (fp32 parity mode keeps the 16-row kernel at every batch size: a row's bits never depend on the batch.)
                    launch_ln<1>(s, ly, lx, dz + r0 * D, dec_g, dec_b, nb);
                    DecGemmArgs<T> w = base; w.N = 2 * Fd; w.K = D; w.W = dec_mlp[l].w1; w.bias = dec_mlp[l].b1; w.A = dz + r0 * D;
                    w.h_out = lhid; w.F = Fd;
                    if (!launch_dec_gemm_wide<EPI_GEGLU>(s, w))
                        launch_gemm_big<T>(s, LoadPlain<T>{dz + r0 * D, D}, dec_mlp[l].w1_16, nb, 2 * Fd, D, EpiGeglu<T>{lhid, dec_mlp[l].b1_16, Fd});
                } else {
                    DecGemmArgs<T> a = base; a.N = 2 * Fd; a.K = D; a.W = dec_mlp[l].w1; a.bias = dec_mlp[l].b1; a.y = ly; a.x_out = lx;
                    a.h_out = lhid; a.F = Fd;
                    if (int r = launch_dec_gemm<PRO_LN2, EPI_GEGLU>(s, a)) return r;
                }
                dbg(s, "ffn1", l);
                DecGemmArgs<T> g = base; g.N = D; g.K = Fd; g.W = dec_mlp[l].w2; g.bias = dec_mlp[l].b2; g.A = lhid;
                g.resid = lx; g.y_out = ly;
                if (int r = launch_dec_gemm<PRO_NONE, EPI_BIAS_RES>(s, g)) return r;   // (blocks of 32 / 64 rows x 16 / 32 columns at K = 3072 on two ranges: 840 / 808 / 823 / 784 img/s against 844 -- not used)
            }
        }
        DecGemmArgs<T> f = base; f.N = V; f.K = D; f.W = wlog; f.bias = blog; f.logits = llog;
        f.y = ly; f.gamma = decn_g; f.beta = decn_b;
        if (int r = launch_dec_gemm<PRO_LNF, EPI_LOGITS>(s, f)) return r;
        dbg(s, "logits");
        StepArgs sa{llog, V, nb, cur_tok + r0, tokens_out ? tokens_out + r0 * out_stride : nullptr, out_stride,
                    logits_out ? logits_out + r0 * (size_t)out_stride * V : nullptr, st + li, eos_seen + r0,
                    done_flag + (size_t)li * Tmax, eos, sample_topk, 1.0f / sample_temp, sample_seed, (int)r0,
                    ses.row_stop ? 1 : 0, ses.row_stop ? row_map + r0 : nullptr,
                    logp_out ? logp_out + r0 * out_stride : nullptr};
        if (ses.forced) {   // prompted decode: the range's slices of the prefix table, indexed through row_map like the outputs
            sa.forced = ftab + r0 * Tmax; sa.forced_stride = Tmax; sa.forced_len = flen + r0; sa.out_cols = prefix_cols; sa.prefix_logp = fplogp + r0 * Tmax;
        }
        if (ses.ruled) {    // constrained decode: the table, and the range's slices of the states (through row_map like the outputs)
            sa.rules = rules_dev; sa.n_states = rules_S; sa.depth_max = rules_dmax; sa.rule_state = rule_state + r0;
            sa.rule_hist = rule_hist + r0 * Tmax; sa.rule_hist_stride = Tmax;
            if (ses.closing) { sa.close_tab = close_dev; sa.rule_close = rule_close + r0; }
        }
        sa.guard_p = ses.guard_p; sa.guard_r = ses.guard_r;
        // alternatives: the raw row's k best in front of whatever pick follows, on the same stream (never a beam step: beam_search refuses)
        if (ses.alts > 0 && !bm)
            hipLaunchKernelGGL(alts_step_kernel, dim3(nb), dim3(64), 0, s, sa,
                               AltsArgs{alt_ids + r0 * Tmax * ses.alts, alt_logp + r0 * Tmax * ses.alts, ses.alts, Tmax});
        if (bm) {
            BeamArgs ba{llog, V, bm->k, nb / bm->k, cur_tok + r0, bscore + r0, bfin + r0, bm->path_cur + r0 * Tmax, bm->path_nxt + r0 * Tmax, Tmax,
                        bparent + r0, btok + r0, Bmax, bm->logp ? blogp + r0 : nullptr, st + li, done_flag + (size_t)li * Tmax, eos, (int)r0};
            // every form of the selection through one launch (beam_guard.h: launch_beam_select).  ra: the table and the range's slice of the
            // slots' states (range-local, like every pointer of ba), nulls without rules; ca: the distance table, null unless closing.  A
            // guarded search is one kernel with or without the rules and the budget; the plain form reads none of ra / ca / the guard's pair
            const BeamRuleArgs ra{bm->ruled ? rules_dev : nullptr, bm->ruled ? rules_S : 0, bm->ruled ? rules_dmax : 0, bm->ruled ? brule_state + r0 : nullptr};
            const BeamCloseArgs ca{bm->closing ? close_dev : nullptr, bm->positions};
            const BeamForm form = bm->guard_p > 0 ? BeamForm::guard : !bm->ruled ? BeamForm::plain : bm->closing ? BeamForm::close : BeamForm::rules;
            launch_beam_select(s, ba, ra, ca, BeamGuardArgs{bm->guard_p, bm->guard_r}, form, bm->logp);
        } else if (ses.guarded()) launch_guard_step(s, nb, sa, sample_mode != 0);   // (with or without rules; never closing: generate refuses)
        else if (ses.closing) launch_rules_close_step(s, nb, sa, sample_mode != 0);
        else if (ses.ruled) launch_rules_step(s, nb, sa, sample_mode != 0);
        else if (ses.forced) launch_prefix_step(s, nb, sa, sample_mode != 0);
        else if (sample_mode) launch_sample_step(s, nb, sa);
        else hipLaunchKernelGGL(argmax_step_kernel, dim3(nb), dim3(64), 0, s, sa);
        dbg(s, "argmax");
        if (prof) { (void)hipEventRecord(e1, s); ev_step.push_back({e0, e1}); }
        return 0;
    }

    // capture lane li's step (tokens into the engine-owned tok_buf) as a graph, or reuse the cached one
    // logp: the step also writes its log-probabilities, into the engine-owned logp_buf (part of the key: it is another StepArgs)
    int lane_graph(int li, int eos, bool logp) {
        const auto& ln = lanes[li];
        const LaneSet::GraphKey key = ses.graph_key(ln, eos, sample_mode, logp, rules_S * 256 + rules_dmax + (ses.closing ? 4096 : 0));   // (ses.alts is in it)   // (S * 256 + depth cap < 4096)
        if (lanes.cached(li, key)) return 0;
        hipStream_t cs = lanes.cap_stream;
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        HIP_TRY(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
        const int r = enqueue_step(cs, li, tok_buf, Tmax, nullptr, logp ? logp_buf : nullptr, eos);
        hipError_t e = hipStreamEndCapture(cs, &graph);
        if (r) return r;
        if (e != hipSuccess) return fail(TXO_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        HIP_TRY(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        lanes.add(li, key, graph, exec);
        return 0;
    }

    int decode_step(const int64_t* tok_in, int t, float* logits_out, int64_t* tok_out, hipStream_t s) override {
        if (!ses.open) return fail(TXO_E_STATE, "txo_decode_begin has not been called");
        if (t < 0 || t >= Tmax)
            return fail(TXO_E_INVALID, "position outside the decoder's positional table (the reference would slide its "
                                       "window, decoder.py:99-100; a KV cache cannot reproduce that)");
        if (lanes.n != 1) return fail(TXO_E_STATE, "decode_step needs a session started by txo_decode_begin");
        lanes[0].stream = s;
        if (tok_in) hipLaunchKernelGGL(copy_tokens_kernel, dim3((ses.rows + 255) / 256), dim3(256), 0, s, cur_tok, tok_in, ses.rows, V);
        hipLaunchKernelGGL(set_position_kernel, dim3(1), dim3(1), 0, s, st, t);
        if (int r = enqueue_step(s, 0, nullptr, 0, nullptr, nullptr, -1, nullptr, t)) return r;
        if (logits_out) HIP_TRY(hipMemcpyAsync(logits_out, dlogits, sizeof(float) * ses.rows * V, hipMemcpyDeviceToDevice, s));
        if (tok_out) HIP_TRY(hipMemcpyAsync(tok_out, cur_tok, sizeof(int64_t) * ses.rows, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // Padding mask of decoder.generate / decoder.net (reference decoder.py:95-101,112; attention.py:130-155): mask [B][cols] bytes,
    // 0 = the position is padding.  Its effect on every position that is NOT itself padding: padded positions are never attended by
    // the causal self attention (energy filled with -FLT_MAX).  Rows of padded positions are computed but unspecified (the reference
    // softmaxes them uniformly over all keys, future ones included; nothing reads them).  Applies to txo_decode_step of this session.
    int decode_set_key_mask(const unsigned char* mask, int cols, hipStream_t s) override {
        if (!ses.open) return fail(TXO_E_STATE, "txo_decode_begin has not been called");
        if (ses.images != ses.rows) return fail(TXO_E_STATE, "key masks are not available inside a beam-search session");
        if (ses.ragged && !rag_fwd) return refuse_ragged_forward("txo_decode_set_key_mask");
        if (!mask) { ses.kmask_on = false; return 0; }
        if (cols < 1 || cols > Tmax) return fail(TXO_E_INVALID, "mask columns must be in [1, max_length]");
        const int n = ses.rows * Tmax;
        hipLaunchKernelGGL(set_key_mask_kernel, dim3((n + 255) / 256), dim3(256), 0, s, mask, kmask, ses.rows, cols, Tmax);
        ses.kmask_on = true;
        HIP_TRY(hipGetLastError());
        return 0;
    }

    struct AttnOut { float* self_p; float* cross_p; float* cross_mean; };   // attention maps of every layer (decode_attn), each may be null
    // the multi-position forward on the open session, with (decode_attn) or without (decode_prefill) the attention maps
    int prefill_entry(const std::string& name, const int64_t* tokens, int t, float* logits_out, const AttnOut* attn, hipStream_t s) {
        if (lanes.n != 1) return fail(TXO_E_STATE, name + " needs a session started by txo_decode_begin");
        if (ses.images != ses.rows) return fail(TXO_E_STATE, name + " is not available inside a beam-search session");
        if (ses.open && ses.ragged && !rag_fwd) return refuse_ragged_forward("txo_" + name);
        lanes[0].stream = s;
        return prefill(tokens, t, t, logits_out, nullptr, s, nullptr, attn);
    }
    int decode_prefill(const int64_t* tokens, int t, float* logits_out, hipStream_t s) override {
        return prefill_entry("decode_prefill", tokens, t, logits_out, nullptr, s);
    }
    // decode_prefill that also writes the attention probabilities of every decoder layer (attn_probs.h): self [Ld][B][heads][t][t],
    // cross [Ld][B][heads][t][N], the head mean of the cross maps [Ld][B][t][N]; each may be null
    int decode_attn(const int64_t* tokens, int t, float* logits_out, float* self_attn_out, float* cross_attn_out, float* cross_mean_out,
                    hipStream_t s) override {
        // (the head walk keeps its statistics in LDS beside the kernel's 32 KB of tiles, inside the 64 KB every launch may ask for)
        if (cross_mean_out && attn_probs_lds_bytes(cfg.dec_heads) > 32768)
            return fail(TXO_E_INVALID, "txo_decode_attn: the head-mean map is built for at most 32 decoder heads");
        const AttnOut ao{self_attn_out, cross_attn_out, cross_mean_out};
        return prefill_entry("decode_attn", tokens, t, logits_out, &ao, s);
    }

    // AutoRegressiveDecoder.forward without autograd (decoder.py:124-145): tokens [B][L]; columns 0..L-2 are fed through the
    // multi-position forward, column p + 1 is the target of position p; per-position scores from the fused kernel of score.h
    // per-position scores [B][L-1] (each may be null), and with k > 0 the k best ids / log-probabilities of every row [B][L-1][k] (score.h: the
    // k-best form of the fused kernel; txo_decode_score_alts / txo_score_alts)
    struct ScoreOut { float* logp; int64_t* top1; float* top1_logp; int k = 0; int32_t* alt_ids = nullptr; float* alt_logp = nullptr; };
    int decode_score(const int64_t* tokens, int L, float* logp_out, int64_t* top1_out, float* top1_logp_out, hipStream_t s) override {
        return decode_score_to(tokens, L, ScoreOut{logp_out, top1_out, top1_logp_out}, s);
    }
    int decode_score_alts(const int64_t* tokens, int L, float* logp_out, int64_t* top1_out, float* top1_logp_out, int k, int32_t* alt_ids_out,
                          float* alt_logp_out, hipStream_t s) override {
        return decode_score_to(tokens, L, ScoreOut{logp_out, top1_out, top1_logp_out, k, alt_ids_out, alt_logp_out}, s);
    }
    int decode_score_to(const int64_t* tokens, int L, const ScoreOut& so, hipStream_t s) {
        if (!ses.open) return fail(TXO_E_STATE, "txo_decode_begin has not been called");
        if (lanes.n != 1) return fail(TXO_E_STATE, "decode_score needs a session started by txo_decode_begin");
        if (ses.images != ses.rows) return fail(TXO_E_STATE, "decode_score is not available inside a beam-search session");
        if (ses.ragged && !rag_fwd) return refuse_ragged_forward("txo_decode_score");
        return score_pass(tokens, L, so, s);
    }
    // (the session is open, has one row per image and one row range: decode_score checked it, or txo_score / txo_score_ragged just opened it)
    int score_pass(const int64_t* tokens, int L, const ScoreOut& so, hipStream_t s) {
        lanes[0].stream = s;
        return prefill(tokens, L, L - 1, nullptr, nullptr, s, &so);
    }

    // OCRModel.forward's path (ocr_model.py:38-44) in one call: encode into the engine's own buffer, open the session, mask, score
    int score(const float* img, int B, int C, int H, int W, const int64_t* tokens, const unsigned char* mask, int L, float* logp_out,
              int64_t* top1_out, float* top1_logp_out, hipStream_t s) override {
        return score_to(img, B, C, H, W, tokens, mask, L, ScoreOut{logp_out, top1_out, top1_logp_out}, s);
    }
    int score_alts(const float* img, int B, int C, int H, int W, const int64_t* tokens, const unsigned char* mask, int L, float* logp_out,
                   int64_t* top1_out, float* top1_logp_out, int k, int32_t* alt_ids_out, float* alt_logp_out, hipStream_t s) override {
        return score_to(img, B, C, H, W, tokens, mask, L, ScoreOut{logp_out, top1_out, top1_logp_out, k, alt_ids_out, alt_logp_out}, s);
    }
    int score_to(const float* img, int B, int C, int H, int W, const int64_t* tokens, const unsigned char* mask, int L, const ScoreOut& so, hipStream_t s) {
        if (ses.open && ses.ragged && !rag_fwd) return refuse_ragged_forward("txo_score (a ragged batch session is open)");
        if (int r = encode(img, B, C, H, W, eenc, s)) return r;
        if (int r = begin_session(eenc, B, 1 + (H / 16) * (W / 16), cfg.eos, s, true)) return r;
        return score_open_session(tokens, mask, L, so, s);
    }
    // the tail txo_score and txo_score_ragged share: the [B][L] mask's first L - 1 columns as the key mask, the scores, the mask cleared
    int score_open_session(const int64_t* tokens, const unsigned char* mask, int L, const ScoreOut& so, hipStream_t s) {
        if (mask) {
            const int n = ses.rows * Tmax;
            hipLaunchKernelGGL(set_key_mask_strided_kernel, dim3((n + 255) / 256), dim3(256), 0, s, mask, kmask, ses.rows, L, L - 1, Tmax);
            ses.kmask_on = true;
        }
        const int rc = score_pass(tokens, L, so, s);
        ses.kmask_on = false;
        return rc;
    }
    // txo_score over a ragged container: every row is what txo_score returns for that image passed on its own
    int score_ragged(const float* img, int B, int C, int Hc, int Wc, const int32_t* sizes, const int64_t* tokens, const unsigned char* mask, int L,
                     float* logp_out, int64_t* top1_out, float* top1_logp_out, hipStream_t s) override {
        ImageBatch ib;
        if (int r = ragged_batch(B, C, Hc, Wc, sizes, s, &ib)) return r;
        if (int r = encode_batch(ib, img, eenc, s)) return r;
        if (int r = begin_session(eenc, B, ib.N, cfg.eos, s, true, KeyCounts{rag_ntok})) return r;
        return score_open_session(tokens, mask, L, ScoreOut{logp_out, top1_out, top1_logp_out}, s);
    }

    // ---- multi-position decoder forward (prefill.h): Transformer.forward over t positions at once, filling the self K/V cache ----
    // tokens [B][tok_stride] (the first t of each row); logits_out [B][t][V] or null; last_logits [B][V] or null (final LN + logits of
    // position t-1 only, on the single-position launch); score: per-position scores [B][t] against the targets tokens[b][p + 1]
    // (tok_stride > t then) or null.  Runs in the encoder's workspace, image chunks of as many rows as fit.
    template <typename TO>
    void launch_attn_mq(hipStream_t s, bool causal, const T* q, const T* k, const T* v, TO* out, int nb, int nq, int nk, int kv_rows,
                        const unsigned char* km = nullptr, const int* lens = nullptr) {
        const dim3 grid((nq + EA_QBLK - 1) / EA_QBLK, nb * cfg.dec_heads);
        if (!causal || lens) km = nullptr;                    // (only the causal self attention of a fixed-shape session reads the padding mask)
        auto kern = attn_mq_kernel<T, TO, false, false, true>;   // lens: cross attention of a ragged session, nk = lens[image], panels kv_rows apart
        if (!lens) {                                          // (assigned in the order the kernels have in the code object: see wide_min_rows)
            if (causal) kern = km ? attn_mq_kernel<T, TO, true, true> : attn_mq_kernel<T, TO, true>;
            else kern = attn_mq_kernel<T, TO, false>;
        }
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, q, k, v, out, nq, nk, kv_rows, cfg.dec_heads, km, km ? Tmax : 0, lens);
    }
    // the probabilities behind a launch_attn_mq call, from the same q / k (attn_probs.h); MEAN: one map per image, the mean over the heads
    template <bool MEAN>
    void launch_attn_probs(hipStream_t s, bool causal, const T* q, const T* k, float* out, int nb, int nq, int nk, int kv_rows,
                           const unsigned char* km = nullptr, const int* lens = nullptr) {
        const int heads = cfg.dec_heads;
        const dim3 grid((nq + EA_QBLK - 1) / EA_QBLK, MEAN ? nb : nb * heads);
        const size_t lds = attn_probs_lds_bytes(MEAN ? heads : 1);
        if (MEAN) causal = false;                             // only the cross maps have a head mean: no causal form of it exists
        if (!causal || lens) km = nullptr;
        auto kern = attn_probs_kernel<T, false, false, MEAN, true>;   // lens: the cross maps of a ragged session
        if (!lens) {
            if constexpr (!MEAN) { if (causal) kern = km ? attn_probs_kernel<T, true, true, false> : attn_probs_kernel<T, true, false, false>; }
            if (!causal) kern = attn_probs_kernel<T, false, false, MEAN>;
        }
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, q, k, out, nq, nk, kv_rows, heads, km, km ? Tmax : 0, lens);
    }
    int prefill(const int64_t* tokens, int tok_stride, int t, float* logits_out, float* last_logits, hipStream_t s, const ScoreOut* score = nullptr,
                const AttnOut* attn = nullptr) {
        if (!ses.open) return fail(TXO_E_STATE, "txo_decode_begin has not been called");
        if (t < 1 || t > Tmax) return fail(TXO_E_INVALID, "prefill length outside the decoder's positional table");
        // (only the logits GEMM's 8-wide store epilogue needs it: the scoring tail takes any vocabulary)
        if (logits_out && V % 8) return fail(TXO_E_INVALID, "prefill needs a vocabulary size that is a multiple of 8");
        const size_t cap = (size_t)Bmax * Nmax;               // rows of the encoder workspace
        if ((size_t)t > cap) return fail(TXO_E_INVALID, "prefill: one prefix does not fit the engine's workspace (max_batch * max_tokens rows)");
        const int B = ses.rows, N = ses.keys, heads = cfg.dec_heads;
        ensure_ckv(s);
        const int bc = (int)std::min<size_t>(B, cap / t);     // images per chunk
        const size_t self_stride = (size_t)B * Id * Tmax, cross_stride = (size_t)ses.images * N * Id;
        T* qbuf = reinterpret_cast<T*>(eqkv);
        for (int b0 = 0; b0 < B; b0 += bc) {
            const int nb = std::min(bc, B - b0), M = nb * t;
            {
                const size_t n4 = (size_t)M * (D / 4);
                hipLaunchKernelGGL(embed_rows_kernel, dim3((n4 + 255) / 256), dim3(256), 0, s, tokens + (size_t)b0 * tok_stride, tok_stride,
                                   tok_emb, pos_emb, ex, M, t, D, V);
            }
            for (int l = 0; l < cfg.dec_layers; ++l) {
                // the shared-LN sandwich exactly as in encode(): x = LN(y) is never written, the GEMM epilogues rebuild it
                const ResidLN res_x{ey, estats, dec_gb, D}, res_first{ex, nullptr, nullptr, D};
                if (l == 0) launch_ln<0, T>(s, ex, nullptr, ez, dec_g, dec_b, M);
                else launch_ln<3, T>(s, ey, estats, ez, dec_g, dec_b, M);
                T* kc = skv + (size_t)(2 * l) * self_stride + (size_t)b0 * heads * Tmax * DH;
                T* vc = skv + (size_t)(2 * l + 1) * self_stride + (size_t)b0 * heads * Tmax * DH;
                gemm_plain(s, ez, dec_self[l].wqkv, M, 3 * Id, D, EpiHeadsKV<T>{qbuf, kc, vc, Id, heads, t, Tmax});
                launch_attn_mq<T>(s, true, qbuf, kc, vc, eao, nb, t, t, Tmax, ses.kmask_on ? kmask + (size_t)b0 * Tmax : nullptr);   // (padding mask of the session, if any)
                if (attn && attn->self_p)                     // [Ld][B][heads][t][t], before the cross attention's q overwrites qbuf
                    launch_attn_probs<false>(s, true, qbuf, kc, attn->self_p + ((size_t)l * B + b0) * heads * t * t, nb, t, t, Tmax,
                                             ses.kmask_on ? kmask + (size_t)b0 * Tmax : nullptr);
                gemm_plain(s, eao, dec_self[l].wo16, M, 2 * D, Id, EpiGluRes<sizeof(T) == 2>{ey, l == 0 ? res_first : res_x, dec_self[l].bo16});
                // cross attention over the cached encoder projections (attention.py:114-126); one row per image: no prefill in a beam session
                launch_ln<3, T>(s, ey, estats, ez, dec_g, dec_b, M);
                gemm_plain(s, ez, dec_cross[l].wq, M, Id, D, EpiHeads<T>{qbuf, 0, Id, heads, t});
                const T* ck = ckv + (size_t)(2 * l) * cross_stride + (size_t)b0 * heads * N * DH;
                const T* cv = ckv + (size_t)(2 * l + 1) * cross_stride + (size_t)b0 * heads * N * DH;
                // a ragged session: N is the slot stride Ns and image b attends its own slens[b] keys; the counts move with the chunk
                const int* lens = ses.ragged ? slens + b0 : nullptr;
                launch_attn_mq<T>(s, false, qbuf, ck, cv, eao, nb, t, N, N, nullptr, lens);
                if (attn && attn->cross_p)                    // [Ld][B][heads][t][N]
                    launch_attn_probs<false>(s, false, qbuf, ck, attn->cross_p + ((size_t)l * B + b0) * heads * t * N, nb, t, N, N, nullptr, lens);
                if (attn && attn->cross_mean)                 // [Ld][B][t][N]
                    launch_attn_probs<true>(s, false, qbuf, ck, attn->cross_mean + ((size_t)l * B + b0) * t * N, nb, t, N, N, nullptr, lens);
                gemm_plain(s, eao, dec_cross[l].wo16, M, 2 * D, Id, EpiGluRes<sizeof(T) == 2>{ey, res_x, dec_cross[l].bo16});
                // GeGLU feed-forward
                launch_ln<3, T>(s, ey, estats, ez, dec_g, dec_b, M);
                gemm_plain(s, ez, dec_mlp[l].w1_16, M, 2 * Fd, D, EpiGeglu<T>{ehid, dec_mlp[l].b1_16, Fd});
                gemm_plain(s, ehid, dec_mlp[l].w2, M, D, Fd, EpiBiasRes{ey, res_x, dec_mlp[l].b2});
            }
            if (logits_out) {                                 // decoder.py:57-60 over every position
                launch_ln<2, T>(s, ey, nullptr, ez, decn_g, decn_b, M);
                gemm_plain(s, ez, wlog, M, V, D, EpiStore<float>{logits_out + (size_t)b0 * t * V, V, blog});
            }
            if (score && (score->logp || score->top1 || score->top1_logp || score->k > 0)) {   // decoder.py:141-145 without the logits: score.h
                launch_ln<2, T>(s, ey, nullptr, ez, decn_g, decn_b, M);
                const int nw = score_waves<T>(D);
                const size_t o = (size_t)b0 * t;
                if (score->k > 0)
                    hipLaunchKernelGGL((score_rows_alts_kernel<T>), dim3((M + nw * SC_ROWS - 1) / (nw * SC_ROWS)), dim3(64 * nw),
                                       (size_t)nw * SC_ROWS * D * sizeof(T), s, ez, wlog, blog, tokens + (size_t)b0 * tok_stride, tok_stride, t, M, D, V,
                                       score->logp ? score->logp + o : nullptr, score->top1 ? score->top1 + o : nullptr,
                                       score->top1_logp ? score->top1_logp + o : nullptr, score->k, score->alt_ids + o * score->k,
                                       score->alt_logp + o * score->k);
                else
                hipLaunchKernelGGL((score_rows_kernel<T>), dim3((M + nw * SC_ROWS - 1) / (nw * SC_ROWS)), dim3(64 * nw),
                                   (size_t)nw * SC_ROWS * D * sizeof(T), s, ez, wlog, blog, tokens + (size_t)b0 * tok_stride, tok_stride, t, M, D, V,
                                   score->logp ? score->logp + o : nullptr, score->top1 ? score->top1 + o : nullptr,
                                   score->top1_logp ? score->top1_logp + o : nullptr);
            }
            if (last_logits) {                                // the last position only: the step path's final-LN + logits launch on gathered rows
                hipLaunchKernelGGL(gather_last_rows_kernel, dim3((nb * D + 255) / 256), dim3(256), 0, s, ey, dy + (size_t)b0 * D, nb, t, D);
            }
        }
        if (last_logits) {
            DecGemmArgs<T> f{};
            f.rows = B; f.D = D; f.inner = Id; f.heads = heads; f.tmax = Tmax; f.t_host = t - 1; f.t_ptr = &st[0].t;
            f.N = V; f.K = D; f.W = wlog; f.bias = blog; f.logits = last_logits; f.y = dy; f.gamma = decn_g; f.beta = decn_b;
            if (int r = launch_dec_gemm<PRO_LNF, EPI_LOGITS>(s, f)) return r;
        }
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // ---- the decode loop as ONE persistent launch (persist.h) -------------------------------------------------------
    // Which decode path?  TXO_PERSIST=1 / 0 forces the persistent launch on / off (where it exists: decoder width 256 with 8
    // heads, or 768 with 12 heads in bf16, FFN factor 4).  Default: where it measured faster on MI355X (config.yml dims, 224x672,
    // 256 steps; profiles/r02_persist_ab.txt, last table): width 256, every batch size up to 256 images in both modes -- bf16
    // 22.9 vs 29.1 ms for ONE image, 1998 vs 1522 images/s at batch 64, 2717 vs 2605 at 256; fp32 1094 vs 903 at batch 64.
    static constexpr int PERSIST_MAX_BF16_GREEDY = 128;
    bool persist_usable(int B) const {
        // sampling: the persistent kernel's sampler keeps a row in registers, 16 logits per lane (step.h: sample_row_regs)
        if (sample_mode && V > 64 * SR_PER) return false;
        if (prof || prof_cross || g_dbg || knobs.run.stamps || knobs.run.graph >= 0 || knobs.run.lanes > 0) return false;
        if (ses.ragged) return false;                                 // a ragged batch decodes with launches (persist.h has no per-row key count)
        if (ses.forced) return false;                                 // so does a prompted decode (persist.h starts at BOS and forces nothing)
        if (ses.ruled) return false;                                  // and a constrained one (persist.h picks without rules)
        if (ses.guarded()) return false;                              // and a guarded one (persist.h keeps no ban set)
        if (ses.alts > 0) return false;                               // and one that keeps alternatives (persist.h picks without them)
        if (cfg.dec_exp != 4 || cfg.dec_layers > PS_MAXLD) return false;
        const bool exists = (D == 256 && cfg.dec_heads == 8) || (D == 768 && cfg.dec_heads == 12 && sizeof(T) == 2);
        if (!exists) return false;
        if (latent_ok && knobs.lat_mode == 1) return false;           // latent form forced: the persistent kernel reads projected K/V panels
        if (knobs.run.persist >= 0) return knobs.run.persist != 0;
        if (persist_cooldown > 0) return false;                // it gave up twice in a row (not all 256 workgroups co-resident?): not tried for a while
        if (D != 256) return false;                            // the 768-wide variant is opt-in (TXO_PERSIST=1): not measured faster
        // bf16 beyond 128 images: launches with the cross attention in latent form (one row range, two from 224 rows on) are ahead of the
        // persistent launch -- greedy 160: 66.6 vs 72.7 ms, 192: 70.6 vs 79.7, 256: 77.9 vs 99.0; sampled 160: 68.9 vs 73.4, 192: 73.0 vs 80.6, 256: 84.5
        // (one range) vs 99.7; at 128 the persistent launch leads (greedy 54.2 vs 56.7, sampled 55.2 vs 58.4).  fp32: persistent up to 256
        if (sizeof(T) == 2 && B > PERSIST_MAX_BF16_GREEDY) return false;
        return B <= 256;                                       // more rows per team than two 16-row tiles: not measured
    }
    template <int D_, int H_>
    int launch_persist(const PersistArgs<T>& pa, hipStream_t s) {
        const size_t lds = persist_lds_bytes<T, D_, H_>();
        auto kern = pa.logp_out ? (sample_mode ? decode_persist_kernel<T, D_, H_, true, true> : decode_persist_kernel<T, D_, H_, false, true>)
                                : (sample_mode ? decode_persist_kernel<T, D_, H_, true, false> : decode_persist_kernel<T, D_, H_, false, false>);
        // per DEVICE, not per process (one process may drive several GPUs through several engines): set on every launch, it is cheap
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return fail(TXO_E_STATE, "persistent decode: the device refused the launch's dynamic LDS size");   // -> decode with launches
        }
        if (prof_persist && pool.used + 2 <= pool.ev.size()) {      // events bound to the dispatch itself (its begin / end timestamps)
            hipEvent_t e0 = pool.next(), e1 = pool.next();
            hipExtLaunchKernelGGL(kern, dim3(PS_TEAMS * PS_TEAM_BLOCKS), dim3(PS_THREADS), lds, s, e0, e1, 0, pa);
            ev_persist.push_back({e0, e1});
        } else {
            hipLaunchKernelGGL(kern, dim3(PS_TEAMS * PS_TEAM_BLOCKS), dim3(PS_THREADS), lds, s, pa);
        }
        return 0;
    }
    // returns 0 (done), TXO_E_STATE (the launch gave up: redo with launches), or an error
    // n_pos positions are decoded; rows of the request's outputs are its max_len positions apart
    // *broke: the reference's GLOBAL eos break fired inside these n_pos positions (possibly at the very last one)
    int generate_persist(const Decode& d, int n_pos, int* n_steps, bool* broke, hipStream_t s) {
        const int B = d.src.B, N = d.src.N, eos = d.q.eos, max_len = n_pos;
        PersistArgs<T> pa{};
        pa.B = B; pa.N = N; pa.V = V; pa.Ld = cfg.dec_layers; pa.Tmax = Tmax; pa.max_len = max_len; pa.eos = eos; pa.bos = cfg.bos;
        for (int l = 0; l < cfg.dec_layers; ++l) {
            PersistLayer<T>& L = pa.L[l];
            L.wqkv = dec_self[l].wqkv; L.wo_s = dec_self[l].wo; L.bo_s = dec_self[l].bo;
            L.wq_c = dec_cross[l].wq; L.wo_c = dec_cross[l].wo; L.bo_c = dec_cross[l].bo;
            L.w1 = dec_mlp[l].w1; L.b1 = dec_mlp[l].b1; L.w2 = dec_mlp[l].w2; L.b2 = dec_mlp[l].b2;
        }
        pa.wlog = wlog;
        {   // the projections' weights as their tiled copies (all of them, or none)
            bool all = knobs.w_tiled_on && wtiled.count(wlog);
            for (int l = 0; l < cfg.dec_layers && all; ++l)
                all = wtiled.count(dec_self[l].wqkv) && wtiled.count(dec_self[l].wo) && wtiled.count(dec_cross[l].wo) && wtiled.count(dec_mlp[l].w1) && wtiled.count(dec_mlp[l].w2);
            pa.w_tiled = all ? 1 : 0;
            if (all) {
                for (int l = 0; l < cfg.dec_layers; ++l) {
                    PersistLayer<T>& L = pa.L[l];
                    L.wqkv = wtiled.at(dec_self[l].wqkv); L.wo_s = wtiled.at(dec_self[l].wo); L.wo_c = wtiled.at(dec_cross[l].wo);
                    L.w1 = wtiled.at(dec_mlp[l].w1); L.w2 = wtiled.at(dec_mlp[l].w2);
                }
                pa.wlog = wtiled.at(wlog);
            }
        }
        pa.gamma = dec_g; pa.beta = dec_b; pa.gamma_f = decn_g; pa.beta_f = decn_b; pa.tok_emb = tok_emb; pa.pos_emb = pos_emb;
        pa.blog = blog;
        pa.dx = dx; pa.dy = dy; pa.dq = dq; pa.dlogits = dlogits; pa.dao = dao; pa.dhid = dhid;
        pa.cur_tok = cur_tok; pa.eos_seen = eos_seen; pa.skv = skv; pa.ckv = ckv;
        pa.self_stride = (size_t)ses.rows * Id * Tmax; pa.cross_stride = (size_t)ses.images * N * Id;
        pa.tokens_out = d.q.tokens; pa.out_stride = d.q.max_len; pa.logits_out = d.q.logits; pa.logp_out = d.q.logp;
        pa.sample = sample_mode; pa.sample_topk = sample_topk; pa.inv_temp = 1.0f / sample_temp; pa.seed = sample_seed;
        pa.ctl = pctl; pa.stamps = pstamps;
        const char* stamp_file = knobs.run.pstamps ? knobs.run.pstamps_file.c_str() : nullptr;
        pa.stamp_step = stamp_file ? std::min(max_len - 1, 200) : -1;
        if (knobs.run.has_stagger) pa.stagger_ticks = knobs.run.stagger_ticks;
        if (knobs.run.has_inject) pa.inject_fail = knobs.run.inject_fail; // tests: the give-up / fall-back path
        HIP_TRY(hipMemsetAsync(pctl, 0, sizeof(PersistCtl), s));
        if (stamp_file) HIP_TRY(hipMemsetAsync(pstamps, 0, sizeof(unsigned long long) * PS_TEAMS * PS_STAMP_RANKS * PS_MAX_STAGES * PS_STAMP_WORDS, s));
        if (D == 256) { if (int r = launch_persist<256, 8>(pa, s)) return r; }
        else if constexpr (sizeof(T) == 2) { if (int r = launch_persist<768, 12>(pa, s)) return r; }
        else return TXO_E_STATE;
        if (hipGetLastError() != hipSuccess) return fail(TXO_E_STATE, "persistent decode: the launch was refused");   // -> decode with launches
        HIP_TRY(hipMemcpyAsync(pctl_host, pctl, sizeof(PersistCtl), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const PersistCtl& c = *pctl_host;
        if (c.fail) { g_err = c.fail & 2u ? "persistent decode: a team spans more than one XCD" : "persistent decode: a hand-off timed out"; return TXO_E_STATE; }
        // GLOBAL eos break (decoder.py:115-116): the loop ends after the first position at which every row contains eos
        const int rpt = (B + PS_TEAMS - 1) / PS_TEAMS, nteams = (B + rpt - 1) / rpt;
        int steps = max_len;
        *broke = false;
        if (eos >= 0) {
            bool all = true; int last = 0;
            for (int k = 0; k < nteams; ++k) {
                const int nr = std::min(rpt, B - k * rpt);
                all = all && (int)c.eos_rows[k] >= nr;
                last = std::max(last, c.last_first_eos[k]);
            }
            if (all) steps = std::min(max_len, last + 1);
            *broke = all && last + 1 <= max_len;
        }
        // every team must have decoded every position that is returned (teams are not synchronised with each other; the kernel
        // lets a team stop only at or beyond the batch's last first-eos position -- checked here, never assumed)
        for (int k = 0; k < nteams; ++k)
            if (c.steps_run[k] < steps) { g_err = "persistent decode: a team stopped before the batch's last position"; return TXO_E_STATE; }
        if (stamp_file) Stamps::dump_persist(stamp_file, pstamps, nteams, cfg.dec_layers);
        *n_steps = steps;
        return 0;
    }
    // the decode itself and the state every call ends in.  q.logp [B][max_len] or null: log_softmax(logits)[token] of every returned position
    // (txo_generate_logp), 0 behind a row's eos under the per-row stop.  A prompted decode starts behind the shortest prefix and forces the
    // rest (step_prefix.h).
    int generate_common(const Decode& d, hipStream_t s) {
        const DecodeReq& q = d.q;
        int steps = 0; last_compactions = 0;
        last_ragged = d.src.ragged();
        const int rc = generate_impl(d, &steps, s);
        ses.row_stop = false;                                     // the decode is over (a txo_decode_step behind it steps every row)
        ses.forced = false;                                       // ... and picks every row's token itself: the prefix table belongs to the finished call
        ses.ruled = false;                                        // ... without rules: they bind the generate family only
        ses.closing = false;
        ses.guard_p = ses.guard_r = 0;                            // ... nor a repeat guard
        ses.alts = 0;                                             // ... and keeps no alternatives
        if (last_alts > 0 && rc == 0) { alts_B = d.src.B; alts_cols = std::min(steps, Tmax); }   // what txo_last_alternatives may read
        rules_rows = (rules_on && rc == 0) ? d.src.B : 0;         // what txo_last_rule_state may read
        if (last_ragged) ses.open = false;                        // nothing ragged outlives the call (stepping on one: txo_decode_begin_ragged)
        if (rc) return rc;
        if (q.n_steps) *q.n_steps = steps;
        if (last_compactions > 0) ses.open = false;               // the session's rows are no longer the batch's: a new decode must begin
        if (stop_mode == 1 && q.eos >= 0 && steps > 0 && !d.prompted()) {   // (a prompted decode has padded already: prefix_finish_kernel)
            hipLaunchKernelGGL(pad_after_eos_kernel, dim3((d.src.B + 255) / 256), dim3(256), 0, s, q.tokens, q.logp, q.max_len, steps, d.src.B, q.eos, cfg.bos, cfg.pad);
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(hipGetLastError());
        }
        return 0;
    }
    // live rows of range li to its front; the range then launches `new_rows` rows (>= its live rows).  t1 = positions decoded so far.
    int compact_lane(int li, int new_rows, int t1, int eos) {
        auto& ln = lanes[li];
        hipStream_t s = ln.stream;
        const size_t r0 = ln.b0;
        CompactArgs ca{ln.nb, new_rows, (int)r0, cur_tok + r0, eos_seen + r0, row_map + r0, cur_tok2 + r0, row_map2 + r0, cmoves + 2 * r0,
                       cinfo + 2 * li, st + li, eos, ses.ragged ? slens + r0 : nullptr, slens2 + r0};   // (a ragged session's key counts move with the rows)
        hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, s, ca);
        const int heads = cfg.dec_heads;
        auto move = [&](void* base, size_t outer_stride, size_t inner_stride, size_t row_stride, int outer_n, int inner_n, size_t len_elems) {
            MoveArgs ma{reinterpret_cast<unsigned char*>(base), outer_stride * sizeof(T), inner_stride * sizeof(T), row_stride * sizeof(T), inner_n,
                        (unsigned)(len_elems * sizeof(T) / 16), cmoves + 2 * r0, cinfo + 2 * li};
            if (ma.len16 == 0) return;
            hipLaunchKernelGGL(move_rows_kernel, dim3((ma.len16 + 255) / 256, outer_n * inner_n), dim3(256), 0, s, ma);
        };
        // self-attention history [Ld][2][rows*heads][Tmax][64]: positions 0 .. t1-1 of every head of every moved row
        move(skv + r0 * heads * Tmax * DH, (size_t)ses.rows * Id * Tmax, (size_t)Tmax * DH, (size_t)heads * Tmax * DH, 2 * cfg.dec_layers, heads, (size_t)t1 * DH);
        // the cross attention's operand: the session's encoder rows (latent form) or the projected K/V panels [Ld][2][rows*heads][N][64]
        if (ses.latent) move(enc_t + r0 * ses.keys * D, 0, 0, (size_t)ses.keys * D, 1, 1, (size_t)ses.keys * D);
        else move(ckv + r0 * ses.keys * Id, (size_t)ses.images * ses.keys * Id, 0, (size_t)ses.keys * Id, 2 * cfg.dec_layers, 1, (size_t)ses.keys * Id);
        ln.nb = new_rows;
        ++last_compactions;
        HIP_TRY(hipGetLastError());
        return 0;
    }
    int generate_impl(const Decode& d, int* steps, hipStream_t s) {
        const DecodeReq& q = d.q;
        const int B = d.src.B, max_len = q.max_len, eos = q.eos;
        // max_len > decoder.max_len: the reference slides its window (decoder.py:99-100).  The first Tmax positions decode with the
        // KV cache as always (n_pos of them; rows of the outputs are max_len apart); every further token re-runs its window of the
        // last Tmax tokens, positions re-indexed from 0, through ONE multi-position forward (prefill) -- generate_window below.
        // A prompted decode (check_prefix saw that it stays inside the table): the loop decodes positions t0 = m-1 .. M+max_len-2.
        const int t0 = d.prompted() ? d.m - 1 : 0;
        const int n_pos = d.prompted() ? d.M + max_len - 1 : std::min(max_len, Tmax);
        const float* rows = d.src.data;
        if (d.src.images) { if (int r = encode_batch(d.src.ib, rows, eenc, s)) return r; rows = eenc; }
        // (eos also decides whether the BOS column counts; a ragged session's key count per slot = the images' token counts)
        if (int r = begin_session(rows, B, d.src.N, eos, s, false, KeyCounts{d.src.ragged() ? rag_ntok : nullptr})) return r;
        ses.forced = d.prompted();
        ses.ruled = rules_on;
        ses.closing = closing();
        ses.guard_p = guard_p; ses.guard_r = guard_r;
        last_guarded = guard_p > 0;
        ses.alts = last_alts = alts_k;
        if (d.prompted()) {   // the prefix into the engine's table (lengths are in flen: generate), no forced token scored yet
            hipLaunchKernelGGL(prefix_table_kernel, dim3((B * Tmax + 255) / 256), dim3(256), 0, s, ftab, Tmax, q.prefix, q.P, flen, B, V);
            HIP_TRY(hipMemsetAsync(fplogp, 0, sizeof(float) * (size_t)B * Tmax, s));
        }
        last_persist = false;
        if (persist_cooldown > 0) --persist_cooldown;
        if (persist_usable(B)) {
            ensure_ckv(s);                                        // (the persistent launch reads projected K/V panels: the session stays in the K/V form)
            bool broke = false;
            const int pr = generate_persist(d, n_pos, steps, &broke, s);
            if (pr == 0) {
                last_persist = true; persist_strikes = 0;
                // (an eos break exactly at position n_pos - 1 also leaves steps == n_pos: the window must not start then)
                if (!broke && max_len > n_pos) return generate_window(d, n_pos, steps, s);
                return 0;
            }
            if (pr != TXO_E_STATE) return pr;
            ++persist_fallbacks;                                  // placement check or a bounded spin gave up: decode with launches
            if (++persist_strikes >= 2) {
                persist_cooldown = 64; persist_strikes = 0;
                fprintf(stderr, "[txo] persistent decode launch gave up twice in a row (%s): decoding with launches for the next 64 generates\n", g_err.c_str());
            }
            lanes.split(ses.rows, 1, s);
            reset_lanes(s, eos);
        }
        // the launch path, in three steps: how to run, the loop, the results to the caller
        LoopPlan plan;
        if (int r = plan_loop(d, s, &plan)) return r;
        DonePoll poll{lanes, done_flag, Tmax, n_pos};              // GLOBAL eos break: poll.done = it fired inside the positional table
        if (int r = run_loop(d, plan, t0, &poll, s)) return r;
        if (int r = deliver(d, plan, poll, steps, s)) return r;
        if (!d.prompted() && !poll.done && max_len > n_pos) return generate_window(d, n_pos, steps, s);
        return 0;
    }
    // How the launch path runs a decode: replaying captured steps or with eager launches, and where its steps write -- a captured step the
    // engine's own buffers (rows Tmax apart: graphs do not bake user pointers), an eager one the caller's
    struct LoopPlan { bool use_graph; int64_t* tdst; float* ldst; int tstride; };
    // Step 1: the session's form, graph or eager, the row ranges (reset, a prompted decode's history filled), the captured steps.
    int plan_loop(const Decode& d, hipStream_t s, LoopPlan* plan) {
        const DecodeReq& q = d.q;
        const int B = d.src.B, max_len = q.max_len, eos = q.eos;
        // lanes: graphs + extra streams unless per-step logits were asked for or a debug/profiling mode is on
        // Measured on MI355X (B=64, 224x672, T=256): the step is bound by the GPU-side latency chain of its ~26
        // dependent launches, not by the host -- graph replay and 2-4 lanes give the same wall time as eager
        // single-stream launches (57.1 vs 58.0 / 58.2 ms) -- so both stay opt-in: TXO_GRAPH=1, TXO_LANES=n.
        // graph replay by default only for very small batches (B <= 4: there the host's enqueue rate bounds the step --
        // 34.2 vs 37.2 ms per generate at B = 1 -- from B = 8 on it is equal); TXO_GRAPH=1 / 0 forces it on / off
        // per-row stop with live-row compaction: inside the positional table, tokens only (a finished row's logits would be unspecified)
        choose_form(stop_mode == 1 && eos >= 0 && q.logits == nullptr && max_len <= Tmax && knobs.stop_every > 0 && !prof && !prof_cross, s);
        if (d.prompted()) ses.lat_self = false;                    // (the multi-position pass fills the K/V history, not the z history)
        const bool want_graph = knobs.run.graph >= 0 ? knobs.run.graph != 0 : B <= 4;
        // per-row stop replays captured steps: as the ranges shrink a position's launches take less time than the host needs to enqueue them
        // (68 launches for two ranges: ~230 us per position on the host against 130 us on the device at 40 % of the rows), and a step
        // per row count (multiples of 16) is captured once and kept (lane_graph).  TXO_STOP_GRAPH=0: eager launches.
        const bool stop_graph = ses.row_stop && !sample_mode && knobs.stop_graph_on;
        const bool eager = q.logits != nullptr || g_dbg || sample_mode || !(want_graph || stop_graph);
        // two row ranges on two streams for a WIDE decoder at >= 256 rows (BASELINE cfg 4): one range's latency-bound projection launches
        // run beside the other's HBM-bound attention launches (816 -> 834 images/s; four ranges: 765).  Greedy and sampled alike: a draw is keyed
        // by (seed; row of the batch, position), not by the range (step.h: StepArgs::row0)
        // (also the narrow decoder's bf16 decode beyond the persistent launch's range, see persist_usable)
        int want = (sizeof(T) == 2 && !prof && !prof_cross &&       // (profiling times whole-batch launches)
                    ((D >= 512 && B >= 256) || (D < 512 && B > PERSIST_MAX_BF16_GREEDY))) ? 2 : 1;
        // in latent form the second range pays from ~224 rows on (160: 66.6 ms with one range vs 71.7 with two, 192: 70.6 vs 72.2, 256: 82.0 vs 77.9;
        // K/V form: two ranges from 129 on, 160: 70.9 vs 66.3)
        if (want == 2 && ses.latent && D < 512 && B < 224) want = 1;
        if (knobs.run.lanes > 0) want = std::min(knobs.run.lanes, MAXL);
        if (B < 32) want = 1;
        if (want == 2 && knobs.tune_lanes && !lanes.tuned) { if (int r = lanes.tune(n_cus, knobs.tune_verbose)) return r; }
        lanes.split(ses.rows, want, s);
        last_ranges = lanes.n;
        reset_lanes(s, eos, d.prompted() ? d.m : 0);
        if (ses.alts > 0) {   // pad / 0.0 in every column no step will write
            const size_t n = (size_t)B * Tmax * ses.alts;
            hipLaunchKernelGGL(alts_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, alt_ids, alt_logp, n, cfg.pad);
        }
        if (ses.ruled)   // every row's automaton at its start, run over the prefix columns the multi-position pass consumes
            hipLaunchKernelGGL(rules_start_kernel, dim3((B + 255) / 256), dim3(256), 0, s, rule_state, B, rules_dev, V, rules_S, rules_dmax, ftab, Tmax,
                               d.prompted() ? d.m : 0);
        if (ses.closing)   // ... and its end position and "has committed eos" (a captured step reads both from here: it bakes no position)
            hipLaunchKernelGGL(rules_close_start_kernel, dim3((B + 255) / 256), dim3(256), 0, s, rule_close, B, d.prompted() ? flen : nullptr, max_len, eos,
                               ftab, Tmax, d.prompted() ? d.m : 0);
        // a prompted decode: positions 0 .. m-2 of every row in ONE multi-position pass, no logits (it fills the K/V history the loop reads)
        if (d.prompted() && d.m > 1) { if (int r = prefill(ftab, Tmax, d.m - 1, nullptr, nullptr, s)) return r; }
        const bool use_graph = !eager && !prof && !prof_cross;     // event-carrying launches cannot be captured
        prefix_cols = use_graph ? Tmax : max_len;                  // (a captured step writes the engine's buffers: every column of theirs exists)
        // a captured step carries the log-probabilities like the tokens: into the engine's buffer
        if (use_graph) for (int i = 0; i < lanes.n; ++i) if (int r = lane_graph(i, eos, q.logp != nullptr)) return r;
        // (rows of q.tokens are max_len apart, of which only n_pos positions are decoded here)
        *plan = use_graph ? LoopPlan{true, tok_buf, q.logp ? logp_buf : nullptr, Tmax} : LoopPlan{false, q.tokens, q.logp, max_len};
        return 0;
    }
    // Step 2: positions t0 .. of the ranges, side by side, until the table ends or the global break fires (poll)
    int run_loop(const Decode& d, const LoopPlan& plan, int t0, DonePoll* poll_, hipStream_t s) {
        DonePoll& poll = *poll_;
        const bool use_graph = plan.use_graph, glogp = d.q.logp != nullptr;
        const int eos = d.q.eos, n_pos = poll.n_pos;
        if (int r = lanes.fork(s)) return r;
        int live_pend = -1;                                        // per-row stop: position behind which the ranges' finished-row counts were requested
        const char* stamp_file = knobs.run.stamps ? knobs.run.stamps_file.c_str() : nullptr;
        if (stamp_file && !stamps.buf) { if (int r = dalloc(&stamps.buf, (size_t)Stamps::KERNELS * Stamps::BLOCKS * 3)) return r; }
        const int stamp_step = stamp_file ? std::min(n_pos - 1, 200) : -1;
        auto decode_loop = [&]() -> int {
        for (int t = t0; t < n_pos; ++t) {
            if (t == stamp_step) { if (int r2 = stamps.begin(s)) return r2; }
            else if (stamps.slot >= 0) stamps.dump(stamp_file, knobs.has_stamps_raw ? &knobs.stamps_raw : nullptr, s);
            for (int i = 0; i < lanes.n; ++i) {
                if (use_graph) HIP_TRY(hipGraphLaunch(lanes[i].exec, lanes[i].stream));
                else if (int r2 = enqueue_step(lanes[i].stream, i, plan.tdst, plan.tstride, d.q.logits, plan.ldst, eos, nullptr, t)) return r2;
            }
            if (eos < 0) continue;
            if (ses.row_stop) {
                // Live-row compaction.  The host only needs an UPPER bound of a range's live rows to size its launches, and live rows only
                // decrease: the finished-row counter of a range is copied to pinned memory behind a step, AHEAD more steps are enqueued,
                // and only then the host reads it (never draining the stream, like the done flags).  compact_scan_kernel works on the
                // state of the moment it runs; slots between its live count and the host's bound are filler rows that count as finished.
                if (live_pend >= 0 && t == live_pend + DonePoll::AHEAD) {
                    for (int i = 0; i < lanes.n; ++i) HIP_TRY(hipEventSynchronize(lanes.ev_live[i]));
                    for (int i = 0; i < lanes.n; ++i) {
                        int bound = lanes[i].nb - lanes.live_host[i];
                        if (use_graph) bound = std::min(lanes[i].nb, (bound + 15) & ~15);      // a captured step per multiple of 16 rows
                        if (bound >= 1 && lanes[i].nb - bound >= knobs.stop_gain) {
                            if (int r2 = compact_lane(i, bound, t + 1, eos)) return r2;
                            if (use_graph) { if (int r2 = lane_graph(i, eos, glogp)) return r2; }
                        }
                    }
                    live_pend = -1;
                }
                if (live_pend < 0 && (t + 1) % knobs.stop_every == 0 && t + 1 + DonePoll::AHEAD < n_pos) {
                    for (int i = 0; i < lanes.n; ++i) {
                        HIP_TRY(hipMemcpyAsync(lanes.live_host + i, &st[i].rows_with_eos, sizeof(int), hipMemcpyDeviceToHost, lanes[i].stream));
                        HIP_TRY(hipEventRecord(lanes.ev_live[i], lanes[i].stream));
                    }
                    live_pend = t;
                }
            }
            if (int r2 = poll.after(t)) return r2;
            if (poll.done) break;
        }
        return 0;
        };
        if (int r = decode_loop()) return abandon_lanes(s, r);
        return lanes.join(s);
    }
    // Step 3: what the captured steps left in the engine's buffers to the caller's rows, a prompted decode's tail, the stream drained
    int deliver(const Decode& d, const LoopPlan& plan, const DonePoll& poll, int* steps, hipStream_t s) {
        const DecodeReq& q = d.q;
        const int B = d.src.B, max_len = q.max_len;
        // a prompted decode returns min(max_len, t_last + 2 - m) columns: the shortest prefix's row wrote column t_last + 1 - m last
        const int n_cols = d.prompted() ? std::min(max_len, poll.steps + 1 - d.m) : poll.n_pos;
        if (plan.use_graph) {
            HIP_TRY(hipMemcpy2DAsync(q.tokens, sizeof(int64_t) * max_len, tok_buf, sizeof(int64_t) * Tmax,
                                     sizeof(int64_t) * n_cols, B, hipMemcpyDeviceToDevice, s));
            if (q.logp)
                HIP_TRY(hipMemcpy2DAsync(q.logp, sizeof(float) * max_len, logp_buf, sizeof(float) * Tmax, sizeof(float) * n_cols, B, hipMemcpyDeviceToDevice, s));
        }
        if (d.prompted())   // pad / 0.0 where a row did not get to (or is finished, per-row stop); the forced tokens' log-probabilities to the caller
            hipLaunchKernelGGL(prefix_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, s, q.tokens, q.logp, max_len, n_cols, B, poll.steps, q.eos,
                               cfg.pad, stop_mode == 1 ? 1 : 0, ftab, Tmax, flen, d.m, fplogp, q.prefix_logp, q.P);
        // the alternatives follow the tokens: pad / 0.0 where a row did not get to or is finished (step_alts.h)
        if (ses.alts > 0 && (d.prompted() || (stop_mode == 1 && q.eos >= 0)))
            hipLaunchKernelGGL(alts_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, s, alt_ids, alt_logp, ses.alts, Tmax, q.tokens, max_len, n_cols, B,
                               poll.steps, q.eos, cfg.bos, cfg.pad, stop_mode == 1 ? 1 : 0, ftab, Tmax, d.prompted() ? flen : nullptr);
        // the rules' states behind the last RETURNED position of every row (the loop may have run ahead of the eos break; a prompted row stops
        // counting at its last returned column).  Under the per-row stop a finished row froze its state itself.
        if (ses.ruled && !ses.row_stop && poll.steps >= 1)
            hipLaunchKernelGGL(rules_settle_kernel, dim3((B + 255) / 256), dim3(256), 0, s, rule_state, rule_hist, Tmax, B, std::min(poll.steps, Tmax) - 1,
                               d.prompted() ? flen : nullptr, n_cols);
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipGetLastError());
        lanes.split(ses.rows, 1, s);
        *steps = d.prompted() ? n_cols : poll.steps;
        return 0;
    }

    // The reference beyond its positional table (decoder.py:97-116 with :99-100 active): token i >= Tmax comes from the window
    // output[:, -Tmax:] = tokens i-Tmax .. i-1 at positions 0 .. Tmax-1 (BOS has left the window), the whole window through the
    // decoder, the last position's logits.  Nothing cached survives the shift, so every such token costs one multi-position
    // forward of Tmax rows per image (prefill) + the single-position final LayerNorm / logits / token selection of the step path.
    // The GLOBAL eos test still looks at the whole output (:115), i.e. the per-row "seen" state carries over.
    int generate_window(const Decode& d, int n_pos, int* steps, hipStream_t s) {
        const int B = d.src.B, max_len = d.q.max_len, eos = d.q.eos;
        int64_t* tokens_out = d.q.tokens;
        lanes.split(ses.rows, 1, s);
        lanes[0].stream = s;
        // the launch path's eos bookkeeping, rebuilt from the tokens decoded so far (a persistent launch keeps its own)
        HIP_TRY(hipMemsetAsync(st, 0, sizeof(StepState), s));
        hipLaunchKernelGGL(rebuild_eos_state_kernel, dim3((B + 255) / 256), dim3(256), 0, s, tokens_out, max_len, n_pos, B, eos, cfg.bos,
                           eos_seen, &st[0].rows_with_eos);
        int* flag = done_flag;                                    // ONE flag, rewritten per token (commit_token indexes it with the token index)
        for (int i = n_pos; i < max_len; ++i) {
            if (int r = prefill(tokens_out + (i - Tmax), max_len, Tmax, nullptr, dlogits, s)) return r;
            hipLaunchKernelGGL(set_position_kernel, dim3(1), dim3(1), 0, s, st, i);
            StepArgs sa{dlogits, V, B, cur_tok, tokens_out, max_len, d.q.logits, st, eos_seen, flag - i, eos, sample_topk, 1.0f / sample_temp, sample_seed, 0,
                        0, nullptr, d.q.logp};
            sa.guard_p = ses.guard_p; sa.guard_r = ses.guard_r;
            if (ses.ruled) { sa.rules = rules_dev; sa.n_states = rules_S; sa.depth_max = rules_dmax; sa.rule_state = rule_state; }
            if (ses.guarded()) launch_guard_step(s, B, sa, sample_mode != 0);   // (the history is the caller's rows: every token so far stands there)
            else
            if (ses.ruled) {   // the loop's states carry over (no history beyond the table: the host looks at every token here, nothing runs ahead)
                if (ses.closing) { sa.close_tab = close_dev; sa.rule_close = rule_close; launch_rules_close_step(s, B, sa, sample_mode != 0); }
                else launch_rules_step(s, B, sa, sample_mode != 0);
            } else
            if (sample_mode) launch_sample_step(s, B, sa);
            else hipLaunchKernelGGL(argmax_step_kernel, dim3(B), dim3(64), 0, s, sa);
            *steps = i + 1;
            if (eos >= 0) {                                       // slow path: one host look per token
                HIP_TRY(hipMemcpyAsync(lanes.flags_host, flag, sizeof(int), hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                if (lanes.flags_host[0]) break;
            }
        }
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // ---- beam search: txo_generate_beam, txo_beam_search, txo_beam_search_ragged -- one loop (beam_impl), two tails ----
    // what all three refuse before anything is encoded or decoded
    int beam_refusals(int B, int beams, int max_len) {
        if (beams < 1 || beams > 8) return fail(TXO_E_INVALID, "beams must be in [1, 8]");
        if (max_len < 1 || max_len > Tmax)
            return fail(TXO_E_INVALID, "max_len exceeds the decoder's max_length (a KV cache cannot slide the window)");
        if (Tmax > 1024) return fail(TXO_E_INVALID, "beam search supports max_length <= 1024");
        if (B < 1 || B * beams > Bmax || B * beams > 32767) return fail(TXO_E_INVALID, "images * beams exceeds engine max_batch");
        return 0;
    }
    int beam_search(const DecodeSrc& q, int beams, int max_len, int eos, const BeamSink& sink, int* n_steps, hipStream_t s) override {
        const bool three = sink.best != nullptr;                  // txo_generate_beam: it leaves last_compactions / last_ragged as they were, as it
        if (!three) { last_compactions = 0; last_ragged = false; }   // always did; the other two report THIS call, also when it is refused, as generate()
        if (int r = beam_refusals(q.B, beams, max_len)) return r;
        if (!three) {
            if (!sink.out || !sink.out->tokens) return fail(TXO_E_INVALID, "beam search: null out / out->tokens");
            // by its bits: the library is built with -fno-honor-nans, which lets a float comparison assume its operand is no NaN
            uint32_t ab; memcpy(&ab, &sink.out->length_alpha, sizeof ab);
            const bool nonfinite = (ab & 0x7f800000u) == 0x7f800000u, negative = (ab >> 31) != 0 && (ab << 1) != 0;
            if (nonfinite || negative) return fail(TXO_E_INVALID, "beam search: length_alpha must be finite and >= 0");
        }
        Source src;
        if (int r = resolve_source(q, s, &src)) return r;
        if (!three) last_ragged = src.ragged();
        if (rules_on && !rules_beam)   // (last: every other refusal of the three entries keeps its place; txo_set_rules_beam lifts it)
            return fail(TXO_E_INVALID, "beam search: not available while token rules are set (txo_set_token_rules with rules_host == NULL switches them off)");
        if (int r = close_refusals("beam search", eos, max_len, true)) return r;   // (behind every other refusal, like the one above)
        if (guard_p > 0 && !guard_beam)   // (txo_set_guard_beam lifts it)
            return fail(TXO_E_INVALID, "beam search: not available while a repeat guard is set (txo_set_repeat_guard(e, 0, 0) switches it off)");
        if (guard_p > 0 && beam_guard_lds_bytes(beams, V, guard_p, guard_r) > BEAM_GUARD_LDS_MAX)
            return fail(TXO_E_INVALID, "beam search: the vocabulary does not fit the guarded selection's LDS (beams * (vocab / 8 bytes + ((max_repeats + 1) * max_period - 1) * 4 bytes) "
                                       "per workgroup, 56 KB; the vocabulary has " + std::to_string(V) + " entries)");
        if (guard_beam) last_guarded = guard_p > 0;               // (off: a beam entry leaves TXO_Q_LAST_GUARDED as it was, as it always did)
        if (alts_k > 0)
            return fail(TXO_E_INVALID, "beam search: alternatives are not available (txo_set_alternatives(e, 0) switches them off)");
        brule_B = brule_k = 0;
        const int rc = beam_impl(src, beams, max_len, eos, sink, n_steps, s);
        if (rules_on && rc == 0) { brule_B = src.B; brule_k = beams; }   // what txo_last_beam_rule_state may read
        if (src.ragged()) ses.open = false;                       // nothing ragged outlives the call (generate_common)
        return rc;
    }
    int beam_impl(const Source& from, int beams, int max_len, int eos, const BeamSink& sink, int* n_steps, hipStream_t s) {
        const int B = from.B, N = from.N, rows = B * beams;
        const ImageBatch* ib = from.batch();
        const float* src = from.data;
        if (ib) { if (int r = encode_batch(*ib, src, eenc, s)) return r; src = eenc; }
        // decode rows are (image, beam) slots for the length of this call: whatever way it ends, the session it leaves has one row per image
        struct Rows { Session& ses; ~Rows() { ses.rows = ses.images; } } restore{ses};
        // (a ragged session's key counts are per IMAGE: the k beams of an image share its cross K/V panel and its count, launch_dec_attn)
        if (int r = begin_session(src, B, N, eos, s, false, KeyCounts{ib && ib->ragged ? rag_ntok : nullptr}, beams)) return r;
        choose_form(false, s);
        last_persist = false;
        // Two row ranges on two streams from 256 rows on, as generate() does beyond 128 images: one range's latency-bound projection
        // launches run beside the other's HBM-bound attention launches.  A range is a whole number of IMAGES (beam_select_kernel ranks
        // an image's k beams together; self-attention slots are range-local); every range has its own step state and done flags.
        int want = (rows >= 256 && B >= 2 && !prof && !prof_cross && !g_dbg) ? 2 : 1;
        if (knobs.run.lanes > 0) want = std::max(1, std::min(std::min(knobs.run.lanes, MAXL), B));
        if (want == 2 && knobs.tune_lanes && !lanes.tuned) { if (int r = lanes.tune(n_cus, knobs.tune_verbose)) return r; }
        if (want > 1) lanes.split(rows, want, s, beams);
        last_ranges = lanes.n;
        const int n = std::max(rows, Tmax);
        hipLaunchKernelGGL(beam_reset_kernel, dim3((n + 255) / 256), dim3(256), 0, s, st, cur_tok, bscore, bfin, done_flag, rows,
                           beams, Tmax, cfg.bos);
        const bool ruled = rules_on;                                  // (beam_search has refused unless txo_set_rules_beam is on) every slot starts at (0, 0)
        if (ruled) HIP_TRY(hipMemsetAsync(brule_state, 0, sizeof(int2) * (size_t)rows, s));
        for (int i = 1; i < lanes.n; ++i)                             // the other ranges' step state and flags (no rows: they were reset above)
            hipLaunchKernelGGL(beam_reset_kernel, dim3((Tmax + 255) / 256), dim3(256), 0, s, st + i, cur_tok, bscore, bfin,
                               done_flag + (size_t)i * Tmax, 0, beams, Tmax, cfg.bos);
        if (int r = lanes.fork(s)) return r;
        // same non-draining eos look as generate(): once every beam is finished further steps only repeat eos at no cost
        // (beam_select_kernel), so the few steps enqueued ahead of the look change neither scores nor slots.  Nor do they change a
        // constrained search's states -- a finished beam's state is frozen (beam_rules.h) --, so those need no history behind every
        // position the way a constrained generate's do (rule_hist).
        DonePoll poll{lanes, done_flag, Tmax, max_len};
        const bool want_logp = sink.out && sink.out->logp;
        int cur = 0;
        auto beam_loop = [&]() -> int {
        for (int t = 0; t < max_len; ++t) {
            BeamCtx bm{beams, bpath[cur], bpath[cur ^ 1], want_logp, ruled, ruled && rules_close, max_len, guard_p, guard_r};   // (a guard set here has passed beam_search: txo_set_guard_beam is on)
            for (int i = 0; i < lanes.n; ++i)
                if (int r2 = enqueue_step(lanes[i].stream, i, nullptr, 0, nullptr, nullptr, eos, &bm, t)) return r2;
            cur ^= 1;
            if (eos < 0) continue;
            if (int r2 = poll.after(t)) return r2;
            if (poll.done) break;
        }
        return 0;
        };
        if (int r = beam_loop()) return abandon_lanes(s, r);
        if (int r = lanes.join(s)) return r;
        const int steps = poll.steps;
        lanes.split(rows, 1, s);
        if (sink.out) {
            // one workgroup per image: lengths, the final order, tokens and increments straight into the caller's rows (step.h)
            const txo_beam_out& o = *sink.out;
            BeamFinishArgs fa{bparent, btok, want_logp ? blogp : nullptr, Bmax, bscore, steps, beams, eos, o.length_alpha,
                              o.tokens, o.logp, o.scores, o.lengths, max_len};
            launch_beam_finish(s, B, fa, ruled ? brule_state : nullptr);   // ... and, under rules, the states into that order
        } else {
            // backtrack every beam into tok_buf rows, then hand out the best beam (slot 0: selection order is by score)
            hipLaunchKernelGGL(beam_backtrack_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, bparent, btok, Bmax, steps, rows,
                               tok_buf, Tmax);
            HIP_TRY(hipMemcpy2DAsync(sink.best, sizeof(int64_t) * max_len, tok_buf, sizeof(int64_t) * Tmax * beams,
                                     sizeof(int64_t) * steps, B, hipMemcpyDeviceToDevice, s));
            if (sink.all)
                HIP_TRY(hipMemcpy2DAsync(sink.all, sizeof(int64_t) * max_len, tok_buf, sizeof(int64_t) * Tmax,
                                         sizeof(int64_t) * steps, rows, hipMemcpyDeviceToDevice, s));
            if (sink.scores) HIP_TRY(hipMemcpyAsync(sink.scores, bscore, sizeof(float) * rows, hipMemcpyDeviceToDevice, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipGetLastError());
        if (n_steps) *n_steps = steps;
        return 0;
    }

    // txo_set_token_rules behind its checks: the table to the device (nothing of the engine is in flight between two calls: every generate drains
    // its stream).  table null: off.
    int set_token_rules(const int32_t* table, int S, int depth_max) override {
        if (table && rules_close) { if (int r = close_install(table, S, depth_max)) return r; }   // (a refused table leaves the installed one in place)
        rules_rows = 0; brule_B = brule_k = 0;
        if (!table) { rules_on = false; rules_S = 0; rules_dmax = 0; rules_host.clear(); close_dist.clear(); close_dist_max = 0; return 0; }
        HIP_TRY(hipMemcpy(rules_dev, table, sizeof(int32_t) * (size_t)S * V, hipMemcpyHostToDevice));
        rules_host.assign(table, table + (size_t)S * V);
        rules_on = true; rules_S = S; rules_dmax = depth_max;
        return 0;
    }
    // txo_set_rules_close behind its check.  The table is (re)computed whenever rules and switch are both set, in either order
    int set_rules_close(bool on) override {
        if (on && rules_on) { if (int r = close_install(rules_host.data(), rules_S, rules_dmax)) return r; }   // (refused: the switch stays as it was)
        if (!on) { close_dist.clear(); close_dist_max = 0; }
        rules_close = on;
        return 0;
    }
    // the distance table of a rule set (rules_close.h) to the host copy and, packed to 16 bits, to the device beside rules_dev.  Refused, with
    // nothing changed: the engine has no eos, or eos cannot be reached from the start state
    int close_install(const int32_t* table, int S, int depth_max) {
        std::vector<int32_t> dist; bool any_inf = false;
        const int dmax = rules_close_dist(table, S, V, depth_max, cfg.eos, dist, &any_inf);
        if (cfg.eos < 0 || cfg.eos >= V || dist[0] == CLOSE_INF)
            return fail(TXO_E_INVALID, "closing decode: eos is unreachable from the start state (the engine's eos id is " + std::to_string(cfg.eos) +
                                       "; the rules must allow a path from state 0, depth 0 to it)");
        std::vector<CloseTable> tab(1);
        for (int i = 0; i < CLOSE_NODES; ++i)
            tab[0].dist[i] = (unsigned short)((size_t)i < dist.size() && dist[(size_t)i] != CLOSE_INF ? dist[(size_t)i] : CLOSE_FAR);
        tab[0].slack = any_inf ? 0x7fffffff : dmax; tab[0].dist_max = dmax; tab[0].pad[0] = tab[0].pad[1] = 0;
        HIP_TRY(hipMemcpy(close_dev, tab.data(), sizeof(CloseTable), hipMemcpyHostToDevice));
        close_dist.swap(dist); close_dist_max = dmax;
        return 0;
    }
    // what a closing call refuses, behind every other refusal of its entry: an eos other than the engine's (the table was computed for that
    // one), and from BOS a call too short to reach eos at all
    int close_refusals(const char* what, int eos, int picks, bool from_bos) {
        if (!closing()) return 0;
        if (eos != cfg.eos)
            return fail(TXO_E_INVALID, std::string(what) + ": a closing decode (txo_set_rules_close) needs eos = " + std::to_string(cfg.eos) + ", the engine's eos id; got " +
                                       std::to_string(eos));
        if (from_bos && close_dist[0] > picks)
            return fail(TXO_E_INVALID, std::string(what) + ": a closing decode needs " + std::to_string(close_dist[0]) + " picks to reach eos from the start state, but the call has " +
                                       std::to_string(picks));
        return 0;
    }
    int last_alternatives(int32_t* ids_out, float* logp_out, int B, int cols, hipStream_t s) override {
        if (last_alts < 1 || alts_B < 1)
            return fail(TXO_E_INVALID, "txo_last_alternatives: the last txo_generate* ran without alternatives (txo_set_alternatives)");
        if (B < 1 || B > alts_B || cols < 1 || cols > alts_cols)
            return fail(TXO_E_INVALID, "txo_last_alternatives: B must be in [1, " + std::to_string(alts_B) + "] and cols in [1, " + std::to_string(alts_cols) +
                                       "], the rows and columns of the last alternatives decode");
        const size_t k = (size_t)last_alts;
        if (ids_out)
            HIP_TRY(hipMemcpy2DAsync(ids_out, sizeof(int32_t) * cols * k, alt_ids, sizeof(int32_t) * Tmax * k, sizeof(int32_t) * cols * k, B, hipMemcpyDeviceToDevice, s));
        if (logp_out)
            HIP_TRY(hipMemcpy2DAsync(logp_out, sizeof(float) * cols * k, alt_logp, sizeof(float) * Tmax * k, sizeof(float) * cols * k, B, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    int last_rule_state(int32_t* out, int B, hipStream_t s) override {
        if (!rules_on) return fail(TXO_E_STATE, "txo_last_rule_state: no token rules are set");
        if (rules_rows < 1) return fail(TXO_E_STATE, "txo_last_rule_state: no generate has run since the token rules were set");
        if (B < 1 || B > rules_rows)
            return fail(TXO_E_INVALID, "txo_last_rule_state: B must be in [1, " + std::to_string(rules_rows) + "], the rows of the last constrained generate");
        hipLaunchKernelGGL(rules_state_out_kernel, dim3((B + 255) / 256), dim3(256), 0, s, out, rule_state, B);
        HIP_TRY(hipGetLastError());
        return 0;
    }

    // txo_last_beam_rule_state: the slots' states in the order of the last beam call's outputs (beam_finish_rules_kernel; txo_generate_beam: slot order)
    int last_beam_rule_state(int32_t* out, int B, int beams, hipStream_t s) override {
        if (!rules_on) return fail(TXO_E_STATE, "txo_last_beam_rule_state: no token rules are set");
        if (brule_B < 1) return fail(TXO_E_STATE, "txo_last_beam_rule_state: no constrained beam search has run since the token rules were set");
        if (B != brule_B || beams != brule_k)
            return fail(TXO_E_STATE, "txo_last_beam_rule_state: B and beams must be " + std::to_string(brule_B) + " and " + std::to_string(brule_k) +
                                     ", the images and beams of the last constrained beam search");
        const int rows = B * beams;
        hipLaunchKernelGGL(rules_state_out_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, out, brule_state, rows);
        HIP_TRY(hipGetLastError());
        return 0;
    }

    int query(int what, int64_t* out) override {
        if (what == TXO_Q_LAST_PERSISTENT) *out = last_persist ? 1 : 0;
        else if (what == TXO_Q_PERSIST_FALLBACKS) *out = persist_fallbacks;
        else if (what == TXO_Q_LAST_ROW_RANGES) *out = last_persist ? 1 : last_ranges;
        else if (what == TXO_Q_LAST_LATENT) *out = (!last_persist && ses.latent) ? 1 : 0;
        else if (what == TXO_Q_RELOAD_KNOBS) { knobs.run.read(); *out = 0; }
        else if (what == TXO_Q_LAST_COMPACTIONS) *out = last_compactions;
        else if (what == TXO_Q_LAST_RAGGED) *out = last_ragged ? 1 : 0;
        else if (what == TXO_Q_LAST_LATENT_SELF) *out = (!last_persist && ses.latent && ses.lat_self) ? 1 : 0;
        else if (what == TXO_Q_LAST_GUARDED) *out = last_guarded ? 1 : 0;
        else if (what == TXO_Q_LAST_ALTS) *out = last_alts;
        else if (what == TXO_Q_SAMPLE_VOCAB_MAX) *out = std::max<int64_t>(64 * SR_PER, (int64_t)(sample_lds_max / sizeof(float)));
        else return fail(TXO_E_INVALID, "unknown query");
        return 0;
    }
    int profile_enable(int on) override {
        prof = on == 1; prof_cross = on == 2; prof_persist = on == 3;
        ev_cross.clear(); ev_enc.clear(); ev_step.clear(); ev_persist.clear(); ev_ingest.clear(); pool.used = 0;
        if (prof_persist) while (pool.ev.size() < 64) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); pool.ev.push_back(e); }
        if (prof_cross) {           // events for 16 generate() calls, created now
            const size_t want = (size_t)16 * 2 * cfg.dec_layers * Tmax / 4;
            while (pool.ev.size() < want) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); pool.ev.push_back(e); }
        }
        return 0;
    }
    int profile_read(int kind, double* avg_ms, int64_t* count) override {
        auto& v = kind == 0 ? ev_cross : (kind == 1 ? ev_enc : (kind == 2 ? ev_step : (kind == 4 ? ev_ingest : ev_persist)));
        double tot = 0; int64_t n = 0;
        for (auto& p : v) {
            float ms = 0;
            if (hipEventSynchronize(p.second) != hipSuccess) continue;
            if (hipEventElapsedTime(&ms, p.first, p.second) != hipSuccess) continue;
            tot += ms; ++n;
        }
        if (avg_ms) *avg_ms = n ? tot / n : 0.0;
        if (count) *count = n;
        return 0;
    }
};

static int validate(const txo_config& c) {
    if (c.canvas_h <= 0 || c.canvas_h % 16 || c.canvas_w <= 0 || c.canvas_w % 16)
        return fail(TXO_E_INVALID, "canvas height/width must be positive multiples of 16");
    if (c.embed != TXO_EMBED_PATCH && c.embed != TXO_EMBED_HYBRID) return fail(TXO_E_INVALID, "embed must be TXO_EMBED_PATCH or TXO_EMBED_HYBRID");
    if (c.embed == TXO_EMBED_HYBRID && c.in_channels != 1)
        return fail(TXO_E_INVALID, "the hybrid ResNetV2 embedder takes single-channel images");
    if (c.embed_dim < 64 || c.embed_dim % 64 || c.embed_dim > 768)
        return fail(TXO_E_INVALID, "embed_dim must be a multiple of 64 in [64, 768]");
    if (c.enc_heads < 1 || c.dec_heads < 1 || c.enc_layers < 1 || c.dec_layers < 1)
        return fail(TXO_E_INVALID, "heads and layers must be >= 1");
    if (c.enc_exp < 1 || c.dec_exp < 1 || (c.enc_exp * c.embed_dim) % 64 || (c.dec_exp * c.embed_dim) % 64)
        return fail(TXO_E_INVALID, "FFN width must be a multiple of 64");
    if (c.in_channels < 1 || c.vocab < 2 || c.max_len < 1) return fail(TXO_E_INVALID, "bad in_channels / vocab / max_len");
    if (c.bos < 0 || c.bos >= c.vocab) return fail(TXO_E_INVALID, "bos token outside the vocabulary");
    if (c.max_batch < 1 || c.max_batch > 65535) return fail(TXO_E_INVALID, "max_batch must be in [1, 65535]");
    if (c.max_tokens < 0 || c.max_tokens > 1 + (c.canvas_h / 16) * (c.canvas_w / 16))
        return fail(TXO_E_INVALID, "max_tokens exceeds 1 + canvas_h*canvas_w/256");
    if (c.dtype != TXO_F32 && c.dtype != TXO_BF16) return fail(TXO_E_INVALID, "dtype must be TXO_F32 or TXO_BF16");
    return 0;
}

}  // namespace txo

using namespace txo;

struct txo_engine { std::unique_ptr<EngineBase> impl; };

extern "C" {

int txo_engine_create(const txo_config* cfg, txo_engine** out) {
    if (!cfg || !out) return fail(TXO_E_INVALID, "null argument");
    if (int r = validate(*cfg)) return r;
    std::unique_ptr<EngineBase> impl;
    int r;
    if (cfg->dtype == TXO_F32) { auto* e = new Engine<float>(); e->cfg = *cfg; impl.reset(e); r = e->init(); }
    else { auto* e = new Engine<bf16>(); e->cfg = *cfg; impl.reset(e); r = e->init(); }
    if (r) return r;
    *out = new txo_engine{std::move(impl)};
    return 0;
}

void txo_engine_destroy(txo_engine* e) { delete e; }

int txo_engine_set_weight(txo_engine* e, const char* key, const float* data, const int64_t* shape, int32_t ndim) {
    if (!e || !key || !data || !shape || ndim < 1 || ndim > 4) return fail(TXO_E_INVALID, "bad argument");
    if (e->impl->ready) return fail(TXO_E_STATE, "weights already finalized");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { if (shape[i] < 1) return fail(TXO_E_INVALID, "bad shape"); t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(data, data + n);
    e->impl->host[key] = std::move(t);
    return 0;
}

int txo_engine_finalize_weights(txo_engine* e) {
    if (!e) return fail(TXO_E_INVALID, "null engine");
    int r = e->impl->finalize();
    if (r == TXO_E_STATE && g_err.empty()) g_err = "missing weights";
    return r;
}

int txo_encode(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t H, int32_t W, float* enc_out, void* stream) {
    if (!e || !img || !enc_out) return fail(TXO_E_INVALID, "null argument");
    return e->impl->encode(img, B, C, H, W, enc_out, (hipStream_t)stream);
}

int txo_decode_begin(txo_engine* e, const float* enc, int32_t B, int32_t N, void* stream) {
    if (!e || !enc) return fail(TXO_E_INVALID, "null argument");
    return e->impl->decode_begin(enc, B, N, e->impl->cfg.eos, (hipStream_t)stream);
}

int txo_encode_ragged(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t Hc, int32_t Wc, const int32_t* sizes, float* enc_out,
                      int32_t* n_slot, void* stream) {
    if (!e || !img || !sizes || !enc_out) return fail(TXO_E_INVALID, "null argument");
    return e->impl->encode_ragged(img, B, C, Hc, Wc, sizes, enc_out, n_slot, (hipStream_t)stream);
}

int txo_decode_begin_ragged(txo_engine* e, const float* enc, int32_t B, int32_t Ns, const int32_t* n_tokens, void* stream) {
    if (!e || !enc || !n_tokens) return fail(TXO_E_INVALID, "null argument");
    return e->impl->decode_begin_ragged(enc, B, Ns, n_tokens, e->impl->cfg.eos, (hipStream_t)stream);
}

int txo_generate_ragged(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t Hc, int32_t Wc, const int32_t* sizes, int32_t max_len,
                        int32_t eos, int64_t* tokens_out, int32_t* n_steps, void* stream) {
    if (!e || !img || !sizes || !tokens_out) return fail(TXO_E_INVALID, "null argument");
    return e->impl->generate(DecodeReq{.src = {.img = img, .sizes = sizes, .B = B, .C = C, .H = Hc, .W = Wc}, .max_len = max_len, .eos = eos,
                                       .tokens = tokens_out, .n_steps = n_steps}, (hipStream_t)stream);
}

int txo_generate_ragged_logp(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t Hc, int32_t Wc, const int32_t* sizes, int32_t max_len,
                             int32_t eos, int64_t* tokens_out, int32_t* n_steps, float* logp_out, void* stream) {
    if (!e || !img || !sizes || !tokens_out || !logp_out) return fail(TXO_E_INVALID, "null argument");
    return e->impl->generate(DecodeReq{.src = {.img = img, .sizes = sizes, .B = B, .C = C, .H = Hc, .W = Wc}, .max_len = max_len, .eos = eos,
                                       .tokens = tokens_out, .n_steps = n_steps, .logp = logp_out}, (hipStream_t)stream);
}

int txo_ingest_box(const int32_t* shapes, int32_t B, int32_t* Hc_out, int32_t* Wc_out) {
    if (!Hc_out || !Wc_out) return fail(TXO_E_INVALID, "ingest: null argument");
    long long box[2];
    if (int r = ingest_check_shapes(shapes, B, box)) return r;
    *Hc_out = (int32_t)box[0]; *Wc_out = (int32_t)box[1];
    return 0;
}

// txo_ingest_u8 / _fit / _view: every refusal that needs neither an engine nor a device (ingest_plan), the engine's one entry, the sizes
static int ingest_run(const IngestReq& q, void* stream) {
    IngestPlan p;
    if (int r = ingest_plan(q, &p)) return r;
    if (int r = q.engine->impl->ingest(p, q, (hipStream_t)stream)) return r;
    for (int b = 0; b < q.src.B; ++b) { q.sizes_out[2 * b] = (int32_t)ingest_round16(p.out_h(b)); q.sizes_out[2 * b + 1] = (int32_t)ingest_round16(p.out_w(b)); }
    return 0;
}

int txo_ingest_u8(txo_engine* e, const uint8_t* pix, const int64_t* offsets, const int32_t* shapes, int32_t B, int32_t C, int32_t Hc, int32_t Wc,
                  float* box_out, int32_t* sizes_out, void* stream) {
    return ingest_run(IngestReq{.engine = e, .src = {.pix = pix, .offsets = offsets, .shapes = shapes, .B = B}, .C = C, .Hc = Hc, .Wc = Wc,
                                .box = box_out, .sizes_out = sizes_out}, stream);
}

int txo_ingest_fit(const int32_t* shapes, int32_t B, int32_t Fh, int32_t Fw, int32_t* fitted_out) {
    if (!fitted_out) return fail(TXO_E_INVALID, "ingest: null argument");
    if (int r = ingest_check_shapes(shapes, B, nullptr)) return r;
    std::vector<int32_t> fitted((size_t)2 * B);                       // (nothing is written on a refusal)
    if (int r = ingest_fit_sizes(shapes, B, {Fh, Fw}, fitted.data(), nullptr)) return r;
    memcpy(fitted_out, fitted.data(), sizeof(int32_t) * 2 * (size_t)B);
    return 0;
}

int txo_ingest_fit_scratch(const int32_t* shapes, int32_t B, int32_t Fh, int32_t Fw, int64_t* bytes_out) {
    if (!bytes_out) return fail(TXO_E_INVALID, "ingest: null argument");
    long long need = 0;
    if (int r = ingest_check_shapes(shapes, B, nullptr)) return r;
    if (int r = ingest_fit_sizes(shapes, B, {Fh, Fw}, nullptr, &need)) return r;
    *bytes_out = need;
    return 0;
}

int txo_ingest_fit_coeffs(int32_t in, int32_t out, int32_t* xmin_out, int32_t* n_out, int32_t* K_out) {
    if (!xmin_out || !n_out || !K_out) return fail(TXO_E_INVALID, "ingest: null argument");
    if (in < 1 || out < 1) return fail(TXO_E_INVALID, "ingest: fit coefficients need in >= 1 and out >= 1");
    if ((long long)in > (long long)FIT_MAX_SCALE * out)
        return fail(TXO_E_INVALID, "ingest: fit coefficients for " + std::to_string(in) + " -> " + std::to_string(out) + ": the axis shrinks by more than " +
                                       std::to_string(FIT_MAX_SCALE) + " times");
    for (int xx = 0; xx < out; ++xx) {
        int* K = K_out + (size_t)xx * TXO_FIT_TAPS;
        std::fill(K, K + TXO_FIT_TAPS, 0);
        int xmin, n;
        fit_axis_coeffs(in, out, xx, &xmin, &n, K, 1, 0, 1);
        xmin_out[xx] = xmin; n_out[xx] = n;
    }
    return 0;
}

int txo_ingest_u8_fit(txo_engine* e, const uint8_t* pix, const int64_t* offsets, const int32_t* shapes, int32_t B, int32_t C, int32_t Fh, int32_t Fw,
                      int32_t Hc, int32_t Wc, float* box_out, int32_t* sizes_out, void* scratch, int64_t scratch_bytes, void* stream) {
    return ingest_run(IngestReq{.engine = e, .src = {.pix = pix, .offsets = offsets, .shapes = shapes, .B = B}, .fit = true, .Fh = Fh, .Fw = Fw,
                                .C = C, .Hc = Hc, .Wc = Wc, .box = box_out, .sizes_out = sizes_out, .scratch = scratch, .scratch_bytes = scratch_bytes}, stream);
}

// (the list, the level and the margin are checked before the engine or the device is looked at)
int txo_ingest_trim_views(txo_engine* e, const uint8_t* pix, const int64_t* offsets, const int32_t* shapes, int32_t B, int32_t level, int32_t margin,
                          int32_t* views_out, void* stream) {
    if (int r = ingest_check_shapes(shapes, B, nullptr)) return r;
    if (!offsets) return fail(TXO_E_INVALID, "ingest: null offsets");
    for (int b = 0; b < B; ++b)
        if (int r = ingest_check_offset(offsets[b], b)) return r;
    if (level < 0 || level > 254)
        return fail(TXO_E_INVALID, "ingest: the trim level is " + std::to_string(level) + "; it must lie in [0, 254] (a pixel is ink where a channel is <= level)");
    if (margin < 0) return fail(TXO_E_INVALID, "ingest: the trim margin is " + std::to_string(margin) + "; it must be >= 0");
    if (!e || !pix || !views_out) return fail(TXO_E_INVALID, "ingest: null argument");
    return e->impl->trim_views(IngestList{pix, offsets, shapes, B}, level, margin, views_out, (hipStream_t)stream);
}

// (the list and the views first, then everything txo_ingest_u8 / txo_ingest_u8_fit check, on the views: before the engine or the device is looked at)
int txo_ingest_u8_view(txo_engine* e, const uint8_t* pix, const int64_t* offsets, const int32_t* shapes, const int32_t* views, int32_t B, int32_t C,
                       int32_t Fh, int32_t Fw, int32_t Hc, int32_t Wc, float* box_out, int32_t* sizes_out, void* scratch, int64_t scratch_bytes,
                       void* stream) {
    return ingest_run(IngestReq{.engine = e, .src = {.pix = pix, .offsets = offsets, .shapes = shapes, .B = B}, .view = true, .views = views,
                                .fit = Fh != 0 || Fw != 0, .Fh = Fh, .Fw = Fw, .C = C, .Hc = Hc, .Wc = Wc, .box = box_out, .sizes_out = sizes_out,
                                .scratch = scratch, .scratch_bytes = scratch_bytes}, stream);
}

int txo_decode_step(txo_engine* e, const int64_t* tok_in, int32_t t, float* logits_out, int64_t* tok_out, void* stream) {
    if (!e) return fail(TXO_E_INVALID, "null engine");
    return e->impl->decode_step(tok_in, t, logits_out, tok_out, (hipStream_t)stream);
}

int txo_decode_prefill(txo_engine* e, const int64_t* tokens, int32_t t, float* logits_out, void* stream) {
    if (!e || !tokens) return fail(TXO_E_INVALID, "null argument");
    return e->impl->decode_prefill(tokens, t, logits_out, (hipStream_t)stream);
}

int txo_decode_attn(txo_engine* e, const int64_t* tokens, int32_t t, float* logits_out, float* self_attn_out, float* cross_attn_out,
                    float* cross_mean_out, void* stream) {
    if (!e || !tokens) return fail(TXO_E_INVALID, "null argument");
    if (!self_attn_out && !cross_attn_out && !cross_mean_out) return fail(TXO_E_INVALID, "txo_decode_attn: no attention map was asked for (all three outputs are NULL)");
    return e->impl->decode_attn(tokens, t, logits_out, self_attn_out, cross_attn_out, cross_mean_out, (hipStream_t)stream);
}

int txo_decode_score(txo_engine* e, const int64_t* tokens, int32_t L, float* logp_out, int64_t* top1_out, float* top1_logp_out, void* stream) {
    if (!e || !tokens) return fail(TXO_E_INVALID, "null argument");
    if (L < 2 || L > e->impl->cfg.max_len + 1) return fail(TXO_E_INVALID, "score: L must be in [2, max_len + 1]");
    return e->impl->decode_score(tokens, L, logp_out, top1_out, top1_logp_out, (hipStream_t)stream);
}

int txo_score(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t H, int32_t W, const int64_t* tokens, const uint8_t* mask, int32_t L,
              float* logp_out, int64_t* top1_out, float* top1_logp_out, void* stream) {
    if (!e || !img || !tokens) return fail(TXO_E_INVALID, "null argument");
    if (L < 2 || L > e->impl->cfg.max_len + 1) return fail(TXO_E_INVALID, "score: L must be in [2, max_len + 1]");
    return e->impl->score(img, B, C, H, W, tokens, mask, L, logp_out, top1_out, top1_logp_out, (hipStream_t)stream);
}

// k and the two outputs of the *_alts scoring entries
static int check_score_alts(txo_engine* e, int32_t k, const int32_t* ids, const float* lp) {
    if (k < 1 || k > txo::ALTS_MAX)
        return fail(TXO_E_INVALID, "alternatives: k is " + std::to_string(k) + "; it must be in [1, " + std::to_string(txo::ALTS_MAX) + "]");
    if (k > e->impl->cfg.vocab)
        return fail(TXO_E_INVALID, "alternatives: k is " + std::to_string(k) + " and the vocabulary has " + std::to_string(e->impl->cfg.vocab) + " entries");
    if (!ids || !lp) return fail(TXO_E_INVALID, "alternatives: alt_ids_out_dev and alt_logp_out_dev must not be NULL");
    return 0;
}

int txo_decode_score_alts(txo_engine* e, const int64_t* tokens, int32_t L, float* logp_out, int64_t* top1_out, float* top1_logp_out, int32_t k,
                          int32_t* alt_ids_out, float* alt_logp_out, void* stream) {
    if (!e || !tokens) return fail(TXO_E_INVALID, "null argument");
    if (L < 2 || L > e->impl->cfg.max_len + 1) return fail(TXO_E_INVALID, "score: L must be in [2, max_len + 1]");
    if (int r = check_score_alts(e, k, alt_ids_out, alt_logp_out)) return r;
    return e->impl->decode_score_alts(tokens, L, logp_out, top1_out, top1_logp_out, k, alt_ids_out, alt_logp_out, (hipStream_t)stream);
}

int txo_score_alts(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t H, int32_t W, const int64_t* tokens, const uint8_t* mask, int32_t L,
                   float* logp_out, int64_t* top1_out, float* top1_logp_out, int32_t k, int32_t* alt_ids_out, float* alt_logp_out, void* stream) {
    if (!e || !img || !tokens) return fail(TXO_E_INVALID, "null argument");
    if (L < 2 || L > e->impl->cfg.max_len + 1) return fail(TXO_E_INVALID, "score: L must be in [2, max_len + 1]");
    if (int r = check_score_alts(e, k, alt_ids_out, alt_logp_out)) return r;
    return e->impl->score_alts(img, B, C, H, W, tokens, mask, L, logp_out, top1_out, top1_logp_out, k, alt_ids_out, alt_logp_out, (hipStream_t)stream);
}

int txo_score_ragged(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t Hc, int32_t Wc, const int32_t* sizes, const int64_t* tokens,
                     const uint8_t* mask, int32_t L, float* logp_out, int64_t* top1_out, float* top1_logp_out, void* stream) {
    if (!e || !img || !sizes || !tokens) return fail(TXO_E_INVALID, "null argument");
    if (L < 2 || L > e->impl->cfg.max_len + 1) return fail(TXO_E_INVALID, "score: L must be in [2, max_len + 1]");
    return e->impl->score_ragged(img, B, C, Hc, Wc, sizes, tokens, mask, L, logp_out, top1_out, top1_logp_out, (hipStream_t)stream);
}

int txo_decode_set_key_mask(txo_engine* e, const uint8_t* mask, int32_t cols, void* stream) {
    if (!e) return fail(TXO_E_INVALID, "null engine");
    return e->impl->decode_set_key_mask(mask, cols, (hipStream_t)stream);
}

int txo_generate(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t H, int32_t W, int32_t max_len,
                 int32_t eos, int64_t* tokens_out, int32_t* n_steps, float* logits_out, void* stream) {
    if (!e || !img || !tokens_out) return fail(TXO_E_INVALID, "null argument");
    return e->impl->generate(DecodeReq{.src = {.img = img, .B = B, .C = C, .H = H, .W = W}, .max_len = max_len, .eos = eos,
                                       .tokens = tokens_out, .n_steps = n_steps, .logits = logits_out}, (hipStream_t)stream);
}

int txo_generate_logp(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t H, int32_t W, int32_t max_len,
                      int32_t eos, int64_t* tokens_out, int32_t* n_steps, float* logits_out, float* logp_out, void* stream) {
    if (!e || !img || !tokens_out || !logp_out) return fail(TXO_E_INVALID, "null argument");
    return e->impl->generate(DecodeReq{.src = {.img = img, .B = B, .C = C, .H = H, .W = W}, .max_len = max_len, .eos = eos,
                                       .tokens = tokens_out, .n_steps = n_steps, .logits = logits_out, .logp = logp_out}, (hipStream_t)stream);
}

int txo_generate_from_enc(txo_engine* e, const float* enc, int32_t B, int32_t N, int32_t max_len, int32_t eos,
                          int64_t* tokens_out, int32_t* n_steps, float* logits_out, void* stream) {
    if (!e || !enc || !tokens_out) return fail(TXO_E_INVALID, "null argument");
    return e->impl->generate(DecodeReq{.src = {.enc = enc, .B = B, .N = N}, .max_len = max_len, .eos = eos,
                                       .tokens = tokens_out, .n_steps = n_steps, .logits = logits_out}, (hipStream_t)stream);
}

int txo_generate_from_enc_logp(txo_engine* e, const float* enc, int32_t B, int32_t N, int32_t max_len, int32_t eos,
                               int64_t* tokens_out, int32_t* n_steps, float* logits_out, float* logp_out, void* stream) {
    if (!e || !enc || !tokens_out || !logp_out) return fail(TXO_E_INVALID, "null argument");
    return e->impl->generate(DecodeReq{.src = {.enc = enc, .B = B, .N = N}, .max_len = max_len, .eos = eos,
                                       .tokens = tokens_out, .n_steps = n_steps, .logits = logits_out, .logp = logp_out}, (hipStream_t)stream);
}

int txo_generate_prefix(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t H, int32_t W, const int64_t* prefix, int32_t P,
                        const int32_t* prefix_len, int32_t max_len, int32_t eos, int64_t* tokens_out, int32_t* n_steps, float* logp_out,
                        float* prefix_logp_out, void* stream) {
    if (!e || !img || !prefix || !tokens_out) return fail(TXO_E_INVALID, "prefix decode: null argument");
    return e->impl->generate(DecodeReq{.src = {.img = img, .B = B, .C = C, .H = H, .W = W}, .max_len = max_len, .eos = eos,
                                       .prefix = prefix, .P = P, .prefix_len = prefix_len,
                                       .tokens = tokens_out, .n_steps = n_steps, .logp = logp_out, .prefix_logp = prefix_logp_out}, (hipStream_t)stream);
}

int txo_generate_prefix_from_enc(txo_engine* e, const float* enc, int32_t B, int32_t N, const int64_t* prefix, int32_t P, const int32_t* prefix_len,
                                 int32_t max_len, int32_t eos, int64_t* tokens_out, int32_t* n_steps, float* logp_out, float* prefix_logp_out,
                                 void* stream) {
    if (!e || !enc || !prefix || !tokens_out) return fail(TXO_E_INVALID, "prefix decode: null argument");
    return e->impl->generate(DecodeReq{.src = {.enc = enc, .B = B, .N = N}, .max_len = max_len, .eos = eos,
                                       .prefix = prefix, .P = P, .prefix_len = prefix_len,
                                       .tokens = tokens_out, .n_steps = n_steps, .logp = logp_out, .prefix_logp = prefix_logp_out}, (hipStream_t)stream);
}

int txo_generate_prefix_ragged(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t Hc, int32_t Wc, const int32_t* sizes,
                               const int64_t* prefix, int32_t P, const int32_t* prefix_len, int32_t max_len, int32_t eos, int64_t* tokens_out,
                               int32_t* n_steps, float* logp_out, float* prefix_logp_out, void* stream) {
    if (!e || !img || !sizes || !prefix || !tokens_out) return fail(TXO_E_INVALID, "prefix decode: null argument");
    return e->impl->generate(DecodeReq{.src = {.img = img, .sizes = sizes, .B = B, .C = C, .H = Hc, .W = Wc}, .max_len = max_len, .eos = eos,
                                       .prefix = prefix, .P = P, .prefix_len = prefix_len,
                                       .tokens = tokens_out, .n_steps = n_steps, .logp = logp_out, .prefix_logp = prefix_logp_out}, (hipStream_t)stream);
}

int txo_generate_beam(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t H, int32_t W, int32_t beams, int32_t max_len,
                      int32_t eos, int64_t* tokens_out, float* scores_out, int64_t* all_tokens_out, int32_t* n_steps, void* stream) {
    if (!e || !img || !tokens_out) return fail(TXO_E_INVALID, "null argument");
    return e->impl->beam_search(DecodeSrc{.img = img, .B = B, .C = C, .H = H, .W = W}, beams, max_len, eos,
                                BeamSink{.best = tokens_out, .scores = scores_out, .all = all_tokens_out}, n_steps, (hipStream_t)stream);
}

int txo_beam_search(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t H, int32_t W, int32_t beams, int32_t max_len,
                    int32_t eos, const txo_beam_out* out, int32_t* n_steps, void* stream) {
    if (!e || !img) return fail(TXO_E_INVALID, "null argument");
    return e->impl->beam_search(DecodeSrc{.img = img, .B = B, .C = C, .H = H, .W = W}, beams, max_len, eos, BeamSink{.out = out}, n_steps, (hipStream_t)stream);
}

int txo_beam_search_ragged(txo_engine* e, const float* img, int32_t B, int32_t C, int32_t Hc, int32_t Wc, const int32_t* sizes,
                           int32_t beams, int32_t max_len, int32_t eos, const txo_beam_out* out, int32_t* n_steps, void* stream) {
    if (!e || !img || !sizes) return fail(TXO_E_INVALID, "null argument");
    return e->impl->beam_search(DecodeSrc{.img = img, .sizes = sizes, .B = B, .C = C, .H = Hc, .W = Wc}, beams, max_len, eos, BeamSink{.out = out}, n_steps,
                                (hipStream_t)stream);
}

int txo_set_sampling(txo_engine* e, int32_t mode, int32_t topk, float temp, uint64_t seed) {
    if (!e) return fail(TXO_E_INVALID, "null engine");
    if (mode != 0 && mode != 1) return fail(TXO_E_INVALID, "sampling mode must be 0 (greedy) or 1 (top-k / temperature / multinomial)");
    if (mode == 1 && (topk < 1 || !(temp > 0.f))) return fail(TXO_E_INVALID, "sampling needs topk >= 1 and temp > 0");
    const int V = e->impl->cfg.vocab;
    if (mode == 1 && !sample_in_regs(V) && (size_t)V * sizeof(float) > e->impl->sample_lds_max)
        return fail(TXO_E_INVALID, "sampling: the vocabulary does not fit the sampler's LDS (vocab * 4 bytes per workgroup: txo_engine_query "
                                   "TXO_Q_SAMPLE_VOCAB_MAX)");
    e->impl->sample_mode = mode; e->impl->sample_topk = topk; e->impl->sample_temp = mode ? temp : 1.f; e->impl->sample_seed = seed;
    return 0;
}

// (the table is checked first: those refusals need neither an engine nor a device)
int txo_set_token_rules(txo_engine* e, const int32_t* rules_host, int32_t S, int32_t V, int32_t depth_max) {
    if (!rules_host) {
        if (!e) return fail(TXO_E_INVALID, "null engine");
        return e->impl->set_token_rules(nullptr, 0, 0);
    }
    if (S < 1 || S > RULES_MAX_STATES)
        return fail(TXO_E_INVALID, "token rules: S is " + std::to_string(S) + "; the number of states must be in [1, " + std::to_string(RULES_MAX_STATES) + "]");
    if (depth_max < 1 || depth_max > 255)
        return fail(TXO_E_INVALID, "token rules: depth_max is " + std::to_string(depth_max) + "; it must be in [1, 255]");
    if (V < 1) return fail(TXO_E_INVALID, "token rules: V must be >= 1");
    for (int s = 0; s < S; ++s) {
        bool always = false;                                          // a token this state allows at every depth
        for (int v = 0; v < V; ++v) {
            const int r = rules_host[(size_t)s * V + v];
            if (rule_next(r) >= S)
                return fail(TXO_E_INVALID, "token rules: rules[" + std::to_string(s) + "][" + std::to_string(v) + "] has next = " + std::to_string(rule_next(r)) +
                                               ", not a state below S = " + std::to_string(S));
            always = always || (!(r & (RULE_BAN | RULE_ONLY_AT_ZERO)) && rule_need(r) == 0 && rule_delta(r) <= 0);
        }
        if (!always)
            return fail(TXO_E_INVALID, "token rules: state " + std::to_string(s) + " has no always-allowed token (not BAN, not ONLY_AT_ZERO, need == 0, delta <= 0): "
                                       "a row could face an empty allowed set");
    }
    if (!e) return fail(TXO_E_INVALID, "null engine");
    if (V != e->impl->cfg.vocab)
        return fail(TXO_E_INVALID, "token rules: V is " + std::to_string(V) + " but the engine's vocabulary has " + std::to_string(e->impl->cfg.vocab) + " entries");
    if (!e->impl->ready) return fail(TXO_E_STATE, "weights not finalized");
    return e->impl->set_token_rules(rules_host, S, depth_max);
}

int txo_last_rule_state(txo_engine* e, int32_t* state_out_dev, int32_t B, void* stream) {
    if (!e || !state_out_dev) return fail(TXO_E_INVALID, "null argument");
    return e->impl->last_rule_state(state_out_dev, B, (hipStream_t)stream);
}

int txo_set_rules_beam(txo_engine* e, int32_t on) {
    if (!e) return fail(TXO_E_INVALID, "null engine");
    if (on != 0 && on != 1) return fail(TXO_E_INVALID, "txo_set_rules_beam: on must be 0 or 1");
    e->impl->rules_beam = on != 0;
    return 0;
}

int txo_set_guard_beam(txo_engine* e, int32_t on) {
    if (!e) return fail(TXO_E_INVALID, "null engine");
    if (on != 0 && on != 1) return fail(TXO_E_INVALID, "txo_set_guard_beam: on must be 0 or 1");
    e->impl->guard_beam = on != 0;
    return 0;
}

int txo_last_beam_rule_state(txo_engine* e, int32_t* state_out_dev, int32_t B, int32_t beams, void* stream) {
    if (!e || !state_out_dev) return fail(TXO_E_INVALID, "null argument");
    return e->impl->last_beam_rule_state(state_out_dev, B, beams, (hipStream_t)stream);
}

int txo_set_rules_close(txo_engine* e, int32_t on) {
    if (!e) return fail(TXO_E_INVALID, "null engine");
    if (on != 0 && on != 1) return fail(TXO_E_INVALID, "txo_set_rules_close: on must be 0 or 1");
    return e->impl->set_rules_close(on != 0);
}

int txo_set_repeat_guard(txo_engine* e, int32_t max_period, int32_t max_repeats) {
    if (max_period == 0 && max_repeats == 0) {
        if (!e) return fail(TXO_E_INVALID, "null engine");
        e->impl->guard_p = e->impl->guard_r = 0;
        return 0;
    }
    if (max_period < 1 || max_period > GUARD_MAX)
        return fail(TXO_E_INVALID, "repeat guard: max_period is " + std::to_string(max_period) + "; it must be in [1, " + std::to_string(GUARD_MAX) + "] (0, 0 switches the guard off)");
    if (max_repeats < 1 || max_repeats > GUARD_MAX)
        return fail(TXO_E_INVALID, "repeat guard: max_repeats is " + std::to_string(max_repeats) + "; it must be in [1, " + std::to_string(GUARD_MAX) + "] (0, 0 switches the guard off)");
    if (!e) return fail(TXO_E_INVALID, "null engine");
    if (e->impl->cfg.vocab <= max_period + 1)
        return fail(TXO_E_INVALID, "repeat guard: the vocabulary has " + std::to_string(e->impl->cfg.vocab) + " entries; it needs more than max_period + 1 = " +
                                   std::to_string(max_period + 1) + " (the guard may ban max_period tokens at a pick)");
    e->impl->guard_p = max_period; e->impl->guard_r = max_repeats;
    return 0;
}

int txo_set_alternatives(txo_engine* e, int32_t k) {
    if (k == 0) {
        if (!e) return fail(TXO_E_INVALID, "null engine");
        e->impl->alts_k = 0;
        return 0;
    }
    if (k < 1 || k > txo::ALTS_MAX)
        return fail(TXO_E_INVALID, "alternatives: k is " + std::to_string(k) + "; it must be in [1, " + std::to_string(txo::ALTS_MAX) + "] (0 switches them off)");
    if (!e) return fail(TXO_E_INVALID, "null engine");
    if (k > e->impl->cfg.vocab)
        return fail(TXO_E_INVALID, "alternatives: k is " + std::to_string(k) + " and the vocabulary has " + std::to_string(e->impl->cfg.vocab) + " entries");
    e->impl->alts_k = k;
    return 0;
}

int txo_last_alternatives(txo_engine* e, int32_t* ids_out, float* logp_out, int32_t B, int32_t cols, void* stream) {
    if (!e) return fail(TXO_E_INVALID, "null engine");
    return e->impl->last_alternatives(ids_out, logp_out, B, cols, (hipStream_t)stream);
}

int txo_rules_close_dist(txo_engine* e, int32_t* out_host, int32_t S, int32_t D) {
    if (!e || !out_host) return fail(TXO_E_INVALID, "null argument");
    if (!e->impl->closing()) return fail(TXO_E_STATE, "txo_rules_close_dist: no table -- token rules and txo_set_rules_close must both be set");
    if (S != e->impl->rules_S || D != e->impl->rules_dmax + 1)
        return fail(TXO_E_INVALID, "txo_rules_close_dist: S and D must be " + std::to_string(e->impl->rules_S) + " and " + std::to_string(e->impl->rules_dmax + 1) +
                                   ", the states and depth_max + 1 of the installed rules");
    std::copy(e->impl->close_dist.begin(), e->impl->close_dist.end(), out_host);
    return 0;
}

int txo_set_ragged_hybrid(txo_engine* e, int32_t on) {
    if (!e) return fail(TXO_E_INVALID, "null engine");
    if (on != 0 && on != 1) return fail(TXO_E_INVALID, "txo_set_ragged_hybrid: on must be 0 or 1");
    e->impl->rag_hybrid = on != 0;
    return 0;
}

int txo_set_ragged_forward(txo_engine* e, int32_t on) {
    if (!e) return fail(TXO_E_INVALID, "null engine");
    if (on != 0 && on != 1) return fail(TXO_E_INVALID, "txo_set_ragged_forward: on must be 0 or 1");
    e->impl->rag_fwd = on != 0;
    return 0;
}

int txo_set_stop_mode(txo_engine* e, int32_t mode) {
    if (!e) return fail(TXO_E_INVALID, "null engine");
    if (mode != TXO_STOP_GLOBAL && mode != TXO_STOP_ROW) return fail(TXO_E_INVALID, "stop mode must be TXO_STOP_GLOBAL or TXO_STOP_ROW");
    e->impl->stop_mode = mode;
    return 0;
}
int txo_profile_enable(txo_engine* e, int32_t on) { return e ? e->impl->profile_enable(on) : fail(TXO_E_INVALID, "null engine"); }
int txo_profile_read(txo_engine* e, int32_t kind, double* avg_ms, int64_t* count) {
    return e ? e->impl->profile_read(kind, avg_ms, count) : fail(TXO_E_INVALID, "null engine");
}

int txo_engine_query(txo_engine* e, int32_t what, int64_t* out) {
    if (!e || !out) return fail(TXO_E_INVALID, "null argument");
    return e->impl->query(what, out);
}

const char* txo_last_error(void) { return g_err.c_str(); }
const char* txo_version(void) { return "texocr-amd 0.1 (gfx950)"; }

}  // extern "C"
