// Session, the open decode session, ImageBatch, what an encode is given, and DecodeReq, what a decode is asked for, as values.  Host code,
// included by engine.hip only (after lanes.h).
#pragma once

namespace txo {
// One decode session.  Engine::begin_session assigns a freshly constructed one, so nothing survives a new session by omission; behind it
// only the transitions of a running decode write a field (Engine::ensure_ckv, the key-mask calls, choose_form and the ends of generate).
struct Session {
    int rows = 0, keys = 0, images = 0;   // decode rows, encoder tokens per image (ragged: the slot stride), images behind the cross K/V cache
    bool open = false, ragged = false;    // ragged: per-slot key counts (Engine::slens)
    bool latent = false;                  // the cross attention runs in latent form (lat_attn.h) ...
    bool lat_self = false;                // ... and the self attention too (the history is z, not k / v)
    bool ckv_valid = false;               // the projected cross K/V panels exist (the prefill needs them; the latent form does not)
    bool kmask_on = false;                // padding mask over the decoded positions (txo_decode_set_key_mask)
    bool row_stop = false;                // this generate compacts the live rows of its row ranges (launch path, stop_mode 1)
    bool forced = false;                  // a prompted decode: the steps force the caller's prefix (step_prefix.h; launch path only)
    bool ruled = false;                   // a constrained decode: the steps pick under the engine's token rules (step_rules.h; launch path only)
    bool closing = false;                 // ... and under the closing budget (txo_set_rules_close; implies ruled)
    int guard_p = 0, guard_r = 0;         // a guarded decode: the steps pick under the repeat guard (step_guard.h; launch path only), 0: none
    bool guarded() const { return guard_p > 0; }
    int alts = 0;                         // the steps keep the k best of every row in front of the pick (step_alts.h; launch path only), 0: off
    // what a captured step was built for (lanes.h): every field a step's launches depend on (strides and row count are baked into them)
    // rules: what a constrained step bakes of the rule set (states * 256 + depth cap, + 4096 for a closing decode's kernels; the tables
    // themselves stay in the engine's buffers; + 8192 * (17 * max_period + max_repeats) for a guarded decode's)
    LaneSet::GraphKey graph_key(const LaneSet::Lane& ln, int eos, int sample_mode, bool logp, int rules = 0) const {
        return {ln.b0, ln.nb, keys, eos, rows, images,
                (int)latent + 2 * (int)lat_self + 4 * (int)row_stop + 8 * sample_mode + 16 * (int)ragged + 32 * (int)logp + 64 * (int)forced + 128 * ((ruled ? rules : 0) + 8192 * (17 * guard_p + guard_r)), alts};
    }
};
struct KeyCounts { const int* dev = nullptr; const int32_t* host = nullptr; };   // a ragged session's key count per image: a device array or the caller's host array (staged)

// What an encode is given: B images of C x H x W, N tokens each.  A ragged batch: H x W is the CONTAINER, N the slot stride of the encoder's
// rows, and the sizes of image b are in Engine::rag_hw / rag_ntok at first + b.  Built by Engine::fixed_batch / ragged_batch, which check it.
struct ImageBatch {
    int B = 0, C = 0, H = 0, W = 0, N = 0;
    bool ragged = false; int first = 0;
    size_t pixels() const { return (size_t)C * H * W; }   // of one image (slot)
    ImageBatch chunk(int b0, int nb) const { ImageBatch c = *this; c.first = first + b0; c.B = nb; return c; }
};

// What a decode is asked to read, as the caller gave it: img = B images [B][C][H][W] (with sizes [B][2] on the host a ragged batch whose
// container is H x W), or enc = encoder rows [B][N][D].  Engine::resolve_source checks it.
struct DecodeSrc {
    const float* img = nullptr; const float* enc = nullptr; const int32_t* sizes = nullptr;
    int B = 0, C = 0, H = 0, W = 0, N = 0;
};
// ... and checked: the images of `ib` (images) or the caller's encoder rows, B rows of N keys either way
struct Source {
    ImageBatch ib; bool images = false; const float* data = nullptr; int B = 0, N = 0;
    const ImageBatch* batch() const { return images ? &ib : nullptr; }
    bool ragged() const { return images && ib.ragged; }
};

// One token decode, what every txo_generate* entry asks for: the source, the loop's bounds, a prefix to force (prefix null: none; [B][P] on
// the device, prefix_len [B] on the host or null = every row has P), where the results go (texocr.h says which may be null).
struct DecodeReq {
    DecodeSrc src;
    int max_len = 0, eos = -1;
    const int64_t* prefix = nullptr; int P = 0; const int32_t* prefix_len = nullptr;
    int64_t* tokens = nullptr; int* n_steps = nullptr; float* logits = nullptr; float* logp = nullptr; float* prefix_logp = nullptr;
};
// The request behind Engine::generate's checks, what the decode loop and its two paths take.  m / M: the shortest / longest prefix
// length of a prompted decode (the lengths themselves are in Engine::flen by then).
struct Decode {
    const DecodeReq& q; Source src; int m = 0, M = 0;
    bool prompted() const { return q.prefix != nullptr; }
};

// Where a beam search's results go: txo_generate_beam's three buffers (best beam [B][max_len] -- never null there --, scores, every beam), or
// the txo_beam_out of txo_beam_search / _ragged (best null)
struct BeamSink { int64_t* best; float* scores; int64_t* all; const txo_beam_out* out; };

}  // namespace txo
