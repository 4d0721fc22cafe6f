/*
 * texocr.h -- C ABI of the MI355X-native engine for TeXOCR's OCRModel.generate() hot path.
 *
 * The reference (olibridge01/TeXOCR) is pure Python; it has no FFI/plugin interface, so the drop-in
 * boundary is its nn.Module call surface.  Each entry point below replaces one reference callable
 * (file:line relative to the reference tree); texocr_amd/model.py binds them through ctypes and presents
 * the reference's own class/method names.  Plain pointers and sizes only -- no torch types.
 *
 * Conventions
 *   - every *_dev pointer is DEVICE memory owned by the caller; the engine owns its weight copy, KV caches
 *     and workspace (allocated in txo_engine_create, freed in txo_engine_destroy; no allocation in any
 *     encode/decode call -- the diagnostic modes TXO_STAMPS=<file> and txo_profile_enable(e, 1) are the exceptions: they
 *     create their stamp buffer / HIP events on first use);
 *   - all work is enqueued on the caller's hipStream_t (`stream`, may be NULL = default stream) and is
 *     asynchronous except where noted; one engine per (device, stream); a handle is not thread-safe;
 *   - return value: 0 = ok, <0 = error (TXO_E_*); txo_last_error() returns a thread-local message;
 *   - images: float32 NCHW; token ids: int64; encoder output / logits: float32.
 */
#ifndef TEXOCR_H
#define TEXOCR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TXO_OK 0
#define TXO_E_INVALID (-1)   /* bad argument / unsupported shape (maps to ValueError)  */
#define TXO_E_STATE (-2)     /* call order / missing weights (maps to RuntimeError)    */
#define TXO_E_HIP (-3)       /* HIP runtime error (maps to RuntimeError)               */

#define TXO_EMBED_PATCH 0
#define TXO_EMBED_HYBRID 1

#define TXO_F32 0            /* parity mode: f32 storage, exact-f32 MFMA               */
#define TXO_BF16 1           /* perf mode: bf16 weights / K,V caches / GEMM operands, f32 accumulate */

typedef struct txo_engine txo_engine;

/* Mirrors the values create_model(config) reads (model/ocr_model.py:113-130, model/encoder.py:172-191,
 * model/decoder.py:148-173) plus capacity limits for the engine-owned buffers. */
typedef struct txo_config {
    int32_t canvas_h;      /* VisionTransformer img_size: max canvas height, pixels (encoder.py:95)       */
    int32_t canvas_w;      /* ... and width; the hybrid factory uses (160, 1008) (encoder.py:183)         */
    int32_t embed;         /* TXO_EMBED_PATCH: PatchEmbedding (encoder.py:11-28) | TXO_EMBED_HYBRID:
                              ResNetV2 [2,4,6] backbone + 1x1 proj, what create_encoder builds (:162-191) */
    int32_t in_channels;   /* image channels (PatchEmbedding in_channels; the hybrid embedder needs 1)    */
    int32_t embed_dim;     /* encoder == decoder width (no enc->dec projection, attention.py:89-91)       */
    int32_t enc_heads, enc_layers, dec_heads, dec_layers;
    int32_t enc_exp, dec_exp;   /* FFN expansion (MLP exp_factor, attention.py:46)                        */
    int32_t vocab;         /* config['vocab_size']                                                        */
    int32_t max_len;       /* config['max_length'] = decoder positional table length, decoder.py:28       */
    int32_t bos, eos, pad; /* config bos_token / eos_token / trg_pad_idx                                  */
    int32_t dtype;         /* TXO_F32 | TXO_BF16                                                          */
    int32_t max_batch;     /* capacity: images per call                                                   */
    int32_t max_tokens;    /* capacity: encoder tokens per image (<= 1 + canvas_h*canvas_w/256); 0 = that maximum */
} txo_config;

/* OCRModel.__init__ / create_model (ocr_model.py:16-32,113-130): allocate the engine. */
int txo_engine_create(const txo_config* cfg, txo_engine** out);
void txo_engine_destroy(txo_engine* e);

/* nn.Module.load_state_dict, one tensor at a time (key layout of OCRModel.state_dict()):
 * `key` is the reference state_dict key, `data` HOST float32, `shape`/`ndim` its shape.  Aliased shared
 * LayerNorm keys (layers.{s}.0.weight for every s, attention.py:200,221) may all be passed; they must
 * carry identical values.  txo_engine_finalize_weights checks completeness, refuses non-finite values (TXO_E_INVALID, the key is
 * named in txo_last_error) and uploads. */
int txo_engine_set_weight(txo_engine* e, const char* key, const float* data, const int64_t* shape, int32_t ndim);
int txo_engine_finalize_weights(txo_engine* e);

/* VisionEncoder.forward (encoder.py:128-152): img_dev [B,C,H,W] -> enc_out_dev [B, 1+(H/16)(W/16), D].
 * Non-finite input: weights are checked (txo_engine_finalize_weights refuses NaN / inf); pixels are not.  A non-finite pixel makes the
 * rows of ITS OWN image unspecified -- encoder rows, logits, and token ids that are unspecified but always inside the vocabulary (the
 * reference would return NaN logits and argmax's pick among them) -- and touches no other image of the batch: rows never interact. */
int txo_encode(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t H, int32_t W,
               float* enc_out_dev, void* stream);

/* Start a decode over `enc_dev` [B,N,D] (the `enc=` kwarg of decoder.generate / net, decoder.py:56,103):
 * projects the cross-attention K/V of every decoder layer once (attention.py:125-126), clears the
 * self-attention cache, position <- 0, current token <- bos. */
int txo_decode_begin(txo_engine* e, const float* enc_dev, int32_t B, int32_t N, void* stream);

/* One position of Transformer.forward in KV-cached form (decoder.py:41-67): feeds tok_in_dev[B] (NULL =
 * the engine's current token: bos, or the previous step's argmax) at position t (t must equal the number
 * of positions decoded since txo_decode_begin, or less to rewind), writes the position's logits
 * [B,vocab] to logits_out_dev (may be NULL) and their argmax to tok_out_dev[B] (may be NULL).  Token ids outside [0, vocab) are
 * forced into the table (the reference's nn.Embedding raises IndexError; the Python facade checks and raises too). */
int txo_decode_step(txo_engine* e, const int64_t* tok_in_dev, int32_t t, float* logits_out_dev,
                    int64_t* tok_out_dev, void* stream);

/* Transformer.forward over a whole prefix in ONE pass (reference model/decoder.py:41-67: token + position embedding, the
 * decoder stack with a causal self attention, final LayerNorm, logits for EVERY position) -- the multi-position form of
 * txo_decode_step.  tokens_dev: int64 [B][t] row-major (B = the batch of the session opened by txo_decode_begin), positions
 * 0..t-1, 1 <= t <= cfg.max_len.  logits_out_dev: float [B][t][vocab] or NULL.  Side effect: the self-attention K/V cache holds
 * rows 0..t-1 afterwards, so txo_decode_step(e, tok, t, ...) continues behind it.  This is what decoder.net(x, mask, enc=) maps to
 * (teacher-forced logits), and what the sliding window of AutoRegressiveDecoder.generate (decoder.py:99-100) costs per token. */
int txo_decode_prefill(txo_engine* e, const int64_t* tokens_dev, int32_t t, float* logits_out_dev, void* stream);

/* AutoRegressiveDecoder.forward (decoder.py:124-145) without autograd, on the session opened by txo_decode_begin.
 * tokens_dev int64 [B][L], 2 <= L <= cfg.max_len + 1: columns 0..L-2 are fed (one causal multi-position pass, key mask of
 * txo_decode_set_key_mask honoured), column p+1 is the target of position p.  Outputs, each [B][L-1], each may be NULL:
 * logp_out (float) log_softmax(logits[b,p])[tokens[b,p+1]];  top1_out (int64) argmax of logits[b,p] (lowest index among equals);
 * top1_logp_out (float) its log-probability.  The logits are formed tile by tile inside one kernel (texocr_amd/csrc/score.h) and
 * never stored: no [B][L-1][vocab] buffer exists, and any vocabulary size is accepted (txo_decode_prefill's logits_out needs a
 * multiple of 8).  Token ids outside [0, vocab) are forced into the table on both sides -- as inputs like txo_decode_step, and as
 * TARGETS: the score returned is the clamped id's (the Python facade raises IndexError first).  Scores at padded positions, and
 * at positions whose target is padding, are unspecified.  Side effect as txo_decode_prefill: self K/V rows 0..L-2 are filled.
 * Asynchronous on `stream`; results are bit-reproducible run to run. */
int txo_decode_score(txo_engine* e, const int64_t* tokens_dev, int32_t L, float* logp_out_dev, int64_t* top1_out_dev,
                     float* top1_logp_out_dev, void* stream);

/* Transformer.forward(x, mask=, enc=, return_attn=True) (model/decoder.py:41-67): txo_decode_prefill that also returns WHERE every
 * position looked -- the `post_softmax_attn` of every attention block (model/attention.py:166-178).  Same session, same preconditions
 * and refusals, same tokens_dev / t / logits_out_dev (may be NULL; a multiple-of-8 vocabulary otherwise) and the same side effect (self
 * K/V rows 0..t-1 are filled) as txo_decode_prefill; the key mask of txo_decode_set_key_mask is honoured.  Outputs, float32, caller-owned,
 * each may be NULL but not all three (TXO_E_INVALID); Ld = cfg.dec_layers, B = the session's batch, heads = cfg.dec_heads, N = the
 * session's encoder token count (the CLS row 0 included):
 *   self_attn_out_dev  [Ld][B][heads][t][t]  causal self attention: entry [i][j] is exactly 0 for j > i, and for a padded key j at a
 *                                            query i that is not padding; the row of a padded query is unspecified but finite;
 *   cross_attn_out_dev [Ld][B][heads][t][N]  cross attention over the encoder rows;
 *   cross_mean_out_dev [Ld][B][t][N]         the mean of the cross maps over the heads, summed in head order inside one kernel: it does
 *                                            not need cross_attn_out_dev to exist (cfg.dec_heads <= 32, TXO_E_INVALID beyond).
 * Every row sums to 1.  The probabilities are recomputed from the q / k operands of the pass (texocr_amd/csrc/attn_probs.h: two
 * sweeps over the keys, nothing of size t x N is held); logits and K/V cache are bit for bit txo_decode_prefill's, and what one output
 * holds does not depend on which others were asked for.  Asynchronous on `stream`; bit-reproducible run to run; no allocation. */
int txo_decode_attn(txo_engine* e, const int64_t* tokens_dev, int32_t t, float* logits_out_dev,
                    float* self_attn_out_dev,   /* [Ld][B][heads][t][t]  or NULL */
                    float* cross_attn_out_dev,  /* [Ld][B][heads][t][N]  or NULL */
                    float* cross_mean_out_dev,  /* [Ld][B][t][N]         or NULL: mean over heads */
                    void* stream);

/* OCRModel.forward's path (ocr_model.py:38-44) in one call: txo_encode + txo_decode_begin + txo_decode_set_key_mask(mask_dev, L) +
 * txo_decode_score.  mask_dev uint8 [B][L] (0 = padding; its first L-1 columns are the fed positions) or NULL.  The key mask is
 * cleared again before the call returns; the session stays open (txo_decode_step(e, tok, L-1, ...) continues behind it). */
int txo_score(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t H, int32_t W, const int64_t* tokens_dev,
              const uint8_t* mask_dev, int32_t L, float* logp_out_dev, int64_t* top1_out_dev, float* top1_logp_out_dev, void* stream);

/* The `mask` argument of decoder.generate / decoder.net (model/decoder.py:95-101,112: a (B, T0) bool over the start tokens, padded
 * with True for every generated token; model/attention.py:130-155: energy filled with -FLT_MAX where query or key is masked).
 * mask_dev: uint8 [B][cols] on the device, 0 = padding; positions >= cols are not padding; NULL clears the mask.  Applies to the
 * txo_decode_step, txo_decode_prefill, txo_decode_attn and txo_decode_score calls of the session opened by txo_decode_begin or
 * txo_decode_begin_ragged: a padded position is never attended by a
 * query that is not padding.  Rows of padded positions themselves are computed but unspecified (the reference softmaxes them
 * uniformly over all keys; nothing downstream reads them). */
int txo_decode_set_key_mask(txo_engine* e, const uint8_t* mask_dev, int32_t cols, void* stream);

/* OCRModel.generate (ocr_model.py:46-66) + AutoRegressiveDecoder.generate (decoder.py:77-122), greedy:
 * encode, then up to max_len steps; stops early only when EVERY row contains `eos` (pass eos < 0 for
 * eos_tok=None).  tokens_out_dev is [B, max_len] int64 (row stride max_len); *n_steps_out (HOST) receives
 * the number of valid columns -- the reference returns output[:, :n_steps].  logits_out_dev (may be
 * NULL) is [B, max_len, vocab].  max_len may exceed cfg.max_len: the reference then slides its window (decoder.py:99-100:
 * every further token sees the last cfg.max_len tokens at positions re-indexed from 0) and so does this call -- the first
 * cfg.max_len positions through the KV cache, each later token through one multi-position forward of its window
 * (txo_decode_prefill's pass).  Synchronises the stream before returning. */
int txo_generate(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t H, int32_t W,
                 int32_t max_len, int32_t eos, int64_t* tokens_out_dev, int32_t* n_steps_out,
                 float* logits_out_dev, void* stream);

/* Same loop over a caller-provided encoder output (decoder.generate(start_tokens=[bos], enc=enc)). */
int txo_generate_from_enc(txo_engine* e, const float* enc_dev, int32_t B, int32_t N, int32_t max_len,
                          int32_t eos, int64_t* tokens_out_dev, int32_t* n_steps_out, float* logits_out_dev,
                          void* stream);

/* txo_generate / txo_generate_from_enc that also return how sure the model was of every token it produced, from the token selection
 * itself: no second pass and no [B, max_len, vocab] buffer.  logp_out_dev float [B, max_len] (row stride max_len like tokens_out_dev,
 * caller-owned, must not be NULL): logp[b][t] = logits[b][t][tokens[b][t]] - logsumexp_v logits[b][t][v], natural log, on the f32
 * logits the selection read, for the *n_steps_out returned positions.  ALWAYS at temperature 1 over the FULL vocabulary, greedy and
 * sampled (txo_set_sampling) alike: it is the quantity txo_score's logp_out reports for the same tokens, NOT the probability under the
 * sampler's top-k / temperature distribution the draw was made from.  TXO_STOP_GLOBAL: every returned position holds the true value,
 * rows beyond their own eos included.  TXO_STOP_ROW: positions behind a row's first eos hold 0.0, so a row's sum is its sequence
 * log-probability.  Every decode path carries it -- the persistent launch, row ranges, captured steps, live-row compaction, the
 * sliding window -- and tokens, logits and draws are bit-identical to the calls without it.  A row whose logits are non-finite (a
 * non-finite pixel) has unspecified logp; other rows are untouched.  logits_out_dev may be NULL as in txo_generate. */
int txo_generate_logp(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t H, int32_t W,
                      int32_t max_len, int32_t eos, int64_t* tokens_out_dev, int32_t* n_steps_out,
                      float* logits_out_dev, float* logp_out_dev, void* stream);
int txo_generate_from_enc_logp(txo_engine* e, const float* enc_dev, int32_t B, int32_t N, int32_t max_len,
                               int32_t eos, int64_t* tokens_out_dev, int32_t* n_steps_out, float* logits_out_dev,
                               float* logp_out_dev, void* stream);

/* Prompted decode -- AutoRegressiveDecoder.generate(start_tokens of any length T, ...) (decoder.py:77-122), with a BUILD EXTENSION: a
 * length per row.  The loop of txo_generate continues a caller's token prefix instead of starting at BOS, with everything that loop has:
 * captured steps, row ranges, TXO_STOP_ROW with live-row compaction, either cross-attention form, the sampler, ragged batches.
 *   prefix_dev      int64 [B][P] on the device.  prefix[b][0] need not be BOS.  Ids outside the vocabulary are forced into it (as
 *                   txo_decode_score does).
 *   prefix_len_host int32 [B] on the HOST, or NULL = every row has length P.  1 <= len_b <= P; columns of row b at and behind len_b are
 *                   never read.  m = min_b len_b, M = max_b len_b.
 * Positions 0 .. m-2 are computed by ONE multi-position pass (txo_decode_prefill's, without logits; nothing when m == 1); the loop then
 * decodes positions t = m-1 .. M+max_len-2.  At position t a row with t + 1 < len_b commits prefix[b][t+1] as its next token -- no arg-max
 * or draw decides, no output column is written, a sampled decode consumes no draw (draws stay keyed by (seed; row, position)) -- and any
 * other row's pick goes to output column j = t + 1 - len_b if j < max_len.  So column j of row b is the j-th token behind row b's OWN
 * prefix; with equal lengths the result is the reference's output[:, T:].
 *   tokens_out_dev  int64 [B][max_len]; *n_steps_out (HOST) = min(max_len, t_last + 2 - m) valid columns, t_last the last position decoded.
 *                   A column a longer-prefix row did not reach holds cfg.pad (and 0.0 in logp).
 *   logp_out_dev    float [B][max_len] or NULL: txo_generate_logp's log-probabilities of the output columns.
 *   prefix_logp_out_dev float [B][P] or NULL: prefix_logp[b][i] = the log-probability of prefix[b][i] given what precedes it, for the
 *                   tokens the loop forced (m <= i < len_b), computed as (logit[forced] - row max) - log sum exp: where the forced token
 *                   is the arg-max it is bit for bit the float txo_generate_logp reports.  Exactly 0.0 for i < m (the multi-position pass
 *                   does not score), for i >= len_b, and for positions an eos break left undecoded.  Under TXO_STOP_ROW also for every
 *                   column of a row whose prefix holds eos: such a row is finished from the start, nothing is scored for it (under
 *                   TXO_STOP_GLOBAL it is scored like any other).
 * eos: a row counts as containing eos from the start if prefix[b][:len_b] holds it (decoder.py:115 tests the whole output); the global
 * break fires after the first position at which every row contains eos.  TXO_STOP_ROW: columns behind a row's first eos -- every column
 * if the prefix holds one -- are cfg.pad and 0.0.
 * Refused with TXO_E_INVALID before anything is encoded (messages name the prefix): len_b outside [1, P]; M - 1 + max_len > cfg.max_len (a
 * prompted decode does not slide the window); m - 1 beyond the multi-position pass's workspace (max_batch * max_tokens rows).  There is no
 * logits_out.  Runs one launch per stage (TXO_Q_LAST_PERSISTENT reads 0), never with the latent self-attention history.
 * Synchronises the stream before returning; leaves the session generate leaves (none behind the ragged call). */
int txo_generate_prefix(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t H, int32_t W, const int64_t* prefix_dev, int32_t P,
                        const int32_t* prefix_len_host, int32_t max_len, int32_t eos, int64_t* tokens_out_dev, int32_t* n_steps_out,
                        float* logp_out_dev, float* prefix_logp_out_dev, void* stream);
int txo_generate_prefix_from_enc(txo_engine* e, const float* enc_dev, int32_t B, int32_t N, const int64_t* prefix_dev, int32_t P,
                                 const int32_t* prefix_len_host, int32_t max_len, int32_t eos, int64_t* tokens_out_dev, int32_t* n_steps_out,
                                 float* logp_out_dev, float* prefix_logp_out_dev, void* stream);
/* ... over a ragged batch (below: txo_encode_ragged's container and sizes), with every refusal of a ragged batch. */
int txo_generate_prefix_ragged(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t Hc, int32_t Wc, const int32_t* sizes_host,
                               const int64_t* prefix_dev, int32_t P, const int32_t* prefix_len_host, int32_t max_len, int32_t eos,
                               int64_t* tokens_out_dev, int32_t* n_steps_out, float* logp_out_dev, float* prefix_logp_out_dev, void* stream);

/* Beam search over txo_generate's loop -- a BUILD EXTENSION: the reference has no beam search (BASELINE config 5 asks for
 * k = 5), so parity is anchored only at beams = 1 (== greedy).  Score = sum of log_softmax(logits) of the chosen tokens
 * (not length-normalised); a beam that has emitted eos is finished and continues with eos at no cost; the loop stops when
 * every beam of every image is finished.  Needs cfg.max_batch >= B * beams, beams <= 8.  tokens_out [B, max_len] receives
 * the best beam per image; scores_out [B, beams] (may be NULL) the final scores, best first; all_tokens_out
 * [B * beams, max_len] (may be NULL) every beam. */
int txo_generate_beam(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t H, int32_t W, int32_t beams,
                      int32_t max_len, int32_t eos, int64_t* tokens_out_dev, float* scores_out_dev,
                      int64_t* all_tokens_out_dev, int32_t* n_steps_out, void* stream);

/* What txo_beam_search / txo_beam_search_ragged return (a BUILD EXTENSION like txo_generate_beam): every beam of every image with its
 * score, its length and the log-probability of each of its tokens.  Device pointers; rows are (image, rank): row b * beams + i is the
 * i-th best beam of image b.
 *   tokens  int64 [B * beams][max_len], never NULL.  Columns 0 .. *n_steps_out - 1 are written, the rest is left as it was.
 *   scores  float [B * beams] or NULL: the sum of the beam's log-probabilities, the value txo_generate_beam reports.
 *   logp    float [B * beams][max_len] or NULL: logp[r][t] = log_softmax(logits)[tokens[r][t]] at the beam's own prefix -- the very float
 *           the search added to the beam's score at position t, so the floats of a row summed left to right give scores[r] bit for bit.
 *   lengths int32 [B * beams] or NULL: index of the beam's first eos + 1, or *n_steps_out if it has none (or eos < 0).
 *           Behind a beam's length tokens hold eos and logp holds exactly 0.0f.
 *   length_alpha  0: beams are ordered by score (txo_generate_beam's order).  > 0: the k beams of an image are ordered by
 *           score / length^alpha, descending, ties in the search's order.  Only this final order: the search itself ranks by the
 *           unnormalised score, so the SET of beams does not depend on length_alpha.  Negative or non-finite: TXO_E_INVALID. */
typedef struct {
    int64_t* tokens;
    float*   scores;
    float*   logp;
    int32_t* lengths;
    float    length_alpha;
} txo_beam_out;

/* txo_generate_beam's search (same loop, same bits for tokens and scores) with the outputs of txo_beam_out.  Refused with TXO_E_INVALID
 * before anything is decoded: beams outside [1, 8], B * beams beyond cfg.max_batch or 32767, max_len outside [1, cfg.max_len], a
 * positional table beyond 1024, out or out->tokens NULL, a bad length_alpha.  Leaves a session of one row per image, as txo_generate_beam. */
int txo_beam_search(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t H, int32_t W, int32_t beams, int32_t max_len,
                    int32_t eos, const txo_beam_out* out, int32_t* n_steps_out, void* stream);

/* txo_beam_search over a ragged batch (below: txo_encode_ragged's container and sizes): one encode and one decode for B images of
 * different sizes; the beams of image b are what txo_beam_search gives that image on its own, over the batch's *n_steps_out (behind
 * the image's own step count its rows hold eos and 0.0f).  Every refusal of txo_beam_search and of a ragged batch (TXO_LATENT=1, the
 * hybrid front end without txo_set_ragged_hybrid); runs in the K/V form; no session is open behind it. */
int txo_beam_search_ragged(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t Hc, int32_t Wc, const int32_t* sizes_host,
                           int32_t beams, int32_t max_len, int32_t eos, const txo_beam_out* out, int32_t* n_steps_out, void* stream);

/* ---- Ragged batches (a BUILD EXTENSION: the reference's callables take one (H, W) per batch) ------------------------------------
 * B images of DIFFERENT sizes in one call.  The container img_dev is float32 [B][C][Hc][Wc]; image b sits in the top-left
 * H_b x W_b corner of its slot, every side a positive multiple of 16, H_b <= min(Hc, canvas_h), W_b <= min(Wc, canvas_w).  Pixels
 * outside that corner are NEVER READ (they may hold anything, NaN included).  Image b has n_b = 1 + (H_b/16)(W_b/16) encoder tokens;
 * the slot stride is Ns = max_b n_b (<= max_tokens).  Everything returned for image b is what the fixed-shape call returns for image b
 * passed on its own: its n_b encoder rows (position ids grid[:h_b, :w_b] of the canvas grid, encoder.py:136-143), its logits, its
 * tokens.  Nothing in a padding row or a padding pixel reaches a valid row.  Sizes are HOST arrays (launch geometry depends on them);
 * the engine copies them into its own device buffer (allocated at creation: no call allocates).
 * The multi-position forward has a ragged form, switched on by txo_set_ragged_forward(e, 1): txo_decode_prefill, txo_decode_attn,
 * txo_decode_score and txo_decode_set_key_mask then work on a session opened by txo_decode_begin_ragged (the cross attention of image b
 * sees its own n_b keys in panels Ns rows apart; N = Ns in every layout those calls document), and the ragged generate calls slide the
 * window beyond cfg.max_len like the fixed-shape ones.  txo_score_ragged (txo_score over a container) needs no switch.  Rows n_b..Ns-1 of
 * a slot are never read by any of them: they may hold anything.  With the switch off -- the default, and the behaviour of every engine
 * before the switch existed -- those session calls, txo_score while a ragged session is open, and max_len > cfg.max_len are refused with
 * TXO_E_INVALID and a message naming ragged batches, so a caller that relied on the refusal still gets it.
 * The hybrid ResNetV2 front end takes ragged batches only under txo_set_ragged_hybrid(e, 1) (below); off, the default, every ragged call on
 * such an engine is refused with TXO_E_INVALID and a message naming ragged batches and the hybrid front end, as before that switch existed.
 * Out of scope in every setting, refused with TXO_E_INVALID and a message naming ragged batches: the latent cross-attention form forced by
 * TXO_LATENT=1.  Beam search and logits_out have no ragged entry point (the beam call takes one (H, W) and opens its own
 * session).  The container's width Wc must be a multiple of 4 (rows are read in 16-byte pieces).  The persistent launch is not taken: a
 * ragged generate runs one launch per stage (TXO_Q_LAST_PERSISTENT reads 0), and its session is closed when it returns.
 *
 * Encode: sizes_host int32 [B][2] = (H_b, W_b).  enc_out_dev float [B][Ns][D]: rows n_b..Ns-1 of slot b are written as zeros.
 * *n_slot_out (HOST, may be NULL) receives Ns.  Asynchronous on `stream`. */
int txo_encode_ragged(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t Hc, int32_t Wc, const int32_t* sizes_host,
                      float* enc_out_dev, int32_t* n_slot_out, void* stream);

/* Open a decode session over a ragged encoder output enc_dev [B][Ns][D]: n_tokens_host int32 [B], 1 <= n_b <= Ns, the rows of slot b
 * the cross attention may see.  txo_decode_step (its logits included) then works as on a fixed-shape session.  Under
 * txo_set_ragged_forward(e, 1) so does every other session call, each row as if its image had been begun alone: txo_decode_prefill,
 * txo_decode_score, txo_decode_set_key_mask (it masks decoder positions, which the image sizes do not touch; txo_decode_step honours it
 * on a ragged session too) and txo_decode_attn -- with N = Ns: cross_attn_out [Ld][B][heads][t][Ns],
 * cross_mean_out [Ld][B][t][Ns], columns n_b..Ns-1 of every row written as exactly 0 (the buffers may be uninitialised); self-attention
 * maps as on a fixed-shape session.  txo_decode_step(e, tok, t, ...) continues behind the multi-position calls. */
int txo_decode_begin_ragged(txo_engine* e, const float* enc_dev, int32_t B, int32_t Ns, const int32_t* n_tokens_host, void* stream);

/* The loop of the fixed-shape generate call over a ragged batch: same eos rules (global break by default, TXO_STOP_ROW as set by
 * txo_set_stop_mode), same token selection (txo_set_sampling; a draw is keyed by the row of the batch).  tokens_out_dev [B, max_len]
 * int64, *n_steps_out (HOST) the valid columns; max_len >= 1.  Under txo_set_ragged_forward(e, 1) max_len may exceed cfg.max_len (refused
 * otherwise): the window slides as in txo_generate (one ragged multi-position forward per further token), under the same two preconditions -- a vocabulary that is a multiple of 8 and
 * cfg.max_len <= max_batch * max_tokens -- checked before anything is decoded (TXO_E_INVALID, tokens_out_dev untouched).  Synchronises
 * the stream before returning. */
int txo_generate_ragged(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t Hc, int32_t Wc, const int32_t* sizes_host,
                        int32_t max_len, int32_t eos, int64_t* tokens_out_dev, int32_t* n_steps_out, void* stream);

/* txo_generate_ragged with the per-token log-probabilities of txo_generate_logp: logp_out_dev float [B, max_len], must not be NULL. */
int txo_generate_ragged_logp(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t Hc, int32_t Wc, const int32_t* sizes_host,
                             int32_t max_len, int32_t eos, int64_t* tokens_out_dev, int32_t* n_steps_out, float* logp_out_dev, void* stream);

/* txo_score over a ragged container: txo_encode_ragged + txo_decode_begin_ragged + txo_decode_set_key_mask(mask_dev, L) + txo_decode_score.
 * img_dev / sizes_host as in txo_encode_ragged; tokens_dev int64 [B][L], mask_dev uint8 [B][L] or NULL, the three outputs [B][L-1], each
 * may be NULL, all as in txo_score.  Row b is what txo_score returns for image b passed on its own with tokens_dev[b] / mask_dev[b].  The key
 * mask is cleared again before the call returns; the (ragged) session stays open: txo_decode_step(e, tok, L-1, ...) continues behind it.
 * Works with txo_set_ragged_forward on or off (the call is new with the ragged forward: nothing relied on its refusal). */
int txo_score_ragged(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t Hc, int32_t Wc, const int32_t* sizes_host,
                     const int64_t* tokens_dev, const uint8_t* mask_dev, int32_t L, float* logp_out_dev, int64_t* top1_out_dev,
                     float* top1_logp_out_dev, void* stream);

/* The ragged form of the multi-position forward, for the following calls on this engine.  on = 0 (default): txo_decode_prefill,
 * txo_decode_attn, txo_decode_score and txo_decode_set_key_mask on a session opened by txo_decode_begin_ragged, txo_score while such a
 * session is open, and txo_generate_ragged[_logp] with max_len > cfg.max_len answer TXO_E_INVALID with a message naming ragged batches,
 * as they did before that form existed.  on = 1: they are accepted (see "Ragged batches" above).  Nothing else depends on it; fixed-shape
 * sessions are not affected. */
int txo_set_ragged_forward(txo_engine* e, int32_t on);

/* Ragged batches on the hybrid ResNetV2 front end (cfg.embed = TXO_EMBED_HYBRID), for the following calls on this engine.  on = 0
 * (default): every ragged call answers TXO_E_INVALID ("ragged batches: the hybrid front end is not supported ..."), as it did before the
 * backbone had a ragged form.  on = 1: txo_encode_ragged, txo_decode_begin_ragged, txo_generate_ragged[_logp] and txo_score_ragged are
 * accepted and keep every promise of "Ragged batches" above: the backbone runs over the smallest box that holds every image of the batch
 * with each convolution, pool and GroupNorm bounded by the image's OWN extent, so padding to a common size never enters a statistic.  That
 * box's patch count must not exceed max_tokens - 1 (only a cfg.max_tokens below the canvas's can make it).  Any other value of `on`:
 * TXO_E_INVALID.  Engines with the patch front end accept the call and are not affected. */
int txo_set_ragged_hybrid(txo_engine* e, int32_t on);

/* ---- Device-side image ingest (a BUILD EXTENSION: the reference prepares every image on the host, data_wrangling/dataset.py:365-371) ----
 * The raw uint8 pixels of B images of DIFFERENT sizes and channel counts -> the float32 container [B][C][Hc][Wc] and the sizes [B][2]
 * every ragged call above takes, in ONE launch (texocr_amd/csrc/ingest.h).  What comes out is bit for bit what the host path makes of the
 * same pixels: ToTensor -> Grayscale -> Invert, i.e. a_c = c / 255.0f (an IEEE division), s = (0.2989f a_r + 0.587f a_g) + 0.114f a_b,
 * out = 1.0f - s, every step rounded to float32 on its own.
 *   pix_dev       one DEVICE byte buffer that holds every image: interleaved channels, rows tightly packed (no row padding).
 *   offsets_host  int64 [B] on the HOST: the byte offset of image b's first pixel in pix_dev, >= 0, any alignment.  Image b occupies
 *                 h_b * w_b * ch_b bytes from there; the caller guarantees that they lie inside the buffer.  No byte outside them is read.
 *   shapes_host   int32 [B][3] on the HOST = (h_b, w_b, ch_b), h_b, w_b >= 1, ch_b 1 (L: r = g = b), 3 (RGB) or 4 (RGBA: alpha is ignored).
 *   box_out_dev   float [B][C][Hc][Wc], 16-byte aligned.  EVERY element is written: image b in the top-left corner of slot b, the same
 *                 plane C times; the image's own pad up to the next multiple of 16 and the rest of the slot are exactly 0.0f (not the value
 *                 white maps to, 9.9957e-05).  Wc must be a multiple of 4.  C is the consumer's in_channels; it is not checked here.
 *   sizes_out_host int32 [B][2] on the HOST = (h_b, w_b) rounded up to multiples of 16: the sizes_host of the ragged calls.
 * The container must hold every rounded-up image; the smallest that does is (Hc, Wc) = the maxima of the rounded-up heights and widths, which
 * txo_ingest_box returns (no engine needed).  Refused with TXO_E_INVALID and a message naming the image, before anything is enqueued and --
 * the list and the container are checked first -- before the engine or the device is looked at: null arguments, B < 1, ch outside
 * {1, 3, 4}, h or w < 1, a negative offset, a rounded-up size beyond (Hc, Wc), Wc % 4, an unaligned container; B beyond cfg.max_batch
 * (the engine's descriptor staging holds that many).  No limit comes from the canvas or max_tokens: the ragged call that takes the container
 * keeps all of its own refusals.  Works before the weights are finalized.  Asynchronous on `stream`; the host arrays are copied before the
 * call returns; no allocation.  Under txo_profile_enable(e, 1) the launch carries events (txo_profile_read kind 4). */
int txo_ingest_box(const int32_t* shapes_host, int32_t B, int32_t* Hc_out, int32_t* Wc_out);
int txo_ingest_u8(txo_engine* e, const uint8_t* pix_dev, const int64_t* offsets_host, const int32_t* shapes_host, int32_t B, int32_t C,
                  int32_t Hc, int32_t Wc, float* box_out_dev, int32_t* sizes_out_host, void* stream);

/* ---- Fit-to-canvas ingest (a BUILD EXTENSION; opt-in: txo_ingest_u8 is unchanged and keeps refusing what does not fit) ----
 * An image with a side beyond the target (Fh, Fw) -- both positive multiples of 16, usually the canvas -- is DOWNSCALED to fit it, aspect
 * ratio kept, on the device in front of the ingest arithmetic (texocr_amd/csrc/ingest_fit.h).  The rule, for an image (h, w), in 64-bit
 * integers:  h <= Fh and w <= Fw: unchanged (never upscaled; it takes txo_ingest_u8's path and bytes);  else if w * Fh <= h * Fw:
 * h' = Fh, w' = max(1, (w * Fh) / h);  else w' = Fw, h' = max(1, (h * Fw) / w).
 * The fitted pixels are bit for bit PIL's Image.resize((w', h'), BILINEAR) applied to the uint8 channels the ingest reads: L as it is, R, G, B
 * of RGB and RGBA (alpha is not read: img.convert('RGB').resize(...), NOT PIL's own RGBA resize, which premultiplies).  That resample is
 * integer arithmetic: two passes (horizontal into a uint8 intermediate, then vertical; a pass whose axis keeps its size is skipped), each
 * out = clamp((2^21 + sum_x K[x] src[xmin + x]) >> 22, 0, 255) over a window and coefficients K[x] = (int)(0.5 + k[x] * 2^22) that
 * txo_ingest_fit_coeffs returns; they come from IEEE double operations rounded one by one (tests/fit_ref.py restates them).  The fitted
 * bytes then go through txo_ingest_u8's arithmetic unchanged.  An axis that would shrink by more than 32 times (in > 32 * out) is refused
 * before anything is enqueued, with a message naming the image: 32 bounds the taps per output pixel (TXO_FIT_TAPS), not the quality.
 *   txo_ingest_fit          fitted_out_host int32 [B][2] = (h', w') by the rule above.  No engine needed.  txo_ingest_box composes with it:
 *                           call it on shapes whose (h, w) are the fitted ones.
 *   txo_ingest_fit_scratch  *bytes_out = the device scratch txo_ingest_u8_fit needs for this list: one uint8 intermediate h x w' x (1 or 3),
 *                           rounded up to 16 bytes, per image whose width changes; 0 when nothing is oversized.  No engine needed.
 *   txo_ingest_fit_coeffs   one axis with `in` source and `out` target pixels, in <= 32 * out: xmin_out [out], n_out [out] and
 *                           K_out [out][TXO_FIT_TAPS] (zeros behind n).  No engine, no device: the very function the kernels run.
 *   txo_ingest_u8_fit       txo_ingest_u8 with the fit in front: the container holds the FITTED images and sizes_out_host is the fitted sizes
 *                           rounded up to 16, so (Hc, Wc) need only hold those.  scratch_dev / scratch_bytes: at least what
 *                           txo_ingest_fit_scratch returns (may be NULL / 0 when that is 0); it is written by this call and free again when
 *                           the call's work on `stream` is done.  Every refusal of txo_ingest_u8 (on the fitted sizes), as early as there,
 *                           and: Fh or Fw not a positive multiple of 16, a scale above 32, scratch too small or null when needed.  With no
 *                           oversized image the launch, the container and the sizes are txo_ingest_u8's.  Asynchronous; no allocation;
 *                           under txo_profile_enable(e, 1) every launch carries events (txo_profile_read kind 4). */
#define TXO_FIT_TAPS 65
int txo_ingest_fit(const int32_t* shapes_host, int32_t B, int32_t Fh, int32_t Fw, int32_t* fitted_out_host);
int txo_ingest_fit_scratch(const int32_t* shapes_host, int32_t B, int32_t Fh, int32_t Fw, int64_t* bytes_out);
int txo_ingest_fit_coeffs(int32_t in, int32_t out, int32_t* xmin_out, int32_t* n_out, int32_t* K_out);
int txo_ingest_u8_fit(txo_engine* e, const uint8_t* pix_dev, const int64_t* offsets_host, const int32_t* shapes_host, int32_t B, int32_t C,
                      int32_t Fh, int32_t Fw, int32_t Hc, int32_t Wc, float* box_out_dev, int32_t* sizes_out_host, void* scratch_dev,
                      int64_t scratch_bytes, void* stream);

/* ---- Trim-to-ink and region ingest (a BUILD EXTENSION; opt-in: the calls above are unchanged and launch the kernels they always did) ----
 * Ingest of a RECTANGLE of a source image, in front of the fit and the ingest arithmetic above: the rectangle -- the VIEW (y0, x0, h', w'),
 * in source pixels -- takes the place of the image.  The fit rule applies to (h', w'), the pad to 16, the container and sizes_out_host come
 * from the view, and what comes out is bit for bit txo_ingest_u8 / txo_ingest_u8_fit of a tightly packed copy of the view's pixels.  The
 * order is always trim, then fit.  The caller names the views (boxes of a detector on a page that went up ONCE), or the engine finds them:
 * Trim-to-ink (texocr_amd/csrc/ingest_trim.h).  Integer-only, on the bytes the ingest reads -- L as it is; R, G, B of RGB / RGBA; the alpha
 * is never read.  A pixel is INK iff min(read channels) <= level, level in [0, 254] (127: the mid-grey convention).  margin >= 0 pixels are
 * kept around the ink box and clamped to the image (2 keeps an anti-aliased rim lighter than level):
 *   y0 = max(0, ymin_ink - margin), y1 = min(h, ymax_ink + 1 + margin), h' = y1 - y0; the same for x.
 * An image with no ink keeps the whole-image view (0, 0, h, w).  Dark backgrounds and polarity detection are out of scope.
 *   txo_ingest_trim_views  pix_dev / offsets_host / shapes_host / B as for txo_ingest_u8.  ONE launch reads every byte of every image once
 *                          and leaves the ink extents; views_out_host int32 [B][4] = (y0, x0, h', w') by the rule above.  SYNCHRONOUS: it
 *                          copies 16 B bytes back and WAITS on `stream` before it returns -- the container's size and sizes depend on the
 *                          answer.  It is the one synchronisation of the path; every other ingest call stays asynchronous.  No allocation.
 *                          Refused with TXO_E_INVALID before anything is enqueued: every refusal of txo_ingest_u8 about the list and the
 *                          offsets, level outside [0, 254], margin < 0.  Under txo_profile_enable(e, 1) the launch carries events (kind 4).
 *   txo_ingest_u8_view     shapes_host / offsets_host describe the FULL images; views_host int32 [B][4] = (y0, x0, h', w') one view per
 *                          entry.  Several entries may name the same source bytes (the same offset) and their views may overlap.
 *                          Fh = Fw = 0: txo_ingest_u8 on the views; otherwise txo_ingest_u8_fit on them under the target (Fh, Fw).
 *                          txo_ingest_box, txo_ingest_fit and txo_ingest_fit_scratch compose unchanged: call them on shapes whose (h, w)
 *                          are the views' (h', w').  Refused with TXO_E_INVALID and a message naming the image, nothing enqueued: a view
 *                          with h' < 1 or w' < 1 or reaching outside its image, and every refusal of txo_ingest_u8 / txo_ingest_u8_fit,
 *                          judged on the view's size.  Asynchronous; no allocation.  Views that all keep their images' widths run the very
 *                          kernels of the calls above; others run their pitched forms (a source row is the image's width apart). */
int txo_ingest_trim_views(txo_engine* e, const uint8_t* pix_dev, const int64_t* offsets_host, const int32_t* shapes_host, int32_t B, int32_t level,
                          int32_t margin, int32_t* views_out_host, void* stream);
int txo_ingest_u8_view(txo_engine* e, const uint8_t* pix_dev, const int64_t* offsets_host, const int32_t* shapes_host, const int32_t* views_host,
                       int32_t B, int32_t C, int32_t Fh, int32_t Fw, int32_t Hc, int32_t Wc, float* box_out_dev, int32_t* sizes_out_host,
                       void* scratch_dev, int64_t scratch_bytes, void* stream);

/* Token selection for the following decode steps / generate calls.  mode 0 (default): greedy argmax.  mode 1:
 * the reference's sampler (decoder.py:104-108 + utils.topk, utils.py:85-91): keep the `topk` largest logits
 * (the reference uses int((1 - 0.9) * vocab) = 99 for vocab 1000), softmax(logits / temp), one multinomial draw,
 * from a counter-based RNG keyed by (`seed`; row of the batch, position): reproducible, independent of the decode path and of
 * how the engine splits the batch into row ranges; a different stream than torch.multinomial.  The draw, exactly: Philox4x32-10 with
 * counter (row, position, 0, 0) and key (seed low 32 bits, seed high 32 bits); u = ((c0 >> 8) + 0.5f) / 2^24 in float32; the kept
 * set is the `topk` largest logits, ties at the k-th value kept lowest index first ("largest" and "tie" by the order of the float bits:
 * a logit of -0.0 ranks below +0.0 and does not tie with it); the token is the first kept entry, in index
 * order, at which the running sum of exp((logit - max) / temp) reaches u times their total (tests/sampler_ref.py restates it).
 * mode 1 with a vocabulary beyond TXO_Q_SAMPLE_VOCAB_MAX: TXO_E_INVALID. */
int txo_set_sampling(txo_engine* e, int32_t mode, int32_t topk, float temp, uint64_t seed);

/* Where a decode stops -- the eos handling of txo_generate / txo_generate_from_enc (AutoRegressiveDecoder.generate, decoder.py:97-118).
 * TXO_STOP_GLOBAL (default) is the reference: rows keep producing tokens after their eos and the loop breaks only when EVERY row contains
 * eos (decoder.py:115-116).  TXO_STOP_ROW is a BUILD EXTENSION: a row that has produced eos is finished -- every later token
 * of that row in tokens_out is cfg.pad -- and the loop still ends at the position at which the last row produced its eos, so *n_steps_out
 * and every row's tokens up to and including its first eos are exactly TXO_STOP_GLOBAL's.  What changes is the cost: beyond 128 rows (one launch per
 * stage) the live rows of a row range are compacted to its front every few positions and the launches shrink with them.  Rows whose
 * BOS equals eos are finished from the start.  Not combined with logits_out (a finished row's logits are unspecified: no compaction then)
 * and not applied to txo_generate_beam (a finished beam already costs nothing there). */
#define TXO_STOP_GLOBAL 0
#define TXO_STOP_ROW 1
int txo_set_stop_mode(txo_engine* e, int32_t mode);

/* Constrained decode, a BUILD EXTENSION: which tokens the loop of the following txo_generate* calls may pick.  An engine knob like
 * txo_set_sampling; rules_host == NULL switches the rules off (the default).
 * A rule set is a table rules[S][V] of packed int32 on the host -- S states, 1 <= S <= 8; V = cfg.vocab -- and depth_max, 1 .. 255.  An entry packs
 *   bits 0-7 need (unsigned)   bits 8-15 delta (signed)   bits 16-23 next   bit 24 BAN (TXO_RULE_BAN)   bit 25 ONLY_AT_ZERO (TXO_RULE_ONLY_AT_ZERO)
 * Every row of the batch carries a state (s, depth), (0, 0) at the start.  In (s, depth) token v with r = rules[s][v] is ALLOWED iff BAN is not
 * set, depth >= need, depth + delta <= depth_max, and ONLY_AT_ZERO is not set or depth == 0.  Committing a token -- picked or forced by a
 * prefix -- moves the row to (next, clamp(depth + delta, 0, depth_max)).  A disallowed logit counts as -3.4e38f in the selection: greedy takes
 * the arg-max of the masked row (ties to the lowest index), sampling runs txo_set_sampling's rule on the masked row (a masked entry inside the
 * kept set has probability exactly 0 and is never drawn).  A forced prefix token is never masked, but advances the state.  logp_out keeps
 * its meaning: log_softmax of the RAW logits over the whole vocabulary at the committed token, what txo_score reports -- a token the rules
 * forced on a row shows its low probability; logits_out holds the raw logits.
 * Refused with TXO_E_INVALID and a text that names the rule: S or depth_max out of range, V != cfg.vocab, an entry whose next >= S, a state
 * without an always-allowed token (not BAN, not ONLY_AT_ZERO, need == 0, delta <= 0): so no row can ever face an empty allowed set.
 * While rules are set every txo_generate* that decodes from BOS or from a prefix (image, _from_enc, _ragged, _logp, _prefix*) runs its loop
 * with one launch per stage (TXO_Q_LAST_PERSISTENT reads 0) and otherwise as ever: captured steps, row ranges, TXO_STOP_ROW with live-row
 * compaction, ragged batches, the sliding window, logp_out.  txo_generate_beam / txo_beam_search / txo_beam_search_ragged refuse, unless
 * txo_set_rules_beam(e, 1) is in effect (below).
 * txo_decode_step picks without rules.  Closure is NOT guaranteed: a row that runs out of positions may end at depth > 0 --
 * txo_last_rule_state: the (s, depth) of rows 0 .. B-1 behind the last position the last txo_generate* returned for them (under TXO_STOP_ROW:
 * behind a finished row's first eos), int32 [B][2] on the device, ordered on `stream`. */
#define TXO_RULE_BAN (1 << 24)
#define TXO_RULE_ONLY_AT_ZERO (1 << 25)
int txo_set_token_rules(txo_engine* e, const int32_t* rules_host, int32_t S, int32_t V, int32_t depth_max);
int txo_last_rule_state(txo_engine* e, int32_t* state_out_dev, int32_t B, void* stream);

/* Constrained beam search, a BUILD EXTENSION and opt-in: txo_set_rules_beam(e, 1) (default 0; TXO_E_INVALID unless on is 0 or 1).  Off, the
 * three beam entries refuse while token rules are set, word for word as before the search had a constrained form.  On, and with rules set,
 * they run the search with the rules inside the beam selection; on, without rules, they run as ever.
 * Every (image, beam) slot carries a state (s, depth); all k slots of an image start at (0, 0) and only slot 0 is live, as ever.  For a live
 * parent j in (s_j, d_j) the candidate (j, v) is score[j] + (logit[j][v] - lse[j]) iff rules[s_j][v] allows v at d_j, and -inf otherwise --
 * the beam search's own dead marker, not the -3.4e38f of the single-row pick.  lse[j] is the log-sum-exp of the RAW row: nothing is
 * renormalised, a beam's score stays the sum of the raw model's log-probabilities of its tokens and txo_beam_out.logp means what logp_out of a
 * constrained txo_generate_logp means.  A finished parent offers eos at + 0 and nothing else, unmasked, and its state is frozen.  A slot takes
 * its parent's state advanced by its token, (next, clamp(depth + delta, 0, depth_max)): the eos that finishes a beam advances the state once,
 * its later repeats do not.  Ranking, the tie order (lower parent * V + token) and *n_steps_out are the unconstrained search's.
 * Fewer than k allowed candidates is a normal case (a state that allows two tokens, k = 5, position 0): the surplus beams are DEAD -- score
 * -inf, like beams 1 .. k-1 before position 0 --, and a dead beam is outside every guarantee: its tokens and its state are unspecified
 * (tokens inside the vocabulary).  A live beam always has an allowed token (txo_set_token_rules has checked the table).  A dead beam does not
 * keep the search running: it ends when every live beam of every image is finished.
 * Closure is NOT guaranteed: a beam that runs out of positions may end at depth > 0 (its state shows it); with ONLY_AT_ZERO on eos a FINISHED
 * beam is at depth 0 by construction.  Works with out->logp, row ranges, ragged batches and all three entries; txo_beam_out keeps its layout.
 * txo_last_beam_rule_state: the (s, depth) of every beam of the last constrained beam search, int32 [B][beams][2] on the device, ordered on
 * `stream`, in the order of that call's outputs (txo_beam_search*: the final order, length_alpha included; txo_generate_beam: the order of
 * all_tokens_out and scores_out).  Refused with TXO_E_STATE: no token rules are set; no constrained beam search has run since the token rules
 * were set; B / beams are not that search's. */
int txo_set_rules_beam(txo_engine* e, int32_t on);
int txo_last_beam_rule_state(txo_engine* e, int32_t* state_out_dev, int32_t B, int32_t beams, void* stream);

/* Closing decode, a BUILD EXTENSION and opt-in: txo_set_rules_close(e, 1) (default 0; TXO_E_INVALID unless on is 0 or 1).  Off, every call
 * does what it did.  On, and with token rules set, a row may only pick a token from which its automaton can still reach eos (cfg.eos) in the
 * positions the call has left, so every constrained row ends at an eos its rules allow -- with ONLY_AT_ZERO on eos: at depth 0, inside max_len.
 * The rule.  dist[s][d], s < S, 0 <= d <= depth_max, is the least number of picks, the eos included, that takes a row from (s, d) to a
 * committed eos when every pick is allowed by the rule set and every move is its own (next, clamp(d + delta, 0, depth_max));
 * TXO_CLOSE_INF: no path.  It is computed on the host whenever rules and switch are both set, in either order.  At a pick, a row in (s, d)
 * that has not yet committed an eos has R picks left in what the call returns, this one included (max_len minus the tokens it has picked;
 * behind a prefix each row counts for itself), and D = dist[s][d].  If D is finite, token v is allowed iff txo_set_token_rules' rule allows it
 * AND (v == eos OR dist[next][depth after v] <= max(R, D) - 1).  The allowed set is never empty.  If D <= R at a row's first pick the row
 * commits an allowed eos within its R picks.  D > R, which only a forced prefix can cause, is the one exception for a row: it takes
 * distance-reducing tokens only and ends open, and txo_last_rule_state shows it.  A row where D is TXO_CLOSE_INF (only a prefix leads there)
 * and a row that has committed its eos (the rest of a TXO_STOP_GLOBAL decode) run the plain rule.  While R - 1 >= the largest finite entry
 * and no entry is TXO_CLOSE_INF, the picks are those of the plain constrained decode, bit for bit.  Everything else keeps its meaning: the
 * masked value, raw logp_out / logits_out, forced tokens (never masked, they advance the state), tie order, the sampler's draws.
 * Beam search (with txo_set_rules_beam): for a live unfinished parent the candidate (j, v) is finite iff the rule above holds with the
 * parent's state and R = max_len - position.  Finished parents and dead slots are untouched.  So every LIVE beam of a closing search is
 * finished; dead beams (score -inf) remain the other exception.
 * Refused with TXO_E_INVALID, behind every other refusal of the entry: by txo_set_rules_close / txo_set_token_rules (nothing changes) when
 * switch and rules would both be set and eos is unreachable from the start state (cfg.eos outside the vocabulary, or dist[0][0] is
 * TXO_CLOSE_INF); by txo_generate* / the beam entries when the call's eos is not cfg.eos, and, from BOS, when dist[0][0] exceeds max_len (the
 * text gives both numbers).
 * txo_rules_close_dist: the table the engine computed, int32 [S][D] on the HOST, D = depth_max + 1.  TXO_E_STATE unless rules and switch are
 * both set; TXO_E_INVALID unless S and D are the installed rules'. */
#define TXO_CLOSE_INF 0x7fffffff
int txo_set_rules_close(txo_engine* e, int32_t on);
int txo_rules_close_dist(txo_engine* e, int32_t* out_host, int32_t S, int32_t D);

/* Repeat guard, a BUILD EXTENSION: stops a row of the following txo_generate* calls from looping on a short block of tokens.  An engine
 * knob like txo_set_token_rules; (0, 0) switches it off (the default).  Two integers: max_period P, 1 <= P <= 16, and max_repeats R,
 * 1 <= R <= 16.
 * A row's HISTORY at a pick is h[0 .. n-1]: every token the row has committed after its start token, in order -- forced prefix tokens first,
 * then the row's own picks.  For a period p in 1 .. P with p <= n, m_p is the number of trailing positions i with i - p >= 0 and
 * h[i] == h[i - p], counted back from n - 1 and stopping at the first mismatch.  Token h[n - p] is BANNED at this pick iff m_p >= R * p - 1:
 * committing it would make the row end in R + 1 consecutive copies of one p-token block.  So a block may stand R times in a row, never R + 1.
 * The eos token (the call's eos) is never banned.  A forced prefix token is never masked.  A banned logit counts as -3.4e38f in the selection,
 * exactly as a rule-disallowed one: greedy takes the arg-max of the masked row (ties to the lowest index), sampling runs txo_set_sampling's
 * rule on the masked row.  logp_out and logits_out stay the RAW row's: nothing is renormalised, a pick the guard forced shows its low
 * probability.  The ban set is computed from the committed tokens at every pick; the engine keeps no per-row counters.
 * With token rules: a token must be rule-allowed AND unbanned.  If no token is both, the ban is dropped for that pick and the rules alone
 * decide.  The automaton advances on the committed token as ever; txo_last_rule_state keeps its meaning.
 * While a guard is set every txo_generate* that decodes from BOS or from a prefix runs its loop with one launch per stage
 * (TXO_Q_LAST_PERSISTENT reads 0, TXO_Q_LAST_GUARDED reads 1) and otherwise as ever: captured steps, row ranges, TXO_STOP_ROW with live-row
 * compaction, ragged batches, the sliding window, logp_out.  txo_decode_step picks without it.
 * Refused with TXO_E_INVALID: max_period or max_repeats out of range; cfg.vocab <= max_period + 1 (the guard may ban max_period tokens at a
 * pick); by txo_generate*, behind every other refusal of the entry, while the closing decode is in effect (token rules and
 * txo_set_rules_close: its guarantee and the guard's ban can conflict), and in sampling mode when vocab * 4 + vocab / 8 bytes exceed the
 * 64 KB of LDS the guarded LDS-form sampler may use; by txo_generate_beam / txo_beam_search / txo_beam_search_ragged while a guard is set,
 * unless txo_set_guard_beam(e, 1) is in effect (below). */
int txo_set_repeat_guard(txo_engine* e, int32_t max_period, int32_t max_repeats);

/* Repeat guard inside beam search, a BUILD EXTENSION and opt-in: txo_set_guard_beam(e, 1) (default 0; TXO_E_INVALID unless on is 0 or 1).  Off,
 * the three beam entries refuse while a guard is set, as above and in the same words.  On, they run the guarded selection
 * (texocr_amd/csrc/beam_guard.h) and TXO_Q_LAST_GUARDED reads 1 behind them (0 behind a beam entry without a guard).
 * Slot j of an image at position t has the history h[0 .. t-1] of the tokens its ancestry committed, and its ban set is the rule above on
 * that history.  For a live, unfinished parent j the candidate (j, v) is score[j] + (logit[j][v] - lse[j]) iff v is allowed and not
 * banned for j, -INFINITY otherwise.  "Allowed": every token without rules; the rule of txo_set_token_rules under rules (which need
 * txo_set_rules_beam as ever); the budgeted rule under txo_set_rules_close.  THE YIELD RULE: a parent with no token both allowed and unbanned
 * drops its ban at that pick, and the rules, or the budget, decide alone.  The guard therefore only shrinks a non-empty allowed set to a
 * non-empty one: a closing beam search keeps its guarantee (every live beam ends finished and balanced), which is why the guard is accepted
 * there while txo_generate* with a closing decode still refuses it.  eos is never banned; a finished parent offers eos at + 0, unmasked;
 * scores and logp stay sums of the RAW row's log-probabilities; dead slots, tie order and txo_last_beam_rule_state are the constrained
 * search's.  With the guard off, or the switch off, a beam search runs the kernels it ran before.
 * Refused with TXO_E_INVALID, behind every other refusal of the entry: beams * (vocab / 8 + ((max_repeats + 1) * max_period - 1) * 4) bytes
 * beyond the 56 KB of LDS the guarded selection may use (the message names the vocabulary). */
int txo_set_guard_beam(txo_engine* e, int32_t on);

/* Alternatives per token, a BUILD EXTENSION: the k best ids of every logits row a pick is made from, and their log-probabilities.  An engine
 * knob like txo_set_repeat_guard: k = 0 switches them off (the default), 1 <= k <= 8 on; the setting stays until it is changed and binds
 * txo_generate, txo_generate_logp, their _from_enc forms, txo_generate_prefix* and txo_generate_ragged*.
 * For the f32 logits row x[0 .. V-1] of a pick:
 *   ids[0 .. k-1]  the indices of the k largest entries in descending value, the LOWER INDEX FIRST among equals (a stable descending sort),
 *                  so ids[0] is the greedy pick;
 *   logp[j]        x[ids[j]] - logsumexp(x): natural log, temperature 1, the whole vocabulary -- the quantity logp_out reports.
 * Always the RAW row: not the sampler's top-k / temperature distribution, and not masked by token rules, the closing decode or the repeat
 * guard.  Under a sampled, constrained or guarded decode the committed token may therefore be missing from its own alternatives: that is how
 * a caller sees that a rule forced it.  In a greedy decode logp[0] is bit for bit the float logp_out holds, and ids[0] the token.  A
 * non-finite row has unspecified alternatives with ids in [0, V); other rows are untouched.
 * The columns are the tokens' own: column t, or t + 1 - prefix_len[b] in a prompted decode; a forced prefix token has none.  Wherever
 * tokens_out / logp_out hold pad / 0.0 -- behind a row's first eos under TXO_STOP_ROW, in columns a longer-prefix row never reached -- the
 * alternatives hold pad / 0.0.
 * While set, every txo_generate* runs its loop with one launch per stage (TXO_Q_LAST_PERSISTENT reads 0, TXO_Q_LAST_ALTS reads k) with one
 * more kernel in front of the pick (texocr_amd/csrc/step_alts.h), and otherwise as ever: greedy and sampled, captured steps, row ranges,
 * TXO_STOP_ROW with live-row compaction, ragged batches, prefix, rules, closing, guard.  txo_decode_step keeps none.
 * Refused with TXO_E_INVALID: k outside [0, 8] or beyond cfg.vocab; by txo_generate*, behind every other refusal of the entry, max_len beyond
 * cfg.max_len (the sliding window's tail does not run the loop that keeps them); by txo_generate_beam / txo_beam_search /
 * txo_beam_search_ragged while they are set.
 * txo_last_alternatives copies [B][cols][k] int32 ids and float log-probabilities (either may be NULL) of the LAST txo_generate* to device
 * memory, on `stream`: TXO_E_INVALID if that call ran without alternatives or failed, or if B / cols exceed its rows / its *n_steps. */
int txo_set_alternatives(txo_engine* e, int32_t k);
int txo_last_alternatives(txo_engine* e, int32_t* ids_out_dev, float* logp_out_dev, int32_t B, int32_t cols, void* stream);

/* txo_decode_score / txo_score with the k best of every scored row, 1 <= k <= 8 and k <= cfg.vocab (TXO_E_INVALID otherwise; independent of
 * txo_set_alternatives): alt_ids_out_dev int32 [B][L-1][k], alt_logp_out_dev float [B][L-1][k], neither NULL, by the rule above on the row
 * the fused kernel forms -- the logits are still never stored.  alt_ids[..][0] is top1 and alt_logp[..][0] is top1_logp bit for bit; logp_out,
 * top1_out and top1_logp_out are bit for bit what the call without alternatives writes. */
int txo_decode_score_alts(txo_engine* e, const int64_t* tokens_dev, int32_t L, float* logp_out_dev, int64_t* top1_out_dev, float* top1_logp_out_dev,
                          int32_t k, int32_t* alt_ids_out_dev, float* alt_logp_out_dev, void* stream);
int txo_score_alts(txo_engine* e, const float* img_dev, int32_t B, int32_t C, int32_t H, int32_t W, const int64_t* tokens_dev, const uint8_t* mask_dev,
                   int32_t L, float* logp_out_dev, int64_t* top1_out_dev, float* top1_logp_out_dev, int32_t k, int32_t* alt_ids_out_dev,
                   float* alt_logp_out_dev, void* stream);

/* Timing hooks for bench.py: average duration (ms) of the decode-step cross-attention launches and of
 * the encoder launches recorded with HIP events on the stream the kernels run on, since profiling was last
 * enabled (txo_profile_enable(e, 1) also clears the previous samples); *count = number of launches averaged.  kind: 0 = cross-attention decode kernel,
 * 1 = encoder (whole txo_encode), 2 = whole decode step, 4 = the ingest kernel of txo_ingest_u8 and the launches of txo_ingest_u8_fit, txo_ingest_u8_view and txo_ingest_trim_views (events bound to the dispatch).
 * on = 1: everything above (adds marker commands around every encode and step -- use in a separate pass); on = 2: only every
 * fourth cross-attention dispatch carries events (bound to the dispatch, no extra commands; safe inside a timed region; samples are
 * kept for the first 16 generate() calls after enabling); on = 3: the persistent decode launch carries events (kind 3 =
 * its duration; the launch-per-stage path is not instrumented in this mode, and modes 1 / 2 make generate() take that path);
 * on = 0: off. */
int txo_profile_enable(txo_engine* e, int32_t on);
int txo_profile_read(txo_engine* e, int32_t kind, double* avg_ms, int64_t* count);

/* Introspection for tests and bench.py.  what = TXO_Q_LAST_PERSISTENT: 1 if the last txo_generate* ran its decode loop as ONE
 * persistent launch (texocr_amd/csrc/persist.h; greedy decode of the reference widths), 0 if it ran one launch per stage
 * (sampling, beam search, profiling modes, other widths, TXO_PERSIST=0, or after a fallback).  TXO_Q_PERSIST_FALLBACKS: how
 * many persistent launches gave up (placement check / bounded spin) and were redone with launches since the engine was created. */
#define TXO_Q_LAST_PERSISTENT 0
#define TXO_Q_PERSIST_FALLBACKS 1
#define TXO_Q_LAST_ROW_RANGES 2   /* row ranges (streams) the last generate decoded on: 1, or 2 beyond 128 images in bf16 (launch path) */
#define TXO_Q_LAST_LATENT 3       /* 1 if the last generate's cross attention ran in latent form (csrc/lat_attn.h: against the raw encoder rows) */
#define TXO_Q_RELOAD_KNOBS 4      /* not a question: re-read the TXO_* development knobs of generate() from the environment (the engine reads them once,
                                   * at creation; tests flip TXO_PERSIST / TXO_LANES on a live engine).  *out = 0 */
#define TXO_Q_LAST_COMPACTIONS 5   /* live-row compactions of the last txo_generate* (TXO_STOP_ROW on the launch path; 0 otherwise) */
#define TXO_Q_SAMPLE_VOCAB_MAX 6   /* the largest vocabulary txo_set_sampling accepts on this device: beyond 1024 entries the sampler stages a row
                                    * in LDS (vocab * 4 bytes per workgroup) */
#define TXO_Q_LAST_RAGGED 7        /* 1 if the last generate decoded a ragged batch (per-image encoder token counts), 0 otherwise */
#define TXO_Q_LAST_LATENT_SELF 8   /* 1 if the last generate's SELF attention ran in latent form too (TXO_LATENT_SELF=1: the history is z, not k / v);
                                    * 0 where the engine declined it (no latent form, per-row stop, a positional table beyond the beam slot table) */
#define TXO_Q_LAST_GUARDED 9       /* 1 if the last txo_generate* picked under a repeat guard (txo_set_repeat_guard), 0 otherwise; with txo_set_guard_beam on,
                                    * also set by the beam entries: 1 behind a guarded beam search, 0 behind one without a guard */
#define TXO_Q_LAST_ALTS 10         /* the k of the last txo_generate* (txo_set_alternatives), 0 where it kept no alternatives */
int txo_engine_query(txo_engine* e, int32_t what, int64_t* out);

const char* txo_last_error(void);
const char* txo_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TEXOCR_H */
