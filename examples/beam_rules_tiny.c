/* Torch-free host program on the C ABI (include/texocr.h), constrained beam search: builds an engine from the flat file written by
 * examples/make_tiny_blob.py, runs a free beam search (txo_beam_search, 3 beams), then installs a ONE-STATE RULE SET THAT BANS every token
 * the free beams produced (txo_set_token_rules).  With txo_set_rules_beam off -- the default -- the search is refused; switched on it runs
 * with the rules inside the beam selection: no live beam may hold a banned token, scores descend, every beam's rule state reads (0, 0)
 * (txo_last_beam_rule_state), and with the rules switched off the first beams come back.  Plain C + the HIP runtime API; no Python, no torch.
 *
 * Build (what __graft_entry__.build() does):
 *   gcc -std=c99 -Iinclude examples/beam_rules_tiny.c -Ltexocr_amd -ltexocr_hip -lamdhip64 -Wl,-rpath,$PWD/texocr_amd -o examples/beam_rules_tiny
 * Run:   python examples/make_tiny_blob.py /tmp/tiny.bin && examples/beam_rules_tiny /tmp/tiny.bin
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "texocr.h"

#define BEAMS 3

static void die(const char* what) { fprintf(stderr, "beam_rules_tiny: %s (%s)\n", what, txo_last_error()); exit(2); }
static void rd(void* p, size_t n, FILE* f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "beam_rules_tiny: short read\n"); exit(2); } }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s BLOB\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    char magic[4];
    rd(magic, 4, f);
    if (memcmp(magic, "TXOB", 4)) { fprintf(stderr, "not a TXOB file\n"); return 2; }
    txo_config cfg;                                      /* 19 int32 fields, written in declaration order */
    rd(&cfg, sizeof cfg, f);
    cfg.max_batch *= BEAMS;                              /* decode rows are (image, beam) slots */
    txo_engine* e = NULL;
    if (txo_engine_create(&cfg, &e)) die("txo_engine_create");
    int32_t nt;
    rd(&nt, 4, f);
    for (int i = 0; i < nt; ++i) {
        int32_t klen, ndim;
        char key[256];
        int64_t shape[4];
        rd(&klen, 4, f);
        if (klen <= 0 || klen >= (int)sizeof key) { fprintf(stderr, "bad key length\n"); return 2; }
        rd(key, (size_t)klen, f); key[klen] = 0;
        rd(&ndim, 4, f);
        if (ndim < 1 || ndim > 4) { fprintf(stderr, "bad rank\n"); return 2; }
        rd(shape, 8 * (size_t)ndim, f);
        size_t n = 1;
        for (int k = 0; k < ndim; ++k) n *= (size_t)shape[k];
        float* w = (float*)malloc(n * 4);
        rd(w, n * 4, f);
        if (txo_engine_set_weight(e, key, w, shape, ndim)) die(key);       /* = load_state_dict, one reference key at a time */
        free(w);
    }
    if (txo_engine_finalize_weights(e)) die("txo_engine_finalize_weights");
    int32_t dims[4], ml[2];
    rd(dims, 16, f);
    const size_t npix = (size_t)dims[0] * dims[1] * dims[2] * dims[3];
    float* img = (float*)malloc(npix * 4);
    rd(img, npix * 4, f);
    rd(ml, 8, f);
    fclose(f);
    const int B = dims[0], max_len = ml[0], rows = B * BEAMS;
    if (rows > 32) { fprintf(stderr, "beam_rules_tiny: more than 32 beams\n"); return 2; }

    float* d_img = NULL; int64_t* d_tok = NULL; float* d_score = NULL; int32_t* d_len = NULL; int32_t* d_state = NULL;
    const size_t nt8 = (size_t)rows * max_len * 8;
    if (hipMalloc((void**)&d_img, npix * 4) != hipSuccess || hipMalloc((void**)&d_tok, nt8) != hipSuccess ||
        hipMalloc((void**)&d_score, (size_t)rows * 4) != hipSuccess || hipMalloc((void**)&d_len, (size_t)rows * 4) != hipSuccess ||
        hipMalloc((void**)&d_state, (size_t)rows * 2 * 4) != hipSuccess) die("hipMalloc");
    if (hipMemcpy(d_img, img, npix * 4, hipMemcpyHostToDevice) != hipSuccess) die("hipMemcpy");
    txo_beam_out out;
    memset(&out, 0, sizeof out);
    out.tokens = d_tok; out.scores = d_score; out.lengths = d_len;         /* logp NULL, length_alpha 0: the search's own order */
    int64_t* free_run = (int64_t*)malloc(nt8);
    int64_t* got = (int64_t*)malloc(nt8);
    float score[32]; int32_t state[64];
    int32_t n_free = 0, n_ruled = 0, n_again = 0;
    if (txo_beam_search(e, d_img, B, dims[1], dims[2], dims[3], BEAMS, max_len, -1, &out, &n_free, NULL)) die("txo_beam_search");
    if (hipMemcpy(free_run, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");

    /* the ban rule: one state, every entry 0 (always allowed) but TXO_RULE_BAN where a free beam holds the token */
    const int V = cfg.vocab;
    int32_t* rules = (int32_t*)calloc((size_t)V, 4);
    int banned = 0;
    for (int r = 0; r < rows; ++r)
        for (int t = 0; t < n_free; ++t) {
            int32_t* q = &rules[free_run[(size_t)r * max_len + t]];
            if (!*q) { *q = TXO_RULE_BAN; ++banned; }
        }
    if (txo_set_token_rules(e, rules, 1, V, 1)) die("txo_set_token_rules");
    /* the switch is off: refused, as before the search had a constrained form */
    int bad = txo_beam_search(e, d_img, B, dims[1], dims[2], dims[3], BEAMS, max_len, -1, &out, &n_ruled, NULL) != TXO_E_INVALID;
    printf("switch off: %s\n", bad ? "NOT REFUSED" : txo_last_error());
    if (!bad) bad = txo_last_beam_rule_state(e, d_state, B, BEAMS, NULL) != TXO_E_STATE;
    if (!bad) {
        if (txo_set_rules_beam(e, 1)) die("txo_set_rules_beam");
        if (txo_beam_search(e, d_img, B, dims[1], dims[2], dims[3], BEAMS, max_len, -1, &out, &n_ruled, NULL)) die("txo_beam_search (rules)");
        if (hipMemcpy(got, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
        if (hipMemcpy(score, d_score, (size_t)rows * 4, hipMemcpyDeviceToHost) != hipSuccess) die("scores back");
        if (txo_last_beam_rule_state(e, d_state, B, BEAMS, NULL)) die("txo_last_beam_rule_state");
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(state, d_state, (size_t)rows * 8, hipMemcpyDeviceToHost) != hipSuccess) die("state back");
        bad = n_ruled != n_free;
        for (int r = 0; r < rows && !bad; ++r) {
            if (!isfinite(score[r])) continue;                             /* a dead beam is outside every guarantee */
            for (int t = 0; t < n_ruled; ++t)
                if (rules[got[(size_t)r * max_len + t]] & TXO_RULE_BAN) { bad = 1; fprintf(stderr, "beam %d step %d: banned token %lld\n", r, t, (long long)got[(size_t)r * max_len + t]); break; }
            if (state[2 * r] != 0 || state[2 * r + 1] != 0) bad = 1;
            if (r % BEAMS && isfinite(score[r - 1]) && score[r] > score[r - 1]) bad = 1;
        }
        printf("%s: %d images x %d beams, %d steps, %d tokens banned: the constrained beams %s\n", txo_version(), B, BEAMS, n_ruled, banned,
               bad ? "BROKE THE RULE" : "hold none of them");
    }
    /* rules off: the free beams again, switch on or off */
    if (!bad) {
        if (txo_set_token_rules(e, NULL, 0, 0, 0)) die("txo_set_token_rules (off)");
        if (txo_beam_search(e, d_img, B, dims[1], dims[2], dims[3], BEAMS, max_len, -1, &out, &n_again, NULL)) die("txo_beam_search (off)");
        if (hipMemcpy(got, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
        bad = n_again != n_free;
        for (int r = 0; r < rows && !bad; ++r) bad = memcmp(got + (size_t)r * max_len, free_run + (size_t)r * max_len, (size_t)n_free * 8) != 0;
        printf("rules off: beams %s\n", bad ? "DIFFER from the first run" : "are the first run's");
    }
    txo_engine_destroy(e);
    hipFree(d_img); hipFree(d_tok); hipFree(d_score); hipFree(d_len); hipFree(d_state);
    free(img); free(got); free(free_run); free(rules);
    return bad;
}
