/* Torch-free host program on the C ABI (include/texocr.h), beam search under the repeat guard: builds an engine from the flat file written
 * by examples/make_tiny_blob.py, runs a free beam search (txo_beam_search, 3 beams) and counts the beams that repeat a token, then sets the
 * repeat guard (1, 1) (txo_set_repeat_guard: no token twice in a row).  With txo_set_guard_beam off -- the default -- the search is refused;
 * switched on it runs with the ban inside the beam selection: no live beam holds the same token twice in a row, scores descend,
 * TXO_Q_LAST_GUARDED reads 1.  With the guard switched off again the first beams come back.  Both sets of beams are printed.
 * Plain C + the HIP runtime API; no Python, no torch.
 *
 * Build (what __graft_entry__.build() does):
 *   gcc -std=c99 -Iinclude examples/beam_guard_tiny.c -Ltexocr_amd -ltexocr_hip -lamdhip64 -Wl,-rpath,$PWD/texocr_amd -o examples/beam_guard_tiny
 * Run:   python examples/make_tiny_blob.py /tmp/tiny.bin && examples/beam_guard_tiny /tmp/tiny.bin
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
#define PERIOD 1
#define REPEATS 1

static void die(const char* what) { fprintf(stderr, "beam_guard_tiny: %s (%s)\n", what, txo_last_error()); exit(2); }
static void rd(void* p, size_t n, FILE* f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "beam_guard_tiny: short read\n"); exit(2); } }

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
    if (rows > 32) { fprintf(stderr, "beam_guard_tiny: more than 32 beams\n"); return 2; }

    float* d_img = NULL; int64_t* d_tok = NULL; float* d_score = NULL; int32_t* d_len = NULL;
    const size_t nt8 = (size_t)rows * max_len * 8;
    if (hipMalloc((void**)&d_img, npix * 4) != hipSuccess || hipMalloc((void**)&d_tok, nt8) != hipSuccess ||
        hipMalloc((void**)&d_score, (size_t)rows * 4) != hipSuccess || hipMalloc((void**)&d_len, (size_t)rows * 4) != hipSuccess) die("hipMalloc");
    if (hipMemcpy(d_img, img, npix * 4, hipMemcpyHostToDevice) != hipSuccess) die("hipMemcpy");
    txo_beam_out out;
    memset(&out, 0, sizeof out);
    out.tokens = d_tok; out.scores = d_score; out.lengths = d_len;         /* logp NULL, length_alpha 0: the search's own order */
    int64_t* free_run = (int64_t*)malloc(nt8);
    int64_t* got = (int64_t*)malloc(nt8);
    float score[32];
    int32_t n_free = 0, n_guard = 0, n_again = 0;
    int64_t guarded = -1;
    if (txo_beam_search(e, d_img, B, dims[1], dims[2], dims[3], BEAMS, max_len, -1, &out, &n_free, NULL)) die("txo_beam_search");
    if (hipMemcpy(free_run, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
    int repeats = 0;
    printf("guard (%d, %d), eos %d\n", PERIOD, REPEATS, -1);
    for (int r = 0; r < rows; ++r) {
        printf("free beam %d %d:", r / BEAMS, r % BEAMS);
        for (int t = 0; t < n_free; ++t) printf(" %lld", (long long)free_run[(size_t)r * max_len + t]);
        printf("\n");
        for (int t = 1; t < n_free; ++t)
            if (free_run[(size_t)r * max_len + t] == free_run[(size_t)r * max_len + t - 1]) { ++repeats; break; }
    }

    if (txo_set_repeat_guard(e, PERIOD, REPEATS)) die("txo_set_repeat_guard");
    /* the switch is off: refused, as before the search had a guarded form */
    int bad = txo_beam_search(e, d_img, B, dims[1], dims[2], dims[3], BEAMS, max_len, -1, &out, &n_guard, NULL) != TXO_E_INVALID;
    printf("switch off: %s\n", bad ? "NOT REFUSED" : txo_last_error());
    if (!bad) {
        if (txo_set_guard_beam(e, 1)) die("txo_set_guard_beam");
        if (txo_beam_search(e, d_img, B, dims[1], dims[2], dims[3], BEAMS, max_len, -1, &out, &n_guard, NULL)) die("txo_beam_search (guard)");
        if (hipMemcpy(got, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
        if (hipMemcpy(score, d_score, (size_t)rows * 4, hipMemcpyDeviceToHost) != hipSuccess) die("scores back");
        if (txo_engine_query(e, TXO_Q_LAST_GUARDED, &guarded)) die("txo_engine_query");
        bad = n_guard != n_free || guarded != 1;
        for (int r = 0; r < rows; ++r) {
            printf("guarded beam %d %d:", r / BEAMS, r % BEAMS);
            for (int t = 0; t < n_guard; ++t) printf(" %lld", (long long)got[(size_t)r * max_len + t]);
            printf("\n");
            if (!isfinite(score[r])) { bad = 1; continue; }                /* (without rules every beam of a vocabulary this size is live) */
            for (int t = 1; t < n_guard; ++t)
                if (got[(size_t)r * max_len + t] == got[(size_t)r * max_len + t - 1]) { bad = 1; fprintf(stderr, "beam %d step %d: token %lld twice\n", r, t, (long long)got[(size_t)r * max_len + t]); break; }
            if (r % BEAMS && score[r] > score[r - 1]) bad = 1;
        }
        printf("%s: %d images x %d beams, %d steps: %d free beams repeat a token, the guarded beams %s\n", txo_version(), B, BEAMS, n_guard, repeats,
               bad ? "BROKE THE GUARD" : "hold no token twice in a row");
    }
    /* guard off: the free beams again, switch on or off */
    if (!bad) {
        if (txo_set_repeat_guard(e, 0, 0)) die("txo_set_repeat_guard (off)");
        if (txo_beam_search(e, d_img, B, dims[1], dims[2], dims[3], BEAMS, max_len, -1, &out, &n_again, NULL)) die("txo_beam_search (off)");
        if (hipMemcpy(got, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
        if (txo_engine_query(e, TXO_Q_LAST_GUARDED, &guarded)) die("txo_engine_query");
        bad = n_again != n_free || guarded != 0;
        for (int r = 0; r < rows && !bad; ++r) bad = memcmp(got + (size_t)r * max_len, free_run + (size_t)r * max_len, (size_t)n_free * 8) != 0;
        printf("guard off: beams %s\n", bad ? "DIFFER from the first run" : "are the first run's");
    }
    txo_engine_destroy(e);
    hipFree(d_img); hipFree(d_tok); hipFree(d_score); hipFree(d_len);
    free(img); free(got); free(free_run);
    return bad;
}
