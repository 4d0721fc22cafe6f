/* Torch-free host program on the C ABI (include/texocr.h), repeat guard: builds an engine from the flat file written by
 * examples/make_tiny_blob.py, decodes once freely, then under txo_set_repeat_guard(e, 1, 1) and (e, 4, 2): no row may end in
 * max_repeats + 1 consecutive copies of a block of at most max_period tokens -- checked here from the definition and printed, one line
 * per row ("guard P R row b: tokens") --, a guard out of range is refused with a text that says why, and with the guard switched off
 * the first tokens come back.  Plain C + the HIP runtime API for device memory; no Python, no torch.
 *
 * Build (what __graft_entry__.build() does):
 *   gcc -std=c99 -Iinclude examples/guard_tiny.c -Ltexocr_amd -ltexocr_hip -lamdhip64 -Wl,-rpath,$PWD/texocr_amd -o examples/guard_tiny
 * Run:   python examples/make_tiny_blob.py /tmp/tiny.bin && examples/guard_tiny /tmp/tiny.bin
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "texocr.h"

static void die(const char* what) { fprintf(stderr, "guard_tiny: %s (%s)\n", what, txo_last_error()); exit(2); }
static void rd(void* p, size_t n, FILE* f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "guard_tiny: short read\n"); exit(2); } }

/* positions of h[0 .. n) whose token the guard (P, R) had banned: token h[i] with h[i] == h[i - p] and m_p >= R * p - 1 trailing matches
 * in front of it, for some period p <= P */
static int violations(const int64_t* h, int n, int P, int R) {
    int bad = 0;
    for (int i = 0; i < n; ++i)
        for (int p = 1; p <= P && p <= i; ++p) {
            int m = 0;
            while (m < R * p - 1 && i - 1 - m - p >= 0 && h[i - 1 - m] == h[i - 1 - m - p]) ++m;
            if (m >= R * p - 1 && h[i] == h[i - p]) { ++bad; break; }
        }
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s BLOB\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    char magic[4];
    rd(magic, 4, f);
    if (memcmp(magic, "TXOB", 4)) { fprintf(stderr, "not a TXOB file\n"); return 2; }
    txo_config cfg;                                      /* 19 int32 fields, written in declaration order */
    rd(&cfg, sizeof cfg, f);
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
    const int B = dims[0], max_len = ml[0], want_steps = ml[1];
    int64_t* want = (int64_t*)malloc((size_t)B * want_steps * 8);
    rd(want, (size_t)B * want_steps * 8, f);
    fclose(f);

    float* d_img = NULL; int64_t* d_tok = NULL;
    if (hipMalloc((void**)&d_img, npix * 4) != hipSuccess || hipMalloc((void**)&d_tok, (size_t)B * max_len * 8) != hipSuccess) die("hipMalloc");
    if (hipMemcpy(d_img, img, npix * 4, hipMemcpyHostToDevice) != hipSuccess) die("hipMemcpy");
    const size_t nt8 = (size_t)B * max_len * 8;
    int64_t* free_run = (int64_t*)malloc(nt8);
    int64_t* got = (int64_t*)malloc(nt8);
    int32_t n_free = 0, n_guard = 0, n_again = 0;
    if (txo_generate(e, d_img, B, dims[1], dims[2], dims[3], max_len, -1, d_tok, &n_free, NULL, NULL)) die("txo_generate");
    if (hipMemcpy(free_run, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
    (void)want; (void)want_steps;

    const int guards[2][2] = {{1, 1}, {4, 2}};
    int bad = 0;
    for (int g = 0; g < 2 && !bad; ++g) {
        const int P = guards[g][0], R = guards[g][1];
        int loops = 0;
        for (int b = 0; b < B; ++b) loops += violations(free_run + (size_t)b * max_len, n_free, P, R);
        if (txo_set_repeat_guard(e, P, R)) die("txo_set_repeat_guard");
        if (txo_generate(e, d_img, B, dims[1], dims[2], dims[3], max_len, -1, d_tok, &n_guard, NULL, NULL)) die("txo_generate (guard)");
        if (hipMemcpy(got, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
        int64_t guarded = 0;
        if (txo_engine_query(e, TXO_Q_LAST_GUARDED, &guarded)) die("txo_engine_query");
        bad = n_guard != n_free || guarded != 1;
        for (int b = 0; b < B; ++b) {
            printf("guard %d %d row %d:", P, R, b);
            for (int t = 0; t < n_guard; ++t) printf(" %lld", (long long)got[(size_t)b * max_len + t]);
            printf("\n");
            if (violations(got + (size_t)b * max_len, n_guard, P, R)) bad = 1;
        }
        printf("%s: guard (%d, %d), %d images, %d steps: the free run completes a banned block %d times, the guarded run %s\n", txo_version(), P, R,
               B, n_guard, loops, bad ? "BROKE THE GUARD" : "never");
    }
    /* a guard the engine refuses says why, and leaves the one that is set */
    if (!bad) {
        bad = txo_set_repeat_guard(e, 17, 1) != TXO_E_INVALID;
        printf("max_period 17: %s\n", bad ? "NOT REFUSED" : txo_last_error());
    }
    /* guard off: the free run again */
    if (!bad) {
        if (txo_set_repeat_guard(e, 0, 0)) die("txo_set_repeat_guard (off)");
        if (txo_generate(e, d_img, B, dims[1], dims[2], dims[3], max_len, -1, d_tok, &n_again, NULL, NULL)) die("txo_generate (off)");
        if (hipMemcpy(got, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
        bad = n_again != n_free;
        for (int b = 0; b < B && !bad; ++b) bad = memcmp(got + (size_t)b * max_len, free_run + (size_t)b * max_len, (size_t)n_free * 8) != 0;
        printf("guard off: tokens %s\n", bad ? "DIFFER from the first run" : "are the first run's");
    }
    txo_engine_destroy(e);
    hipFree(d_img); hipFree(d_tok);
    free(img); free(want); free(got); free(free_run);
    return bad;
}
