/* Torch-free host program on the C ABI (include/texocr.h), alternatives per token: builds an engine from the flat file written by
 * examples/make_tiny_blob.py, decodes once with txo_generate_logp, then again under txo_set_alternatives(e, 3) and reads the 3 best ids and
 * log-probabilities behind every token with txo_last_alternatives.  In a greedy decode the first alternative IS the token and its
 * log-probability the token's own, bit for bit; the log-probabilities of a position never increase -- checked here and printed, one line per
 * row ("alts row b: token [id logp ...] ...") --, a k out of range is refused with a text that says why, and with the alternatives off
 * txo_last_alternatives is refused and the first tokens come back.  Plain C + the HIP runtime API for device memory; no Python, no torch.
 *
 * Build (what __graft_entry__.build() does):
 *   gcc -std=c99 -Iinclude examples/alts_tiny.c -Ltexocr_amd -ltexocr_hip -lamdhip64 -Wl,-rpath,$PWD/texocr_amd -o examples/alts_tiny
 * Run:   python examples/make_tiny_blob.py /tmp/tiny.bin && examples/alts_tiny /tmp/tiny.bin
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "texocr.h"

static void die(const char* what) { fprintf(stderr, "alts_tiny: %s (%s)\n", what, txo_last_error()); exit(2); }
static void rd(void* p, size_t n, FILE* f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "alts_tiny: short read\n"); exit(2); } }

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
    enum { K = 3 };
    const size_t nt8 = (size_t)B * max_len * 8, nl4 = (size_t)B * max_len * 4, na4 = (size_t)B * max_len * K * 4;
    float* d_lp = NULL; int32_t* d_ids = NULL; float* d_alp = NULL;
    if (hipMalloc((void**)&d_lp, nl4) != hipSuccess || hipMalloc((void**)&d_ids, na4) != hipSuccess || hipMalloc((void**)&d_alp, na4) != hipSuccess)
        die("hipMalloc");
    int64_t* first = (int64_t*)malloc(nt8);
    int64_t* got = (int64_t*)malloc(nt8);
    float* lp = (float*)malloc(nl4);
    int32_t* ids = (int32_t*)malloc(na4);
    float* alp = (float*)malloc(na4);
    int32_t n_first = 0, n = 0, n_again = 0;
    (void)want; (void)want_steps;
    if (txo_generate_logp(e, d_img, B, dims[1], dims[2], dims[3], max_len, -1, d_tok, &n_first, NULL, d_lp, NULL)) die("txo_generate_logp");
    if (hipMemcpy(first, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");

    if (txo_set_alternatives(e, K)) die("txo_set_alternatives");
    if (txo_generate_logp(e, d_img, B, dims[1], dims[2], dims[3], max_len, -1, d_tok, &n, NULL, d_lp, NULL)) die("txo_generate_logp (alternatives)");
    if (txo_last_alternatives(e, d_ids, d_alp, B, n, NULL)) die("txo_last_alternatives");    /* [B][n][K], rows n * K apart */
    if (hipDeviceSynchronize() != hipSuccess) die("hipDeviceSynchronize");
    if (hipMemcpy(got, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(lp, d_lp, nl4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ids, d_ids, (size_t)B * n * K * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(alp, d_alp, (size_t)B * n * K * 4, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
    int64_t k_last = 0;
    if (txo_engine_query(e, TXO_Q_LAST_ALTS, &k_last)) die("txo_engine_query");
    int bad = n != n_first || k_last != K;
    for (int b = 0; b < B; ++b) {
        printf("alts row %d:", b);
        for (int t = 0; t < n; ++t) {
            const int32_t* id = ids + ((size_t)b * n + t) * K;
            const float* l = alp + ((size_t)b * n + t) * K;
            const long long tok = (long long)got[(size_t)b * max_len + t];
            printf(" %lld [", tok);
            for (int j = 0; j < K; ++j) printf("%s%d %.3f", j ? ", " : "", (int)id[j], l[j]);
            printf("]");
            if (tok != first[(size_t)b * max_len + t] || id[0] != tok || memcmp(&l[0], &lp[(size_t)b * max_len + t], 4) != 0) bad = 1;
            for (int j = 1; j < K; ++j) if (l[j] > l[j - 1] || id[j] == id[j - 1] || id[j] < 0 || id[j] >= cfg.vocab) bad = 1;
        }
        printf("\n");
    }
    printf("%s: %d alternatives per token, %d images, %d steps: the first alternative %s\n", txo_version(), K, B, n,
           bad ? "IS NOT THE TOKEN" : "is the token and its log-probability, bit for bit");
    /* a k the engine refuses says why, and leaves the one that is set */
    if (!bad) {
        bad = txo_set_alternatives(e, 9) != TXO_E_INVALID;
        printf("k = 9: %s\n", bad ? "NOT REFUSED" : txo_last_error());
    }
    /* alternatives off: the first run again, and nothing to read behind it */
    if (!bad) {
        if (txo_set_alternatives(e, 0)) die("txo_set_alternatives (off)");
        if (txo_generate(e, d_img, B, dims[1], dims[2], dims[3], max_len, -1, d_tok, &n_again, NULL, NULL)) die("txo_generate (off)");
        if (hipMemcpy(got, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
        bad = n_again != n_first;
        for (int b = 0; b < B && !bad; ++b) bad = memcmp(got + (size_t)b * max_len, first + (size_t)b * max_len, (size_t)n_first * 8) != 0;
        printf("alternatives off: tokens %s\n", bad ? "DIFFER from the first run" : "are the first run's");
        if (!bad) {
            bad = txo_last_alternatives(e, d_ids, d_alp, B, n_again, NULL) != TXO_E_INVALID;
            printf("txo_last_alternatives behind it: %s\n", bad ? "NOT REFUSED" : txo_last_error());
        }
    }
    txo_engine_destroy(e);
    hipFree(d_img); hipFree(d_tok); hipFree(d_lp); hipFree(d_ids); hipFree(d_alp);
    free(img); free(want); free(got); free(first); free(lp); free(ids); free(alp);
    return bad;
}
