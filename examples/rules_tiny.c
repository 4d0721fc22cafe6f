/* Torch-free host program on the C ABI (include/texocr.h), constrained decode: builds an engine from the flat file written by
 * examples/make_tiny_blob.py, decodes once freely, then installs a ONE-STATE RULE SET THAT BANS every token the free run produced
 * (txo_set_token_rules) and decodes again: no banned token may appear, every row's rule state must read (0, 0) (txo_last_rule_state), and
 * with the rules switched off the first tokens come back.  Plain C + the HIP runtime API for device memory; no Python, no torch.
 *
 * Build (what __graft_entry__.build() does):
 *   gcc -std=c99 -Iinclude examples/rules_tiny.c -Ltexocr_amd -ltexocr_hip -lamdhip64 -Wl,-rpath,$PWD/texocr_amd -o examples/rules_tiny
 * Run:   python examples/make_tiny_blob.py /tmp/tiny.bin && examples/rules_tiny /tmp/tiny.bin
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "texocr.h"

static void die(const char* what) { fprintf(stderr, "rules_tiny: %s (%s)\n", what, txo_last_error()); exit(2); }
static void rd(void* p, size_t n, FILE* f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "rules_tiny: short read\n"); exit(2); } }

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

    float* d_img = NULL; int64_t* d_tok = NULL; int32_t* d_state = NULL;
    if (hipMalloc((void**)&d_img, npix * 4) != hipSuccess || hipMalloc((void**)&d_tok, (size_t)B * max_len * 8) != hipSuccess ||
        hipMalloc((void**)&d_state, (size_t)B * 2 * 4) != hipSuccess) die("hipMalloc");
    if (hipMemcpy(d_img, img, npix * 4, hipMemcpyHostToDevice) != hipSuccess) die("hipMemcpy");
    const size_t nt8 = (size_t)B * max_len * 8;
    int64_t* free_run = (int64_t*)malloc(nt8);
    int64_t* got = (int64_t*)malloc(nt8);
    int32_t n_free = 0, n_ruled = 0, n_again = 0;
    if (txo_generate(e, d_img, B, dims[1], dims[2], dims[3], max_len, -1, d_tok, &n_free, NULL, NULL)) die("txo_generate");
    if (hipMemcpy(free_run, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
    (void)want; (void)want_steps;

    /* the ban rule: one state, every entry 0 (need 0, delta 0, next 0: always allowed) but TXO_RULE_BAN where the free run picked the token */
    const int V = cfg.vocab;
    int32_t* rules = (int32_t*)calloc((size_t)V, 4);
    int banned = 0;
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < n_free; ++t) {
            int32_t* r = &rules[free_run[(size_t)b * max_len + t]];
            if (!*r) { *r = TXO_RULE_BAN; ++banned; }
        }
    if (txo_set_token_rules(e, rules, 1, V, 1)) die("txo_set_token_rules");
    if (txo_generate(e, d_img, B, dims[1], dims[2], dims[3], max_len, -1, d_tok, &n_ruled, NULL, NULL)) die("txo_generate (rules)");
    if (hipMemcpy(got, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
    int32_t state[64];
    if (B > 32) { fprintf(stderr, "rules_tiny: more than 32 images\n"); return 2; }
    if (txo_last_rule_state(e, d_state, B, NULL)) die("txo_last_rule_state");
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(state, d_state, (size_t)B * 8, hipMemcpyDeviceToHost) != hipSuccess) die("state back");
    int bad = n_ruled != n_free;
    for (int b = 0; b < B && !bad; ++b) {
        for (int t = 0; t < n_ruled; ++t)
            if (rules[got[(size_t)b * max_len + t]] & TXO_RULE_BAN) { bad = 1; fprintf(stderr, "row %d step %d: banned token %lld\n", b, t, (long long)got[(size_t)b * max_len + t]); break; }
        if (state[2 * b] != 0 || state[2 * b + 1] != 0) bad = 1;
    }
    printf("%s: %d images, %d steps, %d tokens banned: the constrained run %s\n", txo_version(), B, n_ruled, banned,
           bad ? "BROKE THE RULE" : "produced none of them");
    /* a table the engine refuses says why */
    if (!bad) {
        for (int v = 0; v < V; ++v) rules[v] = TXO_RULE_BAN;
        bad = txo_set_token_rules(e, rules, 1, V, 1) != TXO_E_INVALID;
        printf("all banned: %s\n", bad ? "NOT REFUSED" : txo_last_error());
    }
    /* rules off: the free run again */
    if (!bad) {
        if (txo_set_token_rules(e, NULL, 0, 0, 0)) die("txo_set_token_rules (off)");
        if (txo_generate(e, d_img, B, dims[1], dims[2], dims[3], max_len, -1, d_tok, &n_again, NULL, NULL)) die("txo_generate (off)");
        if (hipMemcpy(got, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
        bad = n_again != n_free;
        for (int b = 0; b < B && !bad; ++b) bad = memcmp(got + (size_t)b * max_len, free_run + (size_t)b * max_len, (size_t)n_free * 8) != 0;
        printf("rules off: tokens %s\n", bad ? "DIFFER from the first run" : "are the first run's");
    }
    txo_engine_destroy(e);
    hipFree(d_img); hipFree(d_tok); hipFree(d_state);
    free(img); free(want); free(got); free(free_run); free(rules);
    return bad;
}
