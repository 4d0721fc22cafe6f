/* Torch-free host program on the C ABI (include/texocr.h), closing decode: builds an engine from the flat file written by
 * examples/make_tiny_blob.py, installs a brace-like COUNTER RULE (ids % 5 == 0 open a group, ids % 5 == 1 close one, eos only at depth 0,
 * depth_max 8; txo_set_token_rules) and decodes twice: as a plain constrained decode, whose rows may run out of positions with groups
 * open, and with txo_set_rules_close(e, 1), where every row must hold an eos reached at depth 0 inside max_len.  The distance table the
 * engine computed is read back with txo_rules_close_dist.  Plain C + the HIP runtime API for device memory; no Python, no torch.
 *
 * Build (what __graft_entry__.build() does):
 *   gcc -std=c99 -Iinclude examples/rules_close_tiny.c -Ltexocr_amd -ltexocr_hip -lamdhip64 -Wl,-rpath,$PWD/texocr_amd -o examples/rules_close_tiny
 * Run:   python examples/make_tiny_blob.py /tmp/tiny.bin && examples/rules_close_tiny /tmp/tiny.bin
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "texocr.h"

static void die(const char* what) { fprintf(stderr, "rules_close_tiny: %s (%s)\n", what, txo_last_error()); exit(2); }
static void rd(void* p, size_t n, FILE* f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "rules_close_tiny: short read\n"); exit(2); } }

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
    int64_t* got = (int64_t*)malloc(nt8);
    (void)want; (void)want_steps;

    /* the counter: one state; need / delta in bits 0-7 / 8-15; eos (and only eos) carries TXO_RULE_ONLY_AT_ZERO; <BOS> and <PAD> are banned */
    const int V = cfg.vocab, eos = cfg.eos, DEPTH = 8;
    int32_t* rules = (int32_t*)calloc((size_t)V, 4);
    for (int v = 0; v < V; ++v) {
        if (v == eos) rules[v] = TXO_RULE_ONLY_AT_ZERO;
        else if (v == cfg.bos || v == cfg.pad) rules[v] = TXO_RULE_BAN;
        else if (v % 5 == 0) rules[v] = 1 << 8;                       /* delta + 1 */
        else if (v % 5 == 1) rules[v] = 1 | (0xff << 8);              /* need 1, delta - 1 */
    }
    if (txo_set_token_rules(e, rules, 1, V, DEPTH)) die("txo_set_token_rules");
    int bad = 0;
    for (int pass = 0; pass < 2 && !bad; ++pass) {
        if (txo_set_rules_close(e, pass)) die("txo_set_rules_close");
        int32_t n = 0;
        if (txo_generate(e, d_img, B, dims[1], dims[2], dims[3], max_len, eos, d_tok, &n, NULL, NULL)) die("txo_generate");
        if (hipMemcpy(got, d_tok, nt8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
        int open_rows = 0;
        for (int b = 0; b < B; ++b) {                                 /* the rule once more, by hand: depth in front of the row's first eos */
            int depth = 0, closed = 0;
            for (int t = 0; t < n && !closed; ++t) {
                const int v = (int)got[(size_t)b * max_len + t];
                if (v == eos) { closed = depth == 0; break; }
                if (v % 5 == 0 && v != cfg.bos && v != cfg.pad) depth += depth < DEPTH;
                else if (v % 5 == 1) depth -= 1;
                if (depth < 0) { bad = 1; break; }
            }
            open_rows += !closed;
        }
        if (pass == 0) printf("%s: %d images, %d positions, plain constrained decode: %d of %d rows ended open\n", txo_version(), B, n, open_rows, B);
        else {
            bad = bad || open_rows != 0;
            printf("closing decode, %d positions: %s\n", n, bad ? "A ROW ENDED OPEN" : "every row closed at depth 0 with an eos");
        }
    }
    /* the table the engine computed: d closes and the eos from depth d */
    if (!bad) {
        int32_t dist[9];
        if (txo_rules_close_dist(e, dist, 1, DEPTH + 1)) die("txo_rules_close_dist");
        for (int d = 0; d <= DEPTH; ++d) bad = bad || dist[d] != d + 1;
        printf("distance table: dist[0][d] %s d + 1\n", bad ? "IS NOT" : "=");
    }
    /* a call too short to reach eos from the start is refused with both numbers (here: never, dist[0][0] = 1); switch and rules off again */
    if (txo_set_rules_close(e, 0) || txo_set_token_rules(e, NULL, 0, 0, 0)) die("switching off");
    txo_engine_destroy(e);
    hipFree(d_img); hipFree(d_tok);
    free(img); free(want); free(got); free(rules);
    return bad;
}
