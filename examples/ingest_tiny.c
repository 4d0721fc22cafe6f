/* Torch-free host program on the C ABI (include/texocr.h): from raw uint8 pixels to tokens.  Builds an engine from the flat file
 * examples/make_tiny_blob.py writes (only its config and weights are used), draws a few uint8 images of different sizes and channel counts
 * (L, RGB, RGBA), and runs txo_ingest_box + txo_ingest_u8 + txo_generate_ragged on the GPU: one copy of the bytes, one launch for the
 * container, one ragged generate.  It checks itself against the host: the same preprocessing in plain C (a_c = c / 255.0f,
 * s = (0.2989f a_r + 0.587f a_g) + 0.114f a_b, out = 1.0f - s, every step rounded on its own; zero pad) must give the container bit for bit,
 * and the container uploaded from the host must decode to the same tokens.  Plain C + the HIP runtime API; no Python, no torch.
 *
 * Build (what __graft_entry__.build() does):
 *   gcc -std=c99 -O2 -Iinclude -I$ROCM/include examples/ingest_tiny.c -Ltexocr_amd -ltexocr_hip -L$ROCM/lib -lamdhip64 -o examples/ingest_tiny
 * Run:   python examples/make_tiny_blob.py /tmp/tiny.bin && examples/ingest_tiny /tmp/tiny.bin
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "texocr.h"

static void die(const char* what) { fprintf(stderr, "ingest_tiny: %s (%s)\n", what, txo_last_error()); exit(2); }
static void rd(void* p, size_t n, FILE* f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "ingest_tiny: short read\n"); exit(2); } }

/* the host path of one pixel; volatile keeps every step a float32 operation of its own whatever the compiler's contraction rules */
static float luma_inv(uint8_t r, uint8_t g, uint8_t b) {
    volatile float ar = (float)r / 255.0f, ag = (float)g / 255.0f, ab = (float)b / 255.0f;
    volatile float pr = 0.2989f * ar, pg = 0.587f * ag, pb = 0.114f * ab;
    volatile float s = pr + pg;
    s = s + pb;
    return 1.0f - s;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s BLOB\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    char magic[4];
    rd(magic, 4, f);
    if (memcmp(magic, "TXOB", 4)) { fprintf(stderr, "not a TXOB file\n"); return 2; }
    txo_config cfg;
    rd(&cfg, sizeof cfg, f);
    if (cfg.max_batch < 3) cfg.max_batch = 3;
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
        if (txo_engine_set_weight(e, key, w, shape, ndim)) die(key);
        free(w);
    }
    fclose(f);
    if (txo_engine_finalize_weights(e)) die("txo_engine_finalize_weights");

    /* three images inside the canvas: an odd-sized RGB one, a small L one, an RGBA one; rows tightly packed, offsets of any alignment */
    enum { B = 3 };
    const int C = cfg.in_channels, max_len = cfg.max_len < 12 ? cfg.max_len : 12;
    int32_t shapes[B][3] = {{cfg.canvas_h - 3, cfg.canvas_w - 7, 3}, {9, 21, 1}, {17, 33, 4}};
    int64_t offsets[B];
    size_t total = 0;
    for (int b = 0; b < B; ++b) { offsets[b] = (int64_t)total; total += (size_t)shapes[b][0] * shapes[b][1] * shapes[b][2] + 1; /* (+1: odd offsets) */ }
    uint8_t* pix = (uint8_t*)malloc(total);
    uint32_t lcg = 12345u;
    for (size_t i = 0; i < total; ++i) { lcg = lcg * 1664525u + 1013904223u; pix[i] = (uint8_t)(lcg >> 24); }

    int32_t Hc = 0, Wc = 0, sizes[B][2];
    if (txo_ingest_box(&shapes[0][0], B, &Hc, &Wc)) die("txo_ingest_box");
    const size_t nbox = (size_t)B * C * Hc * Wc;
    uint8_t* d_pix = NULL; float *d_box = NULL, *d_box2 = NULL; int64_t* d_tok = NULL;
    if (hipMalloc((void**)&d_pix, total) != hipSuccess || hipMalloc((void**)&d_box, nbox * 4) != hipSuccess ||
        hipMalloc((void**)&d_box2, nbox * 4) != hipSuccess || hipMalloc((void**)&d_tok, (size_t)B * max_len * 8) != hipSuccess) die("hipMalloc");
    if (hipMemcpy(d_pix, pix, total, hipMemcpyHostToDevice) != hipSuccess) die("hipMemcpy");
    if (hipMemset(d_box, 0xff, nbox * 4) != hipSuccess) die("hipMemset");                 /* NaN everywhere: the kernel writes every element */
    if (txo_ingest_u8(e, d_pix, offsets, &shapes[0][0], B, C, Hc, Wc, d_box, &sizes[0][0], NULL)) die("txo_ingest_u8");
    int32_t n_dev = 0, n_host = 0;
    int64_t* tok_dev = (int64_t*)malloc((size_t)B * max_len * 8);
    int64_t* tok_host = (int64_t*)malloc((size_t)B * max_len * 8);
    if (txo_generate_ragged(e, d_box, B, C, Hc, Wc, &sizes[0][0], max_len, cfg.eos, d_tok, &n_dev, NULL)) die("txo_generate_ragged");
    if (hipMemcpy(tok_dev, d_tok, (size_t)B * max_len * 8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");

    /* the same container made on the host */
    float* box = (float*)calloc(nbox, 4);
    float* got = (float*)malloc(nbox * 4);
    for (int b = 0; b < B; ++b) {
        const int h = shapes[b][0], w = shapes[b][1], ch = shapes[b][2];
        const uint8_t* p = pix + offsets[b];
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const uint8_t* q = p + ((size_t)y * w + x) * ch;
                const float v = ch == 1 ? luma_inv(q[0], q[0], q[0]) : luma_inv(q[0], q[1], q[2]);
                for (int c = 0; c < C; ++c) box[(((size_t)b * C + c) * Hc + y) * Wc + x] = v;
            }
    }
    if (hipMemcpy(got, d_box, nbox * 4, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
    const int box_bad = memcmp(got, box, nbox * 4) != 0;
    printf("%s: %d images (%dx%dx%d, %dx%dx%d, %dx%dx%d) -> container %dx%dx%dx%d: %s\n", txo_version(), B, shapes[0][0], shapes[0][1], shapes[0][2],
           shapes[1][0], shapes[1][1], shapes[1][2], shapes[2][0], shapes[2][1], shapes[2][2], B, C, Hc, Wc,
           box_bad ? "DIFFERS from the host preprocessing" : "equals the host preprocessing bit for bit");
    if (hipMemcpy(d_box2, box, nbox * 4, hipMemcpyHostToDevice) != hipSuccess) die("hipMemcpy");
    if (txo_generate_ragged(e, d_box2, B, C, Hc, Wc, &sizes[0][0], max_len, cfg.eos, d_tok, &n_host, NULL)) die("txo_generate_ragged (host container)");
    if (hipMemcpy(tok_host, d_tok, (size_t)B * max_len * 8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
    int tok_bad = n_dev != n_host;
    for (int b = 0; b < B && !tok_bad; ++b)
        for (int t = 0; t < n_dev; ++t)
            if (tok_dev[(size_t)b * max_len + t] != tok_host[(size_t)b * max_len + t]) { tok_bad = 1; break; }
    printf("bytes to tokens: %d steps, first tokens %lld %lld %lld: %s\n", n_dev, (long long)tok_dev[0], (long long)tok_dev[max_len],
           (long long)tok_dev[2 * (size_t)max_len], tok_bad ? "DIFFER from the host container's" : "equal the host container's");
    /* a refusal names the image */
    shapes[1][2] = 2;
    const int rc = txo_ingest_u8(e, d_pix, offsets, &shapes[0][0], B, C, Hc, Wc, d_box, &sizes[0][0], NULL);
    printf("ch = 2 -> %d (%s)\n", rc, txo_last_error());
    txo_engine_destroy(e);
    hipFree(d_pix); hipFree(d_box); hipFree(d_box2); hipFree(d_tok);
    free(pix); free(box); free(got); free(tok_dev); free(tok_host);
    return box_bad || tok_bad || rc != TXO_E_INVALID;
}
