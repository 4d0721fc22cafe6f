/* Torch-free host program on the C ABI (include/texocr.h): raw uint8 pixels, one of the images LARGER than the canvas, to tokens.  Builds an
 * engine from the flat file examples/make_tiny_blob.py writes, draws three uint8 images (RGB and L inside the canvas, an RGBA one 2.3 x 2.7
 * times over it) and runs txo_ingest_fit (the rule) + txo_ingest_box (on the fitted shapes) + txo_ingest_fit_scratch + txo_ingest_u8_fit +
 * txo_generate_ragged on the GPU: one copy of the raw bytes, the oversized image downscaled on the device.  It checks itself against the host:
 * the two-pass integer resample over txo_ingest_fit_coeffs' tables (out = clamp((2^21 + sum K[x] src[xmin + x]) >> 22)) followed by
 * examples/ingest_tiny.c's preprocessing must give the container bit for bit, and that container must decode to the same tokens.
 *
 * Build (what __graft_entry__.build() does):
 *   gcc -std=c99 -O2 -Iinclude -I$ROCM/include examples/ingest_fit_tiny.c -Ltexocr_amd -ltexocr_hip -L$ROCM/lib -lamdhip64 -o examples/ingest_fit_tiny
 * Run:   python examples/make_tiny_blob.py /tmp/tiny.bin && examples/ingest_fit_tiny /tmp/tiny.bin
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "texocr.h"

static void die(const char* what) { fprintf(stderr, "ingest_fit_tiny: %s (%s)\n", what, txo_last_error()); exit(2); }
static void rd(void* p, size_t n, FILE* f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "ingest_fit_tiny: short read\n"); exit(2); } }

/* the host path of one pixel; volatile keeps every step a float32 operation of its own whatever the compiler's contraction rules */
static float luma_inv(uint8_t r, uint8_t g, uint8_t b) {
    volatile float ar = (float)r / 255.0f, ag = (float)g / 255.0f, ab = (float)b / 255.0f;
    volatile float pr = 0.2989f * ar, pg = 0.587f * ag, pb = 0.114f * ab;
    volatile float s = pr + pg;
    s = s + pb;
    return 1.0f - s;
}

/* one pass of the resample along the axis of length n_in -> n_out: `lines` lines, consecutive pixels of the axis `step` bytes apart, consecutive
 * lines `line` bytes apart (in src; dst has the same layout with n_out pixels), cc channels */
static void resample(const uint8_t* src, uint8_t* dst, int n_in, int n_out, int lines, size_t step_s, size_t line_s, size_t step_d, size_t line_d, int cc) {
    int32_t* xmin = (int32_t*)malloc(4 * (size_t)n_out);
    int32_t* n = (int32_t*)malloc(4 * (size_t)n_out);
    int32_t* K = (int32_t*)malloc(4 * (size_t)n_out * TXO_FIT_TAPS);
    if (txo_ingest_fit_coeffs(n_in, n_out, xmin, n, K)) die("txo_ingest_fit_coeffs");
    for (int l = 0; l < lines; ++l)
        for (int xx = 0; xx < n_out; ++xx)
            for (int c = 0; c < cc; ++c) {
                int32_t acc = 1 << 21;
                for (int x = 0; x < n[xx]; ++x) acc += K[(size_t)xx * TXO_FIT_TAPS + x] * src[(size_t)l * line_s + (size_t)(xmin[xx] + x) * step_s + c];
                acc >>= 22;
                dst[(size_t)l * line_d + (size_t)xx * step_d + c] = (uint8_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
            }
    free(xmin); free(n); free(K);
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

    /* an odd-sized RGB image and a small L one inside the canvas, an RGBA one well over it; rows tightly packed, offsets of any alignment */
    enum { B = 3 };
    const int C = cfg.in_channels, Fh = cfg.canvas_h, Fw = cfg.canvas_w, max_len = cfg.max_len < 12 ? cfg.max_len : 12;
    int32_t shapes[B][3] = {{Fh - 3, Fw - 7, 3}, {9, 21, 1}, {Fh * 23 / 10 + 1, Fw * 27 / 10 + 3, 4}};
    int64_t offsets[B];
    size_t total = 0;
    for (int b = 0; b < B; ++b) { offsets[b] = (int64_t)total; total += (size_t)shapes[b][0] * shapes[b][1] * shapes[b][2] + 1; /* (+1: odd offsets) */ }
    uint8_t* pix = (uint8_t*)malloc(total);
    uint32_t lcg = 12345u;
    for (size_t i = 0; i < total; ++i) { lcg = lcg * 1664525u + 1013904223u; pix[i] = (uint8_t)(lcg >> 24); }

    int32_t fitted[B][2], fshapes[B][3], Hc = 0, Wc = 0, sizes[B][2];
    int64_t scratch_bytes = 0;
    if (txo_ingest_fit(&shapes[0][0], B, Fh, Fw, &fitted[0][0])) die("txo_ingest_fit");
    for (int b = 0; b < B; ++b) { fshapes[b][0] = fitted[b][0]; fshapes[b][1] = fitted[b][1]; fshapes[b][2] = shapes[b][2]; }
    if (txo_ingest_box(&fshapes[0][0], B, &Hc, &Wc)) die("txo_ingest_box");
    if (txo_ingest_fit_scratch(&shapes[0][0], B, Fh, Fw, &scratch_bytes)) die("txo_ingest_fit_scratch");
    printf("fit to %dx%d: %dx%d -> %dx%d, %dx%d -> %dx%d, %dx%d -> %dx%d\n", Fh, Fw, shapes[0][0], shapes[0][1], fitted[0][0], fitted[0][1], shapes[1][0],
           shapes[1][1], fitted[1][0], fitted[1][1], shapes[2][0], shapes[2][1], fitted[2][0], fitted[2][1]);
    const size_t nbox = (size_t)B * C * Hc * Wc;
    uint8_t *d_pix = NULL, *d_scratch = NULL; float *d_box = NULL, *d_box2 = NULL; int64_t* d_tok = NULL;
    if (hipMalloc((void**)&d_pix, total) != hipSuccess || hipMalloc((void**)&d_box, nbox * 4) != hipSuccess ||
        hipMalloc((void**)&d_box2, nbox * 4) != hipSuccess || hipMalloc((void**)&d_tok, (size_t)B * max_len * 8) != hipSuccess ||
        hipMalloc((void**)&d_scratch, (size_t)scratch_bytes + 16) != hipSuccess) die("hipMalloc");
    if (hipMemcpy(d_pix, pix, total, hipMemcpyHostToDevice) != hipSuccess) die("hipMemcpy");
    if (hipMemset(d_box, 0xff, nbox * 4) != hipSuccess) die("hipMemset");                 /* NaN everywhere: the kernel writes every element */
    if (txo_ingest_u8_fit(e, d_pix, offsets, &shapes[0][0], B, C, Fh, Fw, Hc, Wc, d_box, &sizes[0][0], d_scratch, scratch_bytes, NULL)) die("txo_ingest_u8_fit");
    int32_t n_dev = 0, n_host = 0;
    int64_t* tok_dev = (int64_t*)malloc((size_t)B * max_len * 8);
    int64_t* tok_host = (int64_t*)malloc((size_t)B * max_len * 8);
    if (txo_generate_ragged(e, d_box, B, C, Hc, Wc, &sizes[0][0], max_len, cfg.eos, d_tok, &n_dev, NULL)) die("txo_generate_ragged");
    if (hipMemcpy(tok_dev, d_tok, (size_t)B * max_len * 8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");

    /* the same container made on the host: fit (horizontal pass, then vertical; a pass whose axis keeps its size is skipped), then preprocess */
    float* box = (float*)calloc(nbox, 4);
    float* got = (float*)malloc(nbox * 4);
    int sizes_bad = 0;
    for (int b = 0; b < B; ++b) {
        const int h = shapes[b][0], w = shapes[b][1], ch = shapes[b][2], fh = fitted[b][0], fw = fitted[b][1];
        const uint8_t* p = pix + offsets[b];
        uint8_t *mid = NULL, *fit = NULL;
        size_t px = (size_t)ch;                                  /* bytes per pixel of the image the preprocessing reads */
        const int cc = ch == 1 ? 1 : 3;
        if (fw != w) {
            mid = (uint8_t*)malloc((size_t)h * fw * cc);
            resample(p, mid, w, fw, h, (size_t)ch, (size_t)w * ch, (size_t)cc, (size_t)fw * cc, cc);
            p = mid; px = (size_t)cc;
        }
        if (fh != h) {
            fit = (uint8_t*)malloc((size_t)fh * fw * cc);
            resample(p, fit, h, fh, fw, (size_t)fw * px, px, (size_t)fw * cc, (size_t)cc, cc);
            p = fit; px = (size_t)cc;
        }
        for (int y = 0; y < fh; ++y)
            for (int x = 0; x < fw; ++x) {
                const uint8_t* q = p + ((size_t)y * fw + x) * px;
                const float v = ch == 1 ? luma_inv(q[0], q[0], q[0]) : luma_inv(q[0], q[1], q[2]);
                for (int c = 0; c < C; ++c) box[(((size_t)b * C + c) * Hc + y) * Wc + x] = v;
            }
        sizes_bad |= sizes[b][0] != (fh + 15) / 16 * 16 || sizes[b][1] != (fw + 15) / 16 * 16;
        free(mid); free(fit);
    }
    if (hipMemcpy(got, d_box, nbox * 4, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
    const int box_bad = memcmp(got, box, nbox * 4) != 0 || sizes_bad;
    printf("%s: %d images, %lld bytes of scratch -> container %dx%dx%dx%d: %s\n", txo_version(), B, (long long)scratch_bytes, B, C, Hc, Wc,
           box_bad ? "DIFFERS from the host resample and preprocessing" : "equals the host resample and preprocessing bit for bit");
    if (hipMemcpy(d_box2, box, nbox * 4, hipMemcpyHostToDevice) != hipSuccess) die("hipMemcpy");
    if (txo_generate_ragged(e, d_box2, B, C, Hc, Wc, &sizes[0][0], max_len, cfg.eos, d_tok, &n_host, NULL)) die("txo_generate_ragged (host container)");
    if (hipMemcpy(tok_host, d_tok, (size_t)B * max_len * 8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
    int tok_bad = n_dev != n_host;
    for (int b = 0; b < B && !tok_bad; ++b)
        for (int t = 0; t < n_dev; ++t)
            if (tok_dev[(size_t)b * max_len + t] != tok_host[(size_t)b * max_len + t]) { tok_bad = 1; break; }
    printf("bytes to tokens: %d steps, first tokens %lld %lld %lld: %s\n", n_dev, (long long)tok_dev[0], (long long)tok_dev[max_len],
           (long long)tok_dev[2 * (size_t)max_len], tok_bad ? "DIFFER from the host container's" : "equal the host container's");
    /* a refusal names the image: a strip that would shrink by more than 32 times (nothing is read: the list is refused first) */
    shapes[1][0] = 2; shapes[1][1] = 40 * Fw;
    const int rc = txo_ingest_u8_fit(e, d_pix, offsets, &shapes[0][0], B, C, Fh, Fw, Hc, Wc, d_box, &sizes[0][0], d_scratch, scratch_bytes, NULL);
    printf("2x%d -> %d (%s)\n", 40 * Fw, rc, txo_last_error());
    txo_engine_destroy(e);
    hipFree(d_pix); hipFree(d_box); hipFree(d_box2); hipFree(d_tok); hipFree(d_scratch);
    free(pix); free(box); free(got); free(tok_dev); free(tok_host);
    return box_bad || tok_bad || rc != TXO_E_INVALID;
}
