/* Torch-free host program on the C ABI (include/texocr.h): raw uint8 pixels with white margins, one of the images LARGER than the canvas, to
 * tokens -- each image cut to its ink on the device first.  Builds an engine from the flat file examples/make_tiny_blob.py writes, draws
 * three uint8 images (an RGB and an RGBA formula-like blob on white, the RGBA one beyond the canvas with ink that fits it, and a blank L one)
 * and runs txo_ingest_trim_views (the one synchronous call) + txo_ingest_box (on the views' shapes) + txo_ingest_u8_view +
 * txo_generate_ragged on the GPU: one copy of the raw bytes, no fit.  Then the same page again through two OVERLAPPING caller-named regions
 * that share its bytes.  It checks itself against the host: the rule in plain C (ink iff min(read channels) <= level, the margin, the clamp)
 * must give the views, and examples/ingest_tiny.c's preprocessing of the views' pixels must give both containers bit for bit.
 * With a second argument it also writes what it fed and what it got to that file, for a caller that wants to compare (tests do):
 *   int32 B, C, Hc, Wc; int32 shapes[B][3]; int32 views[B][4]; int32 sizes[B][2]; int64 offsets[B]; int64 total; uint8 pix[total];
 *   float box[B][C][Hc][Wc].
 *
 * Build (what __graft_entry__.build() does):
 *   gcc -std=c99 -O2 -Iinclude -I$ROCM/include examples/ingest_trim_tiny.c -Ltexocr_amd -ltexocr_hip -L$ROCM/lib -lamdhip64 -o examples/ingest_trim_tiny
 * Run:   python examples/make_tiny_blob.py /tmp/tiny.bin && examples/ingest_trim_tiny /tmp/tiny.bin
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "texocr.h"

static void die(const char* what) { fprintf(stderr, "ingest_trim_tiny: %s (%s)\n", what, txo_last_error()); exit(2); }
static void rd(void* p, size_t n, FILE* f) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "ingest_trim_tiny: short read\n"); exit(2); } }

/* the host path of one pixel; volatile keeps every step a float32 operation of its own whatever the compiler's contraction rules */
static float luma_inv(uint8_t r, uint8_t g, uint8_t b) {
    volatile float ar = (float)r / 255.0f, ag = (float)g / 255.0f, ab = (float)b / 255.0f;
    volatile float pr = 0.2989f * ar, pg = 0.587f * ag, pb = 0.114f * ab;
    volatile float s = pr + pg;
    s = s + pb;
    return 1.0f - s;
}

/* the trim rule on the host: image p (h, w, ch) -> view (y0, x0, h', w') */
static void trim_view(const uint8_t* p, int h, int w, int ch, int level, int margin, int32_t* v) {
    int ymin = h, xmin = w, ymax = -1, xmax = -1;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint8_t* q = p + ((size_t)y * w + x) * ch;
            int m = q[0];
            if (ch > 1) { if (q[1] < m) m = q[1]; if (q[2] < m) m = q[2]; }   /* (the alpha is not read) */
            if (m <= level) { if (y < ymin) ymin = y; if (y > ymax) ymax = y; if (x < xmin) xmin = x; if (x > xmax) xmax = x; }
        }
    if (ymax < 0) { v[0] = 0; v[1] = 0; v[2] = h; v[3] = w; return; }
    const int y0 = ymin - margin < 0 ? 0 : ymin - margin, y1 = ymax + 1 + margin > h ? h : ymax + 1 + margin;
    const int x0 = xmin - margin < 0 ? 0 : xmin - margin, x1 = xmax + 1 + margin > w ? w : xmax + 1 + margin;
    v[0] = y0; v[1] = x0; v[2] = y1 - y0; v[3] = x1 - x0;
}

/* the container the host path makes of the views: box [B][C][Hc][Wc], zero outside every view */
static void host_box(float* box, const uint8_t* pix, const int64_t* offsets, int32_t (*shapes)[3], int32_t (*views)[4], int B, int C, int Hc, int Wc) {
    memset(box, 0, (size_t)B * C * Hc * Wc * 4);
    for (int b = 0; b < B; ++b) {
        const int w = shapes[b][1], ch = shapes[b][2];
        for (int y = 0; y < views[b][2]; ++y)
            for (int x = 0; x < views[b][3]; ++x) {
                const uint8_t* q = pix + offsets[b] + ((size_t)(views[b][0] + y) * w + views[b][1] + x) * ch;
                const float v = ch == 1 ? luma_inv(q[0], q[0], q[0]) : luma_inv(q[0], q[1], q[2]);
                for (int c = 0; c < C; ++c) box[(((size_t)b * C + c) * Hc + y) * Wc + x] = v;
            }
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s BLOB [DUMP]\n", argv[0]); return 2; }
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

    /* white images with a dark, noisy blob well inside: RGB within the canvas, RGBA at 2.5 x 2.2 times the canvas whose blob fits it, and a
     * blank L one; rows tightly packed, offsets of any alignment */
    enum { B = 3 };
    const int C = cfg.in_channels, Ch = cfg.canvas_h, Cw = cfg.canvas_w, max_len = cfg.max_len < 12 ? cfg.max_len : 12, level = 127, margin = 2;
    int32_t shapes[B][3] = {{Ch - 3, Cw - 7, 3}, {Ch * 5 / 2 + 1, Cw * 22 / 10 + 3, 4}, {9, 21, 1}};
    const int ink[B][4] = {{Ch / 4, Cw / 5, Ch / 2, Cw / 2}, {Ch, Cw / 2 + 5, Ch / 2 + 3, Cw * 3 / 4}, {0, 0, 0, 0}};   /* y, x, h, w of each blob */
    int64_t offsets[B];
    size_t total = 0;
    for (int b = 0; b < B; ++b) { offsets[b] = (int64_t)total; total += (size_t)shapes[b][0] * shapes[b][1] * shapes[b][2] + 1; /* (+1: odd offsets) */ }
    uint8_t* pix = (uint8_t*)malloc(total);
    memset(pix, 255, total);
    uint32_t lcg = 12345u;
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < ink[b][2]; ++y)
            for (int x = 0; x < ink[b][3]; ++x)
                for (int c = 0; c < 3 && c < shapes[b][2]; ++c) {
                    lcg = lcg * 1664525u + 1013904223u;
                    const int edge = y == 0 || x == 0 || y == ink[b][2] - 1 || x == ink[b][3] - 1;
                    pix[offsets[b] + ((size_t)(ink[b][0] + y) * shapes[b][1] + ink[b][1] + x) * shapes[b][2] + c] = edge ? 0 : (uint8_t)(lcg >> 24);
                }

    uint8_t* d_pix = NULL;
    if (hipMalloc((void**)&d_pix, total) != hipSuccess) die("hipMalloc");
    if (hipMemcpy(d_pix, pix, total, hipMemcpyHostToDevice) != hipSuccess) die("hipMemcpy");
    int32_t views[B][4], want[B][4], vshapes[B][3], Hc = 0, Wc = 0, sizes[B][2];
    if (txo_ingest_trim_views(e, d_pix, offsets, &shapes[0][0], B, level, margin, &views[0][0], NULL)) die("txo_ingest_trim_views");   /* waits */
    int views_bad = 0;
    for (int b = 0; b < B; ++b) {
        trim_view(pix + offsets[b], shapes[b][0], shapes[b][1], shapes[b][2], level, margin, want[b]);
        views_bad |= memcmp(views[b], want[b], sizeof want[b]) != 0;
        vshapes[b][0] = views[b][2]; vshapes[b][1] = views[b][3]; vshapes[b][2] = shapes[b][2];
        printf("trim %dx%d -> %dx%d at (%d, %d)%s", shapes[b][0], shapes[b][1], views[b][2], views[b][3], views[b][0], views[b][1], b + 1 < B ? ", " : "");
    }
    printf(": %s\n", views_bad ? "DIFFER from the rule on the host" : "equal the rule on the host");
    if (views_bad) return 1;
    if (txo_ingest_box(&vshapes[0][0], B, &Hc, &Wc)) die("txo_ingest_box");
    const size_t nbox = (size_t)B * C * Hc * Wc;
    float *d_box = NULL, *d_box2 = NULL; int64_t* d_tok = NULL;
    if (hipMalloc((void**)&d_box, nbox * 4) != hipSuccess || hipMalloc((void**)&d_box2, nbox * 4) != hipSuccess ||
        hipMalloc((void**)&d_tok, (size_t)B * max_len * 8) != hipSuccess) die("hipMalloc");
    if (hipMemset(d_box, 0xff, nbox * 4) != hipSuccess) die("hipMemset");                 /* NaN everywhere: the kernel writes every element */
    if (txo_ingest_u8_view(e, d_pix, offsets, &shapes[0][0], &views[0][0], B, C, 0, 0, Hc, Wc, d_box, &sizes[0][0], NULL, 0, NULL)) die("txo_ingest_u8_view");
    int32_t n_dev = 0, n_host = 0;
    int64_t* tok_dev = (int64_t*)malloc((size_t)B * max_len * 8);
    int64_t* tok_host = (int64_t*)malloc((size_t)B * max_len * 8);
    if (txo_generate_ragged(e, d_box, B, C, Hc, Wc, &sizes[0][0], max_len, cfg.eos, d_tok, &n_dev, NULL)) die("txo_generate_ragged");
    if (hipMemcpy(tok_dev, d_tok, (size_t)B * max_len * 8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");

    float* box = (float*)malloc(nbox * 4);
    float* got = (float*)malloc(nbox * 4);
    host_box(box, pix, offsets, shapes, views, B, C, Hc, Wc);
    int sizes_bad = 0;
    for (int b = 0; b < B; ++b) sizes_bad |= sizes[b][0] != (views[b][2] + 15) / 16 * 16 || sizes[b][1] != (views[b][3] + 15) / 16 * 16;
    if (hipMemcpy(got, d_box, nbox * 4, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
    const int box_bad = memcmp(got, box, nbox * 4) != 0 || sizes_bad;
    printf("%s: %d images -> container %dx%dx%dx%d inside the %dx%d canvas: %s\n", txo_version(), B, B, C, Hc, Wc, Ch, Cw,
           box_bad ? "DIFFERS from the host crop and preprocessing" : "equals the host crop and preprocessing bit for bit");
    if (argc > 2) {
        FILE* o = fopen(argv[2], "wb");
        if (!o) { perror(argv[2]); return 2; }
        const int32_t head[4] = {B, C, Hc, Wc};
        const int64_t tot = (int64_t)total;
        fwrite(head, 4, 4, o); fwrite(shapes, 4, 3 * B, o); fwrite(views, 4, 4 * B, o); fwrite(sizes, 4, 2 * B, o); fwrite(offsets, 8, B, o);
        fwrite(&tot, 8, 1, o); fwrite(pix, 1, total, o); fwrite(got, 4, nbox, o);
        fclose(o);
    }
    if (hipMemcpy(d_box2, box, nbox * 4, hipMemcpyHostToDevice) != hipSuccess) die("hipMemcpy");
    if (txo_generate_ragged(e, d_box2, B, C, Hc, Wc, &sizes[0][0], max_len, cfg.eos, d_tok, &n_host, NULL)) die("txo_generate_ragged (host container)");
    if (hipMemcpy(tok_host, d_tok, (size_t)B * max_len * 8, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
    int tok_bad = n_dev != n_host;
    for (int b = 0; b < B && !tok_bad; ++b)
        for (int t = 0; t < n_dev; ++t)
            if (tok_dev[(size_t)b * max_len + t] != tok_host[(size_t)b * max_len + t]) { tok_bad = 1; break; }
    printf("bytes to tokens: %d steps, first tokens %lld %lld %lld: %s\n", n_dev, (long long)tok_dev[0], (long long)tok_dev[max_len],
           (long long)tok_dev[2 * (size_t)max_len], tok_bad ? "DIFFER from the host container's" : "equal the host container's");

    /* regions: the big page again, through two overlapping boxes that name the same bytes (the page is on the device once) */
    enum { R = 2 };
    int32_t rshapes[R][3], rviews[R][4] = {{ink[1][0] - 4, ink[1][1] - 4, ink[1][2] / 2 + 8, ink[1][3] / 2 + 8},
                                           {ink[1][0] + ink[1][2] / 4, ink[1][1] + ink[1][3] / 4, ink[1][2] / 2, ink[1][3] / 2 + 1}};
    int32_t rv[R][3], rHc = 0, rWc = 0, rsizes[R][2];
    int64_t roff[R] = {offsets[1], offsets[1]};
    for (int r = 0; r < R; ++r) { memcpy(rshapes[r], shapes[1], sizeof shapes[1]); rv[r][0] = rviews[r][2]; rv[r][1] = rviews[r][3]; rv[r][2] = shapes[1][2]; }
    if (txo_ingest_box(&rv[0][0], R, &rHc, &rWc)) die("txo_ingest_box (regions)");
    const size_t nreg = (size_t)R * C * rHc * rWc;
    if (nreg > nbox) die("regions larger than the first container");
    if (hipMemset(d_box, 0xff, nreg * 4) != hipSuccess) die("hipMemset");
    if (txo_ingest_u8_view(e, d_pix, roff, &rshapes[0][0], &rviews[0][0], R, C, 0, 0, rHc, rWc, d_box, &rsizes[0][0], NULL, 0, NULL)) die("txo_ingest_u8_view (regions)");
    if (hipMemcpy(got, d_box, nreg * 4, hipMemcpyDeviceToHost) != hipSuccess) die("hipMemcpy back");
    host_box(box, pix, roff, rshapes, rviews, R, C, rHc, rWc);
    const int reg_bad = memcmp(got, box, nreg * 4) != 0;
    printf("regions: %d overlapping views of one %dx%d page -> container %dx%dx%dx%d: %s\n", R, shapes[1][0], shapes[1][1], R, C, rHc, rWc,
           reg_bad ? "DIFFERS from the host crops" : "equals the host crops bit for bit");
    /* refusals name what is wrong, and nothing is enqueued: a level outside [0, 254]; a view that reaches outside its image */
    const int rc0 = txo_ingest_trim_views(e, d_pix, offsets, &shapes[0][0], B, 255, margin, &views[0][0], NULL);
    printf("level 255 -> %d (%s)\n", rc0, txo_last_error());
    rviews[1][3] = shapes[1][1];
    const int rc1 = txo_ingest_u8_view(e, d_pix, roff, &rshapes[0][0], &rviews[0][0], R, C, 0, 0, rHc, rWc, d_box, &rsizes[0][0], NULL, 0, NULL);
    printf("a view beyond its image -> %d (%s)\n", rc1, txo_last_error());
    txo_engine_destroy(e);
    hipFree(d_pix); hipFree(d_box); hipFree(d_box2); hipFree(d_tok);
    free(pix); free(box); free(got); free(tok_dev); free(tok_host);
    return box_bad || tok_bad || reg_bad || rc0 != TXO_E_INVALID || rc1 != TXO_E_INVALID;
}
