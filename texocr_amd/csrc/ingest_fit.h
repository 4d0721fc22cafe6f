// Fit-to-canvas ingest (texocr.h: txo_ingest_u8_fit): an image with a side beyond the target (Fh, Fw) is downscaled to fit it, aspect ratio
// kept, on the device and in front of the ingest arithmetic of ingest.h.  The fitted bytes are bit for bit PIL's
// Image.resize((w', h'), BILINEAR) of the image's L / RGB channels (alpha is not read), so the container stays what the host path makes.
//
// PIL's 8-bit resample is integer arithmetic over a coefficient table: per output pixel of one axis a window [xmin, xmin + n) of the source
// and n weights K[x] = (int)(0.5 + k[x] * 2^22), k the normalised triangle filter widened by the scale; the output byte is
// clamp((2^21 + sum K[x] src[xmin + x]) >> 22).  Two passes, horizontal first into a uint8 intermediate h x w' x {1, 3}, then vertical; a pass
// whose axis keeps its size is skipped.  The table comes from a handful of IEEE double operations, each rounded on its own (PIL is plain C):
// fit_axis_coeffs below is that sequence, one body for the host (txo_ingest_fit_coeffs, which the CPU suite pins against a restatement in
// Python) and for both kernels.  Every operation goes through fit_add / fit_sub / fit_mul / fit_div -- __dadd_rn ... on the device, one
// operation per function body on the host -- so -ffp-contract=on can fuse nothing.
//
// Why the tables are computed on the device and not copied: at the default canvas one oversized image has 1008 + 160 output pixels of up to
// 65 taps, 0.3 MB of table against the 24-byte descriptor that goes up today, and 256 images would add 80 MB of host work and copy to a call
// whose point is ONE copy of the raw bytes.  On the device a block computes the table of its own 64 columns (or 4 rows) into LDS: a few
// hundred fp64 operations per lane, amortised over the rows (columns) the block then resamples.
//
// fit_rows_kernel   horizontal pass, only over the images that need one (hlist).  A block is 64 adjacent output columns x 4 lanes over 32 source
//                   rows; adjacent lanes take adjacent columns, whose windows start `scale` pixels apart and overlap, so a wave's loads cover
//                   one contiguous span of the source row.  K[tap][column] in LDS: a wave reads one bank row per tap, no conflict.
// ingest_fit_kernel vertical pass fused with the ingest arithmetic, the launch geometry of ingest_u8_kernel: a lane makes four consecutive
//                   fitted pixels of one row in registers (never stored as bytes) and hands them to the same c / 255.0f table, luma and
//                   16-byte stores.  An image without a horizontal pass reads its source directly; an image that fits, or whose height
//                   stays, goes through the per-pixel code of ingest_u8_kernel.
// Only bytes of pixels inside (h, w) of the source, or inside the intermediate this call wrote, are named; every element of the container
// is written.
#pragma once

namespace txo {

constexpr int FIT_MAX_SCALE = 32;                    // in / out per axis; beyond it the call is refused (bounds the taps, not the quality)
constexpr int FIT_TAPS = 2 * FIT_MAX_SCALE + 1;      // the widest window: support = scale source pixels on either side of the centre
constexpr int FIT_BITS = 22;                         // PIL's PRECISION_BITS for 8-bit channels: 32 - 8 - 2

__host__ __device__ inline double fit_add(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(a, b);
#else
    return a + b;
#endif
}
__host__ __device__ inline double fit_sub(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsub_rn(a, b);
#else
    return a - b;
#endif
}
__host__ __device__ inline double fit_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    return a * b;
#endif
}
__host__ __device__ inline double fit_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}

// the triangle filter at source pixel xmin + x, unnormalised: tri((x + xmin - center + 0.5) * ss), tri(t) = 1 - |t| below 1, else 0
__host__ __device__ inline double fit_tap(int x, int xmin, double center, double ss) {
    double t = fit_mul(fit_add(fit_sub((double)(x + xmin), center), 0.5), ss);
    if (t < 0.0) t = -t;
    return t < 1.0 ? fit_sub(1.0, t) : 0.0;
}

// One output pixel xx of an axis with `in` source and `out` target pixels: its window (*xmin_out, *n_out) and the coefficients
// K[x * stride] for x = first, first + step, ... below n (the host asks for all of them, 0 and 1; the lanes of a block share them out).
// The normalising sum runs over ALL taps, in order from 0.0, whoever asks.  n <= FIT_TAPS when in <= FIT_MAX_SCALE * out.
__host__ __device__ inline void fit_axis_coeffs(int in, int out, int xx, int* xmin_out, int* n_out, int* K, int stride, int first, int step) {
    const double scale = fit_div((double)in, (double)out);
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fit_mul(1.0, fs);
    const double ss = fit_div(1.0, fs);
    const double center = fit_mul(fit_add((double)xx, 0.5), scale);
    int xmin = (int)fit_add(fit_sub(center, support), 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)fit_add(fit_add(center, support), 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww = fit_add(ww, fit_tap(x, xmin, center, ss));
    for (int x = first; x < n; x += step) {
        double k = fit_tap(x, xmin, center, ss);
        if (ww != 0.0) k = fit_div(k, ww);
        K[(size_t)x * stride] = (int)fit_add(0.5, fit_mul(k, (double)(1 << FIT_BITS)));       // (coefficients are >= 0 for this filter)
    }
    *xmin_out = xmin;
    *n_out = n;
}

// the rule of texocr.h "Fit-to-canvas ingest": (h, w) -> the fitted (h', w') under the target (Fh, Fw); 64-bit products
__host__ __device__ inline void fit_size(long long h, long long w, long long Fh, long long Fw, int* fh, int* fw) {
    if (h <= Fh && w <= Fw) { *fh = (int)h; *fw = (int)w; return; }
    if (w * Fh <= h * Fw) { const long long v = (w * Fh) / h; *fh = (int)Fh; *fw = (int)(v < 1 ? 1 : v); }
    else { const long long v = (h * Fw) / w; *fw = (int)Fw; *fh = (int)(v < 1 ? 1 : v); }
}

// One image of the list.  off: its first byte in the pixel buffer; (h, w, ch) its source shape; (fh, fw) its fitted shape (= (h, w) when it
// fits); mid: the byte offset of its horizontal pass's intermediate [h][fw][ch == 1 ? 1 : 3] in the scratch buffer, -1 when fw == w.
// reserved: 0, or -- for the PITCHED forms of the kernels, which read a VIEW of a larger image (txo_ingest_u8_view) -- the pixels from one
// source row to the next; (h, w) is then the view's shape and off the byte of its first pixel.  The intermediate is always fw wide.
struct FitDesc { long long off, mid; int h, w, ch, fh, fw, reserved; };
// bytes one intermediate takes in the scratch buffer (every one starts 16-byte aligned)
inline long long ingest_fit_mid_bytes(long long h, long long fw, int ch) { return (h * fw * (ch == 1 ? 1 : 3) + 15) / 16 * 16; }

__device__ __forceinline__ int fit_byte(int acc) {               // acc starts at 2^21, the rounding term
    const int v = acc >> FIT_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

constexpr int FR_COLS = 64, FR_LANES_Y = 4, FR_ROWS = 32;        // fit_rows_kernel's block: 64 output columns x 4 lanes over 32 source rows

// (PITCHED, here and in ingest_fit_kernel: as in ingest_u8_kernel; the <false> forms are the kernels as they were)
template <bool PITCHED>
__global__ __launch_bounds__(FR_COLS * FR_LANES_Y) void fit_rows_kernel(const unsigned char* __restrict__ pix, const FitDesc* __restrict__ desc,
                                                                       const int* __restrict__ hlist, unsigned char* __restrict__ scratch) {
    __shared__ int K[FIT_TAPS * FR_COLS];                        // [tap][column of the block]
    const FitDesc d = desc[hlist[blockIdx.z]];
    const int tx = threadIdx.x % FR_COLS, ty = threadIdx.x / FR_COLS;
    const int xx = (int)blockIdx.x * FR_COLS + tx, y0 = (int)blockIdx.y * FR_ROWS;
    if ((int)blockIdx.x * FR_COLS >= d.fw || y0 >= d.h) return;  // (block-uniform: the grid is sized by the largest image of hlist)
    int xmin = 0, n = 0;
    if (xx < d.fw) fit_axis_coeffs(d.w, d.fw, xx, &xmin, &n, K + tx, FR_COLS, ty, FR_LANES_Y);   // the column's four lanes share its taps out
    __syncthreads();
    if (xx >= d.fw) return;
    const int y1 = y0 + FR_ROWS < d.h ? y0 + FR_ROWS : d.h;
    const int mch = d.ch == 1 ? 1 : 3;
    for (int y = y0 + ty; y < y1; y += FR_LANES_Y) {
        const unsigned char* p = pix + d.off + ((long long)y * (PITCHED ? d.reserved : d.w) + xmin) * d.ch;   // xmin + n <= w: inside row y
        unsigned char* q = scratch + d.mid + ((long long)y * d.fw + xx) * mch;
        if (d.ch == 1) {
            int a = 1 << (FIT_BITS - 1);
            for (int x = 0; x < n; ++x) a += K[x * FR_COLS + tx] * (int)p[x];
            q[0] = (unsigned char)fit_byte(a);
        } else {
            int a0 = 1 << (FIT_BITS - 1), a1 = a0, a2 = a0;
            for (int x = 0; x < n; ++x) {
                const int k = K[x * FR_COLS + tx];
                const unsigned char* s = p + x * d.ch;
                a0 += k * (int)s[0]; a1 += k * (int)s[1]; a2 += k * (int)s[2];
            }
            q[0] = (unsigned char)fit_byte(a0); q[1] = (unsigned char)fit_byte(a1); q[2] = (unsigned char)fit_byte(a2);
        }
    }
}

// four consecutive fitted pixels (y, x0 .. x0 + 3) of the vertical pass over the view `img` (rows sw pixels apart, of sch bytes each), of which NPX exist:
// the vertical taps in integers, then the ingest arithmetic; returned by value (pixels behind NPX are 0.0f)
template <int NPX>
__device__ __forceinline__ float4 fit_column_piece(const unsigned char* __restrict__ img, int sw, int sch, int x0, int ymin, int n, const int* Kr,
                                                   const float* unit) {
    const long long row = (long long)sw * sch;
    const unsigned char* p = img + ((long long)ymin * sw + x0) * sch;                           // rows ymin .. ymin + n - 1 < h
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f, o3 = 0.0f;
    if (sch == 1) {
        int a0 = 1 << (FIT_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
        for (int t = 0; t < n; ++t, p += row) {
            const int k = Kr[t];
            a0 += k * (int)p[0];
            if (NPX > 1) a1 += k * (int)p[1];
            if (NPX > 2) a2 += k * (int)p[2];
            if (NPX > 3) a3 += k * (int)p[3];
        }
        const float v0 = unit[fit_byte(a0)], v1 = unit[fit_byte(a1)], v2 = unit[fit_byte(a2)], v3 = unit[fit_byte(a3)];
        o0 = ingest_luma_inv(v0, v0, v0);
        if (NPX > 1) o1 = ingest_luma_inv(v1, v1, v1);
        if (NPX > 2) o2 = ingest_luma_inv(v2, v2, v2);
        if (NPX > 3) o3 = ingest_luma_inv(v3, v3, v3);
    } else {
        const int half = 1 << (FIT_BITS - 1);
        int r0 = half, g0 = half, b0 = half, r1 = half, g1 = half, b1 = half, r2 = half, g2 = half, b2 = half, r3 = half, g3 = half, b3 = half;
        for (int t = 0; t < n; ++t, p += row) {
            const int k = Kr[t];
            r0 += k * (int)p[0]; g0 += k * (int)p[1]; b0 += k * (int)p[2];
            if (NPX > 1) { r1 += k * (int)p[sch]; g1 += k * (int)p[sch + 1]; b1 += k * (int)p[sch + 2]; }
            if (NPX > 2) { r2 += k * (int)p[2 * sch]; g2 += k * (int)p[2 * sch + 1]; b2 += k * (int)p[2 * sch + 2]; }
            if (NPX > 3) { r3 += k * (int)p[3 * sch]; g3 += k * (int)p[3 * sch + 1]; b3 += k * (int)p[3 * sch + 2]; }
        }
        o0 = ingest_luma_inv(unit[fit_byte(r0)], unit[fit_byte(g0)], unit[fit_byte(b0)]);
        if (NPX > 1) o1 = ingest_luma_inv(unit[fit_byte(r1)], unit[fit_byte(g1)], unit[fit_byte(b1)]);
        if (NPX > 2) o2 = ingest_luma_inv(unit[fit_byte(r2)], unit[fit_byte(g2)], unit[fit_byte(b2)]);
        if (NPX > 3) o3 = ingest_luma_inv(unit[fit_byte(r3)], unit[fit_byte(g3)], unit[fit_byte(b3)]);
    }
    return make_float4(o0, o1, o2, o3);
}

// The body between the table fill and the stores is ingest_u8_kernel's, statement for statement, on the view (img, fw, sch) -- restated here
// and not shared, because that kernel is pinned register for register (profiles/ingest_resource_usage.txt) and taking its body out into a
// function changed its allocation.
template <bool PITCHED>
__global__ __launch_bounds__(IG_LANES_X * IG_ROWS) void ingest_fit_kernel(const unsigned char* __restrict__ pix, const unsigned char* __restrict__ scratch,
                                                                         const FitDesc* __restrict__ desc, float* __restrict__ box, int C, int Hc, int Wc) {
    __shared__ float unit[256];                                  // c / 255.0f for every byte value
    __shared__ int K[IG_ROWS][FIT_TAPS];                         // the vertical table of the block's four rows
    const FitDesc d = desc[blockIdx.z];
    const int tx = threadIdx.x % IG_LANES_X, ty = threadIdx.x / IG_LANES_X;
    const int x0 = ((int)blockIdx.x * IG_LANES_X + tx) * IG_PIECE, y = (int)blockIdx.y * IG_ROWS + ty;
    // what the vertical pass (or, without one, the pixel code) reads: the intermediate where a horizontal pass ran, else the source; fw wide
    const unsigned char* img = d.mid >= 0 ? scratch + d.mid : pix + d.off;
    const int sch = d.mid >= 0 ? (d.ch == 1 ? 1 : 3) : d.ch;
    const int sw = PITCHED ? (d.mid >= 0 ? d.fw : d.reserved) : d.fw;   // pixels from one row of img to the next (only the source has a pitch)
    float o[IG_PIECE] = {0.0f, 0.0f, 0.0f, 0.0f};
    // (block-uniform, like the branch on fh == h below: a block that lies wholly outside the fitted image only writes zeros)
    if ((int)blockIdx.y * IG_ROWS < d.fh && (int)blockIdx.x * IG_BLOCK_W < d.fw) {
        unit[threadIdx.x] = __fdiv_rn((float)threadIdx.x, 255.0f);
        if (d.fh == d.h) {                                       // the height stays: an image that fits, or one with a horizontal pass only
            __syncthreads();
            if (y < d.fh && x0 < d.fw) {
                const unsigned char* p = img + ((long long)y * sw + x0) * sch;
                const int n = d.fw - x0;                         // pixels of this row from x0 on: the piece reads min(n, 4) of them
                if (n >= IG_PIECE && sch == 1) {                 // a whole piece of L: four loads issued before the first use
                    unsigned char c[IG_PIECE];
#pragma unroll
                    for (int i = 0; i < IG_PIECE; ++i) c[i] = p[i];
#pragma unroll
                    for (int i = 0; i < IG_PIECE; ++i) { const float a = unit[c[i]]; o[i] = ingest_luma_inv(a, a, a); }
                } else if (n >= IG_PIECE) {                      // a whole piece of RGB / RGBA: twelve loads issued before the first use
                    unsigned char c[IG_PIECE][3];
#pragma unroll
                    for (int i = 0; i < IG_PIECE; ++i) { c[i][0] = p[i * sch]; c[i][1] = p[i * sch + 1]; c[i][2] = p[i * sch + 2]; }
#pragma unroll
                    for (int i = 0; i < IG_PIECE; ++i) o[i] = ingest_luma_inv(unit[c[i][0]], unit[c[i][1]], unit[c[i][2]]);
                } else {                                         // the row ends inside the piece: every pixel under its own bound
#pragma unroll
                    for (int i = 0; i < IG_PIECE - 1; ++i) {
                        if (i < n) {
                            const unsigned char* q = p + i * sch;
                            const float ar = unit[q[0]];
                            const float ag = sch == 1 ? ar : unit[q[1]];
                            const float ab = sch == 1 ? ar : unit[q[2]];
                            o[i] = ingest_luma_inv(ar, ag, ab);
                        }
                    }
                }
            }
        } else {
            int ymin = 0, n = 0;
            if (y < d.fh) fit_axis_coeffs(d.h, d.fh, y, &ymin, &n, K[ty], 1, tx, IG_LANES_X);   // the row's 64 lanes share its taps out
            __syncthreads();
            if (y < d.fh && x0 < d.fw) {
                const int npx = d.fw - x0;
                float4 v;
                if (npx >= IG_PIECE) v = fit_column_piece<4>(img, sw, sch, x0, ymin, n, K[ty], unit);
                else if (npx == 3) v = fit_column_piece<3>(img, sw, sch, x0, ymin, n, K[ty], unit);
                else if (npx == 2) v = fit_column_piece<2>(img, sw, sch, x0, ymin, n, K[ty], unit);
                else v = fit_column_piece<1>(img, sw, sch, x0, ymin, n, K[ty], unit);
                o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
            }
        }
    }
    if (x0 < Wc && y < Hc) {
        const float4 v = make_float4(o[0], o[1], o[2], o[3]);
        float* dst = box + (((size_t)blockIdx.z * C) * Hc + y) * Wc + x0;
        for (int c = 0; c < C; ++c) *reinterpret_cast<float4*>(dst + (size_t)c * Hc * Wc) = v;   // in_channels > 1: the same plane C times
    }
}

}  // namespace txo
