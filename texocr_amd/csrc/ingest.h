// Device-side image ingest (texocr.h: txo_ingest_u8): the raw uint8 pixels of B images of different sizes and channel counts -> the float32
// container [B][C][Hc][Wc] of a ragged batch, in ONE launch.  What the wrapper does per image on the host (texocr_amd/wrapper.py:
// preprocess_image = ToTensor -> Grayscale -> Invert, pad to multiples of 16, expand to in_channels, pack_ragged) is this kernel's output
// bit for bit.
//
// The arithmetic, every step rounded to float32 on its own (numpy evaluates preprocess_image's expressions one ufunc at a time):
//     a_c = float(c) / 255.0f          an IEEE division (a multiply by 1/255 differs on a quarter of the pixels)
//     s   = (0.2989f * a_r + 0.587f * a_g) + 0.114f * a_b      three products and two sums, none fused
//     out = 1.0f - s
// The library is built with -ffp-contract=on, which fuses a * b + c inside one source expression: the products and sums below go through
// __fmul_rn / __fadd_rn / __fsub_rn (one operation per function body), so no multiply-add can form.  The division is taken once per block
// for every byte value (256 threads, 256 values) and looked up from LDS afterwards: 12 divisions per lane would make the kernel VALU-bound.
//
// Shape of the work: write-dominated (4 C bytes out per pixel, 1-4 in).  A lane produces four consecutive floats of one container row and
// stores them as one 16-byte piece per channel plane (Wc % 4 == 0 and a 16-byte aligned container, checked by the host); a block is 64 lanes
// across (256 columns) by 4 rows; the grid is (row pieces, container rows / 4, images).  A lane is "pixel" where (y, x) lies inside the image's
// own (h, w) and "zero" elsewhere -- the image's pad up to the next multiple of 16 and the rest of the slot alike are exactly 0.0f, not the
// value white maps to (9.9957e-05: the luma weights sum to 0.9999).  Source rows are tightly packed, so with 3-byte pixels or an odd width a
// row starts at any byte: the pixels are read as BYTES, and only bytes of pixels inside (h, w) are named, so nothing behind an image's last
// byte is touched.  A piece that lies wholly inside its row issues all of its loads before the first use (the compiler may merge bytes of one
// pixel, or the four of an L piece, into a wider unaligned load: still the same bytes); a piece the row ends in reads pixel by pixel, each
// under its own bound.  12 byte loads per lane for RGB against one 16-byte store per plane; a wave's loads are contiguous and stay in L1 / L2.
#pragma once

namespace txo {

// one image of the list: where its first byte lies in the pixel buffer, and its shape.  ch: 1 = L, 3 = RGB, 4 = RGBA (alpha is not read)
// reserved: 0, or -- for the PITCHED form of the kernel, which reads a VIEW of a larger image (ingest_trim.h, txo_ingest_u8_view) -- the pixels
// from one source row to the next; (h, w) is then the view's shape and off the byte of its first pixel
struct IngestDesc { long long off; int h, w, ch, reserved; };

constexpr int IG_LANES_X = 64, IG_ROWS = 4, IG_PIECE = 4;        // block: 64 x 4 lanes, 4 floats per lane
constexpr int IG_BLOCK_W = IG_LANES_X * IG_PIECE;               // container columns per block

__device__ __forceinline__ float ingest_luma_inv(float ar, float ag, float ab) {
    const float pr = __fmul_rn(0.2989f, ar);
    const float pg = __fmul_rn(0.587f, ag);
    const float pb = __fmul_rn(0.114f, ab);
    const float s = __fadd_rn(__fadd_rn(pr, pg), pb);
    return __fsub_rn(1.0f, s);
}

// PITCHED: source rows are d.reserved pixels apart and not d.w (a view of a larger image).  A template parameter: the <false> form is the
// kernel as it was, register for register (profiles/ingest_trim_resource_usage.txt).
template <bool PITCHED>
__global__ __launch_bounds__(IG_LANES_X * IG_ROWS) void ingest_u8_kernel(const unsigned char* __restrict__ pix, const IngestDesc* __restrict__ desc,
                                                                        float* __restrict__ box, int C, int Hc, int Wc) {
    __shared__ float unit[256];                                  // c / 255.0f for every byte value
    const IngestDesc d = desc[blockIdx.z];
    const int tx = threadIdx.x % IG_LANES_X, ty = threadIdx.x / IG_LANES_X;
    const int x0 = ((int)blockIdx.x * IG_LANES_X + tx) * IG_PIECE, y = (int)blockIdx.y * IG_ROWS + ty;
    float o[IG_PIECE] = {0.0f, 0.0f, 0.0f, 0.0f};
    // (block-uniform: a block that lies wholly outside the image only writes zeros)
    if ((int)blockIdx.y * IG_ROWS < d.h && (int)blockIdx.x * IG_BLOCK_W < d.w) {
        unit[threadIdx.x] = __fdiv_rn((float)threadIdx.x, 255.0f);
        __syncthreads();
        // (ingest_fit.h: ingest_fit_kernel restates this block, statement for statement, for the images of a fitted batch that keep their
        // height; a change here goes there too, or a mixed batch stops being bit for bit this kernel's -- tests/test_gpu_ingest_fit.py)
        if (y < d.h && x0 < d.w) {
            const unsigned char* p = pix + d.off + ((long long)y * (PITCHED ? d.reserved : d.w) + x0) * d.ch;
            const int n = d.w - x0;                              // pixels of this row from x0 on: the piece reads min(n, 4) of them
            if (n >= IG_PIECE && d.ch == 1) {                    // a whole piece of L: four loads issued before the first use
                unsigned char c[IG_PIECE];
#pragma unroll
                for (int i = 0; i < IG_PIECE; ++i) c[i] = p[i];
#pragma unroll
                for (int i = 0; i < IG_PIECE; ++i) { const float a = unit[c[i]]; o[i] = ingest_luma_inv(a, a, a); }
            } else if (n >= IG_PIECE) {                          // a whole piece of RGB / RGBA: twelve loads issued before the first use
                unsigned char c[IG_PIECE][3];
#pragma unroll
                for (int i = 0; i < IG_PIECE; ++i) { c[i][0] = p[i * d.ch]; c[i][1] = p[i * d.ch + 1]; c[i][2] = p[i * d.ch + 2]; }
#pragma unroll
                for (int i = 0; i < IG_PIECE; ++i) o[i] = ingest_luma_inv(unit[c[i][0]], unit[c[i][1]], unit[c[i][2]]);
            } else {                                             // the row ends inside the piece: every pixel under its own bound
#pragma unroll
                for (int i = 0; i < IG_PIECE - 1; ++i) {
                    if (i < n) {
                        const unsigned char* q = p + i * d.ch;
                        const float ar = unit[q[0]];
                        const float ag = d.ch == 1 ? ar : unit[q[1]];
                        const float ab = d.ch == 1 ? ar : unit[q[2]];
                        o[i] = ingest_luma_inv(ar, ag, ab);
                    }
                }
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
