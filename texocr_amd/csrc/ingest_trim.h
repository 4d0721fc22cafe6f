// Trim-to-ink ingest (texocr.h: txo_ingest_trim_views): the ink extents of B raw uint8 images, found on the device in ONE launch over the
// bytes txo_ingest_u8 is about to read, so that the ingest (and the fit in front of it) can run on the rectangle that holds the formula and
// not on the white around it.  The rule is integer-only: a pixel is ink iff min(read channels) <= level, i.e. iff ANY read byte of it is
// <= level (L as it is; R, G, B of RGB / RGBA; the alpha is never looked at).  The kernel leaves (ymin, xmin, ymax, xmax) of the ink per
// image; the margin and the clamp to the image are a dozen integer operations per image on the host (engine.hip: trim_views).
//
// Shape of the work: read-bound, every byte touched once, nothing written but 16 bytes per image.  Rows are tightly packed, so an image is
// a BYTE STREAM of n = h * w * ch bytes from pix + off, whatever its width: a lane takes 16-byte pieces of the stream at 16-byte ALIGNED
// addresses (piece j covers the image's bytes [16 j - lead, 16 j - lead + 16), lead = the first byte's address mod 16).  A piece that lies
// wholly inside [0, n) is one 16-byte load; the first and the last piece of an image may hang over either end and are read byte by byte,
// each byte under its own bound, so no byte outside the image's own h * w * ch is named -- a neighbour packed right behind it is never
// seen.  A byte outside counts as 255, which no level (<= 254) calls ink.
// Most pieces of a formula image are white: a piece is first asked whether ANY of its bytes is <= level (the alpha bytes included: a
// conservative question), and only one that says yes pays for the coordinates -- the pixel of its first byte from one division by the
// width, then a step per byte (channel, column, row), skipping every fourth byte of RGBA.
// Reduction: min / max of y and x per lane, per wave with shuffles, per block through LDS, then ONE set of atomicMin / atomicMax per block
// that saw ink into the image's record.  Min and max do not depend on the order, so the result is deterministic.  The record starts as
// (INT_MAX, INT_MAX, -1, -1) from trim_fill_kernel on the same stream; an image without ink leaves it so.
// Grid: (tiles of the largest image, images); a block beyond its image returns at once.
#pragma once

#include <climits>

namespace txo {

constexpr int TB_THREADS = 256, TB_PIECES = 4;                   // trim_bbox_kernel's block: 256 lanes, 4 pieces of 16 bytes per lane
constexpr int TB_TILE = TB_THREADS * TB_PIECES;                  // pieces per block: 16 KiB of the stream

__global__ __launch_bounds__(256) void trim_fill_kernel(int* __restrict__ rec, int B) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b < B) *reinterpret_cast<int4*>(rec + 4 * (size_t)b) = make_int4(INT_MAX, INT_MAX, -1, -1);
}

__device__ __forceinline__ bool trim_any_le(unsigned v, unsigned level) {      // is any of the four bytes of v <= level
    return (v & 255u) <= level || ((v >> 8) & 255u) <= level || ((v >> 16) & 255u) <= level || (v >> 24) <= level;
}

__global__ __launch_bounds__(TB_THREADS) void trim_bbox_kernel(const unsigned char* __restrict__ pix, const IngestDesc* __restrict__ desc,
                                                               int* __restrict__ rec, int level) {
    __shared__ int part[TB_THREADS / 64][4];
    const IngestDesc d = desc[blockIdx.y];
    const long long n = (long long)d.h * d.w * d.ch;             // the image's bytes
    const unsigned char* base = pix + d.off;
    const int lead = (int)(reinterpret_cast<uintptr_t>(base) & 15);
    const long long np = (lead + n + 15) >> 4;                   // aligned pieces that hold a byte of the image
    const long long j0 = (long long)blockIdx.x * TB_TILE;
    if (j0 >= np) return;                                        // (block-uniform: the grid is sized by the largest image)
    const unsigned lv = (unsigned)level;
    int ymin = INT_MAX, xmin = INT_MAX, ymax = -1, xmax = -1;
    for (int it = 0; it < TB_PIECES; ++it) {
        const long long j = j0 + it * TB_THREADS + (int)threadIdx.x;
        if (j >= np) break;
        const long long i0 = j * 16 - lead;                      // the image byte the piece starts at; negative only for j == 0
        unsigned v[4];
        if (i0 >= 0 && i0 + 16 <= n) {                           // wholly inside: one aligned 16-byte load
            const uint4 q = *reinterpret_cast<const uint4*>(base + i0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {                                                 // the head or the tail: every byte under its own bound, 255 outside
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                unsigned word = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const long long at = i0 + 4 * k + i;
                    const unsigned byte = (at >= 0 && at < n) ? (unsigned)base[at] : 255u;
                    word |= byte << (8 * i);
                }
                v[k] = word;
            }
        }
        if (!(trim_any_le(v[0], lv) || trim_any_le(v[1], lv) || trim_any_le(v[2], lv) || trim_any_le(v[3], lv))) continue;
        // the pixel of the first byte that lies inside the image: one division by the width (32-bit where the pixel index allows)
        const int skip = i0 < 0 ? (int)-i0 : 0;
        const long long at = i0 + skip;
        const long long px = d.ch == 1 ? at : (d.ch == 4 ? at >> 2 : at / 3);
        int c = (int)(at - px * d.ch);
        const long long row = (px >> 32) == 0 ? (long long)((unsigned)px / (unsigned)d.w) : px / d.w;
        int y = (int)row, x = (int)(px - row * d.w);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k >= skip) {
                const unsigned byte = (v[k >> 2] >> (8 * (k & 3))) & 255u;
                if (c != 3 && byte <= lv) {                      // (c == 3: the alpha of RGBA)
                    ymin = min(ymin, y); ymax = max(ymax, y);
                    xmin = min(xmin, x); xmax = max(xmax, x);
                }
                if (++c == d.ch) { c = 0; if (++x == d.w) { x = 0; ++y; } }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ymin = min(ymin, __shfl_xor(ymin, o)); xmin = min(xmin, __shfl_xor(xmin, o));
        ymax = max(ymax, __shfl_xor(ymax, o)); xmax = max(xmax, __shfl_xor(xmax, o));
    }
    const int wave = (int)threadIdx.x / 64;
    if (threadIdx.x % 64 == 0) { part[wave][0] = ymin; part[wave][1] = xmin; part[wave][2] = ymax; part[wave][3] = xmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int wv = 1; wv < TB_THREADS / 64; ++wv) {
            ymin = min(ymin, part[wv][0]); xmin = min(xmin, part[wv][1]);
            ymax = max(ymax, part[wv][2]); xmax = max(xmax, part[wv][3]);
        }
        if (ymax >= 0) {                                         // the block saw ink: one set of atomics into the image's record
            int* r = rec + 4 * (size_t)blockIdx.y;
            atomicMin(r, ymin); atomicMin(r + 1, xmin); atomicMax(r + 2, ymax); atomicMax(r + 3, xmax);
        }
    }
}

}  // namespace txo
