// The per-item bodies of the packed uint8 -> I420 conversion, shared by the two files that write I420: mf_i420.hip (a contiguous block of frames) and
// mf_frame_gather.hip (frames gathered from anywhere into chosen frames of a block).  One definition of the integers and of what a work item reads and writes, so
// both entry points give the same bytes for the same source pixels.  The arithmetic is stated in mf_i420.hip's file comment.
//
// A work item is handed four pointers into ONE frame: `src` at its first pixel (row y, column x of the packed [H][W][3] image), `yp` at (y, x) of the Y plane,
// `cb` / `cr` at (y / 2, x / 2) of the chroma planes.  Who computes them (from a block index or from a gather table) is the caller's business.
//   mf_i420_strip<RGB>   2 rows x 8 pixels: 2 x 6 dword loads, two 8-byte Y stores, one dword of Cb, one of Cr.  Needs W % 8 == 0 and the frame's source and
//                        planes 4-byte aligned (every row, plane and strip offset is then a multiple of 4)
//   mf_i420_block<RGB>   one 2 x 2 block, byte loads and byte stores: any even W, any alignment
#pragma once
#include <cstdint>

namespace mf_i420 {

constexpr int STRIP = 8;           // pixels per item along x on the strip path

__device__ __forceinline__ int luma(int r, int g, int b) { return (16829 * r + 33039 * g + 6416 * b + (16 << 16) + 32768) >> 16; }
__device__ __forceinline__ int chroma_b(int sr, int sg, int sb) { return (-9714 * sr - 19070 * sg + 28784 * sb + (128 << 18) + (1 << 17)) >> 18; }
__device__ __forceinline__ int chroma_r(int sr, int sg, int sb) { return (28784 * sr - 24103 * sg - 4681 * sb + (128 << 18) + (1 << 17)) >> 18; }

// byte k of 24 packed bytes held as 6 dwords (k is a constant after unrolling: one v_bfe_u32)
__device__ __forceinline__ int byte_of(const uint32_t (&w)[6], int k) { return (int)((w[k >> 2] >> ((k & 3) * 8)) & 0xffu); }

struct __attribute__((aligned(4))) Bytes8 { uint32_t lo, hi; };     // an 8-byte store that only needs dword alignment

// RGB: channel 0 of the source is R (else B)
template <bool RGB>
__device__ __forceinline__ void mf_i420_strip(const uint8_t* __restrict__ src, int W, uint8_t* __restrict__ yp, uint8_t* __restrict__ cb, uint8_t* __restrict__ cr) {
    uint32_t top[6], bot[6];
    const uint32_t* p0 = reinterpret_cast<const uint32_t*>(src);
    const uint32_t* p1 = reinterpret_cast<const uint32_t*>(src + (int64_t)W * 3);
#pragma unroll
    for (int i = 0; i < 6; ++i) { top[i] = p0[i]; bot[i] = p1[i]; }
    uint32_t y0[2] = {0, 0}, y1[2] = {0, 0}, ub = 0, ur = 0;
#pragma unroll
    for (int i = 0; i < STRIP; i += 2) {
        int sr = 0, sg = 0, sb = 0;
#pragma unroll
        for (int j = i; j < i + 2; ++j) {
            const int t0 = byte_of(top, 3 * j), t1 = byte_of(top, 3 * j + 1), t2 = byte_of(top, 3 * j + 2);
            const int u0 = byte_of(bot, 3 * j), u1 = byte_of(bot, 3 * j + 1), u2 = byte_of(bot, 3 * j + 2);
            const int tr = RGB ? t0 : t2, tb = RGB ? t2 : t0, vr = RGB ? u0 : u2, vb = RGB ? u2 : u0;
            y0[j >> 2] |= (uint32_t)luma(tr, t1, tb) << ((j & 3) * 8);
            y1[j >> 2] |= (uint32_t)luma(vr, u1, vb) << ((j & 3) * 8);
            sr += tr + vr; sg += t1 + u1; sb += tb + vb;
        }
        ub |= (uint32_t)chroma_b(sr, sg, sb) << ((i >> 1) * 8);
        ur |= (uint32_t)chroma_r(sr, sg, sb) << ((i >> 1) * 8);
    }
    *reinterpret_cast<Bytes8*>(yp) = Bytes8{y0[0], y0[1]};
    *reinterpret_cast<Bytes8*>(yp + W) = Bytes8{y1[0], y1[1]};
    *reinterpret_cast<uint32_t*>(cb) = ub;
    *reinterpret_cast<uint32_t*>(cr) = ur;
}

template <bool RGB>
__device__ __forceinline__ void mf_i420_block(const uint8_t* __restrict__ src, int W, uint8_t* __restrict__ yp, uint8_t* __restrict__ cb, uint8_t* __restrict__ cr) {
    const uint8_t* s1 = src + (int64_t)W * 3;
    int sr = 0, sg = 0, sb = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int t0 = src[3 * j], t1 = src[3 * j + 1], t2 = src[3 * j + 2];
        const int u0 = s1[3 * j], u1 = s1[3 * j + 1], u2 = s1[3 * j + 2];
        const int tr = RGB ? t0 : t2, tb = RGB ? t2 : t0, vr = RGB ? u0 : u2, vb = RGB ? u2 : u0;
        yp[j] = (uint8_t)luma(tr, t1, tb);
        yp[W + j] = (uint8_t)luma(vr, u1, vb);
        sr += tr + vr; sg += t1 + u1; sb += tb + vb;
    }
    *cb = (uint8_t)chroma_b(sr, sg, sb);
    *cr = (uint8_t)chroma_r(sr, sg, sb);
}

template <bool RGB, bool VEC>
__device__ __forceinline__ void mf_i420_item(const uint8_t* __restrict__ src, int W, uint8_t* __restrict__ yp, uint8_t* __restrict__ cb, uint8_t* __restrict__ cr) {
    if constexpr (VEC) mf_i420_strip<RGB>(src, W, yp, cb, cr);
    else mf_i420_block<RGB>(src, W, yp, cb, cr);
}

}  // namespace mf_i420
