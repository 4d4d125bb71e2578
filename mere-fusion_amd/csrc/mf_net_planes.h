// The (hi, lo) bf16 planes of an mf_net buffer as the elementwise kernels see them, and the one sampling function two kernels must agree on bit for bit:
// k_bilinear_ac (mf_net.hip, the fp32 output of the parser) and k_fm_argmax_mask (mf_face_mask.hip, the same interpolation ending in a class mask).
#pragma once
#include "mf_conv.h"

namespace {

__device__ __forceinline__ float nbf(uint32_t h16) { return __uint_as_float(h16 << 16); }
struct Pl {   // one buffer's geometry for the elementwise kernels
    bf16_t* hi; bf16_t* lo; int C, H, W, halo;
    __device__ int64_t at(int b, int y, int x) const { return (((int64_t)b * (H + 2 * halo) + y + halo) * (W + 2 * halo) + x + halo) * C; }
    __device__ float ld(int64_t o) const { float v = nbf(hi[o]); if (lo) v += nbf(lo[o]); return v; }
    __device__ void st(int64_t o, float v) const { unsigned h, l; mf_split_bf16(v, h, l); hi[o] = (bf16_t)h; if (lo) lo[o] = (bf16_t)l; }
};
inline Pl pl_of(const ActBuf& b) { return Pl{b.hi, b.lo, b.C, b.H, b.W, b.halo}; }

// F.interpolate(x, (H, W), mode='bilinear', align_corners=True) at output pixel (y, x): aten's upsample_bilinear2d, scale = (in - 1) / (out - 1), src = scale * dst,
// lambda in fp32.  The corner geometry is the same for every channel of a pixel, so it is split off.
struct BilinearAc { int y0, y1, x0, x1; float ly, lx, hy, hx; };
__device__ __forceinline__ BilinearAc bilinear_ac_corners(const Pl& X, int y, int x, float sh, float sw) {
    BilinearAc g;
    const float fy = sh * y, fx = sw * x;
    g.y0 = (int)fy; g.x0 = (int)fx;
    g.y1 = g.y0 + (g.y0 < X.H - 1 ? 1 : 0); g.x1 = g.x0 + (g.x0 < X.W - 1 ? 1 : 0);
    g.ly = fy - g.y0; g.lx = fx - g.x0; g.hy = 1.f - g.ly; g.hx = 1.f - g.lx;
    return g;
}
// Both callers compile this expression under the build's default floating-point contraction (neither file-scope pragma reaches into it: mf_face_mask.hip
// switches contraction off per function, not per file); tests/test_face_mask.py holds the two kernels bit-equal on the device.
__device__ __forceinline__ float bilinear_ac_sample(const Pl& X, const BilinearAc& g, int b, int c) {
    const float v00 = X.ld(X.at(b, g.y0, g.x0) + c), v01 = X.ld(X.at(b, g.y0, g.x1) + c);
    const float v10 = X.ld(X.at(b, g.y1, g.x0) + c), v11 = X.ld(X.at(b, g.y1, g.x1) + c);
    return g.hy * (g.hx * v00 + g.lx * v01) + g.ly * (g.hx * v10 + g.lx * v11);
}

}  // namespace
