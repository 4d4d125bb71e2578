// The sampling arithmetic of `test_gui_with_data`'s resize (utils.py:1212: F.interpolate(mode='bilinear'), align_corners False) and the float -> uint8
// conversion of nerfreal.py:110, stated ONCE for the two kernels that use them: k_nerf_resize (mf_nerf.hip) and k_nerf_frame_out (mf_nerf_frame.hip).
// Both must give the same bits for the same render, so neither restates it.  Contraction is switched off inside each function (the including file's
// own setting does not reach a header included above its pragma): +, -, * round exactly as written; the one fused operation is the explicit fmaf.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

struct NerfBilinearTaps {
    int y0, x0, y1, x1;
    float ly0, ly1, lx0, lx1;
};

// Half-pixel centres: src = max((dst + 0.5) * in / out - 0.5, 0), weights (1 - l, l); the neighbour index stops at the last row / column.
__device__ __forceinline__ NerfBilinearTaps nerf_bilinear_taps(int oy, int ox, int h, int w, int H, int W) {
#pragma clang fp contract(off)
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    float fy = fmaf(sy, (float)oy + 0.5f, -0.5f), fx = fmaf(sx, (float)ox + 0.5f, -0.5f);     // fused, as aten's builds contract it
    fy = fy < 0.f ? 0.f : fy; fx = fx < 0.f ? 0.f : fx;
    NerfBilinearTaps t;
    t.y0 = (int)fy; t.x0 = (int)fx;
    t.y1 = t.y0 + (t.y0 < h - 1 ? 1 : 0); t.x1 = t.x0 + (t.x0 < w - 1 ? 1 : 0);
    t.ly1 = fy - (float)t.y0; t.ly0 = 1.f - t.ly1; t.lx1 = fx - (float)t.x0; t.lx0 = 1.f - t.lx1;
    return t;
}

// The row blend of two column blends, as aten's upsample_bilinear2d forms it.
__device__ __forceinline__ float nerf_bilinear_blend(const NerfBilinearTaps& t, float p00, float p01, float p10, float p11) {
#pragma clang fp contract(off)
    return t.ly0 * (t.lx0 * p00 + t.lx1 * p01) + t.ly1 * (t.lx0 * p10 + t.lx1 * p11);
}

// (image * 255).astype(np.uint8): the product rounded to fp32, then truncated
__device__ __forceinline__ uint8_t nerf_frame_u8(float v) {
#pragma clang fp contract(off)
    return (uint8_t)(v * 255.f);
}
