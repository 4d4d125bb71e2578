// The two ends of one `nerfreal.py` frame (test_step, nerfreal.py:70-127) that sit either side of the ER-NeRF render, on the device:
//
//   k_nerf_frame_background   `NeRFDataset_Test.collate`, provider.py:316-330: the frame's RGBA torso image over the background -> bg_color
//   k_nerf_frame_out          `Trainer.test_gui_with_data`'s resize (utils.py:1208-1212), `(image * 255).astype(np.uint8)` (nerfreal.py:110), the
//                             --fullbody paste with its cvtColor (nerfreal.py:117-122) and the custom-video frame (nerfreal.py:98-107)
//
// Both are one lane per pixel and bandwidth-bound: 4 + 12 B read and 12 B written per pixel for the background, 3 B written (and 3 B of body frame or up to
// 48 B of render taps, mostly shared between neighbours, read) per pixel for the frame.
//
// The background must give the BITS of the torch expression it replaces, so this file is compiled with floating-point contraction OFF: hipcc contracts
// a * b + c into an FMA by default, and __fmul_rn / __fadd_rn are plain operators in this toolchain's headers (they would fuse all the same).  With the
// pragma every +, -, *, / below rounds once, as written; divisions are the correctly rounded default of hipcc.
#include "mf_common.h"
#include "mf_nerf_frame.h"
#include "mf_nerf_frame_batch.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;

// torch's half elementwise ops: operands widened to fp32, the operation rounded to fp32, the result rounded to half (nearest even)
__device__ __forceinline__ float as_half(float v) { return (float)(_Float16)v; }

// bg_color = rgb * a + bg * (1 - a), provider.py:323.  HALF false: the fp32 tensors of preload 0 / 1 (`astype(np.float32) / 255`, provider.py:186, 212, 321).
// HALF true: preload 2, where torso_img and bg_img are half tensors (provider.py:198, 238): every operand and every one of the four operations is rounded to
// half, and the result widened (the render casts bg_color to fp32).
struct __attribute__((packed, aligned(4))) Rgb32 { float v[3]; };      // 12 bytes, moved as one dwordx3

// one pixel of the frame; the single-frame kernel and the frame-indexed one are this function and nothing else
template <bool HALF>
__device__ __forceinline__ void nerf_background_pixel(const uchar4* __restrict__ torso, const Rgb32* __restrict__ bg, float bg_const, int i, Rgb32* __restrict__ out) {
    const uchar4 px = torso[i];
    const Rgb32 b3 = bg ? bg[i] : Rgb32{{bg_const, bg_const, bg_const}};
    const float c[3] = {(float)px.x / 255.f, (float)px.y / 255.f, (float)px.z / 255.f};
    const float a = (float)px.w / 255.f;
    Rgb32 o;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float b = b3.v[k];
        if (HALF) {
            const float ah = as_half(a);
            o.v[k] = as_half(as_half(as_half(c[k]) * ah) + as_half(as_half(b) * as_half(1.f - ah)));
        } else {
            o.v[k] = c[k] * a + b * (1.f - a);
        }
    }
    out[i] = o;
}

template <bool HALF>
__global__ __launch_bounds__(NT) void k_nerf_frame_background(const uchar4* __restrict__ torso, const Rgb32* __restrict__ bg, float bg_const, int n,
                                                              Rgb32* __restrict__ out) {
    const int i = threadIdx.x + blockIdx.x * NT;
    if (i >= n) return;
    nerf_background_pixel<HALF>(torso, bg, bg_const, i, out);
}

// the frame in blockIdx.y: every frame has its own ceil(n / NT) workgroups, the last one partial
__global__ __launch_bounds__(NT) void k_nerf_frame_background_batch(const NerfBgFrame* __restrict__ frames, int n) {
    const int i = threadIdx.x + blockIdx.x * NT;
    if (i >= n) return;
    const NerfBgFrame f = frames[blockIdx.y];
    if (f.half) nerf_background_pixel<true>((const uchar4*)f.torso, (const Rgb32*)f.bg, f.bg_const, i, (Rgb32*)f.out);
    else nerf_background_pixel<false>((const uchar4*)f.torso, (const Rgb32*)f.bg, f.bg_const, i, (Rgb32*)f.out);
}

// utils.py:78-81.  The power goes through double and is rounded once: ocml's fp32 powf carries packed-fp32 forms the library's ISA scan refuses (mf_common.h
// mf_opaque).  Out of line: the twelve calls per output pixel (four taps x three channels, converted in front of the blend as utils.py:1208-1212 orders it) share one
// body.  That is twelve double-precision pows per pixel whenever color_space == 'linear' (DESIGN section 6 states the cost).  The exponent is the fp32 value torch's
// pow receives.
__device__ __noinline__ float linear_to_srgb(float x) {
    return x < 0.0031308f ? 12.92f * x : 1.055f * (float)pow((double)x, (double)0.41666f) - 0.055f;
}

// One lane per pixel of the [FH, FW] output.  Inside the [H, W] rectangle at (x0, y0): the render resized to the GUI size and converted, through the
// device functions k_nerf_resize uses (mf_nerf_frame.h).  Outside it, and everywhere when there is no render: the body pixel, BGR -> RGB.
__device__ __forceinline__ void nerf_frame_out_pixel(const float* __restrict__ render, int h, int w, int H, int W, const uint8_t* __restrict__ body, int FW, int x0,
                                                     int y0, int srgb, int i, uint8_t* __restrict__ out) {
    const int fy = i / FW, fx = i - fy * FW;
    const int oy = fy - y0, ox = fx - x0;
    uint8_t* o = out + (size_t)i * 3;
    if (render && oy >= 0 && oy < H && ox >= 0 && ox < W) {
        const NerfBilinearTaps t = nerf_bilinear_taps(oy, ox, h, w, H, W);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float p00 = render[((size_t)t.y0 * w + t.x0) * 3 + k], p01 = render[((size_t)t.y0 * w + t.x1) * 3 + k];
            float p10 = render[((size_t)t.y1 * w + t.x0) * 3 + k], p11 = render[((size_t)t.y1 * w + t.x1) * 3 + k];
            if (srgb) { p00 = linear_to_srgb(p00); p01 = linear_to_srgb(p01); p10 = linear_to_srgb(p10); p11 = linear_to_srgb(p11); }
            o[k] = nerf_frame_u8(nerf_bilinear_blend(t, p00, p01, p10, p11));
        }
    } else {
        const uint8_t* b = body + (size_t)i * 3;
        const uint8_t b0 = b[0], b1 = b[1], b2 = b[2];
        o[0] = b2; o[1] = b1; o[2] = b0;
    }
}

__global__ __launch_bounds__(NT) void k_nerf_frame_out(const float* __restrict__ render, int h, int w, int H, int W, const uint8_t* __restrict__ body, int FH,
                                                       int FW, int x0, int y0, int srgb, uint8_t* __restrict__ out) {
    const int i = threadIdx.x + blockIdx.x * NT;
    if (i >= FH * FW) return;
    nerf_frame_out_pixel(render, h, w, H, W, body, FW, x0, y0, srgb, i, out);
}

// the frame in blockIdx.y; frame f writes out[f][FH][FW][3]
__global__ __launch_bounds__(NT) void k_nerf_frame_out_batch(const NerfOutFrame* __restrict__ frames, int h, int w, int H, int W, int FH, int FW, int srgb,
                                                             uint8_t* __restrict__ out) {
    const int i = threadIdx.x + blockIdx.x * NT;
    if (i >= FH * FW) return;
    const NerfOutFrame f = frames[blockIdx.y];
    nerf_frame_out_pixel(f.render, h, w, H, W, f.body, FW, f.x0, f.y0, srgb, i, out + (size_t)blockIdx.y * FH * FW * 3);
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + NT - 1) / NT); }

}  // namespace

// the callers (mf_nerf_frame_batch.hip) have checked the sizes and every frame's pointers
int mf_nerf_frame_background_batch_launch(const NerfBgFrame* tab_dev, int n_frames, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_nerf_frame_background_batch, dim3(blocks(n), (unsigned)n_frames), dim3(NT), 0, s, tab_dev, n);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

int mf_nerf_frame_out_batch_launch(const NerfOutFrame* tab_dev, int n_frames, int h, int w, int H, int W, int FH, int FW, int srgb, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_nerf_frame_out_batch, dim3(blocks((int64_t)FH * FW), (unsigned)n_frames), dim3(NT), 0, s, tab_dev, h, w, H, W, FH, FW, srgb, out);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_nerf_frame_background(const uint8_t* torso_rgba, const float* bg_image, float bg_const, int H, int W, int half_mode, float* bg_color,
                                        void* stream) {
    MF_REQUIRE(torso_rgba && bg_color && H > 0 && W > 0, "nerf_frame_background: bad argument");
    MF_REQUIRE((int64_t)H * W < (1ll << 31), "nerf_frame_background: frame too large");
    MF_REQUIRE(((uintptr_t)torso_rgba & 3) == 0, "nerf_frame_background: the RGBA image must be 4-byte aligned");
    const int n = H * W;
    if (half_mode)
        hipLaunchKernelGGL(k_nerf_frame_background<true>, dim3(blocks(n)), dim3(NT), 0, (hipStream_t)stream, (const uchar4*)torso_rgba, (const Rgb32*)bg_image, bg_const, n, (Rgb32*)bg_color);
    else
        hipLaunchKernelGGL(k_nerf_frame_background<false>, dim3(blocks(n)), dim3(NT), 0, (hipStream_t)stream, (const uchar4*)torso_rgba, (const Rgb32*)bg_image, bg_const, n, (Rgb32*)bg_color);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_nerf_frame_out(const float* render, int h, int w, int H, int W, const uint8_t* body_bgr, int FH, int FW, int x0, int y0, int linear_to_srgb,
                                 uint8_t* frame_rgb, void* stream) {
    MF_REQUIRE(frame_rgb && (render || body_bgr), "nerf_frame_out: no output, or neither a render nor a body frame");
    if (render) MF_REQUIRE(h > 0 && w > 0 && H > 0 && W > 0, "nerf_frame_out: render %d x %d to %d x %d", w, h, W, H);
    if (!body_bgr) {
        MF_REQUIRE(x0 == 0 && y0 == 0, "nerf_frame_out: an offset (%d, %d) without a body frame", x0, y0);
        FH = H; FW = W;
    }
    MF_REQUIRE(FH > 0 && FW > 0 && (int64_t)FH * FW < (1ll << 31), "nerf_frame_out: body frame %d x %d", FW, FH);
    if (render) {
        // nerfreal.py:122: the slice assignment raises when the frame does not fit; nothing is clipped
        MF_REQUIRE(x0 >= 0 && y0 >= 0 && (int64_t)x0 + W <= FW && (int64_t)y0 + H <= FH,
                   "nerf_frame_out: a %d x %d frame at (%d, %d) leaves the %d x %d body frame", W, H, x0, y0, FW, FH);
        MF_REQUIRE((int64_t)h * w < (1ll << 31), "nerf_frame_out: render too large");
    }
    hipLaunchKernelGGL(k_nerf_frame_out, dim3(blocks((int64_t)FH * FW)), dim3(NT), 0, (hipStream_t)stream, render, h, w, H, W, body_bgr, FH, FW, x0, y0,
                       linear_to_srgb, frame_rgb);
    MF_HIP(hipGetLastError());
    return MF_OK;
}
