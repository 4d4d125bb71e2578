// Packed uint8 frames -> planar YUV 4:2:0 (I420) on the device: the last per-pixel pass between the generator and the encoder.
//
// The serving loops end a step in packed uint8 [B][H][W][3] frames (BGR: Wav2Lip / MuseTalk after mf_paste_frames; RGB: ER-NeRF after mf_nerf_frame_out) and the
// consumer wraps each in `VideoFrame.from_ndarray(image, format="bgr24" | "rgb24")`; the encoder behind it converts every pixel to yuv420p on a host core.  This
// kernel writes what `VideoFrame.from_ndarray(a, format="yuv420p")` takes instead -- uint8 [H * 3 / 2][W] per frame: H rows of Y, the H/2 x W/2 Cb plane as
// bytes, then Cr -- so the ring and the D2H carry 1.5 bytes per pixel and the host pass is gone.  A separate launch on the finished block: k_paste_frames and
// mf_nerf_frame_out stay as they are.
//
// Arithmetic (the project's own definition; parity with libswscale is unpinned): BT.601 studio swing in 16.16 fixed point, chroma from the SUM of each 2 x 2 block,
//   Y  = (16829 R + 33039 G + 6416 B + (16 << 16) + 32768) >> 16
//   Cb = (-9714 Sr - 19070 Sg + 28784 Sb + (128 << 18) + (1 << 17)) >> 18          Sr, Sg, Sb = sums over the block, 0..1020
//   Cr = (28784 Sr - 24103 Sg -  4681 Sb + (128 << 18) + (1 << 17)) >> 18
// Every intermediate is positive and below 2^26: plain int32, the shifts are exact floors.  Both chroma rows sum to zero, so grey gives 128.
//
// Pure streaming, 3 B/px in, 1.5 B/px out, no reuse: no LDS, no scratch.  Two kernels that give the same bytes; the host picks one per call:
//   k_frames_to_i420<.., true>    a thread owns a 2-row strip of 8 pixels: 2 x 6 dword loads, two 8-byte Y stores, one dword of Cb, one of Cr.  Needs W % 8 == 0
//                                 and both base pointers 4-byte aligned (every row, plane and frame offset is then a multiple of 4)
//   k_frames_to_i420<.., false>   a thread owns one 2 x 2 block, byte loads and byte stores: every other even W, any alignment
// What a thread does with its strip or block is in mf_i420_px.h; the kernel here only says where the item lies in a contiguous block of frames.
#include "mf_common.h"
#include "mf_i420_px.h"                 // luma / chroma and the per-item bodies, shared with mf_frame_gather.hip

namespace {

using mf_i420::STRIP;
constexpr int THREADS = 256;

// frames [B][H][W][3] -> out [B][H * 3 / 2][W].  RGB: channel 0 is R (else B).  VEC: see the file comment.  `items` = B * (H / 2) * (W / (VEC ? 8 : 2)).
template <bool RGB, bool VEC>
__global__ __launch_bounds__(THREADS) void k_frames_to_i420(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int H, int W, int64_t items) {
    const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (g >= items) return;
    constexpr int PX = VEC ? STRIP : 2;
    const int gx = W / PX, hy = H >> 1;
    const int64_t row = g / gx;                                      // over B * H / 2 strip rows
    const int x = (int)(g - row * gx) * PX;
    const int64_t b = row / hy;
    const int y = (int)(row - b * hy) * 2;
    const int64_t plane = (int64_t)H * W;
    const uint8_t* src = frames + ((b * H + y) * W + x) * 3;
    uint8_t* yp = out + b * (plane + (plane >> 1)) + (int64_t)y * W + x;
    uint8_t* cb = out + b * (plane + (plane >> 1)) + plane + (int64_t)(y >> 1) * (W >> 1) + (x >> 1);
    uint8_t* cr = cb + (plane >> 2);
    mf_i420::mf_i420_item<RGB, VEC>(src, W, yp, cb, cr);
}

template <bool RGB, bool VEC>
int launch(const uint8_t* frames, uint8_t* out, int n_frames, int H, int W, hipStream_t s) {
    const int64_t items = (int64_t)n_frames * (H / 2) * (W / (VEC ? STRIP : 2));
    const int64_t blocks = (items + THREADS - 1) / THREADS;
    MF_REQUIRE(blocks <= 0x7fffffffLL, "frames_to_i420: %d frames of %d x %d are more than one launch holds", n_frames, W, H);
    hipLaunchKernelGGL((k_frames_to_i420<RGB, VEC>), dim3((unsigned)blocks), dim3(THREADS), 0, s, frames, out, H, W, items);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

}  // namespace

extern "C" int mf_frames_to_i420(const uint8_t* frames, int n_frames, int H, int W, int rgb_order, uint8_t* out, void* stream) {
    MF_REQUIRE(frames, "frames_to_i420: frames is a null pointer");
    MF_REQUIRE(out, "frames_to_i420: out is a null pointer");
    MF_REQUIRE(n_frames >= 1, "frames_to_i420: n_frames %d (at least one frame)", n_frames);
    MF_REQUIRE(H > 0 && W > 0, "frames_to_i420: frame size %d x %d (H x W) must be positive", H, W);
    MF_REQUIRE(H % 2 == 0, "frames_to_i420: H %d is odd (4:2:0 chroma covers 2 x 2 blocks)", H);
    MF_REQUIRE(W % 2 == 0, "frames_to_i420: W %d is odd (4:2:0 chroma covers 2 x 2 blocks)", W);
    MF_REQUIRE(rgb_order == 0 || rgb_order == 1, "frames_to_i420: rgb_order %d (0: BGR, 1: RGB)", rgb_order);
    hipStream_t s = (hipStream_t)stream;
    // one path per call, chosen here: the strip path needs whole strips per row and dword-aligned bases
    const bool vec = W % STRIP == 0 && (((uintptr_t)frames | (uintptr_t)out) & 3u) == 0;
    if (vec) return rgb_order ? launch<true, true>(frames, out, n_frames, H, W, s) : launch<false, true>(frames, out, n_frames, H, W, s);
    return rgb_order ? launch<true, false>(frames, out, n_frames, H, W, s) : launch<false, false>(frames, out, n_frames, H, W, s);
}
