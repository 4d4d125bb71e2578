// Finished frames from anywhere into chosen frames of one block, packed or as I420: what a serving step shows while a session LISTENS.
//
// Wav2Lip's and MuseTalk's consumers show, for every frame whose two audio chunks carry no speech, the avatar's cached full frame or a frame of a custom video
// (lipreal.py:198-205, musereal.py:229-236) -- picked on the host, in the packed format only.  Here those frames leave through the same ring as the generated
// ones: one launch takes up to 64 source frames -- each a device pointer to a contiguous uint8 [H][W][3] image: a row of an avatar's frame cache, a frame of a
// custom cycle in another allocation -- and writes each into frame `dst` of `out`, as it is (format 0) or converted (format 1: the bytes mf_frames_to_i420 writes
// for the same pixels; the per-item bodies are mf_i420_px.h's, shared with that file).  Frames of `out` that no source names are not touched: the scheduler
// overwrites single frames of a block the paste-back has filled.
//
// The source table travels BY VALUE in the launch arguments (64 x 16 bytes): no handle, no allocation, no upload, nothing to keep alive behind the call.  The
// frame is blockIdx.y, so no work item straddles two frames and the table is read with a wave-uniform index.  Pure streaming: no LDS, no scratch.
//   k_gather_i420<.., true>    2 rows x 8 pixels per thread, as k_frames_to_i420<.., true>: needs W % 8 == 0, `out` and EVERY source 4-byte aligned
//   k_gather_i420<.., false>   one 2 x 2 block per thread, byte accesses: every other even W, any alignment
//   k_gather_copy<true>        16 bytes per thread as four dwords (the last thread of a frame: the up to three dwords left): needs H * W * 3 % 4 == 0 and the
//                              same alignment
//   k_gather_copy<false>       4 bytes per thread, one at a time: any size (odd H and W too), any alignment
// The path is chosen once per call, over all sources, so a call's launches agree.
#include "mf_common.h"
#include "mf_i420_px.h"
#include <algorithm>
#include <utility>
#include <vector>

namespace {

using mf_i420::STRIP;
constexpr int THREADS = 256;
constexpr int TABLE = 64;          // sources per launch; a longer list goes out as several launches

struct GatherEntry { const uint8_t* frame; int64_t dst_off; };       // dst_off: where frame `dst` starts in `out`, in bytes
struct GatherTable { GatherEntry e[TABLE]; };

// one frame per blockIdx.y; `items` = (H / 2) * (W / (VEC ? 8 : 2)) work items per frame
template <bool RGB, bool VEC>
__global__ __launch_bounds__(THREADS) void k_gather_i420(const GatherTable tab, uint8_t* __restrict__ out, int H, int W, int64_t items) {
    const int64_t g = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (g >= items) return;
    const GatherEntry e = tab.e[blockIdx.y];
    constexpr int PX = VEC ? STRIP : 2;
    const int gx = W / PX;
    const int64_t row = g / gx;                                      // over H / 2 strip rows
    const int x = (int)(g - row * gx) * PX;
    const int y = (int)row * 2;
    const int64_t plane = (int64_t)H * W;
    const uint8_t* src = e.frame + ((int64_t)y * W + x) * 3;
    uint8_t* yp = out + e.dst_off + (int64_t)y * W + x;
    uint8_t* cb = out + e.dst_off + plane + (int64_t)(y >> 1) * (W >> 1) + (x >> 1);
    uint8_t* cr = cb + (plane >> 2);
    mf_i420::mf_i420_item<RGB, VEC>(src, W, yp, cb, cr);
}

struct __attribute__((aligned(4))) Bytes16 { uint32_t a, b, c, d; };  // a 16-byte access that only needs dword alignment

// one frame of `bytes` bytes per blockIdx.y.  VEC: thread g owns bytes [16 g, 16 g + 16) (bytes % 4 == 0); else [4 g, 4 g + 4), cut at the frame's end
template <bool VEC>
__global__ __launch_bounds__(THREADS) void k_gather_copy(const GatherTable tab, uint8_t* __restrict__ out, int64_t bytes) {
    constexpr int PER = VEC ? 16 : 4;
    const int64_t off = ((int64_t)blockIdx.x * THREADS + threadIdx.x) * PER;
    if (off >= bytes) return;
    const GatherEntry e = tab.e[blockIdx.y];
    const uint8_t* src = e.frame + off;
    uint8_t* dst = out + e.dst_off + off;
    if constexpr (VEC) {
        if (off + 16 <= bytes) {
            *reinterpret_cast<Bytes16*>(dst) = *reinterpret_cast<const Bytes16*>(src);
        } else {
            const int left = (int)(bytes - off) >> 2;                // 1..3 dwords
            for (int i = 0; i < left; ++i) reinterpret_cast<uint32_t*>(dst)[i] = reinterpret_cast<const uint32_t*>(src)[i];
        }
    } else {
        const int left = (int)(bytes - off < 4 ? bytes - off : 4);
        for (int i = 0; i < left; ++i) dst[i] = src[i];
    }
}

template <bool RGB, bool VEC>
void launch_i420(const GatherTable& tab, int n, uint8_t* out, int H, int W, unsigned blocks, int64_t items, hipStream_t s) {
    hipLaunchKernelGGL((k_gather_i420<RGB, VEC>), dim3(blocks, (unsigned)n), dim3(THREADS), 0, s, tab, out, H, W, items);
}

}  // namespace

extern "C" int mf_frames_gather(const mf_frame_src* srcs, int n, int H, int W, int format, int rgb_order, uint8_t* out, int out_frames, void* stream) {
    MF_REQUIRE(srcs, "frames_gather: srcs is a null pointer");
    MF_REQUIRE(out, "frames_gather: out is a null pointer");
    MF_REQUIRE(n >= 1, "frames_gather: n %d (at least one source frame)", n);
    MF_REQUIRE(out_frames >= 1, "frames_gather: out_frames %d (at least one frame)", out_frames);
    MF_REQUIRE(H > 0 && W > 0, "frames_gather: frame size %d x %d (H x W) must be positive", H, W);
    MF_REQUIRE(format == 0 || format == 1, "frames_gather: format %d (0: packed, 1: I420)", format);
    MF_REQUIRE(rgb_order == 0 || rgb_order == 1, "frames_gather: rgb_order %d (0: BGR, 1: RGB)", rgb_order);
    if (format == 1) {
        MF_REQUIRE(H % 2 == 0, "frames_gather: H %d is odd (4:2:0 chroma covers 2 x 2 blocks)", H);
        MF_REQUIRE(W % 2 == 0, "frames_gather: W %d is odd (4:2:0 chroma covers 2 x 2 blocks)", W);
    }
    const int64_t src_bytes = (int64_t)H * W * 3;
    const int64_t dst_bytes = format ? src_bytes / 2 : src_bytes;    // one frame of `out`
    uintptr_t align = (uintptr_t)out;
    std::vector<std::pair<int, int>> by_dst(n);                      // (dst, source number)
    for (int i = 0; i < n; ++i) {
        MF_REQUIRE(srcs[i].frame, "frames_gather: source %d: frame is a null pointer", i);
        MF_REQUIRE(srcs[i].dst >= 0 && srcs[i].dst < out_frames, "frames_gather: source %d: dst %d is outside [0, %d)", i, srcs[i].dst, out_frames);
        // (a source inside the block it is gathered into would be read while another item writes it)
        const uintptr_t a = (uintptr_t)srcs[i].frame, o = (uintptr_t)out;
        MF_REQUIRE(a + (uintptr_t)src_bytes <= o || o + (uintptr_t)dst_bytes * (uintptr_t)out_frames <= a, "frames_gather: source %d lies inside out", i);
        align |= a;
        by_dst[i] = {srcs[i].dst, i};
    }
    std::sort(by_dst.begin(), by_dst.end());
    for (int i = 1; i < n; ++i)                                       // two writers of one frame: a race within a launch
        MF_REQUIRE(by_dst[i].first != by_dst[i - 1].first, "frames_gather: sources %d and %d both name dst %d", by_dst[i - 1].second, by_dst[i].second, by_dst[i].first);
    const bool aligned = (align & 3u) == 0;
    const bool vec = aligned && (format ? W % STRIP == 0 : src_bytes % 4 == 0);
    const int64_t items = format ? (int64_t)(H / 2) * (W / (vec ? STRIP : 2)) : (src_bytes + (vec ? 15 : 3)) / (vec ? 16 : 4);     // per frame
    const int64_t blocks = (items + THREADS - 1) / THREADS;
    MF_REQUIRE(blocks <= 0x7fffffffLL, "frames_gather: a frame of %d x %d is more than one launch holds", W, H);
    hipStream_t s = (hipStream_t)stream;
    GatherTable tab;
    for (int first = 0; first < n; first += TABLE) {
        const int cnt = std::min(TABLE, n - first);
        for (int i = 0; i < TABLE; ++i) {                             // (entries behind cnt repeat the last one: never read, never garbage)
            const mf_frame_src& d = srcs[first + std::min(i, cnt - 1)];
            tab.e[i] = GatherEntry{d.frame, (int64_t)d.dst * dst_bytes};
        }
        if (format == 0) {
            if (vec) hipLaunchKernelGGL(k_gather_copy<true>, dim3((unsigned)blocks, (unsigned)cnt), dim3(THREADS), 0, s, tab, out, src_bytes);
            else hipLaunchKernelGGL(k_gather_copy<false>, dim3((unsigned)blocks, (unsigned)cnt), dim3(THREADS), 0, s, tab, out, src_bytes);
        } else if (vec) {
            if (rgb_order) launch_i420<true, true>(tab, cnt, out, H, W, (unsigned)blocks, items, s);
            else launch_i420<false, true>(tab, cnt, out, H, W, (unsigned)blocks, items, s);
        } else {
            if (rgb_order) launch_i420<true, false>(tab, cnt, out, H, W, (unsigned)blocks, items, s);
            else launch_i420<false, false>(tab, cnt, out, H, W, (unsigned)blocks, items, s);
        }
        MF_HIP(hipGetLastError());
    }
    return MF_OK;
}
