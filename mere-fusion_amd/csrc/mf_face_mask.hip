// MuseTalk's blend masks on the device: what FaceParsing.__call__ (musetalk/utils/face_parsing/__init__.py:34-51), face_seg (musetalk/utils/blending.py:17-24) and
// get_image_prepare_material (blending.py:62-86) do on the host around the BiSeNet graph, once per avatar frame.
//
//   k_fm_tables        Pillow's resampling tables (Resample.c precompute_coeffs + normalize_coeffs_8bpc): per output index (xmin, n, kk[n]), float64, then
//                      kk = (int)(k * 2^22 +- 0.5).  Bilinear (support 1) and bicubic (a = -0.5, support 2); filter scale max(1, in / out); weights normalised by
//                      the window's sum.
//   k_fm_pass_h        horizontal pass of Image.resize for 8-bit pixels: integer multiply-accumulate, (acc + 2^21) >> 22 clipped to 0..255, to a uint8 intermediate.
//                      The source is a crop box of a larger frame; pixels of the box outside the frame read 0 (Image.crop pads with black); the channel reversal of
//                      `image[:, :, ::-1]` is an index.
//   k_fm_pass_v        vertical pass, with one of two endings: ToTensor + Normalize straight into the parser's input planes (face_parsing/__init__.py:29-33);
//                      uint8 under the window of blending.py:74-82 (outside the face box and above top_boundary the mask is 0).
//   k_fm_argmax_mask   `out = net(img)[0]; parsing = out.argmax(0); parsing[parsing > 13] = 0; parsing[parsing >= 1] = 255` in one pass over the head buffer: the
//                      align_corners bilinear upsampling of mf_net_get_output_bilinear (the same device function), first maximum wins as in numpy; the fp32
//                      [19, 512, 512] tensor is never written.
//   k_fm_blur_taps, k_fm_blur_h / _v   cv2.GaussianBlur(mask, (k, k), 0), k = int(0.1 * width // 2 * 2) + 1 (blending.py:84-85), restated from the published algorithm:
//                      sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8, taps exp(-(i - (k - 1) / 2)^2 / (2 sigma^2)) normalised to sum 1 (computed in float64 once per job by k_fm_blur_taps, used in
//                      fp32), BORDER_REFLECT_101, separable, fp32 between the passes, ONE rounding at the end (half to even).  OpenCV's own 8-bit path may quantise
//                      its kernel to fixed point and round between the passes; OpenCV is not installed where this was written, so nobody could compare against it
//                      here.  The tests hold this kernel to a float64 evaluation of the formulas above, not to OpenCV.
//
// Where the tables are computed.  Pillow computes them on the host in float64.  Here a kernel does, in float64 with contraction off: additions, multiplications,
// divisions and conversions are IEEE operations on both sides, so the integers are the same (tests: 0 differing pixels against Pillow), and the tables reach the device
// without a host-to-device copy -- a copy from pageable memory would block the calling thread, and nothing in this file synchronises with the host.
//
// An axis whose size does not change: Pillow skips the pass.  The horizontal pass is skipped here too (the vertical pass then reads the frame's box directly).  The
// vertical pass carries the ending, so it always runs; for an unchanged axis its table is (xmin = i, n = 1, kk = 2^22) and (v * 2^22 + 2^21) >> 22 == v.
//
// One launch serves up to MF_FM_MAX_JOBS jobs of different sizes (descriptors as kernel arguments, like k_paste_frames); more jobs go out as more launches.
#include "mf_aux.h"
#include "mf_net_planes.h"
#include <cmath>

#define MF_FM_MAX_JOBS 16
#define MF_FM_MAX_TAPS 64                    // per output pixel of a resampling table: ceil(support * in / out) * 2 + 1
#define MF_FM_BLUR_MAX_K 151                 // what the LDS tiles of the blur hold
#define MF_FM_BLUR_R (MF_FM_BLUR_MAX_K / 2)
#define MF_FM_BLUR_TAP_STRIDE 152             // floats per job in the workspace's tap area
#define MF_FM_BLUR_TW 256                    // horizontal pass: outputs per workgroup (one row segment)
#define MF_FM_BLUR_VC 64                     // vertical pass: columns per workgroup ...
#define MF_FM_BLUR_VR 32                     // ... and rows
#define MF_FM_PRECISION_BITS 22

namespace {

struct FmAxis { int in, out, taps, off; };   // off: int index of this table in the table area: [out][2] bounds, then [out][taps] coefficients

struct FmJob {
    int src;                                 // index of the source image
    int bx, by, bw, bh;                      // the box of the source that is resampled (may leave the source: zeros)
    FmAxis ax, ay;
    int skip_h;
    int slot;                                // batch slot of the parser input | unused
    int rx0, ry0, rx1, ry1, top;             // window of the mask-back pass
    int64_t inter, out;                      // byte offsets: uint8 intermediate [bh][ax.out][C] in the workspace, uint8 output [ay.out][ax.out][C]
};

struct FmArgs {
    const uint8_t* src; int SH, SW, rev;     // source images [n][SH][SW][C]
    int filter;                              // 0 bilinear, 1 bicubic
    int* tab; uint8_t* inter; uint8_t* out;
    bf16_t* hi; bf16_t* lo; int halo, NH, NW;   // the parser's input planes (8 channels)
    float mean[3], std[3];
    int n_jobs;
    FmJob job[MF_FM_MAX_JOBS];
};

// ---- tables ---------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double fm_filter(int filter, double x) {
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    if (filter == 0) return x < 1.0 ? 1.0 - x : 0.0;
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

__device__ void fm_table_row(int filter, const FmAxis A, int* __restrict__ tab, int xx) {
#pragma clang fp contract(off)
    int* bounds = tab + A.off + 2 * xx;
    int* kk = tab + A.off + 2 * A.out + (int64_t)xx * A.taps;
    if (A.in == A.out) {                      // (the pass Pillow skips)
        bounds[0] = xx; bounds[1] = 1;
        kk[0] = 1 << MF_FM_PRECISION_BITS;
        for (int x = 1; x < A.taps; ++x) kk[x] = 0;
        return;
    }
    const double scale = (double)((float)A.in - 0.f) / A.out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (filter == 0 ? 1.0 : 2.0) * filterscale;
    const double center = 0.0 + (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > A.in) xmax = A.in;
    xmax -= xmin;
    if (xmax > A.taps) xmax = A.taps;         // cannot happen (taps = ceil(support) * 2 + 1); keeps every store inside the row
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += fm_filter(filter, (x + xmin - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
        double w = fm_filter(filter, (x + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        kk[x] = w < 0 ? (int)(-0.5 + w * (1 << MF_FM_PRECISION_BITS)) : (int)(0.5 + w * (1 << MF_FM_PRECISION_BITS));
    }
    for (int x = xmax; x < A.taps; ++x) kk[x] = 0;
    bounds[0] = xmin; bounds[1] = xmax;
}

// grid (rows of 256 output indices, 2 * jobs): blockIdx.y = 2 * job + axis
__global__ __launch_bounds__(256) void k_fm_tables(const FmArgs a) {
    const FmJob& j = a.job[blockIdx.y >> 1];
    const FmAxis A = (blockIdx.y & 1) ? j.ay : j.ax;
    const int xx = blockIdx.x * 256 + threadIdx.x;
    if (xx >= A.out) return;
    fm_table_row(a.filter, A, a.tab, xx);
}

// ---- passes -----------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> MF_FM_PRECISION_BITS, 0), 255); }

// channel c of pixel (x, y) of the job's box; outside the source image: 0
template <int C>
__device__ __forceinline__ int fm_box_px(const FmArgs& a, const FmJob& j, int x, int y, int c) {
    const int sx = x + j.bx, sy = y + j.by;
    if (sx < 0 || sy < 0 || sx >= a.SW || sy >= a.SH) return 0;
    return a.src[(((int64_t)j.src * a.SH + sy) * a.SW + sx) * C + (a.rev ? C - 1 - c : c)];
}

// grid (pixel groups, jobs): one thread = one pixel of the intermediate [bh][ax.out][C]
template <int C>
__global__ __launch_bounds__(256) void k_fm_pass_h(const FmArgs a) {
    const FmJob& j = a.job[blockIdx.y];
    if (j.skip_h) return;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int ow = j.ax.out;
    if (idx >= (int64_t)j.bh * ow) return;
    const int y = (int)(idx / ow), x = (int)(idx % ow);
    const int xmin = a.tab[j.ax.off + 2 * x], n = a.tab[j.ax.off + 2 * x + 1];
    const int* kk = a.tab + j.ax.off + 2 * ow + (int64_t)x * j.ax.taps;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (MF_FM_PRECISION_BITS - 1);
    for (int t = 0; t < n; ++t) {
        const int k = kk[t];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += fm_box_px<C>(a, j, xmin + t, y, c) * k;
    }
    uint8_t* d = a.inter + j.inter + idx * C;
#pragma unroll
    for (int c = 0; c < C; ++c) d[c] = (uint8_t)clip8(acc[c]);
}

__device__ __forceinline__ float fm_normalize(int u8, float mean, float std) {
#pragma clang fp contract(off)
    return ((float)u8 / 255.f - mean) / std;   // ToTensor's `.div(255)`, then Normalize's `.sub_(mean).div_(std)`: three rounded fp32 operations
}

enum { FM_END_NET = 0, FM_END_WINDOW = 1 };

// grid (pixel groups, jobs): one thread = one output pixel [ay.out][ax.out]
template <int C, int END>
__global__ __launch_bounds__(256) void k_fm_pass_v(const FmArgs a) {
    const FmJob& j = a.job[blockIdx.y];
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int ow = j.ax.out, oh = j.ay.out;
    if (idx >= (int64_t)oh * ow) return;
    const int y = (int)(idx / ow), x = (int)(idx % ow);
    int v[C];
    bool live = true;
    if (END == FM_END_WINDOW) live = x >= j.rx0 && x < j.rx1 && y >= j.ry0 && y < j.ry1 && y >= j.top;
    if (live) {
        const int ymin = a.tab[j.ay.off + 2 * y], n = a.tab[j.ay.off + 2 * y + 1];
        const int* kk = a.tab + j.ay.off + 2 * oh + (int64_t)y * j.ay.taps;
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 1 << (MF_FM_PRECISION_BITS - 1);
        const uint8_t* col = a.inter + j.inter + (int64_t)x * C;
        for (int t = 0; t < n; ++t) {
            const int k = kk[t];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int p = j.skip_h ? fm_box_px<C>(a, j, x, ymin + t, c) : (int)col[(int64_t)(ymin + t) * ow * C + c];
                acc[c] += p * k;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = clip8(acc[c]);
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = 0;
    }
    if (END == FM_END_NET) {                  // C == 3: one 8-channel group (16 B per plane), channels 3..7 zero like k_nchw_to_act
        uint32_t h[3], l[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float f = fm_normalize(v[c < C ? c : 0], a.mean[c], a.std[c]);
            mf_split_bf16(f, h[c], l[c]);
        }
        const int64_t o = (((int64_t)j.slot * (a.NH + 2 * a.halo) + y + a.halo) * (a.NW + 2 * a.halo) + x + a.halo) * 8;
        *reinterpret_cast<uint4*>(a.hi + o) = make_uint4(h[0] | h[1] << 16, h[2], 0u, 0u);
        if (a.lo) *reinterpret_cast<uint4*>(a.lo + o) = make_uint4(l[0] | l[1] << 16, l[2], 0u, 0u);
    } else {
        uint8_t* d = a.out + j.out + idx * C;
#pragma unroll
        for (int c = 0; c < C; ++c) d[c] = (uint8_t)v[c];
    }
}

// ---- upsample + argmax + class mask --------------------------------------------------------------------------------------------------------------------------
// one thread = one output pixel; the 19 channels of a corner are consecutive in the NHWC head buffer
__global__ __launch_bounds__(256) void k_fm_argmax_mask(Pl X, int n_classes, uint8_t* __restrict__ dst, int H, int W, float sh, float sw, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int x = idx % W;
    int64_t t = idx / W;
    const int y = t % H;
    const int b = t / H;
    const BilinearAc g = bilinear_ac_corners(X, y, x, sh, sw);
    float best = bilinear_ac_sample(X, g, b, 0);
    int arg = 0;
    for (int c = 1; c < n_classes; ++c) {
        const float v = bilinear_ac_sample(X, g, b, c);
        if (v > best) { best = v; arg = c; }     // strict: the first maximum wins (numpy.argmax)
    }
    dst[idx] = arg >= 1 && arg <= 13 ? 255 : 0;   // parsing[parsing > 13] = 0; parsing[parsing >= 1] = 255
}

// ---- Gaussian blur --------------------------------------------------------------------------------------------------------------------------------------------
struct BlurJob { int w, h, k; int64_t src, tmp, out; };   // byte offset of the uint8 source / output [h][w]; float index of the fp32 intermediate [h][w]
struct BlurArgs { const uint8_t* src; float* tmp; float* taps; uint8_t* out; BlurJob job[MF_FM_MAX_JOBS]; };

__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

// taps of getGaussianKernel(k, 0), once per job: fp32 values of the float64 formula into the workspace.  grid (jobs), one workgroup each
__global__ __launch_bounds__(256) void k_fm_blur_taps(const BlurArgs a) {
    __shared__ double s_raw[MF_FM_BLUR_MAX_K];
    const int k = a.job[blockIdx.x].k;
    const double sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8;
    const double s2 = -0.5 / (sigma * sigma), c = (k - 1) * 0.5;
    for (int i = threadIdx.x; i < k; i += 256) s_raw[i] = exp(s2 * (i - c) * (i - c));
    __syncthreads();
    double sum = 0.0;
    for (int i = 0; i < k; ++i) sum += s_raw[i];           // in index order, by every thread alike
    for (int i = threadIdx.x; i < k; i += 256) a.taps[blockIdx.x * MF_FM_BLUR_TAP_STRIDE + i] = (float)(s_raw[i] / sum);
}

__device__ __forceinline__ void blur_taps(const BlurArgs& a, int job, int k, float* s_tap) {
    for (int i = threadIdx.x; i < k; i += blockDim.x) s_tap[i] = a.taps[job * MF_FM_BLUR_TAP_STRIDE + i];
    __syncthreads();
}

// grid (row segments, rows, jobs): a workgroup blurs MF_FM_BLUR_TW pixels of one row
__global__ __launch_bounds__(MF_FM_BLUR_TW) void k_fm_blur_h(const BlurArgs a) {
    __shared__ float s_tap[MF_FM_BLUR_MAX_K];
    __shared__ float s_row[MF_FM_BLUR_TW + 2 * MF_FM_BLUR_R];
    const BlurJob& j = a.job[blockIdx.z];
    const int y = blockIdx.y, x0 = blockIdx.x * MF_FM_BLUR_TW;
    if (y >= j.h || x0 >= j.w) return;           // (uniform per workgroup)
    blur_taps(a, blockIdx.z, j.k, s_tap);
    const int r = j.k >> 1;
    const uint8_t* row = a.src + j.src + (int64_t)y * j.w;
    for (int i = threadIdx.x; i < MF_FM_BLUR_TW + 2 * r; i += MF_FM_BLUR_TW) s_row[i] = (float)row[reflect101(x0 - r + i, j.w)];
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= j.w) return;
    float acc = 0.f;
    for (int t = 0; t < j.k; ++t) acc += s_row[threadIdx.x + t] * s_tap[t];
    a.tmp[j.tmp + (int64_t)y * j.w + x] = acc;
}

// grid (column strips, row strips, jobs): a workgroup of 256 = 64 columns x 4 row lanes blurs a 64 x 32 tile
__global__ __launch_bounds__(256) void k_fm_blur_v(const BlurArgs a) {
    __shared__ float s_tap[MF_FM_BLUR_MAX_K];
    __shared__ float s_col[MF_FM_BLUR_VR + 2 * MF_FM_BLUR_R][MF_FM_BLUR_VC];
    const BlurJob& j = a.job[blockIdx.z];
    const int x0 = blockIdx.x * MF_FM_BLUR_VC, y0 = blockIdx.y * MF_FM_BLUR_VR;
    if (x0 >= j.w || y0 >= j.h) return;           // (uniform per workgroup)
    blur_taps(a, blockIdx.z, j.k, s_tap);
    const int r = j.k >> 1;
    const int cx = threadIdx.x & (MF_FM_BLUR_VC - 1), lane = threadIdx.x / MF_FM_BLUR_VC;
    const int x = x0 + cx;
    const float* src = a.tmp + j.tmp;
    if (x < j.w)
        for (int i = lane; i < MF_FM_BLUR_VR + 2 * r; i += 256 / MF_FM_BLUR_VC) s_col[i][cx] = src[(int64_t)reflect101(y0 - r + i, j.h) * j.w + x];
    __syncthreads();
    if (x >= j.w) return;
    for (int dy = lane; dy < MF_FM_BLUR_VR; dy += 256 / MF_FM_BLUR_VC) {
        const int y = y0 + dy;
        if (y >= j.h) break;
        float acc = 0.f;
        for (int t = 0; t < j.k; ++t) acc += s_col[dy + t][cx] * s_tap[t];
        a.out[j.out + (int64_t)y * j.w + x] = (uint8_t)fminf(fmaxf(rintf(acc), 0.f), 255.f);   // the one rounding: half to even
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------------
inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

int blur_kernel_size(int width) { return (int)(std::floor(0.1 * width / 2.0) * 2.0) + 1; }   // int(0.1 * width // 2 * 2) + 1

// taps per output index of one axis, 0 when the geometry is refused
int axis_taps(int filter, int in, int out) {
    if (in == out) return 1;
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
    return (int)std::ceil((filter == 0 ? 1.0 : 2.0) * fs) * 2 + 1;
}

// Workspace of one chunk of <= MF_FM_MAX_JOBS jobs: [tables | uint8 intermediates | (finish) uint8 pre-blur masks | (finish) fp32 blur intermediates | (finish) blur taps].  The chunks of a
// call run one behind the other on the stream, so they share the block.
struct ChunkLayout { size_t tab_bytes, inter_bytes, pre_bytes, tmp_bytes, taps_bytes, total; };

// first: index of the chunk's first job in the call, so that a refusal names the call's job.
// sizes: [n][2] (box width, box height); out_w / out_h: the fixed output size (parse), or <= 0: the output is the box and the source is src_w x src_h (finish)
int chunk_layout(const char* who, int first, int finish, const int* sizes, int n, int S_h, int S_w, int channels, ChunkLayout& L, FmJob* jobs) {
    size_t tab = 0, inter = 0, pre = 0, tmp = 0;
    const int filter = finish ? 1 : 0;
    for (int i = 0; i < n; ++i) {
        const int bw = sizes[2 * i], bh = sizes[2 * i + 1];
        MF_REQUIRE(bw >= 1 && bh >= 1 && bw <= 16384 && bh <= 16384, "%s: job %d: box %d x %d outside [1, 16384]", who, first + i, bw, bh);
        FmAxis ax{finish ? S_w : bw, finish ? bw : S_w, 0, 0}, ay{finish ? S_h : bh, finish ? bh : S_h, 0, 0};
        ax.taps = axis_taps(filter, ax.in, ax.out); ay.taps = axis_taps(filter, ay.in, ay.out);
        MF_REQUIRE(ax.taps <= MF_FM_MAX_TAPS && ay.taps <= MF_FM_MAX_TAPS,
                   "%s: job %d: resampling %d x %d to %d x %d needs %d taps per pixel, the limit is MF_FM_MAX_TAPS = %d", who, first + i, ax.in, ay.in, ax.out, ay.out,
                   ax.taps > ay.taps ? ax.taps : ay.taps, MF_FM_MAX_TAPS);
        ax.off = (int)(tab / sizeof(int)); tab += (size_t)ax.out * (2 + ax.taps) * sizeof(int);
        ay.off = (int)(tab / sizeof(int)); tab += (size_t)ay.out * (2 + ay.taps) * sizeof(int);
        if (jobs) {
            jobs[i].ax = ax; jobs[i].ay = ay; jobs[i].skip_h = ax.in == ax.out ? 1 : 0;
            jobs[i].inter = (int64_t)inter;
        }
        if (ax.in != ax.out) inter += align256((size_t)ay.in * ax.out * channels);
        if (finish) {
            const int k = blur_kernel_size(bw);
            MF_REQUIRE(k <= MF_FM_BLUR_MAX_K, "%s: job %d: a %d-pixel-wide mask needs a %d-tap blur, the LDS tiles hold MF_FM_BLUR_MAX_K = %d taps", who, first + i, bw, k,
                       MF_FM_BLUR_MAX_K);
            pre += align256((size_t)bw * bh);
            tmp += align256((size_t)bw * bh * sizeof(float));
        }
    }
    L.tab_bytes = align256(tab); L.inter_bytes = inter; L.pre_bytes = pre; L.tmp_bytes = tmp;
    L.taps_bytes = finish ? align256((size_t)n * MF_FM_BLUR_TAP_STRIDE * sizeof(float)) : 0;
    L.total = L.tab_bytes + inter + pre + tmp + L.taps_bytes;
    return MF_OK;
}

unsigned groups(int64_t px) { return (unsigned)((px + 255) / 256); }

}  // namespace

extern "C" size_t mf_face_mask_workspace_bytes(int finish, const int* box_sizes, int n_jobs, int mask_h, int mask_w) {
    if (!box_sizes || n_jobs < 1 || mask_h < 1 || mask_w < 1) return 0;
    size_t need = 0;
    for (int j0 = 0; j0 < n_jobs; j0 += MF_FM_MAX_JOBS) {
        ChunkLayout L{};
        const int nj = n_jobs - j0 < MF_FM_MAX_JOBS ? n_jobs - j0 : MF_FM_MAX_JOBS;
        if (chunk_layout("face_mask_workspace_bytes", j0, finish, box_sizes + 2 * j0, nj, mask_h, mask_w, finish ? 1 : 3, L, nullptr)) return 0;
        if (L.total > need) need = L.total;
    }
    return need;
}

extern "C" int mf_face_mask_parse(mf_net* net, int in_buf, int head_buf, int n_classes, const uint8_t* frames, int n_frames, int H, int W, int reverse_channels,
                                  const int* jobs, int n_jobs, const float* mean3, const float* std3, void* workspace, size_t workspace_bytes, uint8_t* masks,
                                  void* stream) {
    MF_REQUIRE(net && frames && jobs && mean3 && std3 && workspace && masks, "face_mask_parse: null argument");
    MF_REQUIRE(n_frames >= 1 && H >= 1 && W >= 1 && n_jobs >= 1, "face_mask_parse: bad size");
    MF_REQUIRE(n_jobs <= mf_net_max_batch(net), "face_mask_parse: %d jobs exceed the graph's capacity %d", n_jobs, mf_net_max_batch(net));
    const ActBuf* ib = mf_net_actbuf(net, in_buf);
    const ActBuf* hb = mf_net_actbuf(net, head_buf);
    MF_REQUIRE(ib && hb, "net: no buffer %d", ib ? head_buf : in_buf);
    MF_REQUIRE(ib->C == 8, "face_mask_parse: buffer %d has %d channels, not the 8 of a 3-channel input", in_buf, ib->C);
    MF_REQUIRE(n_classes >= 14 && n_classes <= hb->C, "face_mask_parse: %d classes do not fit the head buffer's %d channels (classes 1..13 are the mask)", n_classes, hb->C);
    hipStream_t s = (hipStream_t)stream;
    int sizes[2 * MF_FM_MAX_JOBS];
    size_t need = 0;                           // the largest chunk's workspace, as mf_face_mask_workspace_bytes reports it
    // Every refusal is decided before the first launch: a job refused in a later chunk must not leave the earlier chunks' input planes written.
    for (int j0 = 0; j0 < n_jobs; j0 += MF_FM_MAX_JOBS) {
        const int nj = n_jobs - j0 < MF_FM_MAX_JOBS ? n_jobs - j0 : MF_FM_MAX_JOBS;
        for (int i = 0; i < nj; ++i) {
            const int* q = jobs + 5 * (j0 + i);
            MF_REQUIRE(q[0] >= 0 && q[0] < n_frames, "face_mask_parse: job %d: frame index %d out of range (%d frames)", j0 + i, q[0], n_frames);
            MF_REQUIRE(q[3] > q[1] && q[4] > q[2], "face_mask_parse: job %d: crop box (%d, %d, %d, %d) is empty", j0 + i, q[1], q[2], q[3], q[4]);
            MF_REQUIRE(q[1] > -(1 << 20) && q[2] > -(1 << 20) && q[3] < (1 << 20) && q[4] < (1 << 20), "face_mask_parse: job %d: crop box coordinate beyond 2^20", j0 + i);
            sizes[2 * i] = q[3] - q[1]; sizes[2 * i + 1] = q[4] - q[2];
        }
        ChunkLayout L{};
        int rc = chunk_layout("face_mask_parse", j0, 0, sizes, nj, ib->H, ib->W, 3, L, nullptr);
        if (rc) return rc;
        if (L.total > need) need = L.total;
    }
    MF_REQUIRE(need <= workspace_bytes, "face_mask_parse: the workspace holds %zu bytes, %zu are needed (mf_face_mask_workspace_bytes)", workspace_bytes, need);
    for (int j0 = 0; j0 < n_jobs; j0 += MF_FM_MAX_JOBS) {
        const int nj = n_jobs - j0 < MF_FM_MAX_JOBS ? n_jobs - j0 : MF_FM_MAX_JOBS;
        FmArgs a{};
        for (int i = 0; i < nj; ++i) {
            const int* q = jobs + 5 * (j0 + i);
            FmJob& j = a.job[i];
            j.src = q[0]; j.bx = q[1]; j.by = q[2]; j.bw = q[3] - q[1]; j.bh = q[4] - q[2]; j.slot = j0 + i;
            sizes[2 * i] = j.bw; sizes[2 * i + 1] = j.bh;
        }
        ChunkLayout L{};
        int rc = chunk_layout("face_mask_parse", j0, 0, sizes, nj, ib->H, ib->W, 3, L, a.job);
        if (rc) return rc;                     // (accepted above)
        a.src = frames; a.SH = H; a.SW = W; a.rev = reverse_channels ? 1 : 0; a.filter = 0;
        a.tab = (int*)workspace; a.inter = (uint8_t*)workspace + L.tab_bytes; a.out = nullptr;
        a.hi = ib->hi; a.lo = ib->lo; a.halo = ib->halo; a.NH = ib->H; a.NW = ib->W;
        for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.std[c] = std3[c]; }
        a.n_jobs = nj;
        int max_bh = 1;
        bool any_h = false;
        for (int i = 0; i < nj; ++i) { if (a.job[i].bh > max_bh) max_bh = a.job[i].bh; any_h |= !a.job[i].skip_h; }
        hipLaunchKernelGGL(k_fm_tables, dim3(groups(ib->H > ib->W ? ib->H : ib->W), 2 * nj), dim3(256), 0, s, a);
        MF_HIP(hipGetLastError());
        if (any_h) {
            hipLaunchKernelGGL(k_fm_pass_h<3>, dim3(groups((int64_t)max_bh * ib->W), nj), dim3(256), 0, s, a);
            MF_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL((k_fm_pass_v<3, FM_END_NET>), dim3(groups((int64_t)ib->H * ib->W), nj), dim3(256), 0, s, a);
        MF_HIP(hipGetLastError());
    }
    int rc = mf_net_run(net, n_jobs, stream);
    if (rc) return rc;
    const float sh = ib->H > 1 ? (float)(hb->H - 1) / (float)(ib->H - 1) : 0.f, sw = ib->W > 1 ? (float)(hb->W - 1) / (float)(ib->W - 1) : 0.f;
    const int64_t total = (int64_t)n_jobs * ib->H * ib->W;
    hipLaunchKernelGGL(k_fm_argmax_mask, dim3(groups(total)), dim3(256), 0, s, pl_of(*hb), n_classes, masks, ib->H, ib->W, sh, sw, total);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_face_mask_finish(const uint8_t* masks, int mask_h, int mask_w, const int* jobs, int n_jobs, int blur, void* workspace, size_t workspace_bytes,
                                   uint8_t* pre_blur, uint8_t* out, void* stream) {
    MF_REQUIRE(masks && jobs && workspace && (blur ? out != nullptr : pre_blur != nullptr), "face_mask_finish: null argument");
    MF_REQUIRE(mask_h >= 1 && mask_w >= 1 && n_jobs >= 1, "face_mask_finish: bad size");
    hipStream_t s = (hipStream_t)stream;
    int sizes[2 * MF_FM_MAX_JOBS];
    size_t need = 0;                           // the largest chunk's workspace, as mf_face_mask_workspace_bytes reports it
    // Every refusal is decided before the first launch: a job refused in a later chunk must not leave the earlier chunks' masks written.
    for (int j0 = 0; j0 < n_jobs; j0 += MF_FM_MAX_JOBS) {
        const int nj = n_jobs - j0 < MF_FM_MAX_JOBS ? n_jobs - j0 : MF_FM_MAX_JOBS;
        for (int i = 0; i < nj; ++i) {
            const int* q = jobs + 7 * (j0 + i);
            const int w = q[0], h = q[1];
            MF_REQUIRE(w >= 1 && h >= 1, "face_mask_finish: job %d: empty crop %d x %d", j0 + i, w, h);
            MF_REQUIRE(q[2] >= 0 && q[3] >= 0 && q[4] <= w && q[5] <= h && q[4] >= q[2] && q[5] >= q[3],
                       "face_mask_finish: job %d: the face-box rectangle (%d, %d, %d, %d) must lie inside the %d x %d crop", j0 + i, q[2], q[3], q[4], q[5], w, h);
            sizes[2 * i] = w; sizes[2 * i + 1] = h;
        }
        ChunkLayout L{};
        int rc = chunk_layout("face_mask_finish", j0, 1, sizes, nj, mask_h, mask_w, 1, L, nullptr);
        if (rc) return rc;
        if (L.total > need) need = L.total;
    }
    MF_REQUIRE(need <= workspace_bytes, "face_mask_finish: the workspace holds %zu bytes, %zu are needed (mf_face_mask_workspace_bytes)", workspace_bytes, need);
    int64_t packed = 0;                        // job i's mask starts where job i - 1's ended, in `out` and in `pre_blur`
    for (int j0 = 0; j0 < n_jobs; j0 += MF_FM_MAX_JOBS) {
        const int nj = n_jobs - j0 < MF_FM_MAX_JOBS ? n_jobs - j0 : MF_FM_MAX_JOBS;
        FmArgs a{};
        for (int i = 0; i < nj; ++i) {
            const int* q = jobs + 7 * (j0 + i);
            FmJob& j = a.job[i];
            j.src = j0 + i; j.bx = 0; j.by = 0; j.bw = mask_w; j.bh = mask_h;
            j.rx0 = q[2]; j.ry0 = q[3]; j.rx1 = q[4]; j.ry1 = q[5]; j.top = q[6];
            sizes[2 * i] = q[0]; sizes[2 * i + 1] = q[1];
        }
        ChunkLayout L{};
        int rc = chunk_layout("face_mask_finish", j0, 1, sizes, nj, mask_h, mask_w, 1, L, a.job);
        if (rc) return rc;                     // (accepted above)
        uint8_t* ws = (uint8_t*)workspace;
        a.src = masks; a.SH = mask_h; a.SW = mask_w; a.rev = 0; a.filter = 1;
        a.tab = (int*)ws; a.inter = ws + L.tab_bytes;
        a.out = pre_blur ? pre_blur : ws + L.tab_bytes + L.inter_bytes;
        a.n_jobs = nj;
        BlurArgs b{};
        b.src = a.out; b.tmp = (float*)(ws + L.tab_bytes + L.inter_bytes + L.pre_bytes); b.out = out;
        b.taps = (float*)(ws + L.tab_bytes + L.inter_bytes + L.pre_bytes + L.tmp_bytes);
        int max_w = 1, max_h = 1;
        bool any_h = false;
        size_t pre = 0, tmp = 0;
        for (int i = 0; i < nj; ++i) {
            const int w = sizes[2 * i], h = sizes[2 * i + 1];
            a.job[i].out = pre_blur ? packed : (int64_t)pre;
            b.job[i] = BlurJob{w, h, blur_kernel_size(w), a.job[i].out, (int64_t)(tmp / sizeof(float)), packed};
            pre += align256((size_t)w * h); tmp += align256((size_t)w * h * sizeof(float));
            packed += (int64_t)w * h;
            if (w > max_w) max_w = w;
            if (h > max_h) max_h = h;
            any_h |= !a.job[i].skip_h;
        }
        hipLaunchKernelGGL(k_fm_tables, dim3(groups(max_w > max_h ? max_w : max_h), 2 * nj), dim3(256), 0, s, a);
        MF_HIP(hipGetLastError());
        if (any_h) {
            hipLaunchKernelGGL(k_fm_pass_h<1>, dim3(groups((int64_t)mask_h * max_w), nj), dim3(256), 0, s, a);
            MF_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL((k_fm_pass_v<1, FM_END_WINDOW>), dim3(groups((int64_t)max_h * max_w), nj), dim3(256), 0, s, a);
        MF_HIP(hipGetLastError());
        if (!blur) continue;
        hipLaunchKernelGGL(k_fm_blur_taps, dim3(nj), dim3(256), 0, s, b);
        MF_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_fm_blur_h, dim3((max_w + MF_FM_BLUR_TW - 1) / MF_FM_BLUR_TW, max_h, nj), dim3(MF_FM_BLUR_TW), 0, s, b);
        MF_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_fm_blur_v, dim3((max_w + MF_FM_BLUR_VC - 1) / MF_FM_BLUR_VC, (max_h + MF_FM_BLUR_VR - 1) / MF_FM_BLUR_VR, nj), dim3(256), 0, s, b);
        MF_HIP(hipGetLastError());
    }
    return MF_OK;
}
