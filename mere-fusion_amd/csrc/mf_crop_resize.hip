// Avatar preparation between the detector and the generators, on the device: what wav2lip/genavatar.py:80-96,119 and musetalk/mere_musetalk.py:293-296 do on
// the host with numpy and cv2.
//
//   k_lip_boxes       first kept box of every frame (mf_s3fd_detect's `boxes`, `counts`, read where the detector left them) -> clip at 0, truncate to int
//                     (face_detection/api.py:64-79) -> pads, clamp to the frame (genavatar.py:87-90) -> get_smoothened_boxes (genavatar.py:52-59), in integers
//   k_crop_linear     batched crop + cv::resize INTER_LINEAR 8UC3, the coefficients formed in the kernel from each job's box (chains behind k_lip_boxes)
//   k_crop_lanczos4   batched crop + 8-tap separable integer resampler on caller-supplied per-job tables (cv::resize INTER_LANCZOS4 8UC3's fixed-point passes)
//
// get_smoothened_boxes.  The reference loop is in place and sequential, but entry i with i + T <= n averages entries i .. i + T - 1, none of which an earlier
// step has written: that head is parallel (read from the raw boxes, written to the result).  The last T - 1 entries (all of them when n < T) average
// `boxes[n - T:]`, a window that holds entries already smoothed: one thread walks them in order.  `boxes[n - T:]` with n < T is Python's slice of a negative
// start (n - T + n, clamped at 0), kept as written.  np.mean of int64 rows assigned back into the int64 array is the integer sum divided by the count and
// truncated, so everything is integer arithmetic.
//
// Resampling.  Linear is mf_blend.hip's `axis()` arithmetic (fp64 position, float fraction, 11-bit coefficients rounded half to even, `>> 4 .. >> 16 .. + 2 >> 2`),
// and the area fast path when a job's crop is exactly twice the destination.  Lanczos-4: horizontal pass int32 with no shift, vertical pass int32 (two's complement
// wrap-around, as 32-bit hardware gives) then `(sum + (1 << 21)) >> 22` saturated; a tap outside the CROP is clamped to the crop's edge (the reference resizes the
// cropped array).  No floating point touches a Lanczos pixel: the tables come from the host.
// Floating-point contraction is OFF in this file, as in mf_blend.hip.
#include "mf_common.h"

#pragma clang fp contract(off)

namespace {

// ---- boxes ---------------------------------------------------------------------------------------------------------------------------------------------------
struct BoxArgs {
    const float* boxes;         // [n][max_det][5] (x1, y1, x2, y2, score)
    const int* counts;          // [n]
    int n, max_det, H, W;
    int pad_top, pad_bottom, pad_left, pad_right;
    int T;                      // smoothing window; 0: nosmooth
    int* coords;                // [n][4] (y1, y2, x1, x2)
    mf_crop_job* jobs;          // [n]; holds the raw (unsmoothed) boxes until the last phase
    int* n_no_face;
};

__device__ __forceinline__ int trunc_clip0(float v) {
    v = fminf(fmaxf(v, 0.f), 16777216.f);                // np.clip(d, 0, None) then int(): truncation; the upper clamp only keeps the conversion defined
    return (int)v;
}

// box e (0..3 = x1, y1, x2, y2) of entry j as the sequential loop sees it at step i: smoothed when j < i, raw otherwise
__device__ __forceinline__ int box_at(const BoxArgs& a, int j, int i, int e) {
    if (j < i) return a.coords[j * 4 + (e == 0 ? 2 : e == 1 ? 0 : e == 2 ? 3 : 1)];
    const mf_crop_job& r = a.jobs[j];
    return e == 0 ? r.x1 : e == 1 ? r.y1 : e == 2 ? r.x2 : r.y2;
}

__device__ __forceinline__ void put_coords(const BoxArgs& a, int i, int x1, int y1, int x2, int y2) {
    int* c = a.coords + i * 4;
    c[0] = y1; c[1] = y2; c[2] = x1; c[3] = x2;
}

// one workgroup: the phases are separated by workgroup barriers, and the serial tail is T - 1 entries
__global__ __launch_bounds__(256) void k_lip_boxes(const BoxArgs a) {
    __shared__ int s_no_face;
    const int tid = threadIdx.x, n = a.n, T = a.T;
    if (tid == 0) s_no_face = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        mf_crop_job j;
        j.frame_index = i; j.x1 = j.y1 = j.x2 = j.y2 = 0;
        if (a.counts[i] < 1) {
            atomicAdd(&s_no_face, 1);
        } else {
            const float* b = a.boxes + (int64_t)i * a.max_det * 5;
            const int rx1 = trunc_clip0(b[0]), ry1 = trunc_clip0(b[1]), rx2 = trunc_clip0(b[2]), ry2 = trunc_clip0(b[3]);
            j.y1 = max(0, ry1 - a.pad_top);
            j.y2 = min(a.H, ry2 + a.pad_bottom);
            j.x1 = max(0, rx1 - a.pad_left);
            j.x2 = min(a.W, rx2 + a.pad_right);
        }
        a.jobs[i] = j;
    }
    __syncthreads();
    if (T <= 0) {
        for (int i = tid; i < n; i += 256) { const mf_crop_job& r = a.jobs[i]; put_coords(a, i, r.x1, r.y1, r.x2, r.y2); }
    } else {
        const int head = n - T + 1 > 0 ? n - T + 1 : 0;  // entries with i + T <= n
        for (int i = tid; i < head; i += 256) {
            long long s[4] = {0, 0, 0, 0};
            for (int j = i; j < i + T; ++j) { const mf_crop_job& r = a.jobs[j]; s[0] += r.x1; s[1] += r.y1; s[2] += r.x2; s[3] += r.y2; }
            put_coords(a, i, (int)(s[0] / T), (int)(s[1] / T), (int)(s[2] / T), (int)(s[3] / T));
        }
        __syncthreads();
        if (tid == 0) {
            int start = n - T;                           // boxes[len(boxes) - T:]
            if (start < 0) { start += n; if (start < 0) start = 0; }
            const int cnt = n - start;
            for (int i = head; i < n; ++i) {
                long long s[4] = {0, 0, 0, 0};
                for (int j = start; j < n; ++j)
                    for (int e = 0; e < 4; ++e) s[e] += box_at(a, j, i, e);
                put_coords(a, i, (int)(s[0] / cnt), (int)(s[1] / cnt), (int)(s[2] / cnt), (int)(s[3] / cnt));
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int* c = a.coords + i * 4;
        mf_crop_job j;
        j.frame_index = i; j.y1 = c[0]; j.y2 = c[1]; j.x1 = c[2]; j.x2 = c[3];
        a.jobs[i] = j;
    }
    if (tid == 0) *a.n_no_face = s_no_face;
}

// ---- crop + resample -----------------------------------------------------------------------------------------------------------------------------------------
struct CropArgs {
    const uint8_t* frames;      // [n_frames][H][W][3]
    int n_frames, H, W;
    const mf_crop_job* jobs;    // device
    int job0;                   // first job of this launch
    uint8_t* dst;               // [n_jobs][dh][dw][3]
    int dh, dw;
    const int* xofs; const int16_t* xcoef; const int* yofs; const int16_t* ycoef;      // lanczos4 only: [n_jobs][dw], [n_jobs][dw][8], [n_jobs][dh], [n_jobs][dh][8]
};

// A table the host has not seen (written by k_lip_boxes) can hold the empty box of a frame without a face: such a job reads nothing and its destination is zeroed.
__device__ __forceinline__ bool job_ok(const CropArgs& a, const mf_crop_job& j) {
    return j.frame_index >= 0 && j.frame_index < a.n_frames && j.x1 >= 0 && j.y1 >= 0 && j.x2 <= a.W && j.y2 <= a.H && j.x2 > j.x1 && j.y2 > j.y1;
}

// One axis of cv::resize's linear tables: the same statements as mf_blend.hip's `axis()` (kept in step with it by tests/test_crop_resize.py, which holds both
// kernels to the one integer model).
__device__ __forceinline__ void lin_axis(int d, int ssize, int dsize, bool clamp_offset, int& s0, int& s1, int& a0, int& a1) {
    const double inv_scale = (double)dsize / (double)ssize;
    const double scale = 1.0 / inv_scale;
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (clamp_offset) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
    }
    a0 = (int)rintf((1.f - f) * 2048.f);
    a1 = (int)rintf(f * 2048.f);
    s0 = min(max(s, 0), ssize - 1);
    s1 = min(max(s + 1, 0), ssize - 1);
}

// grid (pixel groups, jobs): one thread = one destination pixel, 3 channels
__global__ __launch_bounds__(256) void k_crop_linear(const CropArgs a) {
    const int ji = a.job0 + blockIdx.y;
    const mf_crop_job j = a.jobs[ji];
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.dh * a.dw) return;
    const int dy = p / a.dw, dx = p - dy * a.dw;
    uint8_t* o = a.dst + ((int64_t)ji * a.dh * a.dw + p) * 3;
    if (!job_ok(a, j)) { o[0] = o[1] = o[2] = 0; return; }
    const int cw = j.x2 - j.x1, ch = j.y2 - j.y1;
    const uint8_t* src = a.frames + (((int64_t)j.frame_index * a.H + j.y1) * a.W + j.x1) * 3;       // pixel (0, 0) of the crop; rows are W * 3 bytes apart
    const int pitch = a.W * 3;
    if (cw == 2 * a.dw && ch == 2 * a.dh) {              // exact 2 x 2 decimation: INTER_AREA fast path
        const uint8_t* q = src + (2 * dy) * pitch + (2 * dx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)((q[c] + q[c + 3] + q[c + pitch] + q[c + pitch + 3] + 2) >> 2);
        return;
    }
    int x0, x1, ax0, ax1, y0, y1, by0, by1;
    lin_axis(dx, cw, a.dw, true, x0, x1, ax0, ax1);
    lin_axis(dy, ch, a.dh, false, y0, y1, by0, by1);
    const uint8_t* r0 = src + y0 * pitch;
    const uint8_t* r1 = src + y1 * pitch;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int S0 = r0[x0 * 3 + c] * ax0 + r0[x1 * 3 + c] * ax1;
        const int S1 = r1[x0 * 3 + c] * ax0 + r1[x1 * 3 + c] * ax1;
        const int v = (((by0 * (S0 >> 4)) >> 16) + ((by1 * (S1 >> 4)) >> 16) + 2) >> 2;
        o[c] = (uint8_t)min(max(v, 0), 255);
    }
}

// Lanczos-4.  A workgroup owns a destination tile of LZ_TH x LZ_TW pixels of one job and keeps the horizontally filtered source rows of the tile in LDS (int32,
// LZ_ROWS x LZ_TW x 3 = 24 KB): a source row is filtered once for the up to 8 destination rows that use it.  A strong decimation spreads a tile's rows over more
// source rows than LDS holds; the tile's rows are then taken in chunks whose source span fits (a single row spans 8).  The tables are the caller's: every index
// formed from them is clamped (to the crop for reads, to the chunk for LDS), so a wrong table gives wrong pixels, never a wrong address.
constexpr int LZ_TW = 32, LZ_TH = 16, LZ_ROWS = 64, LZ_TAPS = 8;

__global__ __launch_bounds__(256) void k_crop_lanczos4(const CropArgs a) {
    __shared__ int s_rows[LZ_ROWS][LZ_TW * 3];
    __shared__ int s_xo[LZ_TW], s_yo[LZ_TH];
    __shared__ int16_t s_xc[LZ_TW][LZ_TAPS], s_yc[LZ_TH][LZ_TAPS];
    const int tid = threadIdx.x;
    const int ji = a.job0 + blockIdx.z;
    const mf_crop_job j = a.jobs[ji];
    const int tx0 = blockIdx.x * LZ_TW, ty0 = blockIdx.y * LZ_TH;
    const int tw = min(LZ_TW, a.dw - tx0), th = min(LZ_TH, a.dh - ty0);
    const int tw3 = tw * 3;
    uint8_t* dst = a.dst + (((int64_t)ji * a.dh + ty0) * a.dw + tx0) * 3;                           // tile pixel (0, 0); rows are dw * 3 bytes apart
    if (!job_ok(a, j)) {
        for (int i = tid; i < th * tw3; i += 256) dst[(i / tw3) * a.dw * 3 + i % tw3] = 0;
        return;
    }
    const int cw = j.x2 - j.x1, ch = j.y2 - j.y1;
    if (tid < tw) s_xo[tid] = a.xofs[(int64_t)ji * a.dw + tx0 + tid];
    if (tid < th) s_yo[tid] = a.yofs[(int64_t)ji * a.dh + ty0 + tid];
    for (int i = tid; i < tw * LZ_TAPS; i += 256) s_xc[i / LZ_TAPS][i % LZ_TAPS] = a.xcoef[((int64_t)ji * a.dw + tx0) * LZ_TAPS + i];
    for (int i = tid; i < th * LZ_TAPS; i += 256) s_yc[i / LZ_TAPS][i % LZ_TAPS] = a.ycoef[((int64_t)ji * a.dh + ty0) * LZ_TAPS + i];
    __syncthreads();
    const uint8_t* src = a.frames + (((int64_t)j.frame_index * a.H + j.y1) * a.W + j.x1) * 3;
    const int pitch = a.W * 3;
    for (int ra = 0; ra < th;) {                         // chunk [ra, rb) of the tile's rows: uniform over the workgroup (LDS values only)
        const int r0 = min(max(s_yo[ra], 0), ch - 1);
        int rb = ra + 1;
        while (rb < th && min(max(s_yo[rb] + LZ_TAPS - 1, 0), ch - 1) - r0 < LZ_ROWS && min(max(s_yo[rb], 0), ch - 1) >= r0) ++rb;
        const int r1 = min(max(s_yo[rb - 1] + LZ_TAPS - 1, 0), ch - 1);
        const int nrows = min(max(r1 - r0 + 1, 1), LZ_ROWS);
        for (int i = tid; i < nrows * tw3; i += 256) {   // horizontal pass: source row r0 + r of the crop, tile column x, channel c
            const int r = i / tw3, q = i - r * tw3;
            const int x = q / 3, c = q - x * 3;
            const uint8_t* row = src + (r0 + r) * pitch + c;
            const int xo = s_xo[x];
            int sum = 0;
#pragma unroll
            for (int k = 0; k < LZ_TAPS; ++k) sum += (int)s_xc[x][k] * (int)row[min(max(xo + k, 0), cw - 1) * 3];
            s_rows[r][q] = sum;
        }
        __syncthreads();
        for (int i = tid; i < (rb - ra) * tw3; i += 256) {   // vertical pass
            const int dyl = ra + i / tw3, q = i % tw3;
            const int yo = s_yo[dyl];
            uint32_t sum = 0;                            // int32 accumulation with two's complement wrap-around
#pragma unroll
            for (int k = 0; k < LZ_TAPS; ++k) {
                const int r = min(max(min(max(yo + k, 0), ch - 1) - r0, 0), nrows - 1);
                sum += (uint32_t)((int)s_yc[dyl][k]) * (uint32_t)s_rows[r][q];
            }
            const int v = (int)(sum + (1u << 21)) >> 22;
            dst[dyl * a.dw * 3 + q] = (uint8_t)min(max(v, 0), 255);
        }
        __syncthreads();
        ra = rb;
    }
}

constexpr int MAX_JOBS_PER_LAUNCH = 32768;               // grid y / z limit 65535

}  // namespace

extern "C" int mf_avatar_lip_boxes(const float* boxes, const int* counts, int n, int max_det, int H, int W, const int* pads, int smooth_T, int* coords,
                                   mf_crop_job* jobs, int* n_no_face, void* stream) {
    MF_REQUIRE(boxes && counts && pads && coords && jobs && n_no_face, "avatar_lip_boxes: null argument");
    MF_REQUIRE(n >= 1 && max_det >= 1 && H >= 1 && W >= 1 && smooth_T >= 0, "avatar_lip_boxes: bad size (n %d, max_det %d, frame %d x %d, T %d)", n, max_det, H, W, smooth_T);
    MF_REQUIRE((int64_t)n * max_det * 5 < (int64_t)1 << 31, "avatar_lip_boxes: %d frames x %d boxes exceed 2^31 values", n, max_det);
    for (int i = 0; i < 4; ++i) MF_REQUIRE(pads[i] > -(1 << 24) && pads[i] < (1 << 24), "avatar_lip_boxes: pad %d = %d", i, pads[i]);
    BoxArgs a{boxes, counts, n, max_det, H, W, pads[0], pads[1], pads[2], pads[3], smooth_T, coords, jobs, n_no_face};
    hipLaunchKernelGGL(k_lip_boxes, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_crop_resize_u8(const uint8_t* frames, int n_frames, int H, int W, const mf_crop_job* jobs, const mf_crop_job* jobs_host, int n_jobs, uint8_t* dst,
                                 int dh, int dw, int mode, const int* xofs, const int16_t* xcoef, const int* yofs, const int16_t* ycoef, void* stream) {
    MF_REQUIRE(dh >= 1 && dw >= 1, "crop_resize_u8: destination %d x %d", dh, dw);
    MF_REQUIRE(frames && jobs && dst, "crop_resize_u8: null argument");
    MF_REQUIRE(mode == MF_CROP_LINEAR || mode == MF_CROP_LANCZOS4, "crop_resize_u8: mode %d is neither MF_CROP_LINEAR nor MF_CROP_LANCZOS4", mode);
    MF_REQUIRE(mode == MF_CROP_LINEAR || (xofs && xcoef && yofs && ycoef), "crop_resize_u8: null table (lanczos4 needs xofs, xcoef, yofs, ycoef)");
    MF_REQUIRE(n_frames >= 1 && H >= 1 && W >= 1 && n_jobs >= 1, "crop_resize_u8: bad size (%d frames of %d x %d, %d jobs)", n_frames, H, W, n_jobs);
    MF_REQUIRE((int64_t)n_frames * H * W * 3 < (int64_t)1 << 31, "crop_resize_u8: %d frames of %d x %d x 3 reach 2^31 bytes (32-bit offsets); pass fewer frames per call",
               n_frames, H, W);
    MF_REQUIRE((int64_t)n_jobs * dh * dw * 8 < (int64_t)1 << 31, "crop_resize_u8: %d crops of %d x %d overflow the 32-bit table and pixel offsets", n_jobs, dh, dw);
    if (jobs_host)
        for (int i = 0; i < n_jobs; ++i) {
            const mf_crop_job& j = jobs_host[i];
            MF_REQUIRE(j.frame_index >= 0 && j.frame_index < n_frames, "crop_resize_u8: job %d: frame index %d out of range (%d frames)", i, j.frame_index, n_frames);
            MF_REQUIRE(j.x2 > j.x1 && j.y2 > j.y1, "crop_resize_u8: job %d: crop (%d, %d, %d, %d) is empty", i, j.x1, j.y1, j.x2, j.y2);
            MF_REQUIRE(j.x1 >= 0 && j.y1 >= 0 && j.x2 <= W && j.y2 <= H, "crop_resize_u8: job %d: crop (%d, %d, %d, %d) is outside the %d x %d frame", i, j.x1, j.y1, j.x2,
                       j.y2, W, H);
        }
    hipStream_t s = (hipStream_t)stream;
    for (int j0 = 0; j0 < n_jobs; j0 += MAX_JOBS_PER_LAUNCH) {
        const int nj = n_jobs - j0 < MAX_JOBS_PER_LAUNCH ? n_jobs - j0 : MAX_JOBS_PER_LAUNCH;
        const CropArgs a{frames, n_frames, H, W, jobs, j0, dst, dh, dw, xofs, xcoef, yofs, ycoef};
        if (mode == MF_CROP_LINEAR)
            hipLaunchKernelGGL(k_crop_linear, dim3((dh * dw + 255) / 256, nj), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL(k_crop_lanczos4, dim3((dw + LZ_TW - 1) / LZ_TW, (dh + LZ_TH - 1) / LZ_TH, nj), dim3(256), 0, s, a);
        MF_HIP(hipGetLastError());
    }
    return MF_OK;
}
