// The sliding audio windows of the sessions of one step, pushed by one launch: what lipasr.py:17-21 + :36 do per session on the host.
//
// buf fp32 [n_rows][n] holds every session's window (lip_driver.LipWindowPool: n = (2B + l + r) * chunk samples).  A step brings n_new = 2B * chunk new samples
// for m of the rows; row r = table[i] becomes concat(buf[r][n_new:], new[i]) and the same n values are written to win[i], the contiguous block the mel kernel
// reads next.  The row table travels BY VALUE in the launch arguments (64 rows, as mf_frames_gather passes its sources): no index tensor, no upload, nothing to
// keep alive behind the call.
//
// One workgroup owns one row.  The kept context, ctx = n - n_new floats ((l + r) * chunk: 6 400 floats = 25.6 KB at the defaults), moves DOWN by n_new inside
// the row; when n_new < ctx the ranges overlap, and a workgroup that wrote while another of its waves still read would shift wrong values.  So the context goes
// through LDS: every thread reads its part, one barrier, and only then is the row written.  No atomics, no traffic between workgroups; rows outside the table
// are not touched.
//
// Every copy is 16 bytes per thread where both ends are 16-byte aligned (a workgroup-uniform test: the row base, n_new and ctx decide it), with a scalar tail for
// the last len % 4 floats; a row whose base or n_new breaks the alignment (a chunk that is no multiple of 4) is copied float by float.  The values are the same.
#include "mf_common.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int THREADS = 256;
constexpr int TABLE = 64;                      // rows per launch; a longer list goes out as several launches
constexpr int64_t LDS_BYTES = 160 * 1024;      // gfx950: 160 KB per workgroup

struct RowTable { int row[TABLE]; };

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// dst[0, len) <- src[0, len), by all threads of the workgroup; dst / src global or LDS
__device__ __forceinline__ void wg_copy(float* __restrict__ dst, const float* __restrict__ src, int len) {
    if (aligned16(dst) && aligned16(src)) {
        const int n4 = len >> 2;
        for (int i = threadIdx.x; i < n4; i += THREADS) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
        for (int i = (n4 << 2) + threadIdx.x; i < len; i += THREADS) dst[i] = src[i];          // the scalar tail: at most 3 floats
    } else {
        for (int i = threadIdx.x; i < len; i += THREADS) dst[i] = src[i];
    }
}

// dst_a[0, len) and dst_b[0, len) <- src[0, len): the new samples are read once for the pool row and for the step's window
__device__ __forceinline__ void wg_copy2(float* __restrict__ dst_a, float* __restrict__ dst_b, const float* __restrict__ src, int len) {
    if (aligned16(dst_a) && aligned16(dst_b) && aligned16(src)) {
        const int n4 = len >> 2;
        for (int i = threadIdx.x; i < n4; i += THREADS) {
            const float4 v = reinterpret_cast<const float4*>(src)[i];
            reinterpret_cast<float4*>(dst_a)[i] = v;
            reinterpret_cast<float4*>(dst_b)[i] = v;
        }
        for (int i = (n4 << 2) + threadIdx.x; i < len; i += THREADS) { const float v = src[i]; dst_a[i] = v; dst_b[i] = v; }
    } else {
        for (int i = threadIdx.x; i < len; i += THREADS) { const float v = src[i]; dst_a[i] = v; dst_b[i] = v; }
    }
}

// grid: one workgroup per table entry; dynamic LDS: ctx floats
__global__ __launch_bounds__(THREADS) void k_windows_push(const RowTable tab, float* __restrict__ buf, const float* __restrict__ fresh, float* __restrict__ win,
                                                          int n, int n_new) {
    extern __shared__ __attribute__((aligned(16))) float s_ctx[];
    const int i = blockIdx.x;
    const int ctx = n - n_new;
    float* row = buf + (int64_t)tab.row[i] * n;
    float* w = win + (int64_t)i * n;
    const float* nw = fresh + (int64_t)i * n_new;
    wg_copy(s_ctx, row + n_new, ctx);
    __syncthreads();                                                  // every read of the old row is done before any of its floats is written
    wg_copy2(row, w, s_ctx, ctx);
    wg_copy2(row + ctx, w + ctx, nw, n_new);
}

}  // namespace

extern "C" int mf_windows_push(float* buf, int n_rows, int n, const float* new_samples, int n_new, const int* rows, int m, float* win, void* stream) {
    MF_REQUIRE(buf, "windows_push: buf is a null pointer");
    MF_REQUIRE(new_samples, "windows_push: new_samples is a null pointer");
    MF_REQUIRE(rows, "windows_push: rows is a null pointer");
    MF_REQUIRE(win, "windows_push: win is a null pointer");
    MF_REQUIRE(m >= 1, "windows_push: m %d (at least one row)", m);
    MF_REQUIRE(n_rows >= 1, "windows_push: n_rows %d (at least one window in the pool)", n_rows);
    MF_REQUIRE(n_new >= 1 && n_new <= n, "windows_push: n_new %d must lie in [1, n = %d]", n_new, n);
    const int64_t ctx_bytes = (int64_t)(n - n_new) * 4;
    MF_REQUIRE(ctx_bytes <= LDS_BYTES, "windows_push: the kept context of %d floats (%lld bytes) is too large for the %lld bytes of LDS a workgroup has", n - n_new,
               (long long)ctx_bytes, (long long)LDS_BYTES);
    std::vector<int> sorted(rows, rows + m);
    for (int i = 0; i < m; ++i)
        MF_REQUIRE(rows[i] >= 0 && rows[i] < n_rows, "windows_push: row %d (entry %d) is out of range [0, %d)", rows[i], i, n_rows);
    std::sort(sorted.begin(), sorted.end());
    for (int i = 1; i < m; ++i)                                        // two workgroups on one row: a race within a launch, a double shift across two
        MF_REQUIRE(sorted[i] != sorted[i - 1], "windows_push: duplicate row %d", sorted[i]);
    // (win or the new samples inside the pool would be read while another workgroup writes them)
    const uintptr_t b0 = (uintptr_t)buf, b1 = b0 + (uintptr_t)n_rows * (uintptr_t)n * 4;
    const uintptr_t w0 = (uintptr_t)win, w1 = w0 + (uintptr_t)m * (uintptr_t)n * 4;
    const uintptr_t s0 = (uintptr_t)new_samples, s1 = s0 + (uintptr_t)m * (uintptr_t)n_new * 4;
    MF_REQUIRE(w1 <= b0 || b1 <= w0, "windows_push: win overlaps buf");
    MF_REQUIRE(s1 <= b0 || b1 <= s0, "windows_push: new_samples overlaps buf");
    MF_REQUIRE(s1 <= w0 || w1 <= s0, "windows_push: new_samples overlaps win");
    if (ctx_bytes > 64 * 1024)                                         // (above the default limit of dynamic LDS; per device, so not remembered)
        MF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_windows_push), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
    hipStream_t s = (hipStream_t)stream;
    RowTable tab;
    for (int first = 0; first < m; first += TABLE) {
        const int cnt = std::min(TABLE, m - first);
        for (int i = 0; i < TABLE; ++i) tab.row[i] = rows[first + std::min(i, cnt - 1)];      // (entries behind cnt repeat the last one: never read, never garbage)
        hipLaunchKernelGGL(k_windows_push, dim3((unsigned)cnt), dim3(THREADS), (size_t)ctx_bytes, s, tab, buf, new_samples + (int64_t)first * n_new,
                           win + (int64_t)first * n, n, n_new);
        MF_HIP(hipGetLastError());
    }
    return MF_OK;
}
