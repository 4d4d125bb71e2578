// The audio-feature pool of many ER-NeRF sessions (nerf_serving.NerfFeaturePool): what `NerfASR` keeps per session as torch tensors -- the feature ring
// `feat_queue` [R, dim] (nerfasr.py:48-50) and the attention windows `att_feats` (nerfasr.py:55, 75-103) -- for N sessions in two caller-owned buffers,
// served by stateless launches whatever the number of sessions:
//
//   k_nerf_feat_scatter   nerfasr.py:119-124 + :140-142: rows [left, right) of each picked session's slice of the net output into its ring
//   k_nerf_feat_windows   nerfasr.py:75-103: each picked session's new [dim, 16] windows out of its ring (transposed through LDS), into its circular
//                         history of eight, and the eight, oldest first, to the frame's `auds`
//   k_nerf_feat_rows_load a session joins, starts again or is reset: whole pool rows (ring and history) written from one snapshot row, or zeroed
//
// What the eight windows of a frame hold is what `torch.stack(self.att_feats)` reads at that moment.  A window whose rows wrap round the ring's end was built by
// `torch.cat` (nerfasr.py:81): a copy, which keeps its values -- the history.  A window that does not wrap is `feat_queue[front:tail].permute(1, 0)`
// (:79, 86): a VIEW of the ring, which shows whatever run_step has written under it since -- such a window is read from the ring again every frame.  The four
// zero windows of :55 are tensors of their own: history slots the caller has zeroed.
//
// All three only move fp32 values: the results are the reference's bits.  Session rows and positions travel as launch arguments (one struct of at most
// CHUNK sessions per launch); nothing is read back and nothing waits for the host.
#include "mf_common.h"
#include <vector>

namespace {

constexpr int NT = 256;
constexpr int CHUNK = 64;              // sessions per launch: 11 x 64 ints of launch arguments
constexpr int WIN = 16;                // rows of one attention window (nerfasr.py:52-53: tail - front = 16)
constexpr int HIST = 8;                // windows `auds` holds with att > 0 (nerfasr.py:77)
constexpr int TD = 64;                 // dims per tile: one 256-byte run of a ring row per wave
// Leading dimension of the LDS tile [WIN][TD]: ds_write_b32 / ds_read_b32 bank an address modulo 32 dwords within each half wave.  The writes go along a
// row (32 consecutive dwords: no conflict at any pitch).  The transposed reads of a half wave cover t = 0..15 of two neighbouring dims: t * PITCH + d must be
// distinct modulo 32 for those 32 lanes, which PITCH = 2 (mod 32) gives (2 t + d = 0..31); 65 would leave them two-way.
constexpr int PITCH = TD + 2;

struct ScatterArgs {
    int row[CHUNK];                    // session's row of the pool
    int start[CHUNK];                  // first ring row written (feat_buffer_idx * m)
};

struct WindowArgs {
    int row[CHUNK];
    int front[CHUNK][HIST];            // per window of `out`, oldest first: the ring row it starts at; -1: a zero window of nerfasr.py:55
    int head[CHUNK];                   // history slot the first new window goes to
    int n_new[CHUNK];                  // new windows of this call (the last n_new of `out`): 1, or 4 on a session's first call
};

struct LoadArgs {
    int row[CHUNK];
};

// grid (right - left, sessions of this launch).  One block copies one feature row.
__global__ __launch_bounds__(NT) void k_nerf_feat_scatter(const float* __restrict__ feats, int T, int dim, int left, float* __restrict__ rings, int R,
                                                          ScatterArgs a) {
    const int j = blockIdx.x, s = blockIdx.y;
    const float* src = feats + ((size_t)s * T + left + j) * dim;
    float* dst = rings + ((size_t)a.row[s] * R + a.start[s] + j) * dim;
    for (int d = threadIdx.x; d < dim; d += NT) dst[d] = src[d];
}

// grid (ceil(dim / TD), windows of `out` per session: HIST or 1, sessions of this launch).  One block produces one [TD, WIN] tile of one output window: a new
// window, and an older one that is a view, is read from the ring (rows along the lanes' dims: 256-byte runs), turned in LDS and written as one run of TD * WIN
// floats to `out` (a new one to its history slot too); an older copy is that run copied from its history slot.  New and old slots of a session are disjoint,
// so no block reads what another writes.
__global__ __launch_bounds__(NT) void k_nerf_feat_windows(const float* __restrict__ rings, float* __restrict__ hist, int R, int dim, int n_out, WindowArgs a,
                                                          float* __restrict__ out) {
    __shared__ float tile[WIN * PITCH];
    const int d0 = blockIdx.x * TD, i = blockIdx.y, s = blockIdx.z;
    const int row = a.row[s], n_new = a.n_new[s], head = a.head[s];
    const int n_tile = min(TD, dim - d0) * WIN;                        // floats of this tile, contiguous in a [dim, WIN] window from d0 * WIN
    float* o = out + ((size_t)s * n_out + i) * dim * WIN + (size_t)d0 * WIN;
    const int j = i - (n_out - n_new);                                 // >= 0: the j-th new window of this call
    const int first = a.front[s][i];
    if (j < 0 && (first < 0 || first + WIN >= R)) {                    // nerfasr.py:78-81: `front < tail` fails, the window was concatenated
        const int slot = (head + n_new + i) % HIST;                    // oldest first
        const float* h = hist + ((size_t)row * HIST + slot) * dim * WIN + (size_t)d0 * WIN;
        for (int e = threadIdx.x; e < n_tile; e += NT) o[e] = h[e];
        return;
    }
    const float* ring = rings + (size_t)row * R * dim;
#pragma unroll
    for (int e = threadIdx.x; e < WIN * TD; e += NT) {
        const int t = e / TD, d = e % TD;
        if (d0 + d < dim) tile[t * PITCH + d] = ring[(size_t)((first + t) % R) * dim + d0 + d];
    }
    __syncthreads();
    float* h = (hist && j >= 0) ? hist + ((size_t)row * HIST + (head + j) % HIST) * dim * WIN + (size_t)d0 * WIN : nullptr;
#pragma unroll
    for (int e = threadIdx.x; e < WIN * TD; e += NT) {
        if (e < n_tile) {
            const float v = tile[(e % WIN) * PITCH + e / WIN];         // `feat.permute(1, 0)`: [dim, 16]
            o[e] = v;
            if (h) h[e] = v;
        }
    }
}

// grid (blocks per row, rows of this launch).  A copy: every lane moves 16 bytes per access, a wave one 1 KiB run; the blocks of a row stride over the row's
// ring part and then over its history part.  R is a multiple of 4 and a history row is 128 * dim floats, so both parts are whole 16-byte groups and every row
// starts on one.  src == nullptr: zeros.  The host has checked that no source overlaps a named row, so nothing is read that this launch writes.
typedef float f4v __attribute__((ext_vector_type(4)));                // (the compiler's own vector: float4's union put the zero value on the stack)

__device__ __forceinline__ void load_part(f4v* __restrict__ dst, const f4v* __restrict__ src, int n4, int first, int step) {
    if (src) {
        for (int e = first; e < n4; e += step) dst[e] = src[e];
    } else {
        for (int e = first; e < n4; e += step) dst[e] = (f4v)(0.f);
    }
}

__global__ __launch_bounds__(NT) void k_nerf_feat_rows_load(f4v* __restrict__ rings, f4v* __restrict__ hist, int n4_ring, int n4_hist,
                                                            const f4v* __restrict__ src_ring, const f4v* __restrict__ src_hist, LoadArgs a) {
    const int row = a.row[blockIdx.y], first = blockIdx.x * NT + threadIdx.x, step = gridDim.x * NT;
    load_part(rings + (size_t)row * n4_ring, src_ring, n4_ring, first, step);
    if (hist) load_part(hist + (size_t)row * n4_hist, src_hist, n4_hist, first, step);
}

// every picked session once, inside the pool
int check_rows(const char* who, const int* rows, int n_sessions, int N) {
    std::vector<char> seen((size_t)N, 0);
    for (int s = 0; s < n_sessions; ++s) {
        MF_REQUIRE(rows[s] >= 0 && rows[s] < N, "%s: session row %d out of range (the pool holds %d sessions)", who, rows[s], N);
        MF_REQUIRE(!seen[rows[s]], "%s: session row %d appears twice", who, rows[s]);
        seen[rows[s]] = 1;
    }
    return MF_OK;
}

}  // namespace

extern "C" int mf_nerf_feat_scatter(const float* feats, int n_sessions, int T, int dim, int left, int right, float* rings, int N, int R,
                                    const int* rows, const int* starts, void* stream) {
    MF_REQUIRE(feats && rings && rows && starts, "nerf_feat_scatter: null argument");
    MF_REQUIRE(dim >= 1 && dim <= 1024, "nerf_feat_scatter: dim %d (1..1024)", dim);
    MF_REQUIRE(R >= WIN && R <= (1 << 16), "nerf_feat_scatter: a ring of %d rows (16..65536: a window is 16 rows)", R);
    MF_REQUIRE(N >= 1 && N <= (1 << 16), "nerf_feat_scatter: a pool of %d sessions (1..65536)", N);
    MF_REQUIRE(n_sessions >= 1 && n_sessions <= N, "nerf_feat_scatter: %d picked sessions of %d", n_sessions, N);
    MF_REQUIRE(T >= 1 && T <= (1 << 16) && left >= 0 && left < right && right <= T, "nerf_feat_scatter: rows [%d, %d) of %d net frames", left, right, T);
    const int n = right - left;
    if (const int rc = check_rows("nerf_feat_scatter", rows, n_sessions, N)) return rc;
    for (int s = 0; s < n_sessions; ++s)
        MF_REQUIRE(starts[s] >= 0 && (int64_t)starts[s] + n <= R, "nerf_feat_scatter: %d rows at ring row %d leave the ring of %d (nerfasr.py:123 raises there)", n,
                   starts[s], R);
    for (int s0 = 0; s0 < n_sessions; s0 += CHUNK) {
        const int ns = n_sessions - s0 < CHUNK ? n_sessions - s0 : CHUNK;
        ScatterArgs a{};
        for (int s = 0; s < ns; ++s) { a.row[s] = rows[s0 + s]; a.start[s] = starts[s0 + s]; }
        hipLaunchKernelGGL(k_nerf_feat_scatter, dim3(n, ns), dim3(NT), 0, (hipStream_t)stream, feats + (size_t)s0 * T * dim, T, dim, left, rings, R, a);
        MF_HIP(hipGetLastError());
    }
    return MF_OK;
}

extern "C" int mf_nerf_feat_windows(const float* rings, float* hist, int N, int R, int dim, int n_sessions, const int* rows, const int* fronts,
                                    const int* heads, const int* n_new, int att, float* out, void* stream) {
    MF_REQUIRE(rings && rows && fronts && n_new && out, "nerf_feat_windows: null argument");
    MF_REQUIRE(att == 0 || (hist && heads), "nerf_feat_windows: null history (att > 0 needs the eight windows nerfasr.py:55 keeps)");
    MF_REQUIRE(dim >= 1 && dim <= 1024, "nerf_feat_windows: dim %d (1..1024)", dim);
    MF_REQUIRE(R >= WIN && R <= (1 << 16), "nerf_feat_windows: a ring of %d rows (16..65536: a window is 16 rows)", R);
    MF_REQUIRE(N >= 1 && N <= (1 << 16), "nerf_feat_windows: a pool of %d sessions (1..65536)", N);
    MF_REQUIRE(n_sessions >= 1 && n_sessions <= N, "nerf_feat_windows: %d picked sessions of %d", n_sessions, N);
    if (const int rc = check_rows("nerf_feat_windows", rows, n_sessions, N)) return rc;
    const int n_out = att ? HIST : 1;
    for (int s = 0; s < n_sessions; ++s) {
        if (att) {
            MF_REQUIRE(heads[s] >= 0 && heads[s] < HIST, "nerf_feat_windows: history slot %d (0..7)", heads[s]);
            MF_REQUIRE(n_new[s] >= 1 && n_new[s] <= HIST, "nerf_feat_windows: %d new windows (1..8)", n_new[s]);
        } else {
            MF_REQUIRE(n_new[s] == 1, "nerf_feat_windows: %d new windows without attention (nerfasr.py:92-100 takes one)", n_new[s]);
        }
        for (int i = 0; i < n_out; ++i) {                              // a new window starts inside the ring; an older one may be a zero window (-1)
            const int f = fronts[(size_t)s * n_out + i];
            MF_REQUIRE(f < R && f >= (i >= n_out - n_new[s] ? 0 : -1), "nerf_feat_windows: front %d outside the ring of %d rows", f, R);
        }
    }
    for (int s0 = 0; s0 < n_sessions; s0 += CHUNK) {
        const int ns = n_sessions - s0 < CHUNK ? n_sessions - s0 : CHUNK;
        WindowArgs a{};
        for (int s = 0; s < ns; ++s) {
            a.row[s] = rows[s0 + s]; a.head[s] = att ? heads[s0 + s] : 0; a.n_new[s] = n_new[s0 + s];
            for (int i = 0; i < n_out; ++i) a.front[s][i] = fronts[(size_t)(s0 + s) * n_out + i];
        }
        hipLaunchKernelGGL(k_nerf_feat_windows, dim3((dim + TD - 1) / TD, n_out, ns), dim3(NT), 0, (hipStream_t)stream, rings, att ? hist : nullptr, R, dim,
                           n_out, a, out + (size_t)s0 * n_out * dim * WIN);
        MF_HIP(hipGetLastError());
    }
    return MF_OK;
}

extern "C" int mf_nerf_feat_rows_load(float* rings, float* hist, int N, int R, int dim, int n_rows, const int* rows, const float* src_ring,
                                      const float* src_hist, void* stream) {
    MF_REQUIRE(rings && rows, "nerf_feat_rows_load: null argument");
    MF_REQUIRE(hist || !src_hist, "nerf_feat_rows_load: null history with a history source (att == 0 keeps no history)");
    MF_REQUIRE(dim >= 1 && dim <= 1024, "nerf_feat_rows_load: dim %d (1..1024)", dim);
    MF_REQUIRE(R >= WIN && R <= (1 << 16) && R % 4 == 0, "nerf_feat_rows_load: a ring of %d rows (16..65536 and 4 * m: a row moves in 16-byte groups)", R);
    MF_REQUIRE(N >= 1 && N <= (1 << 16), "nerf_feat_rows_load: a pool of %d sessions (1..65536)", N);
    MF_REQUIRE(n_rows >= 1 && n_rows <= N, "nerf_feat_rows_load: %d picked sessions of %d", n_rows, N);
    for (const void* p : {(const void*)rings, (const void*)hist, (const void*)src_ring, (const void*)src_hist})
        MF_REQUIRE((uintptr_t)p % 16 == 0, "nerf_feat_rows_load: a buffer at %p is not 16-byte aligned", p);
    if (const int rc = check_rows("nerf_feat_rows_load", rows, n_rows, N)) return rc;
    const size_t ring_bytes = (size_t)R * dim * sizeof(float), hist_bytes = (size_t)HIST * dim * WIN * sizeof(float);
    for (int s = 0; s < n_rows; ++s) {                                 // a source may lie in the pool's own allocation (a scratch row), but not under a named row
        const uintptr_t r0 = (uintptr_t)rings + rows[s] * ring_bytes, h0 = (uintptr_t)hist + rows[s] * hist_bytes;
        MF_REQUIRE(!src_ring || (uintptr_t)src_ring + ring_bytes <= r0 || r0 + ring_bytes <= (uintptr_t)src_ring,
                   "nerf_feat_rows_load: the ring source overlaps session row %d", rows[s]);
        MF_REQUIRE(!src_hist || (uintptr_t)src_hist + hist_bytes <= h0 || h0 + hist_bytes <= (uintptr_t)src_hist,
                   "nerf_feat_rows_load: the history source overlaps session row %d", rows[s]);
    }
    const int n4_ring = (int)(ring_bytes / 16), n4_hist = hist ? (int)(hist_bytes / 16) : 0;
    const int most = n4_ring > n4_hist ? n4_ring : n4_hist;
    int blocks = (most + 4 * NT - 1) / (4 * NT);                       // four 16-byte groups per lane and part, up to 64 blocks a row
    blocks = blocks < 1 ? 1 : (blocks > 64 ? 64 : blocks);
    for (int s0 = 0; s0 < n_rows; s0 += CHUNK) {
        const int ns = n_rows - s0 < CHUNK ? n_rows - s0 : CHUNK;
        LoadArgs a{};
        for (int s = 0; s < ns; ++s) a.row[s] = rows[s0 + s];
        hipLaunchKernelGGL(k_nerf_feat_rows_load, dim3(blocks, ns), dim3(NT), 0, (hipStream_t)stream, (f4v*)rings, (f4v*)hist, n4_ring, n4_hist,
                           (const f4v*)src_ring, (const f4v*)src_hist, a);
        MF_HIP(hipGetLastError());
    }
    return MF_OK;
}
