// ER-NeRF occupancy-grid maintenance on gfx950: the four `_raymarching_face` entry points behind `NeRFRenderer.update_extra_state` / `mark_untrained_grid`
// (reference: ernerf/raymarching/src/raymarching.cu:214-335 -- morton3D, morton3D_invert, packbits, morton3D_dilation) and the head grid's whole rebuild
// (ernerf/nerf_triplane/renderer.py:437-485) as three launches that never leave the device:
//
//   k_density_sweep   one 16-wave workgroup owns 256 consecutive MORTON-ordered cells of one cascade (a wave 16 of them, one MFMA fragment column block).  A cell's
//                     index is inverted to (x, y, z), its sample position formed as renderer.py:458-467 forms it (float32 statement by statement, no contraction),
//                     and the density half of the field evaluated by field_tile<X3, DENS> (mf_nerf_field_tile.h: the same gathers and MFMA chain as
//                     k_nerf_field_fused, in the same precision mode).  sigma * density_scale goes to tmp_grid[cascade][morton]: contiguous stores, where the
//                     reference materialises coords / indices / xyzs / a noise tensor / three encoder outputs / ten GEMM results and scatters.
//   k_dilate_ema      six-neighbour max of tmp_grid in Morton order (raymarching.cu:304-335), the masked EMA of renderer.py:478-479, and an fp64 partial sum of
//                     max(grid, 0) per workgroup.  A lane owns the eight cells of one bitfield byte.
//   k_reduce_pack     every workgroup adds the partials in the same fixed order (no floating-point atomics: the mean is the same bits on every run), forms
//                     min(mean, density_thresh) and packs its 2048 cells (raymarching.cu:268-289).
#include "mf_nerf_field_tile.h"

namespace {

constexpr int NT = 128;                 // threads per block of the four shim kernels (the reference's N_THREAD)
constexpr int OCC_T = 256;              // threads per workgroup of k_dilate_ema / k_reduce_pack: 8 cells per lane, 2048 per workgroup
constexpr int OCC_CELLS = OCC_T * 8;
constexpr int MAX_CASCADES = 8;

// inverse of expand_bits (mf_nerf_march.h): every third bit of v, packed
__device__ __forceinline__ uint32_t compact_bits(uint32_t v) {
    v &= 0x49249249u;
    v = (v | (v >> 2)) & 0xC30C30C3u;
    v = (v | (v >> 4)) & 0x0F00F00Fu;
    v = (v | (v >> 8)) & 0xFF0000FFu;
    v = (v | (v >> 16)) & 0x0000FFFFu;
    return v;
}

__global__ __launch_bounds__(NT) void k_morton3d(const int* __restrict__ coords, uint32_t n, int* __restrict__ indices) {
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int* c = coords + (size_t)i * 3;
    indices[i] = (int)morton3d((uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2]);
}

__global__ __launch_bounds__(NT) void k_morton3d_invert(const int* __restrict__ indices, uint32_t n, int* __restrict__ coords) {
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int ind = indices[i];                       // the reference shifts the SIGNED index (raymarching.cu:249-253)
    int* c = coords + (size_t)i * 3;
    c[0] = (int)compact_bits((uint32_t)(ind >> 0));
    c[1] = (int)compact_bits((uint32_t)(ind >> 1));
    c[2] = (int)compact_bits((uint32_t)(ind >> 2));
}

// bit i of the byte of cells g[0..7]: g[i] > thresh (strict)
__device__ __forceinline__ uint32_t pack8(const float (&g)[8], float thresh) {
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) bits |= g[i] > thresh ? (1u << i) : 0u;
    return bits;
}
__device__ __forceinline__ void load8(const float* p, float (&g)[8]) {
    const float4 lo = reinterpret_cast<const float4*>(p)[0], hi = reinterpret_cast<const float4*>(p)[1];
    g[0] = lo.x; g[1] = lo.y; g[2] = lo.z; g[3] = lo.w; g[4] = hi.x; g[5] = hi.y; g[6] = hi.z; g[7] = hi.w;
}

__global__ __launch_bounds__(NT) void k_packbits(const float* __restrict__ grid, uint32_t n_bytes, float thresh, uint8_t* __restrict__ bitfield) {
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i >= n_bytes) return;
    float g[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = grid[(size_t)i * 8 + k];       // (no alignment is promised for a caller's grid)
    bitfield[i] = (uint8_t)pack8(g, thresh);
}

// max over cell `ind` of cascade `base` and its six neighbours, clipped at the borders (raymarching.cu:319-331)
__device__ __forceinline__ float dilate_cell(const float* __restrict__ base, uint32_t ind, uint32_t H) {
    const uint32_t x = compact_bits(ind), y = compact_bits(ind >> 1), z = compact_bits(ind >> 2);
    float r = base[ind];
    if (x + 1 < H) r = fmaxf(r, base[morton3d(x + 1, y, z)]);
    if (x > 0) r = fmaxf(r, base[morton3d(x - 1, y, z)]);
    if (y + 1 < H) r = fmaxf(r, base[morton3d(x, y + 1, z)]);
    if (y > 0) r = fmaxf(r, base[morton3d(x, y - 1, z)]);
    if (z + 1 < H) r = fmaxf(r, base[morton3d(x, y, z + 1)]);
    if (z > 0) r = fmaxf(r, base[morton3d(x, y, z - 1)]);
    return r;
}

__global__ __launch_bounds__(NT) void k_morton3d_dilation(const float* __restrict__ grid, uint32_t C, uint32_t H, float* __restrict__ out) {
    const uint32_t H3 = H * H * H;
    const uint32_t n = blockIdx.x * NT + threadIdx.x;
    if (n >= C * H3) return;
    const uint32_t c = n / H3, ind = n - c * H3;
    out[n] = dilate_cell(grid + (size_t)c * H3, ind, H);
}

// ---- the head grid's rebuild -------------------------------------------------------------------------------------------------------------------------
struct SweepArgs {
    uint32_t H, log2_H3;
    float inv_hm1;                       // 1 / (H - 1) in fp32: torch divides a tensor by a Python scalar as a product with the scalar's fp32 reciprocal
    float scale[MAX_CASCADES];           // float32(bound_c - half)      (renderer.py:462-465; the Python scalars are doubles, rounded when they meet the tensor)
    float half[MAX_CASCADES];            // float32(half) = float32(bound_c / H)
    const float* noise;                  // [C, H^3, 3] in meshgrid order ((x H + y) H + z), or null
    float* xyzs_out;                     // [C, H^3, 3] in Morton order, or null
};

// renderer.py:458, 465, 467 for one coordinate: every operation rounded to fp32 as written
__device__ __forceinline__ float cell_position(uint32_t c, float inv_hm1, float scale, float half, bool noisy, float u) {
#pragma clang fp contract(off)
    float v = 2.0f * (float)c;           // 2 * coords.float()
    v = v * inv_hm1;                     // / (grid_size - 1)
    v = v - 1.0f;                        // - 1
    v = v * scale;                       // * (bound - half_grid_size)
    if (noisy) {
        float r = u * 2.0f;              // torch.rand_like(...) * 2
        r = r - 1.0f;                    // - 1
        r = r * half;                    // * half_grid_size
        v = v + r;                       // cas_xyzs += ...
    }
    return v;
}

template <bool X3>
__global__ __launch_bounds__(NWAVE * 64) void k_density_sweep(const FusedArgs a, const SweepArgs w) {
    extern __shared__ __attribute__((aligned(16))) char smem[];     // NFRAG * NP KiB of weight fragments
    __shared__ LevelTab lt;
    __shared__ float s_scale[MAX_CASCADES], s_half[MAX_CASCADES];   // indexed by the tile's cascade: kernel-argument arrays cannot be indexed dynamically without scratch
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = threadIdx.x & 15, g = (threadIdx.x & 63) >> 4;
    if (threadIdx.x < MAX_CASCADES) { s_scale[threadIdx.x] = w.scale[threadIdx.x]; s_half[threadIdx.x] = w.half[threadIdx.x]; }
    field_stage_weights<X3>(a, smem, lt, NWAVE * 64);               // (ends with a barrier)
    const float eye_v = a.eye_dev ? *a.eye_dev : a.eye;
    const uint32_t H = w.H, H3m = (1u << w.log2_H3) - 1u;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int s0 = tile * TILE + wave * 16 * NSF;
        const uint32_t m = (uint32_t)min(s0 + fr, a.M - 1);        // H^3 is a multiple of the tile for every size served: the clamp only keeps a tail lane's reads in bounds
        const uint32_t cas = m >> w.log2_H3, ind = m & H3m;
        const uint32_t x = compact_bits(ind), y = compact_bits(ind >> 1), z = compact_bits(ind >> 2);
        const float sc = s_scale[cas], hf = s_half[cas];
        float u0 = 0.f, u1 = 0.f, u2 = 0.f;
        if (w.noise) {
            const float* u = w.noise + ((size_t)cas * (H3m + 1u) + ((size_t)x * H + y) * H + z) * 3;
            u0 = u[0]; u1 = u[1]; u2 = u[2];
        }
        const float qx = cell_position(x, w.inv_hm1, sc, hf, w.noise != nullptr, u0);
        const float qy = cell_position(y, w.inv_hm1, sc, hf, w.noise != nullptr, u1);
        const float qz = cell_position(z, w.inv_hm1, sc, hf, w.noise != nullptr, u2);
        if (w.xyzs_out && g == 0 && s0 + fr < a.M) {
            float* o = w.xyzs_out + (size_t)m * 3;
            o[0] = qx; o[1] = qy; o[2] = qz;
        }
        field_tile<X3, true>(a, smem, lt, eye_v, s0, a.M, qx, qy, qz);
    }
}

// fixed-order sum of the workgroup's OCC_T doubles (a tree over LDS: the same association on every run)
__device__ __forceinline__ double block_sum(double v, double* s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int d = OCC_T / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    return s[0];
}

__global__ __launch_bounds__(OCC_T) void k_dilate_ema(const float* __restrict__ tmp, float* __restrict__ grid, uint32_t H, uint32_t log2_H3, float decay,
                                                      double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double s[OCC_T];
    const uint32_t first = (blockIdx.x * OCC_T + threadIdx.x) * 8u;        // 8 | H^3: the eight cells lie in one cascade
    const uint32_t cas = first >> log2_H3, ind0 = first & ((1u << log2_H3) - 1u);
    const float* base = tmp + ((size_t)cas << log2_H3);
    float g[8];
    load8(grid + first, g);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float t = dilate_cell(base, ind0 + i, H);
        if (g[i] >= 0.f && t >= 0.f) g[i] = fmaxf(g[i] * decay, t);       // renderer.py:478-479; a cell marked -1 (or a NaN) stays
        acc += (double)fmaxf(g[i], 0.f);                                    // .clamp(min=0), :480
    }
    float4* o = reinterpret_cast<float4*>(grid + first);
    o[0] = make_float4(g[0], g[1], g[2], g[3]);
    o[1] = make_float4(g[4], g[5], g[6], g[7]);
    const double tot = block_sum(acc, s);
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

__global__ __launch_bounds__(OCC_T) void k_reduce_pack(const float* __restrict__ grid, const double* __restrict__ partials, uint32_t n_partials, double cells,
                                                       float density_thresh, uint8_t* __restrict__ bitfield, double* __restrict__ mean_out) {
    __shared__ double s[OCC_T];
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < n_partials; i += OCC_T) acc += partials[i];
    const double mean = block_sum(acc, s) / cells;
    if (blockIdx.x == 0 && threadIdx.x == 0) *mean_out = mean;
    const float thresh = fminf((float)mean, density_thresh);               // min(self.mean_density, self.density_thresh), renderer.py:484
    const uint32_t byte = blockIdx.x * OCC_T + threadIdx.x;
    float g[8];
    load8(grid + (size_t)byte * 8, g);
    bitfield[byte] = (uint8_t)pack8(g, thresh);
}

// ---- mark_untrained_grid (renderer.py:356-416) -------------------------------------------------------------------------------------------------------
constexpr int MARK_T = 256;             // one cell per lane; 256 | H^3, so a workgroup lies in one cascade
constexpr int MARK_POSES = 64;          // poses staged per round: 12 floats each (R row-major, then t)

struct MarkArgs {
    uint32_t H, log2_H3;
    int n_poses;
    float inv_hm1, kx, ky;               // float32(cx / fx), float32(cy / fy): Python scalars, rounded when they meet the tensor (:407-408)
    float scale[MAX_CASCADES];           // float32(bound_c - half_grid_size) (:394)
    float slack[MAX_CASCADES];           // float32(half_grid_size * 2)
};

// A cell is covered when some camera sees its centre inside the frustum widened by a cell (:402-409); the reference counts the cameras and reads only
// `count == 0` (:416), so the walk over the poses ends for a wave once each of its lanes has found one.
__global__ __launch_bounds__(MARK_T) void k_mark_untrained(const float* __restrict__ poses, float* __restrict__ grid, const MarkArgs a) {
#pragma clang fp contract(off)
    __shared__ float sp[MARK_POSES * 12];
    __shared__ float s_scale[MAX_CASCADES], s_slack[MAX_CASCADES];
    if (threadIdx.x < MAX_CASCADES) { s_scale[threadIdx.x] = a.scale[threadIdx.x]; s_slack[threadIdx.x] = a.slack[threadIdx.x]; }
    __syncthreads();
    const uint32_t n = blockIdx.x * MARK_T + threadIdx.x;
    const uint32_t cas = n >> a.log2_H3, ind = n & ((1u << a.log2_H3) - 1u);
    const float sc = s_scale[cas], h2 = s_slack[cas];
    const float px = cell_position(compact_bits(ind), a.inv_hm1, sc, 0.f, false, 0.f);
    const float py = cell_position(compact_bits(ind >> 1), a.inv_hm1, sc, 0.f, false, 0.f);
    const float pz = cell_position(compact_bits(ind >> 2), a.inv_hm1, sc, 0.f, false, 0.f);
    bool covered = false;
    for (int p0 = 0; p0 < a.n_poses; p0 += MARK_POSES) {
        const int np = min(MARK_POSES, a.n_poses - p0);
        for (int i = threadIdx.x; i < np * 12; i += MARK_T) {
            const int p = i / 12, k = i - p * 12;                                      // k < 9: R[k / 3][k % 3], else t[k - 9]
            sp[i] = poses[(size_t)(p0 + p) * 16 + (k < 9 ? (k / 3) * 4 + k % 3 : (k - 9) * 4 + 3)];
        }
        __syncthreads();
        for (int p = 0; p < np && !__all(covered); ++p) {
            const float* q = sp + p * 12;
            const float dx = px - q[9], dy = py - q[10], dz = pz - q[11];             // cas_world_xyzs - poses[:, :3, 3]
            const float cx = dx * q[0] + dy * q[3] + dz * q[6];                        // @ poses[:, :3, :3]
            const float cy = dx * q[1] + dy * q[4] + dz * q[7];
            const float cz = dx * q[2] + dy * q[5] + dz * q[8];
            covered = covered || (cz > 0.f && fabsf(cx) < a.kx * cz + h2 && fabsf(cy) < a.ky * cz + h2);
        }
        if (!__syncthreads_or(!covered)) break;                                        // (also the barrier in front of the next round's staging)
    }
    if (!covered) grid[n] = -1.0f;
}

inline unsigned blocks(uint64_t n) { return (unsigned)((n + NT - 1) / NT); }

}  // namespace

// ---- C ABI: the four shim entry points ------------------------------------------------------------------------------------------------------------------
extern "C" int mf_morton3d(const int* coords, uint32_t n, int* indices, void* stream) {
    MF_REQUIRE(coords && indices, "morton3D: null argument");
    if (n == 0) return MF_OK;
    hipLaunchKernelGGL(k_morton3d, dim3(blocks(n)), dim3(NT), 0, (hipStream_t)stream, coords, n, indices);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_morton3d_invert(const int* indices, uint32_t n, int* coords, void* stream) {
    MF_REQUIRE(indices && coords, "morton3D_invert: null argument");
    if (n == 0) return MF_OK;
    hipLaunchKernelGGL(k_morton3d_invert, dim3(blocks(n)), dim3(NT), 0, (hipStream_t)stream, indices, n, coords);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_packbits(const float* grid, uint32_t n_bytes, float thresh, uint8_t* bitfield, void* stream) {
    MF_REQUIRE(grid && bitfield, "packbits: null argument");
    if (n_bytes == 0) return MF_OK;
    hipLaunchKernelGGL(k_packbits, dim3(blocks(n_bytes)), dim3(NT), 0, (hipStream_t)stream, grid, n_bytes, thresh, bitfield);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_morton3d_dilation(const float* grid, uint32_t C, uint32_t H, float* out, void* stream) {
    MF_REQUIRE(grid && out && grid != out, "morton3D_dilation: null or aliased argument");
    MF_REQUIRE(H >= 1 && H <= 1024 && C >= 1 && (uint64_t)C * H * H * H < (1ull << 32), "morton3D_dilation: C=%u H=%u (H <= 1024: 10 bits per axis; C * H^3 < 2^32)", C, H);
    hipLaunchKernelGGL(k_morton3d_dilation, dim3(blocks((uint64_t)C * H * H * H)), dim3(NT), 0, (hipStream_t)stream, grid, C, H, out);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

// ---- the rebuild: called by mf_nerf_density_grid_update (mf_nerf_net.hip, where the field handle is defined) after mf_nerf_occupancy_shape accepted the sizes ----------------------------------------------
// the sizes served (checked here once: for the launch below, for mf_nerf_mark_untrained and for the torso grid of mf_nerf_torso_grid_update) and the number of
// per-workgroup partial sums the head grid needs
int mf_nerf_occupancy_shape(const char* what, int cascades, int grid_size, size_t* n_partials) {
    MF_REQUIRE(grid_size == 32 || grid_size == 64 || grid_size == 128, "%s: grid_size %d is not served (32, 64 or 128)", what, grid_size);
    MF_REQUIRE(cascades >= 1 && cascades <= MAX_CASCADES, "%s: cascades %d outside 1..%d", what, cascades, MAX_CASCADES);
    *n_partials = (size_t)cascades * grid_size * grid_size * grid_size / OCC_CELLS;
    return MF_OK;
}

int mf_nerf_occupancy_launch(const NerfFieldConsts& f, const NerfFrameInputs& in, const NerfGridBufs& g, int cascades, int grid_size, float bound, float decay,
                             float density_thresh, const float* noise, hipStream_t s) {
    MF_REQUIRE(bound > 0.f, "nerf_density_grid_update: bound must be positive");
    const uint32_t H = (uint32_t)grid_size, log2_H3 = grid_size == 32 ? 15u : (grid_size == 64 ? 18u : 21u);
    const int cells = cascades << log2_H3;
    FusedArgs a{};
    int rc;
    if ((rc = fused_args(a, f, in, nullptr, nullptr, cells, NerfFieldOut{g.tmp_grid, nullptr, nullptr, nullptr, nullptr}))) return rc;
    SweepArgs w{};
    w.H = H; w.log2_H3 = log2_H3; w.inv_hm1 = 1.0f / (float)(H - 1); w.noise = noise; w.xyzs_out = g.xyzs_out;
    for (int c = 0; c < cascades; ++c) {
        // `bound = min(2 ** cas, self.bound)`, `half_grid_size = bound / self.grid_size`: Python floats (doubles)
        const double bc = std::min((double)(1 << c), (double)bound), half = bc / (double)grid_size;
        w.scale[c] = (float)(bc - half);
        w.half[c] = (float)half;
    }
    const size_t lds = (size_t)NFRAG * (f.x3 ? 2 : 1) * 1024;
    static bool attr_done[2] = {false, false};
    if ((rc = f.x3 ? fused_lds_attr(k_density_sweep<true>, attr_done[1], lds) : fused_lds_attr(k_density_sweep<false>, attr_done[0], lds))) return rc;
    const int grid = std::min(a.ntiles, 256);
    if (f.x3) hipLaunchKernelGGL(k_density_sweep<true>, dim3(grid), dim3(NWAVE * 64), lds, s, a, w);
    else hipLaunchKernelGGL(k_density_sweep<false>, dim3(grid), dim3(NWAVE * 64), lds, s, a, w);
    MF_HIP(hipGetLastError());
    const unsigned nwg = (unsigned)(cells / OCC_CELLS);
    hipLaunchKernelGGL(k_dilate_ema, dim3(nwg), dim3(OCC_T), 0, s, g.tmp_grid, g.density_grid, H, log2_H3, decay, g.partials);
    MF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_reduce_pack, dim3(nwg), dim3(OCC_T), 0, s, g.density_grid, g.partials, nwg, (double)cells, density_thresh, g.bitfield, g.mean_density);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_nerf_mark_untrained(const float* poses, int n_poses, double fx, double fy, double cx, double cy, float bound, int cascades, int grid_size,
                                      float* density_grid, void* stream) {
    MF_REQUIRE(poses && density_grid, "nerf_mark_untrained: null argument");
    MF_REQUIRE(n_poses >= 1, "nerf_mark_untrained: n_poses %d: at least one pose is needed (with none every cell would be marked untrained)", n_poses);
    MF_REQUIRE(bound > 0.f && fx != 0.0 && fy != 0.0, "nerf_mark_untrained: bound and the focal lengths must be non-zero");
    size_t unused = 0;
    int rc;
    if ((rc = mf_nerf_occupancy_shape("nerf_mark_untrained", cascades, grid_size, &unused))) return rc;
    MarkArgs a{};
    a.H = (uint32_t)grid_size; a.log2_H3 = grid_size == 32 ? 15u : (grid_size == 64 ? 18u : 21u);
    a.n_poses = n_poses; a.inv_hm1 = 1.0f / (float)(grid_size - 1);
    a.kx = (float)(cx / fx); a.ky = (float)(cy / fy);
    for (int c = 0; c < cascades; ++c) {
        // `bound = min(2 ** cas, self.bound)`, `half_grid_size = bound / self.grid_size`: Python floats (doubles)
        const double bc = std::min((double)(1 << c), (double)bound), half = bc / (double)grid_size;
        a.scale[c] = (float)(bc - half);
        a.slack[c] = (float)(half * 2);
    }
    const unsigned nwg = (unsigned)(((size_t)cascades << a.log2_H3) / MARK_T);
    hipLaunchKernelGGL(k_mark_untrained, dim3(nwg), dim3(MARK_T), 0, (hipStream_t)stream, poses, density_grid, a);
    MF_HIP(hipGetLastError());
    return MF_OK;
}
