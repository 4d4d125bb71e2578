// ER-NeRF torso branch as ONE kernel on gfx950: `run_torso` (reference: ernerf/nerf_triplane/renderer.py:294-352) over
// `forward_torso` (network.py:166-201) -- frequency encoding of the pixel, the deform MLP, the warp, the 16-level tiled 2-D grid
// encoder, the colour / alpha MLP, the occupancy mask and the background mix -- one lane per pixel, nothing but the frame in HBM.
//
// Why not MFMA: the two MLPs are 32 wide (5 440 multiply-adds per pixel, 1.4 GMAC per 512 x 512 frame).  As six GEMM launches
// (mf_nerf_net.hip, kept behind MF_TORSO=gemm) every layer moved a [N, 32..72] (hi, lo) tensor out and back and the chain of
// twelve launches took ~0.42 ms of a 1.0 ms frame; the arithmetic itself is ~25 us of fp32 FMAs.  Here a lane keeps its pixel's
// 34 frequency features and 32 grid features in registers and parks each 32-wide activation in its own column of a 32 KB LDS slab (no
// barrier: a lane reads only what it wrote); the weights are wave-uniform, so they reach v_fmac as SGPR operands (s_load of one weight
// row at a time from the 21 KB table: scalar cache / L2).
// Arithmetic is plain fp32 (one fused multiply-add per weight; even and odd inputs of a row in two partial sums) in BOTH precision modes: closer to the reference's fp32
// nets than the bf16x3 GEMMs were.  Everything outside the dense layers rounds as written (contraction off), so the frequency
// features, the warp and the grid features are bit-identical to mf_freq_encode_forward / mf_grid_encode_forward.
#include "mf_nerf_host.h"
#include "mf_nerf_frame_batch.h"
#include "mf_nerf_grid.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int FQ = 34, TG = 32, HID = 32, NLEV = 16;
// row-major [out][in] fp32 tables, concatenated: deform net 34 -> 32 -> 32 -> 2, torso net (32 + 34) -> 32 -> 32 -> 4
constexpr int W_D1 = 0, W_D2 = W_D1 + HID * FQ, W_D3 = W_D2 + HID * HID, W_T1 = W_D3 + 2 * HID, W_T2 = W_T1 + HID * (TG + FQ),
              W_T3 = W_T2 + HID * HID, W_TOTAL = W_T3 + 4 * HID;

struct TorsoFusedArgs {
    const float *bg_coords, *w, *emb, *density, *bg;
    float bias_d[HID], bias_t[HID];               // per-frame: W[:, constant inputs] . [freq(wrapped anchors) | individual code]
    float scale[NLEV];
    uint32_t resolution[NLEV], offset[NLEV], hashmap_size[NLEV];
    float shrink, thresh, bg_const;
    int bg_per_ray, G, N;
    float *out, *alpha_out, *deform;
    // the grid sweep (k_torso_fused<true>): the jitter [G^2, 2] in meshgrid order (row x G + y) or null, the positions out (same order) or null, and the
    // Python scalars of renderer.py:511-514 as the float32 values they take when they meet the tensor
    const float* noise;
    float* xys_out;
    float inv_gm1, cell_scale, cell_half;
    // several frames in one launch (k_torso_fused<T_BATCH>): the frame table; what is per frame above (bg_coords, bg, the biases, thresh, bg_const, bg_per_ray and
    // the outputs) is then read from frames[blockIdx.y]
    const NerfTorsoFrame* frames;
};

constexpr int T_FRAME = 0, T_SWEEP = 1, T_BATCH = 2;      // what a launch of k_torso_fused walks: one frame's pixels, the occupancy grid's cells, several frames' pixels

// the frequency features' sine is the reference's own: freqencoder.cu:56 calls __sinf -- the hardware sine of x / 2 pi -- and so does k_freq_encode (mf_nerf.hip);
// rounds 3 - 4 called the accurate sinf() here, 32 range reductions of ~50 instructions per pixel: a quarter of the kernel's VALU work for a feature the
// reference does not compute that way
__device__ __forceinline__ float torso_sin(float x) { return __sinf(x); }

// The weight table is read through the CONSTANT address space: a uniform load from it is always a scalar load (s_load -> SGPR operand of
// v_pk_fma), whatever stores the kernel has issued before -- through a global pointer the compiler falls back to per-lane
// global_load_dwordx4 as soon as it cannot prove the table unclobbered (the LDS slab writes below are enough).
typedef const __attribute__((address_space(4))) float* cw_ptr;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) f32x2* cw2_ptr;

// One output of a layer: the inputs are register PAIRS (x[2j], x[2j+1]), the weight row arrives as aligned SGPR pairs straight from
// s_load, and v_pk_fma_f32 accumulates the even and the odd inputs in the two halves of one register pair -- two multiply-adds per lane and
// instruction with no SGPR shuffling (packing two ROWS instead, which the vectoriser does on its own, costs 52 s_mov + 30 s_nop per 34
// packed instructions to build the pairs).  Every row of the table starts on an even index (all layer widths are even).
template <int IN2>
__device__ __forceinline__ float row_dot(cw_ptr wr, float bias, const f32x2 (&x)[IN2]) {
    cw2_ptr w2 = (cw2_ptr)wr;
    f32x2 acc = {bias, 0.f};
    // <= 17 weight pairs in flight: the 66-wide row goes in two halves (all 66 scalars at once overflow the ~100 SGPRs and spill into VGPR lanes)
#pragma unroll
    for (int c = 0; c < IN2; c += 17) {
#pragma unroll
        for (int j = c; j < (c + 17 < IN2 ? c + 17 : IN2); ++j) acc = __builtin_elementwise_fma(w2[j], x[j], acc);
        if (c + 17 < IN2) __builtin_amdgcn_sched_barrier(0);
    }
    return acc.x + acc.y;
}

// A layer: the inputs sit in registers, the OUTPUT ROW is a real loop -- one weight row is live at a time instead of the whole table (fully
// unrolled, the scheduler hoists every s_load to the top and spills 3 200 SGPRs; the same holds for the 2- and 4-output layers, whose
// loads otherwise migrate into the loop in front of them).  Output o goes to this lane's column of an LDS slab ([32][256] floats; a lane only
// ever touches its own column, so there is no barrier), from where the next stage reads it back with compile-time indices.
template <int IN2, int OUT, bool RELU, bool BIAS>
__device__ __forceinline__ void dense_to_lds(cw_ptr w, const float* __restrict__ bias, const f32x2 (&x)[IN2], float* col) {
    if constexpr (OUT % 2 == 0) {
        // two rows per iteration: their s_loads go out together, and two independent
        // accumulator chains interleave -- a lone chain of v_pk_fma_f32 pays a wait state after every instruction (the packed op's result is not forwarded)
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int o = 0; o < OUT; o += 2) {
            cw2_ptr w0 = (cw2_ptr)(w + o * 2 * IN2), w1 = (cw2_ptr)(w + (o + 1) * 2 * IN2);
            f32x2 a0 = {BIAS ? bias[o] : 0.f, 0.f}, a1 = {BIAS ? bias[o + 1] : 0.f, 0.f};
            // <= 17 weight pairs of each row in flight (2 x 34 scalars): the 66-wide rows go in two halves -- all of a pair of them at once overflows the ~100 SGPRs
#pragma unroll
            for (int c = 0; c < IN2; c += 17) {
#pragma unroll
                for (int j = c; j < (c + 17 < IN2 ? c + 17 : IN2); ++j) {
                    a0 = __builtin_elementwise_fma(w0[j], x[j], a0);
                    a1 = __builtin_elementwise_fma(w1[j], x[j], a1);
                }
                if (c + 17 < IN2) __builtin_amdgcn_sched_barrier(0);
            }
            const float v0 = a0.x + a0.y, v1 = a1.x + a1.y;
            col[o * 256] = RELU ? fmaxf(v0, 0.f) : v0;
            col[(o + 1) * 256] = RELU ? fmaxf(v1, 0.f) : v1;
        }
    } else {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int o = 0; o < OUT; ++o) {
            const float v = row_dot<IN2>(w + o * 2 * IN2, BIAS ? bias[o] : 0.f, x);
            col[o * 256] = RELU ? fmaxf(v, 0.f) : v;
        }
    }
}
__device__ __forceinline__ void from_lds(const float* col, f32x2 (&x)[HID / 2]) {
#pragma unroll
    for (int j = 0; j < HID / 2; ++j) x[j] = f32x2{col[2 * j * 256], col[(2 * j + 1) * 256]};
}

// renderer.py:511-514 for one coordinate of a torso grid cell: every operation rounded to fp32 as written (contraction is off in this file)
__device__ __forceinline__ float torso_cell_position(int c, float inv_gm1, float scale, float half, bool noisy, float u) {
    float v = 2.0f * (float)c;           // 2 * coords.float()
    v = v * inv_gm1;                     // / (grid_size - 1): a tensor over a Python scalar is a product with the scalar's fp32 reciprocal
    v = v - 1.0f;                        // - 1
    v = v * scale;                       // * (1 - half_grid_size)
    if (noisy) {
        float r = u * 2.0f;              // torch.rand_like(xys) * 2
        r = r - 1.0f;                    // - 1
        r = r * half;                    // * half_grid_size
        v = v + r;                       // xys += ...
    }
    return v;
}

// SWEEP off: one frame of `run_torso`, a lane per pixel of bg_coords.  SWEEP on: the torso branch of `update_extra_state` (renderer.py:506-519), a lane per
// cell of the G x G occupancy grid -- lane n is cell (x, y) = (n % G, n / G), its point formed by torso_cell_position, the same per-point arithmetic, and the
// raw alpha stored at alpha_out[y G + x] = alpha_out[n] (the reference's transposed index, :510) with no occupancy mask and no colour mix.
// T_BATCH: T_FRAME for the frames of a table, the frame in blockIdx.y -- every frame has its own ceil(N / 256) workgroups (the last one partial), so a pixel
// sits in the lane and the workgroup it has in a launch of its frame alone, and runs the same statements.
template <int MODE>
__global__ __launch_bounds__(256) void k_torso_fused(const TorsoFusedArgs a) {
    constexpr bool SWEEP = MODE == T_SWEEP, BATCH = MODE == T_BATCH;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= a.N) return;
    // the frame's table entry: read-only for the whole launch, so its uniform loads may be scalar loads like the weights'
    const NerfTorsoFrame* fr = BATCH ? a.frames + blockIdx.y : nullptr;
    const float* bias_d = a.bias_d;
    const float* bias_t = a.bias_t;
    const float* bg_coords = a.bg_coords;
    if constexpr (BATCH) { bias_d = fr->bias_d; bias_t = fr->bias_t; bg_coords = fr->bg_coords; }
    float2 bc;
    int sweep_row = 0;
    if constexpr (SWEEP) {
        const int cx = n % a.G, cy = n / a.G;
        sweep_row = cx * a.G + cy;
        float u0 = 0.f, u1 = 0.f;
        if (a.noise) {
            const float2 u = *reinterpret_cast<const float2*>(a.noise + 2 * (size_t)sweep_row);
            u0 = u.x; u1 = u.y;
        }
        bc.x = torso_cell_position(cx, a.inv_gm1, a.cell_scale, a.cell_half, a.noise != nullptr, u0);
        bc.y = torso_cell_position(cy, a.inv_gm1, a.cell_scale, a.cell_half, a.noise != nullptr, u1);
    } else {
        bc = *reinterpret_cast<const float2*>(bg_coords + 2 * (size_t)n);
    }
    // TH / TX: [grid 32 | x 2 | sin, cos of 2^f x, f = 0..7 (freqencoder.cu:30-58: sinf(scalbnf(x, f) + phase)) ]
    f32x2 in[(TG + FQ) / 2];                      // pairs 0..15: grid features, 16..32: frequency features
    float fq[FQ];
    fq[0] = bc.x * a.shrink;
    fq[1] = bc.y * a.shrink;
#pragma unroll
    for (int col = 0; col < 16; ++col)
#pragma unroll
        for (int d = 0; d < 2; ++d) fq[2 + 2 * col + d] = torso_sin(scalbnf(fq[d], col >> 1) + (float)(col & 1) * 1.57079632679489661923f);
#pragma unroll
    for (int j = 0; j < FQ / 2; ++j) in[TG / 2 + j] = f32x2{fq[2 * j], fq[2 * j + 1]};

    // deform net (network.py:177-185): [freq(x) | anchors | code] -> 32 -> 32 -> 2, the constant inputs folded into bias_d
    __shared__ float slab[HID * 256];
    float* col = slab + threadIdx.x;
    cw_ptr w = (cw_ptr)a.w;
    float dx[2];
    {
        f32x2 fqv[FQ / 2], h[HID / 2];
#pragma unroll
        for (int j = 0; j < FQ / 2; ++j) fqv[j] = in[TG / 2 + j];
        dense_to_lds<FQ / 2, HID, true, true>(w + W_D1, bias_d, fqv, col);
        from_lds(col, h);
        dense_to_lds<HID / 2, HID, true, false>(w + W_D2, nullptr, h, col);
        from_lds(col, h);
        dense_to_lds<HID / 2, 2, false, false>(w + W_D3, nullptr, h, col);
        dx[0] = col[0];
        dx[1] = col[256];
    }
    // x2 = clamp(x + dx, -1, 1) (network.py:187), mapped to [0, 1] for the tiled grid (grid.py:144, bound 1)
    float u[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float x2 = fminf(fmaxf(fq[k] + dx[k], -1.f), 1.f);
        u[k] = (x2 + 1.f) * 0.5f;
    }
    // torso_encoder: tiled grid, D = 2, C = 2, 16 levels, align_corners off (gridencoder.cu:76-165, as k_grid_encode<2, 2>)
    const bool oob = u[0] < 0 || u[0] > 1 || u[1] < 0 || u[1] > 1;
#pragma unroll
    for (int l = 0; l < NLEV; ++l) {
        float r0 = 0, r1 = 0;
        if (!oob) {
            const float* grid = a.emb + (size_t)a.offset[l] * 2;
            float pos[2];
            uint32_t pg[2];
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                pos[d] = u[d] * a.scale[l] + 0.5f;
                pg[d] = (uint32_t)floorf(pos[d]);
                pos[d] -= (float)pg[d];
            }
#pragma unroll
            for (uint32_t idx = 0; idx < 4; ++idx) {
                float w = 1;
                uint32_t pl[2];
#pragma unroll
                for (uint32_t d = 0; d < 2; ++d) {
                    if ((idx & (1u << d)) == 0) { w *= 1 - pos[d]; pl[d] = pg[d]; }
                    else { w *= pos[d]; pl[d] = pg[d] + 1; }
                }
                // get_grid_index (gridencoder.cu:54-72) for D = 2, C = 2, the tiled type, with the level's constants -- wave-uniform kernel arguments -- deciding
                // on the SCALAR unit what the lanes must do: a level whose (res + 1)^2 cells fit the table is addressed directly (`% hashmap_size` is the
                // identity there: no instruction), a larger one wraps by a mask when the table is a power of two (2^log2_hashmap_size, grid.py:108-123) and by
                // the division only otherwise.  grid_index<2>() divided for all 64 corners of a pixel: ~1 600 of the kernel's VALU instructions.
                const uint32_t hs = a.hashmap_size[l], s1 = a.resolution[l] + 1;
                uint32_t index = pl[0];
                if (s1 <= hs) index += pl[1] * s1;
                if (!(s1 <= hs && s1 * s1 <= hs)) index = (hs & (hs - 1)) == 0 ? (index & (hs - 1)) : index % hs;
                index *= 2;
                const float2 g = *reinterpret_cast<const float2*>(grid + index);          // index is a multiple of C = 2: 8-byte aligned
                r0 += w * g.x;
                r1 += w * g.y;
            }
        }
        in[l] = f32x2{r0, r1};
    }
    // torso net (network.py:189-199): [grid | freq(x) | anchors | code] -> 32 -> 32 -> 4, sigmoid
    float o4[4];
    {
        f32x2 h[HID / 2];
        dense_to_lds<(TG + FQ) / 2, HID, true, true>(w + W_T1, bias_t, in, col);
        from_lds(col, h);
        dense_to_lds<HID / 2, HID, true, false>(w + W_T2, nullptr, h, col);
        from_lds(col, h);
        dense_to_lds<HID / 2, 4, false, false>(w + W_T3, nullptr, h, col);
#pragma unroll
        for (int k = 0; k < 4; ++k) o4[k] = col[k * 256];
    }
    if constexpr (SWEEP) {
        // alpha = sigmoid(.) * 1.002 - 0.001 (network.py:198) at every cell: `forward_torso` itself has no mask
        if (a.xys_out) *reinterpret_cast<float2*>(a.xys_out + 2 * (size_t)sweep_row) = bc;
        a.alpha_out[n] = (1.f / (1.f + __expf(-o4[0]))) * 1.002f - 0.001f;
        return;
    }
    // occupancy = grid_sample(density_grid_torso, bg_coords, align_corners=True) (renderer.py:326), mask = occupancy > thresh;
    // alpha / colour = sigmoid(.) * 1.002 - 0.001 (network.py:198-199); bg = colour * alpha + bg * (1 - alpha) (renderer.py:343)
    const int G = a.G;
    const float gx = (bc.x + 1.f) * 0.5f * (float)(G - 1), gy = (bc.y + 1.f) * 0.5f * (float)(G - 1);
    const float fx = floorf(gx), fy = floorf(gy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float wx = gx - fx, wy = gy - fy;
    auto at = [&](int y, int x) { return (x >= 0 && x < G && y >= 0 && y < G) ? a.density[y * G + x] : 0.f; };   // zeros padding
    const float occ = at(y0, x0) * (1 - wx) * (1 - wy) + at(y0, x0 + 1) * wx * (1 - wy) + at(y0 + 1, x0) * (1 - wx) * wy + at(y0 + 1, x0 + 1) * wx * wy;
    float thresh = a.thresh, bg_const = a.bg_const;
    int bg_per_ray = a.bg_per_ray;
    const float* bg = a.bg;
    float *out = a.out, *alpha_out = a.alpha_out, *deform = a.deform;
    if constexpr (BATCH) {
        thresh = fr->thresh; bg_const = fr->bg_const; bg_per_ray = fr->bg_per_ray; bg = fr->bg;
        out = fr->out; alpha_out = fr->alpha_out; deform = fr->deform;
    }
    const bool m = occ > thresh;
    float sg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) sg[k] = m ? (1.f / (1.f + __expf(-o4[k]))) * 1.002f - 0.001f : 0.f;
    // every store sits behind the last weight load: a load the compiler can prove unclobbered since kernel entry becomes a scalar load
    if (deform) *reinterpret_cast<float2*>(deform + 2 * (size_t)n) = make_float2(dx[0], dx[1]);
    if (alpha_out) alpha_out[n] = sg[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float b = bg ? (bg_per_ray ? bg[3 * (size_t)n + k] : bg[k]) : bg_const;
        out[3 * (size_t)n + k] = sg[1 + k] * sg[0] + b * (1.f - sg[0]);
    }
}

// ---- after the sweep: renderer.py:522-528 ------------------------------------------------------------------------------------------------------------
constexpr int TG_T = 256;                 // threads per workgroup of k_torso_dilate_ema: one cell per lane (256 | G^2 for every size served)

// F.max_pool2d(raw, kernel_size=5, stride=1, padding=2) (the padding is -inf: it never wins, and alpha can be -0.001), grid = max(grid * decay, pooled), and the
// workgroup's fp64 sum of the new cells, added over LDS in a fixed tree (no floating-point atomics: the same bits on every run)
__global__ __launch_bounds__(TG_T) void k_torso_dilate_ema(const float* __restrict__ raw, float* __restrict__ grid, int G, float decay, double* __restrict__ partials) {
    __shared__ double s[TG_T];
    const int n = blockIdx.x * TG_T + threadIdx.x, x = n % G, y = n / G;
    float m = -INFINITY;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const int yy = y + dy, xx = x + dx;
            if (yy >= 0 && yy < G && xx >= 0 && xx < G) m = fmaxf(m, raw[yy * G + xx]);
        }
    const float g = fmaxf(grid[n] * decay, m);
    grid[n] = g;
    s[threadIdx.x] = (double)g;
    __syncthreads();
    for (int d = TG_T / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = s[0];
}

// torch.mean(density_grid_torso) (renderer.py:528): the <= 64 partial sums added in index order by one lane
__global__ void k_torso_grid_mean(const double* __restrict__ partials, int n_partials, double cells, float* __restrict__ mean_out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double acc = 0.0;
    for (int i = 0; i < n_partials; ++i) acc += partials[i];
    *mean_out = (float)(acc / cells);
}

// bias: null for a batch (the biases are in the frame table)
int torso_args(TorsoFusedArgs& a, const NerfTorsoConsts& t, const float* bias, int N) {
    a.w = t.w; a.emb = t.emb;
    for (int i = 0; bias && i < HID; ++i) { a.bias_d[i] = bias[i]; a.bias_t[i] = bias[HID + i]; }
    GridLevels lv;
    if (const int rc = mf_grid_levels(lv, t.offsets, NLEV, t.log2_pls, (uint32_t)t.base_res)) return rc;
    for (int l = 0; l < NLEV; ++l) { a.scale[l] = lv.scale[l]; a.resolution[l] = lv.resolution[l]; a.offset[l] = lv.offset[l]; a.hashmap_size[l] = lv.hashmap_size[l]; }
    a.shrink = t.shrink; a.G = t.G; a.N = N;
    return MF_OK;
}

}  // namespace

int mf_nerf_torso_fused_weight_count() { return W_TOTAL; }

// t.w: device table laid out as W_D1 .. W_T3 above
int mf_nerf_torso_fused_launch(const NerfTorsoConsts& t, const float* bias, const float* density, const float* bg_coords, float thresh, const float* bg,
                               int bg_per_ray, float bg_const, int N, float* out, float* alpha_out, float* deform, hipStream_t s) {
    TorsoFusedArgs a{};
    int rc;
    if ((rc = torso_args(a, t, bias, N))) return rc;
    a.bg_coords = bg_coords; a.density = density; a.bg = bg;
    a.thresh = thresh; a.bg_const = bg_const; a.bg_per_ray = bg_per_ray;
    a.out = out; a.alpha_out = alpha_out; a.deform = deform;
    hipLaunchKernelGGL(k_torso_fused<T_FRAME>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, a);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

// tab_dev: n_frames entries on the device (the caller has checked every frame's pointers, N > 0 and 1 <= n_frames <= 64)
int mf_nerf_torso_batch_launch(const NerfTorsoConsts& t, const NerfTorsoFrame* tab_dev, int n_frames, const float* density, int N, hipStream_t s) {
    TorsoFusedArgs a{};
    int rc;
    if ((rc = torso_args(a, t, nullptr, N))) return rc;
    a.density = density; a.frames = tab_dev;
    hipLaunchKernelGGL(k_torso_fused<T_BATCH>, dim3((unsigned)((N + 255) / 256), (unsigned)n_frames), dim3(256), 0, s, a);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

// The torso grid's rebuild (mf_nerf_torso_grid_update, mf_nerf_net.hip, where the handle is defined): sweep, dilate + EMA, mean.  The served sizes were accepted by
// mf_nerf_occupancy_shape.
int mf_nerf_torso_grid_launch(const NerfTorsoConsts& t, const float* bias, const float* noise, float decay, float* density_grid, float* raw_grid, float* xys_out,
                              float* mean, double* partials, hipStream_t s) {
    const int G = t.G, cells = G * G;
    TorsoFusedArgs a{};
    int rc;
    if ((rc = torso_args(a, t, bias, cells))) return rc;
    a.alpha_out = raw_grid; a.noise = noise; a.xys_out = xys_out;
    // `half_grid_size = 1 / self.grid_size` and `1 - half_grid_size` are Python floats (doubles), rounded when they meet the float32 tensor
    const double half = 1.0 / (double)G;
    a.inv_gm1 = 1.0f / (float)(G - 1); a.cell_scale = (float)(1.0 - half); a.cell_half = (float)half;
    const int nwg = cells / TG_T;
    hipLaunchKernelGGL(k_torso_fused<T_SWEEP>, dim3((unsigned)nwg), dim3(256), 0, s, a);
    MF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_torso_dilate_ema, dim3((unsigned)nwg), dim3(TG_T), 0, s, raw_grid, density_grid, G, decay, partials);
    MF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_torso_grid_mean, dim3(1), dim3(64), 0, s, partials, nwg, (double)cells, mean);
    MF_HIP(hipGetLastError());
    return MF_OK;
}
