// Device functions of the fused ER-NeRF radiance field shared by its kernels: k_nerf_field_fused and k_loop_tail (mf_nerf_fused.hip) and the occupancy-grid sweep
// k_density_sweep (mf_nerf_occupancy.hip).  One copy of the gathers, the MFMA layer chain and the weight staging; what the layout is and why is told at the top of
// mf_nerf_fused.hip.
#pragma once
#include "mf_nerf_host.h"
#include "mf_nerf_grid.h"
#include "mf_nerf_march.h"
#include <cmath>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

namespace {

constexpr int NLEV = 12;
constexpr int NSF = 1;          // 16-sample fragments per wave (2 halves the weight reads per MFMA but spills past 256 VGPRs)
constexpr int NWAVE = 16;            // waves per workgroup: ONE workgroup fits a CU (126 KB of weight fragments), so its size IS the occupancy --
                                     // 16 waves = 4 per SIMD hide the gather latency twice as well as 8 did (the kernel needs 120 VGPRs <= 128)
constexpr int TILE = NWAVE * 16 * NSF;   // samples per workgroup tile
// fragment table: (first fragment, out blocks, k-steps) per layer, fragment = blk * nks + ks
enum { L_AUD0, L_AUD1, L_EYE0, L_EYE1, L_SIG0, L_SIG1, L_SIG2, L_COL0, L_COL1, NLAYER };
constexpr int L_NBLK[NLAYER] = {4, 2, 1, 1, 4, 4, 5, 4, 1};
constexpr int L_NKS[NLAYER] = {2, 2, 2, 1, 3, 2, 2, 4, 2};
constexpr int frag_base(int l) { int b = 0; for (int i = 0; i < l; ++i) b += L_NBLK[i] * L_NKS[i]; return b; }
constexpr int NFRAG = frag_base(NLAYER);      // 63

struct FusedArgs {
    const float *xyzs, *dirs, *enc_a, *ind;
    const float* deltas;             // the march's (dt, t) per sample slot, or null: a slot with dt == 0 holds no sample (the ray ended, or missed) and is not evaluated
    const float* emb[3];
    const bf16_t* w;                 // packed fragments [NFRAG][planes][64 lanes][8]
    float scale[NLEV];
    uint32_t resolution[NLEV], offset[NLEV], hashmap_size[NLEV];
    float bound, eye;
    int n_ind, has_eye, M, ntiles;
    const int* M_dev;                // device-side sample count (sync-free render loop), or null
    const float* eye_dev;            // the eye feature read from device memory (mf_nerf_head_set_eye: no host copy of a value that lives on the device), or null
    float sigma_scale;               // NeRFRenderer.density_scale (renderer.py:261)
    float *sigmas, *rgbs, *amb_aud, *amb_eye, *unc;
};

// a B fragment half (4 channels of one 16-block): bf16 (hi, lo) pairs of 4 fp32 values -> 2 + 2 dwords
struct Half { uint32_t h[2], l[2]; };
// (hi, lo) split of two values with gfx950's packed converter: v_cvt_pk_bf16_f32 rounds to nearest even exactly as mf_bf16_rne() does, and the whole
// split is 5 instructions where the integer form needs ~23 -- the kernel packs ~30 of these quads per 16 samples and is VALU-bound
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split2(float v0, float v1, uint32_t& h, uint32_t& l) {
    const f32x2_t v = {v0, v1};
    h = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
    const f32x2_t back = {__uint_as_float(h << 16), __uint_as_float(h & 0xffff0000u)};
    l = __builtin_bit_cast(uint32_t, __builtin_convertvector(v - back, bf16x2_t));
}
__device__ __forceinline__ Half pack4(float v0, float v1, float v2, float v3) {
    Half r;
    split2(v0, v1, r.h[0], r.l[0]);
    split2(v2, v3, r.h[1], r.l[1]);
    return r;
}
__device__ __forceinline__ Half zero_half() { Half r; r.h[0] = r.h[1] = r.l[0] = r.l[1] = 0u; return r; }
struct BFrag { bf16x8 hi, lo; };
__device__ __forceinline__ BFrag join(const Half& p0, const Half& p1) {
    BFrag f;
    f.hi = __builtin_bit_cast(bf16x8, u32x4{p0.h[0], p0.h[1], p1.h[0], p1.h[1]});
    f.lo = __builtin_bit_cast(bf16x8, u32x4{p0.l[0], p0.l[1], p1.l[0], p1.l[1]});
    return f;
}

// per-level constants in LDS: the level index differs from lane to lane, which kernel-argument arrays cannot serve
struct LevelTab { float scale[NLEV]; uint32_t resolution[NLEV], offset[NLEV], hashmap_size[NLEV], mask[NLEV]; };   // mask: hashmap_size - 1 if that is a power of two, else 0

// One 16-sample fragment per wave of the radiance field: samples s0 .. s0 + 15 (those below M) of a.xyzs / a.dirs -> a.sigmas, a.rgbs, a.amb_*, a.unc.
// `smem`: the NFRAG * NP KiB of weight fragments, `lt`: the level constants, both already in LDS.  A sample's result depends on nothing but that sample
// (a column of every MFMA), so any launch shape that calls this gets the same bits.
// DENS: the density half only (`NeRFNetwork.density`, network.py:280-308), for the occupancy-grid sweep.  The lane's sample position is (qx, qy, qz), not a read of
// a.xyzs; no SH, no colour net, and of sigma_net's last layer only the block that holds row 0; the one output is a.sigmas[s0 + lane % 16] = sigma_scale * exp(row 0).
template <bool X3, bool DENS = false>
__device__ __forceinline__ void field_tile(const FusedArgs& a, const char* smem, const LevelTab& lt, const float eye_v, const int s0, const int M, const float qx = 0.f,
                                           const float qy = 0.f, const float qz = 0.f) {
    constexpr int NP = X3 ? 2 : 1;
    const int lane = threadIdx.x & 63, fr = lane & 15, g = lane >> 4;
    const float* const emb0 = a.emb[0];
    const float* const emb1 = a.emb[1];
    const float* const emb2 = a.emb[2];

    auto wfrag = [&](int f, int plane) __attribute__((always_inline)) {
        return *reinterpret_cast<const bf16x8*>(smem + ((size_t)(f * NP + plane) * 64 + lane) * 16);
    };
    // acc[blk][sf] += W(layer, blk, ks) * B[sf]
    auto mma = [&](int f, const BFrag (&b)[NSF], f32x4 (&acc)[NSF]) __attribute__((always_inline)) {
        const bf16x8 whi = wfrag(f, 0);
        if constexpr (X3) {
            const bf16x8 wlo = wfrag(f, 1);
#pragma unroll
            for (int sf = 0; sf < NSF; ++sf) {
                acc[sf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wlo, b[sf].hi, acc[sf], 0, 0, 0);
                acc[sf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(whi, b[sf].lo, acc[sf], 0, 0, 0);
            }
        }
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) acc[sf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(whi, b[sf].hi, acc[sf], 0, 0, 0);
    };
    // between layers: stops the scheduler from hoisting the next layers' 1-KiB weight fragments into registers early
#define LAYER_FENCE() __builtin_amdgcn_sched_barrier(0)

    // The reference runs the network over every slot of the round's [n_alive x n_step] tensors, the zero-filled ones of rays that produced fewer samples included
    // (renderer.py:258-261); composite_rays stops at a slot with dt == 0 before it reads that slot's outputs (raymarching.cu:2180).  A fragment whose 16 slots are
    // all empty -- rays that miss the head in round 1 lie side by side, ended rays leave whole runs -- is skipped: same frame, fewer gathers and MFMAs.
    if (!DENS && a.deltas) {
        const int mq = s0 + fr;
        const bool has = mq < M && a.deltas[2 * (size_t)mq] != 0.f;
        if (!__any(has)) return;
    }
    // (x + bound) / (2 bound), grid.py:144, as a DIVISION: a product with fl(1 / (2 bound)) is the same float only when 2 bound is a power of two (at bound 1.5 it
    // moved a coordinate by one ulp, 9e-5 on a finest-level feature)
    const float two_b = 2.f * a.bound;
    {
        // ---- inputs of this lane's two samples ------------------------------------------------------------------
        float px[NSF], py[NSF], pz[NSF], dx[NSF], dy[NSF], dz[NSF];
        bool live[NSF];
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) {
            int m = s0 + sf * 16 + fr;
            live[sf] = m < M;
            m = live[sf] ? m : M - 1;
            if constexpr (DENS) {
                px[sf] = __fdiv_rn(qx + a.bound, two_b); py[sf] = __fdiv_rn(qy + a.bound, two_b); pz[sf] = __fdiv_rn(qz + a.bound, two_b);
                dx[sf] = dy[sf] = dz[sf] = 0.f;
            } else {
                px[sf] = __fdiv_rn(a.xyzs[3 * m] + a.bound, two_b); py[sf] = __fdiv_rn(a.xyzs[3 * m + 1] + a.bound, two_b); pz[sf] = __fdiv_rn(a.xyzs[3 * m + 2] + a.bound, two_b);
                dx[sf] = a.dirs[3 * m]; dy[sf] = a.dirs[3 * m + 1]; dz[sf] = a.dirs[3 * m + 2];
            }
        }
        // enc_x channel c = plane * 12 + level (network.py:204-219).  The contraction order of a layer is free (the weights are packed to it on the host), so the 36
        // channels are dealt to a sample's four lanes by LEVEL: lane group g gathers levels g, g + 4, g + 8 of all three planes -- nine lookups in every lane (the
        // block order 0..15 | 16..31 | 32..35 gave lane group 0 twelve and made the wave wait for them), the plane of every lookup a compile-time constant (its table a
        // scalar base, its coordinate pair fixed) and the level arithmetic -- constants from LDS, floor / fraction of x, y, z, dense-or-hashed -- done once per level
        // instead of once per lookup.  Values per channel are bit-identical to the per-channel form of rounds 3 - 4.  Slots: X0 = (l0 p0, l0 p1, l0 p2, l1 p0), X1 = (l1 p1, l1 p2, l2 p0,
        // l2 p1), X2 = (l2 p2, 0, 0, 0) of the lane's own three levels (mf_nerf_fused_pack: xblock()).
        Half x0[NSF], x1[NSF], x2[NSF];
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) {
            const bool okx = px[sf] >= 0.f && px[sf] <= 1.f, oky = py[sf] >= 0.f && py[sf] <= 1.f, okz = pz[sf] >= 0.f && pz[sf] <= 1.f;
            // outside [0, 1] a plane's feature is 0 (gridencoder.cu:96-104); the clamp only keeps the discarded lookup's addresses inside the table
            const float cx = __builtin_amdgcn_fmed3f(px[sf], 0.f, 1.f), cy = __builtin_amdgcn_fmed3f(py[sf], 0.f, 1.f), cz = __builtin_amdgcn_fmed3f(pz[sf], 0.f, 1.f);
            float v[3][3];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int lv = g + 4 * t;
                const float scale = lt.scale[lv];
                const uint32_t res = lt.resolution[lv], hs = lt.hashmap_size[lv], msk = lt.mask[lv], off = lt.offset[lv];
                const uint32_t s1 = res + 1;
                const bool dense = s1 * s1 <= hs;
                float fx = cx * scale + 0.5f, fy = cy * scale + 0.5f, fz = cz * scale + 0.5f;
                const float flx = floorf(fx), fly = floorf(fy), flz = floorf(fz);
                const uint32_t ix = (uint32_t)flx, iy = (uint32_t)fly, iz = (uint32_t)flz;
                fx -= flx; fy -= fly; fz -= flz;
                // one plane of this level (gridencoder.cu:76-165 with D = 2, C = 1, hash grid): get_grid_index (gridencoder.cu:54-72) for the four corners at once.
                // With s = res + 1 the level is DENSE iff s * s <= hashmap_size (then index = x + y s, below s * s, so `% hashmap_size` is the identity); otherwise
                // index = x ^ (y * 2654435761) reduced mod hashmap_size -- a mask when the table is a power of two (2^log2_hashmap_size: grid.py:108-123), the
                // division for any other size.  One multiply per form instead of one of each per corner, and no 32-bit urem (~25 instructions) per lookup.
                auto plane = [&](const float* __restrict__ tab, uint32_t iu, uint32_t iv, float pu, float pv, bool ok) __attribute__((always_inline)) {
                    // (a dense level's table size is (res + 1)^2 rounded up to 8 -- not a power of two: taking the hashed form first and selecting afterwards, as
                    // rounds 3 - 4 did, ran the four divisions for every dense level and threw the results away)
                    uint32_t i00, i10, i01, i11;
                    if (dense) {
                        i00 = iu + iv * s1; i10 = i00 + 1; i01 = i00 + s1; i11 = i01 + 1;
                    } else {
                        const uint32_t h0 = iv * 2654435761u, h1 = h0 + 2654435761u;
                        i00 = iu ^ h0; i10 = (iu + 1) ^ h0; i01 = iu ^ h1; i11 = (iu + 1) ^ h1;
                        if (msk) { i00 &= msk; i10 &= msk; i01 &= msk; i11 &= msk; }
                        else { i00 %= hs; i10 %= hs; i01 %= hs; i11 %= hs; }
                    }
                    // scalar table base + 32-bit byte offset (the tables are a few MB): no 64-bit address arithmetic per corner
                    const char* base = reinterpret_cast<const char*>(tab);
                    const float g00 = *reinterpret_cast<const float*>(base + ((off + i00) << 2)), g10 = *reinterpret_cast<const float*>(base + ((off + i10) << 2));
                    const float g01 = *reinterpret_cast<const float*>(base + ((off + i01) << 2)), g11 = *reinterpret_cast<const float*>(base + ((off + i11) << 2));
                    const float qu = 1.f - pu, qv = 1.f - pv;
                    float r = 0.f;                     // corner order and arithmetic of the reference's loop: (0,0), (1,0), (0,1), (1,1)
                    r += (qu * qv) * g00;
                    r += (pu * qv) * g10;
                    r += (qu * pv) * g01;
                    r += (pu * pv) * g11;
                    return ok ? r : 0.f;
                };
                v[t][0] = plane(emb0, ix, iy, fx, fy, okx && oky);                // xy
                v[t][1] = plane(emb1, iy, iz, fy, fz, oky && okz);                // yz
                v[t][2] = plane(emb2, ix, iz, fx, fz, okx && okz);                // xz
                __builtin_amdgcn_sched_barrier(0);      // keep the 12 gathers of one level together, not all 36 of the lane in flight
            }
            x0[sf] = pack4(v[0][0], v[0][1], v[0][2], v[1][0]);
            x1[sf] = pack4(v[1][1], v[1][2], v[2][0], v[2][1]);
            x2[sf] = pack4(v[2][2], 0.f, 0.f, 0.f);
        }
        const Half Z = zero_half();
        BFrag bx0[NSF], bx1[NSF];
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) {
            bx0[sf] = join(x0[sf], x1[sf]);                                      // k-step (X0, X1)
            bx1[sf] = join(x2[sf], Z);                                           // k-step (X2, 0)
        }

        // ---- aud_ch_att_net: 36 -> 64 relu -> 32 (network.py:148, 284-285) ---------------------------------------
        f32x4 h1[4][NSF];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            for (int sf = 0; sf < NSF; ++sf) h1[blk][sf] = f32x4{0.f, 0.f, 0.f, 0.f};
            mma(frag_base(L_AUD0) + blk * 2 + 0, bx0, h1[blk]);
            mma(frag_base(L_AUD0) + blk * 2 + 1, bx1, h1[blk]);
        }
        LAYER_FENCE();
        // ReLU as ONE integer instruction on the float's bits (v_max_i32 with 0: non-negative floats are non-negative integers, every negative one -- -0 included --
        // becomes +0); fmaxf() costs two (it first quiets its operand) and the kernel is VALU-bound
        auto relu1 = [](float x) __attribute__((always_inline)) { const int b = __float_as_int(x); return __int_as_float(b > 0 ? b : 0); };
        auto relu_half = [&](const f32x4& v) __attribute__((always_inline)) { return pack4(relu1(v[0]), relu1(v[1]), relu1(v[2]), relu1(v[3])); };
        auto lin_half = [&](const f32x4& v) __attribute__((always_inline)) { return pack4(v[0], v[1], v[2], v[3]); };
        BFrag t0[NSF], t1[NSF];
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) {
            t0[sf] = join(relu_half(h1[0][sf]), relu_half(h1[1][sf]));
            t1[sf] = join(relu_half(h1[2][sf]), relu_half(h1[3][sf]));
        }
        LAYER_FENCE();
        f32x4 aud[2][NSF];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            for (int sf = 0; sf < NSF; ++sf) aud[blk][sf] = f32x4{0.f, 0.f, 0.f, 0.f};
            mma(frag_base(L_AUD1) + blk * 2 + 0, t0, aud[blk]);
            mma(frag_base(L_AUD1) + blk * 2 + 1, t1, aud[blk]);
        }
        LAYER_FENCE();
        // ambient_aud = ||aud_ch_att||_2 (network.py:306): 8 channels in this lane, the other 24 in lanes g' != g of the same sample
        float amb[NSF];
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) {
            float n2 = 0.f;
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int e = 0; e < 4; ++e) n2 += aud[blk][sf][e] * aud[blk][sf][e];
            n2 += __shfl_xor(n2, 16);
            n2 += __shfl_xor(n2, 32);
            amb[sf] = sqrtf(n2);
        }
        // enc_w = enc_a * aud_ch_att (network.py:286): this lane's channels 16*blk + 4g + e
        Half ew[2][NSF];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const float4 ea = *reinterpret_cast<const float4*>(a.enc_a + blk * 16 + 4 * g);
#pragma unroll
            for (int sf = 0; sf < NSF; ++sf)
                ew[blk][sf] = pack4(ea.x * aud[blk][sf][0], ea.y * aud[blk][sf][1], ea.z * aud[blk][sf][2], ea.w * aud[blk][sf][3]);
        }

        LAYER_FENCE();
        // ---- eye_att_net: 36 -> 16 relu -> 1, sigmoid (network.py:137, 291-292) ----------------------------------
        float eye_att[NSF];
        Half eyeh[NSF];
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) { eye_att[sf] = 0.f; eyeh[sf] = Z; }
        if (a.has_eye) {
            f32x4 e1[NSF], e2[NSF];
            BFrag te[NSF];
#pragma unroll
            for (int sf = 0; sf < NSF; ++sf) e1[sf] = e2[sf] = f32x4{0.f, 0.f, 0.f, 0.f};
            mma(frag_base(L_EYE0) + 0, bx0, e1);
            mma(frag_base(L_EYE0) + 1, bx1, e1);
#pragma unroll
            for (int sf = 0; sf < NSF; ++sf) te[sf] = join(relu_half(e1[sf]), Z);
            mma(frag_base(L_EYE1), te, e2);
#pragma unroll
            for (int sf = 0; sf < NSF; ++sf) {
                // row 0 of the block lives in lanes g == 0 (element 0); the other lanes hold zero-weight rows
                const float s = 1.f / (1.f + __expf(-e2[sf][0]));
                eye_att[sf] = s;
                eyeh[sf] = g == 0 ? pack4(eye_v * s, 0.f, 0.f, 0.f) : Z;
            }
        }

        LAYER_FENCE();
        // ---- sigma_net: [enc_x 36 | enc_w 32 | e 1] -> 64 -> 64 -> 65 (network.py:139, 294-302) -------------------
        BFrag bs1[NSF], bs2[NSF];
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) {
            bs1[sf] = join(x2[sf], ew[0][sf]);                                   // k-step (X2, W0)
            bs2[sf] = join(ew[1][sf], eyeh[sf]);                                 // k-step (W1, eye)
        }
        f32x4 s1[4][NSF];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            for (int sf = 0; sf < NSF; ++sf) s1[blk][sf] = f32x4{0.f, 0.f, 0.f, 0.f};
            mma(frag_base(L_SIG0) + blk * 3 + 0, bx0, s1[blk]);
            mma(frag_base(L_SIG0) + blk * 3 + 1, bs1, s1[blk]);
            mma(frag_base(L_SIG0) + blk * 3 + 2, bs2, s1[blk]);
        }
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) {
            t0[sf] = join(relu_half(s1[0][sf]), relu_half(s1[1][sf]));
            t1[sf] = join(relu_half(s1[2][sf]), relu_half(s1[3][sf]));
        }
        LAYER_FENCE();
        f32x4 s2[4][NSF];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            for (int sf = 0; sf < NSF; ++sf) s2[blk][sf] = f32x4{0.f, 0.f, 0.f, 0.f};
            mma(frag_base(L_SIG1) + blk * 2 + 0, t0, s2[blk]);
            mma(frag_base(L_SIG1) + blk * 2 + 1, t1, s2[blk]);
        }
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) {
            t0[sf] = join(relu_half(s2[0][sf]), relu_half(s2[1][sf]));
            t1[sf] = join(relu_half(s2[2][sf]), relu_half(s2[3][sf]));
        }
        LAYER_FENCE();
        constexpr int NB3 = DENS ? 1 : 5;                                       // the sweep needs row 0 alone
        f32x4 s3[5][NSF];
#pragma unroll
        for (int blk = 0; blk < NB3; ++blk) {
            for (int sf = 0; sf < NSF; ++sf) s3[blk][sf] = f32x4{0.f, 0.f, 0.f, 0.f};
            mma(frag_base(L_SIG2) + blk * 2 + 0, t0, s3[blk]);
            mma(frag_base(L_SIG2) + blk * 2 + 1, t1, s3[blk]);
        }
        // row 0 = log sigma (lanes g == 0, element 0); rows 1..64 = geo_feat (network.py:300-301)
        if constexpr (DENS) {
            static_assert(!DENS || NSF == 1, "the sweep passes one position per lane");
            if (g == 0 && live[0]) a.sigmas[s0 + fr] = a.sigma_scale * expf(s3[0][0][0]);
            return;
        }

        LAYER_FENCE();
        // ---- colour_net: [geo (blocks 0..4) | SH 16 | ind 4] -> 64 -> 3 (network.py:144, 262-272) -----------------
        Half shh[NSF], indh;
        {
            const float4 iv = g == 0 ? make_float4(a.n_ind > 0 ? a.ind[0] : 0.f, a.n_ind > 1 ? a.ind[1] : 0.f, a.n_ind > 2 ? a.ind[2] : 0.f,
                                                   a.n_ind > 3 ? a.ind[3] : 0.f)
                                     : (g == 1 ? make_float4(a.n_ind > 4 ? a.ind[4] : 0.f, a.n_ind > 5 ? a.ind[5] : 0.f, a.n_ind > 6 ? a.ind[6] : 0.f,
                                                             a.n_ind > 7 ? a.ind[7] : 0.f)
                                               : make_float4(0.f, 0.f, 0.f, 0.f));
            indh = pack4(iv.x, iv.y, iv.z, iv.w);
        }
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) {
            const float x = dx[sf], y = dy[sf], z = dz[sf];
            const float xy = x * y, xz = x * z, yz = y * z, x2_ = x * x, y2 = y * y, z2 = z * z;
            float sh[16];
            sh[0] = 0.28209479177387814f;
            sh[1] = -0.48860251190291987f * y; sh[2] = 0.48860251190291987f * z; sh[3] = -0.48860251190291987f * x;
            sh[4] = 1.0925484305920792f * xy; sh[5] = -1.0925484305920792f * yz; sh[6] = 0.94617469575755997f * z2 - 0.31539156525251999f;
            sh[7] = -1.0925484305920792f * xz; sh[8] = 0.54627421529603959f * x2_ - 0.54627421529603959f * y2;
            sh[9] = 0.59004358992664352f * y * (-3.0f * x2_ + y2); sh[10] = 2.8906114426405538f * xy * z;
            sh[11] = 0.45704579946446572f * y * (1.0f - 5.0f * z2); sh[12] = 0.3731763325901154f * z * (5.0f * z2 - 3.0f);
            sh[13] = 0.45704579946446572f * x * (1.0f - 5.0f * z2); sh[14] = 1.4453057213202769f * z * (x2_ - y2);
            sh[15] = 0.59004358992664352f * x * (-x2_ + 3.0f * y2);
            float v0 = sh[0], v1 = sh[1], v2 = sh[2], v3 = sh[3];
            if (g == 1) { v0 = sh[4]; v1 = sh[5]; v2 = sh[6]; v3 = sh[7]; }
            if (g == 2) { v0 = sh[8]; v1 = sh[9]; v2 = sh[10]; v3 = sh[11]; }
            if (g == 3) { v0 = sh[12]; v1 = sh[13]; v2 = sh[14]; v3 = sh[15]; }
            shh[sf] = pack4(v0, v1, v2, v3);
        }
        BFrag c0[NSF], c1[NSF], c2[NSF], c3[NSF];
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) {
            c0[sf] = join(lin_half(s3[0][sf]), lin_half(s3[1][sf]));
            c1[sf] = join(lin_half(s3[2][sf]), lin_half(s3[3][sf]));
            c2[sf] = join(lin_half(s3[4][sf]), shh[sf]);
            c3[sf] = join(indh, Z);
        }
        LAYER_FENCE();
        f32x4 k1[4][NSF];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            for (int sf = 0; sf < NSF; ++sf) k1[blk][sf] = f32x4{0.f, 0.f, 0.f, 0.f};
            mma(frag_base(L_COL0) + blk * 4 + 0, c0, k1[blk]);
            mma(frag_base(L_COL0) + blk * 4 + 1, c1, k1[blk]);
            mma(frag_base(L_COL0) + blk * 4 + 2, c2, k1[blk]);
            mma(frag_base(L_COL0) + blk * 4 + 3, c3, k1[blk]);
        }
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) {
            t0[sf] = join(relu_half(k1[0][sf]), relu_half(k1[1][sf]));
            t1[sf] = join(relu_half(k1[2][sf]), relu_half(k1[3][sf]));
        }
        LAYER_FENCE();
        f32x4 rgb[NSF];
#pragma unroll
        for (int sf = 0; sf < NSF; ++sf) rgb[sf] = f32x4{0.f, 0.f, 0.f, 0.f};
        mma(frag_base(L_COL1) + 0, t0, rgb);
        mma(frag_base(L_COL1) + 1, t1, rgb);

        LAYER_FENCE();
        // ---- outputs: lanes g == 0 hold row 0 of sigma_net (element 0) and rows 0..2 of colour_net ---------------
        if (g == 0) {
#pragma unroll
            for (int sf = 0; sf < NSF; ++sf) {
                if (!live[sf]) continue;
                const int m = s0 + sf * 16 + fr;
                a.sigmas[m] = a.sigma_scale * expf(s3[0][sf][0]);                                                   // network.py:300
#pragma unroll
                for (int k = 0; k < 3; ++k) a.rgbs[3 * m + k] = 1.f / (1.f + __expf(-rgb[sf][k])) * 1.002f - 0.001f;   // network.py:272
                a.amb_aud[m] = amb[sf];
                a.amb_eye[m] = eye_att[sf];
                if (a.unc) a.unc[m] = 0.69314718055994530942f;
            }
        }
    }
}

// weight fragments and level constants into LDS (every thread of the workgroup; ends with a barrier)
template <bool X3>
__device__ __forceinline__ void field_stage_weights(const FusedArgs& a, char* smem, LevelTab& lt, int nthreads) {
    constexpr int NP = X3 ? 2 : 1;
    const int tid = threadIdx.x;
    for (int i = tid; i < NFRAG * NP * 64; i += nthreads)
        reinterpret_cast<u32x4*>(smem)[i] = reinterpret_cast<const u32x4*>(a.w)[i];
    if (tid < NLEV) { lt.scale[tid] = a.scale[tid]; lt.resolution[tid] = a.resolution[tid]; lt.offset[tid] = a.offset[tid]; lt.hashmap_size[tid] = a.hashmap_size[tid]; lt.mask[tid] = (a.hashmap_size[tid] & (a.hashmap_size[tid] - 1)) == 0 ? a.hashmap_size[tid] - 1 : 0u; }
    __syncthreads();
}

// the kernel arguments for M samples at xyzs / dirs (M_dev: their count on the device, deltas: see FusedArgs)
static int fused_args(FusedArgs& a, const NerfFieldConsts& f, const NerfFrameInputs& in, const float* xyzs, const float* dirs, int M, const NerfFieldOut& out,
                      const int* M_dev = nullptr, const float* deltas = nullptr) {
    a.M_dev = M_dev; a.sigma_scale = in.sigma_scale; a.eye_dev = in.eye_dev; a.deltas = deltas;
    a.xyzs = xyzs; a.dirs = dirs; a.enc_a = in.enc_a; a.ind = in.ind; a.w = f.packed;
    for (int p = 0; p < 3; ++p) a.emb[p] = f.emb[p];
    GridLevels lv;
    if (const int rc = mf_grid_levels(lv, f.offsets, NLEV, f.log2_pls, (uint32_t)f.base_res)) return rc;
    for (int l = 0; l < NLEV; ++l) { a.scale[l] = lv.scale[l]; a.resolution[l] = lv.resolution[l]; a.offset[l] = lv.offset[l]; a.hashmap_size[l] = lv.hashmap_size[l]; }
    a.bound = f.bound; a.eye = in.eye; a.n_ind = f.n_ind; a.has_eye = f.has_eye; a.M = M;
    a.ntiles = (M + TILE - 1) / TILE;
    a.sigmas = out.sigmas; a.rgbs = out.rgbs; a.amb_aud = out.amb_aud; a.amb_eye = out.amb_eye; a.unc = out.unc;
    return MF_OK;
}

template <typename K>
static int fused_lds_attr(K kernel, bool& done, size_t lds) {
    if (!done) {
        MF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        done = true;
    }
    return MF_OK;
}

}  // namespace
