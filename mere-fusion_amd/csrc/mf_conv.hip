// Implicit-GEMM convolution (+ folded BatchNorm bias, residual add, ReLU/sigmoid) on gfx950 MFMA.
//
// Replaces the unfused Conv2d -> BatchNorm2d -> (+x) -> ReLU module chain of
// wav2lip/models/conv.py:5-19 and the ConvTranspose2d variant of conv.py:33-44.
//
// GEMM view per phase: D[n][m] = sum_k W[n][k] * P[m][k]
//   m : output pixel of the quotient grid (b, i, j)              (MFMA "B" operand / columns)
//   n : output channel                                          (MFMA "A" operand / rows)
//   k : (tap, input channel), enumerated in 8-channel groups    (contraction)
// Weights are the A operand so that one lane of the 16x16 accumulator tile owns 4 CONSECUTIVE
// channels of one pixel: the NHWC epilogue is an 8-byte store per lane, 32 contiguous bytes per
// 4-lane group.  A stride-2 ConvTranspose2d runs as 4 sub-pixel phases (blockIdx.z), each an
// ordinary gather with 1/2/2/4 taps, so no zero-stuffed input is ever multiplied.
//
// One workgroup = 256 threads = 4 wave64; tile BM pixels x BN channels x BK deep (BK = 64 in bf16,
// 32 in bf16x3 so both modes keep the same LDS footprint).  Both operand tiles travel
// global -> LDS by DMA (global_load_lds_dwordx4, 1 KiB per wave instruction, no staging VGPRs and
// no ds_write pass) into a 2-stage ring: the DMA of tile k+1 is in flight while the MFMAs of tile k
// run.  The DMA image is lane-linear, so the bank-conflict swizzle is applied to the per-lane SOURCE
// address and again on the ds_read side.  The padded-halo activation layout means no load in the
// main loop is predicated.  Layers with few output pixels and a long contraction are split along K
// over blockIdx.y; their fp32 partial tiles are combined by k_splitk_epilogue.
#include "mf_conv.h"
#include <dlfcn.h>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <type_traits>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

// Swizzled LDS byte offset of the 16-byte slot (row, kg) of a [rows][BK] bf16 tile.  The XOR terms
// make every 16-lane service group of ds_read_b128 (rows l&15 at one or two kg values) hit 16
// distinct 16-byte slots of the 256-byte bank row (derivation in DESIGN.md).
template <int BK>
__device__ __forceinline__ int swz(int row) {
    return BK == 32 ? (((row >> 2) & 1) << 1) : (((row >> 1) & 3) << 1);
}
template <int BK>
__device__ __forceinline__ int tile_off(int row, int kg) {
    return row * (BK * 2) + ((kg ^ swz<BK>(row)) << 4);
}

__device__ __forceinline__ float bf2f(uint32_t h16) { return __uint_as_float(h16 << 16); }
__device__ __forceinline__ uint32_t f2bf(float f) {
    // round to nearest even in hardware: gfx950's v_cvt_pk_bf16_f32 (the compiler pairs neighbouring calls), a quarter of the integer form's instructions
    return (uint32_t)__builtin_bit_cast(unsigned short, (__bf16)f);
}

// 64 lanes x 16 bytes, global (per-lane address) -> LDS (wave-uniform base + lane*16)
__device__ __forceinline__ void glds16(const void* g, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ void add_residual(const ConvArgs& a, float (&v)[4], int64_t ro, int c, bool x3) {
    const uint2 rh = *reinterpret_cast<const uint2*>(a.r_hi + ro + c);
    v[0] += bf2f(rh.x & 0xffffu); v[1] += bf2f(rh.x >> 16);
    v[2] += bf2f(rh.y & 0xffffu); v[3] += bf2f(rh.y >> 16);
    if (x3) {
        const uint2 rl = *reinterpret_cast<const uint2*>(a.r_lo + ro + c);
        v[0] += bf2f(rl.x & 0xffffu); v[1] += bf2f(rl.x >> 16);
        v[2] += bf2f(rl.y & 0xffffu); v[3] += bf2f(rl.y >> 16);
    }
}

// act: 0 none, 1 ReLU, 2 sigmoid, 3 GELU (erf form, torch.nn.GELU default), 4 SiLU
// GELU (erf form) of the GEGLU epilogue: erf by Abramowitz & Stegun 7.1.26 -- 1 - (a1 t + ... + a5 t^5) exp(-x^2), t = 1 / (1 + p |x|), |error| <= 1.5e-7 -- in ~12
// vector instructions where the library's erff() takes ~30: a 128 x 128 GEGLU tile evaluates it 32 times per lane, after its MFMAs and with nothing to overlap it
// (one workgroup per CU), and the stored (hi, lo) pair resolves 2^-17 of the value anyway.  MF_GELU_EXACT builds keep erff() (A/B, tools/ab_build.sh).
#ifndef MF_GELU_EXACT
__device__ __forceinline__ float erf_as(float x) {
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float r = 1.f - p * t * __expf(-ax * ax);
    return copysignf(r, x);
}
__device__ __forceinline__ float gelu_erf(float g) { return 0.5f * g * (1.f + erf_as(g * 0.70710678118654752f)); }
#else
__device__ __forceinline__ float gelu_erf(float g) { return 0.5f * g * (1.f + erff(g * 0.70710678118654752f)); }
#endif

// residual / activation / (hi, lo) store of one channel quad; v holds the stored values on return
__device__ __forceinline__ void epilogue_store_v(const ConvArgs& a, float (&v)[4], int64_t yo, int64_t ro, int c, bool x3) {
    if (a.r_hi && !a.res_after_act) add_residual(a, v, ro, c, x3);
    if (a.act == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    } else if (a.act == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = 1.f / (1.f + __expf(-v[e]));
    } else if (a.act == 3) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.f + erff(v[e] * 0.70710678118654752f));
    } else if (a.act == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] / (1.f + expf(-v[e]));
    }
    if (a.r_hi && a.res_after_act) add_residual(a, v, ro, c, x3);
    uint32_t h[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = f2bf(v[e]);
    *reinterpret_cast<uint2*>(a.y_hi + yo + c) = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    if (x3) {
        uint32_t l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) l[e] = f2bf(v[e] - bf2f(h[e]));
        *reinterpret_cast<uint2*>(a.y_lo + yo + c) = make_uint2(l[0] | (l[1] << 16), l[2] | (l[3] << 16));
    }
}
__device__ __forceinline__ void epilogue_store(const ConvArgs& a, const float (&v0)[4], int64_t yo, int64_t ro,
                                               int c, bool x3) {
    float v[4] = {v0[0], v0[1], v0[2], v0[3]};
    epilogue_store_v(a, v, yo, ro, c, x3);
}

template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// Epilogue stores, 16 bytes per lane.  A lane of the 16 x 16 accumulator tile owns 4 consecutive channels (8 bytes of bf16) of one pixel in
// every fragment; lanes fk and fk ^ 1 (lane ^ 16) own the two halves of one 8-channel group.  For a fragment PAIR (p0, p1) the even lane
// takes both halves of p0's group, the odd lane both halves of p1's: one exchange, then ONE dwordx4 store where two dwordx2 went before.
// The store tail is issue-bound (MI355X_MICROARCH.md: 16 x dwordx2 per lane ~ 9.3k cycles; dwordx4 halves it) and is 20-45 % of the
// UNet's small GEMMs.  `c16` = first channel of the 16-channel block of p0; p1's block starts `blk` channels later.
__device__ __forceinline__ void store_pair16(bf16_t* base, int64_t yo, int c16, int blk, int fk, uint2 p0, uint2 p1, int N, bool ok) {
    const bool odd = fk & 1;
    const uint2 send = odd ? p0 : p1;
    uint2 recv;
    recv.x = (uint32_t)__shfl_xor((int)send.x, 16);
    recv.y = (uint32_t)__shfl_xor((int)send.y, 16);
    const uint4 out = odd ? make_uint4(recv.x, recv.y, p1.x, p1.y) : make_uint4(p0.x, p0.y, recv.x, recv.y);
    const int cw = c16 + (odd ? blk : 0) + (fk & ~1) * 4;
    if (ok && cw < N) *reinterpret_cast<uint4*>(base + yo + cw) = out;
}

// NST = LDS stages of the DMA path (2: the DMA of tile k+1 flies under the MFMAs of tile k, drained at a __syncthreads()).
// LD = how the operand tiles reach LDS.  0: LDS-DMA (global_load_lds) into the two stages.  2: through registers into ONE LDS stage (two barriers per
// tile): a DMA piece costs its wave 100-185 issue cycles inside a loaded phase (MI355X_MICROARCH.md), a plain load a few and the ds_write_b128 13; and with
// half the LDS a 64-deep two-plane tile (128-byte rows: every request a full line) still leaves room for 2-3 workgroups per CU, whose MFMAs cover each
// other's barriers.
// Q: operands in the f16 + FP6 format (MF_PREC_F16Q; the two planes are f16 and [q6 | q6] FP6 blocks, see pack_q_block): per 32-deep step ONE
// v_mfma_f32_16x16x32_f16 (wh.xh) and per 64-deep tile ONE v_mfma_scale_f32_16x16x128_f8f6f4 whose K blocks 0 / 1 carry q6(wh).xl / wl.q6(xh) of channels
// 0..31 and blocks 2 / 3 those of channels 32..63 -- 48 matrix cycles per tile and accumulator where bf16x3 spends 96.  A 32-deep tile (the 8-wave tiles)
// leaves blocks 2 / 3 off by a zero scale: 32 cycles against 48.
// LD 3 (round 5): PRODUCER WAVES.  Stamps (MF_DEBUG=times) on the UNet's batch-8 shapes put the DMA loop at 3325 cycles per 64-deep step of the 128 x 128 tile
// and 1816 for 128 x 64, whether 20 or 240 workgroups run and whether the bytes come from L2 or HBM: 96 / 48 MFMAs (1536 / 768 cycles) plus the ISSUE cost of
// the 16 / 12 LDS-DMA pieces each compute wave launches per step (100 - 185 cycles apiece inside a loaded phase, MI355X_MICROARCH.md) plus two exposed LDS
// fragment-read latencies -- the matrix pipe is busy 23 - 46 % by construction.  Here a workgroup is NW compute waves + NW producer waves (one of each per SIMD):
// the producers issue every LDS-DMA piece of a stage (pixel rows gathered through s_goff, weight rows) into a ring of igemm_ring<...>() stages and keep
// (depth - 3) stages in flight behind their own vmcnt; the compute waves touch only LDS and the matrix pipe, and read the fragments of step i + 1 into a
// second register set while the MFMAs of step i run (the stage has landed: the producers stay two steps ahead of the barrier).
template <int BM, int BN, int BK, bool X3>
constexpr int igemm_ring() {
    constexpr int stage = (BM + BN) * BK * 2 * (X3 ? 2 : 1);
    constexpr int by_lds = (144 * 1024) / stage;                                         // 160 KB - 16 KB for the gather-offset table of the longest contraction
    return by_lds < 8 ? by_lds : 8;
}

#ifndef MF_PW_NPW
#define MF_PW_NPW 4          // producer waves per workgroup on the LD 3 path (A/B builds: 8)
#endif
// producer waves of a tile on the LD 3 path: MF_PW_NPW where both operands' 1-KiB pieces divide evenly among them, else 4
template <int BM, int BN, int BK>
constexpr int igemm_producers() {
    constexpr int rpc = 1024 / (BK * 2), pch = (BM + rpc - 1) / rpc, wch = (BN + rpc - 1) / rpc;
    return (pch % MF_PW_NPW == 0 && wch % MF_PW_NPW == 0) ? MF_PW_NPW : 4;
}
template <int BM, int BN, int WGM, int WGN, bool X3, int BK, int NST, int LD = 0, bool Q = false>
__global__ __launch_bounds__((WGM * WGN + (LD == 3 ? igemm_producers<BM, BN, BK>() : 0)) * 64) void k_conv_igemm(const ConvArgs a) {
    static_assert(!Q || X3, "the f16 + FP6 format has two planes");
    constexpr int NW = WGM * WGN;         // compute waves per workgroup (LD 3: producer waves on top)
    constexpr int NS = LD == 3 ? igemm_producers<BM, BN, BK>() : NW;   // waves that share the DMA pieces of a stage
    constexpr int NT = (NW + (LD == 3 ? NS : 0)) * 64;
    static_assert(NW == 4 || NW == 8, "4 or 8 waves per workgroup");
    static_assert(BK == 32 || BK == 64, "LDS tile depth");
    static_assert(NST == 2, "two LDS stages (deeper rings halved the workgroups per CU and measured slower)");
    constexpr int KG = BK / 8;            // 16-byte groups per tile row
    constexpr int ROWB = BK * 2;          // bytes per tile row
    constexpr int RPC = 1024 / ROWB;      // tile rows per 1-KiB DMA chunk
    constexpr int NP = X3 ? 2 : 1;
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int FM = WTM / 16, FN = WTN / 16;
    static_assert(FM >= 1 && FN >= 1, "wave tile must hold a 16x16 fragment");
    constexpr int P_BYTES = BM * ROWB, W_BYTES = BN * ROWB;
    constexpr int PLANE = P_BYTES + W_BYTES;
    constexpr int STAGE = PLANE * NP;
    constexpr int PCH = (BM + RPC - 1) / RPC, WCH = (BN + RPC - 1) / RPC;   // DMA chunks per tile
    constexpr int NPC = (PCH + NS - 1) / NS, NWC = (WCH + NS - 1) / NS;      // ... per wave

    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int LDS_STAGES = LD == 2 ? 1 : NST;
    constexpr int DR = LD == 3 ? igemm_ring<BM, BN, BK, X3>() : 0;                     // ring depth of the producer-wave path
    static_assert(LD != 3 || DR >= 2, "producer-wave path: at least a double buffer");
    int* s_goff = reinterpret_cast<int*>(smem + (LD == 3 ? DR : LDS_STAGES) * STAGE);
    // MF_DEBUG=times: s_memtime stamps of (entry, loop start, loop end, exit) per workgroup
    unsigned long long* dbg = a.dbg ? a.dbg + 4 * ((size_t)blockIdx.x + gridDim.x * ((size_t)blockIdx.y + gridDim.y * blockIdx.z)) : nullptr;
    if (dbg && threadIdx.x == 0) dbg[0] = __builtin_amdgcn_s_memtime();

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    ConvPhase ph = a.ph[a.zgroups ? 0 : blockIdx.z];
    int64_t zx = 0, zy = 0;
    if (a.zgroups) {   // attention: blockIdx.z = (batch, head); operand bases move, geometry does not
        const int zb = blockIdx.z / a.zheads, zh = blockIdx.z - zb * a.zheads;
        zx = zb * a.zx_b + zh * a.zx_h;
        zy = zb * a.zy_b + zh * a.zy_h;
        ph.w_off += (int64_t)blockIdx.z * a.zw;
    }

    // XCD-aware tile order: the dispatcher round-robins blockIdx over the 8 XCDs; give each XCD a
    // contiguous run of tiles (n fastest) so the N tiles of one pixel tile share an L2.
    const int nt = a.tiles_m * a.tiles_n;
    const int bid = blockIdx.x;
    const int q = nt >> 3, r = nt & 7, xcd = bid & 7;
    const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    // n fastest: the N tiles of one pixel tile share the activations in one L2.  m fastest (weights outweigh the
    // activations: the UNet's small maps): an XCD walks all pixel tiles of one or two channel tiles, so each XCD pulls
    // its slice of the weights from HBM once instead of every XCD pulling all of them.
    int tm, tn;
    if (a.m_fastest) { tn = mf_fdiv(t, a.dv_t_mul, a.dv_t_shr); tm = t - tn * a.tiles_m; }
    else { tm = mf_fdiv(t, a.dv_t_mul, a.dv_t_shr); tn = t - tm * a.tiles_n; }
    const int m0 = tm * BM, n0 = tn * BN;

    // split-K slice of this workgroup (ph.KT counts 64-deep packed tiles; this kernel steps BK)
    const int KTk = ph.KT * (64 / BK);
    // (KTk * split index < 2^31; as 64-bit divisions these two lines were ~200 vector instructions at the head of every workgroup)
    const int kt_begin = mf_fdiv(KTk * (int)blockIdx.y, a.dv_s_mul, a.dv_s_shr);
    const int kt_end = mf_fdiv(KTk * ((int)blockIdx.y + 1), a.dv_s_mul, a.dv_s_shr);

    for (int i = tid; i < ph.ngroups; i += NT) s_goff[i] = a.goff[ph.goff_begin + i];

    // ---- DMA assignment: wave w moves chunks w, w+NW, ... of each tile (LD 3: producer wave NW + w does) -------------------------
    const int wq = LD == 3 ? (wave >= NW ? wave - NW : wave) : wave;
    const bf16_t* xp[NPC];
    int p_kg[NPC];
    const int64_t x_delta = X3 ? (a.x_lo - a.x_hi) : 0;
#pragma unroll
    for (int i = 0; i < NPC; ++i) {
        const int row = (wq + NS * i) * RPC + lane / KG;
        p_kg[i] = (lane % KG) ^ swz<BK>(row);
        int m = m0 + row;
        m = m < a.M ? m : a.M - 1;
        const int b = mf_fdiv(m, a.dv_hw_mul, a.dv_hw_shr);
        const int rem = m - b * a.HqWq;
        const int qi = mf_fdiv(rem, a.dv_w_mul, a.dv_w_shr), qj = rem - qi * a.Wq;
        xp[i] = a.x_hi + (zx + (int64_t)b * a.xb + (int64_t)qi * a.xi + (int64_t)qj * a.xj);
    }
    const bf16_t* wp[NWC];
    const int64_t w_delta = X3 ? (a.w_lo - a.w_hi) : 0;
#pragma unroll
    for (int i = 0; i < NWC; ++i) {
        // (LD 3 with a piece count that does not divide among the producers -- the 80-channel tile: a producer without an i-th piece re-issues its
        // previous one, so that every producer retires the same number of vmcnt ticks per stage)
        const int cw = (LD == 3 && WCH % NS != 0 && wq + NS * i >= WCH) ? wq + NS * (i - 1) : wq + NS * i;
        const int row = cw * RPC + lane / KG;
        const int kg = (lane % KG) ^ swz<BK>(row);
        int n = n0 + row;
        n = n < a.Npad ? n : a.Npad - 1;
        wp[i] = a.w_hi + ph.w_off + (int64_t)n * 64 + kg * 8;   // packed [K/64][Npad][64]
    }
    const int64_t w_kstep = (int64_t)a.Npad * 64;
    auto stage = [&](int kt, int s) __attribute__((always_inline)) {
        char* base = smem + s * STAGE;
#pragma unroll
        for (int i = 0; i < NPC; ++i) {
            const int c = wq + NS * i;
            if (PCH % NS == 0 || c < PCH) {
                const bf16_t* src = xp[i] + s_goff[kt * KG + p_kg[i]];
                glds16(src, base + c * 1024);
                if (X3) glds16(src + x_delta, base + PLANE + c * 1024);
            }
        }
#pragma unroll
        for (int i = 0; i < NWC; ++i) {
            const int c = (LD == 3 && WCH % NS != 0 && wq + NS * i >= WCH) ? wq + NS * (i - 1) : wq + NS * i;
            if (LD == 3 || WCH % NS == 0 || c < WCH) {
                const bf16_t* src = BK == 64 ? wp[i] + kt * w_kstep : wp[i] + (kt >> 1) * w_kstep + (kt & 1) * 32;
                glds16(src, base + P_BYTES + c * 1024);
                if (X3) glds16(src + w_delta, base + PLANE + P_BYTES + c * 1024);
            }
        }
    };

    // ---- MFMA fragments -------------------------------------------------------------------
    const int wave_m = wave % WGM, wave_n = wave / WGM;
    const int pm0 = wave_m * WTM, cn0 = wave_n * WTN;
    const int fr = lane & 15, fk = lane >> 4;

    f32x4 acc[FN][FM];
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // pb / wb: plane 0 of the pixel / weight tile of this K step; pps / wps: byte distance to plane 1
    auto compute_at = [&](const char* pb, int pps, const char* wb, int wps) __attribute__((always_inline)) {
        if constexpr (Q) {
            // corrections first (small terms), then the f16 products.  A lane's FP6 block: the 32 bytes at 16-byte slots 2g, 2g + 1 of its plane-1 row, g = its
            // K block (BK 64: lane group fk; BK 32: fk & 1, groups 2 / 3 re-read and are switched off).  The XOR swizzle is even, so the two slots stay adjacent.
            const int g6 = BK == 64 ? fk : (fk & 1);
            const bool off = BK == 32 && fk >= 2;
            i32x8 w6[FN];
#pragma unroll
            for (int i = 0; i < FN; ++i) {
                const char* q = wb + wps + tile_off<BK>(cn0 + i * 16 + fr, 2 * g6);
                w6[i] = __builtin_shufflevector(*reinterpret_cast<const i32x4*>(q), *reinterpret_cast<const i32x4*>(q + 16), 0, 1, 2, 3, 4, 5, 6, 7);
            }
            constexpr int JH = FM > 4 ? 4 : FM;                   // pixel fragments per batch (the 128-pixel wave tiles have no registers for all eight at once)
#pragma unroll
            for (int j0 = 0; j0 < FM; j0 += JH) {
                i32x8 p6[JH];
#pragma unroll
                for (int jj = 0; jj < JH; ++jj) {
                    const char* q = pb + pps + tile_off<BK>(pm0 + (j0 + jj) * 16 + fr, 2 * g6);
                    p6[jj] = __builtin_shufflevector(*reinterpret_cast<const i32x4*>(q), *reinterpret_cast<const i32x4*>(q + 16), 0, 1, 2, 3, 4, 5, 6, 7);
                }
#pragma unroll
                for (int i = 0; i < FN; ++i)
#pragma unroll
                    for (int jj = 0; jj < JH; ++jj)
                        acc[i][j0 + jj] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w6[i], p6[jj], acc[i][j0 + jj], 2, 2, 0, off ? 0 : w6[i][6], 0, off ? 0 : p6[jj][6]);
            }
#pragma unroll
            for (int kk = 0; kk < BK / 32; ++kk) {
                f16x8 pf[FM], wf[FN];
#pragma unroll
                for (int i = 0; i < FM; ++i) pf[i] = *reinterpret_cast<const f16x8*>(pb + tile_off<BK>(pm0 + i * 16 + fr, kk * 4 + fk));
#pragma unroll
                for (int i = 0; i < FN; ++i) wf[i] = *reinterpret_cast<const f16x8*>(wb + tile_off<BK>(cn0 + i * 16 + fr, kk * 4 + fk));
#pragma unroll
                for (int i = 0; i < FN; ++i)
#pragma unroll
                    for (int j = 0; j < FM; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[i], pf[j], acc[i][j], 0, 0, 0);
            }
            return;
        }
#pragma unroll
        for (int kk = 0; kk < BK / 32; ++kk) {
            bf16x8 pf[NP][FM], wf[NP][FN];
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
                for (int i = 0; i < FM; ++i)
                    pf[pl][i] = *reinterpret_cast<const bf16x8*>(pb + pl * pps + tile_off<BK>(pm0 + i * 16 + fr, kk * 4 + fk));
#pragma unroll
                for (int i = 0; i < FN; ++i)
                    wf[pl][i] = *reinterpret_cast<const bf16x8*>(wb + pl * wps + tile_off<BK>(cn0 + i * 16 + fr, kk * 4 + fk));
            }
#pragma unroll
            for (int i = 0; i < FN; ++i)
#pragma unroll
                for (int j = 0; j < FM; ++j) {
                    if (X3) {
                        // small cross terms first, the dominant hi*hi product last
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[NP - 1][i], pf[0][j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][i], pf[NP - 1][j], acc[i][j], 0, 0, 0);
                    }
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][i], pf[0][j], acc[i][j], 0, 0, 0);
                }
        }
    };
    auto compute = [&](int s) __attribute__((always_inline)) {
        const char* base = smem + s * STAGE;
        compute_at(base, PLANE, base + P_BYTES, PLANE);
    };

    __syncthreads();   // s_goff visible
    if (dbg && threadIdx.x == 0) dbg[1] = __builtin_amdgcn_s_memtime();
    const int nk = kt_end - kt_begin;
    if constexpr (LD == 3) {
        // DMA instructions (= vmcnt ticks) one producer wave issues per stage; the wait immediates below are multiples of it
        constexpr int NPI = (NPC + NWC) * NP;
        static_assert(PCH % NS == 0 && WCH >= NS, "producer-wave path: every producer issues the same number of pieces per stage (weight pieces: duplicates fill up)");
        // LEAD: how many stages beyond the one a step multiplies have landed when the step starts.  2: the compute waves read step i + 1's fragments under step
        // i's MFMAs (no exposed LDS latency) and DR - 3 stages stay in flight; 1: a step reads its own stage (the compiler interleaves the reads with the MFMAs)
        // and DR - 2 stages stay in flight.  The ring is what bounds the bytes in flight, and bytes in flight over the loaded L2 / Infinity-Cache round trip is
        // the rate the operands arrive at: a 4-stage ring (the 128 x 128 and 64-deep 64 x 64 tiles) takes LEAD 1, deeper rings LEAD 2.
#ifndef MF_PW_LEAD
        constexpr int LEAD = DR >= 5 ? 2 : 1;
#else
        constexpr int LEAD = MF_PW_LEAD;                           // (A/B builds: tools/ab_build.sh ... "-DMF_PW_LEAD=2")
#endif
        static_assert((DR - 1 - LEAD) * NPI <= 63 && DR - 1 - LEAD >= 0, "vmcnt immediate");   // (DR 2: the classic double buffer -- the next stage lands under this one's MFMAs)
        if (wave >= NW) {
            // ---- producer waves.  Barrier b (b = 0 opens step 0, b = i + 1 closes step i) is reached with stages <= b + LEAD - 1 landed.  Stage i + DR - 1 goes
            // into the slot stage i - 1 had, whose last reader finished before barrier i.
            if (nk > 0) {
                const int pre = nk < DR - 1 ? nk : DR - 1;
                for (int d = 0; d < pre; ++d) stage(kt_begin + d, d);
                if (pre == DR - 1) wait_vm<(DR - 1 - LEAD) * NPI>(); else wait_vm<0>();
                __builtin_amdgcn_s_barrier();
                int slot = DR - 1;
                for (int i = 0; i < nk; ++i) {
                    if (i + DR - 1 < nk) {
                        stage(kt_begin + i + DR - 1, slot);
                        slot = slot + 1 == DR ? 0 : slot + 1;
                        wait_vm<(DR - 1 - LEAD) * NPI>();      // everything but the newest DR - 1 - LEAD stages: stage i + LEAD has landed
                    } else {
                        wait_vm<0>();
                    }
                    __builtin_amdgcn_s_barrier();
                }
            }
            return;                                            // (a finished wave no longer counts at the workgroup's barriers: the epilogue's are the compute waves')
        }
        // ---- compute waves: LDS fragment reads of step i + 1 fly under the MFMAs of step i -------------------------------------------------------------
        constexpr int KK = BK / 32;                            // 32-deep MFMA steps per stage
        bf16x8 pfr[2][NP][FM], wfr[2][NP][FN];
        auto ldf = [&](auto bufc, int slot, int kk) __attribute__((always_inline)) {
            constexpr int b = decltype(bufc)::value;
            const char* base = smem + slot * STAGE;
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
                for (int i = 0; i < FM; ++i) pfr[b][pl][i] = *reinterpret_cast<const bf16x8*>(base + pl * PLANE + tile_off<BK>(pm0 + i * 16 + fr, kk * 4 + fk));
#pragma unroll
                for (int i = 0; i < FN; ++i) wfr[b][pl][i] = *reinterpret_cast<const bf16x8*>(base + pl * PLANE + P_BYTES + tile_off<BK>(cn0 + i * 16 + fr, kk * 4 + fk));
            }
        };
        auto mma = [&](auto bufc) __attribute__((always_inline)) {
            constexpr int b = decltype(bufc)::value;
#pragma unroll
            for (int i = 0; i < FN; ++i)
#pragma unroll
                for (int j = 0; j < FM; ++j) {
                    if (X3) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[b][NP - 1][i], pfr[b][0][j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[b][0][i], pfr[b][NP - 1][j], acc[i][j], 0, 0, 0);
                    }
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[b][0][i], pfr[b][0][j], acc[i][j], 0, 0, 0);
                }
        };
        using B0 = std::integral_constant<int, 0>;
        using B1 = std::integral_constant<int, 1>;
        if (nk > 0 && LEAD == 1) {
            __syncthreads();                                   // barrier 0: stage 0 has landed
            int slot = 0;
            for (int i = 0; i < nk; ++i) {
                ldf(B0{}, slot, 0);
                if constexpr (KK == 2) ldf(B1{}, slot, 1);
                mma(B0{});
                if constexpr (KK == 2) mma(B1{});
                slot = slot + 1 == DR ? 0 : slot + 1;
                __syncthreads();
            }
        } else if (nk > 0) {
            __syncthreads();                                   // barrier 0: stages 0 and 1 have landed
            ldf(B0{}, 0, 0);
            int slot = 0;                                      // ring slot of stage i
            if constexpr (KK == 2) {
                // 64-deep stages: (stage i, kk 0) in set 0, (stage i, kk 1) in set 1
                for (int i = 0; i < nk; ++i) {
                    const int nslot = slot + 1 == DR ? 0 : slot + 1;
                    ldf(B1{}, slot, 1);
                    mma(B0{});
                    if (i + 1 < nk) ldf(B0{}, nslot, 0);
                    mma(B1{});
                    slot = nslot;
                    __syncthreads();
                }
            } else {
                // 32-deep stages: even steps in set 0, odd steps in set 1
                for (int i = 0; i < nk; i += 2) {
                    int nslot = slot + 1 == DR ? 0 : slot + 1;
                    if (i + 1 < nk) ldf(B1{}, nslot, 0);
                    mma(B0{});
                    slot = nslot;
                    __syncthreads();
                    if (i + 1 < nk) {
                        nslot = slot + 1 == DR ? 0 : slot + 1;
                        if (i + 2 < nk) ldf(B0{}, nslot, 0);
                        mma(B1{});
                        slot = nslot;
                        __syncthreads();
                    }
                }
            }
        }
    } else if constexpr (LD != 0) {
        static_assert(LD == 2, "register-staged tiles: one LDS stage");
        u32x4 rp[NP][NPC], rw[NP][NWC];
        auto gload = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < NPC; ++i) {
                const int c = wave + NW * i;
                if (PCH % NW == 0 || c < PCH) {
                    const bf16_t* src = xp[i] + s_goff[kt * KG + p_kg[i]];
                    rp[0][i] = *reinterpret_cast<const u32x4*>(src);
                    if (X3) rp[NP - 1][i] = *reinterpret_cast<const u32x4*>(src + x_delta);
                }
            }
#pragma unroll
            for (int i = 0; i < NWC; ++i) {
                const int c = wave + NW * i;
                if (WCH % NW == 0 || c < WCH) {
                    const bf16_t* src = BK == 64 ? wp[i] + kt * w_kstep : wp[i] + (kt >> 1) * w_kstep + (kt & 1) * 32;
                    rw[0][i] = *reinterpret_cast<const u32x4*>(src);
                    if (X3) rw[NP - 1][i] = *reinterpret_cast<const u32x4*>(src + w_delta);
                }
            }
        };
        auto lstore = [&](int s) __attribute__((always_inline)) {
            char* base = smem + s * STAGE + lane * 16;
#pragma unroll
            for (int i = 0; i < NPC; ++i) {
                const int c = wave + NW * i;
                if (PCH % NW == 0 || c < PCH) {
                    *reinterpret_cast<u32x4*>(base + c * 1024) = rp[0][i];
                    if (X3) *reinterpret_cast<u32x4*>(base + PLANE + c * 1024) = rp[NP - 1][i];
                }
            }
#pragma unroll
            for (int i = 0; i < NWC; ++i) {
                const int c = wave + NW * i;
                if (WCH % NW == 0 || c < WCH) {
                    *reinterpret_cast<u32x4*>(base + P_BYTES + c * 1024) = rw[0][i];
                    if (X3) *reinterpret_cast<u32x4*>(base + PLANE + P_BYTES + c * 1024) = rw[NP - 1][i];
                }
            }
        };
        {
            if (nk > 0) gload(kt_begin);
            for (int kt = kt_begin; kt < kt_end; ++kt) {
                if (kt > kt_begin) __syncthreads();              // everyone is done reading the previous tile
                lstore(0);
                if (kt + 1 < kt_end) gload(kt + 1);              // in flight under this tile's MFMAs
                __syncthreads();
                compute(0);
            }
        }
    } else {
        if (nk > 0) {
            stage(kt_begin, 0);
            __syncthreads();   // drains the DMA (vmcnt) and publishes stage 0
            for (int kt = kt_begin; kt < kt_end; ++kt) {
                const int s = (kt - kt_begin) & 1;
                if (kt + 1 < kt_end) stage(kt + 1, s ^ 1);   // DMA of the next tile flies under the MFMAs
                compute(s);
                __syncthreads();
            }
        }
    }

    // ---- epilogue ---------------------------------------------------------------------------
    if (dbg && threadIdx.x == 0) dbg[2] = __builtin_amdgcn_s_memtime();
    if (a.ws) {
        // split-K: fp32 partial tile, combined by k_splitk_epilogue
#pragma unroll
        for (int j = 0; j < FM; ++j) {
            const int m = m0 + pm0 + j * 16 + fr;
            if (m >= a.M) continue;
            const int b = mf_fdiv(m, a.dv_hw_mul, a.dv_hw_shr);
            const int rem = m - b * a.HqWq;
            const int qi = mf_fdiv(rem, a.dv_w_mul, a.dv_w_shr), qj = rem - qi * a.Wq;
            float* wo = a.ws + (int64_t)blockIdx.y * a.ws_split + (int64_t)b * a.wsb + (int64_t)qi * a.wsi +
                        (int64_t)qj * a.wsj + ph.ws_off;
#pragma unroll
            for (int i = 0; i < FN; ++i) {
                const int c = n0 + cn0 + i * 16 + fk * 4;
                if (c >= a.N) continue;
                *reinterpret_cast<float4*>(wo + c) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
            }
        }
        // (the combine -- bias, residual, activation, the (hi, lo) store -- is k_splitk_epilogue's: doing it here, in the last workgroup of a tile to
        // arrive, measured slower: one workgroup re-reading nsplit tiles behind two fences and an atomic is a longer tail than a 5 us pass over every CU)
        if (dbg && threadIdx.x == 0) dbg[3] = __builtin_amdgcn_s_memtime();
        return;
    }
    // Bias quads of this lane, fetched once and with clamped (never branched-around) addresses; the activation is a
    // compile-time parameter of the body below.  Both keep the per-fragment code straight-line, so the residual loads of a
    // pixel row are issued together instead of one global round trip per 4 channels.
    float4 bq[FN];
#pragma unroll
    for (int i = 0; i < FN; ++i) {
        int c = n0 + cn0 + i * 16 + fk * 4;
        c = c < a.Npad - 3 ? c : a.Npad - 4;
        bq[i] = *reinterpret_cast<const float4*>(a.bias + c);
    }
    const int ACT = a.act;
    if (a.ln_in) {
        // ---- LayerNorm folded into this layer (its consumers have no residual and act 0 or GEGLU: conv_launch_impl checks).  Its own short epilogue: the general one
        // below sits at the register limit of the 128 x 128 tile (two workgroups per CU), and the column-sum quads are fetched per use (L1-resident) ----
#pragma unroll
        for (int j = 0; j < FM; ++j) {
            const int m = m0 + pm0 + j * 16 + fr;
            const bool row_ok = m < a.M;
            const int mc = row_ok ? m : a.M - 1;
            const int b = mf_fdiv(mc, a.dv_hw_mul, a.dv_hw_shr);
            const int rem = mc - b * a.HqWq;
            const int qi = mf_fdiv(rem, a.dv_w_mul, a.dv_w_shr), qj = rem - qi * a.Wq;
            const int64_t yo = zy + (int64_t)b * a.yb + (int64_t)qi * a.yi + (int64_t)qj * a.yj + ph.y_off;
            const double2 sq = *reinterpret_cast<const double2*>(a.ln_in + 2 * (int64_t)mc);
            const double mean = sq.x * (double)a.ln_inv_c, var = sq.y * (double)a.ln_inv_c - mean * mean;
            const float mu = (float)mean, rs = (float)(1.0 / sqrt((var > 0.0 ? var : 0.0) + (double)a.ln_eps));
            auto quad = [&](int i, float (&v)[4]) __attribute__((always_inline)) {       // rstd * (acc - mean * colsum) + bias' of fragment i
                int c = n0 + cn0 + i * 16 + fk * 4;
                c = c < a.Npad - 3 ? c : a.Npad - 4;
                const float4 cs = *reinterpret_cast<const float4*>(a.ln_cs + c);
                // One scalar FMA per value, pinned by empty asm statements.  Left alone the compiler packs these into v_pk_fma_f32 and keeps (mu, rs) in ONE register pair,
                // and for the last fragment of a wave it multiplies by rs as `v_pk_fma_f32 ... op_sel:[0,1,0]` -- the LOW result takes src1's HIGH register.  On gfx950 that
                // form returns a wrong low half in lanes 48..63 (src1 read as zero: the value comes out as the bias alone) whenever another wave of the same SIMD is
                // issuing MFMAs, which the neighbouring workgroups of this kernel are: one channel of a 16-pixel fragment wrong now and then, elsewhere on every call
                // (round 5: 1e-2 noise on the UNet's latents in one build, a 1.6e-5 dependence on the batch position in another).  Round 6 reproduced the erratum in
                // isolation (tools/pkfma_repro.hip: 0.09 % of executions; op_sel_hi forms and src0 / src2 selects are clean) and checks every build for the form
                // (tools/isa_scan.py, mf_common.h mf_opaque).  Eight instructions per fragment quad more than the packed form, in an epilogue.
                float t0 = acc[i][j][0] - mu * cs.x, t1 = acc[i][j][1] - mu * cs.y, t2 = acc[i][j][2] - mu * cs.z, t3 = acc[i][j][3] - mu * cs.w;
                asm volatile("" : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3));
                v[0] = rs * t0 + bq[i].x; v[1] = rs * t1 + bq[i].y; v[2] = rs * t2 + bq[i].z; v[3] = rs * t3 + bq[i].w;
                asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
            };
            auto pack = [&](const float (&v)[4], uint2& hi2, uint2& lo2) __attribute__((always_inline)) {
                uint32_t h[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) h[e] = f2bf(v[e]);
                hi2 = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
                if (X3) {
                    uint32_t l[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) l[e] = f2bf(v[e] - bf2f(h[e]));
                    lo2 = make_uint2(l[0] | (l[1] << 16), l[2] | (l[3] << 16));
                }
            };
            if (FN % 2 == 0 && ACT == 5) {
                const int NO = a.N >> 1;
                uint2 pk_hi[FN / 2 > 0 ? FN / 2 : 1], pk_lo[FN / 2 > 0 ? FN / 2 : 1];
#pragma unroll
                for (int i = 0; i + 1 < FN; i += 2) {
                    float val[4], gate[4];
                    quad(i, val); quad(i + 1, gate);
                    const float v[4] = {val[0] * gelu_erf(gate[0]), val[1] * gelu_erf(gate[1]), val[2] * gelu_erf(gate[2]), val[3] * gelu_erf(gate[3])};
                    pk_lo[i / 2] = make_uint2(0u, 0u);
                    pack(v, pk_hi[i / 2], pk_lo[i / 2]);
                }
                if (FN % 4 == 0 && a.wide_store) {
#pragma unroll
                    for (int q = 0; q + 1 < FN / 2; q += 2) {
                        const int c16 = (n0 + cn0 + 2 * q * 16) / 2;
                        store_pair16(a.y_hi, yo, c16, 16, fk, pk_hi[q], pk_hi[q + 1], NO, row_ok);
                        if (X3) store_pair16(a.y_lo, yo, c16, 16, fk, pk_lo[q], pk_lo[q + 1], NO, row_ok);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < FN / 2; ++q) {
                        const int c = n0 + cn0 + 2 * q * 16 + fk * 4;
                        if (!row_ok || c >= a.N) continue;
                        const int co = (n0 + cn0 + 2 * q * 16) / 2 + fk * 4;
                        *reinterpret_cast<uint2*>(a.y_hi + yo + co) = pk_hi[q];
                        if (X3) *reinterpret_cast<uint2*>(a.y_lo + yo + co) = pk_lo[q];
                    }
                }
            } else {
                uint2 pk_hi[FN], pk_lo[FN];
#pragma unroll
                for (int i = 0; i < FN; ++i) {
                    float v[4];
                    quad(i, v);
                    pk_lo[i] = make_uint2(0u, 0u);
                    pack(v, pk_hi[i], pk_lo[i]);
                }
                if (FN % 2 == 0 && a.wide_store) {
#pragma unroll
                    for (int i = 0; i + 1 < FN; i += 2) {
                        const int c16 = n0 + cn0 + i * 16;
                        store_pair16(a.y_hi, yo, c16, 16, fk, pk_hi[i], pk_hi[i + 1], a.N, row_ok);
                        if (X3) store_pair16(a.y_lo, yo, c16, 16, fk, pk_lo[i], pk_lo[i + 1], a.N, row_ok);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < FN; ++i) {
                        const int c = n0 + cn0 + i * 16 + fk * 4;
                        if (!row_ok || c >= a.N) continue;
                        *reinterpret_cast<uint2*>(a.y_hi + yo + c) = pk_hi[i];
                        if (X3) *reinterpret_cast<uint2*>(a.y_lo + yo + c) = pk_lo[i];
                    }
                }
            }
        }
    } else if (FN % 2 == 0 && ACT == 5) {
        // GEGLU: GEMM rows alternate 16 value channels / their 16 gate channels (packed that way at plan creation), so
        // fragment i holds the values and fragment i + 1 the gates of the same 4 output channels of this lane
#pragma unroll
        for (int j = 0; j < FM; ++j) {
            const int m = m0 + pm0 + j * 16 + fr;
            const bool row_ok = m < a.M;
            const int mc = row_ok ? m : a.M - 1;
            const int b = mf_fdiv(mc, a.dv_hw_mul, a.dv_hw_shr);
            const int rem = mc - b * a.HqWq;
            const int qi = mf_fdiv(rem, a.dv_w_mul, a.dv_w_shr), qj = rem - qi * a.Wq;
            const int64_t yo = zy + (int64_t)b * a.yb + (int64_t)qi * a.yi + (int64_t)qj * a.yj + ph.y_off;
            uint2 pk_hi[FN / 2 > 0 ? FN / 2 : 1], pk_lo[FN / 2 > 0 ? FN / 2 : 1];
#pragma unroll
            for (int i = 0; i + 1 < FN; i += 2) {
                const float v[4] = {(acc[i][j][0] + bq[i].x) * gelu_erf(acc[i + 1][j][0] + bq[i + 1].x), (acc[i][j][1] + bq[i].y) * gelu_erf(acc[i + 1][j][1] + bq[i + 1].y),
                                    (acc[i][j][2] + bq[i].z) * gelu_erf(acc[i + 1][j][2] + bq[i + 1].z), (acc[i][j][3] + bq[i].w) * gelu_erf(acc[i + 1][j][3] + bq[i + 1].w)};
                uint32_t h[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) h[e] = f2bf(v[e]);
                pk_hi[i / 2] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
                if (X3) {
                    uint32_t l[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) l[e] = f2bf(v[e] - bf2f(h[e]));
                    pk_lo[i / 2] = make_uint2(l[0] | (l[1] << 16), l[2] | (l[3] << 16));
                }
            }
            const int NO = a.N >> 1;                                  // output channels
            if (FN % 4 == 0 && a.wide_store) {
#pragma unroll
                for (int q = 0; q + 1 < FN / 2; q += 2) {
                    const int c16 = (n0 + cn0 + 2 * q * 16) / 2;      // output block of fragment pair q; pair q + 1's block is 16 channels on
                    store_pair16(a.y_hi, yo, c16, 16, fk, pk_hi[q], pk_hi[q + 1], NO, row_ok);
                    if (X3) store_pair16(a.y_lo, yo, c16, 16, fk, pk_lo[q], pk_lo[q + 1], NO, row_ok);
                }
            } else {
#pragma unroll
                for (int q = 0; q < FN / 2; ++q) {
                    const int c = n0 + cn0 + 2 * q * 16 + fk * 4;
                    if (!row_ok || c >= a.N) continue;
                    const int co = (n0 + cn0 + 2 * q * 16) / 2 + fk * 4;
                    *reinterpret_cast<uint2*>(a.y_hi + yo + co) = pk_hi[q];
                    if (X3) *reinterpret_cast<uint2*>(a.y_lo + yo + co) = pk_lo[q];
                }
            }
        }
    } else {
        // Residual loads of a whole row group go out in one burst BEFORE that group's stores: a load issued behind a store also waits for
        // the store's acknowledgement (loads and stores retire through one in-order vmcnt on gfx9), so "load row j, store row j, load row
        // j + 1, ..." pays a store round trip per row.  Groups are sized to <= 64 VGPRs of residual.
        constexpr int RB = (FM * FN >= 32) ? 16 : 32;      // (the 256 x 256 tile already sits at the register limit: smaller bursts, no extra spills)
        constexpr int JG = (FM * FN * NP <= RB) ? FM : (RB / (FN * NP) >= 1 ? RB / (FN * NP) : 1);
        const bool has_res = a.r_hi != nullptr;
        const bool after = a.res_after_act;
        // GroupNorm statistics of the output for the layer's consumer (a.gn_out): per-lane fp32 (sum, sum of squares) of its FN channel quads over
        // its FM pixel rows.  4-wave tiles up to 128 x 64 only: the 8-wave tiles sit at the register limit and the 128 x 128 tile would drop from
        // two workgroups per CU to one (184 + 64 -> 206 + 64 registers); the launcher runs k_gn_stats behind those.
        constexpr bool ST = NW == 4 && FM * FN < 16;
        float gs[ST ? FN : 1][4], gq[ST ? FN : 1][4];
#pragma unroll
        for (int i = 0; i < (ST ? FN : 1); ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) { gs[i][e] = 0.f; gq[i][e] = 0.f; }
#pragma unroll
        for (int j0 = 0; j0 < FM; j0 += JG) {
            uint2 rh[JG][FN], rl[JG][FN];
            if (has_res) {
#pragma unroll
                for (int jj = 0; jj < JG; ++jj) {
                    if (j0 + jj >= FM) break;
                    int m = m0 + pm0 + (j0 + jj) * 16 + fr;
                    m = m < a.M ? m : a.M - 1;                      // clamped, never branched around: the stores are masked
                    const int b = mf_fdiv(m, a.dv_hw_mul, a.dv_hw_shr);
                    const int rem = m - b * a.HqWq;
                    const int qi = mf_fdiv(rem, a.dv_w_mul, a.dv_w_shr), qj = rem - qi * a.Wq;
                    const int64_t ro = (int64_t)b * a.rb + (int64_t)qi * a.ri + (int64_t)qj * a.rj;
#pragma unroll
                    for (int i = 0; i < FN; ++i) {
                        int c = n0 + cn0 + i * 16 + fk * 4;
                        c = c < a.N ? c : 0;
                        rh[jj][i] = *reinterpret_cast<const uint2*>(a.r_hi + ro + c);
                        if (X3) rl[jj][i] = *reinterpret_cast<const uint2*>(a.r_lo + ro + c);
                    }
                }
            }
#pragma unroll
            for (int jj = 0; jj < JG; ++jj) {
                const int j = j0 + jj;
                if (j >= FM) break;
                const int m = m0 + pm0 + j * 16 + fr;
                const bool row_ok = m < a.M;
                const int mc = row_ok ? m : a.M - 1;
                const int b = mf_fdiv(mc, a.dv_hw_mul, a.dv_hw_shr);
                const int rem = mc - b * a.HqWq;
                const int qi = mf_fdiv(rem, a.dv_w_mul, a.dv_w_shr), qj = rem - qi * a.Wq;
                const int64_t yo = zy + (int64_t)b * a.yb + (int64_t)qi * a.yi + (int64_t)qj * a.yj + ph.y_off;
                uint2 pk_hi[FN], pk_lo[FN];
                float row_s = 0.f, row_q = 0.f;
#pragma unroll
                for (int i = 0; i < FN; ++i) {
                    float v[4] = {acc[i][j][0] + bq[i].x, acc[i][j][1] + bq[i].y, acc[i][j][2] + bq[i].z, acc[i][j][3] + bq[i].w};
                    float r[4] = {0.f, 0.f, 0.f, 0.f};
                    if (has_res) {
                        r[0] = bf2f(rh[jj][i].x & 0xffffu); r[1] = bf2f(rh[jj][i].x >> 16); r[2] = bf2f(rh[jj][i].y & 0xffffu); r[3] = bf2f(rh[jj][i].y >> 16);
                        if (X3) {
                            r[0] += bf2f(rl[jj][i].x & 0xffffu); r[1] += bf2f(rl[jj][i].x >> 16); r[2] += bf2f(rl[jj][i].y & 0xffffu); r[3] += bf2f(rl[jj][i].y >> 16);
                        }
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float x = v[e] + (after ? 0.f : r[e]);
                        if (ACT == 1) x = fmaxf(x, 0.f);
                        else if (ACT == 2) x = 1.f / (1.f + __expf(-x));
                        else if (ACT == 3) x = gelu_erf(x);
                        else if (ACT == 4) x = x / (1.f + expf(-x));
                        v[e] = x + (after ? r[e] : 0.f);
                    }
                    if (a.ln_out && n0 + cn0 + i * 16 + fk * 4 < a.N) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) { row_s += v[e]; row_q += v[e] * v[e]; }
                    }
                    uint32_t h[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) h[e] = f2bf(v[e]);
                    if (ST && row_ok) {
                        // statistics of the STORED values, as k_gn_stats reads them: bf16 stores the rounded hi alone (hi + lo is v to 2^-17)
#pragma unroll
                        for (int e = 0; e < 4; ++e) { const float s = X3 ? v[e] : bf2f(h[e]); gs[i][e] += s; gq[i][e] += s * s; }
                    }
                    pk_hi[i] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
                    if (X3) {
                        uint32_t l[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) l[e] = f2bf(v[e] - bf2f(h[e]));
                        pk_lo[i] = make_uint2(l[0] | (l[1] << 16), l[2] | (l[3] << 16));
                    }
                }
                if (a.ln_out) {
                    row_s += __shfl_xor(row_s, 16); row_q += __shfl_xor(row_q, 16);
                    row_s += __shfl_xor(row_s, 32); row_q += __shfl_xor(row_q, 32);
                    if (fk == 0 && row_ok) {
                        atomicAdd(a.ln_out + 2 * (int64_t)m, (double)row_s);
                        atomicAdd(a.ln_out + 2 * (int64_t)m + 1, (double)row_q);
                    }
                }
                if (FN % 2 == 0 && a.wide_store) {
#pragma unroll
                    for (int i = 0; i + 1 < FN; i += 2) {
                        const int c16 = n0 + cn0 + i * 16;
                        store_pair16(a.y_hi, yo, c16, 16, fk, pk_hi[i], pk_hi[i + 1], a.N, row_ok);
                        if (X3) store_pair16(a.y_lo, yo, c16, 16, fk, pk_lo[i], pk_lo[i + 1], a.N, row_ok);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < FN; ++i) {
                        const int c = n0 + cn0 + i * 16 + fk * 4;
                        if (!row_ok || c >= a.N) continue;
                        *reinterpret_cast<uint2*>(a.y_hi + yo + c) = pk_hi[i];
                        if (X3) *reinterpret_cast<uint2*>(a.y_lo + yo + c) = pk_lo[i];
                    }
                }
            }
        }
        if (ST && a.gn_out) {
            // sum over the wave's 16 pixel columns, park per (wave row, channel) in LDS (the ring is drained), then one thread per (group, moment)
            // adds its channels in a fixed order and issues ONE fp64 atomic -- the granularity k_gn_stats has.  The launcher guarantees that a
            // pixel tile lies inside one sample (HqWq % BM == 0).
#pragma unroll
            for (int i = 0; i < FN; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int off = 1; off < 16; off <<= 1) { gs[i][e] += __shfl_xor(gs[i][e], off); gq[i][e] += __shfl_xor(gq[i][e], off); }
            __syncthreads();                                   // every wave is done reading the last K tile
            float* sb = reinterpret_cast<float*>(smem);        // [WGM][BN][2]
            if (fr == 0) {
#pragma unroll
                for (int i = 0; i < FN; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int cl = cn0 + i * 16 + fk * 4 + e;
                        *reinterpret_cast<float2*>(sb + ((size_t)wave_m * BN + cl) * 2) = make_float2(gs[i][e], gq[i][e]);
                    }
            }
            __syncthreads();
            const int cpg = a.gn_out_cpg;
            const int c_end = min(a.N, n0 + BN);               // channels [n0, c_end) of this tile exist
            const int g_first = n0 / cpg, ng = (c_end - 1) / cpg - g_first + 1;
            if (tid < 2 * ng) {
                const int g = g_first + (tid >> 1), mo = tid & 1;
                const int c_lo = max(g * cpg, n0), c_hi = min((g + 1) * cpg, c_end);
                double acc_d = 0.0;
                for (int c = c_lo; c < c_hi; ++c)
#pragma unroll
                    for (int wm = 0; wm < WGM; ++wm) acc_d += (double)sb[((size_t)wm * BN + (c - n0)) * 2 + mo];
                const int b = mf_fdiv(m0, a.dv_hw_mul, a.dv_hw_shr);
                atomicAdd(a.gn_out + 2 * ((size_t)b * a.gn_out_groups + g) + mo, acc_d);
            }
        }
    }
    if (dbg && threadIdx.x == 0) dbg[3] = __builtin_amdgcn_s_memtime();
}

// fp32 partials of one channel quad, summed in split order (bias first): the loads of four splits are issued together and added one after the other, so
// the value is the one a serial loop gives while the thread waits for ONE round trip per four splits instead of four (the combine kernels are pure latency:
// 4 - 16 dependent loads of a few MB in all took 6 - 12 us per launch, 111 launches per UNet step and 27 per Wav2Lip step).
__device__ __forceinline__ float4 splitk_sum(const float* w, int64_t ws_split, int nsplit, float4 s) {
    int k = 0;
    for (; k + 4 <= nsplit; k += 4) {
        const float4 v0 = *reinterpret_cast<const float4*>(w + (int64_t)k * ws_split);
        const float4 v1 = *reinterpret_cast<const float4*>(w + (int64_t)(k + 1) * ws_split);
        const float4 v2 = *reinterpret_cast<const float4*>(w + (int64_t)(k + 2) * ws_split);
        const float4 v3 = *reinterpret_cast<const float4*>(w + (int64_t)(k + 3) * ws_split);
        s.x += v0.x; s.y += v0.y; s.z += v0.z; s.w += v0.w;
        s.x += v1.x; s.y += v1.y; s.z += v1.z; s.w += v1.w;
        s.x += v2.x; s.y += v2.y; s.z += v2.z; s.w += v2.w;
        s.x += v3.x; s.y += v3.y; s.z += v3.z; s.w += v3.w;
    }
    if (k + 2 <= nsplit) {
        const float4 v0 = *reinterpret_cast<const float4*>(w + (int64_t)k * ws_split);
        const float4 v1 = *reinterpret_cast<const float4*>(w + (int64_t)(k + 1) * ws_split);
        s.x += v0.x; s.y += v0.y; s.z += v0.z; s.w += v0.w;
        s.x += v1.x; s.y += v1.y; s.z += v1.z; s.w += v1.w;
        k += 2;
    }
    if (k < nsplit) {
        const float4 v0 = *reinterpret_cast<const float4*>(w + (int64_t)k * ws_split);
        s.x += v0.x; s.y += v0.y; s.z += v0.z; s.w += v0.w;
    }
    return s;
}

// the residual quad of a pixel, requested BEFORE the partials are summed (one more load in flight beside them) and applied where epilogue_store_v would
struct ResQuad { uint2 h, l; };
__device__ __forceinline__ ResQuad load_residual(const ConvArgs& a, int64_t ro, int c, bool x3) {
    ResQuad r{make_uint2(0u, 0u), make_uint2(0u, 0u)};
    if (a.r_hi) {
        r.h = *reinterpret_cast<const uint2*>(a.r_hi + ro + c);
        if (x3) r.l = *reinterpret_cast<const uint2*>(a.r_lo + ro + c);
    }
    return r;
}
__device__ __forceinline__ void apply_residual(float (&v)[4], const ResQuad& r, bool x3) {
    v[0] += bf2f(r.h.x & 0xffffu); v[1] += bf2f(r.h.x >> 16);
    v[2] += bf2f(r.h.y & 0xffffu); v[3] += bf2f(r.h.y >> 16);
    if (x3) {
        v[0] += bf2f(r.l.x & 0xffffu); v[1] += bf2f(r.l.x >> 16);
        v[2] += bf2f(r.l.y & 0xffffu); v[3] += bf2f(r.l.y >> 16);
    }
}
// epilogue_store_v with the residual already in registers (same operation order)
__device__ __forceinline__ void epilogue_store_pre(const ConvArgs& a, float (&v)[4], int64_t yo, int c, bool x3, const ResQuad& r) {
    if (a.r_hi && !a.res_after_act) apply_residual(v, r, x3);
    if (a.act == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    } else if (a.act == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = 1.f / (1.f + __expf(-v[e]));
    } else if (a.act == 3) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.f + erff(v[e] * 0.70710678118654752f));
    } else if (a.act == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] / (1.f + expf(-v[e]));
    }
    if (a.r_hi && a.res_after_act) apply_residual(v, r, x3);
    uint32_t h[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = f2bf(v[e]);
    *reinterpret_cast<uint2*>(a.y_hi + yo + c) = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    if (x3) {
        uint32_t l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) l[e] = f2bf(v[e] - bf2f(h[e]));
        *reinterpret_cast<uint2*>(a.y_lo + yo + c) = make_uint2(l[0] | (l[1] << 16), l[2] | (l[3] << 16));
    } else {
        // v leaves as the value stored (bf16: the rounded hi alone), so that k_splitk_epilogue_stats sums the stored output, as k_gn_stats does
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = bf2f(h[e]);
    }
}

// Combines the split-K partial tiles: one thread per (output pixel, 4 channels).
// ws layout: [split][B][Ho][Wo][N] fp32 (unpadded); output / residual are padded NHWC planes.
// (thread index -> (pixel, channel quad) -> (image, row, column) by multiply-shift, EpiDiv: as three 64-bit divisions this was ~400 of the thread's ~450 instructions)
struct EpiDiv { uint32_t nq_mul, nq_shr, w_mul, w_shr, h_mul, h_shr, g_mul, g_shr, c_mul, c_shr; };
__global__ __launch_bounds__(256) void k_splitk_epilogue(const ConvArgs a, int nsplit, int Ho, int Wo, int total, const EpiDiv dv) {
    const int idx0 = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const bool live = idx0 < total;
    if (!live && !a.ln_out) return;
    const int idx = live ? idx0 : total - 1;              // (a LayerNorm producer's tail lanes stay for the wave reduction below: they recompute the last quad, store nothing)
    const bool geglu = a.act == 5;
    const int nq = (geglu ? a.N >> 1 : a.N) >> 2;         // output channel quads
    const int pix0 = mf_fdiv(idx, dv.nq_mul, dv.nq_shr);
    const int co = (idx - pix0 * nq) * 4;                 // output channel
    const int c = geglu ? (co >> 4) * 32 + (co & 15) : co; // GEMM row of its value (GEGLU: the gate sits 16 rows on)
    const int prow = mf_fdiv(pix0, dv.w_mul, dv.w_shr);
    const int ox = pix0 - prow * Wo;
    const int b = mf_fdiv(prow, dv.h_mul, dv.h_shr);
    const int oy = prow - b * Ho;
    const bool x3 = a.y_lo != nullptr;
    // y/r strides of the UNIT output grid are passed in (yi, yj) / (ri, rj) by the launcher
    const int64_t yo = (int64_t)b * a.yb + (int64_t)oy * a.yi + (int64_t)ox * a.yj;
    const int64_t ro = (int64_t)b * a.rb + (int64_t)oy * a.ri + (int64_t)ox * a.rj;
    const ResQuad rq = load_residual(a, ro, co, x3);
    const float* w = a.ws + (((int64_t)b * Ho + oy) * Wo + ox) * a.N + c;
    float v[4];
    if (a.ln_in) {
        // LayerNorm folded into this layer (ConvArgs::ln_in): the partials sum the RAW tensor's products; mean / rstd of the row finish the normalisation
        const int64_t m = ((int64_t)b * Ho + oy) * Wo + ox;
        const double2 sq = *reinterpret_cast<const double2*>(a.ln_in + 2 * m);
        const double mean = sq.x * (double)a.ln_inv_c, var = sq.y * (double)a.ln_inv_c - mean * mean;
        const float mu = (float)mean, rs = (float)(1.0 / sqrt((var > 0.0 ? var : 0.0) + (double)a.ln_eps));
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 s = splitk_sum(w, a.ws_split, nsplit, z), cs = *reinterpret_cast<const float4*>(a.ln_cs + c), bb = *reinterpret_cast<const float4*>(a.bias + c);
        // (scalar FMAs pinned against packing, as in k_conv_igemm's LayerNorm epilogue: the gfx950 packed-fp32 op_sel erratum, see the note there)
        auto ln4 = [&](const float4& q, const float4& cq, const float4& bq4, float (&o)[4]) __attribute__((always_inline)) {
            float t0 = q.x - mu * cq.x, t1 = q.y - mu * cq.y, t2 = q.z - mu * cq.z, t3 = q.w - mu * cq.w;
            asm volatile("" : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3));
            o[0] = rs * t0 + bq4.x; o[1] = rs * t1 + bq4.y; o[2] = rs * t2 + bq4.z; o[3] = rs * t3 + bq4.w;
            asm volatile("" : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]));
        };
        ln4(s, cs, bb, v);
        if (geglu) {
            const float4 g = splitk_sum(w + 16, a.ws_split, nsplit, z), cg = *reinterpret_cast<const float4*>(a.ln_cs + c + 16), bg = *reinterpret_cast<const float4*>(a.bias + c + 16);
            float gt[4];
            ln4(g, cg, bg, gt);
            v[0] *= gelu_erf(gt[0]); v[1] *= gelu_erf(gt[1]); v[2] *= gelu_erf(gt[2]); v[3] *= gelu_erf(gt[3]);
        }
    } else {
        const float4 s = splitk_sum(w, a.ws_split, nsplit, *reinterpret_cast<const float4*>(a.bias + c));
        v[0] = s.x; v[1] = s.y; v[2] = s.z; v[3] = s.w;
        if (geglu) {
            const float4 g = splitk_sum(w + 16, a.ws_split, nsplit, *reinterpret_cast<const float4*>(a.bias + c + 16));
            v[0] *= gelu_erf(g.x); v[1] *= gelu_erf(g.y); v[2] *= gelu_erf(g.z); v[3] *= gelu_erf(g.w);
        }
    }
    if (live) epilogue_store_pre(a, v, yo, co, x3, rq);
    if (a.ln_out) {
        // LayerNorm statistics of the stored row for the consumer: (sum, sum of squares) of this thread's quad, added up over the lanes of the wave that hold the
        // same pixel (a segmented suffix sum: consecutive lanes = consecutive quads of a pixel), one fp64 atomic per (wave, pixel, moment)
        float ps = (v[0] + v[1]) + (v[2] + v[3]), pq = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
        const int64_t pix = live ? (int64_t)pix0 : -1;
        if (!live) { ps = 0.f; pq = 0.f; }
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float os = __shfl_down(ps, off), oq = __shfl_down(pq, off);
            const int64_t op = __shfl_down(pix, off);
            if (lane + off < 64 && op == pix) { ps += os; pq += oq; }
        }
        const int64_t prev = __shfl_up(pix, 1);
        if (live && (lane == 0 || prev != pix)) {
            atomicAdd(a.ln_out + 2 * pix, (double)ps);
            atomicAdd(a.ln_out + 2 * pix + 1, (double)pq);
        }
    }
}

// The same combine for a layer whose consumer is a GroupNorm (a.gn_out): the (sum, sum of squares) of the stored values per (sample, group)
// come out of this pass instead of a k_gn_stats pass over the tensor.  grid (pixel blocks of P, batch); a thread owns a channel quad and walks
// the block's pixels pp, pp + ppi, ... (one pixel's quads are contiguous: coalesced as in k_gn_stats), two pixels per iteration with both pixels' loads in
// flight together; fp32 partials over <= 64 pixels, then fp64 LDS bins per group and one global fp64 atomic per (workgroup, group, moment).  No GEGLU (its
// consumer is a Linear).
__global__ __launch_bounds__(256) void k_splitk_epilogue_stats(const ConvArgs a, int nsplit, int Ho, int Wo, int P, const EpiDiv dv) {
    __shared__ double bins[2 * 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int nq = a.N >> 2;
    const int cols = nq < 256 ? nq : 256;
    const int ppi = 256 / cols;
    const int pp = mf_fdiv(tid, dv.c_mul, dv.c_shr), k0 = tid - pp * cols;
    const int T = Ho * Wo, t0 = blockIdx.x * P, t1 = min(T, t0 + P);
    const int groups = a.gn_out_groups, cpg = a.gn_out_cpg;
    const bool x3 = a.y_lo != nullptr;
    for (int i = tid; i < 2 * groups; i += 256) bins[i] = 0.0;
    __syncthreads();
    if (pp < ppi) {
        for (int k = k0; k < nq; k += 256) {
            const int c = k * 4;
            const float4 bq = *reinterpret_cast<const float4*>(a.bias + c);
            float s4[4] = {0.f, 0.f, 0.f, 0.f}, q4[4] = {0.f, 0.f, 0.f, 0.f};
            for (int t = t0 + pp; t < t1; t += 2 * ppi) {
                const int tb = t + ppi;
                const bool two = tb < t1;
                const int ta = t, tc = two ? tb : t;                  // (the second pixel clamped onto the first when the block ends: loaded, not stored)
                const int oy0 = mf_fdiv(ta, dv.w_mul, dv.w_shr), ox0 = ta - oy0 * Wo, oy1 = mf_fdiv(tc, dv.w_mul, dv.w_shr), ox1 = tc - oy1 * Wo;
                const int64_t yo0 = (int64_t)b * a.yb + (int64_t)oy0 * a.yi + (int64_t)ox0 * a.yj, yo1 = (int64_t)b * a.yb + (int64_t)oy1 * a.yi + (int64_t)ox1 * a.yj;
                const int64_t ro0 = (int64_t)b * a.rb + (int64_t)oy0 * a.ri + (int64_t)ox0 * a.rj, ro1 = (int64_t)b * a.rb + (int64_t)oy1 * a.ri + (int64_t)ox1 * a.rj;
                const ResQuad r0 = load_residual(a, ro0, c, x3), r1 = load_residual(a, ro1, c, x3);
                const float* w0 = a.ws + (((int64_t)b * Ho + oy0) * Wo + ox0) * a.N + c;
                const float* w1 = a.ws + (((int64_t)b * Ho + oy1) * Wo + ox1) * a.N + c;
                float4 sa = bq, sb = bq;
                int sp = 0;
                for (; sp + 2 <= nsplit; sp += 2) {                   // four loads in flight (two pixels x two splits), each pixel's sum in split order
                    const float4 a0 = *reinterpret_cast<const float4*>(w0 + (int64_t)sp * a.ws_split), a1 = *reinterpret_cast<const float4*>(w0 + (int64_t)(sp + 1) * a.ws_split);
                    const float4 b0 = *reinterpret_cast<const float4*>(w1 + (int64_t)sp * a.ws_split), b1 = *reinterpret_cast<const float4*>(w1 + (int64_t)(sp + 1) * a.ws_split);
                    sa.x += a0.x; sa.y += a0.y; sa.z += a0.z; sa.w += a0.w;
                    sa.x += a1.x; sa.y += a1.y; sa.z += a1.z; sa.w += a1.w;
                    sb.x += b0.x; sb.y += b0.y; sb.z += b0.z; sb.w += b0.w;
                    sb.x += b1.x; sb.y += b1.y; sb.z += b1.z; sb.w += b1.w;
                }
                if (sp < nsplit) {
                    const float4 a0 = *reinterpret_cast<const float4*>(w0 + (int64_t)sp * a.ws_split), b0 = *reinterpret_cast<const float4*>(w1 + (int64_t)sp * a.ws_split);
                    sa.x += a0.x; sa.y += a0.y; sa.z += a0.z; sa.w += a0.w;
                    sb.x += b0.x; sb.y += b0.y; sb.z += b0.z; sb.w += b0.w;
                }
                float v[4] = {sa.x, sa.y, sa.z, sa.w};
                epilogue_store_pre(a, v, yo0, c, x3, r0);
#pragma unroll
                for (int e = 0; e < 4; ++e) { s4[e] += v[e]; q4[e] += v[e] * v[e]; }
                if (two) {
                    float u[4] = {sb.x, sb.y, sb.z, sb.w};
                    epilogue_store_pre(a, u, yo1, c, x3, r1);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { s4[e] += u[e]; q4[e] += u[e] * u[e]; }
                }
            }
            int g_cur = mf_fdiv(c, dv.g_mul, dv.g_shr);
            double as = 0.0, aq = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int g = mf_fdiv(c + e, dv.g_mul, dv.g_shr);
                if (g != g_cur) {
                    atomicAdd(&bins[2 * g_cur], as); atomicAdd(&bins[2 * g_cur + 1], aq);
                    g_cur = g; as = 0.0; aq = 0.0;
                }
                as += (double)s4[e]; aq += (double)q4[e];
            }
            atomicAdd(&bins[2 * g_cur], as); atomicAdd(&bins[2 * g_cur + 1], aq);
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * groups; i += 256) atomicAdd(&a.gn_out[2 * ((size_t)b * groups) + i], bins[i]);
}

// the multiply-shift constants of the combine kernels: channel quads per pixel, output width / height, channels per GroupNorm group, quad columns per 256 threads
static EpiDiv epi_div(const ConvArgs& e, int Ho, int Wo) {
    EpiDiv d{};
    const int nq = ((e.act == 5 ? e.N >> 1 : e.N) >> 2);
    const int nq_all = e.N >> 2, cols = nq_all < 256 ? nq_all : 256;
    mf_fastdiv((uint32_t)nq, &d.nq_mul, &d.nq_shr);
    mf_fastdiv((uint32_t)Wo, &d.w_mul, &d.w_shr);
    mf_fastdiv((uint32_t)Ho, &d.h_mul, &d.h_shr);
    mf_fastdiv((uint32_t)(e.gn_out_cpg > 0 ? e.gn_out_cpg : 1), &d.g_mul, &d.g_shr);
    mf_fastdiv((uint32_t)(cols > 0 ? cols : 1), &d.c_mul, &d.c_shr);
    return d;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
namespace {

template <int BM, int BN, int WGM, int WGN, bool X3, int BK, int NST, int LD = 0, bool Q = false>
int launch_cfg_n(const ConvArgs& a, int nphase, int nsplit, int goff_max, hipStream_t s) {
    static bool attr_done = false;
    auto kern = k_conv_igemm<BM, BN, WGM, WGN, X3, BK, NST, LD, Q>;
    if (!attr_done) {
        MF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_done = true;
    }
    size_t lds = (size_t)(LD == 2 ? 1 : NST) * (BM + BN) * BK * 2 * (X3 ? 2 : 1) + (size_t)goff_max * 4;
    if constexpr (LD == 3) {
        lds = (size_t)igemm_ring<BM, BN, BK, X3>() * (BM + BN) * BK * 2 * (X3 ? 2 : 1) + (size_t)goff_max * 4;
        if (lds > 160 * 1024) { mf_set_error("conv: producer-wave tile %dx%d needs %zu bytes of LDS", BM, BN, lds); return MF_ERR_INVALID; }
    }
    dim3 grid(a.tiles_m * a.tiles_n, nsplit, a.zgroups ? a.zgroups : nphase);
    ConvArgs b = a;
    mf_fastdiv((uint32_t)(a.m_fastest ? a.tiles_m : a.tiles_n), &b.dv_t_mul, &b.dv_t_shr);
    mf_fastdiv((uint32_t)nsplit, &b.dv_s_mul, &b.dv_s_shr);
    hipLaunchKernelGGL(kern, grid, dim3((WGM * WGN + (LD == 3 ? igemm_producers<BM, BN, BK>() : 0)) * 64), lds, s, b);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

template <int BM, int BN, int WGM, int WGN, bool X3, int BK, bool Q = false>
int launch_cfg(const ConvArgs& a, int nphase, int nsplit, int goff_max, hipStream_t s) {
    // Two operand paths, a measured choice per layer (ConvArgs::ld, mf_conv_tune):
    //   ld 0  both tiles by LDS-DMA into a 2-stage ring (deeper rings halve the workgroups per CU: measured slower, profiles/r01_ring_ab.md)
    //   ld 2  (4-wave tiles only, their default) operands through registers into ONE LDS stage, so that 64-deep bf16x3 tiles (128-byte operand rows)
    //         still leave 2-3 workgroups per CU; the 8-wave 256-wide tiles have no VGPRs to spare
    // Per-op A/B at batch 8: UNet 11.05 -> 10.62 ms, Wav2Lip 14.6 k -> 15.1 k frames/s with ld 2 as the default; every variant within +-15 % per layer.
    const int regs = a.ld >= 0 ? a.ld : 2;
    if constexpr (WGM * WGN == 4 && X3 && !Q && BN >= 64 && BM >= 64 && igemm_ring<BM, BN, BK, X3>() >= 2) {
        //   ld 3 / 4  producer waves own every LDS-DMA piece, the compute waves only LDS reads and MFMAs (k_conv_igemm's LD 3); 3: 64-deep stages (128-byte
        //         operand rows: every L2 request a full line -- the 64-byte rows of 32-deep stages cap the L2 -> LDS path at 15 - 18 TB/s chip-wide, which is what
        //         the 128 x 128 tile's loop ran at), ring of 4 / 3 / 2 stages for the 64 x 64 / 128 x 64 / 128 x 128 tiles; 4: 32-deep stages, ring of 8 / 6 / 4
        if (regs == 3 || regs == 4) return launch_cfg_n<BM, BN, WGM, WGN, X3, BK, 2, 3, Q>(a, nphase, nsplit, goff_max, s);
    }
    if (regs == 3 || regs == 4) { mf_set_error("conv: no producer-wave kernel for tile %dx%d", BM, BN); return MF_ERR_INVALID; }
    if constexpr (WGM * WGN == 4) {
        if (regs == 2) return launch_cfg_n<BM, BN, WGM, WGN, X3, BK, 2, 2, Q>(a, nphase, nsplit, goff_max, s);
    }
    return launch_cfg_n<BM, BN, WGM, WGN, X3, BK, 2, 0, Q>(a, nphase, nsplit, goff_max, s);
}

// the 128 x 80 tile exists for ONE reason: 320 output channels over 8192 pixels (the UNet's outer level at batch 8) are 64 x 4 = 256 workgroups -- one round of
// the chip's 256 CUs -- where 128 x 64 makes 320 (two rounds, the second a quarter full).  Producer-wave path, bf16x3 only.
template <int BM, int BN, int WGM, int WGN>
int launch_pw_only(const ConvArgs& a, int nphase, int nsplit, int goff_max, bool x3, bool q, hipStream_t s) {
    if (x3 && !q && a.ld == 3) return launch_cfg_n<BM, BN, WGM, WGN, true, 64, 2, 3, false>(a, nphase, nsplit, goff_max, s);
    if (x3 && !q && a.ld == 4) return launch_cfg_n<BM, BN, WGM, WGN, true, 32, 2, 3, false>(a, nphase, nsplit, goff_max, s);
    mf_set_error("conv: the %dx%d tile has only the bf16x3 producer-wave kernels (ld 3 / 4)", BM, BN);
    return MF_ERR_INVALID;
}

template <int BM, int BN, int WGM, int WGN>
int launch_prec(const ConvArgs& a, int nphase, int nsplit, int goff_max, bool x3, bool q, hipStream_t s) {
    if (q) {
        // f16 + FP6 format: 64-deep tiles on the 4-wave tiles (one FP6 instruction covers the tile), 32-deep on the 8-wave ones (two planes of 256 + 256 rows)
        if constexpr (BN >= 64 && BM >= 64) {
            if constexpr (WGM * WGN == 4) return launch_cfg<BM, BN, WGM, WGN, true, 64, true>(a, nphase, nsplit, goff_max, s);
            else return launch_cfg<BM, BN, WGM, WGN, true, 32, true>(a, nphase, nsplit, goff_max, s);
        } else {
            mf_set_error("conv (f16q): no implicit-GEMM kernel for the narrow %dx%d tile", BM, BN);
            return MF_ERR_INVALID;
        }
    }
    if constexpr (WGM * WGN == 4 && BN >= 64) {
        // producer-wave path: ld 3 = 64-deep stages, ld 4 = 32-deep stages
        if ((a.ld == 3 || a.ld == 4) && x3) {
            if (a.ld == 3) return launch_cfg<BM, BN, WGM, WGN, true, 64>(a, nphase, nsplit, goff_max, s);
            return launch_cfg<BM, BN, WGM, WGN, true, 32>(a, nphase, nsplit, goff_max, s);
        }
    }
    // bf16x3 doubles the LDS image: 64-deep tiles only where two stages of (hi, lo) still leave >= 2
    // workgroups per CU (the small tiles of the long-K layers), 32-deep otherwise
    constexpr bool deep = (BM + BN) <= 128;
    // 64-deep bf16x3 tiles (128-byte operand rows: every request a full line) on every 4-wave tile
    if constexpr (WGM * WGN == 4 && !deep) {
        if (x3) return launch_cfg<BM, BN, WGM, WGN, true, 64>(a, nphase, nsplit, goff_max, s);
    }
    return x3 ? launch_cfg<BM, BN, WGM, WGN, true, deep ? 64 : 32>(a, nphase, nsplit, goff_max, s)
              : launch_cfg<BM, BN, WGM, WGN, false, 64>(a, nphase, nsplit, goff_max, s);
}

int cdiv(int a, int b) { return (a + b - 1) / b; }
bool g_no_halo_wide = false;   // set while mf_conv_plan_create builds the implicit-GEMM twin of a wide halo plan

}  // namespace

// f16 + FP6 residual format of one weight set: plane 0 = f16(w) rows [slice][tap][Npad][32]; plane 1 = per (slice, tap, row) 64 bytes
// [q6(f16(w)) | q6(w - f16(w))], each 24 B of e2m3 codes (value t in bits [6t, 6t+6)) + the block's E8M0 byte + pad.  The pixel side stores
// [q6(x - f16(x)) | q6(f16(x))], so K block 0 of the correction instruction is q6(wh).xl and block 1 is wl.q6(xh).  wfun(n, c, tap) = the fp32 weight.
// one 32-channel block of one weight row: hi32 = the 32 f16 values, lo32 (64 bytes) = [q6(f16(w)) | q6(w - f16(w))]
static void pack_q_block(const float* w32, bf16_t* hi32, bf16_t* lo32) {
    auto enc = [](float y) -> uint32_t {
        const uint32_t sgn = y < 0.f ? 0x20u : 0u;
        const float a = std::fmin(std::fabs(y), 7.5f);
        uint32_t code;
        if (a < 1.f) code = (uint32_t)std::nearbyint(a * 8.f);
        else {
            const int e = a < 2.f ? 0 : (a < 4.f ? 1 : 2);
            const uint32_t m = (uint32_t)std::nearbyint((a * (e == 0 ? 1.f : (e == 1 ? 0.5f : 0.25f)) - 1.f) * 8.f);
            code = ((uint32_t)(e + 1) << 3) + m;
            if (code > 0x1fu) code = 0x1fu;
        }
        return sgn | code;
    };
    float blk[2][32], mx[2] = {0.f, 0.f};
    for (int e = 0; e < 32; ++e) {
        const _Float16 h = (_Float16)w32[e];
        blk[0][e] = (float)h; blk[1][e] = w32[e] - blk[0][e];
        uint16_t bits; __builtin_memcpy(&bits, &h, 2);
        hi32[e] = bits;
        mx[0] = std::fmax(mx[0], std::fabs(blk[0][e])); mx[1] = std::fmax(mx[1], std::fabs(blk[1][e]));
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(lo32);     // 64 bytes
    for (int b = 0; b < 2; ++b) {
        int ex = 0;
        if (mx[b] > 0.f) { (void)std::frexp(mx[b], &ex); ex = 3 - ex; }
        const float sc = std::ldexp(1.f, ex);
        uint32_t w8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int e = 0; e < 32; ++e) {
            const uint32_t code = enc(blk[b][e] * sc);
            const int bit = 6 * e;
            w8[bit >> 5] |= code << (bit & 31);
            if ((bit & 31) > 26) w8[(bit >> 5) + 1] |= code >> (32 - (bit & 31));
        }
        w8[6] = (uint32_t)(127 - ex) & 0xffu;
        for (int k = 0; k < 8; ++k) dst[8 * b + k] = w8[k];
    }
}

template <class W>
static void pack_q_weights(int n_slices, int ntaps, int Npad, int cout, int cin, W wfun, bf16_t* hi, bf16_t* lo) {
    float w32[32];
    for (int sl = 0; sl < n_slices; ++sl)
        for (int tap = 0; tap < ntaps; ++tap)
            for (int n = 0; n < cout; ++n) {
                const int64_t row = (((int64_t)sl * ntaps + tap) * Npad + n) * 32;
                for (int e = 0; e < 32; ++e) {
                    const int c = sl * 32 + e;
                    w32[e] = c < cin ? wfun(n, c, tap) : 0.f;
                }
                pack_q_block(w32, &hi[row], &lo[row]);
            }
}

int mf_conv_plan_create(ConvPlan* p, const mf_conv2d_desc& d, const float* weight, const float* bias,
                        const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                        const float* bn_var, int precision) {
    MF_REQUIRE(d.cin > 0 && d.cout > 0 && d.kh > 0 && d.kw > 0, "conv: bad channel/kernel size");
    MF_REQUIRE(d.stride_h > 0 && d.stride_w > 0 && d.in_h > 0 && d.in_w > 0, "conv: bad stride/input size");
    MF_REQUIRE(precision == MF_PREC_BF16 || precision == MF_PREC_BF16X3 || precision == MF_PREC_F16Q, "conv: unknown precision %d", precision);
    std::vector<float> gw, gb;
    if (d.act == 5) {
        // GEGLU (diffusers): out = x[:, :cout/2] * gelu(x[:, cout/2:]).  Rows are re-ordered into alternating blocks of 16
        // value channels and their 16 gate channels, so one lane of the accumulator tile holds a value and its gate.
        MF_REQUIRE(!d.transposed && !bn_gamma && !d.residual && d.cout % 32 == 0, "conv: GEGLU needs a plain conv with cout %% 32 == 0");
        const size_t row = (size_t)d.cin * d.kh * d.kw;
        gw.resize(row * d.cout); gb.assign(d.cout, 0.f);
        for (int r = 0; r < d.cout; ++r) {
            const int q = r / 32, u = r % 32;
            const int src = u < 16 ? 16 * q + u : d.cout / 2 + 16 * q + (u - 16);
            std::copy(weight + row * src, weight + row * (src + 1), gw.begin() + row * r);
            if (bias) gb[r] = bias[src];
        }
        weight = gw.data();
        bias = gb.data();
    }
    // LayerNorm folded into this layer (ConvPlan::ln_gamma set by the network builder): W' = W diag(gamma), bias' = bias + W beta (fp64 sums), and the column sums
    // of W' AS THE KERNEL MULTIPLIES IT (hi + lo bf16, or hi alone in the single-pass mode) for the epilogue's mean correction
    std::vector<float> lw, lb, lcs;
    if (p->ln_gamma) {
        MF_REQUIRE(d.kh == 1 && d.kw == 1 && d.stride_h == 1 && d.stride_w == 1 && d.pad_h == 0 && d.pad_w == 0 && !d.transposed && !d.upsample && !bn_gamma && !d.residual &&
                   precision != MF_PREC_F16Q && p->ln_beta, "conv: LayerNorm folding serves plain 1x1 layers without residual (bf16 / bf16x3)");
        lw.resize((size_t)d.cout * d.cin); lb.assign(d.cout, 0.f); lcs.assign(d.cout, 0.f);
        for (int n = 0; n < d.cout; ++n) {
            double sb = bias ? (double)bias[n] : 0.0, cs = 0.0;
            for (int c = 0; c < d.cin; ++c) {
                const float w0 = weight[(size_t)n * d.cin + c];
                sb += (double)w0 * (double)p->ln_beta[c];
                const float wf = w0 * p->ln_gamma[c];
                lw[(size_t)n * d.cin + c] = wf;
                const bf16_t h = mf_f2bf(wf);
                cs += (double)mf_bf2f(h) + (precision == MF_PREC_BF16 ? 0.0 : (double)mf_bf2f(mf_f2bf(wf - mf_bf2f(h))));
            }
            lb[n] = (float)sb; lcs[n] = (float)cs;
        }
        weight = lw.data();
        bias = lb.data();
    }
    p->d = d;
    p->precision = precision;
    p->cin_pad = (d.cin + 7) / 8 * 8;
    const int cpg = p->cin_pad / 8;
    p->phase_taps.clear(); p->phase_oy.clear(); p->phase_ox.clear();

    if (d.upsample) {
        MF_REQUIRE(!d.transposed && d.kh == 3 && d.kw == 3 && d.stride_h == 1 && d.stride_w == 1 && d.pad_h == 1 && d.pad_w == 1,
                   "conv: upsample is built for 3x3 stride-1 pad-1 convolutions");
        // nearest 2x upsampling folded into the gather: output pixel (2i+py, 2j+px) reads input rows
        // i-1..i (py=0) or i..i+1 (py=1); kernel taps that land on the same input pixel are summed, so each of
        // the 4 phases is a 2x2 convolution on the INPUT grid (16 tap-products per input pixel instead of 36)
        p->out_h = 2 * d.in_h; p->out_w = 2 * d.in_w;
        p->Hq = d.in_h; p->Wq = d.in_w; p->out_step = 2; p->in_step_h = p->in_step_w = 1;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                std::vector<ConvPlan::Tap> taps;
                for (int ty = 0; ty < 2; ++ty)
                    for (int tx = 0; tx < 2; ++tx) {
                        ConvPlan::Tap t{py + ty - 1, px + tx - 1, {}};
                        for (int ky = 0; ky < 3; ++ky)
                            for (int kx = 0; kx < 3; ++kx) {
                                // floor((p + k - 1) / 2) for p in {0,1}, k in {0,1,2}
                                const int dy = (py + ky - 1 + 2) / 2 - 1, dx = (px + kx - 1 + 2) / 2 - 1;
                                if (dy == t.dy && dx == t.dx) t.src.push_back({ky, kx});
                            }
                        taps.push_back(t);
                    }
                p->phase_taps.push_back(taps);
                p->phase_oy.push_back(py); p->phase_ox.push_back(px);
            }
        p->in_halo_need = 1;
    } else if (!d.transposed) {
        MF_REQUIRE(d.pad_hi >= 0, "conv: pad_hi must be >= 0");
        p->out_h = (d.in_h + 2 * d.pad_h + d.pad_hi - d.kh) / d.stride_h + 1;     // pad_hi: extra zeros bottom / right only (VAE encoder downsamplers)
        p->out_w = (d.in_w + 2 * d.pad_w + d.pad_hi - d.kw) / d.stride_w + 1;
        MF_REQUIRE(p->out_h > 0 && p->out_w > 0, "conv: empty output");
        p->Hq = p->out_h; p->Wq = p->out_w;
        p->out_step = 1; p->in_step_h = d.stride_h; p->in_step_w = d.stride_w;
        std::vector<ConvPlan::Tap> taps;
        for (int ky = 0; ky < d.kh; ++ky)
            for (int kx = 0; kx < d.kw; ++kx) taps.push_back({ky - d.pad_h, kx - d.pad_w});
        p->phase_taps.push_back(taps);
        p->phase_oy.push_back(0); p->phase_ox.push_back(0);
        // last anchor + largest displacement may run past the input by (pad - slack)
        int need = std::max(d.pad_h, d.pad_w);
        const int over_h = (p->out_h - 1) * d.stride_h + d.kh - 1 - d.pad_h - (d.in_h - 1);
        const int over_w = (p->out_w - 1) * d.stride_w + d.kw - 1 - d.pad_w - (d.in_w - 1);
        need = std::max(need, std::max(over_h, over_w));
        p->in_halo_need = std::max(need, 0);
    } else {
        MF_REQUIRE(d.stride_h == d.stride_w && d.kh == d.kw && d.pad_h == d.pad_w, "convT: square only");
        const int s = d.stride_h, k = d.kh, pad = d.pad_h;
        p->out_h = (d.in_h - 1) * s - 2 * pad + k + d.output_padding;
        p->out_w = (d.in_w - 1) * s - 2 * pad + k + d.output_padding;
        if (s == 1) {
            MF_REQUIRE(d.in_h == 1 && d.in_w == 1 && pad == 0,
                       "convT stride 1 is only built for 1x1 inputs without padding (wav2lip.py:60)");
            // out[oy][ox] = in[0][0] * w[oy][ox]: k*k single-tap phases on a 1x1 quotient grid
            p->Hq = p->Wq = 1; p->out_step = 1; p->in_step_h = p->in_step_w = 1;
            for (int ky = 0; ky < k; ++ky)
                for (int kx = 0; kx < k; ++kx) {
                    p->phase_taps.push_back({{0, 0}});
                    p->phase_oy.push_back(ky); p->phase_ox.push_back(kx);
                }
            p->in_halo_need = 0;
        } else {
            MF_REQUIRE(p->out_h % s == 0 && p->out_w % s == 0, "convT: output %dx%d not a multiple of stride", p->out_h, p->out_w);
            p->Hq = p->out_h / s; p->Wq = p->out_w / s;
            p->out_step = s; p->in_step_h = p->in_step_w = 1;
            int dmin = 0, dmax = 0;
            for (int ry = 0; ry < s; ++ry)
                for (int rx = 0; rx < s; ++rx) {
                    std::vector<ConvPlan::Tap> taps;
                    for (int ky = 0; ky < k; ++ky) {
                        if ((ry + pad - ky) % s != 0) continue;
                        for (int kx = 0; kx < k; ++kx) {
                            if ((rx + pad - kx) % s != 0) continue;
                            const int dy = (ry + pad - ky) / s, dx = (rx + pad - kx) / s;
                            taps.push_back({dy, dx});
                            dmin = std::min(dmin, std::min(dy, dx));
                            dmax = std::max(dmax, std::max(dy, dx));
                        }
                    }
                    MF_REQUIRE(!taps.empty(), "convT: phase without taps is not supported");
                    p->phase_taps.push_back(taps);
                    p->phase_oy.push_back(ry); p->phase_ox.push_back(rx);
                }
            const int over = std::max(p->Hq - 1 + dmax - (d.in_h - 1), p->Wq - 1 + dmax - (d.in_w - 1));
            p->in_halo_need = std::max(std::max(-dmin, over), 0);
        }
    }
    p->nphase = (int)p->phase_taps.size();
    MF_REQUIRE(p->nphase <= MF_MAX_PHASE, "conv: too many phases");
    p->Npad = (d.cout + 15) / 16 * 16;
    if (precision == MF_PREC_F16Q && d.upsample) {
        // nearest-2x upsample + 3x3 in the f16 + FP6 format: four 2 x 2-tap phases (taps pre-summed), [phase][slice][4 taps][Npad][32] in both planes;
        // the only kernel of such a plan is the f16 + FP6 halo tile, one launch per phase (mf_conv_launch)
        MF_REQUIRE(d.cin % 32 == 0 && d.cout % 128 == 0 && !d.residual && d.act <= 2 && d.in_h >= 16 && d.in_w >= 16 && d.cin <= 1024 && d.cout <= 1024,
                   "conv (f16q): upsample + 3x3 needs cin %% 32 == 0, cout %% 128 == 0, a map of at least 16 x 16, no residual");
        std::vector<float> scale1(d.cout, 1.f), fb(p->Npad, 0.f);
        for (int n = 0; n < d.cout; ++n) fb[n] = bias ? bias[n] : 0.f;
        MF_REQUIRE(!bn_gamma, "conv (f16q): no BatchNorm folding for upsample layers");
        p->n_slices = d.cin / 32;
        p->q = true;
        const int64_t per_phase = (int64_t)p->n_slices * 4 * p->Npad * 32, tot = 4 * per_phase;
        std::vector<bf16_t> uh(tot, 0), ul(tot, 0);
        for (int ph = 0; ph < 4; ++ph)
            pack_q_weights(p->n_slices, 4, p->Npad, d.cout, d.cin,
                           [&](int n, int c, int ti) {
                               double w = 0.0;                      // dy = py + ty - 1, dx = px + tx - 1 with ti = 2 * ty + tx: the kernel's tap order
                               for (const auto& kk : p->phase_taps[ph][ti].src) w += weight[(((int64_t)n * d.cin + c) * 3 + kk.first) * 3 + kk.second];
                               return (float)w;
                           }, uh.data() + ph * per_phase, ul.data() + ph * per_phase);
        MF_HIP(hipMalloc(&p->up_hi, tot * sizeof(bf16_t)));
        MF_HIP(hipMemcpy(p->up_hi, uh.data(), tot * sizeof(bf16_t), hipMemcpyHostToDevice));
        MF_HIP(hipMalloc(&p->up_lo, tot * sizeof(bf16_t)));
        MF_HIP(hipMemcpy(p->up_lo, ul.data(), tot * sizeof(bf16_t), hipMemcpyHostToDevice));
        MF_HIP(hipMalloc(&p->bias, p->Npad * sizeof(float)));
        MF_HIP(hipMemcpy(p->bias, fb.data(), p->Npad * sizeof(float), hipMemcpyHostToDevice));
        p->goff_total = 0;
        p->bound_in_ld = p->bound_in_wp = -1;
        return MF_OK;
    }

    // ---- fold BatchNorm (eval mode, eps 1e-5: conv.py:10) into weight scale and bias ---------
    std::vector<float> scale(d.cout, 1.f), fbias(p->Npad, 0.f);
    for (int n = 0; n < d.cout; ++n) {
        const float b0 = bias ? bias[n] : 0.f;
        if (bn_gamma) {
            const double sc = (double)bn_gamma[n] / std::sqrt((double)bn_var[n] + 1e-5);
            scale[n] = (float)sc;
            fbias[n] = (float)(((double)b0 - (double)bn_mean[n]) * sc + (double)bn_beta[n]);
        } else {
            fbias[n] = b0;
        }
    }

    const int HCK = precision != MF_PREC_BF16 ? 32 : 64;   // channel slice of the halo kernel
    const int BK = 64, KG = BK / 8;                            // packed K tile of the implicit-GEMM kernel
    p->BK = BK;
    // up to 256 channels: the register-weights halo kernel (mf_conv_halo.hip) or the LDS-weights one (mf_conv_halo2.hip);
    // wider (<= 1024, cout a multiple of 128, maps >= 64 x 64): only the LDS-weights kernel's fat tiles, with an implicit-GEMM twin
    // (p->alt) for launches too small to fill the chip with 16 x 16-pixel patches.
    const bool narrow = d.cin <= 256 && d.cout <= 256;
    // ... and the UNet's 320-channel layers on its 32 x 32 maps (cout = 2.5 tiles of 128: the third one half empty): at >= 40 frames per step the 16 x 16 x 128
    // tile beats the implicit GEMM there by 14-25 % (320 -> 320: 394 -> 305 us at 64 frames, 960 -> 320: 1054 -> 827) -- the input is read once per channel
    // slice instead of once per tap; smaller steps launch the twin (mf_halo_w_pick_tile).  Whole step, same-box A/B: 112.6 -> 111.8 ms at 64 frames, equal at
    // 48 and below.  On the 16 x 16 maps (640 channels: one patch per image) it does not pay.
    const bool odd_wide = d.cout >= 256 && d.cout % 128 != 0 && d.cout % 64 == 0 && d.in_h * d.in_w >= 32 * 32;
    const bool q_small = p->q_small_maps && precision == MF_PREC_F16Q && d.cin % 32 == 0 && d.cout % 128 == 0 && d.cin <= 2048 && d.cout <= 1024;
    const bool wide_ok = (!g_no_halo_wide && d.cin <= 1024 && d.cout <= 1024 && (d.cout % 128 == 0 || odd_wide) && d.cin % 32 == 0 &&
                         (d.in_h * d.in_w >= 64 * 64 || (d.cout % 256 == 0 && d.cin >= 512) || odd_wide)) ||   // small maps: only the 256-channel tile pays
                         q_small;   // ... and the f16 + FP6 tile where the caller asked for it: 640 -> 640 @16^2 at 64 frames 360 -> 250 us against the bf16x3 implicit GEMM
    p->halo = !d.transposed && d.kh == 3 && d.kw == 3 && d.stride_h == 1 && d.stride_w == 1 && d.pad_h == 1 &&
              d.pad_w == 1 && d.in_h >= 16 && d.in_w >= 16 && d.cin >= 16 && d.residual != 2 && d.act <= 2 && !d.upsample &&
              (narrow || wide_ok) && d.cout % 4 == 0;
    // the f16 + FP6 format's halo tile is 128 channels wide (the UNet's 320-channel 32 x 32 layers run it with a half-empty third tile: odd_wide); other shapes take the implicit GEMM
    if (precision == MF_PREC_F16Q && !(d.cin % 32 == 0 && (d.cout % 128 == 0 || odd_wide))) p->halo = false;
    // thin input (cin <= 16, cout <= 32) on a large map: Wav2Lip's first face-encoder layers (mf_conv_thin.hip).  MF_CONV_THIN=0: the implicit GEMM as before (A/B, tests).
    {
        const char* e = getenv("MF_CONV_THIN");
        p->thin = !d.transposed && !d.upsample && d.kh == d.kw && d.stride_h == d.stride_w && d.pad_h == d.pad_w && d.pad_h == d.kh / 2 && d.pad_hi == 0 &&
                  mf_thin_supported(d.kh, d.stride_h, d.cin, d.cout) && d.residual == 0 && d.act <= 2 && precision != MF_PREC_F16Q &&
                  (int64_t)p->out_h * p->out_w >= 16 * 16 && !(e && e[0] == '0');
    }
    if (p->thin) {
        p->halo = true;                         // (bind, tuning and naming treat it as a kernel that addresses its input itself)
        p->n_slices = 1;
        p->goff_total = 0;
        std::vector<bf16_t> packed;
        mf_thin_pack(weight, scale.data(), d.cout, d.cin, d.kh, precision != MF_PREC_BF16, packed);
        MF_HIP(hipMalloc(&p->w_hi, packed.size() * sizeof(bf16_t)));
        MF_HIP(hipMemcpy(p->w_hi, packed.data(), packed.size() * sizeof(bf16_t), hipMemcpyHostToDevice));
        MF_HIP(hipMalloc(&p->bias, p->Npad * sizeof(float)));
        MF_HIP(hipMemcpy(p->bias, fbias.data(), p->Npad * sizeof(float), hipMemcpyHostToDevice));
        p->bound_in_ld = p->bound_in_wp = -1;
        return MF_OK;
    }
    const bool want_alt = p->halo && !narrow;
    if (p->halo) {
        // ---- pack for the halo-tile kernel: [slice][tap][Npad][CK], channels past cin are zero --------
        p->n_slices = cdiv(d.cin, HCK);
        p->goff_total = 0;
        const int64_t total = (int64_t)p->n_slices * 9 * p->Npad * HCK;
        std::vector<bf16_t> hi(total, 0), lo(total, 0);
        if (precision == MF_PREC_F16Q) {
            // f16 + FP6 residual format (pack_q_weights)
            MF_REQUIRE(d.cin % 32 == 0 && (d.cout % 128 == 0 || odd_wide), "conv (f16q): the format serves 3x3 layers with cin %% 32 == 0 and cout %% 128 == 0 (or 64-multiples >= 256 on maps >= 32 x 32)");
            p->q = true;
            pack_q_weights(p->n_slices, 9, p->Npad, d.cout, d.cin,
                           [&](int n, int c, int tap) { return weight[(((int64_t)n * d.cin + c) * 3 + tap / 3) * 3 + tap % 3] * scale[n]; }, hi.data(), lo.data());
        } else
        for (int c = 0; c < d.cin; ++c)
            for (int tap = 0; tap < 9; ++tap)
                for (int n = 0; n < d.cout; ++n) {
                    const float wf = weight[(((int64_t)n * d.cin + c) * 3 + tap / 3) * 3 + tap % 3] * scale[n];
                    const int64_t idx = (((int64_t)(c / HCK) * 9 + tap) * p->Npad + n) * HCK + c % HCK;
                    const bf16_t h = mf_f2bf(wf);
                    hi[idx] = h;
                    lo[idx] = mf_f2bf(wf - mf_bf2f(h));
                }
        MF_HIP(hipMalloc(&p->w_hi, total * sizeof(bf16_t)));
        MF_HIP(hipMemcpy(p->w_hi, hi.data(), total * sizeof(bf16_t), hipMemcpyHostToDevice));
        if (precision != MF_PREC_BF16) {
            MF_HIP(hipMalloc(&p->w_lo, total * sizeof(bf16_t)));
            MF_HIP(hipMemcpy(p->w_lo, lo.data(), total * sizeof(bf16_t), hipMemcpyHostToDevice));
        }
        MF_HIP(hipMalloc(&p->bias, p->Npad * sizeof(float)));
        MF_HIP(hipMemcpy(p->bias, fbias.data(), p->Npad * sizeof(float), hipMemcpyHostToDevice));
        p->bound_in_ld = p->bound_in_wp = -1;
        if (want_alt && precision != MF_PREC_F16Q) {
            p->alt = new ConvPlan();
            g_no_halo_wide = true;
            const int rc = mf_conv_plan_create(p->alt, d, weight, bias, bn_gamma, bn_beta, bn_mean, bn_var, precision);
            g_no_halo_wide = false;
            if (rc) return rc;
        }
        return MF_OK;
    }
    // ---- pack: per phase [K/64][Npad][64] ---------------------------------------------------------------
    // K order.  Tap-major (all channels of tap 0, then tap 1, ...) re-reads every input pixel once per tap with C/32 K-tiles in
    // between: by then the lines have left L2 (64 workgroups per XCD x 0.5 MB), so a 3x3 layer pulled its input ~9x from HBM / MALL
    // (PMC: 510-627 MB per launch against 153 MB of tensors on the VAE's 512-channel layers).  Channel-slice-major (for each 64-channel
    // slice: its taps back to back) keeps the taps' overlapping rows within nine consecutive K-tiles -- about 50 KB per workgroup.
    auto kgroup = [&](int ntaps, int ti, int cg) { return (cpg % 8 == 0) ? ((cg / 8) * ntaps + ti) * 8 + cg % 8 : ti * cpg + cg; };
    int64_t total = 0;
    int goff_total = 0;
    for (int ph = 0; ph < p->nphase; ++ph) {
        const int ngroups = (int)p->phase_taps[ph].size() * cpg;
        const int KT = cdiv(ngroups, KG);
        p->ph[ph].goff_begin = goff_total;
        p->ph[ph].ngroups = KT * KG;
        p->ph[ph].KT = KT;
        p->ph[ph].w_off = total;
        p->ph[ph].y_off = 0;
        p->ph[ph].ws_off = 0;
        total += (int64_t)KT * p->Npad * BK;
        goff_total += KT * KG;
    }
    p->goff_total = goff_total;
    std::vector<bf16_t> hi(total, 0), lo(total, 0);
    std::vector<float> wq;                      // f16 + FP6 format: the fp32 weights in packed order, encoded block by block below
    if (precision == MF_PREC_F16Q) {
        // implicit-GEMM layers in the f16 + FP6 format: a 64-deep K tile must be 64 consecutive channels of one tap (two FP6 blocks), and the narrow
        // special tiles (N <= 32) have no kernel in it
        MF_REQUIRE(d.cin % 64 == 0 && d.cout > 32, "conv (f16q): implicit-GEMM layers need cin %% 64 == 0 and cout > 32 (got %d -> %d)", d.cin, d.cout);
        p->q = true;
        wq.assign(total, 0.f);
    }
    const int k = d.kh;  // (transposed: square)
    for (int ph = 0; ph < p->nphase; ++ph) {
        auto& taps = p->phase_taps[ph];
        for (size_t ti = 0; ti < taps.size(); ++ti) {
            if (taps[ti].src.empty()) {   // the kernel tap this gather tap stands for
                int ky, kx;
                if (!d.transposed) {
                    ky = taps[ti].dy + d.pad_h; kx = taps[ti].dx + d.pad_w;
                } else if (d.stride_h == 1) {
                    ky = p->phase_oy[ph]; kx = p->phase_ox[ph];
                } else {
                    ky = p->phase_oy[ph] + d.pad_h - taps[ti].dy * d.stride_h;
                    kx = p->phase_ox[ph] + d.pad_w - taps[ti].dx * d.stride_w;
                }
                taps[ti].src.push_back({ky, kx});
            }
            for (int n = 0; n < d.cout; ++n)
                for (int c = 0; c < d.cin; ++c) {
                    double w = 0.0;
                    for (const auto& kk : taps[ti].src)
                        w += d.transposed ? weight[(((int64_t)c * d.cout + n) * k + kk.first) * k + kk.second]
                                          : weight[(((int64_t)n * d.cin + c) * d.kh + kk.first) * d.kw + kk.second];
                    const float wf = (float)(w * (double)scale[n]);
                    const int g = kgroup((int)taps.size(), (int)ti, c / 8);
                    const int64_t idx = p->ph[ph].w_off + ((int64_t)(g / KG) * p->Npad + n) * BK + (g % KG) * 8 + c % 8;
                    if (p->q) { wq[idx] = wf; continue; }
                    const bf16_t h = mf_f2bf(wf);
                    hi[idx] = h;
                    lo[idx] = mf_f2bf(wf - mf_bf2f(h));
                }
        }
    }
    if (p->q)
        for (int64_t r = 0; r < total; r += 32) pack_q_block(&wq[r], &hi[r], &lo[r]);
    MF_HIP(hipMalloc(&p->w_hi, total * sizeof(bf16_t)));
    MF_HIP(hipMemcpy(p->w_hi, hi.data(), total * sizeof(bf16_t), hipMemcpyHostToDevice));
    if (precision != MF_PREC_BF16) {
        MF_HIP(hipMalloc(&p->w_lo, total * sizeof(bf16_t)));
        MF_HIP(hipMemcpy(p->w_lo, lo.data(), total * sizeof(bf16_t), hipMemcpyHostToDevice));
    }
    MF_HIP(hipMalloc(&p->bias, p->Npad * sizeof(float)));
    MF_HIP(hipMemcpy(p->bias, fbias.data(), p->Npad * sizeof(float), hipMemcpyHostToDevice));
    if (!lcs.empty()) {
        MF_REQUIRE(!p->halo && p->nphase == 1, "conv: LayerNorm folding needs the implicit-GEMM path");
        lcs.resize(p->Npad, 0.f);
        MF_HIP(hipMalloc(&p->ln_cs, p->Npad * sizeof(float)));
        MF_HIP(hipMemcpy(p->ln_cs, lcs.data(), p->Npad * sizeof(float), hipMemcpyHostToDevice));
    }
    p->ln_gamma = p->ln_beta = nullptr;            // (host pointers of the builder: not kept)
    MF_HIP(hipMalloc(&p->goff, goff_total * sizeof(int)));
    p->bound_in_ld = p->bound_in_wp = -1;
    return MF_OK;
}

void mf_conv_plan_destroy(ConvPlan* p) {
    if (!p) return;
    if (p->alt) { mf_conv_plan_destroy(p->alt); delete p->alt; p->alt = nullptr; }
    if (p->w_hi) (void)hipFree(p->w_hi);
    if (p->w_lo) (void)hipFree(p->w_lo);
    if (p->bias) (void)hipFree(p->bias);
    if (p->ln_cs) (void)hipFree(p->ln_cs);
    p->ln_cs = nullptr;
    if (p->goff) (void)hipFree(p->goff);
    if (p->ws) (void)hipFree(p->ws);
    if (p->up_hi) (void)hipFree(p->up_hi);
    if (p->up_lo) (void)hipFree(p->up_lo);
    for (void* r : p->retired) (void)hipFree(r);
    p->retired.clear();
    p->up_hi = p->up_lo = nullptr;
    p->w_hi = p->w_lo = nullptr; p->bias = nullptr; p->goff = nullptr; p->ws = nullptr; p->ws_cap = 0;
}

int mf_conv_bind(ConvPlan* p, const ActBuf& in) {
    // (a plan with the GroupNorm fused into its halo load reads the GroupNorm's INPUT: pixels outside the map are masked by coordinate, no zero ring needed)
    MF_REQUIRE(in.halo >= p->in_halo_need, "conv: input halo %d < required %d", in.halo, p->in_halo_need);
    MF_REQUIRE(in.H == p->d.in_h && in.W == p->d.in_w, "conv: plan built for %dx%d input, bound to %dx%d",
               p->d.in_h, p->d.in_w, in.H, in.W);
    MF_REQUIRE(in.C % 8 == 0 && in.C >= p->cin_pad, "conv: input buffer has %d channels, need >= %d (multiple of 8)", in.C, p->cin_pad);
    if (p->bound_in_ld == in.C && p->bound_in_wp == in.Wp()) return MF_OK;
    if (p->halo || (p->q && p->up_hi)) {        // halo-tile kernels address the input themselves: nothing to precompute
        p->bound_in_ld = in.C; p->bound_in_wp = in.Wp();
        return p->alt ? mf_conv_bind(p->alt, in) : MF_OK;
    }
    const int cpg = p->cin_pad / 8;
    std::vector<int> goff(p->goff_total, 0);
    for (int ph = 0; ph < p->nphase; ++ph) {
        const auto& taps = p->phase_taps[ph];
        const int real = (int)taps.size() * cpg;
        for (int g = 0; g < p->ph[ph].ngroups; ++g) {
            const int gg = g < real ? g : 0;   // padding groups re-read group 0 against zero weights
            int ti = gg / cpg, cg = gg % cpg;
            if (cpg % 8 == 0) {                                // inverse of kgroup() in mf_conv_plan_create
                const int nt = (int)taps.size(), s8 = gg / (nt * 8), rem = gg % (nt * 8);
                ti = rem / 8; cg = s8 * 8 + rem % 8;
            }
            goff[p->ph[ph].goff_begin + g] =
                ((taps[ti].dy + in.halo) * in.Wp() + (taps[ti].dx + in.halo)) * in.C + cg * 8;
        }
    }
    MF_HIP(hipMemcpy(p->goff, goff.data(), goff.size() * sizeof(int), hipMemcpyHostToDevice));
    p->bound_in_ld = in.C; p->bound_in_wp = in.Wp();
    return MF_OK;
}

// Channel-slice split of the fat 256-channel halo tile for a wide layer whose map gives too few patches at this batch (0 = no split).
static int mf_halo_split_count(const ConvPlan* p, int batch) {
    if (!p->halo || !p->alt || p->d.cout % 256 || p->d.cin < 512) return 0;
    const int base = batch * cdiv(p->out_h, 16) * cdiv(p->out_w, 16) * (p->d.cout / 256);
    if (base < 64) return 0;          // (at 32 patches x tiles the split measured +5 % / -2 % on two shapes: not worth the second pass)
    for (int cand : {2, 4, 8})
        if (base * cand >= 256 && p->n_slices / cand >= 2) return cand;
    return 0;
}

// Channel-slice split of the f16 + FP6 tile (16 x 16 pixels x 128 channels) for a layer with fewer tiles than CUs at this batch (1 = no split)
int mf_q_split_count(const ConvPlan* p, int batch) {
    if (!p->q || !p->halo) return 1;
    const int base = batch * cdiv(p->out_h, 16) * cdiv(p->out_w, 16) * (p->d.cout / 128);
    if (base >= 256) return 1;
    int best = 1;
    for (int cand : {2, 4, 8}) {
        if (p->n_slices / cand < 2) break;
        best = cand;
        if (base * cand >= 256) break;
    }
    return best;
}

bool mf_conv_tuned_valid(const ConvTuned& c, int precision, int act) {
    static const int tiles[][4] = {{64, 64, 2, 2}, {128, 64, 2, 2}, {128, 128, 2, 2}, {256, 128, 4, 2}, {256, 256, 2, 4}, {128, 80, 4, 1}};
    bool tile_ok = false;
    for (const auto& t : tiles) tile_ok |= c.tile.bm == t[0] && c.tile.bn == t[1] && c.tile.wgm == t[2] && c.tile.wgn == t[3];
    const char* why = nullptr;
    if (!tile_ok) why = "tile not compiled";
    else if (c.tile.nsplit < 1 || c.tile.nsplit > 16) why = "split outside 1 .. 16";
    else if (!(c.ld == -1 || c.ld == 0 || c.ld == 2 || c.ld == 3 || c.ld == 4)) why = "no such operand path";
    else if ((c.ld == 3 || c.ld == 4) && c.tile.wgm * c.tile.wgn != 4) why = "the producer-wave path (ld 3 / 4) needs a 4-wave tile";
    else if (c.tile.bn == 80 && c.ld != 3 && c.ld != 4) why = "the 128 x 80 tile runs on the producer-wave kernels (ld 3 / 4) only";
    // the producer-wave kernels exist in bf16x3 only (launch_prec / launch_pw_only): in bf16 such an entry would fail at launch
    else if ((c.ld == 3 || c.ld == 4 || c.tile.bn == 80) && precision != MF_PREC_BF16X3) why = "the producer-wave kernels (ld 3 / 4, the 128 x 80 tile) are bf16x3 only";
    // the GEGLU epilogue pairs a wave's value and gate fragments: the 80-channel tile's five fragments per wave do not pair (mf_tile80_ok)
    else if (c.tile.bn == 80 && act == 5) why = "the 128 x 80 tile cannot pair GEGLU value / gate fragments";
    if (why) mf_set_error("conv: configuration %dx%d (%d x %d waves) split %d ld %d: %s", c.tile.bm, c.tile.bn, c.tile.wgm, c.tile.wgn, c.tile.nsplit, c.ld, why);
    return !why;
}

int mf_conv_resolve(const ConvPlan* p, int batch, int tokens, int stats_groups, ConvLaunchCfg* c) {
    *c = ConvLaunchCfg{MF_CONV_FAMILY_IGEMM, ConvTile{0, 0, 0, 0, 1}, -1, 0, p->nphase, MF_CONV_STATS_NONE, false};
    const int groups = stats_groups > 0 ? stats_groups : 0;
    // split-K / channel-split combines that leave the statistics (launch_combine_stats)
    const bool combine_stats = groups && p->d.act != 5 && p->d.cout % 4 == 0 && p->d.cout % groups == 0 && groups <= 64;
    const int halo_ck = p->precision != MF_PREC_BF16 ? 32 : 64;
    auto stats = [&](int src) { c->stats = groups ? src : MF_CONV_STATS_NONE; return MF_OK; };
    if (p->thin) {
        c->family = MF_CONV_FAMILY_THIN; c->tile = ConvTile{p->out_h, p->d.cout, 1, 1, 1}; c->bk = p->d.cin <= 8 ? 8 : 16;
        return stats(MF_CONV_STATS_PASS);
    }
    const bool q_gn = groups && p->d.cout % groups == 0 && (p->d.cout / groups == 4 || p->d.cout / groups == 8 || p->d.cout / groups == 16);
    if (p->halo) {
        c->bk = halo_ck;
        if (p->q) {
            const int ns = mf_q_split_count(p, batch);
            c->family = MF_CONV_FAMILY_F16Q; c->tile = ConvTile{16, 128, 4, 2, ns};
            return stats(ns > 1 ? (combine_stats ? MF_CONV_STATS_COMBINE : MF_CONV_STATS_PASS) : q_gn ? MF_CONV_STATS_EPILOGUE : MF_CONV_STATS_PASS);
        }
        const HaloTile tw = mf_halo_w_pick_tile(p->out_h, p->out_w, p->d.cout, batch, p->d.cin);
        if (tw.ph) {
            c->family = MF_CONV_FAMILY_HALO_W; c->tile = ConvTile{tw.ph, tw.bn, tw.wgm, tw.wgn, 1};
            return stats(MF_CONV_STATS_PASS);
        }
        if (const int ns = mf_halo_split_count(p, batch)) {
            c->family = MF_CONV_FAMILY_HALO_W_SPLIT; c->tile = ConvTile{16, 256, 2, 4, ns};
            return stats(combine_stats ? MF_CONV_STATS_COMBINE : MF_CONV_STATS_PASS);
        }
        if (p->alt) {
            const int rc = mf_conv_resolve(p->alt, batch, 0, stats_groups, c);
            c->family = MF_CONV_FAMILY_TWIN;
            return rc;
        }
        const HaloTile t = mf_halo_pick_tile(p->out_h, p->out_w, p->d.cout, batch, p->d.cin);
        c->family = MF_CONV_FAMILY_HALO; c->tile = ConvTile{t.ph, t.bn, t.wgm, t.wgn, 1};
        return stats(MF_CONV_STATS_PASS);
    }
    if (p->up_hi && p->q) {
        c->family = MF_CONV_FAMILY_F16Q; c->tile = ConvTile{16, 128, 4, 2, 1}; c->bk = 32; c->nphase = 4;
        return stats(q_gn ? MF_CONV_STATS_EPILOGUE : MF_CONV_STATS_PASS);
    }
    // ---- implicit GEMM
    const bool x3 = p->precision != MF_PREC_BF16;
    ConvTile tc = mf_conv_pick_tile(p, batch);
    int ld = -1;
    {
        static const bool forced = getenv("MF_FORCE_TILE") || getenv("MF_FORCE_SPLIT") || getenv("MF_FORCE_LD");
        auto it = p->tuned.find(batch);
        if (it != p->tuned.end()) { ld = it->second.ld; c->pinned = !forced; }
        static const int force_ld = [] { const char* e = getenv("MF_FORCE_LD"); return e ? atoi(e) : -1; }();   // (measurement, with MF_FORCE_TILE / MF_FORCE_SPLIT)
        if (force_ld >= 0 && !(force_ld >= 3 && (!x3 || p->q || tc.wgm * tc.wgn != 4 || tc.bn < 64 || tc.bm < 64))) ld = force_ld;
    }
    const int Wq_eff = tokens > 0 ? tokens : p->Wq;
    const int M = batch * p->Hq * Wq_eff;
    if (tokens > 0) {
        // the cost model priced the full sequence: re-balance the split for the rows actually computed
        const int nt = cdiv(M, tc.bm) * cdiv(p->d.cout, tc.bn);
        int kt_min = p->ph[0].KT;
        tc.nsplit = nt >= 256 ? 1 : std::max(1, std::min(std::min(kt_min, cdiv(512, nt)), 16));
        if (tc.bm > 128 && M <= 256) { tc.bm = 64; tc.bn = 64; tc.wgm = 2; tc.wgn = 2; }
        if (p->d.act == 5 && tc.bn < 32) tc.nsplit = 1;
    }
    // the split-K partials ([split][B][Ho][Wo][N], unpadded rows) are written and combined in float4 channel quads: with a cout that is not a multiple
    // of 4 the last quad of a row would overwrite the next pixel's first channels (and run past the workspace at the last one), and the combine would
    // drop the row's last channels.  Such a layer takes the single-pass epilogue.
    if (p->d.cout % 4) tc.nsplit = 1;
    c->tile = tc;
    // the operand path and stage depth launch_prec / launch_cfg / launch_pw_only take for this (tile, ld)
    const bool four = tc.wgm * tc.wgn == 4;
    const bool pw = ld == 3 || ld == 4;
    MF_REQUIRE(!pw || (x3 && !p->q && four && tc.bm >= 64 && tc.bn >= 64), "conv: no producer-wave kernel (ld %d) for tile %dx%d in this precision", ld, tc.bm, tc.bn);
    MF_REQUIRE(tc.bn != 80 || pw, "conv: the %dx%d tile has only the bf16x3 producer-wave kernels (ld 3 / 4)", tc.bm, tc.bn);
    c->ld = pw ? ld : (four && (ld >= 0 ? ld : 2) == 2) ? 2 : 0;
    c->bk = p->q ? (four ? 64 : 32) : pw ? (ld == 3 ? 64 : 32) : x3 ? (four ? 64 : 32) : 64;
    if (groups && tokens == 0) {
        if (tc.nsplit > 1) return stats(combine_stats ? MF_CONV_STATS_COMBINE : MF_CONV_STATS_PASS);
        // in the epilogue: 4-wave tiles (k_conv_igemm's ST) whose pixel tile lies inside one sample
        if (p->d.act != 5 && p->d.cout % groups == 0 && groups <= 64 && four && tc.bm * tc.bn < 128 * 128 && (p->Hq * Wq_eff) % tc.bm == 0)
            return stats(MF_CONV_STATS_EPILOGUE);
    }
    return stats(MF_CONV_STATS_PASS);
}

static int conv_launch_impl(ConvPlan* p, const ActView& in, const ActView& out, const ActView& res, int batch, hipStream_t stream, int tokens, bool* stats_done);

// split-K combine that also leaves the consumer GroupNorm's statistics (k_splitk_epilogue_stats); false = not applicable, run the plain combine
static bool launch_combine_stats(const ConvPlan* p, ConvArgs e, int nsplit, int Ho, int Wo, int batch, hipStream_t stream) {
    if (!p->out_stats || p->d.act == 5 || p->d.cout % 4 || p->d.cout % p->out_stats_groups || p->out_stats_groups > 64) return false;
    e.gn_out = p->out_stats; e.gn_out_groups = p->out_stats_groups; e.gn_out_cpg = p->d.cout / p->out_stats_groups;
    const int nq = p->d.cout / 4, cols = std::min(256, nq), ppi = 256 / cols, T = Ho * Wo;
    const int target = 1024;                                         // workgroups aimed for (each issues 2 * groups fp64 atomics): 128 / 256 and 2048 / 4096 all measured slower
    const int P = std::max(ppi, std::min(64 * ppi, (int)(((int64_t)T * batch + target - 1) / target)));
    hipLaunchKernelGGL(k_splitk_epilogue_stats, dim3((unsigned)((T + P - 1) / P), batch), dim3(256), 0, stream, e, nsplit, Ho, Wo, P, epi_div(e, Ho, Wo));
    return true;
}

// ConvPlan::out_stats (set by the network builder when the layer's consumer is a GroupNorm of exactly this output): every launch leaves the
// (sum, sum of squares) per (sample, group) of the stored values ADDED to out_stats -- from the kernel's epilogue or the split-K combine where
// the chosen configuration can, else from a k_gn_stats pass behind the conv.  The consumer then skips its own statistics pass.
int mf_conv_launch(ConvPlan* p, const ActView& in, const ActView& out, const ActView& res,
                   int batch, hipStream_t stream, int tokens) {
    bool stats_done = false;
    int rc = conv_launch_impl(p, in, out, res, batch, stream, tokens, &stats_done);
    if (!rc && p->out_stats && !stats_done) rc = mf_groupnorm_stats(out, p->out_stats_groups, p->out_stats, batch, stream);
    // MF_DEBUG=copies (development, eager launches only: it synchronises): for a batch of IDENTICAL items, reports every layer whose input, output or statistics of
    // an item differ from item 0's -- a row's result may not depend on where its image sits in the batch (tools/unet_copies_probe.py)
    static const bool copies = mf_debug_has("copies");
    if (copies && !rc && batch > 1) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(stream, &cs);
        if (cs == hipStreamCaptureStatusNone) {
            MF_HIP(hipStreamSynchronize(stream));
            auto differ = [&](const ActView& v, int* first) -> double {
                const ActBuf& b = *v.buf;
                const size_t n = (size_t)b.per_batch();
                std::vector<bf16_t> h0(n), hk(n), l0(b.lo ? n : 0), lk(b.lo ? n : 0);
                (void)hipMemcpy(h0.data(), b.hi, n * sizeof(bf16_t), hipMemcpyDeviceToHost);
                if (b.lo) (void)hipMemcpy(l0.data(), b.lo, n * sizeof(bf16_t), hipMemcpyDeviceToHost);
                double worst = 0.0;
                for (int k = 1; k < batch; ++k) {
                    (void)hipMemcpy(hk.data(), b.hi + (size_t)k * n, n * sizeof(bf16_t), hipMemcpyDeviceToHost);
                    if (b.lo) (void)hipMemcpy(lk.data(), b.lo + (size_t)k * n, n * sizeof(bf16_t), hipMemcpyDeviceToHost);
                    double w = 0.0;
                    size_t cnt = 0, first_i = 0, last_i = 0;
                    int cmin = 1 << 30, cmax = -1;
                    for (size_t i = 0; i < n; ++i) {
                        const int c = (int)(i % b.C);
                        if (c < v.coff || c >= v.coff + v.C) continue;
                        const double a0 = (double)mf_bf2f(h0[i]) + (b.lo ? (double)mf_bf2f(l0[i]) : 0.0), ak = (double)mf_bf2f(hk[i]) + (b.lo ? (double)mf_bf2f(lk[i]) : 0.0);
                        const double e = std::fabs(a0 - ak);
                        if (e > 1e-3) { if (!cnt) first_i = i; last_i = i; ++cnt; cmin = std::min(cmin, c); cmax = std::max(cmax, c); }
                        w = std::max(w, e);
                    }
                    if (cnt && w > worst)
                        fprintf(stderr, "[MF_DEBUG=copies]   item %d: %zu elements off by > 1e-3, padded pixels %zu .. %zu (row pitch %d px), channels %d .. %d\n", k, cnt, first_i / b.C,
                                last_i / b.C, b.Wp(), cmin, cmax);
                    if (w > worst) { worst = w; *first = k; }
                }
                return worst;
            };
            int ki = 0, ko = 0;
            const double di = differ(in, &ki), dout = differ(out, &ko);
            // the per-token LayerNorm statistics this layer reads / leaves ([item][token][2] doubles)
            auto stats_differ = [&](const double* dev, int tokens_per_item, int* first) -> double {
                if (!dev) return 0.0;
                std::vector<double> h((size_t)batch * tokens_per_item * 2);
                (void)hipMemcpy(h.data(), dev, h.size() * sizeof(double), hipMemcpyDeviceToHost);
                double worst = 0.0;
                for (int k = 1; k < batch; ++k)
                    for (int i = 0; i < tokens_per_item * 2; ++i) {
                        const double w = std::fabs(h[(size_t)k * tokens_per_item * 2 + i] - h[i]);
                        if (w > worst) { worst = w; *first = k; }
                    }
                return worst;
            };
            int ksi = 0, kso = 0;
            const double dsi = stats_differ(p->ln_in, in.buf->H * in.buf->W, &ksi), dso = stats_differ(p->ln_out, out.buf->H * out.buf->W, &kso);
            if (dsi > 0.0 || dso > 0.0) fprintf(stderr, "[MF_DEBUG=copies] LayerNorm statistics: read differ by %.3e (item %d), left differ by %.3e (item %d)\n", dsi, ksi, dso, kso);
            // MF_DEBUG_DUMP=<prefix>: the first layer whose copies disagree although its inputs agree leaves both items' outputs, its LayerNorm statistics, column sums and
            // bias as raw files (<prefix>_meta.txt, _y0.f32, _yk.f32, _stats.f64, _cs.f32, _bias.f32) for offline analysis (tools/pkfma_dump_analyze.py)
            static bool dumped = false;
            const char* dump = getenv("MF_DEBUG_DUMP");
            if (dump && !dumped && di == 0.0 && dout > 0.0) {
                dumped = true;
                const ActBuf& b = *out.buf;
                const size_t n = (size_t)b.per_batch();
                auto plane = [&](int item, std::vector<float>& f) {
                    std::vector<bf16_t> h(n), l(b.lo ? n : 0);
                    (void)hipMemcpy(h.data(), b.hi + (size_t)item * n, n * sizeof(bf16_t), hipMemcpyDeviceToHost);
                    if (b.lo) (void)hipMemcpy(l.data(), b.lo + (size_t)item * n, n * sizeof(bf16_t), hipMemcpyDeviceToHost);
                    f.resize(n);
                    for (size_t i = 0; i < n; ++i) f[i] = mf_bf2f(h[i]) + (b.lo ? mf_bf2f(l[i]) : 0.f);
                };
                auto put = [&](const char* suffix, const void* data, size_t bytes) {
                    const std::string path = std::string(dump) + suffix;
                    if (FILE* f = fopen(path.c_str(), "wb")) { fwrite(data, 1, bytes, f); fclose(f); }
                };
                std::vector<float> y0, yk;
                plane(0, y0); plane(ko, yk);
                put("_y0.f32", y0.data(), n * 4); put("_yk.f32", yk.data(), n * 4);
                const int tok = in.buf->H * in.buf->W;
                if (p->ln_in) {
                    std::vector<double> st((size_t)tok * 2);
                    (void)hipMemcpy(st.data(), p->ln_in, st.size() * 8, hipMemcpyDeviceToHost);
                    put("_stats.f64", st.data(), st.size() * 8);
                    std::vector<float> cs(p->Npad);
                    (void)hipMemcpy(cs.data(), p->ln_cs, cs.size() * 4, hipMemcpyDeviceToHost);
                    put("_cs.f32", cs.data(), cs.size() * 4);
                }
                std::vector<float> bias(p->Npad);
                (void)hipMemcpy(bias.data(), p->bias, bias.size() * 4, hipMemcpyDeviceToHost);
                put("_bias.f32", bias.data(), bias.size() * 4);
                char kn2[96], meta[512];
                mf_conv_kernel_name(p, batch, kn2, sizeof(kn2));
                snprintf(meta, sizeof(meta), "C %d\nWp %d\nH %d\nW %d\nhalo %d\ncoff %d\nvC %d\ncin %d\ncout %d\nNpad %d\nitem %d\ntokens %d\nln_eps %g\nact %d\nkernel %s\n", b.C, b.Wp(), b.H, b.W,
                         b.halo, out.coff, out.C, p->d.cin, p->d.cout, p->Npad, ko, tok, (double)p->ln_eps, p->d.act, kn2);
                put("_meta.txt", meta, strlen(meta));
            }
            if (di > 0.0 || dout > 0.0) {
                char kn[96];
                mf_conv_kernel_name(p, batch, kn, sizeof(kn));
                fprintf(stderr, "[MF_DEBUG=copies] %d->%d k%d @%dx%d act %d%s%s: input differs by %.3e (item %d), output by %.3e (item %d)  %s\n", p->d.cin, p->d.cout, p->d.kh, p->d.in_h,
                        p->d.in_w, p->d.act, p->ln_in ? " ln_in" : "", p->ln_out ? " ln_out" : "", di, ki, dout, ko, kn);
            }
        }
    }
    return rc;
}

static int conv_launch_impl(ConvPlan* p, const ActView& in, const ActView& out, const ActView& res,
                            int batch, hipStream_t stream, int tokens, bool* stats_done) {
    const ActBuf& ib = *in.buf;
    const ActBuf& ob = *out.buf;
    MF_REQUIRE(tokens >= 0 && (tokens == 0 || (!p->halo && !p->up_hi && p->Hq == 1 && p->nphase == 1 && p->out_step == 1 && tokens <= p->Wq)),
               "conv: a token prefix (%d) needs a single-row sequence layer on the implicit-GEMM path with at least that many positions", tokens);
    const int Wq_eff = tokens > 0 ? tokens : p->Wq;       // output positions per batch item this launch computes
    const int out_w_eff = tokens > 0 ? tokens : p->out_w;
    MF_REQUIRE(p->bound_in_ld == ib.C && p->bound_in_wp == ib.Wp(), "conv: plan not bound to this input geometry");
    MF_REQUIRE(in.C >= p->cin_pad && in.coff % 8 == 0 && in.coff + in.C <= ib.C, "conv: bad input view");
    // the epilogue stores channel quads: a cout that is not a multiple of 4 spills zero-weight channels
    // into the next (up to 3) channels of the buffer, which must exist
    MF_REQUIRE(out.C == (p->d.act == 5 ? p->d.cout / 2 : p->d.cout) && out.coff % 4 == 0 && out.coff + (out.C + 3) / 4 * 4 <= ob.C, "conv: bad output view");
    MF_REQUIRE(ob.H == p->out_h && ob.W == p->out_w, "conv: output buffer %dx%d != %dx%d", ob.H, ob.W, p->out_h, p->out_w);
    const bool x3 = p->precision != MF_PREC_BF16;                      // two planes per tensor (bf16x3, and the f16 + FP6 format)
    MF_REQUIRE(!x3 || (ib.lo && ob.lo), "conv: BF16X3 needs lo planes");
    MF_REQUIRE(p->precision != MF_PREC_F16Q || p->q, "conv (f16q): the plan was not packed in this format");
    ConvLaunchCfg cfg;
    if (const int rc = mf_conv_resolve(p, batch, tokens, p->out_stats ? p->out_stats_groups : 0, &cfg)) return rc;

    if (cfg.family == MF_CONV_FAMILY_THIN) {
        MF_REQUIRE(!res.buf && ib.halo >= p->d.pad_h, "thin conv: no residual, and the input buffer's zero ring must cover the padding");
        ThinArgs ta{};
        ta.x_hi = ib.hi + in.coff; ta.x_lo = x3 ? ib.lo + in.coff : nullptr;
        ta.w = p->w_hi; ta.bias = p->bias;
        ta.batch = batch; ta.H = p->out_h; ta.W = p->out_w; ta.N = p->d.cout;
        ta.pad = p->d.pad_h; ta.in_halo = ib.halo; ta.in_hp = ib.Hp(); ta.in_wp = ib.Wp(); ta.x_ld = ib.C; ta.xb = ib.per_batch();
        const int64_t yb0 = ((int64_t)ob.halo * ob.Wp() + ob.halo) * ob.C + out.coff;
        ta.y_hi = ob.hi + yb0; ta.y_lo = x3 ? ob.lo + yb0 : nullptr;
        ta.yb = ob.per_batch(); ta.yi = ob.Wp() * ob.C; ta.yj = ob.C;
        ta.act = p->d.act;
        return mf_thin_launch(ta, p->d.kh, p->d.stride_h, p->d.cin, p->d.cout, x3, stream);
    }
    if (p->halo) {
        HaloArgs ha{};
        ha.q = p->q ? 1 : 0;
        ha.x_hi = ib.hi + in.coff; ha.x_lo = x3 ? ib.lo + in.coff : nullptr;
        ha.w_hi = p->w_hi; ha.w_lo = p->w_lo; ha.bias = p->bias;
        ha.batch = batch; ha.H = p->out_h; ha.W = p->out_w; ha.N = p->d.cout; ha.Npad = p->Npad; ha.n_slices = p->n_slices;
        ha.in_halo = ib.halo; ha.in_hp = ib.Hp(); ha.in_wp = ib.Wp(); ha.x_ld = ib.C; ha.xb = ib.per_batch();
        const int64_t yb0 = ((int64_t)ob.halo * ob.Wp() + ob.halo) * ob.C + out.coff;
        ha.y_hi = ob.hi + yb0; ha.y_lo = x3 ? ob.lo + yb0 : nullptr;
        ha.yb = ob.per_batch(); ha.yi = ob.Wp() * ob.C; ha.yj = ob.C;
        if (res.buf) {
            const ActBuf& rb = *res.buf;
            MF_REQUIRE(rb.H == p->out_h && rb.W == p->out_w && res.C == p->d.cout, "conv: residual view does not match the output");
            if (res.buf == in.buf && res.coff == in.coff && p->d.cin == p->d.cout) {
                ha.res_from_halo = 1;   // the residual is the input itself (conv.py:17-18): read it from LDS
            } else {
                const int64_t rb0 = ((int64_t)rb.halo * rb.Wp() + rb.halo) * rb.C + res.coff;
                ha.r_hi = rb.hi + rb0; ha.r_lo = x3 ? rb.lo + rb0 : nullptr;
                ha.rb = rb.per_batch(); ha.ri = rb.Wp() * rb.C; ha.rj = rb.C;
            }
        }
        ha.act = p->d.act;
        if (cfg.family == MF_CONV_FAMILY_F16Q) {   // the f16 + FP6 format has one kernel: the 8-wave 16 x 16 x 128-channel tile
            MF_REQUIRE(!ha.res_from_halo, "conv (f16q): residual-from-input is not built for this format");
            if (cfg.stats == MF_CONV_STATS_EPILOGUE) {   // (other group widths: k_gn_stats behind the conv)
                ha.gn_out = p->out_stats; ha.gn_out_cpg = p->d.cout / p->out_stats_groups; ha.gn_out_groups = p->out_stats_groups;
                *stats_done = true;
            }
            ha.wide_store = out.coff % 8 == 0 && ob.C % 8 == 0 && p->d.cout % 32 == 0;   // 16-byte epilogue stores (lane pairs exchange halves)
            const HaloTile qtile{16, 128, 4, 2};
            // A map too small to give every CU a 16 x 16 patch (the VAE's 512-channel 32 x 32 levels at batch 8: 32 patches x 4 channel tiles): the
            // channel slices split over blockIdx.y, fp32 partial tiles combined by k_splitk_epilogue[_stats] -- as the bf16x3 256-channel tile does.
            const int ns = cfg.tile.nsplit;
            if (ns > 1) {
                const int64_t per_split = (int64_t)batch * p->out_h * p->out_w * p->d.cout;
                const int64_t need = per_split * ns;
                if (need > p->ws_cap) {
                    // (eager launches only; the outgrown buffer is retired, not freed: graphs captured at other batch sizes still hold its address)
                    if (p->ws) { p->retired.push_back(p->ws); p->ws = nullptr; p->ws_cap = 0; }
                    MF_HIP(hipMalloc(&p->ws, need * sizeof(float)));
                    p->ws_cap = need;
                }
                HaloArgs hs = ha;
                hs.ws = p->ws; hs.ws_split = per_split; hs.nsplit = ns;
                hs.gn_out = nullptr;
                *stats_done = false;
                int rc = mf_halo_w_launch(hs, qtile, true, stream);
                if (rc) return rc;
                ConvArgs e{};
                e.ws = p->ws; e.ws_split = per_split; e.bias = p->bias; e.N = p->d.cout; e.act = p->d.act;
                e.y_hi = ha.y_hi; e.y_lo = ha.y_lo; e.yb = ha.yb; e.yi = ha.yi; e.yj = ha.yj;
                e.r_hi = ha.r_hi; e.r_lo = ha.r_lo; e.rb = ha.rb; e.ri = ha.ri; e.rj = ha.rj;
                const int64_t total = (int64_t)batch * p->out_h * p->out_w * (p->d.cout / 4);
                MF_REQUIRE(total < 0x7fffffffll, "conv: split-K combine over %lld channel quads (32-bit thread index)", (long long)total);
                if (launch_combine_stats(p, e, ns, p->out_h, p->out_w, batch, stream)) *stats_done = true;
                else hipLaunchKernelGGL(k_splitk_epilogue, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, e, ns, p->out_h, p->out_w, (int)total, epi_div(e, p->out_h, p->out_w));
                MF_HIP(hipGetLastError());
                return MF_OK;
            }
            return mf_halo_w_launch(ha, qtile, true, stream);
        }
        if (cfg.family == MF_CONV_FAMILY_HALO_W) return mf_halo_w_launch(ha, HaloTile{cfg.tile.bm, cfg.tile.bn, cfg.tile.wgm, cfg.tile.wgn}, x3, stream);
        // Wide layer on a map too small to give every CU a 16 x 16 patch (the VAE's 512-channel 32 x 32 levels at batch 8: 64 patches x
        // channel tiles): the 256-channel tile with the channel slices split over blockIdx.y, fp32 partials combined by
        // k_splitk_epilogue -- the same two-pass scheme as the implicit GEMM's split-K, with half its L2 -> LDS bytes.  MF_HALO_SPLIT=0: off.
        {
            const int ns = cfg.tile.nsplit;
            if (cfg.family == MF_CONV_FAMILY_HALO_W_SPLIT) {
                const int64_t per_split = (int64_t)batch * p->out_h * p->out_w * p->d.cout;
                const int64_t need = per_split * ns;
                if (need > p->ws_cap) {
                    // only reached on an eager (un-captured) launch: the first forward at a batch size runs eagerly.  The outgrown
                    // buffer is retired, not freed: graphs captured at other batch sizes still hold its address.
                    if (p->ws) { p->retired.push_back(p->ws); p->ws = nullptr; p->ws_cap = 0; }
                    MF_HIP(hipMalloc(&p->ws, need * sizeof(float)));
                    p->ws_cap = need;
                }
                HaloArgs hs = ha;
                hs.ws = p->ws; hs.ws_split = per_split; hs.nsplit = ns;
                hs.res_from_halo = 0;
                int rc = mf_halo_w_launch(hs, HaloTile{16, 256, 2, 4}, x3, stream);
                if (rc) return rc;
                ConvArgs e{};
                e.ws = p->ws; e.ws_split = per_split; e.bias = p->bias; e.N = p->d.cout; e.act = p->d.act;
                e.y_hi = ha.y_hi; e.y_lo = ha.y_lo; e.yb = ha.yb; e.yi = ha.yi; e.yj = ha.yj;
                if (res.buf) {
                    const ActBuf& rb = *res.buf;
                    const int64_t rb0 = ((int64_t)rb.halo * rb.Wp() + rb.halo) * rb.C + res.coff;
                    e.r_hi = rb.hi + rb0; e.r_lo = x3 ? rb.lo + rb0 : nullptr;
                    e.rb = rb.per_batch(); e.ri = rb.Wp() * rb.C; e.rj = rb.C;
                }
                const int64_t total = (int64_t)batch * p->out_h * p->out_w * (p->d.cout / 4);
                MF_REQUIRE(total < 0x7fffffffll, "conv: split-K combine over %lld channel quads (32-bit thread index)", (long long)total);
                if (launch_combine_stats(p, e, ns, p->out_h, p->out_w, batch, stream)) *stats_done = true;
                else hipLaunchKernelGGL(k_splitk_epilogue, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, e, ns, p->out_h, p->out_w, (int)total, epi_div(e, p->out_h, p->out_w));
                MF_HIP(hipGetLastError());
                return MF_OK;
            }
        }
        if (cfg.family == MF_CONV_FAMILY_TWIN) {   // wide layer, too few patches for the fat tiles at this batch: implicit GEMM
            p->alt->prof_mid = p->prof_mid;
            p->alt->out_stats = p->out_stats; p->alt->out_stats_groups = p->out_stats_groups;
            const int rc = conv_launch_impl(p->alt, in, out, res, batch, stream, 0, stats_done);
            p->alt->prof_mid = nullptr;
            return rc;
        }
        return mf_halo_launch(ha, HaloTile{cfg.tile.bm, cfg.tile.bn, cfg.tile.wgm, cfg.tile.wgn}, x3, stream);
    }

    if (cfg.family == MF_CONV_FAMILY_F16Q) {
        // upsample + 3x3 in the f16 + FP6 format: four launches of the 16 x 16 x 128-channel tile, phase (py, px) writes output pixels (2i + py, 2j + px)
        MF_REQUIRE(ib.halo >= 1 && !res.buf, "conv (f16q): upsample path needs an input halo and no residual");
        HaloArgs ha{};
        ha.q = 1;
        ha.x_hi = ib.hi + in.coff; ha.x_lo = ib.lo + in.coff;
        ha.bias = p->bias;
        ha.batch = batch; ha.H = p->d.in_h; ha.W = p->d.in_w; ha.N = p->d.cout; ha.Npad = p->Npad; ha.n_slices = p->n_slices;
        ha.in_halo = ib.halo; ha.in_hp = ib.Hp(); ha.in_wp = ib.Wp(); ha.x_ld = ib.C; ha.xb = ib.per_batch();
        ha.yb = ob.per_batch(); ha.yi = 2 * ob.Wp() * ob.C; ha.yj = 2 * ob.C;
        ha.act = p->d.act;
        ha.wide_store = out.coff % 8 == 0 && ob.C % 8 == 0 && p->d.cout % 32 == 0;
        if (cfg.stats == MF_CONV_STATS_EPILOGUE) {
            ha.gn_out = p->out_stats; ha.gn_out_cpg = p->d.cout / p->out_stats_groups; ha.gn_out_groups = p->out_stats_groups;    // every phase adds its quarter of the pixels
            *stats_done = true;
        }
        const int64_t per_phase = (int64_t)p->n_slices * 4 * p->Npad * 32;
        for (int ph = 0; ph < 4; ++ph) {
            const int64_t yb0 = ((int64_t)(ob.halo + (ph >> 1)) * ob.Wp() + ob.halo + (ph & 1)) * ob.C + out.coff;
            ha.y_hi = ob.hi + yb0; ha.y_lo = ob.lo + yb0;
            ha.w_hi = p->up_hi + ph * per_phase; ha.w_lo = p->up_lo + ph * per_phase;
            const int rc = mf_halo_w_launch(ha, HaloTile{16, 128, 4, 2}, true, stream, ph);
            if (rc) return rc;
        }
        return MF_OK;
    }
    ConvArgs a{};
    a.x_hi = ib.hi + in.coff; a.x_lo = x3 ? ib.lo + in.coff : nullptr;
    a.w_hi = p->w_hi; a.w_lo = p->w_lo; a.bias = p->bias; a.goff = p->goff;
    a.M = batch * p->Hq * Wq_eff; a.N = p->d.cout; a.Npad = p->Npad;
    a.HqWq = p->Hq * Wq_eff; a.Wq = Wq_eff;
    mf_fastdiv((uint32_t)a.HqWq, &a.dv_hw_mul, &a.dv_hw_shr); mf_fastdiv((uint32_t)a.Wq, &a.dv_w_mul, &a.dv_w_shr);
    a.xb = ib.per_batch(); a.xi = p->in_step_h * ib.Wp() * ib.C; a.xj = p->in_step_w * ib.C;
    const int64_t ybase = ((int64_t)ob.halo * ob.Wp() + ob.halo) * ob.C + out.coff;
    a.y_hi = ob.hi + ybase; a.y_lo = x3 ? ob.lo + ybase : nullptr;
    a.yb = ob.per_batch(); a.yi = p->out_step * ob.Wp() * ob.C; a.yj = p->out_step * ob.C;
    if (res.buf) {
        const ActBuf& rb = *res.buf;
        MF_REQUIRE(rb.H == p->out_h && rb.W == p->out_w && res.C == p->d.cout && p->out_step == 1,
                   "conv: residual view does not match the output");
        const int64_t rbase = ((int64_t)rb.halo * rb.Wp() + rb.halo) * rb.C + res.coff;
        a.r_hi = rb.hi + rbase; a.r_lo = x3 ? rb.lo + rbase : nullptr;
        a.rb = rb.per_batch(); a.ri = rb.Wp() * rb.C; a.rj = rb.C;
    }
    a.act = p->d.act;
    a.res_after_act = p->d.residual == 2;
    if (p->ln_cs) {
        MF_REQUIRE(p->ln_in && !res.buf && (p->d.act == 0 || p->d.act == 5), "conv: a LayerNorm-folded layer needs its statistics buffer, no residual and act 0 or GEGLU");
        a.ln_in = p->ln_in; a.ln_cs = p->ln_cs; a.ln_inv_c = 1.f / (float)p->d.cin; a.ln_eps = p->ln_eps;
    }
    if (p->ln_out) {
        MF_REQUIRE(p->d.act != 5 && p->nphase == 1 && p->out_step == 1, "conv: LayerNorm statistics come from plain 1x1 producers");
        a.ln_out = p->ln_out;
    }
    {
        const int n_out = p->d.act == 5 ? p->d.cout / 2 : p->d.cout;
        a.wide_store = out.coff % 8 == 0 && ob.C % 8 == 0 && n_out % 8 == 0 && p->d.cout % 16 == 0;
    }
    a.goff_total = p->goff_total;
    int goff_max = 0;
    for (int ph = 0; ph < p->nphase; ++ph) {
        a.ph[ph] = p->ph[ph];
        a.ph[ph].y_off = ((int64_t)p->phase_oy[ph] * ob.Wp() + p->phase_ox[ph]) * ob.C;
        a.ph[ph].ws_off = ((int64_t)p->phase_oy[ph] * p->out_w + p->phase_ox[ph]) * a.N;
        goff_max = std::max(goff_max, p->ph[ph].ngroups);
    }

    const ConvTile tc = cfg.tile;            // tile, split and operand path as mf_conv_resolve settled them
    a.ld = cfg.ld;
    a.tiles_m = cdiv(a.M, tc.bm); a.tiles_n = cdiv(a.N, tc.bn);
    {
        // XCD tile order by which operand is heavier: weights N x K vs the input tensor M x Cin (both x planes)
        const int64_t w_elems = (int64_t)a.Npad * p->ph[0].KT * 64 * p->nphase;
        const int64_t x_elems = (int64_t)batch * ib.H * ib.W * in.C;
        a.m_fastest = w_elems > x_elems;
        static const bool dbg_times = mf_debug_has("times");
        if (dbg_times) {
            static unsigned long long* dbg_buf = nullptr;
            if (!dbg_buf) MF_HIP(hipMalloc(&dbg_buf, (size_t)4 * 65536 * sizeof(unsigned long long)));
            a.dbg = (int64_t)a.tiles_m * a.tiles_n * tc.nsplit * p->nphase <= 65536 ? dbg_buf : nullptr;
        }
    }
    if (tc.nsplit > 1) {
        // fp32 partial tiles [split][B][Ho][Wo][N]; combined by k_splitk_epilogue below
        const int64_t per_split = (int64_t)batch * p->out_h * out_w_eff * a.N;
        const int64_t need = per_split * tc.nsplit;
        if (need > p->ws_cap) {
            // only reached on an eager (un-captured) launch: the first forward at a batch size runs eagerly.  The outgrown buffer is
            // retired, not freed: graphs captured at other batch sizes still hold its address (ConvPlan::retired).
            if (p->ws) { p->retired.push_back(p->ws); p->ws = nullptr; p->ws_cap = 0; }
            MF_HIP(hipMalloc(&p->ws, need * sizeof(float)));
            p->ws_cap = need;
        }
        a.ws = p->ws; a.ws_split = per_split;
        a.wsb = (int64_t)p->out_h * out_w_eff * a.N;
        a.wsi = p->out_step * out_w_eff * a.N; a.wsj = p->out_step * a.N;
    }
    if (p->out_stats && p->d.act != 5 && p->d.cout % p->out_stats_groups == 0 && p->out_stats_groups <= 64 && tokens == 0) {
        a.gn_out_cpg = p->d.cout / p->out_stats_groups; a.gn_out_groups = p->out_stats_groups;
        // in the epilogue (mf_conv_resolve: 4-wave tiles whose pixel tile lies inside one sample); split-K layers: in the combine pass below
        if (cfg.stats == MF_CONV_STATS_EPILOGUE) { a.gn_out = p->out_stats; *stats_done = true; }
    }
    int rc = MF_ERR_INVALID;
#define MF_CASE(BM, BN, WGM, WGN)                                                          \
    if (tc.bm == BM && tc.bn == BN) rc = launch_prec<BM, BN, WGM, WGN>(a, p->nphase, tc.nsplit, goff_max, x3, p->q, stream);
    MF_CASE(128, 16, 4, 1)
    MF_CASE(128, 32, 4, 1)
    MF_CASE(16, 64, 1, 4)
    MF_CASE(256, 256, 2, 4)
    MF_CASE(256, 128, 4, 2)
    MF_CASE(128, 128, 2, 2)
    MF_CASE(128, 64, 2, 2)
    MF_CASE(64, 64, 2, 2)
#undef MF_CASE
    if (tc.bm == 128 && tc.bn == 80) rc = launch_pw_only<128, 80, 4, 1>(a, p->nphase, tc.nsplit, goff_max, x3, p->q, stream);
    if (rc != MF_OK) {
        if (rc == MF_ERR_INVALID) mf_set_error("conv: no kernel for tile %dx%d", tc.bm, tc.bn);
        return rc;
    }
    if (a.dbg) {
        static int reports = 0;
        if (++reports > 3 && reports <= 5) {   // skip the warm-up launches
            MF_HIP(hipStreamSynchronize(stream));
            const size_t nwg = (size_t)a.tiles_m * a.tiles_n * tc.nsplit * p->nphase;
            std::vector<unsigned long long> t(4 * nwg);
            MF_HIP(hipMemcpy(t.data(), a.dbg, t.size() * sizeof(t[0]), hipMemcpyDeviceToHost));
            unsigned long long lo = ~0ull, hi = 0;
            std::vector<double> d[3], start, end;
            for (size_t w = 0; w < nwg; ++w) {
                lo = std::min(lo, t[4 * w]); hi = std::max(hi, t[4 * w + 3]);
                for (int k = 0; k < 3; ++k) d[k].push_back((double)(t[4 * w + k + 1] - t[4 * w + k]));
            }
            for (size_t w = 0; w < nwg; ++w) { start.push_back((double)(t[4 * w] - lo)); end.push_back((double)(t[4 * w + 3] - lo)); }
            auto med = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
            auto mx = [](const std::vector<double>& v) { return *std::max_element(v.begin(), v.end()); };
            fprintf(stderr, "[MF_DEBUG=times] %zu WGs tile %dx%d split %d: span %llu ticks; prologue med %.0f max %.0f; loop med %.0f max %.0f; "
                            "epilogue med %.0f max %.0f; WG start med %.0f max %.0f; WG end med %.0f\n",
                    nwg, tc.bm, tc.bn, tc.nsplit, hi - lo, med(d[0]), mx(d[0]), med(d[1]), mx(d[1]), med(d[2]), mx(d[2]), med(start), mx(start), med(end));
        }
    }
    if (tc.nsplit > 1 && p->prof_mid) MF_HIP(hipEventRecord(p->prof_mid, stream));
    if (tc.nsplit > 1) {
        ConvArgs e = a;   // unit-grid strides for the combine pass
        e.yi = ob.Wp() * ob.C; e.yj = ob.C;
        const int64_t total = (int64_t)batch * p->out_h * out_w_eff * ((a.act == 5 ? a.N / 2 : a.N) / 4);
        MF_REQUIRE(total < 0x7fffffffll, "conv: split-K combine over %lld channel quads (32-bit thread index)", (long long)total);
        if (tokens == 0 && launch_combine_stats(p, e, tc.nsplit, p->out_h, out_w_eff, batch, stream)) *stats_done = true;
        else hipLaunchKernelGGL(k_splitk_epilogue, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, e,
                                tc.nsplit, p->out_h, out_w_eff, (int)total, epi_div(e, p->out_h, out_w_eff));
        MF_HIP(hipGetLastError());
    }
    return MF_OK;
}

int mf_gemm_grouped_launch(ConvPlan* p, const GroupedGemm& g, hipStream_t stream) {
    MF_REQUIRE(!p->halo && p->nphase == 1 && p->bound_in_ld > 0, "grouped gemm: plan must be a bound mf_gemm_plan_create shell");
    const bool x3 = p->precision == MF_PREC_BF16X3;
    ConvArgs a{};
    a.x_hi = g.x_hi; a.x_lo = x3 ? g.x_lo : nullptr;
    a.w_hi = p->w_hi; a.w_lo = p->w_lo; a.bias = p->bias; a.goff = p->goff;
    a.M = g.M; a.N = p->d.cout; a.Npad = p->Npad;
    a.HqWq = g.M; a.Wq = g.M;          // rows are linear: (b, i, j) = (0, 0, m)
    mf_fastdiv((uint32_t)a.HqWq, &a.dv_hw_mul, &a.dv_hw_shr); mf_fastdiv((uint32_t)a.Wq, &a.dv_w_mul, &a.dv_w_shr);
    a.xb = 0; a.xi = 0; a.xj = g.x_row;
    a.y_hi = g.y_hi; a.y_lo = x3 ? g.y_lo : nullptr;
    a.yb = 0; a.yi = 0; a.yj = g.y_row;
    a.act = 0;
    a.ld = -1;
    a.goff_total = p->goff_total;
    a.ph[0] = p->ph[0];
    a.zgroups = g.groups; a.zheads = g.heads;
    a.zx_b = g.zx_b; a.zx_h = g.zx_h; a.zy_b = g.zy_b; a.zy_h = g.zy_h;
    a.zw = (int64_t)p->ph[0].KT * p->Npad * 64;
    const int M = g.M, N = a.N;
    int rc = MF_ERR_INVALID;
#define MF_GCASE(BM, BN, WGM, WGN)                                                         \
    { a.tiles_m = cdiv(M, BM); a.tiles_n = cdiv(N, BN);                                    \
      rc = launch_prec<BM, BN, WGM, WGN>(a, 1, 1, p->ph[0].ngroups, x3, false, stream); }
    if (N <= 16) MF_GCASE(128, 16, 4, 1)
    else if (N <= 32) MF_GCASE(128, 32, 4, 1)
    else if (M <= 16) MF_GCASE(16, 64, 1, 4)
    else if (cdiv(M, 128) * cdiv(N, 128) * g.groups >= 512 && N % 128 == 0) MF_GCASE(128, 128, 2, 2)
    else if (cdiv(M, 128) * cdiv(N, 64) * g.groups >= 512) MF_GCASE(128, 64, 2, 2)
    else MF_GCASE(64, 64, 2, 2)
#undef MF_GCASE
    return rc;
}

// Tile / split-K selection by a cost model of the loop (profiles/r01_igemm_bandwidth_study.md): a workgroup streams
// (BM + BN) x K/S operand elements at min(per-CU DMA rate, chip L2->LDS rate / resident workgroups); workgroups run in
// rounds of (256 CUs x resident per CU); a split pays the fp32 partial round trip and one more launch.  Constants were
// fitted to 386 measured (shape, tile, split) points of the MuseTalk UNet / VAE layers (mean loss vs the best measured
// configuration 3.5 %).
// layers the 128 x 80 producer-wave tile can run: bf16x3, channel count a multiple of 80, no GEGLU pairing (its 5 channel fragments do not pair)
static bool mf_tile80_ok(const ConvPlan* p) { return p->precision == MF_PREC_BF16X3 && !p->q && p->d.act != 5 && p->d.cout % 80 == 0; }

ConvTile mf_conv_pick_tile(const ConvPlan* p, int batch) {
    {
        static const bool forced = getenv("MF_FORCE_TILE") || getenv("MF_FORCE_SPLIT") || getenv("MF_FORCE_LD");
        auto it = p->tuned.find(batch);
        if (!forced && it != p->tuned.end()) return it->second.tile;
    }
    const int M = batch * p->Hq * p->Wq, N = p->d.cout;
    int kt_min = p->ph[0].KT;
    double kt_sum = 0;
    for (int ph = 0; ph < p->nphase; ++ph) { kt_min = std::min(kt_min, p->ph[ph].KT); kt_sum += p->ph[ph].KT; }
    ConvTile t;
    if (N <= 16) t = {128, 16, 4, 1, 1};
    else if (N <= 32) t = {128, 32, 4, 1, 1};
    else if (M <= 16 && p->d.act != 5 && !p->q) t = {16, 64, 1, 4, 1};   // (its 16-channel wave tile cannot pair GEGLU blocks; no f16 + FP6 form)
    else t = {64, 64, 2, 2, 1};
    const bool modelled = N > 32 && (M > 16 || p->d.act == 5 || p->q);
    // exploration knobs (tools/unet_shape_sweep.py): MF_FORCE_TILE=128x64, MF_FORCE_SPLIT=4
    static const int force_tile = [] { const char* e = getenv("MF_FORCE_TILE"); int a = 0, b = 0; return e && sscanf(e, "%dx%d", &a, &b) == 2 ? a * 1000 + b : 0; }();
    static const int force_split = [] { const char* e = getenv("MF_FORCE_SPLIT"); return e ? atoi(e) : 0; }();
    struct Cand { int bm, bn, wgm, wgn, resident; };
    static const Cand cands[] = {{64, 64, 2, 2, 2}, {128, 64, 2, 2, 2}, {128, 128, 2, 2, 2}, {256, 128, 4, 2, 1}, {256, 256, 2, 4, 1}, {128, 80, 4, 1, 1}};
    static const int splits[] = {1, 2, 3, 4, 6, 8, 12, 16};
    if (modelled) {
        const double planes = p->precision != MF_PREC_BF16 ? 2.0 : 1.0;
        const double Kavg = kt_sum / p->nphase * 64.0;
        const double PW = 46e9, CHIP = 10.5e12, EPI_BW = 2.5e12, EPI_FIX = 6e-6, WG_FIX = 2e-6;
        const int fs = force_split ? std::max(1, std::min(std::min(kt_min, force_split), 16)) : 0;
        double best = 1e30;
        for (const Cand& c : cands) {
            if (force_tile && (c.bm != force_tile / 1000 || c.bn != force_tile % 1000)) continue;
            if (c.bn == 80 && (force_tile != 128080 || !mf_tile80_ok(p))) continue;   // measured only (mf_conv_tune), never the model's pick
            if (c.bn == 128 && c.bm == 128 && N % 128) continue;
            for (int si = 0; si < (fs ? 1 : (int)(sizeof(splits) / sizeof(splits[0]))); ++si) {
                const int S = fs ? fs : splits[si];
                if (S > kt_min) continue;
                if (c.bm == 256 && Kavg / S < 512 && !force_tile) continue;    // too few K tiles to amortise a 256-wide prologue / epilogue
                const double wg = (double)cdiv(M, c.bm) * cdiv(N, c.bn) * p->nphase * S;
                const double slots = 256.0 * c.resident;
                const double rate = std::min(PW, CHIP / std::min(wg, slots));
                const double bytes_wg = (double)(c.bm + c.bn) * (Kavg / S) * 2.0 * planes;
                double cost = std::ceil(wg / slots) * (bytes_wg / rate + WG_FIX);
                if (S > 1) cost += S * (double)M * N * p->nphase * 4.0 * 2.0 / EPI_BW + EPI_FIX;
                if (cost < best) { best = cost; t = {c.bm, c.bn, c.wgm, c.wgn, S}; }
            }
        }
        return t;
    }
    const int nt = cdiv(M, t.bm) * cdiv(N, t.bn) * p->nphase;
    if (nt < 256 && kt_min >= 2) t.nsplit = std::max(1, std::min(std::min(kt_min, cdiv(512, nt)), 16));
    if (force_split) t.nsplit = std::max(1, std::min(std::min(kt_min, force_split), 16));
    return t;
}

namespace {
// reads a buffer (pulls it into the Infinity Cache the way the producing layer leaves it there)
__global__ __launch_bounds__(256) void k_tune_touch(const uint4* __restrict__ p, int64_t n, unsigned* sink) {
    unsigned acc = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) { const uint4 v = p[i]; acc += v.x ^ v.y ^ v.z ^ v.w; }
    if (acc == 0x9e3779b9u) *sink = acc;
}
}  // namespace

namespace {
// Measured configurations by layer signature: layers of one shape share a measurement (the UNet's 188 GEMMs are ~60 distinct shapes).
// Where they come from, in this order:
//   MF_TUNE_CACHE=<file>   read at first use; every new measurement (mf_*_tune) is appended to it
//   <library dir>/tune/gfx950.txt   the table shipped with the library for the BASELINE.json shapes (tools/make_tune_cache.py on an MI355X): with it a
//                          process launches the same configurations -- hence the same fp32 summation order, the same output bits -- on every box
// A forward NEVER measures (tuning inside run() stalled a serving loop for seconds at every new session count): it only looks its
// layers up here; a shape that is not in the table runs the cost model's pick.  Measuring is an explicit call (mf_unet_tune, mf_vae_tune,
// mf_wav2lip_tune, mf_net_tune), or, for development, MF_AUTOTUNE=1 (measure on the first forward at a batch size, as rounds 1-2 did).
// bm == 0 records "the cost model's pick stays".
std::string shipped_tune_table() {
    Dl_info info{};
    if (!dladdr(reinterpret_cast<const void*>(&mf_conv_tune), &info) || !info.dli_fname) return "";
    std::string path = info.dli_fname;
    const size_t slash = path.rfind('/');
    return (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/tune/gfx950.txt";
}
std::map<std::string, ConvTuned>& tune_cache() {
    static std::map<std::string, ConvTuned> cache;
    static bool loaded = false;
    if (!loaded) {
        loaded = true;
        const char* env = getenv("MF_TUNE_CACHE");
        const std::string path = env ? std::string(env) : shipped_tune_table();
        // Entries are validated on load: a stale or hand-edited file must not put a tile the library no longer compiles, an impossible split or an
        // operand path that was removed into launch selection.  Keys carry the kernel generation ("g950k4": tile list / operand paths of round 4's library).
        // KEEP IN SYNC with loader_rejects() in tests/test_tune_table.py, which holds the shipped table to these rules.
        auto valid = [](const std::string& k, const ConvTuned& c) {
            if (k.rfind("g950k4:", 0) != 0) return false;
            if (c.tile.bm == 0) return true;                                          // "the cost model's pick stays"
            // a compiled tile, a split of 1 .. 16, an operand path that exists and that the tile runs -- in the key's precision (the producer-wave kernels,
            // hence ld 3 / 4 and the 128 x 80 tile, are bf16x3 only) and with the key's activation (no 128 x 80 GEGLU).  ld 3 / 4 (round 5's producer-wave path) are additions to generation k4: every older
            // entry still names a kernel this library has
            int f[14] = {0};   // precision, batch, cin, cout, kh, kw, stride_h, stride_w, pad_h, pad_w, transposed, output_padding, residual, act
            if (sscanf(k.c_str() + 7, "%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d", f, f + 1, f + 2, f + 3, f + 4, f + 5, f + 6, f + 7, f + 8, f + 9, f + 10, f + 11,
                       f + 12, f + 13) != 14) return false;
            return mf_conv_tuned_valid(c, f[0], f[13]);
        };
        int dropped = 0;
        if (FILE* f = path.empty() ? nullptr : fopen(path.c_str(), "r")) {
            char key[256];
            ConvTuned c{};
            while (fscanf(f, "%255s %d %d %d %d %d %d", key, &c.tile.bm, &c.tile.bn, &c.tile.wgm, &c.tile.wgn, &c.tile.nsplit, &c.ld) == 7) {
                if (valid(key, c)) cache[key] = c; else ++dropped;
            }
            fclose(f);
            if (dropped) fprintf(stderr, "[mere-fusion_amd] tuning table %s: %d entries ignored (other kernel generation or invalid configuration)\n", path.c_str(), dropped);
        } else {
            // said once: without a table every layer runs the cost model's pick, and frames are no longer bit-identical from box to box
            fprintf(stderr, "[mere-fusion_amd] no tuning table (%s): implicit-GEMM layers use the cost model's launch configurations\n", path.empty() ? "library path unknown" : path.c_str());
        }
    }
    return cache;
}
void tune_cache_store(const std::string& key, const ConvTuned& c) {
    tune_cache()[key] = c;
    if (const char* path = getenv("MF_TUNE_CACHE")) {
        if (FILE* f = fopen(path, "a")) {
            fprintf(f, "%s %d %d %d %d %d %d\n", key.c_str(), c.tile.bm, c.tile.bn, c.tile.wgm, c.tile.wgn, c.tile.nsplit, c.ld);
            fclose(f);
        }
    }
}
bool tunable_layer(const ConvPlan* p, int batch) {
    static const bool forced = getenv("MF_FORCE_TILE") || getenv("MF_FORCE_SPLIT") || getenv("MF_FORCE_LD");
    if (p->halo || p->up_hi || forced) return false;                                 // halo-kernel layers keep their own tile choice
    const int M = batch * p->Hq * p->Wq, N = p->d.cout;
    return !(N <= 32 || (M <= 16 && p->d.act != 5 && !p->q));                         // the narrow special tiles have no alternatives
}
ConvTuned split_clamped(const ConvPlan* p, ConvTuned c) {
    int kt_min = p->ph[0].KT;
    for (int ph = 0; ph < p->nphase; ++ph) kt_min = std::min(kt_min, p->ph[ph].KT);
    c.tile.nsplit = std::max(1, std::min(c.tile.nsplit, kt_min));                     // (a split deeper than the layer's K tiles cannot launch)
    return c;
}
std::string tune_key(const ConvPlan* p, const ActView& in, int batch) {
    char keybuf[256];
    snprintf(keybuf, sizeof(keybuf), "g950k4:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d", p->precision, batch, p->d.cin, p->d.cout, p->d.kh, p->d.kw, p->d.stride_h, p->d.stride_w,
             p->d.pad_h, p->d.pad_w, p->d.transposed, p->d.output_padding, p->d.residual, p->d.act, p->d.in_h, p->d.in_w, p->d.upsample, p->d.pad_hi,
             in.buf ? in.buf->C : 0);
    return std::string(keybuf) + (p->out_stats ? ":s" : "");     // a layer that also leaves GroupNorm statistics times (and may pick) differently
}
}  // namespace

bool mf_autotune_enabled() {
    const char* e = getenv("MF_AUTOTUNE");         // (read at every use: tests switch it per case)
    return e && atoi(e) != 0;
}

int mf_conv_tune_lookup(ConvPlan* p, const ActView& in, int batch) {
    if (p->halo && p->alt && !p->q) {
        // a wide halo layer at a batch too small for the fat tiles launches its implicit-GEMM twin: the twin takes the table entry of the layer's signature
        // (same descriptor; the ':s' suffix follows the statistics request the launch will hand over)
        p->alt->out_stats = p->out_stats; p->alt->out_stats_groups = p->out_stats_groups;
        return mf_conv_tune_lookup(p->alt, in, batch);
    }
    if (!tunable_layer(p, batch)) return 0;
    auto it = tune_cache().find(tune_key(p, in, batch));
    if (it == tune_cache().end()) return 0;
    if (it->second.tile.bm > 0) p->tuned[batch] = split_clamped(p, it->second);
    else p->tuned.erase(batch);
    return 1;
}

int mf_conv_pin(ConvPlan* p, int batch, const ConvTuned& c) {
    if (p->halo && p->alt && !p->q) return mf_conv_pin(p->alt, batch, c);          // (as mf_conv_tune_lookup: the wide halo layer's twin takes the entry)
    if (c.tile.bm == 0) { p->tuned.erase(batch); return MF_OK; }
    MF_REQUIRE(!p->halo && !p->up_hi, "conv: this layer runs on a halo-tile or thin kernel: the tuning table does not serve it");
    MF_REQUIRE(tunable_layer(p, batch), "conv: at batch %d this layer runs a narrow special tile (cout <= 32, or <= 16 pixels; or MF_FORCE_* is set): "
               "the tuning table does not serve it", batch);
    if (!mf_conv_tuned_valid(c, p->precision, p->d.act)) return MF_ERR_INVALID;
    p->tuned[batch] = split_clamped(p, c);
    return MF_OK;
}

int mf_conv_tune(ConvPlan* p, const ActView& in, const ActView& out, const ActView& res, int batch, hipStream_t stream) {
    if (p->halo && p->alt && !p->q) {             // (as mf_conv_tune_lookup: the twin is what launches when the fat tiles decline this batch)
        if (mf_halo_w_pick_tile(p->out_h, p->out_w, p->d.cout, batch, p->d.cin).ph || mf_halo_split_count(p, batch)) return MF_OK;
        p->alt->out_stats = p->out_stats; p->alt->out_stats_groups = p->out_stats_groups;
        return mf_conv_tune(p->alt, in, out, res, batch, stream);
    }
    if (!tunable_layer(p, batch)) return MF_OK;
    const std::string key = tune_key(p, in, batch);
    // MF_TUNE_EXTEND=80 (table maintenance): a layer that HAS an entry is measured again, its entry against the tiles of that channel width only (a tile added
    // to the library after the table was made), and the entry is replaced where the new tile is clearly ahead -- minutes instead of the full hour of measurements
    static const int extend_bn = [] { const char* e = getenv("MF_TUNE_EXTEND"); return e ? atoi(e) : 0; }();
    const bool found = mf_conv_tune_lookup(p, in, batch);                             // measured before (this process, MF_TUNE_CACHE, or the shipped table)
    static std::set<std::string> extended;                                            // (layers of one signature share the measurement)
    const bool extend = found && extend_bn == 80 && mf_tile80_ok(p) && extended.insert(key).second;
    if (found && !extend) return MF_OK;
    const bool had_entry = p->tuned.count(batch) != 0;
    const ConvTuned entry = had_entry ? p->tuned[batch] : ConvTuned{ConvTile{0, 0, 0, 0, 0}, -1};
    if (!extend) p->tuned.erase(batch);
    const int M = batch * p->Hq * p->Wq, N = p->d.cout;
    const ConvTile base = mf_conv_pick_tile(p, batch);                                // what the cost model would launch
    int kt_min = p->ph[0].KT;
    for (int ph = 0; ph < p->nphase; ++ph) kt_min = std::min(kt_min, p->ph[ph].KT);
    struct Cand { int bm, bn, wgm, wgn; };
    static const Cand tiles[] = {{64, 64, 2, 2}, {128, 64, 2, 2}, {128, 128, 2, 2}, {256, 128, 4, 2}, {256, 256, 2, 4}, {128, 80, 4, 1}};
    static const int splits[] = {1, 2, 3, 4, 6, 8, 12, 16};
    hipEvent_t e0, e1;
    MF_HIP(hipEventCreate(&e0)); MF_HIP(hipEventCreate(&e1));
    // In the network a layer finds its INPUT in the Infinity Cache (the previous layer just wrote it) and its WEIGHTS in HBM (3.4 GB of them
    // cycle through per step); timed back to back it would find both warm.  So before every timed launch a 384 MB
    // memset evicts the caches and a read pass brings the input (and residual) planes back.
    const bool cold = true;
    static void* scratch = nullptr;
    static unsigned* sink = nullptr;
    const size_t scratch_bytes = (size_t)384 << 20;
    if (cold && !scratch) { MF_HIP(hipMalloc(&scratch, scratch_bytes)); MF_HIP(hipMalloc(&sink, 4)); }
    auto prepare = [&]() -> int {
        if (!cold) return MF_OK;
        MF_HIP(hipMemsetAsync(scratch, 1, scratch_bytes, stream));
        for (const ActView* v : {&in, &res}) {
            if (!v->buf) continue;
            const int64_t n16 = (int64_t)batch * v->buf->per_batch() * (int64_t)sizeof(bf16_t) / 16;
            hipLaunchKernelGGL(k_tune_touch, dim3(1024), dim3(256), 0, stream, reinterpret_cast<const uint4*>(v->buf->hi), n16, sink);
            if (v->buf->lo) hipLaunchKernelGGL(k_tune_touch, dim3(1024), dim3(256), 0, stream, reinterpret_cast<const uint4*>(v->buf->lo), n16, sink);
        }
        MF_HIP(hipGetLastError());
        return MF_OK;
    };
    auto measure = [&](const ConvTuned& c, float* us) -> int {
        p->tuned[batch] = c;
        int rc = mf_conv_launch(p, in, out, res, batch, stream);                     // warm-up: also sizes the split-K workspace
        if (rc) return rc;
        float best = 1e30f;
        for (int i = 0; i < 3; ++i) {
            if ((rc = prepare())) return rc;
            MF_HIP(hipEventRecord(e0, stream));
            if ((rc = mf_conv_launch(p, in, out, res, batch, stream))) return rc;
            MF_HIP(hipEventRecord(e1, stream));
            MF_HIP(hipEventSynchronize(e1));
            float ms = 0.f;
            MF_HIP(hipEventElapsedTime(&ms, e0, e1));
            best = std::min(best, ms * 1e3f);
        }
        *us = best;
        return MF_OK;
    };
    ConvTuned best_c{base, extend && had_entry ? entry.ld : -1};
    float base_us = 0.f;
    int rc = measure(best_c, &base_us);
    float best_us = base_us;
    for (const Cand& t : tiles) {
        if (rc) break;
        if (t.bn == 128 && t.bm == 128 && N % 128) continue;
        if (t.bn == 80 && !mf_tile80_ok(p)) continue;
        if (extend && t.bn != extend_bn) continue;
        if (t.bm >= 256 && M < 256) continue;
        const int64_t nt = (int64_t)cdiv(M, t.bm) * cdiv(N, t.bn) * p->nphase;
        for (int S : splits) {
            if (S > kt_min || (S > 1 && nt >= 1024) || nt * S > 4096) continue;
            if (p->d.act == 5 && t.bn < 32 && S > 1) continue;
            for (int ld : {2, 0, 3, 4}) {
                if (t.wgm * t.wgn == 8 && ld != 0) continue;                        // the 8-wave tiles only have the LDS-DMA loop
                // producer-wave path: bf16x3 only (ld 3: 64-deep stages, ld 4: 32-deep ones)
                if (ld >= 3 && (p->precision != MF_PREC_BF16X3 || p->q || t.bn < 64)) continue;
                if (t.bn == 80 && ld < 3) continue;
                const ConvTuned c{ConvTile{t.bm, t.bn, t.wgm, t.wgn, S}, ld};
                float us = 0.f;
                if ((rc = measure(c, &us))) break;
                if (us < best_us) { best_us = us; best_c = c; }
            }
            if (rc) break;
        }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc) { p->tuned.erase(batch); return rc; }
    // keep the model's pick unless the measured winner is clearly ahead (event timing of a 10-100 us launch is good to ~1 us)
    if (extend && best_us > 0.97f * base_us) {                                        // the entry stands (nothing is appended)
        if (had_entry) p->tuned[batch] = entry; else p->tuned.erase(batch);
    } else if (best_us > 0.97f * base_us) { p->tuned.erase(batch); tune_cache_store(key, ConvTuned{ConvTile{0, 0, 0, 0, 0}, -1}); }
    else { p->tuned[batch] = best_c; tune_cache_store(key, best_c); }
    static const bool verbose = mf_debug_has("tune");
    if (verbose)
        fprintf(stderr, "[mf_conv_tune] M %d N %d K %d: model %dx%d split %d %.1f us -> %s %dx%d split %d ld %d %.1f us\n", M, N, kt_min * 64, base.bm, base.bn, base.nsplit,
                base_us, p->tuned.count(batch) ? "tuned" : "kept", best_c.tile.bm, best_c.tile.bn, best_c.tile.nsplit, best_c.ld, best_us);
    return MF_OK;
}

void mf_conv_kernel_name(const ConvPlan* p, int batch, char* buf, int cap) {
    const char* x3 = p->precision != MF_PREC_BF16 ? "true" : "false";
    ConvLaunchCfg c;
    if (mf_conv_resolve(p, batch, 0, 0, &c)) { snprintf(buf, cap, "(no kernel: %s)", mf_last_error()); return; }
    const ConvTile& t = c.tile;
    // (the f16 + FP6 tile: the specialised workgroup <16,128,2,2,...> -- 4 compute + 4 producer waves)
    const char* qt = "2,2";
    switch (c.family) {
    case MF_CONV_FAMILY_F16Q:
        if (p->up_hi) { snprintf(buf, cap, "4 x k_conv3x3_halo_w<16,128,%s,true,1,phase> f16+fp6", qt); return; }
        {
            // (" grid N": the launch's thread count as rocprofv3 reports it, so that a counter pass can be matched to exactly these launches -- the split
            // and unsplit launches share one kernel symbol)
            const long grid = (long)batch * cdiv(p->out_h, 16) * cdiv(p->out_w, 16) * cdiv(p->d.cout, 128) * t.nsplit * 512;
            if (t.nsplit > 1) snprintf(buf, cap, "k_conv3x3_halo_w<16,128,%s,true,1> f16+fp6 split %d grid %ld", qt, t.nsplit, grid);
            else snprintf(buf, cap, "k_conv3x3_halo_w<16,128,%s,true,1> f16+fp6 grid %ld", qt, grid);
        }
        return;
    case MF_CONV_FAMILY_THIN:
        snprintf(buf, cap, "k_conv_thin<%d,%d,%d,%d,%s>", p->d.kh, p->d.stride_h, p->d.cin <= 8 ? 8 : 16, (p->d.cout + 15) / 16, x3);
        return;
    case MF_CONV_FAMILY_HALO_W_SPLIT:
        snprintf(buf, cap, "k_conv3x3_halo_w<16,256,2,4,%s,1> split %d", x3, t.nsplit);
        return;
    case MF_CONV_FAMILY_HALO_W:
    case MF_CONV_FAMILY_HALO:
        // last template argument: halo stages (register-weights kernel) / taps per weight-ring slot (LDS-weights kernel)
        snprintf(buf, cap, "k_conv3x3_halo%s<%d,%d,%d,%d,%s,%d>", c.family == MF_CONV_FAMILY_HALO_W ? "_w" : "", t.bm, t.bn, t.wgm, t.wgn, x3,
                 c.family == MF_CONV_FAMILY_HALO_W ? (t.bn >= 128 ? 1 : 3) : 2);
        return;
    default:   // implicit GEMM, or a wide halo plan's twin
        if (c.ld >= 3) snprintf(buf, cap, "k_conv_igemm<%d,%d,%d,%d,%s,%d,pw>", t.bm, t.bn, t.wgm, t.wgn, x3, c.bk);   // pw: producer waves
        else snprintf(buf, cap, "k_conv_igemm<%d,%d,%d,%d,%s,%d>%s", t.bm, t.bn, t.wgm, t.wgn, x3, c.bk, p->q ? " f16+fp6" : "");
    }
}

double mf_conv_flops(const ConvPlan* p, int batch) {
    const mf_conv2d_desc& d = p->d;
    const double taps = (double)d.kh * d.kw;
    const double sites = d.transposed ? (double)d.in_h * d.in_w : (double)p->out_h * p->out_w;
    return 2.0 * batch * sites * d.cin * d.cout * taps;
}
