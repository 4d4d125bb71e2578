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

template <int BM, int BN, int WGM, int WGN>
int launch_tile(const ConvArgs& a, int nphase, int nsplit, int goff_max, bool x3, bool q, hipStream_t s) {
    if constexpr (BN == 80) return launch_pw_only<BM, BN, WGM, WGN>(a, nphase, nsplit, goff_max, x3, q, s);
    else return launch_prec<BM, BN, WGM, WGN>(a, nphase, nsplit, goff_max, x3, q, s);
}

// the literal tile list names the rows of MF_IGEMM_TILES, all of them, in order
#define MF_ROW_CHECK(I, BM, BN, WGM, WGN) \
    static_assert(MF_IGEMM_TILES[I].bm == BM && MF_IGEMM_TILES[I].bn == BN && MF_IGEMM_TILES[I].wgm == WGM && MF_IGEMM_TILES[I].wgn == WGN, "MF_IGEMM_TILE_LIST != MF_IGEMM_TILES");
MF_IGEMM_TILE_LIST(MF_ROW_CHECK)
#define MF_ROW_COUNT(I, BM, BN, WGM, WGN) +1
static_assert(0 MF_IGEMM_TILE_LIST(MF_ROW_COUNT) == sizeof(MF_IGEMM_TILES) / sizeof(MF_IGEMM_TILES[0]), "MF_IGEMM_TILE_LIST != MF_IGEMM_TILES");

}  // namespace

int mf_igemm_launch(const ConvArgs& a, const ConvTile& t, int nphase, int goff_max, bool x3, bool q, hipStream_t s) {
#define MF_ROW_LAUNCH(I, BM, BN, WGM, WGN) \
    if (t.bm == BM && t.bn == BN) return launch_tile<BM, BN, WGM, WGN>(a, nphase, t.nsplit, goff_max, x3, q, s);
    MF_IGEMM_TILE_LIST(MF_ROW_LAUNCH)
    mf_set_error("conv: no kernel for tile %dx%d", t.bm, t.bn);
    return MF_ERR_INVALID;
}

int mf_splitk_combine(const ConvArgs& e0, int nsplit, int batch, int Ho, int Wo, double* gn_out, int gn_groups, bool* with_stats, hipStream_t s) {
    ConvArgs e = e0;
    const int64_t total = (int64_t)batch * Ho * Wo * ((e.act == 5 ? e.N / 2 : e.N) / 4);
    MF_REQUIRE(total < 0x7fffffffll, "conv: split-K combine over %lld channel quads (32-bit thread index)", (long long)total);
    *with_stats = gn_out && e.act != 5 && e.N % 4 == 0 && e.N % gn_groups == 0 && gn_groups <= 64;
    if (*with_stats) {
        e.gn_out = gn_out; e.gn_out_groups = gn_groups; e.gn_out_cpg = e.N / gn_groups;
        const int nq = e.N / 4, cols = std::min(256, nq), ppi = 256 / cols, T = Ho * Wo;
        const int target = 1024;                                         // workgroups aimed for (each issues 2 * groups fp64 atomics): 128 / 256 and 2048 / 4096 all measured slower
        const int P = std::max(ppi, std::min(64 * ppi, (int)(((int64_t)T * batch + target - 1) / target)));
        hipLaunchKernelGGL(k_splitk_epilogue_stats, dim3((unsigned)((T + P - 1) / P), batch), dim3(256), 0, s, e, nsplit, Ho, Wo, P, epi_div(e, Ho, Wo));
    } else {
        hipLaunchKernelGGL(k_splitk_epilogue, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, e, nsplit, Ho, Wo, (int)total, epi_div(e, Ho, Wo));
    }
    MF_HIP(hipGetLastError());
    return MF_OK;
}
