// S3FD's post-process on the device: what face_detection/detection/sfd/detect.py:58-94 (batch_detect), bbox.py:44-64 (nms), bbox.py:111-129
// (batch_decode) and sfd_detector.py:41-47 (detect_from_batch) do on the host, per batch, in a Python loop over positions.
//
//   k_s3fd_u8_input   uint8 [B, H, W, 3] frame -> the graph's input planes, `- (104, 117, 123)` (detect.py:59-60) and the channel reversal of
//                     api.py:65 fused; the values are small integers, so the planes are bit-equal to mf_net_set_input of (img - mean).float()
//   k_s3fd_candidates one launch over all six levels and the whole batch: max-out background (level 1), two-class softmax, threshold, decode, append
//   k_s3fd_nms        one workgroup per image: sort by (score descending, key ascending), greedy NMS, boxes out in keep order
//
// Thresholds.  The reference cuts candidates at 0.05, runs NMS at 0.3, then drops boxes with score <= 0.5; its batch loop also emits a row in EVERY image for
// a position that passes in ANY image, so a list holds sub-threshold and duplicated rows.  None of that changes the answer: greedy NMS in score order lets a
// box be suppressed only by a higher-scoring one, and a duplicate has overlap 1 with its original.  The boxes that survive with score > final_thresh are
// therefore exactly the greedy NMS of the image's own boxes with score > final_thresh, and k_s3fd_nms stops at the first sorted candidate at or below it.
// A caller may pass cand_thresh = final_thresh and get the identical answer from shorter lists (tests/test_s3fd_detect.py checks both against the reference).
//
// Arithmetic.  Everything the reference rounds separately is rounded separately here (no fused multiply-add: the pragma below), exp is the precise expf,
// divisions are IEEE.  The NMS is the reference's, `+ 1` convention included (bbox.py:48,58), suppression on `ovr > thresh`.
#include "mf_aux.h"
#include <cmath>

#pragma clang fp contract(off)

#define MF_S3FD_LEVELS 6
#define MF_S3FD_MAX_CANDIDATES 4096          // per image: what one workgroup sorts in LDS
#define MF_S3FD_NMS_THREADS 1024
#define MF_S3FD_PER_THREAD (MF_S3FD_MAX_CANDIDATES / MF_S3FD_NMS_THREADS)
#define MF_S3FD_CAND_FLOATS 6                // x1, y1, x2, y2, score, key

namespace {

__device__ __forceinline__ uint32_t f2bf_d(float f) { return (uint32_t)__builtin_bit_cast(unsigned short, (__bf16)f); }   // as mf_aux.hip: round to nearest even
__device__ __forceinline__ float bf2f_d(uint32_t h) { return __uint_as_float(h << 16); }

struct Mean3 { float v[3]; };

// one thread = one pixel: 3 bytes in, one 8-channel group (16 B per plane) out; channels 3..7 zero like k_nchw_to_act
__global__ __launch_bounds__(256) void k_s3fd_u8_input(const uint8_t* __restrict__ img, Mean3 mean, int reverse, int H, int W, bf16_t* hi, bf16_t* lo, int halo, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int x = idx % W;
    int64_t t = idx / W;
    const int y = t % H;
    const int b = t / H;
    const uint8_t* p = img + idx * 3;
    uint32_t h[3], l[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = (float)p[reverse ? 2 - c : c] - mean.v[c];
        h[c] = f2bf_d(v);
        l[c] = f2bf_d(v - bf2f_d(h[c]));
    }
    const int64_t o = (((int64_t)b * (H + 2 * halo) + y + halo) * (W + 2 * halo) + x + halo) * 8;
    *reinterpret_cast<uint4*>(hi + o) = make_uint4(h[0] | h[1] << 16, h[2], 0u, 0u);
    if (lo) *reinterpret_cast<uint4*>(lo + o) = make_uint4(l[0] | l[1] << 16, l[2], 0u, 0u);
}

// One level's heads.  planes != 0: the 8-channel buffer of the graph (halo 0; conf in channels 0..3, loc in 4..7), hi / lo bf16 planes.
// planes == 0: the tensors s3fd.__call__ returns, fp32 NCHW cls [B, 2, h, w] (level 1 already maxed out) and reg [B, 4, h, w].
struct Level { const void* a; const void* b; int h, w; };
struct Levels { Level l[MF_S3FD_LEVELS]; int start[MF_S3FD_LEVELS + 1]; int planes; };

__device__ __forceinline__ uint32_t pack_key(int level, int h, int w) { return (uint32_t)level << 28 | (uint32_t)h << 14 | (uint32_t)w; }

__global__ __launch_bounds__(256) void k_s3fd_candidates(Levels L, int batch, float cand_thresh, int cap, float* __restrict__ cand, int* __restrict__ n_cand) {
    const int P = L.start[MF_S3FD_LEVELS];
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)batch * P) return;
    const int b = (int)(idx / P), p = (int)(idx % P);
    int lv = 0;
#pragma unroll
    for (int i = 1; i < MF_S3FD_LEVELS; ++i) lv += p >= L.start[i] ? 1 : 0;
    const Level S = L.l[lv];
    const int q = p - L.start[lv], hw = S.h * S.w;
    const int hy = q / S.w, wx = q % S.w;
    float bg, face, loc[4];
    if (L.planes) {
        const int64_t o = ((int64_t)b * hw + q) * 8;
        const uint4 uh = *reinterpret_cast<const uint4*>((const bf16_t*)S.a + o);
        const uint32_t wh[4] = {uh.x, uh.y, uh.z, uh.w};
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[2 * e] = bf2f_d(wh[e] & 0xffffu); v[2 * e + 1] = bf2f_d(wh[e] >> 16); }
        if (S.b) {
            const uint4 ul = *reinterpret_cast<const uint4*>((const bf16_t*)S.b + o);
            const uint32_t wl[4] = {ul.x, ul.y, ul.z, ul.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[2 * e] += bf2f_d(wl[e] & 0xffffu); v[2 * e + 1] += bf2f_d(wl[e] >> 16); }
        }
        if (lv == 0) { bg = fmaxf(fmaxf(v[0], v[1]), v[2]); face = v[3]; }       // max-out background label, net_s3fd.py:123-126
        else { bg = v[0]; face = v[1]; }
#pragma unroll
        for (int e = 0; e < 4; ++e) loc[e] = v[4 + e];
    } else {
        const float* cls = (const float*)S.a + (int64_t)b * 2 * hw + q;
        const float* reg = (const float*)S.b + (int64_t)b * 4 * hw + q;
        bg = cls[0]; face = cls[hw];
#pragma unroll
        for (int e = 0; e < 4; ++e) loc[e] = reg[(int64_t)e * hw];
    }
    // F.softmax(., dim=1)[:, 1] (detect.py:72): exp(x - max) / sum
    const float m = fmaxf(bg, face);
    const float e0 = expf(bg - m), e1 = expf(face - m);
    const float score = e1 / (e0 + e1);
    if (!(score > cand_thresh)) return;
    // batch_decode (bbox.py:124-128) on the prior (stride / 2 + w * stride, stride / 2 + h * stride, 4 * stride, 4 * stride), variances (0.1, 0.2)
    const float stride = (float)(4 << lv), anchor = 4.f * stride;
    const float axc = stride * 0.5f + (float)wx * stride, ayc = stride * 0.5f + (float)hy * stride;
    const float cx = axc + loc[0] * 0.1f * anchor, cy = ayc + loc[1] * 0.1f * anchor;
    const float bw = anchor * expf(loc[2] * 0.2f), bh = anchor * expf(loc[3] * 0.2f);
    const float x1 = cx - bw / 2.f, y1 = cy - bh / 2.f;
    const float x2 = bw + x1, y2 = bh + y1;
    const int slot = atomicAdd(n_cand + b, 1);           // keeps counting past the capacity: the caller sees the overflow
    if (slot >= cap) return;
    float* d = cand + ((int64_t)b * cap + slot) * MF_S3FD_CAND_FLOATS;
    d[0] = x1; d[1] = y1; d[2] = x2; d[3] = y2; d[4] = score; d[5] = __uint_as_float(pack_key(lv, hy, wx));
}

// One workgroup per image.  Sort: bitonic in LDS on the 64-bit word (~score bits : key) ascending == (score descending, key ascending); scores are positive
// floats, so their bit patterns order like their values, and a key is unique within an image: the order is total and does not depend on the order in which
// the appends landed.  NMS: thread t owns the sorted candidates t, t + 1024, ... in registers.  The kept boxes are visited in order; for each one every
// thread tests its own later candidates and a wave's 64 verdicts leave as one ballot word (no atomics: each word of the suppression mask has one writer).
// The work is (kept boxes) x (candidates), not the n^2 of a full pairwise mask, and needs no scratch beyond LDS; a face yields a handful of kept boxes.
__global__ __launch_bounds__(MF_S3FD_NMS_THREADS) void k_s3fd_nms(const float* __restrict__ cand, const int* __restrict__ n_cand, int cap, float nms_thresh, float final_thresh,
                                                                  int max_det, float* __restrict__ boxes, int* __restrict__ counts) {
    __shared__ unsigned long long s_key[MF_S3FD_MAX_CANDIDATES];
    __shared__ unsigned short s_idx[MF_S3FD_MAX_CANDIDATES];
    __shared__ unsigned long long s_sup[MF_S3FD_MAX_CANDIDATES / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(n_cand[b], cap);
    const float* C = cand + (int64_t)b * cap * MF_S3FD_CAND_FLOATS;
    float* out = boxes + (int64_t)b * max_det * 5;
    if (n == 0) { if (tid == 0) counts[b] = 0; return; }
    int N = 64;
    while (N < n) N <<= 1;
    for (int i = tid; i < N; i += MF_S3FD_NMS_THREADS) {
        unsigned long long k = ~0ull;
        if (i < n) k = (unsigned long long)(~__float_as_uint(C[i * MF_S3FD_CAND_FLOATS + 4])) << 32 | __float_as_uint(C[i * MF_S3FD_CAND_FLOATS + 5]);
        s_key[i] = k; s_idx[i] = (unsigned short)i;
    }
    if (tid < MF_S3FD_MAX_CANDIDATES / 64) s_sup[tid] = 0ull;
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N; i += MF_S3FD_NMS_THREADS) {
                const int p = i ^ j;
                if (p > i) {
                    const unsigned long long a = s_key[i], c = s_key[p];
                    if ((a > c) == ((i & k) == 0)) {
                        s_key[i] = c; s_key[p] = a;
                        const unsigned short t = s_idx[i]; s_idx[i] = s_idx[p]; s_idx[p] = t;
                    }
                }
            }
            __syncthreads();
        }
    // own candidates -> registers (slot q of thread t is sorted position q * 1024 + t: a wave's 64 lanes cover one word of the mask)
    float x1[MF_S3FD_PER_THREAD], y1[MF_S3FD_PER_THREAD], x2[MF_S3FD_PER_THREAD], y2[MF_S3FD_PER_THREAD], ar[MF_S3FD_PER_THREAD];
#pragma unroll
    for (int q = 0; q < MF_S3FD_PER_THREAD; ++q) {
        const int i = q * MF_S3FD_NMS_THREADS + tid;
        x1[q] = y1[q] = x2[q] = y2[q] = ar[q] = 0.f;
        if (i < n) {
            const float* c = C + (int)s_idx[i] * MF_S3FD_CAND_FLOATS;
            x1[q] = c[0]; y1[q] = c[1]; x2[q] = c[2]; y2[q] = c[3];
            ar[q] = (x2[q] - x1[q] + 1.f) * (y2[q] - y1[q] + 1.f);
        }
    }
    int kept = 0, i = 0;
    while (true) {
        // next sorted candidate that no kept box suppressed (uniform: every thread reads the same words)
        for (; i < n; i = (i | 63) + 1) {
            const unsigned long long live = ~s_sup[i >> 6] & (~0ull << (i & 63));
            if (live) { i = (i & ~63) + __ffsll(live) - 1; break; }
        }
        if (i >= n) break;
        const float* c = C + (int)s_idx[i] * MF_S3FD_CAND_FLOATS;
        const float bx1 = c[0], by1 = c[1], bx2 = c[2], by2 = c[3], bs = c[4];
        if (!(bs > final_thresh)) break;                 // sorted: nothing below can pass, and nothing below can suppress anything above
        if (tid == 0 && kept < max_det) { float* o = out + kept * 5; o[0] = bx1; o[1] = by1; o[2] = bx2; o[3] = by2; o[4] = bs; }
        ++kept;
        const float bar = (bx2 - bx1 + 1.f) * (by2 - by1 + 1.f);
#pragma unroll
        for (int q = 0; q < MF_S3FD_PER_THREAD; ++q) {
            if (q * MF_S3FD_NMS_THREADS >= n) break;     // uniform
            const int j = q * MF_S3FD_NMS_THREADS + tid;
            const float w = fmaxf(0.f, fminf(bx2, x2[q]) - fmaxf(bx1, x1[q]) + 1.f), h = fmaxf(0.f, fminf(by2, y2[q]) - fmaxf(by1, y1[q]) + 1.f);
            const float inter = w * h;
            const float ovr = inter / (bar + ar[q] - inter);
            const unsigned long long word = __ballot(j > i && j < n && ovr > nms_thresh);
            if ((tid & 63) == 0 && word) s_sup[j >> 6] |= word;
        }
        ++i;
        __syncthreads();
    }
    if (tid == 0) counts[b] = kept;                      // keeps counting past max_det: the caller sees the overflow
}

int detect_run(const Levels& L, int batch, float cand_thresh, float nms_thresh, float final_thresh, int max_candidates, int max_det, float* cand, float* boxes, int* counts,
               int* n_candidates, hipStream_t s) {
    const int64_t total = (int64_t)batch * L.start[MF_S3FD_LEVELS];
    MF_HIP(hipMemsetAsync(n_candidates, 0, (size_t)batch * sizeof(int), s));
    hipLaunchKernelGGL(k_s3fd_candidates, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, L, batch, cand_thresh, max_candidates, cand, n_candidates);
    MF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_s3fd_nms, dim3(batch), dim3(MF_S3FD_NMS_THREADS), 0, s, cand, n_candidates, max_candidates, nms_thresh, final_thresh, max_det, boxes, counts);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

int check_common(const char* who, int batch, int max_candidates, int max_det, const void* boxes, const void* counts, const void* n_candidates) {
    MF_REQUIRE(boxes && counts && n_candidates, "%s: null output", who);
    MF_REQUIRE(batch >= 1 && max_det >= 1, "%s: batch %d, max_det %d", who, batch, max_det);
    MF_REQUIRE(max_candidates >= 1 && max_candidates <= MF_S3FD_MAX_CANDIDATES, "%s: max_candidates %d outside [1, %d] (one workgroup sorts an image's list in LDS)", who,
               max_candidates, MF_S3FD_MAX_CANDIDATES);
    return MF_OK;
}

int add_level(const char* who, Levels& L, int i, const void* a, const void* b, int h, int w, int batch) {
    MF_REQUIRE(h >= 1 && w >= 1 && h < (1 << 14) && w < (1 << 14), "%s: level %d map %d x %d does not fit the 14-bit row / column fields of the sort key", who, i + 1, h, w);
    L.l[i] = Level{a, b, h, w};
    L.start[i + 1] = L.start[i] + h * w;
    MF_REQUIRE((int64_t)batch * L.start[i + 1] < (int64_t)1 << 31, "%s: %d positions per image x batch %d exceed 2^31", who, L.start[i + 1], batch);
    return MF_OK;
}

}  // namespace

extern "C" size_t mf_s3fd_detect_workspace_bytes(int batch, int max_candidates) {
    return batch >= 1 && max_candidates >= 1 ? (size_t)batch * max_candidates * MF_S3FD_CAND_FLOATS * sizeof(float) : 0;
}

extern "C" int mf_net_set_input_u8(mf_net* h, int buf, const uint8_t* u8_nhwc, const float* mean3, int reverse_channels, int batch, void* stream) {
    MF_REQUIRE(h && u8_nhwc && mean3 && batch >= 1 && batch <= mf_net_max_batch(h), "net_set_input_u8: bad argument (batch %d, capacity %d)", batch, mf_net_max_batch(h));
    const ActBuf* b = mf_net_actbuf(h, buf);
    MF_REQUIRE(b, "net: no buffer %d", buf);
    MF_REQUIRE(b->C == 8, "net_set_input_u8: buffer %d has %d channels, not the 8 of a 3-channel input", buf, b->C);
    const int64_t total = (int64_t)batch * b->H * b->W;
    hipLaunchKernelGGL(k_s3fd_u8_input, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u8_nhwc, Mean3{{mean3[0], mean3[1], mean3[2]}}, reverse_channels ? 1 : 0,
                       b->H, b->W, b->hi, b->lo, b->halo, total);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_s3fd_detect(mf_net* net, const int* head_bufs, int batch, float cand_thresh, float nms_thresh, float final_thresh, int max_candidates, int max_det, float* boxes,
                              int* counts, int* n_candidates, void* stream) {
    MF_REQUIRE(net && head_bufs, "s3fd_detect: null argument");
    int rc = check_common("s3fd_detect", batch, max_candidates, max_det, boxes, counts, n_candidates);
    if (rc) return rc;
    MF_REQUIRE(batch <= mf_net_max_batch(net), "s3fd_detect: batch %d exceeds the capacity %d", batch, mf_net_max_batch(net));
    Levels L{};
    L.planes = 1;
    for (int i = 0; i < MF_S3FD_LEVELS; ++i) {
        const ActBuf* b = mf_net_actbuf(net, head_bufs[i]);
        MF_REQUIRE(b, "net: no buffer %d", head_bufs[i]);
        MF_REQUIRE(b->C == 8 && b->halo == 0, "s3fd_detect: head buffer %d must have 8 channels and no halo (has %d, halo %d)", head_bufs[i], b->C, b->halo);
        if ((rc = add_level("s3fd_detect", L, i, b->hi, b->lo, b->H, b->W, batch))) return rc;
    }
    void* ws = nullptr;
    if ((rc = mf_net_scratch(net, mf_s3fd_detect_workspace_bytes(mf_net_max_batch(net), MF_S3FD_MAX_CANDIDATES), &ws))) return rc;
    return detect_run(L, batch, cand_thresh, nms_thresh, final_thresh, max_candidates, max_det, (float*)ws, boxes, counts, n_candidates, (hipStream_t)stream);
}

extern "C" int mf_s3fd_detect_tensors(const float* const* heads, const int* map_hw, int batch, float cand_thresh, float nms_thresh, float final_thresh, int max_candidates, int max_det,
                                      void* workspace, float* boxes, int* counts, int* n_candidates, void* stream) {
    MF_REQUIRE(heads && map_hw && workspace, "s3fd_detect_tensors: null argument");
    int rc = check_common("s3fd_detect_tensors", batch, max_candidates, max_det, boxes, counts, n_candidates);
    if (rc) return rc;
    Levels L{};
    L.planes = 0;
    for (int i = 0; i < MF_S3FD_LEVELS; ++i) {
        MF_REQUIRE(heads[2 * i] && heads[2 * i + 1], "s3fd_detect_tensors: null head tensor of level %d", i + 1);
        if ((rc = add_level("s3fd_detect_tensors", L, i, heads[2 * i], heads[2 * i + 1], map_hw[2 * i], map_hw[2 * i + 1], batch))) return rc;
    }
    return detect_run(L, batch, cand_thresh, nms_thresh, final_thresh, max_candidates, max_det, (float*)workspace, boxes, counts, n_candidates, (hipStream_t)stream);
}
