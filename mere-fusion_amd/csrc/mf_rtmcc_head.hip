// RTMCCHead of mmpose after its final convolution (the DWPose landmark network, musetalk/utils/preprocessing.py:17-19): the K keypoint maps of a net buffer are K
// tokens of H * W values; ScaleNorm -> Linear -> one gated attention unit (RTMCCBlock: ScaleNorm, uv Linear, SiLU, gamma / beta for q and k, relu(q k^T / sqrt(s))^2,
// u * (kernel v), the out Linear, the scaled shortcut) -> cls_x, cls_y.  Everything is fp32 FMA: K = 133 tokens of 256 values is no MFMA workload.
//
// Two launches per forward, each a grid of (token tiles of 8) x batch.  A token tile stays in LDS through every token-local step; what the attention needs from ALL
// tokens of an image (q's partner k, transposed, and v) and what the second launch needs back (u, the shortcut) passes through a device workspace of the handle
// (0.7 MB per image, L2-resident).  Weights are transposed on the host to [in][out], so a thread owns one output column for its 8 tokens and a wave reads
// consecutive floats; the token values it multiplies them with are LDS broadcasts.
#include "mf_nn.h"
#include "mf_aux.h"
#include "mf_net_planes.h"
#include <cmath>
#include <memory>
#include <vector>

namespace {

constexpr int TT = 8;                                                          // tokens per workgroup

struct HeadDims { int K, D, Hd, S, E, BX, BY; };
struct HeadPtrs {
    const float *w_mlp, *w_uv, *gamma, *beta, *w_o, *res_scale, *w_cls;       // [D][Hd], [Hd][2E+S], [2][S], [2][S], [E][Hd], [Hd], [Hd][BX+BY]
    float *x0, *u, *v, *q, *kT;                                                // [B][K][Hd], [B][K][E], [B][K][E], [B][K][S], [B][S][K]
    float g_mlp, g_ln, eps, inv_sqrt_s;
};

// ScaleNorm's factor for each of the tile's tokens: g / max(|x| * n^-1/2, eps); wave w takes tokens w, w + 4
__device__ __forceinline__ void scale_norm_factors(const float* rows, int n, float g, float eps, float* fac) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int t = wave; t < TT; t += 4) {
        float ss = 0.f;
        for (int i = lane; i < n; i += 64) { const float v = rows[t * n + i]; ss = fmaf(v, v, ss); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
        if (lane == 0) fac[t] = g / fmaxf(sqrtf(ss) * rsqrtf((float)n), eps);
    }
}

// acc[t] = sum_i rows[t][i] * wt[i][j] for the tile's tokens (rows in LDS, wt [n][ld] in global memory)
__device__ __forceinline__ void column_dot(const float* rows, int n, const float* __restrict__ wt, int ld, int j, float* acc) {
#pragma unroll
    for (int t = 0; t < TT; ++t) acc[t] = 0.f;
    for (int i = 0; i < n; ++i) {
        const float w = wt[(int64_t)i * ld + j];
#pragma unroll
        for (int t = 0; t < TT; ++t) acc[t] = fmaf(rows[t * n + i], w, acc[t]);
    }
}

__device__ __forceinline__ float silu(float v) { return v / (1.f + __expf(-v)); }

// maps -> ScaleNorm -> mlp Linear (x0, kept for the shortcut) -> ScaleNorm -> uv Linear -> SiLU -> u, v, q, k^T
__global__ __launch_bounds__(256) void k_head_tokens(Pl P, int coff, HeadDims d, HeadPtrs p) {
    extern __shared__ float lds[];
    float *in = lds, *xs = in + TT * d.D, *fac = xs + TT * d.Hd;               // [TT][D], [TT][Hd], [TT]
    const int b = blockIdx.y, k0 = blockIdx.x * TT;
    for (int idx = threadIdx.x; idx < TT * d.D; idx += 256) {                  // consecutive lanes: consecutive tokens = consecutive channels of one pixel
        const int t = idx % TT, i = idx / TT;
        in[t * d.D + i] = k0 + t < d.K ? P.ld(P.at(b, i / P.W, i % P.W) + coff + k0 + t) : 0.f;
    }
    __syncthreads();
    scale_norm_factors(in, d.D, p.g_mlp, p.eps, fac);
    __syncthreads();
    float acc[TT];
    for (int j = threadIdx.x; j < d.Hd; j += 256) {
        column_dot(in, d.D, p.w_mlp, d.Hd, j, acc);
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            const float v = acc[t] * fac[t];
            xs[t * d.Hd + j] = v;
            if (k0 + t < d.K) p.x0[((int64_t)b * d.K + k0 + t) * d.Hd + j] = v;
        }
    }
    __syncthreads();
    scale_norm_factors(xs, d.Hd, p.g_ln, p.eps, fac);                          // (fac is read again only after the barrier below; the mlp loop above is done with it)
    __syncthreads();
    const int N = 2 * d.E + d.S;
    for (int j = threadIdx.x; j < N; j += 256) {
        column_dot(xs, d.Hd, p.w_uv, N, j, acc);
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            if (k0 + t >= d.K) break;
            const float v = silu(acc[t] * fac[t]);
            const int64_t tok = (int64_t)b * d.K + k0 + t;
            if (j < d.E) p.u[tok * d.E + j] = v;
            else if (j < 2 * d.E) p.v[tok * d.E + j - d.E] = v;
            else {
                const int i = j - 2 * d.E;
                p.q[tok * d.S + i] = fmaf(v, p.gamma[i], p.beta[i]);
                p.kT[((int64_t)b * d.S + i) * d.K + k0 + t] = fmaf(v, p.gamma[d.S + i], p.beta[d.S + i]);
            }
        }
    }
}

// kernel rows of the tile against every token -> u * (kernel v) -> out Linear + scaled shortcut -> cls_x | cls_y
__global__ __launch_bounds__(256) void k_head_attend(HeadDims d, HeadPtrs p, float* __restrict__ lx, float* __restrict__ ly) {
    extern __shared__ float lds[];
    float *qs = lds, *att = qs + TT * d.S, *ys = att + TT * d.K, *x1 = ys + TT * d.E;   // [TT][S], [TT][K], [TT][E], [TT][Hd]
    const int b = blockIdx.y, k0 = blockIdx.x * TT;
    for (int idx = threadIdx.x; idx < TT * d.S; idx += 256) {
        const int t = idx / d.S, i = idx % d.S;
        qs[idx] = k0 + t < d.K ? p.q[((int64_t)b * d.K + k0 + t) * d.S + i] : 0.f;
    }
    __syncthreads();
    const float* kT = p.kT + (int64_t)b * d.S * d.K;
    for (int idx = threadIdx.x; idx < TT * d.K; idx += 256) {
        const int t = idx / d.K, m = idx % d.K;
        float dot = 0.f;
        for (int i = 0; i < d.S; ++i) dot = fmaf(qs[t * d.S + i], kT[(int64_t)i * d.K + m], dot);
        const float r = fmaxf(dot * p.inv_sqrt_s, 0.f);
        att[idx] = r * r;
    }
    __syncthreads();
    float acc[TT];
    for (int c = threadIdx.x; c < d.E; c += 256) {
        column_dot(att, d.K, p.v + (int64_t)b * d.K * d.E, d.E, c, acc);
#pragma unroll
        for (int t = 0; t < TT; ++t) ys[t * d.E + c] = k0 + t < d.K ? acc[t] * p.u[((int64_t)b * d.K + k0 + t) * d.E + c] : 0.f;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < d.Hd; j += 256) {
        column_dot(ys, d.E, p.w_o, d.Hd, j, acc);
#pragma unroll
        for (int t = 0; t < TT; ++t) x1[t * d.Hd + j] = k0 + t < d.K ? fmaf(p.res_scale[j], p.x0[((int64_t)b * d.K + k0 + t) * d.Hd + j], acc[t]) : 0.f;
    }
    __syncthreads();
    const int N = d.BX + d.BY;
    for (int j = threadIdx.x; j < N; j += 256) {
        column_dot(x1, d.Hd, p.w_cls, N, j, acc);
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            if (k0 + t >= d.K) break;
            const int64_t tok = (int64_t)b * d.K + k0 + t;
            if (j < d.BX) lx[tok * d.BX + j] = acc[t];
            else ly[tok * d.BY + j - d.BX] = acc[t];
        }
    }
}

}  // namespace

struct mf_rtmcc_head {
    HeadDims d{};
    HeadPtrs p{};
    int cap = 1;
    std::vector<float*> dev;
    ~mf_rtmcc_head() { for (float* x : dev) (void)hipFree(x); }
    int alloc(size_t n, float** out) {
        float* x = nullptr;
        MF_HIP(hipMalloc(&x, n * sizeof(float)));
        dev.push_back(x);
        MF_HIP(hipMemset(x, 0, n * sizeof(float)));
        *out = x;
        return MF_OK;
    }
    int upload(const std::vector<float>& v, const float** out) {
        float* x = nullptr;
        const int rc = alloc(v.size(), &x);
        if (rc) return rc;
        MF_HIP(hipMemcpy(x, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
        *out = x;
        return MF_OK;
    }
};

static std::vector<float> transposed(const float* w, int rows, int cols) {    // [rows][cols] -> [cols][rows]
    std::vector<float> t((size_t)rows * cols);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) t[(size_t)c * rows + r] = w[(size_t)r * cols + c];
    return t;
}

extern "C" int mf_rtmcc_head_create(int tokens, int flat, int hidden, int s, int bins_x, int bins_y, const float* mlp_g, const float* mlp_w, const float* ln_g, const float* uv_w,
                                    const float* gamma, const float* beta, const float* o_w, const float* res_scale, const float* cls_x_w, const float* cls_y_w, int max_batch,
                                    mf_rtmcc_head** out) {
    MF_REQUIRE(out && mlp_g && mlp_w && ln_g && uv_w && gamma && beta && o_w && res_scale && cls_x_w && cls_y_w, "rtmcc_head_create: null argument");
    MF_REQUIRE(tokens >= 1 && tokens <= 256 && flat >= 1 && flat <= 1024 && hidden >= 1 && hidden <= 1024 && s >= 1 && s <= 512 && bins_x >= 1 && bins_y >= 1 && max_batch >= 1 &&
               max_batch <= 512, "rtmcc_head_create: bad dimensions");
    std::unique_ptr<mf_rtmcc_head> h(new mf_rtmcc_head());
    HeadDims& d = h->d;
    d = HeadDims{tokens, flat, hidden, s, 2 * hidden, bins_x, bins_y};         // expansion factor 2
    h->cap = max_batch;
    const size_t lds = sizeof(float) * (size_t)TT * std::max(d.D + d.Hd + 1, d.S + d.K + d.E + d.Hd);
    MF_REQUIRE(lds <= 64 * 1024, "rtmcc_head_create: a tile of %d tokens needs %zu bytes of LDS", TT, lds);
    HeadPtrs& p = h->p;
    p.g_mlp = mlp_g[0]; p.g_ln = ln_g[0]; p.eps = 1e-5f; p.inv_sqrt_s = (float)(1.0 / std::sqrt((double)s));
    const int N = 2 * d.E + d.S;
    std::vector<float> cls = transposed(cls_x_w, bins_x, hidden), cy = transposed(cls_y_w, bins_y, hidden), both((size_t)hidden * (bins_x + bins_y));
    for (int i = 0; i < hidden; ++i) {
        std::copy(cls.begin() + (size_t)i * bins_x, cls.begin() + (size_t)(i + 1) * bins_x, both.begin() + (size_t)i * (bins_x + bins_y));
        std::copy(cy.begin() + (size_t)i * bins_y, cy.begin() + (size_t)(i + 1) * bins_y, both.begin() + (size_t)i * (bins_x + bins_y) + bins_x);
    }
    int rc;
    if ((rc = h->upload(transposed(mlp_w, hidden, flat), &p.w_mlp)) || (rc = h->upload(transposed(uv_w, N, hidden), &p.w_uv)) ||
        (rc = h->upload(std::vector<float>(gamma, gamma + 2 * s), &p.gamma)) || (rc = h->upload(std::vector<float>(beta, beta + 2 * s), &p.beta)) ||
        (rc = h->upload(transposed(o_w, hidden, d.E), &p.w_o)) || (rc = h->upload(std::vector<float>(res_scale, res_scale + hidden), &p.res_scale)) ||
        (rc = h->upload(both, &p.w_cls)))
        return rc;
    const size_t B = max_batch;
    if ((rc = h->alloc(B * tokens * hidden, &p.x0)) || (rc = h->alloc(B * tokens * d.E, &p.u)) || (rc = h->alloc(B * tokens * d.E, &p.v)) ||
        (rc = h->alloc(B * tokens * s, &p.q)) || (rc = h->alloc(B * tokens * s, &p.kT)))
        return rc;
    *out = h.release();
    return MF_OK;
}

extern "C" int mf_rtmcc_head_forward(mf_rtmcc_head* h, mf_net* net, int buf, int coff, int batch, float* logits_x, float* logits_y, void* stream) {
    MF_REQUIRE(h && net && logits_x && logits_y, "rtmcc_head_forward: null argument");
    MF_REQUIRE(batch >= 1 && batch <= h->cap && batch <= mf_net_max_batch(net), "rtmcc_head_forward: batch %d exceeds the capacity (%d, net %d)", batch, h->cap, mf_net_max_batch(net));
    const ActBuf* b = mf_net_actbuf(net, buf);
    MF_REQUIRE(b, "net: no buffer %d", buf);
    const HeadDims& d = h->d;
    MF_REQUIRE(coff >= 0 && coff + d.K <= b->C && b->H * b->W == d.D, "rtmcc_head_forward: buffer %d (%d channels, %dx%d) does not hold %d maps of %d values at channel %d", buf,
               b->C, b->H, b->W, d.K, d.D, coff);
    const dim3 grid((d.K + TT - 1) / TT, batch);
    hipLaunchKernelGGL(k_head_tokens, grid, dim3(256), sizeof(float) * TT * (d.D + d.Hd + 1), (hipStream_t)stream, pl_of(*b), coff, d, h->p);
    MF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_head_attend, grid, dim3(256), sizeof(float) * TT * (d.S + d.K + d.E + d.Hd), (hipStream_t)stream, d, h->p, logits_x, logits_y);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

extern "C" void mf_rtmcc_head_destroy(mf_rtmcc_head* h) { delete h; }
