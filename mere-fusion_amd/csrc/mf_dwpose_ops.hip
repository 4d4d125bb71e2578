// Two more ops of the static-graph executor (mf_net.hip), the ones a CSPNeXt backbone (mmdet, the DWPose landmark network of
// musetalk/utils/preprocessing.py:17-19) needs beside the MFMA convolutions: the depthwise k x k convolution of its DepthwiseSeparableConvModule and the
// hard-sigmoid channel attention of its CSPLayer.  Neither is matrix work: both are built for coalesced access to the padded NHWC (hi, lo) planes, channels innermost.
#include "mf_nn.h"
#include "mf_aux.h"
#include "mf_schedule.h"
#include "mf_net_planes.h"
#include "mf_net_handle.h"
#include <vector>

namespace {

constexpr int DW_T = 8;        // output tile: DW_T x DW_T pixels ...
constexpr int DW_C = 32;       // ... of DW_C channels per workgroup; thread = (channel, tile row)

__device__ __forceinline__ float dw_act(float v, int act) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 4) return v / (1.f + __expf(-v));
    return v;
}

// Depthwise conv, BatchNorm folded into (w, bias) by the host, then the activation.  The input tile with its halo -- ((DW_T - 1) * stride + K)^2 pixels x DW_C
// channels -- is staged once in LDS as fp32 (hi + lo summed on the way in), channels innermost: a wave's 64 lanes are 32 channels x 2 tile rows, so a read is
// one bank per lane in each 32-lane half and every tap is reused by up to K^2 outputs.  Pixels outside the image are zeros (the conv's padding), whatever halo
// the buffer has.  w: [K * K][C] (tap-major, so lanes read consecutive floats).
template <int K>
__global__ __launch_bounds__(256) void k_dwconv(Pl X, int xoff, Pl Y, int yoff, const float* __restrict__ w, const float* __restrict__ bias, int C, int stride, int act, int tiles_x) {
    extern __shared__ float tile[];
    const int span = (DW_T - 1) * stride + K;                                  // input rows / columns under one output tile
    const int b = blockIdx.z, c0 = blockIdx.y * DW_C;
    const int ty0 = (blockIdx.x / tiles_x) * DW_T, tx0 = (blockIdx.x % tiles_x) * DW_T;
    const int iy0 = ty0 * stride - K / 2, ix0 = tx0 * stride - K / 2;
    const int cl = threadIdx.x & (DW_C - 1), c = c0 + cl;
    for (int p = threadIdx.x >> 5; p < span * span; p += 256 / DW_C) {
        const int iy = iy0 + p / span, ix = ix0 + p % span;
        float v = 0.f;
        if (c < C && iy >= 0 && iy < X.H && ix >= 0 && ix < X.W) v = X.ld(X.at(b, iy, ix) + xoff + c);
        tile[p * DW_C + cl] = v;
    }
    __syncthreads();
    if (c >= C) return;
    float wr[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) wr[t] = w[t * C + c];
    const float bs = bias[c];
    const int oy = ty0 + (threadIdx.x >> 5);
    if (oy >= Y.H) return;
    const int ly = (threadIdx.x >> 5) * stride;
    for (int j = 0; j < DW_T; ++j) {
        const int ox = tx0 + j;
        if (ox >= Y.W) break;
        float acc = 0.f;
#pragma unroll
        for (int dy = 0; dy < K; ++dy)
#pragma unroll
            for (int dx = 0; dx < K; ++dx) acc = fmaf(tile[((ly + dy) * span + j * stride + dx) * DW_C + cl], wr[dy * K + dx], acc);
        Y.st(Y.at(b, oy, ox) + yoff + c, dw_act(acc + bs, act));
    }
}

// s[b][c] = hardsigmoid(fc(pooled)[c]) = clamp(z / 6 + 1 / 2, 0, 1): one wave per output channel, lanes over the input channels (w: [C][C] row-major)
__global__ __launch_bounds__(256) void k_ca_fc(Pl P, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ s, int C) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, b = blockIdx.y;
    if (c >= C) return;
    const int64_t po = P.at(b, 0, 0);
    float z = 0.f;
    for (int j = lane; j < C; j += 64) z = fmaf(w[(int64_t)c * C + j], P.ld(po + j), z);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o);
    if (lane == 0) s[(int64_t)b * C + c] = fminf(fmaxf((z + bias[c]) / 6.f + 0.5f, 0.f), 1.f);
}

__global__ __launch_bounds__(256) void k_ca_scale(Pl X, int xoff, const float* __restrict__ s, Pl Y, int yoff, int C, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = idx % C;
    int64_t t = idx / C;
    const int x = t % X.W; t /= X.W;
    const int y = t % X.H;
    const int b = t / X.H;
    Y.st(Y.at(b, y, x) + yoff + c, X.ld(X.at(b, y, x) + xoff + c) * s[(int64_t)b * C + c]);
}

int upload(mf_net* h, const std::vector<float>& v, float** out) { return h->upload(v.data(), v.size(), out); }

}  // namespace

extern "C" int mf_net_dwconv(mf_net* h, int C, int k, int stride, int act, const float* weight, const float* bias, const float* bn_gamma, const float* bn_beta,
                             const float* bn_mean, const float* bn_var, float bn_eps, int in_buf, int in_coff, int out_buf, int out_coff) {
    MF_REQUIRE(h && weight && C > 0 && in_coff >= 0 && out_coff >= 0, "net_dwconv: bad argument");
    MF_REQUIRE((k == 3 || k == 5) && (stride == 1 || stride == 2), "net_dwconv: k must be 3 or 5 and stride 1 or 2 (got %d, %d)", k, stride);
    MF_REQUIRE(act == 0 || act == 1 || act == 4, "net_dwconv: activation %d (0 none, 1 ReLU, 4 SiLU)", act);
    NET_BUF(ib, in_buf); NET_BUF(ob, out_buf);
    MF_REQUIRE(in_coff + C <= ib->C && out_coff + C <= ob->C, "net_dwconv: channel slice outside a buffer");
    const int pad = k / 2;
    MF_REQUIRE(ob->H == (ib->H + 2 * pad - k) / stride + 1 && ob->W == (ib->W + 2 * pad - k) / stride + 1, "net_dwconv: output buffer %dx%d does not match the %dx%d input", ob->H,
               ob->W, ib->H, ib->W);
    const bool bn = bn_gamma && bn_beta && bn_mean && bn_var;
    MF_REQUIRE(bn || (!bn_gamma && !bn_beta && !bn_mean && !bn_var), "net_dwconv: give all four BatchNorm vectors or none");
    std::vector<float> wt((size_t)k * k * C), bs(C);
    for (int c = 0; c < C; ++c) {                                              // fold in double; [C][1][k][k] -> [k * k][C]
        const double sc = bn ? (double)bn_gamma[c] / std::sqrt((double)bn_var[c] + (double)bn_eps) : 1.0;
        for (int t = 0; t < k * k; ++t) wt[(size_t)t * C + c] = (float)(weight[(size_t)c * k * k + t] * sc);
        const double b0 = bias ? bias[c] : 0.0;
        bs[c] = (float)(bn ? (b0 - bn_mean[c]) * sc + bn_beta[c] : b0);
    }
    float *dw = nullptr, *db = nullptr;
    int rc = upload(h, wt, &dw);
    if (rc || (rc = upload(h, bs, &db))) return rc;
    const int span = (DW_T - 1) * stride + k;
    const size_t lds = (size_t)span * span * DW_C * sizeof(float);             // at most 19 * 19 * 32 * 4 = 46 208 bytes
    h->sch.push("dwconv", "", 2.0 * k * k * C * ob->H * ob->W, [=](int B, hipStream_t s) {
        const int tx = (ob->W + DW_T - 1) / DW_T, ty = (ob->H + DW_T - 1) / DW_T;
        const dim3 grid(tx * ty, (C + DW_C - 1) / DW_C, B);
        if (k == 3) hipLaunchKernelGGL(k_dwconv<3>, grid, dim3(256), lds, s, pl_of(*ib), in_coff, pl_of(*ob), out_coff, dw, db, C, stride, act, tx);
        else hipLaunchKernelGGL(k_dwconv<5>, grid, dim3(256), lds, s, pl_of(*ib), in_coff, pl_of(*ob), out_coff, dw, db, C, stride, act, tx);
        MF_HIP(hipGetLastError());
        return MF_OK;
    });
    return MF_OK;
}

extern "C" int mf_net_chan_attn(mf_net* h, int x_buf, int x_coff, int C, int pooled_buf, const float* fc_weight, const float* fc_bias, int out_buf, int out_coff) {
    MF_REQUIRE(h && fc_weight && fc_bias && C > 0 && x_coff >= 0 && out_coff >= 0, "net_chan_attn: bad argument");
    NET_BUF(xb, x_buf); NET_BUF(pb, pooled_buf); NET_BUF(ob, out_buf);
    MF_REQUIRE(xb->H == ob->H && xb->W == ob->W && x_coff + C <= xb->C && out_coff + C <= ob->C, "net_chan_attn: x / out mismatch");
    MF_REQUIRE(pb->H == 1 && pb->W == 1 && pb->C >= C, "net_chan_attn: the pooled input must be a 1x1 map with >= %d channels", C);
    float *dw = nullptr, *db = nullptr, *ds = nullptr;
    int rc = upload(h, std::vector<float>(fc_weight, fc_weight + (size_t)C * C), &dw);
    if (rc || (rc = upload(h, std::vector<float>(fc_bias, fc_bias + C), &db)) || (rc = upload(h, std::vector<float>((size_t)h->cap * C, 0.f), &ds))) return rc;
    h->sch.push("chan_attn", "", 2.0 * C * C, [=](int B, hipStream_t s) {
        hipLaunchKernelGGL(k_ca_fc, dim3((C + 3) / 4, B), dim3(256), 0, s, pl_of(*pb), dw, db, ds, C);
        MF_HIP(hipGetLastError());
        const int64_t total = (int64_t)B * xb->H * xb->W * C;
        hipLaunchKernelGGL(k_ca_scale, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, pl_of(*xb), x_coff, ds, pl_of(*ob), out_coff, C, total);
        MF_HIP(hipGetLastError());
        return MF_OK;
    });
    return MF_OK;
}
