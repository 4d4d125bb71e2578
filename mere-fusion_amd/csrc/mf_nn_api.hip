// C ABI test seams of the token-sequence ops (mf_nn.hip) and of the composite attention, like mf_attention_forward: fp32 [batch][T][C] device
// tensors in and out, every op launched exactly as the model builders launch it.  Each call owns its buffers: they are filled with a fixed finite
// poison value first (MF_NN_POISON_*), the input view is loaded over it, and `y_full` hands the whole padded output buffer back, so a test sees
// every element an op wrote outside its view (halo ring, neighbouring channels of a wider buffer, tokens past a prefix).
// mf_conv_view_forward and mf_attention_view_forward launch a conv layer and the fused attention on views the same way (sequence layers, token prefixes,
// packed q | k | v).  mf_faces_u8_forward, mf_vae_image_u8_forward and mf_head_sigmoid_forward are the seams of mf_aux.hip's uint8 producers and head.  mf_act_q_encode is the same kind of seam for the producers of the f16 + FP6-block activation format (mf_aux.hip): it hands back the raw planes.
#include "mf_nn.h"
#include "mf_aux.h"
#include <cmath>

namespace {

constexpr bf16_t POISON_HI = 0xC49A;   // -1232
constexpr bf16_t POISON_LO = 0x3F20;   // 0.625: hi + lo = -1231.375 is exact in fp32, and a write to either plane alone changes it

__global__ __launch_bounds__(256) void k_fill_planes(bf16_t* hi, bf16_t* lo, int64_t n, bf16_t vh, bf16_t vl) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    hi[i] = vh;
    if (lo) lo[i] = vl;
}

__global__ __launch_bounds__(256) void k_planes_to_f32(const bf16_t* hi, const bf16_t* lo, float* dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = __uint_as_float((uint32_t)hi[i] << 16);
    if (lo) v += __uint_as_float((uint32_t)lo[i] << 16);
    dst[i] = v;
}

bool geom_ok(const mf_rows_geom* g) {
    return g && g->c > 0 && g->coff >= 0 && g->coff + g->c <= g->cbuf && g->h > 0 && g->w > 0 && g->halo >= 0;
}

// a poisoned activation buffer of `batch` items
struct PBuf {
    ActBuf b;
    int64_t n = 0;     // elements of the batch (without the tail pad every buffer of the library carries)
    ~PBuf() {
        if (b.hi) (void)hipFree(b.hi);
        if (b.lo) (void)hipFree(b.lo);
    }
    int alloc(int C, int H, int W, int halo, int batch, bool x3, hipStream_t s) {
        b.C = C; b.H = H; b.W = W; b.halo = halo;
        n = (int64_t)batch * b.per_batch();
        const int64_t total = n + 64;
        MF_HIP(hipMalloc(&b.hi, total * sizeof(bf16_t)));
        if (x3) MF_HIP(hipMalloc(&b.lo, total * sizeof(bf16_t)));
        hipLaunchKernelGGL(k_fill_planes, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, b.hi, b.lo, total, POISON_HI, POISON_LO);
        MF_HIP(hipGetLastError());
        return MF_OK;
    }
    int alloc(const mf_rows_geom& g, int batch, bool x3, hipStream_t s) { return alloc(g.cbuf, g.h, g.w, g.halo, batch, x3, s); }
    ActView view(const mf_rows_geom& g) const { return ActView{&b, g.coff, g.c}; }
    ActView all() const { return ActView{&b, 0, b.C}; }
    int full(float* dst, hipStream_t s, int64_t tail = 0) const {      // [batch][Hp][Wp][C] (+ `tail` elements of the allocation's pad) as fp32 (hi + lo), or nothing
        if (!dst) return MF_OK;
        hipLaunchKernelGGL(k_planes_to_f32, dim3((unsigned)((n + tail + 255) / 256)), dim3(256), 0, s, b.hi, b.lo, dst, n + tail);
        MF_HIP(hipGetLastError());
        return MF_OK;
    }
};

// fp32 NCHW [batch][C][P] -> the [batch][P][C] rows mf_rows_from_f32 reads
__global__ __launch_bounds__(256) void k_nchw_to_rows_f32(const float* __restrict__ src, float* __restrict__ dst, int C, int P, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const int64_t r = i / C;
    const int p = (int)(r % P);
    const int64_t b = r / P;
    dst[i] = src[(b * C + c) * P + p];
}

struct DevMem {
    void* p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) { MF_HIP(hipMalloc(&p, bytes)); return MF_OK; }
};

struct PlanGuard {
    ConvPlan p;
    ~PlanGuard() { mf_conv_plan_destroy(&p); }
};

// the halo ring of every item, and the allocation's tail, as mf_actbuf_alloc leaves them: zero (a conv reads its padding there)
__global__ __launch_bounds__(256) void k_zero_ring(bf16_t* hi, bf16_t* lo, int C, int H, int W, int halo, int64_t n, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if (i < n) {
        const int64_t px = i / C;
        const int Wp = W + 2 * halo, Hp = H + 2 * halo;
        const int col = (int)(px % Wp), row = (int)((px / Wp) % Hp);
        if (col >= halo && col < halo + W && row >= halo && row < halo + H) return;
    }
    hi[i] = 0;
    if (lo) lo[i] = 0;
}

int zero_ring(const PBuf& b, hipStream_t s) {
    const int64_t total = b.n + 64;
    hipLaunchKernelGGL(k_zero_ring, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, b.b.hi, b.b.lo, b.b.C, b.b.H, b.b.W, b.b.halo, b.n, total);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

bool same_buffer(const mf_rows_geom* a, const mf_rows_geom* b) { return a->cbuf == b->cbuf && a->h == b->h && a->w == b->w && a->halo == b->halo; }

#define API_PREC(name)                                                                                                                  \
    MF_REQUIRE(precision == MF_PREC_BF16 || precision == MF_PREC_BF16X3, name ": unknown precision %d", precision);                       \
    const bool x3 = precision == MF_PREC_BF16X3;                                                                                          \
    hipStream_t s = (hipStream_t)stream;                                                                                                  \
    int rc

}  // namespace

extern "C" int mf_rows_roundtrip(const float* x, const float* addend, float* y, float* y_layered, const mf_rows_geom* g, int batch, int tokens,
                                 int layer, int n_layers, int precision, float* y_full, void* stream) {
    MF_REQUIRE(x && geom_ok(g) && batch > 0, "rows_roundtrip: null argument or bad geometry");
    API_PREC("rows_roundtrip");
    PBuf b;
    if ((rc = b.alloc(*g, batch, x3, s))) return rc;
    if ((rc = mf_rows_from_f32(x, addend, b.view(*g), batch, s))) return rc;
    if (y && (rc = mf_rows_to_f32(b.view(*g), y, batch, s))) return rc;
    if (y_layered && (rc = mf_rows_to_f32_layered(b.view(*g), y_layered, batch, tokens, layer, n_layers, s))) return rc;
    if ((rc = b.full(y_full, s))) return rc;
    MF_HIP(hipStreamSynchronize(s));
    return MF_OK;
}

extern "C" int mf_layernorm_forward(const float* x, const float* gamma, const float* beta, float* y, const mf_rows_geom* gx, const mf_rows_geom* gy,
                                    int batch, float eps, int tokens, int act, int precision, float* y_full, void* stream) {
    MF_REQUIRE(x && gamma && beta && y && geom_ok(gx) && geom_ok(gy) && batch > 0, "layernorm_forward: null argument or bad geometry");
    API_PREC("layernorm_forward");
    PBuf bx, by;
    if ((rc = bx.alloc(*gx, batch, x3, s)) || (rc = by.alloc(*gy, batch, x3, s))) return rc;
    if ((rc = mf_rows_from_f32(x, nullptr, bx.view(*gx), batch, s))) return rc;
    if ((rc = mf_layernorm(bx.view(*gx), by.view(*gy), gamma, beta, eps, batch, s, tokens, act))) return rc;
    if ((rc = mf_rows_to_f32(by.view(*gy), y, batch, s))) return rc;
    if ((rc = by.full(y_full, s))) return rc;
    MF_HIP(hipStreamSynchronize(s));
    return MF_OK;
}

extern "C" int mf_softmax_rows_forward(const float* scores, float* probs, const mf_rows_geom* gs, const mf_rows_geom* gp, int batch, int n_keys,
                                       float scale, int precision, float* y_full, void* stream) {
    MF_REQUIRE(scores && probs && geom_ok(gs) && geom_ok(gp) && batch > 0, "softmax_rows_forward: null argument or bad geometry");
    API_PREC("softmax_rows_forward");
    PBuf bs, bp;
    if ((rc = bs.alloc(*gs, batch, x3, s)) || (rc = bp.alloc(*gp, batch, x3, s))) return rc;
    if ((rc = mf_rows_from_f32(scores, nullptr, bs.view(*gs), batch, s))) return rc;
    if ((rc = mf_softmax_rows(bs.view(*gs), bp.view(*gp), n_keys, scale, batch, s))) return rc;
    if ((rc = mf_rows_to_f32(bp.view(*gp), probs, batch, s))) return rc;
    if ((rc = bp.full(y_full, s))) return rc;
    MF_HIP(hipStreamSynchronize(s));
    return MF_OK;
}

extern "C" int mf_groupnorm_forward(const float* x, const float* gamma, const float* beta, float* y, const mf_rows_geom* gx, const mf_rows_geom* gy,
                                    int batch, int groups, float eps, int silu, int have_stats, double* stats, float* scale, float* shift,
                                    int precision, float* y_full, void* stream) {
    MF_REQUIRE(x && gamma && beta && y && geom_ok(gx) && geom_ok(gy) && batch > 0 && groups > 0, "groupnorm_forward: null argument or bad geometry");
    MF_REQUIRE(!have_stats || stats, "groupnorm_forward: have_stats needs the statistics");
    MF_REQUIRE((scale == nullptr) == (shift == nullptr), "groupnorm_forward: scale and shift come together");
    API_PREC("groupnorm_forward");
    PBuf bx, by;
    DevMem own;
    const int ns = batch * groups * 2;
    if ((rc = own.alloc((size_t)ns * 2 * sizeof(double)))) return rc;
    double* st = stats ? stats : (double*)own.p;
    double* st2 = (double*)own.p + ns;           // mf_groupnorm_affine's own statistics
    if ((rc = bx.alloc(*gx, batch, x3, s)) || (rc = by.alloc(*gy, batch, x3, s))) return rc;
    if ((rc = mf_rows_from_f32(x, nullptr, bx.view(*gx), batch, s))) return rc;
    if (!have_stats && (rc = mf_zero_f64(st, ns, s))) return rc;
    if ((rc = mf_groupnorm(bx.view(*gx), by.view(*gy), gamma, beta, groups, eps, silu != 0, st, batch, s, have_stats != 0))) return rc;
    if (scale) {
        if (have_stats) MF_HIP(hipMemcpyAsync(st2, st, (size_t)ns * sizeof(double), hipMemcpyDeviceToDevice, s));
        else if ((rc = mf_zero_f64(st2, ns, s))) return rc;
        if ((rc = mf_groupnorm_affine(bx.view(*gx), gamma, beta, groups, eps, st2, scale, shift, batch, s, have_stats != 0))) return rc;
    }
    if ((rc = mf_rows_to_f32(by.view(*gy), y, batch, s))) return rc;
    if ((rc = by.full(y_full, s))) return rc;
    MF_HIP(hipStreamSynchronize(s));
    return MF_OK;
}

extern "C" int mf_gemm_bt_forward(const float* a, const float* b, float* out, int t, int n, int k, int b_rows, int b_cols, int64_t stride_n,
                                  int64_t stride_k, int pack_n, int pack_k, int precision, float* y_full, void* stream) {
    MF_REQUIRE(a && b && out && t > 0 && n > 0 && k > 0 && b_rows > 0 && b_cols > 0, "gemm_bt_forward: null argument or empty shape");
    MF_REQUIRE(pack_n > 0 && pack_n <= n && pack_k > 0 && pack_k <= k, "gemm_bt_forward: packs %d x %d of a %d x %d operand", pack_n, pack_k, n, k);
    MF_REQUIRE(stride_n >= 0 && stride_k >= 0 && (int64_t)(pack_n - 1) * stride_n + (int64_t)(pack_k - 1) * stride_k < (int64_t)b_rows * b_cols,
               "gemm_bt_forward: the strides leave the %d x %d source", b_rows, b_cols);
    API_PREC("gemm_bt_forward");
    // token sequences as the Whisper encoder holds them: one row, halo 1
    PBuf ba, bb, bo;
    const int n8 = (n + 7) / 8 * 8;
    if ((rc = ba.alloc(k, 1, t, 1, 1, x3, s)) || (rc = bb.alloc(b_cols, 1, b_rows, 0, 1, x3, s)) || (rc = bo.alloc(n8, 1, t, 1, 1, x3, s))) return rc;
    PlanGuard pg;
    if ((rc = mf_gemm_plan_create(&pg.p, k, n, t, precision))) return rc;
    if ((rc = mf_conv_bind(&pg.p, ba.b))) return rc;
    if ((rc = mf_rows_from_f32(a, nullptr, ba.all(), 1, s))) return rc;
    if ((rc = mf_rows_from_f32(b, nullptr, bb.all(), 1, s))) return rc;
    // a first pack of the whole operand when the call asks for a smaller one: the entries the second pack leaves out must come back zero
    if ((pack_n < n || pack_k < k) && (rc = mf_pack_b(&pg.p, bb.b.hi, bb.b.lo, stride_n, stride_k, n, k, s))) return rc;
    if ((rc = mf_pack_b(&pg.p, bb.b.hi, bb.b.lo, stride_n, stride_k, pack_n, pack_k, s))) return rc;
    if ((rc = mf_conv_launch(&pg.p, ba.all(), ActView{&bo.b, 0, n}, ActView{}, 1, s))) return rc;
    if ((rc = mf_rows_to_f32(ActView{&bo.b, 0, n}, out, 1, s))) return rc;
    if ((rc = bo.full(y_full, s))) return rc;
    MF_HIP(hipStreamSynchronize(s));
    return MF_OK;
}

extern "C" int mf_vae_post_u8_forward(const float* x, uint8_t* dst, const mf_rows_geom* gx, int batch, int precision, void* stream) {
    MF_REQUIRE(x && dst && geom_ok(gx) && batch > 0, "vae_post_u8_forward: null argument or bad geometry");
    API_PREC("vae_post_u8_forward");
    PBuf bx;
    if ((rc = bx.alloc(*gx, batch, x3, s))) return rc;
    if ((rc = mf_rows_from_f32(x, nullptr, bx.view(*gx), batch, s))) return rc;
    if ((rc = mf_vae_post_u8(bx.view(*gx), dst, batch, s))) return rc;
    MF_HIP(hipStreamSynchronize(s));
    return MF_OK;
}

// ---- the Wav2Lip and VAE edge kernels of mf_aux.hip: uint8 in, head out ------------------------------------------------------------------------------
// The uint8 producers write whole 8-channel pixels of a buffer of their own, so nothing is loaded first: the buffer is poisoned for batch + 1 items, the
// kernel fills the interior of the first `batch`, and y_full takes all of it back with the allocation's tail -- halo ring, the item behind the batch and
// the tail must still be the poison.
namespace {
int u8_planes_args(const char* name, const void* src, int H, int W, int halo, int batch, const float* y_full) {
    MF_REQUIRE(src && y_full, "%s: null argument", name);
    MF_REQUIRE(H > 0 && W > 0 && halo >= 0 && batch > 0, "%s: H=%d W=%d halo=%d batch=%d", name, H, W, halo, batch);
    MF_REQUIRE(((int64_t)batch + 1) * (H + 2 * halo) * (W + 2 * halo) * 8 < (int64_t)1 << 31, "%s: %d + 1 items of %d x %d (halo %d) reach 2^31 elements", name, batch, H, W, halo);
    return MF_OK;
}
}  // namespace

extern "C" int mf_faces_u8_forward(const uint8_t* faces, const int* rows, int n_pool, int H, int W, int halo, int batch, int precision, float* y_full, void* stream) {
    int rc;
    if ((rc = u8_planes_args("faces_u8_forward", faces, H, W, halo, batch, y_full))) return rc;
    if (rows) {
        MF_REQUIRE(n_pool > 0, "faces_u8_forward: a row table needs a pool, got n_pool=%d", n_pool);
        for (int i = 0; i < batch; ++i)
            MF_REQUIRE(rows[i] >= 0 && rows[i] < n_pool, "faces_u8_forward: rows[%d] = %d is outside the pool of %d faces", i, rows[i], n_pool);
    }
    MF_REQUIRE(precision == MF_PREC_BF16 || precision == MF_PREC_BF16X3, "faces_u8_forward: unknown precision %d", precision);
    hipStream_t s = (hipStream_t)stream;
    PBuf b;
    if ((rc = b.alloc(8, H, W, halo, batch + 1, precision == MF_PREC_BF16X3, s))) return rc;
    if ((rc = rows ? mf_faces_u8_rows_to_act(faces, rows, b.b, batch, s) : mf_faces_u8_to_act(faces, b.b, batch, s))) return rc;
    if ((rc = b.full(y_full, s, 64))) return rc;
    MF_HIP(hipStreamSynchronize(s));
    return MF_OK;
}

extern "C" int mf_vae_image_u8_forward(const uint8_t* img, int H, int W, int halo, int half_mask, int batch, int precision, float* y_full, void* stream) {
    int rc;
    if ((rc = u8_planes_args("vae_image_u8_forward", img, H, W, halo, batch, y_full))) return rc;
    MF_REQUIRE(half_mask == 0 || half_mask == 1, "vae_image_u8_forward: half_mask is 0 or 1, got %d", half_mask);
    MF_REQUIRE(precision == MF_PREC_BF16 || precision == MF_PREC_BF16X3, "vae_image_u8_forward: unknown precision %d", precision);
    hipStream_t s = (hipStream_t)stream;
    PBuf b;
    if ((rc = b.alloc(8, H, W, halo, batch + 1, precision == MF_PREC_BF16X3, s))) return rc;
    if ((rc = mf_vae_image_u8_to_act(img, b.b, half_mask, batch, s))) return rc;
    if ((rc = b.full(y_full, s, 64))) return rc;
    MF_HIP(hipStreamSynchronize(s));
    return MF_OK;
}

extern "C" int mf_head_sigmoid_forward(const float* x, const mf_rows_geom* g, const float* w, const float* b, int hwc255, float* out, int batch, int precision,
                                       void* stream) {
    MF_REQUIRE(x && w && b && out && geom_ok(g) && batch > 0, "head_sigmoid_forward: null argument or bad geometry");
    MF_REQUIRE(g->c == 32 && g->coff % 8 == 0 && g->cbuf % 8 == 0, "head_sigmoid_forward: the head reads 32 channels in 8-channel groups, got c=%d coff=%d cbuf=%d", g->c,
               g->coff, g->cbuf);
    MF_REQUIRE(hwc255 == 0 || hwc255 == 1, "head_sigmoid_forward: hwc255 is 0 or 1, got %d", hwc255);
    API_PREC("head_sigmoid_forward");
    PBuf bx;
    if ((rc = bx.alloc(*g, batch, x3, s))) return rc;
    if ((rc = mf_rows_from_f32(x, nullptr, bx.view(*g), batch, s))) return rc;
    if ((rc = mf_head_1x1_sigmoid(bx.view(*g), w, b, out, hwc255, batch, s))) return rc;
    MF_HIP(hipStreamSynchronize(s));
    return MF_OK;
}

extern "C" int mf_attention_composite_forward(const float* q, const float* k, const float* v, float* out, int batch, int tq, int tk, int heads,
                                              int head_dim, int precision, float* y_full, void* stream) {
    MF_REQUIRE(q && k && v && out, "attention_composite_forward: null argument");
    MF_REQUIRE(batch > 0 && tq > 0 && tk > 0 && heads > 0, "attention_composite_forward: batch=%d tq=%d tk=%d heads=%d", batch, tq, tk, heads);
    MF_REQUIRE(head_dim > 0 && head_dim % 8 == 0, "attention_composite_forward: head_dim %d is not a multiple of 8", head_dim);
    API_PREC("attention_composite_forward");
    const int C = heads * head_dim, tk8 = (tk + 7) / 8 * 8, tk64 = (tk + 63) / 64 * 64;
    PBuf bq, bk, bv, bo, sc, pm;
    if ((rc = bq.alloc(C, 1, tq, 0, batch, x3, s)) || (rc = bk.alloc(C, 1, tk, 0, batch, x3, s)) || (rc = bv.alloc(C, 1, tk, 0, batch, x3, s)) ||
        (rc = bo.alloc(C, 1, tq, 0, batch, x3, s)) || (rc = sc.alloc(tk8, heads, tq, 0, batch, x3, s)) || (rc = pm.alloc(tk64, heads, tq, 0, batch, x3, s)))
        return rc;
    PlanGuard ps, pv;
    if ((rc = mf_attention_composite_plans(&ps.p, &pv.p, head_dim, tq, tk, batch * heads, precision))) return rc;
    if ((rc = mf_rows_from_f32(q, nullptr, bq.all(), batch, s))) return rc;
    if ((rc = mf_rows_from_f32(k, nullptr, bk.all(), batch, s))) return rc;
    if ((rc = mf_rows_from_f32(v, nullptr, bv.all(), batch, s))) return rc;
    if ((rc = mf_attention_composite(&ps.p, &pv.p, &sc.b, &pm.b, bq.all(), bk.all(), bv.all(), bo.all(), heads, batch, precision, s))) return rc;
    if ((rc = mf_rows_to_f32(bo.all(), out, batch, s))) return rc;
    if ((rc = bo.full(y_full, s))) return rc;
    MF_HIP(hipStreamSynchronize(s));
    return MF_OK;
}

// The fused attention on views, as the model builders launch it: q | k | v slices of one packed buffer (self-attention), q alone beside a shared k | v
// buffer (cross-attention), or three buffers; every buffer poisoned before its views are loaded, so the four row pitches, offsets and batch strides differ
// wherever the geometries do.
extern "C" int mf_attention_view_forward(const float* q, const float* k, const float* v, float* out, const mf_rows_geom* gq, const mf_rows_geom* gk,
                                         const mf_rows_geom* gv, const mf_rows_geom* go, int packing, int batch, int heads, int tq, int tk, int precision,
                                         float* y_full, void* stream) {
    MF_REQUIRE(q && k && v && out && geom_ok(gq) && geom_ok(gk) && geom_ok(gv) && geom_ok(go) && batch > 0 && heads > 0,
               "attention_view_forward: null argument or bad geometry");
    MF_REQUIRE(packing >= 0 && packing <= 2, "attention_view_forward: packing %d (0: three buffers, 1: q alone, k and v share one, 2: one buffer)", packing);
    MF_REQUIRE(packing == 0 || same_buffer(gk, gv), "attention_view_forward: k and v share a buffer, their geometries must name the same one");
    MF_REQUIRE(packing != 2 || same_buffer(gq, gk), "attention_view_forward: q, k and v share a buffer (Tq == Tk), their geometries must name the same one");
    auto apart = [](const mf_rows_geom* a, const mf_rows_geom* b) { return a->coff + a->c <= b->coff || b->coff + b->c <= a->coff; };
    MF_REQUIRE(packing == 0 || apart(gk, gv), "attention_view_forward: the k and v views of one buffer overlap");
    MF_REQUIRE(packing != 2 || (apart(gq, gk) && apart(gq, gv)), "attention_view_forward: the q view overlaps k or v");
    API_PREC("attention_view_forward");
    PBuf bq, bk, bv, bo;
    if ((rc = bq.alloc(*gq, batch, x3, s)) || (rc = bo.alloc(*go, batch, x3, s))) return rc;
    if (packing < 2 && (rc = bk.alloc(*gk, batch, x3, s))) return rc;
    if (packing < 1 && (rc = bv.alloc(*gv, batch, x3, s))) return rc;
    const PBuf& pk = packing == 2 ? bq : bk;
    const PBuf& pv = packing == 0 ? bv : pk;
    if ((rc = mf_rows_from_f32(q, nullptr, bq.view(*gq), batch, s))) return rc;
    if ((rc = mf_rows_from_f32(k, nullptr, pk.view(*gk), batch, s))) return rc;
    if ((rc = mf_rows_from_f32(v, nullptr, pv.view(*gv), batch, s))) return rc;
    if ((rc = mf_attention(bq.view(*gq), pk.view(*gk), pv.view(*gv), bo.view(*go), heads, batch, precision, s, tq, tk))) return rc;
    if ((rc = mf_rows_to_f32(bo.view(*go), out, batch, s))) return rc;
    if ((rc = bo.full(y_full, s))) return rc;
    MF_HIP(hipStreamSynchronize(s));
    return MF_OK;
}

// One mf_conv_plan_create layer (or `groups` of them, one per channel group, as mf_wav2vec2::body launches its positional convolution) through
// mf_conv_launch on views: the input in a view of a buffer whose other channels are poisoned and whose halo ring is zero, the output in a view of a fully
// poisoned buffer, the residual in a view of a third buffer -- or, with desc->residual set and no gr, the input's own view.
extern "C" int mf_conv_view_forward(const mf_conv2d_desc* desc, const float* weight, const float* bias, const float* x, const float* res, float* y,
                                    const mf_rows_geom* gx, const mf_rows_geom* gy, const mf_rows_geom* gr, int batch, int tokens, int groups,
                                    int only_group, const int* pin, int* info, int precision, float* y_full, void* stream) {
    MF_REQUIRE(desc && weight && x && y && geom_ok(gx) && geom_ok(gy) && batch > 0, "conv_view_forward: null argument or bad geometry");
    MF_REQUIRE(groups > 0 && only_group >= -1 && only_group < groups, "conv_view_forward: group %d of %d", only_group, groups);
    MF_REQUIRE((res != nullptr) == (gr != nullptr) && (!gr || geom_ok(gr)), "conv_view_forward: the residual and its geometry come together");
    MF_REQUIRE(!gr || desc->residual, "conv_view_forward: a residual operand needs desc->residual 1 (before the activation) or 2 (after it)");
    const int n_out = desc->act == 5 ? desc->cout / 2 : desc->cout;
    MF_REQUIRE(gx->c % groups == 0 && gy->c == groups * n_out && (!gr || gr->c == gy->c),
               "conv_view_forward: views of %d (in), %d (out) channels for %d groups of %d output channels", gx->c, gy->c, groups, n_out);
    API_PREC("conv_view_forward");
    const int gci = gx->c / groups;
    PBuf bx, by, br;
    if ((rc = bx.alloc(*gx, batch, x3, s)) || (rc = zero_ring(bx, s)) || (rc = by.alloc(*gy, batch, x3, s))) return rc;
    if (gr && (rc = br.alloc(*gr, batch, x3, s))) return rc;
    if ((rc = mf_rows_from_f32(x, nullptr, bx.view(*gx), batch, s))) return rc;
    if (gr && (rc = mf_rows_from_f32(res, nullptr, br.view(*gr), batch, s))) return rc;
    const size_t wsz = (size_t)desc->cout * desc->cin * desc->kh * desc->kw;
    bool reported = false;
    for (int g = 0; g < groups; ++g) {
        if (only_group >= 0 && g != only_group) continue;
        PlanGuard pg;
        if ((rc = mf_conv_plan_create(&pg.p, *desc, weight + g * wsz, bias ? bias + (size_t)g * desc->cout : nullptr, nullptr, nullptr, nullptr, nullptr, precision)))
            return rc;
        if ((rc = mf_conv_bind(&pg.p, bx.b))) return rc;
        if (pin && (pin[0] || pin[1] || pin[2] || pin[3] || pin[4] || pin[5]) &&
            (rc = mf_conv_pin(&pg.p, batch, ConvTuned{ConvTile{pin[0], pin[1], pin[2], pin[3], pin[4]}, pin[5]})))
            return rc;
        const ActView in{&bx.b, gx->coff + g * gci, gci}, out{&by.b, gy->coff + g * n_out, n_out};
        ActView r{};
        if (gr) r = ActView{&br.b, gr->coff + g * n_out, n_out};
        else if (desc->residual) r = ActView{&bx.b, in.coff, n_out};
        if ((rc = mf_conv_launch(&pg.p, in, out, r, batch, s, tokens))) return rc;
        if (info && !reported) {
            ConvLaunchCfg c;
            if ((rc = mf_conv_resolve(&pg.p, batch, tokens, 0, &c))) return rc;
            const int v[11] = {c.family, c.tile.bm, c.tile.bn, c.tile.wgm, c.tile.wgn, c.tile.nsplit, c.ld, c.bk, c.nphase, c.stats, c.pinned ? 1 : 0};
            for (int i = 0; i < 11; ++i) info[i] = v[i];
            reported = true;
        }
        MF_HIP(hipStreamSynchronize(s));          // the plan (weights, split-K workspace) goes away with this iteration
    }
    if ((rc = mf_rows_to_f32(by.view(*gy), y, batch, s))) return rc;
    if ((rc = by.full(y_full, s))) return rc;
    MF_HIP(hipStreamSynchronize(s));
    return MF_OK;
}

extern "C" int mf_act_q_encode(const float* x, const mf_rows_geom* gx, int batch, int dst_c, int dst_halo, int mode, int silu, const float* scale, const float* shift,
                               const float* post, const float* gamma, const float* beta, int groups, float eps, uint16_t* dst_hi, uint16_t* dst_lo, float* src_full,
                               void* stream) {
    MF_REQUIRE(x && dst_hi && dst_lo && geom_ok(gx) && batch > 0, "act_q_encode: null argument or bad geometry");
    MF_REQUIRE(mode >= 0 && mode <= 3, "act_q_encode: unknown mode %d", mode);
    MF_REQUIRE(dst_halo >= 0 && dst_c >= gx->c && dst_c % 32 == 0, "act_q_encode: a destination of %d channels (halo %d) for %d", dst_c, dst_halo, gx->c);
    MF_REQUIRE(mode == 0 || (dst_c == gx->c && gx->coff % 8 == 0 && gx->cbuf % 8 == 0), "act_q_encode: the producers write whole 32-channel blocks of a slice at a multiple of 8");
    MF_REQUIRE(mode != 1 || (scale && shift), "act_q_encode: mode 1 takes scale and shift");
    MF_REQUIRE(mode < 2 || (gamma && beta && groups > 0 && groups <= 64 && gx->c % groups == 0), "act_q_encode: the GroupNorm modes take gamma, beta and a group count that divides C");
    MF_REQUIRE((int64_t)batch * ((int64_t)(gx->h + 2 * gx->halo) * (gx->w + 2 * gx->halo) * gx->cbuf) < ((int64_t)1 << 31) &&
               (int64_t)batch * ((int64_t)(gx->h + 2 * dst_halo) * (gx->w + 2 * dst_halo) * dst_c) < ((int64_t)1 << 31), "act_q_encode: tensors of 2^31 elements or more");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    PBuf bx, bq;
    DevMem rows, aff;
    if ((rc = bq.alloc(dst_c, gx->h, gx->w, dst_halo, batch, true, s))) return rc;
    if (mode == 0) {
        if ((rc = mf_nchw_to_act_q(x, gx->c, bq.b, batch, s))) return rc;
    } else {
        const int P = gx->h * gx->w, ns = batch * groups * 2;
        const int64_t total = (int64_t)batch * P * gx->c;
        if ((rc = bx.alloc(*gx, batch, true, s)) || (rc = rows.alloc((size_t)total * sizeof(float)))) return rc;
        hipLaunchKernelGGL(k_nchw_to_rows_f32, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, (float*)rows.p, gx->c, P, total);
        MF_HIP(hipGetLastError());
        if ((rc = mf_rows_from_f32((const float*)rows.p, nullptr, bx.view(*gx), batch, s))) return rc;
        if (mode == 1) {
            if ((rc = mf_affine_silu_to_act_q(bx.view(*gx), scale, shift, silu, bq.b, batch, s, post))) return rc;
        } else {
            // the statistics and the [batch][C] affine arrays a network keeps next to its activations (mf_musetalk.hip gn_silu_to_q)
            if ((rc = aff.alloc((size_t)ns * sizeof(double) + (size_t)2 * batch * gx->c * sizeof(float)))) return rc;
            double* st = (double*)aff.p;
            float* sc = (float*)(st + ns);
            float* sh = sc + (size_t)batch * gx->c;
            if ((rc = mf_zero_f64(st, ns, s))) return rc;
            if (mode == 2) {
                if ((rc = mf_groupnorm_stats(bx.view(*gx), groups, st, batch, s))) return rc;
                if ((rc = mf_affine_silu_to_act_q(bx.view(*gx), sc, sh, 1, bq.b, batch, s, post, st, gamma, beta, groups, eps))) return rc;
            } else {
                if ((rc = mf_groupnorm_affine(bx.view(*gx), gamma, beta, groups, eps, st, sc, sh, batch, s, false))) return rc;
                if ((rc = mf_affine_silu_to_act_q(bx.view(*gx), sc, sh, 1, bq.b, batch, s, post))) return rc;
            }
        }
        if ((rc = bx.full(src_full, s, 64))) return rc;
    }
    MF_HIP(hipMemcpyAsync(dst_hi, bq.b.hi, (size_t)(bq.n + 64) * sizeof(bf16_t), hipMemcpyDeviceToDevice, s));
    MF_HIP(hipMemcpyAsync(dst_lo, bq.b.lo, (size_t)(bq.n + 64) * sizeof(bf16_t), hipMemcpyDeviceToDevice, s));
    MF_HIP(hipStreamSynchronize(s));
    return MF_OK;
}
