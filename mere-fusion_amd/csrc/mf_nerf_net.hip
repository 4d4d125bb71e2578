// ER-NeRF field and torso handles on gfx950 (mf_nerf_field_*, mf_nerf_density_grid_update, mf_nerf_torso_*): weights, buffers and the PER-LAYER route of both nets.
// By default a handle runs its net as one kernel (mf_nerf_fused.hip, mf_nerf_torso.hip, through mf_nerf_host.h); the route here -- every Linear a launch -- stays for
// A/B and as the tests' independent cross-check (MF_NERF_FIELD=gemm, MF_TORSO=gemm).  The head render loop over a field is mf_nerf_head.hip.
//
// The radiance field: tri-plane hash-grid features -> audio / eye attention -> sigma MLP -> colour MLP.
// Replaces `NeRFNetwork.forward` + `density` + `encode_x` (reference: ernerf/nerf_triplane/network.py:204-219, 249-308) for the
// inference call `self.forward(xyzs, dirs, enc_a, ind_code, eye)` of the render loop (renderer.py:260): per sample 36 grid
// features, SH(dir), and ten bias-free Linear layers (23 184 MACs).
//
// The reference runs ~10 tiny cuBLAS GEMMs plus cat / repeat / elementwise passes per loop iteration.  Here the samples are a
// token sequence ([M/1024] "images" of 1 x 1024 tokens) and every Linear is a 1x1 convolution on the MFMA implicit-GEMM kernel
// (mf_conv.hip) with its ReLU / sigmoid epilogue; the torch.cat calls disappear because producers write channel slices of the
// consumer's input buffer:
//     SI [72] = [ enc_x 36 | enc_a * aud_ch_att 32 | e * eye_att 1 | 0 0 0 ]        <- sigma_net input   (network.py:287-296)
//     CI [96] = [ h0 | geo_feat 64 | 0 x7 | SH 16 | ind_code 4 | 0 x4 ]             <- colour_net input  (network.py:262-269)
// sigma_net's last layer writes its 65 outputs straight into CI[0..64]; colour_net's weight columns are permuted to that layout
// (and zero on h0), so geo_feat is never copied.
#include "mf_nerf_host.h"
#include "mf_nerf_frame_batch.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

namespace {

constexpr int ENC = 36, AUD = 32, GEO = 64, SHD = 16;
constexpr int SI_C = 72, CI_C = 96, CI_SH = 72, CI_IND = 88;

__device__ __forceinline__ uint32_t qf2bf(float f) {
    return (uint32_t)__builtin_bit_cast(unsigned short, (__bf16)f);      // round to nearest even in hardware (v_cvt_pk_bf16_f32)
}
__device__ __forceinline__ float qbf2f(uint32_t h) { return __uint_as_float(h << 16); }
__device__ __forceinline__ void put(bf16_t* hi, bf16_t* lo, int64_t o, float v) {
    const uint32_t h = qf2bf(v);
    hi[o] = (bf16_t)h;
    if (lo) lo[o] = (bf16_t)qf2bf(v - qbf2f(h));
}
__device__ __forceinline__ float get(const bf16_t* hi, const bf16_t* lo, int64_t o) {
    float v = qbf2f(hi[o]);
    if (lo) v += qbf2f(lo[o]);
    return v;
}

// per sample: plane coordinates mapped to [0, 1] (grid.py:144 + network.py:204-208), SH basis of the view direction
// (shencoder.cu:50-68, degree 4) and the individual code into the colour-net input
__global__ __launch_bounds__(256) void k_nf_prep(const float* __restrict__ xyzs, const float* __restrict__ dirs, const float* __restrict__ ind,
                                                 int n_ind, float bound, int M, float* coords, bf16_t* ci_hi, bf16_t* ci_lo) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const float two_b = 2.f * bound;      // divided, as grid.py:144 does: a product with the rounded reciprocal differs by an ulp unless 2 bound is a power of two
    const float x = __fdiv_rn(xyzs[3 * m] + bound, two_b), y = __fdiv_rn(xyzs[3 * m + 1] + bound, two_b), z = __fdiv_rn(xyzs[3 * m + 2] + bound, two_b);
    float* cxy = coords + (size_t)m * 2;
    float* cyz = coords + (size_t)M * 2 + (size_t)m * 2;
    float* cxz = coords + (size_t)M * 4 + (size_t)m * 2;
    cxy[0] = x; cxy[1] = y;
    cyz[0] = y; cyz[1] = z;
    cxz[0] = x; cxz[1] = z;
    const float dx = dirs[3 * m], dy = dirs[3 * m + 1], dz = dirs[3 * m + 2];
    const float xy = dx * dy, xz = dx * dz, yz = dy * dz, x2 = dx * dx, y2 = dy * dy, z2 = dz * dz;
    float sh[SHD];
    sh[0] = 0.28209479177387814f;
    sh[1] = -0.48860251190291987f * dy; sh[2] = 0.48860251190291987f * dz; sh[3] = -0.48860251190291987f * dx;
    sh[4] = 1.0925484305920792f * xy; sh[5] = -1.0925484305920792f * yz; sh[6] = 0.94617469575755997f * z2 - 0.31539156525251999f;
    sh[7] = -1.0925484305920792f * xz; sh[8] = 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
    sh[9] = 0.59004358992664352f * dy * (-3.0f * x2 + y2); sh[10] = 2.8906114426405538f * xy * dz;
    sh[11] = 0.45704579946446572f * dy * (1.0f - 5.0f * z2); sh[12] = 0.3731763325901154f * dz * (5.0f * z2 - 3.0f);
    sh[13] = 0.45704579946446572f * dx * (1.0f - 5.0f * z2); sh[14] = 1.4453057213202769f * dz * (x2 - y2);
    sh[15] = 0.59004358992664352f * dx * (-x2 + 3.0f * y2);
    // 16 SH values + 8 individual-code slots per sample as 16-byte stores (CI_SH and CI_IND are multiples of 8 channels)
    const int64_t o = (int64_t)m * CI_C;
    float v[SHD + 8];
#pragma unroll
    for (int i = 0; i < SHD; ++i) v[i] = sh[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[SHD + i] = i < n_ind ? ind[i] : 0.f;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        uint32_t hb[8], lb[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { hb[e] = qf2bf(v[q * 8 + e]); lb[e] = qf2bf(v[q * 8 + e] - qbf2f(hb[e])); }
        const int64_t oo = o + (q < 2 ? CI_SH + q * 8 : CI_IND);
        *reinterpret_cast<uint4*>(ci_hi + oo) = make_uint4(hb[0] | (hb[1] << 16), hb[2] | (hb[3] << 16), hb[4] | (hb[5] << 16), hb[6] | (hb[7] << 16));
        if (ci_lo) *reinterpret_cast<uint4*>(ci_lo + oo) = make_uint4(lb[0] | (lb[1] << 16), lb[2] | (lb[3] << 16), lb[4] | (lb[5] << 16), lb[6] | (lb[7] << 16));
    }
}

// fp32 grid features [3][M][12] -> SI[m][0..35]
__global__ __launch_bounds__(256) void k_nf_pack(const float* __restrict__ enc, int M, bf16_t* si_hi, bf16_t* si_lo) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)M * ENC) return;
    const int m = (int)(idx / ENC), c = (int)(idx - (int64_t)m * ENC);
    const int plane = c / 12, l = c - plane * 12;
    put(si_hi, si_lo, (int64_t)m * SI_C + c, enc[((size_t)plane * M + m) * 12 + l]);
}

// enc_w = enc_a * aud_ch_att, e * eye_att into the sigma-net input; the two ambient outputs (network.py:284-306).
// One lane per (sample, audio channel): 32 lanes read / write one sample's 64 contiguous bytes, the norm is a 32-lane butterfly.
__global__ __launch_bounds__(256) void k_nf_mix(const bf16_t* __restrict__ a_hi, const bf16_t* __restrict__ a_lo, const bf16_t* __restrict__ e_hi,
                                                const bf16_t* __restrict__ e_lo, const float* __restrict__ enc_a, float eye, int has_eye, int M,
                                                bf16_t* si_hi, bf16_t* si_lo, float* amb_aud, float* amb_eye) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int m = (int)(idx >> 5), c = (int)(idx & 31);
    const bool live = m < M;
    const float a = live ? get(a_hi, a_lo, (int64_t)m * AUD + c) : 0.f;
    float n2 = a * a;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) n2 += __shfl_xor(n2, o, 32);
    if (!live) return;
    const int64_t so = (int64_t)m * SI_C + ENC;
    put(si_hi, si_lo, so + c, enc_a[c] * a);
    if (c < 4) {
        const float ea = has_eye ? get(e_hi, e_lo, (int64_t)m * 8) : 0.f;
        put(si_hi, si_lo, so + AUD + c, (c == 0 && has_eye) ? eye * ea : 0.f);
        if (c == 0) { amb_aud[m] = sqrtf(n2); amb_eye[m] = ea; }
    }
}

// sigma = exp(h0) (network.py:300), colour = sigmoid(.) * 1.002 - 0.001 (network.py:272; the sigmoid ran in the GEMM epilogue),
// uncertainty = log(1 + exp(0)) in test mode (network.py:240-246, 275)
__global__ __launch_bounds__(256) void k_nf_out(const bf16_t* __restrict__ ci_hi, const bf16_t* __restrict__ ci_lo, const bf16_t* __restrict__ c_hi,
                                                const bf16_t* __restrict__ c_lo, int M, float* sigmas, float* rgbs, float* unc) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    sigmas[m] = expf(get(ci_hi, ci_lo, (int64_t)m * CI_C));
#pragma unroll
    for (int k = 0; k < 3; ++k) rgbs[3 * m + k] = get(c_hi, c_lo, (int64_t)m * 8 + k) * (1.f + 2.f * 0.001f) - 0.001f;
    if (unc) unc[m] = 0.69314718055994530942f;
}

}  // namespace

static const mf_tensor* nf_find(const std::map<std::string, const mf_tensor*>& sd, const std::string& k, int64_t r, int64_t c) {
    auto it = sd.find(k);
    if (it == sd.end()) { mf_set_error("nerf_field_create: tensor '%s' missing", k.c_str()); return nullptr; }
    const mf_tensor* t = it->second;
    if (t->ndim != 2 || t->shape[0] != r || t->shape[1] != c) {
        mf_set_error("nerf_field_create: '%s' has shape [%lld, %lld], expected [%lld, %lld]", k.c_str(), (long long)t->shape[0],
                     (long long)(t->ndim > 1 ? t->shape[1] : 0), (long long)r, (long long)c);
        return nullptr;
    }
    return t;
}

extern "C" int mf_nerf_field_create(const mf_nerf_field_config* cfg, const mf_tensor* weights, int n_weights, int precision,
                                    int max_samples, mf_nerf_field** out) {
    MF_REQUIRE(cfg && weights && out && n_weights > 0 && max_samples > 0, "nerf_field_create: bad argument");
    MF_REQUIRE(precision == MF_PREC_BF16 || precision == MF_PREC_BF16X3, "nerf_field_create: unknown precision %d", precision);
    MF_REQUIRE(cfg->num_levels == 12 && cfg->level_dim == 1 && cfg->audio_dim == AUD && cfg->geo_feat_dim == GEO && cfg->hidden_dim == 64,
               "nerf_field_create: built for the reference's fixed field (12 levels x 1, audio 32, hidden 64, geo 64: network.py:122-143)");
    MF_REQUIRE(cfg->individual_dim >= 0 && cfg->individual_dim <= 8 && cfg->bound > 0, "nerf_field_create: individual_dim / bound");
    *out = nullptr;
    MfStateDict sd;
    int rc = mf_sd_build(weights, n_weights, "nerf_field_create", {}, &sd);
    if (rc) return rc;
    std::unique_ptr<mf_nerf_field> h(new mf_nerf_field());
    h->precision = precision;
    h->cfg = *cfg;
    h->cap_batches = (max_samples + TW - 1) / TW;
    const int n_emb = cfg->offsets[cfg->num_levels];
    const int eye = cfg->exp_eye ? 1 : 0, nind = cfg->individual_dim;
    const int sig_in = ENC + AUD + eye, col_in = SHD + GEO + nind;

    h->SI = h->seq(SI_C); h->CI = h->seq(CI_C); h->T1 = h->seq(64); h->AU = h->seq(AUD); h->T2 = h->seq(16); h->EY = h->seq(8);
    h->S1 = h->seq(64); h->S2 = h->seq(64); h->C1 = h->seq(64); h->RGB = h->seq(8);
    if ((rc = h->alloc())) return rc;
    const size_t cap = (size_t)h->cap_batches * TW;
    MF_HIP(hipMalloc(&h->coords, cap * 6 * sizeof(float))); h->dev.push_back(h->coords);
    MF_HIP(hipMalloc(&h->enc, cap * ENC * sizeof(float))); h->dev.push_back(h->enc);
    MF_HIP(hipMalloc(&h->d_enc_a, AUD * sizeof(float))); h->dev.push_back(h->d_enc_a);
    MF_HIP(hipMalloc(&h->d_ind, 8 * sizeof(float))); h->dev.push_back(h->d_ind);
    const char* planes[3] = {"encoder_xy.embeddings", "encoder_yz.embeddings", "encoder_xz.embeddings"};
    for (int p = 0; p < 3; ++p) {
        const mf_tensor* t = nf_find(sd, planes[p], n_emb, 1);
        if (!t) return MF_ERR_INVALID;
        MF_HIP(hipMalloc(&h->emb[p], (size_t)n_emb * sizeof(float))); h->dev.push_back(h->emb[p]);
        MF_HIP(hipMemcpy(h->emb[p], t->data, (size_t)n_emb * sizeof(float), hipMemcpyHostToDevice));
    }

    // Linear weights, re-laid onto the channel order of the buffers they read (zero columns for padding / unused channels)
    auto relay = [&](const char* name, int cout, int cin_ref, int cin_buf, const std::vector<int>& col_of, std::vector<float>& w) -> int {
        const mf_tensor* t = nf_find(sd, name, cout, cin_ref);
        if (!t) return MF_ERR_INVALID;
        const float* src = (const float*)t->data;
        w.assign((size_t)cout * cin_buf, 0.f);
        for (int o = 0; o < cout; ++o)
            for (int i = 0; i < cin_ref; ++i) w[(size_t)o * cin_buf + col_of[i]] = src[(size_t)o * cin_ref + i];
        return MF_OK;
    };
    auto iota = [](int n, int start = 0) { std::vector<int> v(n); for (int i = 0; i < n; ++i) v[i] = start + i; return v; };
    std::vector<float> w;
    if ((rc = relay("aud_ch_att_net.net.0.weight", 64, ENC, 40, iota(ENC), w)) || (rc = h->linear(&h->a1, w, 40, 64, 1, h->SI))) return rc;
    if ((rc = relay("aud_ch_att_net.net.1.weight", AUD, 64, 64, iota(64), w)) || (rc = h->linear(&h->a2, w, 64, AUD, 0, h->T1))) return rc;
    if (eye) {
        if ((rc = relay("eye_att_net.net.0.weight", 16, ENC, 40, iota(ENC), w)) || (rc = h->linear(&h->e1, w, 40, 16, 1, h->SI))) return rc;
        if ((rc = relay("eye_att_net.net.1.weight", 1, 16, 16, iota(16), w)) || (rc = h->linear(&h->e2, w, 16, 1, 2, h->T2))) return rc;
    }
    if ((rc = relay("sigma_net.net.0.weight", 64, sig_in, SI_C, iota(sig_in), w)) || (rc = h->linear(&h->s1, w, SI_C, 64, 1, h->SI))) return rc;
    if ((rc = relay("sigma_net.net.1.weight", 64, 64, 64, iota(64), w)) || (rc = h->linear(&h->s2, w, 64, 64, 1, h->S1))) return rc;
    if ((rc = relay("sigma_net.net.2.weight", 1 + GEO, 64, 64, iota(64), w)) || (rc = h->linear(&h->s3, w, 64, 1 + GEO, 0, h->S2))) return rc;
    {
        // colour-net input order in the reference: [SH 16 | geo 64 | ind] (network.py:265); in CI: geo at 1..64, SH at 72.., ind at 88..
        std::vector<int> col(col_in);
        for (int i = 0; i < SHD; ++i) col[i] = CI_SH + i;
        for (int i = 0; i < GEO; ++i) col[SHD + i] = 1 + i;
        for (int i = 0; i < nind; ++i) col[SHD + GEO + i] = CI_IND + i;
        if ((rc = relay("color_net.net.0.weight", 64, col_in, CI_C, col, w)) || (rc = h->linear(&h->c1, w, CI_C, 64, 1, h->CI))) return rc;
    }
    if ((rc = relay("color_net.net.1.weight", 3, 64, 64, iota(64), w)) || (rc = h->linear(&h->c2, w, 64, 3, 2, h->C1))) return rc;
    {
        const char* e = getenv("MF_NERF_FIELD");
        if (!(e && !strcmp(e, "gemm"))) {
            const char* names[9] = {"aud_ch_att_net.net.0.weight", "aud_ch_att_net.net.1.weight", "eye_att_net.net.0.weight", "eye_att_net.net.1.weight",
                                    "sigma_net.net.0.weight", "sigma_net.net.1.weight", "sigma_net.net.2.weight", "color_net.net.0.weight",
                                    "color_net.net.1.weight"};
            const float* w9[9];
            for (int i = 0; i < 9; ++i) {
                auto it = sd.find(names[i]);
                w9[i] = it == sd.end() ? nullptr : (const float*)it->second->data;   // shapes were checked by the relay() calls above
                MF_REQUIRE(w9[i] || ((i == 2 || i == 3) && !eye), "nerf_field_create: tensor '%s' missing", names[i]);
            }
            if ((rc = mf_nerf_fused_pack(w9, nind, eye != 0, precision == MF_PREC_BF16X3, &h->fused_w))) return rc;
            h->dev.push_back(h->fused_w);
        }
    }
    MF_HIP(hipDeviceSynchronize());
    *out = h.release();
    return MF_OK;
}

extern "C" int mf_nerf_density_grid_update(mf_nerf_field* h, float* density_grid, uint8_t* density_bitfield, int cascades, int grid_size, float bound,
                                           const float* enc_a, float eye, int use_eye, float density_scale, float decay, float density_thresh, const float* noise,
                                           float* tmp_grid, float* xyzs_out, double* mean_density, void* stream) {
    MF_REQUIRE(h && density_grid && density_bitfield && enc_a && tmp_grid && mean_density, "nerf_density_grid_update: null argument");
    MF_REQUIRE(h->fused_w, "nerf_density_grid_update: needs the fused field kernel (the field was created under MF_NERF_FIELD=gemm)");
    MF_REQUIRE(!use_eye || h->cfg.exp_eye, "nerf_density_grid_update: use_eye on a field created without exp_eye");
    size_t need = 0;
    int rc;
    if ((rc = mf_nerf_occupancy_shape("nerf_density_grid_update", cascades, grid_size, &need))) return rc;
    if (need > h->occ_cap) {
        // (first call for this size: the only allocation; a grown buffer leaves the old one to mf_nerf_field_destroy, which frees h->dev -- a launch may still read it)
        double* p = nullptr;
        MF_HIP(hipMalloc(&p, need * sizeof(double)));
        h->dev.push_back(p);
        h->occ_partials = p; h->occ_cap = need;
    }
    NerfFieldConsts f = h->consts();
    f.n_ind = 0; f.has_eye = use_eye ? 1 : 0;                                   // the density half: no individual code; the eye feature only when the caller feeds it
    return mf_nerf_occupancy_launch(f, NerfFrameInputs{enc_a, nullptr, eye, nullptr, density_scale},
                                    NerfGridBufs{density_grid, density_bitfield, tmp_grid, xyzs_out, mean_density, h->occ_partials}, cascades, grid_size, bound, decay,
                                    density_thresh, noise, (hipStream_t)stream);
}

extern "C" int mf_nerf_field_forward(mf_nerf_field* h, const float* xyzs, const float* dirs, const float* enc_a, const float* ind_code,
                                     float eye, int n_samples, float* sigmas, float* rgbs, float* amb_aud, float* amb_eye,
                                     float* uncertainty, void* stream) {
    MF_REQUIRE(h && xyzs && dirs && enc_a && sigmas && rgbs && amb_aud && amb_eye, "nerf_field_forward: null argument");
    MF_REQUIRE(n_samples >= 0 && n_samples <= h->cap_batches * TW, "nerf_field_forward: %d samples exceed the capacity %d", n_samples,
               h->cap_batches * TW);
    MF_REQUIRE(h->cfg.individual_dim == 0 || ind_code, "nerf_field_forward: the field was built with an individual code");
    if (n_samples == 0) return MF_OK;
    hipStream_t s = (hipStream_t)stream;
    const int M = n_samples, nb = (M + TW - 1) / TW, gb = (M + 255) / 256;
    const bool x3 = h->precision == MF_PREC_BF16X3;
    const mf_nerf_field_config& c = h->cfg;
    if (h->fused_w)
        return mf_nerf_fused_launch(h->consts(), NerfFrameInputs{enc_a, ind_code, eye, nullptr, 1.f}, xyzs, dirs, M, NerfFieldOut{sigmas, rgbs, amb_aud, amb_eye, uncertainty}, s);
    MF_HIP(hipMemcpyAsync(h->d_enc_a, enc_a, AUD * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (c.individual_dim) MF_HIP(hipMemcpyAsync(h->d_ind, ind_code, c.individual_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_nf_prep, dim3(gb), dim3(256), 0, s, xyzs, dirs, h->d_ind, c.individual_dim, c.bound, M, h->coords, h->CI->hi, h->CI->lo);
    MF_HIP(hipGetLastError());
    int rc;
    for (int p = 0; p < 3; ++p)
        if ((rc = mf_grid_encode_forward(h->coords + (size_t)p * M * 2, h->emb[p], c.offsets, h->enc + (size_t)p * M * 12, M, 2, 1, 12,
                                         c.log2_per_level_scale, c.base_resolution, 0, 0, 1, stream)))
            return rc;
    hipLaunchKernelGGL(k_nf_pack, dim3((unsigned)(((int64_t)M * ENC + 255) / 256)), dim3(256), 0, s, h->enc, M, h->SI->hi, h->SI->lo);
    MF_HIP(hipGetLastError());
    auto V = [](ActBuf* b, int coff, int C) { return ActView{b, coff, C}; };
    if ((rc = mf_conv_launch(h->a1, V(h->SI, 0, 40), V(h->T1, 0, 64), ActView{}, nb, s))) return rc;
    if ((rc = mf_conv_launch(h->a2, V(h->T1, 0, 64), V(h->AU, 0, AUD), ActView{}, nb, s))) return rc;
    if (c.exp_eye) {
        if ((rc = mf_conv_launch(h->e1, V(h->SI, 0, 40), V(h->T2, 0, 16), ActView{}, nb, s))) return rc;
        if ((rc = mf_conv_launch(h->e2, V(h->T2, 0, 16), V(h->EY, 0, 1), ActView{}, nb, s))) return rc;
    }
    hipLaunchKernelGGL(k_nf_mix, dim3((unsigned)(((int64_t)M * 32 + 255) / 256)), dim3(256), 0, s, h->AU->hi, h->AU->lo, h->EY->hi, h->EY->lo, h->d_enc_a, eye, c.exp_eye, M, h->SI->hi,
                       h->SI->lo, amb_aud, amb_eye);
    MF_HIP(hipGetLastError());
    if ((rc = mf_conv_launch(h->s1, V(h->SI, 0, SI_C), V(h->S1, 0, 64), ActView{}, nb, s))) return rc;
    if ((rc = mf_conv_launch(h->s2, V(h->S1, 0, 64), V(h->S2, 0, 64), ActView{}, nb, s))) return rc;
    if ((rc = mf_conv_launch(h->s3, V(h->S2, 0, 64), V(h->CI, 0, 1 + GEO), ActView{}, nb, s))) return rc;
    if ((rc = mf_conv_launch(h->c1, V(h->CI, 0, CI_C), V(h->C1, 0, 64), ActView{}, nb, s))) return rc;
    if ((rc = mf_conv_launch(h->c2, V(h->C1, 0, 64), V(h->RGB, 0, 3), ActView{}, nb, s))) return rc;
    hipLaunchKernelGGL(k_nf_out, dim3(gb), dim3(256), 0, s, h->CI->hi, x3 ? h->CI->lo : nullptr, h->RGB->hi, x3 ? h->RGB->lo : nullptr, M, sigmas, rgbs,
                       uncertainty);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

extern "C" void mf_nerf_field_destroy(mf_nerf_field* h) { delete h; }

// =========================================================================================================================
// Torso branch: `run_torso` (renderer.py:294-352) + `forward_torso` (network.py:166-201).
//
// The reference gathers the pixels whose torso occupancy exceeds a threshold (boolean mask -> host sync), runs the deform and
// colour MLPs on them and scatters back.  Here every pixel goes through the (cheap: 8.6 kMAC) nets and the mask is applied in the
// final mix, so there is no compaction and no sync.  The per-frame constant part of the MLP inputs -- the frequency-encoded
// wrapped anchors (42) and the individual code (8) -- never becomes a channel: it is folded into a per-frame BIAS of the first
// layer of each MLP (W[:, const columns] . const), written into the plans' bias arrays before the launch.
//     TX [40] = [ freq(x, 8) 34 | 0 x6 ]                         <- deform-net input (+ bias)     (network.py:177-185)
//     TH [72] = [ tiled-grid(x + dx) 32 | freq(x, 8) 34 | 0 x6 ] <- torso-net input (+ bias)     (network.py:189-196)
// =========================================================================================================================
namespace {

constexpr int TX_C = 40, TH_C = 72, FQ = 34, TG = 32, NCONST = 50;

// x = bg_coords * shrink; FreqEncoder(2, 8) (freqencoder.cu:30-58, with the accurate sinf) into TX[0..33] and TH[32..65]
__global__ __launch_bounds__(256) void k_torso_prep(const float* __restrict__ bg_coords, float shrink, int N, float* xs, bf16_t* tx_hi, bf16_t* tx_lo,
                                                    bf16_t* th_hi, bf16_t* th_lo) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int n = (int)(idx / TX_C), c = (int)(idx - (int64_t)n * TX_C);
    if (n >= N) return;
    float v = 0.f;
    if (c < FQ) {
        if (c < 2) {
            v = bg_coords[2 * n + c] * shrink;
            xs[2 * n + c] = v;
        } else {
            const int col = c / 2 - 1, d = c & 1, freq = col >> 1;
            v = sinf(scalbnf(bg_coords[2 * n + d] * shrink, freq) + (float)(col & 1) * 1.57079632679489661923f);
        }
        put(th_hi, th_lo, (int64_t)n * TH_C + TG + c, v);
    } else {
        put(th_hi, th_lo, (int64_t)n * TH_C + TG + c, 0.f);      // TH[66..71]
    }
    put(tx_hi, tx_lo, (int64_t)n * TX_C + c, v);
}

// x2 = clamp(x + dx, -1, 1) (network.py:187), mapped to [0, 1] for the tiled grid (grid.py:144, bound 1)
__global__ __launch_bounds__(256) void k_torso_warp(const float* __restrict__ xs, const bf16_t* __restrict__ d_hi, const bf16_t* __restrict__ d_lo, int N,
                                                    float* coords01, float* deform) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float dx = get(d_hi, d_lo, (int64_t)n * 8 + k);
        const float x2 = fminf(fmaxf(xs[2 * n + k] + dx, -1.f), 1.f);
        coords01[2 * n + k] = (x2 + 1.f) * 0.5f;
        if (deform) deform[2 * n + k] = dx;
    }
}

__global__ __launch_bounds__(256) void k_torso_pack(const float* __restrict__ feat, int N, bf16_t* th_hi, bf16_t* th_lo) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)N * TG) return;
    const int n = (int)(idx / TG), c = (int)(idx - (int64_t)n * TG);
    put(th_hi, th_lo, (int64_t)n * TH_C + c, feat[idx]);
}

// occupancy = grid_sample(density_grid_torso, bg_coords, align_corners=True) (renderer.py:326), mask = occupancy > thresh;
// alpha / colour = sigmoid(.) * 1.002 - 0.001 (network.py:198-199, the sigmoid ran in the GEMM epilogue);
// bg = colour * alpha + bg * (1 - alpha) (renderer.py:343)
__global__ __launch_bounds__(256) void k_torso_mix(const float* __restrict__ bg_coords, const float* __restrict__ density, int G, float thresh,
                                                   const bf16_t* __restrict__ o_hi, const bf16_t* __restrict__ o_lo, const float* __restrict__ bg,
                                                   int bg_per_ray, float bg_const, int N, float* out, float* alpha_out) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float gx = (bg_coords[2 * n] + 1.f) * 0.5f * (float)(G - 1), gy = (bg_coords[2 * n + 1] + 1.f) * 0.5f * (float)(G - 1);
    const float fx = floorf(gx), fy = floorf(gy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float wx = gx - fx, wy = gy - fy;
    auto at = [&](int y, int x) { return (x >= 0 && x < G && y >= 0 && y < G) ? density[y * G + x] : 0.f; };   // zeros padding
    const float occ = at(y0, x0) * (1 - wx) * (1 - wy) + at(y0, x0 + 1) * wx * (1 - wy) + at(y0 + 1, x0) * (1 - wx) * wy + at(y0 + 1, x0 + 1) * wx * wy;
    const bool m = occ > thresh;
    const float a = m ? get(o_hi, o_lo, (int64_t)n * 8) * 1.002f - 0.001f : 0.f;
    if (alpha_out) alpha_out[n] = a;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float col = m ? get(o_hi, o_lo, (int64_t)n * 8 + 1 + k) * 1.002f - 0.001f : 0.f;
        const float b = bg ? (bg_per_ray ? bg[3 * n + k] : bg[k]) : bg_const;
        out[3 * n + k] = col * a + b * (1.f - a);
    }
}

}  // namespace

struct mf_nerf_torso : TokenNet {
    mf_nerf_torso_config cfg{};
    ActBuf *TX = nullptr, *TH = nullptr, *D1 = nullptr, *D2 = nullptr, *DX = nullptr, *U1 = nullptr, *U2 = nullptr, *OUT = nullptr;
    ConvPlan *d1, *d2, *d3, *t1, *t2, *t3;
    float *emb = nullptr, *density = nullptr, *xs = nullptr, *coords01 = nullptr, *feat = nullptr;
    std::vector<float> wd_const, wt_const;     // [32][50]: the constant-input columns of the two first layers
    float* wf = nullptr;                       // fp32 [out][in] tables of the six layers for the fused kernel (mf_nerf_torso.hip)
    bool fused = true;
    const float* grid = nullptr;               // mf_nerf_torso_set_grid / _grid_update: the caller's density_grid_torso, borrowed; null = `density`, the copy of creation
    double* grid_partials = nullptr;           // per-workgroup sums of mf_nerf_torso_grid_update (grid_size^2 / 256 <= 64 at the sizes served)
    const float* sampled() const { return grid ? grid : density; }
    NerfTorsoConsts consts() const { return {wf, emb, cfg.offsets, cfg.log2_per_level_scale, cfg.base_resolution, cfg.torso_shrink, cfg.grid_size}; }
    void frame_bias(const float* frame_consts_host, float* bias) const;      // bias [64]: deform net | torso net
};

extern "C" int mf_nerf_torso_create(const mf_nerf_torso_config* cfg, const mf_tensor* weights, int n_weights, int precision, int max_pixels,
                                    mf_nerf_torso** out) {
    MF_REQUIRE(cfg && weights && out && n_weights > 0 && max_pixels > 0, "nerf_torso_create: bad argument");
    MF_REQUIRE(precision == MF_PREC_BF16 || precision == MF_PREC_BF16X3, "nerf_torso_create: unknown precision %d", precision);
    MF_REQUIRE(cfg->num_levels == 16 && cfg->level_dim == 2 && cfg->individual_dim >= 0 && cfg->individual_dim <= 8 && cfg->grid_size > 1,
               "nerf_torso_create: built for the reference's torso nets (tiled grid 16 x 2, ind_dim_torso <= 8: network.py:155-159)");
    *out = nullptr;
    MfStateDict sd;
    int rc = mf_sd_build(weights, n_weights, "nerf_torso_create", {}, &sd);
    if (rc) return rc;
    std::unique_ptr<mf_nerf_torso> h(new mf_nerf_torso());
    h->precision = precision;
    h->cfg = *cfg;
    h->cap_batches = (max_pixels + TW - 1) / TW;
    const int nind = cfg->individual_dim, ncst = 42 + nind;                 // anchors freq(6, 3) = 42 (network.py:151) + code
    const int din = FQ + ncst, tin = TG + FQ + ncst;
    h->TX = h->seq(TX_C); h->TH = h->seq(TH_C); h->D1 = h->seq(32); h->D2 = h->seq(32); h->DX = h->seq(8); h->U1 = h->seq(32); h->U2 = h->seq(32);
    h->OUT = h->seq(8);
    if ((rc = h->alloc())) return rc;
    const size_t cap = (size_t)h->cap_batches * TW;
    auto dmalloc = [&](float** p, size_t n) -> int { MF_HIP(hipMalloc(p, n * sizeof(float))); h->dev.push_back(*p); return MF_OK; };
    if ((rc = dmalloc(&h->xs, cap * 2)) || (rc = dmalloc(&h->coords01, cap * 2)) || (rc = dmalloc(&h->feat, cap * TG))) return rc;
    const int n_emb = cfg->offsets[cfg->num_levels];
    const mf_tensor* te = nf_find(sd, "torso_encoder.embeddings", n_emb, 2);
    if (!te) return MF_ERR_INVALID;
    if ((rc = dmalloc(&h->emb, (size_t)n_emb * 2))) return rc;
    MF_HIP(hipMemcpy(h->emb, te->data, (size_t)n_emb * 2 * sizeof(float), hipMemcpyHostToDevice));
    {
        auto it = sd.find("density_grid_torso");
        MF_REQUIRE(it != sd.end(), "nerf_torso_create: tensor 'density_grid_torso' missing");
        int64_t n = 1;
        for (int d = 0; d < it->second->ndim; ++d) n *= it->second->shape[d];
        MF_REQUIRE(n == (int64_t)cfg->grid_size * cfg->grid_size, "nerf_torso_create: density_grid_torso has %lld entries, expected %d^2", (long long)n, cfg->grid_size);
        if ((rc = dmalloc(&h->density, (size_t)n))) return rc;
        MF_HIP(hipMemcpy(h->density, it->second->data, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        MF_HIP(hipMalloc(&h->grid_partials, 64 * sizeof(double)));
        h->dev.push_back(h->grid_partials);
    }
    auto first_layer = [&](const char* name, int cin_ref, int var_cols, int cin_buf, const std::vector<int>& col_of, std::vector<float>& w,
                           std::vector<float>& wconst) -> int {
        const mf_tensor* t = nf_find(sd, name, 32, cin_ref);
        if (!t) return MF_ERR_INVALID;
        const float* src = (const float*)t->data;
        w.assign((size_t)32 * cin_buf, 0.f);
        wconst.assign((size_t)32 * NCONST, 0.f);
        for (int o = 0; o < 32; ++o) {
            for (int i = 0; i < var_cols; ++i) w[(size_t)o * cin_buf + col_of[i]] = src[(size_t)o * cin_ref + i];
            for (int i = var_cols; i < cin_ref; ++i) wconst[(size_t)o * NCONST + (i - var_cols)] = src[(size_t)o * cin_ref + i];
        }
        return MF_OK;
    };
    auto plain = [&](const char* name, int cout, int cin, std::vector<float>& w) -> int {
        const mf_tensor* t = nf_find(sd, name, cout, cin);
        if (!t) return MF_ERR_INVALID;
        w.assign((const float*)t->data, (const float*)t->data + (size_t)cout * cin);
        return MF_OK;
    };
    std::vector<float> w;
    std::vector<int> col(FQ + TG);
    for (int i = 0; i < FQ; ++i) col[i] = i;
    // deform net input order: [freq(x) 34 | anchors 42 | code] (network.py:180-183)
    if ((rc = first_layer("torso_deform_net.net.0.weight", din, FQ, TX_C, col, w, h->wd_const)) || (rc = h->linear(&h->d1, w, TX_C, 32, 1, h->TX))) return rc;
    if ((rc = plain("torso_deform_net.net.1.weight", 32, 32, w)) || (rc = h->linear(&h->d2, w, 32, 32, 1, h->D1))) return rc;
    if ((rc = plain("torso_deform_net.net.2.weight", 2, 32, w)) || (rc = h->linear(&h->d3, w, 32, 2, 0, h->D2))) return rc;
    // torso net input order: [grid 32 | freq(x) 34 | anchors 42 | code] (network.py:189-194) -- the same layout as TH
    for (int i = 0; i < TG + FQ; ++i) col[i] = i;
    if ((rc = first_layer("torso_net.net.0.weight", tin, TG + FQ, TH_C, col, w, h->wt_const)) || (rc = h->linear(&h->t1, w, TH_C, 32, 1, h->TH))) return rc;
    if ((rc = plain("torso_net.net.1.weight", 32, 32, w)) || (rc = h->linear(&h->t2, w, 32, 32, 1, h->U1))) return rc;
    if ((rc = plain("torso_net.net.2.weight", 4, 32, w)) || (rc = h->linear(&h->t3, w, 32, 4, 2, h->U2))) return rc;
    {
        // the fused kernel's table: the variable-input columns of the two first layers ([freq 34], [grid 32 | freq 34]: the leading columns of
        // the reference's weight rows, network.py:180-183 / 189-194) and the four other matrices as they are
        std::vector<float> tab;
        auto take = [&](const char* name, int cout, int cin_ref, int cols) -> int {
            const mf_tensor* t = nf_find(sd, name, cout, cin_ref);
            if (!t) return MF_ERR_INVALID;
            const float* src = (const float*)t->data;
            for (int o = 0; o < cout; ++o) tab.insert(tab.end(), src + (size_t)o * cin_ref, src + (size_t)o * cin_ref + cols);
            return MF_OK;
        };
        if ((rc = take("torso_deform_net.net.0.weight", 32, din, FQ)) || (rc = take("torso_deform_net.net.1.weight", 32, 32, 32)) ||
            (rc = take("torso_deform_net.net.2.weight", 2, 32, 32)) || (rc = take("torso_net.net.0.weight", 32, tin, TG + FQ)) ||
            (rc = take("torso_net.net.1.weight", 32, 32, 32)) || (rc = take("torso_net.net.2.weight", 4, 32, 32)))
            return rc;
        MF_REQUIRE((int)tab.size() == mf_nerf_torso_fused_weight_count(), "nerf_torso_create: fused table has %zu entries", tab.size());
        if ((rc = dmalloc(&h->wf, tab.size()))) return rc;
        MF_HIP(hipMemcpy(h->wf, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
        const char* e = std::getenv("MF_TORSO");
        h->fused = !(e && std::strcmp(e, "gemm") == 0);
    }
    MF_HIP(hipDeviceSynchronize());
    *out = h.release();
    return MF_OK;
}

// per-frame biases of the two first layers: W[:, constant columns] . [freq(wrapped anchors) | individual code]
void mf_nerf_torso::frame_bias(const float* frame_consts_host, float* bias) const {
    const int ncst = 42 + cfg.individual_dim;
    for (int o = 0; o < 32; ++o) {
        double a = 0, b = 0;
        for (int i = 0; i < ncst; ++i) {
            a += (double)wd_const[(size_t)o * NCONST + i] * frame_consts_host[i];
            b += (double)wt_const[(size_t)o * NCONST + i] * frame_consts_host[i];
        }
        bias[o] = (float)a; bias[32 + o] = (float)b;
    }
}

namespace {
struct FrameBias { float v[64]; };
__global__ void k_torso_bias(FrameBias fb, float* bd, float* bt) {
    if (threadIdx.x < 32) bd[threadIdx.x] = fb.v[threadIdx.x];
    else bt[threadIdx.x - 32] = fb.v[threadIdx.x];
}
}  // namespace

extern "C" int mf_nerf_torso_forward(mf_nerf_torso* h, const float* bg_coords, const float* frame_consts_host, const float* bg_color,
                                     int bg_per_ray, float bg_const, float density_thresh, int n_pixels, float* bg_out, float* torso_alpha,
                                     float* deform, void* stream) {
    MF_REQUIRE(h && bg_coords && frame_consts_host && bg_out, "nerf_torso_forward: null argument");
    MF_REQUIRE(n_pixels >= 0 && n_pixels <= h->cap_batches * TW, "nerf_torso_forward: %d pixels exceed the capacity %d", n_pixels, h->cap_batches * TW);
    if (n_pixels == 0) return MF_OK;
    hipStream_t s = (hipStream_t)stream;
    const int N = n_pixels, nb = (N + TW - 1) / TW, gb = (N + 255) / 256;
    FrameBias fb;
    h->frame_bias(frame_consts_host, fb.v);
    if (h->fused)
        return mf_nerf_torso_fused_launch(h->consts(), fb.v, h->sampled(), bg_coords, density_thresh, bg_color, bg_per_ray, bg_const, N, bg_out, torso_alpha, deform, s);
    hipLaunchKernelGGL(k_torso_bias, dim3(1), dim3(64), 0, s, fb, h->d1->bias, h->t1->bias);   // by value: no staging copy, no host sync
    hipLaunchKernelGGL(k_torso_prep, dim3((unsigned)(((int64_t)N * TX_C + 255) / 256)), dim3(256), 0, s, bg_coords, h->cfg.torso_shrink, N, h->xs,
                       h->TX->hi, h->TX->lo, h->TH->hi, h->TH->lo);
    MF_HIP(hipGetLastError());
    auto V = [](ActBuf* b, int C) { return ActView{b, 0, C}; };
    int rc;
    if ((rc = mf_conv_launch(h->d1, V(h->TX, TX_C), V(h->D1, 32), ActView{}, nb, s))) return rc;
    if ((rc = mf_conv_launch(h->d2, V(h->D1, 32), V(h->D2, 32), ActView{}, nb, s))) return rc;
    if ((rc = mf_conv_launch(h->d3, V(h->D2, 32), V(h->DX, 2), ActView{}, nb, s))) return rc;
    hipLaunchKernelGGL(k_torso_warp, dim3(gb), dim3(256), 0, s, h->xs, h->DX->hi, h->DX->lo, N, h->coords01, deform);
    MF_HIP(hipGetLastError());
    if ((rc = mf_grid_encode_forward(h->coords01, h->emb, h->cfg.offsets, h->feat, N, 2, 2, 16, h->cfg.log2_per_level_scale, h->cfg.base_resolution, 1, 0,
                                     1, stream)))
        return rc;
    hipLaunchKernelGGL(k_torso_pack, dim3((unsigned)(((int64_t)N * TG + 255) / 256)), dim3(256), 0, s, h->feat, N, h->TH->hi, h->TH->lo);
    MF_HIP(hipGetLastError());
    if ((rc = mf_conv_launch(h->t1, V(h->TH, TH_C), V(h->U1, 32), ActView{}, nb, s))) return rc;
    if ((rc = mf_conv_launch(h->t2, V(h->U1, 32), V(h->U2, 32), ActView{}, nb, s))) return rc;
    if ((rc = mf_conv_launch(h->t3, V(h->U2, 32), V(h->OUT, 4), ActView{}, nb, s))) return rc;
    hipLaunchKernelGGL(k_torso_mix, dim3(gb), dim3(256), 0, s, bg_coords, h->sampled(), h->cfg.grid_size, density_thresh, h->OUT->hi, h->OUT->lo, bg_color,
                       bg_per_ray, bg_const, N, bg_out, torso_alpha);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

// mf_nerf_torso_forward for the frames of a table in one launch: the biases are formed here exactly as above and travel in the batch handle's table
extern "C" int mf_nerf_torso_forward_batch(mf_nerf_torso* torso, mf_nerf_frame_batch* h, const mf_nerf_torso_desc* descs, int n_frames, int n_pixels, void* stream) {
    MF_REQUIRE(h && descs, "nerf_torso_forward_batch: null handle or descriptor table");
    int max_frames = 0, max_pixels = 0, rc;
    if ((rc = mf_nerf_frame_batch_limits(h, &max_frames, &max_pixels))) return rc;
    MF_REQUIRE(n_frames >= 1 && n_frames <= max_frames, "nerf_torso_forward_batch: n_frames=%d (the handle holds 1..%d)", n_frames, max_frames);
    MF_REQUIRE(n_pixels >= 1 && n_pixels <= max_pixels, "nerf_torso_forward_batch: n_pixels=%d (the handle's max_pixels is %d)", n_pixels, max_pixels);
    MF_REQUIRE(torso, "nerf_torso_forward_batch: null torso handle");
    MF_REQUIRE(torso->fused, "nerf_torso_forward_batch: needs the fused torso kernel (unset MF_TORSO=gemm)");
    for (int i = 0; i < n_frames; ++i)
        MF_REQUIRE(descs[i].bg_coords && descs[i].bg_out, "nerf_torso_forward_batch: frame %d: null bg_coords or bg_out", i);
    hipStream_t s = (hipStream_t)stream;
    auto fill = [&](NerfTorsoFrame* tab) {
        for (int i = 0; i < n_frames; ++i) {
            const mf_nerf_torso_desc& d = descs[i];
            NerfTorsoFrame& t = tab[i];
            float bias[64];
            torso->frame_bias(d.frame_consts, bias);
            for (int o = 0; o < 32; ++o) { t.bias_d[o] = bias[o]; t.bias_t[o] = bias[32 + o]; }
            t.bg_coords = d.bg_coords; t.bg = d.bg_color; t.out = d.bg_out; t.alpha_out = d.torso_alpha; t.deform = d.deform;
            t.thresh = d.density_thresh; t.bg_const = d.bg_const; t.bg_per_ray = d.bg_per_ray; t.pad = 0;
        }
    };
    return mf_nerf_frame_batch_ring(h).call<NerfTorsoFrame>(n_frames, s, fill, [&](const NerfTorsoFrame* dev) {
        return mf_nerf_torso_batch_launch(torso->consts(), dev, n_frames, torso->sampled(), n_pixels, s);
    });
}

extern "C" int mf_nerf_torso_set_grid(mf_nerf_torso* h, const float* density_grid) {
    MF_REQUIRE(h, "nerf_torso_set_grid: null handle");
    h->grid = density_grid;
    return MF_OK;
}

extern "C" int mf_nerf_torso_grid_update(mf_nerf_torso* h, const float* frame_consts_host, const float* noise, float decay, float* density_grid, float* raw_grid,
                                         float* xys_out, float* mean, void* stream) {
    MF_REQUIRE(h && frame_consts_host && density_grid && raw_grid && mean, "nerf_torso_grid_update: null argument");
    MF_REQUIRE(density_grid != raw_grid, "nerf_torso_grid_update: density_grid and raw_grid are the same buffer");
    MF_REQUIRE(h->fused, "nerf_torso_grid_update: needs the fused torso kernel (unset MF_TORSO=gemm)");
    size_t unused = 0;
    int rc;
    if ((rc = mf_nerf_occupancy_shape("nerf_torso_grid_update", 1, h->cfg.grid_size, &unused))) return rc;
    float bias[64];
    h->frame_bias(frame_consts_host, bias);
    if ((rc = mf_nerf_torso_grid_launch(h->consts(), bias, noise, decay, density_grid, raw_grid, xys_out, mean, h->grid_partials, (hipStream_t)stream))) return rc;
    h->grid = density_grid;
    return MF_OK;
}

extern "C" void mf_nerf_torso_destroy(mf_nerf_torso* h) { delete h; }
