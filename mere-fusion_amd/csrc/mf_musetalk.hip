// MuseTalk UNet (one conditional evaluation at t = 0) and SD-VAE decoder on gfx950 (H4, H5):
// musereal.py:102-108 -> musetalk/models/unet.py:29-44, vae.py:96-108 -> diffusers UNet2DConditionModel /
// AutoencoderKL (un-vendored; architecture per include/merefusion.h mf_unet_config / mf_vae_config).
//
// Both networks are static schedules of the same fused building blocks as the Wav2Lip generator:
//   * every Conv2d / Linear is an MFMA convolution (3x3 halo-tile or implicit GEMM, 1x1 = GEMM) with
//     bias / residual / SiLU epilogues; the t = 0 time embedding is a per-channel constant folded into
//     each resnet's conv1 bias at create time;
//   * `torch.cat([hidden, skip])` of the up path is free: producer layers write channel slices of one buffer;
//   * nearest-2x upsample + conv3x3 runs as 4 sub-pixel phases of pre-summed 2x2 taps (2.25x fewer FLOPs);
//   * attention = grouped (batch x head) GEMMs with device-packed K / V^T operands + fp32 row softmax;
//   * GroupNorm(+SiLU) = fp64 statistics pass + one apply pass.
//
// This file holds the three topologies and their C ABI; the layers and blocks they are made of are the builder's (mf_musetalk_build.h), the op list and its
// execution the schedule's (mf_schedule.h).
#include "mf_musetalk_build.h"
#include <cmath>

namespace {

std::vector<float> silu_vec(const std::vector<float>& v) {
    std::vector<float> o(v.size());
    for (size_t i = 0; i < v.size(); ++i) o[i] = (float)((double)v[i] / (1.0 + std::exp(-(double)v[i])));
    return o;
}

}  // namespace

// ==========================================================================================================
struct mf_unet {
    mf_unet_config cfg{};
    Builder net;
    ActBuf* in_lat = nullptr;
    ActBuf* ctx = nullptr;
    ActBuf* out_buf = nullptr;
    float* pe = nullptr;       // [ctx_len][cross_dim] positional encoding (unet.py:12-27)
};

extern "C" int mf_unet_create(const mf_unet_config* c, const mf_tensor* weights, int n_weights, int precision, int max_batch,
                              mf_unet** out) {
    MF_REQUIRE(c && weights && out && n_weights > 0 && max_batch > 0, "unet_create: bad argument");
    MF_REQUIRE(c->n_blocks >= 1 && c->n_blocks <= 4 && c->layers_per_block >= 1, "unet_create: bad block config");
    *out = nullptr;
    std::unique_ptr<mf_unet> h(new mf_unet());
    h->cfg = *c;
    Builder& net = h->net;
    // token slots per sample of the folded LayerNorms: three per transformer block, each over the block's map
    int ln_tokens = 0;
    {
        int sz = c->sample_size;
        for (int b = 0; b < c->n_blocks; ++b) {
            if (c->down_attn[b]) ln_tokens += 3 * c->layers_per_block * sz * sz;
            if (b < c->n_blocks - 1) sz /= 2;
        }
        ln_tokens += 3 * sz * sz;                                                  // mid block
        for (int b = 0; b < c->n_blocks; ++b) {
            if (c->up_attn[b]) ln_tokens += 3 * (c->layers_per_block + 1) * sz * sz;
            if (b < c->n_blocks - 1) sz *= 2;
        }
    }
    int rc = net.init(weights, n_weights, precision, max_batch, c->norm_num_groups, ln_tokens);
    if (rc) return rc;
    net.q_dual_allowed = true;   // (tests/test_musetalk_full.py holds the 40-frame handle to the batch-8 parity gate with it)
    const int nb = c->n_blocks, L = c->layers_per_block, G = c->norm_num_groups, heads = c->attention_heads;
    const int* boc = c->block_out_channels;
    const int S = c->sample_size, X = c->cross_attention_dim;

    // ---- time embedding at t = 0 (musereal.py:59): cos(0) = 1 for the first half, sin(0) = 0 for the second -----
    std::vector<float> temb_act;
    {
        const int d0 = boc[0], td = 4 * boc[0];
        const float *w1 = net.T("time_embedding.linear_1.weight", (int64_t)td * d0), *b1 = net.T("time_embedding.linear_1.bias", td);
        const float *w2 = net.T("time_embedding.linear_2.weight", (int64_t)td * td), *b2 = net.T("time_embedding.linear_2.bias", td);
        NET_TRY(net.got(w1, b1, w2, b2));
        std::vector<float> e1(td), e2(td);
        for (int o = 0; o < td; ++o) {
            double a = b1[o];
            for (int i = 0; i < d0 / 2; ++i) a += (double)w1[(size_t)o * d0 + i];   // emb = [1]*half + [0]*half
            e1[o] = (float)a;
        }
        e1 = silu_vec(e1);
        for (int o = 0; o < td; ++o) {
            double a = b2[o];
            for (int i = 0; i < td; ++i) a += (double)w2[(size_t)o * td + i] * e1[i];
            e2[o] = (float)a;
        }
        temb_act = silu_vec(e2);
    }

    // ---- positional encoding table -------------------------------------------------------------------------------
    {
        std::vector<float> pe((size_t)c->ctx_len * X);
        for (int t = 0; t < c->ctx_len; ++t)
            for (int i = 0; i < X; i += 2) {
                const float div = std::exp((float)i * (float)(-std::log(10000.0) / X));
                pe[(size_t)t * X + i] = std::sin((float)t * div);
                if (i + 1 < X) pe[(size_t)t * X + i + 1] = std::cos((float)t * div);
            }
        h->pe = net.upload(pe.data(), pe.size());
        NET_TRY(net.got(h->pe));
    }

    // ---- skip bookkeeping: skip k is consumed by up-resnet (n_skips-1-k); both live in one concat buffer ------------
    std::vector<int> skip_c, skip_s;   // channels / spatial size of each skip, in production order
    {
        int s = S;
        skip_c.push_back(boc[0]); skip_s.push_back(s);
        for (int b = 0; b < nb; ++b) {
            for (int i = 0; i < L; ++i) { skip_c.push_back(boc[b]); skip_s.push_back(s); }
            if (b < nb - 1) { s /= 2; skip_c.push_back(boc[b]); skip_s.push_back(s); }
        }
    }
    const int n_skips = (int)skip_c.size();
    // hidden channels entering each up-resnet
    std::vector<int> up_h(n_skips), up_out(n_skips);
    {
        int ch = boc[nb - 1], j = 0;
        for (int b = 0; b < nb; ++b)
            for (int i = 0; i < L + 1; ++i, ++j) { up_h[j] = ch; up_out[j] = boc[nb - 1 - b]; ch = boc[nb - 1 - b]; }
    }
    std::vector<ActBuf*> cat(n_skips);   // cat[j] = [hidden | skip] read by up-resnet j
    for (int j = 0; j < n_skips; ++j) {
        const int k = n_skips - 1 - j;
        cat[j] = net.buf(up_h[j] + skip_c[k], skip_s[k], skip_s[k], 1);
        NET_TRY(net.got(cat[j]));
    }
    auto skip_view = [&](int k) { const int j = n_skips - 1 - k; return ActView{cat[j], up_h[j], skip_c[k]}; };

    h->in_lat = net.buf(c->in_channels, S, S, 1);
    h->ctx = net.buf(X, 1, c->ctx_len, 0);
    h->out_buf = net.buf(c->out_channels, S, S, 1);
    NET_TRY(net.got(h->in_lat, h->ctx, h->out_buf));
    const ActView ctx{h->ctx, 0, X};

    KvHoist kv;
    {
        int kv_total = 0;
        for (int b = 0; b < nb; ++b) {
            if (c->down_attn[b]) kv_total += L * 2 * boc[b];
            if (c->up_attn[b]) kv_total += (L + 1) * 2 * boc[nb - 1 - b];
        }
        kv_total += 2 * boc[nb - 1];                                   // mid block
        NET_TRY(net.hoist_kv_begin(&kv, ctx, kv_total));
    }
    // ---- down path ------------------------------------------------------------------------------------------------
    int k = 0, s = S, ch = boc[0];
    NET_TRY(net.conv("conv_in", ActView{h->in_lat, 0, h->in_lat->C}, skip_view(k), c->in_channels, boc[0], 3, 1, 1));
    ActView x = skip_view(k++);
    for (int b = 0; b < nb; ++b) {
        for (int i = 0; i < L; ++i) {
            const std::string rp = "down_blocks." + std::to_string(b) + ".resnets." + std::to_string(i);
            if (c->down_attn[b]) {
                ActBuf* r = net.tmp("down.r", boc[b], s, s, 1);
                NET_TRY(net.got(r));
                NET_TRY(net.resnet(rp, x, ActView{r, 0, boc[b]}, ch, boc[b], G, 1e-5f, &temb_act));
                NET_TRY(net.transformer("down_blocks." + std::to_string(b) + ".attentions." + std::to_string(i),
                                        ActView{r, 0, boc[b]}, skip_view(k), boc[b], heads, G, ctx, &kv));
            } else {
                NET_TRY(net.resnet(rp, x, skip_view(k), ch, boc[b], G, 1e-5f, &temb_act));
            }
            ch = boc[b];
            x = skip_view(k++);
        }
        if (b < nb - 1) {
            // Downsample2D: conv 3x3 stride 2 padding 1
            ActView o = skip_view(k);
            NET_TRY(net.conv("down_blocks." + std::to_string(b) + ".downsamplers.0.conv", x, o, ch, ch, 3, 2, 1));
            s /= 2;
            x = skip_view(k++);
        }
    }
    // ---- mid ------------------------------------------------------------------------------------------------------
    {
        ActBuf *m0 = net.buf(ch, s, s, 1), *m1 = net.buf(ch, s, s, 1);
        NET_TRY(net.got(m0, m1));
        NET_TRY(net.resnet("mid_block.resnets.0", x, ActView{m0, 0, ch}, ch, ch, G, 1e-5f, &temb_act));
        NET_TRY(net.transformer("mid_block.attentions.0", ActView{m0, 0, ch}, ActView{m1, 0, ch}, ch, heads, G, ctx, &kv));
        // the second mid resnet writes the hidden slice of the first up-resnet's concat buffer
        NET_TRY(net.resnet("mid_block.resnets.1", ActView{m1, 0, ch}, ActView{cat[0], 0, up_h[0]}, ch, ch, G, 1e-5f, &temb_act));
    }
    // ---- up path --------------------------------------------------------------------------------------------------
    int j = 0;
    ActView last{};
    ConvOpts up2x; up2x.upsample = 1;
    for (int b = 0; b < nb; ++b) {
        const int co = boc[nb - 1 - b];
        for (int i = 0; i < L + 1; ++i, ++j) {
            const std::string rp = "up_blocks." + std::to_string(b) + ".resnets." + std::to_string(i);
            const int cin = cat[j]->C;
            const bool tail = (i == L);                               // last resnet of the block
            const bool has_up = b < nb - 1;
            // where this sub-block's result goes: next concat buffer (same resolution), or a staging buffer in
            // front of the upsampler, or the final buffer
            ActView dst;
            ActBuf* stage = nullptr;
            if (!tail) dst = ActView{cat[j + 1], 0, up_h[j + 1]};
            else {
                stage = net.buf(co, s, s, 1);
                NET_TRY(net.got(stage));
                dst = ActView{stage, 0, co};
            }
            if (c->up_attn[b]) {
                ActBuf* r = net.tmp("up.r", co, s, s, 1);
                NET_TRY(net.got(r));
                NET_TRY(net.resnet(rp, ActView{cat[j], 0, cin}, ActView{r, 0, co}, cin, co, G, 1e-5f, &temb_act));
                NET_TRY(net.transformer("up_blocks." + std::to_string(b) + ".attentions." + std::to_string(i), ActView{r, 0, co}, dst, co, heads, G, ctx, &kv));
            } else {
                NET_TRY(net.resnet(rp, ActView{cat[j], 0, cin}, dst, cin, co, G, 1e-5f, &temb_act));
            }
            if (tail && has_up) {
                // Upsample2D: nearest 2x + conv 3x3, written into the hidden slice of the next concat buffer
                NET_TRY(net.conv("up_blocks." + std::to_string(b) + ".upsamplers.0.conv", dst, ActView{cat[j + 1], 0, up_h[j + 1]}, co, co, 3, 1, 1, up2x));
                s *= 2;
            }
            last = dst;
        }
    }
    {
        NET_TRY(net.gn_conv_tail("conv_norm_out", "conv_out", last, ActView{h->out_buf, 0, c->out_channels}, boc[0], c->out_channels, G, 1e-5f));
    }
    NET_TRY(net.hoist_kv_finish(&kv));
    *out = h.release();
    return MF_OK;
}

extern "C" int mf_unet_forward(mf_unet* h, const float* latents, const float* audio, int add_pe, float* out, int batch, void* stream) {
    MF_REQUIRE(h && latents && audio && out, "unet_forward: null argument");
    MF_REQUIRE(batch > 0 && batch <= h->net.cap, "unet_forward: batch %d exceeds the handle's max_batch %d", batch, h->net.cap);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = mf_nchw_to_act(latents, h->cfg.in_channels, *h->in_lat, batch, s))) return rc;
    if ((rc = mf_rows_from_f32(audio, add_pe ? h->pe : nullptr, ActView{h->ctx, 0, h->cfg.cross_attention_dim}, batch, s))) return rc;
    if ((rc = h->net.sch.run(batch, s))) return rc;
    return mf_act_to_nchw(ActView{h->out_buf, 0, h->cfg.out_channels}, out, batch, s);
}

extern "C" int mf_unet_num_ops(const mf_unet* h) { return h ? (int)h->net.sch.ops.size() : 0; }
extern "C" int mf_unet_op_info(const mf_unet* h, int i, char* name, int ncap, char* kernel, int kcap, double* flops_per_frame) {
    MF_REQUIRE(h, "unet_op_info: null handle");
    return h->net.sch.op_info(i, name, ncap, kernel, kcap, flops_per_frame);
}
extern "C" int mf_unet_profile(mf_unet* h, int batch, int iters, float* ms_per_op, void* stream) {
    MF_REQUIRE(h && ms_per_op && batch > 0 && batch <= h->net.cap && iters > 0, "unet_profile: bad argument");
    return h->net.sch.profile(batch, iters, ms_per_op, (hipStream_t)stream);
}
extern "C" int mf_unet_tune(mf_unet* h, int batch, void* stream) {
    MF_REQUIRE(h && batch >= 1 && batch <= h->net.cap, "unet_tune: batch %d exceeds the capacity %d", batch, h ? h->net.cap : 0);
    return h->net.sch.tune(batch, (hipStream_t)stream, "tune: run one forward");
}
extern "C" void mf_unet_destroy(mf_unet* h) { delete h; }

// ==========================================================================================================
struct mf_vae {
    mf_vae_config cfg{};
    Builder net;
    ActBuf* in_lat = nullptr;
    ActBuf* out_buf = nullptr;
};

extern "C" int mf_vae_create(const mf_vae_config* c, const mf_tensor* weights, int n_weights, int precision, int max_batch,
                             mf_vae** out) {
    MF_REQUIRE(c && weights && out && n_weights > 0 && max_batch > 0, "vae_create: bad argument");
    MF_REQUIRE(c->n_blocks >= 1 && c->n_blocks <= 4 && c->scaling_factor > 0.f, "vae_create: bad config");
    *out = nullptr;
    std::unique_ptr<mf_vae> h(new mf_vae());
    h->cfg = *c;
    Builder& net = h->net;
    int rc = net.init(weights, n_weights, precision, max_batch, c->norm_num_groups);
    if (rc) return rc;
    net.q_allowed = true;        // decoder resnet convs on maps >= 64 x 64 in the f16 + FP6 format (tests/test_musetalk_full.py holds the parity bound with it)
    const int nb = c->n_blocks, L = c->layers_per_block, G = c->norm_num_groups, Z = c->latent_channels;
    const int* boc = c->block_out_channels;
    int s = c->sample_size, ch = boc[nb - 1];
    h->in_lat = net.buf(Z, s, s, 1);
    ActBuf *pq = net.buf(Z, s, s, 1), *x0 = net.buf(ch, s, s, 1), *x1 = net.buf(ch, s, s, 1);
    NET_TRY(net.got(h->in_lat, pq, x0, x1));
    // latents = (1 / scaling_factor) * latents (vae.py:102) folded into post_quant_conv's weights
    ConvOpts unscale; unscale.w_scale = 1.f / c->scaling_factor;
    NET_TRY(net.conv("post_quant_conv", ActView{h->in_lat, 0, h->in_lat->C}, ActView{pq, 0, Z}, Z, Z, 1, 1, 0, unscale));
    NET_TRY(net.conv("decoder.conv_in", ActView{pq, 0, pq->C}, ActView{x0, 0, ch}, Z, ch, 3, 1, 1));
    NET_TRY(net.resnet("decoder.mid_block.resnets.0", ActView{x0, 0, ch}, ActView{x1, 0, ch}, ch, ch, G, 1e-6f, nullptr));
    NET_TRY(net.vae_mid_attention("decoder.mid_block.attentions.0", ActView{x1, 0, ch}, ActView{x0, 0, ch}, ActView{x1, 0, ch}, G));
    NET_TRY(net.resnet("decoder.mid_block.resnets.1", ActView{x0, 0, ch}, ActView{x1, 0, ch}, ch, ch, G, 1e-6f, nullptr));
    ActView x{x1, 0, ch};
    for (int b = 0; b < nb; ++b) {
        const int co = boc[nb - 1 - b];
        for (int i = 0; i < L + 1; ++i) {
            ActBuf* y = net.buf(co, s, s, 1);
            NET_TRY(net.got(y));
            NET_TRY(net.resnet("decoder.up_blocks." + std::to_string(b) + ".resnets." + std::to_string(i), x, ActView{y, 0, co}, ch, co, G, 1e-6f, nullptr));
            ch = co;
            x = ActView{y, 0, co};
        }
        if (b < nb - 1) {
            ActBuf* y = net.buf(ch, 2 * s, 2 * s, 1);
            NET_TRY(net.got(y));
            NET_TRY(net.upsample_conv("decoder.up_blocks." + std::to_string(b) + ".upsamplers.0.conv", x, ActView{y, 0, ch}, ch));
            s *= 2;
            x = ActView{y, 0, ch};
        }
    }
    h->out_buf = net.buf(c->out_channels, s, s, 1);
    NET_TRY(net.got(h->out_buf));
    NET_TRY(net.gn_conv_tail("decoder.conv_norm_out", "decoder.conv_out", x, ActView{h->out_buf, 0, c->out_channels}, ch, c->out_channels, G, 1e-6f));
    *out = h.release();
    return MF_OK;
}

extern "C" int mf_vae_decode_latents(mf_vae* h, const float* latents, uint8_t* frames, float* image_f32, int batch, void* stream) {
    MF_REQUIRE(h && latents && (frames || image_f32), "vae_decode_latents: null argument");
    MF_REQUIRE(batch > 0 && batch <= h->net.cap, "vae_decode_latents: batch %d exceeds the handle's max_batch %d", batch, h->net.cap);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = mf_nchw_to_act(latents, h->cfg.latent_channels, *h->in_lat, batch, s))) return rc;
    if ((rc = h->net.sch.run(batch, s))) return rc;
    const ActView o{h->out_buf, 0, h->cfg.out_channels};
    if (image_f32 && (rc = mf_act_to_nchw(o, image_f32, batch, s))) return rc;
    if (frames && (rc = mf_vae_post_u8(o, frames, batch, s))) return rc;
    return MF_OK;
}

extern "C" int mf_vae_num_ops(const mf_vae* h) { return h ? (int)h->net.sch.ops.size() : 0; }
extern "C" int mf_vae_op_info(const mf_vae* h, int i, char* name, int ncap, char* kernel, int kcap, double* flops_per_frame) {
    MF_REQUIRE(h, "vae_op_info: null handle");
    return h->net.sch.op_info(i, name, ncap, kernel, kcap, flops_per_frame);
}
extern "C" int mf_vae_profile(mf_vae* h, int batch, int iters, float* ms_per_op, void* stream) {
    MF_REQUIRE(h && ms_per_op && batch > 0 && batch <= h->net.cap && iters > 0, "vae_profile: bad argument");
    return h->net.sch.profile(batch, iters, ms_per_op, (hipStream_t)stream);
}
extern "C" int mf_vae_tune(mf_vae* h, int batch, void* stream) {
    MF_REQUIRE(h && batch >= 1 && batch <= h->net.cap, "vae_tune: batch %d exceeds the capacity %d", batch, h ? h->net.cap : 0);
    return h->net.sch.tune(batch, (hipStream_t)stream, "tune: run one forward");
}
extern "C" void mf_vae_destroy(mf_vae* h) { delete h; }


// ==========================================================================================================
// sd-vae ENCODER (avatar preparation): `vae.encode(image).latent_dist` of musetalk/models/vae.py:84-94 -- diffusers
// AutoencoderKL.encode = Encoder (conv_in, 4 DownEncoderBlock2D of 2 resnets (+ Downsample2D: F.pad(x, (0, 1, 0, 1)), conv k3 s2 p0),
// mid resnet - attention - resnet, GroupNorm + SiLU, conv_out -> 2 * latent channels) followed by quant_conv; the result holds the
// distribution's (mean | logvar) "moments".  Sampling (mean + std * noise, then * scaling_factor) stays with the caller, who owns the RNG.
struct mf_vae_encoder {
    mf_vae_config cfg{};
    Builder net;
    ActBuf* in_img = nullptr;
    ActBuf* out_buf = nullptr;
    int image_size = 0;
};

extern "C" int mf_vae_encoder_create(const mf_vae_config* c, const mf_tensor* weights, int n_weights, int precision, int max_batch,
                                     mf_vae_encoder** out) {
    MF_REQUIRE(c && weights && out && n_weights > 0 && max_batch > 0, "vae_encoder_create: bad argument");
    MF_REQUIRE(c->n_blocks >= 1 && c->n_blocks <= 4, "vae_encoder_create: bad config");
    *out = nullptr;
    std::unique_ptr<mf_vae_encoder> h(new mf_vae_encoder());
    h->cfg = *c;
    Builder& net = h->net;
    int rc = net.init(weights, n_weights, precision, max_batch, c->norm_num_groups);
    if (rc) return rc;
    const int nb = c->n_blocks, L = c->layers_per_block, G = c->norm_num_groups, Z = c->latent_channels;
    const int* boc = c->block_out_channels;
    int s = c->sample_size << (nb - 1);                     // image size: the latent grid times 2 per downsampler
    h->image_size = s;
    h->in_img = net.buf(c->out_channels, s, s, 1);          // RGB image, channels padded to 8
    ActBuf* x0 = net.buf(boc[0], s, s, 1);
    NET_TRY(net.got(h->in_img, x0));
    NET_TRY(net.conv("encoder.conv_in", ActView{h->in_img, 0, h->in_img->C}, ActView{x0, 0, boc[0]}, c->out_channels, boc[0], 3, 1, 1));
    ActView x{x0, 0, boc[0]};
    int ch = boc[0];
    for (int b = 0; b < nb; ++b) {
        for (int i = 0; i < L; ++i) {
            ActBuf* y = net.buf(boc[b], s, s, 1);
            NET_TRY(net.got(y));
            NET_TRY(net.resnet("encoder.down_blocks." + std::to_string(b) + ".resnets." + std::to_string(i), x, ActView{y, 0, boc[b]}, ch, boc[b], G, 1e-6f, nullptr));
            ch = boc[b];
            x = ActView{y, 0, ch};
        }
        if (b < nb - 1) {
            ActBuf* y = net.buf(ch, s / 2, s / 2, 1);
            NET_TRY(net.got(y));
            ConvOpts o; o.pad_hi = 1;                       // F.pad(x, (0, 1, 0, 1)) + conv(k3, s2, p0): the buffer's own zero ring is the pad
            NET_TRY(net.conv("encoder.down_blocks." + std::to_string(b) + ".downsamplers.0.conv", x, ActView{y, 0, ch}, ch, ch, 3, 2, 0, o));
            s /= 2;
            x = ActView{y, 0, ch};
        }
    }
    ActBuf *m0 = net.buf(ch, s, s, 1), *m1 = net.buf(ch, s, s, 1);
    NET_TRY(net.got(m0, m1));
    NET_TRY(net.resnet("encoder.mid_block.resnets.0", x, ActView{m0, 0, ch}, ch, ch, G, 1e-6f, nullptr));
    NET_TRY(net.vae_mid_attention("encoder.mid_block.attentions.0", ActView{m0, 0, ch}, ActView{m1, 0, ch}, ActView{m0, 0, ch}, G));
    NET_TRY(net.resnet("encoder.mid_block.resnets.1", ActView{m1, 0, ch}, ActView{m0, 0, ch}, ch, ch, G, 1e-6f, nullptr));
    ActBuf *t = net.buf(ch, s, s, 1), *co = net.buf(2 * Z, s, s, 1);
    h->out_buf = net.buf(2 * Z, s, s, 1);
    NET_TRY(net.got(t, co, h->out_buf));
    NET_TRY(net.gn("encoder.conv_norm_out", ActView{m0, 0, ch}, ActView{t, 0, ch}, G, 1e-6f, true));
    NET_TRY(net.conv("encoder.conv_out", ActView{t, 0, ch}, ActView{co, 0, 2 * Z}, ch, 2 * Z, 3, 1, 1));
    NET_TRY(net.conv("quant_conv", ActView{co, 0, 2 * Z}, ActView{h->out_buf, 0, 2 * Z}, 2 * Z, 2 * Z, 1, 1, 0));
    *out = h.release();
    return MF_OK;
}

extern "C" int mf_vae_encode(mf_vae_encoder* h, const float* image, const uint8_t* image_u8_bgr, int half_mask, float* moments, int batch, void* stream) {
    MF_REQUIRE(h && moments && (image || image_u8_bgr) && !(image && image_u8_bgr), "vae_encode: give exactly one of image / image_u8_bgr, and moments");
    MF_REQUIRE(batch > 0 && batch <= h->net.cap, "vae_encode: batch %d exceeds the handle's max_batch %d", batch, h->net.cap);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (image) { if ((rc = mf_nchw_to_act(image, h->cfg.out_channels, *h->in_img, batch, s))) return rc; }
    else if ((rc = mf_vae_image_u8_to_act(image_u8_bgr, *h->in_img, half_mask, batch, s))) return rc;
    if ((rc = h->net.sch.run(batch, s))) return rc;
    return mf_act_to_nchw(ActView{h->out_buf, 0, 2 * h->cfg.latent_channels}, moments, batch, s);
}

extern "C" int mf_vae_encoder_image_size(const mf_vae_encoder* h) { return h ? h->image_size : 0; }
extern "C" void mf_vae_encoder_destroy(mf_vae_encoder* h) { delete h; }
