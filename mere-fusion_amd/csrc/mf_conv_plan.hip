// Convolution plans: BatchNorm / LayerNorm folding, the weight packs of every kernel family (implicit GEMM, halo tiles, thin input, f16 + FP6), the upload,
// and the binding of a plan to its input geometry (the goff table).  Host code only; the kernels are in mf_conv.hip, mf_conv_halo*.hip and mf_conv_thin.hip.
#include "mf_conv.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
static bool g_no_halo_wide = false;   // set while mf_conv_plan_create builds the implicit-GEMM twin of a wide halo plan

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

double mf_conv_flops(const ConvPlan* p, int batch) {
    const mf_conv2d_desc& d = p->d;
    const double taps = (double)d.kh * d.kw;
    const double sites = d.transposed ? (double)d.in_h * d.in_w : (double)p->out_h * p->out_w;
    return 2.0 * batch * sites * d.cin * d.cout * taps;
}
