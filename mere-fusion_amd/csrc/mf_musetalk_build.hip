#include "mf_musetalk_build.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>

namespace {

// ---- switches and thresholds --------------------------------------------------------------------------------------------------------------------------
bool env_on(const char* name) { const char* e = getenv(name); return !e || atoi(e) != 0; }
// latched once per process (an A/B of one of them is a child process: tests/test_musetalk.py).  MF_GN_AFFINE_FUSE is per handle: Builder::init.
struct Switches {
    bool conv_q = env_on("MF_CONV_Q");           // 0: bf16x3 everywhere, no f16 + FP6 conv
    bool q_equalize = env_on("MF_Q_EQUALIZE");   // 0: no channel equalisation of the f16 + FP6 operands
    bool tail_fuse = env_on("MF_TAIL_FUSE");     // 0: GroupNorm + conv_out always as the two-op chain (A/B)
    // a transformer block's ff.net.2 and proj_out as one layer (Builder::ff_proj_out).  Unset: where the tuning table holds the fused layer at the handle's
    // capacity (ff_fold_measured); 0: never, the two-op chain (A/B); any other value: always (tests, and measuring the fused shapes for the table)
    int ff_proj_fold = getenv("MF_FF_PROJ_FOLD") ? (atoi(getenv("MF_FF_PROJ_FOLD")) != 0 ? 2 : 0) : 1;
};
const Switches& switches() { static const Switches s{}; return s; }

const int Q_DUAL_MIN = 16;   // frames per step from which the dual-path convs take the f16 + FP6 tile (profiles/r04_unet_q_dual.md)
// (whole step, same box, bf16x3 -> f16 + FP6 on those twenty layers: 8 frames 18.78 -> 18.78 ms, 16: 32.0 -> 31.6, 24: 45.5 -> 44.7, 32: 58.7 -> 57.4, 64: 109.05 -> 107.66)
// (maps below 64 x 64 -- the 512-channel 32 x 32 levels -- run it with the channel slices split over two workgroups per tile, mf_q_split_count)
const int Q_MIN_PX = 32 * 32;
#ifndef MF_UP_Q_MIN_WG
#define MF_UP_Q_MIN_WG 256            // workgroups per phase launch from which the f16 + FP6 phases beat the bf16x3 implicit GEMM (A/B build with 128 -- the 512-channel 32^2 -> 64^2 upsampler at batch 8 as four 128-workgroup phase launches: 18.29 vs 18.32 ms per step, no gain)
#endif

// a k x k stride-1 conv over `in` (callers set what else they need)
mf_conv2d_desc desc_s1(int cin, int cout, int k, int pad, const ActBuf& in, const ActView& res) {
    mf_conv2d_desc d{};
    d.cin = cin; d.cout = cout; d.kh = d.kw = k; d.stride_h = d.stride_w = 1; d.pad_h = d.pad_w = pad;
    d.residual = res.buf ? 1 : 0; d.in_h = in.H; d.in_w = in.W;
    return d;
}

// row blocks stacked into one matrix: the q | k | v and k | v weights (and biases) of one GEMM
std::vector<float> cat_rows(std::initializer_list<const float*> parts, size_t n_each) {
    std::vector<float> w;
    w.reserve(parts.size() * n_each);
    for (const float* p : parts) w.insert(w.end(), p, p + n_each);
    return w;
}

// f(i) for i in [0, n) on a few host threads (create-time weight arithmetic)
template <class F> void parallel_for(int n, F f) {
    const int nt = std::max(1, std::min({n, 8, (int)std::thread::hardware_concurrency()}));
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back([=] { for (int i = t; i < n; i += nt) f(i); });
    for (int i = 0; i < n; i += nt) f(i);
    for (auto& x : th) x.join();
}

// GroupNorm -> SiLU -> the f16 + FP6 format in front of a conv of that format.  `fuse` (maps of a multiple of 64 pixels): the conversion kernel forms the per-channel
// affine itself from the statistics -- the k_gn_affine launch in front of each of the VAE decoder's 28 conversions goes (same bits: mf_gn_affine_pair).
// MF_GN_AFFINE_FUSE=0 keeps the two launches (A/B, tests).
int gn_silu_to_q(const ActView& x, const float* dg, const float* db, int groups, float eps, double* st, float* scale, float* shift, const ActBuf& tq, int B,
                 hipStream_t s, bool have_stats, const float* post, bool fuse) {
    const ActBuf& xb = *x.buf;
    if (fuse && (xb.H * xb.W) % 64 == 0) {
        if (!have_stats) { const int rc = mf_groupnorm_stats(x, groups, st, B, s); if (rc) return rc; }
        return mf_affine_silu_to_act_q(x, scale, shift, 1, tq, B, s, post, st, dg, db, groups, eps);
    }
    const int r1 = mf_groupnorm_affine(x, dg, db, groups, eps, st, scale, shift, B, s, have_stats);
    return r1 ? r1 : mf_affine_silu_to_act_q(x, scale, shift, 1, tq, B, s, post);
}

}  // namespace

// Channel equalisation of the MX blocks (MF_Q_EQUALIZE=0: off).  The FP6 correction planes share one E8M0 scale per 32 CHANNELS: a block's scale follows
// its largest member and a channel more than ~60 x below it loses its correction altogether (e2m3 spans 0.125 ... 7.5) -- with the random-init weights
// of the test suite all channels are alike, in a trained decoder they are not (tools/vae_stress_probe.py: image L-inf 1.4e-4 -> 1.5e-3 with channel
// scales over four decades, bf16x3 7e-5 throughout).  Both operands are known per channel at load time: the activation's expected magnitude
// m_c = E|silu(gamma_c z + beta_c)|, z ~ N(0, 1) (GroupNorm's output is standardised), and the weights' rms over (cout, taps) w_c.  Channel c of the
// activation is divided by e_c = 2^round(log2 sqrt(m_c / w_c)) (median-normalised) and input channel c of the weights multiplied by it: a power of two
// on both sides, so the product and every f16 / FP6 split are unchanged and only the composition of the blocks is -- both operands end up with the
// per-channel profile sqrt(m_c w_c) (the SmoothQuant balance).
bool mf_q_equalize_channels(const float* g, const float* b, const float* w, int cin, int cout, std::vector<float>* post, std::vector<float>* wq) {
    std::vector<double> tt(cin);
    for (int c = 0; c < cin; ++c) {
        double m = 0.0, wsum = 0.0;
        for (int k = 0; k < 64; ++k) {                                        // midpoint rule over z in [-4, 4] against the normal density
            const double z = -4.0 + (k + 0.5) * 0.125, u = (double)g[c] * z + (double)b[c];
            m += std::fabs(u / (1.0 + std::exp(-u))) * std::exp(-0.5 * z * z) * 0.125 * 0.3989422804014327;
        }
        for (int o = 0; o < cout; ++o)
            for (int k = 0; k < 9; ++k) { const double v = w[((int64_t)o * cin + c) * 9 + k]; wsum += v * v; }
        const double wr = std::sqrt(wsum / (9.0 * cout));
        tt[c] = (m > 1e-30 && wr > 1e-30) ? std::sqrt(m / wr) : 0.0;
    }
    std::vector<double> srt;
    for (double v : tt) if (v > 0.0) srt.push_back(v);
    std::sort(srt.begin(), srt.end());
    const double med = srt.empty() ? 1.0 : srt[srt.size() / 2];
    post->assign(cin, 1.f);
    bool any = false;
    wq->assign(w, w + (int64_t)cin * cout * 9);
    for (int c = 0; c < cin; ++c) {
        if (tt[c] <= 0.0) continue;
        int ex = (int)std::lround(std::log2(tt[c] / med));
        ex = std::max(-12, std::min(12, ex));
        if (ex == 0) continue;
        any = true;
        (*post)[c] = (float)std::ldexp(1.0, -ex);
        const float e = (float)std::ldexp(1.0, ex);
        for (int o = 0; o < cout; ++o)
            for (int k = 0; k < 9; ++k) (*wq)[((int64_t)o * cin + c) * 9 + k] *= e;
    }
    return any;
}

Builder::~Builder() {
    sch.graph.drop_all();
    for (auto& p : plans) mf_conv_plan_destroy(p.get());
    for (auto& t : tails) mf_tail_conv_destroy(t.get());
    for (auto& b : bufs) mf_actbuf_free(b.get());
    for (void* d : dev) (void)hipFree(d);
}

int Builder::init(const mf_tensor* weights, int n, int prec, int max_batch, int max_groups, int ln_tokens_per_sample) {
    precision = prec; cap = max_batch;
    gn_affine_fuse = env_on("MF_GN_AFFINE_FUSE");
    if (mf_sd_build(weights, n, "", {}, &sd)) return MF_ERR_INVALID;
    // one slice of fp64 (sum, sum of squares) per GroupNorm op; the whole array is zeroed by ONE kernel at the head
    // of the op list, so a GroupNorm is two launches (statistics, apply) instead of four
    gn_slice = (size_t)max_batch * max_groups * 2;
    // ... and behind them the LayerNorm statistics: two doubles per token and LayerNorm (ln_slot); the caller says how many token slots per sample its
    // transformer blocks need (mf_unet_create counts them from the config; 0: no folding)
    ln_cap_doubles = (size_t)max_batch * ln_tokens_per_sample * 2;
    MF_HIP(hipMalloc(&gn_stats, (GN_MAX_OPS * gn_slice + ln_cap_doubles) * sizeof(double)));
    dev.push_back(gn_stats);
    ln_stats = gn_stats + GN_MAX_OPS * gn_slice;
    {
        double* st = gn_stats;
        const int n = (int)(GN_MAX_OPS * gn_slice + ln_cap_doubles);
        sch.push("groupnorm / layernorm statistics reset", "k_zero_f64", 0.0, [=](int, hipStream_t s) { return mf_zero_f64(st, n, s); });
    }
    // MF_NO_GRAPH=1: every forward an eager launch chain (side branches still forked onto the second stream).  MF_NO_GRAPH=2: eager AND single-stream, no
    // side branches -- the host-lean mode of a serving rank: on ROCm 7.2 any graph launch or cross-stream event wait keeps a runtime thread spinning for
    // as long as the GPU is busy (0.8 - 0.9 host core per process, tools/host_wait_probe2.py), a plain launch chain on one stream does not.
    const int ng = mf_no_graph_mode();
    return sch.init(ng == 0, ng != 2);
}

// ---- resources ----------------------------------------------------------------------------------------
ActBuf* Builder::buf(int C, int H, int W, int halo) {
    bufs.emplace_back(new ActBuf());
    ActBuf* b = bufs.back().get();
    b->C = (C + 7) / 8 * 8; b->H = H; b->W = W; b->halo = halo;
    if (mf_actbuf_alloc(b, cap, precision)) { err = "hipMalloc failed for an activation buffer"; fail_rc = MF_ERR_HIP; return nullptr; }
    return b;
}
ActBuf* Builder::tmp(const std::string& slot, int C, int H, int W, int halo) {
    auto key = std::make_tuple(slot, C, H, W, halo);
    auto it = scratch.find(key);
    if (it != scratch.end()) return it->second;
    ActBuf* b = buf(C, H, W, halo);
    scratch[key] = b;
    return b;
}
float* Builder::upload(const float* host, size_t n) {
    float* d = nullptr;
    if (hipMalloc(&d, n * sizeof(float)) != hipSuccess || (host && hipMemcpy(d, host, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)) {
        err = "upload failed"; fail_rc = MF_ERR_HIP;
        return nullptr;
    }
    dev.push_back(d);
    return d;
}
const float* Builder::T(const std::string& k, int64_t numel) {
    const mf_tensor* t = mf_sd_find(sd, "", k, numel);
    if (!t) { err = mf_last_error(); fail_rc = MF_ERR_INVALID; return nullptr; }
    return t->data;
}
double* Builder::gn_slot() {
    if (gn_count >= GN_MAX_OPS) { err = "more GroupNorm layers than GN_MAX_OPS"; fail_rc = MF_ERR_INVALID; return nullptr; }
    return gn_stats + (size_t)(gn_count++) * gn_slice;
}
double* Builder::ln_slot(const ActBuf* t) {
    const size_t n = (size_t)2 * cap * t->H * t->W;
    if (!ln_stats || ln_used + n > ln_cap_doubles) return nullptr;
    double* p = ln_stats + ln_used;
    ln_used += n;
    return p;
}
int Builder::norm_params(const std::string& name, int C, NormParams* np) {
    np->g = T(name + ".weight", C);
    np->b = T(name + ".bias", C);
    if (!np->g || !np->b) return MF_ERR_INVALID;
    np->dg = upload(np->g, C);
    np->db = upload(np->b, C);
    return got(np->dg, np->db);
}

void Builder::stats_forget(const ActBuf* b) {
    stats_srcs.erase(std::remove_if(stats_srcs.begin(), stats_srcs.end(), [b](const StatsSrc& e) { return e.v.buf == b; }), stats_srcs.end());
}
void Builder::stats_remember(ConvPlan* p, const ActView& v) {
    stats_forget(v.buf);
    stats_srcs.push_back(StatsSrc{p, v});
    if (stats_srcs.size() > 4) stats_srcs.erase(stats_srcs.begin());
}
bool Builder::take_stats(const ActView& x, int groups, double* st) {
    if (x.C % groups || groups > 64 || x.C % 8 || x.coff % 8) return false;
    for (size_t i = 0; i < stats_srcs.size(); ++i) {
        const StatsSrc& e = stats_srcs[i];
        if (e.v.buf != x.buf || e.v.coff != x.coff || e.v.C != x.C || e.p->d.cout != x.C || e.p->out_stats) continue;
        e.p->out_stats = st; e.p->out_stats_groups = groups;
        stats_srcs.erase(stats_srcs.begin() + i);
        return true;
    }
    return false;
}

// ---- ops ----------------------------------------------------------------------------------------------
// one conv launch as an op: names the kernel, pushes the op and (implicit-GEMM candidates) registers it for the tuning table
int Builder::push_conv(const std::string& name, ConvPlan* p, ActView in, ActView out, ActView res, bool tunable, int slot) {
    char kn[96];
    mf_conv_kernel_name(p, cap, kn, sizeof(kn));
    const int op = sch.push(name, kn, mf_conv_flops(p, 1), [p, in, out, res](int B, hipStream_t s) { return mf_conv_launch(p, in, out, res, B, s); }, slot);
    if (tunable) sch.tunable(Schedule::Tunable{p, in, out, res, op});
    return op;
}

// the plan of Conv2d / Linear `name` (k x k, stride, pad) bound to its input; *out may widen (below)
int Builder::conv_plan(const std::string& name, ActView in, ActView* out, int cin, int cout, int k, int stride, int pad, const ConvOpts& o, ConvPlan** plan) {
    const float* w = T(name + ".weight", (int64_t)cin * cout * k * k);
    const float* b = o.bias ? T(name + ".bias", cout) : nullptr;
    if (!w || (o.bias && !b)) return MF_ERR_INVALID;
    float w_scale = o.w_scale;
    std::vector<float> bb(cout, 0.f), ws;
    for (int i = 0; i < cout; ++i) bb[i] = (b ? b[i] : 0.f) + (o.extra_bias ? (*o.extra_bias)[i] : 0.f);
    // A 3x3 layer with a channel count that is not a multiple of 4 (the decoder's conv_out, 128 -> 3) would fall to the
    // implicit-GEMM kernel and re-gather its input once per tap; one zero-weight channel makes it eligible for the LDS
    // halo-tile kernel, which reads the input once (330 -> ~90 us at 256x256).
    if (k == 3 && stride == 1 && pad == 1 && !o.upsample && cout % 4 && cin >= 16 && cin <= 256 && in.buf->H >= 16 && in.buf->W >= 16 &&
        !o.res.buf && out->coff % 4 == 0 && out->coff + (cout + 3) / 4 * 4 <= out->buf->C) {
        const int cp = (cout + 3) / 4 * 4;
        const size_t row = (size_t)cin * k * k;
        std::vector<float> wp(row * cp, 0.f);
        for (int oc = 0; oc < cout; ++oc)
            for (size_t i = 0; i < row; ++i) wp[row * oc + i] = w[row * oc + i] * w_scale;
        bb.resize(cp, 0.f);
        ws.swap(wp);
        w = ws.data();
        w_scale = 1.f;
        cout = cp;
        out->C = cp;
    }
    if (w_scale != 1.f) {
        ws.assign(w, w + (size_t)cin * cout * k * k);
        for (auto& v : ws) v *= w_scale;
        w = ws.data();
    }
    mf_conv2d_desc d = desc_s1(cin, cout, k, pad, *in.buf, o.res);
    d.stride_h = d.stride_w = stride; d.act = o.act; d.upsample = o.upsample; d.pad_hi = o.pad_hi;
    stats_forget(out->buf);
    ConvPlan* p = *plan = new_plan();
    p->ln_gamma = o.ln_gamma; p->ln_beta = o.ln_beta;
    int rc = mf_conv_plan_create(p, d, w, bb.data(), nullptr, nullptr, nullptr, nullptr, precision);
    if (o.ln_in) { p->ln_in = o.ln_in; p->ln_eps = 1e-5f; }
    p->ln_out = o.ln_out;
    return rc ? rc : mf_conv_bind(p, *in.buf);
}
// Conv2d / Linear `name` (k x k, stride, pad) with what ConvOpts asks for
int Builder::conv(const std::string& name, ActView in, ActView out, int cin, int cout, int k, int stride, int pad, const ConvOpts& o) {
    ConvPlan* p = nullptr;
    const int rc = conv_plan(name, in, &out, cin, cout, k, stride, pad, o, &p);
    if (rc) return rc;
    push_conv(name, p, in, out, o.res);
    if (o.act != 5) stats_remember(p, out);
    return MF_OK;
}
int Builder::linear_raw(const float* w, const float* b, ActView in, ActView out, int cin, int cout, const ConvOpts& o) {
    ConvPlan* p = new_plan();
    p->ln_gamma = o.ln_gamma; p->ln_beta = o.ln_beta;
    int rc = mf_conv_plan_create(p, desc_s1(cin, cout, 1, 0, *in.buf, o.res), w, b, nullptr, nullptr, nullptr, nullptr, precision);
    if (o.ln_in) { p->ln_in = o.ln_in; p->ln_eps = 1e-5f; }
    p->ln_out = o.ln_out;
    if (rc) return rc;
    if ((rc = mf_conv_bind(p, *in.buf))) return rc;
    push_conv("fused linear " + std::to_string(cin) + "->" + std::to_string(cout), p, in, out, o.res, true, o.slot);
    return MF_OK;
}

int Builder::gn(const std::string& name, ActView in, ActView out, int groups, float eps, bool silu) {
    NormParams np;
    const int rc = norm_params(name, in.C, &np);
    if (rc) return rc;
    double* st = gn_slot();
    if (!st) return MF_ERR_INVALID;
    const bool epi = take_stats(in, groups, st);
    stats_forget(out.buf);
    const float *dg = np.dg, *db = np.db;
    sch.push(name, epi ? "k_gn_apply (statistics from the producer's epilogue)" : "k_gn_stats+k_gn_apply", 0.0,
             [=](int B, hipStream_t s) { return mf_groupnorm(in, out, dg, db, groups, eps, silu, st, B, s, epi); });
    return MF_OK;
}
int Builder::ln(const std::string& name, ActView in, ActView out) {
    NormParams np;
    const int rc = norm_params(name, in.C, &np);
    if (rc) return rc;
    const float *dg = np.dg, *db = np.db;
    sch.push(name, "k_layernorm", 0.0, [=](int B, hipStream_t s) { return mf_layernorm(in, out, dg, db, 1e-5f, B, s); });
    return MF_OK;
}

// Which path `GroupNorm + SiLU -> conv 3x3 (cin -> cout)` over the normalised tensor `t` takes.
// f16 + FP6 operand format for the wide 3x3 convs on large maps (MF_CONV_Q=0: bf16x3 everywhere): GroupNorm-apply writes the conv's input in the new
// format, the conv runs one f16 + half a block-scaled FP6 MFMA per tap where bf16x3 runs three; outputs and residuals stay bf16 (hi, lo).
Builder::QPath Builder::q_path(int cin, int cout, const ActBuf* t) const {
    if (!switches().conv_q || precision != MF_PREC_BF16X3 || cin % 32 || t->C != cin) return Q_NONE;
    // The UNet's 320-channel convs on its 32 x 32 maps (cout = 2.5 tiles of 128): from 16 frames per step (Q_DUAL_MIN) the f16 + FP6 tile runs them at 640-730 TF where the
    // bf16x3 LDS-weights tile reaches 405-440 (conv alone, 64 frames: 320 -> 320 298 -> 222 us, 640 -> 320 570 -> 412, 960 -> 320 824 -> 599).  A handle serves
    // steps of every size up to its capacity, so BOTH paths are built and a launch picks by its batch.
    // ... and its 640-channel convs on the 16 x 16 maps (one patch per image, five channel tiles): 640 -> 640 360 -> 250 us, 1280 -> 640 651 -> 455, 1920 -> 640 934 -> 675
    // at 64 frames against the bf16x3 implicit GEMM.
    // (bounds as mf_conv_plan_create's q_small / odd_wide predicates: a layer outside them gets no f16 + FP6 plan and must stay on the bf16x3 path -- ADVICE r04:
    // 1280-channel convs on 16 x 16 maps at sample_size 64, or 320-out convs with cin > 1024, failed the whole handle instead)
    const bool q_dual32 = cout >= 256 && cout % 128 != 0 && cout % 64 == 0 && cin <= 1024 && t->H * t->W >= Q_MIN_PX;
    const bool q_dual16 = cout >= 512 && cout <= 1024 && cout % 128 == 0 && cin <= 2048 && t->H == 16 && t->W == 16;
    if (q_dual_allowed && (q_dual32 || q_dual16) && t->H % 16 == 0 && t->W % 16 == 0 && cap >= Q_DUAL_MIN) return Q_DUAL;
    if (q_allowed && cout % 128 == 0 && t->H * t->W >= Q_MIN_PX && cin >= 128 && (int64_t)cap * ((t->H + 15) / 16) * ((t->W + 15) / 16) * (cout / 128) >= 64) return Q_F16Q;
    return Q_NONE;
}

// what both f16 + FP6 paths need: norm parameters, statistics slot, the per-sample affine, the (equalised) f16 + FP6 plan
int Builder::gn_q_prepare(const std::string& gname, const std::string& cname, const ActBuf* t, int cin, int cout, ActView res, const std::vector<float>* extra_bias, bool dual, GnQ* q) {
    int rc = norm_params(gname, cin, &q->np);
    if (rc) return rc;
    const float* w = T(cname + ".weight", (int64_t)cin * cout * 9);
    const float* cb = T(cname + ".bias", cout);
    if (!w || !cb) return MF_ERR_INVALID;
    if (!(q->st = gn_slot())) return MF_ERR_INVALID;
    float* aff = upload(nullptr, (size_t)2 * cap * cin);
    if (!aff) { err = "hipMalloc failed for a GroupNorm affine"; return MF_ERR_HIP; }
    q->scale = aff; q->shift = aff + (size_t)cap * cin;
    std::vector<float> bb(cout), post, wq;
    for (int i = 0; i < cout; ++i) bb[i] = cb[i] + (extra_bias ? (*extra_bias)[i] : 0.f);
    q->d_post = nullptr;
    if (switches().q_equalize && mf_q_equalize_channels(q->np.g, q->np.b, w, cin, cout, &post, &wq)) {
        if (!(q->d_post = upload(post.data(), cin))) return MF_ERR_HIP;
        w = wq.data();
    }
    q->p = new_plan();
    q->p->q_small_maps = dual;
    if ((rc = mf_conv_plan_create(q->p, desc_s1(cin, cout, 3, 1, *t, res), w, bb.data(), nullptr, nullptr, nullptr, nullptr, MF_PREC_F16Q))) return rc;
    if (!q->p->q) { err = cname + ": no kernel in the f16 + FP6 format for this layer"; return MF_ERR_INVALID; }
    return MF_OK;
}

// GroupNorm + SiLU written in the f16 + FP6 format, then the conv of that format
// (GroupNorm-apply + SiLU + the format conversion INSIDE this conv -- the producer waves rewriting each landed halo image -- was built in round 4,
// bit-identical and 2 x slower than the pass it replaces, and removed in round 5: profiles/r04_gn_fuse_q.md keeps the measurement)
int Builder::gn_conv_q(const GnQ& q, const std::string& gname, const std::string& cname, ActView x, ActBuf* t, ActView out, int cin, int groups, float eps, ActView res) {
    const bool epi = take_stats(x, groups, q.st);
    const int rc = mf_conv_bind(q.p, *t);
    if (rc) return rc;
    const ActBuf* tq = t;
    const bool fuse = gn_affine_fuse;
    sch.push(gname, epi ? "k_affine_silu_to_q (statistics from the producer's epilogue)" : "k_gn_stats+k_affine_silu_to_q", 0.0, [=](int B, hipStream_t s) {
        return gn_silu_to_q(x, q.np.dg, q.np.db, groups, eps, q.st, q.scale, q.shift, *tq, B, s, epi, q.d_post, fuse);
    });
    push_conv(cname, q.p, ActView{t, 0, cin}, out, res, false);
    stats_remember(q.p, out);
    return MF_OK;
}

// Both paths of one layer: the bf16x3 path for steps below Q_DUAL_MIN frames (its own plan, LDS-weights tile / implicit-GEMM twin as before), the f16 + FP6
// path from there on; both read the normalised tensor from `t`, whose second plane holds bf16 lo values or FP6 blocks as the path writes them
int Builder::gn_conv_dual(const GnQ& q, const std::string& gname, const std::string& cname, ActView x, ActBuf* t, ActView out, int cin, int cout, int groups, float eps,
                          ActView res, const std::vector<float>* extra_bias) {
    const ActView tv{t, 0, cin};
    ConvPlan *p3 = nullptr, *p = q.p;
    ConvOpts o; o.res = res; o.extra_bias = extra_bias;
    int rc = conv_plan(cname, tv, &out, cin, cout, 3, 1, 1, o, &p3);
    if (rc) return rc;
    if ((rc = mf_conv_bind(p, *t))) return rc;
    const ActBuf* tq = t;
    const bool epi = take_stats(x, groups, q.st);
    const bool fuse = gn_affine_fuse;
    sch.push(gname, epi ? "k_gn_apply | k_affine_silu_to_q from q_dual_min frames (statistics from the producer's epilogue)" : "k_gn_stats+k_gn_apply | +k_affine_silu_to_q from q_dual_min frames", 0.0,
             [=](int B, hipStream_t s) {
                 if (B < Q_DUAL_MIN) return mf_groupnorm(x, tv, q.np.dg, q.np.db, groups, eps, true, q.st, B, s, epi);
                 return gn_silu_to_q(x, q.np.dg, q.np.db, groups, eps, q.st, q.scale, q.shift, *tq, B, s, epi, q.d_post, fuse);
             });
    char kn[96];
    mf_conv_kernel_name(p, cap, kn, sizeof(kn));                   // (a dual-path layer exists only on a handle of >= Q_DUAL_MIN frames)
    const int op = sch.push(cname, kn, mf_conv_flops(p3, 1), [=](int B, hipStream_t s) {
        if (B < Q_DUAL_MIN) return mf_conv_launch(p3, tv, out, res, B, s);
        p->out_stats = p3->out_stats; p->out_stats_groups = p3->out_stats_groups;      // (the consumer GroupNorm asked the remembered plan)
        return mf_conv_launch(p, tv, out, res, B, s);
    });
    sch.tunable(Schedule::Tunable{p3, tv, out, res, op, p, Q_DUAL_MIN});
    stats_remember(p3, out);
    return MF_OK;
}

// `gname` (GroupNorm + SiLU) into scratch `t`, then `cname` (Conv2d 3x3, cin -> cout) from there into `out`
int Builder::gn_conv(const std::string& gname, const std::string& cname, ActView x, ActBuf* t, ActView out, int cin, int cout, int groups, float eps,
                     ActView res, const std::vector<float>* extra_bias) {
    const QPath path = q_path(cin, cout, t);
    if (path == Q_NONE) {
        ConvOpts o; o.res = res; o.extra_bias = extra_bias;
        const int rc = gn(gname, x, ActView{t, 0, cin}, groups, eps, true);
        return rc ? rc : conv(cname, ActView{t, 0, cin}, out, cin, cout, 3, 1, 1, o);
    }
    GnQ q;
    const int rc = gn_q_prepare(gname, cname, t, cin, cout, res, extra_bias, path == Q_DUAL, &q);
    if (rc) return rc;
    return path == Q_DUAL ? gn_conv_dual(q, gname, cname, x, t, out, cin, cout, groups, eps, res, extra_bias) : gn_conv_q(q, gname, cname, x, t, out, cin, groups, eps, res);
}

// `gname` (GroupNorm + SiLU) followed by `cname` (Conv2d 3x3 to <= 16 channels) as ONE pass (mf_conv_tail.hip) where that kernel applies, else the
// two-op chain through a scratch buffer.  MF_TAIL_FUSE=0: always the chain (A/B).
int Builder::gn_conv_tail(const std::string& gname, const std::string& cname, ActView x, ActView out, int cin, int cout, int groups, float eps) {
    // (maps that give a batch of 8 at least 256 patches of 16 x 16: on the UNet's 32 x 32 map the 32 workgroups of the fused kernel measured 63 us against 35)
    if (!switches().tail_fuse || !mf_tail_conv_supported(cin, cout, precision) || x.buf->H % 16 || x.buf->W % 16 || (x.buf->H / 16) * (x.buf->W / 16) < 32) {
        ActBuf* t = buf(cin, x.buf->H, x.buf->W, 1);     // the normalised tensor, only materialised on this path
        if (!t) return MF_ERR_HIP;
        const ActView tv{t, 0, cin};
        const int rc = gn(gname, x, tv, groups, eps, true);
        return rc ? rc : conv(cname, tv, out, cin, cout, 3, 1, 1);
    }
    NormParams np;
    int rc = norm_params(gname, cin, &np);
    if (rc) return rc;
    const float* w = T(cname + ".weight", (int64_t)cout * cin * 9);
    const float* cb = T(cname + ".bias", cout);
    if (!w || !cb) return MF_ERR_INVALID;
    double* st = gn_slot();
    if (!st) return MF_ERR_INVALID;
    tails.emplace_back(new TailConv());
    TailConv* tp = tails.back().get();
    if ((rc = mf_tail_conv_create(tp, w, cb, cin, cout))) return rc;
    const bool epi = take_stats(x, groups, st);
    stats_forget(out.buf);
    const float *dg = np.dg, *db = np.db;
    sch.push(gname + " + " + cname, epi ? "k_gn_conv3_tail (statistics from the producer's epilogue)" : "k_gn_stats+k_gn_conv3_tail",
             2.0 * 9 * cin * cout * x.buf->H * x.buf->W,
             [=](int B, hipStream_t s) { return mf_gn_conv3_tail(*tp, x, dg, db, groups, eps, true, st, epi, out, B, s); });
    return MF_OK;
}

// softmax(q k^T * dh^-0.5) v for `heads` heads; q / k / v / out are views of contiguous (halo 0) token buffers
int Builder::attention(ActView q, ActView k, ActView v, ActView out, int heads) {
    const int C = q.C, dh = C / heads;
    const int Tq = q.buf->H * q.buf->W, Tk = k.buf->H * k.buf->W;
    if (q.buf->halo || k.buf->halo || v.buf->halo || out.buf->halo || dh % 8 || k.C != C || v.C != C || out.C != C) {
        err = "attention: needs contiguous token buffers and a head dim that is a multiple of 8";
        return MF_ERR_INVALID;
    }
    const std::string name = "attention " + std::to_string(Tq) + "x" + std::to_string(Tk) + " heads " + std::to_string(heads) + " dh " + std::to_string(dh);
    const int prec = precision;
    // one fused kernel (mf_attn.hip) for the UNet's head dims; the five-launch composite below serves the others (the VAE mid-block's dh 512)
    if (mf_attention_supported(dh)) {
        sch.push(name, "k_attention", 4.0 * Tq * Tk * C, [=](int B, hipStream_t s) { return mf_attention(q, k, v, out, heads, B, prec, s); });
        return MF_OK;
    }
    const int Tk8 = (Tk + 7) / 8 * 8, Tk64 = (Tk + 63) / 64 * 64;
    auto key = std::make_tuple(dh, Tq, Tk, heads);
    if (!attn_plans.count(key)) {
        ConvPlan* ps = new_plan();
        ConvPlan* pv = new_plan();
        const int rc = mf_attention_composite_plans(ps, pv, dh, Tq, Tk, cap * heads, precision);
        if (rc) return rc;
        attn_plans[key] = {ps, pv};
    }
    ConvPlan* ps = attn_plans[key].first;
    ConvPlan* pv = attn_plans[key].second;
    ActBuf* sc = tmp("attn.scores", Tk8, heads, Tq, 0);
    ActBuf* pm = tmp("attn.probs", Tk64, heads, Tq, 0);
    if (!sc || !pm) return MF_ERR_HIP;
    sch.push(name, "pack+gemm+softmax+pack+gemm", 4.0 * Tq * Tk * C,
             [=](int B, hipStream_t s) { return mf_attention_composite(ps, pv, sc, pm, q, k, v, out, heads, B, prec, s); });
    return MF_OK;
}

// diffusers Upsample2D (nearest 2x + conv 3x3) in the f16 + FP6 operand format where the layer fills the chip that way: a converter pass writes
// the input in the format (identity affine, no SiLU), then four 2 x 2-tap phase launches of the f16 + FP6 halo tile, which also leave the
// consumer GroupNorm's statistics.  Elsewhere (small maps, other precisions, MF_CONV_Q=0): the 4-phase implicit GEMM on bf16x3.
int Builder::upsample_conv(const std::string& name, ActView x, ActView out, int C) {
    const int H = x.buf->H, W = x.buf->W;
    if (!(switches().conv_q && q_allowed && precision == MF_PREC_BF16X3 && C % 128 == 0 && x.C == C && x.coff % 8 == 0 && H * W >= 32 * 32 &&
          (int64_t)cap * ((H + 15) / 16) * ((W + 15) / 16) * (C / 128) >= MF_UP_Q_MIN_WG)) {
        ConvOpts o; o.upsample = 1;
        return conv(name, x, out, C, C, 3, 1, 1, o);
    }
    const float* w = T(name + ".weight", (int64_t)C * C * 9);
    const float* b = T(name + ".bias", C);
    if (!w || !b) return MF_ERR_INVALID;
    ActBuf* tq = tmp("up.q", C, H, W, 1);
    if (!tq) return MF_ERR_HIP;
    std::vector<float> ones((size_t)cap * C, 1.f), zeros((size_t)cap * C, 0.f);
    float *d1 = upload(ones.data(), ones.size()), *d0 = upload(zeros.data(), zeros.size());
    if (!d1 || !d0) return MF_ERR_HIP;
    mf_conv2d_desc d = desc_s1(C, C, 3, 1, *x.buf, ActView{});
    d.upsample = 1;
    ConvPlan* p = new_plan();
    int rc = mf_conv_plan_create(p, d, w, b, nullptr, nullptr, nullptr, nullptr, MF_PREC_F16Q);
    if (rc) return rc;
    if ((rc = mf_conv_bind(p, *tq))) return rc;
    stats_forget(out.buf);
    const ActBuf* tqc = tq;
    sch.push(name + " (input -> f16 + FP6)", "k_affine_silu_to_q (identity)", 0.0, [=](int B, hipStream_t s) { return mf_affine_silu_to_act_q(x, d1, d0, 0, *tqc, B, s); });
    push_conv(name, p, ActView{tq, 0, C}, out, ActView{}, false);
    stats_remember(p, out);
    return MF_OK;
}

// ---- blocks -------------------------------------------------------------------------------------------
// diffusers ResnetBlock2D; temb_act = silu(time_embedding) on the host (nullptr: VAE)
int Builder::resnet(const std::string& p, ActView x, ActView y, int cin, int cout, int groups, float eps, const std::vector<float>* temb_act) {
    const int H = x.buf->H, W = x.buf->W;
    ActBuf *t1 = tmp("rn.t1", cin, H, W, 1), *c1 = tmp("rn.c1", cout, H, W, 1), *t2 = tmp("rn.t2", cout, H, W, 1);
    if (!t1 || !c1 || !t2) return MF_ERR_HIP;
    int rc;
    std::vector<float> tb;
    if (temb_act && has(p + ".time_emb_proj.weight")) {
        const int td = (int)temb_act->size();
        const float* w = T(p + ".time_emb_proj.weight", (int64_t)cout * td);
        const float* b = T(p + ".time_emb_proj.bias", cout);
        if (!w || !b) return MF_ERR_INVALID;
        tb.resize(cout);
        for (int o = 0; o < cout; ++o) {
            double a = b[o];
            for (int i = 0; i < td; ++i) a += (double)w[(size_t)o * td + i] * (*temb_act)[i];
            tb[o] = (float)a;
        }
    }
    // the 1x1 shortcut reads only the block's input: first in the list, on the side branch, joined where conv2 adds it
    ActView res = x;
    int sc_op = -1;
    if (has(p + ".conv_shortcut.weight")) {
        ActBuf* sc = tmp("rn.sc", cout, H, W, 1);
        if (!sc) return MF_ERR_HIP;
        if ((rc = conv(p + ".conv_shortcut", x, ActView{sc, 0, cout}, cin, cout, 1, 1, 0))) return rc;
        res = ActView{sc, 0, cout};
        sc_op = (int)sch.ops.size() - 1;
        sch.mark_side(sc_op);
    } else if (cin != cout) {
        err = p + ": cin != cout but no conv_shortcut in the state dict";
        return MF_ERR_INVALID;
    }
    if ((rc = gn_conv(p + ".norm1", p + ".conv1", x, t1, ActView{c1, 0, cout}, cin, cout, groups, eps, ActView{}, tb.empty() ? nullptr : &tb))) return rc;
    if (sc_op >= 0) sch.join_here(sc_op);
    return gn_conv(p + ".norm2", p + ".conv2", ActView{c1, 0, cout}, t2, y, cout, cout, groups, eps, res);
}

// diffusers Transformer2DModel (conv projections) with one BasicTransformerBlock; ctx = audio tokens
int Builder::transformer(const std::string& p, ActView x, ActView y, int C, int heads, int groups, ActView ctx, KvHoist* kv) {
    const int H = x.buf->H, W = x.buf->W, X = ctx.C;
    ActBuf *g0 = tmp("xf.gn", C, H, W, 0), *hA = tmp("xf.hA", C, H, W, 0), *hB = tmp("xf.hB", C, H, W, 0);
    ActBuf *nb = tmp("xf.ln", C, H, W, 0), *qkv = tmp("xf.qkv", 3 * C, H, W, 0), *ao = tmp("xf.ao", C, H, W, 0);
    // ff.net.2 and proj_out folded into one layer (ff_proj_out): the feed-forward buffer is [GEGLU output (4C) | residual stream behind the cross-attention (C)],
    // the one input of that layer; attn2.to_out writes the slice, norm3 / ff.net.0.proj read it
    const bool ffold = switches().ff_proj_fold == 2 || (switches().ff_proj_fold == 1 && ff_fold_measured(C, H, W));
    ActBuf *kvb = tmp("xf.kv", 2 * C, ctx.buf->H, ctx.buf->W, 0), *gg = tmp("xf.geglu", (ffold ? 5 : 4) * C, H, W, 0);
    if (!g0 || !hA || !hB || !nb || !qkv || !ao || !kvb || !gg) return MF_ERR_HIP;
    const std::string t = p + ".transformer_blocks.0";
    const ActView vg{g0, 0, C}, vA{hA, 0, C}, vB{hB, 0, C}, vn{nb, 0, C}, va{ao, 0, C}, vq{qkv, 0, C};
    const ActView vR = ffold ? ActView{gg, 4 * C, C} : vA;
    int rc;
    // The three LayerNorms are FOLDED into the GEMMs around them where the statistics buffer has room (it has, for the shipped configurations): the producer of
    // the residual stream (proj_in, attn1.to_out + x, attn2.to_out + x) leaves every token's (sum, sum of squares), the consumer (q | k | v, attn2.to_q, the
    // GEGLU projection) multiplies the RAW stream by gamma-scaled weights and its epilogue applies rstd * (acc - mean * colsum) + (bias + W beta).
    double *st1 = ln_slot(hA), *st2 = ln_slot(hB), *st3 = ln_slot(hA);
    const bool fold = st1 && st2 && st3;
    // norm `name` over `stream` in front of a GEMM: folded (the producer left `st`, the consumer's options take gamma / beta / st and read the raw stream) or as its own op into nb
    auto norm = [&](const std::string& name, ActView stream, double* st, ConvOpts* o, ActView* in) {
        *in = fold ? stream : vn;
        if (!fold) return ln(name, stream, vn);
        o->ln_gamma = T(name + ".weight", C); o->ln_beta = T(name + ".bias", C); o->ln_in = st;
        return got(o->ln_gamma, o->ln_beta);
    };
    auto producer = [&](ActView res, double* st) { ConvOpts o; o.res = res; if (fold) o.ln_out = st; return o; };
    if ((rc = gn(p + ".norm", x, vg, groups, 1e-6f, false))) return rc;
    if ((rc = conv(p + ".proj_in", vg, vA, C, C, 1, 1, 0, producer(ActView{}, st1)))) return rc;
    // self attention: q | k | v in one GEMM (no bias)
    ActView in;
    {
        ConvOpts o;
        if ((rc = norm(t + ".norm1", vA, st1, &o, &in))) return rc;
        const float *wq = T(t + ".attn1.to_q.weight", (int64_t)C * C), *wk = T(t + ".attn1.to_k.weight", (int64_t)C * C), *wv = T(t + ".attn1.to_v.weight", (int64_t)C * C);
        if (!wq || !wk || !wv) return MF_ERR_INVALID;
        if ((rc = linear_raw(cat_rows({wq, wk, wv}, (size_t)C * C).data(), nullptr, in, ActView{qkv, 0, 3 * C}, C, 3 * C, o))) return rc;
    }
    if ((rc = attention(vq, ActView{qkv, C, C}, ActView{qkv, 2 * C, C}, va, heads))) return rc;
    if ((rc = conv(t + ".attn1.to_out.0", va, vB, C, C, 1, 1, 0, producer(vA, st2)))) return rc;
    // cross attention over the audio tokens: k | v in one GEMM
    {
        ConvOpts o; o.bias = false;
        if ((rc = norm(t + ".norm2", vB, st2, &o, &in))) return rc;
        if ((rc = conv(t + ".attn2.to_q", in, vq, C, C, 1, 1, 0, o))) return rc;
    }
    ActView kk{kvb, 0, C}, vv{kvb, C, C};
    {
        const float *wk = T(t + ".attn2.to_k.weight", (int64_t)C * X), *wv = T(t + ".attn2.to_v.weight", (int64_t)C * X);
        if (!wk || !wv) return MF_ERR_INVALID;
        if (kv && kv->all && kv->off + 2 * C <= kv->all->C && ctx.buf == kv->ctx.buf) {
            // rows [off, off + 2 C) of the hoisted GEMM (hoist_kv_finish); the side branch is joined before the first cross-attention
            kv->w.insert(kv->w.end(), wk, wk + (size_t)C * X);
            kv->w.insert(kv->w.end(), wv, wv + (size_t)C * X);
            kk = ActView{kv->all, kv->off, C}; vv = ActView{kv->all, kv->off + C, C};
            kv->off += 2 * C;
            if (!kv->joined) { sch.join_here(kv->op); kv->joined = true; }
        } else if ((rc = linear_raw(cat_rows({wk, wv}, (size_t)C * X).data(), nullptr, ctx, ActView{kvb, 0, 2 * C}, X, 2 * C))) return rc;
    }
    if ((rc = attention(vq, kk, vv, va, heads))) return rc;
    if ((rc = conv(t + ".attn2.to_out.0", va, vR, C, C, 1, 1, 0, producer(vB, st3)))) return rc;
    // GEGLU feed-forward; GEGLU in the GEMM epilogue (act 5): the 8C-wide projection never reaches HBM, only value * gelu(gate)
    {
        ConvOpts o; o.act = 5;
        if ((rc = norm(t + ".norm3", vR, st3, &o, &in))) return rc;
        if ((rc = conv(t + ".ff.net.0.proj", in, ActView{gg, 0, 4 * C}, C, 8 * C, 1, 1, 0, o))) return rc;
    }
    if (ffold) return ff_proj_out(t + ".ff.net.2", p + ".proj_out", ActView{gg, 0, 5 * C}, y, x, C);
    ConvOpts ff2, po; ff2.res = vR; po.res = x;
    if ((rc = conv(t + ".ff.net.2", ActView{gg, 0, 4 * C}, vB, 4 * C, C, 1, 1, 0, ff2))) return rc;
    return conv(p + ".proj_out", vB, y, C, C, 1, 1, 0, po);
}

// The fold is taken by default only where the fused layer (K = 5C, N = C, block-input residual) has a measured row in the tuning table at this handle's capacity,
// with or without the GroupNorm-statistics hand-off: a fused layer on the cost model's default tile is the likeliest way for the fold to lose, and the gain was
// measured on the 8-frame handle (profiles/unet_ff_proj_fold.md).  Handles for more frames, and networks the table does not serve, keep the two-op chain.
bool Builder::ff_fold_measured(int C, int H, int W) {
    ActBuf b;
    b.C = 5 * C; b.H = H; b.W = W;
    const ActView in{&b, 0, 5 * C};
    ConvPlan pl;
    pl.d = desc_s1(5 * C, C, 1, 0, b, ActView{&b, 0, C});
    pl.precision = precision; pl.Hq = pl.out_h = H; pl.Wq = pl.out_w = W;
    if (mf_conv_tune_lookup(&pl, in, cap)) return true;
    double stats_asked = 0.0;
    pl.out_stats = &stats_asked;                     // (the key of a layer whose consumer GroupNorm takes its statistics)
    return mf_conv_tune_lookup(&pl, in, cap) != 0;
}

// ff.net.2 (+ the residual stream r) followed by proj_out (+ the block's input x) as ONE 1x1 layer: nothing nonlinear lies between them, so
//     y = W_po (W_f2 gg + b_f2 + r) + b_po + x = [W_po W_f2 | W_po] [gg ; r] + (W_po b_f2 + b_po) + x
// with K = 5C over the buffer `in` = [gg | r].  The products are formed in double and rounded once (as the time embedding in mf_unet_create); the layer's FLOP
// figure, 2 * 5C * C per token, is the sum of the two layers it replaces.  Per block: one launch, one write and one read of the token stream less.
int Builder::ff_proj_out(const std::string& f2, const std::string& po, ActView in, ActView y, ActView x, int C) {
    const int K4 = 4 * C, K = 5 * C;
    const float *w2 = T(f2 + ".weight", (int64_t)C * K4), *b2 = T(f2 + ".bias", C);
    const float *wp = T(po + ".weight", (int64_t)C * C), *bp = T(po + ".bias", C);
    if (!w2 || !b2 || !wp || !bp) return MF_ERR_INVALID;
    std::vector<float> w((size_t)C * K), b(C);
    // W_po W_f2, eight output rows at a time against column blocks of W_f2 that stay in cache
    const int OB = 8, KB = 512;
    parallel_for((C + OB - 1) / OB, [&](int ob) {
        const int o0 = ob * OB, on = std::min(OB, C - o0);
        std::vector<double> acc((size_t)OB * KB);
        for (int k0 = 0; k0 < K4; k0 += KB) {
            const int kn = std::min(KB, K4 - k0);
            std::fill(acc.begin(), acc.end(), 0.0);
            for (int m = 0; m < C; ++m) {
                const float* r2 = w2 + (size_t)m * K4 + k0;
                for (int o = 0; o < on; ++o) {
                    const double a = wp[(size_t)(o0 + o) * C + m];
                    double* row = acc.data() + (size_t)o * KB;
                    for (int k = 0; k < kn; ++k) row[k] += a * (double)r2[k];
                }
            }
            for (int o = 0; o < on; ++o)
                for (int k = 0; k < kn; ++k) w[(size_t)(o0 + o) * K + k0 + k] = (float)acc[(size_t)o * KB + k];
        }
        for (int o = o0; o < o0 + on; ++o) {
            double bias = bp[o];
            for (int m = 0; m < C; ++m) bias += (double)wp[(size_t)o * C + m] * (double)b2[m];
            b[o] = (float)bias;
            std::copy(wp + (size_t)o * C, wp + (size_t)(o + 1) * C, w.begin() + (size_t)o * K + K4);
        }
    });
    ConvPlan* pl = new_plan();
    stats_forget(y.buf);
    int rc = mf_conv_plan_create(pl, desc_s1(K, C, 1, 0, *in.buf, x), w.data(), b.data(), nullptr, nullptr, nullptr, nullptr, precision);
    if (rc) return rc;
    if ((rc = mf_conv_bind(pl, *in.buf))) return rc;
    push_conv(f2 + "+proj_out", pl, in, y, x);
    stats_remember(pl, y);
    return MF_OK;
}

// the VAE mid block's single-head attention over all channels (decoder and encoder): GroupNorm, q | k | v in one GEMM, attention, to_out + residual
int Builder::vae_mid_attention(const std::string& a, ActView x, ActView y, ActView residual, int groups) {
    const int ch = x.C, s = x.buf->H;
    ActBuf *g0 = tmp("va.gn", ch, s, s, 0), *qkv = tmp("va.qkv", 3 * ch, s, s, 0), *ao = tmp("va.ao", ch, s, s, 0);
    if (!g0 || !qkv || !ao) return MF_ERR_HIP;
    int rc;
    if ((rc = gn(a + ".group_norm", x, ActView{g0, 0, ch}, groups, 1e-6f, false))) return rc;
    const float *wq = T(a + ".to_q.weight", (int64_t)ch * ch), *wk = T(a + ".to_k.weight", (int64_t)ch * ch), *wv = T(a + ".to_v.weight", (int64_t)ch * ch);
    const float *bq = T(a + ".to_q.bias", ch), *bk = T(a + ".to_k.bias", ch), *bv = T(a + ".to_v.bias", ch);
    if (!wq || !wk || !wv || !bq || !bk || !bv) return MF_ERR_INVALID;
    if ((rc = linear_raw(cat_rows({wq, wk, wv}, (size_t)ch * ch).data(), cat_rows({bq, bk, bv}, ch).data(), ActView{g0, 0, ch}, ActView{qkv, 0, 3 * ch}, ch, 3 * ch))) return rc;
    if ((rc = attention(ActView{qkv, 0, ch}, ActView{qkv, ch, ch}, ActView{qkv, 2 * ch, ch}, ActView{ao, 0, ch}, 1))) return rc;
    ConvOpts o; o.res = residual;
    return conv(a + ".to_out.0", ActView{ao, 0, ch}, y, ch, ch, 1, 1, 0, o);
}

// hoisted cross-attention k | v: reserve the op slot before the blocks are built ...
int Builder::hoist_kv_begin(KvHoist* kv, ActView ctx, int total) {
    if (total <= 0) return MF_OK;
    if (!(kv->all = buf(total, ctx.buf->H, ctx.buf->W, 0))) return MF_ERR_HIP;
    kv->ctx = ctx;
    kv->op = sch.reserve("cross-attention k | v of every block");
    sch.mark_side(kv->op);                 // depends on the audio tokens only: a side branch until the first cross-attention
    return MF_OK;
}
// ... and fill it once every block has handed in its rows
int Builder::hoist_kv_finish(KvHoist* kv) {
    if (!kv->all) return MF_OK;
    if (kv->off != kv->all->C) { err = "hoisted k | v width does not match the blocks that were built"; return MF_ERR_INVALID; }
    ConvOpts o; o.slot = kv->op;
    const int rc = linear_raw(kv->w.data(), nullptr, kv->ctx, ActView{kv->all, 0, kv->off}, kv->ctx.C, kv->off, o);
    if (rc) return rc;
    sch.info[kv->op].name += " (cross-attention k | v of every block)";
    kv->w.clear(); kv->w.shrink_to_fit();
    return MF_OK;
}
