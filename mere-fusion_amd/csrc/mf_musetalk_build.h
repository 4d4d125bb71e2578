// The builder of the MuseTalk schedules (mf_musetalk.hip: UNet, VAE decoder, VAE encoder): it owns a handle's resources -- state dict, activation buffers,
// scratch slots, uploads, conv plans, the GroupNorm / LayerNorm statistics slab -- and turns layers (conv, GroupNorm + conv, attention) and blocks (resnet,
// transformer) into ops of a Schedule (mf_schedule.h).  What one op hands to another is an argument: ConvOpts for a conv, KvHoist for the hoisted k | v GEMM.
#pragma once
#include "mf_nn.h"
#include "mf_aux.h"
#include "mf_schedule.h"
#include <memory>
#include <tuple>

// What a conv() / linear_raw() call may ask for beyond its geometry.
struct ConvOpts {
    int act = 0;                                   // 0 none, SiLU etc., 5 GEGLU (mf_conv2d_desc::act)
    ActView res{};                                 // residual added in the epilogue
    int upsample = 0;                              // nearest 2x in front
    const std::vector<float>* extra_bias = nullptr;   // per-channel constant added to the bias
    float w_scale = 1.f;                           // input scale, folded into the weights
    bool bias = true;
    int pad_hi = 0;                                // extra zero rows / columns bottom-right (the VAE encoder's Downsample2D)
    // LayerNorm folded into the GEMMs either side of it (ConvArgs::ln_*): per LayerNorm one fp64 (sum, sum of squares) pair per token, zeroed by the
    // statistics-reset kernel at the head of the list, filled by the producing layer's epilogue (ln_out), consumed by the epilogue of the layer that
    // follows the norm (ln_gamma / ln_beta: host, cin floats; ln_in: the statistics)
    const float* ln_gamma = nullptr; const float* ln_beta = nullptr; const double* ln_in = nullptr;
    double* ln_out = nullptr;
    int slot = -1;                                 // fill this reserved op of the schedule instead of appending
};

// Cross-attention keys / values depend on the audio tokens only: the k | v projections of EVERY transformer block as one GEMM at the head of
// the schedule (all = [ctx_len][sum of 2 C]) instead of one small launch per block inside the chain (16 x ~14 us in the UNet at batch 8).
// hoist_kv_begin reserves the op, each transformer() hands in its rows and takes its slice, hoist_kv_finish fills the op.
struct KvHoist { ActBuf* all = nullptr; ActView ctx{}; int off = 0, op = -1; std::vector<float> w; bool joined = false; };

struct Builder {
    int precision = MF_PREC_BF16X3;
    int cap = 1;
    Schedule sch;
    MfStateDict sd;
    std::vector<std::unique_ptr<ActBuf>> bufs;
    std::vector<std::unique_ptr<ConvPlan>> plans;
    std::vector<std::unique_ptr<TailConv>> tails;
    std::vector<void*> dev;
    std::map<std::tuple<std::string, int, int, int, int>, ActBuf*> scratch;
    std::map<std::tuple<int, int, int, int>, std::pair<ConvPlan*, ConvPlan*>> attn_plans;   // (dh, Tq, Tk, heads)
    double* gn_stats = nullptr;
    static constexpr int GN_MAX_OPS = 96;
    size_t gn_slice = 0;
    int gn_count = 0;
    double* ln_stats = nullptr;              // [ln_total] doubles behind gn_stats (one allocation, one reset launch)
    size_t ln_used = 0, ln_cap_doubles = 0;
    bool gn_affine_fuse = true;              // MF_GN_AFFINE_FUSE, read per handle (tests build both in one process)
    bool q_allowed = false;     // the f16 + FP6 conv format: the VAE decoder's resnets (set by the builder of a network whose parity was established with it)
    bool q_dual_allowed = false;   // ... and, from Q_DUAL_MIN frames per step, the UNet's 320-channel 3x3 convs on its 32 x 32 maps (gn_conv builds both paths, a launch picks by its batch)
    std::string err;
    int fail_rc = MF_ERR_HIP;   // what got() returns: the status of the resource call that failed last
    // the last conv and the view it filled: a GroupNorm that reads exactly that view next takes its statistics from the conv's launch
    // (ConvPlan::out_stats: epilogue, split-K combine, or a statistics pass behind the conv) instead of running its own pass over the tensor.
    // Cleared by any other op that writes the buffer.
    // (A few recent producers are remembered: a resnet's shortcut conv runs between conv1 and the norm2 that reads conv1's output.)
    struct StatsSrc { ConvPlan* p; ActView v; };
    std::vector<StatsSrc> stats_srcs;

    ~Builder();
    int init(const mf_tensor* weights, int n, int prec, int max_batch, int max_groups, int ln_tokens_per_sample = 0);

    // ---- resources: null on failure, with err and fail_rc set -----------------------------------------------
    ActBuf* buf(int C, int H, int W, int halo);
    ActBuf* tmp(const std::string& slot, int C, int H, int W, int halo);   // scratch reused by every block that asks for the same (slot, shape): blocks run one after another
    float* upload(const float* host, size_t n);
    const float* T(const std::string& k, int64_t numel);
    bool has(const std::string& k) const { return sd.count(k) != 0; }
    template <class... P> int got(const P*... p) const { return (... && p) ? MF_OK : fail_rc; }   // every pointer the calls above handed back is there
    ConvPlan* new_plan() { plans.emplace_back(new ConvPlan()); return plans.back().get(); }
    double* gn_slot();                                             // statistics of one GroupNorm op
    double* ln_slot(const ActBuf* t);                              // statistics of one LayerNorm over token buffer t (null: no room, the norm is not folded)
    struct NormParams { const float *g = nullptr, *b = nullptr; float *dg = nullptr, *db = nullptr; };   // gamma / beta on the host and on the device
    int norm_params(const std::string& name, int C, NormParams* np);

    // ---- ops --------------------------------------------------------------------------------------------------
    int push_conv(const std::string& name, ConvPlan* p, ActView in, ActView out, ActView res, bool tunable = true, int slot = -1);
    int conv(const std::string& name, ActView in, ActView out, int cin, int cout, int k, int stride, int pad, const ConvOpts& o = ConvOpts());
    int linear_raw(const float* w, const float* b, ActView in, ActView out, int cin, int cout, const ConvOpts& o = ConvOpts());
    int gn(const std::string& name, ActView in, ActView out, int groups, float eps, bool silu);
    int ln(const std::string& name, ActView in, ActView out);
    int gn_conv(const std::string& gname, const std::string& cname, ActView x, ActBuf* t, ActView out, int cin, int cout, int groups, float eps, ActView res,
                const std::vector<float>* extra_bias = nullptr);
    int gn_conv_tail(const std::string& gname, const std::string& cname, ActView x, ActView out, int cin, int cout, int groups, float eps);
    int upsample_conv(const std::string& name, ActView x, ActView out, int C);
    int attention(ActView q, ActView k, ActView v, ActView out, int heads);

    // ---- blocks -----------------------------------------------------------------------------------------------
    int resnet(const std::string& p, ActView x, ActView y, int cin, int cout, int groups, float eps, const std::vector<float>* temb_act);
    int transformer(const std::string& p, ActView x, ActView y, int C, int heads, int groups, ActView ctx, KvHoist* kv);
    int ff_proj_out(const std::string& f2, const std::string& po, ActView in, ActView y, ActView x, int C);   // a transformer block's ff.net.2 + proj_out as one layer
    bool ff_fold_measured(int C, int H, int W);   // the tuning table holds the fused layer of a C-channel block on an H x W map at this handle's capacity
    int vae_mid_attention(const std::string& a, ActView x, ActView y, ActView residual, int groups);
    int hoist_kv_begin(KvHoist* kv, ActView ctx, int total);
    int hoist_kv_finish(KvHoist* kv);

private:
    enum QPath { Q_NONE, Q_F16Q, Q_DUAL };
    struct GnQ { NormParams np; double* st; float *scale, *shift, *d_post; ConvPlan* p; };   // what the two f16 + FP6 builders share
    QPath q_path(int cin, int cout, const ActBuf* t) const;
    int gn_q_prepare(const std::string& gname, const std::string& cname, const ActBuf* t, int cin, int cout, ActView res, const std::vector<float>* extra_bias, bool dual, GnQ* q);
    int gn_conv_q(const GnQ& q, const std::string& gname, const std::string& cname, ActView x, ActBuf* t, ActView out, int cin, int groups, float eps, ActView res);
    int gn_conv_dual(const GnQ& q, const std::string& gname, const std::string& cname, ActView x, ActBuf* t, ActView out, int cin, int cout, int groups, float eps, ActView res,
                     const std::vector<float>* extra_bias);
    int conv_plan(const std::string& name, ActView in, ActView* out, int cin, int cout, int k, int stride, int pad, const ConvOpts& o, ConvPlan** plan);
    void stats_forget(const ActBuf* b);
    void stats_remember(ConvPlan* p, const ActView& v);
    bool take_stats(const ActView& x, int groups, double* st);     // statistics for GroupNorm(groups) of `x` come from its producer's epilogue?
};

// Channel equalisation of the f16 + FP6 operands (host arithmetic only; the comment at its definition).  g, b: GroupNorm gamma / beta [cin]; w: conv weights
// [cout][cin][3][3].  True: post[cin] holds the activation's per-channel factors and wq the rescaled weights; false: nothing to do.
bool mf_q_equalize_channels(const float* g, const float* b, const float* w, int cin, int cout, std::vector<float>* post, std::vector<float>* wq);

#define NET_TRY(expr)                                                                      \
    do {                                                                                   \
        int rc_ = (expr);                                                                  \
        if (rc_ != MF_OK) {                                                                \
            if (!net.err.empty()) mf_set_error("%s", net.err.c_str());                     \
            return rc_;                                                                    \
        }                                                                                  \
    } while (0)
