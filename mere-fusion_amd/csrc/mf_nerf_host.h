// Host-side declarations shared by the ER-NeRF translation units (mf_nerf*.hip): every host function that one of them defines and another calls, the plain
// structs that carry the argument groups between them, and the field handle the render loop reads.  The file that defines a function and every file that calls it
// include this header, so a prototype that drifts is a compile error.  Nothing here is passed to a kernel: the launchers copy what they need into their own
// kernel-argument structs (FusedArgs, TailArgs, TorsoFusedArgs, ...).
#pragma once
#include "mf_nn.h"
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

// ---- argument groups (aggregate-initialised where they are used, passed by const&) ---------------------------------------------------------------
struct NerfFieldConsts {                 // what a field handle holds for the fused kernels (mf_nerf_field::consts)
    const bf16_t* packed;                // weight fragments of mf_nerf_fused_pack
    bool x3;
    const float* emb[3];                 // tri-plane embedding tables (xy, yz, xz)
    const int* offsets;                  // host: num_levels + 1 level offsets
    float log2_pls;
    int base_res;
    float bound;
    int n_ind, has_eye;
};
struct NerfFrameInputs {                 // per frame
    const float *enc_a, *ind;            // device: audio feature [32], individual code [n_ind] (or null)
    float eye;
    const float* eye_dev;                // the eye feature read on the device instead of `eye`, or null
    float sigma_scale;                   // NeRFRenderer.density_scale (renderer.py:261)
};
struct NerfFieldOut { float *sigmas, *rgbs, *amb_aud, *amb_eye, *unc; };     // per sample; unc may be null
struct NerfRaySums { float *wsum, *depth, *image, *aasum, *aesum, *unsum; };  // per ray
struct NerfLoop {                        // the device-controlled render loop of one frame
    int* ctl;                            // control block (mf_nerf_march.h)
    int N, max_steps;
    int* alive[2];                       // round r reads alive[r & 1] and appends its survivors to the other
    float *rays_t, *fars;                // (fars: written by the init launch)
    const float *rays_o, *rays_d;
    const uint8_t* bitfield;
    uint32_t cascades, grid_size;
    float dt_gamma, T_thresh;
    float *xyzs, *dirs, *deltas;         // the round's samples
    bool skip_empty;                     // MF_NERF_SKIP_EMPTY, read once per frame: the field skips fragments whose slots hold no sample
    const float* skip_deltas() const { return skip_empty ? deltas : nullptr; }    // what the field kernels get as FusedArgs::deltas
};
struct LoopFrame;                        // mf_nerf_march.h: one frame of a batch as the kernels read it
struct NerfBatchLoop {                   // the render loops of the frames of one mf_nerf_head_batch_render call: what the frames share
    const LoopFrame* frames;             // device table, n_frames entries
    int n_frames, N, max_steps;
    const uint8_t* bitfield;
    uint32_t cascades, grid_size;
    float dt_gamma, T_thresh;
    bool skip_empty;                     // as NerfLoop::skip_empty
};
struct NerfGridBufs { float* density_grid; uint8_t* bitfield; float *tmp_grid, *xyzs_out; double *mean_density, *partials; };   // mf_nerf_density_grid_update's
struct NerfTorsoConsts {                 // what a torso handle holds for the fused kernel
    const float *w, *emb;                // device: the six layers' fp32 tables (mf_nerf_torso_fused_weight_count entries), the tiled grid's embedding
    const int* offsets;                  // host: 17 level offsets
    float log2_pls;
    int base_res;
    float shrink;
    int G;                               // density_grid_torso is G x G
};

// ---- mf_nerf_fused.hip: the whole field as one kernel ---------------------------------------------------------------------------------------------
// w: the nine [cout][cin] matrices in reference order (aud0, aud1, eye0, eye1, sig0, sig1, sig2, col0, col1; eye* may be null)
int mf_nerf_fused_pack(const float* const w[9], int n_ind, bool has_eye, bool x3, bf16_t** dev_out);
// round: the samples are a render-loop round's (their count is read on the device from ctl[3], empty fragments are skipped as round->skip_empty says)
int mf_nerf_fused_launch(const NerfFieldConsts& f, const NerfFrameInputs& in, const float* xyzs, const float* dirs, int M, const NerfFieldOut& out, hipStream_t s,
                         const NerfLoop* round = nullptr);
// the rounds after the `rounds_launched` that were enqueued as launches, in one launch (k_loop_tail)
int mf_nerf_tail_launch(const NerfFieldConsts& f, const NerfFrameInputs& in, const NerfFieldOut& out, const NerfLoop& loop, const NerfRaySums& sums,
                        int rounds_launched, hipStream_t s);

// one launch for the round's samples of every frame of a batch: a workgroup stages the weights once and walks (frame, tile) pairs (k_nerf_field_batch)
int mf_nerf_fused_batch_launch(const NerfFieldConsts& f, float sigma_scale, const NerfBatchLoop& b, hipStream_t s);

// ---- the render loop's limits and switches shared by mf_nerf_head.hip and mf_nerf_head_batch.hip ---------------------------------------------------
constexpr int HEAD_MAX_ROUNDS = 1024;     // max_steps accepted by mf_nerf_head_render (one round per step at least: renderer.py:270); the control block holds tail tickets for as many
// MF_NERF_TAIL_AFTER=<k> fixes how many rounds go out as launches (tests, A/B: 0 = the tail runs the whole loop, "off" = launches only, as before round 6); read per
// call.  Returns that count, or -1 when the variable is not set.
inline int nerf_tail_after_env(int max_steps) {
    const char* e = getenv("MF_NERF_TAIL_AFTER");
    if (!(e && *e)) return -1;
    if (!strcmp(e, "off")) return max_steps;
    const int k = atoi(e);
    return k < 0 ? max_steps : (k < max_steps ? k : max_steps);
}
// MF_NERF_SKIP_EMPTY=0: evaluate every slot as the reference does (A/B); read per call.  What NerfLoop::skip_empty / NerfBatchLoop::skip_empty get
inline bool nerf_skip_empty_env() {
    const char* e = getenv("MF_NERF_SKIP_EMPTY");
    return !(e && e[0] == '0');
}

// ---- mf_nerf.hip: the launches of a round --------------------------------------------------------------------------------------------------------
// init: alive[0] = 0..N-1, near / far of every ray (raymarching.cu:92-145), zeroed sums, the first round's head
int mf_nerf_loop_init(const NerfLoop& loop, const NerfRaySums& sums, float* nears, const float* aabb, float min_near, hipStream_t s);
int mf_nerf_loop_march(const NerfLoop& loop, int round, float bound, hipStream_t s);
// composite + compaction + head of the next round
int mf_nerf_loop_composite(const NerfLoop& loop, int round, const NerfFieldOut& field, const NerfRaySums& sums, hipStream_t s);
// the same launches with a frame index in blockIdx.y (and the finish of every frame whose bg_per_ray >= 0)
int mf_nerf_batch_init(const NerfBatchLoop& b, const float* aabb, float min_near, hipStream_t s);
int mf_nerf_batch_march(const NerfBatchLoop& b, int round, float bound, hipStream_t s);
int mf_nerf_batch_composite(const NerfBatchLoop& b, int round, hipStream_t s);
int mf_nerf_batch_finish(const NerfBatchLoop& b, hipStream_t s);

// ---- mf_nerf_occupancy.hip: the occupancy-grid rebuild over the fused field's weight fragments (sweep, dilate + EMA, reduce + pack) -----------------
int mf_nerf_occupancy_shape(const char* what, int cascades, int grid_size, size_t* n_partials);      // the one place the served sizes are checked
// in.sigma_scale: density_scale; f.has_eye: whether this rebuild feeds the eye feature
int mf_nerf_occupancy_launch(const NerfFieldConsts& f, const NerfFrameInputs& in, const NerfGridBufs& g, int cascades, int grid_size, float bound, float decay,
                             float density_thresh, const float* noise, hipStream_t s);

// ---- mf_nerf_torso.hip: the whole torso branch as one fp32 kernel, and the torso grid's rebuild through the same per-point code ------------------------
int mf_nerf_torso_fused_weight_count();
// bias: host, [64] = the per-frame first-layer biases of the deform net | the torso net
int mf_nerf_torso_fused_launch(const NerfTorsoConsts& t, const float* bias, const float* density, const float* bg_coords, float thresh, const float* bg,
                               int bg_per_ray, float bg_const, int N, float* out, float* alpha_out, float* deform, hipStream_t s);
// sweep, 5 x 5 dilate + EMA, mean; partials: G^2 / 256 doubles
int mf_nerf_torso_grid_launch(const NerfTorsoConsts& t, const float* bias, const float* noise, float decay, float* density_grid, float* raw_grid, float* xys_out,
                              float* mean, double* partials, hipStream_t s);

// ---- the handles' shared base and the field handle (defined in mf_nerf_net.hip; mf_nerf_head.hip renders through a field) ---------------------------
constexpr int TW = 1024;                 // tokens per "image" of the token buffers

// shared by the field and the torso net: token buffers of 1 x TW "images", bias-free Linears as bound 1x1-conv plans
struct TokenNet : NetStore {
    int precision = MF_PREC_BF16X3;
    int cap_batches = 0;

    ActBuf* seq(int C) { return buf(C, 1, TW, 0); }
    int alloc() { return NetStore::alloc(cap_batches, precision); }
    // Linear(cin -> cout, bias=False) (network.py:79) as a 1x1 convolution; `w` is [cout][cin_buf] with the input-channel order of
    // the buffer view it reads
    int linear(ConvPlan** out, const std::vector<float>& w, int cin, int cout, int act, ActBuf* in) {
        ConvPlan* p = new_plan();
        int rc = mf_seq_conv_plan(p, w.data(), nullptr, cin, cout, TW, act, 0, precision);
        if (rc) return rc;
        if ((rc = mf_conv_bind(p, *in))) return rc;
        *out = p;
        return MF_OK;
    }
};

struct mf_nerf_field : TokenNet {
    mf_nerf_field_config cfg{};
    ActBuf *SI = nullptr, *CI = nullptr, *T1 = nullptr, *AU = nullptr, *T2 = nullptr, *EY = nullptr, *S1 = nullptr, *S2 = nullptr, *C1 = nullptr, *RGB = nullptr;
    ConvPlan *a1, *a2, *e1, *e2, *s1, *s2, *s3, *c1, *c2;
    float* emb[3] = {nullptr, nullptr, nullptr};
    float *coords = nullptr, *enc = nullptr, *d_enc_a = nullptr, *d_ind = nullptr;
    bf16_t* fused_w = nullptr;      // weight fragments of k_nerf_field_fused, or null (MF_NERF_FIELD=gemm)
    double* occ_partials = nullptr; // per-workgroup sums of mf_nerf_density_grid_update, allocated at its first call
    size_t occ_cap = 0;
    NerfFieldConsts consts() const {
        return {fused_w, precision == MF_PREC_BF16X3, {emb[0], emb[1], emb[2]}, cfg.offsets, cfg.log2_per_level_scale, cfg.base_resolution, cfg.bound,
                cfg.individual_dim, cfg.exp_eye};
    }
};
