// What the two ER-NeRF head handles are made of (mf_nerf_head: one frame per call, mf_nerf_head.hip; mf_nerf_head_batch: several, mf_nerf_head_batch.hip): a
// frame's working set (HeadSlot), the round planner (RoundPlan) and what a handle holds besides its slots (HeadCommon).  Host only: nothing here is passed to a
// kernel; a slot hands out the argument groups of mf_nerf_host.h and the table entry of mf_nerf_march.h.
#pragma once
#include "mf_nerf_host.h"
#include "mf_nerf_march.h"

// One frame's working set: the control block, the two alive lists and the per-ray and per-sample arrays, carved from one allocation.
struct HeadSlot {
    void* mem = nullptr;
    float *nears, *fars, *rays_t, *xyzs, *dirs, *deltas, *sig, *rgb, *aa, *ae, *un, *wsum, *aasum, *aesum, *unsum;
    int *alive[2], *ctl;
    HeadSlot() = default;
    HeadSlot(const HeadSlot&) = delete;
    ~HeadSlot() { if (mem) (void)hipFree(mem); }
    // fb_words: the slot's two mapped-pinned feedback words, which the device posts to through the pointer at ctl[LOOP_CTL_FB]
    int alloc(int max_rays, volatile int* fb_words) {
        const size_t N = ((size_t)max_rays + 63) & ~(size_t)63;          // every member starts on a 256-byte boundary (the composite's 64-bit atomic at ctl + 6 needs 8)
        const size_t ctl_ints = (loop_ctl_ints(HEAD_MAX_ROUNDS) + 63) & ~(size_t)63;
        const size_t words = 22 * N + 2 * N + ctl_ints;                  // 22 floats and 2 ints per ray: 96 bytes
        MF_HIP(hipMalloc(&mem, words * 4));
        float* p = (float*)mem;
        auto take = [&](size_t n) { float* q = p; p += n; return q; };
        nears = take(N); fars = take(N); rays_t = take(N); xyzs = take(3 * N); dirs = take(3 * N); deltas = take(2 * N); sig = take(N);
        rgb = take(3 * N); aa = take(N); ae = take(N); un = take(N); wsum = take(N); aasum = take(N); aesum = take(N); unsum = take(N);
        alive[0] = (int*)take(N); alive[1] = (int*)take(N); ctl = (int*)take(ctl_ints);
        MF_HIP(hipMemset(ctl, 0, ctl_ints * sizeof(int)));
        void* fb_dev = nullptr;
        MF_HIP(hipHostGetDevicePointer(&fb_dev, (void*)fb_words, 0));
        MF_HIP(hipMemcpy(ctl + LOOP_CTL_FB, &fb_dev, sizeof(fb_dev), hipMemcpyHostToDevice));
        return MF_OK;
    }
    NerfLoop loop(int n_rays, int max_steps, const float* rays_o, const float* rays_d, const uint8_t* bitfield, int cascades, int grid_size, float dt_gamma,
                  float T_thresh, bool skip_empty) const {
        return {ctl, n_rays, max_steps, {alive[0], alive[1]}, rays_t, fars, rays_o, rays_d, bitfield, (uint32_t)cascades, (uint32_t)grid_size, dt_gamma, T_thresh,
                xyzs, dirs, deltas, skip_empty};
    }
    NerfFieldOut out() const { return {sig, rgb, aa, ae, un}; }
    // weights_sum: the caller's, or null for the slot's own
    NerfRaySums sums(float* weights_sum, float* depth, float* image) const { return {weights_sum ? weights_sum : wsum, depth, image, aasum, aesum, unsum}; }
    LoopFrame frame(const mf_nerf_frame_desc& d) const {
        return {ctl, alive[0], alive[1], rays_t, nears, fars, xyzs, dirs, deltas, sig, rgb, aa, ae, un, d.weights_sum ? d.weights_sum : wsum, d.depth, d.image, aasum,
                aesum, unsum, d.rays_o, d.rays_d, d.enc_a, d.ind_code, d.eye_dev, d.bg_color, d.frame_u8, d.eye, d.bg_const, d.bg_per_ray};
    }
    // background mix, depth normalisation and uint8 frame of a frame whose loop ran in this slot
    int finish(int n_rays, const float* bg_color, int bg_per_ray, float bg_const, float* image, float* depth, const float* weights_sum, uint8_t* frame_u8,
               void* stream) const {
        return mf_nerf_finish(image, depth, weights_sum ? weights_sum : wsum, nears, fars, bg_color, bg_per_ray, bg_const, n_rays, frame_u8, stream);
    }
    int copy_sums(int n_rays, float* ambient_aud, float* ambient_eye, float* uncertainty, hipStream_t s) const {
        const size_t bytes = (size_t)n_rays * sizeof(float);
        if (ambient_aud) MF_HIP(hipMemcpyAsync(ambient_aud, aasum, bytes, hipMemcpyDeviceToDevice, s));
        if (ambient_eye) MF_HIP(hipMemcpyAsync(ambient_eye, aesum, bytes, hipMemcpyDeviceToDevice, s));
        if (uncertainty) MF_HIP(hipMemcpyAsync(uncertainty, unsum, bytes, hipMemcpyDeviceToDevice, s));
        return MF_OK;
    }
};

// How many rounds of the next call are enqueued as (march, field, composite) launches; the tail launch covers the rest.  The most rounds any of the last four
// observed calls ran; every round (no tail) until a first one has reported.  MF_NERF_TAIL_AFTER=<k> fixes it (nerf_tail_after_env, mf_nerf_host.h).
struct RoundPlan {
    int hist[4] = {0, 0, 0, 0}, hist_n = 0;
    // seen: the rounds the feedback words show, of a call that finished some calls ago (0: none has reported)
    int next(int seen, int max_steps) {
        const int fixed = nerf_tail_after_env(max_steps);
        if (fixed >= 0) return fixed;
        if (seen > 0) { hist[hist_n & 3] = seen; hist_n++; }
        if (hist_n == 0) return max_steps;
        int m = 0;
        for (int i = 0; i < 4; ++i) m = hist[i] > m ? hist[i] : m;
        // no margin: a frame that needs more rounds than its predecessors runs them in the tail launch (and the next frames follow); a margin of one round was three
        // launches per frame that found nothing to do (2 043 -> 2 068 frames/s)
        return m < max_steps ? m : max_steps;
    }
};

// What a head handle holds besides its slots.  The handles differ in their slots and in how they read "rounds seen" from the feedback block.
struct HeadCommon {
    mf_nerf_field* field = nullptr;
    int cap = 0;                         // rays per slot
    float* aabb = nullptr;               // the box from the field's bound (device), read unless the caller brings its own aabb_infer
    // round-count feedback: per slot two words of mapped pinned host memory the device posts to when the slot's frame ends its loop ([0] rounds the frame ran, [1] the
    // tail's error flag); read without a sync, so they tell about a frame that finished some calls ago
    volatile int* fb = nullptr;
    RoundPlan plan;
    ~HeadCommon() {
        if (aabb) (void)hipFree(aabb);
        if (fb) (void)hipHostFree((void*)fb);
    }
    int init(mf_nerf_field* f, int max_rays, int n_slots) {
        field = f; cap = max_rays;
        MF_HIP(hipHostMalloc((void**)&fb, (size_t)n_slots * 2 * sizeof(int), hipHostMallocMapped));
        for (int i = 0; i < 2 * n_slots; ++i) fb[i] = 0;
        const float b = f->cfg.bound;
        const float box[6] = {-b, -b / 2, -b, b, b / 2, b};                                     // aabb_infer, renderer.py:86-89
        MF_HIP(hipMalloc((void**)&aabb, sizeof(box)));
        MF_HIP(hipMemcpy(aabb, box, sizeof(box), hipMemcpyHostToDevice));
        return MF_OK;
    }
};
