// ER-NeRF head render loop without host round trips: `run_cuda`'s inference branch (reference: ernerf/nerf_triplane/renderer.py:231-291) with the round
// control (n_alive, n_step, step) kept in HBM.  Host code only: this file launches the kernels of mf_nerf.hip and mf_nerf_fused.hip through mf_nerf_host.h.
//
// The reference compacts `rays_alive` with a boolean mask and reads its length back on the host every round; here k_loop_init / k_loop_composite (mf_nerf.hip)
// do both on the device, every launch has a fixed grid and exits when its round has nothing to do.  A frame needs ~5 of the max_steps = 16 rounds the
// reference allows, so only as many rounds as the frames before needed are enqueued as launches and ONE tail launch (k_loop_tail, mf_nerf_fused.hip) stands for
// the rest: it finds the loop ended, or runs the remaining rounds itself -- no round is ever dropped, and nothing waits for the host.  The whole frame is
// capturable as one hipGraph.
#include "mf_nerf_head_slot.h"

struct mf_nerf_head : HeadCommon {
    HeadSlot slot;
    const float* eye_dev = nullptr;      // mf_nerf_head_set_eye: the eye feature stays on the device
    const float* aabb_user = nullptr;    // mf_nerf_head_set_aabb: the caller's aabb_infer (device), read instead of `aabb`
    int fixed_rounds = -1;               // mf_nerf_head_set_rounds: >= 0 pins the launched-round count (a captured graph is keyed on it), -1 = follow the feedback
    int plan_rounds(int max_steps) { return plan.next(fb[0], max_steps); }
};

extern "C" int mf_nerf_head_create(mf_nerf_field* field, int max_rays, mf_nerf_head** out) {
    MF_REQUIRE(field && out && max_rays > 0, "nerf_head_create: bad argument");
    MF_REQUIRE(field->fused_w, "nerf_head_create: needs the fused field kernel (unset MF_NERF_FIELD=gemm)");
    MF_REQUIRE(max_rays <= field->cap_batches * TW, "nerf_head_create: %d rays exceed the field's sample capacity %d", max_rays, field->cap_batches * TW);
    *out = nullptr;
    std::unique_ptr<mf_nerf_head> h(new mf_nerf_head());
    int rc;
    if ((rc = h->init(field, max_rays, 1)) || (rc = h->slot.alloc(max_rays, h->fb))) return rc;
    *out = h.release();
    return MF_OK;
}

extern "C" int mf_nerf_head_render(mf_nerf_head* h, const float* rays_o, const float* rays_d, int n_rays, const uint8_t* density_bitfield, int cascades,
                                   int grid_size, float min_near, float dt_gamma, int max_steps, float T_thresh, float density_scale, const float* enc_a,
                                   const float* ind_code, float eye, const float* bg_color, int bg_per_ray, float bg_const, float* image, float* depth,
                                   float* weights_sum, uint8_t* frame_u8, void* stream) {
    MF_REQUIRE(h && rays_o && rays_d && density_bitfield && enc_a && image && depth, "nerf_head_render: null argument");
    MF_REQUIRE(n_rays > 0 && n_rays <= h->cap && max_steps > 0 && max_steps <= HEAD_MAX_ROUNDS, "nerf_head_render: n_rays=%d (capacity %d) max_steps=%d", n_rays, h->cap, max_steps);
    hipStream_t s = (hipStream_t)stream;
    const NerfFieldConsts f = h->field->consts();
    MF_REQUIRE(f.n_ind == 0 || ind_code, "nerf_head_render: the field was built with an individual code");
    const HeadSlot& k = h->slot;
    const NerfLoop loop = k.loop(n_rays, max_steps, rays_o, rays_d, density_bitfield, cascades, grid_size, dt_gamma, T_thresh, nerf_skip_empty_env());
    const NerfFrameInputs in{enc_a, ind_code, eye, h->eye_dev, density_scale};
    const NerfFieldOut out = k.out();
    const NerfRaySums sums = k.sums(weights_sum, depth, image);
    int rc;
    if ((rc = mf_nerf_loop_init(loop, sums, k.nears, h->aabb_user ? h->aabb_user : h->aabb, min_near, s))) return rc;
    MF_REQUIRE(h->fb[1] == 0, "nerf_head_render: the tail kernel of an earlier frame gave up waiting for a round (control block error flag)");
    const int rounds = h->fixed_rounds >= 0 ? (h->fixed_rounds < max_steps ? h->fixed_rounds : max_steps) : h->plan_rounds(max_steps);
    for (int it = 0; it < rounds; ++it)
        if ((rc = mf_nerf_loop_march(loop, it, f.bound, s)) || (rc = mf_nerf_fused_launch(f, in, loop.xyzs, loop.dirs, loop.N, out, s, &loop)) ||
            (rc = mf_nerf_loop_composite(loop, it, out, sums, s)))
            return rc;
    // at least one sample per alive ray and round, so max_steps rounds always suffice (step += n_step >= 1, renderer.py:270): with every round enqueued there is no tail
    if (rounds < max_steps && (rc = mf_nerf_tail_launch(f, in, out, loop, sums, rounds, s))) return rc;
    if (bg_per_ray < 0) return MF_OK;                                                       // finished later by mf_nerf_head_finish
    return k.finish(n_rays, bg_color, bg_per_ray, bg_const, image, depth, weights_sum, frame_u8, stream);
}

extern "C" int mf_nerf_head_finish(mf_nerf_head* h, int n_rays, const float* bg_color, int bg_per_ray, float bg_const, float* image, float* depth,
                                   const float* weights_sum, uint8_t* frame_u8, void* stream) {
    MF_REQUIRE(h && image && depth && n_rays > 0 && n_rays <= h->cap && bg_per_ray >= 0, "nerf_head_finish: bad argument");
    return h->slot.finish(n_rays, bg_color, bg_per_ray, bg_const, image, depth, weights_sum, frame_u8, stream);
}

extern "C" int mf_nerf_head_set_eye(mf_nerf_head* h, const float* eye_dev) {
    MF_REQUIRE(h, "nerf_head_set_eye: null handle");
    h->eye_dev = eye_dev;
    return MF_OK;
}

extern "C" int mf_nerf_head_set_aabb(mf_nerf_head* h, const float* aabb_dev) {
    MF_REQUIRE(h, "nerf_head_set_aabb: null handle");
    h->aabb_user = aabb_dev;
    return MF_OK;
}

extern "C" int mf_nerf_head_plan_rounds(mf_nerf_head* h, int max_steps, int* rounds) {
    MF_REQUIRE(h && rounds && max_steps > 0 && max_steps <= HEAD_MAX_ROUNDS, "nerf_head_plan_rounds: bad argument");
    *rounds = h->plan_rounds(max_steps);
    return MF_OK;
}

extern "C" int mf_nerf_head_set_rounds(mf_nerf_head* h, int rounds) {
    MF_REQUIRE(h && rounds >= -1 && rounds <= HEAD_MAX_ROUNDS, "nerf_head_set_rounds: bad argument");
    h->fixed_rounds = rounds;
    return MF_OK;
}

extern "C" int mf_nerf_head_last_rounds(mf_nerf_head* h, int* rounds, int* error_flag) {
    MF_REQUIRE(h && h->fb, "nerf_head_last_rounds: null handle");
    if (rounds) *rounds = h->fb[0];
    if (error_flag) *error_flag = h->fb[1];
    return MF_OK;
}

extern "C" int mf_nerf_head_ctl_snapshot(mf_nerf_head* h, int* out, int n_ints) {
    MF_REQUIRE(h && out && n_ints > 0 && (size_t)n_ints <= loop_ctl_ints(HEAD_MAX_ROUNDS), "nerf_head_ctl_snapshot: bad argument");
    MF_HIP(hipMemcpy(out, h->slot.ctl, (size_t)n_ints * sizeof(int), hipMemcpyDeviceToHost));
    return MF_OK;
}

extern "C" int mf_nerf_head_sums(mf_nerf_head* h, int n_rays, float* ambient_aud, float* ambient_eye, float* uncertainty, void* stream) {
    MF_REQUIRE(h && n_rays > 0 && n_rays <= h->cap, "nerf_head_sums: bad argument");
    return h->slot.copy_sums(n_rays, ambient_aud, ambient_eye, uncertainty, (hipStream_t)stream);
}

extern "C" void mf_nerf_head_destroy(mf_nerf_head* h) { delete h; }
