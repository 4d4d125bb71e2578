// Several ER-NeRF head frames in one device loop: mf_nerf_head_render's chain of launches (mf_nerf_head.hip) with a frame index in the grid.  Host code only: the
// frame-indexed kernels are in mf_nerf.hip (init, march, composite, finish) and mf_nerf_fused.hip (the field over every frame's samples), launched through
// mf_nerf_host.h; the tail is the single-frame k_loop_tail, enqueued once per frame.
//
// The handle owns one HeadSlot per frame -- the type a mf_nerf_head owns one of (mf_nerf_head_slot.h) -- and a TableRing of frame tables four deep
// (mf_nerf_table_ring.h), allocated with the handle: a call never overwrites the table of an earlier call that may still be in flight, and nothing waits for the
// host unless four calls are.
#include "mf_nerf_head_slot.h"
#include "mf_nerf_table_ring.h"

namespace {
constexpr int RING = 4;
constexpr int MAX_FRAMES = 64;           // = BATCH_MAX_FRAMES of k_nerf_field_batch (the launcher refuses more)
}  // namespace

struct mf_nerf_head_batch : HeadCommon {
    int max_frames = 0;
    std::vector<HeadSlot> slots;
    TableRing ring{RING};
    // the most rounds any of the call's frame slots reported
    int plan_rounds(int n_frames, int max_steps) {
        int seen = 0;
        for (int i = 0; i < n_frames; ++i) seen = fb[2 * i] > seen ? fb[2 * i] : seen;
        return plan.next(seen, max_steps);
    }
};

extern "C" int mf_nerf_head_batch_create(mf_nerf_field* field, int max_rays, int max_frames, mf_nerf_head_batch** out) {
    MF_REQUIRE(field && out && max_rays > 0, "nerf_head_batch_create: bad argument");
    MF_REQUIRE(max_frames >= 1 && max_frames <= MAX_FRAMES, "nerf_head_batch_create: max_frames %d (1..%d)", max_frames, MAX_FRAMES);
    MF_REQUIRE(field->fused_w, "nerf_head_batch_create: needs the fused field kernel (unset MF_NERF_FIELD=gemm)");
    MF_REQUIRE(max_rays <= field->cap_batches * TW, "nerf_head_batch_create: %d rays exceed the field's sample capacity %d", max_rays, field->cap_batches * TW);
    *out = nullptr;
    std::unique_ptr<mf_nerf_head_batch> h(new mf_nerf_head_batch());
    h->max_frames = max_frames;
    h->slots = std::vector<HeadSlot>((size_t)max_frames);
    h->ring.bytes = (size_t)max_frames * sizeof(LoopFrame);
    int rc;
    if ((rc = h->init(field, max_rays, max_frames))) return rc;
    for (int i = 0; i < max_frames; ++i)
        if ((rc = h->slots[(size_t)i].alloc(max_rays, h->fb + 2 * i))) return rc;
    if ((rc = h->ring.ensure())) return rc;
    *out = h.release();
    return MF_OK;
}

extern "C" int mf_nerf_head_batch_render(mf_nerf_head_batch* h, const mf_nerf_frame_desc* frames, int n_frames, int n_rays, const uint8_t* density_bitfield,
                                         int cascades, int grid_size, float min_near, float dt_gamma, int max_steps, float T_thresh, float density_scale,
                                         const float* aabb_dev, void* stream) {
    MF_REQUIRE(h && frames && density_bitfield, "nerf_head_batch_render: null argument");
    MF_REQUIRE(n_frames >= 1 && n_frames <= h->max_frames, "nerf_head_batch_render: n_frames=%d (the handle holds 1..%d)", n_frames, h->max_frames);
    MF_REQUIRE(n_rays > 0 && n_rays <= h->cap && max_steps > 0 && max_steps <= HEAD_MAX_ROUNDS, "nerf_head_batch_render: n_rays=%d (capacity %d) max_steps=%d", n_rays,
               h->cap, max_steps);
    const NerfFieldConsts f = h->field->consts();
    bool finish = false;
    for (int i = 0; i < n_frames; ++i) {
        const mf_nerf_frame_desc& d = frames[i];
        MF_REQUIRE(d.rays_o && d.rays_d && d.enc_a && d.image && d.depth, "nerf_head_batch_render: frame %d: null rays_o, rays_d, enc_a, image or depth", i);
        MF_REQUIRE(f.n_ind == 0 || d.ind_code, "nerf_head_batch_render: frame %d: the field was built with an individual code (null ind_code)", i);
        MF_REQUIRE(h->fb[2 * i + 1] == 0, "nerf_head_batch_render: the tail kernel of an earlier frame in slot %d gave up waiting for a round (control block error flag)", i);
        finish |= d.bg_per_ray >= 0;
    }
    hipStream_t s = (hipStream_t)stream;
    const bool skip_empty = nerf_skip_empty_env();
    auto fill = [&](LoopFrame* tab) {
        for (int i = 0; i < n_frames; ++i) tab[i] = h->slots[(size_t)i].frame(frames[i]);
    };
    auto enqueue = [&](const LoopFrame* tab_dev) -> int {
        const NerfBatchLoop b{tab_dev, n_frames, n_rays, max_steps, density_bitfield, (uint32_t)cascades, (uint32_t)grid_size, dt_gamma, T_thresh, skip_empty};
        int rc;
        if ((rc = mf_nerf_batch_init(b, aabb_dev ? aabb_dev : h->aabb, min_near, s))) return rc;
        const int rounds = h->plan_rounds(n_frames, max_steps);
        for (int it = 0; it < rounds; ++it)
            if ((rc = mf_nerf_batch_march(b, it, f.bound, s)) || (rc = mf_nerf_fused_batch_launch(f, density_scale, b, s)) || (rc = mf_nerf_batch_composite(b, it, s)))
                return rc;
        // the rounds not enqueued: the single-frame tail on every frame's own control block and slot (a frame-indexed tail is not built)
        for (int i = 0; rounds < max_steps && i < n_frames; ++i) {
            const mf_nerf_frame_desc& d = frames[i];
            const HeadSlot& k = h->slots[(size_t)i];
            if ((rc = mf_nerf_tail_launch(f, NerfFrameInputs{d.enc_a, d.ind_code, d.eye, d.eye_dev, density_scale}, k.out(),
                                          k.loop(n_rays, max_steps, d.rays_o, d.rays_d, density_bitfield, cascades, grid_size, dt_gamma, T_thresh, skip_empty),
                                          k.sums(d.weights_sum, d.depth, d.image), rounds, s)))
                return rc;
        }
        return finish ? mf_nerf_batch_finish(b, s) : MF_OK;
    };
    return h->ring.call<LoopFrame>(n_frames, s, fill, enqueue);
}

extern "C" int mf_nerf_head_batch_finish(mf_nerf_head_batch* h, int frame, int n_rays, const float* bg_color, int bg_per_ray, float bg_const, float* image,
                                         float* depth, const float* weights_sum, uint8_t* frame_u8, void* stream) {
    MF_REQUIRE(h && image && depth && frame >= 0 && frame < h->max_frames && n_rays > 0 && n_rays <= h->cap && bg_per_ray >= 0, "nerf_head_batch_finish: bad argument");
    return h->slots[(size_t)frame].finish(n_rays, bg_color, bg_per_ray, bg_const, image, depth, weights_sum, frame_u8, stream);
}

extern "C" int mf_nerf_head_batch_sums(mf_nerf_head_batch* h, int frame, int n_rays, float* ambient_aud, float* ambient_eye, float* uncertainty, void* stream) {
    MF_REQUIRE(h && frame >= 0 && frame < h->max_frames && n_rays > 0 && n_rays <= h->cap, "nerf_head_batch_sums: bad argument");
    return h->slots[(size_t)frame].copy_sums(n_rays, ambient_aud, ambient_eye, uncertainty, (hipStream_t)stream);
}

extern "C" int mf_nerf_head_batch_last_rounds(mf_nerf_head_batch* h, int* rounds, int* error_flags) {
    MF_REQUIRE(h && h->fb, "nerf_head_batch_last_rounds: null handle");
    for (int i = 0; i < h->max_frames; ++i) {
        if (rounds) rounds[i] = h->fb[2 * i];
        if (error_flags) error_flags[i] = h->fb[2 * i + 1];
    }
    return MF_OK;
}

extern "C" void mf_nerf_head_batch_destroy(mf_nerf_head_batch* h) { delete h; }
