// Several ER-NeRF head frames in one device loop: mf_nerf_head_render's chain of launches (mf_nerf_head.hip) with a frame index in the grid.  Host code only: the
// frame-indexed kernels are in mf_nerf.hip (init, march, composite, finish) and mf_nerf_fused.hip (the field over every frame's samples), launched through
// mf_nerf_host.h; the tail is the single-frame k_loop_tail, enqueued once per frame.
//
// The handle owns one SLOT per frame -- what a mf_nerf_head owns for its one frame -- and a ring of frame tables.  A call fills the next table in pinned host
// memory, copies it to the ring entry's device table on the caller's stream and records an event behind its last launch; the entry is written again only after
// that event, so a call never overwrites the table of an earlier call that may still be in flight, and nothing waits for the host unless the whole ring is.
#include "mf_nerf_host.h"
#include "mf_nerf_march.h"

namespace {
struct BatchSlot {
    void* mem = nullptr;                 // one allocation, carved into the members below
    float *nears, *fars, *rays_t, *xyzs, *dirs, *deltas, *sig, *rgb, *aa, *ae, *un, *wsum, *aasum, *aesum, *unsum;
    int *alive[2], *ctl;
};
constexpr int RING = 4;
constexpr int MAX_FRAMES = 64;           // = BATCH_MAX_FRAMES of k_nerf_field_batch (the launcher refuses more)
}  // namespace

struct mf_nerf_head_batch {
    mf_nerf_field* field = nullptr;
    int cap = 0, max_frames = 0;
    std::vector<BatchSlot> slots;
    float* aabb = nullptr;               // the box from the field's bound (device)
    volatile int* fb = nullptr;          // pinned: per slot [0] rounds the slot's last finished frame ran, [1] its tail's error flag
    LoopFrame* tab_host[RING] = {};      // pinned staging
    LoopFrame* tab_dev[RING] = {};
    hipEvent_t done[RING] = {};          // behind the last launch of the call that used the entry
    bool used[RING] = {};
    int next = 0;
    int hist[4] = {0, 0, 0, 0}, hist_n = 0;
    ~mf_nerf_head_batch() {
        for (int r = 0; r < RING; ++r) {
            if (done[r]) { if (used[r]) (void)hipEventSynchronize(done[r]); (void)hipEventDestroy(done[r]); }
            if (tab_host[r]) (void)hipHostFree(tab_host[r]);
            if (tab_dev[r]) (void)hipFree(tab_dev[r]);
        }
        for (BatchSlot& s : slots) if (s.mem) (void)hipFree(s.mem);
        if (aabb) (void)hipFree(aabb);
        if (fb) (void)hipHostFree((void*)fb);
    }
};

// mf_nerf_head's head_plan over the slots' feedback words: the most rounds any frame of the last four observed batches ran
static int batch_plan(mf_nerf_head_batch* h, int n_frames, int max_steps) {
    const int fixed = nerf_tail_after_env(max_steps);
    if (fixed >= 0) return fixed;
    int seen = 0;
    for (int i = 0; i < n_frames; ++i) seen = h->fb[2 * i] > seen ? h->fb[2 * i] : seen;
    if (seen > 0) { h->hist[h->hist_n & 3] = seen; h->hist_n++; }
    if (h->hist_n == 0) return max_steps;
    int m = 0;
    for (int i = 0; i < 4; ++i) m = h->hist[i] > m ? h->hist[i] : m;
    return m < max_steps ? m : max_steps;
}

extern "C" int mf_nerf_head_batch_create(mf_nerf_field* field, int max_rays, int max_frames, mf_nerf_head_batch** out) {
    MF_REQUIRE(field && out && max_rays > 0, "nerf_head_batch_create: bad argument");
    MF_REQUIRE(max_frames >= 1 && max_frames <= MAX_FRAMES, "nerf_head_batch_create: max_frames %d (1..%d)", max_frames, MAX_FRAMES);
    MF_REQUIRE(field->fused_w, "nerf_head_batch_create: needs the fused field kernel (unset MF_NERF_FIELD=gemm)");
    MF_REQUIRE(max_rays <= field->cap_batches * TW, "nerf_head_batch_create: %d rays exceed the field's sample capacity %d", max_rays, field->cap_batches * TW);
    *out = nullptr;
    std::unique_ptr<mf_nerf_head_batch> h(new mf_nerf_head_batch());
    h->field = field; h->cap = max_rays; h->max_frames = max_frames;
    h->slots.resize((size_t)max_frames);
    {
        int* fb = nullptr;
        MF_HIP(hipHostMalloc((void**)&fb, (size_t)max_frames * 2 * sizeof(int), hipHostMallocMapped));
        for (int i = 0; i < 2 * max_frames; ++i) fb[i] = 0;
        h->fb = fb;
    }
    const size_t N = ((size_t)max_rays + 63) & ~(size_t)63;          // every member starts on a 256-byte boundary
    const size_t ctl_ints = (loop_ctl_ints(HEAD_MAX_ROUNDS) + 63) & ~(size_t)63;
    const size_t words = 22 * N + 2 * N + ctl_ints;                  // 22 floats and 2 ints per ray: 96 bytes
    for (int i = 0; i < max_frames; ++i) {
        BatchSlot& s = h->slots[(size_t)i];
        MF_HIP(hipMalloc(&s.mem, words * 4));
        float* p = (float*)s.mem;
        auto take = [&](size_t n) { float* q = p; p += n; return q; };
        s.nears = take(N); s.fars = take(N); s.rays_t = take(N); s.xyzs = take(3 * N); s.dirs = take(3 * N); s.deltas = take(2 * N); s.sig = take(N);
        s.rgb = take(3 * N); s.aa = take(N); s.ae = take(N); s.un = take(N); s.wsum = take(N); s.aasum = take(N); s.aesum = take(N); s.unsum = take(N);
        s.alive[0] = (int*)take(N); s.alive[1] = (int*)take(N); s.ctl = (int*)take(ctl_ints);
        MF_HIP(hipMemset(s.ctl, 0, ctl_ints * sizeof(int)));
        void* fb_dev = nullptr;
        MF_HIP(hipHostGetDevicePointer(&fb_dev, (void*)(h->fb + 2 * i), 0));
        MF_HIP(hipMemcpy(s.ctl + LOOP_CTL_FB, &fb_dev, sizeof(fb_dev), hipMemcpyHostToDevice));
    }
    for (int r = 0; r < RING; ++r) {
        MF_HIP(hipHostMalloc((void**)&h->tab_host[r], (size_t)max_frames * sizeof(LoopFrame), hipHostMallocDefault));
        MF_HIP(hipMalloc((void**)&h->tab_dev[r], (size_t)max_frames * sizeof(LoopFrame)));
        MF_HIP(hipEventCreateWithFlags(&h->done[r], hipEventDisableTiming));
    }
    const float b = field->cfg.bound;
    const float aabb[6] = {-b, -b / 2, -b, b, b / 2, b};                                    // aabb_infer, renderer.py:86-89
    MF_HIP(hipMalloc((void**)&h->aabb, sizeof(aabb)));
    MF_HIP(hipMemcpy(h->aabb, aabb, sizeof(aabb), hipMemcpyHostToDevice));
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
    for (int i = 0; i < n_frames; ++i) {
        const mf_nerf_frame_desc& d = frames[i];
        MF_REQUIRE(d.rays_o && d.rays_d && d.enc_a && d.image && d.depth, "nerf_head_batch_render: frame %d: null rays_o, rays_d, enc_a, image or depth", i);
        MF_REQUIRE(f.n_ind == 0 || d.ind_code, "nerf_head_batch_render: frame %d: the field was built with an individual code (null ind_code)", i);
        MF_REQUIRE(h->fb[2 * i + 1] == 0, "nerf_head_batch_render: the tail kernel of an earlier frame in slot %d gave up waiting for a round (control block error flag)", i);
    }
    hipStream_t s = (hipStream_t)stream;
    const int r = h->next;
    if (h->used[r]) MF_HIP(hipEventSynchronize(h->done[r]));           // returns at once unless RING calls are in flight
    h->next = (r + 1) % RING;
    LoopFrame* tab = h->tab_host[r];
    bool finish = false;
    for (int i = 0; i < n_frames; ++i) {
        const mf_nerf_frame_desc& d = frames[i];
        const BatchSlot& k = h->slots[(size_t)i];
        tab[i] = LoopFrame{k.ctl, k.alive[0], k.alive[1], k.rays_t, k.nears, k.fars, k.xyzs, k.dirs, k.deltas, k.sig, k.rgb, k.aa, k.ae, k.un,
                           d.weights_sum ? d.weights_sum : k.wsum, d.depth, d.image, k.aasum, k.aesum, k.unsum, d.rays_o, d.rays_d, d.enc_a, d.ind_code, d.eye_dev,
                           d.bg_color, d.frame_u8, d.eye, d.bg_const, d.bg_per_ray};
        finish |= d.bg_per_ray >= 0;
    }
    MF_HIP(hipMemcpyAsync(h->tab_dev[r], tab, (size_t)n_frames * sizeof(LoopFrame), hipMemcpyHostToDevice, s));
    h->used[r] = true;
    const char* skip_env = getenv("MF_NERF_SKIP_EMPTY");                       // as mf_nerf_head_render
    const NerfBatchLoop b{h->tab_dev[r], n_frames, n_rays, max_steps, density_bitfield, (uint32_t)cascades, (uint32_t)grid_size, dt_gamma, T_thresh,
                          !(skip_env && skip_env[0] == '0')};
    auto enqueue = [&]() -> int {
        int rc;
        if ((rc = mf_nerf_batch_init(b, aabb_dev ? aabb_dev : h->aabb, min_near, s))) return rc;
        const int rounds = batch_plan(h, n_frames, max_steps);
        for (int it = 0; it < rounds; ++it)
            if ((rc = mf_nerf_batch_march(b, it, f.bound, s)) || (rc = mf_nerf_fused_batch_launch(f, density_scale, b, s)) || (rc = mf_nerf_batch_composite(b, it, s)))
                return rc;
        // the rounds not enqueued: the single-frame tail on every frame's own control block and slot (a frame-indexed tail is not built)
        for (int i = 0; rounds < max_steps && i < n_frames; ++i) {
            const LoopFrame& t = tab[i];
            const NerfLoop loop{t.ctl, n_rays, max_steps, {t.alive0, t.alive1}, t.rays_t, t.fars, t.rays_o, t.rays_d, density_bitfield, b.cascades, b.grid_size,
                                dt_gamma, T_thresh, t.xyzs, t.dirs, t.deltas, b.skip_empty};
            if ((rc = mf_nerf_tail_launch(f, NerfFrameInputs{t.enc_a, t.ind, t.eye, t.eye_dev, density_scale}, NerfFieldOut{t.sigmas, t.rgbs, t.amb_aud, t.amb_eye, t.unc},
                                          loop, NerfRaySums{t.wsum, t.depth, t.image, t.aasum, t.aesum, t.unsum}, rounds, s)))
                return rc;
        }
        return finish ? mf_nerf_batch_finish(b, s) : MF_OK;
    };
    const int rc = enqueue();
    MF_HIP(hipEventRecord(h->done[r], s));                                  // also after a failed enqueue: the copy of the table is on the stream
    return rc;
}

extern "C" int mf_nerf_head_batch_finish(mf_nerf_head_batch* h, int frame, int n_rays, const float* bg_color, int bg_per_ray, float bg_const, float* image,
                                         float* depth, const float* weights_sum, uint8_t* frame_u8, void* stream) {
    MF_REQUIRE(h && image && depth && frame >= 0 && frame < h->max_frames && n_rays > 0 && n_rays <= h->cap && bg_per_ray >= 0, "nerf_head_batch_finish: bad argument");
    const BatchSlot& k = h->slots[(size_t)frame];
    return mf_nerf_finish(image, depth, weights_sum ? weights_sum : k.wsum, k.nears, k.fars, bg_color, bg_per_ray, bg_const, n_rays, frame_u8, stream);
}

extern "C" int mf_nerf_head_batch_sums(mf_nerf_head_batch* h, int frame, int n_rays, float* ambient_aud, float* ambient_eye, float* uncertainty, void* stream) {
    MF_REQUIRE(h && frame >= 0 && frame < h->max_frames && n_rays > 0 && n_rays <= h->cap, "nerf_head_batch_sums: bad argument");
    const BatchSlot& k = h->slots[(size_t)frame];
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = (size_t)n_rays * sizeof(float);
    if (ambient_aud) MF_HIP(hipMemcpyAsync(ambient_aud, k.aasum, bytes, hipMemcpyDeviceToDevice, s));
    if (ambient_eye) MF_HIP(hipMemcpyAsync(ambient_eye, k.aesum, bytes, hipMemcpyDeviceToDevice, s));
    if (uncertainty) MF_HIP(hipMemcpyAsync(uncertainty, k.unsum, bytes, hipMemcpyDeviceToDevice, s));
    return MF_OK;
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
