// The three stages around the batched ER-NeRF head render for every frame of a step in ONE launch each: the torso image over the background
// (mf_nerf_frame_batch_background), the torso branch (mf_nerf_torso_forward_batch, in mf_nerf_net.hip beside the torso handle) and the finished uint8 frame
// (mf_nerf_frame_batch_out).  Host code only: each frame-indexed kernel stands beside the single-frame kernel whose per-pixel function it calls
// (mf_nerf_frame.hip, mf_nerf_torso.hip), so frame i of a call is the same bits as the single-frame entry point gives.
//
// The handle owns a TableRing of frame tables (mf_nerf_table_ring.h), the type mf_nerf_head_batch holds for its own.  A serving step makes up to three calls per
// group of frames, so the ring is 16 deep: nothing waits for the host unless 16 calls are in flight.  The ring is allocated at the first accepted call, so creating a
// handle and every refusal touch no device.
#include "mf_nerf_frame_batch.h"

namespace {
constexpr int RING = 16;
constexpr int MAX_FRAMES = 64;           // as mf_nerf_head_batch: the frames of one head call are the frames of one call here
}  // namespace

struct mf_nerf_frame_batch {
    int max_frames = 0, max_pixels = 0;
    TableRing ring{RING};                // entries of max_frames x NERF_FRAME_BATCH_ENTRY bytes
};

extern "C" int mf_nerf_frame_batch_create(int max_frames, int max_pixels, mf_nerf_frame_batch** out) {
    MF_REQUIRE(out, "nerf_frame_batch_create: null argument");
    *out = nullptr;
    MF_REQUIRE(max_frames >= 1 && max_frames <= MAX_FRAMES, "nerf_frame_batch_create: max_frames %d (1..%d)", max_frames, MAX_FRAMES);
    MF_REQUIRE(max_pixels >= 1, "nerf_frame_batch_create: max_pixels %d", max_pixels);
    mf_nerf_frame_batch* h = new mf_nerf_frame_batch();
    h->max_frames = max_frames; h->max_pixels = max_pixels;
    h->ring.bytes = (size_t)max_frames * NERF_FRAME_BATCH_ENTRY;
    *out = h;
    return MF_OK;
}

extern "C" void mf_nerf_frame_batch_destroy(mf_nerf_frame_batch* h) { delete h; }

int mf_nerf_frame_batch_limits(const mf_nerf_frame_batch* h, int* max_frames, int* max_pixels) {
    MF_REQUIRE(h, "nerf_frame_batch: null handle");
    *max_frames = h->max_frames; *max_pixels = h->max_pixels;
    return MF_OK;
}

TableRing& mf_nerf_frame_batch_ring(mf_nerf_frame_batch* h) { return h->ring; }

// what every call checks first, before anything touches a device
static int check_call(const char* who, const mf_nerf_frame_batch* h, const void* descs, int n_frames) {
    MF_REQUIRE(h && descs, "%s: null handle or descriptor table", who);
    MF_REQUIRE(n_frames >= 1 && n_frames <= h->max_frames, "%s: n_frames=%d (the handle holds 1..%d)", who, n_frames, h->max_frames);
    return MF_OK;
}

extern "C" int mf_nerf_frame_batch_background(mf_nerf_frame_batch* h, const mf_nerf_bg_desc* descs, int n_frames, int H, int W, void* stream) {
    int rc;
    if ((rc = check_call("nerf_frame_batch_background", h, descs, n_frames))) return rc;
    MF_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "nerf_frame_batch_background: frame %d x %d", W, H);
    MF_REQUIRE((int64_t)H * W <= h->max_pixels, "nerf_frame_batch_background: n_pixels=%lld exceed the handle's max_pixels %d", (long long)H * W, h->max_pixels);
    for (int i = 0; i < n_frames; ++i) {
        MF_REQUIRE(descs[i].torso_rgba && descs[i].bg_color, "nerf_frame_batch_background: frame %d: null torso_rgba or bg_color", i);
        MF_REQUIRE(((uintptr_t)descs[i].torso_rgba & 3) == 0, "nerf_frame_batch_background: frame %d: the RGBA image must be 4-byte aligned", i);
    }
    hipStream_t s = (hipStream_t)stream;
    return h->ring.call<NerfBgFrame>(
        n_frames, s,
        [&](NerfBgFrame* tab) {
            for (int i = 0; i < n_frames; ++i) tab[i] = NerfBgFrame{descs[i].torso_rgba, descs[i].bg_image, descs[i].bg_color, descs[i].bg_const, descs[i].half_mode != 0};
        },
        [&](const NerfBgFrame* dev) { return mf_nerf_frame_background_batch_launch(dev, n_frames, H * W, s); });
}

extern "C" int mf_nerf_frame_batch_out(mf_nerf_frame_batch* h, const mf_nerf_out_desc* descs, int n_frames, int rh, int rw, int H, int W, int FH, int FW,
                                       int linear_to_srgb, uint8_t* frames_rgb, void* stream) {
    int rc;
    if ((rc = check_call("nerf_frame_batch_out", h, descs, n_frames))) return rc;
    MF_REQUIRE(frames_rgb, "nerf_frame_batch_out: null output");
    MF_REQUIRE(rh > 0 && rw > 0 && H > 0 && W > 0 && (int64_t)rh * rw < (1ll << 31), "nerf_frame_batch_out: render %d x %d to %d x %d", rw, rh, W, H);
    MF_REQUIRE(FH > 0 && FW > 0 && (int64_t)FH * FW < (1ll << 31), "nerf_frame_batch_out: body frame %d x %d", FW, FH);
    MF_REQUIRE((int64_t)rh * rw <= h->max_pixels, "nerf_frame_batch_out: n_pixels=%lld exceed the handle's max_pixels %d", (long long)rh * rw, h->max_pixels);
    for (int i = 0; i < n_frames; ++i) {
        const mf_nerf_out_desc& d = descs[i];
        MF_REQUIRE(d.render || d.body_bgr, "nerf_frame_batch_out: frame %d: neither a render nor a body frame", i);
        if (!d.body_bgr) {
            MF_REQUIRE(d.x0 == 0 && d.y0 == 0, "nerf_frame_batch_out: frame %d: an offset (%d, %d) without a body frame", i, d.x0, d.y0);
            MF_REQUIRE(FH == H && FW == W, "nerf_frame_batch_out: frame %d: no body frame, and the block's frames are %d x %d, not %d x %d", i, FW, FH, W, H);
        }
        // nerfreal.py:122: the slice assignment raises when the frame does not fit; nothing is clipped
        if (d.render)
            MF_REQUIRE(d.x0 >= 0 && d.y0 >= 0 && (int64_t)d.x0 + W <= FW && (int64_t)d.y0 + H <= FH,
                       "nerf_frame_batch_out: frame %d: a %d x %d frame at (%d, %d) leaves the %d x %d body frame", i, W, H, d.x0, d.y0, FW, FH);
    }
    hipStream_t s = (hipStream_t)stream;
    return h->ring.call<NerfOutFrame>(
        n_frames, s,
        [&](NerfOutFrame* tab) {
            for (int i = 0; i < n_frames; ++i)
                tab[i] = NerfOutFrame{descs[i].render, descs[i].body_bgr, descs[i].render ? descs[i].x0 : 0, descs[i].render ? descs[i].y0 : 0};
        },
        [&](const NerfOutFrame* dev) { return mf_nerf_frame_out_batch_launch(dev, n_frames, rh, rw, H, W, FH, FW, linear_to_srgb, frames_rgb, s); });
}
