// The frame-indexed launches around the batched ER-NeRF head render (mf_nerf_frame_batch.hip): one table entry per frame as the kernels read it, the launchers
// of the three kernels (each stands beside its single-frame kernel, whose per-pixel code it shares) and what mf_nerf_torso_forward_batch (mf_nerf_net.hip, where
// the torso handle is defined) needs of the batch handle.
#pragma once
#include "mf_nerf_host.h"
#include "mf_nerf_table_ring.h"

struct NerfBgFrame {                     // k_nerf_frame_background_batch (mf_nerf_frame.hip)
    const uint8_t* torso;
    const float* bg;
    float* out;
    float bg_const;
    int half;
};
struct NerfOutFrame {                    // k_nerf_frame_out_batch (mf_nerf_frame.hip)
    const float* render;
    const uint8_t* body;
    int x0, y0;
};
struct NerfTorsoFrame {                  // k_torso_fused<T_BATCH> (mf_nerf_torso.hip)
    float bias_d[32], bias_t[32];        // mf_nerf_torso::frame_bias of the frame's constants
    const float *bg_coords, *bg;
    float *out, *alpha_out, *deform;
    float thresh, bg_const;
    int bg_per_ray, pad;
};
constexpr size_t NERF_FRAME_BATCH_ENTRY = sizeof(NerfTorsoFrame);       // the largest of the three: a ring entry holds max_frames of them
static_assert(sizeof(NerfBgFrame) <= NERF_FRAME_BATCH_ENTRY && sizeof(NerfOutFrame) <= NERF_FRAME_BATCH_ENTRY, "ring entries are sized by the torso table");

// n: pixels per frame
int mf_nerf_frame_background_batch_launch(const NerfBgFrame* tab_dev, int n_frames, int n, hipStream_t s);
int mf_nerf_frame_out_batch_launch(const NerfOutFrame* tab_dev, int n_frames, int h, int w, int H, int W, int FH, int FW, int srgb, uint8_t* out, hipStream_t s);
int mf_nerf_torso_batch_launch(const NerfTorsoConsts& t, const NerfTorsoFrame* tab_dev, int n_frames, const float* density, int N, hipStream_t s);

// ---- the handle's limits and ring, for the entry points that fill a table ---------------------------------------------------------------------------
int mf_nerf_frame_batch_limits(const mf_nerf_frame_batch* h, int* max_frames, int* max_pixels);
TableRing& mf_nerf_frame_batch_ring(mf_nerf_frame_batch* h);           // 16 entries of max_frames x NERF_FRAME_BATCH_ENTRY bytes, allocated at the first call
