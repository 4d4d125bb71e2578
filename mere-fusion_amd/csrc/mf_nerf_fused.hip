// ER-NeRF radiance field as ONE kernel on gfx950: tri-plane hash-grid gathers, SH, and the nine Linear layers of
// `NeRFNetwork.forward` / `density` (reference: ernerf/nerf_triplane/network.py:249-308, 23 184 MACs per sample) without a
// single intermediate in HBM.
//
// Why: as separate launches (mf_nerf_net.hip) each Linear moves a [M, 64] (hi, lo) tensor out and back -- at M = 262 144 that
// is ~70 MB per layer and the nine GEMMs are memory-bound at ~45 us each.  Fused, a sample costs 12 B in and 28 B out.
//
// How (wave64, MFMA 16x16x32 bf16, fp32 accumulate, bf16x3 = (hi, lo) operands and 3 MFMAs per product):
//   * one wave owns 16 samples (one MFMA fragment column block); D[out channel][sample] = W * X^T, so the weights are the MFMA A
//     operand and a lane of the accumulator tile holds 4 consecutive OUT channels of ONE sample (lane % 16).
//   * a layer's accumulators ARE the next layer's B operand: the contraction index of a 32-deep step is defined as
//     (8g + j) <-> channel 16*(2s + j/4) + 4g + j%4, i.e. exactly what lane (sample, g) already holds from blocks 2s and 2s+1
//     of the previous layer.  Activations never move between lanes or through LDS; the weights are packed on the host in that
//     K order (mf_nerf_fused_pack).
//   * torch.cat is an ordering of K blocks: sigma_net reads [enc_x | enc_a * aud_ch_att | e * eye_att], colour_net reads
//     [geo_feat (sigma_net blocks 0..4, its row 0 = log sigma has zero weights) | SH | individual code].
//   * every weight fragment (63 x 1 KB x planes) sits in LDS, lane-linear, loaded once per workgroup; workgroups are persistent
//     over 256-sample tiles (16 waves x 16 samples).
//   * each lane gathers only the grid features its own B fragments need (channels 4g..4g+3 of each 16-block): 36 bilinear
//     lookups per sample spread over its 4 lanes, straight from the L2-resident tables.
#include "mf_nerf_field_tile.h"

namespace {

template <bool X3>
__global__ __launch_bounds__(NWAVE * 64) void k_nerf_field_fused(const FusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];     // NFRAG * NP KiB of weight fragments
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    __shared__ LevelTab lt;
    const int M = a.M_dev ? *a.M_dev : a.M;
    const int ntiles = (M + TILE - 1) / TILE;
    if ((int)blockIdx.x >= ntiles) return;          // also the "round already finished" case of the device-controlled loop (M == 0)
    field_stage_weights<X3>(a, smem, lt, NWAVE * 64);
    const float eye_v = a.eye_dev ? *a.eye_dev : a.eye;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
        field_tile<X3>(a, smem, lt, eye_v, tile * TILE + wave * 16 * NSF, M);
}

// ---- the field over the round's samples of EVERY frame of a batch (mf_nerf_head_batch_render), one launch ----------------------------------------------
// A (tiles, n_frames) grid would stage the 63 - 126 KB of weight fragments once per frame and workgroup.  Here a workgroup reads every frame's sample count
// (ctl[3]; 0 for a frame whose loop has ended), forms the prefix of the per-frame tile counts in LDS (n_frames <= 64: one wave), stages the weights ONCE and walks
// the flattened (frame, tile) pairs with stride gridDim.x, calling the unchanged field_tile with that frame's pointers -- a sample's result depends on nothing but
// the sample, so a frame is the same bits as through k_nerf_field_fused.  Frame index, counts and pointers are wave-uniform scalars.
constexpr int BATCH_MAX_FRAMES = 64;
template <bool X3>
__global__ __launch_bounds__(NWAVE * 64) void k_nerf_field_batch(const FusedArgs a, const LoopFrame* __restrict__ frames, const int n_frames, const int skip_empty) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ LevelTab lt;
    __shared__ int s_first[BATCH_MAX_FRAMES + 16], s_M[BATCH_MAX_FRAMES];     // s_first[f]: tiles of the frames before f, s_first[n_frames ...]: all tiles
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    auto uni = [](int x) __attribute__((always_inline)) { return __builtin_amdgcn_readfirstlane(x); };
    if (wave == 0) {
        const int lane = threadIdx.x;
        const int M = lane < n_frames ? frames[lane].ctl[3] : 0;
        int upto = (M + TILE - 1) / TILE;                                     // inclusive prefix over the 64 lanes
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(upto, d);
            if (lane >= d) upto += o;
        }
        s_M[lane] = M;
        s_first[lane + 1] = upto;
        if (lane == 0) s_first[0] = 0;
    }
    __syncthreads();
    const int total = uni(s_first[n_frames]);
    if ((int)blockIdx.x >= total) return;           // (every frame's round already finished: total == 0)
    field_stage_weights<X3>(a, smem, lt, NWAVE * 64);
    int f = 0;
    for (int p = blockIdx.x; p < total; p += gridDim.x) {
        while (uni(s_first[f + 1]) <= p) ++f;       // p only grows, so does its frame
        const int tile = p - uni(s_first[f]), M = uni(s_M[f]);
        const LoopFrame& fr = frames[f];
        FusedArgs af = a;
        af.xyzs = fr.xyzs; af.dirs = fr.dirs; af.deltas = skip_empty ? fr.deltas : nullptr; af.enc_a = fr.enc_a; af.ind = fr.ind;
        af.sigmas = fr.sigmas; af.rgbs = fr.rgbs; af.amb_aud = fr.amb_aud; af.amb_eye = fr.amb_eye; af.unc = fr.unc;
        const float eye_v = fr.eye_dev ? *fr.eye_dev : fr.eye;
        field_tile<X3>(af, smem, lt, eye_v, tile * TILE + wave * 16 * NSF, M);
    }
}

// ---- the render loop's TAIL: every round the launch chain did not enqueue, in one launch ------------------------------------------------------
// mf_nerf_head_render enqueues R rounds as (march, field, composite) launches -- R follows the round counts of the frames before (a frame needs ~5 of the
// max_steps = 16 the reference allows: renderer.py:246-270) -- and then this kernel ONCE.  It finds the loop ended (ctl[1] == 0: the usual case, one empty launch
// instead of 3 x (16 - R)) or runs the remaining rounds itself:
//   * a round is cut into chunks of 512 alive rays; a workgroup takes a chunk by ticket and carries it through the WHOLE round -- march (one ray per lane, the
//     reference's loop: march_ray_ref), field (field_tile over the chunk's own samples), composite (composite_ray) and the append of its survivors.  Rays do not
//     interact inside a round, so the only grid-wide step is the head of the next round (survivor count -> n_step): the workgroup that finishes the round's last
//     chunk computes it and publishes `ready[j + 1]`; the others wait for that flag -- and only for that flag, which a RUNNING workgroup will set.  No workgroup
//     ever waits for one that has not started, so the kernel needs no co-residency (two sessions' tails on one GPU cannot block each other).
//   * same per-ray and per-sample arithmetic as the launches (the survivors' order differs; results do not depend on it), so a frame is the same bits wherever the
//     chain hands over (tests/test_ernerf.py: hand-over after 0, 1, 2, 3 rounds against the launch-only loop).
// Visibility between workgroups (other XCDs have their own L2): agent-scope release (fence + atomic) by the writer, acquire (atomic + fence) by the readers.
struct TailArgs {
    int* ctl;
    int N, max_steps, first_parity;      // first_parity: which of alive[0 / 1] the first tail round reads
    float T_thresh, dt_gamma;
    uint32_t C, H;
    int *alive0, *alive1;                // (two fields, selected -- a dynamically indexed array in the kernel arguments goes through scratch, and a kernel with scratch
                                         // costs more to dispatch: the EMPTY tail launch is what every frame pays)
    float* rays_t;
    const float *rays_o, *rays_d, *fars;
    const uint8_t* grid;
    float *xyzs, *dirs, *deltas;
    float *wsum, *depth, *image, *aasum, *aesum, *unsum;
};
constexpr int TAIL_NW = 8;               // waves per tail workgroup: two per SIMD, so the compiler has 256 registers per lane -- with the field's 16 waves (128) the loop
                                         // state around field_tile spilled, and a kernel with SCRATCH costs more to dispatch: 4.8 us for the empty tail launch every frame pays
constexpr int TAIL_RC = TAIL_NW * 64;    // rays per chunk: one per lane
constexpr int TAIL_TILE = TAIL_NW * 16 * NSF;
#ifndef MF_TAIL_SPINS
#define MF_TAIL_SPINS (1 << 20)
#endif
constexpr int TAIL_SPINS = MF_TAIL_SPINS;   // polls of ~2 us before a waiting workgroup gives up (seconds)

template <bool X3>
__global__ __launch_bounds__(TAIL_NW * 64) void k_loop_tail(const FusedArgs a, const TailArgs t) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ LevelTab lt;
    __shared__ int s_i[4], s_wave[TAIL_NW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the round about to run, as the last composite launch (or k_loop_init) left it; nothing writes ctl[0..2] while this kernel runs
    int n_alive = t.ctl[0], n_step = t.ctl[1], step_after = t.ctl[2];
    if (n_step <= 0) return;                                                       // the loop has ended: the usual case
    field_stage_weights<X3>(a, smem, lt, TAIL_NW * 64);
    const float eye_v = a.eye_dev ? *a.eye_dev : a.eye;
    const int TS = t.max_steps + 1;
    int* const take = t.ctl + LOOP_CTL_TAIL;
    int* const fin = take + TS;
    int* const surv = fin + TS;
    int* const ready = surv + TS;
    int* const p_alive = ready + TS;
    int* const p_step = p_alive + TS;
    int* const p_after = p_step + TS;
    // every loop condition below is a wave-uniform SCALAR (readfirstlane of a value all lanes read from LDS): the workgroup's 16 waves take every branch together
    // and meet at every barrier.  (Written with plain ints the compiler cannot prove the ticket loop's exit uniform, builds per-lane exit masks around the
    // barriers, and the waves of a workgroup left the loop at different times -- a hang, found with the stage markers of profiles/r06_tail_trace.patch.)
    auto uni = [](int x) __attribute__((always_inline)) { return __builtin_amdgcn_readfirstlane(x); };
    auto next_ticket = [&](int j) __attribute__((always_inline)) {
        if (tid == 0) s_i[0] = atomicAdd(&take[j], 1);
        __syncthreads();
        const int c = uni(s_i[0]);
        __syncthreads();
        return c;
    };
    n_alive = uni(n_alive); n_step = uni(n_step); step_after = uni(step_after);
    for (int j = 0; j < t.max_steps; ++j) {
        const bool odd = ((t.first_parity + j) & 1) != 0;
        const int* a_in = odd ? t.alive1 : t.alive0;
        int* a_out = odd ? t.alive0 : t.alive1;
        const int nchunks = (n_alive + TAIL_RC - 1) / TAIL_RC;
        for (int c = next_ticket(j); c < nchunks; c = next_ticket(j)) {
            const int base = c * TAIL_RC;
            const int rays_here = min(TAIL_RC, n_alive - base);
            const uint32_t n = (uint32_t)(base + tid);
            int v = -1;
            if (tid < rays_here) {
                v = a_in[n];
                march_ray_ref(n, (uint32_t)n_step, v, 0.f, t.rays_t, t.rays_o, t.rays_d, a.bound, t.dt_gamma, (uint32_t)t.max_steps, t.C, t.H, t.grid, t.fars,
                              t.xyzs, t.dirs, t.deltas, true);
            }
            __threadfence();
            __syncthreads();
            const int m0 = base * n_step, mend = m0 + rays_here * n_step;
            for (int s0 = m0; s0 < mend; s0 += TAIL_TILE) field_tile<X3>(a, smem, lt, eye_v, s0 + wave * 16 * NSF, mend);
            __threadfence();
            __syncthreads();
            bool keep = false;
            if (tid < rays_here)
                keep = !composite_ray(n, (uint32_t)n_step, t.T_thresh, v, t.rays_t, a.sigmas, a.rgbs, t.deltas, a.amb_aud, a.amb_eye, a.unc, t.wsum, t.depth, t.image,
                                      t.aasum, t.aesum, t.unsum);
            // `rays_alive = rays_alive[rays_alive >= 0]` (renderer.py:266): wave-aggregated append, one atomic per chunk
            const unsigned long long m = __ballot(keep);
            if (lane == 0) s_wave[wave] = __popcll(m);
            __syncthreads();
            int before = 0, mine = 0;
#pragma unroll
            for (int w = 0; w < TAIL_NW; ++w) { before += w < wave ? s_wave[w] : 0; mine += s_wave[w]; }
            if (tid == 0) s_i[1] = atomicAdd(&surv[j], mine);
            __syncthreads();
            if (keep) a_out[s_i[1] + before + __popcll(m & ((1ull << lane) - 1))] = v;
            __threadfence();
            __syncthreads();
            if (tid == 0) {
                const int done = atomicAdd(&fin[j], 1);
                if (done == nchunks - 1) {                                          // the round's last chunk: head of the next round
                    const int na = __hip_atomic_load(&surv[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const int ns = j + 1 < t.max_steps ? loop_n_step(na, step_after, t.N, t.max_steps) : 0;
                    p_alive[j + 1] = ns ? na : 0; p_step[j + 1] = ns; p_after[j + 1] = step_after + ns;
                    if (ns) t.ctl[LOOP_CTL_ROUNDS] += 1;
                    else loop_post_feedback(t.ctl);
                    __hip_atomic_store(&ready[j + 1], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        if (tid == 0) {
            // every chunk of round j is taken, each by a workgroup that is running it: the flag WILL be set.  The bound only turns a protocol bug into an error the
            // host sees (ctl[9] -> the feedback word) instead of a hung GPU.
            int spins = 0;
            while (__hip_atomic_load(&ready[j + 1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == 0 && spins < TAIL_SPINS) { __builtin_amdgcn_s_sleep(32); ++spins; }
            if (spins >= TAIL_SPINS) {
                __hip_atomic_store(&t.ctl[LOOP_CTL_ERR], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                loop_post_feedback(t.ctl);
                s_i[1] = 0; s_i[2] = 0; s_i[3] = 0;
            } else {
                s_i[1] = p_alive[j + 1]; s_i[2] = p_step[j + 1]; s_i[3] = p_after[j + 1];
            }
        }
        __syncthreads();
        n_alive = uni(s_i[1]); n_step = uni(s_i[2]); step_after = uni(s_i[3]);
        __syncthreads();
        if (n_step <= 0) return;
        __threadfence();                                                            // every lane sees what the other workgroups wrote in round j
    }
}
}  // namespace

// ---- host: weight fragments in the kernel's K order ----------------------------------------------------------------------
// `blocks`: the 16-channel K blocks of a layer in k-step order (pairs), each entry a source column of `w` ([cout][cin]) or -1.
static void pack_layer(const float* w, int cout, int cin, const std::vector<std::vector<int>>& blocks, int nblk, int nks, bool x3,
                       std::vector<bf16_t>& dst, int frag0) {
    const int np = x3 ? 2 : 1;
    for (int blk = 0; blk < nblk; ++blk)
        for (int ks = 0; ks < nks; ++ks) {
            const int f = frag0 + blk * nks + ks;
            for (int lane = 0; lane < 64; ++lane) {
                const int m = lane & 15, g = lane >> 4;
                for (int j = 0; j < 8; ++j) {
                    const std::vector<int>& kb = blocks[2 * ks + (j >> 2)];
                    const int src = kb[4 * g + (j & 3)];
                    const int row = blk * 16 + m;
                    const float v = (src >= 0 && row < cout) ? w[(size_t)row * cin + src] : 0.f;
                    const bf16_t hi = mf_f2bf(v);
                    dst[((size_t)(f * np + 0) * 64 + lane) * 8 + j] = hi;
                    if (x3) dst[((size_t)(f * np + 1) * 64 + lane) * 8 + j] = mf_f2bf(v - mf_bf2f(hi));
                }
            }
        }
}

static std::vector<int> kblock(int first, int n = 16) {   // n real channels first..first+n-1, padded with -1
    std::vector<int> b(16, -1);
    for (int i = 0; i < n; ++i) b[i] = first + i;
    return b;
}

// weights: the nine [cout][cin] matrices in reference order (aud0, aud1, eye0, eye1, sig0, sig1, sig2, col0, col1; eye* may be null)
int mf_nerf_fused_pack(const float* const w[9], int n_ind, bool has_eye, bool x3, bf16_t** dev_out) {
    const int np = x3 ? 2 : 1;
    std::vector<bf16_t> buf((size_t)NFRAG * np * 64 * 8, 0);
    const std::vector<int> Z(16, -1);
    const int sig_in = 36 + 32 + (has_eye ? 1 : 0), col_in = 16 + 64 + n_ind;
    // enc_x blocks in the kernel's gather order: lane group g holds levels g, g + 4, g + 8; slot i of block b is (level t, plane p) of that lane, channel p * 12 + level
    auto xblock = [](int which) {
        static const int tp[3][4][2] = {{{0, 0}, {0, 1}, {0, 2}, {1, 0}}, {{1, 1}, {1, 2}, {2, 0}, {2, 1}}, {{2, 2}, {-1, -1}, {-1, -1}, {-1, -1}}};
        std::vector<int> b(16, -1);
        for (int g = 0; g < 4; ++g)
            for (int i = 0; i < 4; ++i)
                if (tp[which][i][0] >= 0) b[4 * g + i] = tp[which][i][1] * 12 + g + 4 * tp[which][i][0];
        return b;
    };
    const std::vector<std::vector<int>> X = {xblock(0), xblock(1), xblock(2), Z};
    const std::vector<std::vector<int>> H64 = {kblock(0), kblock(16), kblock(32), kblock(48)};
    pack_layer(w[0], 64, 36, X, 4, 2, x3, buf, frag_base(L_AUD0));
    pack_layer(w[1], 32, 64, H64, 2, 2, x3, buf, frag_base(L_AUD1));
    if (has_eye) {
        pack_layer(w[2], 16, 36, X, 1, 2, x3, buf, frag_base(L_EYE0));
        pack_layer(w[3], 1, 16, {kblock(0), Z}, 1, 1, x3, buf, frag_base(L_EYE1));
    }
    // sigma_net.0: reference columns [enc_x 0..35 | enc_w 36..67 | e 68]; K blocks (X0, X1), (X2, W0), (W1, eye)
    pack_layer(w[4], 64, sig_in, {xblock(0), xblock(1), xblock(2), kblock(36), kblock(52), has_eye ? kblock(68, 1) : Z}, 4, 3, x3, buf, frag_base(L_SIG0));
    pack_layer(w[5], 64, 64, H64, 4, 2, x3, buf, frag_base(L_SIG1));
    pack_layer(w[6], 65, 64, H64, 5, 2, x3, buf, frag_base(L_SIG2));
    {
        // colour_net.0: reference columns [SH 0..15 | geo 16..79 | ind 80..]; K blocks = sigma_net rows (row 0 = log sigma -> no column,
        // row r -> geo r-1 -> column 16 + r - 1), then SH, then the individual code
        std::vector<std::vector<int>> kb;
        for (int blk = 0; blk < 5; ++blk) {
            std::vector<int> b(16, -1);
            for (int i = 0; i < 16; ++i) {
                const int r = blk * 16 + i;
                if (r >= 1 && r <= 64) b[i] = 16 + r - 1;
            }
            kb.push_back(b);
        }
        kb.push_back(kblock(0));
        kb.push_back(kblock(80, n_ind));
        kb.push_back(Z);
        pack_layer(w[7], 64, col_in, kb, 4, 4, x3, buf, frag_base(L_COL0));
    }
    pack_layer(w[8], 3, 64, H64, 1, 2, x3, buf, frag_base(L_COL1));
    bf16_t* d = nullptr;
    MF_HIP(hipMalloc(&d, buf.size() * sizeof(bf16_t)));
    MF_HIP(hipMemcpy(d, buf.data(), buf.size() * sizeof(bf16_t), hipMemcpyHostToDevice));
    *dev_out = d;
    return MF_OK;
}

int mf_nerf_fused_launch(const NerfFieldConsts& f, const NerfFrameInputs& in, const float* xyzs, const float* dirs, int M, const NerfFieldOut& out, hipStream_t s,
                         const NerfLoop* round) {
    FusedArgs a{};
    int rc;
    if ((rc = fused_args(a, f, in, xyzs, dirs, M, out, round ? round->ctl + 3 : nullptr, round ? round->skip_deltas() : nullptr))) return rc;
    const size_t lds = (size_t)NFRAG * (f.x3 ? 2 : 1) * 1024;
    static bool attr_done[2] = {false, false};
    if ((rc = f.x3 ? fused_lds_attr(k_nerf_field_fused<true>, attr_done[1], lds) : fused_lds_attr(k_nerf_field_fused<false>, attr_done[0], lds))) return rc;
    const int grid = std::min(a.ntiles, 256);
    if (f.x3) hipLaunchKernelGGL(k_nerf_field_fused<true>, dim3(grid), dim3(NWAVE * 64), lds, s, a);
    else hipLaunchKernelGGL(k_nerf_field_fused<false>, dim3(grid), dim3(NWAVE * 64), lds, s, a);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

int mf_nerf_fused_batch_launch(const NerfFieldConsts& f, float sigma_scale, const NerfBatchLoop& b, hipStream_t s) {
    MF_REQUIRE(b.n_frames >= 1 && b.n_frames <= BATCH_MAX_FRAMES, "nerf_fused_batch_launch: %d frames (1..%d)", b.n_frames, BATCH_MAX_FRAMES);
    FusedArgs a{};
    int rc;
    // (the per-frame members -- samples, outputs, enc_a, ind, eye -- are filled in by the kernel from the frame table; a.ntiles: one frame's upper bound)
    if ((rc = fused_args(a, f, NerfFrameInputs{nullptr, nullptr, 0.f, nullptr, sigma_scale}, nullptr, nullptr, b.N, NerfFieldOut{nullptr, nullptr, nullptr, nullptr, nullptr}))) return rc;
    const size_t lds = (size_t)NFRAG * (f.x3 ? 2 : 1) * 1024;
    static bool attr_done[2] = {false, false};
    if ((rc = f.x3 ? fused_lds_attr(k_nerf_field_batch<true>, attr_done[1], lds) : fused_lds_attr(k_nerf_field_batch<false>, attr_done[0], lds))) return rc;
    const int grid = (int)std::min<int64_t>((int64_t)a.ntiles * b.n_frames, 256);
    if (f.x3) hipLaunchKernelGGL(k_nerf_field_batch<true>, dim3(grid), dim3(NWAVE * 64), lds, s, a, b.frames, b.n_frames, (int)b.skip_empty);
    else hipLaunchKernelGGL(k_nerf_field_batch<false>, dim3(grid), dim3(NWAVE * 64), lds, s, a, b.frames, b.n_frames, (int)b.skip_empty);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

int mf_nerf_tail_launch(const NerfFieldConsts& f, const NerfFrameInputs& in, const NerfFieldOut& out, const NerfLoop& l, const NerfRaySums& r, int rounds_launched,
                        hipStream_t s) {
    FusedArgs a{};
    int rc;
    if ((rc = fused_args(a, f, in, l.xyzs, l.dirs, l.N, out, nullptr, l.skip_deltas()))) return rc;
    TailArgs t{};
    t.ctl = l.ctl; t.N = l.N; t.max_steps = l.max_steps; t.first_parity = rounds_launched & 1; t.T_thresh = l.T_thresh; t.dt_gamma = l.dt_gamma; t.C = l.cascades;
    t.H = l.grid_size; t.alive0 = l.alive[0]; t.alive1 = l.alive[1]; t.rays_t = l.rays_t; t.rays_o = l.rays_o; t.rays_d = l.rays_d; t.fars = l.fars; t.grid = l.bitfield;
    t.xyzs = l.xyzs; t.dirs = l.dirs; t.deltas = l.deltas; t.wsum = r.wsum; t.depth = r.depth; t.image = r.image; t.aasum = r.aasum; t.aesum = r.aesum; t.unsum = r.unsum;
    const size_t lds = (size_t)NFRAG * (f.x3 ? 2 : 1) * 1024;
    static bool attr_done[2] = {false, false};
    if ((rc = f.x3 ? fused_lds_attr(k_loop_tail<true>, attr_done[1], lds) : fused_lds_attr(k_loop_tail<false>, attr_done[0], lds))) return rc;
    // workgroups: 64 (one per 512 rays if the frame has fewer).  When the loop has ended -- the usual case -- each of them reads three words and leaves, and the
    // launch costs what its waves cost to start: 4.9 us with 256 workgroups of 16 waves, a quarter of that with 64; when it has not, the late rounds the tail is
    // there for have a few ten thousand rays at most (a 512 x 512 frame's fifth round: 30 k)
    const char* e = getenv("MF_NERF_TAIL_WGS");                                  // read per call (A/B)
    const int grid = std::min(std::max(1, (l.N + TAIL_RC - 1) / TAIL_RC), e && atoi(e) > 0 ? std::min(atoi(e), 256) : 64);
    if (f.x3) hipLaunchKernelGGL(k_loop_tail<true>, dim3(grid), dim3(TAIL_NW * 64), lds, s, a, t);
    else hipLaunchKernelGGL(k_loop_tail<false>, dim3(grid), dim3(TAIL_NW * 64), lds, s, a, t);
    MF_HIP(hipGetLastError());
    return MF_OK;
}
