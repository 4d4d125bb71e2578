// The exact steps around the DWPose landmark network (musetalk/utils/preprocessing.py:96-131 over mmpose's inference_topdown), each restated as integer or
// one-rounding-per-operation arithmetic so that tests/dwpose_ref.py can be matched bit for bit:
//   mf_warp_affine_u8        cv2.warpAffine(INTER_LINEAR, constant 0 border) of TopdownAffine + the BGR -> RGB, (x - mean) / std of PoseDataPreprocessor, written into the
//                            net's input buffer, with the mirrored image of the flip test behind it
//   mf_simcc_decode          flip_vectors + average, get_simcc_maximum, / split ratio, the map back to frame pixels
//   mf_muse_landmark_boxes   preprocessing.py:100-101, 113-131: the landmark box, its fallbacks and the two sums of the printed adjustment range
// Floating-point contraction is OFF in this file, as in mf_crop_resize.hip: every product and sum below rounds on its own, as numpy's do.
#include "mf_nn.h"
#include "mf_aux.h"
#include "mf_net_planes.h"

#pragma clang fp contract(off)

namespace {

struct F3 { float v[3]; };
struct FlipTab { unsigned char pair[256]; };

// The integer warp model: X = (rint(m0 * x * 1024) + rint((m1 * y + m2) * 1024) + 16) >> 5 in 1/32 pixel, taps weighted (32 - fy)(32 - fx) * 32
// ... (sum 32768), a tap outside the frame reads 0, code = (sum + 16384) >> 15.  m: the input -> source map of job j, float64 [6].
__global__ __launch_bounds__(256) void k_warp_affine_u8(const uint8_t* __restrict__ frames, int H, int W, const double* __restrict__ minv, int n, Pl X, F3 mean, F3 stdv,
                                                        int reverse_channels, int flip, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int x = idx % X.W;
    int64_t t = idx / X.W;
    const int y = t % X.H;
    const int j = t / X.H;
    const double* m = minv + (int64_t)j * 6;
    const long long Xq = ((long long)rint(m[0] * (double)x * 1024.0) + (long long)rint((m[1] * (double)y + m[2]) * 1024.0) + 16) >> 5;
    const long long Yq = ((long long)rint(m[3] * (double)x * 1024.0) + (long long)rint((m[4] * (double)y + m[5]) * 1024.0) + 16) >> 5;
    const long long sx = Xq >> 5, sy = Yq >> 5;
    const int fx = (int)(Xq & 31), fy = (int)(Yq & 31);
    const int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32, w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
    const bool y0 = sy >= 0 && sy < H, y1 = sy + 1 >= 0 && sy + 1 < H, x0 = sx >= 0 && sx < W, x1 = sx + 1 >= 0 && sx + 1 < W;
    const uint8_t* f = frames + (int64_t)j * H * W * 3;
    const int64_t o = X.at(j, y, x), of = flip ? X.at(n + j, y, X.W - 1 - x) : 0;
    for (int c = 0; c < 3; ++c) {
        const int sc = reverse_channels ? 2 - c : c;
        int acc = 16384;
        if (y0 && x0) acc += w00 * f[(sy * W + sx) * 3 + sc];
        if (y0 && x1) acc += w01 * f[(sy * W + sx + 1) * 3 + sc];
        if (y1 && x0) acc += w10 * f[((sy + 1) * W + sx) * 3 + sc];
        if (y1 && x1) acc += w11 * f[((sy + 1) * W + sx + 1) * 3 + sc];
        const float v = ((float)(acc >> 15) - mean.v[c]) / stdv.v[c];
        X.st(o + c, v);
        if (flip) X.st(of + c, v);
    }
    for (int c = 3; c < X.C; ++c) {                                            // the padding channels the first conv reads
        X.st(o + c, 0.f);
        if (flip) X.st(of + c, 0.f);
    }
}

// one wave per (image, keypoint): each lane keeps the first maximum of its bins, the wave keeps the larger value and, among equal values, the lower bin
__device__ __forceinline__ void wave_argmax(float& best, int& at) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oa = __shfl_xor(at, o);
        if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
}

__global__ __launch_bounds__(256) void k_simcc_decode(const float* __restrict__ lx, const float* __restrict__ ly, const float* __restrict__ fx, const float* __restrict__ fy,
                                                      FlipTab tab, int B, int K, int BX, int BY, float in_w, float in_h, float cx, float cy, float sw, float sh,
                                                      float* __restrict__ kpts, float* __restrict__ scores) {
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (item >= B * K) return;
    const int b = item / K, k = item % K;
    const int64_t row = (int64_t)b * K + k, frow = (int64_t)b * K + tab.pair[k];
    float bx = -INFINITY, by = -INFINITY;
    int ax = 0x7fffffff, ay = 0x7fffffff;
    for (int i = lane; i < BX; i += 64) {
        float v = lx[row * BX + i];
        if (fx) v = (v + fx[frow * BX + (BX - 1 - i)]) * 0.5f;
        if (v > bx || ax == 0x7fffffff) { bx = v; ax = i; }
    }
    for (int i = lane; i < BY; i += 64) {
        float v = ly[row * BY + i];
        if (fy) v = (v + fy[frow * BY + i]) * 0.5f;
        if (v > by || ay == 0x7fffffff) { by = v; ay = i; }
    }
    wave_argmax(bx, ax);
    wave_argmax(by, ay);
    if (lane != 0) return;
    const float score = fminf(bx, by);
    float px = (float)ax, py = (float)ay;
    if (score <= 0.f) { px = -1.f; py = -1.f; }
    px = px / 2.f; py = py / 2.f;                                               // simcc_split_ratio
    kpts[row * 2 + 0] = ((px / in_w) * sw + cx) - sw * 0.5f;
    kpts[row * 2 + 1] = ((py / in_h) * sh + cy) - sh * 0.5f;
    scores[row] = score;
}

// One thread per frame.  flags: 0 placeholder (no face), 1 landmark box, 2 the detector's box.  sums: (sum range_minus, sum range_plus, frames counted), zeroed before.
__global__ __launch_bounds__(256) void k_muse_landmark_boxes(const float* __restrict__ kpts, int K, int face0, int n_face, const float* __restrict__ boxes, const int* __restrict__ counts,
                                                             int max_det, int n, int H, int W, int bbox_shift, int* __restrict__ coords, int* __restrict__ flags, int* __restrict__ sums) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int* c = coords + (int64_t)i * 4;
    if (counts[i] <= 0) {                                                       // :109-111 coord_placeholder
        c[0] = c[1] = c[2] = c[3] = 0;
        flags[i] = 0;
        return;
    }
    const float* lm = kpts + ((int64_t)i * K + face0) * 2;
    int minx = 0x7fffffff, maxx = -0x7fffffff - 1, maxy = -0x7fffffff - 1;
    for (int p = 0; p < n_face; ++p) {                                          // .astype(np.int32): toward zero
        const int x = (int)lm[2 * p], y = (int)lm[2 * p + 1] + (p == 29 ? bbox_shift : 0);   // :113, :119: half_face_coord is a VIEW of row 29, the shift lands in the array
        minx = min(minx, x); maxx = max(maxx, x); maxy = max(maxy, y);
    }
    const int y28 = (int)lm[2 * 28 + 1], y29 = (int)lm[2 * 29 + 1], y30 = (int)lm[2 * 30 + 1];
    atomicAdd(sums + 0, y30 - y29);
    atomicAdd(sums + 1, y29 - y28);
    atomicAdd(sums + 2, 1);
    const int half = y29 + bbox_shift;                                          // :118-119
    const int upper = half - (maxy - half);                                     // :120-121
    const int x1 = minx, y1 = upper, x2 = maxx, y2 = maxy;
    if (y2 - y1 <= 0 || x2 - x1 <= 0 || x1 < 0) {                               // :126-128: the detector's first box, clipped at 0, truncated, clipped to the frame
        const float* d = boxes + (int64_t)i * max_det * 5;
        c[0] = min((int)fmaxf(d[0], 0.f), W); c[1] = min((int)fmaxf(d[1], 0.f), H);
        c[2] = min((int)fmaxf(d[2], 0.f), W); c[3] = min((int)fmaxf(d[3], 0.f), H);
        flags[i] = 2;
    } else {
        c[0] = x1; c[1] = y1; c[2] = x2; c[3] = y2;
        flags[i] = 1;
    }
}

}  // namespace

extern "C" int mf_warp_affine_u8(mf_net* net, int buf, const uint8_t* frames, int n, int H, int W, const double* minv, const float* mean3, const float* std3,
                                 int reverse_channels, int flip, void* stream) {
    MF_REQUIRE(net && frames && minv && mean3 && std3, "warp_affine_u8: null argument");
    MF_REQUIRE(n >= 1 && H >= 1 && W >= 1 && H < 32768 && W < 32768, "warp_affine_u8: bad geometry (%d frames of %dx%d)", n, H, W);
    MF_REQUIRE(n * (flip ? 2 : 1) <= mf_net_max_batch(net), "warp_affine_u8: %d images exceed the net's capacity %d", n * (flip ? 2 : 1), mf_net_max_batch(net));
    MF_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "warp_affine_u8: zero std");
    const ActBuf* b = mf_net_actbuf(net, buf);
    MF_REQUIRE(b, "net: no buffer %d", buf);
    MF_REQUIRE(b->C == 8, "warp_affine_u8: buffer %d has %d channels, not the 8 of a 3-channel input", buf, b->C);
    const int64_t total = (int64_t)n * b->H * b->W;
    hipLaunchKernelGGL(k_warp_affine_u8, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, frames, H, W, minv, n, pl_of(*b), F3{{mean3[0], mean3[1], mean3[2]}},
                       F3{{std3[0], std3[1], std3[2]}}, reverse_channels ? 1 : 0, flip ? 1 : 0, total);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_simcc_decode(const float* logits_x, const float* logits_y, const float* flip_x, const float* flip_y, const int* flip_pairs, int batch, int keypoints, int bins_x,
                               int bins_y, int in_w, int in_h, const float* center, const float* scale, float* kpts, float* scores, void* stream) {
    MF_REQUIRE(logits_x && logits_y && center && scale && kpts && scores, "simcc_decode: null argument");
    MF_REQUIRE((flip_x == nullptr) == (flip_y == nullptr) && (!flip_x || flip_pairs), "simcc_decode: the flipped pass needs both logits and the pair table");
    MF_REQUIRE(batch >= 1 && keypoints >= 1 && keypoints <= 256 && bins_x >= 1 && bins_y >= 1 && in_w >= 1 && in_h >= 1, "simcc_decode: bad dimensions");
    FlipTab tab{};
    for (int k = 0; k < keypoints; ++k) {
        const int p = flip_x ? flip_pairs[k] : k;
        MF_REQUIRE(p >= 0 && p < keypoints, "simcc_decode: flip pair %d of keypoint %d is outside [0, %d)", p, k, keypoints);
        tab.pair[k] = (unsigned char)p;
    }
    const int64_t items = (int64_t)batch * keypoints;
    hipLaunchKernelGGL(k_simcc_decode, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits_x, logits_y, flip_x, flip_y, tab, batch, keypoints, bins_x, bins_y,
                       (float)in_w, (float)in_h, center[0], center[1], scale[0], scale[1], kpts, scores);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_muse_landmark_boxes(const float* kpts, int keypoints, const float* boxes, const int* counts, int n, int max_det, int H, int W, int bbox_shift, int* coords,
                                      int* flags, int* range_sums, void* stream) {
    MF_REQUIRE(kpts && boxes && counts && coords && flags && range_sums, "muse_landmark_boxes: null argument");
    MF_REQUIRE(n >= 1 && max_det >= 1 && H >= 1 && W >= 1, "muse_landmark_boxes: bad geometry");
    MF_REQUIRE(keypoints >= 91, "muse_landmark_boxes: the face landmarks are keypoints [23, 91) of COCO-WholeBody; got %d keypoints", keypoints);
    MF_HIP(hipMemsetAsync(range_sums, 0, 3 * sizeof(int), (hipStream_t)stream));
    hipLaunchKernelGGL(k_muse_landmark_boxes, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, kpts, keypoints, 23, 68, boxes, counts, max_det, n, H, W, bbox_shift, coords,
                       flags, range_sums);
    MF_HIP(hipGetLastError());
    return MF_OK;
}
