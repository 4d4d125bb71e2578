/*
 * merefusion.h -- C ABI of libmerefusion_hip.so, the MI355X (gfx950) frame generator that sits
 * underneath mere-fusion's lipreal.py / musereal.py render loops.
 *
 * The reference has no native FFI on this path (its hot loop is torch modules called from
 * Python); each entry point below names the Python interface it replaces (paths relative to the
 * reference checkout).  INTEGRATION.md shows the ctypes stub a maintainer adds on the reference
 * side.  All functions return 0 on success or a negative mf_status; they never throw across
 * the boundary.  mf_last_error() returns a thread-local message for the last failure.
 *
 * Pointers marked "device" are HIP device pointers borrowed for the duration of the call
 * (caller owns them, lipreal.py:121-126); "host" pointers are read during the call only.
 * A handle owns its packed weights, its activation workspace and its captured hipGraphs.
 * Handles are not thread-safe: one handle per (session, stream), as the reference runs one
 * single-threaded inference process per session (lipreal.py:85, app.py:549).
 */
#ifndef MEREFUSION_H
#define MEREFUSION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mf_status {
    MF_OK = 0,
    MF_ERR_INVALID = -1,   /* bad argument / shape / missing tensor */
    MF_ERR_HIP = -2,       /* a HIP runtime call failed */
    MF_ERR_NODEVICE = -3,  /* no gfx950 device visible */
    MF_ERR_NOMEM = -4
} mf_status;

/* Arithmetic mode of the MFMA convolution kernels.
 * MF_PREC_BF16   : bf16 activations/weights, fp32 accumulate (BASELINE config 2).
 * MF_PREC_BF16X3 : activations and weights carried as bf16 (hi, lo) pairs, three bf16 MFMAs per
 *                  product (hi*hi + lo*hi + hi*lo), fp32 accumulate: ~2^-17 relative operand
 *                  error; meets the north-star parity bound (L-inf <= 1e-3 vs the fp32 CPU
 *                  generator) that plain bf16 cannot. */
typedef enum mf_precision { MF_PREC_BF16 = 0, MF_PREC_BF16X3 = 1, MF_PREC_F16Q = 2 } mf_precision;
/* MF_PREC_F16Q (mf_conv2d_* test seam; inside the VAE decoder it is chosen by the schedule; wide 3x3 stride-1 layers, optionally behind a nearest 2x upsample): operands as f16 + FP6 (e2m3, OCP-MX block scales) residuals --
 * w.x = wh.xh (one f16 MFMA) + q6(wh).xl + wl.q6(xh) (one block-scaled 16x16x128 MFMA at 4x the rate); outputs stay bf16 (hi, lo).  DESIGN.md. */

/* One named fp32 host tensor of a checkpoint (a state_dict item). */
typedef struct mf_tensor {
    const char* name;   /* e.g. "face_encoder_blocks.0.0.conv_block.0.weight" */
    const float* data;  /* host, contiguous, fp32 */
    int ndim;
    int64_t shape[4];
} mf_tensor;

/* ---- library ---------------------------------------------------------------------------- */
/* Selects the HIP device (replaces `device = 'cuda'`, lipreal.py:29). */
int mf_init(int device);
const char* mf_last_error(void);
/* ABI version, bumped on any signature change. */
int mf_abi_version(void);

/* ---- Wav2Lip generator (H2) -------------------------------------------------------------- */
typedef struct mf_wav2lip mf_wav2lip;

/* Replaces `Wav2Lip()` + `load_state_dict` + `.to(device).eval()` (lipreal.py:43-53,
 * wav2lip/models/wav2lip.py:12-85).  `weights` are the state-dict tensors (101 weight, 101 bias,
 * 50 x running_mean / running_var; num_batches_tracked is ignored); a leading "module." in a name
 * is stripped as lipreal.py:48-49 does.  BatchNorm (eval, eps 1e-5, conv.py:10) is folded in. */
int mf_wav2lip_create(const mf_tensor* weights, int n_weights, int precision, mf_wav2lip** out);

/* Replaces `pred = model(mel_batch, img_batch)` (lipreal.py:124-125 -> wav2lip.py:87-125).
 * mel  : device fp32 [B,1,80,16]    face : device fp32 [B,6,96,96] (NCHW, values in [0,1])
 * out  : device fp32 [B,3,96,96] in [0,1], BGR.  Enqueued on `stream` (a hipStream_t; NULL =
 * default stream); returns without synchronising. */
int mf_wav2lip_forward(mf_wav2lip* h, const float* mel, const float* face, float* out, int batch,
                       void* stream);

/* Fuses the per-batch glue around the generator (lipreal.py:115-126): faces arrive as uint8
 * [B,96,96,3] BGR crops, are masked (rows >= 48 zeroed in the first 3 channels), concatenated
 * and scaled by 1/255 on the fly; frames leave as fp32 [B,96,96,3] = pred*255 (HWC, what
 * lipreal.py:126 hands to process_frames).  mel: device fp32 [B,1,80,16]. */
int mf_wav2lip_forward_u8(mf_wav2lip* h, const float* mel, const uint8_t* faces_u8,
                          float* frames_hwc, int batch, void* stream);

/* mf_wav2lip_forward_u8 with the faces picked from a pool (cross-session batching, lip_driver.LipBatcher): face_pool is device uint8
 * [n_pool_rows,96,96,3] -- every session's cached crops, concatenated -- and batch row b is generated from face rows[b] (lipreal.py:112-114: the
 * mirror-indexed crop).  rows: HOST array of `batch` pool rows, range-checked before anything is enqueued; it is read during the call only.  Bit-equal to
 * mf_wav2lip_forward_u8 on the gathered faces at the same batch, with or without the hipGraph (the rows never enter the captured part). */
int mf_wav2lip_forward_u8_rows(mf_wav2lip* h, const float* mel, const uint8_t* face_pool, int n_pool_rows,
                               const int* rows, float* frames_hwc, int batch, void* stream);

/* 1 when the handle holds an instantiated hipGraph for this batch size (the next forward at it is a replay), else 0 (first forward: eager; second: capture;
 * always 0 under MF_NO_GRAPH=1).  Growing the handle's workspace -- a forward at a batch larger than any before -- drops every captured graph, so a
 * warm-up sizes the handle with its LARGEST batch first (lip_driver.LipBatcher.prewarm). */
int mf_wav2lip_graph_captured(const mf_wav2lip* h, int batch);

/* Copies the NCHW fp32 activation named `tap` of the LAST forward into `dst` (device), for
 * parity tests.  tap: "audio_embedding", "face_encoder_blocks.N", "face_decoder_blocks.N". */
int mf_wav2lip_read_tap(mf_wav2lip* h, const char* tap, float* dst, int batch, void* stream);

/* Measurement seam for bench.py (roofline): the generator's KERNEL launches in execution order at a
 * batch size (a split-K layer is two launches: the MFMA kernel and its combine pass).
 * launch_info: name = the reference module path ("face_decoder_blocks.4.1"), kernel = the HIP kernel
 * name as rocprofv3 prints it (template arguments without spaces), flops = algorithmic FLOPs of that
 * launch (2 x conv MACs; 0 for layout / combine kernels).
 * profile: runs `iters` forwards WITHOUT the hipGraph on `stream`, a hipEvent before every launch,
 * and returns the mean milliseconds of each launch. */
int mf_wav2lip_num_launches(const mf_wav2lip* h, int batch);
int mf_wav2lip_launch_info(const mf_wav2lip* h, int index, int batch, char* name, int name_cap,
                           char* kernel, int kernel_cap, double* flops);
int mf_wav2lip_profile(mf_wav2lip* h, const float* mel, const float* face, float* out, int batch,
                       int iters, float* ms_per_launch, void* stream);

/* Launch configurations.  A forward never measures: at the first forward of a batch size every implicit-GEMM layer looks its signature up in the
 * tuning table -- the file MF_TUNE_CACHE names, else `tune/gfx950.txt` beside the library (measured on an MI355X for the BASELINE.json shapes) --
 * and a signature that is not there runs the cost model's pick.  mf_*_tune is the explicit warm-up a server calls at start-up for every batch size its
 * loop can emit: it times each layer's tile x split-K x operand-path candidates on the buffers the last forward at `batch` filled (one forward at
 * that batch must have run), records the winners in the table (appended to MF_TUNE_CACHE when set) and drops the hipGraph captured with the old
 * ones.  Seconds per full-size network; results differ from the un-tuned ones by fp32 summation order only.  (ABI version 4) */
int mf_wav2lip_tune(mf_wav2lip* h, int batch, void* stream);

void mf_wav2lip_destroy(mf_wav2lip* h);

/* ---- single fused convolution layer (building block, also the per-geometry test seam) ---- */
typedef struct mf_conv2d mf_conv2d;

typedef struct mf_conv2d_desc {
    int cin, cout;
    int kh, kw;
    int stride_h, stride_w;
    int pad_h, pad_w;
    int transposed;       /* 0 = Conv2d (conv.py:5), 1 = ConvTranspose2d (conv.py:33) */
    int output_padding;   /* transposed only */
    int residual;         /* 1: add the layer input before the activation (conv.py:17-18); 2: after it */
    int act;              /* 0 none, 1 ReLU, 2 sigmoid, 3 GELU (erf), 4 SiLU, 5 GEGLU: y = x[:, :cout/2] * gelu(x[:, cout/2:])
                           * (diffusers GEGLU of the UNet feed-forward), cout % 32 == 0, the output has cout/2 channels */
    int in_h, in_w;       /* spatial size of the input this layer is built for */
    int upsample;         /* 1: nearest-neighbour 2x upsampling in front of a 3x3 s1 p1 conv (diffusers Upsample2D) */
    int pad_hi;           /* extra zero rows / columns at the BOTTOM / RIGHT only (diffusers Downsample2D of the VAE encoder: F.pad(x, (0, 1, 0, 1)) +
                           * conv k3 s2 p0); 0 for every other layer.  (ABI version 2) */
} mf_conv2d_desc;

/* weight: host fp32, [cout,cin,kh,kw] (Conv2d) or [cin,cout,kh,kw] (ConvTranspose2d);
 * bias: host fp32 [cout] or NULL; bn_*: host fp32 [cout] or all NULL (no BatchNorm). */
int mf_conv2d_create(const mf_conv2d_desc* desc, const float* weight, const float* bias,
                     const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                     const float* bn_var, int precision, mf_conv2d** out);
/* x: device fp32 NCHW [B,cin,in_h,in_w]; y: device fp32 NCHW [B,cout,out_h,out_w]. */
int mf_conv2d_forward(mf_conv2d* h, const float* x, float* y, int batch, void* stream);
int mf_conv2d_out_shape(const mf_conv2d* h, int* out_h, int* out_w);
/* The same layer as the producer of a GroupNorm(groups) (diffusers ResnetBlock2D: conv -> norm): besides y, the launch leaves the (sum, sum of
 * squares) of the stored output per (sample, group) in stats -- device fp64 [B][groups][2] -- from the kernel's epilogue or split-K combine
 * where the chosen configuration can, else from a statistics pass behind it (test seam of what the UNet / VAE schedules do between layers). */
int mf_conv2d_forward_stats(mf_conv2d* h, const float* x, float* y, int groups, double* stats, int batch, void* stream);
/* Measurement seam: mean milliseconds of the convolution launch alone (layout passes excluded) over
 * `iters` repeats on the buffers of the last mf_conv2d_forward, bracketed by hipEvents on `stream`. */
int mf_conv2d_time(mf_conv2d* h, int batch, int iters, float* ms, void* stream);
void mf_conv2d_destroy(mf_conv2d* h);
/* Test seam of the launch selection.  mf_conv2d_launch_config: what mf_conv2d_forward (stats_groups == 0) or mf_conv2d_forward_stats(stats_groups) at
 * `batch` will launch -- resolved by the code the launch itself runs.  info[0 .. 11): family (MF_CONV_FAMILY_*), bm, bn, wgm, wgn (halo families: patch
 * rows, channels, waves), the split that launches (after every clamp; halo families: the channel split), the operand path ld that runs (-1 resolved;
 * -1 outside the implicit GEMM), K depth BK (halo families: the channel slice), phases, the GroupNorm statistics source (MF_CONV_STATS_*), and 1 when the
 * configuration is pinned (by mf_conv2d_pin_config or the tuning table).  n >= 11.
 * mf_conv2d_pin_config: the implicit-GEMM configuration (tile, split-K, ld) the layer launches at `batch`, in the slot the tuning table fills, with the
 * table's split clamp; refused for a configuration no compiled kernel of the layer's precision runs, and for layers the table does not serve.
 * bm == 0 unpins. */
#define MF_CONV_FAMILY_IGEMM 0        /* implicit GEMM (mf_conv.hip) */
#define MF_CONV_FAMILY_HALO 1         /* register-weights halo tile (mf_conv_halo.hip) */
#define MF_CONV_FAMILY_HALO_W 2       /* LDS-weights halo tile (mf_conv_halo2.hip) */
#define MF_CONV_FAMILY_HALO_W_SPLIT 3 /* ... its 256-channel tile with the channel slices split, combined by the split-K epilogue */
#define MF_CONV_FAMILY_TWIN 4         /* the implicit-GEMM twin of a wide halo plan */
#define MF_CONV_FAMILY_THIN 5         /* thin-input kernel (mf_conv_thin.hip) */
#define MF_CONV_FAMILY_F16Q 6         /* f16 + FP6 halo tile */
#define MF_CONV_STATS_NONE 0
#define MF_CONV_STATS_EPILOGUE 1      /* the conv's own epilogue */
#define MF_CONV_STATS_COMBINE 2       /* the split-K combine (k_splitk_epilogue_stats) */
#define MF_CONV_STATS_PASS 3          /* a k_gn_stats pass behind the conv */
int mf_conv2d_launch_config(const mf_conv2d* h, int batch, int stats_groups, int* info, int n);
int mf_conv2d_pin_config(mf_conv2d* h, int batch, int bm, int bn, int wgm, int wgn, int nsplit, int ld);

/* ---- Wav2Lip mel-spectrogram (H1) -------------------------------------------------------- */
/* Replaces `audio.melspectrogram(inputs)` (lipasr.py:23 -> wav2lip/audio.py:45-51 with the
 * constants of wav2lip/hparams.py:33-73): pre-emphasis 0.97, centred STFT n_fft=800 hop=200
 * periodic Hann, 80 Slaney mel bands 55-7600 Hz, 20*log10(max(1e-5,.)) - 20, clip-normalise
 * to [-4,4].  wav: device fp32 [n]; out: device fp32 [80, T], T = 1 + n/200.
 * pad_mode: 0 = zeros (librosa >= 0.10 default "constant"), 1 = reflect (librosa < 0.10). */
int mf_melspec(const float* wav, int n, float* out, int pad_mode, void* stream);
int mf_melspec_frames(int n);
/* The mel windows of MANY sessions' run_steps in one launch (lipasr.py:24-35): wav is device fp32 [n_windows][n], each row one session's whole
 * sliding window of (2B + l + r) x 320 samples; starts: HOST array of the n_starts start columns lip_driver.mel_chunk_starts returns (shared: every
 * row has the same n), each in [0, T - 16]; chunks: device fp32 [n_windows * n_starts][1][80][16], window-major -- per row exactly
 * mf_melspec(row)[:, s : s + 16] for every start s, bit for bit.  Padding happens at each row's own ends.  n_starts <= 256. */
int mf_melspec_windows(const float* wav, int n, int n_windows, const int* starts, int n_starts,
                       float* chunks, int pad_mode, void* stream);
/* The sliding windows of the sessions of one step, pushed by one launch (lipasr.py:17-21 + :36; csrc/mf_window_push.hip).
 * buf: device fp32 [n_rows][n], every session's window; new_samples: device fp32 [m][n_new], the step's new samples;
 * rows: HOST array of m distinct pool rows, read during the call only (the table travels in the launch arguments, 64 rows
 * per launch; a longer list goes out as several launches); win: device fp32 [m][n].  For i in [0, m), r = rows[i]:
 * buf[r] <- concat(buf[r][n_new:], new_samples[i]) and win[i] <- the same n values; rows the table does not name keep
 * their bytes.  One workgroup per row: the kept context of n - n_new floats goes through LDS, so the overlapping shift
 * (n_new < n - n_new) is exact.  Refuses null pointers, m < 1, n_rows < 1, an n_new outside [1, n], a row outside
 * [0, n_rows), a row named twice, a context of more than 160 KB and win / new_samples that overlap buf or each other
 * (MF_ERR_INVALID, the value named in mf_last_error) before anything is launched. */
int mf_windows_push(float* buf, int n_rows, int n, const float* new_samples, int n_new, const int* rows, int m, float* win, void* stream);

/* ---- fused multi-head attention (test seam of the kernel both transformer stages run on) ---- */
/* out = softmax(q k^T / sqrt(head_dim)) v per (batch, head): the `Attention` of the diffusers
 * BasicTransformerBlock that musetalk/models/unet.py:36-47 instantiates (attn1: tk == tq; attn2: tk = audio
 * tokens) and `MultiHeadAttention.qkv_attention` of musetalk/whisper/whisper/model.py:62-93.
 * q, out: device fp32 [batch][tq][heads*head_dim]; k, v: device fp32 [batch][tk][heads*head_dim];
 * head_dim in {40, 64, 80, 160}.  Synchronises the stream before returning. */
int mf_attention_forward(const float* q, const float* k, const float* v, float* out, int batch, int tq, int tk,
                         int heads, int head_dim, int precision, void* stream);

/* ---- token-sequence ops one at a time (test seams of LayerNorm, row softmax, GroupNorm, the plane conversions, the device-packed GEMM, the VAE's
 * uint8 tail and the five-launch composite attention) ------------------------------------------------------------------------------------------ */
/* A view of an activation buffer: channels [coff, coff + c) of a padded NHWC buffer [batch][h + 2*halo][w + 2*halo][cbuf]; token t of the view is
 * pixel (t / w, t % w).  Tensors cross this ABI as device fp32 [batch][h*w][c]. */
typedef struct mf_rows_geom { int cbuf, coff, c, h, w, halo; } mf_rows_geom;
/* Every buffer these calls own is filled with a poison value before the input view is loaded over it: MF_NN_POISON_X3 where the (hi, lo) planes both
 * exist (bf16x3), MF_NN_POISON_BF16 for the hi plane alone.  A non-null `y_full` receives the whole padded OUTPUT buffer [batch][h + 2*halo][w +
 * 2*halo][cbuf] as fp32 (hi + lo): everything outside the written view must still read as the poison.  All calls synchronise the stream. */
#define MF_NN_POISON_X3 (-1231.375f)
#define MF_NN_POISON_BF16 (-1232.0f)
/* fp32 -> planes (+ optional addend [h*w][c], broadcast over the batch) -> fp32.  y (optional): [batch][h*w][c].  y_layered (optional): the first
 * `tokens` tokens into layer `layer` of a caller-initialised [batch][tokens][n_layers][c] tensor (Whisper's embedding gather). */
int mf_rows_roundtrip(const float* x, const float* addend, float* y, float* y_layered, const mf_rows_geom* g, int batch, int tokens, int layer,
                      int n_layers, int precision, float* y_full, void* stream);
/* y = act((x - mean) / sqrt(var + eps) * gamma + beta) per token; tokens > 0: only that prefix of every batch item; act 0 none, 3 GELU (erf).
 * gamma, beta: device fp32 [c].  At most 2048 channels. */
int mf_layernorm_forward(const float* x, const float* gamma, const float* beta, float* y, const mf_rows_geom* gx, const mf_rows_geom* gy, int batch,
                         float eps, int tokens, int act, int precision, float* y_full, void* stream);
/* probs[t][j] = softmax_j(scale * scores[t][j]) over j < n_keys; columns n_keys .. gp->c - 1 are written as zero.  Rows of at most 2048 columns. */
int mf_softmax_rows_forward(const float* scores, float* probs, const mf_rows_geom* gs, const mf_rows_geom* gp, int batch, int n_keys, float scale,
                            int precision, float* y_full, void* stream);
/* GroupNorm [+ SiLU] over (h*w x c/groups) per (batch, group); at most 64 groups and 4096 channels.  stats: device fp64 [batch][groups][2] (sum, sum of
 * squares) -- read when have_stats (the apply kernel alone runs), else optional and filled by the statistics kernel.  scale, shift (optional, together):
 * device fp32 [batch][c], the per-channel affine mf_groupnorm_affine derives (y = x * scale + shift before the SiLU). */
int mf_groupnorm_forward(const float* x, const float* gamma, const float* beta, float* y, const mf_rows_geom* gx, const mf_rows_geom* gy, int batch,
                         int groups, float eps, int silu, int have_stats, double* stats, float* scale, float* shift, int precision, float* y_full,
                         void* stream);
/* out[i][j] = sum_{l < pack_k} a[i][l] * B[j][l] for j < pack_n, 0 for pack_n <= j < n, with B[j][l] = b[j * stride_n + l * stride_k] packed on the device
 * out of the planes of the fp32 matrix b [b_rows][b_cols].  a: [t][k], out: [t][n]; k % 8 == 0.  When pack_n < n or pack_k < k the plan is first packed
 * with the whole n x k operand, so the smaller pack has stale entries to clear.  y_full: [1][3][t + 2][n rounded up to 8]; the GEMM's epilogue stores
 * channel quads, so columns n .. (n rounded up to 4) - 1 of the interior are written too, as zero. */
int mf_gemm_bt_forward(const float* a, const float* b, float* out, int t, int n, int k, int b_rows, int b_cols, int64_t stride_n, int64_t stride_k,
                       int pack_n, int pack_k, int precision, float* y_full, void* stream);
/* (x / 2 + 0.5).clamp(0, 1) * 255, rounded half to even -> dst device uint8 [batch][h][w][3] with the channel order reversed; gx->c == 3. */
int mf_vae_post_u8_forward(const float* x, uint8_t* dst, const mf_rows_geom* gx, int batch, int precision, void* stream);
/* The uint8 producers and the head of Wav2Lip and of the VAE encoder, one launch each.  The two producers write 8-channel buffers of their own: a buffer of
 * batch + 1 items [H + 2*halo][W + 2*halo][8] is poisoned, the kernel fills the interior of the first `batch`, and y_full (required) receives all of it
 * with the allocation's tail, (batch + 1) * (H + 2*halo) * (W + 2*halo) * 8 + 64 fp32 values (hi + lo): ring, last item and tail must still be the poison.
 * faces: device uint8 [.][H][W][3].  rows == NULL: face b of `faces` -> item b (channels 0-2 the face / 255 with rows y >= H / 2 zeroed, 3-5 the whole face,
 * 6-7 zero).  rows: HOST int[batch], item b reads face rows[b] of a pool of n_pool faces (the table travels in the launch arguments, 256 rows per launch);
 * a row outside [0, n_pool) is refused (MF_ERR_INVALID, the row named in mf_last_error) before anything is allocated or launched. */
int mf_faces_u8_forward(const uint8_t* faces, const int* rows, int n_pool, int H, int W, int halo, int batch, int precision, float* y_full, void* stream);
/* img: device uint8 BGR [batch][H][W][3] -> channels 0-2 = ((float)(c / 255.) [0 where half_mask and y >= H / 2] - 0.5) / 0.5 in R, G, B order, 3-7 zero. */
int mf_vae_image_u8_forward(const uint8_t* img, int H, int W, int halo, int half_mask, int batch, int precision, float* y_full, void* stream);
/* sigmoid(w x + b) of a 32-channel view: x device fp32 [batch][g->h * g->w][32] loaded into view g (g->c == 32, coff and cbuf multiples of 8) of a poisoned
 * buffer; w: device fp32 [3][32], b: device fp32 [3].  out: device fp32 [batch][3][h][w] in [0, 1] (hwc255 == 0) or [batch][h][w][3] * 255 (hwc255 == 1). */
int mf_head_sigmoid_forward(const float* x, const mf_rows_geom* g, const float* w, const float* b, int hwc255, float* out, int batch, int precision,
                            void* stream);
/* mf_attention_forward's contract on the five-launch path (pack K, GEMM, row softmax, pack V^T, GEMM) the VAE mid-block runs: any head_dim % 8 == 0. */
int mf_attention_composite_forward(const float* q, const float* k, const float* v, float* out, int batch, int tq, int tk, int heads, int head_dim,
                                   int precision, float* y_full, void* stream);
/* The fused attention kernel (mf_attention_forward's) launched on VIEWS, as the networks launch it.  q, out: device fp32 [batch][gq->h * gq->w][c]; k, v:
 * [batch][gk->h * gk->w][c]; c = heads * head_dim, the same for all four views.  packing 0: q, k and v each in a buffer of their own; 1: q alone, k and v
 * as two slices of ONE buffer (cross-attention: gk and gv name the same cbuf, h, w, halo); 2: all three as slices of one buffer (packed self-attention:
 * gq, gk and gv name the same buffer).  Buffers are sequences (h == 1, any halo) or halo-free maps; every view starts on an 8-channel group.  tq, tk > 0:
 * only the first tq queries attend to the first tk keys of every item; output rows >= tq stay poison.  y_full: the whole padded output buffer of go. */
int mf_attention_view_forward(const float* q, const float* k, const float* v, float* out, const mf_rows_geom* gq, const mf_rows_geom* gk,
                              const mf_rows_geom* gv, const mf_rows_geom* go, int packing, int batch, int heads, int tq, int tk, int precision,
                              float* y_full, void* stream);
/* One convolution layer launched on VIEWS, as the networks launch it (the test seam of the sequence layers: (1 x k) kernels on h == 1 buffers, token
 * prefixes, channel-slice operands).  weight, bias: HOST fp32 [groups][cout][cin][kh][kw] and [groups][cout] (bias optional), no BatchNorm.
 * x: device fp32 [batch][in_h * in_w][gx->c], loaded into the view gx of a buffer whose halo ring is zero and whose other interior channels are poison;
 * gx->h, gx->w are the layer's input size, gx->halo at least what its padding needs, gx->c / groups >= cin rounded up to 8 (the caller fills the padding
 * channels: zero, as the networks do).  The output view gy (gy->c == groups * cout; GEGLU: cout / 2) lies in a fully poisoned buffer of the layer's output
 * size.  res / gr (optional, together): the residual operand [batch][out_h * out_w][gy->c] in view gr of a third buffer; with desc->residual set and no
 * gr the residual is the input's own view.  Group g is a plan of its own from weight[g], launched on channels g * (c / groups) of each view;
 * only_group >= 0 launches that one alone (-1: all).  tokens > 0: the prefix handed to the launch.  pin (optional): HOST int[6] (bm, bn, wgm, wgn, split,
 * ld) for mf_conv2d_pin_config's slot, all zero = unpinned.  info (optional): HOST int[11], what ran, as mf_conv2d_launch_config reports it (resolved with
 * the prefix).  y: the view gy as fp32 [batch][out_h * out_w][gy->c]; y_full: the whole padded output buffer. */
int mf_conv_view_forward(const mf_conv2d_desc* desc, const float* weight, const float* bias, const float* x, const float* res, float* y,
                         const mf_rows_geom* gx, const mf_rows_geom* gy, const mf_rows_geom* gr, int batch, int tokens, int groups, int only_group,
                         const int* pin, int* info, int precision, float* y_full, void* stream);
/* The producers of the MF_PREC_F16Q activation format, one call each: the bytes a convolution of that precision reads.  Per pixel and 32-channel block the
 * first plane holds 32 f16 words and the second 64 bytes [q6(v - f16(v)) | q6(f16(v))], each half 24 bytes of e2m3 codes (channel t of the block in bits
 * [6t, 6t + 6)), one E8M0 scale byte 127 + floor(log2 max) - 2 and 7 zero bytes.
 * x: device fp32 NCHW [batch][gx->c][gx->h][gx->w].  The destination has dst_c channels (a multiple of 32) and its own halo.
 *   mode 0: mf_conv2d_forward's software encoder straight from x (gx->cbuf, coff, halo unused); dst_c >= gx->c, the channels past gx->c encode zero.
 *   mode 1: x is loaded into the slice [coff, coff + c) of a bf16x3 buffer of geometry gx; v = x * scale[b][c] + shift[b][c], SiLU when `silu`, times post[c]
 *           when `post` is not null (powers of two) -- the conversion kernel of the VAE decoder, chosen by the map size as a network's call would.
 *   mode 2: GroupNorm + SiLU [* post] with the affine formed inside the conversion kernel from the statistics (maps of a multiple of 64 pixels only).
 *   mode 3: the same through the statistics + affine launch and the array form of mode 1.
 * Modes 1 to 3 need dst_c == gx->c and coff % 8 == 0.  gamma, beta, post: device fp32 [c]; scale, shift: device fp32 [batch][c].
 * Both buffers are filled with the words MF_ACT_Q_POISON_HI / _LO first.  dst_hi, dst_lo: device, batch * (h + 2*dst_halo) * (w + 2*dst_halo) * dst_c + 64
 * 16-bit words each -- the whole padded destination planes with the allocation's tail.  src_full (optional, modes 1 to 3): the whole source buffer with its
 * tail, batch * (h + 2*halo) * (w + 2*halo) * cbuf + 64 fp32 values (hi + lo; MF_NN_POISON_X3 where nothing was loaded).  Synchronises the stream; nothing is
 * written to the outputs when the call fails. */
#define MF_ACT_Q_POISON_HI 0xC49A
#define MF_ACT_Q_POISON_LO 0x3F20
int mf_act_q_encode(const float* x, const mf_rows_geom* gx, int batch, int dst_c, int dst_halo, int mode, int silu, const float* scale, const float* shift,
                    const float* post, const float* gamma, const float* beta, int groups, float eps, uint16_t* dst_hi, uint16_t* dst_lo, float* src_full,
                    void* stream);

/* ---- MuseTalk Whisper audio features (H3) -------------------------------------------------- */
typedef struct mf_whisper mf_whisper;

/* Replaces `load_model(path)` of musetalk/whisper/whisper/__init__.py:108-116 for the ENCODER half
 * (`Whisper.encoder`, model.py:131-171): weights = the encoder state-dict tensors ("conv1.weight",
 * "blocks.N.attn.query.weight", ...; an "encoder." prefix is accepted); n_head comes from the checkpoint's
 * dims (6 for tiny); n_state / n_layer are inferred from the tensors, n_ctx is 1500 (30 s). */
int mf_whisper_create(const mf_tensor* weights, int n_weights, int n_head, int precision, mf_whisper** out);
int mf_whisper_dims(const mf_whisper* h, int* n_layer, int* n_ctx, int* n_state);

/* Replaces `log_mel_spectrogram(audio)` (whisper/audio.py:92-125): wav device fp32 [n], 160 <= n <= 480000
 * -> out device fp32 [80, n/160]. */
int mf_whisper_log_mel(mf_whisper* h, const float* wav, int n, float* out, void* stream);

/* One segment of `transcribe` (transcribe.py:103-126): log-mel, pad to 3000 frames,
 * `encoder(segment, include_embeddings=True)`.  emb: device fp32 [n_layer+1][1500][n_state]
 * (= the reference's embeddings[0], model.py:158-168).  n <= 480000 samples (one 30 s segment). */
int mf_whisper_encode_audio(mf_whisper* h, const float* wav, int n, float* emb, void* stream);

/* The streaming form of the same stage: what `MuseASR.run_step` needs from `audio2feat` for the
 * sliding windows of one or several sessions (museasr.py:25-26 -> audio2feature.py:99-112 -> transcribe.py:103-126).
 * wav: device fp32 [n_windows][n], every window the same length (the render loop's (2B + l + r) * 320 samples);
 * feat: device fp32 [n_windows][n/320][n_layer+1][n_state] -- `concatenated_array` of audio2feature.py:110 per window.
 * ctx_tokens = 0 keeps the reference's 1500-token context; the result equals mf_whisper_encode_audio's first n/320 tokens
 * (the last block evaluates only the consumed queries -- its keys / values still span the whole context -- and all
 * windows share every launch).  ctx_tokens > 0 shortens the context to that many tokens: an approximation, because the
 * encoder's attention is global and unmasked; bench.py reports its error next to its time.
 * mf_whisper_set_batch sizes the workspace for up to max_windows windows per call (default 1). */
int mf_whisper_set_batch(mf_whisper* h, int max_windows);
int mf_whisper_encode_windows(mf_whisper* h, const float* wav, int n, int n_windows, int ctx_tokens, float* feat, void* stream);
void mf_whisper_destroy(mf_whisper* h);

/* ---- Whisper text decoder: transcription by greedy decoding ------------------------------------ */
/* The handle is untyped (void*): what mf_whisper_decoder_create stores in *out, passed back as `h`. */

/* The DECODER half of the same checkpoint (`Whisper.decoder`, model.py:174-217): weights = the tensors named "decoder.*" as a Whisper
 * state dict names them ("decoder.token_embedding.weight", "decoder.positional_embedding", "decoder.blocks.N.attn.query.weight",
 * "decoder.blocks.N.cross_attn.key.weight", "decoder.ln.weight", ...).  "encoder.ln_post.weight" / ".bias" are optional: when present,
 * mf_whisper_decoder_begin applies that LayerNorm (model.py:165) to the encoder states first -- mf_whisper_encode_audio returns the last
 * block's output without it.  n_state / n_layer / n_text_ctx / n_vocab are inferred; n_state = 64 * n_head and a multiple of 128.
 * max_batch: sequences decoded together, 1..8. */
int mf_whisper_decoder_create(const mf_tensor* weights, int n_weights, int n_head, int precision, int max_batch, void** out);
int mf_whisper_decoder_dims(const void* h, int* n_layer, int* n_text_ctx, int* n_state, int* n_vocab);

/* Starts a segment for `batch` sequences: enc_states device fp32 [batch][T_audio][n_state], 1 <= T_audio <= 1500 (only these rows are read);
 * projects the cross-attention keys and values of every layer once, zeroes the self-attention caches, sets every sequence's length to 0. */
int mf_whisper_decoder_begin(void* h, const float* enc_states, int T_audio, int batch, void* stream);

/* `TextDecoder.forward(tokens, xa, kv_cache)`: appends n tokens per sequence at the caches' current offset (0 after begin) under the causal
 * mask and returns their logits.  tokens: device int32 [batch][n]; logits: device fp32 [batch][n][n_vocab].  n = 1 repeated is the decode
 * step fed by the caller.  Refused when the offset + n exceeds n_text_ctx, and after a greedy run until the next begin. */
int mf_whisper_decoder_logits(void* h, const int* tokens, int n, float* logits, int batch, void* stream);

/* Greedy decoding of the segment begun last (GreedyDecoder of decoding.py at temperature 0, without timestamp rules): prefill of every prompt
 * in one pass, then one token per sequence and step, chosen on the device as argmax(logits + suppress_mask), lowest index on a tie.
 * prompts: HOST int32, the sequences' prompt tokens one after the other; prompt_lens: HOST int32 [batch], each 1..n_text_ctx / 2;
 * suppress_mask: device fp32 [n_vocab] of 0 / -inf, or NULL; out_tokens: HOST int32 [batch][max_new] (the tokens before end-of-text, the
 * rest 0); out_lens: HOST int32 [batch]; sum_logprobs: HOST fp32 [batch], log-softmax of the masked logits at every chosen token, the
 * end-of-text token's included.  A sequence stops at `eot`, after max_new tokens, or when its cache is full (n_text_ctx rows); from then on no
 * launch writes its cache rows, output or counters.  The host reads the done flags every `check_every` steps (>= 1) and at no other time;
 * the result does not depend on check_every.  max_new <= n_text_ctx - (shortest prompt) + 1.  Returns when the tokens are on the host. */
int mf_whisper_decoder_greedy(void* h, const int* prompts, const int* prompt_lens, const float* suppress_mask, int eot, int max_new,
                              int check_every, int* out_tokens, int* out_lens, float* sum_logprobs, int batch, void* stream);

/* mf_whisper_decoder_greedy under the reference's logit filters, applied in the launch that chooses the token, in the reference's order
 * (decoding.py:387-441): SuppressBlank, SuppressTokens (suppress_mask), ApplyTimestampRules; then GreedyDecoder.update at temperature 0.  Each
 * sequence reads its own history on the device (tokens sampled so far, the last two), so "first sampled position" is per sequence.
 *   timestamp_begin              eot < timestamp_begin <= n_vocab; -1: no timestamp rules (no_timestamps and the cap are then not read)
 *   no_timestamps                the <|notimestamps|> id, never chosen under the timestamp rules; -1: none
 *   max_initial_timestamp_index  at the first sampled position timestamps above timestamp_begin + index are out; -1: none
 *   blank                        at the first sampled position this id and eot are out; -1: off
 *   no_speech                    -1: none.  Otherwise sot_index (HOST int32 [batch], the index of <|startoftranscript|> inside each prompt) names one
 *                                more prefill row per sequence, and no_speech_probs (HOST fp32 [batch]) receives softmax(its logits)[no_speech]
 * A step makes the launches of a greedy step, one for one (the rule kernel stands in k_dec_choose's place), and waits for no host read.  With timestamp_begin, blank and no_speech all -1 the tokens and the
 * summed log-probabilities are those of mf_whisper_decoder_greedy, bit for bit.  Every id is checked against the vocabulary before anything
 * is enqueued. */
int mf_whisper_decoder_decode(void* h, const int* prompts, const int* prompt_lens, const float* suppress_mask, int eot, int max_new, int check_every,
                              int timestamp_begin, int no_timestamps, int max_initial_timestamp_index, int blank, int no_speech, const int* sot_index,
                              int* out_tokens, int* out_lens, float* sum_logprobs, float* no_speech_probs, int batch, void* stream);

/* `detect_language` (decoding.py:19-69) directly after mf_whisper_decoder_begin: forwards the single token `sot` per sequence, takes the argmax
 * (lowest id on a tie) and the softmax over language_tokens (HOST int32 [n_languages], distinct ids) on the device, and reads both back at once.
 * out_tokens: HOST int32 [batch]; out_probs: HOST fp32 [batch][n_languages] in the list's order.  Afterwards the handle stands as after begin:
 * lengths 0, cache row 0 zeroed again. */
int mf_whisper_decoder_detect_language(void* h, int sot, const int* language_tokens, int n_languages, int* out_tokens, float* out_probs, int batch,
                                       void* stream);

/* Test seam: the token choice of mf_whisper_decoder_decode alone.  logits: device fp32 [batch][n_vocab]; history: HOST int32 [batch][3] = tokens
 * sampled so far, the last one, the one before it (read only as far as the count says); tokens / logprobs / done: HOST [batch], in and out --
 * a sequence whose done flag is set on entry keeps all three; otherwise tokens = the argmax (-1: no admissible finite logit, done = 1),
 * logprobs = its log-softmax under the filters, done = 1 at eot.  batch <= max_batch.  Touches none of the handle's decode state.  Synchronises. */
int mf_whisper_decoder_choose(void* h, const float* logits, const int* history, const float* suppress_mask, int eot, int timestamp_begin, int no_timestamps,
                              int max_initial_timestamp_index, int blank, int* tokens, float* logprobs, int* done, int batch, void* stream);

/* Test seam: the self-attention cache of one layer and sequence, k and v HOST fp32 [n_text_ctx][n_state] each, and the sequence's length.
 * Synchronises the device. */
int mf_whisper_decoder_cache_read(const void* h, int layer, int seq, float* k, float* v, int* len);
void mf_whisper_decoder_destroy(void* h);

/* ---- MuseTalk UNet (H4) and VAE decode (H5) --------------------------------------------------- */
/* The reference builds both from diffusers with config files it does not ship (musetalk/models/unet.py:34-37,
 * vae.py:24), so the architecture is a parameter here.  Field meaning = the diffusers config keys. */
typedef struct mf_unet_config {
    int in_channels, out_channels;      /* 8, 4 */
    int n_blocks;                        /* len(block_out_channels), <= 4 */
    int block_out_channels[4];          /* 320, 640, 1280, 1280 */
    int layers_per_block;               /* 2 */
    int cross_attention_dim;            /* 384 */
    int attention_heads;                /* config key "attention_head_dim": 8 heads */
    int norm_num_groups;                /* 32 */
    int down_attn[4], up_attn[4];       /* CrossAttn{Down,Up}Block2D vs {Down,Up}Block2D */
    int sample_size;                    /* latent H = W: 32 */
    int ctx_len;                        /* audio tokens per frame: 50 */
} mf_unet_config;

typedef struct mf_vae_config {
    int latent_channels, out_channels;  /* 4, 3 */
    int n_blocks;
    int block_out_channels[4];          /* 128, 256, 512, 512 */
    int layers_per_block;               /* 2 */
    int norm_num_groups;                /* 32 */
    int sample_size;                    /* latent H = W: 32 */
    float scaling_factor;               /* 0.18215 */
} mf_vae_config;

typedef struct mf_unet mf_unet;
typedef struct mf_vae mf_vae;

/* Replaces `UNet(unet_config, model_path)` (musetalk/models/unet.py:29-44): weights = the
 * UNet2DConditionModel state dict (diffusers key names).  The timestep is fixed to 0 as musereal.py:59 does;
 * its embedding is folded into the resnet biases at create time. */
int mf_unet_create(const mf_unet_config* cfg, const mf_tensor* weights, int n_weights, int precision, int max_batch,
                   mf_unet** out);
/* Replaces `pe(audio)` + `unet.model(latent_batch, timesteps, encoder_hidden_states=audio).sample`
 * (musereal.py:102-107).  latents: device fp32 [B,in_channels,S,S]; audio: device fp32 [B,ctx_len,cross_dim];
 * add_pe != 0 adds the PositionalEncoding of unet.py:12-27 to `audio` first; out: device fp32 [B,out_channels,S,S]. */
int mf_unet_forward(mf_unet* h, const float* latents, const float* audio, int add_pe, float* out, int batch, void* stream);
/* Measurement seam (bench.py roofline): the schedule's ops in execution order on the buffers of the last forward.
 * op_info: name = the diffusers module path, kernel = HIP kernel(s) it launches, flops_per_frame = 2 x MACs.
 * profile: every op alone between two hipEvents on `stream`, hipGraph off; mean milliseconds per op. */
int mf_unet_num_ops(const mf_unet* h);
int mf_unet_op_info(const mf_unet* h, int i, char* name, int ncap, char* kernel, int kcap, double* flops_per_frame);
int mf_unet_profile(mf_unet* h, int batch, int iters, float* ms_per_op, void* stream);
int mf_unet_tune(mf_unet* h, int batch, void* stream);                       /* explicit launch-configuration warm-up: see mf_wav2lip_tune */
void mf_unet_destroy(mf_unet* h);

/* Replaces `AutoencoderKL.from_pretrained` for the DECODER half (musetalk/models/vae.py:24,96-108). */
int mf_vae_create(const mf_vae_config* cfg, const mf_tensor* weights, int n_weights, int precision, int max_batch,
                  mf_vae** out);
/* `VAE.decode_latents` (vae.py:96-108): latents device fp32 [B,4,S,S] -> frames device uint8 [B,8S,8S,3] BGR.
 * image_f32 (optional, may be NULL): the decoder output before post-processing, device fp32 [B,3,8S,8S]. */
int mf_vae_decode_latents(mf_vae* h, const float* latents, uint8_t* frames, float* image_f32, int batch, void* stream);
int mf_vae_num_ops(const mf_vae* h);
int mf_vae_op_info(const mf_vae* h, int i, char* name, int ncap, char* kernel, int kcap, double* flops_per_frame);
int mf_vae_profile(mf_vae* h, int batch, int iters, float* ms_per_op, void* stream);
int mf_vae_tune(mf_vae* h, int batch, void* stream);                         /* explicit launch-configuration warm-up: see mf_wav2lip_tune */
void mf_vae_destroy(mf_vae* h);

/* ---- ER-NeRF inference kernels (H6): the functions of the reference's four torch extensions ------------------
 * Same argument order and in-place output conventions as the pybind entry points the Python wrappers call, so
 * `ernerf/raymarching/raymarching.py`, `gridencoder/grid.py`, `shencoder/sphere_harmonics.py`, `freqencoder/freq.py`
 * run unchanged on top of them.  All pointers are device fp32 / int32 / uint8 unless
 * noted; all calls are asynchronous on `stream`. */

/* `_backend.near_far_from_aabb(rays_o, rays_d, aabb, N, min_near, nears, fars)` (raymarching.py:44 ->
 * kernel_near_far_from_aabb, raymarching.cu:92-145).  rays_o/d [N,3], aabb [6]; a miss writes FLT_MAX to both. */
int mf_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb, uint32_t n_rays, float min_near,
                          float* nears, float* fars, void* stream);
/* `_backend.march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H,
 * density_bitfield, near, far, xyzs, dirs, deltas, noises)` (raymarching.py:393 -> kernel_march_rays,
 * raymarching.cu:828-929).  xyzs/dirs [n_alive*n_step,3] and deltas [n_alive*n_step,2] must be zero-filled by the
 * caller (raymarching.py:383-385): dt == 0 marks "no sample". */
int mf_march_rays(uint32_t n_alive, uint32_t n_step, const int* rays_alive, const float* rays_t, const float* rays_o,
                  const float* rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t cascades, uint32_t grid_size,
                  const uint8_t* density_bitfield, const float* nears, const float* fars, float* xyzs, float* dirs,
                  float* deltas, const float* noises, void* stream);
/* `_backend.composite_rays_triplane(...)` (raymarching.py:666 -> kernel_composite_rays_triplane,
 * raymarching.cu:2142-2249): updates rays_alive (-1 = terminated), rays_t and the [N]-sized accumulators in place. */
int mf_composite_rays_triplane(uint32_t n_alive, uint32_t n_step, float T_thresh, int* rays_alive, float* rays_t,
                               const float* sigmas, const float* rgbs, const float* deltas, const float* ambs_aud,
                               const float* ambs_eye, const float* uncertainties, float* weights_sum, float* depth,
                               float* image, float* amb_aud_sum, float* amb_eye_sum, float* uncertainty_sum, void* stream);
/* `_backend.grid_encode_forward(inputs, embeddings, offsets, outputs, B, D, C, L, S, H, dy_dx, gridtype,
 * align_corners)` (grid.py:49 -> kernel_grid, gridencoder.cu:76-165), inference only (no dy_dx).
 * inputs [B,D] in [0,1]; embeddings [offsets[L], C]; offsets_host: HOST int32 [L+1]; S = log2(per_level_scale);
 * outputs [L,B,C] as the extension writes it, or -- out_blc != 0 -- [B, L*C], the layout grid.py:52 permutes to.
 * D in {2,3}, C in {1,2,4,8}, L <= 32. */
int mf_grid_encode_forward(const float* inputs, const float* embeddings, const int* offsets_host, float* outputs, uint32_t B,
                           uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                           int out_blc, void* stream);
/* `_backend.sh_encode_forward(inputs, outputs, B, input_dim, degree, dy_dx)` (sphere_harmonics.py:32 -> kernel_sh,
 * shencoder.cu:28-110), inference only; inputs [B,3], outputs [B,degree^2], degree 1..4. */
int mf_sh_encode_forward(const float* inputs, float* outputs, uint32_t B, uint32_t degree, void* stream);
/* `_backend.freq_encode_forward(inputs, B, input_dim, degree, output_dim, outputs)` (freq.py:29 -> kernel_freq,
 * freqencoder.cu:30-58); outputs [B, D + 2*D*degree]. */
int mf_freq_encode_forward(const float* inputs, uint32_t B, uint32_t D, uint32_t degree, uint32_t C, float* outputs, void* stream);

/* `_backend.morton3D(coords, N, indices)` (raymarching.py:98 -> kernel_morton3D, raymarching.cu:214-226): coords int32 [N,3] ->
 * indices int32 [N], 10 bits per axis interleaved (x in bit 0, y in bit 1, z in bit 2). */
int mf_morton3d(const int* coords, uint32_t n, int* indices, void* stream);
/* `_backend.morton3D_invert(indices, N, coords)` (raymarching.py:120 -> kernel_morton3D_invert, raymarching.cu:237-254):
 * indices int32 [N] -> coords int32 [N,3]. */
int mf_morton3d_invert(const int* indices, uint32_t n, int* coords, void* stream);
/* `_backend.packbits(grid, N, density_thresh, bitfield)` (raymarching.py:149 -> kernel_packbits, raymarching.cu:268-289):
 * grid fp32 [N*8] -> bitfield uint8 [N]; bit i of byte n is (grid[8n + i] > density_thresh), a strict comparison. */
int mf_packbits(const float* grid, uint32_t n_bytes, float density_thresh, uint8_t* bitfield, void* stream);
/* `_backend.morton3D_dilation(grid, C, H, grid_dilation)` (raymarching.py:175 -> kernel_morton3D_dilation, raymarching.cu:304-335):
 * grid fp32 [C, H^3] in Morton order -> out [C, H^3], fmaxf over a cell and its six neighbours, clipped at the borders.
 * H <= 1024, C * H^3 < 2^32; out must not alias grid. */
int mf_morton3d_dilation(const float* grid, uint32_t cascades, uint32_t grid_size, float* out, void* stream);

/* Tail of `run_cuda` (renderer.py:275-280) and the uint8 conversion of nerfreal.py:111, in place:
 * image[N,3] = clamp(image + (1 - weights_sum) * bg, 0, 1); depth[N] = clamp(depth - near, 0) / (far - near);
 * frame_u8 (optional, may be NULL) = uint8(image * 255), truncating like ndarray.astype.  bg_color: device fp32 [N,3]
 * (bg_per_ray != 0), [3], or NULL for the scalar bg_const (`bg_color = 1`, renderer.py:309-310). */
int mf_nerf_finish(float* image, float* depth, const float* weights_sum, const float* nears, const float* fars, const float* bg_color,
                   int bg_per_ray, float bg_const, uint32_t n_rays, uint8_t* frame_u8, void* stream);

/* ---- ER-NeRF radiance field (H6) ---------------------------------------------------------- */
typedef struct mf_nerf_field mf_nerf_field;
typedef struct mf_nerf_field_config {
    float bound;                 /* opt.bound (app.py:603): positions live in [-bound, bound] */
    int num_levels;              /* 12 (network.py:122) */
    int level_dim;               /* 1 */
    int base_resolution;         /* 64 */
    float log2_per_level_scale;  /* S of grid.py:33 */
    int offsets[33];             /* GridEncoder.offsets (grid.py:108-123), num_levels + 1 entries */
    int audio_dim;               /* 32 */
    int geo_feat_dim;            /* 64 */
    int hidden_dim;              /* 64 */
    int individual_dim;          /* opt.ind_dim, 4 */
    int exp_eye;                 /* opt.exp_eye */
} mf_nerf_field_config;
/* Replaces the inference half of `NeRFNetwork` (network.py:93-160): weights = the state-dict tensors
 * "encoder_{xy,yz,xz}.embeddings", "{sigma_net,color_net,aud_ch_att_net,eye_att_net}.net.N.weight" (fp32, host). */
int mf_nerf_field_create(const mf_nerf_field_config* cfg, const mf_tensor* weights, int n_weights, int precision,
                         int max_samples, mf_nerf_field** out);
/* Replaces `self.forward(xyzs, dirs, enc_a, ind_code, eye)` (renderer.py:260 -> network.py:249-277, density :280-308).
 * xyzs, dirs: device fp32 [M,3]; enc_a: device fp32 [32]; ind_code: device fp32 [individual_dim] or NULL; eye: the
 * scalar of opt.exp_eye.  Outputs (device fp32): sigmas [M], rgbs [M,3], amb_aud [M] (= ||aud_ch_att||), amb_eye [M],
 * uncertainty [M] (ln 2 in test mode, may be NULL). */
int mf_nerf_field_forward(mf_nerf_field* h, const float* xyzs, const float* dirs, const float* enc_a, const float* ind_code,
                          float eye, int n_samples, float* sigmas, float* rgbs, float* amb_aud, float* amb_eye,
                          float* uncertainty, void* stream);
/* Replaces the head branch of `NeRFRenderer.update_extra_state` (renderer.py:437-485) as three launches, no host
 * synchronisation: (a) the density half of the field (network.py:280-308) swept over the cascades x grid_size^3 cell
 * centres of :458-467 -- bound_c = min(2^cas, bound), half = bound_c / grid_size, position = (2 c / (H - 1) - 1) *
 * (bound_c - half) + (2 u - 1) * half in the reference's float32 statement order -- sigma * density_scale written to
 * tmp_grid in Morton order; (b) six-neighbour max of tmp_grid and, where grid >= 0 and the max >= 0, grid =
 * fmaxf(grid * decay, max) (:475-479), cells marked -1 kept; (c) mean_density = mean of max(grid, 0) as an fp64 sum in a
 * fixed order, density_bitfield = packbits(grid, min((float)mean_density, density_thresh)) (:480-485).
 * density_grid: device fp32 [cascades, grid_size^3], in/out; density_bitfield: uint8 [cascades * grid_size^3 / 8], out;
 * enc_a: device fp32 [32]; eye: the scalar of opt.exp_eye, used when use_eye (the field must have been created with
 * exp_eye; without use_eye such a field sees e = 0); noise: device fp32 [cascades, grid_size^3, 3], the torch.rand values
 * of :467 in meshgrid order ((x H + y) H + z), or NULL for cell centres; tmp_grid: fp32 [cascades, grid_size^3], holds
 * the sweep's (undilated) values afterwards; xyzs_out: fp32 [cascades, grid_size^3, 3] in Morton order, or NULL;
 * mean_density: device fp64, 1 value.  grid_size 32, 64 or 128, cascades 1..8, else MF_ERR_INVALID with the limit named in
 * mf_last_error.  Needs the fused field kernel and runs in the field's precision mode. */
int mf_nerf_density_grid_update(mf_nerf_field* field, float* density_grid, uint8_t* density_bitfield, int cascades, int grid_size, float bound,
                                const float* enc_a, float eye, int use_eye, float density_scale, float decay, float density_thresh,
                                const float* noise, float* tmp_grid, float* xyzs_out, double* mean_density, void* stream);
/* Replaces `NeRFRenderer.mark_untrained_grid` (renderer.py:356-416) as one launch: one lane per (cascade, Morton index) forms
 * the cell centre world = (2 c / (H - 1) - 1) * (bound_c - bound_c / H) (:387-394, float32 statement order) and walks the poses
 * (camera-to-world, device fp32 [n_poses, 4, 4]): cam = (world - t) @ R; the cell is covered when cam.z > 0 and
 * |cam.x| < (cx / fx) cam.z + 2 bound_c / H and |cam.y| < (cy / fy) cam.z + 2 bound_c / H (:402-408; the Python scalars are formed in
 * double and rounded to fp32 where they meet the tensor).  A cell no pose covers gets -1 (:416); every other cell keeps its bits.
 * density_grid: device fp32 [cascades, grid_size^3] in Morton order, in/out.  grid_size 32, 64 or 128, cascades 1..8,
 * n_poses >= 1, else MF_ERR_INVALID with the limit named in mf_last_error. */
int mf_nerf_mark_untrained(const float* poses, int n_poses, double fx, double fy, double cx, double cy, float bound, int cascades,
                           int grid_size, float* density_grid, void* stream);
void mf_nerf_field_destroy(mf_nerf_field* h);

/* a24, `Trainer.test_gui_with_data` utils.py:1208-1216 + nerfreal.py:111: the [h,w] render resized to the GUI's [H,W].
 * image [h,w,3] -> out_image [H,W,3] as F.interpolate(mode='bilinear') (align_corners False, no antialias); depth [h,w] ->
 * out_depth [H,W] as mode='nearest'; frame_u8 [H,W,3] = uint8(out_image * 255) truncating.  Any of the three outputs may
 * be NULL (depth may be NULL when out_depth is). */
int mf_nerf_resize_frame(const float* image, const float* depth, int h, int w, int H, int W, float* out_image, float* out_depth,
                         uint8_t* frame_u8, void* stream);

/* `NeRFDataset_Test.collate`, provider.py:316-330 (the default deployment: --torso_imgs with a head-only model, app.py:368-369): the frame's torso image
 * over the background, bg_color = rgb * a + bg * (1 - a) (provider.py:323), as one launch.  torso_rgba: device uint8 [H,W,4] RGBA (4-byte aligned);
 * bg_image: device fp32 [H,W,3], or NULL for the constant bg_const in every channel (`--bg_img white` / `black`, provider.py:203-206);
 * bg_color: device fp32 [H*W,3].  The bits are those of the torch expression: half_mode == 0 (preload 0 / 1) t = float(u8) / 255 as
 * `astype(np.float32) / 255` gives (provider.py:186, 321), then product, 1 - a, product, sum, each rounded to fp32; half_mode != 0 (preload 2: torso_img
 * and bg_img are half tensors, provider.py:198, 238) t = half(float(u8) / 255), bg = half(bg), each of the four operations computed in fp32 and
 * rounded to half, the result widened to fp32. */
int mf_nerf_frame_background(const uint8_t* torso_rgba, const float* bg_image, float bg_const, int H, int W, int half_mode, float* bg_color,
                             void* stream);
/* The rest of one `nerfreal.py` frame behind the render, as one launch that ends in the uint8 RGB frame a VideoFrame takes: the resize of
 * `Trainer.test_gui_with_data` (utils.py:1208-1212; linear_to_srgb != 0 applies utils.py:78-81 to the render first, as :1208-1209 orders it),
 * `(image * 255).astype(np.uint8)` (nerfreal.py:110) and, with a body frame, the --fullbody paste and its cvtColor (nerfreal.py:117-122).
 * render: device fp32 [h,w,3] or NULL; (H, W): the GUI size; body_bgr: device uint8 BGR [FH,FW,3] or NULL; (x0, y0): opt.fullbody_offset_x / _y.
 * frame_rgb: device uint8 RGB [FH,FW,3], or [H,W,3] without a body frame (FH, FW, x0, y0 are then ignored and must leave the offset at 0).
 * Inside the [H,W] rectangle at (x0, y0) a pixel is mf_nerf_resize_frame's frame_u8 of the same render, bit for bit (one device function serves both); outside
 * it the body pixel with its channels reversed.  render NULL: the whole output is the channel-reversed body_bgr -- the custom-video frame of
 * nerfreal.py:98-107.  A rectangle that leaves the body frame is MF_ERR_INVALID with both sizes in mf_last_error, as the reference's slice assignment
 * raises; nothing is clipped. */
int mf_nerf_frame_out(const float* render, int h, int w, int H, int W, const uint8_t* body_bgr, int FH, int FW, int x0, int y0, int linear_to_srgb,
                      uint8_t* frame_rgb, void* stream);

/* ---- the three stages around the batched head render, for every frame of a step in one launch each (mf_nerf_frame_batch.hip) ----
 * mf_nerf_frame_background, mf_nerf_torso_forward and mf_nerf_frame_out with a frame index in the grid (blockIdx.y): frame i of a call is the same
 * bits as the single-frame entry point gives for the same inputs -- the per-pixel code is shared, and a frame's pixels keep tiles of their own (a frame
 * whose pixel count is no multiple of the tile has a partial last tile; pixels of two frames never share one).
 * The handle owns a ring of 16 descriptor tables in pinned host memory with their device copies, allocated at the first accepted call.  A call
 * fills the next table, copies it to the device asynchronously on the caller's stream, launches, and records an event; it waits for the host only
 * when all 16 entries belong to calls still in flight.  What the descriptors point at must stay valid until the call's launch has run.
 * All frames of a call share the sizes; what a descriptor holds is per frame.  max_frames 1..64; max_pixels is per frame (the torso kernel keeps
 * every pixel's activations on chip, so the handle holds no per-pixel scratch: max_pixels bounds n_pixels and nothing else). */
typedef struct mf_nerf_frame_batch mf_nerf_frame_batch;
typedef struct mf_nerf_bg_desc {
    const uint8_t* torso_rgba;         /* device, uint8 [H, W, 4], 4-byte aligned */
    const float* bg_image;             /* device, fp32 [H, W, 3], or NULL: bg_const */
    float bg_const;
    int half_mode;
    float* bg_color;                   /* output, device fp32 [H * W, 3] */
} mf_nerf_bg_desc;
typedef struct mf_nerf_torso_desc {
    float frame_consts[50];            /* the [42 + individual_dim] constants of mf_nerf_torso_forward, by value */
    const float* bg_coords;            /* device, [n_pixels, 2] */
    const float* bg_color;             /* as mf_nerf_torso_forward */
    int bg_per_ray;
    float bg_const, density_thresh;
    float *bg_out, *torso_alpha, *deform;   /* outputs, device: [n_pixels, 3], [n_pixels] or NULL, [n_pixels, 2] or NULL */
} mf_nerf_torso_desc;
typedef struct mf_nerf_out_desc {
    const float* render;               /* device fp32 [h, w, 3], or NULL: a custom-video frame (body_bgr alone, channels reversed) */
    const uint8_t* body_bgr;           /* device uint8 [FH, FW, 3], or NULL (then FH x FW = H x W and the offset is 0) */
    int x0, y0;
} mf_nerf_out_desc;
int mf_nerf_frame_batch_create(int max_frames, int max_pixels, mf_nerf_frame_batch** out);
void mf_nerf_frame_batch_destroy(mf_nerf_frame_batch* h);
/* mf_nerf_frame_background for n_frames frames of H x W pixels */
int mf_nerf_frame_batch_background(mf_nerf_frame_batch* h, const mf_nerf_bg_desc* descs, int n_frames, int H, int W, void* stream);
/* (mf_nerf_torso_forward_batch stands with the torso handle below) */
/* mf_nerf_frame_out for n_frames frames into one block frames_rgb uint8 [n_frames, FH, FW, 3] (what mf_frames_to_i420 takes) */
int mf_nerf_frame_batch_out(mf_nerf_frame_batch* h, const mf_nerf_out_desc* descs, int n_frames, int rh, int rw, int H, int W, int FH, int FW,
                            int linear_to_srgb, uint8_t* frames_rgb, void* stream);

/* ---- the audio features of many ER-NeRF sessions (mf_nerf_featpool.hip; nerf_serving.NerfFeaturePool) ---- */
/* What `NerfASR` keeps per session in torch tensors, for N sessions in two caller-owned device buffers: rings fp32 [N][R][dim] (`feat_queue`,
 * nerfasr.py:48-50; R = feat_buffer_size * m = 32) and hist fp32 [N][8][dim][16] (`att_feats`, nerfasr.py:55, as a circular buffer).  All entries are
 * stateless, take HOST int arrays of one value per picked session (read during the call only; they travel as launch arguments), check every argument
 * before anything is enqueued and never wait for the host: one launch per 64 picked sessions.  dim 1..1024, R >= 16, rows distinct and inside N, else
 * MF_ERR_INVALID.  They move fp32 values only.
 *
 * mf_nerf_feat_scatter (nerfasr.py:119-124, 140-142): feats is the net's output for the n_sessions picked sessions, device fp32 [n_sessions][T][dim];
 * rows [left, right) of feats[i] are copied to ring rows starts[i] .. starts[i] + right - left of session rows[i] (starts[i] = feat_buffer_idx * m); a
 * block that leaves the ring is refused, as the slice assignment raises. */
int mf_nerf_feat_scatter(const float* feats, int n_sessions, int T, int dim, int left, int right, float* rings, int N, int R,
                         const int* rows, const int* starts, void* stream);
/* mf_nerf_feat_windows (nerfasr.py:75-103), per picked session i: out[i] (device fp32 [n_sessions][8][dim][16]) receives the session's eight windows,
 * oldest first; fronts (HOST int [n_sessions][8]) names the ring row each starts at, or -1 for a zero window of nerfasr.py:55.  A window is ring rows
 * (front + t) mod R, t = 0..15, transposed to [dim][16].  The last n_new[i] windows are new: read from the ring and also stored in history slots
 * (heads[i] + j) mod 8.  The older ones occupy the slots from (heads[i] + n_new[i]) mod 8 on and come out as `torch.stack` finds them in the reference: a
 * window that wraps round the ring's end (front + 16 >= R) was concatenated, a copy -- from its history slot, as a zero window is (the caller zeroes
 * those slots); one that does not wrap is a view of `feat_queue` and shows what has been written under it since -- read from the ring again.  n_new is 1
 * in steady state and 4 on a session's first call.  att == 0: no history (hist, heads may be NULL), fronts is [n_sessions][1], n_new[i] must be 1 and
 * out is [n_sessions][1][dim][16]. */
int mf_nerf_feat_windows(const float* rings, float* hist, int N, int R, int dim, int n_sessions, const int* rows, const int* fronts,
                         const int* heads, const int* n_new, int att, float* out, void* stream);
/* mf_nerf_feat_rows_load: a session joins, starts again or is reset.  For each of the n_rows named rows (HOST int array, as above) the ring row [R][dim]
 * is written from src_ring (device fp32 [R][dim]; NULL: zeros) and, when hist is not NULL, the history row [8][dim][16] from src_hist (NULL: zeros): the
 * state a warmed-up `NerfASR` holds, taken once, reaches any number of rows without running the net.  One launch per 64 rows, 16-byte accesses: R must be
 * a multiple of 4 (it is 4 * m) and every buffer 16-byte aligned.  A source may lie in the same allocation as the pool (a row that is never named) but
 * must not overlap a named row.  Refused with MF_ERR_INVALID before any launch: rings or rows NULL, src_hist without hist, dim / R / N outside the
 * ranges above, a row out of range or named twice, a misaligned buffer, an overlapping source. */
int mf_nerf_feat_rows_load(float* rings, float* hist, int N, int R, int dim, int n_rows, const int* rows, const float* src_ring,
                           const float* src_hist, void* stream);

/* ---- ER-NeRF head frame without host round trips ----------------------------------------------- */
typedef struct mf_nerf_head mf_nerf_head;
/* Scratch for up to max_rays rays over `field` (which must outlive the head and use the fused field kernel). */
int mf_nerf_head_create(mf_nerf_field* field, int max_rays, mf_nerf_head** out);
/* The inference branch of `NeRFRenderer.run_cuda` (renderer.py:231-291) for one frame, enqueued in one go: near/far,
 * up to max_steps rounds of (round control -> march_rays -> field -> composite_rays_triplane -> compaction) whose counters
 * (n_alive, n_step = max(min(N // n_alive, 8), 1), step) live on the device, then the background mix / depth
 * normalisation of :275-280.  No host synchronisation: the call only enqueues (capturable in a hipGraph).
 * Only the rounds the frames before needed (every round until a first frame has reported) go out as launches; ONE
 * further launch stands for the rest of the max_steps rounds and runs them itself if the loop has not ended by then
 * (mf_nerf_head_plan_rounds / _set_rounds below; MF_NERF_TAIL_AFTER=<k>|off overrides).
 * rays_o, rays_d [N,3]; density_bitfield [cascades * grid_size^3 / 8]; enc_a [32]; ind_code [individual_dim] or NULL;
 * bg as in mf_nerf_finish.  Outputs: image [N,3], depth [N], weights_sum [N] (optional), frame_u8 [N,3] (optional).
 * Survivors of a round keep no particular order (rays are independent), unlike the reference's boolean mask.
 * bg_per_ray < 0 leaves image / depth unfinished (no background mix, depth not normalised): the caller finishes with
 * mf_nerf_head_finish, e.g. after joining a stream on which the torso (mf_nerf_torso_forward) produced bg_color. */
int mf_nerf_head_render(mf_nerf_head* h, const float* rays_o, const float* rays_d, int n_rays, const uint8_t* density_bitfield, int cascades,
                        int grid_size, float min_near, float dt_gamma, int max_steps, float T_thresh, float density_scale, const float* enc_a,
                        const float* ind_code, float eye, const float* bg_color, int bg_per_ray, float bg_const, float* image, float* depth,
                        float* weights_sum, uint8_t* frame_u8, void* stream);
/* renderer.py:275-280 + nerfreal.py:111 for the frame a mf_nerf_head_render(bg_per_ray < 0) left unfinished; weights_sum may be
 * NULL when none was passed to the render call. */
int mf_nerf_head_finish(mf_nerf_head* h, int n_rays, const float* bg_color, int bg_per_ray, float bg_const, float* image, float* depth,
                        const float* weights_sum, uint8_t* frame_u8, void* stream);
/* The eye feature `e` of `NeRFNetwork.forward` (network.py:249, `data['eye']`: a [1, 1] device tensor in the reference's loader) read from DEVICE memory by every
 * later mf_nerf_head_render on `h` instead of its by-value `eye` argument: no host copy of a value that lives on the device, and a captured graph follows a changing
 * value.  NULL: back to the by-value argument.  The float must stay valid until the renders that use it have finished. */
int mf_nerf_head_set_eye(mf_nerf_head* h, const float* eye_dev);
/* `self.aabb_infer` (renderer.py:86-89, a persistent buffer a checkpoint may carry) read from DEVICE memory by every later mf_nerf_head_render on `h`
 * (near / far, raymarching.py:44) instead of the box the head derives from the field's bound: aabb_dev is device fp32 [6] (xmin, ymin, zmin, xmax, ymax,
 * zmax) and must stay valid until the renders that use it have finished.  NULL, or never called: the box from `bound`, as before. */
int mf_nerf_head_set_aabb(mf_nerf_head* h, const float* aabb_dev);
/* Rounds of a frame enqueued as (march, field, composite) launches before the tail launch.  _plan_rounds returns what the next mf_nerf_head_render would
 * choose from the round counts earlier frames posted (device -> pinned host word, read without a sync); _set_rounds(r >= 0) pins the count -- a caller that
 * captures the enqueue in a hipGraph pins what it keyed the graph on -- and _set_rounds(-1) returns to following the feedback.  _last_rounds: the round count
 * the most recently FINISHED frame posted (0 before the first), and the tail's error flag. */
int mf_nerf_head_plan_rounds(mf_nerf_head* h, int max_steps, int* rounds);
int mf_nerf_head_set_rounds(mf_nerf_head* h, int rounds);
int mf_nerf_head_last_rounds(mf_nerf_head* h, int* rounds, int* error_flag);
/* Diagnostics: the first n_ints words of the loop's control block (synchronous copy; layout in csrc/mf_nerf_march.h). */
int mf_nerf_head_ctl_snapshot(mf_nerf_head* h, int* out, int n_ints);
/* Diagnostics: the two per-round kernels of the loop, launched on the caller's device buffers instead of a handle's, so that a test can look at what they
 * write.  ctl_dev is a control block of at least 12 ints the caller has written (layout in csrc/mf_nerf_march.h): [0] n_alive, [1] n_step, [2] the step count
 * after this round, [3] n_alive * n_step, [6..7] and [10..11] zero, [8] the rounds so far.  Both calls copy its head back and check it before they launch (they
 * wait for `stream` once); the launch itself is only enqueued.
 * mf_nerf_loop_march_debug: the march of one round over blocks of 256 of the n_rays rays, as mf_march_rays with noises = 0 writes it -- and the slots a ray does
 * not reach zeroed; xyzs / dirs [n_alive * n_step, 3], deltas [n_alive * n_step, 2], nothing beyond.  variant 0: the kernel mf_nerf_head_render would pick
 * (the one-cascade kernel iff cascades == 1 and grid_size is a power of two up to 128), 1: the generic kernel, 2: the one-cascade kernel, MF_ERR_INVALID
 * where the rule does not allow it.  Refused too: what mf_march_rays refuses, n_alive > n_rays, n_step outside 1..8.
 * mf_nerf_loop_composite_debug: the tail of one round as mf_nerf_head_render launches it: the blend of mf_composite_rays_triplane, the survivors appended to
 * alive_out (at least n_alive ints; in no particular order), and the head of the next round written to ctl_dev[0..3], [6..8] for a frame of N rays. */
int mf_nerf_loop_march_debug(const int* ctl_dev, const int* rays_alive, const float* rays_t, const float* rays_o, const float* rays_d, uint32_t n_rays,
                             float bound, float dt_gamma, uint32_t max_steps, uint32_t cascades, uint32_t grid_size, const uint8_t* bitfield,
                             const float* fars, float* xyzs, float* dirs, float* deltas, int variant, void* stream);
int mf_nerf_loop_composite_debug(int* ctl_dev, int N, int max_steps, float T_thresh, const int* alive_in, int* alive_out, float* rays_t,
                                 const float* sigmas, const float* rgbs, const float* deltas, const float* ambs_aud, const float* ambs_eye,
                                 const float* uncertainties, float* weights_sum, float* depth, float* image, float* amb_aud_sum, float* amb_eye_sum,
                                 float* uncertainty_sum, void* stream);
/* The per-ray sums `run_cuda` also returns at inference (`results['ambient_aud' | 'ambient_eye' | 'uncertainty']`, renderer.py:286-288) of the LAST frame
 * rendered through `h`: device-to-device copies enqueued on `stream` behind that frame (any of the three may be NULL). */
int mf_nerf_head_sums(mf_nerf_head* h, int n_rays, float* ambient_aud, float* ambient_eye, float* uncertainty, void* stream);
void mf_nerf_head_destroy(mf_nerf_head* h);

/* ---- several head frames in one device loop ------------------------------------------------------------------
 * The F frames of a serving step (4 per session) rendered by ONE chain of launches: init, the rounds of (march, field, composite) and the finish carry a
 * frame index in the grid, so the chain's launch latency is paid once and the late rounds, which hold few rays per frame, are filled with other frames' rays.
 * Every frame keeps its own round control (n_alive, n_step, step: its own control block), so the per-ray and per-sample arithmetic is mf_nerf_head_render's:
 * a frame rendered in a batch is the same bits as the same frame rendered alone.
 * All frames of a call share the field, the bitfield, the ray count and the scalar render parameters; what a descriptor holds is per frame. */
typedef struct mf_nerf_frame_desc {
    const float *rays_o, *rays_d;      /* device, [n_rays, 3] */
    const float *enc_a, *ind_code;     /* device, [32] / [individual_dim] or NULL */
    const float* eye_dev;              /* device, the eye feature; NULL: `eye` below */
    float eye;
    const float* bg_color;             /* bg_color / bg_per_ray / bg_const as mf_nerf_head_render; bg_per_ray < 0: the frame is left unfinished */
    int bg_per_ray;
    float bg_const;
    float *image, *depth, *weights_sum;   /* outputs, device: [n_rays, 3], [n_rays], [n_rays] or NULL */
    uint8_t* frame_u8;                 /* [n_rays, 3] or NULL */
} mf_nerf_frame_desc;
typedef struct mf_nerf_head_batch mf_nerf_head_batch;
/* Scratch for up to max_frames (1..64) frames of up to max_rays rays over `field`.  The handle owns, per frame slot, what a mf_nerf_head owns for its one
 * frame: the per-ray and per-sample buffers, two alive lists, one control block and two pinned feedback words -- 96 bytes per ray and slot, 25 MB per
 * 512 x 512 slot (1.6 GB for 64 of them: size max_frames to the serving step) -- and a ring of four frame tables (pinned staging + device). */
int mf_nerf_head_batch_create(mf_nerf_field* field, int max_rays, int max_frames, mf_nerf_head_batch** out);
/* frames: HOST array of n_frames descriptors, read before the call returns; the table reaches the device by an asynchronous copy from pinned memory on
 * `stream` (no host synchronisation; a call waits only if the four calls before it are all still in flight).  aabb_dev: device fp32 [6] as
 * mf_nerf_head_set_aabb takes, or NULL for the box from the field's bound.  Frame i uses slot i.  Rounds enqueued as launches: the most any frame of the
 * batches observed so far needed (the slots' feedback words, read without a sync; every round until a first batch has reported; MF_NERF_TAIL_AFTER
 * overrides), then one tail launch per frame on that frame's control block, which in the usual case reads three words and leaves.  MF_NERF_MARCH and
 * MF_NERF_SKIP_EMPTY apply as in mf_nerf_head_render.  Not capturable in a hipGraph.
 * A slot whose tail kernel once gave up waiting (its error flag, see mf_nerf_head_batch_last_rounds) refuses every later call that uses the slot, i.e. every call
 * with n_frames above its index, before anything is launched; as with mf_nerf_head the flag is cleared only by a later frame of that slot, so the way out is to
 * destroy the handle and create a new one. */
int mf_nerf_head_batch_render(mf_nerf_head_batch* h, const mf_nerf_frame_desc* frames, int n_frames, int n_rays, const uint8_t* density_bitfield,
                              int cascades, int grid_size, float min_near, float dt_gamma, int max_steps, float T_thresh, float density_scale,
                              const float* aabb_dev, void* stream);
/* mf_nerf_head_finish for the frame rendered last in slot `frame` with bg_per_ray < 0. */
int mf_nerf_head_batch_finish(mf_nerf_head_batch* h, int frame, int n_rays, const float* bg_color, int bg_per_ray, float bg_const, float* image,
                              float* depth, const float* weights_sum, uint8_t* frame_u8, void* stream);
/* mf_nerf_head_sums for the frame rendered last in slot `frame`. */
int mf_nerf_head_batch_sums(mf_nerf_head_batch* h, int frame, int n_rays, float* ambient_aud, float* ambient_eye, float* uncertainty, void* stream);
/* rounds / error_flags: HOST int [max_frames] (either may be NULL): per slot, what mf_nerf_head_last_rounds reports for a head. */
int mf_nerf_head_batch_last_rounds(mf_nerf_head_batch* h, int* rounds, int* error_flags);
void mf_nerf_head_batch_destroy(mf_nerf_head_batch* h);

/* ---- ER-NeRF torso branch --------------------------------------------------------------------- */
typedef struct mf_nerf_torso mf_nerf_torso;
typedef struct mf_nerf_torso_config {
    float torso_shrink;          /* opt.torso_shrink, 0.8 (app.py:595) */
    int num_levels;              /* 16: tiled grid of network.py:158 */
    int level_dim;               /* 2 */
    int base_resolution;         /* 16 */
    float log2_per_level_scale;
    int offsets[33];             /* GridEncoder.offsets of torso_encoder */
    int individual_dim;          /* opt.ind_dim_torso, 8 */
    int grid_size;               /* 128: density_grid_torso is grid_size^2 (renderer.py:121) */
} mf_nerf_torso_config;
/* weights: "torso_deform_net.net.N.weight", "torso_net.net.N.weight", "torso_encoder.embeddings", "density_grid_torso". */
int mf_nerf_torso_create(const mf_nerf_torso_config* cfg, const mf_tensor* weights, int n_weights, int precision, int max_pixels,
                         mf_nerf_torso** out);
/* Replaces `run_torso` + `forward_torso` (renderer.py:294-352, network.py:166-201) for one frame.
 * bg_coords: device fp32 [N,2] in [-1,1]; frame_consts_host: HOST fp32 [42 + individual_dim] = FreqEncoder(6,3) of the
 * wrapped anchors (network.py:175-178) followed by the torso individual code; bg_color as in mf_nerf_finish;
 * density_thresh = min(opt.density_thresh_torso, mean_density_torso) (renderer.py:325).
 * bg_out: device fp32 [N,3] = torso_color * torso_alpha + bg * (1 - torso_alpha); torso_alpha [N] and deform [N,2] optional. */
int mf_nerf_torso_forward(mf_nerf_torso* h, const float* bg_coords, const float* frame_consts_host, const float* bg_color,
                          int bg_per_ray, float bg_const, float density_thresh, int n_pixels, float* bg_out, float* torso_alpha,
                          float* deform, void* stream);
/* The occupancy grid mf_nerf_torso_forward samples: `density_grid` (device fp32 [grid_size^2], row y, column x) is BORROWED, as
 * mf_nerf_head_render borrows the bitfield -- the reference rebinds `self.density_grid_torso` at every torso update
 * (renderer.py:527), so the caller hands over the tensor of the frame.  It must stay valid until the forwards that use it have
 * finished.  NULL: back to the copy of "density_grid_torso" taken at creation. */
int mf_nerf_torso_set_grid(mf_nerf_torso* h, const float* density_grid);
/* Replaces the torso branch of `NeRFRenderer.update_extra_state` (renderer.py:488-528) as three launches, no host
 * synchronisation: (a) one lane per cell (x, y): position = (2 c / (G - 1) - 1) * (1 - 1/G) + (2 u - 1) * (1/G) in the
 * reference's float32 statement order (:511-514), through the per-point arithmetic of mf_nerf_torso_forward (no occupancy mask,
 * no colour mix), alpha written to raw_grid[y G + x] (the reference transposes, :510); (b) 5 x 5 max of raw_grid (stride 1, the
 * border padded with -inf as max_pool2d pads) and grid = fmaxf(grid * decay, max) (:522-527); (c) mean = mean of grid (:528) as an
 * fp64 sum in a fixed order, rounded to fp32.
 * frame_consts_host as in mf_nerf_torso_forward (the pose and code row of :492-499); noise: device fp32 [G^2, 2], the
 * torch.rand values of :514 in meshgrid order (row x G + y), or NULL for cell centres; density_grid: device fp32 [G^2], in/out,
 * and the grid later forwards sample (as mf_nerf_torso_set_grid); raw_grid: fp32 [G^2], holds the sweep's (undilated) alpha
 * afterwards; xys_out: fp32 [G^2, 2] in meshgrid order, or NULL; mean: device fp32, 1 value.  G = the handle's grid_size: 32, 64 or
 * 128, else MF_ERR_INVALID with the limit named in mf_last_error.  Needs the fused torso kernel (not MF_TORSO=gemm). */
int mf_nerf_torso_grid_update(mf_nerf_torso* h, const float* frame_consts_host, const float* noise, float decay, float* density_grid,
                              float* raw_grid, float* xys_out, float* mean, void* stream);
void mf_nerf_torso_destroy(mf_nerf_torso* h);
/* mf_nerf_torso_forward for n_frames frames of n_pixels pixels in one launch, through the descriptor table of a mf_nerf_frame_batch (above): frame i
 * is the same bits as mf_nerf_torso_forward gives for descs[i] -- the first-layer biases are formed on the host the same way and travel in the table,
 * and a frame's pixels fill 256-pixel tiles of their own.  Every frame samples the grid bound by mf_nerf_torso_set_grid.  Needs the fused torso kernel
 * (MF_TORSO=gemm is refused). */
int mf_nerf_torso_forward_batch(mf_nerf_torso* torso, mf_nerf_frame_batch* h, const mf_nerf_torso_desc* descs, int n_frames, int n_pixels, void* stream);

/* ---- ER-NeRF audio features ------------------------------------------------------------------- */
typedef struct mf_audio_encoder mf_audio_encoder;
/* weights: "audio_net.*" and (use_att) "audio_att_net.*" of the NeRFNetwork state dict (network.py:9-66), fp32 host.  audio_in_dim (the
 * second dimension of audio_net.encoder_conv.0.weight) is 1..1024: esperanto 44, deepspeech 29, default 32, hubert 1024; anything wider is
 * refused.  Above 64 the first conv runs as a launch of its own into a buffer the handle owns, and the windows must be 16-byte aligned. */
int mf_audio_encoder_create(const mf_tensor* weights, int n_weights, int use_att, mf_audio_encoder** out);
/* Replaces `NeRFNetwork.encode_audio(a)` (network.py:222-237): auds device fp32 [n_windows, audio_in_dim, 16]
 * (8 windows with the attention net, 1 without) -> enc_a device fp32 [32]. */
int mf_audio_encoder_forward(mf_audio_encoder* h, const float* auds, int n_windows, float* enc_a, void* stream);
/* The same followed by the lip-smoothing step of `NeRFRenderer.run_cuda` (ernerf/nerf_triplane/renderer.py:190-194):
 * enc_a = 0.35 * prev_enc_a + (1 - 0.35) * encode_audio(a), in torch's fp32 evaluation order (bit-identical to the three torch launches it replaces).
 * prev_enc_a: device fp32 [32], the previous frame's smoothed features (may alias enc_a); null = no smoothing (first frame). */
int mf_audio_encoder_forward_smooth(mf_audio_encoder* h, const float* auds, int n_windows, const float* prev_enc_a, float* enc_a, void* stream);
void mf_audio_encoder_destroy(mf_audio_encoder* h);

/* ---- sd-vae encoder: avatar preparation -------------------------------------------------------- */
typedef struct mf_vae_encoder mf_vae_encoder;
/* Replaces `self.vae.encode(image).latent_dist` of musetalk/models/vae.py:84-94 (diffusers AutoencoderKL.encode: Encoder +
 * quant_conv; used once per avatar frame by mere_musetalk.py:175-188, 303-304).  cfg as for mf_vae_create (sample_size = the
 * LATENT grid, 32; the image is sample_size * 2^(n_blocks-1) = 256); weights: the `encoder.*` and `quant_conv.*` tensors. */
int mf_vae_encoder_create(const mf_vae_config* cfg, const mf_tensor* weights, int n_weights, int precision, int max_batch,
                          mf_vae_encoder** out);
/* Exactly one of image / image_u8_bgr: image = device fp32 [B,3,256,256], already normalised (the tensor vae.py:84 receives);
 * image_u8_bgr = device uint8 [B,256,256,3] BGR crops, preprocessed on the device as vae.py:52-82 does (RGB, / 255.,
 * half_mask: rows >= 128 zeroed, Normalize(.5, .5)).  moments: device fp32 [B, 2 * latent_channels, 32, 32] = (mean | logvar) of
 * `latent_dist`; `sample()` = mean + exp(0.5 * clamp(logvar, -30, 20)) * noise and the scaling factor stay with the caller. */
int mf_vae_encode(mf_vae_encoder* h, const float* image, const uint8_t* image_u8_bgr, int half_mask, float* moments, int batch,
                  void* stream);
int mf_vae_encoder_image_size(const mf_vae_encoder* h);
void mf_vae_encoder_destroy(mf_vae_encoder* h);

/* ---- per-batch glue of the MuseTalk loop ------------------------------------------------ */
/* musereal.py:92-97: `latent_batch = torch.cat([input_latent_list_cycle[__mirror_index(length, index + i)] ...])`.
 * pool: device fp32 [n_pool_rows][row_elems] (every session's cached latents, 8*32*32 = 8192 floats per row);
 * rows: HOST int[n], the pool row of each batch entry (mirror index + the session's offset); out: device fp32
 * [n][row_elems].  row_elems must be a multiple of 4. */
int mf_gather_rows_f32(const float* pool, int n_pool_rows, int64_t row_elems, const int* rows, int n, float* out, void* stream);

/* Audio2Feature.feature2chunks / get_sliced_feature (musetalk/whisper/audio2feature.py:16-45, called at museasr.py:27)
 * on the device: chunk i = feature rows [left_rows[i], left_rows[i] + rows_per_chunk), each clamped to [0, T-1]
 * (`min(length - 1, max(0, idx))`), concatenated.  feat: device fp32 [T][row_elems] (row_elems = 5 * 384 for
 * Whisper-tiny); left_rows: HOST int[n_chunks] = int(vid_idx * 50 / fps) - 2 * audio_feat_length[0]; out: device fp32
 * [n_chunks][rows_per_chunk][row_elems] == [n_chunks][50][384]. */
int mf_whisper_feature_chunks(const float* feat, int T, int row_elems, const int* left_rows, int rows_per_chunk, int n_chunks,
                              float* out, void* stream);

/* ---- paste-back of the generated face into the cached full frame --------------------------- */
/* One output frame.  Wav2Lip (lipreal.py:207-214): `combine_frame = deepcopy(frame_list_cycle[idx]);
 * res = cv2.resize(res_frame.astype(np.uint8), (x2 - x1, y2 - y1)); combine_frame[y1:y2, x1:x2] = res` -> mask == NULL.
 * MuseTalk (musereal.py:238-247 + musetalk/utils/blending.py:103-125): the same resize, then
 * `get_image_blending(ori_frame, res, bbox, mask, mask_crop_box)`: inside the crop box the frame becomes
 * cv2.blendLinear(crop with the face pasted in, crop, gray(mask) / 255, 1 - gray(mask) / 255). */
typedef struct mf_paste_job {
    int frame_index;          /* cached full frame this output starts from (frame_list_cycle[idx]) */
    int x1, y1, x2, y2;       /* face bbox, x / y order as blending.py:105 (lipreal.py's coords are (y1, y2, x1, x2): reorder) */
    int cx1, cy1, cx2, cy2;   /* MuseTalk: mask crop box (x_s, y_s, x_e, y_e), blending.py:106; ignored when mask == NULL */
    const uint8_t* mask;      /* device uint8 [cy2-cy1][cx2-cx1][3] BGR (mask_list_cycle[idx]), or NULL: rectangle copy */
} mf_paste_job;
/* res: device, n_jobs generated frames [res_h][res_w][3], uint8, or fp32 with res_is_f32 (Wav2Lip's pred * 255, truncated as
 * `astype(np.uint8)` does); frames: device uint8 [n_frames][H][W][3] BGR; jobs: HOST array; out: device uint8
 * [n_jobs][H][W][3].  Bit-exact with OpenCV's 8-bit INTER_LINEAR resize / BGR2GRAY / blendLinear (csrc/mf_blend.hip). */
int mf_paste_frames(const void* res, int res_is_f32, int res_h, int res_w, const uint8_t* frames, int n_frames, int H, int W,
                    const mf_paste_job* jobs, int n_jobs, uint8_t* out, void* stream);
/* cv2.resize(src, (dw, dh)) for uint8 [sh][sw][3] with the default INTER_LINEAR (lipreal.py:211, musereal.py:241). */
int mf_resize_linear_u8(const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw, void* stream);

/* ---- finished frames as planar YUV 4:2:0 (I420): what the encoder behind `VideoFrame` wants ---------- */
/* frames: device uint8 [n_frames][H][W][3], packed, rgb_order 0: BGR (mf_paste_frames' output), 1: RGB (mf_nerf_frame_out's);
 * out: device uint8 [n_frames][H * 3 / 2][W] -- per frame H rows of Y, then the H/2 x W/2 Cb plane as bytes, then Cr: the
 * array `VideoFrame.from_ndarray(a, format="yuv420p")` takes.  BT.601 studio swing in 16.16 fixed point, chroma from the
 * sum of each 2 x 2 block (csrc/mf_i420.hip states the integers; parity with libswscale is unpinned).  One launch for the
 * whole block: 8-pixel strips per thread when W % 8 == 0 and both pointers are 4-byte aligned, else 2 x 2 blocks with byte
 * accesses; the bytes are the same.  Refuses null pointers, n_frames < 1, non-positive or odd H / W and an rgb_order other
 * than 0 / 1 (MF_ERR_INVALID, the value named in mf_last_error) before anything is launched. */
int mf_frames_to_i420(const uint8_t* frames, int n_frames, int H, int W, int rgb_order, uint8_t* out, void* stream);
/* Finished frames from anywhere into chosen frames of one block (csrc/mf_frame_gather.hip): the idle and custom-video frames
 * a session shows while it listens (lipreal.py:198-205, musereal.py:229-236), delivered like the generated ones. */
typedef struct mf_frame_src {
    const uint8_t* frame;     /* device, contiguous uint8 [H][W][3]: a cached avatar frame, a frame of a custom cycle, ... */
    int dst;                  /* frame number inside `out` */
} mf_frame_src;
/* srcs: HOST array of n entries, read during the call only (the table travels in the launch arguments, 64 sources per
 * launch; a longer list goes out as several launches).  out: device uint8 [out_frames][H][W][3] (format 0: a copy; odd H and
 * W are fine) or [out_frames][H * 3 / 2][W] (format 1: the layout and the bytes of mf_frames_to_i420 for the same pixels,
 * rgb_order as there; H and W even).  Frames of `out` that no source names keep their bytes.  One path per call: 8-pixel
 * strips (format 1, W % 8 == 0) or 16-byte units (format 0, H * W * 3 % 4 == 0) when `out` and EVERY source are 4-byte
 * aligned, byte accesses otherwise; the bytes are the same.  Refuses null pointers, n < 1, out_frames < 1, non-positive H / W,
 * odd H / W in format 1, a format or rgb_order other than 0 / 1, a dst outside [0, out_frames), two sources with one dst and a
 * source that lies inside `out` (MF_ERR_INVALID, the value named in mf_last_error) before anything is launched. */
int mf_frames_gather(const mf_frame_src* srcs, int n, int H, int W, int format, int rgb_order, uint8_t* out, int out_frames, void* stream);

/* ---- ER-NeRF audio front-end: wav2vec2 / HuBERT CTC network ----------------------------------- */
/* Replaces `self.processor(frame, ...)` + `self.model(inputs.input_values)` of NerfASR.__frame_to_text (nerfasr.py:128-143):
 * transformers' Wav2Vec2FeatureExtractor normalisation, then Wav2Vec2ForCTC (`.logits`) or HubertModel (`.last_hidden_state`, out_hidden = 1)
 * -- feature extractor (conv -> LayerNorm -> GELU per layer, feat_extract_norm = "layer"), feature projection, weight-normed grouped
 * positional convolution, pre-LN ("do_stable_layer_norm") or post-LN transformer layers, final LayerNorm, lm_head.  Field names follow
 * transformers' Wav2Vec2Config; weights = the model's state dict ("wav2vec2." / "hubert." prefixes accepted, the positional conv as
 * `weight`, `weight_g` / `weight_v` or `parametrizations.weight.original0 / 1`).  (ABI version 3) */
typedef struct mf_wav2vec2 mf_wav2vec2;
typedef struct {
    int hidden, n_layer, n_head, ffn, vocab;            /* hidden_size, num_hidden_layers, num_attention_heads, intermediate_size, vocab_size */
    int n_conv, conv_dim[8], conv_kernel[8], conv_stride[8], conv_bias;
    int feat_norm_layer;                                /* 1: feat_extract_norm == "layer" (required) */
    int stable_ln;                                      /* do_stable_layer_norm */
    int pos_k, pos_groups;                              /* num_conv_pos_embeddings, num_conv_pos_embedding_groups */
    float layer_norm_eps;
    int do_normalize;                                   /* the processor's zero-mean / unit-variance step */
    int out_hidden;                                     /* 0: logits [T][vocab]; 1: the final hidden state [T][hidden] */
} mf_wav2vec2_config;
/* One handle serves windows of exactly n_samples samples (NerfASR feeds (l + m + r) * 320 every step), up to max_windows per call. */
int mf_wav2vec2_create(const mf_wav2vec2_config* cfg, const mf_tensor* weights, int n_weights, int n_samples, int max_windows, int precision,
                       mf_wav2vec2** out);
/* frames per window (20 ms each) and the width of an output row */
int mf_wav2vec2_frames(const mf_wav2vec2* h, int* n_frames, int* width);
/* wav: device fp32 [n_windows][n_samples] (raw samples: the normalisation happens here); out: device fp32 [n_windows][n_frames][width]. */
int mf_wav2vec2_forward(mf_wav2vec2* h, const float* wav, int n_samples, int n_windows, float* out, void* stream);
void mf_wav2vec2_destroy(mf_wav2vec2* h);

/* ---- avatar preparation: static CNN graphs --------------------------------------------------------- */
/* The S3FD face detector (`s3fd.forward`, face_detection/detection/sfd/net_s3fd.py:72-129; called through `detect` / `batch_detect`,
 * sfd/detect.py:19-92, from genavatar.py:61-99 and musetalk/utils/preprocessing.py:63,104) and the BiSeNet face parser (`BiSeNet.forward`,
 * musetalk/utils/face_parsing/model.py:245-262 over resnet.py:60-95; called at face_parsing/__init__.py:51) are plain Python module trees
 * in the reference.  The drop-in modules (mere-fusion_amd/avatar/) walk the same trees and emit one op per module through this builder; all
 * arithmetic runs in the library.  Buffers are padded NHWC (hi, lo) planes; `coff` arguments select channel slices (torch.cat = two
 * producers writing slices of one buffer).  Build: mf_net_create, mf_net_buffer (returns a buffer id >= 0), ops in execution order.
 * Run: mf_net_set_input -> mf_net_run (captured into a hipGraph per batch size) -> mf_net_get_output*.  (ABI version 3) */
typedef struct mf_net mf_net;
int mf_net_create(int max_batch, int precision, mf_net** out);
int mf_net_buffer(mf_net* h, int C, int H, int W, int halo);
/* nn.Conv2d (+ eval-mode BatchNorm2d folded when bn_* are given, + residual, + d->act) on the MFMA kernels; in_h / in_w of `d` are taken from
 * the input buffer; bias may be NULL; res_buf < 0: no residual. */
int mf_net_conv(mf_net* h, const mf_conv2d_desc* d, const float* weight, const float* bias, const float* bn_gamma, const float* bn_beta,
                const float* bn_mean, const float* bn_var, int in_buf, int in_coff, int out_buf, int out_coff, int res_buf, int res_coff,
                const char* name);
int mf_net_maxpool(mf_net* h, int in_buf, int out_buf, int k, int stride, int pad);                       /* F.max_pool2d / nn.MaxPool2d */
int mf_net_l2norm(mf_net* h, int in_buf, int out_buf, const float* weight, int C, float eps);            /* L2Norm, net_s3fd.py:6-19 */
int mf_net_global_avgpool(mf_net* h, int in_buf, int in_coff, int C, int out_buf);                       /* F.avg_pool2d(x, x.size()[2:]) -> 1x1 map */
/* out = x * s[b][c] + t + v[b][c]: s, v are 1x1 maps (channel attention `torch.mul(feat, atten)`, the nearest-upsampled global feature of
 * model.py:103-107), t a map of x's size (`feat_atten + feat`, `feat16_arm + feat32_up`); any of s_buf / t_buf / v_buf may be < 0 */
int mf_net_scale_add(mf_net* h, int x_buf, int x_coff, int C, int s_buf, int t_buf, int t_coff, int v_buf, int out_buf, int out_coff);
int mf_net_upsample_nearest(mf_net* h, int in_buf, int out_buf);                                         /* F.interpolate(x, size, mode='nearest') */
int mf_net_num_ops(const mf_net* h);
double mf_net_flops_per_item(const mf_net* h);                                                           /* 2 x MACs of the convolutions, one batch item */
int mf_net_set_input(mf_net* h, int buf, const float* nchw, int C, int batch, void* stream);             /* device fp32 [batch][C][H][W] */
int mf_net_run(mf_net* h, int batch, void* stream);
int mf_net_tune(mf_net* h, int batch, void* stream);                                                     /* explicit launch-configuration warm-up: see mf_wav2lip_tune */
int mf_net_get_output(mf_net* h, int buf, int coff, int C, float* nchw, int batch, void* stream);        /* device fp32 [batch][C][H][W] */
/* F.interpolate(x, (H, W), mode='bilinear', align_corners=True) of a channel slice -> device fp32 [batch][C][H][W] (model.py:257-259) */
int mf_net_get_output_bilinear(mf_net* h, int buf, int coff, int C, float* nchw, int H, int W, int batch, void* stream);
/* "max-out background label" of net_s3fd.py:123-126: device fp32 [batch][4][hw] -> [batch][2][hw] = (max(c0, c1, c2), c3) */
int mf_s3fd_maxout_bg(const float* cls4, float* cls2, int batch, int hw, void* stream);
/* uint8 [batch][H][W][3] device frames -> an input buffer of 3 channels: channel c = (float)img[..][reverse_channels ? 2 - c : c] - mean3[c] (host floats).  The
 * `imgs - np.array([104, 117, 123])` of sfd/detect.py:59-60 and the `images[..., ::-1]` of face_detection/api.py:65 in one pass; bit-equal to mf_net_set_input of the
 * same values as fp32 (they are exact integers). */
int mf_net_set_input_u8(mf_net* h, int buf, const uint8_t* u8_nhwc, const float* mean3, int reverse_channels, int batch, void* stream);
/* Served uint8 frames -> an input buffer of 3 * T channels in one launch (csrc/mf_sync.hip): frames is device uint8 [n_frames][H][W][3], starts a HOST array of
 * n_windows first frames; batch slot w, channel 3 * t + c, row y, column x = (float)frames[starts[w] + t][row0 + y][x][c] / 255.f.  The buffer must be rows x W with
 * 3 * T channels.  SyncNet's face windows are T = 5, row0 = H / 2, rows = H / 2 (5 BGR frames on the channel axis, / 255., lower half: upstream Wav2Lip's
 * color_syncnet_train.py).  Bit-equal to mf_net_set_input of the same values as fp32.  Windows may overlap; the frames are read in place.  MF_ERR_INVALID, before any
 * launch, when starts[w] < 0 or starts[w] + T > n_frames, row0 + rows > H, n_windows exceeds the net's capacity, or the buffer's channels or size do not match. */
int mf_net_set_input_u8_windows(mf_net* h, int buf, const uint8_t* frames, int n_frames, int H, int W, const int* starts, int n_windows, int T, int row0, int rows,
                                void* stream);
/* Banded audio / video similarity of two embedding sequences and its reduction (csrc/mf_sync.hip).  face_emb, audio_emb: device fp32 [W][dim], raw or normalised;
 * sim: device fp32 [W][2 S + 1], sim[w][s] = <f_w, a_j> / (max(|f_w|, 1e-12) * max(|a_j|, 1e-12)) with j = w + s - S (a positive shift: the audio window is later than
 * the video window; an all-zero row gives 0), 0 where j is outside [0, W); counts: device int [2 S + 1], the valid windows per shift; curve: device fp32 [2 S + 1], the
 * mean of the valid entries (0 where counts is 0), summed in a fixed order: two runs give the same bits.  dim % 4 == 0, 4 <= dim <= 1024, 0 <= S <= 64, W >= 1. */
int mf_sync_score(const float* face_emb, const float* audio_emb, int W, int dim, int max_shift, float* sim, float* curve, int* counts, void* stream);
/* S3FD's post-process on the device (sfd/detect.py:58-94 batch_detect, bbox.py:111-129 batch_decode, bbox.py:44-64 nms, sfd_detector.py:41-47): after mf_net_run,
 * reads the six 8-channel head buffers (conf in channels 0..3, loc in 4..7; level 1's max-out background fused) in place.  Per image: candidates with softmax face
 * probability > cand_thresh are decoded and appended (at most max_candidates <= 4096 stored; n_candidates[b] counts them all, so n_candidates[b] > max_candidates
 * reports an overflow), sorted by (score descending, (level, row, column) ascending), greedy NMS with `ovr > nms_thresh` suppression, and the kept boxes with score >
 * final_thresh written in keep order as boxes[b][i] = (x1, y1, x2, y2, score), i < min(counts[b], max_det); counts[b] counts every kept box.  The reference's values are
 * 0.05 / 0.3 / 0.5; cand_thresh = final_thresh gives the identical boxes from shorter lists (mf_s3fd_detect.hip says why).  boxes: device fp32 [batch][max_det][5];
 * counts, n_candidates: device int32 [batch].  Nothing synchronises with the host. */
int mf_s3fd_detect(mf_net* net, const int* head_bufs, int batch, float cand_thresh, float nms_thresh, float final_thresh, int max_candidates, int max_det, float* boxes,
                   int* counts, int* n_candidates, void* stream);
/* The same on the twelve tensors s3fd.__call__ returns: heads[2 * l] = cls [batch][2][h][w] (level 1 already maxed out), heads[2 * l + 1] = reg [batch][4][h][w], device
 * fp32; map_hw[2 * l], map_hw[2 * l + 1] = h, w of level l + 1 (host).  workspace: device memory of mf_s3fd_detect_workspace_bytes(batch, max_candidates) bytes. */
int mf_s3fd_detect_tensors(const float* const* heads, const int* map_hw, int batch, float cand_thresh, float nms_thresh, float final_thresh, int max_candidates, int max_det,
                           void* workspace, float* boxes, int* counts, int* n_candidates, void* stream);
size_t mf_s3fd_detect_workspace_bytes(int batch, int max_candidates);
/* MuseTalk's blend masks on the device (mf_face_mask.hip): what FaceParsing.__call__ (face_parsing/__init__.py:34-51), face_seg and get_image_prepare_material
 * (musetalk/utils/blending.py:17-24, 62-86) do on the host around the BiSeNet graph.  Nothing synchronises with the host; a geometry the kernels cannot serve is
 * MF_ERR_INVALID with the limit named in mf_last_error (more than 64 resampling taps per pixel: for mf_face_mask_finish a crop under 34 pixels from a 512 x 512 mask, which mf_face_mask_parse still serves; a blur wider than 151 taps: a crop over 1519 pixels); there is no fallback.
 *
 * mf_face_mask_parse: jobs[i] = (frame index, x_s, y_s, x_e, y_e) (host int32 [n_jobs][5]): the crop box of a uint8 [n_frames][H][W][3] device frame, black outside
 * the frame like Image.crop, channels reversed when reverse_channels (`image[:, :, ::-1]`), is resized to the input buffer's size exactly as Pillow's
 * Image.resize(size, BILINEAR) does for 8-bit pixels and written into batch slot i of in_buf as ((float)u8 / 255.f - mean3[c]) / std3[c] (bit-equal to mf_net_set_input
 * of those floats); the graph runs at batch n_jobs <= its capacity; masks[i] (device uint8 [n_jobs][in_h][in_w]) = 255 where the argmax over the n_classes channels of
 * head_buf, upsampled as mf_net_get_output_bilinear does, is a class in 1..13 (first maximum wins), else 0.
 *
 * mf_face_mask_finish: jobs[i] = (w, h, rx0, ry0, rx1, ry1, top) (host int32 [n_jobs][7]): masks[i] (device uint8 [n_jobs][mask_h][mask_w]) is resized to w x h as
 * Image.resize(size) does for mode L (BICUBIC), zeroed outside the rectangle [rx0, rx1) x [ry0, ry1) and above row `top` (blending.py:74-82) -> pre_blur (optional),
 * then blurred as cv2.GaussianBlur(., (k, k), 0), k = int(0.1 * w // 2 * 2) + 1, is defined (float64 taps, fp32 passes, one rounding) -> out.  Both outputs are packed:
 * job i starts at the sum of w * h of the jobs before it.  blur = 0 stops at pre_blur (face_seg alone: the whole crop as rectangle, top = 0).
 *
 * workspace: device memory of mf_face_mask_workspace_bytes(finish, box_sizes, n_jobs, mask_h, mask_w) bytes, box_sizes = host int32 [n_jobs][2] (w, h) of the crop
 * boxes, mask_h x mask_w = the size of the parser's input; 0 for a geometry that is refused. */
size_t mf_face_mask_workspace_bytes(int finish, const int* box_sizes, int n_jobs, int mask_h, int mask_w);
int mf_face_mask_parse(mf_net* net, int in_buf, int head_buf, int n_classes, const uint8_t* frames, int n_frames, int H, int W, int reverse_channels, const int* jobs,
                       int n_jobs, const float* mean3, const float* std3, void* workspace, size_t workspace_bytes, uint8_t* masks, void* stream);
int mf_face_mask_finish(const uint8_t* masks, int mask_h, int mask_w, const int* jobs, int n_jobs, int blur, void* workspace, size_t workspace_bytes, uint8_t* pre_blur,
                        uint8_t* out, void* stream);
void mf_net_destroy(mf_net* h);

/* ---- DWPose landmark network (mf_dwpose_ops.hip, mf_rtmcc_head.hip, mf_dwpose.hip): mmdet CSPNeXt + mmpose RTMCCHead + SimCC, and the landmark box of
 * musetalk/utils/preprocessing.py:96-131.  Two more ops of the mf_net builder, then free functions that read / fill a net's buffers in place. */
/* depthwise k x k conv (k 3 or 5, stride 1 or 2, pad k / 2) + eval BatchNorm (all four vectors or none; eps = bn_eps) + act (0 none, 1 ReLU, 4 SiLU) on C channels at
 * in_coff of in_buf -> C channels at out_coff of out_buf.  weight: host fp32 [C][1][k][k]; bias may be null. */
int mf_net_dwconv(mf_net* h, int C, int k, int stride, int act, const float* weight, const float* bias, const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                  const float* bn_var, float bn_eps, int in_buf, int in_coff, int out_buf, int out_coff);
/* mmdet ChannelAttention after its average pool: out = x * hardsigmoid(fc(pooled)); pooled_buf: a 1x1 map (mf_net_global_avgpool); fc_weight host fp32 [C][C], fc_bias [C] */
int mf_net_chan_attn(mf_net* h, int x_buf, int x_coff, int C, int pooled_buf, const float* fc_weight, const float* fc_bias, int out_buf, int out_coff);
/* RTMCCHead behind its final conv.  Weights: host fp32 in torch layout ([out][in]); mlp_g / ln_g: the ScaleNorm scalars; expansion factor 2.  forward reads `tokens` maps
 * of `flat` = H * W values at channel coff of net buffer buf (after mf_net_run) and writes device fp32 logits_x [batch][tokens][bins_x], logits_y [batch][tokens][bins_y].
 * The intermediate workspace belongs to the handle: forwards of one handle must be ordered on one stream (two streams would race on it); use one handle per stream. */
typedef struct mf_rtmcc_head mf_rtmcc_head;
int mf_rtmcc_head_create(int tokens, int flat, int hidden, int s, int bins_x, int bins_y, const float* mlp_g, const float* mlp_w, const float* ln_g, const float* uv_w,
                         const float* gamma, const float* beta, const float* o_w, const float* res_scale, const float* cls_x_w, const float* cls_y_w, int max_batch,
                         mf_rtmcc_head** out);
int mf_rtmcc_head_forward(mf_rtmcc_head* h, mf_net* net, int buf, int coff, int batch, float* logits_x, float* logits_y, void* stream);
void mf_rtmcc_head_destroy(mf_rtmcc_head* h);
/* SimCC decode on the device, no host sync: with flip_x / flip_y (the logits of the mirrored images; flip_pairs: HOST int [keypoints], the dataset's flip_indices) the
 * two passes are averaged first (simcc_x's bin axis reversed, keypoints swapped).  argmax per axis (first maximum), score = the smaller maximum, location -1 where
 * score <= 0, / 2, then keypoints / (in_w, in_h) * scale + center - scale / 2 in fp32, one rounding per operation.  center, scale: host float [2].
 * kpts: device fp32 [batch][keypoints][2]; scores: device fp32 [batch][keypoints]. */
int mf_simcc_decode(const float* logits_x, const float* logits_y, const float* flip_x, const float* flip_y, const int* flip_pairs, int batch, int keypoints, int bins_x,
                    int bins_y, int in_w, int in_h, const float* center, const float* scale, float* kpts, float* scores, void* stream);
/* cv2.warpAffine(INTER_LINEAR, constant 0 border) as an integer model + channel reversal + (x - mean3[c]) / std3[c] into batch slot j of the 3-channel
 * input buffer `buf`, and with flip != 0 the mirrored image into slot n + j.  frames: device uint8 [n][H][W][3]; minv: device float64 [n][6], the input -> source map. */
int mf_warp_affine_u8(mf_net* net, int buf, const uint8_t* frames, int n, int H, int W, const double* minv, const float* mean3, const float* std3, int reverse_channels,
                      int flip, void* stream);
/* preprocessing.py:100-101, 113-131 in integer arithmetic.  kpts: device fp32 [n][keypoints][2] (keypoints >= 91: the face is [23, 91)); boxes / counts: the outputs of
 * mf_s3fd_detect.  coords: device int32 [n][4] (x1, y1, x2, y2); flags: device int32 [n]: 0 no face (coords 0), 1 landmark box, 2 detector's box (clipped to the frame);
 * range_sums: device int32 [3]: sum of range_minus, sum of range_plus, frames counted. */
int mf_muse_landmark_boxes(const float* kpts, int keypoints, const float* boxes, const int* counts, int n, int max_det, int H, int W, int bbox_shift, int* coords, int* flags,
                           int* range_sums, void* stream);

/* ---- avatar preparation: boxes and crops (mf_crop_resize.hip) ------------------------------------------------------------ */
/* The steps between the detector and the generators that wav2lip/genavatar.py:80-96,119 and musetalk/mere_musetalk.py:293-296 do with numpy and cv2.  Nothing here
 * synchronises with the host.  (ABI version 4: additions only) */
typedef struct mf_crop_job {
    int frame_index;
    int x1, y1, x2, y2;                                 /* the crop frames[frame_index][y1:y2, x1:x2] */
} mf_crop_job;
/* genavatar.py:80-96 on what the detector left on the device: boxes device fp32 [n][max_det][5] and counts device int32 [n] as written by the detect entry points
 * above.  Per frame the first kept box is clipped at 0 and truncated to int (face_detection/api.py:64-79), padded by pads = (top, bottom, left, right) (host int32 [4])
 * and clamped to the H x W frame; then, unless smooth_T is 0 (`nosmooth`), get_smoothened_boxes(boxes, smooth_T) exactly as written: in place, sequential, Python's
 * slice of a negative start when n < smooth_T, means as truncated integer quotients (the reference passes T = 5).  coords: device int32 [n][4] in the reference's
 * (y1, y2, x1, x2) order; jobs: device mf_crop_job [n] (frame_index = i) for the resampler below; n_no_face: device int32, 1 value, the number of frames with
 * counts < 1 (their raw box is (0, 0, 0, 0); the reference raises on the first of them). */
int mf_avatar_lip_boxes(const float* boxes, const int* counts, int n, int max_det, int H, int W, const int* pads, int smooth_T, int* coords, mf_crop_job* jobs,
                        int* n_no_face, void* stream);
/* Batched crop + resample: dst[i] (device uint8 [n_jobs][dh][dw][3]) = the crop of jobs[i] out of frames (device uint8 [n_frames][H][W][3]) resized to dw x dh.
 * jobs is DEVICE memory.  jobs_host, when not NULL, is the host's copy of the same table: every job is checked before anything is launched (frame index in range,
 * crop not empty, crop inside the frame; MF_ERR_INVALID names the job).  With jobs_host NULL (a table the device wrote and the host never saw) the kernel makes the
 * same checks and zero-fills the destination of a job that fails them.  n_frames * H * W * 3 must stay below 2^31.
 * MF_CROP_LINEAR: cv::resize INTER_LINEAR for 8UC3 as the paste entry point above defines it, the coefficients formed in the kernel from each job's box; a crop of
 * exactly 2 dw x 2 dh takes INTER_AREA's fast path, decided per job.  The four table arguments are ignored.
 * MF_CROP_LANCZOS4: 8-tap separable integer resampler on per-job device tables xofs int32 [n_jobs][dw], xcoef int16 [n_jobs][dw][8], yofs int32 [n_jobs][dh],
 * ycoef int16 [n_jobs][dh][8] (coefficients scaled by 2048): tap k of destination column d reads crop column clamp(xofs[d] + k, 0, crop width - 1), the same for
 * rows; horizontal sums int32 without a shift; vertical sums int32 (wrapping), then (sum + (1 << 21)) >> 22 saturated to 0..255. */
enum { MF_CROP_LINEAR = 0, MF_CROP_LANCZOS4 = 1 };
int mf_crop_resize_u8(const uint8_t* frames, int n_frames, int H, int W, const mf_crop_job* jobs, const mf_crop_job* jobs_host, int n_jobs, uint8_t* dst, int dh,
                      int dw, int mode, const int* xofs, const int16_t* xcoef, const int* yofs, const int16_t* ycoef, void* stream);

/* ---- measurement seam --------------------------------------------------------------------------------------------- */
/* TFLOP/s of the convolution's own arithmetic that a kernel issuing NOTHING but matrix instructions sustains on this device (random operand bits, 8
 * waves per CU) for the instruction mix one product costs: mix 0 = bf16x3 as shipped (3 bf16 MFMAs), 1 = f16 + two FP8 block-scaled correction
 * terms, 2 = f16 + two FP6 ones.  bench.py reports it beside the nominal peak.  (ABI version 3)
 * mix 3 / 4 = mix 2 / 0 with operand VALUES drawn the way the layers' are (activations silu(z), z ~ N(0, 1); He-initialised weights) and split by the packers'
 * own rules: the ceiling is data dependent (the chip clocks to its power budget), random bits are the pessimistic end. */
int mf_probe_mfma_ceiling(int mix, float* tflops_algorithmic);

/* ---- frame transport ----------------------------------------------------------------------- */
/* Host-side plumbing of the shared-memory frame ring that replaces the pickled `res_frame_queue` items of
 * lipreal.py:136,161 / musereal.py:116,153 (mere-fusion_amd/transport.py keeps the (res_frame, idx, audio_frames) tuple
 * contract).  mf_host_register page-locks a host range (the ring's shared-memory block) once, so that
 * mf_copy_d2h_async of a batch of frames is one asynchronous DMA into the slot the consumer reads;
 * mf_stream_synchronize is the fence before the slot is published. */
int mf_host_register(void* host, size_t bytes);
int mf_host_unregister(void* host);
int mf_copy_d2h_async(const void* dev, void* host, size_t bytes, void* stream);
/* `rows` pieces of width_bytes each: dense on the device (dev_pitch apart), one ring slot apart on the host (host_pitch): a batch of
 * frames into consecutive slots as one DMA. */
int mf_copy_d2h_2d_async(const void* dev, size_t dev_pitch, void* host, size_t host_pitch, size_t width_bytes, size_t rows, void* stream);
int mf_stream_synchronize(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MEREFUSION_H */
