// Whisper's text decoder on gfx950: teacher-forced logits, prefill and greedy decoding with the token choice on the device
// (musetalk/whisper/whisper/model.py:57-128, 174-217; the greedy rule of decoding.py: suppression mask, argmax, summed log-probabilities).
//
// Decoding is one token per sequence per step: every Linear is a GEMV over at most 8 rows, bound by the bytes of its weights.  All launches
// take a list of ROWS, each row one token of one sequence at one cache position; a decode step is `batch` rows, a prompt is all its tokens at
// once (the causal mask is "row at position p reads cache rows 0..p"), so prefill and step run the SAME kernels and the same per-row arithmetic.
//   k_dec_embed    token embedding + learned positional embedding
//   k_dec_linear   [LayerNorm ->] x W^T [+ bias] [-> GELU | += residual | -> q and the K / V cache rows]: weights as bf16 (hi, lo) planes read
//                  16 bytes per lane, 16 lanes per output column, up to 8 rows per pass held in LDS, fp32 accumulation, wave shuffles to reduce
//   k_dec_attn     one query against the cached keys of its sequence (self: 0..position, cross: the T_audio encoder keys), softmax in fp32
//   k_dec_choose   suppression mask, argmax (lowest index wins a tie), log-probability, end-of-text / budget / cache-full -> done flag
//   k_dec_choose_rules   the same choice under the reference's logit filters (decoding.py:387-441: SuppressBlank, SuppressTokens,
//                  ApplyTimestampRules), read from the sequence's own history on the device; takes k_dec_choose's place in a step, launch for launch
// A step is 2 + 8 * n_layer launches and depends on no host read: a sequence whose done flag is set is skipped by every kernel (its cache rows,
// its output and its counters are not written again), so the host reads the flags only every `check_every` steps.
#include "mf_common.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {

constexpr int DH = 64;                 // head width of every published Whisper size
constexpr int N_AUDIO_CTX = 1500;      // encoder tokens of one 30 s segment
constexpr int LIN_THREADS = 256, LIN_COLS = 16, LIN_KSTEP = 128;   // 16 lanes x 8 bf16 per output column and pass over K
constexpr int MAX_DEC_BATCH = 8;

enum { OUT_STORE = 0, OUT_GELU = 1, OUT_ADD = 2, OUT_QKV = 3 };

// which token of which sequence a row is.  seq == null: row m is sequence m; pos == null: the row sits at its sequence's current length
struct Rows {
    const int* seq;
    const int* pos;
    const int* len;    // [batch] cache rows filled so far
    const int* done;   // [batch] or null (teacher-forced calls)
};
__device__ __forceinline__ int row_seq(const Rows& r, int m) { return r.seq ? r.seq[m] : m; }
__device__ __forceinline__ int row_pos(const Rows& r, int m) { return r.pos ? r.pos[m] : r.len[row_seq(r, m)]; }
__device__ __forceinline__ bool row_idle(const Rows& r, int m) { return r.done && r.done[row_seq(r, m)] != 0; }

__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ float round_bf16(float v) { return bf_lo(mf_bf16_rne(v)); }
__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(128) void k_dec_embed(const int* __restrict__ tokens, const bf16_t* __restrict__ emb_hi, const bf16_t* __restrict__ emb_lo,
                                                   const float* __restrict__ pos_emb, float* __restrict__ x, int C, int n_vocab, Rows rows) {
    const int m = blockIdx.x;
    if (row_idle(rows, m)) return;
    const int tok = min(max(tokens[m], 0), n_vocab - 1), p = row_pos(rows, m);
    const bf16_t* hi = emb_hi + (int64_t)tok * C;
    const bf16_t* lo = emb_lo + (int64_t)tok * C;
    for (int c = threadIdx.x; c < C; c += 128)
        x[(int64_t)m * C + c] = (bf_lo(hi[c]) + bf_lo(lo[c])) + pos_emb[(int64_t)p * C + c];
}

struct LinArgs {
    const float* x; int x_stride; const int* gather;      // input row m = x + (gather ? gather[m] : m) * x_stride, K values
    const float* ln_g; const float* ln_b;                 // LayerNorm over the K inputs first (null: none)
    const bf16_t* w_hi; const bf16_t* w_lo; const float* bias;   // W [N][K] as bf16 planes; bias [N] or null
    int M, N, K, cols_per_block, mode;
    float* out; int out_stride;
    float* kcache; float* vcache; int64_t cache_seq_stride; int C;   // OUT_QKV: columns [C, 2C) and [2C, 3C) go to the cache row of the token
    Rows rows;
};

// R rows of x (normalised, and rounded to bf16 in the single-plane mode) wait in LDS; each group of 16 lanes owns one output column and walks its
// weight row 128 elements a pass, 16 bytes a lane and plane; hi + lo is exact in fp32, so bf16x3 here is an fp32 product with a 16-bit weight
template <int R, bool X3>
__global__ __launch_bounds__(LIN_THREADS) void k_dec_linear(LinArgs a) {
    extern __shared__ float s_x[];   // [R][K]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * R, K = a.K;
    for (int r = wave; r < R; r += LIN_THREADS / 64) {
        float* dst = s_x + r * K;
        const int m = m0 + r;
        if (m >= a.M) {
            for (int k = lane; k < K; k += 64) dst[k] = 0.f;
            continue;
        }
        const float* src = a.x + (int64_t)(a.gather ? a.gather[m] : m) * a.x_stride;
        float mean = 0.f, rstd = 1.f;
        if (a.ln_g) {
            float s = 0.f;
            for (int k = lane; k < K; k += 64) s += src[k];
            mean = wave_sum(s) / (float)K;
            float q = 0.f;
            for (int k = lane; k < K; k += 64) { const float d = src[k] - mean; q = fmaf(d, d, q); }
            rstd = 1.0f / sqrtf(wave_sum(q) / (float)K + 1e-5f);
        }
        for (int k = lane; k < K; k += 64) {
            float v = src[k];
            if (a.ln_g) v = fmaf((v - mean) * rstd, a.ln_g[k], a.ln_b[k]);
            dst[k] = X3 ? v : round_bf16(v);
        }
    }
    __syncthreads();
    const int g = tid >> 4, gl = tid & 15;
    const int c_end = min(a.N, (int)(blockIdx.x + 1) * a.cols_per_block);
    for (int c0 = blockIdx.x * a.cols_per_block; c0 < c_end; c0 += LIN_COLS) {
        const int n = c0 + g;
        const bool valid = n < a.N;
        const int64_t wrow = (int64_t)(valid ? n : a.N - 1) * K;
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
        for (int k0 = gl * 8; k0 < K; k0 += LIN_KSTEP) {
            const uint4 h = *reinterpret_cast<const uint4*>(a.w_hi + wrow + k0);
            float w[8] = {bf_lo(h.x), bf_hi(h.x), bf_lo(h.y), bf_hi(h.y), bf_lo(h.z), bf_hi(h.z), bf_lo(h.w), bf_hi(h.w)};
            if (X3) {
                const uint4 l = *reinterpret_cast<const uint4*>(a.w_lo + wrow + k0);
                // mf_opaque: the two halves of one loaded word must not meet in one packed add (the gfx950 erratum form, mf_common.h)
                w[0] += mf_opaque(bf_lo(l.x)); w[1] += mf_opaque(bf_hi(l.x)); w[2] += mf_opaque(bf_lo(l.y)); w[3] += mf_opaque(bf_hi(l.y));
                w[4] += mf_opaque(bf_lo(l.z)); w[5] += mf_opaque(bf_hi(l.z)); w[6] += mf_opaque(bf_lo(l.w)); w[7] += mf_opaque(bf_hi(l.w));
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float4 x0 = *reinterpret_cast<const float4*>(s_x + r * K + k0);
                const float4 x1 = *reinterpret_cast<const float4*>(s_x + r * K + k0 + 4);
                float s = acc[r];
                s = fmaf(w[0], x0.x, s); s = fmaf(w[1], x0.y, s); s = fmaf(w[2], x0.z, s); s = fmaf(w[3], x0.w, s);
                s = fmaf(w[4], x1.x, s); s = fmaf(w[5], x1.y, s); s = fmaf(w[6], x1.z, s); s = fmaf(w[7], x1.w, s);
                acc[r] = s;
            }
        }
        float mine = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float v = acc[r];
            for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (gl == r) mine = v;
        }
        const int m = m0 + gl;
        if (gl < R && valid && m < a.M && !row_idle(a.rows, m)) {
            float v = mine + (a.bias ? a.bias[n] : 0.f);
            if (a.mode == OUT_QKV && n >= a.C) {
                float* cache = n < 2 * a.C ? a.kcache : a.vcache;
                cache[(int64_t)row_seq(a.rows, m) * a.cache_seq_stride + (int64_t)row_pos(a.rows, m) * a.C + (n % a.C)] = v;
            } else {
                float* o = a.out + (int64_t)m * a.out_stride + n;
                if (a.mode == OUT_GELU) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
                if (a.mode == OUT_ADD) v += *o;
                *o = v;
            }
        }
    }
}

struct AttnArgs {
    const float* q; int q_stride;                 // [M][C]
    const float* k; const float* v;               // key j of sequence s, head h: k + s * seq_stride + j * row_stride + h * 64
    int64_t seq_stride; int row_stride;
    int n_keys;                                   // cross attention: T_audio; self attention: 0 = the row's position + 1 (the causal mask)
    float* out; int out_stride;
    Rows rows;
};

// one (row, head) per workgroup: scores by thread over the keys, softmax in fp32 (model.py:99), P V by (key quarter, channel)
__global__ __launch_bounds__(256) void k_dec_attn(AttnArgs a) {
    extern __shared__ float s_p[];   // [n_keys]
    __shared__ __align__(16) float s_q[DH];
    __shared__ float s_red[4];
    __shared__ float s_acc[4][DH];
    const int m = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (row_idle(a.rows, m)) return;
    const int L = a.n_keys ? a.n_keys : row_pos(a.rows, m) + 1;
    const float* kb = a.k + (int64_t)row_seq(a.rows, m) * a.seq_stride + h * DH;
    const float* vb = a.v + (int64_t)row_seq(a.rows, m) * a.seq_stride + h * DH;
    if (tid < DH) s_q[tid] = a.q[(int64_t)m * a.q_stride + h * DH + tid] * 0.125f;   // dh^-0.25 on q and on k (model.py:90-92), dh = 64
    __syncthreads();
    float mx = -INFINITY;
    for (int j = tid; j < L; j += 256) {
        const float4* kp = reinterpret_cast<const float4*>(kb + (int64_t)j * a.row_stride);
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < DH / 4; ++d) {
            const float4 kv = kp[d];
            const float4 qv = *reinterpret_cast<const float4*>(s_q + 4 * d);
            s = fmaf(kv.x, qv.x, s); s = fmaf(kv.y, qv.y, s); s = fmaf(kv.z, qv.z, s); s = fmaf(kv.w, qv.w, s);
        }
        s_p[j] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    if (lane == 0) s_red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int j = tid; j < L; j += 256) {
        const float e = expf(s_p[j] - mx);
        s_p[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) s_red[wave] = sum;
    __syncthreads();
    const float s01 = s_red[0] + s_red[1], s23 = s_red[2] + s_red[3];
    sum = mf_opaque(s01) + mf_opaque(s23);
    float acc = 0.f;
    for (int j = wave; j < L; j += 4) acc = fmaf(s_p[j], vb[(int64_t)j * a.row_stride + lane], acc);
    s_acc[wave][lane] = acc;
    __syncthreads();
    if (tid < DH) a.out[(int64_t)m * a.out_stride + h * DH + tid] = mf_sum4(s_acc[0][tid], s_acc[1][tid], s_acc[2][tid], s_acc[3][tid]) / sum;
}

struct ChooseArgs {
    const float* logits; int n_vocab;      // [batch][n_vocab]
    const float* mask;                     // [n_vocab] added to the logits (0 or -inf), or null
    int eot, max_new, n_ctx, advance;      // advance: the step fed one token, the cache is one row longer
    int* len; int* done; int* cur_tok; int* out_len; float* sum_lp; int* out_tok; int out_stride;
};

// one workgroup per sequence.  Ties go to the lowest index (torch.argmax on the reference's CPU path returns the first maximum)
__global__ __launch_bounds__(256) void k_dec_choose(ChooseArgs a) {
    __shared__ float s_v[256];
    __shared__ int s_i[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (a.done[b]) return;
    const float* lg = a.logits + (int64_t)b * a.n_vocab;
    float best = -INFINITY;
    int idx = INT_MAX;
    for (int n = tid; n < a.n_vocab; n += 256) {
        const float v = lg[n] + (a.mask ? a.mask[n] : 0.f);
        if (v > best) { best = v; idx = n; }
    }
    s_v[tid] = best; s_i[tid] = idx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const float v = s_v[tid + o];
            const int i = s_i[tid + o];
            if (v > s_v[tid] || (v == s_v[tid] && i < s_i[tid])) { s_v[tid] = v; s_i[tid] = i; }
        }
        __syncthreads();
    }
    best = s_v[0]; idx = s_i[0];
    __syncthreads();
    float sum = 0.f;
    for (int n = tid; n < a.n_vocab; n += 256) sum += expf(lg[n] + (a.mask ? a.mask[n] : 0.f) - best);
    s_v[tid] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_v[tid] += s_v[tid + o];
        __syncthreads();
    }
    if (tid != 0) return;
    const int len = a.len[b] + (a.advance ? 1 : 0);
    a.len[b] = len;
    if (idx >= a.n_vocab) { a.done[b] = 1; return; }       // no admissible finite logit: stop the sequence
    a.sum_lp[b] += -logf(s_v[0]);                            // log_softmax at the maximum (decoding.py: the end-of-text token's own term counts)
    if (idx == a.eot) { a.done[b] = 1; return; }
    const int n_out = a.out_len[b];
    a.out_tok[(int64_t)b * a.out_stride + n_out] = idx;
    a.out_len[b] = n_out + 1;
    a.cur_tok[b] = idx;
    if (n_out + 1 >= a.max_new || len >= a.n_ctx) a.done[b] = 1;   // budget spent, or no cache row left to feed this token into
}

struct RuleArgs {
    ChooseArgs c;
    const int* hist;                   // test seam: [batch][3] = tokens sampled so far, the last, the one before; null: the sequence's own out_len / out_tok
    int tb, no_ts, max_init, blank;    // timestamp_begin (n_vocab: no timestamp rules), <|notimestamps|>, max_initial_timestamp_index, blank; -1: none
};

// the logit of token n after SuppressBlank, SuppressTokens and the masks of ApplyTimestampRules (decoding.py:392-433).  first: nothing sampled yet;
// pair: 0 none, 1 the last two were timestamps (or the only one was): [timestamp_begin:] is out, 2 a timestamp after text: [:eot] is out
__device__ __forceinline__ float rule_logit(const RuleArgs& a, const float* lg, int n, bool first, int pair) {
    const float v = lg[n] + (a.c.mask ? a.c.mask[n] : 0.f);
    const bool out = (first && a.blank >= 0 && (n == a.blank || n == a.c.eot)) || n == a.no_ts || (pair == 1 && n >= a.tb) || (pair == 2 && n < a.c.eot) ||
                     (first && a.max_init >= 0 && n > a.tb + a.max_init);
    return out ? -INFINITY : v;
}

// first maximum of 256 (value, index) pairs and the sum of 256 partial sums, in k_dec_choose's order
__device__ __forceinline__ void block_argmax(float* s_v, int* s_i, int tid) {
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const float v = s_v[tid + o];
            const int i = s_i[tid + o];
            if (v > s_v[tid] || (v == s_v[tid] && i < s_i[tid])) { s_v[tid] = v; s_i[tid] = i; }
        }
        __syncthreads();
    }
}
__device__ __forceinline__ void block_sum(float* s_v, int tid) {
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_v[tid] += s_v[tid + o];
        __syncthreads();
    }
}

// one workgroup per sequence, two passes over its logits.  Pass 1: the first maximum of the filtered text range [:timestamp_begin] and of the
// filtered timestamps.  Pass 2: sum exp(v - its range's maximum) per range.  Then one thread decides: if logsumexp(timestamps) > max(text), the
// text range is out (decoding.py:436-441; log_softmax moves both sides by the same amount, so unnormalised logits give the same answer), and the
// log-probability of the argmax is -log of the sums brought to its maximum.  With tb = n_vocab every token is text and the arithmetic is
// k_dec_choose's, operation for operation.
__global__ __launch_bounds__(256) void k_dec_choose_rules(RuleArgs a) {
    __shared__ float s_tv[256], s_sv[256];
    __shared__ int s_ti[256], s_si[256];
    const int b = blockIdx.x, tid = threadIdx.x, V = a.c.n_vocab;
    if (a.c.done[b]) return;
    const float* lg = a.c.logits + (int64_t)b * V;
    int n_hist, last = -1, prev = -1;
    if (a.hist) {
        n_hist = a.hist[3 * b]; last = a.hist[3 * b + 1]; prev = a.hist[3 * b + 2];
    } else {
        n_hist = a.c.out_len[b];
        const int* t = a.c.out_tok + (int64_t)b * a.c.out_stride;
        if (n_hist >= 1) last = t[n_hist - 1];
        if (n_hist >= 2) prev = t[n_hist - 2];
    }
    const bool first = n_hist == 0;
    const int pair = (a.tb < V && n_hist >= 1 && last >= a.tb) ? ((n_hist < 2 || prev >= a.tb) ? 1 : 2) : 0;
    float bt = -INFINITY, bs = -INFINITY;
    int it = INT_MAX, is = INT_MAX;
    for (int n = tid; n < V; n += 256) {
        const float v = rule_logit(a, lg, n, first, pair);
        if (n < a.tb) { if (v > bt) { bt = v; it = n; } }
        else if (v > bs) { bs = v; is = n; }
    }
    s_tv[tid] = bt; s_ti[tid] = it; s_sv[tid] = bs; s_si[tid] = is;
    block_argmax(s_tv, s_ti, tid);
    block_argmax(s_sv, s_si, tid);
    bt = s_tv[0]; it = s_ti[0]; bs = s_sv[0]; is = s_si[0];
    __syncthreads();
    const bool has_t = it < V, has_s = is < V;
    float st = 0.f, ss = 0.f;
    for (int n = tid; n < V; n += 256) {
        const float v = rule_logit(a, lg, n, first, pair);
        if (n < a.tb) { if (has_t) st += expf(v - bt); }
        else if (has_s) ss += expf(v - bs);
    }
    s_tv[tid] = st; s_sv[tid] = ss;
    block_sum(s_tv, tid);
    block_sum(s_sv, tid);
    if (tid != 0) return;
    st = s_tv[0]; ss = s_sv[0];
    const int len = a.c.len[b] + (a.c.advance ? 1 : 0);
    a.c.len[b] = len;
    if (!has_t && !has_s) { a.c.done[b] = 1; a.c.cur_tok[b] = -1; return; }   // no admissible finite logit: stop the sequence
    // ss >= 1 (its maximum's own term), so the logsumexp is never below bs: a timestamp above every text token always takes this branch
    const bool ts_wins = has_s && (!has_t || bs + logf(ss) > bt);
    const int idx = ts_wins ? is : it;
    const float sum = ts_wins ? ss : (has_s ? st + ss * expf(bs - bt) : st);
    a.c.sum_lp[b] += -logf(sum);
    a.c.cur_tok[b] = idx;
    if (idx == a.c.eot) { a.c.done[b] = 1; return; }
    const int n_out = a.c.out_len[b];
    a.c.out_tok[(int64_t)b * a.c.out_stride + n_out] = idx;
    a.c.out_len[b] = n_out + 1;
    if (n_out + 1 >= a.c.max_new || len >= a.c.n_ctx) a.c.done[b] = 1;
}

// softmax(logits of the <|startoftranscript|> row)[no_speech] per sequence (decoding.py:602-604); rows = the prefill head's second half
__global__ __launch_bounds__(256) void k_dec_no_speech(const float* __restrict__ logits, int n_vocab, int no_speech, float* __restrict__ prob) {
    __shared__ float s_v[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* lg = logits + (int64_t)b * n_vocab;
    float mx = -INFINITY;
    for (int n = tid; n < n_vocab; n += 256) mx = fmaxf(mx, lg[n]);
    s_v[tid] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_v[tid] = fmaxf(s_v[tid], s_v[tid + o]);
        __syncthreads();
    }
    mx = s_v[0];
    __syncthreads();
    float sum = 0.f;
    for (int n = tid; n < n_vocab; n += 256) sum += expf(lg[n] - mx);
    s_v[tid] = sum;
    block_sum(s_v, tid);
    if (tid == 0) prob[b] = expf(lg[no_speech] - mx) / s_v[0];
}

// detect_language (decoding.py:50-55): every token but the listed language tokens is out; argmax (lowest id on a tie) and softmax over the list.
// out [batch][1 + n_lang]: the chosen id's bits, then the probabilities in the list's order
__global__ __launch_bounds__(256) void k_dec_language(const float* __restrict__ logits, int n_vocab, const int* __restrict__ ids, int n_lang, float* __restrict__ out) {
    __shared__ float s_v[256];
    __shared__ int s_i[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* lg = logits + (int64_t)b * n_vocab;
    float* o = out + (int64_t)b * (n_lang + 1);
    float best = -INFINITY;
    int idx = INT_MAX;
    for (int j = tid; j < n_lang; j += 256) {
        const float v = lg[ids[j]];
        if (v > best || (v == best && ids[j] < idx)) { best = v; idx = ids[j]; }
    }
    s_v[tid] = best; s_i[tid] = idx;
    block_argmax(s_v, s_i, tid);
    best = s_v[0]; idx = s_i[0];
    __syncthreads();
    float sum = 0.f;
    for (int j = tid; j < n_lang; j += 256) sum += expf(lg[ids[j]] - best);
    s_v[tid] = sum;
    block_sum(s_v, tid);
    sum = s_v[0];
    for (int j = tid; j < n_lang; j += 256) o[1 + j] = expf(lg[ids[j]] - best) / sum;
    if (tid == 0) o[0] = __int_as_float(idx < n_vocab ? idx : -1);
}

__global__ void k_dec_rows_fill(int* seq, int* pos, const int* len, int n, int M) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    seq[m] = m / n;
    pos[m] = len[m / n] + m % n;
}
__global__ void k_dec_len_add(int* len, int n, int batch) {
    if ((int)threadIdx.x < batch) len[threadIdx.x] += n;
}

struct Planes { bf16_t* hi = nullptr; bf16_t* lo = nullptr; };

}  // namespace

// the rule parameters of a decode call (-1: none), checked against the vocabulary by rules_check
struct DecodeRules { int tb, no_ts, max_init, blank, no_speech; };

// the C ABI hands this out as an untyped handle (void*)
struct mf_whisper_decoder {
    int precision = MF_PREC_BF16X3;
    int C = 0, n_head = 0, n_layer = 0, n_ctx = 0, n_vocab = 0, max_batch = 1;
    std::vector<void*> owned;
    Planes emb;
    float *pos_emb = nullptr, *ln_g = nullptr, *ln_b = nullptr, *post_g = nullptr, *post_b = nullptr;
    struct Layer {
        Planes qkv, out, cq, ckv, cout, fc1, fc2;
        float *qkv_b, *out_b, *cq_b, *ckv_b, *cout_b, *fc1_b, *fc2_b;
        float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *ln3_g, *ln3_b;
        float *kc, *vc;      // self cache  [max_batch][n_ctx][C]
        float* ckv_out;      // cross K | V [batch * T_audio][2C], written by begin()
    };
    std::vector<Layer> layers;
    float *x = nullptr, *q = nullptr, *ao = nullptr, *h1 = nullptr, *logits = nullptr, *sum_lp = nullptr;   // logits [2 * max_batch][n_vocab]: the sot rows of a prefill follow the last rows
    float *no_speech = nullptr, *lang_out = nullptr;   // [max_batch]; [max_batch][1 + lang_cap], grown by detect_language
    int *lang_ids = nullptr, lang_cap = 0;
    int *row_tok = nullptr, *row_seq = nullptr, *row_pos = nullptr, *last_row = nullptr;
    int *len = nullptr, *done = nullptr, *cur_tok = nullptr, *out_len = nullptr, *out_tok = nullptr;
    int batch = 0, T_audio = 0;   // of the last begin(); 0: none yet
    int fed = -1;                 // tokens the teacher-forced calls appended since begin(); -1: the lengths are ragged (after greedy) or begin() has not run

    ~mf_whisper_decoder() { for (void* p : owned) (void)hipFree(p); }

    template <typename T> int dev_alloc(T** p, size_t n) {
        MF_HIP(hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T)));
        owned.push_back(*p);
        return MF_OK;
    }
    int upload(const float* host, size_t n, float** dev) {
        int rc = dev_alloc(dev, n);
        if (rc) return rc;
        MF_HIP(hipMemcpy(*dev, host, n * sizeof(float), hipMemcpyHostToDevice));
        return MF_OK;
    }
    int upload_planes(const float* host, size_t n, Planes* p) {
        std::vector<bf16_t> hi(n), lo(n);
        for (size_t i = 0; i < n; ++i) {
            hi[i] = mf_f2bf(host[i]);
            lo[i] = mf_f2bf(host[i] - mf_bf2f(hi[i]));
        }
        int rc;
        if ((rc = dev_alloc(&p->hi, n)) || (rc = dev_alloc(&p->lo, n))) return rc;
        MF_HIP(hipMemcpy(p->hi, hi.data(), n * sizeof(bf16_t), hipMemcpyHostToDevice));
        MF_HIP(hipMemcpy(p->lo, lo.data(), n * sizeof(bf16_t), hipMemcpyHostToDevice));
        return MF_OK;
    }
    int linear(LinArgs a, hipStream_t s) const;
    int attention(AttnArgs a, int M, int max_keys, hipStream_t s) const;
    int forward(int M, const int* tokens, Rows rows, hipStream_t s);
    int head(int M, const int* gather, float* out, Rows rows, hipStream_t s) const;
    int choose(const float* mask, int eot, int max_new, int advance, int B, hipStream_t s) const;
    int choose_rules(const DecodeRules& r, const float* mask, int eot, int max_new, int advance, int B, hipStream_t s) const;
    int decode(const char* who, const int* prompts, const int* prompt_lens, const float* mask, int eot, int max_new, int check_every, const DecodeRules* rules,
               const int* sot_index, int* out_tokens, int* out_lens, float* sum_logprobs, float* no_speech_probs, int batch, hipStream_t s);
};

int mf_whisper_decoder::linear(LinArgs a, hipStream_t s) const {
    int R = a.M >= 5 ? 8 : a.M >= 3 ? 4 : a.M;
    while (R > 1 && (size_t)R * a.K * sizeof(float) > 48 * 1024) R /= 2;
    a.cols_per_block = a.N > 4096 ? 4 * LIN_COLS : LIN_COLS;      // the vocabulary head: fewer, longer workgroups per staged x
    const dim3 grid((a.N + a.cols_per_block - 1) / a.cols_per_block, (a.M + R - 1) / R);
    const size_t lds = (size_t)R * a.K * sizeof(float);
    const bool x3 = precision == MF_PREC_BF16X3;
#define MF_DEC_LIN(RR)                                                                                              \
    if (x3) hipLaunchKernelGGL((k_dec_linear<RR, true>), grid, dim3(LIN_THREADS), lds, s, a);                       \
    else hipLaunchKernelGGL((k_dec_linear<RR, false>), grid, dim3(LIN_THREADS), lds, s, a)
    switch (R) {
        case 1: MF_DEC_LIN(1); break;
        case 2: MF_DEC_LIN(2); break;
        case 4: MF_DEC_LIN(4); break;
        default: MF_DEC_LIN(8); break;
    }
#undef MF_DEC_LIN
    MF_HIP(hipGetLastError());
    return MF_OK;
}

int mf_whisper_decoder::attention(AttnArgs a, int M, int max_keys, hipStream_t s) const {
    hipLaunchKernelGGL(k_dec_attn, dim3(M, n_head), dim3(256), (size_t)max_keys * sizeof(float), s, a);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

// the blocks of TextDecoder.forward over M rows: x <- embedding, then per layer self attention, cross attention, MLP (model.py:124-127)
int mf_whisper_decoder::forward(int M, const int* tokens, Rows rows, hipStream_t s) {
    int rc;
    hipLaunchKernelGGL(k_dec_embed, dim3(M), dim3(128), 0, s, tokens, emb.hi, emb.lo, pos_emb, x, C, n_vocab, rows);
    MF_HIP(hipGetLastError());
    const int64_t self_stride = (int64_t)n_ctx * C, cross_stride = (int64_t)T_audio * 2 * C;
    for (Layer& L : layers) {
        LinArgs a{};
        a.M = M; a.rows = rows; a.C = C;
        // x + attn(attn_ln(x)): q | k | v in one pass over the weights, k and v straight into the cache rows
        a.x = x; a.x_stride = C; a.ln_g = L.ln1_g; a.ln_b = L.ln1_b; a.w_hi = L.qkv.hi; a.w_lo = L.qkv.lo; a.bias = L.qkv_b;
        a.N = 3 * C; a.K = C; a.mode = OUT_QKV; a.out = q; a.out_stride = C; a.kcache = L.kc; a.vcache = L.vc; a.cache_seq_stride = self_stride;
        if ((rc = linear(a, s))) return rc;
        if ((rc = attention(AttnArgs{q, C, L.kc, L.vc, self_stride, C, 0, ao, C, rows}, M, n_ctx, s))) return rc;
        LinArgs o{};
        o.M = M; o.rows = rows; o.C = C;
        o.x = ao; o.x_stride = C; o.w_hi = L.out.hi; o.w_lo = L.out.lo; o.bias = L.out_b; o.N = C; o.K = C; o.mode = OUT_ADD; o.out = x; o.out_stride = C;
        if ((rc = linear(o, s))) return rc;
        // x + cross_attn(cross_attn_ln(x), xa): the keys and values of xa were projected once, by begin()
        a.ln_g = L.ln2_g; a.ln_b = L.ln2_b; a.w_hi = L.cq.hi; a.w_lo = L.cq.lo; a.bias = L.cq_b; a.N = C; a.mode = OUT_STORE;
        if ((rc = linear(a, s))) return rc;
        if ((rc = attention(AttnArgs{q, C, L.ckv_out, L.ckv_out + C, cross_stride, 2 * C, T_audio, ao, C, rows}, M, T_audio, s))) return rc;
        o.w_hi = L.cout.hi; o.w_lo = L.cout.lo; o.bias = L.cout_b;
        if ((rc = linear(o, s))) return rc;
        // x + mlp(mlp_ln(x)), exact GELU
        a.ln_g = L.ln3_g; a.ln_b = L.ln3_b; a.w_hi = L.fc1.hi; a.w_lo = L.fc1.lo; a.bias = L.fc1_b; a.N = 4 * C; a.mode = OUT_GELU; a.out = h1; a.out_stride = 4 * C;
        if ((rc = linear(a, s))) return rc;
        o.x = h1; o.x_stride = 4 * C; o.K = 4 * C; o.w_hi = L.fc2.hi; o.w_lo = L.fc2.lo; o.bias = L.fc2_b;
        if ((rc = linear(o, s))) return rc;
    }
    return MF_OK;
}

// ln(x) @ token_embedding^T (weights tied, model.py:210-211) for the rows gather names (null: rows 0..M-1)
int mf_whisper_decoder::head(int M, const int* gather, float* out, Rows rows, hipStream_t s) const {
    LinArgs a{};
    a.M = M; a.rows = rows; a.C = C; a.x = x; a.x_stride = C; a.gather = gather; a.ln_g = ln_g; a.ln_b = ln_b;
    a.w_hi = emb.hi; a.w_lo = emb.lo; a.N = n_vocab; a.K = C; a.mode = OUT_STORE; a.out = out; a.out_stride = n_vocab;
    return linear(a, s);
}

int mf_whisper_decoder::choose(const float* mask, int eot, int max_new, int advance, int B, hipStream_t s) const {
    const ChooseArgs c{logits, n_vocab, mask, eot, max_new, n_ctx, advance, len, done, cur_tok, out_len, sum_lp, out_tok, n_ctx};
    hipLaunchKernelGGL(k_dec_choose, dim3(B), dim3(256), 0, s, c);
    MF_HIP(hipGetLastError());
    return MF_OK;
}

static RuleArgs rule_args(const ChooseArgs& c, const DecodeRules& r, const int* hist) {
    const bool ts = r.tb >= 0;
    return RuleArgs{c, hist, ts ? r.tb : c.n_vocab, ts ? r.no_ts : -1, ts ? r.max_init : -1, r.blank};
}

int mf_whisper_decoder::choose_rules(const DecodeRules& r, const float* mask, int eot, int max_new, int advance, int B, hipStream_t s) const {
    const ChooseArgs c{logits, n_vocab, mask, eot, max_new, n_ctx, advance, len, done, cur_tok, out_len, sum_lp, out_tok, n_ctx};
    hipLaunchKernelGGL(k_dec_choose_rules, dim3(B), dim3(256), 0, s, rule_args(c, r, nullptr));
    MF_HIP(hipGetLastError());
    return MF_OK;
}

// every id of a rule set against the vocabulary; timestamp_begin = -1 turns the timestamp rules off (no_timestamps and the initial cap are then not read)
static int rules_check(const char* who, const DecodeRules& r, int eot, int n_vocab) {
    MF_REQUIRE(eot >= 0 && eot < n_vocab, "%s: end-of-text token %d outside the vocabulary (%d)", who, eot, n_vocab);
    MF_REQUIRE(r.tb == -1 || (eot < r.tb && r.tb <= n_vocab), "%s: timestamp_begin = %d; eot (%d) < timestamp_begin <= n_vocab (%d), or -1 for no timestamp rules",
               who, r.tb, eot, n_vocab);
    MF_REQUIRE(r.no_ts >= -1 && r.no_ts < n_vocab, "%s: no_timestamps token %d outside the vocabulary (%d)", who, r.no_ts, n_vocab);
    MF_REQUIRE(r.max_init >= -1 && (r.tb < 0 || r.max_init < std::max(n_vocab - r.tb, 1)), "%s: max_initial_timestamp_index = %d, the vocabulary holds %d timestamps (-1: none)",
               who, r.max_init, r.tb < 0 ? 0 : n_vocab - r.tb);
    MF_REQUIRE(r.blank >= -1 && r.blank < n_vocab, "%s: blank token %d outside the vocabulary (%d)", who, r.blank, n_vocab);
    MF_REQUIRE(r.no_speech >= -1 && r.no_speech < n_vocab, "%s: no_speech token %d outside the vocabulary (%d)", who, r.no_speech, n_vocab);
    return MF_OK;
}

// ------------------------------------------------------------------------------------------------------
extern "C" int mf_whisper_decoder_create(const mf_tensor* weights, int n_weights, int n_head, int precision, int max_batch, void** out) {
    MF_REQUIRE(weights && out && n_weights > 0 && n_head > 0, "whisper_decoder_create: bad argument");
    MF_REQUIRE(precision == MF_PREC_BF16 || precision == MF_PREC_BF16X3, "whisper_decoder_create: unknown precision %d", precision);
    MF_REQUIRE(max_batch >= 1 && max_batch <= MAX_DEC_BATCH, "whisper_decoder_create: max_batch = %d, 1..%d sequences decode together", max_batch, MAX_DEC_BATCH);
    *out = nullptr;
    MfStateDict sd;
    int rc = mf_sd_build(weights, n_weights, "whisper_decoder_create", {}, &sd);
    if (rc) return rc;
    auto it = sd.find("decoder.token_embedding.weight");
    MF_REQUIRE(it != sd.end() && it->second->ndim == 2, "whisper_decoder_create: decoder.token_embedding.weight [n_vocab, n_state] missing");
    auto ip = sd.find("decoder.positional_embedding");
    MF_REQUIRE(ip != sd.end() && ip->second->ndim == 2, "whisper_decoder_create: decoder.positional_embedding [n_text_ctx, n_state] missing");
    std::unique_ptr<mf_whisper_decoder> h(new mf_whisper_decoder());
    h->precision = precision; h->n_head = n_head; h->max_batch = max_batch;
    h->n_vocab = (int)it->second->shape[0];
    const int C = h->C = (int)it->second->shape[1];
    h->n_ctx = (int)ip->second->shape[0];
    MF_REQUIRE((int)ip->second->shape[1] == C, "whisper_decoder_create: positional_embedding is %d wide, token_embedding %d", (int)ip->second->shape[1], C);
    MF_REQUIRE(C == n_head * DH, "whisper_decoder_create: n_state %d / n_head %d: the head width must be 64", C, n_head);
    MF_REQUIRE(C % LIN_KSTEP == 0, "whisper_decoder_create: n_state %d must be a multiple of %d", C, LIN_KSTEP);
    MF_REQUIRE(h->n_ctx >= 2 && h->n_vocab >= 2, "whisper_decoder_create: n_text_ctx %d, n_vocab %d", h->n_ctx, h->n_vocab);
    int L = 0;
    while (sd.count("decoder.blocks." + std::to_string(L) + ".attn.query.weight")) ++L;
    MF_REQUIRE(L > 0, "whisper_decoder_create: no decoder blocks in the state dict");
    h->n_layer = L;
    const char* who = "whisper_decoder";
    auto get = [&](const std::string& k, int64_t n) { return mf_sd_find(sd, who, k, n); };
    const size_t CC = (size_t)C * C;
    if ((rc = h->upload_planes(it->second->data, (size_t)h->n_vocab * C, &h->emb))) return rc;
    if ((rc = h->upload(ip->second->data, (size_t)h->n_ctx * C, &h->pos_emb))) return rc;
    const mf_tensor *lg = get("decoder.ln.weight", C), *lb = get("decoder.ln.bias", C);
    if (!lg || !lb) return MF_ERR_INVALID;
    if ((rc = h->upload(lg->data, C, &h->ln_g)) || (rc = h->upload(lb->data, C, &h->ln_b))) return rc;
    // the encoder handle returns its last block's output; ln_post (model.py:165) is applied here, in begin(), when the caller hands it over
    if (sd.count("encoder.ln_post.weight")) {
        const mf_tensor *pg = get("encoder.ln_post.weight", C), *pb = get("encoder.ln_post.bias", C);
        if (!pg || !pb) return MF_ERR_INVALID;
        if ((rc = h->upload(pg->data, C, &h->post_g)) || (rc = h->upload(pb->data, C, &h->post_b))) return rc;
    }
    const size_t cache_n = (size_t)max_batch * h->n_ctx * C, cross_n = (size_t)max_batch * N_AUDIO_CTX * 2 * C;
    for (int l = 0; l < L; ++l) {
        const std::string p = "decoder.blocks." + std::to_string(l) + ".";
        mf_whisper_decoder::Layer Ly{};
        struct Att { const mf_tensor *qw, *qb, *kw, *vw, *vb, *ow, *ob, *g, *b; } at[2];
        bool ok = true;
        for (int c = 0; c < 2; ++c) {
            const std::string a = p + (c ? "cross_attn" : "attn");
            at[c] = Att{get(a + ".query.weight", CC), get(a + ".query.bias", C), get(a + ".key.weight", CC), get(a + ".value.weight", CC), get(a + ".value.bias", C),
                        get(a + ".out.weight", CC), get(a + ".out.bias", C), get(a + "_ln.weight", C), get(a + "_ln.bias", C)};
            ok = ok && at[c].qw && at[c].qb && at[c].kw && at[c].vw && at[c].vb && at[c].ow && at[c].ob && at[c].g && at[c].b;
        }
        const mf_tensor *f1w = get(p + "mlp.0.weight", 4 * CC), *f1b = get(p + "mlp.0.bias", 4 * C), *f2w = get(p + "mlp.2.weight", 4 * CC), *f2b = get(p + "mlp.2.bias", C);
        const mf_tensor *g3 = get(p + "mlp_ln.weight", C), *b3 = get(p + "mlp_ln.bias", C);
        if (!ok || !f1w || !f1b || !f2w || !f2b || !g3 || !b3) return MF_ERR_INVALID;
        // q | k | v rows of one weight matrix (key has no bias, model.py:62); cross attention: q alone per step, k | v once per segment
        std::vector<float> w(3 * CC), b((size_t)3 * C, 0.f);
        std::copy(at[0].qw->data, at[0].qw->data + CC, w.begin());
        std::copy(at[0].kw->data, at[0].kw->data + CC, w.begin() + CC);
        std::copy(at[0].vw->data, at[0].vw->data + CC, w.begin() + 2 * CC);
        std::copy(at[0].qb->data, at[0].qb->data + C, b.begin());
        std::copy(at[0].vb->data, at[0].vb->data + C, b.begin() + 2 * C);
        if ((rc = h->upload_planes(w.data(), 3 * CC, &Ly.qkv)) || (rc = h->upload(b.data(), 3 * C, &Ly.qkv_b))) return rc;
        std::copy(at[1].kw->data, at[1].kw->data + CC, w.begin());
        std::copy(at[1].vw->data, at[1].vw->data + CC, w.begin() + CC);
        std::fill(b.begin(), b.begin() + C, 0.f);
        std::copy(at[1].vb->data, at[1].vb->data + C, b.begin() + C);
        if ((rc = h->upload_planes(w.data(), 2 * CC, &Ly.ckv)) || (rc = h->upload(b.data(), 2 * C, &Ly.ckv_b))) return rc;
        if ((rc = h->upload_planes(at[0].ow->data, CC, &Ly.out)) || (rc = h->upload(at[0].ob->data, C, &Ly.out_b))) return rc;
        if ((rc = h->upload_planes(at[1].qw->data, CC, &Ly.cq)) || (rc = h->upload(at[1].qb->data, C, &Ly.cq_b))) return rc;
        if ((rc = h->upload_planes(at[1].ow->data, CC, &Ly.cout)) || (rc = h->upload(at[1].ob->data, C, &Ly.cout_b))) return rc;
        if ((rc = h->upload_planes(f1w->data, 4 * CC, &Ly.fc1)) || (rc = h->upload(f1b->data, 4 * C, &Ly.fc1_b))) return rc;
        if ((rc = h->upload_planes(f2w->data, 4 * CC, &Ly.fc2)) || (rc = h->upload(f2b->data, C, &Ly.fc2_b))) return rc;
        if ((rc = h->upload(at[0].g->data, C, &Ly.ln1_g)) || (rc = h->upload(at[0].b->data, C, &Ly.ln1_b))) return rc;
        if ((rc = h->upload(at[1].g->data, C, &Ly.ln2_g)) || (rc = h->upload(at[1].b->data, C, &Ly.ln2_b))) return rc;
        if ((rc = h->upload(g3->data, C, &Ly.ln3_g)) || (rc = h->upload(b3->data, C, &Ly.ln3_b))) return rc;
        if ((rc = h->dev_alloc(&Ly.kc, cache_n)) || (rc = h->dev_alloc(&Ly.vc, cache_n)) || (rc = h->dev_alloc(&Ly.ckv_out, cross_n))) return rc;
        h->layers.push_back(Ly);
    }
    const size_t rows = (size_t)max_batch * h->n_ctx;
    if ((rc = h->dev_alloc(&h->x, rows * C)) || (rc = h->dev_alloc(&h->q, rows * C)) || (rc = h->dev_alloc(&h->ao, rows * C)) ||
        (rc = h->dev_alloc(&h->h1, rows * 4 * C)) || (rc = h->dev_alloc(&h->logits, (size_t)2 * max_batch * h->n_vocab)) || (rc = h->dev_alloc(&h->no_speech, max_batch)) ||
        (rc = h->dev_alloc(&h->row_tok, rows)) || (rc = h->dev_alloc(&h->row_seq, rows)) || (rc = h->dev_alloc(&h->row_pos, rows)) ||
        (rc = h->dev_alloc(&h->out_tok, rows)) || (rc = h->dev_alloc(&h->last_row, 2 * max_batch)) || (rc = h->dev_alloc(&h->len, max_batch)) ||
        (rc = h->dev_alloc(&h->done, max_batch)) || (rc = h->dev_alloc(&h->cur_tok, max_batch)) || (rc = h->dev_alloc(&h->out_len, max_batch)) ||
        (rc = h->dev_alloc(&h->sum_lp, max_batch))) return rc;
    MF_HIP(hipMemset(h->x, 0, rows * C * sizeof(float)));
    *out = h.release();
    return MF_OK;
}

extern "C" int mf_whisper_decoder_dims(const void* handle, int* n_layer, int* n_text_ctx, int* n_state, int* n_vocab) {
    const mf_whisper_decoder* h = static_cast<const mf_whisper_decoder*>(handle);
    MF_REQUIRE(h && n_layer && n_text_ctx && n_state && n_vocab, "whisper_decoder_dims: null argument");
    *n_layer = h->n_layer; *n_text_ctx = h->n_ctx; *n_state = h->C; *n_vocab = h->n_vocab;
    return MF_OK;
}

extern "C" int mf_whisper_decoder_begin(void* handle, const float* enc_states, int T_audio, int batch, void* stream) {
    mf_whisper_decoder* h = static_cast<mf_whisper_decoder*>(handle);
    MF_REQUIRE(h && enc_states, "whisper_decoder_begin: null argument");
    MF_REQUIRE(batch >= 1 && batch <= h->max_batch, "whisper_decoder_begin: batch %d exceeds the handle's max_batch %d", batch, h->max_batch);
    MF_REQUIRE(T_audio >= 1 && T_audio <= N_AUDIO_CTX, "whisper_decoder_begin: T_audio = %d, one segment holds 1..%d encoder tokens", T_audio, N_AUDIO_CTX);
    hipStream_t s = (hipStream_t)stream;
    const int C = h->C;
    h->batch = 0; h->fed = -1;
    MF_HIP(hipMemsetAsync(h->len, 0, h->max_batch * sizeof(int), s));
    MF_HIP(hipMemsetAsync(h->done, 0, h->max_batch * sizeof(int), s));
    const size_t cache_bytes = (size_t)h->max_batch * h->n_ctx * C * sizeof(float);
    for (auto& L : h->layers) {
        MF_HIP(hipMemsetAsync(L.kc, 0, cache_bytes, s));
        MF_HIP(hipMemsetAsync(L.vc, 0, cache_bytes, s));
        LinArgs a{};
        a.M = batch * T_audio; a.C = C; a.x = enc_states; a.x_stride = C; a.ln_g = h->post_g; a.ln_b = h->post_b;
        a.w_hi = L.ckv.hi; a.w_lo = L.ckv.lo; a.bias = L.ckv_b; a.N = 2 * C; a.K = C; a.mode = OUT_STORE; a.out = L.ckv_out; a.out_stride = 2 * C;
        const int rc = h->linear(a, s);
        if (rc) return rc;
    }
    h->batch = batch; h->T_audio = T_audio; h->fed = 0;
    return MF_OK;
}

extern "C" int mf_whisper_decoder_logits(void* handle, const int* tokens, int n, float* logits, int batch, void* stream) {
    mf_whisper_decoder* h = static_cast<mf_whisper_decoder*>(handle);
    MF_REQUIRE(h && tokens && logits, "whisper_decoder_logits: null argument");
    MF_REQUIRE(h->batch > 0 && h->fed >= 0, "whisper_decoder_logits: call mf_whisper_decoder_begin first (a greedy run leaves the caches ragged)");
    MF_REQUIRE(batch == h->batch, "whisper_decoder_logits: batch %d, mf_whisper_decoder_begin was given %d", batch, h->batch);
    MF_REQUIRE(n >= 1 && h->fed + n <= h->n_ctx, "whisper_decoder_logits: %d tokens after the %d already fed exceed n_text_ctx = %d", n, h->fed, h->n_ctx);
    hipStream_t s = (hipStream_t)stream;
    const int M = batch * n;
    hipLaunchKernelGGL(k_dec_rows_fill, dim3((M + 255) / 256), dim3(256), 0, s, h->row_seq, h->row_pos, h->len, n, M);
    MF_HIP(hipGetLastError());
    const Rows rows{h->row_seq, h->row_pos, h->len, nullptr};
    int rc;
    if ((rc = h->forward(M, tokens, rows, s))) return rc;
    if ((rc = h->head(M, nullptr, logits, rows, s))) return rc;
    hipLaunchKernelGGL(k_dec_len_add, dim3(1), dim3(64), 0, s, h->len, n, batch);
    MF_HIP(hipGetLastError());
    h->fed += n;
    return MF_OK;
}

// the body of both decode calls.  rules == null: mf_whisper_decoder_greedy, launch for launch what it always was (k_dec_choose, `batch` head rows)
int mf_whisper_decoder::decode(const char* who, const int* prompts, const int* prompt_lens, const float* suppress_mask, int eot, int max_new, int check_every,
                               const DecodeRules* rules, const int* sot_index, int* out_tokens, int* out_lens, float* sum_logprobs, float* no_speech_probs, int batch,
                               hipStream_t s) {
    MF_REQUIRE(prompts && prompt_lens && out_tokens && out_lens && sum_logprobs, "%s: null argument", who);
    MF_REQUIRE(this->batch > 0, "%s: call mf_whisper_decoder_begin first", who);
    MF_REQUIRE(batch == this->batch, "%s: batch %d, mf_whisper_decoder_begin was given %d", who, batch, this->batch);
    MF_REQUIRE(check_every >= 1, "%s: check_every = %d", who, check_every);
    MF_REQUIRE(eot >= 0 && eot < n_vocab, "%s: end-of-text token %d outside the vocabulary (%d)", who, eot, n_vocab);
    const bool want_nsp = rules && rules->no_speech >= 0;
    if (rules) {
        const int rc = rules_check(who, *rules, eot, n_vocab);
        if (rc) return rc;
        MF_REQUIRE(!want_nsp || (sot_index && no_speech_probs), "%s: a no_speech token needs the sot index of every prompt and an output array", who);
    }
    int total = 0, shortest = INT_MAX;
    std::vector<int> tok, seq, pos, last(want_nsp ? 2 * batch : batch);
    for (int b = 0; b < batch; ++b) {
        const int n = prompt_lens[b];
        MF_REQUIRE(n >= 1 && n <= n_ctx / 2, "%s: prompt %d has %d tokens; a prompt holds 1..n_text_ctx / 2 = %d", who, b, n, n_ctx / 2);
        for (int i = 0; i < n; ++i) {
            const int t = prompts[total + i];
            MF_REQUIRE(t >= 0 && t < n_vocab, "%s: prompt %d token %d = %d is outside the vocabulary (%d)", who, b, i, t, n_vocab);
            tok.push_back(t); seq.push_back(b); pos.push_back(i);
        }
        if (want_nsp) {
            MF_REQUIRE(sot_index[b] >= 0 && sot_index[b] < n, "%s: sot index %d of prompt %d lies outside its %d tokens", who, sot_index[b], b, n);
            last[batch + b] = total + sot_index[b];
        }
        total += n;
        last[b] = total - 1;
        shortest = std::min(shortest, n);
    }
    // a sequence of p prompt tokens can emit n_text_ctx - p + 1 tokens before no cache row is left to feed the last one into
    MF_REQUIRE(max_new >= 1 && max_new <= n_ctx - shortest + 1, "%s: max_new = %d, the cache holds at most %d new tokens after the shortest prompt (%d)",
               who, max_new, n_ctx - shortest + 1, shortest);
    fed = -1;
    int rc;
    MF_HIP(hipMemcpyAsync(row_tok, tok.data(), total * sizeof(int), hipMemcpyHostToDevice, s));
    MF_HIP(hipMemcpyAsync(row_seq, seq.data(), total * sizeof(int), hipMemcpyHostToDevice, s));
    MF_HIP(hipMemcpyAsync(row_pos, pos.data(), total * sizeof(int), hipMemcpyHostToDevice, s));
    MF_HIP(hipMemcpyAsync(last_row, last.data(), last.size() * sizeof(int), hipMemcpyHostToDevice, s));
    MF_HIP(hipMemcpyAsync(len, prompt_lens, batch * sizeof(int), hipMemcpyHostToDevice, s));
    MF_HIP(hipMemsetAsync(done, 0, batch * sizeof(int), s));
    MF_HIP(hipMemsetAsync(out_len, 0, batch * sizeof(int), s));
    MF_HIP(hipMemsetAsync(sum_lp, 0, batch * sizeof(float), s));
    MF_HIP(hipMemsetAsync(out_tok, 0, (size_t)batch * n_ctx * sizeof(int), s));
    MF_HIP(hipStreamSynchronize(s));   // the host vectors above are read by then
    // prefill: every prompt token in one pass, the logits of each sequence's last one (and, for the no-speech probability, of its sot token)
    const Rows pre{row_seq, row_pos, len, nullptr};
    if ((rc = forward(total, row_tok, pre, s))) return rc;
    const Rows step{nullptr, nullptr, len, done};
    auto pick = [&](int advance) { return rules ? choose_rules(*rules, suppress_mask, eot, max_new, advance, batch, s) : choose(suppress_mask, eot, max_new, advance, batch, s); };
    if (want_nsp) {
        // 2 * batch head rows: a row's arithmetic does not depend on how many rows share its pass.  No done flag is set yet, and none is read here
        if ((rc = head(2 * batch, last_row, logits, Rows{nullptr, nullptr, len, nullptr}, s))) return rc;
        hipLaunchKernelGGL(k_dec_no_speech, dim3(batch), dim3(256), 0, s, logits + (size_t)batch * n_vocab, n_vocab, rules->no_speech, no_speech);
        MF_HIP(hipGetLastError());
    } else if ((rc = head(batch, last_row, logits, step, s))) return rc;
    if ((rc = pick(0))) return rc;
    std::vector<int> flags(batch);
    for (int steps = 0; steps < max_new - 1;) {
        for (int i = 0; i < check_every && steps < max_new - 1; ++i, ++steps) {
            if ((rc = forward(batch, cur_tok, step, s))) return rc;
            if ((rc = head(batch, nullptr, logits, step, s))) return rc;
            if ((rc = pick(1))) return rc;
        }
        MF_HIP(hipMemcpyAsync(flags.data(), done, batch * sizeof(int), hipMemcpyDeviceToHost, s));
        MF_HIP(hipStreamSynchronize(s));
        if (std::all_of(flags.begin(), flags.end(), [](int d) { return d != 0; })) break;
    }
    std::vector<int> all((size_t)batch * n_ctx);
    MF_HIP(hipMemcpyAsync(all.data(), out_tok, all.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    MF_HIP(hipMemcpyAsync(out_lens, out_len, batch * sizeof(int), hipMemcpyDeviceToHost, s));
    MF_HIP(hipMemcpyAsync(sum_logprobs, sum_lp, batch * sizeof(float), hipMemcpyDeviceToHost, s));
    if (want_nsp) MF_HIP(hipMemcpyAsync(no_speech_probs, no_speech, batch * sizeof(float), hipMemcpyDeviceToHost, s));
    MF_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < batch; ++b) std::copy(all.begin() + (size_t)b * n_ctx, all.begin() + (size_t)b * n_ctx + max_new, out_tokens + (size_t)b * max_new);
    return MF_OK;
}

extern "C" int mf_whisper_decoder_greedy(void* handle, const int* prompts, const int* prompt_lens, const float* suppress_mask, int eot, int max_new,
                                         int check_every, int* out_tokens, int* out_lens, float* sum_logprobs, int batch, void* stream) {
    mf_whisper_decoder* h = static_cast<mf_whisper_decoder*>(handle);
    MF_REQUIRE(h, "whisper_decoder_greedy: null argument");
    return h->decode("whisper_decoder_greedy", prompts, prompt_lens, suppress_mask, eot, max_new, check_every, nullptr, nullptr, out_tokens, out_lens, sum_logprobs, nullptr,
                     batch, (hipStream_t)stream);
}

extern "C" int mf_whisper_decoder_decode(void* handle, const int* prompts, const int* prompt_lens, const float* suppress_mask, int eot, int max_new, int check_every,
                                         int timestamp_begin, int no_timestamps, int max_initial_timestamp_index, int blank, int no_speech, const int* sot_index,
                                         int* out_tokens, int* out_lens, float* sum_logprobs, float* no_speech_probs, int batch, void* stream) {
    mf_whisper_decoder* h = static_cast<mf_whisper_decoder*>(handle);
    MF_REQUIRE(h, "whisper_decoder_decode: null argument");
    const DecodeRules r{timestamp_begin, no_timestamps, max_initial_timestamp_index, blank, no_speech};
    return h->decode("whisper_decoder_decode", prompts, prompt_lens, suppress_mask, eot, max_new, check_every, &r, sot_index, out_tokens, out_lens, sum_logprobs, no_speech_probs,
                     batch, (hipStream_t)stream);
}

extern "C" int mf_whisper_decoder_detect_language(void* handle, int sot, const int* language_tokens, int n_languages, int* out_tokens, float* out_probs, int batch, void* stream) {
    mf_whisper_decoder* h = static_cast<mf_whisper_decoder*>(handle);
    MF_REQUIRE(h && language_tokens && out_tokens && out_probs, "whisper_decoder_detect_language: null argument");
    MF_REQUIRE(h->batch > 0 && h->fed == 0, "whisper_decoder_detect_language: runs directly after mf_whisper_decoder_begin, before any token is fed");
    MF_REQUIRE(batch == h->batch, "whisper_decoder_detect_language: batch %d, mf_whisper_decoder_begin was given %d", batch, h->batch);
    MF_REQUIRE(sot >= 0 && sot < h->n_vocab, "whisper_decoder_detect_language: sot token %d outside the vocabulary (%d)", sot, h->n_vocab);
    MF_REQUIRE(n_languages >= 1 && n_languages <= h->n_vocab, "whisper_decoder_detect_language: %d language tokens", n_languages);
    std::vector<char> seen(h->n_vocab, 0);
    for (int j = 0; j < n_languages; ++j) {
        const int t = language_tokens[j];
        MF_REQUIRE(t >= 0 && t < h->n_vocab, "whisper_decoder_detect_language: language token %d = %d is outside the vocabulary (%d)", j, t, h->n_vocab);
        MF_REQUIRE(!seen[t], "whisper_decoder_detect_language: language token %d is listed twice", t);
        seen[t] = 1;
    }
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (n_languages > h->lang_cap) {
        // a longer list than any before: the old pair is given back first (no launch of an earlier call is in flight, each call ends in a read-back)
        for (void* old : {(void*)h->lang_ids, (void*)h->lang_out})
            if (old) {
                h->owned.erase(std::remove(h->owned.begin(), h->owned.end(), old), h->owned.end());
                (void)hipFree(old);
            }
        h->lang_ids = nullptr; h->lang_out = nullptr; h->lang_cap = 0;
        if ((rc = h->dev_alloc(&h->lang_ids, n_languages)) || (rc = h->dev_alloc(&h->lang_out, (size_t)h->max_batch * (n_languages + 1)))) return rc;
        h->lang_cap = n_languages;
    }
    const std::vector<int> tok(batch, sot);
    MF_HIP(hipMemcpyAsync(h->row_tok, tok.data(), batch * sizeof(int), hipMemcpyHostToDevice, s));
    MF_HIP(hipMemcpyAsync(h->lang_ids, language_tokens, n_languages * sizeof(int), hipMemcpyHostToDevice, s));
    MF_HIP(hipStreamSynchronize(s));
    // one token per sequence at position 0 (every length is 0 after begin and stays 0); cache row 0 is zeroed again below
    const Rows rows{nullptr, nullptr, h->len, nullptr};
    if ((rc = h->forward(batch, h->row_tok, rows, s))) return rc;
    if ((rc = h->head(batch, nullptr, h->logits, rows, s))) return rc;
    hipLaunchKernelGGL(k_dec_language, dim3(batch), dim3(256), 0, s, h->logits, h->n_vocab, h->lang_ids, n_languages, h->lang_out);
    MF_HIP(hipGetLastError());
    const size_t pitch = (size_t)h->n_ctx * h->C * sizeof(float);
    for (auto& L : h->layers) {
        MF_HIP(hipMemset2DAsync(L.kc, pitch, 0, h->C * sizeof(float), batch, s));
        MF_HIP(hipMemset2DAsync(L.vc, pitch, 0, h->C * sizeof(float), batch, s));
    }
    std::vector<float> got((size_t)batch * (n_languages + 1));
    MF_HIP(hipMemcpyAsync(got.data(), h->lang_out, got.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    MF_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < batch; ++b) {
        const float* g = got.data() + (size_t)b * (n_languages + 1);
        std::memcpy(out_tokens + b, g, sizeof(int));
        std::copy(g + 1, g + 1 + n_languages, out_probs + (size_t)b * n_languages);
    }
    return MF_OK;
}

extern "C" int mf_whisper_decoder_choose(void* handle, const float* logits, const int* history, const float* suppress_mask, int eot, int timestamp_begin, int no_timestamps,
                                         int max_initial_timestamp_index, int blank, int* tokens, float* logprobs, int* done, int batch, void* stream) {
    mf_whisper_decoder* h = static_cast<mf_whisper_decoder*>(handle);
    MF_REQUIRE(h && logits && history && tokens && logprobs && done, "whisper_decoder_choose: null argument");
    MF_REQUIRE(batch >= 1 && batch <= h->max_batch, "whisper_decoder_choose: batch %d exceeds the handle's max_batch %d", batch, h->max_batch);
    const DecodeRules r{timestamp_begin, no_timestamps, max_initial_timestamp_index, blank, -1};
    int rc = rules_check("whisper_decoder_choose", r, eot, h->n_vocab);
    if (rc) return rc;
    for (int b = 0; b < batch; ++b) {
        const int n = history[3 * b];
        MF_REQUIRE(n >= 0, "whisper_decoder_choose: sequence %d has sampled %d tokens", b, n);
        for (int i = 1; i <= std::min(n, 2); ++i)
            MF_REQUIRE(history[3 * b + i] >= 0 && history[3 * b + i] < h->n_vocab, "whisper_decoder_choose: sequence %d history token %d is outside the vocabulary (%d)",
                       b, history[3 * b + i], h->n_vocab);
    }
    hipStream_t s = (hipStream_t)stream;
    // scratch of its own: [0, 3B) history, then length, done, chosen, sampled count, output slot (B each) and the log-probabilities.  The handle's decode state is not touched
    int* d = nullptr;
    MF_HIP(hipMalloc((void**)&d, (size_t)9 * batch * sizeof(int)));
    std::vector<int> host((size_t)9 * batch, 0);
    std::copy(history, history + 3 * batch, host.begin());
    // the kernel adds to the sum: the sequences that run start from 0, a done one keeps the log-probability the caller gave
    for (int b = 0; b < batch; ++b) {
        host[4 * batch + b] = done[b] != 0;
        host[5 * batch + b] = tokens[b];
        const float lp0 = done[b] ? logprobs[b] : 0.f;
        std::memcpy(host.data() + 8 * batch + b, &lp0, sizeof(float));
    }
    hipError_t e = hipMemcpyAsync(d, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) {
        const ChooseArgs c{logits, h->n_vocab, suppress_mask, eot, INT_MAX, INT_MAX, 0, d + 3 * batch, d + 4 * batch, d + 5 * batch, d + 6 * batch,
                           reinterpret_cast<float*>(d + 8 * batch), d + 7 * batch, 1};
        hipLaunchKernelGGL(k_dec_choose_rules, dim3(batch), dim3(256), 0, s, rule_args(c, r, d));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), d, host.size() * sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d);
    MF_HIP(e);
    for (int b = 0; b < batch; ++b) { done[b] = host[4 * batch + b]; tokens[b] = host[5 * batch + b]; }
    std::memcpy(logprobs, host.data() + 8 * batch, batch * sizeof(float));
    return MF_OK;
}

extern "C" int mf_whisper_decoder_cache_read(const void* handle, int layer, int seq, float* k, float* v, int* len) {
    const mf_whisper_decoder* h = static_cast<const mf_whisper_decoder*>(handle);
    MF_REQUIRE(h && k && v && len, "whisper_decoder_cache_read: null argument");
    MF_REQUIRE(layer >= 0 && layer < h->n_layer && seq >= 0 && seq < h->max_batch, "whisper_decoder_cache_read: layer %d / sequence %d out of range", layer, seq);
    MF_HIP(hipDeviceSynchronize());
    const size_t n = (size_t)h->n_ctx * h->C;
    MF_HIP(hipMemcpy(k, h->layers[layer].kc + seq * n, n * sizeof(float), hipMemcpyDeviceToHost));
    MF_HIP(hipMemcpy(v, h->layers[layer].vc + seq * n, n * sizeof(float), hipMemcpyDeviceToHost));
    MF_HIP(hipMemcpy(len, h->len + seq, sizeof(int), hipMemcpyDeviceToHost));
    return MF_OK;
}

extern "C" void mf_whisper_decoder_destroy(void* handle) { delete static_cast<mf_whisper_decoder*>(handle); }
