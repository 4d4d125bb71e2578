// Which implicit-GEMM configuration a layer launches: the rules of a tuning-table entry, the cost model behind mf_conv_pick_tile, the tuning table and its cache,
// and the measurement that fills it (mf_conv_tune).  mf_conv_resolve (mf_conv_launch.hip) turns the pick into what launches.
#include "mf_conv.h"
#include <dlfcn.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <set>
#include <string>

const ConvForce& mf_conv_force() {
    static const ConvForce f = [] {
        const char *t = getenv("MF_FORCE_TILE"), *s = getenv("MF_FORCE_SPLIT"), *l = getenv("MF_FORCE_LD");
        int bm = 0, bn = 0;
        return ConvForce{t || s || l, t && sscanf(t, "%dx%d", &bm, &bn) == 2 ? bm * 1000 + bn : 0, s ? atoi(s) : 0, l ? atoi(l) : -1};
    }();
    return f;
}

bool mf_conv_tuned_valid(const ConvTuned& c, int precision, int act) {
    bool tile_ok = false;
    for (const IgemmTile& t : MF_IGEMM_TILES) tile_ok |= t.tunable && c.tile.bm == t.bm && c.tile.bn == t.bn && c.tile.wgm == t.wgm && c.tile.wgn == t.wgn;
    const char* why = nullptr;
    if (!tile_ok) why = "tile not compiled";
    else if (c.tile.nsplit < 1 || c.tile.nsplit > 16) why = "split outside 1 .. 16";
    else if (!(c.ld == -1 || c.ld == 0 || c.ld == 2 || c.ld == 3 || c.ld == 4)) why = "no such operand path";
    else if ((c.ld == 3 || c.ld == 4) && c.tile.wgm * c.tile.wgn != 4) why = "the producer-wave path (ld 3 / 4) needs a 4-wave tile";
    else if (c.tile.bn == 80 && c.ld != 3 && c.ld != 4) why = "the 128 x 80 tile runs on the producer-wave kernels (ld 3 / 4) only";
    // the producer-wave kernels exist in bf16x3 only (launch_prec / launch_pw_only): in bf16 such an entry would fail at launch
    else if ((c.ld == 3 || c.ld == 4 || c.tile.bn == 80) && precision != MF_PREC_BF16X3) why = "the producer-wave kernels (ld 3 / 4, the 128 x 80 tile) are bf16x3 only";
    // the GEGLU epilogue pairs a wave's value and gate fragments: the 80-channel tile's five fragments per wave do not pair (mf_tile80_ok)
    else if (c.tile.bn == 80 && act == 5) why = "the 128 x 80 tile cannot pair GEGLU value / gate fragments";
    if (why) mf_set_error("conv: configuration %dx%d (%d x %d waves) split %d ld %d: %s", c.tile.bm, c.tile.bn, c.tile.wgm, c.tile.wgn, c.tile.nsplit, c.ld, why);
    return !why;
}

// Tile / split-K selection by a cost model of the loop (profiles/r01_igemm_bandwidth_study.md): a workgroup streams
// (BM + BN) x K/S operand elements at min(per-CU DMA rate, chip L2->LDS rate / resident workgroups); workgroups run in
// rounds of (256 CUs x resident per CU); a split pays the fp32 partial round trip and one more launch.  Constants were
// fitted to 386 measured (shape, tile, split) points of the MuseTalk UNet / VAE layers (mean loss vs the best measured
// configuration 3.5 %).
ConvTile mf_conv_pick_tile(const ConvPlan* p, int batch) {
    const ConvForce& force = mf_conv_force();
    auto it = p->tuned.find(batch);
    if (!force.any && it != p->tuned.end()) return it->second.tile;
    const int M = batch * p->Hq * p->Wq, N = p->d.cout, ktm = kt_min(p);
    double kt_sum = 0;
    for (int ph = 0; ph < p->nphase; ++ph) kt_sum += p->ph[ph].KT;
    ConvTile t;
    if (N <= 16) t = {128, 16, 4, 1, 1};
    else if (N <= 32) t = {128, 32, 4, 1, 1};
    else if (M <= 16 && p->d.act != 5 && !p->q) t = {16, 64, 1, 4, 1};   // (its 16-channel wave tile cannot pair GEGLU blocks; no f16 + FP6 form)
    else t = {64, 64, 2, 2, 1};
    const bool modelled = N > 32 && (M > 16 || p->d.act == 5 || p->q);
    const int force_tile = force.tile, fs = force.split ? std::max(1, std::min(std::min(ktm, force.split), 16)) : 0;
    if (modelled) {
        const double planes = p->precision != MF_PREC_BF16 ? 2.0 : 1.0;
        const double Kavg = kt_sum / p->nphase * 64.0;
        const double PW = 46e9, CHIP = 10.5e12, EPI_BW = 2.5e12, EPI_FIX = 6e-6, WG_FIX = 2e-6;
        double best = 1e30;
        for (const IgemmTile& c : MF_IGEMM_TILES) {
            if (!c.tunable) continue;
            if (force_tile && (c.bm != force_tile / 1000 || c.bn != force_tile % 1000)) continue;
            if (c.bn == 80 && (force_tile != 128080 || !mf_tile80_ok(p))) continue;   // measured only (mf_conv_tune), never the model's pick
            if (c.bn == 128 && c.bm == 128 && N % 128) continue;
            for (int S0 : MF_CONV_SPLITS) {
                const int S = fs ? fs : S0;
                if (S > ktm || (fs && S0 > 1)) continue;                        // (a forced split is priced once)
                if (c.bm == 256 && Kavg / S < 512 && !force_tile) continue;    // too few K tiles to amortise a 256-wide prologue / epilogue
                const double wg = (double)cdiv(M, c.bm) * cdiv(N, c.bn) * p->nphase * S;
                const double slots = 256.0 * c.resident;
                const double rate = std::min(PW, CHIP / std::min(wg, slots));
                const double bytes_wg = (double)(c.bm + c.bn) * (Kavg / S) * 2.0 * planes;
                double cost = std::ceil(wg / slots) * (bytes_wg / rate + WG_FIX);
                if (S > 1) cost += S * (double)M * N * p->nphase * 4.0 * 2.0 / EPI_BW + EPI_FIX;
                if (cost < best) { best = cost; t = {c.bm, c.bn, c.wgm, c.wgn, S}; }
            }
        }
        return t;
    }
    const int nt = cdiv(M, t.bm) * cdiv(N, t.bn) * p->nphase;
    if (nt < 256 && ktm >= 2) t.nsplit = std::max(1, std::min(std::min(ktm, cdiv(512, nt)), 16));
    if (fs) t.nsplit = fs;
    return t;
}

namespace {
// reads a buffer (pulls it into the Infinity Cache the way the producing layer leaves it there)
__global__ __launch_bounds__(256) void k_tune_touch(const uint4* __restrict__ p, int64_t n, unsigned* sink) {
    unsigned acc = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) { const uint4 v = p[i]; acc += v.x ^ v.y ^ v.z ^ v.w; }
    if (acc == 0x9e3779b9u) *sink = acc;
}

// Measured configurations by layer signature: layers of one shape share a measurement (the UNet's 188 GEMMs are ~60 distinct shapes).
// Where they come from, in this order:
//   MF_TUNE_CACHE=<file>   read at first use; every new measurement (mf_*_tune) is appended to it
//   <library dir>/tune/gfx950.txt   the table shipped with the library for the BASELINE.json shapes (tools/make_tune_cache.py on an MI355X): with it a
//                          process launches the same configurations -- hence the same fp32 summation order, the same output bits -- on every box
// A forward NEVER measures (tuning inside run() stalled a serving loop for seconds at every new session count): it only looks its
// layers up here; a shape that is not in the table runs the cost model's pick.  Measuring is an explicit call (mf_unet_tune, mf_vae_tune,
// mf_wav2lip_tune, mf_net_tune), or, for development, MF_AUTOTUNE=1 (measure on the first forward at a batch size, as rounds 1-2 did).
// bm == 0 records "the cost model's pick stays".
std::string shipped_tune_table() {
    Dl_info info{};
    if (!dladdr(reinterpret_cast<const void*>(&mf_conv_tune), &info) || !info.dli_fname) return "";
    std::string path = info.dli_fname;
    const size_t slash = path.rfind('/');
    return (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/tune/gfx950.txt";
}
std::map<std::string, ConvTuned>& tune_cache() {
    static std::map<std::string, ConvTuned> cache;
    static bool loaded = false;
    if (!loaded) {
        loaded = true;
        const char* env = getenv("MF_TUNE_CACHE");
        const std::string path = env ? std::string(env) : shipped_tune_table();
        // Entries are validated on load: a stale or hand-edited file must not put a tile the library no longer compiles, an impossible split or an
        // operand path that was removed into launch selection.  Keys carry the kernel generation ("g950k4": tile list / operand paths of round 4's library).
        // KEEP IN SYNC with loader_rejects() in tests/test_tune_table.py, which holds the shipped table to these rules.
        auto valid = [](const std::string& k, const ConvTuned& c) {
            if (k.rfind("g950k4:", 0) != 0) return false;
            if (c.tile.bm == 0) return true;                                          // "the cost model's pick stays"
            // a compiled tile, a split of 1 .. 16, an operand path that exists and that the tile runs -- in the key's precision (the producer-wave kernels,
            // hence ld 3 / 4 and the 128 x 80 tile, are bf16x3 only) and with the key's activation (no 128 x 80 GEGLU).  ld 3 / 4 (round 5's producer-wave path) are additions to generation k4: every older
            // entry still names a kernel this library has
            int f[14] = {0};   // precision, batch, cin, cout, kh, kw, stride_h, stride_w, pad_h, pad_w, transposed, output_padding, residual, act
            if (sscanf(k.c_str() + 7, "%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d", f, f + 1, f + 2, f + 3, f + 4, f + 5, f + 6, f + 7, f + 8, f + 9, f + 10, f + 11,
                       f + 12, f + 13) != 14) return false;
            return mf_conv_tuned_valid(c, f[0], f[13]);
        };
        int dropped = 0;
        if (FILE* f = path.empty() ? nullptr : fopen(path.c_str(), "r")) {
            char key[256];
            ConvTuned c{};
            while (fscanf(f, "%255s %d %d %d %d %d %d", key, &c.tile.bm, &c.tile.bn, &c.tile.wgm, &c.tile.wgn, &c.tile.nsplit, &c.ld) == 7) {
                if (valid(key, c)) cache[key] = c; else ++dropped;
            }
            fclose(f);
            if (dropped) fprintf(stderr, "[mere-fusion_amd] tuning table %s: %d entries ignored (other kernel generation or invalid configuration)\n", path.c_str(), dropped);
        } else {
            // said once: without a table every layer runs the cost model's pick, and frames are no longer bit-identical from box to box
            fprintf(stderr, "[mere-fusion_amd] no tuning table (%s): implicit-GEMM layers use the cost model's launch configurations\n", path.empty() ? "library path unknown" : path.c_str());
        }
    }
    return cache;
}
void tune_cache_store(const std::string& key, const ConvTuned& c) {
    tune_cache()[key] = c;
    if (const char* path = getenv("MF_TUNE_CACHE")) {
        if (FILE* f = fopen(path, "a")) {
            fprintf(f, "%s %d %d %d %d %d %d\n", key.c_str(), c.tile.bm, c.tile.bn, c.tile.wgm, c.tile.wgn, c.tile.nsplit, c.ld);
            fclose(f);
        }
    }
}
bool tunable_layer(const ConvPlan* p, int batch) {
    if (p->halo || p->up_hi || mf_conv_force().any) return false;                                // halo-kernel layers keep their own tile choice
    const int M = batch * p->Hq * p->Wq, N = p->d.cout;
    return !(N <= 32 || (M <= 16 && p->d.act != 5 && !p->q));                         // the narrow special tiles have no alternatives
}
ConvTuned split_clamped(const ConvPlan* p, ConvTuned c) {
    c.tile.nsplit = std::max(1, std::min(c.tile.nsplit, kt_min(p)));                    // (a split deeper than the layer's K tiles cannot launch)
    return c;
}
std::string tune_key(const ConvPlan* p, const ActView& in, int batch) {
    char keybuf[256];
    snprintf(keybuf, sizeof(keybuf), "g950k4:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d:%d", p->precision, batch, p->d.cin, p->d.cout, p->d.kh, p->d.kw, p->d.stride_h, p->d.stride_w,
             p->d.pad_h, p->d.pad_w, p->d.transposed, p->d.output_padding, p->d.residual, p->d.act, p->d.in_h, p->d.in_w, p->d.upsample, p->d.pad_hi,
             in.buf ? in.buf->C : 0);
    return std::string(keybuf) + (p->out_stats ? ":s" : "");     // a layer that also leaves GroupNorm statistics times (and may pick) differently
}
}  // namespace

bool mf_autotune_enabled() {
    const char* e = getenv("MF_AUTOTUNE");         // (read at every use: tests switch it per case)
    return e && atoi(e) != 0;
}

int mf_conv_tune_lookup(ConvPlan* p, const ActView& in, int batch) {
    if (p->halo && p->alt && !p->q) {
        // a wide halo layer at a batch too small for the fat tiles launches its implicit-GEMM twin: the twin takes the table entry of the layer's signature
        // (same descriptor; the ':s' suffix follows the statistics request the launch will hand over)
        p->alt->out_stats = p->out_stats; p->alt->out_stats_groups = p->out_stats_groups;
        return mf_conv_tune_lookup(p->alt, in, batch);
    }
    if (!tunable_layer(p, batch)) return 0;
    auto it = tune_cache().find(tune_key(p, in, batch));
    if (it == tune_cache().end()) return 0;
    if (it->second.tile.bm > 0) p->tuned[batch] = split_clamped(p, it->second);
    else p->tuned.erase(batch);
    return 1;
}

int mf_conv_pin(ConvPlan* p, int batch, const ConvTuned& c) {
    if (p->halo && p->alt && !p->q) return mf_conv_pin(p->alt, batch, c);          // (as mf_conv_tune_lookup: the wide halo layer's twin takes the entry)
    if (c.tile.bm == 0) { p->tuned.erase(batch); return MF_OK; }
    MF_REQUIRE(!p->halo && !p->up_hi, "conv: this layer runs on a halo-tile or thin kernel: the tuning table does not serve it");
    MF_REQUIRE(tunable_layer(p, batch), "conv: at batch %d this layer runs a narrow special tile (cout <= 32, or <= 16 pixels; or MF_FORCE_* is set): "
               "the tuning table does not serve it", batch);
    if (!mf_conv_tuned_valid(c, p->precision, p->d.act)) return MF_ERR_INVALID;
    p->tuned[batch] = split_clamped(p, c);
    return MF_OK;
}

int mf_conv_tune(ConvPlan* p, const ActView& in, const ActView& out, const ActView& res, int batch, hipStream_t stream) {
    if (p->halo && p->alt && !p->q) {             // (as mf_conv_tune_lookup: the twin is what launches when the fat tiles decline this batch)
        if (mf_halo_w_pick_tile(p->out_h, p->out_w, p->d.cout, batch, p->d.cin).ph || mf_halo_split_count(p, batch)) return MF_OK;
        p->alt->out_stats = p->out_stats; p->alt->out_stats_groups = p->out_stats_groups;
        return mf_conv_tune(p->alt, in, out, res, batch, stream);
    }
    if (!tunable_layer(p, batch)) return MF_OK;
    const std::string key = tune_key(p, in, batch);
    // MF_TUNE_EXTEND=80 (table maintenance): a layer that HAS an entry is measured again, its entry against the tiles of that channel width only (a tile added
    // to the library after the table was made), and the entry is replaced where the new tile is clearly ahead -- minutes instead of the full hour of measurements
    static const int extend_bn = [] { const char* e = getenv("MF_TUNE_EXTEND"); return e ? atoi(e) : 0; }();
    const bool found = mf_conv_tune_lookup(p, in, batch);                             // measured before (this process, MF_TUNE_CACHE, or the shipped table)
    static std::set<std::string> extended;                                            // (layers of one signature share the measurement)
    const bool extend = found && extend_bn == 80 && mf_tile80_ok(p) && extended.insert(key).second;
    if (found && !extend) return MF_OK;
    const bool had_entry = p->tuned.count(batch) != 0;
    const ConvTuned entry = had_entry ? p->tuned[batch] : ConvTuned{ConvTile{0, 0, 0, 0, 0}, -1};
    if (!extend) p->tuned.erase(batch);
    const int M = batch * p->Hq * p->Wq, N = p->d.cout;
    const ConvTile base = mf_conv_pick_tile(p, batch);                                // what the cost model would launch
    const int ktm = kt_min(p);
    hipEvent_t e0, e1;
    MF_HIP(hipEventCreate(&e0)); MF_HIP(hipEventCreate(&e1));
    // In the network a layer finds its INPUT in the Infinity Cache (the previous layer just wrote it) and its WEIGHTS in HBM (3.4 GB of them
    // cycle through per step); timed back to back it would find both warm.  So before every timed launch a 384 MB
    // memset evicts the caches and a read pass brings the input (and residual) planes back.
    const bool cold = true;
    static void* scratch = nullptr;
    static unsigned* sink = nullptr;
    const size_t scratch_bytes = (size_t)384 << 20;
    if (cold && !scratch) { MF_HIP(hipMalloc(&scratch, scratch_bytes)); MF_HIP(hipMalloc(&sink, 4)); }
    auto prepare = [&]() -> int {
        if (!cold) return MF_OK;
        MF_HIP(hipMemsetAsync(scratch, 1, scratch_bytes, stream));
        for (const ActView* v : {&in, &res}) {
            if (!v->buf) continue;
            const int64_t n16 = (int64_t)batch * v->buf->per_batch() * (int64_t)sizeof(bf16_t) / 16;
            hipLaunchKernelGGL(k_tune_touch, dim3(1024), dim3(256), 0, stream, reinterpret_cast<const uint4*>(v->buf->hi), n16, sink);
            if (v->buf->lo) hipLaunchKernelGGL(k_tune_touch, dim3(1024), dim3(256), 0, stream, reinterpret_cast<const uint4*>(v->buf->lo), n16, sink);
        }
        MF_HIP(hipGetLastError());
        return MF_OK;
    };
    auto measure = [&](const ConvTuned& c, float* us) -> int {
        p->tuned[batch] = c;
        int rc = mf_conv_launch(p, in, out, res, batch, stream);                     // warm-up: also sizes the split-K workspace
        if (rc) return rc;
        float best = 1e30f;
        for (int i = 0; i < 3; ++i) {
            if ((rc = prepare())) return rc;
            MF_HIP(hipEventRecord(e0, stream));
            if ((rc = mf_conv_launch(p, in, out, res, batch, stream))) return rc;
            MF_HIP(hipEventRecord(e1, stream));
            MF_HIP(hipEventSynchronize(e1));
            float ms = 0.f;
            MF_HIP(hipEventElapsedTime(&ms, e0, e1));
            best = std::min(best, ms * 1e3f);
        }
        *us = best;
        return MF_OK;
    };
    ConvTuned best_c{base, extend && had_entry ? entry.ld : -1};
    float base_us = 0.f;
    int rc = measure(best_c, &base_us);
    float best_us = base_us;
    // ... and the fastest single-pass configuration beside it: a split-K winner costs a second launch (the combine) on the step's dependent chain, which a
    // layer timed alone does not show, so it has to be clearly ahead of the best configuration without one
    ConvTuned best1_c = best_c;
    float best1_us = base.nsplit > 1 ? 1e30f : base_us;
    for (const IgemmTile& t : MF_IGEMM_TILES) {
        if (rc) break;
        if (!t.tunable) continue;
        if (t.bn == 128 && t.bm == 128 && N % 128) continue;
        if (t.bn == 80 && !mf_tile80_ok(p)) continue;
        if (extend && t.bn != extend_bn) continue;
        if (t.bm >= 256 && M < 256) continue;
        const int64_t nt = (int64_t)cdiv(M, t.bm) * cdiv(N, t.bn) * p->nphase;
        for (int S : MF_CONV_SPLITS) {
            if (S > ktm || (S > 1 && nt >= 1024) || nt * S > 4096) continue;
            if (p->d.act == 5 && t.bn < 32 && S > 1) continue;
            for (int ld : {2, 0, 3, 4}) {
                if (t.wgm * t.wgn == 8 && ld != 0) continue;                        // the 8-wave tiles only have the LDS-DMA loop
                // producer-wave path: bf16x3 only (ld 3: 64-deep stages, ld 4: 32-deep ones)
                if (ld >= 3 && (p->precision != MF_PREC_BF16X3 || p->q || t.bn < 64)) continue;
                if (t.bn == 80 && ld < 3) continue;
                const ConvTuned c{ConvTile{t.bm, t.bn, t.wgm, t.wgn, S}, ld};
                float us = 0.f;
                if ((rc = measure(c, &us))) break;
                if (us < best_us) { best_us = us; best_c = c; }
                if (S == 1 && us < best1_us) { best1_us = us; best1_c = c; }
            }
            if (rc) break;
        }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc) { p->tuned.erase(batch); return rc; }
    const float split_us = best_us;                                                  // (what MF_DEBUG=tune reports beside the single-pass time)
    if (best_c.tile.nsplit > 1 && 0.97f * best1_us <= best_us) { best_c = best1_c; best_us = best1_us; }
    // keep the model's pick unless the measured winner is clearly ahead (event timing of a 10-100 us launch is good to ~1 us)
    if (extend && best_us > 0.97f * base_us) {                                        // the entry stands (nothing is appended)
        if (had_entry) p->tuned[batch] = entry; else p->tuned.erase(batch);
    } else if (best_us > 0.97f * base_us) { p->tuned.erase(batch); tune_cache_store(key, ConvTuned{ConvTile{0, 0, 0, 0, 0}, -1}); }
    else { p->tuned[batch] = best_c; tune_cache_store(key, best_c); }
    static const bool verbose = mf_debug_has("tune");
    if (verbose)
        fprintf(stderr, "[mf_conv_tune] %s M %d N %d K %d: model %dx%d split %d %.1f us -> %s %dx%d split %d ld %d %.1f us (best overall %.1f us, best single-pass %dx%d ld %d %.1f us)\n",
                key.c_str(), M, N, ktm * 64, base.bm, base.bn, base.nsplit, base_us, p->tuned.count(batch) ? "tuned" : "kept", best_c.tile.bm, best_c.tile.bn, best_c.tile.nsplit,
                best_c.ld, best_us, split_us, best1_c.tile.bm, best1_c.tile.bn, best1_c.ld, best1_us);
    return MF_OK;
}
