// The launch path of the convolution engine: which kernel family and configuration a layer runs at a batch (mf_conv_resolve, the ONE place that decides), and the
// launch itself -- validate, resolve, then one short function per family.  Host code only: the implicit-GEMM kernels and their two launchers (mf_igemm_launch,
// mf_splitk_combine) are in mf_conv.hip, the halo and thin kernels in mf_conv_halo.hip, mf_conv_halo2.hip and mf_conv_thin.hip.
#include "mf_conv.h"
#include <algorithm>

// Channel-slice split of the fat 256-channel halo tile for a wide layer whose map gives too few patches at this batch (0 = no split).
int mf_halo_split_count(const ConvPlan* p, int batch) {
    if (!p->halo || !p->alt || p->d.cout % 256 || p->d.cin < 512) return 0;
    const int base = batch * cdiv(p->out_h, 16) * cdiv(p->out_w, 16) * (p->d.cout / 256);
    if (base < 64) return 0;          // (at 32 patches x tiles the split measured +5 % / -2 % on two shapes: not worth the second pass)
    for (int cand : {2, 4, 8})
        if (base * cand >= 256 && p->n_slices / cand >= 2) return cand;
    return 0;
}

// Channel-slice split of the f16 + FP6 tile (16 x 16 pixels x 128 channels) for a layer with fewer tiles than CUs at this batch (1 = no split)
int mf_q_split_count(const ConvPlan* p, int batch) {
    if (!p->q || !p->halo) return 1;
    const int base = batch * cdiv(p->out_h, 16) * cdiv(p->out_w, 16) * (p->d.cout / 128);
    if (base >= 256) return 1;
    int best = 1;
    for (int cand : {2, 4, 8}) {
        if (p->n_slices / cand < 2) break;
        best = cand;
        if (base * cand >= 256) break;
    }
    return best;
}

int mf_conv_resolve(const ConvPlan* p, int batch, int tokens, int stats_groups, ConvLaunchCfg* c) {
    *c = ConvLaunchCfg{MF_CONV_FAMILY_IGEMM, ConvTile{0, 0, 0, 0, 1}, -1, 0, p->nphase, MF_CONV_STATS_NONE, false};
    const int groups = stats_groups > 0 ? stats_groups : 0;
    // split-K / channel-split combines that leave the statistics (mf_splitk_combine)
    const bool combine_stats = groups && p->d.act != 5 && p->d.cout % 4 == 0 && p->d.cout % groups == 0 && groups <= 64;
    const int halo_ck = p->precision != MF_PREC_BF16 ? 32 : 64;
    auto stats = [&](int src) { c->stats = groups ? src : MF_CONV_STATS_NONE; return MF_OK; };
    if (p->thin) {
        c->family = MF_CONV_FAMILY_THIN; c->tile = ConvTile{p->out_h, p->d.cout, 1, 1, 1}; c->bk = p->d.cin <= 8 ? 8 : 16;
        return stats(MF_CONV_STATS_PASS);
    }
    const bool q_gn = groups && p->d.cout % groups == 0 && (p->d.cout / groups == 4 || p->d.cout / groups == 8 || p->d.cout / groups == 16);
    if (p->halo) {
        c->bk = halo_ck;
        if (p->q) {
            const int ns = mf_q_split_count(p, batch);
            c->family = MF_CONV_FAMILY_F16Q; c->tile = ConvTile{16, 128, 4, 2, ns};
            return stats(ns > 1 ? (combine_stats ? MF_CONV_STATS_COMBINE : MF_CONV_STATS_PASS) : q_gn ? MF_CONV_STATS_EPILOGUE : MF_CONV_STATS_PASS);
        }
        const HaloTile tw = mf_halo_w_pick_tile(p->out_h, p->out_w, p->d.cout, batch, p->d.cin);
        if (tw.ph) {
            c->family = MF_CONV_FAMILY_HALO_W; c->tile = ConvTile{tw.ph, tw.bn, tw.wgm, tw.wgn, 1};
            return stats(MF_CONV_STATS_PASS);
        }
        if (const int ns = mf_halo_split_count(p, batch)) {
            c->family = MF_CONV_FAMILY_HALO_W_SPLIT; c->tile = ConvTile{16, 256, 2, 4, ns};
            return stats(combine_stats ? MF_CONV_STATS_COMBINE : MF_CONV_STATS_PASS);
        }
        if (p->alt) {
            const int rc = mf_conv_resolve(p->alt, batch, 0, stats_groups, c);
            c->family = MF_CONV_FAMILY_TWIN;
            return rc;
        }
        const HaloTile t = mf_halo_pick_tile(p->out_h, p->out_w, p->d.cout, batch, p->d.cin);
        c->family = MF_CONV_FAMILY_HALO; c->tile = ConvTile{t.ph, t.bn, t.wgm, t.wgn, 1};
        return stats(MF_CONV_STATS_PASS);
    }
    if (p->up_hi && p->q) {
        c->family = MF_CONV_FAMILY_F16Q; c->tile = ConvTile{16, 128, 4, 2, 1}; c->bk = 32; c->nphase = 4;
        return stats(q_gn ? MF_CONV_STATS_EPILOGUE : MF_CONV_STATS_PASS);
    }
    // ---- implicit GEMM
    const bool x3 = p->precision != MF_PREC_BF16;
    const int pick = p->pick_batch > 0 ? p->pick_batch : batch;   // (ConvPlan::pick_batch: one K summation order for every batch a handle serves)
    ConvTile tc = mf_conv_pick_tile(p, pick);
    int ld = -1;
    const ConvForce& force = mf_conv_force();
    auto it = p->tuned.find(pick);
    if (it != p->tuned.end()) { ld = it->second.ld; c->pinned = !force.any; }
    if (force.ld >= 0 && !(force.ld >= 3 && (!x3 || p->q || tc.wgm * tc.wgn != 4 || tc.bn < 64 || tc.bm < 64))) ld = force.ld;   // (measurement, with MF_FORCE_TILE / MF_FORCE_SPLIT)
    const int Wq_eff = tokens > 0 ? tokens : p->Wq;
    const int M = pick * p->Hq * Wq_eff;
    if (tokens > 0) {
        // the cost model priced the full sequence: re-balance the split for the rows actually computed
        const int nt = cdiv(M, tc.bm) * cdiv(p->d.cout, tc.bn);
        tc.nsplit = nt >= 256 ? 1 : std::max(1, std::min(std::min(kt_min(p), cdiv(512, nt)), 16));
        if (tc.bm > 128 && M <= 256) { tc.bm = 64; tc.bn = 64; tc.wgm = 2; tc.wgn = 2; }
        if (p->d.act == 5 && tc.bn < 32) tc.nsplit = 1;
    }
    // the split-K partials ([split][B][Ho][Wo][N], unpadded rows) are written and combined in float4 channel quads: with a cout that is not a multiple
    // of 4 the last quad of a row would overwrite the next pixel's first channels (and run past the workspace at the last one), and the combine would
    // drop the row's last channels.  Such a layer takes the single-pass epilogue.
    if (p->d.cout % 4) tc.nsplit = 1;
    c->tile = tc;
    // the operand path and stage depth launch_prec / launch_cfg / launch_pw_only take for this (tile, ld)
    const bool four = tc.wgm * tc.wgn == 4;
    const bool pw = ld == 3 || ld == 4;
    MF_REQUIRE(!pw || (x3 && !p->q && four && tc.bm >= 64 && tc.bn >= 64), "conv: no producer-wave kernel (ld %d) for tile %dx%d in this precision", ld, tc.bm, tc.bn);
    MF_REQUIRE(tc.bn != 80 || pw, "conv: the %dx%d tile has only the bf16x3 producer-wave kernels (ld 3 / 4)", tc.bm, tc.bn);
    c->ld = pw ? ld : (four && (ld >= 0 ? ld : 2) == 2) ? 2 : 0;
    c->bk = p->q ? (four ? 64 : 32) : pw ? (ld == 3 ? 64 : 32) : x3 ? (four ? 64 : 32) : 64;
    if (groups && tokens == 0) {
        if (tc.nsplit > 1) return stats(combine_stats ? MF_CONV_STATS_COMBINE : MF_CONV_STATS_PASS);
        // in the epilogue: 4-wave tiles (k_conv_igemm's ST) whose pixel tile lies inside one sample
        if (p->d.act != 5 && p->d.cout % groups == 0 && groups <= 64 && four && tc.bm * tc.bn < 128 * 128 && (p->Hq * Wq_eff) % tc.bm == 0)
            return stats(MF_CONV_STATS_EPILOGUE);
    }
    return stats(MF_CONV_STATS_PASS);
}

namespace {

// The split-K / channel-split workspace holds at least `floats` on return.  Growth is only reached on an eager (un-captured) launch: the first forward at a batch
// size runs eagerly.  The outgrown buffer is retired, not freed: graphs captured at other batch sizes still hold its address (ConvPlan::retired).
int ensure_workspace(ConvPlan* p, int64_t floats) {
    if (floats <= p->ws_cap) return MF_OK;
    if (p->ws) { p->retired.push_back(p->ws); p->ws = nullptr; p->ws_cap = 0; }
    MF_HIP(hipMalloc(&p->ws, floats * sizeof(float)));
    p->ws_cap = floats;
    return MF_OK;
}

// one launch: the views, the resolved configuration, and whether a kernel of the launch left the GroupNorm statistics
struct Launch {
    ConvPlan* p; const ActView &in, &out, &res; int batch, tokens; hipStream_t stream;
    bool x3;                      // two planes per tensor (bf16x3, and the f16 + FP6 format)
    ConvLaunchCfg cfg; bool* stats_done;
};

int launch_thin(const Launch& l) {
    const ConvPlan* p = l.p;
    const ActBuf &ib = *l.in.buf, &ob = *l.out.buf;
    MF_REQUIRE(!l.res.buf && ib.halo >= p->d.pad_h, "thin conv: no residual, and the input buffer's zero ring must cover the padding");
    ThinArgs ta{};
    ta.x_hi = ib.hi + l.in.coff; ta.x_lo = l.x3 ? ib.lo + l.in.coff : nullptr;
    ta.w = p->w_hi; ta.bias = p->bias;
    ta.batch = l.batch; ta.H = p->out_h; ta.W = p->out_w; ta.N = p->d.cout;
    ta.pad = p->d.pad_h; ta.in_halo = ib.halo; ta.in_hp = ib.Hp(); ta.in_wp = ib.Wp(); ta.x_ld = ib.C; ta.xb = ib.per_batch();
    ta.y_hi = ob.hi + view_origin(l.out); ta.y_lo = l.x3 ? ob.lo + view_origin(l.out) : nullptr;
    ta.yb = ob.per_batch(); ta.yi = ob.Wp() * ob.C; ta.yj = ob.C;
    ta.act = p->d.act;
    return mf_thin_launch(ta, p->d.kh, p->d.stride_h, p->d.cin, p->d.cout, l.x3, l.stream);
}

// the input side of a halo-tile launch, which addresses the input itself
void set_halo_input(HaloArgs& ha, const Launch& l) {
    const ActBuf& ib = *l.in.buf;
    ha.x_hi = ib.hi + l.in.coff; ha.x_lo = l.x3 ? ib.lo + l.in.coff : nullptr;
    ha.bias = l.p->bias;
    ha.batch = l.batch; ha.N = l.p->d.cout; ha.Npad = l.p->Npad; ha.n_slices = l.p->n_slices;
    ha.in_halo = ib.halo; ha.in_hp = ib.Hp(); ha.in_wp = ib.Wp(); ha.x_ld = ib.C; ha.xb = ib.per_batch();
    ha.act = l.p->d.act;
}

// f16 + FP6 tiles: 16-byte epilogue stores (lane pairs exchange halves), and the GroupNorm statistics from the epilogue where the group width allows
// (other widths: k_gn_stats behind the conv)
void set_q_epilogue(HaloArgs& ha, const Launch& l) {
    ha.wide_store = l.out.coff % 8 == 0 && l.out.buf->C % 8 == 0 && l.p->d.cout % 32 == 0;
    if (l.cfg.stats == MF_CONV_STATS_EPILOGUE) {
        ha.gn_out = l.p->out_stats; ha.gn_out_cpg = l.p->d.cout / l.p->out_stats_groups; ha.gn_out_groups = l.p->out_stats_groups;
        *l.stats_done = true;
    }
}

// A map too small to give every CU a 16 x 16 patch (the VAE's 512-channel 32 x 32 levels at batch 8: 32 - 64 patches x channel tiles): the LDS-weights tile with
// the channel slices split over blockIdx.y, fp32 partial tiles combined by k_splitk_epilogue[_stats] -- the same two-pass scheme as the implicit GEMM's split-K,
// with half its L2 -> LDS bytes.  Serves the bf16x3 / bf16 256-channel tile (MF_HALO_SPLIT=0: off) and the f16 + FP6 tile alike; in the split form
//   - the residual is always added by the combine, from global memory -- also where it is the layer's own input, which the unsplit 256-channel tile would take from
//     its LDS halo image (the f16 + FP6 path has refused such a layer before it gets here);
//   - the partial launch never writes GroupNorm statistics: the combine leaves them where it can.
int launch_halo_split(const Launch& l, const HaloArgs& ha, const HaloTile& tile) {
    ConvPlan* p = l.p;
    const int ns = l.cfg.tile.nsplit;
    const int64_t per_split = (int64_t)l.batch * p->out_h * p->out_w * p->d.cout;
    if (const int rc = ensure_workspace(p, per_split * ns)) return rc;
    HaloArgs hs = ha;
    hs.ws = p->ws; hs.ws_split = per_split; hs.nsplit = ns;
    hs.res_from_halo = 0;
    hs.gn_out = nullptr;
    if (const int rc = mf_halo_w_launch(hs, tile, l.x3, l.stream)) return rc;
    ConvArgs e{};
    e.ws = p->ws; e.ws_split = per_split; e.bias = p->bias; e.N = p->d.cout; e.act = p->d.act;
    e.y_hi = ha.y_hi; e.y_lo = ha.y_lo; e.yb = ha.yb; e.yi = ha.yi; e.yj = ha.yj;
    if (l.res.buf) set_residual(e, l.res, l.x3);
    return mf_splitk_combine(e, ns, l.batch, p->out_h, p->out_w, p->out_stats, p->out_stats_groups, l.stats_done, l.stream);
}

// 3x3 s1 p1 on the halo-tile kernels: register-weights tiles (HALO), LDS-weights tiles (HALO_W, and the f16 + FP6 format's one kernel, the 8-wave
// 16 x 16 x 128-channel tile), and their channel-split forms
int launch_halo(const Launch& l) {
    const ConvPlan* p = l.p;
    const ActBuf& ob = *l.out.buf;
    HaloArgs ha{};
    ha.q = p->q ? 1 : 0;
    set_halo_input(ha, l);
    ha.w_hi = p->w_hi; ha.w_lo = p->w_lo;
    ha.H = p->out_h; ha.W = p->out_w;
    ha.y_hi = ob.hi + view_origin(l.out); ha.y_lo = l.x3 ? ob.lo + view_origin(l.out) : nullptr;
    ha.yb = ob.per_batch(); ha.yi = ob.Wp() * ob.C; ha.yj = ob.C;
    if (l.res.buf) {
        MF_REQUIRE(l.res.buf->H == p->out_h && l.res.buf->W == p->out_w && l.res.C == p->d.cout, "conv: residual view does not match the output");
        if (l.res.buf == l.in.buf && l.res.coff == l.in.coff && p->d.cin == p->d.cout) ha.res_from_halo = 1;   // the residual is the input itself (conv.py:17-18): read it from LDS
        else set_residual(ha, l.res, l.x3);
    }
    if (l.cfg.family == MF_CONV_FAMILY_F16Q) {
        MF_REQUIRE(!ha.res_from_halo, "conv (f16q): residual-from-input is not built for this format");
        set_q_epilogue(ha, l);
    }
    const HaloTile tile{l.cfg.tile.bm, l.cfg.tile.bn, l.cfg.tile.wgm, l.cfg.tile.wgn};
    if (l.cfg.tile.nsplit > 1) return launch_halo_split(l, ha, tile);
    return l.cfg.family == MF_CONV_FAMILY_HALO ? mf_halo_launch(ha, tile, l.x3, l.stream) : mf_halo_w_launch(ha, tile, l.x3, l.stream);
}

// upsample + 3x3 in the f16 + FP6 format: four launches of the 16 x 16 x 128-channel tile, phase (py, px) writes output pixels (2i + py, 2j + px)
int launch_q_upsample(const Launch& l) {
    const ConvPlan* p = l.p;
    const ActBuf &ib = *l.in.buf, &ob = *l.out.buf;
    MF_REQUIRE(ib.halo >= 1 && !l.res.buf, "conv (f16q): upsample path needs an input halo and no residual");
    HaloArgs ha{};
    ha.q = 1;
    set_halo_input(ha, l);
    ha.H = p->d.in_h; ha.W = p->d.in_w;
    ha.yb = ob.per_batch(); ha.yi = 2 * ob.Wp() * ob.C; ha.yj = 2 * ob.C;
    set_q_epilogue(ha, l);                                     // (statistics: every phase adds its quarter of the pixels)
    const int64_t per_phase = (int64_t)p->n_slices * 4 * p->Npad * 32;
    for (int ph = 0; ph < 4; ++ph) {
        const int64_t yb0 = view_origin(l.out) + ((int64_t)(ph >> 1) * ob.Wp() + (ph & 1)) * ob.C;
        ha.y_hi = ob.hi + yb0; ha.y_lo = ob.lo + yb0;
        ha.w_hi = p->up_hi + ph * per_phase; ha.w_lo = p->up_lo + ph * per_phase;
        if (const int rc = mf_halo_w_launch(ha, HaloTile{16, 128, 4, 2}, true, l.stream, ph)) return rc;
    }
    return MF_OK;
}

int launch_igemm(const Launch& l) {
    ConvPlan* p = l.p;
    const ActView &in = l.in, &out = l.out, &res = l.res;
    const ActBuf &ib = *in.buf, &ob = *out.buf;
    const bool x3 = l.x3; const int batch = l.batch, tokens = l.tokens;
    const int Wq_eff = tokens > 0 ? tokens : p->Wq;       // output positions per batch item this launch computes
    const int out_w_eff = tokens > 0 ? tokens : p->out_w;
    ConvArgs a{};
    a.x_hi = ib.hi + in.coff; a.x_lo = x3 ? ib.lo + in.coff : nullptr;
    a.w_hi = p->w_hi; a.w_lo = p->w_lo; a.bias = p->bias; a.goff = p->goff;
    a.M = batch * p->Hq * Wq_eff; a.N = p->d.cout; a.Npad = p->Npad;
    a.HqWq = p->Hq * Wq_eff; a.Wq = Wq_eff;
    mf_fastdiv((uint32_t)a.HqWq, &a.dv_hw_mul, &a.dv_hw_shr); mf_fastdiv((uint32_t)a.Wq, &a.dv_w_mul, &a.dv_w_shr);
    a.xb = ib.per_batch(); a.xi = p->in_step_h * ib.Wp() * ib.C; a.xj = p->in_step_w * ib.C;
    a.y_hi = ob.hi + view_origin(out); a.y_lo = x3 ? ob.lo + view_origin(out) : nullptr;
    a.yb = ob.per_batch(); a.yi = p->out_step * ob.Wp() * ob.C; a.yj = p->out_step * ob.C;
    if (res.buf) {
        MF_REQUIRE(res.buf->H == p->out_h && res.buf->W == p->out_w && res.C == p->d.cout && p->out_step == 1, "conv: residual view does not match the output");
        set_residual(a, res, x3);
    }
    a.act = p->d.act;
    a.res_after_act = p->d.residual == 2;
    if (p->ln_cs) {
        MF_REQUIRE(p->ln_in && !res.buf && (p->d.act == 0 || p->d.act == 5), "conv: a LayerNorm-folded layer needs its statistics buffer, no residual and act 0 or GEGLU");
        a.ln_in = p->ln_in; a.ln_cs = p->ln_cs; a.ln_inv_c = 1.f / (float)p->d.cin; a.ln_eps = p->ln_eps;
    }
    if (p->ln_out) {
        MF_REQUIRE(p->d.act != 5 && p->nphase == 1 && p->out_step == 1, "conv: LayerNorm statistics come from plain 1x1 producers");
        a.ln_out = p->ln_out;
    }
    const int n_out = p->d.act == 5 ? p->d.cout / 2 : p->d.cout;
    a.wide_store = out.coff % 8 == 0 && ob.C % 8 == 0 && n_out % 8 == 0 && p->d.cout % 16 == 0;
    a.goff_total = p->goff_total;
    int goff_max = 0;
    for (int ph = 0; ph < p->nphase; ++ph) {
        a.ph[ph] = p->ph[ph];
        a.ph[ph].y_off = ((int64_t)p->phase_oy[ph] * ob.Wp() + p->phase_ox[ph]) * ob.C;
        a.ph[ph].ws_off = ((int64_t)p->phase_oy[ph] * p->out_w + p->phase_ox[ph]) * a.N;
        goff_max = std::max(goff_max, p->ph[ph].ngroups);
    }

    const ConvTile tc = l.cfg.tile;          // tile, split and operand path as mf_conv_resolve settled them
    a.ld = l.cfg.ld;
    a.tiles_m = cdiv(a.M, tc.bm); a.tiles_n = cdiv(a.N, tc.bn);
    // XCD tile order by which operand is heavier: weights N x K vs the input tensor M x Cin (both x planes)
    const int64_t w_elems = (int64_t)a.Npad * p->ph[0].KT * 64 * p->nphase, x_elems = (int64_t)batch * ib.H * ib.W * in.C;
    a.m_fastest = w_elems > x_elems;
    static const bool dbg_times = mf_debug_has("times");
    if (dbg_times) a.dbg = mf_conv_debug_times_buffer((int64_t)a.tiles_m * a.tiles_n * tc.nsplit * p->nphase);
    if (tc.nsplit > 1) {
        // fp32 partial tiles [split][B][Ho][Wo][N]; combined by mf_splitk_combine below
        const int64_t per_split = (int64_t)batch * p->out_h * out_w_eff * a.N;
        if (const int rc = ensure_workspace(p, per_split * tc.nsplit)) return rc;
        a.ws = p->ws; a.ws_split = per_split;
        a.wsb = (int64_t)p->out_h * out_w_eff * a.N;
        a.wsi = p->out_step * out_w_eff * a.N; a.wsj = p->out_step * a.N;
    }
    if (p->out_stats && p->d.act != 5 && p->d.cout % p->out_stats_groups == 0 && p->out_stats_groups <= 64 && tokens == 0) {
        a.gn_out_cpg = p->d.cout / p->out_stats_groups; a.gn_out_groups = p->out_stats_groups;
        // in the epilogue (mf_conv_resolve: 4-wave tiles whose pixel tile lies inside one sample); split-K layers: in the combine pass below
        if (l.cfg.stats == MF_CONV_STATS_EPILOGUE) { a.gn_out = p->out_stats; *l.stats_done = true; }
    }
    if (const int rc = mf_igemm_launch(a, tc, p->nphase, goff_max, x3, p->q, l.stream)) return rc;
    if (const int rc = a.dbg ? mf_conv_debug_times_report(a, tc, p->nphase, l.stream) : MF_OK) return rc;
    if (tc.nsplit > 1) {
        if (p->prof_mid) MF_HIP(hipEventRecord(p->prof_mid, l.stream));
        ConvArgs e = a;   // unit-grid strides for the combine pass
        e.yi = ob.Wp() * ob.C; e.yj = ob.C;
        bool with_stats = false;
        if (const int rc = mf_splitk_combine(e, tc.nsplit, batch, p->out_h, out_w_eff, tokens == 0 ? p->out_stats : nullptr, p->out_stats_groups, &with_stats, l.stream)) return rc;
        if (with_stats) *l.stats_done = true;
    }
    return MF_OK;
}

int conv_launch_impl(ConvPlan* p, const ActView& in, const ActView& out, const ActView& res, int batch, hipStream_t stream, int tokens, bool* stats_done) {
    const ActBuf &ib = *in.buf, &ob = *out.buf;
    MF_REQUIRE(tokens >= 0 && (tokens == 0 || (!p->halo && !p->up_hi && p->Hq == 1 && p->nphase == 1 && p->out_step == 1 && tokens <= p->Wq)),
               "conv: a token prefix (%d) needs a single-row sequence layer on the implicit-GEMM path with at least that many positions", tokens);
    MF_REQUIRE(p->bound_in_ld == ib.C && p->bound_in_wp == ib.Wp(), "conv: plan not bound to this input geometry");
    MF_REQUIRE(in.C >= p->cin_pad && in.coff % 8 == 0 && in.coff + in.C <= ib.C, "conv: bad input view");
    // the epilogue stores channel quads: a cout that is not a multiple of 4 spills zero-weight channels
    // into the next (up to 3) channels of the buffer, which must exist
    MF_REQUIRE(out.C == (p->d.act == 5 ? p->d.cout / 2 : p->d.cout) && out.coff % 4 == 0 && out.coff + (out.C + 3) / 4 * 4 <= ob.C, "conv: bad output view");
    MF_REQUIRE(ob.H == p->out_h && ob.W == p->out_w, "conv: output buffer %dx%d != %dx%d", ob.H, ob.W, p->out_h, p->out_w);
    const bool x3 = p->precision != MF_PREC_BF16;
    MF_REQUIRE(!x3 || (ib.lo && ob.lo), "conv: BF16X3 needs lo planes");
    MF_REQUIRE(p->precision != MF_PREC_F16Q || p->q, "conv (f16q): the plan was not packed in this format");
    Launch l{p, in, out, res, batch, tokens, stream, x3, {}, stats_done};
    if (const int rc = mf_conv_resolve(p, batch, tokens, p->out_stats ? p->out_stats_groups : 0, &l.cfg)) return rc;

    switch (l.cfg.family) {
    case MF_CONV_FAMILY_THIN: return launch_thin(l);
    case MF_CONV_FAMILY_TWIN: {   // wide halo layer, too few patches for the fat tiles at this batch: its implicit-GEMM twin
        p->alt->prof_mid = p->prof_mid;
        p->alt->out_stats = p->out_stats; p->alt->out_stats_groups = p->out_stats_groups;
        const int rc = conv_launch_impl(p->alt, in, out, res, batch, stream, 0, stats_done);
        p->alt->prof_mid = nullptr;
        return rc;
    }
    case MF_CONV_FAMILY_F16Q: return p->halo ? launch_halo(l) : launch_q_upsample(l);
    case MF_CONV_FAMILY_HALO: case MF_CONV_FAMILY_HALO_W: case MF_CONV_FAMILY_HALO_W_SPLIT: return launch_halo(l);
    default: return launch_igemm(l);
    }
}

}  // namespace

// ConvPlan::out_stats (set by the network builder when the layer's consumer is a GroupNorm of exactly this output): every launch leaves the
// (sum, sum of squares) per (sample, group) of the stored values ADDED to out_stats -- from the kernel's epilogue or the split-K combine where
// the chosen configuration can, else from a k_gn_stats pass behind the conv.  The consumer then skips its own statistics pass.
int mf_conv_launch(ConvPlan* p, const ActView& in, const ActView& out, const ActView& res, int batch, hipStream_t stream, int tokens) {
    bool stats_done = false;
    int rc = conv_launch_impl(p, in, out, res, batch, stream, tokens, &stats_done);
    if (!rc && p->out_stats && !stats_done) rc = mf_groupnorm_stats(out, p->out_stats_groups, p->out_stats, batch, stream);
    static const bool copies = mf_debug_has("copies");       // (development, eager launches only: the probe synchronises)
    if (copies && !rc && batch > 1) rc = mf_conv_debug_copies(p, in, out, batch, stream);
    return rc;
}

int mf_gemm_grouped_launch(ConvPlan* p, const GroupedGemm& g, hipStream_t stream) {
    MF_REQUIRE(!p->halo && p->nphase == 1 && p->bound_in_ld > 0, "grouped gemm: plan must be a bound mf_gemm_plan_create shell");
    const bool x3 = p->precision == MF_PREC_BF16X3;
    ConvArgs a{};
    a.x_hi = g.x_hi; a.x_lo = x3 ? g.x_lo : nullptr;
    a.w_hi = p->w_hi; a.w_lo = p->w_lo; a.bias = p->bias; a.goff = p->goff;
    a.M = g.M; a.N = p->d.cout; a.Npad = p->Npad;
    a.HqWq = g.M; a.Wq = g.M;          // rows are linear: (b, i, j) = (0, 0, m)
    mf_fastdiv((uint32_t)a.HqWq, &a.dv_hw_mul, &a.dv_hw_shr); mf_fastdiv((uint32_t)a.Wq, &a.dv_w_mul, &a.dv_w_shr);
    a.xb = 0; a.xi = 0; a.xj = g.x_row;
    a.y_hi = g.y_hi; a.y_lo = x3 ? g.y_lo : nullptr;
    a.yb = 0; a.yi = 0; a.yj = g.y_row;
    a.act = 0;
    a.ld = -1;
    a.goff_total = p->goff_total;
    a.ph[0] = p->ph[0];
    a.zgroups = g.groups; a.zheads = g.heads;
    a.zx_b = g.zx_b; a.zx_h = g.zx_h; a.zy_b = g.zy_b; a.zy_h = g.zy_h;
    a.zw = (int64_t)p->ph[0].KT * p->Npad * 64;
    const int M = g.M, N = a.N;
    // the tile by this path's own rule (no split-K, one GEMM per group on blockIdx.z)
    ConvTile t{64, 64, 2, 2, 1};
    if (N <= 16) t = {128, 16, 4, 1, 1};
    else if (N <= 32) t = {128, 32, 4, 1, 1};
    else if (M <= 16) t = {16, 64, 1, 4, 1};
    else if (cdiv(M, 128) * cdiv(N, 128) * g.groups >= 512 && N % 128 == 0) t = {128, 128, 2, 2, 1};
    else if (cdiv(M, 128) * cdiv(N, 64) * g.groups >= 512) t = {128, 64, 2, 2, 1};
    a.tiles_m = cdiv(M, t.bm); a.tiles_n = cdiv(N, t.bn);
    return mf_igemm_launch(a, t, 1, p->ph[0].ngroups, x3, false, stream);
}

void mf_conv_kernel_name(const ConvPlan* p, int batch, char* buf, int cap) {
    const char* x3 = p->precision != MF_PREC_BF16 ? "true" : "false";
    ConvLaunchCfg c;
    if (mf_conv_resolve(p, batch, 0, 0, &c)) { snprintf(buf, cap, "(no kernel: %s)", mf_last_error()); return; }
    const ConvTile& t = c.tile;
    // (the f16 + FP6 tile: the specialised workgroup <16,128,2,2,...> -- 4 compute + 4 producer waves)
    const char* qt = "2,2";
    switch (c.family) {
    case MF_CONV_FAMILY_F16Q:
        if (p->up_hi) { snprintf(buf, cap, "4 x k_conv3x3_halo_w<16,128,%s,true,1,phase> f16+fp6", qt); return; }
        {
            // (" grid N": the launch's thread count as rocprofv3 reports it, so that a counter pass can be matched to exactly these launches -- the split
            // and unsplit launches share one kernel symbol)
            const long grid = (long)batch * cdiv(p->out_h, 16) * cdiv(p->out_w, 16) * cdiv(p->d.cout, 128) * t.nsplit * 512;
            if (t.nsplit > 1) snprintf(buf, cap, "k_conv3x3_halo_w<16,128,%s,true,1> f16+fp6 split %d grid %ld", qt, t.nsplit, grid);
            else snprintf(buf, cap, "k_conv3x3_halo_w<16,128,%s,true,1> f16+fp6 grid %ld", qt, grid);
        }
        return;
    case MF_CONV_FAMILY_THIN:
        snprintf(buf, cap, "k_conv_thin<%d,%d,%d,%d,%s>", p->d.kh, p->d.stride_h, p->d.cin <= 8 ? 8 : 16, (p->d.cout + 15) / 16, x3);
        return;
    case MF_CONV_FAMILY_HALO_W_SPLIT:
        snprintf(buf, cap, "k_conv3x3_halo_w<16,256,2,4,%s,1> split %d", x3, t.nsplit);
        return;
    case MF_CONV_FAMILY_HALO_W:
    case MF_CONV_FAMILY_HALO:
        // last template argument: halo stages (register-weights kernel) / taps per weight-ring slot (LDS-weights kernel)
        snprintf(buf, cap, "k_conv3x3_halo%s<%d,%d,%d,%d,%s,%d>", c.family == MF_CONV_FAMILY_HALO_W ? "_w" : "", t.bm, t.bn, t.wgm, t.wgn, x3,
                 c.family == MF_CONV_FAMILY_HALO_W ? (t.bn >= 128 ? 1 : 3) : 2);
        return;
    default:   // implicit GEMM, or a wide halo plan's twin
        if (c.ld >= 3) snprintf(buf, cap, "k_conv_igemm<%d,%d,%d,%d,%s,%d,pw>", t.bm, t.bn, t.wgm, t.wgn, x3, c.bk);   // pw: producer waves
        else snprintf(buf, cap, "k_conv_igemm<%d,%d,%d,%d,%s,%d>%s", t.bm, t.bn, t.wgm, t.wgn, x3, c.bk, p->q ? " f16+fp6" : "");
    }
}
