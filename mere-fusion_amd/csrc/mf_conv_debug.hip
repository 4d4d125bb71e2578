// Development probes of the convolution launch path, behind MF_DEBUG words (mf_common.h).  mf_conv_launch.hip calls them only when the word is set; nothing here
// runs in a normal forward.  Their output text and dump files are read by tools/unet_copies_probe.py and tools/pkfma_dump_analyze.py.
#include "mf_conv.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
// MF_DEBUG=copies (eager launches only: it synchronises): for a batch of IDENTICAL items, reports every layer whose input, output or statistics of
// an item differ from item 0's -- a row's result may not depend on where its image sits in the batch (tools/unet_copies_probe.py)
int mf_conv_debug_copies(const ConvPlan* p, const ActView& in, const ActView& out, int batch, hipStream_t stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &cs);
    if (cs != hipStreamCaptureStatusNone) return MF_OK;
    MF_HIP(hipStreamSynchronize(stream));
    auto differ = [&](const ActView& v, int* first) -> double {
        const ActBuf& b = *v.buf;
        const size_t n = (size_t)b.per_batch();
        std::vector<bf16_t> h0(n), hk(n), l0(b.lo ? n : 0), lk(b.lo ? n : 0);
        (void)hipMemcpy(h0.data(), b.hi, n * sizeof(bf16_t), hipMemcpyDeviceToHost);
        if (b.lo) (void)hipMemcpy(l0.data(), b.lo, n * sizeof(bf16_t), hipMemcpyDeviceToHost);
        double worst = 0.0;
        for (int k = 1; k < batch; ++k) {
            (void)hipMemcpy(hk.data(), b.hi + (size_t)k * n, n * sizeof(bf16_t), hipMemcpyDeviceToHost);
            if (b.lo) (void)hipMemcpy(lk.data(), b.lo + (size_t)k * n, n * sizeof(bf16_t), hipMemcpyDeviceToHost);
            double w = 0.0;
            size_t cnt = 0, first_i = 0, last_i = 0;
            int cmin = 1 << 30, cmax = -1;
            for (size_t i = 0; i < n; ++i) {
                const int c = (int)(i % b.C);
                if (c < v.coff || c >= v.coff + v.C) continue;
                const double a0 = (double)mf_bf2f(h0[i]) + (b.lo ? (double)mf_bf2f(l0[i]) : 0.0), ak = (double)mf_bf2f(hk[i]) + (b.lo ? (double)mf_bf2f(lk[i]) : 0.0);
                const double e = std::fabs(a0 - ak);
                if (e > 1e-3) { if (!cnt) first_i = i; last_i = i; ++cnt; cmin = std::min(cmin, c); cmax = std::max(cmax, c); }
                w = std::max(w, e);
            }
            if (cnt && w > worst)
                fprintf(stderr, "[MF_DEBUG=copies]   item %d: %zu elements off by > 1e-3, padded pixels %zu .. %zu (row pitch %d px), channels %d .. %d\n", k, cnt, first_i / b.C,
                        last_i / b.C, b.Wp(), cmin, cmax);
            if (w > worst) { worst = w; *first = k; }
        }
        return worst;
    };
    int ki = 0, ko = 0;
    const double di = differ(in, &ki), dout = differ(out, &ko);
    // the per-token LayerNorm statistics this layer reads / leaves ([item][token][2] doubles)
    auto stats_differ = [&](const double* dev, int tokens_per_item, int* first) -> double {
        if (!dev) return 0.0;
        std::vector<double> h((size_t)batch * tokens_per_item * 2);
        (void)hipMemcpy(h.data(), dev, h.size() * sizeof(double), hipMemcpyDeviceToHost);
        double worst = 0.0;
        for (int k = 1; k < batch; ++k)
            for (int i = 0; i < tokens_per_item * 2; ++i) {
                const double w = std::fabs(h[(size_t)k * tokens_per_item * 2 + i] - h[i]);
                if (w > worst) { worst = w; *first = k; }
            }
        return worst;
    };
    int ksi = 0, kso = 0;
    const double dsi = stats_differ(p->ln_in, in.buf->H * in.buf->W, &ksi), dso = stats_differ(p->ln_out, out.buf->H * out.buf->W, &kso);
    if (dsi > 0.0 || dso > 0.0) fprintf(stderr, "[MF_DEBUG=copies] LayerNorm statistics: read differ by %.3e (item %d), left differ by %.3e (item %d)\n", dsi, ksi, dso, kso);
    // MF_DEBUG_DUMP=<prefix>: the first layer whose copies disagree although its inputs agree leaves both items' outputs, its LayerNorm statistics, column sums and
    // bias as raw files (<prefix>_meta.txt, _y0.f32, _yk.f32, _stats.f64, _cs.f32, _bias.f32) for offline analysis (tools/pkfma_dump_analyze.py)
    static bool dumped = false;
    const char* dump = getenv("MF_DEBUG_DUMP");
    if (dump && !dumped && di == 0.0 && dout > 0.0) {
        dumped = true;
        const ActBuf& b = *out.buf;
        const size_t n = (size_t)b.per_batch();
        auto plane = [&](int item, std::vector<float>& f) {
            std::vector<bf16_t> h(n), l(b.lo ? n : 0);
            (void)hipMemcpy(h.data(), b.hi + (size_t)item * n, n * sizeof(bf16_t), hipMemcpyDeviceToHost);
            if (b.lo) (void)hipMemcpy(l.data(), b.lo + (size_t)item * n, n * sizeof(bf16_t), hipMemcpyDeviceToHost);
            f.resize(n);
            for (size_t i = 0; i < n; ++i) f[i] = mf_bf2f(h[i]) + (b.lo ? mf_bf2f(l[i]) : 0.f);
        };
        auto put = [&](const char* suffix, const void* data, size_t bytes) {
            const std::string path = std::string(dump) + suffix;
            if (FILE* f = fopen(path.c_str(), "wb")) { fwrite(data, 1, bytes, f); fclose(f); }
        };
        std::vector<float> y0, yk;
        plane(0, y0); plane(ko, yk);
        put("_y0.f32", y0.data(), n * 4); put("_yk.f32", yk.data(), n * 4);
        const int tok = in.buf->H * in.buf->W;
        if (p->ln_in) {
            std::vector<double> st((size_t)tok * 2);
            (void)hipMemcpy(st.data(), p->ln_in, st.size() * 8, hipMemcpyDeviceToHost);
            put("_stats.f64", st.data(), st.size() * 8);
            std::vector<float> cs(p->Npad);
            (void)hipMemcpy(cs.data(), p->ln_cs, cs.size() * 4, hipMemcpyDeviceToHost);
            put("_cs.f32", cs.data(), cs.size() * 4);
        }
        std::vector<float> bias(p->Npad);
        (void)hipMemcpy(bias.data(), p->bias, bias.size() * 4, hipMemcpyDeviceToHost);
        put("_bias.f32", bias.data(), bias.size() * 4);
        char kn2[96], meta[512];
        mf_conv_kernel_name(p, batch, kn2, sizeof(kn2));
        snprintf(meta, sizeof(meta), "C %d\nWp %d\nH %d\nW %d\nhalo %d\ncoff %d\nvC %d\ncin %d\ncout %d\nNpad %d\nitem %d\ntokens %d\nln_eps %g\nact %d\nkernel %s\n", b.C, b.Wp(), b.H, b.W,
                 b.halo, out.coff, out.C, p->d.cin, p->d.cout, p->Npad, ko, tok, (double)p->ln_eps, p->d.act, kn2);
        put("_meta.txt", meta, strlen(meta));
    }
    if (di > 0.0 || dout > 0.0) {
        char kn[96];
        mf_conv_kernel_name(p, batch, kn, sizeof(kn));
        fprintf(stderr, "[MF_DEBUG=copies] %d->%d k%d @%dx%d act %d%s%s: input differs by %.3e (item %d), output by %.3e (item %d)  %s\n", p->d.cin, p->d.cout, p->d.kh, p->d.in_h,
                p->d.in_w, p->d.act, p->ln_in ? " ln_in" : "", p->ln_out ? " ln_out" : "", di, ki, dout, ko, kn);
    }
    return MF_OK;
}

// MF_DEBUG=times: 4 s_memtime stamps per workgroup of k_conv_igemm (ConvArgs::dbg); launches with more workgroups than the buffer holds are not stamped
unsigned long long* mf_conv_debug_times_buffer(int64_t workgroups) {
    static unsigned long long* dbg_buf = nullptr;
    if (!dbg_buf && hipMalloc(&dbg_buf, (size_t)4 * 65536 * sizeof(unsigned long long)) != hipSuccess) dbg_buf = nullptr;
    return workgroups <= 65536 ? dbg_buf : nullptr;
}

int mf_conv_debug_times_report(const ConvArgs& a, const ConvTile& tc, int nphase, hipStream_t stream) {
    static int reports = 0;
    if (++reports <= 3 || reports > 5) return MF_OK;   // skip the warm-up launches
    MF_HIP(hipStreamSynchronize(stream));
    const size_t nwg = (size_t)a.tiles_m * a.tiles_n * tc.nsplit * nphase;
    std::vector<unsigned long long> t(4 * nwg);
    MF_HIP(hipMemcpy(t.data(), a.dbg, t.size() * sizeof(t[0]), hipMemcpyDeviceToHost));
    unsigned long long lo = ~0ull, hi = 0;
    std::vector<double> d[3], start, end;
    for (size_t w = 0; w < nwg; ++w) {
        lo = std::min(lo, t[4 * w]); hi = std::max(hi, t[4 * w + 3]);
        for (int k = 0; k < 3; ++k) d[k].push_back((double)(t[4 * w + k + 1] - t[4 * w + k]));
    }
    for (size_t w = 0; w < nwg; ++w) { start.push_back((double)(t[4 * w] - lo)); end.push_back((double)(t[4 * w + 3] - lo)); }
    auto med = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    auto mx = [](const std::vector<double>& v) { return *std::max_element(v.begin(), v.end()); };
    fprintf(stderr, "[MF_DEBUG=times] %zu WGs tile %dx%d split %d: span %llu ticks; prologue med %.0f max %.0f; loop med %.0f max %.0f; "
                    "epilogue med %.0f max %.0f; WG start med %.0f max %.0f; WG end med %.0f\n",
            nwg, tc.bm, tc.bn, tc.nsplit, hi - lo, med(d[0]), mx(d[0]), med(d[1]), mx(d[1]), med(d[2]), mx(d[2]), med(start), mx(start), med(end));
    return MF_OK;
}
