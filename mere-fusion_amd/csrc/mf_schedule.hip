#include "mf_schedule.h"

Schedule::~Schedule() {
    graph.drop_all();
    if (side_stream) (void)hipStreamDestroy(side_stream);
    for (hipEvent_t e : ev_fork) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_join) (void)hipEventDestroy(e);
}

int Schedule::init(bool use_graph, bool may_fork) {
    const int rc = graph.init(use_graph);
    if (rc) return rc;
    if (may_fork) MF_HIP(hipStreamCreateWithFlags(&side_stream, hipStreamNonBlocking));
    return MF_OK;
}

int Schedule::push(const std::string& name, const std::string& kernel, double flops, Op op, int slot) {
    if (slot < 0) {
        ops.push_back(std::move(op));
        info.push_back(OpInfo{name, kernel, flops});
        return (int)ops.size() - 1;
    }
    ops[slot] = std::move(op);
    info[slot] = OpInfo{name, kernel, flops};
    return slot;
}

int Schedule::profile(int B, int iters, float* ms, hipStream_t s) {
    const int n = (int)ops.size();
    std::vector<hipEvent_t> ev(n + 1);
    for (auto& e : ev) MF_HIP(hipEventCreate(&e));
    std::vector<double> acc(n, 0.0);
    for (int it = 0; it < iters; ++it) {
        for (int i = 0; i < n; ++i) {
            MF_HIP(hipEventRecord(ev[i], s));
            int rc = ops[i](B, s);
            if (rc) return rc;
        }
        MF_HIP(hipEventRecord(ev[n], s));
        MF_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < n; ++i) { float t = 0.f; MF_HIP(hipEventElapsedTime(&t, ev[i], ev[i + 1])); acc[i] += t; }
    }
    for (int i = 0; i < n; ++i) ms[i] = (float)(acc[i] / iters);
    for (auto& e : ev) (void)hipEventDestroy(e);
    return MF_OK;
}

int Schedule::op_info(int i, char* name, int ncap, char* kernel, int kcap, double* flops) const {
    MF_REQUIRE(i >= 0 && i < (int)info.size() && name && kernel && flops, "op_info: bad argument");
    snprintf(name, ncap, "%s", info[i].name.c_str());
    snprintf(kernel, kcap, "%s", info[i].kernel.c_str());
    *flops = info[i].flops_per_frame;
    return MF_OK;
}

double Schedule::flops_per_frame() const {
    double f = 0.0;
    for (const OpInfo& i : info) f += i.flops_per_frame;
    return f;
}

// ---- execution ----------------------------------------------------------------------------------------
int Schedule::run_body(int B, hipStream_t s) {
    if (!side_stream || side_ops.empty()) {
        for (auto& op : ops) { int rc = op(B, s); if (rc) return rc; }
        return MF_OK;
    }
    while (ev_fork.size() < side_ops.size()) {
        hipEvent_t a = nullptr, b = nullptr;
        MF_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        MF_HIP(hipEventCreateWithFlags(&b, hipEventDisableTiming));
        ev_fork.push_back(a); ev_join.push_back(b);
    }
    std::vector<char> open(side_ops.size(), 0);
    for (size_t i = 0; i < ops.size(); ++i) {
        auto jr = join_before.equal_range((int)i);
        for (auto it = jr.first; it != jr.second; ++it)
            if (open[it->second]) { MF_HIP(hipStreamWaitEvent(s, ev_join[it->second], 0)); open[it->second] = 0; }
        auto so = side_ops.find((int)i);
        if (so == side_ops.end()) {
            int rc = ops[i](B, s);
            if (rc) return rc;
            continue;
        }
        const int k = so->second;
        MF_HIP(hipEventRecord(ev_fork[k], s));
        MF_HIP(hipStreamWaitEvent(side_stream, ev_fork[k], 0));
        int rc = ops[i](B, side_stream);
        if (rc) return rc;
        MF_HIP(hipEventRecord(ev_join[k], side_stream));
        open[k] = 1;
    }
    for (size_t k = 0; k < open.size(); ++k)                       // a branch nobody consumed inside the list still ends inside it
        if (open[k]) MF_HIP(hipStreamWaitEvent(s, ev_join[k], 0));
    return MF_OK;
}

void Schedule::name_kernel(const Tunable& t, int B) {
    char kn[96];
    mf_conv_kernel_name(t.p_big && B >= t.big_from ? t.p_big : t.p, B, kn, sizeof(kn));   // the measurement seam names the kernel that actually runs
    info[t.op].kernel = kn;
}

// every buffer holds real data (a forward at this batch size has run): time each implicit-GEMM layer's launch configurations in place
int Schedule::measure(int B, hipStream_t s) {
    for (auto& t : tunables) {
        int rc = mf_conv_tune(t.p, t.in, t.out, t.res, B, s);
        if (rc) return rc;
        name_kernel(t, B);
    }
    return MF_OK;
}

// launch configurations: a table lookup per implicit-GEMM layer, never a measurement
void Schedule::lookup(int B) {
    for (auto& t : tunables)
        if (mf_conv_tune_lookup(t.p, t.in, B)) name_kernel(t, B);
}

int Schedule::tune(int B, hipStream_t s, const char* who) {
    return graph.retune(B, s, who, [&](hipStream_t st) { return measure(B, st); });
}

int Schedule::run(int B, hipStream_t s) {
    return graph.run(B, s, [&](hipStream_t st) { return run_body(B, st); }, [&] { lookup(B); }, [&](hipStream_t st) { return measure(B, st); });
}
