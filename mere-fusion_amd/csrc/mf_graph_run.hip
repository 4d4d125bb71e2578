#include "mf_graph_run.h"
#include "mf_conv.h"

int mf_no_graph_mode() {
    const char* e = getenv("MF_NO_GRAPH");
    const int v = e ? atoi(e) : 0;
    return v == 2 ? 2 : v != 0;
}

GraphRunner::~GraphRunner() {
    drop_all();
    if (stream) (void)hipStreamDestroy(stream);
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_out) (void)hipEventDestroy(ev_out);
}

int GraphRunner::init(bool use_graph_) {
    use_graph = use_graph_;
    MF_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    MF_HIP(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
    MF_HIP(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
    return MF_OK;
}

int GraphRunner::run(int key, hipStream_t s, const Launch& body, const std::function<void()>& lookup, const Launch& measure) {
    if (!use_graph) {
        if (looked_up.insert(key).second && lookup) lookup();        // one table lookup per layer and key, not one per forward
        return body(s);
    }
    auto it = graphs.find(key);
    if (it == graphs.end()) {
        // the first forward at a key runs eagerly (split-K workspaces grow and the kernels' LDS attributes are set here, neither may happen inside a capture)
        graphs.emplace(key, nullptr);
        // launch configurations: a table lookup per layer (MF_TUNE_CACHE / the table shipped beside the library), never a measurement -- a serving loop that
        // meets a new batch size pays one eager forward and one capture, nothing more
        if (lookup) lookup();
        int rc = body(s);
        if (rc || !measure || !mf_autotune_enabled()) return rc;
        if ((rc = measure(s))) return rc;                            // MF_AUTOTUNE=1 (development): the buffers hold real data now
        return body(s);
    }
    if (!it->second) {
        hipGraph_t graph = nullptr;
        MF_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        int rc = body(stream);
        hipError_t e = hipStreamEndCapture(stream, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess) { mf_set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return MF_ERR_HIP; }
        hipGraphExec_t exec = nullptr;
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { mf_set_error("instantiating the captured graph: %s", hipGetErrorString(e)); return MF_ERR_HIP; }
        it->second = exec;
    }
    // the graph replays on the runner's own stream, fenced by events against the caller's stream: the
    // caller usually hands in the legacy NULL stream, whose implicit ordering a graph launch does not inherit
    MF_HIP(hipEventRecord(ev_in, s));
    MF_HIP(hipStreamWaitEvent(stream, ev_in, 0));
    MF_HIP(hipGraphLaunch(it->second, stream));
    MF_HIP(hipEventRecord(ev_out, stream));
    MF_HIP(hipStreamWaitEvent(s, ev_out, 0));
    return MF_OK;
}

int GraphRunner::retune(int key, hipStream_t s, const char* who, const Launch& measure) {
    auto it = graphs.find(key);
    if (use_graph && it == graphs.end()) { mf_set_error("%s at batch %d first (the layers are timed on its buffers)", who, key); return MF_ERR_INVALID; }
    MF_HIP(hipStreamSynchronize(stream));
    MF_HIP(hipStreamSynchronize(s));
    int rc = measure(s);
    if (rc) return rc;
    MF_HIP(hipStreamSynchronize(s));
    if (use_graph) { if (it->second) (void)hipGraphExecDestroy(it->second); graphs.erase(it); }
    return MF_OK;
}

bool GraphRunner::captured(int key) const {
    auto it = graphs.find(key);
    return it != graphs.end() && it->second != nullptr;
}

void GraphRunner::drop_all() {
    for (auto& g : graphs) if (g.second) (void)hipGraphExecDestroy(g.second);
    graphs.clear();
}
