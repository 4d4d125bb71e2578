// A static schedule and its runner: the op list of a handle whose forward is a fixed sequence of launches (the MuseTalk UNet / VAE handles, mf_net), the measurement
// seam over it, the side branches of the list, the implicit-GEMM layers whose launch configurations come from the tuning table, and the hipGraph per batch size
// (mf_graph_run.h).  It knows ops, streams and conv plans -- nothing of weights, norms or operand formats: those are the builder's (mf_musetalk_build.h).
#pragma once
#include "mf_conv.h"
#include "mf_graph_run.h"
#include <functional>
#include <map>
#include <string>
#include <vector>

struct Schedule {
    typedef std::function<int(int, hipStream_t)> Op;          // (batch, stream) -> mf_status
    struct OpInfo { std::string name, kernel; double flops_per_frame; };
    // an implicit-GEMM layer with its bound views: measured launch configurations (mf_conv_tune) on the first forward at a batch size.
    // p_big: a second plan of the same layer that takes the launches of >= big_from frames (the builder's dual-path convs); the seam names the one that runs.
    struct Tunable { ConvPlan* p; ActView in, out, res; int op; ConvPlan* p_big = nullptr; int big_from = 0; };

    std::vector<Op> ops;
    std::vector<OpInfo> info;   // parallel to ops (measurement seam)
    std::vector<Tunable> tunables;
    GraphRunner graph;
    // Side branches of the schedule: an op whose result is not needed by its successors in the list -- the hoisted k | v GEMM, a resnet's 1x1
    // shortcut conv -- runs on a second stream beside the chain (a parallel branch of the captured graph) and is joined right before its first
    // consumer.  The UNet's batch-8 launches leave most CUs idle, so the branch costs the chain nothing (Wav2Lip's forked audio encoder is worth
    // 11 % of its step the same way).
    std::map<int, int> side_ops;                 // op index -> branch number
    std::multimap<int, int> join_before;         // op index -> branch to wait for before that op
    std::vector<hipEvent_t> ev_fork, ev_join;
    hipStream_t side_stream = nullptr;           // only a schedule that may fork owns one

    Schedule() = default;
    Schedule(const Schedule&) = delete;
    ~Schedule();
    // use_graph: one hipGraph per batch size, else every forward an eager launch chain.  may_fork: side ops run on the second stream, else everything in line.
    int init(bool use_graph, bool may_fork);

    // append an op -- or, slot >= 0, fill the op reserved at that index; returns the op's index
    int push(const std::string& name, const std::string& kernel, double flops, Op op, int slot = -1);
    int reserve(const std::string& name) { return push(name, "(reserved)", 0.0, [](int, hipStream_t) { return MF_OK; }); }
    void tunable(const Tunable& t) { tunables.push_back(t); }
    void mark_side(int op) { side_ops[op] = (int)side_ops.size(); }
    void join_here(int op) { join_before.insert({(int)ops.size(), side_ops.at(op)}); }   // ... before the NEXT op pushed

    int run(int B, hipStream_t s);
    // The explicit warm-up behind mf_unet_tune / mf_vae_tune / mf_net_tune (GraphRunner::retune).  Seconds per full-size network: call it at start-up for every
    // batch size the serving loop can emit, or ship MF_TUNE_CACHE.
    int tune(int B, hipStream_t s, const char* who);
    // measurement seam: every op alone between two hipEvents on `s`, no graph
    int profile(int B, int iters, float* ms, hipStream_t s);
    int op_info(int i, char* name, int ncap, char* kernel, int kcap, double* flops) const;
    double flops_per_frame() const;

private:
    int run_body(int B, hipStream_t s);
    int measure(int B, hipStream_t s);
    void lookup(int B);
    void name_kernel(const Tunable& t, int B);
};
