// One hipGraph per key (batch size, window count) for a handle whose forward is a fixed launch list -- the contract is DESIGN.md "hipGraph notes":
// forward 1 at a key runs eagerly behind the table lookup, forward 2 captures on the runner's own stream, every later one replays there, fenced
// against the caller's stream by an event pair.  Graphs are never updated in place: retune() and drop_all() drop them, the next forwards start over.
#pragma once
#include "mf_common.h"
#include <functional>
#include <map>
#include <set>

// MF_NO_GRAPH as a number, read where a handle is created: 0 (unset, "0", no number), 2, or 1 for every other value.  What 1 and 2 mean is the handle's business.
int mf_no_graph_mode();

struct GraphRunner {
    typedef std::function<int(hipStream_t)> Launch;   // enqueues on the stream it is given, returns mf_status

    hipStream_t stream = nullptr;                     // capture origin; the graphs replay here
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    std::map<int, hipGraphExec_t> graphs;             // key -> graph; null: the eager forward has run, the next one captures
    std::set<int> looked_up;                          // use_graph == false: keys whose lookup() has run
    bool use_graph = true;

    GraphRunner() = default;
    GraphRunner(const GraphRunner&) = delete;
    ~GraphRunner();
    int init(bool use_graph);
    // One forward.  lookup (may be empty) runs once per key, in front of its first eager forward.  measure (may be empty) runs behind that forward in graph mode
    // under MF_AUTOTUNE=1 only, followed by body once more so that the outputs belong to the configurations the graph will capture.
    int run(int key, hipStream_t caller, const Launch& body, const std::function<void()>& lookup, const Launch& measure);
    // The explicit warm-up: measure on what the last forward at `key` left in the buffers (refused before the first one: "<who> at batch <key> first ..."),
    // then drop that key's graph -- the next forward runs eagerly again (split-K workspaces of the new configurations are sized there), then re-captures.
    int retune(int key, hipStream_t caller, const char* who, const Launch& measure);
    bool captured(int key) const;
    void drop_all();                                  // the buffers the graphs point into are about to move
};
