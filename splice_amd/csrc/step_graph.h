// Graph executables of the step handles and the process-wide pool they retire to (step_graph.hip).  Nothing here knows what a step is.
#pragma once
#include <map>

#include "common.h"

// signature of a captured graph: what hipGraphExecUpdate needs to be equal between a capture and the executable it updates
struct GraphSig {
    unsigned long long h = 1469598103934665603ull;   // FNV-1a over (device, node types / kernel functions, edges)
    size_t nodes = 0, edges = 0;
    void mix(unsigned long long v) { for (int i = 0; i < 8; ++i) { h ^= (v >> (8 * i)) & 0xff; h *= 1099511628211ull; } }
    bool operator<(const GraphSig& o) const { return h != o.h ? h < o.h : nodes != o.nodes ? nodes < o.nodes : edges < o.edges; }
};

// The executables one handle owns, by variant (the caller's number for a launch sequence it replays).
class StepGraphs {
public:
    hipGraphExec_t find(int variant) const {   // nullptr: not captured yet
        auto it = graphs_.find(variant);
        return it == graphs_.end() ? nullptr : it->second.ex;
    }
    // Makes the captured graph `g` the executable of `variant`: a pooled executable of the same signature updated in place, else a new
    // one.  salt != 0 joins the pool key (what a caller's launch sequences differ in beyond their nodes).  `g` is destroyed either way;
    // nullptr (splice_set_error called) when the instantiation fails.
    hipGraphExec_t adopt(int variant, hipGraph_t g, unsigned long long salt = 0);
    void retire();   // every executable of the handle goes to the pool; the handle captures again
    // captures that updated a pooled executable in place / updates the runtime refused (executable parked for good) / executables instantiated
    long long updates = 0, refusals = 0, instantiations = 0;

private:
    struct Entry { hipGraphExec_t ex; GraphSig sig; };
    std::map<int, Entry> graphs_;
};
