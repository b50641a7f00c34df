// Graph executables are NEVER destroyed while the process lives: destroying one, even behind a stream synchronize, freed objects under the
// runtime's asynchronous completion-handler thread (a segmentation fault inside that thread once per ~15 runs of 2000 steps; DESIGN.md
// section 7b).  This unit has no call that destroys an executable, and it is the only one that holds them: a handle RETIRES its executables to
// a process-wide pool, and the next capture of the same launch sequence -- by any handle -- updates one of them in place
// (hipGraphExecUpdate) instead of instantiating.
// The pool is keyed by what an in-place update requires to be equal: the device, the node sequence (type and, for kernel nodes, the kernel
// FUNCTION and workgroup shape of every node in the capture's order) and the edge list, hashed from the captured graph itself.  Anything
// else two captures can differ in (pointers, grids, scalars) is kernel parameters, which the update rewrites -- so an update of a pooled
// executable is not expected to be refused.  If the runtime refuses one anyway, that executable is parked for good: a bounded leak of one
// executable per refusal instead of a destroy.  Executables per process <= (distinct launch sequences run) x (handles alive at once).
#include "step_graph.h"

#include <mutex>
#include <vector>

static std::mutex g_pool_mu;
static std::map<GraphSig, std::vector<hipGraphExec_t>> g_spare;   // guarded by g_pool_mu
static std::vector<hipGraphExec_t> g_parked;                       // guarded by g_pool_mu; kept, never launched again

static bool graph_signature(hipGraph_t g, GraphSig* sig) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    size_t nn = 0, ne = 0;
    if (hipGraphGetNodes(g, nullptr, &nn) != hipSuccess || hipGraphGetEdges(g, nullptr, nullptr, &ne) != hipSuccess) return false;
    std::vector<hipGraphNode_t> nodes(nn), from(ne), to(ne);
    if (nn && hipGraphGetNodes(g, nodes.data(), &nn) != hipSuccess) return false;
    if (ne && hipGraphGetEdges(g, from.data(), to.data(), &ne) != hipSuccess) return false;
    GraphSig s;
    s.nodes = nn; s.edges = ne;
    s.mix((unsigned long long)dev);
    std::map<hipGraphNode_t, unsigned> index;
    for (size_t i = 0; i < nn; ++i) {
        index[nodes[i]] = (unsigned)i;
        hipGraphNodeType ty;
        if (hipGraphNodeGetType(nodes[i], &ty) != hipSuccess) return false;
        s.mix((unsigned long long)ty);
        if (ty == hipGraphNodeTypeKernel) {
            hipKernelNodeParams kp;
            if (hipGraphKernelNodeGetParams(nodes[i], &kp) != hipSuccess) return false;
            s.mix((unsigned long long)(uintptr_t)kp.func);
            s.mix(((unsigned long long)kp.blockDim.x << 32) ^ ((unsigned long long)kp.blockDim.y << 16) ^ kp.blockDim.z);   // (a workgroup shape is part of the kernel choice here)
        }
    }
    // edges as index pairs, order-independent (sum of per-edge hashes): the runtime may list them in any order
    unsigned long long eh = 0;
    for (size_t i = 0; i < ne; ++i) {
        GraphSig e1;
        e1.mix(index[from[i]]); e1.mix(index[to[i]]);
        eh += e1.h;
    }
    s.mix(eh);
    *sig = s;
    return true;
}

hipGraphExec_t StepGraphs::adopt(int variant, hipGraph_t g, unsigned long long salt) {
    GraphSig sig;
    const bool have_sig = graph_signature(g, &sig);
    if (have_sig && salt) { sig.mix(0x67726f7570ull); sig.mix(salt); }
    hipGraphExec_t ex = nullptr, spare = nullptr;
    if (have_sig) {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        auto sp = g_spare.find(sig);
        if (sp != g_spare.end() && !sp->second.empty()) { spare = sp->second.back(); sp->second.pop_back(); }
    }
    if (spare) {   // a retired executable of exactly this launch sequence on this device: update it in place
        hipGraphNode_t bad_node = nullptr;
        hipGraphExecUpdateResult res = hipGraphExecUpdateSuccess;
        // (its last launch -- possibly by another handle -- is long finished when its launch sequence is captured again; the device-wide wait is
        // for the case of a worker that destroys and re-creates handles back to back)
        (void)hipDeviceSynchronize();
        if (hipGraphExecUpdate(spare, g, &bad_node, &res) == hipSuccess && res == hipGraphExecUpdateSuccess) {
            ex = spare;
            ++updates;
        } else {
            (void)hipGetLastError();
            std::lock_guard<std::mutex> lk(g_pool_mu);
            g_parked.push_back(spare);
            ++refusals;
        }
    }
    hipError_t ei = hipSuccess;
    if (!ex && (ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0)) == hipSuccess) ++instantiations;
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) { splice_set_error("splice_step_run: hipGraphInstantiate: %s", hipGetErrorString(ei)); return nullptr; }
    if (!have_sig) { sig = GraphSig(); sig.mix((unsigned long long)(uintptr_t)ex); }   // (signature unavailable: a key of its own, never shared)
    graphs_[variant] = Entry{ex, sig};
    return ex;
}

void StepGraphs::retire() {
    if (graphs_.empty()) return;
    // (no synchronize needed here: nothing is destroyed; the next user's update waits for the device)
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (auto& kv : graphs_) g_spare[kv.second.sig].push_back(kv.second.ex);
    graphs_.clear();
}
