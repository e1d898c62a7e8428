// rmc_graph.h -- the kept state graph (rmc_set_graph_keep) and the analyses on it (rmc_graph.hip).
// Nothing here knows the spec: a graph is n_states global ids, a list of (src, dst) pairs of them, a
// u16 of invariant values per state (bit b: invariant b TRUE; bit 8 + b: it raised the evaluation
// error) and the gid at which each BFS level starts.  The engine fills it level by level
// (graph_level), rmc_graph_import from host arrays.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "rmc.h"

struct GraphFail {
    int code;
    std::string msg;
};

struct KeptGraph {
    hipStream_t stream = nullptr;
    // ---- the store ----
    uint2 *edges = nullptr;  // (src, dst)
    uint64_t n_edges = 0, e_cap = 0;
    uint16_t *inv = nullptr;  // by gid
    uint64_t n_states = 0, s_cap = 0;
    std::vector<uint64_t> level_start;  // gid of the first state of each BFS level (an imported graph: one level)
    // ---- reverse CSR: built on first use, dropped when the graph grows ----
    bool csr = false;
    uint32_t *row = nullptr;      // n_states + 1: predecessors of g are col[row[g] .. row[g + 1])
    uint32_t *col = nullptr;      // n_edges sources, self-edges and duplicates included
    uint32_t *out_all = nullptr;  // out-degree, every edge
    uint32_t *out_ns = nullptr;   // out-degree without self-edges
    uint32_t *work = nullptr;     // cursors (scatter) / counters (peeling)
    uint32_t *fr[2] = {nullptr, nullptr};  // frontiers
    uint32_t *dist = nullptr;     // the last query's distances
    unsigned long long *acc = nullptr;  // small accumulators (ACC_WORDS)
    unsigned long long *hacc = nullptr; // pinned copy
    void *tmp = nullptr;          // scan scratch
    size_t tmp_bytes = 0;
    uint64_t a_states = 0, a_edges = 0;  // what the analysis buffers are sized for
    uint64_t self_edges = 0, back_edges = 0;
    double csr_seconds = 0;  // the last build
    bool have_query = false;

    ~KeptGraph() { free_all(); }
    void free_all();
    void clear();  // empty graph, buffers kept
    bool empty() const { return n_states == 0; }
    // the store (engine side): room for gids below n (doubling), then k_inv_values writes inv[gid0 ..)
    void reserve_states(uint64_t n);
    void set_states(uint64_t n) { n_states = n; grown(); }
    void append_edges(const unsigned long long *src, const unsigned long long *dst, uint64_t n);
    void import(uint64_t ns, uint64_t ne, const uint32_t *src, const uint32_t *dst, const uint16_t *iv);
    // analyses
    void reach(const rmc_reach_query *q, rmc_reach_result *res, uint32_t *dist_out);
    void reach_levels(uint64_t *can, uint64_t *cannot, uint32_t cap, uint32_t *n);
    void shape(struct rmc_graph_shape *out);
    void inv_values(uint16_t *out, uint64_t cap);
    // liveness (include/rmc.h "liveness over the state graph")
    void eventually(const rmc_live_query *q, rmc_live_result *res, uint32_t *within_out);
    void eventually_levels(uint64_t *must, uint64_t *avoid, uint32_t cap, uint32_t *n);
    void avoid_path(uint64_t gid, uint64_t *gids, uint32_t cap, uint32_t *len, int32_t *loop_at);
    void scc(rmc_scc_result *res, uint32_t *comp_out);

private:
    void grown() { csr = false; have_query = false; have_live = false; next_avoid.clear(); }
    void build_csr();
    void analysis_alloc();
    void analysis_free();
    uint64_t peel(uint32_t *rounds = nullptr);  // Kahn peeling on `work`: the states removed (the counters at 0)
    std::vector<uint64_t> last_can, last_cannot;
    // the last rmc_graph_eventually: `dist` holds within (a rmc_graph_reach in between takes it back)
    bool have_live = false;
    std::vector<uint64_t> last_must, last_avoid;
    std::vector<uint32_t> next_avoid;  // host copy, filled by the first avoid_path after a query
    uint32_t *comp = nullptr;          // rmc_graph_scc's labels, allocated by its first call
};
