// rmc_graph.hip -- the kept state graph and the analyses on it (rmc_graph.h; include/rmc.h
// "reachability queries").  Spec-independent: states are global ids, edges (src, dst) pairs.
//
// Kernels (gfx950, wave64, vector atomics only):
//   k_edge_append   a chunk's (src, dst) as u32 pairs behind the store
//   k_degrees       in-degree by dst, out-degree by src (all edges / without self-edges), self and back edge counts
//   k_scatter       reverse CSR: src into its dst's row through a per-row atomic cursor (row order unspecified)
//   k_targets       dist = 0 and frontier entry for the states of the target set
//   k_round<false>  backward BFS round: a wave per frontier state strides over its predecessor row; dist claimed by
//                   one CAS; the claimed states appended to the next frontier with one atomic per wave and 64 edges
//   k_peel_seed / k_round<true>  Kahn peeling on the out-degree counters, the same frontier shape with atomicSub
//   k_reach_stats   first state that cannot, per-level can / cannot counts
//   k_shape         degree histograms, maxima, sinks
//   k_round<true, true>  the attractor of rmc_graph_eventually: the peeling round on counters seeded with the whole
//                   out-degree, from the target set; a state whose counter reaches zero gets within = round
//   k_live_stats    terminal avoiders, the source set and its avoiders (leads-to)
//   k_next_seed / k_next_avoid  per avoider the smallest successor that is an avoider (edge-parallel atomicMin)
//   k_scc_*         strongly connected components: trimming (the peeling, then k_scc_trim_in on the in-edges), forward
//                   colour propagation (atomicMax per edge), the backward closure inside a colour (atomicOr per edge),
//                   min-gid labels and sizes; every round is one launch bounded by the edge or state count
// Every launch is bounded by the counts passed to it; frontiers hold each state at most once (a state
// enters when its CAS wins / its counter reaches zero), so n_states entries always suffice.
#include "rmc_graph.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstring>

namespace {

constexpr uint32_t UNSET = 0xFFFFFFFFu;
// accumulator words (KeptGraph::acc)
enum { A_SELF = 0, A_BACK, A_COUNT0, A_COUNT1, A_FIRST, A_SINKS, A_MAXIN, A_MAXOUT, A_INH, A_OUTH = A_INH + 64,
       A_LEVELS = A_OUTH + 64 };
constexpr uint32_t MAX_LEVELS = 4096;  // BFS levels reach_levels can report
// behind the level counts: rmc_graph_eventually's and rmc_graph_scc's words
enum { A_TERM = A_LEVELS + 2 * MAX_LEVELS, A_SRC, A_SRC_AVOID, A_SRC_FIRST, A_COMPS, A_NONTRIV, A_NT_STATES, A_LARGEST, A_END };
constexpr size_t ACC_WORDS = A_END;
constexpr uint32_t NOT_AVOIDER = 0xFFFFFFFEu;  // next_avoid of a state in `must` (gids stay below 2^31)
constexpr uint32_t IN_SCC = 0x80000000u;       // colour word: the state reaches its colour's root (likewise)

#define GCHK(x)                                                                                       \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess) throw GraphFail{RMC_E_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)}; \
    } while (0)

template <class T>
T *galloc(size_t n) {
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, (n ? n : 1) * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        throw GraphFail{RMC_E_MEMORY, "graph: hipMalloc(" + std::to_string(n * sizeof(T)) + " B): " + hipGetErrorString(e)};
    }
    return (T *)p;
}
template <class T>
void gfree(T *&p) {
    if (p) (void)hipFree((void *)p);
    p = nullptr;
}

unsigned grid_of(uint64_t items, unsigned per_block, unsigned cap = 8192) {
    const uint64_t b = (items + per_block - 1) / per_block;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(b, cap));
}

// ---- device helpers ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}
// Appends v of the lanes with `take` to list[*count ..): one atomic per wave.  Every lane of the wave calls it.
__device__ __forceinline__ void wave_append(bool take, uint32_t v, uint32_t *list, unsigned long long *count) {
    const unsigned long long m = __ballot(take);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(m));
    base = __shfl(base, leader, 64);
    if (take) list[base + __popcll(m & ((1ull << lane) - 1ull))] = v;
}

// ---- kernels ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_edge_append(const unsigned long long *src, const unsigned long long *dst, uint64_t n,
                                                     uint2 *out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = make_uint2((uint32_t)src[i], (uint32_t)dst[i]);
}

// ideg[g] = edges into g (the host's exclusive scan turns the counts into row starts)
__global__ __launch_bounds__(256) void k_degrees(const uint2 *e, uint64_t n, uint32_t *ideg, uint32_t *out_all, uint32_t *out_ns,
                                                 unsigned long long *acc) {
    unsigned long long self = 0, back = 0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += step) {  // (whole waves: the sums below)
        const uint64_t i = base + threadIdx.x;
        if (i < n) {
            const uint2 p = e[i];
            atomicAdd(&ideg[p.y], 1u);
            atomicAdd(&out_all[p.x], 1u);
            if (p.x != p.y) atomicAdd(&out_ns[p.x], 1u);
            self += p.x == p.y;
            back += p.y < p.x;
        }
    }
    self = wave_sum(self);
    back = wave_sum(back);
    if ((threadIdx.x & 63) == 0) {
        if (self) atomicAdd(&acc[A_SELF], self);
        if (back) atomicAdd(&acc[A_BACK], back);
    }
}

__global__ __launch_bounds__(256) void k_scatter(const uint2 *e, uint64_t n, const uint32_t *row, uint32_t *cursor, uint32_t *col) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint2 p = e[i];
        col[row[p.y] + atomicAdd(&cursor[p.y], 1u)] = p.x;
    }
}

// want_set: bit `bit` must be set (TRUE) or clear (FALSE); a state whose evaluation raised the error is in neither set
__global__ __launch_bounds__(256) void k_targets(const uint16_t *inv, uint64_t n, uint32_t bit, uint32_t want_set, uint32_t *dist,
                                                 uint32_t *frontier, unsigned long long *count) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += step) {
        const uint64_t g = base + threadIdx.x;
        bool t = false;
        if (g < n) {
            const uint32_t v = inv[g];
            t = !((v >> (8 + bit)) & 1u) && ((v >> bit) & 1u) == want_set;
            if (t) dist[g] = 0u;
        }
        wave_append(t, (uint32_t)g, frontier, count);
    }
}

// PEEL = false: backward BFS round `round` (dist[p]: UNSET -> round).  PEEL = true: the frontier's states leave the
// graph; a predecessor whose last non-self edge into a present state goes leaves in the next round.
// PEEL and MARK (the attractor): the counters run on the same way, and the state whose counter reaches zero gets
// mark[p] = round -- unless it is marked already: a target's counter is counted down by its successors as every other
// state's, and a target is in the first frontier and in no later one.  (mark[p] of a target was written by an earlier
// launch; that of any other state is written by the one lane that saw its counter go 1 -> 0.)
template <bool PEEL, bool MARK = false>
__global__ __launch_bounds__(256) void k_round(const uint32_t *row, const uint32_t *col, const uint32_t *frontier, uint64_t nf,
                                               uint32_t round, uint32_t *word, uint32_t *next, unsigned long long *count,
                                               uint32_t *mark = nullptr) {
    const int lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t f = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); f < nf; f += waves) {
        const uint32_t v = frontier[f];
        const uint32_t r0 = row[v], r1 = row[v + 1];
        for (uint32_t b = r0; b < r1; b += 64) {  // (wave-uniform bounds: the ballot sees the whole wave)
            const uint32_t i = b + lane;
            bool take = false;
            uint32_t p = 0;
            if (i < r1) {
                p = col[i];
                if (p != v) {  // self-edges are ignored
                    if (PEEL) take = atomicSub(&word[p], 1u) == 1u;
                    else take = atomicCAS(&word[p], UNSET, round) == UNSET;
                    if (MARK) {
                        take = take && mark[p] == UNSET;
                        if (take) mark[p] = round;
                    }
                }
            }
            wave_append(take, p, next, count);
        }
    }
}

__global__ __launch_bounds__(256) void k_peel_seed(const uint32_t *out_ns, uint64_t n, uint32_t *cnt, uint32_t *frontier,
                                                   unsigned long long *count) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += step) {
        const uint64_t g = base + threadIdx.x;
        bool t = false;
        if (g < n) {
            const uint32_t c = out_ns[g];
            cnt[g] = c;
            t = c == 0u;
        }
        wave_append(t, (uint32_t)g, frontier, count);
    }
}

// lv[0 .. nl] = level starts (lv[nl] = n); per level the states that can / cannot; the smallest gid that cannot
__global__ __launch_bounds__(256) void k_reach_stats(const uint32_t *dist, uint64_t n, const uint32_t *lv, uint32_t nl,
                                                     unsigned long long *acc) {
    const int lane = threadIdx.x & 63;
    unsigned long long first = ~0ull;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += step) {
        const uint64_t g = base + threadIdx.x;
        const bool in = g < n;
        bool can = false;
        uint32_t L = 0;
        if (in) {
            can = dist[g] != UNSET;
            if (!can && g < first) first = g;
            uint32_t lo = 0, hi = nl;  // the last level whose start is <= g
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (lv[mid] <= g) lo = mid; else hi = mid;
            }
            L = lo;
        }
        // consecutive gids: a wave meets one level, seldom two or more
        unsigned long long todo = __ballot(in);
        while (todo) {
            const int ld = __ffsll((long long)todo) - 1;
            const uint32_t Ll = __shfl(L, ld, 64);
            const unsigned long long same = __ballot(in && L == Ll);
            const unsigned long long cm = __ballot(in && L == Ll && can);
            if (lane == ld) {
                const unsigned long long c = __popcll(cm), x = __popcll(same) - c;
                if (c) atomicAdd(&acc[A_LEVELS + 2 * Ll], c);
                if (x) atomicAdd(&acc[A_LEVELS + 2 * Ll + 1], x);
            }
            todo &= ~same;
        }
    }
    first = wave_min(first);
    if (lane == 0 && first != ~0ull) atomicMin(&acc[A_FIRST], first);
}

__global__ __launch_bounds__(256) void k_shape(const uint32_t *row, const uint32_t *out_all, uint64_t n, unsigned long long *acc) {
    __shared__ uint32_t h[128];
    if (threadIdx.x < 128) h[threadIdx.x] = 0u;
    __syncthreads();
    unsigned long long mi = 0, mo = 0, sinks = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t di = row[g + 1] - row[g], dout = out_all[g];
        atomicAdd(&h[di < 63u ? di : 63u], 1u);
        atomicAdd(&h[64 + (dout < 63u ? dout : 63u)], 1u);
        mi = di > mi ? di : mi;
        mo = dout > mo ? dout : mo;
        sinks += dout == 0u;
    }
    mi = wave_max(mi);
    mo = wave_max(mo);
    sinks = wave_sum(sinks);
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&acc[A_MAXIN], mi);
        atomicMax(&acc[A_MAXOUT], mo);
        if (sinks) atomicAdd(&acc[A_SINKS], sinks);
    }
    __syncthreads();
    if (threadIdx.x < 128 && h[threadIdx.x]) atomicAdd(&acc[A_INH + threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// ---- inevitability ------------------------------------------------------------------------------------
// avoiders without a non-self edge out; with a source set (has_src) its size, its avoiders and the first of them
__global__ __launch_bounds__(256) void k_live_stats(const uint32_t *within, const uint32_t *out_ns, const uint16_t *inv, uint64_t n,
                                                    uint32_t has_src, uint32_t bit, uint32_t want_set, unsigned long long *acc) {
    unsigned long long term = 0, srcs = 0, sav = 0, first = ~0ull;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (uint64_t)gridDim.x * blockDim.x) {
        const bool avoid = within[g] == UNSET;
        term += avoid && out_ns[g] == 0u;
        if (has_src) {
            const uint32_t v = inv[g];
            const bool s = !((v >> (8 + bit)) & 1u) && ((v >> bit) & 1u) == want_set;
            srcs += s;
            sav += s && avoid;
            if (s && avoid && g < first) first = g;
        }
    }
    term = wave_sum(term);
    srcs = wave_sum(srcs);
    sav = wave_sum(sav);
    first = wave_min(first);
    if ((threadIdx.x & 63) == 0) {
        if (term) atomicAdd(&acc[A_TERM], term);
        if (srcs) atomicAdd(&acc[A_SRC], srcs);
        if (sav) atomicAdd(&acc[A_SRC_AVOID], sav);
        if (first != ~0ull) atomicMin(&acc[A_SRC_FIRST], first);
    }
}

__global__ __launch_bounds__(256) void k_next_seed(const uint32_t *within, uint64_t n, uint32_t *next) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (uint64_t)gridDim.x * blockDim.x)
        next[g] = within[g] == UNSET ? UNSET : NOT_AVOIDER;
}

// next[s] = the smallest dst over the non-self edges from an avoider s into an avoider (UNSET stays: s is terminal)
__global__ __launch_bounds__(256) void k_next_avoid(const uint2 *e, uint64_t n, const uint32_t *within, uint32_t *next) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint2 p = e[i];
        if (p.x != p.y && within[p.x] == UNSET && within[p.y] == UNSET) atomicMin(&next[p.x], p.y);
    }
}

// ---- strongly connected components --------------------------------------------------------------------
// comp[g] = UNSET while g is present.  After the peeling cnt[g] == 0 exactly on the states it removed.
__global__ __launch_bounds__(256) void k_scc_seed(const uint32_t *cnt, uint64_t n, uint32_t *comp) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (uint64_t)gridDim.x * blockDim.x)
        comp[g] = cnt[g] == 0u ? (uint32_t)g : UNSET;
}

// A wave per present state: it leaves as a component of its own when no non-self edge comes in from a present state.
// (A predecessor that leaves in the same launch may be seen either way; the fixpoint over the launches is the same.)
__global__ __launch_bounds__(256) void k_scc_trim_in(const uint32_t *row, const uint32_t *col, uint64_t n, uint32_t *comp,
                                                     unsigned long long *count) {
    const int lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    unsigned long long gone = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); g < n; g += waves) {
        if (comp[g] != UNSET) continue;  // (wave-uniform)
        const uint32_t r0 = row[g], r1 = row[g + 1];
        bool fed = false;
        for (uint32_t b = r0; b < r1 && !fed; b += 64) {
            const uint32_t i = b + lane;
            bool in = false;
            if (i < r1) {
                const uint32_t p = col[i];
                in = p != (uint32_t)g && comp[p] == UNSET;
            }
            fed = __ballot(in) != 0ull;
        }
        if (!fed) {
            if (lane == 0) comp[g] = (uint32_t)g;
            gone++;
        }
    }
    if (lane == 0 && gone) atomicAdd(count, gone);
}

// present states: colour = own gid, flag clear
__global__ __launch_bounds__(256) void k_scc_colour_seed(const uint32_t *comp, uint64_t n, uint32_t *colour) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (uint64_t)gridDim.x * blockDim.x)
        if (comp[g] == UNSET) colour[g] = (uint32_t)g;
}

// one round of forward propagation over the present subgraph: colour[d] = max(colour[d], colour[s]); counts the raises
__global__ __launch_bounds__(256) void k_scc_colour(const uint2 *e, uint64_t n, const uint32_t *comp, uint32_t *colour,
                                                    unsigned long long *count) {
    unsigned long long ch = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint2 p = e[i];
        if (p.x == p.y || comp[p.x] != UNSET || comp[p.y] != UNSET) continue;
        const uint32_t cs = colour[p.x];
        if (cs > colour[p.y]) ch += atomicMax(&colour[p.y], cs) < cs;
    }
    ch = wave_sum(ch);
    if ((threadIdx.x & 63) == 0 && ch) atomicAdd(count, ch);
}

// the fixpoint reached: the state whose colour is its own gid roots that colour
__global__ __launch_bounds__(256) void k_scc_roots(const uint32_t *comp, uint64_t n, uint32_t *colour) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (uint64_t)gridDim.x * blockDim.x)
        if (comp[g] == UNSET && colour[g] == (uint32_t)g) colour[g] = (uint32_t)g | IN_SCC;
}

// one round of the backward closure inside each colour: s joins when an edge leads from it to a member of its colour
__global__ __launch_bounds__(256) void k_scc_back(const uint2 *e, uint64_t n, const uint32_t *comp, uint32_t *colour,
                                                  unsigned long long *count) {
    unsigned long long ch = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint2 p = e[i];
        if (p.x == p.y || comp[p.x] != UNSET || comp[p.y] != UNSET) continue;
        const uint32_t cs = colour[p.x], cd = colour[p.y];
        if ((cd & IN_SCC) && !(cs & IN_SCC) && (cd & ~IN_SCC) == cs) ch += !(atomicOr(&colour[p.x], IN_SCC) & IN_SCC);
    }
    ch = wave_sum(ch);
    if ((threadIdx.x & 63) == 0 && ch) atomicAdd(count, ch);
}

// the members found leave with their root's gid (the largest of the component) as the label; the rest start over
__global__ __launch_bounds__(256) void k_scc_commit(uint64_t n, uint32_t *comp, uint32_t *colour, unsigned long long *count) {
    unsigned long long gone = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (uint64_t)gridDim.x * blockDim.x) {
        if (comp[g] != UNSET) continue;
        const uint32_t c = colour[g];
        if (c & IN_SCC) {
            comp[g] = c & ~IN_SCC;
            gone++;
        } else {
            colour[g] = (uint32_t)g;
        }
    }
    gone = wave_sum(gone);
    if ((threadIdx.x & 63) == 0 && gone) atomicAdd(count, gone);
}

// low[label] = the smallest gid, size[label] = the number of states that carry the label (both zero / UNSET before)
__global__ __launch_bounds__(256) void k_scc_low(const uint32_t *comp, uint64_t n, uint32_t *low, uint32_t *size) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = comp[g];
        atomicMin(&low[c], (uint32_t)g);
        atomicAdd(&size[c], 1u);
    }
}

// the component counts, from the one state of each component that carries its own gid as the label (the root; a
// trimmed state); k_scc_relabel then turns the labels into the smallest gid of the component
__global__ __launch_bounds__(256) void k_scc_sizes(uint64_t n, const uint32_t *size, const uint32_t *comp, unsigned long long *acc) {
    unsigned long long comps = 0, nt = 0, nts = 0, big = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = comp[g];
        if (c == (uint32_t)g) {  // one state per component: its root
            const uint32_t sz = size[c];
            comps++;
            nt += sz >= 2u;
            nts += sz >= 2u ? sz : 0u;
            big = sz > big ? sz : big;
        }
    }
    comps = wave_sum(comps);
    nt = wave_sum(nt);
    nts = wave_sum(nts);
    big = wave_max(big);
    if ((threadIdx.x & 63) == 0) {
        if (comps) atomicAdd(&acc[A_COMPS], comps);
        if (nt) atomicAdd(&acc[A_NONTRIV], nt);
        if (nts) atomicAdd(&acc[A_NT_STATES], nts);
        atomicMax(&acc[A_LARGEST], big);
    }
}

__global__ __launch_bounds__(256) void k_scc_relabel(uint64_t n, const uint32_t *low, uint32_t *comp) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (uint64_t)gridDim.x * blockDim.x)
        comp[g] = low[comp[g]];
}

}  // namespace

// ---- the store ------------------------------------------------------------------------------------
void KeptGraph::analysis_free() {
    gfree(row); gfree(col); gfree(out_all); gfree(out_ns); gfree(work); gfree(fr[0]); gfree(fr[1]); gfree(dist); gfree(tmp);
    gfree(comp);
    tmp_bytes = 0;
    a_states = a_edges = 0;
    csr = have_query = have_live = false;
}

void KeptGraph::free_all() {
    analysis_free();
    gfree(edges); gfree(inv); gfree(acc);
    if (hacc) (void)hipHostFree(hacc);
    hacc = nullptr;
    n_edges = e_cap = n_states = s_cap = 0;
    level_start.clear();
}

void KeptGraph::clear() {
    n_edges = n_states = 0;
    level_start.clear();
    grown();
}

void KeptGraph::reserve_states(uint64_t n) {
    if (n >= (1ull << 32)) throw GraphFail{RMC_E_MEMORY, "graph keep: 2^32 states or more"};
    if (n <= s_cap) return;
    uint64_t nc = std::max<uint64_t>(s_cap, 1024);
    while (nc < n) nc *= 2;
    uint16_t *ni = galloc<uint16_t>(nc);
    if (n_states) {
        hipError_t e = hipMemcpyAsync(ni, inv, n_states * 2, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) {
            gfree(ni);
            GCHK(e);
        }
    } else {
        GCHK(hipStreamSynchronize(stream));
    }
    gfree(inv);
    inv = ni;
    s_cap = nc;
}

void KeptGraph::append_edges(const unsigned long long *src, const unsigned long long *dst, uint64_t n) {
    if (!n) return;
    const uint64_t need = n_edges + n;
    if (need >= (1ull << 32)) throw GraphFail{RMC_E_MEMORY, "graph keep: 2^32 edges or more"};
    if (need > e_cap) {
        uint64_t nc = std::max<uint64_t>(e_cap, 4096);
        while (nc < need) nc *= 2;
        uint2 *ne = galloc<uint2>(nc);
        hipError_t e = n_edges ? hipMemcpyAsync(ne, edges, n_edges * sizeof(uint2), hipMemcpyDeviceToDevice, stream) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) {
            gfree(ne);
            GCHK(e);
        }
        gfree(edges);
        edges = ne;
        e_cap = nc;
    }
    hipLaunchKernelGGL(k_edge_append, dim3(grid_of(n, 256)), dim3(256), 0, stream, src, dst, n, edges + n_edges);
    n_edges = need;
    grown();
}

void KeptGraph::import(uint64_t ns, uint64_t ne, const uint32_t *src, const uint32_t *dst, const uint16_t *iv) {
    if (!ns) throw GraphFail{RMC_E_ARG, "rmc_graph_import: no states"};
    if (ne && (!src || !dst)) throw GraphFail{RMC_E_ARG, "rmc_graph_import: null edge arrays"};
    if (!iv) throw GraphFail{RMC_E_ARG, "rmc_graph_import: null invariant values"};
    if (ns >= (1ull << 32) || ne >= (1ull << 32)) throw GraphFail{RMC_E_MEMORY, "rmc_graph_import: 2^32 states or edges, or more"};
    std::vector<uint2> pairs(ne);
    for (uint64_t i = 0; i < ne; i++) {
        if (src[i] >= ns || dst[i] >= ns) throw GraphFail{RMC_E_ARG, "rmc_graph_import: edge " + std::to_string(i) + " names a state past n_states"};
        pairs[i] = make_uint2(src[i], dst[i]);
    }
    clear();
    reserve_states(ns);
    if (ne > e_cap) {
        GCHK(hipStreamSynchronize(stream));
        uint64_t nc = std::max<uint64_t>(e_cap, 4096);
        while (nc < ne) nc *= 2;
        uint2 *nb = galloc<uint2>(nc);
        gfree(edges);
        edges = nb;
        e_cap = nc;
    }
    GCHK(hipMemcpyAsync(inv, iv, ns * 2, hipMemcpyHostToDevice, stream));
    if (ne) GCHK(hipMemcpyAsync(edges, pairs.data(), ne * sizeof(uint2), hipMemcpyHostToDevice, stream));
    GCHK(hipStreamSynchronize(stream));
    n_states = ns;
    n_edges = ne;
    level_start.assign(1, 0);
    grown();
}

void KeptGraph::inv_values(uint16_t *out, uint64_t cap) {
    if (!out) throw GraphFail{RMC_E_ARG, "rmc_graph_inv_values: null buffer"};
    if (cap < n_states) throw GraphFail{RMC_E_ARG, "rmc_graph_inv_values: buffer too small"};
    GCHK(hipMemcpyAsync(out, inv, n_states * 2, hipMemcpyDeviceToHost, stream));
    GCHK(hipStreamSynchronize(stream));
}

// ---- reverse CSR --------------------------------------------------------------------------------------
void KeptGraph::analysis_alloc() {
    if (!acc) {
        acc = galloc<unsigned long long>(ACC_WORDS);
        GCHK(hipHostMalloc((void **)&hacc, ACC_WORDS * 8, hipHostMallocDefault));
    }
    if (n_states > a_states || n_edges > a_edges) {
        GCHK(hipStreamSynchronize(stream));
        analysis_free();
        const uint64_t ns = n_states, ne = n_edges;
        row = galloc<uint32_t>(ns + 1);
        col = galloc<uint32_t>(ne);
        out_all = galloc<uint32_t>(ns);
        out_ns = galloc<uint32_t>(ns);
        work = galloc<uint32_t>(ns + 1);
        fr[0] = galloc<uint32_t>(ns);
        fr[1] = galloc<uint32_t>(ns);
        dist = galloc<uint32_t>(ns);
        size_t t = 0;
        GCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, t, work, row, (int)std::min<uint64_t>(ns + 1, 0x7FFFFFFFull), stream));
        tmp = galloc<uint8_t>(t);
        tmp_bytes = t;
        a_states = ns;
        a_edges = ne;
    }
}

void KeptGraph::build_csr() {
    if (csr) return;
    if (n_states + 1 > 0x7FFFFFFFull) throw GraphFail{RMC_E_MEMORY, "graph: more states than the row scan takes (2^31 - 2)"};
    analysis_alloc();
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t ns = n_states, ne = n_edges;
    GCHK(hipMemsetAsync(work, 0, (ns + 1) * 4, stream));
    GCHK(hipMemsetAsync(out_all, 0, ns * 4, stream));
    GCHK(hipMemsetAsync(out_ns, 0, ns * 4, stream));
    GCHK(hipMemsetAsync(acc, 0, 2 * 8, stream));
    if (ne) hipLaunchKernelGGL(k_degrees, dim3(grid_of(ne, 256)), dim3(256), 0, stream, edges, ne, work, out_all, out_ns, acc);
    // (counts by dst sit at work[g]; scanning ns + 1 of them gives row[g] = edges into states below g, row[ns] = ne)
    GCHK(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, work, row, (int)(ns + 1), stream));
    GCHK(hipMemsetAsync(work, 0, (ns + 1) * 4, stream));
    if (ne) hipLaunchKernelGGL(k_scatter, dim3(grid_of(ne, 256)), dim3(256), 0, stream, edges, ne, row, work, col);
    GCHK(hipMemcpyAsync(hacc, acc, 2 * 8, hipMemcpyDeviceToHost, stream));
    GCHK(hipStreamSynchronize(stream));
    GCHK(hipGetLastError());
    self_edges = hacc[A_SELF];
    back_edges = hacc[A_BACK];
    csr_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    csr = true;
}

// ---- analyses -------------------------------------------------------------------------------------------
void KeptGraph::reach(const rmc_reach_query *q, rmc_reach_result *res, uint32_t *dist_out) {
    if (!q || !res) throw GraphFail{RMC_E_ARG, "rmc_graph_reach: null argument"};
    if (q->invariant_bit >= 7 || (q->value != 0 && q->value != 1))
        throw GraphFail{RMC_E_ARG, "rmc_graph_reach: invariant_bit 0..6, value 0 or 1"};
    const uint32_t nl = (uint32_t)level_start.size();
    if (nl > MAX_LEVELS) throw GraphFail{RMC_E_ARG, "rmc_graph_reach: more BFS levels than the per-level counts hold"};
    have_query = have_live = false;  // (dist is about to hold this query's distances)
    build_csr();
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t ns = n_states;
    std::memset(res, 0, sizeof *res);
    GCHK(hipMemsetAsync(dist, 0xFF, ns * 4, stream));
    GCHK(hipMemsetAsync(acc + A_COUNT0, 0, 2 * 8, stream));
    hipLaunchKernelGGL(k_targets, dim3(grid_of(ns, 256)), dim3(256), 0, stream, inv, ns, q->invariant_bit, (uint32_t)q->value, dist,
                       fr[0], acc + A_COUNT0);
    GCHK(hipMemcpyAsync(hacc + A_COUNT0, acc + A_COUNT0, 8, hipMemcpyDeviceToHost, stream));
    GCHK(hipStreamSynchronize(stream));
    uint64_t nf = hacc[A_COUNT0], can = nf;
    res->targets = nf;
    uint32_t round = 0, maxd = 0;
    int cur = 0;
    while (nf) {
        round++;
        unsigned long long *cnt = acc + A_COUNT0 + (cur ^ 1);
        GCHK(hipMemsetAsync(cnt, 0, 8, stream));
        hipLaunchKernelGGL((k_round<false>), dim3(grid_of(nf, 4)), dim3(256), 0, stream, row, col, fr[cur], nf, round, dist,
                           fr[cur ^ 1], cnt);
        GCHK(hipMemcpyAsync(hacc + A_COUNT0, cnt, 4, hipMemcpyDeviceToHost, stream));  // (fewer than 2^32 states: the low word)
        GCHK(hipStreamSynchronize(stream));
        nf = (uint32_t)hacc[A_COUNT0];
        if (nf) maxd = round;
        can += nf;
        cur ^= 1;
    }
    // the first state that cannot, the per-level counts
    std::vector<uint32_t> lv(nl + 1);
    for (uint32_t l = 0; l < nl; l++) lv[l] = (uint32_t)level_start[l];
    lv[nl] = (uint32_t)ns;
    GCHK(hipMemcpyAsync(work, lv.data(), (nl + 1) * 4, hipMemcpyHostToDevice, stream));  // (work: ns + 1 >= nl + 1 words)
    GCHK(hipMemsetAsync(acc + A_FIRST, 0xFF, 8, stream));
    GCHK(hipMemsetAsync(acc + A_LEVELS, 0, (size_t)2 * nl * 8, stream));
    hipLaunchKernelGGL(k_reach_stats, dim3(grid_of(ns, 256)), dim3(256), 0, stream, dist, ns, work, nl, acc);
    GCHK(hipMemcpyAsync(hacc + A_FIRST, acc + A_FIRST, 8, hipMemcpyDeviceToHost, stream));
    GCHK(hipMemcpyAsync(hacc + A_LEVELS, acc + A_LEVELS, (size_t)2 * nl * 8, hipMemcpyDeviceToHost, stream));
    uint32_t d0 = UNSET;
    GCHK(hipMemcpyAsync(&d0, dist, 4, hipMemcpyDeviceToHost, stream));
    if (dist_out) GCHK(hipMemcpyAsync(dist_out, dist, ns * 4, hipMemcpyDeviceToHost, stream));
    GCHK(hipStreamSynchronize(stream));
    GCHK(hipGetLastError());
    last_can.assign(nl, 0);
    last_cannot.assign(nl, 0);
    for (uint32_t l = 0; l < nl; l++) {
        last_can[l] = hacc[A_LEVELS + 2 * l];
        last_cannot[l] = hacc[A_LEVELS + 2 * l + 1];
    }
    res->states = ns;
    res->edges = n_edges;
    res->self_edges = self_edges;
    res->can_reach = can;
    res->cannot_reach = ns - can;
    res->first_cannot = hacc[A_FIRST];
    res->first_cannot_level = 0;
    if (res->first_cannot != ~0ull)
        res->first_cannot_level =
            (int32_t)(std::upper_bound(level_start.begin(), level_start.end(), res->first_cannot) - level_start.begin());
    res->max_distance = (int32_t)maxd;
    res->init_distance = d0 == UNSET ? -1 : (int32_t)d0;
    res->rounds = round;
    res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    res->csr_seconds = csr_seconds;
    have_query = true;
}

void KeptGraph::reach_levels(uint64_t *can, uint64_t *cannot, uint32_t cap, uint32_t *n) {
    if (!can || !cannot || !n) throw GraphFail{RMC_E_ARG, "rmc_graph_reach_levels: null argument"};
    if (!have_query) throw GraphFail{RMC_E_STATE, "rmc_graph_reach_levels: no query on this graph (rmc_graph_reach)"};
    *n = (uint32_t)last_can.size();
    if (last_can.size() > cap) throw GraphFail{RMC_E_ARG, "rmc_graph_reach_levels: buffer too small"};
    for (size_t l = 0; l < last_can.size(); l++) {
        can[l] = last_can[l];
        cannot[l] = last_cannot[l];
    }
}

void KeptGraph::shape(struct rmc_graph_shape *out) {
    if (!out) throw GraphFail{RMC_E_ARG, "rmc_graph_shape: null argument"};
    build_csr();
    const uint64_t ns = n_states;
    std::memset(out, 0, sizeof *out);
    GCHK(hipMemsetAsync(acc + A_SINKS, 0, (A_LEVELS - A_SINKS) * 8, stream));
    hipLaunchKernelGGL(k_shape, dim3(grid_of(ns, 256, 1024)), dim3(256), 0, stream, row, out_all, ns, acc);
    GCHK(hipMemcpyAsync(hacc + A_SINKS, acc + A_SINKS, (A_LEVELS - A_SINKS) * 8, hipMemcpyDeviceToHost, stream));
    const uint64_t removed = peel();
    GCHK(hipGetLastError());
    out->states = ns;
    out->edges = n_edges;
    out->self_edges = self_edges;
    out->back_edges = back_edges;
    out->sinks = hacc[A_SINKS];
    out->max_in = hacc[A_MAXIN];
    out->max_out = hacc[A_MAXOUT];
    out->cyclic_states = ns - removed;
    for (int b = 0; b < 64; b++) {
        out->in_hist[b] = hacc[A_INH + b];
        out->out_hist[b] = hacc[A_OUTH + b];
    }
}

// Kahn peeling: the states without a non-self edge into a present state leave, round after round
uint64_t KeptGraph::peel(uint32_t *rounds) {
    const uint64_t ns = n_states;
    GCHK(hipMemsetAsync(acc + A_COUNT0, 0, 8, stream));
    hipLaunchKernelGGL(k_peel_seed, dim3(grid_of(ns, 256)), dim3(256), 0, stream, out_ns, ns, work, fr[0], acc + A_COUNT0);
    GCHK(hipMemcpyAsync(hacc + A_COUNT0, acc + A_COUNT0, 8, hipMemcpyDeviceToHost, stream));
    GCHK(hipStreamSynchronize(stream));
    uint64_t nf = hacc[A_COUNT0], removed = nf;
    uint32_t r = 1;
    int cur = 0;
    while (nf) {
        unsigned long long *cnt = acc + A_COUNT0 + (cur ^ 1);
        GCHK(hipMemsetAsync(cnt, 0, 8, stream));
        hipLaunchKernelGGL((k_round<true>), dim3(grid_of(nf, 4)), dim3(256), 0, stream, row, col, fr[cur], nf, 0u, work, fr[cur ^ 1],
                           cnt, (uint32_t *)nullptr);
        GCHK(hipMemcpyAsync(hacc + A_COUNT0, cnt, 4, hipMemcpyDeviceToHost, stream));
        GCHK(hipStreamSynchronize(stream));
        nf = (uint32_t)hacc[A_COUNT0];
        removed += nf;
        cur ^= 1;
        r++;
    }
    if (rounds) *rounds = r;
    return removed;
}

// ---- liveness -------------------------------------------------------------------------------------------
void KeptGraph::eventually(const rmc_live_query *q, rmc_live_result *res, uint32_t *within_out) {
    if (!q || !res) throw GraphFail{RMC_E_ARG, "rmc_graph_eventually: null argument"};
    if (q->invariant_bit >= 7 || (q->value != 0 && q->value != 1))
        throw GraphFail{RMC_E_ARG, "rmc_graph_eventually: invariant_bit 0..6, value 0 or 1"};
    if (q->source_bit < -1 || q->source_bit >= 7 || (q->source_value != 0 && q->source_value != 1))
        throw GraphFail{RMC_E_ARG, "rmc_graph_eventually: source_bit -1 (none) or 0..6, source_value 0 or 1"};
    const uint32_t nl = (uint32_t)level_start.size();
    if (nl > MAX_LEVELS) throw GraphFail{RMC_E_ARG, "rmc_graph_eventually: more BFS levels than the per-level counts hold"};
    have_query = have_live = false;  // (dist is about to hold this query's within)
    next_avoid.clear();
    build_csr();
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t ns = n_states;
    const bool has_src = q->source_bit >= 0;
    std::memset(res, 0, sizeof *res);
    uint32_t *within = dist;
    // counters: the whole out-degree without self-edges; the first frontier: the target set with within = 0
    GCHK(hipMemcpyAsync(work, out_ns, ns * 4, hipMemcpyDeviceToDevice, stream));
    GCHK(hipMemsetAsync(within, 0xFF, ns * 4, stream));
    GCHK(hipMemsetAsync(acc + A_COUNT0, 0, 2 * 8, stream));
    hipLaunchKernelGGL(k_targets, dim3(grid_of(ns, 256)), dim3(256), 0, stream, inv, ns, q->invariant_bit, (uint32_t)q->value, within,
                       fr[0], acc + A_COUNT0);
    GCHK(hipMemcpyAsync(hacc + A_COUNT0, acc + A_COUNT0, 8, hipMemcpyDeviceToHost, stream));
    GCHK(hipStreamSynchronize(stream));
    uint64_t nf = hacc[A_COUNT0], must = nf;
    res->targets = nf;
    uint32_t round = 0, maxw = 0;
    int cur = 0;
    while (nf) {
        round++;
        if (must > ns) throw GraphFail{RMC_E_DEVICE, "rmc_graph_eventually: a state entered two frontiers"};
        unsigned long long *cnt = acc + A_COUNT0 + (cur ^ 1);
        GCHK(hipMemsetAsync(cnt, 0, 8, stream));
        hipLaunchKernelGGL((k_round<true, true>), dim3(grid_of(nf, 4)), dim3(256), 0, stream, row, col, fr[cur], nf, round, work,
                           fr[cur ^ 1], cnt, within);
        GCHK(hipMemcpyAsync(hacc + A_COUNT0, cnt, 4, hipMemcpyDeviceToHost, stream));  // (fewer than 2^32 states: the low word)
        GCHK(hipStreamSynchronize(stream));
        nf = (uint32_t)hacc[A_COUNT0];
        if (nf) maxw = round;
        must += nf;
        cur ^= 1;
    }
    // the first avoider and the per-level counts (k_reach_stats reads within as it reads dist), then the rest
    std::vector<uint32_t> lv(nl + 1);
    for (uint32_t l = 0; l < nl; l++) lv[l] = (uint32_t)level_start[l];
    lv[nl] = (uint32_t)ns;
    GCHK(hipMemcpyAsync(work, lv.data(), (nl + 1) * 4, hipMemcpyHostToDevice, stream));  // (work: ns + 1 >= nl + 1 words)
    GCHK(hipMemsetAsync(acc + A_FIRST, 0xFF, 8, stream));
    GCHK(hipMemsetAsync(acc + A_LEVELS, 0, (size_t)2 * nl * 8, stream));
    GCHK(hipMemsetAsync(acc + A_TERM, 0, 3 * 8, stream));
    GCHK(hipMemsetAsync(acc + A_SRC_FIRST, 0xFF, 8, stream));
    hipLaunchKernelGGL(k_reach_stats, dim3(grid_of(ns, 256)), dim3(256), 0, stream, within, ns, work, nl, acc);
    hipLaunchKernelGGL(k_live_stats, dim3(grid_of(ns, 256, 1024)), dim3(256), 0, stream, within, out_ns, inv, ns, has_src ? 1u : 0u,
                       has_src ? (uint32_t)q->source_bit : 0u, (uint32_t)q->source_value, acc);
    GCHK(hipMemcpyAsync(hacc + A_FIRST, acc + A_FIRST, 8, hipMemcpyDeviceToHost, stream));
    GCHK(hipMemcpyAsync(hacc + A_LEVELS, acc + A_LEVELS, (size_t)2 * nl * 8, hipMemcpyDeviceToHost, stream));
    GCHK(hipMemcpyAsync(hacc + A_TERM, acc + A_TERM, 4 * 8, hipMemcpyDeviceToHost, stream));
    uint32_t w0 = UNSET;
    GCHK(hipMemcpyAsync(&w0, within, 4, hipMemcpyDeviceToHost, stream));
    if (within_out) GCHK(hipMemcpyAsync(within_out, within, ns * 4, hipMemcpyDeviceToHost, stream));
    GCHK(hipStreamSynchronize(stream));
    GCHK(hipGetLastError());
    last_must.assign(nl, 0);
    last_avoid.assign(nl, 0);
    for (uint32_t l = 0; l < nl; l++) {
        last_must[l] = hacc[A_LEVELS + 2 * l];
        last_avoid[l] = hacc[A_LEVELS + 2 * l + 1];
    }
    auto level_of = [&](uint64_t g) {
        return g == ~0ull ? 0 : (int32_t)(std::upper_bound(level_start.begin(), level_start.end(), g) - level_start.begin());
    };
    res->states = ns;
    res->edges = n_edges;
    res->self_edges = self_edges;
    res->must = must;
    res->avoiders = ns - must;
    res->avoid_terminal = hacc[A_TERM];
    res->first_avoid = hacc[A_FIRST];
    res->first_avoid_level = level_of(res->first_avoid);
    res->sources = hacc[A_SRC];
    res->source_avoiders = hacc[A_SRC_AVOID];
    res->first_source_avoid = hacc[A_SRC_FIRST];
    res->first_source_avoid_level = level_of(res->first_source_avoid);
    res->max_within = (int32_t)maxw;
    res->init_within = w0 == UNSET ? -1 : (int32_t)w0;
    res->rounds = round;
    res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    res->csr_seconds = csr_seconds;
    have_live = true;
}

void KeptGraph::eventually_levels(uint64_t *must, uint64_t *avoid, uint32_t cap, uint32_t *n) {
    if (!must || !avoid || !n) throw GraphFail{RMC_E_ARG, "rmc_graph_eventually_levels: null argument"};
    if (!have_live) throw GraphFail{RMC_E_STATE, "rmc_graph_eventually_levels: no query on this graph (rmc_graph_eventually)"};
    *n = (uint32_t)last_must.size();
    if (last_must.size() > cap) throw GraphFail{RMC_E_ARG, "rmc_graph_eventually_levels: buffer too small"};
    for (size_t l = 0; l < last_must.size(); l++) {
        must[l] = last_must[l];
        avoid[l] = last_avoid[l];
    }
}

void KeptGraph::avoid_path(uint64_t gid, uint64_t *gids, uint32_t cap, uint32_t *len, int32_t *loop_at) {
    if (!gids || !len || !loop_at) throw GraphFail{RMC_E_ARG, "rmc_graph_avoid_path: null argument"};
    if (!have_live) throw GraphFail{RMC_E_STATE, "rmc_graph_avoid_path: no query on this graph (rmc_graph_eventually)"};
    const uint64_t ns = n_states;
    if (next_avoid.empty()) {  // one edge-parallel pass over the store; fr[0] is free between queries
        GCHK(hipStreamSynchronize(stream));
        hipLaunchKernelGGL(k_next_seed, dim3(grid_of(ns, 256)), dim3(256), 0, stream, dist, ns, fr[0]);
        if (n_edges)
            hipLaunchKernelGGL(k_next_avoid, dim3(grid_of(n_edges, 256)), dim3(256), 0, stream, edges, n_edges, dist, fr[0]);
        std::vector<uint32_t> nx(ns);
        GCHK(hipMemcpyAsync(nx.data(), fr[0], ns * 4, hipMemcpyDeviceToHost, stream));
        GCHK(hipStreamSynchronize(stream));
        GCHK(hipGetLastError());
        next_avoid.swap(nx);
    }
    if (gid >= ns || next_avoid[gid] == NOT_AVOIDER)
        throw GraphFail{RMC_E_ARG, "rmc_graph_avoid_path: state " + std::to_string(gid) + " is no avoider of the last query"};
    // follow next_avoid until it ends or names a state of the path
    std::vector<uint64_t> path;
    int32_t loop = -1;
    {
        std::vector<uint32_t> idx;  // by gid, allocated only for walks past 64 states
        uint32_t g = (uint32_t)gid;
        for (;;) {
            if (path.size() == 64 && idx.empty()) {
                idx.assign(ns, UNSET);
                for (size_t i = 0; i < path.size(); i++) idx[path[i]] = (uint32_t)i;
            }
            if (!idx.empty()) idx[g] = (uint32_t)path.size();
            path.push_back(g);
            const uint32_t nx = next_avoid[g];
            if (nx == UNSET) break;  // a terminal avoider
            uint32_t seen = UNSET;
            if (!idx.empty()) seen = idx[nx];
            else
                for (size_t i = 0; i < path.size(); i++)
                    if (path[i] == nx) seen = (uint32_t)i;
            if (seen != UNSET) {
                loop = (int32_t)seen;
                break;
            }
            g = nx;
        }
    }
    *len = (uint32_t)path.size();
    *loop_at = loop;
    if (path.size() > cap) throw GraphFail{RMC_E_ARG, "rmc_graph_avoid_path: buffer too small (" + std::to_string(path.size()) + " states)"};
    std::copy(path.begin(), path.end(), gids);
}

void KeptGraph::scc(rmc_scc_result *res, uint32_t *comp_out) {
    if (!res) throw GraphFail{RMC_E_ARG, "rmc_graph_scc: null argument"};
    build_csr();
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t ns = n_states, ne = n_edges;
    std::memset(res, 0, sizeof *res);
    if (!comp) comp = galloc<uint32_t>(a_states);
    const dim3 gs(grid_of(ns, 256)), ge(grid_of(ne, 256)), blk(256);
    unsigned long long *cnt = acc + A_COUNT0;
    // the count of the launch before it (states gone / words changed): a round the host reads
    uint32_t rounds = 0;
    auto read_count = [&]() -> uint64_t {
        GCHK(hipMemcpyAsync(hacc + A_COUNT0, cnt, 8, hipMemcpyDeviceToHost, stream));
        GCHK(hipStreamSynchronize(stream));
        rounds++;
        return hacc[A_COUNT0];
    };
    // trimming: the peeling removes what has no edge into a present state, then the same on the in-edges
    uint32_t peel_rounds = 0;
    uint64_t gone = peel(&peel_rounds);
    rounds += peel_rounds;
    hipLaunchKernelGGL(k_scc_seed, gs, blk, 0, stream, work, ns, comp);
    for (uint64_t r = 0; gone < ns; r++) {
        if (r > ns) throw GraphFail{RMC_E_DEVICE, "rmc_graph_scc: the trimming did not end"};
        GCHK(hipMemsetAsync(cnt, 0, 8, stream));
        hipLaunchKernelGGL(k_scc_trim_in, dim3(grid_of(ns, 4)), blk, 0, stream, row, col, ns, comp, cnt);
        const uint64_t k = read_count();
        gone += k;
        if (!k) break;
    }
    res->trimmed = gone;
    // colouring on what is left: forward max-gid propagation, the backward closure of each root inside its colour
    uint32_t *colour = fr[0];
    if (gone < ns) hipLaunchKernelGGL(k_scc_colour_seed, gs, blk, 0, stream, comp, ns, colour);
    for (uint64_t it = 0; gone < ns; it++) {
        if (it > ns) throw GraphFail{RMC_E_DEVICE, "rmc_graph_scc: the colouring did not end"};
        for (uint64_t r = 0;; r++) {
            if (r > ns) throw GraphFail{RMC_E_DEVICE, "rmc_graph_scc: the propagation did not end"};
            GCHK(hipMemsetAsync(cnt, 0, 8, stream));
            hipLaunchKernelGGL(k_scc_colour, ge, blk, 0, stream, edges, ne, comp, colour, cnt);
            if (!read_count()) break;
        }
        hipLaunchKernelGGL(k_scc_roots, gs, blk, 0, stream, comp, ns, colour);
        for (uint64_t r = 0;; r++) {
            if (r > ns) throw GraphFail{RMC_E_DEVICE, "rmc_graph_scc: the closure did not end"};
            GCHK(hipMemsetAsync(cnt, 0, 8, stream));
            hipLaunchKernelGGL(k_scc_back, ge, blk, 0, stream, edges, ne, comp, colour, cnt);
            if (!read_count()) break;
        }
        GCHK(hipMemsetAsync(cnt, 0, 8, stream));
        hipLaunchKernelGGL(k_scc_commit, gs, blk, 0, stream, ns, comp, colour, cnt);
        const uint64_t k = read_count();
        if (!k) throw GraphFail{RMC_E_DEVICE, "rmc_graph_scc: a colouring round found no component"};
        gone += k;
    }
    // labels: the smallest gid of each component; sizes
    uint32_t *low = fr[0], *size = fr[1];
    GCHK(hipMemsetAsync(low, 0xFF, ns * 4, stream));
    GCHK(hipMemsetAsync(size, 0, ns * 4, stream));
    GCHK(hipMemsetAsync(acc + A_COMPS, 0, 4 * 8, stream));
    hipLaunchKernelGGL(k_scc_low, gs, blk, 0, stream, comp, ns, low, size);
    hipLaunchKernelGGL(k_scc_sizes, dim3(grid_of(ns, 256, 1024)), blk, 0, stream, ns, size, comp, acc);
    hipLaunchKernelGGL(k_scc_relabel, gs, blk, 0, stream, ns, low, comp);
    GCHK(hipMemcpyAsync(hacc + A_COMPS, acc + A_COMPS, 4 * 8, hipMemcpyDeviceToHost, stream));
    if (comp_out) GCHK(hipMemcpyAsync(comp_out, comp, ns * 4, hipMemcpyDeviceToHost, stream));
    GCHK(hipStreamSynchronize(stream));
    GCHK(hipGetLastError());
    res->components = hacc[A_COMPS];
    res->nontrivial = hacc[A_NONTRIV];
    res->nontrivial_states = hacc[A_NT_STATES];
    res->largest = hacc[A_LARGEST];
    res->rounds = rounds;
    res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    res->csr_seconds = csr_seconds;
}
