// Round trip of the frontier record codec (tla-raft_amd/csrc/rmc_spec.h Codec): every field of
// the nibble core, drawn from its domain in Raft.tla (tla:93-105 initial values, the ranges the
// actions keep: terms <= MaxElection <= 7, indices <= |Vals| + 2, restarts <= 15, |msgs| <= 255),
// must come back bit-exact after encode_core -> decode_core, for every compiled (servers, values):
// on random cores (check), with every field swept over its whole domain up to the top value
// (check_domains), and for the message info word's fields (check_minfo).
#include <cstdint>
#include <cstdio>
#include <random>

#include "rmc_spec.h"

using namespace rmc;

template <int N, int V>
static int check(std::mt19937_64 &rng, int iters) {
    using L = Layout<N, V>;
    using C = Codec<N, V>;
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
    int bad = 0;
    for (int it = 0; it < iters; it++) {
        uint32_t c[L::NW] = {0}, w[C::CCW + 1] = {0}, d[L::NW] = {0};
        for (int i = 0; i < N; i++) {
            const uint32_t vf = pick(0, N);  // N = None
            c[L::W_VF] = setnib(c[L::W_VF], i, vf == (uint32_t)N ? VF_NONE : vf);
            c[L::W_CT] = setnib(c[L::W_CT], i, pick(0, 7));
            c[L::W_ROLE] = setnib(c[L::W_ROLE], i, pick(0, 2));
            c[L::W_CI] = setnib(c[L::W_CI], i, pick(1, V + 1));
            const uint32_t ll = pick(1, V + 1);
            c[L::W_LL] = setnib(c[L::W_LL], i, ll);
            for (uint32_t x = 2; x <= ll; x++)
                c[L::W_LOG + i] |= (pick(0, 7) | (pick(0, V - 1) << 4)) << (8 * (x - 2));
            for (int j = 0; j < N; j++) {
                c[L::W_MI + i] = setnib(c[L::W_MI + i], j, pick(1, V + 1));
                c[L::W_NI + i] = setnib(c[L::W_NI + i], j, pick(2, V + 2));
            }
        }
        c[L::W_PEND] = (uint32_t)(rng() & ((1ull << (N * N)) - 1));
        uint32_t misc = pick(0, 7) | (pick(0, 15) << 4) | (pick(0, 255) << 16);
        for (int v = 0; v < V; v++) misc |= pick(0, 1) << (8 + v);
        c[L::W_MISC] = misc;
        encode_core<N, V>(c, w);
        decode_core<N, V>(w, d);
        for (int k = 0; k < L::NW; k++)
            if (c[k] != d[k]) {
                if (bad < 5) std::printf("N=%d V=%d word %d: %08x -> %08x\n", N, V, k, c[k], d[k]);
                bad++;
            }
        if (core_nm<N, V>(w) != ((misc >> 16) & 0xFFu)) bad++;
        if (w[C::CCW] != 0) bad++;  // nothing beyond the packed words
    }
    std::printf("N=%d V=%d: %d bits in %d words, %d mismatches\n", N, V, C::BITS, C::CCW, bad);
    return bad;
}

// One core -> encode -> decode; counts the words that differ, |msgs| read back and a write past CCW.
template <int N, int V>
static int round_trip(const uint32_t *c) {
    using L = Layout<N, V>;
    using C = Codec<N, V>;
    uint32_t w[C::CCW + 1] = {0}, d[L::NW] = {0};
    int bad = 0;
    encode_core<N, V>(c, w);
    decode_core<N, V>(w, d);
    for (int k = 0; k < L::NW; k++)
        if (c[k] != d[k]) {
            if (bad < 5) std::printf("N=%d V=%d word %d: %08x -> %08x\n", N, V, k, c[k], d[k]);
            bad++;
        }
    if (core_nm<N, V>(w) != ((c[L::W_MISC] >> 16) & 0xFFu)) bad++;
    if (w[C::CCW] != 0) bad++;
    return bad;
}

// Every field at every value of its spec domain, the top one included (currentTerm 7, electionCount 7,
// restartCount 15, log-entry term 7, |msgs| 255, votedFor N - 1 and None): the field under test sweeps its
// domain while all the others sit at their minimum and then at their maximum, so a field one bit too
// narrow loses its top value or spills into a neighbour that would otherwise read zero / all ones.
template <int N, int V>
static int check_domains() {
    using L = Layout<N, V>;
    int bad = 0, cores = 0;
    // field ids: 0 votedFor 1 currentTerm 2 role 3 commitIndex 4 Len(logs) 5 entry term 6 entry val
    //            7 matchIndex 8 nextIndex 9 electionCount 10 restartCount 11 |msgs| 12 pendingResponse 13 valSent
    const uint32_t lo[14] = {0, 0, 0, 1, 1, 0, 0, 1, 2, 0, 0, 0, 0, 0};
    const uint32_t hi[14] = {(uint32_t)N, 7, 2, V + 1, V + 1, 7, V - 1, V + 1, V + 2, 7, 15, 255, 1, 1};
    auto build = [&](int field, uint32_t val, bool others_hi, uint32_t *c) {
        auto f = [&](int id) { return id == field ? val : (others_hi ? hi[id] : lo[id]); };
        for (int k = 0; k < L::NW; k++) c[k] = 0u;
        for (int i = 0; i < N; i++) {
            const uint32_t vf = f(0);  // N = None, else a server; at `hi` server N - 1 and None alternate
            const uint32_t vfi = (field != 0 && others_hi) ? ((i & 1) ? (uint32_t)N : (uint32_t)N - 1) : vf;
            c[L::W_VF] = setnib(c[L::W_VF], i, vfi == (uint32_t)N ? VF_NONE : vfi);
            c[L::W_CT] = setnib(c[L::W_CT], i, f(1));
            c[L::W_ROLE] = setnib(c[L::W_ROLE], i, f(2));
            c[L::W_CI] = setnib(c[L::W_CI], i, f(3));
            // the log holds V entries whenever an entry field is under test or the others are at their top
            const uint32_t ll = (field == 5 || field == 6) ? (uint32_t)V + 1 : f(4);
            c[L::W_LL] = setnib(c[L::W_LL], i, ll);
            for (uint32_t x = 2; x <= ll; x++) c[L::W_LOG + i] |= (f(5) | (f(6) << 4)) << (8 * (x - 2));
            for (int j = 0; j < N; j++) {
                c[L::W_MI + i] = setnib(c[L::W_MI + i], j, f(7));
                c[L::W_NI + i] = setnib(c[L::W_NI + i], j, f(8));
            }
        }
        c[L::W_PEND] = f(12) ? (uint32_t)((1ull << (N * N)) - 1) : 0u;
        uint32_t misc = f(9) | (f(10) << 4) | (f(11) << 16);
        for (int v = 0; v < V; v++) misc |= f(13) << (8 + v);
        c[L::W_MISC] = misc;
    };
    for (int field = 0; field < 14; field++)
        for (uint32_t val = lo[field]; val <= hi[field]; val++)
            for (int oh = 0; oh < 2; oh++) {
                uint32_t c[L::NW];
                build(field, val, oh != 0, c);
                bad += round_trip<N, V>(c);
                cores++;
            }
    std::printf("N=%d V=%d: %d domain cores (every field at every value, top included), %d mismatches\n", N, V, cores, bad);
    return bad;
}

// The message info word (minfo / mi_*): every field at every value up to its maximum -- term 7 (and the
// field's own 15), x1..x3 15, entry term 7 (and 15), entry value 7, src / dst 7 -- against all-zero and
// all-ones neighbours.
static int check_minfo() {
    const uint32_t top[10] = {3, 7, 7, 15, 15, 15, 15, 1, 15, 7};  // type src dst term x1 x2 x3 ent et ev
    int bad = 0, words = 0;
    for (int field = 0; field < 10; field++)
        for (uint32_t val = 0; val <= top[field]; val++)
            for (int oh = 0; oh < 2; oh++) {
                uint32_t f[10];
                for (int k = 0; k < 10; k++) f[k] = k == field ? val : (oh ? top[k] : 0u);
                const uint32_t m = minfo(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9]);
                const uint32_t g[10] = {mi_type(m), mi_src(m), mi_dst(m), mi_term(m), mi_x1(m), mi_x2(m), mi_x3(m),
                                        mi_ent(m), mi_et(m), mi_ev(m)};
                for (int k = 0; k < 10; k++)
                    if (f[k] != g[k]) {
                        if (bad < 5) std::printf("minfo field %d: %u -> %u (word %08x)\n", k, f[k], g[k], m);
                        bad++;
                    }
                words++;
            }
    // the records the actions build at MaxElection 7 (Universe::build's calls), field by field
    for (uint32_t term = 1; term <= 7; term++)
        for (uint32_t lt = 0; lt <= 7; lt++)
            for (uint32_t et = 1; et <= 7; et++) {
                const uint32_t q = minfo(AREQ, 4, 3, term, MAXV + 1, lt, MAXV + 1, 1, et, MAXV - 1);
                bad += !(mi_type(q) == AREQ && mi_src(q) == 4 && mi_dst(q) == 3 && mi_term(q) == term &&
                         mi_x1(q) == MAXV + 1 && mi_x2(q) == lt && mi_x3(q) == MAXV + 1 && mi_ent(q) == 1 &&
                         mi_et(q) == et && mi_ev(q) == MAXV - 1);
                const uint32_t v = minfo(VREQ, 4, 3, term, MAXV + 1, lt, 0, 0, 0, 0);
                bad += !(mi_type(v) == VREQ && mi_term(v) == term && mi_x1(v) == MAXV + 1 && mi_x2(v) == lt &&
                         mi_ent(v) == 0 && mi_et(v) == 0);
                words += 2;
            }
    std::printf("minfo: %d words, %d mismatches\n", words, bad);
    return bad;
}

int main() {
    std::mt19937_64 rng(12345);
    int bad = 0;
    bad += check_domains<2, 1>();
    bad += check_domains<2, 2>();
    bad += check_domains<3, 1>();
    bad += check_domains<3, 2>();
    bad += check_domains<3, 3>();
    bad += check_domains<4, 1>();
    bad += check_domains<4, 2>();
    bad += check_domains<5, 1>();
    bad += check_domains<5, 2>();
    bad += check_minfo();
    bad += check<2, 1>(rng, 20000);
    bad += check<2, 2>(rng, 20000);
    bad += check<3, 1>(rng, 20000);
    bad += check<3, 2>(rng, 20000);
    bad += check<3, 3>(rng, 20000);
    bad += check<4, 1>(rng, 20000);
    bad += check<4, 2>(rng, 20000);
    bad += check<5, 1>(rng, 20000);
    bad += check<5, 2>(rng, 20000);
    static_assert(Codec<3, 2>::CCW == 4, "Raft.cfg's packed core is 128 bits");
    return bad ? 1 : 0;
}
