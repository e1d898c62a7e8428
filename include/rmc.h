/*
 * rmc.h -- C-ABI of the MI355X-native Raft model checker (librmc.so).
 *
 * The reference (kikimo/tla-raft) has no library API: its only interface is the
 * TLC command line in myrun.sh:3
 *
 *     java -Xms4g -Xmx12g -jar tla2tools.jar -deadlock -workers 4 -config Raft.cfg Raft.tla $@
 *
 * which reads Raft.tla + Raft.cfg, runs TLC's breadth-first model checker and
 * prints TLC text.  Every entry point below replaces one piece of that run and
 * cites what it replaces.  A TLC-compatible host driver (tla-raft_amd/launcher,
 * or a Java FFM / Python ctypes binding -- INTEGRATION.md) sits on top.
 *
 * Conventions: plain C types only; every function returns RMC_OK (0) or a
 * negative RMC_E_* code, with text from rmc_last_error().  A context is owned by
 * one host thread.  All device memory is owned by the context.  The library
 * never falls back to a CPU path: without a usable gfx950 device rmc_create
 * fails with RMC_E_DEVICE.
 */
#ifndef RMC_H
#define RMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMC_ABI_VERSION 5

/* ---- return codes ---------------------------------------------------------- */
#define RMC_OK 0
#define RMC_DONE 1          /* rmc_step: the state space is exhausted */
#define RMC_VIOLATION 2     /* an INVARIANT is FALSE in a new state (TLC exit 12) */
#define RMC_ASSERT 3        /* Assert(role[s] # Leader, "split brain") failed, Raft.tla:185 */
#define RMC_EVAL_ERROR 4    /* TLC evaluation error while checking an invariant (Raft.tla:499) */
#define RMC_DEADLOCK 5      /* a state without successors while deadlock checking is on */
#define RMC_E_ARG -1
#define RMC_E_DEVICE -2
#define RMC_E_MEMORY -3
#define RMC_E_CAPACITY -4   /* a state exceeded the packed layout (|msgs| > msg_cap) */
#define RMC_E_STATE -5      /* call out of sequence */
#define RMC_E_PARSE -6      /* cfg / spec validation failed */
#define RMC_E_COMM -7       /* multi-GPU communicator failure */

/* ---- invariants (Raft.cfg:33-34 selects Inv) --------------------------------- */
#define RMC_INV_LEADER_HAS_ALL_COMMITTED (1u << 0) /* Inv == LeaderHasAllCommittedEntries, Raft.tla:491-503 */
#define RMC_INV_NO_SPLIT_VOTE (1u << 1)            /* Raft.tla:444-448 */
#define RMC_INV_RAFT_CAN_COMMIT (1u << 2)          /* RaftCanCommt, Raft.tla:434 */
#define RMC_INV_FOLLOWER_CAN_COMMIT (1u << 3)      /* Raft.tla:436-439 */
#define RMC_INV_COMMIT_ALL (1u << 4)               /* Raft.tla:442 */
#define RMC_INV_NO_ALL_COMMIT (1u << 5)            /* Raft.tla:451-481 (reads msgs) */
#define RMC_INV_EXIST_LEADER_AND_CANDIDATE (1u << 6) /* Raft.tla:483-487 */

/* ---- spec variants ------------------------------------------------------------ */
#define RMC_SPEC_RAFT 0    /* Raft.tla as shipped */
#define RMC_SPEC_SEEDED 1  /* RaftSeeded: Median's threshold (Raft.tla:72) is Cardinality(Servers) */
#define RMC_SPEC_BECOME_FOLLOWER 2  /* Raft.tla with Next's `\/ BecomeFollower(s)` uncommented (Raft.tla:420):
                                       FollowerUpdateTerm / CandidateToFollower / LeaderToFollower
                                       (Raft.tla:190-229) right after UpdateTerm; trace action id 12 */
/* Test variants (tools/make_seeded_spec.py --split-brain / --commit-past-log) in which TLC's two error
 * kinds other than an invariant violation are reachable in a BFS, so their precedence and counters
 * are checked end to end (the shipped specs reach neither): */
#define RMC_SPEC_SPLIT_BRAIN 3      /* RaftSplitBrain: BecomeLeader's quorum (Raft.tla:164) is 1 -> two
                                       leaders of one term -> UpdateTerm's Assert (Raft.tla:185) fails */
#define RMC_SPEC_COMMIT_PAST_LOG 4  /* RaftCommitPastLog: FollowerAcceptEntry's newCommitIndex (Raft.tla:294)
                                       is Max(commitIndex, leaderCommit) -> Inv's logs[p][index]
                                       (Raft.tla:499) out of its domain */

/* Model configuration: what Raft.cfg's CONSTANTS (Raft.cfg:1-21), INVARIANT
 * (Raft.cfg:33-34) and TLC's -deadlock flag (myrun.sh:3) bind.  VIEW view
 * (Raft.cfg:26) is on unless rmc_set_full_state turns it off (below: the whole
 * state is then the identity); SYMMETRY symmServers (Raft.cfg:24) unless
 * no_symmetry.  A zero-initialised struct plus the four constants and
 * invariants = RMC_INV_LEADER_HAS_ALL_COMMITTED is Raft.cfg under myrun.sh.
 *
 * Kernels are compiled for these (n_servers, n_vals, message lanes) only; rmc_create refuses
 * every other combination with RMC_E_ARG ("no compiled kernels for ..."), before it touches the
 * device:
 *     64 lanes  (msg_cap 1..64):   (2,1) (2,2) (3,1) (3,2) (3,3)
 *     128 lanes (msg_cap above 64): (3,1) (3,2) (4,1) (4,2) (5,1) (5,2)
 * each with and without RMC_SPEC_BECOME_FOLLOWER.  So 4 and 5 servers need the 128 lanes (the
 * default there) and take at most 2 values; 3 values exist only at 3 servers with 64 lanes.
 *
 * Message ids are 16 bit, so the static message universe of (n_servers, n_vals, max_election) must hold
 * fewer than 65,535 records.  That caps max_election per pair:
 *     (2,1) (2,2) (3,1) (4,1) (5,1): 7     (3,2): 6     (3,3): 4     (4,2): 5     (5,2): 4
 * rmc_create refuses a larger one with RMC_E_ARG ("... max_election is at most 6 for this pair"), like a
 * pair without kernels before it touches the device, and rmc_parse_config refuses such a cfg with
 * RMC_E_PARSE and the same limit in its text. */
typedef struct rmc_config {
    int32_t n_servers;      /* |Servers|   Raft.cfg:18, 2..5 (see the table above) */
    int32_t n_vals;         /* |Vals|      Raft.cfg:21, 1..2; 3 at 3 servers with 64 lanes */
    int32_t max_election;   /* MaxElection Raft.cfg:4,  0..7, and at most the pair's cap above */
    int32_t max_restart;    /* MaxRestart  Raft.cfg:3,  0..15 */
    uint32_t invariants;    /* RMC_INV_* bits (order: invariant_order) */
    int32_t check_deadlock; /* 0 = TLC -deadlock (myrun.sh:3) */
    int32_t spec_variant;   /* RMC_SPEC_* */
    int32_t device;         /* HIP device ordinal (-1 = current) */
    int32_t msg_cap;        /* max |msgs| per state: 0 = auto (64 for n<=3, 128 otherwise).  It selects the
                               message lanes and is rounded up to them: 1..64 is 64 (msg_cap = 8 behaves as
                               64), anything above 64 is 128; a state or successor past the lanes is RMC_E_CAPACITY */
    int32_t seen_log2;      /* initial seen-set slots = 2^seen_log2 (0 = auto); grows on demand */
    int32_t no_symmetry;    /* 0 = SYMMETRY symmServers (Raft.cfg:24); 1 = cfg without SYMMETRY */
    uint64_t chunk_successors; /* successors per device chunk (0 = auto) */
    /* multi-GPU (one process per GPU): world_size 0 or 1 = single GPU */
    int32_t rank, world_size;  /* world_size 0 or 1 = single GPU; world_size 1 WITH comm_unique_id = a one-rank
                                  RCCL communicator running the sharded protocol (self send/recv) */
    const void *comm_unique_id; /* 128-byte RCCL unique id (rmc_comm_unique_id on rank 0), same on every rank;
                                  NULL with world_size > 1: the host-staged transport (rmc_set_transport) */
    int32_t virtual_shards;    /* > 1: run that many fingerprint-owner shards in this process on one device
                                  (the multi-GPU partition/exchange logic with device copies for transport) */
    uint32_t timing_phases;    /* bit i: HIP-event time phase i into rmc_level_stats.kernel_ms (0 = all) */
    uint32_t device_levels;    /* single GPU: BFS levels enqueued per host round trip by rmc_run /
                                  rmc_run_levels (0 = auto, 1 = the host drives every level) */
    uint64_t shard_min_states; /* world_size or virtual_shards > 1: levels with fewer states than this are
                                  expanded whole on every shard (replicated, no exchange, TLC order); the run
                                  switches to the sharded level (block-cyclic frontier, fingerprint-owner seen
                                  set, TLC-order election by global key) at the first level that reaches it
                                  and stays sharded (0 = auto: 2^20; 1 = sharded from Init's level) */
    /* ---- ABI 3 ---- */
    uint32_t invariant_order;  /* the INVARIANTs in cfg order (Raft.cfg:33-34; TLC checks them in that order):
                                  invariant bit index + 1 per 4-bit nibble, first in the low nibble;
                                  0 = the bits of `invariants` in bit order */
    uint32_t compact_log2;     /* seen set: 16-B slots {fp} while the table has at most 2^compact_log2 slots,
                                  then one migration to 8-B slots sized from seen_mem_bytes and never grown
                                  (0 = auto: 27) */
    uint64_t seen_mem_bytes;   /* device bytes for the compact seen set (0 = auto: half of the free memory
                                  at migration, per shard) */
    uint64_t frontier_mem_bytes; /* device bytes for the frontier ring once the seen set is compact (0 = auto:
                                  70 % of the free memory left then, per shard) */
} rmc_config;

/* Statistics of one BFS level (what TLC's progress line reports). */
typedef struct rmc_level_stats {
    int32_t level;            /* BFS level whose states were just expanded (1 = Init's level) */
    int32_t status;           /* RMC_OK / RMC_DONE / RMC_VIOLATION / ... */
    uint64_t expanded;        /* states of that level expanded (all ranks) */
    uint64_t generated;       /* successors generated while expanding it (all ranks) */
    uint64_t new_states;      /* distinct states first found (all ranks) */
    uint64_t total_generated; /* TLC "states generated", Init included */
    uint64_t total_distinct;  /* TLC "distinct states found" */
    uint64_t queue;           /* TLC "states left on queue" */
    double seconds;           /* wall time of this level */
    double kernel_ms[6];      /* expand-count, expand-hash, dedup, materialize, exchange, other */
    uint64_t kernel_launches[6];
    uint64_t new_bytes;       /* ABI 3: bytes of the new states' frontier records (packed core + message ids) */
    uint64_t self_loops;      /* ABI 5: generated successors equal to their parent (FollowerAcceptEntry that
                                 changes nothing), among `generated`.  Single-GPU levels set them apart (never
                                 fingerprinted: the parent is in the seen set); sharded rounds set them apart in
                                 split rounds and route them in smaller rounds, counting them either way */
} rmc_level_stats;

/* Final result of a run: TLC's closing lines. */
typedef struct rmc_result {
    int32_t status;           /* RMC_DONE / RMC_VIOLATION / RMC_ASSERT / RMC_EVAL_ERROR / RMC_DEADLOCK */
    int32_t depth;            /* "The depth of the complete state graph search is D" */
    uint64_t generated, distinct, queue;
    int32_t violated;         /* index (bit) of the violated invariant, -1 if none */
    uint32_t trace_len;
    double seconds;
    /* ABI 3: memory of the run (this rank) */
    uint64_t seen_slots;          /* seen-set capacity in slots */
    int32_t seen_slot_bytes;      /* 16 (full fingerprints) or 8 (compact) */
    int32_t pad_;
    uint64_t frontier_ring_bytes; /* device bytes of the frontier ring */
    uint64_t frontier_peak_bytes; /* largest live frontier (current + next level records) */
} rmc_result;

int rmc_abi_version(void);

/* RCCL unique id for a multi-GPU run (call on rank 0, broadcast the 128 bytes to every
 * rank, pass as rmc_config.comm_unique_id).  Replaces nothing in the reference: TLC runs
 * in one JVM; this is the seen-set sharding of SURVEY.md 8(e). */
int rmc_comm_unique_id(void *out128);

/* ABI 4: a host-staged transport for the sharded protocol (world_size > 1 without comm_unique_id).
 * The ranks' collectives go through these callbacks instead of RCCL: every rank of the run installs
 * one (process-wide, before rmc_create; NULL removes it) whose calls meet their peers' -- e.g. a
 * torch.distributed gloo group (raftmc.HostTransport).  It carries the same protocol as RCCL through
 * host memory, so the multi-rank path runs as separate processes on one device (tests) or on hosts
 * without a GPU interconnect.  Each callback returns 0 on success; anything else fails the step with
 * RMC_E_COMM.
 *   allreduce_u64  v[0..n) <- the elementwise sum (is_max = 0) or maximum over the ranks, in place
 *   allgather_u64  out[0..W*k) <- every rank's row[0..k), in rank order
 *   alltoallv      bytes send + send_off[p] .. + send_bytes[p] go to rank p, bytes from rank p land at
 *                  recv + recv_off[p] (recv_bytes[p] of them); the caller's own entries are 0 */
typedef struct rmc_transport {
    void *user;
    int32_t (*allreduce_u64)(void *user, uint64_t *v, int32_t n, int32_t is_max);
    int32_t (*allgather_u64)(void *user, const uint64_t *row, int32_t k, uint64_t *out);
    int32_t (*alltoallv)(void *user, const void *send, const uint64_t *send_off, const uint64_t *send_bytes,
                         void *recv, const uint64_t *recv_off, const uint64_t *recv_bytes);
} rmc_transport;
int rmc_set_transport(const rmc_transport *t);

/* Parse Raft.cfg text (replaces TLC's ModelConfig for the subset Raft.cfg uses,
 * Raft.cfg:1-34) and validate Raft.tla text by content (replaces SANY; only
 * Raft.tla, the documented RaftSeeded variant and Raft.tla with FollowerAppendEntry
 * uncommented in Next -- never enabled, so RMC_SPEC_RAFT -- are recognised).  tla_text
 * may be NULL to skip the spec check (then spec_variant is left unchanged). */
int rmc_parse_config(const char *cfg_text, const char *tla_text, rmc_config *out, char *err, size_t err_cap);

/* Replaces TLC start-up (myrun.sh:3): allocates device state, builds the
 * message universe and symmetry tables for the configuration. */
int rmc_create(const rmc_config *cfg, void **ctx_out);

/* Init (Raft.tla:93-105): level 1, invariant check on the initial state. */
int rmc_init(void *ctx, rmc_level_stats *st);

/* One BFS level of TLC's worker loop: successors of every state of the current
 * level (Next, Raft.tla:416-430), SYMMETRY+VIEW fingerprint (Raft.tla:21,38),
 * seen-set insertion with TLC -workers 1 first-discovery order, INVARIANT check
 * on new states (Raft.cfg:33).  Returns RMC_OK, RMC_DONE or an error status. */
int rmc_step(void *ctx, rmc_level_stats *st);

/* As many BFS levels as one host round trip covers: on a single GPU up to
 * cfg.device_levels levels enqueued back to back, each level's kernels taking its
 * size from the previous level's commit on the device (stopping early at the end,
 * an error, or a level that needs larger buffers); otherwise one rmc_step.
 * Per-level statistics go to levels[0..*n); cap >= 1.  Same return as rmc_step for
 * the last level reported. */
int rmc_steps(void *ctx, rmc_level_stats *levels, uint32_t cap, uint32_t *n);

/* Phase timing from now on: 0 = off (no HIP events between kernels), 0xFFFFFFFF = every
 * phase, otherwise a mask as cfg.timing_phases. */
int rmc_set_timing(void *ctx, uint32_t phases);

/* Forget every explored state (seen set, levels, trace) but keep the device
 * buffers, so the next rmc_init starts a fresh run (TLC: a new invocation). */
int rmc_reset(void *ctx);

/* Checkpoint / resume between BFS levels (TLC's states/ metadir and -recover, .gitignore:2;
 * SURVEY 8(f) item 4).  rmc_checkpoint writes the seen set, the current level, every state's
 * parent reference and TLC's counters to `path`, after rmc_init and before the run finishes.
 * Sharded runs too: a context with virtual shards writes all of them to `path`; an RCCL rank of
 * a world_size > 1 run writes its own shards to `path` + ".rank<r>" (every rank calls it between
 * the same two levels).  rmc_resume loads such a file into a context created with the same
 * configuration and shard layout (world size, rank, virtual shards, chunk size, shard_min) and
 * not yet initialised; rmc_step / rmc_run then carry on as if the run had never stopped (same
 * counts, same TLC order, same counterexample). */
int rmc_checkpoint(void *ctx, const char *path);
int rmc_resume(void *ctx, const char *path);

/* Loop rmc_step until done or an error; fills the final result. */
int rmc_run(void *ctx, rmc_result *res);
int rmc_get_result(void *ctx, rmc_result *res);

/* rmc_init + rmc_step until done inside the library (no per-level host round trip of the
 * caller); per-level statistics go to levels[0..*n_levels) (as many as fit in cap). */
int rmc_run_levels(void *ctx, rmc_level_stats *levels, uint32_t cap, uint32_t *n_levels, rmc_result *res);

/* Counterexample (TLC's "The behavior up to this point is"): states 1..len from
 * Init to the error state.  Unpacked layout below.  action/server/witness
 * describe how state i was reached (action -1 for state 0 = Initial predicate). */
int rmc_trace_len(void *ctx, uint32_t *len);
int rmc_trace_state(void *ctx, uint32_t i, int32_t *unpacked, size_t cap_ints,
                    int32_t *action, int32_t *server, int32_t *witness);

/* ---- simulation mode (TLC's -simulate) -------------------------------------------------------
 * TLC's -simulate runs random behaviours instead of the breadth-first search: each starts at Init,
 * takes a random enabled successor per step up to -depth states (TLC's default 100) and checks the
 * INVARIANTs on every state; -seed makes a run repeatable.  rmc_simulate does the same on the GPU, a
 * wave per walker, for the configurations whose state space cannot be exhausted.  TLC's own random
 * generator is NOT reproduced: the choice below is this project's definition, fixed so that a CPU
 * oracle can replay every walk bit for bit.
 *
 * A behaviour starts at Init, which is state 1; depth >= 1 is the largest number of states in it.
 * From state k (k = 1, 2, ...) of walk w, with c the number of successors rmc_successors lists for it
 * (Next in TLC order, duplicates and self-loops included), the next state is entry (r * c) >> 32 of
 * that list, r the 32-bit value (arithmetic mod 2^64, step = k - 1):
 *     z = seed ^ (w * 0x9E3779B97F4A7C15)
 *     z = z + (step + 1) * 0x9E3779B97F4A7C15
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z = z ^ (z >> 31);   r = z >> 32
 * A walk ends at the first of: it has `depth` states (the last is not expanded); its state has no
 * successor (RMC_DEADLOCK with check_deadlock, otherwise the walk just ends: TLC's -deadlock);
 * evaluating Next at its state fails UpdateTerm's Assert (RMC_ASSERT, the behaviour ends at that
 * state); the state just chosen violates an INVARIANT in cfg order or raises the evaluation error
 * (RMC_VIOLATION / RMC_EVAL_ERROR).  Init's invariants are checked once before any walk; an error
 * there is walk 0, length 1.  The error reported is that of the smallest walk index, under every
 * schedule.  Accounted walks are 0..err_walk on an error and all of them otherwise: `states` is the
 * sum of their lengths, `generated` the sum of c over every state they expanded (a state that
 * asserted or had no successor adds 0) -- both deterministic.  A successor past the message lanes
 * in an accounted walk fails the call with RMC_E_CAPACITY.
 *
 * The host runs batches of batch_walks walkers (0 = auto: up to 2^18, fewer while the device log of
 * the steps' slot keys, batch x (depth - 1) x 2 B, would pass 64 MiB) and stops after the first batch
 * that holds an error.  Single GPU only: world_size > 1 or virtual_shards > 1, depth == 0 or
 * num_walks == 0 is RMC_E_ARG.  The call touches none of the BFS state and may come on a fresh
 * context, between BFS steps or after a run.  After an error rmc_trace_len / rmc_trace_state return
 * the erring behaviour (replayed from Init with the logged keys) until the next BFS error, rmc_reset
 * or rmc_simulate.  lens_out (num_walks) and keys_out (num_walks x (depth - 1), rmc_successors' key
 * format, 0 past a walk's end) may be NULL; walks that are not accounted stay 0. */
typedef struct rmc_sim_config {
    uint64_t num_walks;
    uint64_t seed;        /* TLC -seed */
    uint32_t depth;       /* TLC -depth */
    uint32_t batch_walks; /* walkers per launch, 0 = auto */
} rmc_sim_config;
typedef struct rmc_sim_result {
    int32_t status;       /* RMC_DONE, or the error status of err_walk */
    int32_t violated;     /* invariant bit index, -1 if none */
    uint64_t walks, states, generated; /* accounted, as defined above */
    uint64_t err_walk;    /* valid when status != RMC_DONE */
    uint32_t err_len;
    uint32_t longest;     /* longest accounted behaviour */
    uint64_t ended_early; /* accounted walks that ended in a state without successors */
    double seconds;
} rmc_sim_result;
/* Returns the result's status, or a negative RMC_E_* code. */
int rmc_simulate(void *ctx, const rmc_sim_config *sc, rmc_sim_result *res, uint32_t *lens_out, uint32_t *keys_out);

/* ---- action coverage (TLC's -coverage) -----------------------------------------------------------
 * Which disjuncts of Next do the work: per action, the successors it generated and the states first
 * found through it -- what TLC prints at the end of a -coverage run as distinct:generated.  Action ids
 * are those of rmc_successors' keys: 0..10 BecomeCandidate .. Restart in Next's order, 11
 * FollowerAppendEntry (never enabled: always 0), 12 BecomeFollower (the tla:420 variant only).
 *   generated[a]  successors of action a among those "states generated" counts: self-loops and
 *                 duplicates included.
 *   distinct[a]   explored states with global id >= 1 whose trace key carries action a (the action of
 *                 the successor that TLC -workers 1 met first).
 *   Init          apart, 1:1 (init_generated / init_distinct).
 * At every level boundary and in every outcome (done, violation, evaluation error, Assert, deadlock)
 *     1 + sum(generated) == total generated        1 + sum(distinct) == total distinct
 * so on an error the counts stop where TLC's counters stop: with p the erring parent and the (server,
 * action) group of the error's key, the parents before p in the level count in full; at p the
 * sub-action batches up to and including that group for an invariant or evaluation error (TLC adds a
 * batch before it fingerprints it), only the batches before it for an Assert, none for a deadlock;
 * distinct covers the global ids below the total.
 * Off by default, and then nothing is allocated or launched for it.  rmc_set_coverage: after rmc_create
 * or rmc_reset and before rmc_init (RMC_E_STATE otherwise); rmc_reset zeroes the counts and keeps the
 * setting.  While it is on, levels run one per host round trip (device_levels has no effect on the
 * results), every shard layout counts (levels expanded replicated are counted once, ranks are summed in
 * the rounds' all-reduces: rmc_get_coverage is local and returns the global totals on every rank), and
 * rmc_simulate neither reads nor changes the counts.  Checkpoints do not carry them: rmc_resume on a
 * context with coverage on returns RMC_E_ARG.  rmc_get_coverage: after rmc_init, between steps or after
 * the run (the counts of the levels finished so far); RMC_E_STATE while coverage is off. */
typedef struct rmc_coverage {
    uint64_t generated[16], distinct[16];
    uint64_t init_generated, init_distinct;
} rmc_coverage;
int rmc_set_coverage(void *ctx, int on);
int rmc_get_coverage(void *ctx, rmc_coverage *out);

/* The whole state as the identity.  By default a state is identified by the cfg's VIEW (Raft.tla:38), which
 * leaves out electionCount, restartCount, pendingResponse and valSent although each guards an action
 * (Raft.tla:108, :411, :246 / :380, :236): two states that differ only there are one "distinct state", and the
 * one found first stands for both, successors included.  With this setting on, the 128-bit fingerprint is
 * a function of all twelve variables -- under SYMMETRY the minimum over the same coset of server
 * permutations, pendingResponse permuted on both indices -- so a "distinct state" is a SYMMETRY class of
 * whole states (a whole state without SYMMETRY) and the search no longer depends on which member of a VIEW
 * class is met first.  Everything that works on fingerprints follows: the seen set, the sharded owners,
 * coverage's distinct counts, continuation, graph mode and the kept graph's queries, rmc_fingerprint(s) and
 * rmc_seen_contains.  rmc_simulate keeps no seen set and is not affected.
 * rmc_set_full_state: after rmc_create or rmc_reset and before rmc_init / rmc_init_from / rmc_resume
 * (RMC_E_STATE once a search holds states); rmc_reset keeps the setting; every rank of a sharded run sets
 * it.  A checkpoint stores it: rmc_resume under the other setting fails with "not a checkpoint of this
 * configuration" (checkpoints written before the setting existed are VIEW checkpoints).  Off by default. */
int rmc_set_full_state(void *ctx, int on);

/* Continuation (TLC's -continue): search past invariant violations and count them per invariant.
 * With it on, a new state on which an invariant evaluates to FALSE no longer ends the search: it is
 * inserted, enqueued and expanded like any other.  Per new state the invariants are evaluated in cfg
 * order up to the first FALSE one (TLC's break), so every violating state is attributed to exactly one
 * invariant, and an invariant listed after a FALSE one is not evaluated on that state (it cannot raise
 * its evaluation error there).  Init is checked the same way (a violation at Init: first_level 1).
 * Everything else stops the run as without it -- an invariant's evaluation error, UpdateTerm's Assert,
 * a deadlock with deadlock checking on, RMC_E_CAPACITY -- with the same precedence, counters, trace and
 * codes.  A run that exhausts the state space ends with status RMC_DONE and violated = -1, its counters
 * those of the same configuration without invariants; the violations are reported on the side:
 *   count[b]        explored states attributed to the invariant with bit index b (RMC_INV_* = 1 << b)
 *   first_level[b]  level of the first such state in TLC -workers 1 order, i.e. of the smallest global
 *                   id (1 = Init's level; 0 = none)
 *   total           sum of count[]
 * rmc_get_violation_levels: count[b] per BFS level, per_level[0] Init's level, *n levels (the depth
 * reached so far; RMC_E_ARG if cap is smaller); they sum to count[b].  rmc_violation_trace makes the
 * behaviour from Init to that invariant's first violating state the current trace of rmc_trace_len /
 * rmc_trace_state, until the next error, rmc_reset or rmc_simulate; RMC_E_ARG if the invariant has no
 * violation.  With ranks it walks the distributed trace: every rank calls it.
 * When another error stops the run, the counts cover exactly the explored states with global id below
 * the reported `distinct` (the cut rmc_get_coverage's distinct[] uses): a violating state of the erring
 * level that TLC -workers 1 would not have reached is not counted and cannot be first.  Counts, levels
 * and first states are the same under every execution path and shard layout.
 * Off by default, and then nothing is launched for it (one device word behind each set of error slots is all
 * that is allocated).  rmc_set_continue: after rmc_create
 * or rmc_reset and before rmc_init (RMC_E_STATE otherwise); rmc_reset zeroes the counts and keeps the
 * setting.  While it is on each finished level is counted by a pass of its own over its records, inside the
 * device-driven level loop as well (device_levels has no effect on the results); levels expanded
 * replicated are counted once, ranks are summed in all-reduces: rmc_get_violations is local and returns
 * the global totals on every rank.  rmc_simulate neither reads nor changes the counts and stops at its
 * first error.  It composes with coverage: rmc_get_coverage is then that of the run that did not stop.
 * Checkpoints do not carry the counts: rmc_resume on a context with continuation on returns RMC_E_ARG.
 * rmc_get_violations / rmc_get_violation_levels: after rmc_init, between steps or after the run (the
 * levels finished so far); RMC_E_STATE while continuation is off. */
typedef struct rmc_violations {
    uint64_t count[16];        /* by invariant bit index */
    int32_t  first_level[16];  /* 0 = none */
    uint64_t total;
} rmc_violations;
int rmc_set_continue(void *ctx, int on);
int rmc_get_violations(void *ctx, rmc_violations *out);
int rmc_get_violation_levels(void *ctx, uint32_t invariant_bit, uint64_t *per_level, uint32_t cap, uint32_t *n);
int rmc_violation_trace(void *ctx, uint32_t invariant_bit);

/* ---- state graph (TLC's -dump FILE / -dump dot FILE) ------------------------------------------------
 * The states a run finds and every resolved edge between them, streamed to callbacks while the search runs.
 * The search itself knows only the BFS tree (each state's parent and slot key); with graph mode on, every
 * finished level is visited again on the side: its new states go into a map from fingerprint to global id
 * (a device table of its own; the seen set, the election and the commits are untouched), then its parents
 * are re-evaluated in chunks and each successor -- duplicates and self-loops included, Next's order -- is
 * looked up there.
 *   states(user, gid0, n, unpacked, stride_ints)  the states with global ids gid0 .. gid0 + n - 1 (BFS order,
 *       Init = 0) in the unpacked layout below, stride_ints apart: the record the search stored, i.e. the
 *       first-found member of its SYMMETRY/VIEW class, which is what TLC dumps.  NULL: states are not copied.
 *   edges(user, n, src, key, dst)  n edges in TLC -workers 1 order (ascending src, each src's successors in
 *       Next's order): global ids and the key in rmc_successors' format.  A successor in its parent's class has
 *       dst == src.  NULL: the pass runs and nothing is delivered.
 * Order of delivery: rmc_init delivers states(0, 1, Init); each step that expands level L first delivers the
 * states of the level it made, ascending, then level L's edges.  A callback that returns non-zero fails
 * the step with RMC_E_SINK and ends the run (rmc_destroy / rmc_reset may follow).
 * Without an error the number of edges is `generated` - 1.  At an error the edges stop where TLC -workers 1
 * stops: the parents before the erring parent p give all their edges; p gives, for an invariant violation or
 * an evaluation error, the edges up to and including the erring successor, for UpdateTerm's Assert those of
 * the sub-action batches before the failing one, for a deadlock none; later parents give nothing; the
 * states delivered are those with global id below the reported `distinct`, so every dst < distinct.
 * Limits: single GPU (RMC_E_ARG with world_size > 1 or virtual_shards > 1).  The pass reads level L after
 * level L + 1 is complete, so both stay resident in the frontier ring: a run whose seen set would move to
 * its compact form (2^compact_log2 slots; the default 2^27 is about 67 M states) fails that step with
 * RMC_E_MEMORY -- raise compact_log2.  Levels run one per host round trip (device_levels has no effect on the
 * results).  It composes with coverage and with continuation (the graph is then that of the search that did
 * not stop).  Checkpoints do not carry the map: rmc_resume with graph mode on returns RMC_E_ARG.
 * rmc_set_graph: after rmc_create or rmc_reset and before rmc_init (RMC_E_STATE otherwise); NULL = off (nothing more is
 * launched; what graph mode had allocated stays with the context for a later rmc_set_graph, until rmc_destroy).
 * rmc_reset keeps the setting and empties the map.  Off by default, and then nothing is allocated or launched. */
#define RMC_E_SINK -8   /* a graph sink callback returned non-zero */
typedef struct rmc_graph_sink {
    void *user;
    int32_t (*states)(void *user, uint64_t gid0, uint64_t n, const int32_t *unpacked, size_t stride_ints);
    int32_t (*edges)(void *user, uint64_t n, const uint64_t *src, const uint32_t *key, const uint64_t *dst);
    uint32_t chunk_parents;  /* parents per edge launch, 0 = auto (8192) */
    uint32_t map_log2;       /* initial gid-map slots = 2^map_log2, 0 = auto (16); kept at load <= 1/2 by rehashing */
} rmc_graph_sink;
int rmc_set_graph(void *ctx, const rmc_graph_sink *sink);

/* ---- reachability queries over the state graph (AG EF P; nothing in TLC) ---------------------------------
 * Every mode above answers whether a state is reachable.  These answer, for each reachable state, whether a
 * state with a property can still be reached FROM it -- e.g. "can a commit still happen from here" -- and
 * name the first state from which it cannot.  rmc_set_graph_keep turns the graph pass on (with or without a
 * sink: without one the pass runs and delivers nothing) and keeps what it resolves on the device: every
 * edge's (src, dst) as u32 pairs in a store that grows by doubling, and per state a u16 with ALL seven
 * compiled invariants evaluated on it, whatever the cfg lists and without check_invs' stop at the first
 * FALSE one: bit b set = the invariant with bit index b is TRUE, bit 8 + b set = it raised the evaluation
 * error (then bit b is clear).  A failed growth, 2^32 states or 2^32 edges fail that step with
 * RMC_E_MEMORY.  When the run stops at an error the store holds exactly what graph mode delivers: the states
 * with global id below the reported `distinct` and the edges up to TLC's stopping point, every dst < distinct.
 * It has graph mode's limits (single GPU: RMC_E_ARG otherwise; no compact seen set; no rmc_resume) and
 * composes with sinks, coverage and continuation as graph mode does.  rmc_set_graph_keep: after rmc_create
 * or rmc_reset and before rmc_init (RMC_E_STATE otherwise); rmc_reset empties the store and keeps the
 * setting.  Off by default, and then nothing is allocated or launched.
 *
 * What the verdict is about: the graph is the one TLC explores and dumps.  Each state is the first-found
 * member of its SYMMETRY/VIEW class; the VIEW hides electionCount / restartCount, so a class's successors are
 * those of its first-found member.  "Cannot" therefore includes states that are stuck only because
 * MaxElection / MaxRestart are spent in that member.
 *
 * The analyses run on the device over a reverse CSR (in-degree histogram, exclusive scan, scatter through
 * per-row cursors) that is built on first use and dropped when the graph grows; no reported number depends
 * on the order inside a row.  They may be called between steps (the graph of the levels finished so far) or
 * after the run; each returns RMC_E_STATE while keep is off or nothing has been kept or imported.
 *   rmc_graph_reach         the target set is the states on which invariant `invariant_bit` (bit index 0..6)
 *                           evaluated to `value` (1 TRUE, 0 FALSE); a state whose evaluation raised the error is
 *                           in neither set.  A level-synchronous backward BFS from it, self-edges ignored:
 *                           dist_out[g] (`states` entries, or NULL) = the fewest edges from g to a target, 0 for
 *                           a target, 0xFFFFFFFF if there is no path.
 *   rmc_graph_reach_levels  the last query's can / cannot counts per BFS level of the run ([0] = Init's level;
 *                           an imported graph is one level); *n levels, RMC_E_ARG if cap is smaller.  The rows
 *                           sum to can_reach / cannot_reach.
 *   rmc_graph_shape         counts and degrees; cyclic_states by Kahn peeling: the states left after repeatedly
 *                           removing every state with no non-self edge into a state still present.  0 = the
 *                           graph has no cycle other than self-edges.
 *   rmc_graph_inv_values    the u16 per state, cap >= states entries. */
typedef struct rmc_reach_query {
    uint32_t invariant_bit;   /* 0..6 */
    int32_t value;            /* 1 = TRUE, 0 = FALSE */
} rmc_reach_query;
typedef struct rmc_reach_result {
    uint64_t states, edges, self_edges;
    uint64_t targets;         /* states in the target set */
    uint64_t can_reach;       /* targets included (distance 0) */
    uint64_t cannot_reach;
    uint64_t first_cannot;    /* smallest global id that cannot reach a target; all ones if there is none */
    int32_t first_cannot_level; /* its BFS level (1 = Init's level); 0 if there is none */
    int32_t max_distance;     /* the farthest state that can */
    int32_t init_distance;    /* -1: Init cannot */
    uint32_t rounds;          /* frontier launches of the backward pass */
    double seconds;           /* the backward pass */
    double csr_seconds;       /* the build of the reverse CSR this query ran on (done once per kept graph) */
} rmc_reach_result;
/* (a struct tag only: the function below has the name) */
struct rmc_graph_shape {
    uint64_t states, edges, self_edges;
    uint64_t back_edges;      /* dst < src */
    uint64_t sinks;           /* states with no edge out at all */
    uint64_t max_in, max_out; /* every edge counts, duplicates and self-edges included */
    uint64_t cyclic_states;
    uint64_t in_hist[64], out_hist[64]; /* states by degree; the last bin: 63 or more */
};
int rmc_set_graph_keep(void *ctx, int on);
int rmc_graph_reach(void *ctx, const rmc_reach_query *q, rmc_reach_result *res, uint32_t *dist_out);
int rmc_graph_reach_levels(void *ctx, uint64_t *can, uint64_t *cannot, uint32_t cap, uint32_t *n);
int rmc_graph_shape(void *ctx, struct rmc_graph_shape *out);
int rmc_graph_inv_values(void *ctx, uint16_t *out, uint64_t cap);

/* ---- liveness over the state graph: inevitability (AF P), leads-to (Q ~> P), components ------------------
 * rmc_graph_reach answers "can P still happen from here"; these answer "must P happen from here", over the
 * same kept graph, under the same state rules (keep on, something kept or imported: RMC_E_STATE otherwise;
 * between steps or after the run; imported graphs), spec-independent and off unless called.
 *
 * Semantics, in graph terms.  Self-edges are ignored.  A fair behaviour is a maximal path: it is infinite, or it
 * ends in a state with no non-self edge out (a terminal state).  That is weak fairness on Next over the graph
 * TLC explores (with the caveat above: each state is its class's first-found member); Raft.tla states no
 * fairness, so TLC itself has no verdict to compare with.  The target set T is chosen as in rmc_graph_reach
 * (invariant_bit, value; an evaluation error is in neither set).  `must` is the least fixpoint of
 *     X = T  u  { s : s has at least one non-self edge out, and every non-self edge out of s ends in X }
 * and within[g] = 0 for a target, otherwise 1 + the maximum of within over g's non-self successors, 0xFFFFFFFF
 * for a state outside `must` -- an "avoider": some fair behaviour from it never meets T.
 *   rmc_graph_eventually         a level-synchronous attractor over the reverse CSR: counters start at the
 *                                out-degree without self-edges (duplicates counted, and each duplicate entry
 *                                counts down once), the first frontier is T, every predecessor entry of a frontier
 *                                state takes one decrement, and the state whose counter goes 1 -> 0 gets within =
 *                                the round and enters the next frontier (a target never enters a second time).
 *                                rounds = max_within + 1 (0 with an empty T).  within_out: `states` entries, or
 *                                NULL.  source_bit >= 0 adds a source set Q (source_bit, source_value, chosen the
 *                                same way): Q ~> P fails iff source_avoiders > 0.
 *   rmc_graph_eventually_levels  the last query's must / avoid counts per BFS level, as rmc_graph_reach_levels.
 *   rmc_graph_avoid_path         the counterexample from an avoider `gid` of the last query.  Every non-terminal
 *                                avoider has a non-self edge into an avoider; next_avoid[g] is the smallest such
 *                                dst (one edge-parallel pass after the query).  gids[0] = gid, gids[i + 1] =
 *                                next_avoid[gids[i]]; the walk ends at a terminal avoider (*loop_at = -1) or at
 *                                the first state whose next_avoid is already on the path (*loop_at = the index of
 *                                that successor: a lasso).  Deterministic.  *len states; RMC_E_ARG if gid is no
 *                                avoider of the last query or cap < *len, RMC_E_STATE without a query (a later
 *                                rmc_graph_reach, or growth of the graph, ends the query).
 *   rmc_graph_scc                strongly connected components, self-edges ignored (a state with only a self-edge
 *                                is a component of its own).  comp_out[g] (`states` entries, or NULL) = the
 *                                smallest gid of g's component.  Trimming first (Kahn peeling on the out-edges,
 *                                then on the in-edges), then forward max-gid colour propagation and a backward
 *                                closure inside each colour, repeated on what is left; an acyclic graph ends in
 *                                the trimming (trimmed == components == states).  Every host loop is bounded by
 *                                `states` rounds, every launch by the counts passed to it. */
typedef struct rmc_live_query {
    uint32_t invariant_bit;   /* 0..6: the target set P */
    int32_t value;            /* 1 = TRUE, 0 = FALSE */
    int32_t source_bit;       /* -1: no source set; 0..6: the source set Q of a leads-to */
    int32_t source_value;     /* 1 = TRUE, 0 = FALSE */
} rmc_live_query;
typedef struct rmc_live_result {
    uint64_t states, edges, self_edges;
    uint64_t targets;
    uint64_t must;            /* targets included (within 0) */
    uint64_t avoiders;
    uint64_t avoid_terminal;  /* avoiders with no non-self edge out */
    uint64_t first_avoid;     /* smallest global id among the avoiders; all ones if there is none */
    uint64_t sources;         /* with a source set: its states, ... */
    uint64_t source_avoiders; /* ... those of them that are avoiders, ... */
    uint64_t first_source_avoid; /* ... and the smallest of these (all ones if none, or no source set) */
    int32_t first_avoid_level;   /* BFS level (1 = Init's level); 0 if there is none */
    int32_t first_source_avoid_level;
    int32_t max_within;       /* the latest state of `must` */
    int32_t init_within;      /* -1: Init is an avoider */
    uint32_t rounds;          /* frontier launches of the attractor */
    uint32_t pad_;
    double seconds;           /* the attractor and its statistics */
    double csr_seconds;       /* as in rmc_reach_result */
} rmc_live_result;
typedef struct rmc_scc_result {
    uint64_t components;
    uint64_t nontrivial;        /* components of two states or more */
    uint64_t nontrivial_states; /* the states in them */
    uint64_t largest;           /* states of the largest component */
    uint64_t trimmed;           /* states removed as components of their own before any colouring */
    uint32_t rounds;            /* launches whose count the host read */
    uint32_t pad_;
    double seconds;
    double csr_seconds;
} rmc_scc_result;
int rmc_graph_eventually(void *ctx, const rmc_live_query *q, rmc_live_result *res, uint32_t *within_out);
int rmc_graph_eventually_levels(void *ctx, uint64_t *must, uint64_t *avoid, uint32_t cap, uint32_t *n);
int rmc_graph_avoid_path(void *ctx, uint64_t gid, uint64_t *gids, uint32_t cap, uint32_t *len, int32_t *loop_at);
int rmc_graph_scc(void *ctx, rmc_scc_result *res, uint32_t *comp_out);

/* Measurement support (bench.py): the random-probe peak of the seen-set layout -- `probes`
 * one-slot reads of 16-B slots at uniformly random indices of a 2^table_log2-slot table,
 * best of 3 timed launches; no model-checking state is touched. */
int rmc_probe_peak(int device, uint32_t table_log2, uint64_t probes, double *probes_per_s, double *seconds);

/* The text of the context's last error; ctx = NULL: that of the calling thread's last failed rmc_create
 * (which leaves no context to ask). */
const char *rmc_last_error(void *ctx);
void rmc_destroy(void *ctx);
/* Frees every device allocation of the context (seen set, frontier ring, chunk buffers, streams, the
 * communicator) and its pinned buffers, but not the host copy of the trace (~110 GB at Raft.cfg): a
 * process about to exit returns the device at once and leaves the host memory to the kernel.  Only
 * rmc_destroy may follow (every other call returns RMC_E_STATE).  The launcher's detached worker calls it
 * before it reports TLC's exit code, so a GPU job started when myrun.sh returns finds the device free. */
int rmc_release_device(void *ctx);

/* ---- single-state hooks (parity tests; same kernels as rmc_step) -------------- */
/* Successors of one state, in TLC enumeration order.  keys[i] = server<<24 |
 * action<<16 | witness (witness: index into the sorted msgs for message actions,
 * value for ClientReq, destination for LeaderAppendEntry, else 0).  fps gets the
 * 128-bit symmetry+view fingerprint of each successor (2 words).  Returns the
 * count, or RMC_ASSERT if UpdateTerm's Assert fails. */
int rmc_successors(void *ctx, const int32_t *unpacked, int32_t *out, size_t stride_ints, uint32_t cap,
                   uint32_t *keys, uint64_t *fps, uint32_t *count);
int rmc_fingerprint(void *ctx, const int32_t *unpacked, uint64_t fp[2]);
/* ABI 4 -- checks of a finished run's deep levels (tests/test_gpu_deep.py).  The path of the explored
 * state with global id `gid` (BFS order, Init = 0): len = its depth, keys[i] = how state i of the path
 * was reached from state i - 1 (rmc_successors' key format; keys[0] = 0), gids[i] = its global id
 * (gids[0] = the initial state the path starts at: 0, Init, unless the run was seeded with rmc_init_from,
 * then the root's id; gids[len - 1] = gid); from TLC's parent pointers (the trace), any shard layout. */
int rmc_state_path(void *ctx, uint64_t gid, uint32_t *keys, uint64_t *gids, uint32_t cap, uint32_t *len);
/* Fingerprints of n unpacked states, stride_ints apart (2 words each), in one launch. */
int rmc_fingerprints(void *ctx, const int32_t *unpacked, size_t stride_ints, uint64_t n, uint64_t *fps);
/* Seen-set membership (TLC's FPSet) of n fingerprints: out[i] = 1 if present.  Not for RCCL ranks. */
int rmc_seen_contains(void *ctx, const uint64_t *fps, uint64_t n, uint8_t *out);
/* 1 = TRUE, 0 = FALSE, RMC_EVAL_ERROR; one invariant bit */
int rmc_eval_invariant(void *ctx, const int32_t *unpacked, uint32_t invariant_bit, int32_t *value);
/* A graph from host arrays in place of a run's kept graph, so that tests reach the analyses' kernels with
 * shapes no Raft graph has (cycles, hubs, long chains): n_states global ids, n_edges (src[i], dst[i]) pairs
 * of them (RMC_E_ARG if one is past n_states), inv_values[g] in rmc_graph_inv_values' format.  Keep must be
 * on and the context not mid-run (before rmc_init, or after the run has finished: RMC_E_STATE otherwise).
 * It is one level as far as rmc_graph_reach_levels is concerned; the next rmc_init or rmc_reset drops it. */
int rmc_graph_import(void *ctx, uint64_t n_states, uint64_t n_edges, const uint32_t *src, const uint32_t *dst,
                     const uint16_t *inv_values);
/* Test hook, called in place of rmc_init: a level of given states stands where Init's would, so that tests
 * reach the search's batch kernels with states no test search gets to (msgs only grows, Raft.tla:43-45: the
 * message-heavy states lie deep).  It is TLC's behaviour with several initial states.  n (1..65,536) unpacked
 * states, stride_ints apart; a field out of range is RMC_E_ARG, more messages than the lanes RMC_E_CAPACITY.
 * The first state of each SYMMETRY/VIEW class in argument order is kept: the m kept roots get global ids
 * 0 .. m - 1 in that order, have no parent, and are level 1 (total_generated = n, total_distinct = m, depth 1,
 * queue m).  The INVARIANTs are evaluated on the roots in order; the first root that fails gives the verdict
 * Init would give, with a one-state trace holding that root (continuation counts violating roots at level 1).
 * Only each field's range is checked: a state no run reaches may still leave the kernels' domain later -- one at
 * term MaxElection with elections left sends, after BecomeCandidate, VoteReqs of a term the static message
 * universe does not hold (in a reachable state no term is past electionCount); the caller keeps its roots clear
 * of that over the levels it runs.  Everything after the call is the unchanged search.  Traces, rmc_state_path and rmc_violation_trace end at a
 * root; coverage's Init entry is (m, n); graph mode and keep deliver the roots as level 1, without edges.
 * rmc_reset returns to "before init": a following rmc_init starts from the real Init, a following
 * rmc_init_from seeds again.  rmc_simulate is untouched (walks start at Init).  Virtual shards take it when
 * the run starts replicated (shard_min_states > m; the roots stand on shard 0, as Init does); RCCL ranks, the
 * host-staged transport and shard_min_states <= m are refused with RMC_E_STATE, and so is rmc_checkpoint of a
 * seeded run (the file format has no place for the roots). */
int rmc_init_from(void *ctx, const int32_t *unpacked, size_t stride_ints, uint64_t n, rmc_level_stats *st);

/* Unpacked state (int32), the interchange format of every hook:
 *   votedFor[n] (-1 = None)  currentTerm[n]  role[n] (0 F, 1 C, 2 L)  commitIndex[n]  logLen[n]
 *   logs[n][V+1][2]          (term, val) per index 1..V+1; index 1 = (0,-1); unused = (0,0)
 *   matchIndex[n][n]  nextIndex[n][n]  pendingResponse[n][n]
 *   electionCount  restartCount  valSent[V] (-1 = None, 0 = FALSE)
 *   nmsgs  msgs[nmsgs][8], sorted in TLC order:
 *     type (0 VoteReq, 1 VoteResp, 2 AppendReq, 3 AppendResp) src dst term x1 x2 x3 x4
 *     VoteReq x1 = lastLogIndex x2 = lastLogTerm; AppendResp x1 = prevLogIndex x2 = succ;
 *     AppendReq x1 = prevLogIndex x2 = prevLogTerm x3 = leaderCommit x4 = entry (-1 none, else term*8+val)
 */
#define RMC_UNPACKED_INTS(n, V, nmsgs) (5 * (n) + (n) * ((V) + 1) * 2 + 3 * (n) * (n) + 3 + (V) + 8 * (nmsgs))

#ifdef __cplusplus
}
#endif
#endif /* RMC_H */
