"""raftmc -- Python binding of librmc.so, the MI355X-native model checker for kikimo/tla-raft.

This is the host-side mirror of the reference's only interface, the TLC run in
``myrun.sh:3`` (``-deadlock -workers 4 -config Raft.cfg Raft.tla``): parse the
model config, exhaust ``Raft.tla``'s state space breadth-first and report TLC's
numbers (states generated, distinct states, depth, counterexample).  Everything
runs in the HIP kernels behind the C-ABI declared in ``include/rmc.h``; there is
no CPU fallback -- ``ModelChecker`` raises if the library or the GPU is missing.
"""
from __future__ import annotations

import ctypes
from collections.abc import Sequence as _SeqABC
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RMC_LIBRARY") or os.path.join(os.path.dirname(_HERE), "build", "librmc.so")

RMC_OK, RMC_DONE, RMC_VIOLATION, RMC_ASSERT, RMC_EVAL_ERROR, RMC_DEADLOCK = 0, 1, 2, 3, 4, 5
STATUS_NAMES = {RMC_OK: "ok", RMC_DONE: "done", RMC_VIOLATION: "invariant", RMC_ASSERT: "assert",
                RMC_EVAL_ERROR: "eval_error", RMC_DEADLOCK: "deadlock"}
ERRORS = {-1: "RMC_E_ARG", -2: "RMC_E_DEVICE", -3: "RMC_E_MEMORY", -4: "RMC_E_CAPACITY",
          -5: "RMC_E_STATE", -6: "RMC_E_PARSE", -7: "RMC_E_COMM", -8: "RMC_E_SINK"}

# invariant bits (include/rmc.h), Raft.tla:434-503
INVARIANT_BITS = {
    "Inv": 1 << 0, "LeaderHasAllCommittedEntries": 1 << 0, "NoSplitVote": 1 << 1, "RaftCanCommt": 1 << 2,
    "FollowerCanCommit": 1 << 3, "CommitAll": 1 << 4, "NoAllCommit": 1 << 5, "ExistLeaderAndCandidate": 1 << 6,
}
INVARIANT_BY_BIT = ["Inv", "NoSplitVote", "RaftCanCommt", "FollowerCanCommit", "CommitAll", "NoAllCommit",
                    "ExistLeaderAndCandidate"]
ACTIONS = ("BecomeCandidate", "UpdateTerm", "ResponseVote", "BecomeLeader", "ClientReq", "LeaderAppendEntry",
           "FollowerAcceptEntry", "FollowerRejectEntry", "HandleAppendResp", "LeaderCanCommit", "Restart",
           "FollowerAppendEntry", "BecomeFollower")  # 11: never enabled (tla:425 variant); 12: tla:420 variant
SPEC_RAFT, SPEC_SEEDED, SPEC_BECOME_FOLLOWER = 0, 1, 2
SPEC_SPLIT_BRAIN, SPEC_COMMIT_PAST_LOG = 3, 4  # test variants: Assert / evaluation error reachable in a BFS
# include/rmc.h RMC_ABI_VERSION: the struct layouts below (_Config, _LevelStats, _Result) follow this ABI; a
# library of another ABI would be decoded with the wrong strides, so load_library refuses it
ABI_VERSION = 5


class RmcError(RuntimeError):
    pass


class _Config(ctypes.Structure):
    _fields_ = [
        ("n_servers", ctypes.c_int32), ("n_vals", ctypes.c_int32), ("max_election", ctypes.c_int32),
        ("max_restart", ctypes.c_int32), ("invariants", ctypes.c_uint32), ("check_deadlock", ctypes.c_int32),
        ("spec_variant", ctypes.c_int32), ("device", ctypes.c_int32), ("msg_cap", ctypes.c_int32),
        ("seen_log2", ctypes.c_int32), ("no_symmetry", ctypes.c_int32), ("chunk_successors", ctypes.c_uint64),
        ("rank", ctypes.c_int32), ("world_size", ctypes.c_int32), ("comm_unique_id", ctypes.c_void_p),
        ("virtual_shards", ctypes.c_int32), ("timing_phases", ctypes.c_uint32),
        ("device_levels", ctypes.c_uint32), ("shard_min_states", ctypes.c_uint64),
        ("invariant_order", ctypes.c_uint32), ("compact_log2", ctypes.c_uint32),
        ("seen_mem_bytes", ctypes.c_uint64), ("frontier_mem_bytes", ctypes.c_uint64),
    ]


class _LevelStats(ctypes.Structure):
    _fields_ = [
        ("level", ctypes.c_int32), ("status", ctypes.c_int32), ("expanded", ctypes.c_uint64),
        ("generated", ctypes.c_uint64), ("new_states", ctypes.c_uint64), ("total_generated", ctypes.c_uint64),
        ("total_distinct", ctypes.c_uint64), ("queue", ctypes.c_uint64), ("seconds", ctypes.c_double),
        ("kernel_ms", ctypes.c_double * 6), ("kernel_launches", ctypes.c_uint64 * 6),
        ("new_bytes", ctypes.c_uint64), ("self_loops", ctypes.c_uint64),
    ]


class _Result(ctypes.Structure):
    _fields_ = [
        ("status", ctypes.c_int32), ("depth", ctypes.c_int32), ("generated", ctypes.c_uint64),
        ("distinct", ctypes.c_uint64), ("queue", ctypes.c_uint64), ("violated", ctypes.c_int32),
        ("trace_len", ctypes.c_uint32), ("seconds", ctypes.c_double),
        ("seen_slots", ctypes.c_uint64), ("seen_slot_bytes", ctypes.c_int32), ("pad_", ctypes.c_int32),
        ("frontier_ring_bytes", ctypes.c_uint64), ("frontier_peak_bytes", ctypes.c_uint64),
    ]


class _SimConfig(ctypes.Structure):
    _fields_ = [("num_walks", ctypes.c_uint64), ("seed", ctypes.c_uint64), ("depth", ctypes.c_uint32),
                ("batch_walks", ctypes.c_uint32)]


class _SimResult(ctypes.Structure):
    _fields_ = [
        ("status", ctypes.c_int32), ("violated", ctypes.c_int32), ("walks", ctypes.c_uint64),
        ("states", ctypes.c_uint64), ("generated", ctypes.c_uint64), ("err_walk", ctypes.c_uint64),
        ("err_len", ctypes.c_uint32), ("longest", ctypes.c_uint32), ("ended_early", ctypes.c_uint64),
        ("seconds", ctypes.c_double),
    ]


class _Coverage(ctypes.Structure):
    _fields_ = [("generated", ctypes.c_uint64 * 16), ("distinct", ctypes.c_uint64 * 16),
                ("init_generated", ctypes.c_uint64), ("init_distinct", ctypes.c_uint64)]


class _Violations(ctypes.Structure):
    _fields_ = [("count", ctypes.c_uint64 * 16), ("first_level", ctypes.c_int32 * 16), ("total", ctypes.c_uint64)]


_U64P = ctypes.POINTER(ctypes.c_uint64)
_ALLREDUCE = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, _U64P, ctypes.c_int32, ctypes.c_int32)
_ALLGATHER = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, _U64P, ctypes.c_int32, _U64P)
_ALLTOALLV = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, _U64P, _U64P, ctypes.c_void_p,
                              _U64P, _U64P)


class _Transport(ctypes.Structure):
    _fields_ = [("user", ctypes.c_void_p), ("allreduce_u64", _ALLREDUCE), ("allgather_u64", _ALLGATHER),
                ("alltoallv", _ALLTOALLV)]


_I32P = ctypes.POINTER(ctypes.c_int32)
_U32P = ctypes.POINTER(ctypes.c_uint32)
_GRAPH_STATES = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, _I32P, ctypes.c_size_t)
_GRAPH_EDGES = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64, _U64P, _U32P, _U64P)


class _GraphSink(ctypes.Structure):
    _fields_ = [("user", ctypes.c_void_p), ("states", _GRAPH_STATES), ("edges", _GRAPH_EDGES),
                ("chunk_parents", ctypes.c_uint32), ("map_log2", ctypes.c_uint32)]


class _ReachQuery(ctypes.Structure):
    _fields_ = [("invariant_bit", ctypes.c_uint32), ("value", ctypes.c_int32)]


class _ReachResult(ctypes.Structure):
    _fields_ = [("states", ctypes.c_uint64), ("edges", ctypes.c_uint64), ("self_edges", ctypes.c_uint64),
                ("targets", ctypes.c_uint64), ("can_reach", ctypes.c_uint64), ("cannot_reach", ctypes.c_uint64),
                ("first_cannot", ctypes.c_uint64), ("first_cannot_level", ctypes.c_int32),
                ("max_distance", ctypes.c_int32), ("init_distance", ctypes.c_int32), ("rounds", ctypes.c_uint32),
                ("seconds", ctypes.c_double), ("csr_seconds", ctypes.c_double)]


class _GraphShape(ctypes.Structure):
    _fields_ = [("states", ctypes.c_uint64), ("edges", ctypes.c_uint64), ("self_edges", ctypes.c_uint64),
                ("back_edges", ctypes.c_uint64), ("sinks", ctypes.c_uint64), ("max_in", ctypes.c_uint64),
                ("max_out", ctypes.c_uint64), ("cyclic_states", ctypes.c_uint64),
                ("in_hist", ctypes.c_uint64 * 64), ("out_hist", ctypes.c_uint64 * 64)]


class _LiveQuery(ctypes.Structure):
    _fields_ = [("invariant_bit", ctypes.c_uint32), ("value", ctypes.c_int32), ("source_bit", ctypes.c_int32),
                ("source_value", ctypes.c_int32)]


class _LiveResult(ctypes.Structure):
    _fields_ = [("states", ctypes.c_uint64), ("edges", ctypes.c_uint64), ("self_edges", ctypes.c_uint64),
                ("targets", ctypes.c_uint64), ("must", ctypes.c_uint64), ("avoiders", ctypes.c_uint64),
                ("avoid_terminal", ctypes.c_uint64), ("first_avoid", ctypes.c_uint64), ("sources", ctypes.c_uint64),
                ("source_avoiders", ctypes.c_uint64), ("first_source_avoid", ctypes.c_uint64),
                ("first_avoid_level", ctypes.c_int32), ("first_source_avoid_level", ctypes.c_int32),
                ("max_within", ctypes.c_int32), ("init_within", ctypes.c_int32), ("rounds", ctypes.c_uint32),
                ("pad_", ctypes.c_uint32), ("seconds", ctypes.c_double), ("csr_seconds", ctypes.c_double)]


class _SccResult(ctypes.Structure):
    _fields_ = [("components", ctypes.c_uint64), ("nontrivial", ctypes.c_uint64), ("nontrivial_states", ctypes.c_uint64),
                ("largest", ctypes.c_uint64), ("trimmed", ctypes.c_uint64), ("rounds", ctypes.c_uint32),
                ("pad_", ctypes.c_uint32), ("seconds", ctypes.c_double), ("csr_seconds", ctypes.c_double)]


_lib = None


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load librmc.so; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RmcError(f"librmc.so not found at {path}: run __graft_entry__.build() (make -C tla-raft_amd)")
    lib = ctypes.CDLL(path)
    vp, i32, u32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64
    P = ctypes.POINTER
    lib.rmc_abi_version.restype = ctypes.c_int
    abi = lib.rmc_abi_version()
    if abi != ABI_VERSION:
        raise RmcError(f"{path} has ABI {abi}, this binding decodes ABI {ABI_VERSION}: rebuild it "
                       f"(make -C tla-raft_amd)")
    lib.rmc_parse_config.argtypes = [ctypes.c_char_p, ctypes.c_char_p, P(_Config), ctypes.c_char_p, ctypes.c_size_t]
    lib.rmc_create.argtypes = [P(_Config), P(vp)]
    lib.rmc_init.argtypes = [vp, P(_LevelStats)]
    lib.rmc_step.argtypes = [vp, P(_LevelStats)]
    lib.rmc_steps.argtypes = [vp, P(_LevelStats), u32, P(u32)]
    lib.rmc_set_timing.argtypes = [vp, u32]
    lib.rmc_probe_peak.argtypes = [i32, u32, u64, P(ctypes.c_double), P(ctypes.c_double)]
    lib.rmc_run.argtypes = [vp, P(_Result)]
    lib.rmc_reset.argtypes = [vp]
    lib.rmc_checkpoint.argtypes = [vp, ctypes.c_char_p]
    lib.rmc_resume.argtypes = [vp, ctypes.c_char_p]
    lib.rmc_run_levels.argtypes = [vp, P(_LevelStats), u32, P(u32), P(_Result)]
    lib.rmc_comm_unique_id.argtypes = [vp]
    lib.rmc_get_result.argtypes = [vp, P(_Result)]
    lib.rmc_trace_len.argtypes = [vp, P(u32)]
    lib.rmc_trace_state.argtypes = [vp, u32, P(i32), ctypes.c_size_t, P(i32), P(i32), P(i32)]
    lib.rmc_last_error.argtypes = [vp]
    lib.rmc_last_error.restype = ctypes.c_char_p
    lib.rmc_destroy.argtypes = [vp]
    lib.rmc_destroy.restype = None
    lib.rmc_successors.argtypes = [vp, P(i32), P(i32), ctypes.c_size_t, u32, P(u32), P(u64), P(u32)]
    lib.rmc_fingerprint.argtypes = [vp, P(i32), P(u64)]
    lib.rmc_eval_invariant.argtypes = [vp, P(i32), u32, P(i32)]
    lib.rmc_set_transport.argtypes = [P(_Transport)]
    lib.rmc_state_path.argtypes = [vp, u64, P(u32), P(u64), u32, P(u32)]
    lib.rmc_fingerprints.argtypes = [vp, P(i32), ctypes.c_size_t, u64, P(u64)]
    lib.rmc_seen_contains.argtypes = [vp, P(u64), u64, P(ctypes.c_uint8)]
    lib.rmc_simulate.argtypes = [vp, P(_SimConfig), P(_SimResult), P(u32), P(u32)]
    # (additive within ABI 5: an older library of the same ABI, as an A/B run loads through RMC_LIBRARY,
    # lacks the two; set_coverage() then raises)
    if hasattr(lib, "rmc_set_coverage"):
        lib.rmc_set_coverage.argtypes = [vp, i32]
        lib.rmc_get_coverage.argtypes = [vp, P(_Coverage)]
    if hasattr(lib, "rmc_set_full_state"):  # (likewise)
        lib.rmc_set_full_state.argtypes = [vp, i32]
    if hasattr(lib, "rmc_set_continue"):  # (likewise)
        lib.rmc_set_continue.argtypes = [vp, i32]
        lib.rmc_get_violations.argtypes = [vp, P(_Violations)]
        lib.rmc_get_violation_levels.argtypes = [vp, u32, P(u64), u32, P(u32)]
        lib.rmc_violation_trace.argtypes = [vp, u32]
    if hasattr(lib, "rmc_set_graph"):  # (likewise)
        lib.rmc_set_graph.argtypes = [vp, P(_GraphSink)]
    if hasattr(lib, "rmc_set_graph_keep"):  # (likewise)
        lib.rmc_set_graph_keep.argtypes = [vp, i32]
        lib.rmc_graph_reach.argtypes = [vp, P(_ReachQuery), P(_ReachResult), vp]
        lib.rmc_graph_reach_levels.argtypes = [vp, P(u64), P(u64), u32, P(u32)]
        lib.rmc_graph_shape.argtypes = [vp, P(_GraphShape)]
        lib.rmc_graph_inv_values.argtypes = [vp, vp, u64]
        lib.rmc_graph_import.argtypes = [vp, u64, u64, vp, vp, vp]
    if hasattr(lib, "rmc_graph_eventually"):  # (likewise)
        lib.rmc_graph_eventually.argtypes = [vp, P(_LiveQuery), P(_LiveResult), vp]
        lib.rmc_graph_eventually_levels.argtypes = [vp, P(u64), P(u64), u32, P(u32)]
        lib.rmc_graph_avoid_path.argtypes = [vp, u64, P(u64), u32, P(u32), P(i32)]
        lib.rmc_graph_scc.argtypes = [vp, P(_SccResult), vp]
    if hasattr(lib, "rmc_init_from"):  # (likewise)
        lib.rmc_init_from.argtypes = [vp, vp, ctypes.c_size_t, u64, P(_LevelStats)]
    _lib = lib
    return lib


# ------------------------------------------------------------------------------ config
@dataclass
class ModelConfig:
    """What Raft.cfg binds (Raft.cfg:1-34) plus TLC's -deadlock flag (myrun.sh:3)."""
    n_servers: int = 3
    n_vals: int = 2
    max_election: int = 3
    max_restart: int = 3
    invariants: Tuple[str, ...] = ("Inv",)
    check_deadlock: bool = False
    spec_variant: int = SPEC_RAFT
    symmetry: bool = True
    view: bool = True                # False: states are identified by all twelve variables (set_full_state)
    device: int = -1
    msg_cap: int = 0
    seen_log2: int = 0
    chunk_successors: int = 0
    virtual_shards: int = 0          # >1: that many fingerprint-owner shards on one device
    rank: int = 0                    # multi-GPU: this process's rank
    world_size: int = 1              # multi-GPU: ranks (one process per GPU)
    comm_unique_id: Optional[bytes] = None  # 128 bytes from comm_unique_id() on rank 0
    timing_phases: int = 0           # bit i: time phase i with HIP events (0 = all phases)
    device_levels: int = 0           # levels per host round trip in run() (0 = auto, 1 = host-driven)
    shard_min_states: int = 0        # >1 shards: replicate levels below this size (0 = auto 2^20, 1 = always shard)
    compact_log2: int = 0            # seen set: 16-B slots up to 2^compact_log2 slots, then 8-B slots (0 = auto 27)
    seen_mem_bytes: int = 0          # compact seen-set budget (0 = auto: half the free device memory)
    frontier_mem_bytes: int = 0      # frontier ring budget once the seen set is compact (0 = auto)

    def to_c(self) -> _Config:
        c = _Config()
        c.n_servers, c.n_vals = self.n_servers, self.n_vals
        c.max_election, c.max_restart = self.max_election, self.max_restart
        mask, order, k = 0, 0, 0
        for name in self.invariants:  # cfg order: TLC checks the invariants in that order
            bit = INVARIANT_BITS[name]
            if not mask & bit:
                order |= (bit.bit_length()) << (4 * k)
                k += 1
            mask |= bit
        c.invariants = mask
        c.invariant_order = order
        c.check_deadlock = int(self.check_deadlock)
        c.spec_variant = self.spec_variant
        c.device = self.device
        c.msg_cap = self.msg_cap
        c.seen_log2 = self.seen_log2
        c.no_symmetry = 0 if self.symmetry else 1
        c.chunk_successors = self.chunk_successors
        c.rank, c.world_size = self.rank, self.world_size
        c.virtual_shards = self.virtual_shards
        c.timing_phases = self.timing_phases
        c.device_levels = self.device_levels
        c.shard_min_states = self.shard_min_states
        c.compact_log2 = self.compact_log2
        c.seen_mem_bytes = self.seen_mem_bytes
        c.frontier_mem_bytes = self.frontier_mem_bytes
        if self.comm_unique_id is not None:
            self._idbuf = ctypes.create_string_buffer(bytes(self.comm_unique_id), 128)
            c.comm_unique_id = ctypes.cast(self._idbuf, ctypes.c_void_p)
        return c


_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def sim_random(seed: int, walk: int, step: int) -> int:
    """The 32-bit value r of simulation mode's choice (include/rmc.h): this project's own definition,
    not TLC's random generator."""
    z = (seed & _M64) ^ ((walk * _GOLDEN) & _M64)
    z = (z + (step + 1) * _GOLDEN) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return z >> 32


def sim_choice(seed: int, walk: int, step: int, count: int) -> int:
    """Index of the successor that walk `walk` takes at step `step` (0 = from Init) among `count`
    successors in TLC order: (r * count) >> 32."""
    return (sim_random(seed, walk, step) * count) >> 32


def probe_peak(device: int = -1, table_log2: int = 28, probes: int = 1 << 28) -> float:
    """Random one-slot probes/s of a seen-set-shaped table (16-B slots) on the GPU."""
    lib = load_library()
    r, t = ctypes.c_double(), ctypes.c_double()
    rc = lib.rmc_probe_peak(device, table_log2, probes, ctypes.byref(r), ctypes.byref(t))
    if rc != RMC_OK:
        raise RmcError(f"rmc_probe_peak failed: {ERRORS.get(rc, rc)}")
    return r.value


def parse_config(cfg_text: str, tla_text: Optional[str] = None) -> ModelConfig:
    """Parse Raft.cfg text (and identify Raft.tla by content) through the library's parser."""
    lib = load_library()
    c = _Config()
    err = ctypes.create_string_buffer(512)
    rc = lib.rmc_parse_config(cfg_text.encode(), tla_text.encode() if tla_text is not None else None,
                              ctypes.byref(c), err, 512)
    if rc != RMC_OK:
        raise RmcError(err.value.decode())
    invs, o = [], c.invariant_order
    while o:
        invs.append(INVARIANT_BY_BIT[(o & 15) - 1])
        o >>= 4
    invs = tuple(invs) or tuple(name for bit, name in enumerate(INVARIANT_BY_BIT) if c.invariants & (1 << bit))
    return ModelConfig(n_servers=c.n_servers, n_vals=c.n_vals, max_election=c.max_election,
                       max_restart=c.max_restart, invariants=invs, check_deadlock=bool(c.check_deadlock),
                       spec_variant=c.spec_variant, symmetry=not c.no_symmetry)


def comm_unique_id() -> bytes:
    """RCCL unique id for a multi-GPU run (rank 0 creates it, every rank passes it in)."""
    lib = load_library()
    buf = ctypes.create_string_buffer(128)
    rc = lib.rmc_comm_unique_id(buf)
    if rc != RMC_OK:
        raise RmcError(f"rmc_comm_unique_id failed: {ERRORS.get(rc, rc)}")
    return buf.raw


class HostTransport:
    """The sharded protocol's collectives through host memory and a torch.distributed process group
    (include/rmc.h rmc_transport) instead of RCCL: every rank of a world_size > 1 run installs one
    before creating its ModelChecker (without comm_unique_id).  With a gloo group the ranks may share
    one device -- the multi-rank path of SURVEY 8(e) as separate processes on a one-GPU box (tests) --
    since RCCL refuses two ranks on one device.  A callback that raises fails the step (RMC_E_COMM)."""

    def __init__(self, group=None):
        import numpy as np
        import torch
        import torch.distributed as dist
        self._np, self._torch, self._dist, self._group = np, torch, dist, group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self._c = _Transport(None, _ALLREDUCE(self._allreduce), _ALLGATHER(self._allgather),
                             _ALLTOALLV(self._alltoallv))

    @staticmethod
    def _failed():
        import sys
        import traceback
        traceback.print_exc(file=sys.stderr)
        return 1

    def _u64(self, ptr, n):
        return self._np.ctypeslib.as_array(ptr, shape=(n,))

    def _allreduce(self, _user, v, n, is_max):
        try:
            a = self._u64(v, n)
            t = self._torch.from_numpy(a.astype(self._np.int64))  # values < 2^63 (counts, keys, codes)
            self._dist.all_reduce(t, op=self._dist.ReduceOp.MAX if is_max else self._dist.ReduceOp.SUM,
                                  group=self._group)
            a[:] = t.numpy().astype(self._np.uint64)
            return 0
        except Exception:  # noqa: BLE001 -- the library raises RMC_E_COMM
            return self._failed()

    def _allgather(self, _user, row, k, out):
        try:
            t = self._torch.from_numpy(self._u64(row, k).astype(self._np.int64))
            parts = [self._torch.empty_like(t) for _ in range(self.world)]
            self._dist.all_gather(parts, t, group=self._group)
            self._u64(out, self.world * k)[:] = self._torch.cat(parts).numpy().astype(self._np.uint64)
            return 0
        except Exception:  # noqa: BLE001
            return self._failed()

    def _alltoallv(self, _user, send, send_off, send_bytes, recv, recv_off, recv_bytes):
        try:
            W = self.world
            sb, rb = self._u64(send_bytes, W).tolist(), self._u64(recv_bytes, W).tolist()
            so, ro = self._u64(send_off, W).tolist(), self._u64(recv_off, W).tolist()
            send_end = max([int(o + b) for o, b in zip(so, sb)] + [1])
            recv_end = max([int(o + b) for o, b in zip(ro, rb)] + [1])
            src = self._np.ctypeslib.as_array(ctypes.cast(send, ctypes.POINTER(ctypes.c_uint8)), shape=(send_end,))
            dst = self._np.ctypeslib.as_array(ctypes.cast(recv, ctypes.POINTER(ctypes.c_uint8)), shape=(recv_end,))
            # all_to_all_single takes the parts in rank order, contiguous
            ti = self._torch.from_numpy(self._np.concatenate([src[int(so[q]):int(so[q] + sb[q])] for q in range(W)]))
            to = self._torch.empty(int(sum(rb)), dtype=self._torch.uint8)
            self._dist.all_to_all_single(to, ti, [int(x) for x in rb], [int(x) for x in sb], group=self._group)
            got, at = to.numpy(), 0
            for q in range(W):
                dst[int(ro[q]):int(ro[q] + rb[q])] = got[at:at + int(rb[q])]
                at += int(rb[q])
            return 0
        except Exception:  # noqa: BLE001
            return self._failed()

    def install(self):
        """Route the collectives of every ModelChecker created from now on in this process through this group."""
        rc = load_library().rmc_set_transport(ctypes.byref(self._c))
        if rc != RMC_OK:
            raise RmcError(f"rmc_set_transport failed: {ERRORS.get(rc, rc)}")
        return self

    @staticmethod
    def uninstall():
        load_library().rmc_set_transport(None)


# ------------------------------------------------------------------------------ unpacked states
MSG_TYPES = ("VoteReq", "VoteResp", "AppendReq", "AppendResp")


def unpacked_len(n: int, V: int, nmsgs: int) -> int:
    return 5 * n + n * (V + 1) * 2 + 3 * n * n + 3 + V + 8 * nmsgs


def state_to_unpacked(d: dict, n: int, V: int) -> List[int]:
    """JSON state (oracle fixture format) -> rmc unpacked int32 layout (include/rmc.h)."""
    u: List[int] = []
    u += d["votedFor"] + d["currentTerm"] + d["role"] + d["commitIndex"] + [len(l) for l in d["logs"]]
    for log in d["logs"]:
        for x in range(V + 1):
            if x < len(log):
                u += [log[x][0], log[x][1]]
            else:
                u += [0, 0]
    for r in d["matchIndex"]:
        u += r
    for r in d["nextIndex"]:
        u += r
    for r in d["pendingResponse"]:
        u += [1 if b else 0 for b in r]
    u += [d["electionCount"], d["restartCount"]] + list(d["valSent"]) + [len(d["msgs"])]
    for m in d["msgs"]:
        t = MSG_TYPES.index(m["type"])
        rec = [t, m["src"], m["dst"], m["term"], 0, 0, 0, 0]
        if m["type"] == "VoteReq":
            rec[4:6] = [m["lastLogIndex"], m["lastLogTerm"]]
        elif m["type"] == "AppendResp":
            rec[4:6] = [m["prevLogIndex"], 1 if m["succ"] else 0]
        elif m["type"] == "AppendReq":
            e = m["entries"]
            rec[4:8] = [m["prevLogIndex"], m["prevLogTerm"], m["leaderCommit"], e[0][0] * 8 + e[0][1] if e else -1]
        u += rec
    return u


def unpacked_to_state(u: Sequence[int], n: int, V: int) -> dict:
    k = 0

    def take(c):
        nonlocal k
        r = list(u[k:k + c])
        k += c
        return r

    d: Dict[str, object] = {}
    d["votedFor"] = take(n)
    d["currentTerm"] = take(n)
    d["role"] = take(n)
    d["commitIndex"] = take(n)
    ll = take(n)
    logs = []
    for i in range(n):
        ent = take(2 * (V + 1))
        logs.append([[ent[2 * x], ent[2 * x + 1]] for x in range(ll[i])])
    d["logs"] = logs
    d["matchIndex"] = [take(n) for _ in range(n)]
    d["nextIndex"] = [take(n) for _ in range(n)]
    d["pendingResponse"] = [[bool(x) for x in take(n)] for _ in range(n)]
    d["electionCount"], d["restartCount"] = take(2)
    d["valSent"] = take(V)
    nm = take(1)[0]
    msgs = []
    for _ in range(nm):
        t, src, dst, term, x1, x2, x3, x4 = take(8)
        m = {"type": MSG_TYPES[t], "src": src, "dst": dst, "term": term}
        if t == 0:
            m.update(lastLogIndex=x1, lastLogTerm=x2)
        elif t == 3:
            m.update(prevLogIndex=x1, succ=bool(x2))
        elif t == 2:
            m.update(prevLogIndex=x1, prevLogTerm=x2, leaderCommit=x3,
                     entries=[] if x4 < 0 else [[x4 // 8, x4 % 8]])
        msgs.append(m)
    d["msgs"] = msgs
    return d


# ------------------------------------------------------------------------------ checker
@dataclass
class LevelStats:
    level: int
    status: str
    expanded: int
    generated: int
    new_states: int
    total_generated: int
    total_distinct: int
    queue: int
    seconds: float
    kernel_ms: List[float] = field(default_factory=list)
    kernel_launches: List[int] = field(default_factory=list)
    new_bytes: int = 0
    self_loops: int = 0  # ABI 5: successors equal to their parent, set apart (single-GPU split chunks)


class _LazyLevels(_SeqABC):
    """Per-level statistics of one run, converted to LevelStats on first access (a run's levels come
    back from the library as one array; building dozens of Python objects per exhaustion would cost
    more host time than a small configuration's whole GPU run)."""

    def __init__(self, raw, n: int):
        self._raw = (_LevelStats * n)()
        ctypes.memmove(self._raw, raw, ctypes.sizeof(_LevelStats) * n)
        self._cache: List[Optional[LevelStats]] = [None] * n

    def __len__(self):
        return len(self._cache)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        if self._cache[i] is None:
            self._cache[i] = ModelChecker._stats(self._raw[i])
        return self._cache[i]

    def __eq__(self, other):
        return list(self) == list(other)

    def __repr__(self):
        return repr(list(self))


@dataclass
class Result:
    status: str
    depth: int
    generated: int
    distinct: int
    queue: int
    violated: Optional[str]
    trace_len: int
    seconds: float
    levels: List[LevelStats] = field(default_factory=list)
    seen_slots: int = 0
    seen_slot_bytes: int = 0
    frontier_ring_bytes: int = 0
    frontier_peak_bytes: int = 0


@dataclass
class ReachResult:
    """rmc_graph_reach's result (include/rmc.h rmc_reach_result); first_cannot / first_cannot_level / init_distance
    are None where the library reports none; dist: numpy u32 per state (0xFFFFFFFF = cannot) with want_dist."""
    invariant: str
    value: bool
    states: int
    edges: int
    self_edges: int
    targets: int
    can_reach: int
    cannot_reach: int
    first_cannot: Optional[int]
    first_cannot_level: Optional[int]
    max_distance: int
    init_distance: Optional[int]
    rounds: int
    seconds: float
    csr_seconds: float
    dist: object = None


@dataclass
class LiveResult:
    """rmc_graph_eventually's result (include/rmc.h rmc_live_result); first_avoid / first_avoid_level / init_within
    are None where the library reports none, the source fields None without a source set; within: numpy u32 per state
    (0xFFFFFFFF = avoider) with want_within."""
    invariant: str
    value: bool
    source: Optional[str]
    source_value: Optional[bool]
    states: int
    edges: int
    self_edges: int
    targets: int
    must: int
    avoiders: int
    avoid_terminal: int
    first_avoid: Optional[int]
    first_avoid_level: Optional[int]
    max_within: int
    init_within: Optional[int]
    sources: Optional[int]
    source_avoiders: Optional[int]
    first_source_avoid: Optional[int]
    first_source_avoid_level: Optional[int]
    rounds: int
    seconds: float
    csr_seconds: float
    within: object = None


@dataclass
class SccResult:
    """rmc_graph_scc's result (include/rmc.h rmc_scc_result); comp: numpy u32 per state, the smallest gid of its
    component, with want_comp."""
    components: int
    nontrivial: int
    nontrivial_states: int
    largest: int
    trimmed: int
    rounds: int
    seconds: float
    csr_seconds: float
    comp: object = None


@dataclass
class SimResult:
    """ModelChecker.simulate: the accounted walks (0..err_walk on an error, all of them otherwise)."""
    status: str
    violated: Optional[str]
    walks: int
    states: int
    generated: int
    err_walk: Optional[int]
    err_len: Optional[int]
    longest: int
    ended_early: int
    seconds: float
    lengths: Optional[List[int]] = None  # keep_walks: states per walk (0: not accounted)
    keys: Optional[List[List[Tuple[int, int, int]]]] = None  # keep_walks: (server, action, witness) per step


class ModelChecker:
    """One GPU model-checking run (TLC's ModelChecker for myrun.sh:3)."""

    def __init__(self, cfg: ModelConfig):
        self.lib = load_library()
        self.cfg = cfg
        self._c = cfg.to_c()
        h = ctypes.c_void_p()
        rc = self.lib.rmc_create(ctypes.byref(self._c), ctypes.byref(h))
        if rc != RMC_OK:
            raise RmcError(f"rmc_create failed: {ERRORS.get(rc, rc)}: {self.lib.rmc_last_error(None).decode()}")
        self.h = h
        self.levels: List[LevelStats] = []
        self._inited = False
        if not cfg.view:
            try:
                self.set_full_state(True)
            except RmcError:
                self.close()
                raise

    def close(self):
        if getattr(self, "h", None):
            self.lib.rmc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _levels_list(self) -> list:
        if not isinstance(self.levels, list):
            self.levels = list(self.levels)
        return self.levels

    def _check(self, rc: int) -> int:
        if rc < 0:
            raise RmcError(f"{ERRORS.get(rc, rc)}: {self.lib.rmc_last_error(self.h).decode()}")
        return rc

    @staticmethod
    def _stats(s: _LevelStats) -> LevelStats:
        return LevelStats(s.level, STATUS_NAMES.get(s.status, str(s.status)), s.expanded, s.generated,
                          s.new_states, s.total_generated, s.total_distinct, s.queue, s.seconds,
                          list(s.kernel_ms), list(s.kernel_launches), s.new_bytes, s.self_loops)

    def init(self) -> LevelStats:
        st = _LevelStats()
        self._check(self.lib.rmc_init(self.h, ctypes.byref(st)))
        self._inited = True
        self._g_import_n = None
        ls = self._stats(st)
        self._levels_list().append(ls)
        return ls

    def init_from(self, states) -> LevelStats:
        """Test hook (rmc_init_from), in place of init(): the given states stand where Init's level would --
        TLC's behaviour with several initial states.  `states`: state dicts, or a 2-D int32 array of unpacked
        rows.  The first state of each symmetry/VIEW class is kept as a root (global ids in that order)."""
        import numpy as np
        if not hasattr(self.lib, "rmc_init_from"):
            raise RmcError("this librmc.so has no rmc_init_from")
        if isinstance(states, np.ndarray):
            arr = np.ascontiguousarray(states, dtype=np.int32)
        else:
            rows = [state_to_unpacked(d, self.cfg.n_servers, self.cfg.n_vals) for d in states]
            arr = np.zeros((len(rows), max([len(r) for r in rows] + [1])), dtype=np.int32)
            for i, r in enumerate(rows):
                arr[i, :len(r)] = r
        if arr.ndim != 2:
            raise RmcError("RMC_E_ARG: init_from: a 2-D array of unpacked rows")
        st = _LevelStats()
        self._check(self.lib.rmc_init_from(self.h, arr.ctypes.data, arr.shape[1], arr.shape[0], ctypes.byref(st)))
        self._inited = True
        self._g_import_n = None
        ls = self._stats(st)
        self._levels_list().append(ls)
        return ls

    def reset(self) -> None:
        """Start over from Init on the next run(), keeping the device buffers."""
        self._check(self.lib.rmc_reset(self.h))
        self._g_import_n = None
        self.levels = []
        self._inited = False

    def checkpoint(self, path: str) -> None:
        """Write the run so far (seen set, current level, parent references, counters) to path (an RCCL
        rank of a world_size > 1 run: path + ".rank<r>"; virtual shards: all in path)."""
        self._check(self.lib.rmc_checkpoint(self.h, os.fsencode(path)))

    def resume(self, path: str) -> None:
        """Continue a checkpointed run of the same configuration (on a fresh or reset checker)."""
        self._check(self.lib.rmc_resume(self.h, os.fsencode(path)))
        self._inited = True

    def step(self) -> LevelStats:
        st = _LevelStats()
        self._check(self.lib.rmc_step(self.h, ctypes.byref(st)))
        ls = self._stats(st)
        self._levels_list().append(ls)
        return ls

    def set_timing(self, phases: int) -> None:
        """HIP-event phase timing from now on: 0 = off, 0xFFFFFFFF = all phases, else a phase mask."""
        self._check(self.lib.rmc_set_timing(self.h, phases))

    def steps(self, cap: int = 65) -> List[LevelStats]:
        """The levels one host round trip covers (rmc_steps): a device-driven batch on one GPU."""
        buf = (_LevelStats * cap)()
        n = ctypes.c_uint32()
        self._check(self.lib.rmc_steps(self.h, buf, cap, ctypes.byref(n)))
        out = [self._stats(buf[i]) for i in range(n.value)]
        self._levels_list().extend(out)
        return out

    def run(self) -> Result:
        """Exhaust the state space (or stop at the first error) inside the library."""
        cap = 4096
        if getattr(self, "_runbuf", None) is None:
            self._runbuf = (_LevelStats * cap)()  # reused by every run of this checker
        n = ctypes.c_uint32()
        if not getattr(self, "_inited", False):
            self._g_import_n = None
        self._check(self.lib.rmc_run_levels(self.h, self._runbuf, cap, ctypes.byref(n), None))
        self._inited = True
        lazy = _LazyLevels(self._runbuf, n.value)
        self.levels = lazy if not self.levels else list(self.levels) + list(lazy)
        return self.result()

    def result(self) -> Result:
        r = _Result()
        self._check(self.lib.rmc_get_result(self.h, ctypes.byref(r)))
        return Result(STATUS_NAMES.get(r.status, str(r.status)), r.depth, r.generated, r.distinct, r.queue,
                      INVARIANT_BY_BIT[r.violated] if r.violated >= 0 else None, r.trace_len, r.seconds,
                      self.levels if isinstance(self.levels, _LazyLevels) else list(self.levels), r.seen_slots,
                      r.seen_slot_bytes, r.frontier_ring_bytes,
                      r.frontier_peak_bytes)

    def simulate(self, num_walks: int, depth: int = 100, seed: int = 0, batch_walks: int = 0,
                 keep_walks: bool = False) -> SimResult:
        """TLC's -simulate on the GPU: num_walks seeded random behaviours of at most `depth` states from
        Init, the invariants checked on every state (include/rmc.h rmc_simulate).  After an error,
        trace() returns the erring behaviour.  keep_walks: also every walk's length and step keys."""
        sc = _SimConfig(num_walks, seed & _M64, depth, batch_walks)
        r = _SimResult()
        lens = keys = None
        if keep_walks and num_walks > 0 and depth > 0:
            lens = (ctypes.c_uint32 * num_walks)()
            keys = (ctypes.c_uint32 * max(1, num_walks * (depth - 1)))()
        rc = self._check(self.lib.rmc_simulate(self.h, ctypes.byref(sc), ctypes.byref(r), lens, keys))
        err = rc != RMC_DONE
        out = SimResult(STATUS_NAMES.get(rc, str(rc)), INVARIANT_BY_BIT[r.violated] if r.violated >= 0 else None,
                        r.walks, r.states, r.generated, r.err_walk if err else None, r.err_len if err else None,
                        r.longest, r.ended_early, r.seconds)
        if lens is not None:
            out.lengths = list(lens)
            d1 = depth - 1
            out.keys = [[(k >> 24, (k >> 16) & 0xFF, k & 0xFFFF) for k in keys[w * d1:w * d1 + max(n - 1, 0)]]
                        for w, n in enumerate(out.lengths)]
        return out

    def set_full_state(self, on: bool = True) -> None:
        """Identify states by all twelve variables instead of the cfg's VIEW (include/rmc.h
        rmc_set_full_state): the seen set, coverage, continuation, graph mode, fingerprint(s) and
        seen_contains then work on whole states.  On a fresh or reset checker, before init() / run();
        reset() keeps it.  ModelConfig(view=False) calls this right after create."""
        if not hasattr(self.lib, "rmc_set_full_state"):
            raise RmcError("this librmc.so cannot search on the whole state (rmc_set_full_state): rebuild it")
        self._check(self.lib.rmc_set_full_state(self.h, 1 if on else 0))

    def set_coverage(self, on: bool = True) -> None:
        """TLC's -coverage: count, per action of Next, the successors generated and the states first found
        (include/rmc.h rmc_set_coverage).  On a fresh or reset checker, before init() / run()."""
        if not hasattr(self.lib, "rmc_set_coverage"):
            raise RmcError("this librmc.so has no action coverage (rmc_set_coverage): rebuild it")
        self._check(self.lib.rmc_set_coverage(self.h, 1 if on else 0))

    def coverage(self) -> dict:
        """{action name: (distinct, generated)} over ACTIONS, plus "Init": the levels finished so far (on an
        error: up to TLC's counters at the error).  1 + the sums equal the run's distinct / generated."""
        c = _Coverage()
        self._check(self.lib.rmc_get_coverage(self.h, ctypes.byref(c)))
        out = {"Init": (c.init_distinct, c.init_generated)}
        for a, name in enumerate(ACTIONS):
            out[name] = (c.distinct[a], c.generated[a])
        return out

    def set_continue(self, on: bool = True) -> None:
        """TLC's -continue: search past invariant violations and count them per invariant (include/rmc.h
        rmc_set_continue).  On a fresh or reset checker, before init() / run()."""
        if not hasattr(self.lib, "rmc_set_continue"):
            raise RmcError("this librmc.so has no continuation (rmc_set_continue): rebuild it")
        self._check(self.lib.rmc_set_continue(self.h, 1 if on else 0))

    @staticmethod
    def _inv_bit(name: str) -> int:
        return INVARIANT_BY_BIT.index("Inv" if name == "LeaderHasAllCommittedEntries" else name)

    def violations(self) -> dict:
        """{invariant name: (count, first_level or None)} over the configured invariants in cfg order: the
        explored states attributed to each (the first FALSE one in cfg order) over the levels finished so
        far, and the level of the first of them in TLC -workers 1 order."""
        v = _Violations()
        self._check(self.lib.rmc_get_violations(self.h, ctypes.byref(v)))
        out = {}
        for name in self.cfg.invariants:
            b = self._inv_bit(name)
            out[name] = (v.count[b], v.first_level[b] or None)
        return out

    def violation_levels(self, name: str) -> List[int]:
        """The invariant's violation count per BFS level ([0]: Init's level); sums to its count."""
        cap = 4096
        buf, n = (ctypes.c_uint64 * cap)(), ctypes.c_uint32()
        self._check(self.lib.rmc_get_violation_levels(self.h, self._inv_bit(name), buf, cap, ctypes.byref(n)))
        return list(buf[:n.value])

    def violation_trace(self, name: str) -> List[Tuple[Optional[Tuple[int, int, int]], dict]]:
        """The behaviour from Init to the invariant's first violating state, as trace() returns one (it
        becomes the current trace)."""
        self._check(self.lib.rmc_violation_trace(self.h, self._inv_bit(name)))
        return self.trace()

    def set_graph(self, states: bool = True, chunk_parents: int = 0, map_log2: int = 0, on_states=None,
                  on_edges=None) -> None:
        """TLC's -dump: stream the state graph of the run (include/rmc.h rmc_set_graph).  On a fresh or
        reset checker, before init() / run().  Without callbacks the binding collects: graph_edges() and
        graph_states() return what has been delivered so far.  on_states(gid0, unpacked) gets a numpy int32
        array of shape (n, stride) and on_edges(src, key, dst) three numpy arrays (u64, u32, u64), all views
        valid only during the call; a callback that raises or returns a true value fails the step with
        RMC_E_SINK.  states=False: the states are not copied back."""
        import numpy as np
        if not hasattr(self.lib, "rmc_set_graph"):
            raise RmcError("this librmc.so has no graph mode (rmc_set_graph): rebuild it")
        self._g_src, self._g_key, self._g_dst, self._g_states = [], [], [], []

        def failed():
            import sys
            import traceback
            traceback.print_exc(file=sys.stderr)
            return 1

        def c_states(_user, gid0, n, unpacked, stride):
            try:
                a = np.ctypeslib.as_array(unpacked, shape=(n, stride))
                if on_states is not None:
                    return 1 if on_states(gid0, a) else 0
                self._g_states.append(a.copy())
                return 0
            except Exception:  # noqa: BLE001 -- the library raises RMC_E_SINK
                return failed()

        def c_edges(_user, n, src, key, dst):
            try:
                s, k, d = (np.ctypeslib.as_array(p, shape=(n,)) for p in (src, key, dst))
                if on_edges is not None:
                    return 1 if on_edges(s, k, d) else 0
                self._g_src.append(s.copy())
                self._g_key.append(k.copy())
                self._g_dst.append(d.copy())
                return 0
            except Exception:  # noqa: BLE001
                return failed()

        # (the callback objects live as long as the checker: the library calls them from every step)
        self._g_sink = _GraphSink(None, _GRAPH_STATES(c_states) if states else _GRAPH_STATES(), _GRAPH_EDGES(c_edges),
                                  chunk_parents, map_log2)
        self._g_on = False
        self._check(self.lib.rmc_set_graph(self.h, ctypes.byref(self._g_sink)))
        self._g_on = True

    def clear_graph(self) -> None:
        """Graph mode off (on a fresh or reset checker); what was collected is dropped."""
        if getattr(self, "_g_on", False):
            self._g_on = False
            self._check(self.lib.rmc_set_graph(self.h, None))

    def _graph_check(self):
        if not getattr(self, "_g_on", False):
            raise RmcError("RMC_E_STATE: graph mode is off (set_graph)")

    def graph_edges(self):
        """(src u64, key u32, dst u64) numpy arrays of the edges delivered so far, in TLC -workers 1 order;
        key = server << 24 | action << 16 | witness."""
        import numpy as np
        self._graph_check()
        cat = lambda parts, t: np.concatenate(parts) if parts else np.zeros(0, dtype=t)  # noqa: E731
        return cat(self._g_src, np.uint64), cat(self._g_key, np.uint32), cat(self._g_dst, np.uint64)

    def graph_states(self) -> List[dict]:
        """The states delivered so far in global-id order (Init first), as unpacked_to_state dicts."""
        self._graph_check()
        n, V = self.cfg.n_servers, self.cfg.n_vals
        return [unpacked_to_state(row.tolist(), n, V) for part in self._g_states for row in part]

    # ---- reachability queries over the kept state graph (include/rmc.h rmc_set_graph_keep) ----
    def set_graph_keep(self, on: bool = True) -> None:
        """Keep the run's state graph on the device for graph_reach() / graph_shape(): the graph pass runs
        with or without set_graph().  On a fresh or reset checker, before init() / run()."""
        if not hasattr(self.lib, "rmc_set_graph_keep"):
            raise RmcError("this librmc.so keeps no graph (rmc_set_graph_keep): rebuild it")
        self._check(self.lib.rmc_set_graph_keep(self.h, 1 if on else 0))

    def graph_reach(self, invariant: str, value: bool = True, want_dist: bool = False) -> ReachResult:
        """Which states can still reach a state on which `invariant` is `value`: a backward BFS on the device
        over the kept graph (the levels finished so far, or the imported graph)."""
        import numpy as np
        q, r = _ReachQuery(self._inv_bit(invariant), 1 if value else 0), _ReachResult()
        dist = None
        if want_dist:
            dist = np.empty(self._kept_states(), dtype=np.uint32)
        self._check(self.lib.rmc_graph_reach(self.h, ctypes.byref(q), ctypes.byref(r),
                                             dist.ctypes.data if dist is not None else None))
        none = r.first_cannot == 0xFFFFFFFFFFFFFFFF
        return ReachResult(invariant, bool(value), r.states, r.edges, r.self_edges, r.targets, r.can_reach,
                           r.cannot_reach, None if none else r.first_cannot, None if none else r.first_cannot_level,
                           r.max_distance, None if r.init_distance < 0 else r.init_distance, r.rounds, r.seconds,
                           r.csr_seconds, dist)

    def _kept_states(self) -> int:
        # the kept graph's states: the imported graph's, else every state found so far (also at an error stop)
        n = getattr(self, "_g_import_n", None)
        return n if n is not None else self.result().distinct

    def graph_reach_levels(self) -> List[Tuple[int, int]]:
        """The last graph_reach()'s (can, cannot) per BFS level ([0]: Init's level)."""
        cap = 4096
        can, cannot, n = (ctypes.c_uint64 * cap)(), (ctypes.c_uint64 * cap)(), ctypes.c_uint32()
        self._check(self.lib.rmc_graph_reach_levels(self.h, can, cannot, cap, ctypes.byref(n)))
        return list(zip(can[:n.value], cannot[:n.value]))

    def graph_shape(self) -> dict:
        """Counts and degrees of the kept graph (include/rmc.h rmc_graph_shape) as a dict; in_hist / out_hist
        are lists of 64 (the last bin: 63 or more)."""
        g = _GraphShape()
        self._check(self.lib.rmc_graph_shape(self.h, ctypes.byref(g)))
        out = {k: getattr(g, k) for k in ("states", "edges", "self_edges", "back_edges", "sinks", "max_in", "max_out",
                                           "cyclic_states")}
        out["in_hist"], out["out_hist"] = list(g.in_hist), list(g.out_hist)
        return out

    def graph_inv_values(self):
        """numpy u16 per state of the kept graph: bit b = invariant INVARIANT_BY_BIT[b] is TRUE, bit 8 + b = it
        raised the evaluation error."""
        import numpy as np
        out = np.empty(self._kept_states(), dtype=np.uint16)
        self._check(self.lib.rmc_graph_inv_values(self.h, out.ctypes.data, out.size))
        return out

    def graph_import(self, n_states: int, src, dst, inv_values) -> None:
        """A graph from arrays in place of a run's kept graph (test hook; include/rmc.h rmc_graph_import)."""
        import numpy as np
        s = np.ascontiguousarray(src, dtype=np.uint32)
        d = np.ascontiguousarray(dst, dtype=np.uint32)
        v = np.ascontiguousarray(inv_values, dtype=np.uint16)
        if s.shape != d.shape or s.ndim != 1 or v.shape != (n_states,):
            raise RmcError("RMC_E_ARG: graph_import: src / dst of one length, inv_values of n_states entries")
        self._check(self.lib.rmc_graph_import(self.h, n_states, s.size, s.ctypes.data if s.size else None,
                                              d.ctypes.data if d.size else None, v.ctypes.data))
        self._g_import_n = n_states

    # ---- liveness over the kept state graph (include/rmc.h rmc_graph_eventually) ----
    def graph_eventually(self, invariant: str, value: bool = True, source: Optional[str] = None,
                         source_value: bool = True, want_within: bool = False) -> LiveResult:
        """Which states must reach a state on which `invariant` is `value` on every fair behaviour (a maximal path,
        self-edges ignored), and which can avoid it forever: an attractor on the device over the kept graph.  With
        `source`, the leads-to `source = source_value ~> invariant = value`: it fails iff source_avoiders > 0."""
        import numpy as np
        if not hasattr(self.lib, "rmc_graph_eventually"):
            raise RmcError("this librmc.so has no liveness queries (rmc_graph_eventually): rebuild it")
        q = _LiveQuery(self._inv_bit(invariant), 1 if value else 0, -1 if source is None else self._inv_bit(source),
                       1 if source_value else 0)
        r = _LiveResult()
        within = np.empty(self._kept_states(), dtype=np.uint32) if want_within else None
        self._check(self.lib.rmc_graph_eventually(self.h, ctypes.byref(q), ctypes.byref(r),
                                                  within.ctypes.data if within is not None else None))
        ones = 0xFFFFFFFFFFFFFFFF
        none, snone, src = r.first_avoid == ones, r.first_source_avoid == ones, source is not None
        return LiveResult(invariant, bool(value), source, bool(source_value) if src else None, r.states, r.edges,
                          r.self_edges, r.targets, r.must, r.avoiders, r.avoid_terminal,
                          None if none else r.first_avoid, None if none else r.first_avoid_level, r.max_within,
                          None if r.init_within < 0 else r.init_within, r.sources if src else None,
                          r.source_avoiders if src else None, None if snone or not src else r.first_source_avoid,
                          None if snone or not src else r.first_source_avoid_level, r.rounds, r.seconds, r.csr_seconds,
                          within)

    def graph_eventually_levels(self) -> List[Tuple[int, int]]:
        """The last graph_eventually()'s (must, avoid) per BFS level ([0]: Init's level)."""
        cap = 4096
        must, avoid, n = (ctypes.c_uint64 * cap)(), (ctypes.c_uint64 * cap)(), ctypes.c_uint32()
        self._check(self.lib.rmc_graph_eventually_levels(self.h, must, avoid, cap, ctypes.byref(n)))
        return list(zip(must[:n.value], avoid[:n.value]))

    def graph_avoid_path(self, gid: int) -> Tuple[List[int], Optional[int]]:
        """The counterexample from an avoider of the last graph_eventually(): (gids, loop_at) -- gids[0] = gid, each
        next one the smallest successor that is an avoider; loop_at = the index on the path the last state steps back
        to (a lasso), or None when the walk ends in a state with no step out."""
        cap = 1024
        while True:
            gids, n, at = (ctypes.c_uint64 * cap)(), ctypes.c_uint32(), ctypes.c_int32()
            rc = self.lib.rmc_graph_avoid_path(self.h, gid, gids, cap, ctypes.byref(n), ctypes.byref(at))
            if rc < 0 and n.value > cap:  # (the walk is longer than the buffer: its length came back)
                cap = n.value
                continue
            self._check(rc)
            return list(gids[:n.value]), None if at.value < 0 else at.value

    def graph_scc(self, want_comp: bool = False) -> SccResult:
        """The strongly connected components of the kept graph, self-edges ignored (include/rmc.h rmc_graph_scc)."""
        import numpy as np
        if not hasattr(self.lib, "rmc_graph_scc"):
            raise RmcError("this librmc.so has no liveness queries (rmc_graph_scc): rebuild it")
        r = _SccResult()
        comp = np.empty(self._kept_states(), dtype=np.uint32) if want_comp else None
        self._check(self.lib.rmc_graph_scc(self.h, ctypes.byref(r), comp.ctypes.data if comp is not None else None))
        return SccResult(r.components, r.nontrivial, r.nontrivial_states, r.largest, r.trimmed, r.rounds, r.seconds,
                         r.csr_seconds, comp)

    def trace(self) -> List[Tuple[Optional[Tuple[int, int, int]], dict]]:
        n = ctypes.c_uint32()
        self._check(self.lib.rmc_trace_len(self.h, ctypes.byref(n)))
        cap = unpacked_len(self.cfg.n_servers, self.cfg.n_vals, 256)
        buf = (ctypes.c_int32 * cap)()
        out = []
        for i in range(n.value):
            a, s, w = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
            k = self._check(self.lib.rmc_trace_state(self.h, i, buf, cap, ctypes.byref(a), ctypes.byref(s),
                                                     ctypes.byref(w)))
            st = unpacked_to_state(list(buf[:k]), self.cfg.n_servers, self.cfg.n_vals)
            out.append((None if a.value < 0 else (s.value, a.value, w.value), st))
        return out

    # ---- single-state hooks ------------------------------------------------------------
    def _unpacked(self, state: dict):
        u = state_to_unpacked(state, self.cfg.n_servers, self.cfg.n_vals)
        return (ctypes.c_int32 * len(u))(*u)

    def successors(self, state: dict, cap: int = 512):
        """[(key(server, action, witness), successor_state, fp128)] in TLC order; raises on Assert."""
        n, V = self.cfg.n_servers, self.cfg.n_vals
        stride = unpacked_len(n, V, 256)
        out = (ctypes.c_int32 * (stride * cap))()
        keys = (ctypes.c_uint32 * cap)()
        fps = (ctypes.c_uint64 * (2 * cap))()
        cnt = ctypes.c_uint32()
        rc = self._check(self.lib.rmc_successors(self.h, self._unpacked(state), out, stride, cap, keys, fps,
                                                 ctypes.byref(cnt)))
        if rc == RMC_ASSERT:
            raise AssertionError("split brain")
        res = []
        for i in range(cnt.value):
            k = keys[i]
            st = unpacked_to_state(list(out[i * stride:(i + 1) * stride]), n, V)
            res.append(((k >> 24, (k >> 16) & 0xFF, k & 0xFFFF), st, (fps[2 * i], fps[2 * i + 1])))
        return res

    def fingerprint(self, state: dict) -> Tuple[int, int]:
        fp = (ctypes.c_uint64 * 2)()
        self._check(self.lib.rmc_fingerprint(self.h, self._unpacked(state), fp))
        return fp[0], fp[1]

    # ---- checks of a finished run's deep levels (tests/test_gpu_deep.py) -----------------
    def state_path(self, gid: int):
        """(keys, gids): how each state on the path from Init to the explored state `gid` was reached
        ((server, action, witness) per step) and the global ids of the path's states (Init's 0 first)."""
        cap = 4096
        keys, gids, n = (ctypes.c_uint32 * cap)(), (ctypes.c_uint64 * cap)(), ctypes.c_uint32()
        self._check(self.lib.rmc_state_path(self.h, gid, keys, gids, cap, ctypes.byref(n)))
        return ([(k >> 24, (k >> 16) & 0xFF, k & 0xFFFF) for k in keys[1:n.value]], list(gids[:n.value]))

    def fingerprints_unpacked(self, unpacked, stride: int, n: int):
        """Fingerprints of n unpacked states (a contiguous int32 buffer, `stride` ints apart), one launch."""
        fps = (ctypes.c_uint64 * (2 * max(n, 1)))()
        buf = ctypes.cast(unpacked.ctypes.data if hasattr(unpacked, "ctypes") else unpacked,
                          ctypes.POINTER(ctypes.c_int32))
        self._check(self.lib.rmc_fingerprints(self.h, buf, stride, n, fps))
        return [(fps[2 * i], fps[2 * i + 1]) for i in range(n)]

    def fingerprints_array(self, unpacked):
        """fingerprints_unpacked for a C-contiguous int32 numpy array of shape (n, stride), as a (n, 2) uint64
        array (no Python object per state: millions of states a call)."""
        import numpy as np
        n, stride = unpacked.shape
        assert unpacked.dtype == np.int32 and unpacked.flags["C_CONTIGUOUS"]
        fps = np.empty((max(n, 1), 2), dtype=np.uint64)
        self._check(self.lib.rmc_fingerprints(self.h, unpacked.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), stride, n,
                                              fps.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return fps[:n]

    def seen_contains(self, fps: Sequence[Tuple[int, int]]) -> List[bool]:
        """Membership of each fingerprint in the seen set (TLC's FPSet)."""
        n = len(fps)
        arr = (ctypes.c_uint64 * (2 * max(n, 1)))(*[w for f in fps for w in f])
        out = (ctypes.c_uint8 * max(n, 1))()
        self._check(self.lib.rmc_seen_contains(self.h, arr, n, out))
        return [bool(out[i]) for i in range(n)]

    def eval_invariant(self, state: dict, name: str) -> Optional[bool]:
        """True / False, or None for a TLC evaluation error."""
        bit = INVARIANT_BY_BIT.index("Inv" if name == "LeaderHasAllCommittedEntries" else name)
        v = ctypes.c_int32()
        rc = self.lib.rmc_eval_invariant(self.h, self._unpacked(state), bit, ctypes.byref(v))
        if rc == RMC_EVAL_ERROR:
            return None
        self._check(rc)
        return bool(v.value)
