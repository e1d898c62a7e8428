"""What raftmc -dump FILE and -dump dot FILE write, rendered by the tests from fixture states and edges
(test helper), independently of the launcher's sink (tla-raft_amd/launcher/raftmc.cpp).  States are printed as
in a counterexample (tests/tla_render.py; a msgs set of several records continues on lines indented by three
blanks); a dot label is that text with backslashes and quotes escaped and newlines as \\n."""
import hashlib

import numpy as np

from tla_render import render_state

ACTIONS = ("BecomeCandidate", "UpdateTerm", "ResponseVote", "BecomeLeader", "ClientReq", "LeaderAppendEntry",
           "FollowerAcceptEntry", "FollowerRejectEntry", "HandleAppendResp", "LeaderCanCommit", "Restart",
           "FollowerAppendEntry", "BecomeFollower")
EDGE_DTYPE = np.dtype([("src", "<u8"), ("key", "<u4"), ("dst", "<u8")])  # packed: 20 bytes


def state_text(st, servers, vals):
    lines = render_state(st, servers, vals)
    return "\n".join(l.replace("], [", "],\n   [") if l.startswith("/\\ msgs") else l for l in lines) + "\n"


def dump_text(states, servers, vals):
    return "".join(f"State {i + 1}:\n{state_text(st, servers, vals)}\n" for i, st in enumerate(states))


def dot_label(st, servers, vals):
    return state_text(st, servers, vals)[:-1].replace("\\", "\\\\").replace('"', '\\"').replace("\n", "\\n")


def dot_text(states, edges, servers, vals, actionlabels):
    out = ["strict digraph DiskGraph {", "nodesep=0.35;", "subgraph cluster_graph {", 'color="white";']
    for i, st in enumerate(states):
        out.append(f'{i + 1} [label="{dot_label(st, servers, vals)}"{",style = filled" if i == 0 else ""}]')
    for src, key, dst in edges:
        name = ACTIONS[(key >> 16) & 0xFF] if actionlabels else ""
        out.append(f'{src + 1} -> {dst + 1} [label="{name}",color="black",fontcolor="black"];')
    return "\n".join(out + ["}", "}"]) + "\n"


class StatesDigest:
    """The fixture's state digest -- sha256 over json.dumps(unpacked_to_state(row), sort_keys=True) + "\\n" per
    state in gid order -- of a run of any size, fed the states callback's pieces as they arrive (nothing is kept).
    A state's line is put together from its twelve variables' texts, each taken from json.dumps of that variable
    of unpacked_to_state(row) the first time its ints are met and from a table afterwards (a message's text
    likewise), so the text is json.dumps' own; `lines` (kept when keep=True) lets a test compare them one by one
    with the plain rendering.  sample_hexdigest(): the same over the states with gid % 64 == 0."""
    KEYS = ("commitIndex", "currentTerm", "electionCount", "logs", "matchIndex", "msgs", "nextIndex",
            "pendingResponse", "restartCount", "role", "valSent", "votedFor")  # sorted

    def __init__(self, n, V, keep=False):
        import raftmc
        self._unpack = lambda row: raftmc.unpacked_to_state(row, n, V)
        self.h, self.hs, self.count, self.lines = hashlib.sha256(), hashlib.sha256(), 0, [] if keep else None
        o, spans = 0, {}
        for name, k in (("votedFor", n), ("currentTerm", n), ("role", n), ("commitIndex", n),
                        ("logs", n + 2 * n * (V + 1)), ("matchIndex", n * n), ("nextIndex", n * n),
                        ("pendingResponse", n * n), ("electionCount", 1), ("restartCount", 1), ("valSent", V)):
            spans[name] = (4 * o, 4 * (o + k))  # byte span of the ints that decide the variable
            o += k
        self.nm_col, self.msg0 = o, 4 * (o + 1)
        self.spans = [(name, spans[name]) for name in self.KEYS if name != "msgs"]
        self.cache = {name: {} for name in spans}
        self.mcache, self.scache = {}, {}

    def update(self, gid0, a):
        import json
        assert gid0 == self.count  # ascending, no gap
        buf, stride, nms = a.tobytes(), 4 * a.shape[1], a[:, self.nm_col].tolist()
        for i, nm in enumerate(nms):
            base, d = i * stride, None
            parts = {}
            for name, (b0, b1) in self.spans:
                k = buf[base + b0:base + b1]
                t = self.cache[name].get(k)
                if t is None:
                    d = d or self._unpack(a[i].tolist())
                    t = self.cache[name][k] = f'"{name}": ' + json.dumps(d[name], sort_keys=True)
                parts[name] = t
            mk = buf[base + self.msg0:base + self.msg0 + 32 * nm]  # the whole set first, then message by message
            mt = self.scache.get(mk)
            if mt is None:
                ms = []
                for j in range(nm):
                    k = mk[32 * j:32 * (j + 1)]
                    t = self.mcache.get(k)
                    if t is None:
                        d = d or self._unpack(a[i].tolist())
                        t = self.mcache[k] = json.dumps(d["msgs"][j], sort_keys=True)
                    ms.append(t)
                mt = self.scache[mk] = '"msgs": [' + ", ".join(ms) + "]"
            parts["msgs"] = mt
            line = ("{" + ", ".join(parts[name] for name in self.KEYS) + "}\n").encode()
            self.h.update(line)
            if (gid0 + i) % 64 == 0:
                self.hs.update(line)
            if self.lines is not None:
                self.lines.append(line)
        self.count += len(nms)

    def hexdigest(self):
        return self.h.hexdigest()

    def sample_hexdigest(self):
        return self.hs.hexdigest()


def edges_sha256(src, key, dst):
    """The fixture's edge digest: (u64 src, u32 key, u64 dst) little-endian, packed, in order."""
    a = np.empty(len(src), dtype=EDGE_DTYPE)
    a["src"], a["key"], a["dst"] = src, key, dst
    return hashlib.sha256(a.tobytes()).hexdigest()
