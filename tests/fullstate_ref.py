"""The whole state as the identity (ModelConfig(view=False), rmc_set_full_state), on the CPU.

oracle/raft_ref.py identifies a state by `canonical`: the orbit minimum of the VIEW (Raft.tla:38), and
with Config(view=False) the whole state, but only without SYMMETRY.  This module wraps it: `canonical`
here is the whole state -- the view's eight variables plus electionCount, restartCount, pendingResponse
and valSent -- and under SYMMETRY its minimum over the server permutations, pendingResponse permuted
on both indices, values left alone (Raft.cfg:28 is commented out).  `bfs` is raft_ref.bfs itself, run
with that identity; with view=True everything is raft_ref's own."""
import contextlib
import itertools

import raft_ref as R


def permute_state(st: R.State, pi) -> R.State:
    """The concrete state with server k renamed pi[k], hidden variables included."""
    n = len(pi)
    pv = R.permute_view(st.view(), pi)
    inv = [0] * n
    for a in range(n):
        inv[pi[a]] = a
    return R.State(votedFor=pv[0], currentTerm=pv[1], logs=pv[2], matchIndex=pv[3], nextIndex=pv[4],
                   commitIndex=pv[5], msgs=frozenset(pv[6]), role=pv[7], electionCount=st.electionCount,
                   restartCount=st.restartCount,
                   pendingResponse=tuple(tuple(st.pendingResponse[inv[a]][inv[b]] for b in range(n))
                                         for a in range(n)),
                   valSent=st.valSent)


def whole(st: R.State):
    return st.view() + (st.electionCount, st.restartCount, st.pendingResponse, st.valSent)


def canonical(cfg: R.Config, st: R.State):
    """A state's identity under cfg: raft_ref's for the VIEW; else the whole state, minimised over the
    server permutations under SYMMETRY."""
    if cfg.view:
        return R.canonical(cfg, st)
    if not cfg.symmetry:
        return whole(st)
    n = cfg.n
    best = None
    for pi in itertools.permutations(range(n)):
        inv = [0] * n
        for a in range(n):
            inv[pi[a]] = a
        c = R.permute_view(st.view(), pi) + (
            st.electionCount, st.restartCount,
            tuple(tuple(st.pendingResponse[inv[a]][inv[b]] for b in range(n)) for a in range(n)), st.valSent)
        if best is None or c < best:
            best = c
    return best


@contextlib.contextmanager
def _identity():
    saved = R.canonical
    R.canonical = canonical
    try:
        yield
    finally:
        R.canonical = saved


def bfs(cfg: R.Config, **kw) -> R.Result:
    """raft_ref.bfs (TLC's order, first discovery wins) with this module's identity."""
    with _identity():
        return R.bfs(cfg, **kw)


def view_classes(cfg: R.Config, states) -> int:
    """How many VIEW classes (under cfg's SYMMETRY setting) the given states fall into."""
    vcfg = R.Config(**{**cfg.__dict__, "view": True})
    return len({R.canonical(vcfg, st) for st in states})


def hidden_copies(st: R.State):
    """Copies of st with exactly one hidden component changed: every pendingResponse[i][j] (i != j), one
    diagonal bit, electionCount and restartCount one up and one down (inside the ranges below), one valSent.
    [(label, state)]; the copies are pairwise different whole states."""
    n = len(st.votedFor)
    out = []
    flip = lambda i, j: tuple(tuple((not x) if (a, b) == (i, j) else x for b, x in enumerate(row))
                              for a, row in enumerate(st.pendingResponse))
    rep = lambda **kw: R.State(**{**st.__dict__, **kw})
    for i in range(n):
        for j in range(n):
            if i != j:
                out.append((f"pend[{i}][{j}]", rep(pendingResponse=flip(i, j))))
    d = st.electionCount % n
    out.append((f"pend[{d}][{d}]", rep(pendingResponse=flip(d, d))))
    # (the ranges the unpacked layout takes, include/rmc.h: electionCount 0..7, restartCount 0..15)
    for name, cur, top in (("electionCount", st.electionCount, 7), ("restartCount", st.restartCount, 15)):
        for delta in (1, -1):
            if 0 <= cur + delta <= top:
                out.append((f"{name}{delta:+d}", rep(**{name: cur + delta})))
    if st.valSent:
        v = st.restartCount % len(st.valSent)
        vs = tuple((0 if x == R.NONE else R.NONE) if k == v else x for k, x in enumerate(st.valSent))
        out.append((f"valSent[{v}]", rep(valSent=vs)))
    return out
