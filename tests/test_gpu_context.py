"""asr_ctx_step (csrc/context.hip, the step of csrc/context.h) against ContextGraph.step (utils/context.py): integers, so the results
are held to the host's exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 14


def _graph(seed=31):
    """Forty random phrases of one to five labels over the labels 3..11 (12 and 13 open no phrase): shared prefixes, shared suffixes and
    phrases inside phrases all occur."""
    from utils.context import ContextGraph
    rng = np.random.default_rng(seed)
    return ContextGraph.from_phrases([rng.integers(3, 12, size=int(rng.integers(1, 6))).tolist() for _ in range(40)], V)


def _kind(graph, stored, s, c):
    from utils.context import pack
    if not 0 <= c <= 65534:
        return "outside"
    if pack(s, c) in stored:
        return "hit"
    return "eps" if pack(0, c) in stored else "miss"


def test_steps_equal_the_host():
    """2000 (state, symbol) pairs: stored transitions, fall-throughs to (eps, c), misses to eps and symbols outside 0..65534 (to eps,
    -hold).  torch.equal to ContextGraph.step; the outputs lie inside buffers of sentinels that stay untouched."""
    from asr_hip import lib as L
    from asr_hip import ops
    graph = _graph()
    rng = np.random.default_rng(32)
    n = 2000
    state = rng.integers(0, graph.states, size=n).astype(np.int32)
    sym = rng.integers(0, V, size=n).astype(np.int32)
    stored = set(graph.transitions()[0].tolist())
    keys = sorted(stored)
    for i in range(0, n, 2):                                   # every other pair is a stored transition
        k = keys[int(rng.integers(len(keys)))]
        state[i], sym[i] = (k >> 16) - 1, (k & 0xffff) - 1
    sym[1:400:8] = rng.choice([-1, -7, 65535, 65536, 1 << 30], size=len(sym[1:400:8]))
    want = np.array([graph.step(int(s), int(c)) if 0 <= c <= 65534 else (0, -int(graph.hold[s])) for s, c in zip(state, sym)],
                    dtype=np.int32)
    kinds = [_kind(graph, stored, int(s), int(c)) for s, c in zip(state, sym)]
    for kind in ("hit", "eps", "miss", "outside"):
        assert kinds.count(kind) >= 40, (kind, kinds.count(kind))
    assert sum(1 for k, s in zip(kinds, state) if k != "hit" and graph.hold[s] > 0) >= 100       # something is given back
    dev = torch.device("cuda")
    t = graph.device_table(dev)
    assert graph.device_table(dev) is t                                              # built once
    nxt, delta = torch.full((n + 64,), -77, dtype=torch.int32, device=dev), torch.full((n + 64,), -88, dtype=torch.int32, device=dev)
    s, c = torch.from_numpy(state).to(dev), torch.from_numpy(sym).to(dev)
    L.call("asr_ctx_step", L.ptr(t["keys"]), L.ptr(t["vals"]), t["capacity"], t["max_probe"], L.ptr(t["hold"]), t["states"], L.ptr(s),
           L.ptr(c), n, L.ptr(nxt[32:]), L.ptr(delta[32:]), L.stream())
    torch.cuda.synchronize()
    nxt, delta = nxt.cpu(), delta.cpu()
    for buf, fill in ((nxt, -77), (delta, -88)):
        assert torch.all(buf[:32] == fill) and torch.all(buf[32 + n:] == fill)
    assert torch.equal(nxt[32:32 + n], torch.from_numpy(want[:, 0].copy())), np.flatnonzero(nxt[32:32 + n].numpy() != want[:, 0])[:8]
    assert torch.equal(delta[32:32 + n], torch.from_numpy(want[:, 1].copy())), np.flatnonzero(delta[32:32 + n].numpy() != want[:, 1])[:8]
    a, b = ops.context_step(t, s, c)
    assert torch.equal(a.cpu(), nxt[32:32 + n]) and torch.equal(b.cpu(), delta[32:32 + n])
    # a state outside the table is taken for eps
    a, b = ops.context_step(t, torch.tensor([graph.states, -1, 1 << 30], dtype=torch.int32, device=dev),
                            torch.tensor([sym[0]] * 3, dtype=torch.int32, device=dev))
    assert a.tolist() == [graph.step(0, int(sym[0]))[0]] * 3 and b.tolist() == [graph.step(0, int(sym[0]))[1]] * 3


def test_refusals_and_no_steps():
    from asr_hip import lib as L
    from asr_hip import ops
    dev = torch.device("cuda")
    graph = _graph()
    t = graph.device_table(dev)
    s, c = torch.zeros(4, dtype=torch.int32, device=dev), torch.full((4,), 3, dtype=torch.int32, device=dev)
    nxt, delta = torch.full((4,), -77, dtype=torch.int32, device=dev), torch.full((4,), -88, dtype=torch.int32, device=dev)
    good = dict(keys=L.ptr(t["keys"]), vals=L.ptr(t["vals"]), capacity=t["capacity"], max_probe=t["max_probe"], hold=L.ptr(t["hold"]),
                states=t["states"], state=L.ptr(s), sym=L.ptr(c), n=4, next=L.ptr(nxt), delta=L.ptr(delta))

    def call(**over):
        L.call("asr_ctx_step", *dict(good, **over).values(), L.stream())
    for over in (dict(capacity=t["capacity"] - 1), dict(capacity=0), dict(max_probe=0), dict(states=0), dict(n=-1), dict(keys=None),
                 dict(vals=None), dict(hold=None), dict(state=None), dict(sym=None), dict(next=None), dict(delta=None)):
        with pytest.raises(L.AsrHipError):
            call(**over)
    call(n=0)                                                                        # a no-op: nothing is written
    torch.cuda.synchronize()
    assert torch.all(nxt == -77) and torch.all(delta == -88)
    call()
    assert nxt.tolist() == [graph.step(0, 3)[0]] * 4 and delta.tolist() == [graph.step(0, 3)[1]] * 4
    with pytest.raises(L.AsrHipError):
        ops.context_step(graph.device_table(torch.device("cpu")), s.cpu(), c.cpu())      # host tensors
    a, b = ops.context_step(t, s[:0], c[:0])
    assert a.numel() == 0 and b.numel() == 0
