"""asr_ngram_logp (csrc/ngram.hip, the query of csrc/ngram.h) against NgramLM.logp (utils/ngram.py): the same float32 adds in the same
order, so the results are held to the host's bits."""
import numpy as np
import pytest
import torch

import ctc_beam_lm_reference as M

pytestmark = pytest.mark.gpu

V_SEEN, V = 12, 14            # the corpus uses the ids 1..11: 12 and 13 are never seen and have only their smoothed unigram


def _lm(order):
    from utils.ngram import NgramLM
    return NgramLM.estimate(M.synthetic_corpus(V_SEEN, 11, 300), V, order, M.BOS, M.EOS)


def _queries(lm, n, seed):
    """Contexts drawn half from the stored n-grams (full hits and shallow backoffs) and half at random with -1 and unseen ids among
    them (deep backoffs), symbols from 0..V+1 (V and V + 1: no id of the table)."""
    rng = np.random.default_rng(seed)
    width = lm.order - 1
    grams = [[((int(k) >> (16 * j)) & 0xffff) - 1 for j in range(3, -1, -1) if (int(k) >> (16 * j)) & 0xffff] for k in lm.keys]
    ctx = rng.integers(-1, V, size=(n, max(width, 1))).astype(np.int32)[:, :width]
    sym = rng.integers(0, V + 2, size=n).astype(np.int32)
    for i in range(0, n, 2):
        g = grams[int(rng.integers(len(grams)))]
        if width:
            h = ([-1] * width + g[:-1])[-width:] if rng.integers(2) else ([-1] * width + g)[-width:]
            ctx[i] = h
        if rng.integers(4):
            sym[i] = g[-1]
    return np.ascontiguousarray(ctx), sym


def _depth(lm, h, c):
    """How many symbols of context the answer used (-1: no unigram)."""
    key = lm.context(h)
    m = 0
    while m < lm.order - 1 and (key >> (16 * m)) & 0xffff:
        m += 1
    for m in range(m, 0, -1):
        if ((key & ((1 << (16 * m)) - 1)) << 16 | (c + 1)) in lm._map:
            return m
    return 0 if (c + 1) in lm._map and c < V else -1


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_queries_equal_the_host_bits(order):
    """500 queries per order (2000 in all): full hits, every backoff depth, contexts with -1, symbols never seen and symbols outside the
    table (-inf).  torch.equal to NgramLM.logp; the output lies inside a buffer of sentinels that stay untouched."""
    from asr_hip import lib as L
    lm = _lm(order)
    n = 500
    ctx, sym = _queries(lm, n, 100 + order)
    want = np.array([lm.logp(ctx[i].tolist(), int(sym[i])) for i in range(n)], dtype=np.float32)
    depth = np.array([_depth(lm, ctx[i].tolist(), int(sym[i])) for i in range(n)])
    for d in range(-1, order):
        assert int((depth == d).sum()) >= 5, (order, d, np.bincount(depth + 1))
    assert int((ctx == -1).any(axis=1).sum()) >= (20 if order > 1 else 0) and int((sym >= V_SEEN).sum()) >= 20
    assert np.array_equal(np.isneginf(want), depth < 0)
    dev = torch.device("cuda")
    t = lm.device_table(dev)
    assert lm.device_table(dev) is t                                     # built once
    buf = torch.full((n + 64,), 123.0, device=dev)
    c, s = torch.from_numpy(ctx).to(dev), torch.from_numpy(sym).to(dev)
    L.call("asr_ngram_logp", L.ptr(t["keys"]), L.ptr(t["vals"]), t["capacity"], t["max_probe"], order, L.ptr(c) if order > 1 else None,
           L.ptr(s), n, L.ptr(buf[32:]), L.stream())
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.all(got[:32] == 123.0) and torch.all(got[32 + n:] == 123.0)
    assert torch.equal(got[32:32 + n], torch.from_numpy(want)), (order, np.flatnonzero(got[32:32 + n].numpy() != want)[:8])
    from asr_hip import ops
    assert torch.equal(ops.ngram_logp(t, c, s).cpu(), torch.from_numpy(want))


def test_refusals_and_no_queries():
    from asr_hip import lib as L
    from asr_hip import ops
    dev = torch.device("cuda")
    lm = _lm(3)
    t = lm.device_table(dev)
    c, s, out = torch.zeros((4, 2), dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, device=dev)

    def call(capacity, max_probe, order, n=4):
        L.call("asr_ngram_logp", L.ptr(t["keys"]), L.ptr(t["vals"]), capacity, max_probe, order, L.ptr(c), L.ptr(s), n, L.ptr(out),
               L.stream())
    for capacity, max_probe, order in ((t["capacity"] - 1, t["max_probe"], 3), (0, t["max_probe"], 3), (t["capacity"], t["max_probe"], 0),
                                       (t["capacity"], t["max_probe"], 5), (t["capacity"], 0, 3)):
        with pytest.raises(L.AsrHipError):
            call(capacity, max_probe, order)
    with pytest.raises(L.AsrHipError):
        call(t["capacity"], t["max_probe"], 3, n=-1)
    call(t["capacity"], t["max_probe"], 3, n=0)
    with pytest.raises(L.AsrHipError):
        ops.ngram_logp(lm.device_table(torch.device("cpu")), c.cpu(), s.cpu())      # host tensors
    assert ops.ngram_logp(t, c[:0], s[:0]).numel() == 0
