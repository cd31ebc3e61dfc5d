"""asr_rnnt_beam_search_lm / asr_rnnt_beam_search_ctx, the fused arms of the transducer beam search (csrc/rnnt_beam.hip), against the
float64 restatement tests/rnnt_beam_fused_reference.py (pinned on the CPU by tests/test_rnnt_beam_fused_host.py).

V 37 (the last 16-column tile of the MFMA arm is masked), B 3 with T_b = (6, 0, 2) of T 6, exact data (rnnt_beam_reference.exact_case:
the logits are the same bits in every arm and in the restatement).  The grid covers the three dtype / projection arms -- bf16 J 32 (MFMA),
bf16 J 40 (plain), fp32 J 24 -- with W in {1, 3, 16}, K in {1, 4, 16}, S in {1, 3}, a predictor context of 1 and 2 labels, n-gram orders
1, 2 and 4 (4 outlasts the predictor's context), the LM alone, the phrases alone and both; one more case fills D (W 16, S 63, T 2: 1024
entries with the fused state; Gaussian data, the restatement on the project's own logits), one runs the widest fp32 joint the fused arms' LDS admits.  Both tables are small: max_probe > 1, so some
first probes meet another key (asserted).

Weights zero: ids, lengths and scores torch.equal to asr_rnnt_beam_search's.  Weights on: every margin of the restatement's pruning and
final order, taken on the fused key, is at least 1e-3 (asserted on the CPU side; the seeds were searched on the CPU for that), so there
is ONE right answer: sequences and lengths torch.equal; scores (the acoustic log-probability) under the rule of
tests/test_gpu_rnnt_beam.py, |score - ref64| <= 4 max(|ref32 - ref64|, eps32 * the largest magnitude that entered a sum); lm and
alpha * lm + beta * len within 2e-5 * max(1, |ref|) of the restatement (the rule of tests/test_gpu_ctc_beam_lm.py); credit exactly.
Every call runs between sentinels around ids, lengths, scores, lm, credit and the workspace."""
import functools
import math

import numpy as np
import pytest
import torch

import rnnt_beam_fused_reference as F
import rnnt_beam_reference as R
from test_gpu_rnnt_beam import PAD, _tensors, cpu_rows, gpu_rows, to_gpu
from test_gpu_rnnt_beam import launch as plain_launch

pytestmark = pytest.mark.gpu

V, B, T, FRAMES = 37, 3, 6, (6, 0, 2)
F32, BF16 = torch.float32, torch.bfloat16
TOL = 2e-5
# name: (dtype, J, C, W, K, S, nbest, n-gram order (0: no LM), phrases, data seed)
GRID = {
    "bf16_j32_w3_k4_s3_o4_both": (BF16, 32, 2, 3, 4, 3, 3, 4, True, 0),
    "bf16_j32_w16_k16_s1_o2_lm": (BF16, 32, 1, 16, 16, 1, 8, 2, False, 0),
    "bf16_j40_w1_k1_s3_o1_both": (BF16, 40, 1, 1, 1, 3, 1, 1, True, 0),
    "bf16_j40_w3_k16_s1_ctx": (BF16, 40, 2, 3, 16, 1, 3, 0, True, 0),
    "f32_j24_w16_k4_s3_o2_both": (F32, 24, 2, 16, 4, 3, 16, 2, True, 2),
    "f32_j24_w3_k1_s1_o4_lm": (F32, 24, 1, 3, 1, 1, 2, 4, False, 0),
}
# D full: T 2, W 16, S 63 on Gaussian data -> (dtype, J, C, K, order, data seed); frames (2,).  K 1: with a stateless predictor the label
# steps of ONE frame are a Markov chain, and with two candidates per row sequences that share their transitions tie to the last bit (no
# seed separates 126 such steps); one candidate per row leaves 16 candidates for 16 places, and D's 1024 entries are ranked by the fused key
FULL = (BF16, 32, 2, 1, 4, 11)
# the widest fp32 joint of the fused arms: 16 z rows of 1388 floats + 33 728 bytes of state are 122 560 of the 122 880 bytes granted
WIDE_J = 1384


def case_graph(plain, seed):
    """A phrase list for a case: pieces of one to three labels cut from the plain search's second and third entries of the last D (so
    that the bonus moves hypotheses past each other), each also with its first label doubled in front (a shared suffix: failure links
    are taken) and with a random label behind it (a match that breaks off), and four random ones."""
    g = np.random.default_rng(seed)
    phrases = []
    for res in plain:
        for y, _ in res["last_d"][1:3]:
            if len(y) > 0:
                i = int(g.integers(0, len(y)))
                piece = list(y[i:i + int(g.integers(1, 4))])
                phrases += [piece, [piece[0]] + piece, piece + [int(g.integers(1, V))]]
    phrases += [g.integers(1, V, size=int(g.integers(1, 4))).tolist() for _ in range(4)]
    return F.graph_of(phrases, V)


def fused_kw(lm, graph, on=True):
    return dict(lm=lm, alpha=F.ALPHA if on and lm is not None else 0.0, beta=F.BETA if on else 0.0, bos=F.BOS, eos=F.EOS, graph=graph,
                gamma=F.GAMMA if on and graph is not None else 0.0)


def build_case(dtype, J, C, W, K, S, nbest, order, phrases, seed, frames=FRAMES, Tn=T, Vn=V, random=False, make_rows=None):
    """-> dict(Pt, rows, lm, graph, kw, r64, r32, shape): the parameters, the restatement's callbacks (they record the predictor-table
    rows asked for) and its fused results in float64 and float32.  CPU only, unless make_rows(Pt) supplies the project's own logits
    (random data: the search is compared, not the projection's rounding)."""
    Pt = _tensors((R.random_case if random else R.exact_case)(len(frames), Tn, J, Vn, C, seed), dtype)
    rows = make_rows(Pt) if make_rows else [cpu_rows(Pt, b) for b in range(len(frames))]
    plain = [R.search(rows[b], frames[b], Vn, W, K, S, nbest, C) for b in range(len(frames))]
    lm = F.synthetic_lm(Vn, order) if order else None
    graph = case_graph(plain, 100 + seed) if phrases else None
    kw = fused_kw(lm, graph)
    r64 = [F.search(rows[b], frames[b], Vn, W, K, S, nbest, C, **kw) for b in range(len(frames))]
    r32 = [F.search(rows[b], frames[b], Vn, W, K, S, nbest, C, dtype=np.float32, **kw) for b in range(len(frames))]
    return dict(Pt=Pt, rows=rows, lm=lm, graph=graph, kw=kw, r64=r64, r32=r32, plain=plain, shape=(Vn, C, W, K, S, nbest), frames=frames)


@functools.lru_cache(maxsize=None)
def grid_case(name):
    return build_case(*GRID[name])


def full_case(make_rows=None):
    dtype, J, C, K, order, seed = FULL
    return build_case(dtype, J, C, 16, K, 63, 16, order, True, seed, frames=(2,), Tn=2, random=True, make_rows=make_rows)


def launch(Pg, frames, W, K, S, nbest, lm=None, graph=None, alpha=0.0, beta=0.0, gamma=0.0, bos=F.BOS, eos=F.EOS, blank=0, sos=1,
           over=None):
    """One call of asr_rnnt_beam_search_lm (graph None) or asr_rnnt_beam_search_ctx between sentinels -> (dict of CPU tensors, return
    code).  over: table entries replaced for the refusal tests."""
    from asr_hip import lib as L
    e = Pg["e"]
    Bn, Tn, J = e.shape
    Vn = Pg["w_out"].shape[0]
    dev = e.device
    n = L.load().asr_rnnt_beam_workspace(Bn, Tn, Vn, W, K, S)
    cols = Tn * S

    def guarded(numel, dtype, fill):
        buf = torch.full((numel + 2 * PAD,), fill, device=dev, dtype=dtype)
        return buf, buf[PAD:PAD + numel]
    ws_all, ws = guarded(max(n, 4), torch.float32, -77.0)
    ids_all, ids = guarded(Bn * nbest * cols, torch.int32, -7)
    len_all, lens = guarded(Bn * nbest, torch.int32, -7)
    sc_all, sc = guarded(Bn * nbest, torch.float32, -77.0)
    lm_all, lmv = guarded(Bn * nbest, torch.float32, -77.0)
    cr_all, cr = guarded(Bn * nbest, torch.int32, -7)
    fl = torch.tensor(list(frames), dtype=torch.int32, device=dev)
    tabs = Pg["tables"]
    head = (L.ptr(e), L.ptr(tabs[0]), L.ptr(tabs[1]) if len(tabs) == 2 else None, L.ptr(Pg["w_out"]), L.ptr(Pg["b_out"]), L.ptr(fl), Bn, Tn,
            J, Vn, W, K, S, nbest, blank, sos, L.dt(e), L.ptr(ws), n, L.ptr(ids), L.ptr(lens), L.ptr(sc))
    t = dict(lm.device_table(dev)) if lm is not None else dict(keys=None, vals=None, capacity=0, max_probe=0, order=0)
    t.update({k[3:]: v for k, v in (over or {}).items() if k.startswith("ng_")})
    if graph is None:
        rc = L.load().asr_rnnt_beam_search_lm(*head, L.ptr(t["keys"]), L.ptr(t["vals"]), t["capacity"], t["max_probe"], t["order"], bos, eos,
                                              alpha, beta, L.ptr(lmv) if (over or {}).get("lm", 1) else None, L.stream())
    else:
        c = dict(graph.device_table(dev))
        c.update({k[3:]: v for k, v in (over or {}).items() if k.startswith("cx_")})
        rc = L.load().asr_rnnt_beam_search_ctx(*head, L.ptr(t["keys"]), L.ptr(t["vals"]), t["capacity"], t["max_probe"], t["order"], bos, eos,
                                               alpha, beta, L.ptr(c["keys"]), L.ptr(c["vals"]), c["capacity"], c["max_probe"],
                                               L.ptr(c["hold"]), c["states"], gamma, L.ptr(lmv) if (over or {}).get("lm", 1) else None,
                                               L.ptr(cr) if (over or {}).get("credit", 1) else None, L.stream())
    torch.cuda.synchronize()
    for buf, fill in ((ws_all, -77.0), (ids_all, -7), (len_all, -7), (sc_all, -77.0), (lm_all, -77.0), (cr_all, -7)):
        assert bool((buf[:PAD] == fill).all()) and bool((buf[-PAD:] == fill).all()), "a sentinel was overwritten"
    if graph is None:
        assert bool((cr_all == -7).all()), "the LM arm wrote a credit"
    out = dict(ids=ids.view(Bn, nbest, cols).cpu(), lengths=lens.view(Bn, nbest).cpu(), scores=sc.view(Bn, nbest).cpu(),
               lm=lmv.view(Bn, nbest).cpu())
    if graph is not None:
        out["credit"] = cr.view(Bn, nbest).cpu()
    return out, rc


def run(case, Pg=None, frames=None, on=True):
    Vn, C, W, K, S, nbest = case["shape"]
    kw = case["kw"] if on else fused_kw(case["lm"], case["graph"], False)
    return launch(Pg if Pg is not None else to_gpu(case["Pt"]), frames if frames is not None else case["frames"], W, K, S, nbest,
                  lm=kw["lm"], graph=kw["graph"], alpha=kw["alpha"], beta=kw["beta"], gamma=kw["gamma"])


def assert_margins(case, what):
    for b, res in enumerate(case["r64"]):
        assert F.min_margin(res) >= F.MARGIN, (what, b, res["margins"])


def compare(got, case, what):
    """The rules of the module docstring -> the worst score error over its bound."""
    r64, r32, kw = case["r64"], case["r32"], case["kw"]
    assert_margins(case, what)
    nbest, cols = got["ids"].shape[1], got["ids"].shape[2]
    ids, lens, sc, lm, credit = F.as_arrays(r64, nbest, cols)
    assert got["ids"].dtype == torch.int32 and got["lengths"].dtype == torch.int32 and got["scores"].dtype == got["lm"].dtype == torch.float32
    assert torch.equal(got["lengths"], torch.from_numpy(lens)), (what, got["lengths"].tolist(), lens.tolist())
    assert torch.equal(got["ids"], torch.from_numpy(ids)), what
    g, glm = got["scores"].double().numpy(), got["lm"].double().numpy()
    assert np.array_equal(np.isneginf(g), lens < 0) and not np.isnan(g).any() and np.isfinite(glm).all(), (what, g.tolist(), glm.tolist())
    assert np.all(glm[lens < 0] == 0.0), (what, "lm of a missing entry")
    if kw["lm"] is None:
        assert np.all(glm == 0.0), (what, "lm without a table")
    if "credit" in got:
        assert got["credit"].dtype == torch.int32 and torch.equal(got["credit"], torch.from_numpy(credit)), (
            what, got["credit"].tolist(), credit.tolist())
    worst = 0.0
    for b, (a64, a32) in enumerate(zip(r64, r32)):
        s32 = {h[0]: float(h[1]) for h in a32["hyps"]}
        err32 = max([abs(s32[h[0]] - float(h[1])) for h in a64["hyps"] if h[0] in s32] + [0.0])
        bound = 4.0 * max(err32, R.EPS32 * a64["maxabs"])
        for n, (y, s, lmv, _) in enumerate(a64["hyps"]):
            err = abs(g[b, n] - float(s))
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else math.inf))
            assert err <= bound, (what, b, n, y, g[b, n], float(s), err, bound)
            assert abs(glm[b, n] - lmv) <= TOL * max(1.0, abs(lmv)), (what, b, n, y, glm[b, n], lmv)
            fused, want = kw["alpha"] * glm[b, n] + kw["beta"] * len(y), kw["alpha"] * lmv + kw["beta"] * len(y)
            assert abs(fused - want) <= TOL * max(1.0, abs(want)), (what, b, n, y, fused, want)
    print("%s: worst score error / bound %.3f" % (what, worst))
    return worst


def assert_crowded_tables(case):
    """Both tables are small enough that a first probe meets another key: a stored key's search reads more than one slot."""
    if case["lm"] is not None and case["lm"].order > 1:
        assert case["lm"].hash_table()[2] > 1
    if case["graph"] is not None:
        assert case["graph"].hash_table()[2] > 1


# ------------------------------------------------------------------------------------------------ the grid
@pytest.mark.parametrize("name", sorted(GRID))
def test_weights_on_matches_the_restatement_in_every_arm(name):
    case = grid_case(name)
    assert_margins(case, name)
    assert_crowded_tables(case)
    got, rc = run(case)
    assert rc == 0
    compare(got, case, name)
    nbest = case["shape"][5]
    assert got["lengths"][1].tolist() == [0] + [-1] * (nbest - 1) and float(got["scores"][1, 0]) == 0.0      # T_b = 0
    want = float(case["lm"].logp((F.BOS,), F.EOS)) if case["lm"] is not None else 0.0
    assert float(got["lm"][1, 0]) == want and ("credit" not in got or int(got["credit"][1, 0]) == 0)


def test_the_grid_is_not_the_plain_search_in_disguise():
    """In at least four of the six cases the fused n-best differs from the plain restatement's: the bonus took part in the pruning."""
    n = 0
    for name in GRID:
        case = grid_case(name)
        n += [h[0] for res in case["r64"] for h in res["hyps"]] != [y for res in case["plain"] for y, _ in res["hyps"]]
    assert n >= 4, n


@pytest.mark.parametrize("name", sorted(GRID))
def test_weights_zero_is_the_plain_search_bit_for_bit(name):
    """Tables present, alpha = beta = gamma = 0 (with and without the end term): ids, lengths and scores are asr_rnnt_beam_search's; lm
    is the LM's log-probability of every hypothesis and credit what it earned."""
    case = grid_case(name)
    Vn, C, W, K, S, nbest = case["shape"]
    Pg = to_gpu(case["Pt"])
    plain, rc = plain_launch(Pg, FRAMES, W, K, S, nbest)
    assert rc == 0
    for eos in (F.EOS, -1):
        got, rc = launch(Pg, FRAMES, W, K, S, nbest, lm=case["lm"], graph=case["graph"], eos=eos)
        assert rc == 0
        for k in plain:
            assert torch.equal(plain[k], got[k]), (name, eos, k)
        for b in range(B):
            for n in range(nbest):
                if got["lengths"][b, n] < 0:
                    assert float(got["lm"][b, n]) == 0.0 and ("credit" not in got or int(got["credit"][b, n]) == 0)
                    continue
                y = got["ids"][b, n, :got["lengths"][b, n]].tolist()
                want = case["lm"].score(y, F.BOS, eos) if case["lm"] is not None else 0.0
                assert abs(float(got["lm"][b, n]) - want) <= TOL * max(1.0, abs(want)), (name, eos, b, n)
                if case["graph"] is not None:
                    assert int(got["credit"][b, n]) == case["graph"].earned(y), (name, eos, b, n)


@pytest.fixture
def compute_dtype():
    from asr_hip import ops
    old = ops.compute_dtype()
    yield ops.set_compute_dtype
    ops.set_compute_dtype(old)


def test_d_full_at_1024_entries_with_the_fused_state(compute_dtype):
    """W 16, S 63, T 2: the second frame starts from 16 hypotheses and every one of its 64 steps adds 16 new sequences to D.  Gaussian
    data; the restatement takes its logits from the project's own joint and projection (tests/test_gpu_rnnt_beam.py's gpu_rows)."""
    compute_dtype(FULL[0])
    held = {}

    def make_rows(Pt):
        held["Pg"] = to_gpu(Pt)
        return [gpu_rows(held["Pg"], 0)]
    case = full_case(make_rows)
    assert len(case["r64"][0]["last_d"]) == 1024
    assert_crowded_tables(case)
    got, rc = run(case, held["Pg"])
    assert rc == 0
    compare(got, case, "D full")


def test_the_widest_fp32_joint_the_fused_arms_admit():
    case = build_case(F32, WIDE_J, 2, 4, 3, 2, 4, 2, True, 0, Vn=5)
    got, rc = run(case)
    assert rc == 0
    compare(got, case, "J %d" % WIDE_J)


# ------------------------------------------------------------------------------------------------ survival
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_the_favoured_sequence_survives_only_through_the_bonus_in_the_pruning(dtype):
    """rnnt_beam_fused_reference.survival_case: [3] is third among the first frame's candidates and the beam holds two.  The plain
    search's n-best does not contain it; the phrase arm's does, and the LM arm's does, each with its own table."""
    Pt = _tensors(F.survival_case(), dtype)
    Pg = to_gpu(Pt)
    row = cpu_rows(Pt, 0)
    plain, rc = plain_launch(Pg, [2], 2, 3, 1, 2)
    assert rc == 0
    found = [plain["ids"][0, n, :plain["lengths"][0, n]].tolist() for n in range(2)]
    assert found == [[2], [4]]
    for kw in (dict(graph=F.graph_of([[3]], 5), gamma=3.0), dict(lm=F.survival_lm(), alpha=2.0)):
        full = dict(fused_kw(None, None, False), **kw)
        case = dict(r64=[F.search(row, 2, 5, 2, 3, 1, 2, 1, **full)], r32=[F.search(row, 2, 5, 2, 3, 1, 2, 1, dtype=np.float32, **full)], kw=full)
        got, rc = launch(Pg, [2], 2, 3, 1, 2, lm=full["lm"], graph=full["graph"], alpha=full["alpha"], gamma=full["gamma"])
        assert rc == 0
        compare(got, case, "survival %s" % sorted(kw))
        assert got["ids"][0, 0, :got["lengths"][0, 0]].tolist() == [3]
        if "graph" in kw:
            assert got["credit"][0].tolist()[0] == 1 and torch.all(got["lm"] == 0)


# ------------------------------------------------------------------------------------------------ what is never read, determinism
@pytest.mark.parametrize("name", ["bf16_j32_w3_k4_s3_o4_both", "bf16_j40_w3_k16_s1_ctx", "f32_j24_w16_k4_s3_o2_both"])
def test_dead_frames_unreachable_table_rows_repeat_calls_and_batch_invariance(name):
    case = grid_case(name)
    Pg = to_gpu(case["Pt"])
    first, rc = run(case, Pg)
    again, rc2 = run(case, Pg)
    assert rc == 0 and rc2 == 0
    for k in first:
        assert torch.equal(first[k], again[k]), (name, k, "two identical calls")
    # NaN in the frames >= T_b of e and in every predictor-table row no hypothesis has as context (the restatement's callbacks recorded
    # which they were asked for)
    poisoned = dict(Pg, e=Pg["e"].clone(), tables=[t.clone() for t in Pg["tables"]])
    for b, n in enumerate(FRAMES):
        poisoned["e"][b, n:] = math.nan
    for k, tab in enumerate(poisoned["tables"]):
        used = set().union(*[r.used[k] for r in case["rows"]])
        dead = [v for v in range(V) if v not in used]
        assert 0 in dead
        tab[dead] = math.nan
    got, rc = run(case, poisoned)
    assert rc == 0
    for k in first:
        assert torch.equal(first[k], got[k]), (name, k, "NaN where nothing may be read")
    for b in range(B):
        alone, rc = run(case, dict(Pg, e=Pg["e"][b:b + 1].contiguous()), FRAMES[b:b + 1])
        assert rc == 0
        for k in first:
            assert torch.equal(first[k][b:b + 1], alone[k]), (name, k, b, "batch invariance")


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_code():
    EINVAL, EUNSUPPORTED = -1, -3
    case = grid_case("f32_j24_w16_k4_s3_o2_both")
    Pg = to_gpu(case["Pt"])
    lm, graph = case["lm"], case["graph"]

    def rc(W=4, K=3, S=2, nbest=2, lm=lm, graph=graph, **kw):
        return launch(Pg, FRAMES, W, K, S, nbest, lm=lm, graph=graph, **kw)[1]
    for g in (None, graph):
        assert rc(graph=g) == 0
        # whatever the plain entry refuses
        assert rc(graph=g, W=17) == EUNSUPPORTED and rc(graph=g, K=17) == EUNSUPPORTED and rc(graph=g, nbest=5) == EUNSUPPORTED
        assert rc(graph=g, W=16, S=64) == EUNSUPPORTED and rc(graph=g, W=16, S=63, nbest=1) == 0
        assert rc(graph=g, blank=-1) == EINVAL and rc(graph=g, sos=V) == EINVAL and rc(graph=g, W=0) == EINVAL
        # the n-gram table and the sentence marks
        cap = lm.device_table("cuda")["capacity"]
        for over in (dict(ng_order=5), dict(ng_order=0), dict(ng_capacity=cap - 1), dict(ng_capacity=0), dict(ng_max_probe=0), dict(lm=0)):
            assert rc(graph=g, over=over) == EINVAL, (g is None, over)
        assert rc(graph=g, bos=-1) == EINVAL and rc(graph=g, bos=V) == EINVAL and rc(graph=g, eos=-2) == EINVAL and rc(graph=g, eos=V) == EINVAL
        assert rc(graph=g, eos=-1) == 0 and rc(graph=g, eos=V - 1) == 0
    assert rc(lm=None, graph=None) == EINVAL                                      # the LM entry without a table
    assert rc(lm=None) == 0 and rc(lm=None, bos=-1, eos=V) == 0                    # phrases only: bos and eos are not looked at
    ccap = graph.device_table("cuda")["capacity"]
    for over in (dict(cx_capacity=ccap + 1), dict(cx_capacity=0), dict(cx_max_probe=0), dict(cx_states=0), dict(cx_keys=None),
                 dict(cx_vals=None), dict(cx_hold=None), dict(credit=0), dict(lm=0)):
        assert rc(over=over) == EINVAL and rc(lm=None, over=over) == EINVAL, over
    # the fused arms' own J limit: their state sits behind the z rows.  fp32 J 1392 is refused before any launch (the pointers are
    # never followed); the plain entry takes it
    from asr_hip import lib as L
    lib, dev = L.load(), torch.device("cuda")
    fl = torch.tensor(FRAMES, dtype=torch.int32, device=dev)
    n = lib.asr_rnnt_beam_workspace(B, T, V, 4, 3, 2)
    ws, ids = torch.zeros(n + 8, device=dev), torch.zeros(B * 2 * T * 2, dtype=torch.int32, device=dev)
    lens, sc, lmv = torch.zeros(B * 2, dtype=torch.int32, device=dev), torch.zeros(B * 2, device=dev), torch.zeros(B * 2, device=dev)
    cr = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    t, c = lm.device_table(dev), graph.device_table(dev)

    def raw(J, entry):
        head = (L.ptr(Pg["e"]), L.ptr(Pg["tables"][0]), L.ptr(Pg["tables"][1]), L.ptr(Pg["w_out"]), L.ptr(Pg["b_out"]), L.ptr(fl), B, T, J, V,
                4, 3, 2, 2, 0, 1, 0, L.ptr(ws), n, L.ptr(ids), L.ptr(lens), L.ptr(sc))
        ng = (L.ptr(t["keys"]), L.ptr(t["vals"]), t["capacity"], t["max_probe"], t["order"], 0, 0, 0.5, 0.3)
        if entry == "lm":
            return lib.asr_rnnt_beam_search_lm(*head, *ng, L.ptr(lmv), L.stream())
        return lib.asr_rnnt_beam_search_ctx(*head, *ng, L.ptr(c["keys"]), L.ptr(c["vals"]), c["capacity"], c["max_probe"], L.ptr(c["hold"]),
                                            c["states"], 1.5, L.ptr(lmv), L.ptr(cr), L.stream())
    assert raw(24, "lm") == 0 and raw(24, "ctx") == 0
    assert raw(1392, "lm") == EUNSUPPORTED and raw(1392, "ctx") == EUNSUPPORTED and raw(20, "lm") == EUNSUPPORTED
    torch.cuda.synchronize()


def test_the_op_picks_the_entry_and_returns_lm_and_credit():
    """ops.rnnt_beam_search: both None makes the plain call (no lm, no credit); ngram alone adds lm; context adds credit; the values are
    the C entries'."""
    from asr_hip import ops
    case = grid_case("bf16_j32_w3_k4_s3_o4_both")
    Vn, C, W, K, S, nbest = case["shape"]
    Pg = to_gpu(case["Pt"])
    fl = torch.tensor(FRAMES, dtype=torch.int32, device="cuda")
    a = (Pg["e"], Pg["tables"], Pg["w_out"], Pg["b_out"], fl, W, K, S, nbest)
    plain = ops.rnnt_beam_search(*a)
    assert sorted(plain) == ["ids", "lengths", "scores"]
    want, _ = plain_launch(Pg, FRAMES, W, K, S, nbest)
    assert all(torch.equal(plain[k].cpu(), want[k]) for k in want)
    kw = case["kw"]
    both = ops.rnnt_beam_search(*a, ngram=kw["lm"], alpha=kw["alpha"], beta=kw["beta"], bos=F.BOS, eos=F.EOS, context=kw["graph"],
                                gamma=kw["gamma"])
    want, _ = run(case, Pg)
    assert sorted(both) == sorted(want) and all(torch.equal(both[k].cpu(), want[k]) for k in want)
    only = ops.rnnt_beam_search(*a, ngram=kw["lm"], alpha=kw["alpha"], beta=kw["beta"], bos=F.BOS, eos=F.EOS)
    want, _ = launch(Pg, FRAMES, W, K, S, nbest, lm=kw["lm"], alpha=kw["alpha"], beta=kw["beta"])
    assert sorted(only) == ["ids", "lengths", "lm", "scores"] and all(torch.equal(only[k].cpu(), want[k]) for k in want)
    assert len(kw["lm"]._tables) == 1 and len(kw["graph"]._tables) == 1          # each table went to the device once
