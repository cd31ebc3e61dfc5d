"""asr_rnnt_beam_search (csrc/rnnt_beam.hip) against the float64 restatement tests/rnnt_beam_reference.py (pinned on the CPU by
tests/test_rnnt_beam_host.py).  B 3 with T_b = (7, 1, 0) of T 7; the grid below samples C in {1, 2}, V in {5, 17, 63, 64, 65, 257, 4364},
J in {8, 72} (plain arm, fp32 and bf16) and {32, 64, 256} (MFMA arm, bf16; fp32 takes the plain arm there too), W in {1, 4, 16}, K in
{1, 3, 16}, S in {1, 2, 4}.

Sequences, lengths and the length -1 slots: torch.equal to the restatement in EVERY case.  That has one right answer because every
margin of the restatement (the K-th against the next logit, the W-th against the next candidate, the W-th against the next entry of D,
neighbours in the result) is at least 1e-3, asserted here on the CPU side; the seeds were searched on the CPU for that.
Scores: |score - ref64| <= 4 max(|ref32 - ref64|, eps32 * the largest magnitude that entered a sum), ref32 = the SAME restatement run in
fp32 on the same logits rows: the bound comes from the two CPU evaluations, never from the kernel's output.
Exact data: e and table entries in {-20, 0, 20}, so z is exactly -1, 0 or 1 in either dtype; w_out small integers and halves, b_out
multiples of 1/512: the logits are the same bits in every arm and in the restatement.
Random data: the restatement's callback takes its logits from the project's own ops.rnnt_joint + F_.linear on the same parameters, so the
search is compared, not the projection's rounding.
Every call runs between sentinels: around ids, lengths, scores and the workspace nothing is written."""
import math

import numpy as np
import pytest
import torch

import rnnt_beam_reference as R
import rnnt_reference as RL

pytestmark = pytest.mark.gpu

B, T, FRAMES = 3, 7, (7, 1, 0)
F32, BF16 = torch.float32, torch.bfloat16
# name: (dtype, J, V, C, W, K, S, nbest, exact seed, random seed)
GRID = {
    "f32_j8_v5": (F32, 8, 5, 1, 1, 1, 1, 1, 0, 0),
    "f32_j72_v17": (F32, 72, 17, 2, 4, 3, 2, 4, 0, 0),
    "f32_j32_v65": (F32, 32, 65, 2, 4, 3, 2, 2, 0, 1),
    "bf16_j8_v63": (BF16, 8, 63, 2, 16, 16, 4, 16, 0, 2),
    "bf16_j72_v65": (BF16, 72, 65, 1, 4, 16, 1, 2, 0, 4),
    "bf16_j32_v64": (BF16, 32, 64, 2, 4, 3, 2, 4, 0, 0),
    "bf16_j64_v257": (BF16, 64, 257, 1, 16, 3, 1, 8, 0, 4),
    "bf16_j256_v17": (BF16, 256, 17, 2, 1, 3, 4, 1, 0, 0),
    "bf16_j256_v4364": (BF16, 256, 4364, 2, 4, 16, 2, 4, 0, 3),
}
# random data: (W, K, S, nbest) where the exact case's would leave no seed with every margin above 1e-3 (16 candidates of 4363 Gaussian
# logits, or 256 candidates for 16 places five times a frame, always hold a pair closer than that)
RANDOM_SHAPE = {"bf16_j256_v4364": (4, 3, 2, 4), "bf16_j8_v63": (16, 3, 1, 16)}
# ... and those two at the exact case's full (W, K, S) on real-valued logits of a sharpened head: name -> (scale of w_out, seed)
SHARP = {"bf16_j256_v4364": (8.0, 1), "bf16_j8_v63": (12.0, 13)}
PAD = 64                                       # sentinel elements on either side of every output and of the workspace


@pytest.fixture
def compute_dtype():
    from asr_hip import ops
    old = ops.compute_dtype()
    yield ops.set_compute_dtype
    ops.set_compute_dtype(old)


def _tensors(P, dtype):
    """The parameters as the kernel reads them: everything in `dtype` (bf16: rounded once), b_out fp32."""
    return dict(e=torch.from_numpy(P["e"]).to(dtype), tables=[torch.from_numpy(t).to(dtype) for t in P["tables"]],
                w_out=torch.from_numpy(P["w_out"]).to(dtype), b_out=torch.from_numpy(P["b_out"]).float())


def cpu_rows(Pt, b):
    """row(t, ctx) of utterance b in float64 from the tensors of _tensors(), with the kernel's roundings: p = the table rows added in the
    compute dtype, z = tanh(e + p) rounded to it.  Records the contexts it was asked for (the table rows the kernel may read)."""
    cd = Pt["e"].dtype
    w, bias = Pt["w_out"].double().numpy(), Pt["b_out"].double().numpy()
    cache, used = {}, [set() for _ in Pt["tables"]]

    def row(t, ctx):
        key = (t, tuple(ctx))
        if key not in cache:
            p = Pt["tables"][0][ctx[0]]
            for tab, c in zip(Pt["tables"][1:], ctx[1:]):
                p = p + tab[c]
            z = torch.tanh(Pt["e"][b, t].float() + p.float()).to(cd)
            cache[key] = w @ z.double().numpy() + bias
            for k, c in enumerate(ctx):
                used[k].add(int(c))
        return cache[key]
    row.used = used
    return row


def gpu_rows(Pg, b):
    """row(t, ctx) of utterance b from the project's own joint and projection on the device tensors Pg (the compute dtype is set)."""
    from asr_hip import functions as F_, ops
    J = Pg["e"].shape[2]
    wp, bp = torch.nn.Parameter(Pg["w_out"].float()), torch.nn.Parameter(Pg["b_out"])
    cache = {}

    def row(t, ctx):
        key = (t, tuple(ctx))
        if key not in cache:
            p = Pg["tables"][0][ctx[0]]
            for tab, c in zip(Pg["tables"][1:], ctx[1:]):
                p = p + tab[c]
            with torch.no_grad():
                z = ops.rnnt_joint(Pg["e"][b:b + 1, t:t + 1].contiguous(), p.view(1, 1, J))
                cache[key] = F_.linear(z.view(1, J), wp, bp, True, True)[0].double().cpu().numpy()
        return cache[key]
    return row


def launch(Pg, frames, W, K, S, nbest, blank=0, sos=1):
    """One call of the C entry between sentinels -> (dict of CPU tensors, return code)."""
    from asr_hip import lib as L
    e = Pg["e"]
    Bn, Tn, J = e.shape
    V = Pg["w_out"].shape[0]
    dev = e.device
    n = L.load().asr_rnnt_beam_workspace(Bn, Tn, V, W, K, S)
    cols = Tn * S

    def guarded(numel, dtype, fill):
        buf = torch.full((numel + 2 * PAD,), fill, device=dev, dtype=dtype)
        return buf, buf[PAD:PAD + numel]
    ws_all, ws = guarded(max(n, 4), torch.float32, -77.0)
    ids_all, ids = guarded(Bn * nbest * cols, torch.int32, -7)
    len_all, lens = guarded(Bn * nbest, torch.int32, -7)
    sc_all, sc = guarded(Bn * nbest, torch.float32, -77.0)
    fl = torch.tensor(list(frames), dtype=torch.int32, device=dev)
    tabs = Pg["tables"]
    rc = L.load().asr_rnnt_beam_search(L.ptr(e), L.ptr(tabs[0]), L.ptr(tabs[1]) if len(tabs) == 2 else None, L.ptr(Pg["w_out"]),
                                       L.ptr(Pg["b_out"]), L.ptr(fl), Bn, Tn, J, V, W, K, S, nbest, blank, sos, L.dt(e), L.ptr(ws), n,
                                       L.ptr(ids), L.ptr(lens), L.ptr(sc), L.stream())
    torch.cuda.synchronize()
    for buf, fill in ((ws_all, -77.0), (ids_all, -7), (len_all, -7), (sc_all, -77.0)):
        assert bool((buf[:PAD] == fill).all()) and bool((buf[-PAD:] == fill).all()), "a sentinel was overwritten"
    return dict(ids=ids.view(Bn, nbest, cols).cpu(), lengths=lens.view(Bn, nbest).cpu(), scores=sc.view(Bn, nbest).cpu()), rc


def to_gpu(Pt):
    return dict(e=Pt["e"].cuda().contiguous(), tables=[t.cuda().contiguous() for t in Pt["tables"]], w_out=Pt["w_out"].cuda().contiguous(),
                b_out=Pt["b_out"].cuda().contiguous())


def expect(rows, frames, V, C, W, K, S, nbest):
    """The restatement in float64 and in fp32 on the same rows -> (results64, results32)."""
    r64 = [R.search(rows[b], frames[b], V, W, K, S, nbest, C) for b in range(len(frames))]
    r32 = [R.search(rows[b], frames[b], V, W, K, S, nbest, C, dtype=np.float32) for b in range(len(frames))]
    return r64, r32


def compare(got, r64, r32, what, S):
    """The rules of the module docstring -> the worst score error over its bound."""
    nbest, cols = got["ids"].shape[1], got["ids"].shape[2]
    for b, res in enumerate(r64):
        assert R.min_margin(res) >= R.MARGIN, (what, b, res["margins"])
    ids, lens, sc = R.as_arrays(r64, nbest, cols)
    assert got["ids"].dtype == torch.int32 and got["lengths"].dtype == torch.int32 and got["scores"].dtype == torch.float32
    assert torch.equal(got["lengths"], torch.from_numpy(lens)), (what, got["lengths"].tolist(), lens.tolist())
    assert torch.equal(got["ids"], torch.from_numpy(ids)), what
    g = got["scores"].double().numpy()
    assert np.array_equal(np.isneginf(g), lens < 0) and not np.isnan(g).any(), (what, g.tolist())
    worst = 0.0
    for b, (a64, a32) in enumerate(zip(r64, r32)):
        s32 = {y: float(s) for y, s in a32["hyps"]}
        err32 = max([abs(s32[y] - float(s)) for y, s in a64["hyps"] if y in s32] + [0.0])
        bound = 4.0 * max(err32, R.EPS32 * a64["maxabs"])
        for n, (y, s) in enumerate(a64["hyps"]):
            err = abs(g[b, n] - float(s))
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else math.inf))
            assert err <= bound, (what, b, n, y, g[b, n], float(s), err, bound)
    print("%s: worst score error / bound %.3f" % (what, worst))
    return worst


def grid_case(name, exact):
    dtype, J, V, C, W, K, S, nbest, seed_exact, seed_random = GRID[name]
    if not exact:
        W, K, S, nbest = RANDOM_SHAPE.get(name, (W, K, S, nbest))
    P = R.exact_case(B, T, J, V, C, seed_exact) if exact else R.random_case(B, T, J, V, C, seed_random)
    return _tensors(P, dtype), (V, C, W, K, S, nbest)


# ------------------------------------------------------------------------------------------------ the grid
@pytest.mark.parametrize("name", sorted(GRID))
def test_exact_data_matches_the_restatement_in_every_arm(name):
    Pt, (V, C, W, K, S, nbest) = grid_case(name, True)
    rows = [cpu_rows(Pt, b) for b in range(B)]
    r64, r32 = expect(rows, FRAMES, V, C, W, K, S, nbest)
    got, rc = launch(to_gpu(Pt), FRAMES, W, K, S, nbest)
    assert rc == 0
    compare(got, r64, r32, name + " exact", S)
    assert got["lengths"][2].tolist() == [0] + [-1] * (nbest - 1) and float(got["scores"][2, 0]) == 0.0      # T_b = 0


@pytest.mark.parametrize("name", sorted(GRID))
def test_random_data_matches_the_restatement_on_the_projects_own_logits(name, compute_dtype):
    Pt, (V, C, W, K, S, nbest) = grid_case(name, False)
    compute_dtype(Pt["e"].dtype)
    Pg = to_gpu(Pt)
    rows = [gpu_rows(Pg, b) for b in range(B)]
    r64, r32 = expect(rows, FRAMES, V, C, W, K, S, nbest)
    got, rc = launch(Pg, FRAMES, W, K, S, nbest)
    assert rc == 0
    compare(got, r64, r32, name + " random", S)


@pytest.mark.parametrize("name", sorted(SHARP))
def test_random_data_of_a_sharpened_head_at_16_candidates(name, compute_dtype):
    """K 16 at V 4364 and W 16 x K 16 on real-valued logits: w_out eight / twelve times larger spreads the rows enough for a seed with
    every margin above 1e-3 to exist."""
    dtype, J, V, C, W, K, S, nbest, _, _ = GRID[name]
    scale, seed = SHARP[name]
    Pt = _tensors(R.random_case(B, T, J, V, C, seed, scale=scale), dtype)
    compute_dtype(dtype)
    Pg = to_gpu(Pt)
    rows = [gpu_rows(Pg, b) for b in range(B)]
    r64, r32 = expect(rows, FRAMES, V, C, W, K, S, nbest)
    got, rc = launch(Pg, FRAMES, W, K, S, nbest)
    assert rc == 0
    compare(got, r64, r32, name + " sharp", S)


CROWD = [4, 5, 6, 7, 260, 261, 262, 263, 516, 517]


def crowded_case(dtype, seed):
    """Exact data (J 32, V 777, C 1) whose ten best labels of every row are columns of ONE lane of the row pass (lane 1 owns 4..7,
    260..263, 516..519): their biases are 16 above the rest, so K = 8 needs more than the 4 entries a lane keeps and the lane scans
    its columns again."""
    P = R.exact_case(B, T, 32, 777, 1, seed)
    P["b_out"][CROWD] += 16.0
    return _tensors(P, dtype)


@pytest.mark.parametrize("dtype,seed", [(BF16, 0), (F32, 0)])
def test_candidates_crowded_into_one_lanes_columns(dtype, seed):
    Pt = crowded_case(dtype, seed)
    rows = [cpu_rows(Pt, b) for b in range(B)]
    r64, r32 = expect(rows, FRAMES, 777, 1, 4, 8, 1, 4)
    assert all(set(y) <= set(CROWD) for res in r64 for y, _ in res["last_d"])
    got, rc = launch(to_gpu(Pt), FRAMES, 4, 8, 1, 4)
    assert rc == 0
    compare(got, r64, r32, "crowded", 1)


def test_the_widest_joint_the_lds_admits():
    """fp32, J 1912: 16 z rows of 1916 floats are 122 624 of the 122 880 bytes of dynamic LDS the entry grants beside its static 36 KB."""
    Pt = _tensors(R.exact_case(B, T, 1912, 5, 2, 1), F32)
    rows = [cpu_rows(Pt, b) for b in range(B)]
    r64, r32 = expect(rows, FRAMES, 5, 2, 4, 3, 2, 4)
    got, rc = launch(to_gpu(Pt), FRAMES, 4, 3, 2, 4)
    assert rc == 0
    compare(got, r64, r32, "J 1912", 2)


# ------------------------------------------------------------------------------------------------ the identity, the merge, the cut
def _identity(dtype, J, V, K, frames, seed):
    """W 16, S 3: every returned sequence y with len(y) <= S whose search was not pruned scores -nll(y) of the training lattice."""
    S, W, C = 3, 16, 2
    P = R.random_case(len(frames), 3, J, V, C, seed)
    Pt = _tensors(P, dtype)
    rows = [cpu_rows(Pt, b) for b in range(len(frames))]
    got, rc = launch(to_gpu(Pt), frames, W, K, S, W)
    assert rc == 0
    out = []
    for b, Tb in enumerate(frames):
        res = R.search(rows[b], Tb, V, W, K, S, W, C)
        r32 = R.search(rows[b], Tb, V, W, K, S, W, C, dtype=np.float32)
        found = {tuple(got["ids"][b, n, :got["lengths"][b, n]].tolist()): float(got["scores"][b, n]) for n in range(W)
                 if got["lengths"][b, n] >= 0}
        assert min(res["margins"][k] for k in ("topk", "cand", "beam")) >= R.MARGIN, (b, res["margins"])
        assert set(found) == {y for y, _ in res["hyps"]}, (b, sorted(found), res["hyps"])
        s32 = {y: float(s) for y, s in r32["hyps"]}
        bound = 4.0 * max(max(abs(s32[y] - float(s)) for y, s in res["hyps"]), R.EPS32 * res["maxabs"])
        for y, s in res["hyps"]:
            assert abs(found[y] - float(s)) <= bound, (b, y, found[y], float(s), bound)
            if not res["pruned"] and len(y) <= S and Tb > 0:
                lg = torch.from_numpy(R.training_logits(rows[b], y, Tb, V, C))[None]
                nll = float(RL.loss_and_grad(lg, torch.tensor([list(y) + [0]]), [Tb], [len(y)])["nll"][0])
                assert abs(found[y] + nll) <= bound, (b, y, found[y], -nll, bound)
        out.append((res["pruned"], len(found)))
    return out


@pytest.mark.parametrize("arm", ["plain", "mfma"])
def test_without_pruning_every_score_is_the_training_likelihood(arm):
    """T 3, V 3, S 3, W 16, K 2.  With T_b = 1 the 15 sequences of at most 3 labels all come back, nothing is pruned, and each score is
    -nll of tests/rnnt_reference.py.  With T_b = 3 the second frame already has 30 candidates for 16 places, so there the 16 returned
    sequences and scores are the restatement's; V 2, K 1 (one label: 10 sequences after three frames, never more than 4 candidates) is
    the unpruned three-frame identity."""
    dtype, J = (F32, 8) if arm == "plain" else (BF16, 32)
    a = _identity(dtype, J, 3, 2, (3, 1, 0), 5)
    assert a[1] == (False, 15) and a[0] == (True, 16) and a[2] == (False, 1)
    b = _identity(dtype, J, 2, 1, (3, 2), 6)
    assert b == [(False, 10), (False, 7)]


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_the_winner_of_the_merge_input_wins_only_through_the_merge(dtype):
    Pt = _tensors(R.merge_case(), dtype)
    row = cpu_rows(Pt, 0)
    r64, r32 = expect([row], [2], 4, 1, 4, 3, 1, 4)
    got, rc = launch(to_gpu(Pt), [2], 4, 3, 1, 4)
    assert rc == 0
    compare(got, r64, r32, "merge", 1)
    assert got["ids"][0, 0].tolist() == [2, 0] and got["ids"][0, 1].tolist() == [3, 0]
    assert math.exp(float(got["scores"][0, 0])) > 0.44 > 0.41 > math.exp(float(got["scores"][0, 1])) > 0.40


@pytest.mark.parametrize("S", [1, 2])
def test_max_symbols_cuts_a_head_that_never_offers_the_blank(S):
    Pt = _tensors(R.cut_case(2), F32)
    row = cpu_rows(Pt, 0)
    r64, r32 = expect([row], [2], 3, 1, 16, 1, S, 16)
    got, rc = launch(to_gpu(Pt), [2], 16, 1, S, 16)
    assert rc == 0
    compare(got, r64, r32, "cut S %d" % S, S)
    lens = got["lengths"][0].tolist()
    assert sorted(x for x in lens if x >= 0) == list(range(2 * S + 1)) and lens.count(-1) == 16 - (2 * S + 1)


# ------------------------------------------------------------------------------------------------ what is never read, determinism
@pytest.mark.parametrize("name", ["f32_j72_v17", "bf16_j32_v64", "bf16_j64_v257"])
def test_dead_frames_unreachable_table_rows_repeat_calls_and_batch_invariance(name):
    Pt, (V, C, W, K, S, nbest) = grid_case(name, True)
    Pg = to_gpu(Pt)
    plain, rc = launch(Pg, FRAMES, W, K, S, nbest)
    again, rc2 = launch(Pg, FRAMES, W, K, S, nbest)
    assert rc == 0 and rc2 == 0
    for k in plain:
        assert torch.equal(plain[k], again[k]), (name, k, "two identical calls")
    # NaN in the frames >= T_b of e and in every table row no hypothesis has as context (the restatement says which it asked for)
    rows = [cpu_rows(Pt, b) for b in range(B)]
    expect(rows, FRAMES, V, C, W, K, S, nbest)
    poisoned = dict(Pg, e=Pg["e"].clone(), tables=[t.clone() for t in Pg["tables"]])
    for b, n in enumerate(FRAMES):
        poisoned["e"][b, n:] = math.nan
    for k, tab in enumerate(poisoned["tables"]):
        used = set().union(*[r.used[k] for r in rows])
        dead = [v for v in range(V) if v not in used]
        assert 0 in dead and len(dead) >= 1
        tab[dead] = math.nan
    got, rc = launch(poisoned, FRAMES, W, K, S, nbest)
    assert rc == 0
    for k in plain:
        assert torch.equal(plain[k], got[k]), (name, k, "NaN where nothing may be read")
    # every utterance run alone
    for b in range(B):
        alone, rc = launch(dict(Pg, e=Pg["e"][b:b + 1].contiguous()), FRAMES[b:b + 1], W, K, S, nbest)
        assert rc == 0
        for k in plain:
            assert torch.equal(plain[k][b:b + 1], alone[k]), (name, k, b, "batch invariance")


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_code():
    from asr_hip import lib as L
    EINVAL, EUNSUPPORTED = -1, -3
    Pt, _ = grid_case("f32_j72_v17", True)
    Pg = to_gpu(Pt)

    def rc(W=4, K=3, S=2, nbest=2, blank=0, sos=1, P=Pg):
        return launch(P, FRAMES, W, K, S, nbest, blank, sos)[1]
    assert rc() == 0
    assert rc(W=17) == EUNSUPPORTED and rc(K=17, W=4) == EUNSUPPORTED and rc(nbest=5) == EUNSUPPORTED
    assert rc(W=16, S=64) == EUNSUPPORTED and rc(W=16, S=63, nbest=1) == 0           # W (S + 1) <= 1024 entries of D
    assert rc(blank=-1) == EINVAL and rc(blank=17) == EINVAL and rc(sos=17) == EINVAL and rc(K=16) == 0 and rc(W=0) == EINVAL
    lib, dev = L.load(), torch.device("cuda")
    fl = torch.tensor(FRAMES, dtype=torch.int32, device=dev)
    n = lib.asr_rnnt_beam_workspace(B, T, 17, 4, 3, 2)
    assert n > 0 and lib.asr_rnnt_beam_workspace(B, T, 17, 4, 3, 0) == 0 and lib.asr_rnnt_beam_workspace(0, T, 17, 4, 3, 2) == 0
    ws = torch.zeros(n + 8, device=dev)
    ids = torch.zeros(B * 2 * T * 2, dtype=torch.int32, device=dev)
    lens = torch.zeros(B * 2, dtype=torch.int32, device=dev)
    sc = torch.zeros(B * 2, device=dev)

    def raw(e=Pg["e"], t0=Pg["tables"][0], w=Pg["w_out"], J=72, V=17, K=3, S=2, wsp=ws, nws=n, dtype=0, Tn=T):
        return lib.asr_rnnt_beam_search(L.ptr(e), L.ptr(t0), L.ptr(Pg["tables"][1]), L.ptr(w), L.ptr(Pg["b_out"]), L.ptr(fl), B, Tn, J, V, 4,
                                        K, S, 2, 0, 1, dtype, L.ptr(wsp), nws, L.ptr(ids), L.ptr(lens), L.ptr(sc), L.stream())
    assert raw() == 0
    assert raw(S=0) == EUNSUPPORTED                        # (its workspace is 0 floats: refused before the size is looked at)
    assert raw(J=68) == EUNSUPPORTED                       # J % 8
    assert raw(Tn=1 << 21, S=255) == EUNSUPPORTED          # T S W >= 2^30 trie nodes (W (S + 1) = 1024 still fits D)
    assert raw(J=1920) == EUNSUPPORTED                     # 16 z rows of 1924 floats: beyond 120 KB of LDS (J 1912 runs: see above)
    assert raw(e=Pg["e"].view(-1)[1:]) == EUNSUPPORTED and raw(w=Pg["w_out"].view(-1)[2:]) == EUNSUPPORTED      # off 16 bytes
    assert raw(wsp=ws[1:]) == EUNSUPPORTED
    assert raw(nws=n - 1) == EINVAL and raw(e=None) == EINVAL and raw(dtype=2) == EINVAL
    assert raw(V=3, K=3) == EINVAL                         # K >= V
    torch.cuda.synchronize()
