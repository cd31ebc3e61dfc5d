"""The rank-64 low-rank step at the widths `bench.py --workload lowrank` measures (BASELINE configs[4]: d_model 512, 8 heads x 64, inner
2048, every projection in -> 64 -> out), in bf16, on the fp8 path and under a replayed hipGraph.  tests/test_gpu_lowrank.py builds
d_model 128 / rank 16 and runs eagerly; the raw GEMM arms are pinned by tests/test_gpu_gemm_exact.py.  This file covers what lies between
those kernels and the benchmark's number: the LinearActFn pair at N = 64 / K = 64 with the three backward routes of functions._lin_bwd, the
fp8 quantise -> GEMM -> re-quantise chain, and all of it under capture.  (The model family has no reference code: PARITY UNPINNED -- the
CPU restatements are tests/lowrank_reference.py and oracle/asr_oracle.py:proj, held against each other by
tests/test_lowrank_chain_host.py, which also asserts the exactness premise of every case of section 1 without a GPU.)

Section 1 -- one factor pair through autograd, BIT for bit (test_pair_exact).  Shapes: `sq` 512 -> 64 -> 512; `up` 512 -> 64 -> 2048 with
relu=True; `chain` = `up` feeding 2048 -> 64 -> 512 with input_is_relu=True, so that the ReLU mask of the second pair's data gradient is a
real one.  Data as in tests/test_gpu_gemm_exact.py: seeded small integers (x in [-2, 2], U, V in {-1, 0, 1}, a 2048-wide U seven eighths
zeros), biases multiples of 1/4, dy integers in [-2, 2] ([-1, 1] for the chain).  The weight gradients contract over M, so for large M zeros are mixed into dy
by ROWS, and only where the premise needs them (dy_rows, NZ_BUDGET): `sq` and `up` are dense up to 36 000 rows -- every case but the two
fp32 / one-launch thresholds at 108 736 and 153 536 rows -- the chain (whose second pair multiplies dy with an h of a few thousand) up to
1200 rows.  Beyond that every stage of 32 rows holds the same number of non-zero rows (at least one), and row 0 and row M - 1 always
are: the row that opens a new tile, stage or slice on the far side of a threshold carries a gradient and has a non-zero dx
(tests/test_lowrank_chain_host.py asserts both for every case).  Every partial sum is then a multiple of 1/4 below 2^22: fp32 accumulation is exact in
any order, h is an exact number rounded ONCE to the compute dtype, and so is every other stored activation.  `_check_premise` asserts that
on the CPU before anything is launched (test_gpu_gemm_exact._premise with the largest |A| |B|^T -- or a row-sum bound above it -- times 4
for the quarter unit).  No shape needed the float64-with-a-bound fall-back.

Routes (each must give the reference's bits for y, dx and the gradients of u.weight, v.weight, v.bias):
  fp32   (a) fp32 compute dtype, eager: per-layer asr_gemm_tn next to asr_gemm_nn (rung 3 of _lin_bwd, no second stream outside a capture)
  bf16   (b) bf16 eager: rung 1, the deferred, grouped weight gradient (asr_gemm_tn_grouped at the end of backward);
             ops.defer_wgrad_now() is recorded inside backward and must have been true for every layer
  graph  (c) bf16 inside torch.cuda.graph: eager warm-up, capture of forward + backward + join_deferred(), gradient buffers zeroed, one
             replay.  ops.gemm_nn_tn_supported() is asserted true inside the capture for every layer of every shape: the size cap
             (ops._nn_tn_max = 2^21 weight elements) lets all of them be -- 64 x 512 = 2^15 and 64 x 2048 / 2048 x 64 = 2^17.  As
             _lin_bwd stands, rung 1 is tried first and applies whenever rung 2 would (both need bf16, gemm_tn_supported and a
             deferral point), so the captured step runs asr_gemm_nn + the grouped launch, NOT asr_gemm_nn_tn: the test asserts that
             ops.queue_wgrad took every layer.  The headline step is the same.
  graph1 (d) as (c) with the deferred queue declining (ops.defer_wgrad_now patched to False: what an active gradient reducer that
             exchanges layer by layer makes it): rung 2, dX and dW workgroups in ONE launch (asr_gemm_nn_tn), folded by the next
             launch and by flush_tn_reduces().  The only way the product reaches that kernel; asserted by counting its calls.

Rows M: 48 (the model tests' row count), 3200 and 6400 (the benchmark's decoder and encoder rows), and one M on each side of every
threshold in M that the dispatch applies at N = 64 or K = 64 (left: the last M before, right: the first M after):
  asr_gemm_nt, bf16 (forward)
    csrc/gemm_big.hip:448  eight-wave 128 x 128 blocks from t128 = 128 on (150 from K = 2048 on):
        x U^T (N = 64): 16256 | 16257 at K = 512 [sq], 19072 | 19073 at K = 2048 [chain];  h V^T (K = 64): 3968 | 3969 at N = 512 [sq],
        896 | 897 at N = 2048 [up]
    csrc/gemm_big.hip:454  4 stages up to t128 = 256 when K >= 2048: 32768 | 32769 [chain]
    csrc/gemm_nt.hip:413   (the ring, K >= 256 and <= 512 blocks: N = 64 gives <= 255 blocks below the eight-wave threshold: always on)
  asr_gemm_nt, fp32 (forward)
    csrc/gemm_nt.hip:430   128 x 64 blocks from t64 = 2400 on: 153536 | 153537 at N = 64 [sq; K does not enter, so the 2048-wide shapes
        are not run at 300 MB of fp32 input per tensor], 19136 | 19137 at N = 512 [sq], 4736 | 4737 at N = 2048 [up]
  asr_gemm_nn, bf16 (data gradient)
    csrc/gemm_big.hip:474  eight-wave blocks from t128 = 150 on: dy V (N = 64) 19072 | 19073 [sq, up, chain];  dh U (K = 64): 4736 | 4737 at
        N = 512 [sq], 1152 | 1153 at N = 2048 with the ReLU mask [chain]
    csrc/gemm_big.hip:475  4 stages up to t128 = 256 when K >= 2048 (dy V of a 2048-wide dy): 32768 | 32769 [up, chain]
    csrc/gemm_nn.hip:357   (the ring, K >= 256 and <= 512 blocks: always on below the eight-wave threshold at N = 64)
  asr_gemm_nn, fp32
    csrc/gemm_nn.hip:353   128-row blocks from kNnBig = 1700 blocks on: 108736 | 108737 at N = 64 [sq], 13568 | 13569 at N = 512 [sq],
        3392 | 3393 at N = 2048 [chain]
  asr_gemm_tn (fp32 route; bf16 goes to the grouped launch, and csrc/gemm_tn.hip:448 keeps the 128 x 128 kernel away from N or K < 128)
    csrc/gemm_tn.hip:424-426  slices of M through the workspace: min(8, stages / 4) with stages = ceil(M / 64): 1 | 2 at 448 | 449, then
        704 | 705, 960 | 961, 1216 | 1217, 1472 | 1473, 1728 | 1729 and 7 | 8 at 1984 | 1985 [sq; 448 | 449 also up]
  asr_gemm_tn_grouped (bf16 routes b and c; the list is the pair's two problems)
    csrc/gemm_tn.hip:925-957 (tn_rot_plan)  whole blocks of dW up to 98 stages of 32 rows, slices that meet in fp32 atomics from 99 on
        (a slice of <= 8 stages + FIXED_ATOMIC = 108 against 99 + FIXED = 109): 3136 | 3137 [sq, up]; the chain's four problems
        (20 blocks) from 102 stages on: 3232 | 3233 [chain]
    csrc/gemm_tn.hip:961-964  the plan declines a list whose sliced blocks need more than one round of the 256 CUs: 26208 | 26209
        [up], 12800 | 12801 [chain]; csrc/gemm_tn.hip:1034 then takes the per-slice form (gemm_tn256g_kernel<3, true, false>, slices of
        mrows = 3200 rows: max M >= slice_min = 9600 in every such list, so the equal-pieces form is not reached).  Above these M the
        decision alternates with the block count (13024, 13472, ... for the chain); both forms run at 19072 .. 32769.
        Every side is asserted through asr_gemm_tn_grouped_plan (PLAN_EDGE).
  asr_gemm_nn_tn (route d)
    csrc/gemm_nn.hip:585-586  one weight-gradient slice per 16 stages of 64 rows: 1024 | 1025 [sq, up]
    csrc/gemm_nn.hip:628      128-row data-gradient blocks from kNnBig on: 13568 | 13569 at K = 512 [sq], 3392 | 3393 at K = 2048 [chain],
        108736 | 108737 at K = 64 [sq]

Section 2 -- the fp8 pair (test_fp8_pair_*).  Section 3 -- model W against the oracle (test_model_w_matches_oracle).  Section 4 --
cross_kv_all declines factor pairs (test_cross_kv_all_declines_factor_pairs).  Section 5 -- graph replay equals eager for model W, bf16
and fp8, with a stale-weight negative control (test_model_w_graph_replay_equals_eager).  test_vocabulary_projection_fp32_logits_exact adds
the one GEMM-family kernel of the benchmark's step that no factor pair reaches.  Model W: two layers of the benchmark's widths,
V = 40, the batch of test_gpu_lowrank._batch (B = 3, 64 frames ragged to 64 / 48 / 20, targets 20 / 11 / 4).
"""
import argparse
import ctypes
import zlib

import numpy as np
import pytest
import torch

import lowrank_reference as R
from test_gpu_gemm_exact import _premise, _same
from test_gpu_lowrank import _batch, _e4m3_decode

pytestmark = pytest.mark.gpu

D = "cuda:0"
F32, BF = torch.float32, torch.bfloat16
RANK = 64
# rows of dy that are not zero (dy_rows): what the exactness premise leaves room for -- the weight gradients contract over M.  |dh| |x| and
# |dy| |h| add about 100 per row for `sq` and `up` (times 4 for the quarter unit: 2^24 is 40 000 rows away); the chain's second pair
# multiplies dy with an h of a few thousand (a 2048-wide contraction of ReLU outputs), which leaves room for about 2 500 rows
NZ_BUDGET = {"sq": 36000, "up": 36000, "chain": 1200}

FLAGS_W = ["--num-layers", "2", "--num-heads", "8", "--dim-model", "512", "--dim-key", "64", "--dim-value", "64", "--dim-inner", "2048",
           "--dim-emb", "512", "--feat_extractor", "vgg_cnn", "--label-smoothing", "0.1", "--dropout", "0.0", "--tgt-max-len", "24",
           "--src-max-len", "64"]

# (in, out, relu, input_is_relu) of each pair of a shape
SHAPES = {"sq": [(512, 512, False, False)], "up": [(512, 2048, True, False)],
          "chain": [(512, 2048, True, False), (2048, 512, False, True)]}
COMMON_M = (48, 3200, 6400)
ROUTE_M = {
    ("sq", "fp32"): (448, 449, 704, 705, 960, 961, 1216, 1217, 1472, 1473, 1728, 1729, 1984, 1985, 13568, 13569, 19136, 19137, 108736, 108737,
                     153536, 153537),
    ("up", "fp32"): (448, 449, 4736, 4737),
    ("chain", "fp32"): (3392, 3393),
    ("sq", "bf16"): (3136, 3137, 3968, 3969, 4736, 4737, 16256, 16257, 19072, 19073),
    ("up", "bf16"): (896, 897, 3136, 3137, 19072, 19073, 26208, 26209, 32768, 32769),
    ("chain", "bf16"): (1152, 1153, 3232, 3233, 12800, 12801, 19072, 19073, 32768, 32769),
    ("sq", "graph1"): (1024, 1025, 13568, 13569, 108736, 108737),
    ("up", "graph1"): (1024, 1025),
    ("chain", "graph1"): (3392, 3393),
}
ROUTE_M.update({(s, "graph"): ROUTE_M[(s, "bf16")] for s in SHAPES})
ROUTES = ("fp32", "bf16", "graph", "graph1")
# asr_gemm_tn_grouped_plan of the pairs' problem list on either side of its thresholds: (whole blocks?, a block cut into slices?)
PLAN_EDGE = {("sq", 3136): (1, False), ("sq", 3137): (1, True), ("up", 3136): (1, False), ("up", 3137): (1, True), ("up", 26208): (1, True),
             ("up", 26209): (0, True), ("chain", 3232): (1, False), ("chain", 3233): (1, True), ("chain", 12800): (1, True), ("chain", 12801): (0, True)}


def pair_cases():
    """[(shape, M, route)] of section 1, the routes of one (shape, M) next to each other (they share one reference per compute dtype)."""
    out = []
    for s in SHAPES:
        ms = sorted(set(COMMON_M).union(*[ROUTE_M[(s, r)] for r in ROUTES]))
        for m in ms:
            out += [(s, m, r) for r in ROUTES if m in COMMON_M or m in ROUTE_M[(s, r)]]
    return out


def route_dtype(route):
    return F32 if route == "fp32" else BF


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def dy_rows(shape, M, g):
    """The rows of dy that are not zero: all of them up to NZ_BUDGET[shape] rows (what the premise leaves room for); beyond that the
    same number in every stage of 32 rows (the finest unit any weight-gradient kernel or slice plan walks M in), chosen at random inside
    the stage, plus row 0 and row M - 1 -- the row that opens a new tile, stage or slice on the far side of a threshold always counts."""
    budget = NZ_BUDGET[shape]
    if M <= budget:
        return torch.arange(M)
    stages = (M + 31) // 32
    per = max(1, budget // stages)
    offs = torch.rand((stages, 32), generator=g).argsort(1)[:, :per]
    rows = (torch.arange(stages)[:, None] * 32 + offs).reshape(-1)
    # (a short last stage keeps what falls inside it; rows M - 32 .. M - 1 cover it whatever M % 32 is)
    rows = torch.cat([rows[rows < M], torch.tensor([0, M - 1]), (M - 32 + torch.rand(32, generator=g).argsort()[:per]).clamp_min(0)])
    return rows.unique()


def pair_data(shape, M):
    """Seeded integer data of one case (module docstring) -> dict(x, dy, pairs=[dict(U, V, b, relu, input_is_relu)], nz = the rows of dy
    that are not zero)."""
    g = torch.Generator().manual_seed(zlib.crc32(("%s-%d" % (shape, M)).encode()))
    spec = SHAPES[shape]
    pairs = []
    for din, dout, relu, inrelu in spec:
        U = _ints(g, (RANK, din), -1, 1)
        if din > 512:
            U = U * (torch.rand((RANK, din), generator=g) < 0.125)
        pairs.append({"U": U, "V": _ints(g, (dout, RANK), -1, 1), "b": torch.randint(-8, 9, (dout,), generator=g).double() / 4.0,
                      "relu": relu, "input_is_relu": inrelu})
    x = _ints(g, (M, spec[0][0]), -2, 2)
    nz = dy_rows(shape, M, g)
    dy = torch.zeros((M, spec[-1][1]), dtype=torch.float64)
    amp = 1 if len(spec) > 1 else 2
    vals = _ints(g, (len(nz), spec[-1][1]), -amp, amp)
    vals[:, 0] = vals[:, 0] + (vals == 0).all(1) * 1.0         # (no chosen row is a zero row)
    dy[nz] = vals
    return {"x": x, "dy": dy, "pairs": pairs, "nz": nz}


def pair_reference(data, dtype):
    """The chain of pairs through tests/lowrank_reference.py -> dict(y, dx (both un-rounded), acts=[(x, h, y)], grads=[dict])."""
    rnd = R.rounder(dtype)
    x, acts = data["x"], []
    for p in data["pairs"]:
        h, y = R.pair_forward(x, p["U"], p["V"], p["b"], p["relu"], dtype)
        acts.append((x, h, y))
        x = rnd(y)
    dy, grads = data["dy"], []
    for p, (xi, h, _) in zip(reversed(data["pairs"]), reversed(acts)):
        gr = R.pair_backward(xi, p["U"], p["V"], h, dy, p["input_is_relu"], dtype)
        gr["dy"] = dy
        grads.insert(0, gr)
        dy = rnd(gr["dx"])
    return {"y": acts[-1][2], "dx": grads[0]["dx"], "acts": acts, "grads": grads}


def _rowsum_bound(A, B):
    """An upper bound of the largest entry of |A| |B|^T (A (M, K), B (N, K)) that costs no product."""
    return float(min(A.abs().sum(1).max() * B.abs().max(), A.abs().max() * B.abs().sum(1).max()))


def check_premise(name, data, ref):
    """Every product of the case is exact in fp32 whatever the order of its partial sums: test_gpu_gemm_exact._premise with four times
    the bound (the partial sums are multiples of 1/4).  The weight gradients contract over M: their |A|^T |B| is computed on the rows
    where dy is not zero (every other row adds exact zeros)."""
    nz = data["nz"]
    for i, (p, (x, h, y), gr) in enumerate(zip(data["pairs"], ref["acts"], ref["grads"])):
        tag = "%s pair %d " % (name, i)
        _premise(tag + "h", x @ p["U"].t(), 4 * _rowsum_bound(x, p["U"]))
        _premise(tag + "y", h @ p["V"].t() + p["b"], 4 * (_rowsum_bound(h, p["V"]) + 2))
        dy = gr["dy"]
        _premise(tag + "dh", dy @ p["V"], 4 * _rowsum_bound(dy, p["V"].t()))
        _premise(tag + "dx", gr["dx"], 4 * _rowsum_bound(gr["dh"], p["U"].t()))
        _premise(tag + "dU", gr["dU"], 4 * float((gr["dh"][nz].abs().t() @ x[nz].abs()).max()))
        _premise(tag + "dV", gr["dV"], 4 * float((dy[nz].abs().t() @ h[nz].abs()).max()))
        _premise(tag + "db", gr["db"], 4 * float(dy.abs().sum(0).max()))


_ref_cache = {}


def _case(shape, M, dtype):
    """(data, reference) of a case: computed once, shared by the routes of one compute dtype (the latest case only: the tensors are large)."""
    key = (shape, M, dtype)
    if _ref_cache.get("key") != key:
        _ref_cache.clear()
        data = pair_data(shape, M)
        ref = pair_reference(data, dtype)
        check_premise("%s M=%d %s" % (shape, M, dtype), data, ref)
        _ref_cache.update(key=key, val=(data, ref))
    return _ref_cache["val"]


class _Pairs(torch.nn.Module):
    def __init__(self, spec):
        super().__init__()
        from models.common_layers import LowRankLinear
        self.spec = spec
        self.pairs = torch.nn.ModuleList([LowRankLinear(din, dout, RANK) for din, dout, _, _ in spec])

    def forward(self, x):
        for p, (_, _, relu, inrelu) in zip(self.pairs, self.spec):
            x = p(x, relu=relu, input_is_relu=inrelu)
        return x


def _pair_module(shape, dtype, weights=None):
    """The pairs of a shape on the GPU with their optimiser created through init_optimizer (flat buffers, P.grad_of as in the model)."""
    from asr_hip import ops
    from utils.functions import init_optimizer
    ops.set_compute_dtype(dtype)
    ops.set_fp8(False)
    torch.manual_seed(5)
    mod = _Pairs(SHAPES[shape]).to(D)
    opt = init_optimizer(argparse.Namespace(dim_input=512, k_lr=1.0, warmup=4000, min_lr=1e-5, parallel=False), mod, "noam")
    assert opt.optimizer.flat is not None
    if weights is not None:
        with torch.no_grad():
            for p, w in zip(mod.pairs, weights):
                p.u.weight.copy_(w["U"])
                p.v.weight.copy_(w["V"])
                p.v.bias.copy_(w["b"])
    return mod, opt


def _grouped_plan(layers):
    from asr_hip import lib as L
    n = len(layers)
    I = ctypes.c_int * n
    sp = I()
    whole = L.load().asr_gemm_tn_grouped_plan(n, I(*[l[0] for l in layers]), I(*[l[1] for l in layers]), I(*[l[2] for l in layers]), sp)
    return whole, list(sp)


@pytest.mark.parametrize("shape,M,route", pair_cases(), ids=lambda v: str(v))
def test_pair_exact(shape, M, route, monkeypatch):
    """Section 1 of the module docstring: y, dx and the three parameter gradients of every pair of the shape, torch.equal to the reference."""
    from asr_hip import ops
    dtype = route_dtype(route)
    data, ref = _case(shape, M, dtype)
    name = "pair %s M=%d %s" % (shape, M, route)
    x_d = data["x"].to(dtype).to(D).requires_grad_(True)
    dy_d = data["dy"].to(dtype).to(D)
    seen = {"defer": [], "queued": 0, "nn_tn": 0}
    defer_now, queue, nn_tn = ops.defer_wgrad_now, ops.queue_wgrad, ops.gemm_nn_tn

    def recorded_defer(*a):          # route d: the queue declines, as under a gradient reducer that exchanges layer by layer
        seen["defer"].append(False if route == "graph1" else defer_now(*a))
        return seen["defer"][-1]

    monkeypatch.setattr(ops, "defer_wgrad_now", recorded_defer)
    monkeypatch.setattr(ops, "queue_wgrad", lambda *a: (seen.__setitem__("queued", seen["queued"] + 1), queue(*a))[1])
    monkeypatch.setattr(ops, "gemm_nn_tn", lambda *a, **k: (seen.__setitem__("nn_tn", seen["nn_tn"] + 1), nn_tn(*a, **k))[1])
    layers = 2 * len(SHAPES[shape])

    def run():
        y = mod(x_d)
        y.backward(dy_d)
        ops.join_deferred()
        return y

    try:
        mod, opt = _pair_module(shape, dtype, data["pairs"])        # (sets the compute dtype: inside the try that restores it)
        opt.zero_grad()
        if route in ("fp32", "bf16"):
            y = run()
            if route == "bf16":
                assert seen["defer"] == [True] * layers and seen["queued"] == layers, seen
                if (shape, M) in PLAN_EDGE:   # the grouped launch's own thresholds: this M is on the side the table says
                    probs = [q for din, dout, _, _ in SHAPES[shape] for q in ((M, dout, RANK), (M, RANK, din))]
                    whole, sp = _grouped_plan(probs)
                    assert (whole, max(sp) > 1) == PLAN_EDGE[(shape, M)], (whole, sp)
            else:
                assert seen["queued"] == 0 and seen["nn_tn"] == 0, seen
        else:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                monkeypatch.setattr(ops, "defer_wgrad_now", defer_now)      # (the warm-up is the eager step)
                run()
                monkeypatch.setattr(ops, "defer_wgrad_now", recorded_defer)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            ops.reset_pending()
            seen.update(defer=[], queued=0, nn_tn=0)
            x_d.grad = None
            probe = [(torch.empty((M, p.v.weight.shape[0]), device=D, dtype=BF), torch.empty((M, RANK), device=D, dtype=BF), p) for p in mod.pairs]
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                for dyo, hh, p in probe:         # (a host-side predicate: nothing is recorded)
                    assert ops.gemm_nn_tn_supported(dyo, torch.empty_like(p.v.weight, dtype=BF), hh)
                    assert ops.gemm_nn_tn_supported(hh, torch.empty_like(p.u.weight, dtype=BF), torch.empty((M, p.u.weight.shape[1]), device=D, dtype=BF))
                y = run()
            if route == "graph":
                assert seen["defer"] == [True] * layers and seen["queued"] == layers and seen["nn_tn"] == 0, seen
            else:
                assert seen["queued"] == 0 and seen["nn_tn"] == layers, seen
            opt.zero_grad()                      # the gradient buffers: the replay must fill them by itself
            graph.replay()
        torch.cuda.synchronize()
    finally:
        ops.reset_pending()
        ops.set_compute_dtype(BF)
    _same(name + " y", y.detach(), ref["y"].to(dtype))
    _same(name + " dx", x_d.grad, ref["dx"].to(dtype))
    for i, (p, gr) in enumerate(zip(mod.pairs, ref["grads"])):
        _same(name + " pair %d u.weight.grad" % i, p.u.weight.grad, gr["dU"].float())
        _same(name + " pair %d v.weight.grad" % i, p.v.weight.grad, gr["dV"].float())
        _same(name + " pair %d v.bias.grad" % i, p.v.bias.grad.view(1, -1), gr["db"].float().view(1, -1))


def test_vocabulary_projection_fp32_logits_exact():
    """The one GEMM-family kernel of the benchmark's low-rank step that no factor pair can reach (tools/kernel_coverage.py diff): the
    vocabulary projection, fp32 logits from bf16 operands at N = 4364 >= 2048 -- gemm_big_nt_kernel<256, 256, 2, float>
    (csrc/gemm_big.hip:446; no block-count floor for that tile, so 130 rows reach it) -- through functions.linear and its backward (the
    fp32 gradient cast and zero padded to 4416 columns by functions._as_compute, then the data gradient and the queued weight gradient),
    on integer data: bit equality with the float64 products."""
    from asr_hip import functions as F_
    from asr_hip import ops
    from utils.functions import init_optimizer
    M, V, K = 130, 4364, 512
    g = torch.Generator().manual_seed(V)
    x, W, dy = _ints(g, (M, K), -2, 2), _ints(g, (V, K), -1, 1), _ints(g, (M, V), -2, 2)
    y, dx, dW = x @ W.t(), dy @ W, dy.t() @ x
    _premise("vocabulary y", y, _rowsum_bound(x, W))
    _premise("vocabulary dx", dx, _rowsum_bound(dy, W.t()))
    _premise("vocabulary dW", dW, float((dy.abs().t() @ x.abs()).max()))
    ops.set_compute_dtype(BF)
    ops.set_fp8(False)
    lin = torch.nn.Linear(K, V, bias=False).to(D)
    opt = init_optimizer(argparse.Namespace(dim_input=512, k_lr=1.0, warmup=4000, min_lr=1e-5, parallel=False), lin, "noam")
    with torch.no_grad():
        lin.weight.copy_(W)
    try:
        opt.zero_grad()
        x_d = x.to(BF).to(D).requires_grad_(True)
        out = F_.linear(x_d, lin.weight, None, True, True)
        out.backward(dy.float().to(D))
        ops.join_deferred()
        torch.cuda.synchronize()
    finally:
        ops.reset_pending()
    _same("vocabulary projection logits", out.detach(), y.float())
    _same("vocabulary projection dx", x_d.grad, dx.to(BF))
    _same("vocabulary projection weight.grad", lin.weight.grad, dW.float())


# ================================================================================================ section 2: the fp8 pair
def e4m3_step(xs):
    """Spacing of the e4m3 values around xs (the expression of tests/test_gpu_lowrank.py:112): 2^(floor(log2 |xs|) - 3), 2^-9 below 2^-6."""
    return torch.clamp(2.0 ** (torch.floor(torch.log2(xs.abs().clamp_min(2.0 ** -6))) - 3), min=2.0 ** -9)


def _fp8_data(shape, M):
    """Random bf16 data as in test_fp8_gemm_is_exact_on_its_quantised_operands: x ~ N(0, 1), weights ~ N(0, 1 / fan-in), biases ~ N(0, 1)."""
    g = torch.Generator().manual_seed(M + sum(a + b for a, b, _, _ in SHAPES[shape]))
    x = torch.randn(M, SHAPES[shape][0][0], generator=g).bfloat16()
    ws = [{"U": (torch.randn(RANK, din, generator=g) / din ** 0.5).bfloat16(), "V": (torch.randn(dout, RANK, generator=g) / RANK ** 0.5).bfloat16(),
           "b": torch.randn(dout, generator=g)} for din, dout, _, _ in SHAPES[shape]]
    dy = torch.randn(M, SHAPES[shape][-1][1], generator=g).bfloat16()
    return x, ws, dy


def _record_fp8(monkeypatch, ops):
    calls = []
    real = ops.gemm_nt_fp8
    monkeypatch.setattr(ops, "gemm_nt_fp8", lambda qa, sa, qb, sb, **k: (calls.append([qa, sa, qb, sb, k, real(qa, sa, qb, sb, **k)]), calls[-1][-1])[1])
    return calls


def _check_fp8_chain(name, ops, mod, x_d, calls):
    """Every fp8 GEMM the forward of `mod` issued (calls, in order) against the float64 product of the DECODED e4m3 bytes of ITS input (x,
    then the product's own previous output) and of the CURRENT weight, both quantised here with ops.quant_fp8: the recorded operands
    must be those bytes and scales, and the bf16 output must be the rounding of a number within 1e-4 max|exact| of the exact one (the bound
    test_fp8_gemm_is_exact_on_its_quantised_operands measured for the instruction).  The issue states the check as |out - bf16(exact)| <=
    1e-4 max|exact|; a result within that distance of a rounding boundary may round to the neighbour, one bf16 step (2^-8 of the element)
    away, so the check is made on the interval [bf16(exact - tol), bf16(exact + tol)], which asks the same of the accumulation
    (measured: about 1 % of the outputs are such neighbours, 4741 of 409600 for x U^T at 6400 rows; the count is printed)."""
    weights = [w for p in mod.pairs for w in ((p.u.weight, None, False), (p.v.weight, p.v.bias, None))]
    assert len(calls) == len(weights), (len(calls), len(weights))
    a = x_d.detach()
    worst = 0.0
    for i, ((w, b, _), (qa, sa, qb, sb, kw, out)) in enumerate(zip(weights, calls)):
        tag = "%s fp8 GEMM %d" % (name, i)
        relu = bool(kw.get("relu"))
        qa2, sa2 = ops.quant_fp8(a.reshape(-1, a.shape[-1]).contiguous())
        qb2, sb2 = ops.quant_fp8(w.data.view(w.shape[0], -1))
        for got, want, what in ((qa, qa2, "activation bytes"), (sa, sa2, "activation scales"), (qb, qb2, "weight bytes"), (sb, sb2, "weight scales")):
            assert torch.equal(got, want), "%s: the product's %s are not those of its current operand" % (tag, what)
        K = w.shape[1]
        assert not bool(((qa2 & 0x7F) == 0x7F).any()) and not bool(((qb2 & 0x7F) == 0x7F).any())       # (no NaN code: _e4m3_decode has none)
        da, db = _e4m3_decode(qa2.cpu())[:, :K], _e4m3_decode(qb2.cpu())[:, :K]
        exact = (da @ db.t()) * (sa2.double().cpu()[:, None] * sb2.double().cpu()[None, :])
        if b is not None:
            exact = exact + b.data.double().cpu()
        if relu:
            exact = exact.clamp_min(0.0)
        tol = 1e-4 * float(exact.abs().max())
        o = out.detach().double().cpu()
        lo, hi = (exact - tol).to(BF).double(), (exact + tol).to(BF).double()
        if relu:
            lo = lo.clamp_min(0.0)
        bad = (o < lo) | (o > hi)
        flips = int((o != exact.to(BF).double()).sum())
        err = float((o - exact).abs().max())
        worst = max(worst, err / max(float(exact.abs().max()), 1e-30))
        print("%s: max |out - exact| %.3e (max |exact| %.3e), %d of %d outputs are not bf16(exact)" % (tag, err, float(exact.abs().max()), flips, o.numel()))
        assert not bool(bad.any()), "%s: %d outputs outside [bf16(exact - tol), bf16(exact + tol)], tol %.3e" % (tag, int(bad.sum()), tol)
        a = out
    return worst


def _bytes_changed(ops, w, before):
    q, _ = ops.quant_fp8(w.data.view(w.shape[0], -1))
    return float((q[:, :w.shape[1]] != before[:, :w.shape[1]]).float().mean())


@pytest.mark.parametrize("M", [48, 6400])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fp8_pair_forward_and_freshness(shape, M, monkeypatch):
    """Forward of the fp8 pair on the CPU chain of decoded bytes (_check_fp8_chain), then FRESHNESS: u.weight doubled in place through
    torch (the version counter), and an optimiser step through the C ABI (the generation counter) with a learning rate of 0.05 -- about the
    standard deviation of the weights, so that most e4m3 bytes change (asserted: more than half) -- each followed by a forward that must
    be the chain of the NEW bytes.  (Doubling moves the row scales and leaves the bytes: a stale cache halves h.)"""
    from asr_hip import ops
    x, ws, dy = _fp8_data(shape, M)
    mod, opt = _pair_module(shape, BF, ws)
    name = "fp8 pair %s M=%d" % (shape, M)
    x_d, dy_d = x.to(D).requires_grad_(True), dy.to(D)
    calls = _record_fp8(monkeypatch, ops)
    try:
        ops.set_fp8(True)
        opt.zero_grad()
        y = mod(x_d)
        _check_fp8_chain(name, ops, mod, x_d, calls)
        u = mod.pairs[0].u.weight
        h0 = calls[0][-1].detach().float().clone()
        with torch.no_grad():
            u.mul_(2.0)
        del calls[:]
        mod(x_d)
        _check_fp8_chain(name + " after u.weight *= 2", ops, mod, x_d, calls)
        # doubling a weight doubles its power-of-two-scaled row scales and leaves the bytes: every product doubles exactly
        assert torch.equal(calls[0][-1].float(), 2 * h0) and float(h0.abs().max()) > 0
        before = [ops.quant_fp8(p.data.view(p.shape[0], -1))[0].clone() for pr in mod.pairs for p in (pr.u.weight, pr.v.weight)]
        y.backward(dy_d)
        ops.join_deferred()
        for grp in opt.optimizer.param_groups:
            grp["lr"] = 0.05
        opt.optimizer.step()
        changed = [_bytes_changed(ops, p, b) for p, b in zip([p for pr in mod.pairs for p in (pr.u.weight, pr.v.weight)], before)]
        print("%s: fraction of e4m3 bytes changed by the optimiser step %s" % (name, ["%.3f" % c for c in changed]))
        assert min(changed) > 0.5, changed
        del calls[:]
        mod(x_d)
        _check_fp8_chain(name + " after an optimiser step", ops, mod, x_d, calls)
        torch.cuda.synchronize()
    finally:
        ops.set_fp8(False)
        ops.reset_pending()


@pytest.mark.parametrize("M", [48, 6400])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fp8_pair_backward_is_the_bf16_backward(shape, M):
    """functions.LinearActFn documents its fp8 backward as the bf16 straight-through expression on the bf16 operands: for single calls
    with the same x, W and dy (each layer of the shape's pairs: in -> 64 without a bias, 64 -> out with one, with the shape's relu /
    input_is_relu flags) dx, dW and db in fp8 mode are torch.equal to those in bf16 mode.
    M = 48: random bf16 x and dy.  M = 6400: the weight and bias gradients of 6400 rows are sums whose slices meet in fp32 atomics
    (csrc/gemm_tn.hip tn_rot_plan from 3137 rows on; the column sums always), so two runs of the SAME mode on random data differ in the
    last bits (measured: 25052 of 32768 elements of a 64 x 512 dW).  There the case runs twice: on random bf16 x and dy, where dx -- one
    data-gradient launch, no atomics -- must still be equal; and with x and dy small integers (the weights stay random bf16, and the fp8
    forward is asserted to differ from the bf16 one), where every order of a sum gives the same bits and dW and db are compared too."""
    from asr_hip import functions as F_
    from asr_hip import ops
    x, ws, dy = _fp8_data(shape, M)
    g = torch.Generator().manual_seed(M)

    def rnd(kind, rows, cols):
        return (torch.randint(-2, 3, (rows, cols), generator=g).float() if kind == "integer" else torch.randn(rows, cols, generator=g)).bfloat16()

    try:
        mod, opt = _pair_module(shape, BF, ws)
        for kind in (("random",) if M <= 3136 else ("random", "integer")):
            sums_too = kind == "integer" or M <= 3136
            for i, (pr, (din, dout, relu, inrelu)) in enumerate(zip(mod.pairs, SHAPES[shape])):
                xin = (rnd(kind, M, din).clamp_min(0) if inrelu else rnd(kind, M, din)).to(D)
                layers = [(pr.u.weight, None, False, inrelu, xin, rnd(kind, M, RANK).to(D)),
                          (pr.v.weight, pr.v.bias, relu, False, rnd(kind, M, RANK).to(D), rnd(kind, M, dout).to(D))]
                for j, (w, b, rl, ir, xi, dyi) in enumerate(layers):
                    got = {}
                    for mode in (False, True):
                        ops.set_fp8(mode)
                        opt.zero_grad()
                        xi_ = xi.clone().requires_grad_(True)
                        yy = F_.LinearActFn.apply(xi_, w, b, rl, ir)
                        yy.backward(dyi)
                        ops.join_deferred()
                        torch.cuda.synchronize()
                        got[mode] = (yy.detach().clone(), xi_.grad.clone(), w.grad.clone(), None if b is None else b.grad.clone())
                    tag = "fp8 backward %s M=%d %s data pair %d layer %d" % (shape, M, kind, i, j)
                    assert not torch.equal(got[True][0], got[False][0]), tag + ": the fp8 forward did not run"
                    _same(tag + " dx", got[True][1], got[False][1])
                    if sums_too:
                        _same(tag + " dW", got[True][2], got[False][2])
                        if b is not None:
                            _same(tag + " db", got[True][3].view(1, -1), got[False][3].view(1, -1))
                    assert float(got[False][2].abs().max()) > 0 and float(got[False][1].abs().max()) > 0
    finally:
        ops.set_fp8(False)
        ops.set_compute_dtype(BF)
        ops.reset_pending()


# ================================================================================================ model W
def _build_w(precision, rank=RANK, extra=()):
    """Model W (module docstring) as tests/test_gpu_lowrank.py builds its model: seed 7, 0.1 N(0, 1) added to every vector parameter."""
    from utils import constant
    from utils.functions import init_transformer_model
    flags = FLAGS_W + (["--rank", str(rank)] if rank else []) + list(extra)
    args = constant.parse(flags + ["--precision", precision, "--cuda"])
    V = 40
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + [chr(0x4E00 + i) for i in range(V - 3)]
    l2i = {c: i for i, c in enumerate(chars)}
    torch.manual_seed(7)
    model = init_transformer_model(args, l2i, {i: c for c, i in l2i.items()})
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in sorted(model.named_parameters()):
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    return args, model, V


_oracle_cache = {}


def _oracle(rank, dtype=torch.float64):
    """oracle.asr_oracle.train_step of model W (rank 64) or of the full-rank model of the same widths (rank 0) on the batch, from the
    state_dict _build_w gives (the same for every precision: seeded): computed once per (rank, dtype)."""
    from oracle import asr_oracle as O
    if (rank, dtype) not in _oracle_cache:
        _, model, V = _build_w("fp32", rank)
        src, src_len, tgt = _batch(V)
        w = {k: v.detach().to(dtype).cpu() if v.dtype.is_floating_point else v.cpu() for k, v in model.state_dict().items()}
        _oracle_cache[(rank, dtype)] = O.train_step(w, O.Cfg.from_flags(" ".join(FLAGS_W)), src.to(dtype), src_len, tgt, 0.1)
    return _oracle_cache[(rank, dtype)]


def _errors(pred, loss, grads, ref):
    """(logit error / max(1, max |logit|), |loss error|, worst and median relative L2 error of the gradients) against an oracle result."""
    amax = float(ref["pred"].abs().max())
    perr = float((pred.double() - ref["pred"].double()).abs().max())
    rel = {}
    for k, gk in grads.items():
        if k.endswith("key_linear.v.bias") or k.endswith("key_linear.bias"):
            continue                                  # exact gradient is zero (softmax shift invariance)
        a, b = gk.double().reshape(-1), ref["grads"][k].double().reshape(-1)
        rel[k] = float((a - b).norm() / (b.norm() + 1e-30))
    worst = max(rel, key=rel.get)
    return {"logit": perr, "amax": amax, "loss": abs(loss - ref["loss"]), "worst": rel[worst], "worst_name": worst,
            "median": float(np.median(list(rel.values())))}


def _gpu_step(precision, rank):
    from utils.functions import init_optimizer
    from utils.metrics import calculate_metrics
    args, model, V = _build_w(precision, rank)
    src, src_len, tgt = _batch(V)
    model = model.cuda().train()
    opt = init_optimizer(args, model, "noam")
    opt.zero_grad()
    pred, gold, _, _ = model(src.cuda(), src_len, tgt.cuda())
    loss, _ = calculate_metrics(pred, gold, smoothing=0.1, loss_type="ce")
    loss.backward()
    torch.cuda.synchronize()
    return model, pred.detach().cpu(), float(loss.item()), {k: p.grad.detach().cpu() for k, p in model.named_parameters()}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_model_w_matches_oracle(precision):
    """Section 3.  Model W against oracle/asr_oracle.py from the same state_dict: logits, loss and every gradient, all .u.weight /
    .v.weight pairs included (PARITY UNPINNED: the oracle's proj is this repository's own restatement of the low-rank projection).
    The bounds are those of tests/test_gpu_lowrank.py test_lowrank_model_matches_oracle:
        fp32  logits 5e-5 max(1, max |logit|), loss 2e-5, gradient relative L2 worst 2e-3, median 2e-5
        bf16  logits 6e-2 max |logit|, loss 3e-2, gradient relative L2 median 6e-2, worst 0.25
    Where model W misses one of them the bound of THAT figure becomes 4 x a baseline (margin 4: summation order), computed then and
    printed beside the measured value: fp32 mode -- the error of the oracle evaluated in float32 against its own float64 on the same
    weights and batch; bf16 mode -- the error of the full-rank model of the same widths (the same flags without --rank) against its
    oracle on the same batch.
    Measured on an MI355X (max |logit| 4.50): model W meets every inherited bound, so no baseline was needed and none is computed --
        fp32  logits 2.96e-6, loss 4.5e-7, gradients worst 1.73e-4 (conv.0.weight), median 2.97e-7
        bf16  logits 3.33e-2 (bound 0.27), loss 3.3e-3, gradients median 6.6e-3, worst 0.128 (conv.0.weight)"""
    ref = _oracle(RANK)
    model, pred, loss, grads = _gpu_step(precision, RANK)
    names = [k for k in model.state_dict() if ".u.weight" in k]
    assert len(names) == 2 * (4 + 2) + 2 * (4 + 4 + 2) and model.encoder.layers[0].self_attn.query_linear.u.weight.shape == (RANK, 512)
    assert model.decoder.layers[1].pos_ffn.linear_1.v.weight.shape == (2048, RANK)
    e = _errors(pred, loss, grads, ref)
    amax = e["amax"]
    print("model W %s: logits max err %.3e (max |logit| %.2f), loss err %.2e, gradient rel L2 worst %s %.3e median %.3e"
          % (precision, e["logit"], amax, e["loss"], e["worst_name"], e["worst"], e["median"]))
    if precision == "fp32":
        inherited = {"logit": 5e-5 * max(1.0, amax), "loss": 2e-5, "worst": 2e-3, "median": 2e-5}
    else:
        inherited = {"logit": 6e-2 * amax, "loss": 3e-2, "worst": 0.25, "median": 6e-2}
    missed = [k for k in inherited if not e[k] <= inherited[k]]
    assert all(np.isfinite(e[k]) for k in inherited), e
    if missed:
        if precision == "fp32":
            r32 = _oracle(RANK, torch.float32)
            base = _errors(r32["pred"], r32["loss"], r32["grads"], ref)
        else:
            _, fpred, floss, fgrads = _gpu_step("bf16", 0)
            base = _errors(fpred, floss, fgrads, _oracle(0))
        for k in missed:
            print("model W %s: %s %.3e misses the inherited bound %.3e; baseline %.3e, margin 4 -> bound %.3e" % (precision, k, e[k], inherited[k], base[k], 4 * base[k]))
        for k in missed:
            assert e[k] <= 4 * base[k], (k, e[k], base[k], e["worst_name"] if k == "worst" else "")


def test_cross_kv_all_declines_factor_pairs():
    """Section 4.  functions.cross_kv_all (reached only with more than one decoder layer) stacks the layers' key / value WEIGHTS into one
    GEMM through the flat parameter layout; a factor pair has no such weight.  For model W's decoder it returns None, for the same flags
    without --rank it does not, and W's decoder output with functions._cross_kv_on off is bit-equal to that with it on."""
    from asr_hip import functions as F_
    from asr_hip import ops
    from utils.functions import init_optimizer
    got = {}
    for rank in (RANK, 0):
        args, model, V = _build_w("bf16", rank)
        model = model.cuda().train()
        init_optimizer(args, model, "noam")
        src, src_len, tgt = _batch(V)
        enc = torch.randn(3, 16, 512, generator=torch.Generator().manual_seed(1)).to(ops.compute_dtype()).to(D)
        assert len(model.decoder.layers) == 2
        got[rank] = F_.cross_kv_all(enc, model.decoder.layers)
        if rank:
            outs = []
            old = F_._cross_kv_on
            try:
                for on in (True, False):
                    F_._cross_kv_on = on
                    with torch.no_grad():
                        outs.append(model.decoder(tgt.cuda(), enc, torch.tensor([16, 12, 5], dtype=torch.int32))[0].float().cpu())
            finally:
                F_._cross_kv_on = old
            assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    assert got[RANK] is None
    assert got[0] is not None and len(got[0][0]) == 2 and tuple(got[0][0][0].shape) == (3, 16, 2 * 8 * 64)


# ---- section 5
STEP_LR = ["--k-lr", "1", "--warmup", "2"]      # Noam over model_size 5120: lr 4.9e-3, 9.9e-3, 8.1e-3 at steps 1, 2, 3 -- an e4m3 step of a
#                                                typical factor entry (0.04 under a row maximum of 0.2) is 3.6e-3


def _three_steps(precision, graphed, stale=False):
    """Three training steps of model W from its seeded state_dict -> (losses [3], the flat gradient of step 3, the e4m3 bytes of one
    factor as step 1 and as step 3 read it).  graphed: GraphedTrainStep(warmup_steps=1) = one eager step + the capture, then two
    replays; else the same step body (GraphedTrainStep._eager_step: the launches a capture records) issued eagerly three times."""
    from asr_hip import functions as F_
    from asr_hip import ops
    from asr_hip.graph import GraphedTrainStep
    from utils.functions import init_optimizer

    class EagerStep(GraphedTrainStep):
        def _capture(self):
            pass

        def _replay(self):
            self.loss, self.sums = self._eager_step()

    args, model, V = _build_w(precision, RANK, STEP_LR)
    src, src_len, tgt = _batch(V)
    model = model.cuda().train()
    opt = init_optimizer(args, model, "noam")
    factor = model.encoder.layers[1].pos_ffn.linear_1.u.weight
    real = F_._fp8_weight
    first = {}

    def first_for_ever(w):
        if id(w) not in first:
            first[id(w)] = real(w)
        return first[id(w)]

    if stale:
        F_._fp8_weight = first_for_ever
    try:
        assert ops.fp8_enabled() == (precision == "fp8")
        q1 = ops.quant_fp8(factor.data.view(RANK, -1))[0].clone()
        gs = (GraphedTrainStep if graphed else EagerStep)(model, opt, 0.1, src.cuda(), src_len, tgt.cuda(), warmup_steps=1, replay_after_capture=False)
        losses = [float(gs.warm[0].item())]
        losses.append(float(gs()[0].item()))
        q3 = ops.quant_fp8(factor.data.view(RANK, -1))[0].clone()
        losses.append(float(gs()[0].item()))
        torch.cuda.synchronize()
        assert opt._step == 3
        return losses, opt.optimizer.flat.grad.detach().double().cpu().clone(), (q1.cpu(), q3.cpu())
    finally:
        F_._fp8_weight = real
        ops.set_fp8(False)
        ops.reset_pending()


@pytest.mark.parametrize("precision", ["bf16", "fp8"])
def test_model_w_graph_replay_equals_eager(precision):
    """Section 5.  One eager step + two replays of the captured step against three eager steps from the same state_dict (--k-lr 1
    --warmup 2: every Adam step moves a weight by 5e-3 .. 1e-2, more than an e4m3 step; more than half of one factor's e4m3 bytes
    differ between the weights step 1 and step 3 read -- asserted).  The loss of each step and the flat gradient of step 3 must agree
    within 4 x the difference between two eager runs (atomics in the bias gradients), floor 1e-6 relative; both are printed.
    The eager steps are GraphedTrainStep._eager_step -- the very body a capture records (step_advance, zero_grad, forward, loss, backward,
    the device-side Noam / Adam launch) -- issued eagerly through a subclass that overrides the private _capture / _replay: that is what
    makes a 1e-6 bound meaningful, it ties this test to graph.py's internals, and it is NOT an independent loss.backward() + opt.step()
    loop (tests/test_gpu_graph.py test_graph_replay_equals_eager holds a replay against that loop, at its own tolerance).
    fp8: functions._fp8_weight keys its cache on a generation counter a replay cannot see; a replay is right only because the capture
    recorded the re-quantising launches.  Negative control: the eager sequence with _fp8_weight returning its first result per weight
    for ever -- what a replay without those launches would compute -- must leave the bound at step 3.
    Measured on an MI355X: two eager runs agree to the bit at this size (bounds = the 1e-6 floor), replay = eager to the bit in both
    modes, 86 % of the factor's bytes change, and the stale control's step-3 loss is 3.895 against 4.990 (0.22 relative)."""
    def rel(a, b):
        return abs(a - b) / max(abs(b), 1e-30)

    def grel(a, b):
        return float((a - b).norm() / b.norm().clamp_min(1e-30))

    e1, g1, (q1, q3) = _three_steps(precision, graphed=False)
    e2, g2, _ = _three_steps(precision, graphed=False)
    gr, gg, _ = _three_steps(precision, graphed=True)
    assert all(np.isfinite(v) for v in e1 + e2 + gr), (e1, e2, gr)
    assert float(g1.norm()) > 0 and float(gg.norm()) > 0          # (the step leaves its gradient in the flat buffer: something is compared)
    changed = float((q1[:, :512] != q3[:, :512]).float().mean())
    noise_l = max(rel(a, b) for a, b in zip(e2, e1))
    noise_g = grel(g2, g1)
    bound_l, bound_g = max(4 * noise_l, 1e-6), max(4 * noise_g, 1e-6)
    diff_l = [rel(a, b) for a, b in zip(gr, e1)]
    diff_g = grel(gg, g1)
    print("model W %s: losses eager %s, eager again %s, graph %s" % (precision, e1, e2, gr))
    print("model W %s: eager run-to-run loss %.3e gradient %.3e -> bounds %.3e / %.3e; graph vs eager loss %s gradient %.3e; e4m3 bytes "
          "of one factor changed between step 1 and step 3: %.3f" % (precision, noise_l, noise_g, bound_l, bound_g, ["%.3e" % d for d in diff_l], diff_g, changed))
    assert changed > 0.5, changed
    assert max(diff_l) <= bound_l, (diff_l, bound_l)
    assert diff_g <= bound_g, (diff_g, bound_g)
    if precision == "fp8":
        s, _, _ = _three_steps(precision, graphed=False, stale=True)
        print("model W fp8: stale quantised weights give losses %s: step 3 differs by %.3e (bound %.3e)" % (s, rel(s[2], e1[2]), bound_l))
        assert rel(s[2], e1[2]) > bound_l, "the learning rate is too small for a stale weight to show"
