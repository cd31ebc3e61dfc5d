"""Decision table of the linear backward in asr_hip/functions.py (_linear_bwd, _Fused.bwd, _out_proj_bwd) and the hand-over slot, on the
host: every ops / params function the ladder touches is a recorder on CPU tensors, no kernel runs.  The expectations restate the rules,
not the code:

  rung 1  defer_wgrad_now and gemm_tn_supported (and, with need_dx, a usable W and gemm_nn_supported): gemm_nn now, weight gradient queued;
          need_dx=False: queued only
  rung 2  need_dx, a usable W and gemm_nn_tn_supported: the one gemm_nn_tn launch
  rung 3  weight gradient (inside the fork when need_dx, else on the launching stream, no fork), then the data gradient, then join
          weight gradient: gemm_tn when supported, else transpose_padded(dy, db), transpose_padded(x), gemm_nt(accumulate, splits=0)
          data gradient:   gemm_nn when W is usable and supported, else gemm_nt against W^T (plain: params' shadow; fused: a fresh transpose)

A usable W is one whose row length is K (the per-weight shadow is column padded otherwise).  defer_wgrad_now is consulted first and once
(the output projection may consult it twice); gemm_nn_tn_supported only with need_dx, a usable W and rung 1 not taken."""
import itertools

import torch

M, N, K, TQ = 16, 72, 64, 8
BF = torch.bfloat16


class Stage:
    """Recorders in place of ops.* and params.*; operands are named by the storage they start at."""

    def __init__(self, monkeypatch, defer, tn, nn, nntn, padded=False, rowdot_pair=True):
        from asr_hip import functions as Fn
        self.Fn, self.log, self.asked, self.in_fork, self.names, self.keep = Fn, [], {"defer": 0, "nntn": 0}, False, {}, []
        t = self.tensor
        self.dy, self.x, self.out, self.mask = t("dy", M, N), t("x", M, K), t("out", M, K), t("mask", M, K)
        self.o, self.o32 = t("o", M, K), t("o32", M // TQ, TQ, K, dtype=torch.float32)
        self.W = t("W", N, K + 8 if padded else K)
        self.Wt = t("Wt_shadow", K, N)
        self.dw, self.db = t("dw", N, K, dtype=torch.float32), t("db", N, dtype=torch.float32)
        self.wparam, self.bparam = torch.nn.Parameter(torch.zeros(N, K)), torch.nn.Parameter(torch.zeros(N))
        grads = {id(self.wparam): self.dw, id(self.bparam): self.db}
        stage = self

        def asked(key, val):
            def f(*a, **k):
                self.asked[key] += 1
                return val
            return f

        def produce(kind, out):
            return out if out is not None else t(kind, M, K)

        def gemm_nn(dy, w, out=None, accumulate=False, relu_mask=None):
            self.rec("gemm_nn", dy, w, out, accumulate, relu_mask is not None)
            return produce("dx", out)

        def gemm_nn_tn(dy, w, x, dw, db=None, out=None, accumulate=False, relu_mask=None):
            self.rec("gemm_nn_tn", dy, w, x, dw, db, out, accumulate, relu_mask is not None)
            return produce("dx", out)

        def gemm_nt(A, B, out=None, accumulate=False, relu_mask=None, splits=1):
            self.rec("gemm_nt", A, B, out, accumulate, relu_mask is not None, splits)
            return produce("dx", out)

        def gemm_tn(dy, x, dw, colsum_acc=None, N=None, K=None):
            self.rec("gemm_tn", dy, x, dw, colsum_acc, N, K)

        def queue_wgrad(dy, x, dw, db, N, K):
            self.rec("queue_wgrad", dy, x, dw, db, N, K)

        def transpose_padded(x, colsum_acc=None):
            self.rec("transpose_padded", x, colsum_acc)
            return t("T(%s)" % self.name(x), x.shape[1], x.shape[0])

        def gemm_nn_rowdot(dy, w, o, o32, T):
            self.rec("gemm_nn_rowdot", dy, w, o, o32, T)
            return (t("dx_rowdot", M, K), t("delta", M // T, K // 64, T, dtype=torch.float32)) if rowdot_pair else None

        class fork:
            def __enter__(self):
                stage.rec("fork")
                stage.in_fork = True
                return self

            def __exit__(self, *exc):
                stage.in_fork = False
                return False

            def join(self):
                stage.rec("join")

        from asr_hip import ops, params
        for name, fn in (("defer_wgrad_now", asked("defer", defer)), ("gemm_nn_tn_supported", asked("nntn", nntn)),
                         ("gemm_tn_supported", lambda dy, x: tn), ("gemm_nn_supported", lambda dy, w: nn), ("gemm_nn", gemm_nn),
                         ("gemm_nn_tn", gemm_nn_tn), ("gemm_nt", gemm_nt), ("gemm_tn", gemm_tn), ("queue_wgrad", queue_wgrad),
                         ("transpose_padded", transpose_padded), ("gemm_nn_rowdot", gemm_nn_rowdot), ("fork", fork),
                         ("compute_dtype", lambda: BF)):
            monkeypatch.setattr(ops, name, fn)
        monkeypatch.setattr(params, "linear_weight", lambda p, dtype=None: self.W)
        monkeypatch.setattr(params, "linear_shadow", lambda p, dtype=None: (self.W, self.Wt))
        monkeypatch.setattr(params, "grad_of", lambda p: grads[id(p)])

    def tensor(self, name, *shape, dtype=BF):
        x = torch.zeros(*shape, dtype=dtype)
        self.keep.append(x)                       # alive to the end: no two names for one address
        self.names[x.data_ptr()] = name
        return x

    def name(self, v):
        return self.names[v.data_ptr()] if isinstance(v, torch.Tensor) else v

    def rec(self, call, *args):
        self.log.append((call,) + tuple(self.name(a) for a in args) + (self.in_fork,))

    def fused(self):
        f = object.__new__(self.Fn._Fused)        # two adjacent weights as one (N,K) view of the flat buffers
        f.ok, f.N, f.K, f.W, f.w_grad, f.b_grad = True, N, K, self.W, self.dw.view(-1), self.db
        return f


def wgrad_calls(tn, in_fork):
    if tn:
        return [("gemm_tn", "dy", "x", "dw", "db", N, K, in_fork)]
    return [("transpose_padded", "dy", "db", in_fork), ("transpose_padded", "x", None, in_fork),
            ("gemm_nt", "T(dy)", "T(x)", "dw", True, False, 0, in_fork)]


def expected(defer, tn, nn, nntn, need_dx, usable, out, acc, mask, fused):
    """-> (calls, name of the returned dx or None, times gemm_nn_tn_supported is consulted)"""
    queue = ("queue_wgrad", "dy", "x", "dw", "db", N, K, False)
    if not need_dx:
        return ([queue] if defer and tn else wgrad_calls(tn, False)), None, 0
    dx = out or "dx"
    if defer and tn and usable and nn:
        return [("gemm_nn", "dy", "W", out, acc, mask, False), queue], dx, 0
    if usable and nntn:
        return [("gemm_nn_tn", "dy", "W", "x", "dw", "db", out, acc, mask, False)], dx, 1
    if usable and nn:
        dgrad = [("gemm_nn", "dy", "W", out, acc, mask, False)]
    elif fused:
        dgrad = [("transpose_padded", "W", None, False), ("gemm_nt", "dy", "T(W)", out, acc, mask, 1, False)]
    else:
        dgrad = [("gemm_nt", "dy", "Wt_shadow", out, acc, mask, 1, False)]
    return [("fork", False)] + wgrad_calls(tn, True) + dgrad + [("join", False)], dx, 1 if usable else 0


FLAGS = list(itertools.product((True, False), repeat=4))           # defer_wgrad_now, gemm_tn_supported, gemm_nn_supported, gemm_nn_tn_supported


def test_plain_layer_walks_the_ladder(monkeypatch):
    for (defer, tn, nn, nntn), need_dx, with_mask, with_out, padded in itertools.product(FLAGS, *[(True, False)] * 4):
        row = dict(defer=defer, tn=tn, nn=nn, nntn=nntn, need_dx=need_dx, mask=with_mask, out=with_out, padded=padded)
        with monkeypatch.context() as mp:
            s = Stage(mp, defer, tn, nn, nntn, padded=padded)
            dx = s.Fn._linear_bwd(s.dy, s.x, s.wparam, s.bparam, dx_out=s.out if with_out else None, accumulate=with_out,
                                  need_dx=need_dx, relu_mask=s.mask if with_mask else None)
        calls, ret, n_nntn = expected(defer, tn, nn, nntn, need_dx, not padded, "out" if with_out else None, with_out, with_mask, False)
        assert s.log == calls, row
        assert s.name(dx) == ret, row
        assert s.asked == {"defer": 1, "nntn": n_nntn}, row


def test_fused_projections_walk_the_same_ladder(monkeypatch):
    for (defer, tn, nn, nntn), need_dx, with_out in itertools.product(FLAGS, *[(True, False)] * 2):
        row = dict(defer=defer, tn=tn, nn=nn, nntn=nntn, need_dx=need_dx, out=with_out)
        with monkeypatch.context() as mp:
            s = Stage(mp, defer, tn, nn, nntn)
            dx = s.fused().bwd(s.dy, s.x, dx_out=s.out if with_out else None, accumulate=with_out, need_dx=need_dx)
        calls, ret, n_nntn = expected(defer, tn, nn, nntn, need_dx, True, "out" if with_out else None, with_out, False, True)
        assert s.log == calls, row
        assert s.name(dx) == ret, row
        assert s.asked == {"defer": 1, "nntn": n_nntn}, row


def test_output_projection_takes_delta_from_rung_one(monkeypatch):
    for (defer, tn, nn, nntn), padded, dk, pair, with_o32 in itertools.product(FLAGS, (False, True), (64, 32), (True, False), (True, False)):
        row = dict(defer=defer, tn=tn, nn=nn, nntn=nntn, padded=padded, dk=dk, pair=pair, o32=with_o32)
        with monkeypatch.context() as mp:
            s = Stage(mp, defer, tn, nn, nntn, padded=padded, rowdot_pair=pair)
            s.x = s.o                                                  # the layer's input is the attention output
            dx, delta = s.Fn._out_proj_bwd(s.dy, s.o, s.o32 if with_o32 else None, s.wparam, s.bparam, TQ, dk)
        calls, ret, n_nntn = expected(defer, tn, nn, nntn, True, not padded, None, False, False, False)
        calls = [tuple({"x": "o", "T(x)": "T(o)"}.get(a, a) if isinstance(a, str) else a for a in c) for c in calls]
        if dk == 64 and defer and tn and nn and not padded:            # rung 1: the row-dot launch is tried in gemm_nn's place
            tried = ("gemm_nn_rowdot", "dy", "W", "o", "o32" if with_o32 else None, TQ, False)
            calls = [tried] + (calls[1:] if pair else calls)
            ret = "dx_rowdot" if pair else ret
        assert s.log == calls, row
        assert s.name(dx) == ret, row
        if ret == "dx_rowdot":
            assert s.name(delta) == "delta" and tuple(delta.shape) == (M // TQ, K // 64, TQ), row
        else:
            assert delta is None, row
        assert 1 <= s.asked["defer"] <= 2 and s.asked["nntn"] == n_nntn, row


def test_hand_over_slot():
    from asr_hip.functions import _Handover
    slot, box = _Handover(), {}
    out = torch.zeros(4, 6)
    slot.leave(out, out, box)
    assert slot[0] is not None
    assert slot.claim(out.view(24)) is box                             # the producer's output (any view of all of it)
    assert slot[0] is None and slot.claim(out) is None                 # a second claim finds the slot empty
    slot.leave(out, out, box)
    assert slot.claim(out[:2]) is None and slot[0] is None             # same address, another numel: not the output; the try empties the slot
    slot.leave(out, out, box)
    other = torch.zeros(4, 6)
    assert slot.claim(other) is None
    twin = torch.zeros(4, 6)
    slot.leave(twin, out, box)                                         # the output's storage outlives the output tensor itself
    del twin
    assert slot.claim(out) is None                                     # the producer's output died: its memory may have been recycled
    slot.leave(out, out, box)
    slot.clear()
    assert slot[0] is None and slot.claim(out) is None
