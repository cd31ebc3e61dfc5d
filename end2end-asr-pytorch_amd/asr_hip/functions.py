"""torch.autograd glue: one Function per fused sub-layer of the reference model.  Each forward/backward is a fixed
sequence of launches into libasr_hip.so; parameter gradients are ACCUMULATED in place into the fp32 buffers returned
by params.grad_of() (so the Functions return None for them) and reported to the DDP reducer with params.grad_ready().

Sub-layer -> reference code
  MHAFn      models/common_layers.py:170-200 (+ :211-225) and the `*= non_pad_mask` that follows every call
  RopeFn     (no reference code: rotary position embedding, --pos-encoding rope; MHAFn applies it through cfg["rope"])
  FFNFn      models/common_layers.py:135-142 (+ mask)
  ConvModuleFn  (no reference code: the Conformer convolution module of --conv-module-kernel)
  EncInFn    models/asr/transformer.py:172-173
  EmbedFn    models/asr/transformer.py:292-293
  LinearFn   models/asr/transformer.py:302 (output_linear) and any plain nn.Linear
  VGGFn      models/asr/transformer.py:42-53, :70-76
  EmbCNNFn   models/asr/transformer.py:33-40, :70-76
  CEFn       utils/metrics.py:102-132
  RnntJointFn, RnntFn  (no reference code: the transducer head of --transducer-weight)
  RnntSimpleFn, RnntJointPrunedFn, RnntPrunedFn  (no reference code: pruned transducer training, --transducer-prune-range)
"""
import collections
import functools
import os
import weakref

import torch
from torch.autograd import Function

from . import ops
from . import params as P


def _as_compute(dy2d):
    """(M,N) gradient in any float dtype -> (M,Np) zero padded copy in the compute dtype (contiguous rows).  Np = N rounded up
    to 64: the data-gradient kernel contracts N in stages of 64 and relies on the zero columns (vocabulary projection: 4364)."""
    cd = ops.compute_dtype()
    if dy2d.dtype == torch.float32 and cd != torch.float32:
        return ops.cast_and_transpose(dy2d, cd, want_t=False, pad=64)[0]
    if dy2d.dtype != cd:
        dy2d = dy2d.to(cd)
    return _pad_cols(dy2d, 64)


def _pad_cols(x2d, pad=8):
    """(M,K) -> itself if rows are contiguous and K is already padded, else a zero padded copy (M, pad(K))."""
    K = x2d.shape[1]
    Kp = (K + pad - 1) // pad * pad
    if K == Kp and x2d.is_contiguous():
        return x2d
    out = torch.zeros((x2d.shape[0], Kp), device=x2d.device, dtype=x2d.dtype)
    out[:, :K].copy_(x2d)
    return out


def _linear_fwd(x2d, wparam, bparam, relu=False, out_dtype=None):
    W = P.linear_weight(wparam)
    xp = _pad_cols(x2d) if W.shape[1] != x2d.shape[1] or not x2d.is_contiguous() else x2d
    return ops.gemm_nt(xp, W, bias=bparam.data if bparam is not None else None, relu=relu, out_dtype=out_dtype)


# A linear layer as its backward sees it.  W: the weight in the compute dtype and natural (N,K) layout, or None where the NN kernels
# cannot read it (the per-weight shadow is column padded when K is not a whole number of 16-byte chunks; nobody asked for dX);
# wt(): W^T for the NT fallback; dw (N,K) / db (N) or None: the fp32 gradient buffers the launches accumulate into.
_Lin = collections.namedtuple("_Lin", "W wt dw db N K")


def _plain_lin(wparam, bparam, need_dx=True):
    N, K = wparam.shape[0], wparam.numel() // wparam.shape[0]
    W = P.linear_weight(wparam) if need_dx else None
    return _Lin(W if W is not None and W.shape[1] == K else None, lambda: P.linear_shadow(wparam)[1],
                P.grad_of(wparam).view(N, K), P.grad_of(bparam) if bparam is not None else None, N, K)


def _wgrad_bias(lin, dy2d, x2d):
    """dW (N,K) += dy^T x and db (N) += column sums of dy, both accumulated in place into the fp32 gradient buffers.
    Fast path: transpose-free TN kernel (natural layouts, bias gradient fused).  Fallback (rows not a multiple of the
    kernel's stage, odd strides): explicit zero padded transposes + the NT kernel."""
    if ops.gemm_tn_supported(dy2d, x2d):
        ops.gemm_tn(dy2d, x2d, lin.dw, colsum_acc=lin.db, N=lin.N, K=lin.K)
        return
    dy_t = ops.transpose_padded(dy2d[:, :lin.N], lin.db)
    x_t = ops.transpose_padded(x2d[:, :lin.K])
    ops.gemm_nt(dy_t, x_t, out=lin.dw, accumulate=True, splits=0)      # 0 = let the library choose split-K


def _lin_bwd(lin, dy2d, x2d, dx_out=None, accumulate=False, need_dx=True, relu_mask=None, dgrad_now=None):
    """THE linear backward: dy2d (M,N[p]) and x2d (M,K) in the compute dtype.  Accumulates dW / db, returns dx (M,K) (+)= dy W or None.
    Four rungs, the first that applies: (1) data gradient now, weight gradient queued for the grouped launch; (2) dX and dW
    workgroups in ONE launch; (3) dW / db on the second stream next to dX on this one; the transposing fallbacks inside (3).
    dgrad_now(W), when given, is tried in place of rung 1's data-gradient launch and its result returned for dx (None from it:
    the plain launch runs, the walk goes on from there)."""
    W = lin.W
    defer = ops.defer_wgrad_now(dy2d.dtype) and ops.gemm_tn_supported(dy2d, x2d) and x2d.dtype == dy2d.dtype
    nn_ok = need_dx and W is not None and ops.gemm_nn_supported(dy2d, W)
    if defer and (nn_ok or not need_dx):
        # data gradient now (it is what the rest of backward waits for), weight gradient with the other layers' at the end
        dx = None
        if need_dx:
            dx = dgrad_now(W) if dgrad_now is not None else None
            if dx is None:
                dx = ops.gemm_nn(dy2d, W, out=dx_out, accumulate=accumulate, relu_mask=relu_mask)
        ops.queue_wgrad(dy2d, x2d, lin.dw, lin.db, lin.N, lin.K)
        return dx
    if not need_dx:
        _wgrad_bias(lin, dy2d, x2d)
        return None
    if W is not None and ops.gemm_nn_tn_supported(dy2d, W, x2d):      # graph capture, bf16: dX and dW workgroups in ONE launch
        return ops.gemm_nn_tn(dy2d, W, x2d, lin.dw, lin.db, out=dx_out, accumulate=accumulate, relu_mask=relu_mask)
    f = ops.fork()
    with f:                                   # dW / db on the second stream, next to dX on this one
        _wgrad_bias(lin, dy2d, x2d)
    if nn_ok:                                 # natural-layout weight + transposing LDS reads when the shape allows, else the NT kernel on W^T
        dx = ops.gemm_nn(dy2d, W, out=dx_out, accumulate=accumulate, relu_mask=relu_mask)
    else:
        dx = ops.gemm_nt(_pad_cols(dy2d), lin.wt(), out=dx_out, accumulate=accumulate, relu_mask=relu_mask)
    f.join()
    return dx


def _linear_bwd(dy2d, x2d, wparam, bparam, dx_out=None, accumulate=False, need_dx=True, relu_mask=None):
    """_lin_bwd of a plain layer: the weight's shadows and gradient buffers come from params."""
    return _lin_bwd(_plain_lin(wparam, bparam, need_dx), dy2d, x2d, dx_out, accumulate, need_dx, relu_mask)


# The output projection's data gradient IS the attention backward's dO: its epilogue also writes delta = rowsum(dO * O) per head
# (asr_gemm_nn_rowdot), one dependent launch less per attention block (where the library refuses the shape, asr_attn_bwd computes delta
# itself: the form tests/test_gpu_ops.py holds the epilogue against).


def _out_proj_bwd(dy2d, o2d, o32, wparam, bparam, Tq, dk):
    """(dO, delta or None) for MHAFn.backward: _linear_bwd of the output projection, with delta from the same launch where possible."""
    lin = _plain_lin(wparam, bparam)
    o32 = o32.view(-1, lin.K) if o32 is not None else None
    got = _lin_bwd(lin, dy2d, o2d, dgrad_now=(lambda W: ops.gemm_nn_rowdot(dy2d, W, o2d, o32, Tq)) if dk == 64 else None)
    return (got[0], got[1].view(-1, lin.K // 64, Tq)) if isinstance(got, tuple) else (got, None)


class _Fused:
    """Several projections that read the same input, run as ONE GEMM because their weights (and biases) are adjacent in
    the flat parameter buffers (FusedAdam lays Q/K/V out that way).  Duck-types the few things the helpers need."""

    def __init__(self, weights, biases):
        fw, fb = P.fused(weights), P.fused(biases)
        self.ok = fw is not None and fb is not None and ops.compute_dtype() in (torch.float32, torch.bfloat16)
        if not self.ok:
            return
        self.N = sum(w.shape[0] for w in weights)
        self.K = weights[0].shape[1]
        self.ok = self.K % 8 == 0
        if not self.ok:
            return
        self.w_master, self.w_grad, flat, off = fw
        self.b_master, self.b_grad = fb[0], fb[1]
        cd = ops.compute_dtype()
        if cd == torch.float32:
            self.W = self.w_master.view(self.N, self.K)
        else:
            flat.shadow_view(weights[0], off, cd)                       # make sure the flat shadow is fresh
            self.W = flat._shadow[cd][0][off:off + self.N * self.K].view(self.N, self.K)

    def fwd(self, x2d):
        return ops.gemm_nt(x2d, self.W, bias=self.b_master)

    def bwd(self, dy2d, x2d, dx_out=None, accumulate=False, need_dx=True):
        lin = _Lin(self.W, lambda: ops.transpose_padded(self.W), self.w_grad.view(self.N, self.K), self.b_grad, self.N, self.K)
        return _lin_bwd(lin, dy2d, x2d, dx_out, accumulate, need_dx)


# ================================================================================================ plain linear
class _Handover:
    """One slot through which a producer's forward leaves a box for the consumer of its output: (weakref to the output, the
    data_ptr and numel of its storage, the box).  The claim is made at FORWARD time and empties the slot: the association is by a
    live weak reference to the producer's output tensor (while it is alive its memory cannot have been recycled) plus address and
    size, never by an address alone, and it cannot outlive the forward that made it.  (slot[0] reads the slot.)"""

    def __init__(self):
        self.slot = None

    def __getitem__(self, i):
        return (self.slot,)[i]

    def leave(self, out, storage, box):
        self.slot = (weakref.ref(out), storage.data_ptr(), storage.numel(), box)

    def clear(self):
        self.slot = None

    def claim(self, tensor):
        """The box left by the forward that produced `tensor` (or a view of all of it), or None."""
        slot, self.slot = self.slot, None
        if slot is None or slot[0]() is None:
            return None
        return slot[3] if (slot[1] == tensor.data_ptr() and slot[2] == tensor.numel()) else None


_logit_handover = _Handover()         # LinearFn (the latest fp32 logits) -> CEFn.forward
_logit_handover_on = os.environ.get("ASR_LOGIT_HANDOVER", "1") != "0"


_grad_mode = [False]      # torch.is_grad_enabled() at the call site of the running LinearFn (inside Function.forward it always reads False)


def linear(x, weight, bias, out_fp32=False, mark_ready=True):
    """LinearFn.apply with the caller's grad mode recorded: under torch.no_grad() no hand-over slot is left behind."""
    _grad_mode[0] = torch.is_grad_enabled()
    try:
        return LinearFn.apply(x, weight, bias, out_fp32, mark_ready)
    finally:
        _grad_mode[0] = False


class LinearFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, out_fp32, mark_ready):
        cd = ops.compute_dtype()
        x2 = x.reshape(-1, x.shape[-1])
        if x2.dtype != cd:
            x2 = x2.to(cd)
        y = _linear_fwd(x2, weight, bias, out_dtype=torch.float32 if out_fp32 else None)
        ctx.x2 = x2
        ctx.weight, ctx.bias, ctx.mark_ready = weight, bias, mark_ready
        ctx.in_shape = x.shape
        ctx.need_dx = x.requires_grad
        ctx.box = None
        out = y.view(*x.shape[:-1], weight.shape[0])
        _logit_handover.clear()                # one slot, and only for the forward that has just run (never across a no_grad forward)
        if out_fp32 and cd == torch.bfloat16 and _logit_handover_on and _grad_mode[0] and any(ctx.needs_input_grad):
            # fp32 logits of a bf16 model (the vocabulary projection): the loss's backward may leave ITS part of the gradient in the
            # compute dtype, zero padded to the data-gradient kernel's stage, in this box instead of an fp32 tensor that would be cast
            # and padded here (CEFn claims the box in its forward)
            ctx.box = {}
            _logit_handover.leave(out, y, ctx.box)
        return out

    @staticmethod
    def backward(ctx, dy):
        N = ctx.weight.shape[0]
        dy_c = ctx.box.pop("dy", None) if ctx.box is not None else None
        if dy_c is None:
            dy_c = _as_compute(dy.reshape(-1, N))
        elif dy is not None and any(st != 0 for st in dy.stride()):
            # the logits had a second differentiable consumer (an auxiliary loss, a regulariser): autograd has summed its gradient with
            # the loss's stride-0 zero placeholder into a dense tensor -- add it to the handed-over part instead of dropping it
            dy_c = dy_c + _as_compute(dy.reshape(-1, N))
        dx = _linear_bwd(dy_c, ctx.x2, ctx.weight, ctx.bias, need_dx=ctx.need_dx)
        if ctx.mark_ready:
            P.grad_ready(*[p for p in (ctx.weight, ctx.bias) if p is not None])
        if dx is not None:
            dx = dx.view(ctx.in_shape)
        return dx, None, None, None, None


# ================================================================================================ encoder output fan-out
class FanOutFn(Function):
    """The encoder output feeds the cross-attention of EVERY decoder layer (reference: transformer.py:296-299).  Autograd
    would sum the per-layer gradients with one elementwise add per layer; here the layers' backward GEMMs accumulate into
    ONE buffer (`box['buf']`: the first to run allocates it, the others use the GEMM's accumulate epilogue, MHAFn.backward)
    and this node hands that buffer on."""

    @staticmethod
    def forward(ctx, x, n, box):
        ctx.box = box
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        g = ctx.box.pop("buf", None)
        for x in grads:                      # layers that did not use the shared buffer (un-fused K/V projections)
            if x is not None:
                g = x if g is None else g + x
        return g, None, None


# ================================================================================================ cross-attention K | V of all layers
_cross_kv_on = os.environ.get("ASR_CROSS_KV", "1") != "0"        # (test arm: tests/test_gpu_model.py holds the one-GEMM form against the per-layer one)


class CrossKVFn(Function):
    """K | V projections of the encoder output for EVERY decoder layer as one GEMM (reference: transformer.py:296-299 calls each layer's
    encoder_attn on the same encoder output; common_layers.py:181-187 projects it per layer).  The layers' weights (k0 v0 k1 v1 ...) and
    biases are adjacent in the flat parameter buffers (FusedAdam._slot_order), so the stacked (L 2 H dk, D) weight is a view.
    forward -> L views (B, Tk, 2 H dk) of one (B, Tk, L 2 H dk) tensor.  backward: the layers' attention backward kernels have written
    dK | dV into box['dkv'] (the same layout) and returned no gradient for their views; here ONE data-gradient GEMM (contraction over all
    layers: a single rounding of the sum the per-layer form rounded L times) and ONE weight-gradient problem."""

    @staticmethod
    def forward(ctx, enc, box, n_layers, *params):
        ws, bs = list(params[:2 * n_layers]), list(params[2 * n_layers:])
        fused = _Fused(ws, bs)
        assert fused.ok
        B, Tk, D = enc.shape
        kv2 = enc.reshape(B * Tk, D).contiguous()
        kv_all = fused.fwd(kv2).view(B, Tk, fused.N)
        w = fused.N // n_layers
        ctx.fused, ctx.box, ctx.kv2, ctx.shape, ctx.params = fused, box, kv2, (B, Tk, D), tuple(params)
        ctx.set_materialize_grads(False)
        return tuple(kv_all[:, :, l * w:(l + 1) * w] for l in range(n_layers))

    @staticmethod
    def backward(ctx, *grads):
        B, Tk, D = ctx.shape
        assert all(g is None for g in grads), "a consumer of the stacked K | V returned a gradient instead of writing box['dkv']"
        dkv = ctx.box.pop("dkv", None)
        assert dkv is not None and ctx.box.pop("written", 0) == len(grads), "not every decoder layer wrote its dK | dV"
        d_enc = ctx.fused.bwd(dkv.view(B * Tk, ctx.fused.N), ctx.kv2, need_dx=ctx.needs_input_grad[0])
        P.grad_ready(*ctx.params)
        return (None if d_enc is None else d_enc.view(B, Tk, D), None, None) + (None,) * len(ctx.params)


def cross_kv_all(enc_out, layers):
    """-> (per-layer K | V views, gradient box) when every layer's cross-attention block can take them, else None (per-layer projections)."""
    if not _cross_kv_on or not enc_out.is_cuda or not all(hasattr(l, "encoder_attn") for l in layers):
        return None
    eas = [l.encoder_attn for l in layers]
    # plain projections only (the low-rank blocks' key_linear / value_linear are factor pairs)
    if not all(isinstance(getattr(ea, "key_linear", None), torch.nn.Linear) and isinstance(getattr(ea, "value_linear", None), torch.nn.Linear)
               and hasattr(ea, "dim_key") for ea in eas):
        return None
    if any(ea.dim_key != ea.dim_value or ea.dim_key not in (16, 32, 64) for ea in eas):
        return None
    ws = [w for ea in eas for w in (ea.key_linear.weight, ea.value_linear.weight)]
    bs = [b for ea in eas for b in (ea.key_linear.bias, ea.value_linear.bias)]
    if not _Fused(ws, bs).ok:
        return None
    x = enc_out if enc_out.dtype == ops.compute_dtype() else enc_out.to(ops.compute_dtype())
    box = {"n_layers": len(layers)}
    return CrossKVFn.apply(x, box, len(layers), *ws, *bs), box


# ================================================================================================ attention sub-layer
class MHAFn(Function):
    @staticmethod
    def forward(ctx, q_in, kv_in, Wq, bq, Wk, bk, Wv, bv, Wo, bo, gamma, beta, cfg, kv_pre=None):
        H, dk = cfg["H"], cfg["dk"]
        HD = H * dk
        B, Tq, D = q_in.shape
        self_attn = kv_in is None
        kv = q_in if self_attn else kv_in
        Tk = kv.shape[1]
        q2 = q_in.reshape(B * Tq, D).contiguous()
        kv2 = None if kv_pre is not None else kv.reshape(B * Tk, D).contiguous()
        # one GEMM for Q|K|V (self attention) or K|V (cross attention) when the flat layout allows it
        fused = None if kv_pre is not None else (_Fused([Wq, Wk, Wv], [bq, bk, bv]) if self_attn else _Fused([Wk, Wv], [bk, bv]))
        if kv_pre is not None:             # cross attention, K | V projected for all layers at once (CrossKVFn)
            Q = _linear_fwd(q2, Wq, bq).view(B, Tq, HD)
            K, V = kv_pre[:, :, :HD], kv_pre[:, :, HD:]
        elif fused.ok and self_attn:
            qkv = fused.fwd(q2).view(B, Tq, 3 * HD)
            Q, K, V = qkv[:, :, :HD], qkv[:, :, HD:2 * HD], qkv[:, :, 2 * HD:]
        elif fused.ok:
            Q = _linear_fwd(q2, Wq, bq).view(B, Tq, HD)
            kvp = fused.fwd(kv2).view(B, Tk, 2 * HD)
            K, V = kvp[:, :, :HD], kvp[:, :, HD:]
        else:
            Q = _linear_fwd(q2, Wq, bq).view(B, Tq, HD)
            K = _linear_fwd(kv2, Wk, bk).view(B, Tk, HD)
            V = _linear_fwd(kv2, Wv, bv).view(B, Tk, HD)
        rope = cfg.get("rope")
        if rope is not None:               # rotary position embedding (csrc/rope.hip): Q and K in place, V untouched; ctx keeps the rotated ones
            if not self_attn or kv_pre is not None:
                raise ValueError("cfg['rope'] is for self-attention only (kv_in is None, no kv_pre)")
            if fused.ok:
                ops.rope_(qkv[:, :, :2 * HD], rope, 2 * H, dk)
            else:
                ops.rope_(Q, rope, H, dk)
                ops.rope_(K, rope, H, dk)
        p_att = cfg["p"]
        seed_a, seed_o = P.next_seed(), P.next_seed()
        scale = 1.0 / (dk ** 0.5)
        # bf16 storage + backward coming: keep an un-rounded fp32 copy of the attention output for delta = rowsum(dO * O)
        O32 = None
        if Q.dtype != torch.float32 and any(ctx.needs_input_grad):
            O32 = torch.empty((B, Tq, HD), device=Q.device, dtype=torch.float32)
        O, lse, attn = ops.attn_fwd(Q, K, V, H, dk, key_len=cfg.get("key_len"), key_pad=cfg.get("key_pad"),
                                    causal=cfg.get("causal", False), scale=scale, p=p_att, seed=seed_a,
                                    want_attn=cfg.get("want_attn", False), o32=O32)
        # (output projection, then dropout + residual + LayerNorm + row mask: the one-launch form lost -- 50 - 100 workgroups of whole rows on
        # 256 CUs, profiles/r03_gemm_ln_ab.txt -- and was removed in round 4)
        Y = _linear_fwd(O.view(B * Tq, HD), Wo, bo)
        out, mean, rstd = ops.add_ln_fwd(Y, q2, gamma.data, beta.data, row_keep=cfg.get("row_keep"), p=p_att, seed=seed_o)
        ctx.cfg, ctx.self_attn, ctx.fused = cfg, self_attn, fused
        ctx.seeds = (seed_a, seed_o)
        ctx.scale = scale
        ctx.t = (q2, kv2, Q, K, V, O, lse, Y, mean, rstd, O32)      # Y now holds z
        ctx.params = (Wq, bq, Wk, bk, Wv, bv, Wo, bo, gamma, beta)
        ctx.shape = (B, Tq, Tk, D)
        ctx.kv_pre = kv_pre is not None
        ctx.kv_pre_width = kv_pre.shape[2] if kv_pre is not None else 0
        ctx.need_dkv = (not self_attn) and kv_pre is None and kv_in.requires_grad
        out = out.view(B, Tq, D)
        if attn is not None:
            ctx.mark_non_differentiable(attn)
            return out, attn
        return out

    @staticmethod
    def backward(ctx, dout, *unused):
        cfg, fused = ctx.cfg, ctx.fused
        H, dk = cfg["H"], cfg["dk"]
        HD = H * dk
        B, Tq, Tk, D = ctx.shape
        q2, kv2, Q, K, V, O, lse, Z, mean, rstd, O32 = ctx.t
        Wq, bq, Wk, bk, Wv, bv, Wo, bo, gamma, beta = ctx.params
        seed_a, seed_o = ctx.seeds
        dout2 = dout.reshape(B * Tq, D).contiguous()
        d_res, d_y = ops.add_ln_bwd(dout2, Z, mean, rstd, gamma.data, cfg.get("row_keep"), P.grad_of(gamma),
                                    P.grad_of(beta), p=cfg["p"], seed=seed_o)
        dO, delta = _out_proj_bwd(d_y, O.view(B * Tq, HD), O32, Wo, bo, Tq, dk)
        # gradient buffers mirror the forward layout so that the fused projections see one contiguous (M, 2|3*HD) operand
        if ctx.kv_pre:
            # this layer's dK | dV go straight into the stacked (B, Tk, L 2 HD) buffer CrossKVFn.backward contracts (the first layer to run
            # -- the last of the decoder -- allocates it; every layer writes its whole slice)
            box, li = cfg["kv_pre_box"], cfg["kv_pre_layer"]
            buf = box.get("dkv")
            if buf is None:
                buf = torch.empty((B, Tk, box["n_layers"] * 2 * HD), device=dout.device, dtype=Q.dtype)
                box["dkv"] = buf
            dQ = torch.empty((B, Tq, HD), device=dout.device, dtype=Q.dtype)
            dK, dV = buf[:, :, li * 2 * HD:li * 2 * HD + HD], buf[:, :, li * 2 * HD + HD:(li + 1) * 2 * HD]
        elif fused.ok and ctx.self_attn:
            dqkv = torch.empty((B, Tq, 3 * HD), device=dout.device, dtype=Q.dtype)
            dQ, dK, dV = dqkv[:, :, :HD], dqkv[:, :, HD:2 * HD], dqkv[:, :, 2 * HD:]
        elif fused.ok:
            dQ = torch.empty((B, Tq, HD), device=dout.device, dtype=Q.dtype)
            dkv = torch.empty((B, Tk, 2 * HD), device=dout.device, dtype=Q.dtype)
            dK, dV = dkv[:, :, :HD], dkv[:, :, HD:]
        else:
            dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
        ops.attn_bwd(Q, K, V, O, dO.view(B, Tq, HD), lse, H, dk, key_len=cfg.get("key_len"), key_pad=cfg.get("key_pad"),
                     causal=cfg.get("causal", False), scale=ctx.scale, p=cfg["p"], seed=seed_a, out=(dQ, dK, dV), o32=O32, delta=delta)
        d_kv = None
        rope = cfg.get("rope")
        if rope is not None:               # dQ and dK are gradients of the rotated Q and K: the transposed rotation takes them back
            if fused.ok:
                ops.rope_(dqkv[:, :, :2 * HD], rope, 2 * H, dk, inverse=True)
            else:
                ops.rope_(dQ, rope, H, dk, inverse=True)
                ops.rope_(dK, rope, H, dk, inverse=True)
        # dq_in = d_res + dQ.Wq (+ dK.Wk + dV.Wv for self attention): accumulated straight into d_res
        if ctx.kv_pre:
            _linear_bwd(dQ.view(B * Tq, HD), q2, Wq, bq, dx_out=d_res, accumulate=True)
            cfg["kv_pre_box"]["written"] = cfg["kv_pre_box"].get("written", 0) + 1
            P.grad_ready(Wq, bq, Wo, bo, gamma, beta)           # (Wk, bk, Wv, bv: CrossKVFn.backward, after the last layer)
            return (d_res.view(B, Tq, D), None) + (None,) * 12
        if fused.ok and ctx.self_attn:
            fused.bwd(dqkv.view(B * Tq, 3 * HD), q2, dx_out=d_res, accumulate=True)
        elif fused.ok:
            _linear_bwd(dQ.view(B * Tq, HD), q2, Wq, bq, dx_out=d_res, accumulate=True)
            box = cfg.get("kv_grad_box") if ctx.need_dkv else None
            if box is not None and box.get("buf") is not None:     # a later decoder layer already produced d(enc_out)
                fused.bwd(dkv.view(B * Tk, 2 * HD), kv2, dx_out=box["buf"].view(B * Tk, D), accumulate=True)
            else:
                d_kv = fused.bwd(dkv.view(B * Tk, 2 * HD), kv2, need_dx=ctx.need_dkv)
                if box is not None:
                    box["buf"] = d_kv.view(B, Tk, D)
                    d_kv = None
        else:
            dQ2, dK2, dV2 = dQ.view(B * Tq, HD), dK.view(B * Tk, HD), dV.view(B * Tk, HD)
            _linear_bwd(dQ2, q2, Wq, bq, dx_out=d_res, accumulate=True)
            if ctx.self_attn:
                _linear_bwd(dK2, q2, Wk, bk, dx_out=d_res, accumulate=True)
                _linear_bwd(dV2, q2, Wv, bv, dx_out=d_res, accumulate=True)
            else:
                d_kv = _linear_bwd(dK2, kv2, Wk, bk, need_dx=ctx.need_dkv)
                _linear_bwd(dV2, kv2, Wv, bv, dx_out=d_kv, accumulate=True, need_dx=ctx.need_dkv)
        if d_kv is not None:
            d_kv = d_kv.view(B, Tk, D)
        P.grad_ready(*ctx.params)
        return (d_res.view(B, Tq, D), d_kv) + (None,) * 12


# ================================================================================================ rotary position embedding
class RopeFn(Function):
    """RopeFn.apply(x, cs, nheads, d) -> x (B, T, nheads d) rotated by the table cs (T, d/2, 2), out of place (ops.rope_ on a clone); the
    gradient is the transposed rotation of the incoming one.  MHAFn rotates its own Q and K in place (cfg["rope"]); this is for callers
    outside it."""

    @staticmethod
    def forward(ctx, x, cs, nheads, d):
        ctx.cs, ctx.nheads, ctx.d = cs, nheads, d
        return ops.rope_(x.clone(), cs, nheads, d)

    @staticmethod
    def backward(ctx, dy):
        return ops.rope_(dy.clone(), ctx.cs, ctx.nheads, ctx.d, inverse=True), None, None, None


# ================================================================================================ feed-forward sub-layer
# Debug tap: set to a list and every forward appends the tensors holding its discrete selections (ReLU outputs, pooled
# activations) in call order: FFN hidden activations, and for vgg_cnn (y1, y2, y3, y4).  Parity tests evaluate their fp64
# restatement's gradient under the SAME selections (tests/test_gpu_baseline_shapes.py); never set on the training path.
capture_selections = None


class FFNFn(Function):
    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, gamma, beta, cfg):
        B, T, D = x.shape
        x2 = x.reshape(B * T, D).contiguous()
        h = _linear_fwd(x2, W1, b1, relu=True)
        if capture_selections is not None:
            capture_selections.append(("ffn", h))
        y = _linear_fwd(h, W2, b2)
        seed = P.next_seed()
        out, mean, rstd = ops.add_ln_fwd(y, x2, gamma.data, beta.data, row_keep=cfg.get("row_keep"), p=cfg["p"], seed=seed)
        ctx.t = (x2, h, y, mean, rstd)
        ctx.params = (W1, b1, W2, b2, gamma, beta)
        ctx.cfg, ctx.seed, ctx.shape = cfg, seed, (B, T, D)
        return out.view(B, T, D)

    @staticmethod
    def backward(ctx, dout):
        B, T, D = ctx.shape
        x2, h, z, mean, rstd = ctx.t
        W1, b1, W2, b2, gamma, beta = ctx.params
        cfg = ctx.cfg
        dout2 = dout.reshape(B * T, D).contiguous()
        d_res, d_y = ops.add_ln_bwd(dout2, z, mean, rstd, gamma.data, cfg.get("row_keep"), P.grad_of(gamma),
                                    P.grad_of(beta), p=cfg["p"], seed=ctx.seed)
        # dh = (d_y . W2) * (h > 0)   -- ReLU mask fused into the dgrad epilogue
        dh = _linear_bwd(d_y, h, W2, b2, relu_mask=h)
        _linear_bwd(dh, x2, W1, b1, dx_out=d_res, accumulate=True)
        P.grad_ready(*ctx.params)
        return (d_res.view(B, T, D),) + (None,) * 7


# ================================================================================================ convolution module
class ConvModuleFn(Function):
    """LN(dropout(W2 swish(dwconv(glu(W1 x)))) + x) * row_keep (csrc/convmod.hip has the definition): the two
    pointwise layers on the linear path of every other sub-layer, the three launches of the module between them, FFNFn's epilogue."""

    @staticmethod
    def forward(ctx, x, W1, b1, wd, bd, W2, b2, gamma, beta, cfg):
        B, T, D = x.shape
        K = wd.shape[-1]
        lens = cfg["key_len"]
        x2 = x.reshape(B * T, D).contiguous()
        u = _linear_fwd(x2, W1, b1)
        s, v = ops.convmod_fwd(u, wd.data, bd.data, lens, B, T, D, K)
        y = _linear_fwd(v, W2, b2)
        seed = P.next_seed()
        out, mean, rstd = ops.add_ln_fwd(y, x2, gamma.data, beta.data, row_keep=cfg.get("row_keep"), p=cfg["p"], seed=seed)
        ctx.t = (x2, u, s, v, y, mean, rstd, lens)
        ctx.params = (W1, b1, wd, bd, W2, b2, gamma, beta)
        ctx.cfg, ctx.seed, ctx.shape = cfg, seed, (B, T, D, K)
        return out.view(B, T, D)

    @staticmethod
    def backward(ctx, dout):
        B, T, D, K = ctx.shape
        x2, u, s, v, z, mean, rstd, lens = ctx.t
        W1, b1, wd, bd, W2, b2, gamma, beta = ctx.params
        cfg = ctx.cfg
        dout2 = dout.reshape(B * T, D).contiguous()
        d_res, d_y = ops.add_ln_bwd(dout2, z, mean, rstd, gamma.data, cfg.get("row_keep"), P.grad_of(gamma),
                                    P.grad_of(beta), p=cfg["p"], seed=ctx.seed)
        dv = _linear_bwd(d_y, v, W2, b2)
        ops.convmod_bwd_weight(dv, s, u, lens, B, T, D, K, P.grad_of(wd), P.grad_of(bd))
        du = ops.convmod_bwd_data(dv, s, u, wd.data, lens, B, T, D, K)
        _linear_bwd(du, x2, W1, b1, dx_out=d_res, accumulate=True)
        P.grad_ready(*ctx.params)
        return (d_res.view(B, T, D),) + (None,) * 9


# ================================================================================================ encoder input
# Hand-over between the conv front end and the encoder input projection (round 6).  The second max-pool's backward used to be a launch of
# its own between the projection's data gradient and conv.7's backward (asr_maxpool_bwd_code: 58 us, 65 MB written by the GEMM, read
# back with 33 MB of selection bytes, 262 MB written).  When VGGFn.forward produced its selection bytes channel last it leaves a slot
# here; EncInFn.forward claims it if the features it is given ARE that output (_Handover), and then its backward runs
# asr_gemm_nn_poolbwd -- the pooling backward in the data-gradient GEMM's epilogue -- and leaves the un-pooled gradient in the box for
# VGGFn.backward, returning a stride-0 zero as the formal gradient.
_pool_handover = _Handover()          # VGGFn (the pooled features) -> EncInFn.forward
_pool_handover_on = os.environ.get("ASR_POOL_HANDOVER", "1") != "0"


class EncInFn(Function):
    @staticmethod
    def forward(ctx, x, Win, bin_, gamma, beta, pe):
        cd = ops.compute_dtype()
        B, T, Din = x.shape
        x2 = x.reshape(B * T, Din)
        if x2.dtype != cd:
            x2 = x2.to(cd)
        x2 = x2.contiguous()
        y = _linear_fwd(x2, Win, bin_)
        # (pe None: --pos-encoding rope, the encoder adds no absolute sinusoid)
        out, mean, rstd = ops.add_ln_fwd(y, None, gamma.data, beta.data, post_add=None if pe is None else pe[:T].contiguous())
        ctx.t = (x2, y, mean, rstd)
        ctx.params = (Win, bin_, gamma, beta)
        ctx.shape = (B, T, Din)
        ctx.need_dx = x.requires_grad
        ctx.in_dtype = x.dtype
        ctx.pool_box = _pool_handover.claim(x) if (x.requires_grad and x.dtype == cd and x.is_contiguous()) else None
        if ctx.pool_box is not None:
            ctx.pool_box["claimed"] = True
        return out.view(B, T, -1)

    @staticmethod
    def backward(ctx, dout):
        B, T, Din = ctx.shape
        x2, z, mean, rstd = ctx.t
        Win, bin_, gamma, beta = ctx.params
        dout2 = dout.reshape(B * T, -1).contiguous()
        dz, _ = ops.add_ln_bwd(dout2, z, mean, rstd, gamma.data, None, P.grad_of(gamma), P.grad_of(beta))
        box = ctx.pool_box
        dx = None
        if box is not None and ctx.need_dx:
            # the data gradient straight into the gradient of conv.7's un-pooled output (the pooling backward in the GEMM's epilogue)
            Bc, Hc, Wc, Cc = box["x_shape"]
            dy4 = ops.gemm_nn_poolbwd(dz, P.tcf_perm_shadow(Win, Cc, Hc // 2), box["code"], box["x_shape"])
            if dy4 is not None:
                box["dy4"] = dy4
                _linear_bwd(dz, x2, Win, bin_, need_dx=False)                       # weight / bias gradient as ever
                dx = ops.zero_scalar(dz.device, ctx.in_dtype).expand(B, T, Din)   # formal gradient: VGGFn.backward reads the box
        if dx is None:
            dx = _linear_bwd(dz, x2, Win, bin_, need_dx=ctx.need_dx)
            if dx is not None:
                dx = dx.view(B, T, Din).to(ctx.in_dtype)
        ops.flush_wgrads(final=True)                      # the transformer's backward ends here: every queued weight gradient in grouped launches
        P.grad_ready(*ctx.params)
        return dx, None, None, None, None, None


# ================================================================================================ target embedding
class EmbedFn(Function):
    @staticmethod
    def forward(ctx, tok, table, pe, scale, p, pad_id, mark_ready):
        seed = P.next_seed()
        T = tok.shape[1]
        out = ops.embed_fwd(tok, table.data, pe[:T].contiguous(), scale, p, seed, ops.compute_dtype())
        ctx.tok, ctx.table, ctx.scale, ctx.p, ctx.seed, ctx.pad_id = tok, table, scale, p, seed, pad_id
        ctx.mark_ready = mark_ready
        return out

    @staticmethod
    def backward(ctx, dout):
        ops.embed_bwd(ctx.tok, dout.contiguous(), P.grad_of(ctx.table), ctx.scale, ctx.p, ctx.seed, ctx.pad_id)
        if ctx.mark_ready:
            P.grad_ready(ctx.table)
        return (None,) * 7


# ================================================================================================ vgg front end
# Round 6 removed the A/B switches of this front end (ASR_CONV7_POOL, ASR_POOL_CODES, ASR_LEVEL0, ASR_RELU_BITS: every one measured, the
# fused forms won -- DESIGN.md section 4): each fused form is taken where the library has it (its wrapper returns None otherwise: fp32
# parity mode, odd shapes) and when the parity tests' activation tap does not need the stored tensors.
#   * pools from their convolution's epilogue with one selection byte per pooled element (the un-pooled outputs are never stored);
#   * the full-resolution level (conv.0, conv.2, first pool) as three launches that never store a 64-channel full-resolution tensor
#     (csrc/conv_level0.hip): forward, weight side and data side of the backward;
#   * conv.5's ReLU mask for conv.7's data gradient as one bit per element written by conv.5's own epilogue (asr_conv3x3_igemm_bits).
# (conv weight gradients -- or the fold of their partial blocks -- on the second stream next to the following data gradient measured
#  slower, 7.82-7.94 / 7.50-7.59 vs 7.70 / 7.44 ms per step in round 2: both kernels are MFMA- and HBM-bound, sharing the CUs slows both)


class VGGFn(Function):
    @staticmethod
    def forward(ctx, src, w0, b0, w2, b2, w5, b5, w7, b7):
        cd = ops.compute_dtype()
        src = src.contiguous().float()
        P.conv_shadows((w2, w5, w7))                      # the three packed weight sets of the step in one launch
        wk2, _ = P.conv_shadow(w2)
        tap = capture_selections is not None
        # conv.0 + ReLU recomputed inside conv.2's loader, conv.2 + ReLU + MaxPool2d + selection codes from its epilogue: the log-mel
        # frames in, the pooled tensor out (bf16 compute; the parity tests' tap needs the stored activations)
        lvl0 = None
        if cd == torch.bfloat16 and not tap and w0.shape[0] == 64 and tuple(w2.shape[:2]) == (64, 64):
            lvl0 = ops.vgg_level0_fwd(src, w0.data, b0.data, wk2, b2.data)
        if lvl0 is not None:
            y1 = y2 = None
            p1, c1 = lvl0
        else:
            y1 = ops.conv1_fwd(src, w0.data, b0.data, cd)
            # conv.2 + ReLU + MaxPool2d in one epilogue.  With selection codes (one byte per pooled element) the backward never reads the
            # un-pooled activations again, so y2 (527 MB at the benchmark shape) is not even stored -- unless the parity tests' tap
            # (capture_selections) or a no-code fallback needs it.
            fused = ops.conv3x3_relu_pool_code(y1, wk2, b2.data, w2.shape[0], keep_y=tap)
            if fused is not None:
                y2, p1, c1 = fused
            else:
                y2, p1 = ops.conv3x3_relu_pool(y1, wk2, b2.data, w2.shape[0])
                c1 = None
        wk5, _ = P.conv_shadow(w5)
        with_bits = ops.conv3x3_relu_bits(p1, wk5, b5.data, w5.shape[0]) if (cd == torch.bfloat16 and not tap) else None
        y3, m3 = with_bits if with_bits is not None else (ops.conv3x3(p1, wk5, b5.data, w5.shape[0], relu=True), None)
        wk7, _ = P.conv_shadow(w7)
        y4_shape = tuple(y3.shape[:3]) + (w7.shape[0],)
        # conv.7 + ReLU + MaxPool2d + the (B, T', C F') transpose from the convolution's epilogue: y4 is never stored (not for the tap)
        fused7, box = None, None
        if not tap:
            # selection bytes channel last when a consumer may take the pooling backward into its own epilogue (EncInFn, see _pool_handover)
            if _pool_handover_on and cd == torch.bfloat16 and any(ctx.needs_input_grad):
                fused7 = ops.conv3x3_relu_pool_tcf_code(y3, wk7, b7.data, w7.shape[0], code_cl=True)
                if fused7 is not None:
                    box = {"code": fused7[1], "x_shape": y4_shape, "claimed": False, "dy4": None}
            if fused7 is None:
                fused7 = ops.conv3x3_relu_pool_tcf_code(y3, wk7, b7.data, w7.shape[0])
        if fused7 is not None:
            y4 = None
            out, c4 = fused7
        else:
            y4 = ops.conv3x3(y3, wk7, b7.data, w7.shape[0], relu=True)
            pooled = ops.maxpool_fwd_code(y4, tcf=True)
            if pooled is not None:
                out, c4 = pooled
            else:
                out, c4 = ops.maxpool_fwd(y4, tcf=True), None
        if tap:
            capture_selections.append(("vgg", (y1, y2, y3, y4)))
        # what backward reads: the conv inputs (y1, p1, y3), the ReLU masks (y1, y3) and either the codes or the pre-pool activations
        ctx.t = (src, y1, None if c1 is not None else y2, p1, y3, None if c4 is not None else y4, c1, c4, y4_shape, m3)
        ctx.params = (w0, b0, w2, b2, w5, b5, w7, b7)
        ctx.pool_box = box
        _pool_handover.clear()
        if box is not None:
            _pool_handover.leave(out, out, box)
        return out

    @staticmethod
    def backward(ctx, dout):
        src, y1, y2, p1, y3, y4, c1, c4, y4_shape, m3 = ctx.t
        w0, b0, w2, b2, w5, b5, w7, b7 = ctx.params

        def wgrad(x, dy, w, b, tag):
            # dW and db straight from the NHWC tensors (transposing LDS reads; no planar copies)
            ops.conv3x3_wgrad_nhwc(x, dy, P.grad_of(w), P.grad_of(b))

        box = ctx.pool_box
        dy4 = box.pop("dy4", None) if box is not None else None
        if dy4 is None:
            if box is not None:
                # channel-last selection bytes, but nobody took the pooling backward (the features went somewhere else than EncInFn):
                # back to the pooled tensor's own layout for the stand-alone kernel (a copy on the device; not the training path)
                Bq, Hq, Wq, Cq = y4_shape
                c4 = c4.permute(0, 1, 3, 2).reshape(Bq, Wq // 2, Cq * (Hq // 2)).contiguous()
            dy4 = ops.maxpool_bwd_code(c4, dout.contiguous(), y4_shape, tcf=True) if c4 is not None else ops.maxpool_bwd(y4, dout.contiguous(), tcf=True)
        wgrad(y3, dy4, w7, b7, "c7")
        P.grad_ready(w7, b7)
        _, wd7 = P.conv_shadow(w7)
        dy3 = ops.conv3x3_masked_by_bits(dy4, wd7, None, w7.shape[1], m3) if m3 is not None else None
        if dy3 is None:
            dy3 = ops.conv3x3(dy4, wd7, None, w7.shape[1], relu=False, mask_src=y3)
        wgrad(p1, dy3, w5, b5, "c5")
        P.grad_ready(w5, b5)
        _, wd5 = P.conv_shadow(w5)
        dp1 = ops.conv3x3(dy3, wd5, None, w5.shape[1], relu=False)
        if y1 is None:
            # full-resolution level from the frames, the pooled gradient and the selection codes (forward ran asr_vgg_level0_fwd)
            ops.vgg_level0_wgrad(src, w0.data, b0.data, dp1, c1, P.grad_of(w2), P.grad_of(b2))
            P.grad_ready(w2, b2)
            _, wd2 = P.conv_shadow(w2)
            ops.vgg_level0_dgrad(dp1, c1, src, w0.data, b0.data, wd2, P.grad_of(w0), P.grad_of(b0))
            P.grad_ready(w0, b0)
            return (None,) * 9
        dy2 = ops.maxpool_bwd_code(c1, dp1, tuple(y1.shape[:3]) + (w2.shape[0],), tcf=False) if c1 is not None else ops.maxpool_bwd(y2, dp1)
        wgrad(y1, dy2, w2, b2, "c2")
        P.grad_ready(w2, b2)
        _, wd2 = P.conv_shadow(w2)
        dy1 = ops.conv3x3(dy2, wd2, None, w2.shape[1], relu=False, mask_src=y1)
        ops.conv1_wgrad(src, dy1, P.grad_of(w0), P.grad_of(b0))
        P.grad_ready(w0, b0)
        return (None,) * 9


# ================================================================================================ emb_cnn front end
def _conv_gemm_fwd(x_nhwc, g, w, b, tag):
    """Strided big-window convolution as im2col + MFMA GEMM.  Returns (col (Mp,ld), Ws (64,ld), y fp32 (Mp,64), M, K)."""
    cd = ops.compute_dtype()
    dev = x_nhwc.device
    Cout = w.shape[0]
    M, K = g[0] * g[10] * g[11], g[3] * g[4] * g[5]
    Mp, ld = (M + 127) // 128 * 128, max(64, ops._pad8(K))
    col = ops.im2col(x_nhwc, g, ops.workspace(tag + "_col", (Mp, ld), cd, dev))
    Ws = ops.workspace(tag + "_w", (64, ld), cd, dev)                  # rows >= Cout and columns >= K stay zero
    Ws[:Cout, :K].copy_(w.data.permute(0, 2, 3, 1).reshape(Cout, K))   # (co, ky, kx, ci): the im2col column order
    bias = ops.workspace(tag + "_b", (64,), torch.float32, dev)
    bias[:Cout].copy_(b.data)
    y = ops.gemm_nt(col, Ws, bias=bias, out=ops.workspace(tag + "_y", (Mp, 64), torch.float32, dev))
    return col, Ws, y, M, K


# (Round 6 removed ASR_EMB_WINDOW / ASR_EMB_SHIFT_FWD / ASR_EMB_SHIFT_WGRAD: the time-window and packet formulations below won every
#  measurement of rounds 2 - 3; the full im2col path stays as the fallback for geometries they do not cover.  The two attributes below
#  are not switches but test arms: tests/test_host.py checks the index algebra of BOTH forms of each contraction on CPU stand-ins.)
_emb_shift_fwd = True          # unit time stride: one dense product over single-step patches + asr_window_sum (else the window-view GEMM)
_emb_shift_wgrad = True        # weight gradient as ONE packet-of-rows contraction against the shifted dy view (else per window view)


def _window_ok(g):
    """The time-window formulation below applies to a convolution without padding along the frequency axis whose padded time
    extent is a whole number of strides (both emb_cnn layers: 1 -> 32, 41 x 11, stride (2,2), time padding 10, and 32 -> 32,
    21 x 11, stride (2,1)); bf16 operands."""
    B, H, W, C, KH, KW, SH, SW, PH, PW, OH, OW = g
    return PH == 0 and KW > 1 and (W + 2 * PW) % SW == 0 and ops.compute_dtype() == torch.bfloat16


def _window_geom(g):
    """-> (g1: the KW = 1, stride-1 im2col geometry, blk: elements of one time step's (ky, c) block padded to 16 bytes,
    Wg: GEMM rows per (b, oh) group, R: GEMM rows)"""
    B, H, W, C, KH, KW, SH, SW, PH, PW, OH, OW = g
    g1 = ops.conv_geom(B, H, W, C, KH, 1, SH, 1, 0, PW)              # OH x (W + 2 PW) positions, one (padded) time step per row
    # a wide block (32 channels x 21 rows = 672) is padded to whole 64-element steps (704): X2 is then the A operand of the eight-wave
    # GEMM of the unit-stride form below; the one-channel block of the first convolution (41 -> 48) stays as tight as 16 bytes allow
    blk = (KH * C + 63) // 64 * 64 if KH * C >= 256 else (KH * C + 7) // 8 * 8
    Wg = g1[11] // SW
    return g1, blk, Wg, B * OH * Wg


def _conv_window_fwd(x_nhwc, g, w, b, tag):
    """The same convolution WITHOUT the kx axis in im2col: X2[(b, oh, t), (ky, c)] = x[b, SH*oh + ky, t - PW, c] for every
    (padded) input time step t (about KW / SW times fewer bytes than the full im2col), and the GEMM's A operand is the
    overlapping-rows view A[(b, oh, j)] = X2 flat[row * SW * blk : ... + KW * blk] -- KW consecutive X2 rows ARE the patch of
    output step j, in column order (kx, ky, c).  Rows j >= OW of a (b, oh) group run into the next group; the BatchNorm kernels
    that read y skip them through the row grid (Wg, OW) returned here ((0, 0): y is compact -- the unit-stride form below writes
    it that way).  Returns (X2, A view, y fp32, M, ygrid)."""
    cd = ops.compute_dtype()
    dev = x_nhwc.device
    B, H, W, C, KH, KW, SH, SW, PH, PW, OH, OW = g
    Cout = w.shape[0]
    g1, blk, Wg, R = _window_geom(g)
    M, K = B * OH * OW, KW * blk
    Kp = ops._pad8(K)
    rows1 = B * OH * g1[11]
    slack = (Kp + blk - 1) // blk + SW                               # rows the last window reads past the last group
    X2 = ops.im2col(x_nhwc, g1, ops.workspace(tag + "_x2", (rows1 + slack, blk), cd, dev))
    A = torch.as_strided(X2, (R, Kp), (SW * blk, 1))
    bias = ops.workspace(tag + "_b", (64,), torch.float32, dev)
    bias[:Cout].copy_(b.data)
    if _emb_shift_fwd and SW == 1 and PW == 0 and blk % 64 == 0 and Cout % 4 == 0:
        # unit time stride: ONE dense product over the single-step patches, Z[r', (kx, co)] = X2[r'] . W[co, kx] (N = KW * Cout = 352
        # useful columns instead of 32 padded to 64, X2 read once instead of through the KW-fold window view), then the taps are
        # folded along time into the compact rows of y (asr_window_sum: every element of Z read once, bias added there)
        Nz = ops._pad8(KW * Cout)
        y = ops.workspace(tag + "_y", ((M + 127) // 128 * 128, 64), torch.float32, dev)
        Wz = ops.workspace(tag + "_wz", ((Nz + 127) // 128 * 128, blk), cd, dev)          # rows >= KW * Cout and the ky padding stay zero
        Wz[:KW * Cout, :KH * C].copy_(w.data.permute(3, 0, 2, 1).reshape(KW * Cout, KH * C))       # [(kx, co), (ky, ci)]
        Z = ops.gemm_nt(X2[:R + KW - 1], Wz[:Nz], out=ops.workspace(tag + "_z", (R + KW - 1, Nz), torch.float32, dev, zero=False))   # written whole by the product
        ops.window_sum(Z, y, bias, B * OH, Wg, OW, KW, Cout)
        return X2, A, y, M, (0, 0)
    Ws = ops.workspace(tag + "_w", (64, Kp), cd, dev)                # rows >= Cout, columns >= K and the ky padding stay zero
    Ws[:Cout, :K].view(Cout, KW, blk)[:, :, :KH * C].copy_(w.data.permute(0, 3, 2, 1).reshape(Cout, KW, KH * C))   # (co, kx, ky, ci)
    yf = ops.gemm_nt(A, Ws, bias=bias, out=ops.workspace(tag + "_yf", (R, 64), torch.float32, dev))
    return X2, A, yf, M, (Wg, OW)


def _window_dy(g, Cout, tag, dev):
    """The dense dy operand D of the window gradients: dy's Cout columns on the GEMM's row grid (rows j >= OW of a group stay zero)
    with KW - 1 zero rows in front, so that D flat[r * Cout : r * Cout + KW * Cout] = dy rows r - (KW - 1) .. r.  The BatchNorm
    backward writes its output straight into it (asr_bn_act_bwd's dy grid).  -> (D, the (R, Cout) view the rows go to, (Wg, OW))"""
    B, H, W, C, KH, KW, SH, SW, PH, PW, OH, OW = g
    g1, blk, Wg, R = _window_geom(g)
    Kdp = ops._pad8(KW * Cout)
    lead = KW - 1
    tail = (Kdp + Cout - 1) // Cout + 1
    # zero at creation; only output rows (j < OW of every group of Wg) are ever written -- so the row grid is part of the key: two batches
    # with equal B * Wg but different (B, Wg, OW) put their gap rows in different places, and a stale dy in a gap row would be contracted
    D = ops.workspace(tag + "_d", (lead + R + tail, Cout), ops.compute_dtype(), dev, geom=(B, OH, Wg, OW, lead))
    return D, D[lead:lead + R], (Wg, OW)


def _conv_window_bwd(D, A, w, b_grad, g, tag, need_dx):
    """D = _window_dy(...) filled with dy -> weight gradient (Cout, Cin, KH, KW) fp32 (returned), bias gradient (accumulated) and,
    for a unit time stride, the data gradient dx (B, H, W, C): the data gradient of X2 is ONE GEMM against the weights in
    (kx reversed, co) order, and the weight gradient one TN GEMM against the window view A (asr_gemm_tn with ldb < K)."""
    cd = ops.compute_dtype()
    dev = D.device
    B, H, W, C, KH, KW, SH, SW, PH, PW, OH, OW = g
    Cout = w.shape[0]
    g1, blk, Wg, R = _window_geom(g)
    M = B * OH * OW
    Kd = KW * Cout
    Kdp = ops._pad8(Kd)
    lead = KW - 1
    K = KW * blk
    Ad = torch.as_strided(D, (R, Kdp), (Cout, 1))
    Q = (KW + SW - 1) // SW
    if _emb_shift_wgrad and Wg - OW >= Q - 1 and lead >= Q - 1:
        # Tap kx = SW q + p of output step r reads X2 row SW r + kx = row p of the SW-row packet r + q, i.e. packet r'' meets dy row
        # r'' - q under (q, p):   G[(p, ky, c), (j, co)] = sum_r'' Xp[r'', (p, ky, c)] * dy[r'' - (Q - 1) + j, co],   j = Q - 1 - q,
        # with Xp = X2 seen as packets of SW rows and the second operand the SAME kind of shifted view of D the data gradient
        # contracts (the zero rows behind each group and in front of the first absorb the shifts).  One contraction over the rows with
        # an (SW blk) x (Q Cout) result -- 704 x 352 for the 32 -> 32 convolution, 96 x 192 for the 1 -> 32 one -- on the equal-piece
        # 256 x 256 kernel, X2 read once; the 32-column contraction against the KW-fold window view it replaces ran at 30 - 100 TF/s.
        Xp = torch.as_strided(A, (R, SW * blk), (SW * blk, 1))
        AdQ = torch.as_strided(D, (R, Q * Cout), (Cout, 1), (lead - (Q - 1)) * Cout)
        G = torch.zeros((SW * blk, Q * Cout), device=dev, dtype=torch.float32)
        ops.gemm_tn_grouped([(Xp, AdQ, G, None, SW * blk, Q * Cout)])
        if b_grad is not None:
            ops.colsum_acc(D[lead:lead + R], b_grad)
        T = G.view(SW, blk, Q, Cout)[:, :KH * C].flip(2).reshape(SW, KH, C, Q, Cout)             # (p, ky, ci, q, co)
        dw = T.permute(4, 2, 1, 3, 0).reshape(Cout, C, KH, Q * SW)[..., :KW]                     # (co, ci, ky, kx = SW q + p)
    else:
        dw = torch.zeros((Cout, K), device=dev, dtype=torch.float32)
        ops.gemm_tn(D[lead:lead + R], A, dw, colsum_acc=b_grad, N=Cout, K=K)
        dw = dw.view(Cout, KW, blk)[:, :, :KH * C].reshape(Cout, KW, KH, C).permute(0, 3, 2, 1)  # (co, kx, ky, ci) -> (co, ci, ky, kx)
    if not need_dx:
        return dw, None
    assert SW == 1 and PW == 0
    Wd = ops.workspace(tag + "_wd", ((blk + 63) // 64 * 64, Kdp), cd, dev)
    Wd[:KH * C, :Kd].copy_(w.data.flip(3).permute(2, 1, 3, 0).reshape(KH * C, Kd))     # [(ky, ci), (j = KW-1-kx, co)]
    dX2 = ops.gemm_nt(Ad, Wd[:blk], out=ops.workspace(tag + "_dx2", (R, blk), cd, dev))
    return dw, ops.col2im(dX2, g1)


# Length mask of emb_cnn's BatchNorm statistics (round 6): a device int32[2] = valid time steps of the first / second convolution's
# output, set by whoever pads the batch BEYOND its collated length (asr_hip/graph.py under trainer --graph-buckets); None = every row
# counts, as in the reference (whose BatchNorm does run over the collate padding -- that part is kept).
emb_valid = None


def _bn_stats(bn, y, M, C, training, ygrid=(0, 0), valid=None):
    """nn.BatchNorm2d statistics (eps / momentum of the module; unbiased running variance) -> (mean, rstd)."""
    if training:
        track = bn.track_running_stats and bn.running_mean is not None
        # the kernel updates fp32 buffers with a fixed momentum in its own launch; anything else nn.BatchNorm2d allows -- buffers in
        # another dtype (model.half() / .bfloat16()), momentum=None (cumulative average) -- is updated here through torch, never skipped
        fused = track and bn.momentum is not None and bn.running_mean.dtype == torch.float32 and bn.running_var.dtype == torch.float32 \
            and bn.num_batches_tracked is not None and bn.num_batches_tracked.dtype == torch.int64
        if valid is not None and track and not fused:
            raise NotImplementedError("length-masked BatchNorm statistics need fp32 running buffers and a fixed momentum (the count is "
                                      "known on the device only); run this model with --graph-buckets 0")
        mean, rstd = ops.bn_train_stats(y, M, C, bn.eps, bn.momentum if fused else -1.0, bn.running_mean if fused else None,
                                        bn.running_var if fused else None, bn.num_batches_tracked if fused else None, ygrid, valid)
        if track and not fused:
            with torch.no_grad():
                if bn.num_batches_tracked is not None:
                    bn.num_batches_tracked.add_(1)
                f = bn.momentum if bn.momentum is not None else 1.0 / float(max(int(bn.num_batches_tracked), 1))
                var_unbiased = (1.0 / (rstd * rstd) - bn.eps) * (float(M) / float(max(M - 1, 1)))
                bn.running_mean.mul_(1.0 - f).add_((f * mean).to(bn.running_mean.dtype))
                bn.running_var.mul_(1.0 - f).add_((f * var_unbiased).to(bn.running_var.dtype))
        return mean, rstd
    else:
        mean, var = bn.running_mean.float(), bn.running_var.float()
    return mean.contiguous(), torch.rsqrt(var + bn.eps).contiguous()


_emb_generation = [0]


class EmbCNNFn(Function):
    """Conv2d(1,32,(41,11),(2,2),(0,10)) -> BN -> Hardtanh(0,20) -> Conv2d(32,32,(21,11),(2,1)) -> BN -> Hardtanh(0,20)
    -> (B, T', 32*F')   (reference: transformer.py:33-40, :70-76)."""

    @staticmethod
    def forward(ctx, src, w0, b0, g1, be1, w3, b3, g4, be4, bn1, bn4, training):
        cd = ops.compute_dtype()
        src = src.contiguous().float()
        B, _, Fq, T = src.shape
        C1, C2 = w0.shape[0], w3.shape[0]
        gA = ops.conv_geom(B, Fq, T, 1, w0.shape[2], w0.shape[3], 2, 2, 0, 10)
        winA = _window_ok(gA)
        if winA:
            colA, WsA, yA, MA, ygA = _conv_window_fwd(src.view(B, Fq, T, 1), gA, w0, b0, "embV")      # colA = X2, WsA = the window view
            KA = gA[3] * gA[4] * gA[5]
        else:
            colA, WsA, yA, MA, KA = _conv_gemm_fwd(src.view(B, Fq, T, 1), gA, w0, b0, "embA")
            ygA = (0, 0)
        # bucket padding behind the collated batch stays out of the batch statistics (emb_valid: device int32[2], see above)
        ev = emb_valid if (training and emb_valid is not None) else None
        vA = (ev[0:1], gA[11]) if ev is not None else None
        meanA, rstdA = _bn_stats(bn1, yA, MA, C1, training, ygA, vA)
        a1 = torch.empty((B, gA[10], gA[11], C1), device=src.device, dtype=cd)
        ops.bn_act_fwd(yA, MA, C1, meanA, rstdA, g1.data, be1.data, 0.0, 20.0, a1.view(MA, C1), ygrid=ygA)
        gB = ops.conv_geom(B, gA[10], gA[11], C1, w3.shape[2], w3.shape[3], 2, 1, 0, 0)
        win = _window_ok(gB)
        if win:
            colB, WsB, yB, MB, ygB = _conv_window_fwd(a1, gB, w3, b3, "embW")       # colB = X2, WsB = the window view
            KB = gB[3] * gB[4] * gB[5]
        else:
            colB, WsB, yB, MB, KB = _conv_gemm_fwd(a1, gB, w3, b3, "embB")
            ygB = (0, 0)
        vB = (ev[1:2], gB[11]) if ev is not None else None
        meanB, rstdB = _bn_stats(bn4, yB, MB, C2, training, ygB, vB)
        out = torch.empty((B, gB[11], C2 * gB[10]), device=src.device, dtype=cd)
        ops.bn_act_fwd(yB, MB, C2, meanB, rstdB, g4.data, be4.data, 0.0, 20.0, out, tH=gB[10], tW=gB[11], ygrid=ygB)
        ctx.t = (colA, WsA, yA, meanA, rstdA, colB, WsB, yB, meanB, rstdB)
        # colA / yA / colB / yB are SHARED grow-only workspaces (ops.workspace): a later forward overwrites them
        _emb_generation[0] += 1
        ctx.generation = _emb_generation[0]
        ctx.geo = (gA, gB, MA, KA, MB, KB)
        ctx.ygrid = (ygA, ygB)
        ctx.valid = (vA, vB)
        ctx.win, ctx.winA = win, winA
        ctx.params = (w0, b0, g1, be1, w3, b3, g4, be4)
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.generation != _emb_generation[0]:
            raise RuntimeError("emb_cnn backward after a later emb_cnn forward: the im2col workspaces of this forward were "
                               "overwritten (run backward before the next forward)")
        colA, WsA, yA, meanA, rstdA, colB, WsB, yB, meanB, rstdB = ctx.t
        gA, gB, MA, KA, MB, KB = ctx.geo
        w0, b0, g1, be1, w3, b3, g4, be4 = ctx.params
        cd = ops.compute_dtype()
        dev = dout.device
        C1, C2 = w0.shape[0], w3.shape[0]
        dout = dout.contiguous()
        if dout.dtype != cd:
            dout = dout.to(cd)
        # ---- second conv block
        ygA, ygB = ctx.ygrid
        vA, vB = ctx.valid
        if ctx.win:
            DB, dyB, dgB = _window_dy(gB, C2, "embW", dev)
        else:
            dyB, dgB = ops.workspace("embB_dy", (yB.shape[0], 64), cd, dev), (0, 0)
        sB = ops.bn_act_bwd(dout, yB, MB, C2, meanB, rstdB, g4.data, be4.data, 0.0, 20.0, dyB, tH=gB[10], tW=gB[11], ygrid=ygB, dygrid=dgB,
                            valid=vB)
        P.grad_of(be4).add_(sB[:C2])
        P.grad_of(g4).add_(sB[C2:])
        if ctx.win:
            dwB, da1 = _conv_window_bwd(DB, WsB, w3, P.grad_of(b3), gB, "embW", True)
            P.grad_of(w3).add_(dwB)
            P.grad_ready(w3, b3, g4, be4)
        else:
            dwB = torch.zeros((C2, KB), device=dev, dtype=torch.float32)
            ops.gemm_tn(dyB, colB, dwB, colsum_acc=P.grad_of(b3), N=C2, K=KB)
            P.grad_of(w3).add_(dwB.view(C2, gB[4], gB[5], gB[3]).permute(0, 3, 1, 2))
            P.grad_ready(w3, b3, g4, be4)
            dcolB = ops.gemm_nn(dyB, WsB, out=colB)          # colB is dead after the weight gradient: reuse its storage
            da1 = ops.col2im(dcolB, gB)
        # ---- first conv block (no data gradient: the input is the spectrogram)
        if ctx.winA:
            DA, dyA, dgA = _window_dy(gA, C1, "embV", dev)
        else:
            dyA, dgA = ops.workspace("embA_dy", (yA.shape[0], 64), cd, dev), (0, 0)
        sA = ops.bn_act_bwd(da1.view(MA, C1), yA, MA, C1, meanA, rstdA, g1.data, be1.data, 0.0, 20.0, dyA, ygrid=ygA, dygrid=dgA, valid=vA)
        P.grad_of(be1).add_(sA[:C1])
        P.grad_of(g1).add_(sA[C1:])
        if ctx.winA:
            dwA, _ = _conv_window_bwd(DA, WsA, w0, P.grad_of(b0), gA, "embV", False)
            P.grad_of(w0).add_(dwA)
        else:
            ops.gemm_tn(dyA, colA, P.grad_of(w0).view(C1, KA), colsum_acc=P.grad_of(b0), N=C1, K=KA)
        P.grad_ready(w0, b0, g1, be1)
        return (None,) * 12


# ================================================================================================ loss
# The logit hand-over, stated once.  Every loss Function whose input may be the fp32 logits of a bf16 model's vocabulary projection
# (CEFn, DistillFn, RnntFn, RnntPrunedFn, SeqLogProbFn) follows it:
#   forward   _claim_logits(ctx, logits): if the input needs a gradient, claim the box LinearFn left for these logits (_Handover.claim:
#             matched by a live weak reference plus address and size).  The claim EMPTIES the slot whoever makes it and whatever it
#             finds -- the slot holds one box, for the projection that ran last -- so a Function must run right behind the projection
#             whose logits it takes, before the next fp32 projection or claim.
#   backward  _hand_back(ctx, bwd, shape): with a box, the gradient goes into it as bf16, zero padded to 64 columns (what the
#             projection's data-gradient GEMM reads), and a stride-0 zero is the formal fp32 gradient -- that saves the fp32 tensor
#             (56 MB at the benchmark's CE), its cast / pad launch and half of the kernel's stores; LinearFn.backward adds whatever a
#             second consumer of the logits contributed.  Without a box (an fp32 model, logits from elsewhere) the fp32 gradient itself.
def _claim_logits(ctx, logits):
    ctx.handover = _logit_handover.claim(logits) if ctx.needs_input_grad[0] else None


def _hand_back(ctx, bwd, shape):
    """bwd(**kw) is the Function's ops.*_bwd call, open in out_dtype and pad; `shape` the formal shape of the input's gradient."""
    if ctx.handover is None:
        return bwd().reshape(shape)
    dy = ctx.handover["dy"] = bwd(out_dtype=torch.bfloat16, pad=64)
    return ops.zero_scalar(dy.device).expand(shape)


def _f32c(t):
    """fp32 and contiguous: what the loss kernels read."""
    return (t if t.dtype == torch.float32 else t.float()).contiguous()


def _lengths_i32(lengths, dev):
    return torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()


def _scalar_f32(dloss):
    return dloss.reshape(1).float().contiguous()


class CEFn(Function):
    """loss = sum over non-PAD rows of the (label smoothed) row loss / count        (reference: utils/metrics.py:102-132).

    Single process: `count` is the batch's non-PAD count (or `global_count`, a device scalar, when given).
    Data parallel (a GradReducer is active and gradients are enabled): the reference's loss is the mean over the GATHERED
    batch, so the three statistics [loss_sum, count, num_correct] are written into FlatParams.stats -- the tail of the flat
    gradient buffer, summed over ranks by the gradient all-reduce itself -- and backward propagates the UN-normalised local
    sum; FusedAdam multiplies the reduced gradients by 1 / global count (asr_grad_coef).  The value returned here is the
    LOCAL mean (a per-rank progress figure); the exact global loss is FusedAdam.global_loss() after the step."""

    @staticmethod
    def forward(ctx, pred, gold, smoothing, pad_id, global_count):
        ctx.set_materialize_grads(False)       # no zero-filled gradients for the two statistics outputs (one fill launch each per step)
        V = pred.shape[-1]
        logits = _f32c(pred.reshape(-1, V))
        g = gold.reshape(-1).contiguous()
        red = P._state["reducer"]
        # (grad mode is always off inside Function.forward: "will backward run" is ctx.needs_input_grad)
        deferred = (global_count is None and red is not None and red.active and ctx.needs_input_grad[0]
                    and red.flat.stats.device == logits.device)
        if deferred:
            lse, am, sums = ops.ce_fwd(logits, g, smoothing, pad_id, sums=red.flat.stats)      # (summed over ranks with the gradients: atomics into the zeroed tail)
            count = None                                               # backward: un-normalised sum
            sums = sums[:3]
            loss = ops.ratio(sums[0:1], sums[1:2]).reshape(())
        else:
            # per-block partial sums added in a fixed order: the same bits run to run, no zero fill, the mean from the same finish launch
            lse, am, sums, loss = ops.ce_fwd_det(logits, g, smoothing, pad_id, den=global_count)
            loss = loss.reshape(())
            count = global_count if global_count is not None else sums[1:2]
        ctx.t = (logits, g, lse, count)
        ctx.smoothing, ctx.pad_id, ctx.shape = smoothing, pad_id, pred.shape
        _claim_logits(ctx, logits)
        ctx.mark_non_differentiable(sums, am)
        return loss, sums, am

    @staticmethod
    def backward(ctx, dloss, *unused):
        logits, g, lse, count = ctx.t
        if count is None:
            count = ops.ones_scalar(logits.device)
        # (reference: loss.backward() through utils/metrics.py:118-130)
        bwd = functools.partial(ops.ce_bwd, logits, g, lse, ctx.smoothing, ctx.pad_id, _scalar_f32(dloss), count)
        return _hand_back(ctx, bwd, ctx.shape), None, None, None, None


class DistillFn(Function):
    """loss = (ce_scale * sum of CEFn's row losses + kd_scale * sum_m kd_m) / count over the live rows (gold != pad_id), with
    kd_m = tau^2 KL(softmax(teacher / tau) || softmax(student / tau)) of row m (ops.distill_fwd).  count is the
    live-row count.  with_ce=False: the KD term alone -- gold only marks the live rows
    and ce_scale is taken as 0.  -> (loss, sums (4,) = [sum ce, #live, #correct, sum kd], argmax (M,) or an empty tensor without with_ce),
    the last two not differentiable; the teacher logits never get a gradient.
    backward: ONE asr_distill_bwd launch writes the combined CE + KD gradient.  The logit hand-over (_claim_logits / _hand_back above)
    takes one gradient per logits tensor, which is why the two terms share a Function; and since a claim empties the slot, of two
    DistillFn calls in one step the one on the projection's logits comes first."""

    @staticmethod
    def forward(ctx, student_logits, teacher_logits, gold, smoothing, pad_id, temperature, ce_scale, kd_scale, with_ce):
        ctx.set_materialize_grads(False)
        V = student_logits.shape[-1]
        if teacher_logits.shape != student_logits.shape:
            raise ValueError("DistillFn: student logits %s and teacher logits %s differ in shape"
                             % (tuple(student_logits.shape), tuple(teacher_logits.shape)))
        logits = _f32c(student_logits.reshape(-1, V))
        teach = _f32c(teacher_logits.detach().reshape(-1, V))
        g = gold.reshape(-1).contiguous()
        if not with_ce:
            ce_scale = 0.0
        stats, am, sums, loss = ops.distill_fwd(logits, teach, g, smoothing, pad_id, temperature, ce_scale, kd_scale, with_ce=with_ce)
        if am is None:
            am = g.new_empty(0)
        ctx.t = (logits, teach, g, stats, sums[1:2])
        ctx.cfg = (float(smoothing), int(pad_id), float(temperature), float(ce_scale), float(kd_scale))
        ctx.shape = student_logits.shape
        _claim_logits(ctx, logits)
        ctx.mark_non_differentiable(sums, am)
        return loss.reshape(()), sums, am

    @staticmethod
    def backward(ctx, dloss, *unused):
        logits, teach, g, stats, count = ctx.t
        bwd = functools.partial(ops.distill_bwd, logits, teach, g, stats, *ctx.cfg, _scalar_f32(dloss), count)
        return (_hand_back(ctx, bwd, ctx.shape),) + (None,) * 8


class CTCFn(Function):
    """loss = F.ctc_loss(F.log_softmax(pred, 2).transpose(0, 1), gold, input_lengths, target_lengths, reduction="mean")
    (reference: utils/metrics.py:133-154; blank = PAD = 0)."""

    @staticmethod
    def forward(ctx, pred, gold, input_lengths, target_lengths, blank):
        logits = _f32c(pred)
        dev = logits.device
        tg = gold.to(device=dev, dtype=torch.int64).contiguous()
        il, tl = _lengths_i32(input_lengths, dev), _lengths_i32(target_lengths, dev)
        loss, ws = ops.ctc_fwd(logits, tg, il, tl, blank)
        ctx.t = (logits, tg, il, tl, ws)
        ctx.blank = blank
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        logits, tg, il, tl, ws = ctx.t
        dl = ops.ctc_bwd(logits, tg, il, tl, ws, _scalar_f32(dloss), ctx.blank)
        return dl, None, None, None, None


# ================================================================================================ transducer head
RNNT_MAX_LOGIT_BYTES = 1 << 31


class RnntJointFn(Function):
    """z (B,T,U+1,J) = tanh(e (B,T,J) + p (B,U+1,J)) in the compute dtype (ops.rnnt_joint).
    backward: ONE launch (ops.rnnt_joint_bwd) reads dz and z once and leaves de = sum_u dz (1 - z^2) and dp = sum_t dz (1 - z^2)."""

    @staticmethod
    def forward(ctx, e, p):
        cd = ops.compute_dtype()
        z = ops.rnnt_joint(e if e.dtype == cd else e.to(cd), p if p.dtype == cd else p.to(cd))
        ctx.z = z
        ctx.dtypes = (e.dtype, p.dtype)
        return z

    @staticmethod
    def backward(ctx, dz):
        z = ctx.z
        de, dp = ops.rnnt_joint_bwd(dz if dz.dtype == z.dtype else dz.to(z.dtype), z)
        return de.to(ctx.dtypes[0]), dp.to(ctx.dtypes[1])


class RnntFn(Function):
    """loss = mean_b nll_b / max(U_b, 1) of the transducer lattice (ops.rnnt_fwd): pred (B,T,U+1,V) fp32 joint
    logits, gold (B,>=U) label ids without SOS / EOS, frame_lengths = true encoder frames T_b, target_lengths = U_b, blank = PAD.  The
    reduction is CTCFn's, so --ctc-weight and --transducer-weight compare.  An utterance without an alignment (T_b = 0, a label that
    is the blank or outside [0,V)) makes the loss +inf and gets zero gradient rows.
    backward: ONE launch (ops.rnnt_bwd), through the logit hand-over (_claim_logits / _hand_back above).  The model applies this Function
    right behind the joint's vocabulary projection and before the decoder runs (Transformer.transducer_loss), so the slot it claims is
    that projection's and the decoder's projection leaves a fresh one for CEFn afterwards.  Memory at B 32, T' 75, V 4364: the fp32
    logits are B T' (U+1) V 4 bytes = 0.88 GB at U 20 and 1.72 GB at U 40 (kept for the backward), the handed-over gradient half of a
    4416-wide copy of that, 0.45 / 0.87 GB; returning the formal fp32 gradient instead would cost another 0.88 / 1.72 GB plus the cast
    and pad launch.
    A shape whose fp32 logits (rows 64-column padded) reach 2^31 bytes is refused with a ValueError before any launch.  The new
    kernels index in 64 bits; the vocabulary projection then runs B T' (U+1) rows through the GEMM arms of _linear_fwd / _lin_bwd, whose
    row bases are 64 bit but whose M, tile counts and per-thread chunk offsets (csrc/gemm_tn.hip, csrc/gemm_nn.hip: offA / offB,
    stage relative) are 32 bit, and not every arm has been read for products of them: the bound keeps every byte offset below 2^31
    whatever an arm computes."""

    @staticmethod
    def forward(ctx, pred, gold, frame_lengths, target_lengths, blank):
        if pred.dim() != 4:
            raise ValueError("RnntFn: joint logits (B,T,U+1,V) expected, got %s" % (tuple(pred.shape),))
        B, T, U1, V = pred.shape
        check_rnnt_shape(B, T, U1, V)
        logits = _f32c(pred)
        dev = logits.device
        tg = torch.as_tensor(gold).to(device=dev, dtype=torch.int64)
        if U1 == 1 and tg.shape[1] == 0:
            tg = tg.new_zeros((B, 1))
        if tg.shape[1] < max(U1 - 1, 1):
            raise ValueError("RnntFn: %d label columns for logits with U + 1 = %d" % (tg.shape[1], U1))
        tg = tg[:, :max(U1 - 1, 1)].contiguous()
        fl, tl = _lengths_i32(frame_lengths, dev), _lengths_i32(target_lengths, dev)
        loss, ws = ops.rnnt_fwd(logits, tg, fl, tl, blank)
        ctx.t = (logits, tg, fl, tl, ws)
        ctx.blank, ctx.shape = blank, pred.shape
        _claim_logits(ctx, logits)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        logits, tg, fl, tl, ws = ctx.t
        bwd = functools.partial(ops.rnnt_bwd, logits, tg, fl, tl, ws, _scalar_f32(dloss), ctx.blank)
        return _hand_back(ctx, bwd, ctx.shape), None, None, None, None


def check_rnnt_shape(B, T, U1, V):
    """ValueError for joint logits (B,T,U1,V) whose fp32 bytes (rows 64-column padded, as their gradient is) reach 2^31."""
    n = int(B) * int(T) * int(U1) * ((int(V) + 63) // 64 * 64) * 4
    if n >= RNNT_MAX_LOGIT_BYTES:
        raise ValueError("transducer joint logits (B %d, T %d, U+1 %d, V %d) take %d bytes in fp32: 2^31 or more is refused (the "
                         "vocabulary projection's GEMMs keep 32-bit sizes and chunk offsets); use a smaller batch or shorter targets, "
                         "or train on a band of the lattice with --transducer-prune-range" % (B, T, U1, V, n))


# ------------------------------------------------------------------------------------------------ pruned transducer (csrc/rnnt_pruned.hip)
def _rnnt_labels(gold, B, U, dev):
    tg = torch.as_tensor(gold).to(device=dev, dtype=torch.int64)
    if U == 0 and tg.shape[1] == 0:
        tg = tg.new_zeros((B, 1))
    if tg.shape[1] < max(U, 1):
        raise ValueError("%d label columns for U = %d" % (tg.shape[1], U))
    return tg[:, :max(U, 1)].contiguous()


class RnntSimpleFn(Function):
    """(loss, gb, gl) of the simple joiner am (B,T,V) + lm (B,U+1,V) (ops.rnnt_simple_fwd): loss = mean_b nll_b /
    max(U_b, 1) with RnntFn's lengths, labels and edge rules; gb, gl (B,T,U+1) fp32, not differentiable: the arc posteriors the band is
    chosen from (ops.rnnt_prune_ranges).  No (B,T,U+1,V) tensor exists: the log-normalisers are one batched fp32 contraction over V.
    backward: three launches (ops.rnnt_simple_bwd), formal fp32 gradients of am and lm.  This Function does NOT claim the logit hand-over
    slot (two projections feed it, the slot holds one): the slot its second projection left stays unclaimed until the next LinearFn
    clears it, and both projections' backwards cast the fp32 gradient themselves."""

    @staticmethod
    def forward(ctx, am, lm, gold, frame_lengths, target_lengths, blank):
        if am.dim() != 3 or lm.dim() != 3 or am.shape[0] != lm.shape[0] or am.shape[2] != lm.shape[2]:
            raise ValueError("RnntSimpleFn: am (B,T,V) and lm (B,U+1,V) expected, got %s and %s" % (tuple(am.shape), tuple(lm.shape)))
        B, U = am.shape[0], lm.shape[1] - 1
        a, l = _f32c(am), _f32c(lm)
        dev = a.device
        tg = _rnnt_labels(gold, B, U, dev)
        fl, tl = _lengths_i32(frame_lengths, dev), _lengths_i32(target_lengths, dev)
        loss, ws, gb, gl = ops.rnnt_simple_fwd(a, l, tg, fl, tl, blank)
        ctx.t = (tg, fl, tl, ws)
        ctx.blank, ctx.shapes = blank, (am.shape, lm.shape)
        ctx.mark_non_differentiable(gb, gl)
        return loss.reshape(()), gb, gl

    @staticmethod
    def backward(ctx, dloss, *unused):
        tg, fl, tl, ws = ctx.t
        dam, dlm = ops.rnnt_simple_bwd(ctx.shapes[0], ctx.shapes[1], tg, fl, tl, ws, _scalar_f32(dloss), ctx.blank)
        return dam, dlm, None, None, None, None


class RnntJointPrunedFn(Function):
    """z (B,T,W,J) = tanh(e (B,T,J) + p (B,U+1,J)[s_begin[b,t] + w]) in the compute dtype (ops.rnnt_joint_pruned): RnntJointFn on a band.
    s_begin (B,T) int32 is a constant of the step.  backward: ONE launch, de = sum_w, dp[b,u] = the sum over the frames whose window
    holds u in ascending t, one owner per element (torch index_add's GPU backward is not reproducible)."""

    @staticmethod
    def forward(ctx, e, p, s_begin, W):
        cd = ops.compute_dtype()
        z = ops.rnnt_joint_pruned(e if e.dtype == cd else e.to(cd), p if p.dtype == cd else p.to(cd), s_begin, int(W))
        ctx.z, ctx.s, ctx.U1 = z, s_begin, p.shape[1]
        ctx.dtypes = (e.dtype, p.dtype)
        return z

    @staticmethod
    def backward(ctx, dz):
        z = ctx.z
        de, dp = ops.rnnt_joint_pruned_bwd(dz if dz.dtype == z.dtype else dz.to(z.dtype), z, ctx.s, ctx.U1)
        return de.to(ctx.dtypes[0]), dp.to(ctx.dtypes[1]), None, None


class RnntPrunedFn(Function):
    """RnntFn on a band (ops.rnnt_pruned_fwd): pred (B,T,W,V) fp32 logits whose row (b,t,w) is lattice cell
    (t, s_begin[b,t] + w) of the T x (U + 1) lattice, U = `umax`; every node outside the band has no outgoing arc.  An utterance without a
    complete path inside its band makes the loss +inf and gets zero gradient rows, like any utterance without an alignment.
    backward: ONE launch, through the logit hand-over as RnntFn's: rnnt_out on the banded z must be the last fp32 projection before
    this Function, and both must run before the decoder.  check_rnnt_shape(B, T, W, V) applies."""

    @staticmethod
    def forward(ctx, pred, gold, frame_lengths, target_lengths, s_begin, umax, blank):
        if pred.dim() != 4:
            raise ValueError("RnntPrunedFn: band logits (B,T,W,V) expected, got %s" % (tuple(pred.shape),))
        B, T, W, V = pred.shape
        U = int(umax)
        if not 1 <= W <= U + 1:
            raise ValueError("RnntPrunedFn: a band of %d label positions for U + 1 = %d" % (W, U + 1))
        check_rnnt_shape(B, T, W, V)
        logits = _f32c(pred)
        dev = logits.device
        tg = _rnnt_labels(gold, B, U, dev)
        fl, tl = _lengths_i32(frame_lengths, dev), _lengths_i32(target_lengths, dev)
        loss, ws = ops.rnnt_pruned_fwd(logits, tg, fl, tl, s_begin, U, blank)
        ctx.t = (logits, tg, fl, tl, s_begin, ws)
        ctx.blank, ctx.shape, ctx.U = blank, pred.shape, U
        _claim_logits(ctx, logits)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        logits, tg, fl, tl, s, ws = ctx.t
        bwd = functools.partial(ops.rnnt_pruned_bwd, logits, tg, fl, tl, s, ctx.U, ws, _scalar_f32(dloss), ctx.blank)
        return (_hand_back(ctx, bwd, ctx.shape),) + (None,) * 6


# ================================================================================================ MWER over the n-best
class SeqLogProbFn(Function):
    """score[r] = sum over the rows of segment r of log_softmax(logits)[m, tgt[m]] (ops.seq_logprob), differentiable in the logits
    (MWER training).  -> (score (R,) fp32, tok (M,) fp32, not differentiable).
    backward: ONE launch of asr_seq_logprob_bwd with the incoming gradient of `score` as the per-segment coefficients, through the
    logit hand-over (_claim_logits / _hand_back above)."""

    @staticmethod
    def forward(ctx, logits, tgt, seg_off):
        assert logits.dim() == 2 and logits.dtype == torch.float32
        out = ops.seq_logprob(logits, tgt, seg_off)
        ctx.t = (logits, tgt, seg_off)
        _claim_logits(ctx, logits)
        ctx.mark_non_differentiable(out["tok"])
        return out["score"], out["tok"]

    @staticmethod
    def backward(ctx, dscore, *unused):
        logits, tgt, seg_off = ctx.t
        bwd = functools.partial(ops.seq_logprob_bwd, logits, tgt, seg_off, dscore.float().contiguous())
        return _hand_back(ctx, bwd, logits.shape), None, None


class MwerLossFn(Function):
    """m * mean risk + (1 - m)(1 - w) * NLL of a step from its R segment scores (ops.mwer_loss): risk_scale = m / B,
    gold_scale = (1 - m)(1 - w) / sum_b (len(gold_b) + 1); the first segment of an utterance is its gold.
    -> (loss, prob (R,), risk (B,), sums (2,)), the last three not differentiable.  backward hands asr_mwer_loss's coefficients, times
    the incoming gradient, to the scores (SeqLogProbFn.backward multiplies them into the rows)."""

    @staticmethod
    def forward(ctx, score, err, utt_off, risk_scale, gold_scale):
        out = ops.mwer_loss(score.contiguous(), err, utt_off, risk_scale, gold_scale)
        loss = out["sums"][0] * float(risk_scale)
        if gold_scale != 0.0:                    # (with m = 1 an infinite gold score must not turn the risk into a NaN)
            loss = loss - out["sums"][1] * float(gold_scale)
        ctx.coef = out["coef"]
        ctx.mark_non_differentiable(out["prob"], out["risk"], out["sums"])
        return loss, out["prob"], out["risk"], out["sums"]

    @staticmethod
    def backward(ctx, dloss, *unused):
        return ctx.coef * dloss.reshape(()).float(), None, None, None, None


# ================================================================================================ composable pieces
# The fused sub-layer Functions above cover the reference's layers.  The low-rank variant (BASELINE configs[4]) factorises
# every projection W (out, in) into V (out, r) . U (r, in); its sub-layers are assembled from LinearFn plus these two.
class SDPAFn(Function):
    """Scaled-dot-product attention on projected (B,T,H*d) tensors: softmax(Q K^T / sqrt(d) + masks) V with in-kernel
    dropout (reference: models/common_layers.py:211-225, head split / merge at :185-195)."""

    @staticmethod
    def forward(ctx, Q, K, V, cfg):
        H, dk = cfg["H"], cfg["dk"]
        B, Tq, HD = Q.shape
        seed = P.next_seed()
        scale = cfg.get("scale") or 1.0 / (dk ** 0.5)          # (heads zero-padded to a common width keep the reference's sqrt(dim_key))
        O32 = torch.empty((B, Tq, HD), device=Q.device, dtype=torch.float32) if (Q.dtype != torch.float32 and any(ctx.needs_input_grad)) else None
        O, lse, attn = ops.attn_fwd(Q, K, V, H, dk, key_len=cfg.get("key_len"), key_pad=cfg.get("key_pad"),
                                    causal=cfg.get("causal", False), scale=scale, p=cfg["p"], seed=seed, o32=O32,
                                    want_attn=cfg.get("want_attn", False))
        ctx.t = (Q, K, V, O, lse, O32)
        ctx.cfg, ctx.seed, ctx.scale = cfg, seed, scale
        if attn is not None:                                   # the reference's returned attention matrices, (H*B, Tq, Tk)
            ctx.mark_non_differentiable(attn)
            return O, attn
        return O

    @staticmethod
    def backward(ctx, dO, *unused):
        Q, K, V, O, lse, O32 = ctx.t
        cfg = ctx.cfg
        dQ, dK, dV = ops.attn_bwd(Q, K, V, O, dO.contiguous(), lse, cfg["H"], cfg["dk"], key_len=cfg.get("key_len"),
                                  key_pad=cfg.get("key_pad"), causal=cfg.get("causal", False), scale=ctx.scale, p=cfg["p"],
                                  seed=ctx.seed, o32=O32)
        return dQ, dK, dV, None


class AddLNFn(Function):
    """out = LayerNorm(dropout(y) + residual) * row_keep   (reference: common_layers.py:140-141, :197-198 and the
    `*= non_pad_mask` after every sub-layer)."""

    @staticmethod
    def forward(ctx, y, residual, gamma, beta, cfg):
        shape = y.shape
        D = shape[-1]
        y2 = y.reshape(-1, D).clone() if y.requires_grad or y.data_ptr() == residual.data_ptr() else y.reshape(-1, D).contiguous()
        r2 = residual.reshape(-1, D).contiguous()
        seed = P.next_seed()
        out, mean, rstd = ops.add_ln_fwd(y2, r2, gamma.data, beta.data, row_keep=cfg.get("row_keep"), p=cfg["p"], seed=seed)
        ctx.t = (y2, mean, rstd)                       # y2 now holds z = dropout(y) + residual
        ctx.params, ctx.cfg, ctx.seed, ctx.shape = (gamma, beta), cfg, seed, shape
        return out.view(shape)

    @staticmethod
    def backward(ctx, dout):
        z, mean, rstd = ctx.t
        gamma, beta = ctx.params
        D = ctx.shape[-1]
        d_res, d_y = ops.add_ln_bwd(dout.reshape(-1, D).contiguous(), z, mean, rstd, gamma.data, ctx.cfg.get("row_keep"),
                                    P.grad_of(gamma), P.grad_of(beta), p=ctx.cfg["p"], seed=ctx.seed)
        P.grad_ready(gamma, beta)
        return d_y.view(ctx.shape), d_res.view(ctx.shape), None, None, None


def _fp8_weight(weight):
    """e4m3 bytes + row scales of a weight, re-quantised when the optimiser stepped or the parameter was modified."""
    key = (P._state["generation"], weight._version)
    ent = weight.__dict__.get("_asr_fp8")
    if ent is None or ent[0] != key:
        q, sc = ops.quant_fp8(weight.data.view(weight.shape[0], -1))
        ent = (key, q, sc)
        weight.__dict__["_asr_fp8"] = ent
    return ent[1], ent[2]


class LinearActFn(Function):
    """y = act(x W^T + b) with act = ReLU or identity, for chains of projections: `relu` fuses the ReLU into this GEMM's
    epilogue; `input_is_relu` says x is the ReLU output of the previous projection, whose mask (x > 0) is then applied in
    THIS layer's data-gradient epilogue (the same fusion FFNFn uses), so no stand-alone activation kernel exists."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, input_is_relu):
        cd = ops.compute_dtype()
        x2 = x.reshape(-1, x.shape[-1])
        if x2.dtype != cd:
            x2 = x2.to(cd)
        x2 = x2.contiguous()
        if ops.fp8_enabled() and cd == torch.bfloat16:
            # fp8 forward (e4m3, one scale per row of either operand, fp32 accumulation on the K = 128 block-scaled MFMA); the backward pass
            # below differentiates the bf16 expression (straight-through), from the bf16 operands
            qa, sa = ops.quant_fp8(x2)
            qb, sb = _fp8_weight(weight)
            y = ops.gemm_nt_fp8(qa, sa, qb, sb, bias=bias.data if bias is not None else None, relu=relu)
        else:
            y = _linear_fwd(x2, weight, bias, relu=relu)
        ctx.x2, ctx.weight, ctx.bias = x2, weight, bias
        ctx.in_shape, ctx.input_is_relu, ctx.need_dx = x.shape, input_is_relu, x.requires_grad
        return y.view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        N = ctx.weight.shape[0]
        dy_c = _as_compute(dy.reshape(-1, N))
        dx = _linear_bwd(dy_c, ctx.x2, ctx.weight, ctx.bias, need_dx=ctx.need_dx,
                         relu_mask=ctx.x2 if (ctx.input_is_relu and ctx.need_dx) else None)
        P.grad_ready(*[p for p in (ctx.weight, ctx.bias) if p is not None])
        if dx is not None:
            dx = dx.view(ctx.in_shape)
        return dx, None, None, None, None
