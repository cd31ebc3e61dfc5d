"""Transformer building blocks with the reference's constructor signatures and state_dict keys
(reference: models/common_layers.py), executed by the hand-written HIP kernels in libasr_hip.so.

The nn.Linear / nn.Conv1d / nn.LayerNorm children are PARAMETER CONTAINERS only (same names, shapes and default
initialisation as the reference, so checkpoints interchange); their own forward() is never called on the hot path.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from asr_hip import functions as F_
from asr_hip import ops
from utils import constant


def pad_list(xs, pad_value):
    """reference: common_layers.py:14-22 -- pads to --tgt-max-len (a flag, not the batch maximum)."""
    max_len = constant.args.tgt_max_len
    out = xs[0].new_full((len(xs), max_len) + tuple(xs[0].shape[1:]), pad_value)
    for i, x in enumerate(xs):
        out[i, :x.size(0)] = x
    return out


# ---- mask helpers: kept for API compatibility (reference: common_layers.py:28-74).  The fused kernels take
# ---- lengths / pad bytes / a causal flag instead and never materialise (B,T,T) masks.
def get_non_pad_mask(padded_input, input_lengths=None, pad_idx=None):
    assert input_lengths is not None or pad_idx is not None
    if input_lengths is not None:
        T = padded_input.size(1)
        lens = torch.as_tensor(input_lengths, device=padded_input.device).to(torch.int64)
        mask = (torch.arange(T, device=padded_input.device)[None, :] < lens[:, None]).to(padded_input.dtype)
    if pad_idx is not None:
        assert padded_input.dim() == 2
        mask = padded_input.ne(pad_idx).float()
    return mask.unsqueeze(-1)


def get_attn_key_pad_mask(seq_k, seq_q, pad_idx):
    return seq_k.eq(pad_idx).unsqueeze(1).expand(-1, seq_q.size(1), -1)


def get_attn_pad_mask(padded_input, input_lengths, expand_length):
    pad = get_non_pad_mask(padded_input, input_lengths=input_lengths).squeeze(-1).lt(1)
    return pad.unsqueeze(1).expand(-1, expand_length, -1)


def get_subsequent_mask(seq):
    b, n = seq.size()
    m = torch.triu(torch.ones((n, n), device=seq.device, dtype=torch.bool), diagonal=1)
    return m.unsqueeze(0).expand(b, -1, -1)


class PositionalEncoding(nn.Module):
    """Sinusoid table kept as the buffer `pe` (1, max_length, dim_model) exactly like the reference
    (common_layers.py:80-98) so that it round-trips through state_dict."""

    def __init__(self, dim_model, max_length=2000):
        super().__init__()
        pos = torch.arange(0, max_length).unsqueeze(1).float()
        freq = torch.exp(torch.arange(0, dim_model, 2).float() * -(math.log(10000.0) / dim_model))
        pe = torch.zeros(max_length, dim_model)
        pe[:, 0::2] = torch.sin(pos * freq)
        pe[:, 1::2] = torch.cos(pos * freq)
        self.register_buffer('pe', pe.unsqueeze(0))

    def forward(self, input):
        return self.pe[:, :input.size(1)]


def _to_compute(x):
    cd = ops.compute_dtype()
    return x if x.dtype == cd else x.to(cd)


def _mask_to_u8(mask):
    if mask is None:
        return None
    return mask.to(torch.uint8).contiguous()


_HEAD_WIDTHS = (16, 32, 64)          # head widths the attention kernels contract (csrc/attention.hip dispatch)


class MultiHeadAttention(nn.Module):
    """forward(query, key, value, mask=None) -> (output, attn)   (reference: common_layers.py:144-200).

    Fast path arguments (used by Encoder/Decoder): key_len (B int32: keys >= len masked), key_pad ((B,Tk) uint8),
    causal, row_keep ((B*Tq) uint8: the `*= non_pad_mask` that follows every call in the reference), need_attn.
    A generic boolean `mask` (B,Tq,Tk) is also accepted, as in the reference."""

    def __init__(self, num_heads, dim_model, dim_key, dim_value, dropout=0.1):
        super().__init__()
        # dim_key != dim_value is a signature the reference accepts (common_layers.py:144-168; no BASELINE config uses it): the
        # attention kernels contract ONE head width (16, 32 or 64), so such a block runs them at the next width >= both on zero-padded heads
        # (forward()'s _forward_padded) -- zero query / key columns add nothing to a score, zero value columns give output columns
        # that are dropped again.
        self.num_heads, self.dim_model, self.dim_key, self.dim_value = num_heads, dim_model, dim_key, dim_value
        self.query_linear = nn.Linear(dim_model, num_heads * dim_key)
        self.key_linear = nn.Linear(dim_model, num_heads * dim_key)
        self.value_linear = nn.Linear(dim_model, num_heads * dim_value)
        nn.init.normal_(self.query_linear.weight, mean=0, std=np.sqrt(2.0 / (dim_model + dim_key)))
        nn.init.normal_(self.key_linear.weight, mean=0, std=np.sqrt(2.0 / (dim_model + dim_key)))
        nn.init.normal_(self.value_linear.weight, mean=0, std=np.sqrt(2.0 / (dim_model + dim_value)))
        self.attention = ScaledDotProductAttention(temperature=np.power(dim_key, 0.5), attn_dropout=dropout)
        self.layer_norm = nn.LayerNorm(dim_model)
        self.output_linear = nn.Linear(num_heads * dim_value, dim_model)
        nn.init.xavier_normal_(self.output_linear.weight)
        self.dropout = nn.Dropout(dropout)
        self.query_linear.weight._asr_qkv = True      # hint for the flat-parameter layout: q/k/v weights adjacent

    def forward(self, query, key, value, mask=None, key_len=None, key_pad=None, causal=False, row_keep=None,
                need_attn=True, kv_grad_box=None, kv_pre=None, rope=None):
        """kv_pre: (projections (B, Tk, 2 H dk) of `key` by this block's K | V weights, their shared gradient box, layer index) when the
        decoder ran all its layers' cross-attention projections as one GEMM (asr_hip.functions.cross_kv_all); `key` is then only a shape.
        rope: the (Tq, dim_key / 2, 2) slice of an ops.rope_table that rotates Q and K (--pos-encoding rope); self-attention only."""
        if key is not value:
            raise NotImplementedError("key and value must be the same tensor (as everywhere in the reference model)")
        if self.dim_key != self.dim_value or self.dim_key not in _HEAD_WIDTHS:
            if rope is not None:
                raise ValueError("rope needs dim_key == dim_value in %s, got %d and %d" % (list(_HEAD_WIDTHS), self.dim_key, self.dim_value))
            return self._forward_padded(query, key, mask, key_len, key_pad, causal, row_keep, need_attn)
        if rope is not None and (key is not query or kv_pre is not None):
            raise ValueError("rope is for self-attention only (query, key and value the same tensor, no kv_pre)")
        cfg = dict(H=self.num_heads, dk=self.dim_key, p=self.dropout.p if self.training else 0.0, key_len=key_len,
                   key_pad=key_pad if key_pad is not None else _mask_to_u8(mask), causal=causal, row_keep=row_keep,
                   want_attn=need_attn, kv_grad_box=kv_grad_box)
        if rope is not None:
            cfg["rope"] = rope
        q = _to_compute(query)
        kv = None if key is query else _to_compute(key)
        pre = None
        if kv_pre is not None:
            pre, cfg["kv_pre_box"], cfg["kv_pre_layer"] = kv_pre
            kv = kv.detach()              # a shape only: the encoder output's gradient leaves through CrossKVFn
        res = F_.MHAFn.apply(q, kv, self.query_linear.weight, self.query_linear.bias, self.key_linear.weight,
                             self.key_linear.bias, self.value_linear.weight, self.value_linear.bias,
                             self.output_linear.weight, self.output_linear.bias, self.layer_norm.weight,
                             self.layer_norm.bias, cfg, pre)
        if need_attn:
            return res[0], res[1]
        return res, None


    def _forward_padded(self, query, key, mask, key_len, key_pad, causal, row_keep, need_attn):
        """dim_key != dim_value (reference: common_layers.py:170-200 with separate widths): projections by LinearFn, heads zero-padded to
        the kernels' next head width (16 / 32 / 64) >= both, SDPAFn on the padded heads with the reference's temperature sqrt(dim_key), the first dim_value
        columns of every output head into the output projection, AddLNFn.  The pads and slices are torch views / copies on the device
        (autograd differentiates them): the compatibility path of a boundary footnote, not the tuned one."""
        import torch.nn.functional as TF
        H, dk, dv = self.num_heads, self.dim_key, self.dim_value
        fit = [w for w in _HEAD_WIDTHS if w >= max(dk, dv)]
        if not fit:
            raise NotImplementedError("attention heads wider than %d (dim_key %d, dim_value %d): the attention kernels contract 16, 32 or "
                                      "64 columns per head" % (_HEAD_WIDTHS[-1], dk, dv))
        d = fit[0]
        p = self.dropout.p if self.training else 0.0
        q_in, kv_in = _to_compute(query), _to_compute(key)
        B, Tq, _ = q_in.shape
        Tk = kv_in.shape[1]
        Q = F_.linear(q_in, self.query_linear.weight, self.query_linear.bias).view(B, Tq, H, dk)
        K = F_.linear(kv_in, self.key_linear.weight, self.key_linear.bias).view(B, Tk, H, dk)
        V = F_.linear(kv_in, self.value_linear.weight, self.value_linear.bias).view(B, Tk, H, dv)
        pad = lambda t, w: (TF.pad(t, (0, d - w)) if w < d else t).reshape(t.shape[0], t.shape[1], H * d).contiguous()
        cfg = dict(H=H, dk=d, scale=1.0 / float(dk) ** 0.5, p=p, key_len=key_len,
                   key_pad=key_pad if key_pad is not None else _mask_to_u8(mask), causal=causal, want_attn=need_attn)
        res = F_.SDPAFn.apply(pad(Q, dk), pad(K, dk), pad(V, dv), cfg)
        O, attn = (res if isinstance(res, tuple) else (res, None))
        O = O.view(B, Tq, H, d)[..., :dv].reshape(B, Tq, H * dv)
        y = F_.linear(O, self.output_linear.weight, self.output_linear.bias)
        out = F_.AddLNFn.apply(y, q_in, self.layer_norm.weight, self.layer_norm.bias, dict(p=p, row_keep=row_keep))
        return out, attn


class ScaledDotProductAttention(nn.Module):
    """forward(q, k, v, mask=None) on head-major (H*B, T, d) tensors (reference: common_layers.py:202-225), run by the
    fused attention kernel with H = 1 (no gradient path: the training graph goes through MultiHeadAttention)."""

    def __init__(self, temperature, attn_dropout=0.1):
        super().__init__()
        self.temperature = temperature
        self.dropout = nn.Dropout(attn_dropout)

    def forward(self, q, k, v, mask=None):
        d = q.shape[-1]
        p = self.dropout.p if self.training else 0.0
        from asr_hip import params as P
        o, _, attn = ops.attn_fwd(_to_compute(q).contiguous(), _to_compute(k).contiguous(), _to_compute(v).contiguous(),
                                  1, d, key_pad=_mask_to_u8(mask), scale=1.0 / float(self.temperature), p=p,
                                  seed=P.next_seed(), want_attn=True)
        return o, attn


class PositionwiseFeedForwardWithConv(nn.Module):
    """LN(dropout(W2 relu(W1 x)) + x) with the weights stored as Conv1d(k=1) (reference: common_layers.py:124-142)."""

    def __init__(self, dim_model, dim_hidden, dropout=0.1):
        super().__init__()
        self.conv_1 = nn.Conv1d(dim_model, dim_hidden, 1)
        self.conv_2 = nn.Conv1d(dim_hidden, dim_model, 1)
        self.dropout = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(dim_model)

    def forward(self, x, row_keep=None):
        cfg = dict(p=self.dropout.p if self.training else 0.0, row_keep=row_keep)
        return F_.FFNFn.apply(_to_compute(x), self.conv_1.weight, self.conv_1.bias, self.conv_2.weight, self.conv_2.bias,
                              self.layer_norm.weight, self.layer_norm.bias, cfg)


POS_ENCODINGS = ("abs", "rope")


def check_pos_encoding(pos_encoding, dim_key=None, dim_value=None, rank=0):
    """--pos-encoding: abs (the reference's sinusoid, added once after the input projection) or rope (rotary position embedding of Q and K
    in every encoder self-attention, csrc/rope.hip).  rope rotates whole heads of the attention kernels' own widths, so it needs
    --dim-key == --dim-value in {16, 32, 64} (not the padded compatibility path); the low-rank encoder (--rank) has no such hook."""
    pe = "abs" if pos_encoding is None else str(pos_encoding)
    if pe not in POS_ENCODINGS:
        raise ValueError("--pos-encoding must be one of %s, got %r" % (", ".join(POS_ENCODINGS), pos_encoding))
    if pe == "abs":
        return pe
    if rank and rank > 0:
        raise ValueError("--pos-encoding rope with --rank %d is not supported: the Low-Rank Transformer's attention has no rotation of "
                         "Q and K" % rank)
    if dim_key is not None and dim_value is not None and dim_key != dim_value:
        raise ValueError("--pos-encoding rope needs --dim-key == --dim-value, got --dim-key %d --dim-value %d" % (dim_key, dim_value))
    if dim_key is not None and dim_key not in _HEAD_WIDTHS:
        raise ValueError("--pos-encoding rope needs --dim-key in %s, got --dim-key %d" % (list(_HEAD_WIDTHS), dim_key))
    return pe


CONV_MODULE_KERNELS = range(3, 32, 2)          # odd 3 .. 31: what csrc/convmod.hip keeps in registers per lane


def check_conv_module_kernel(kernel_size, dim_model=None, rank=0):
    """--conv-module-kernel K: 0 (no module) or odd with 3 <= K <= 31; the kernels take channels in whole 16-byte chunks (dim_model % 8 == 0);
    the low-rank encoder (--rank) has no such module."""
    K = int(kernel_size or 0)
    if K == 0:
        return 0
    if K not in CONV_MODULE_KERNELS:
        raise ValueError("--conv-module-kernel must be 0 (off) or odd with 3 <= K <= 31, got %d" % K)
    if dim_model is not None and dim_model % 8 != 0:
        raise ValueError("--conv-module-kernel %d needs --dim-model to be a multiple of 8, got %d" % (K, dim_model))
    if rank and rank > 0:
        raise ValueError("--conv-module-kernel %d with --rank %d is not supported: the Low-Rank Transformer's encoder layers have no "
                         "convolution module" % (K, rank))
    return K


class ConvolutionModule(nn.Module):
    """ConvolutionModule(dim_model, kernel_size, dropout): the convolution module of the Conformer (arXiv:2005.08100) as a post-LN
    sub-layer, LN(dropout(W2 swish(dwconv_K(glu(W1 x)))) + x) * row_keep, without the paper's BatchNorm.  The
    depthwise convolution sees zeros at and behind each utterance's length (`key_len`, the length the layer hands to attention).
    No reference code: the reference has no such module."""

    def __init__(self, dim_model, kernel_size, dropout=0.1):
        super().__init__()
        kernel_size = check_conv_module_kernel(kernel_size, dim_model)
        if kernel_size == 0:
            raise ValueError("ConvolutionModule needs a kernel size (odd, 3 <= K <= 31)")
        self.dim_model, self.kernel_size = dim_model, kernel_size
        self.pointwise_1 = nn.Linear(dim_model, 2 * dim_model)
        self.depthwise = nn.Conv1d(dim_model, dim_model, kernel_size, padding=(kernel_size - 1) // 2, groups=dim_model)
        self.pointwise_2 = nn.Linear(dim_model, dim_model)
        self.dropout = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(dim_model)
        self.depthwise.weight._asr_keep_init = True       # (D,1,K) is no matrix: the model's closing xavier pass leaves it alone

    def forward(self, x, key_len=None, row_keep=None):
        B, T, _ = x.shape
        if key_len is None:           # reference-style call with materialised masks: every frame is a frame
            key_len = torch.full((B,), T, device=x.device, dtype=torch.int32)
        cfg = dict(p=self.dropout.p if self.training else 0.0, row_keep=row_keep, key_len=key_len)
        return F_.ConvModuleFn.apply(_to_compute(x), self.pointwise_1.weight, self.pointwise_1.bias, self.depthwise.weight,
                                     self.depthwise.bias, self.pointwise_2.weight, self.pointwise_2.bias, self.layer_norm.weight,
                                     self.layer_norm.bias, cfg)


class PositionwiseFeedForward(nn.Module):
    """Linear variant (reference: common_layers.py:100-122; unused by the reference model, kept for the API)."""

    def __init__(self, dim_model, dim_ff, dropout=0.1):
        super().__init__()
        self.linear_1 = nn.Linear(dim_model, dim_ff)
        self.linear_2 = nn.Linear(dim_ff, dim_model)
        self.dropout = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(dim_model)

    def forward(self, x, row_keep=None):
        cfg = dict(p=self.dropout.p if self.training else 0.0, row_keep=row_keep)
        return F_.FFNFn.apply(_to_compute(x), self.linear_1.weight, self.linear_1.bias, self.linear_2.weight,
                              self.linear_2.bias, self.layer_norm.weight, self.layer_norm.bias, cfg)


# ================================================================================================ low-rank variant
# BASELINE configs[4] / SURVEY 8(f) #4: the Low-Rank Transformer of the reference's authors (arXiv:1910.13923, cited in the
# reference README; the reference tree holds no code for it -- parity unpinned, checked against the test suite's CPU
# restatement).  Every projection W (out, in) of the attention and feed-forward sub-layers is replaced by a linear
# encoder-decoder unit V (out, r) . U (r, in) with no non-linearity in between: 2 r (in + out) instead of in * out weights.
class LowRankLinear(nn.Module):
    """y = V (U x) + b.  state_dict keys: <name>.u.weight (rank, in), <name>.v.weight (out, rank), <name>.v.bias."""

    def __init__(self, dim_in, dim_out, rank, bias=True):
        super().__init__()
        self.u = nn.Linear(dim_in, rank, bias=False)
        self.v = nn.Linear(rank, dim_out, bias=bias)
        nn.init.xavier_normal_(self.u.weight)
        nn.init.xavier_normal_(self.v.weight)

    def forward(self, x, relu=False, input_is_relu=False):
        h = F_.LinearActFn.apply(_to_compute(x), self.u.weight, None, False, input_is_relu)
        return F_.LinearActFn.apply(h, self.v.weight, self.v.bias, relu, False)


class LowRankMultiHeadAttention(nn.Module):
    """MultiHeadAttention (reference: common_layers.py:170-200) with low-rank query / key / value / output projections."""

    def __init__(self, num_heads, dim_model, dim_key, dim_value, rank, dropout=0.1):
        super().__init__()
        self.num_heads, self.dim_model, self.dim_key, self.dim_value, self.rank = num_heads, dim_model, dim_key, dim_value, rank
        self.query_linear = LowRankLinear(dim_model, num_heads * dim_key, rank)
        self.key_linear = LowRankLinear(dim_model, num_heads * dim_key, rank)
        self.value_linear = LowRankLinear(dim_model, num_heads * dim_value, rank)
        self.output_linear = LowRankLinear(num_heads * dim_value, dim_model, rank)
        self.layer_norm = nn.LayerNorm(dim_model)
        self.dropout = nn.Dropout(dropout)

    def forward(self, query, key, value, mask=None, key_len=None, key_pad=None, causal=False, row_keep=None,
                need_attn=False, kv_grad_box=None):
        if key is not value:
            raise NotImplementedError("key and value must be the same tensor (as everywhere in the reference model)")
        p = self.dropout.p if self.training else 0.0
        q_in, kv_in = _to_compute(query), _to_compute(key)
        cfg = dict(H=self.num_heads, dk=self.dim_key, p=p, key_len=key_len,
                   key_pad=key_pad if key_pad is not None else _mask_to_u8(mask), causal=causal)
        Q, K, V = self.query_linear(q_in), self.key_linear(kv_in), self.value_linear(kv_in)
        O = F_.SDPAFn.apply(Q.contiguous(), K.contiguous(), V.contiguous(), cfg)
        y = self.output_linear(O)
        out = F_.AddLNFn.apply(y, q_in, self.layer_norm.weight, self.layer_norm.bias, dict(p=p, row_keep=row_keep))
        return out, None


class LowRankPositionwiseFeedForward(nn.Module):
    """LN(dropout(W2 relu(W1 x)) + x) (reference: common_layers.py:124-142) with W1, W2 low rank."""

    def __init__(self, dim_model, dim_hidden, rank, dropout=0.1):
        super().__init__()
        self.linear_1 = LowRankLinear(dim_model, dim_hidden, rank)
        self.linear_2 = LowRankLinear(dim_hidden, dim_model, rank)
        self.dropout = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(dim_model)

    def forward(self, x, row_keep=None):
        p = self.dropout.p if self.training else 0.0
        xc = _to_compute(x)
        h = self.linear_1(xc, relu=True)
        y = self.linear_2(h, input_is_relu=True)
        return F_.AddLNFn.apply(y, xc, self.layer_norm.weight, self.layer_norm.bias, dict(p=p, row_keep=row_keep))
