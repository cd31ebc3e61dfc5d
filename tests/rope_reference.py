"""Rotary position embedding (RoPE, arXiv:2104.09864) restated in plain torch: the yardstick of tests/test_rope_host.py,
tests/test_gpu_rope.py and tests/test_gpu_rope_model.py.  Nothing here calls the library.

  table64(n, d)                          (n, d/2, 2) float64 [cos, sin] of the angle t * 10000^(-2i/d)
  rope64(x, cs, nheads, d, inverse)      the rotation in float64, out of place, differentiable; cs is cast up (the fp32 table the kernel reads,
                                         or table64 itself)
  torch_rope_(x, cs, nheads, d, inverse) the signature of asr_hip.ops.rope_ as fp32 torch, in place
  mha_block(x, w, cs, H, dk, key_len)    the self-attention sub-layer at dropout 0 in the dtype of its arguments: Q | K | V projections, rotation of
                                         Q and K, softmax masked by key_len, output projection, residual + LayerNorm + row mask
  mha_block64                            the same with everything cast to float64
Pairs are interleaved: (x[2i], x[2i+1]) of each head, rotated by cs[t, i]."""
import torch

PARAMS = ("query_linear.weight", "query_linear.bias", "key_linear.weight", "key_linear.bias", "value_linear.weight", "value_linear.bias",
          "output_linear.weight", "output_linear.bias", "layer_norm.weight", "layer_norm.bias")


def table64(n, d, base=10000.0):
    t = torch.arange(n, dtype=torch.float64).unsqueeze(1)
    inv = torch.pow(torch.tensor(float(base), dtype=torch.float64), -torch.arange(0, d, 2, dtype=torch.float64) / d)
    ang = t * inv.unsqueeze(0)
    return torch.stack((torch.cos(ang), torch.sin(ang)), dim=-1)


def _rotate(x, cs, nheads, d, inverse):
    B, T, W = x.shape
    assert W == nheads * d and tuple(cs.shape) == (T, d // 2, 2)
    xr = x.reshape(B, T, nheads, d // 2, 2)
    c, s = cs[None, :, None, :, 0], cs[None, :, None, :, 1]
    if inverse:
        s = -s
    x0, x1 = xr[..., 0], xr[..., 1]
    return torch.stack((x0 * c - x1 * s, x0 * s + x1 * c), dim=-1).reshape(B, T, W)


def rope64(x, cs, nheads, d, inverse=False):
    return _rotate(x.double(), cs.double(), nheads, d, inverse)


def torch_rope_(x, cs, nheads, d, inverse=False):
    assert x.dim() == 3 and x.stride(2) == 1 and cs.dtype == torch.float32
    with torch.no_grad():
        x.copy_(_rotate(x.float(), cs, nheads, d, inverse))
    return x


def mha_block(x, w, cs, H, dk, key_len):
    """x (B,T,D), w = the ten tensors of PARAMS in order, cs (T, dk/2, 2) or None (no rotation), key_len (B) integers.  Every operand in
    one dtype, which the arithmetic follows."""
    Wq, bq, Wk, bk, Wv, bv, Wo, bo, gamma, beta = w
    B, T, D = x.shape
    Q, K, V = x @ Wq.t() + bq, x @ Wk.t() + bk, x @ Wv.t() + bv
    if cs is not None:
        cs = cs.to(x.dtype)
        Q, K = _rotate(Q, cs, H, dk, False), _rotate(K, cs, H, dk, False)
    heads = lambda t: t.reshape(B, T, H, dk).permute(0, 2, 1, 3)
    scores = heads(Q) @ heads(K).transpose(-1, -2) / dk ** 0.5
    pad = torch.arange(T, device=x.device)[None, :] >= key_len.to(x.device).long()[:, None]              # (B, T)
    attn = torch.softmax(scores.masked_fill(pad[:, None, None, :], float("-inf")), dim=-1)
    O = (attn @ heads(V)).permute(0, 2, 1, 3).reshape(B, T, H * dk)
    z = O @ Wo.t() + bo + x
    out = torch.nn.functional.layer_norm(z, (D,), gamma, beta, 1e-5)
    return out * (~pad)[:, :, None].to(x.dtype)


def mha_block64(x, w, cs, H, dk, key_len):
    return mha_block(x.double(), [t.double() for t in w], None if cs is None else cs.double(), H, dk, key_len)
