"""The convolution module's three kernels restated from their definition (csrc/convmod.hip), in NumPy at the
dtype of the inputs (float64 unless a test asks otherwise), plus the same thing as a plain-torch autograd composition.

  u (B,T,2D) = [a | gate],  P = (K-1)/2,  len_b clamped to [0,T]
  g[b,t,c] = a * sigma(gate)                          t < len_b;  0 for t >= len_b and outside [0,T)
  s[b,t,c] = bd[c] + sum_k wd[c,k] * g[b,t+k-P,c]     (cross-correlation, as torch's Conv1d)
  v[b,t,c] = s * sigma(s)                             t < len_b;  0 for t >= len_b
  ds = dv * sigma(s) * (1 + s * (1 - sigma(s)))       t < len_b;  else 0
  dg[t'] = sum_k wd[c,k] * ds[t'+P-k]                 t' < len_b; else 0
  du[..., :D] = dg * sigma(gate);   du[..., D:] = dg * a * sigma(gate) * (1 - sigma(gate))
  dwd[c,k] = sum_{b,t} ds[b,t,c] * g[b,t+k-P,c];   dbd[c] = sum_{b,t} ds[b,t,c]

Frames t >= len_b of u and dv are never read (np.where selects, it does not multiply): an inf or 1e30 there changes nothing.
"""
import numpy as np
import torch
import torch.nn.functional as TF


def sigmoid(x):
    """1 / (1 + exp(-x)): exactly 1 once exp(-x) falls below half an ulp of 1, exactly 0 once exp(-x) overflows."""
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _keep(lens, T):
    lens = np.clip(np.asarray(lens, dtype=np.int64), 0, T)
    return (np.arange(T)[None, :] < lens[:, None])[:, :, None]             # (B,T,1)


def glu_masked(u, lens):
    B, T, D2 = u.shape
    D = D2 // 2
    keep = _keep(lens, T)
    a = np.where(keep, u[..., :D], 0)
    gate = np.where(keep, u[..., D:], 0)
    return np.where(keep, a * sigmoid(gate), 0).astype(u.dtype), a, gate, keep


def forward(u, wd, bd, lens):
    """-> (s, v, g): wd (D,K) or (D,1,K)."""
    B, T, D2 = u.shape
    D = D2 // 2
    wd = np.asarray(wd).reshape(D, -1)
    K = wd.shape[1]
    P = (K - 1) // 2
    g, _, _, keep = glu_masked(u, lens)
    gp = np.zeros((B, T + 2 * P, D), dtype=u.dtype)
    gp[:, P:P + T] = g
    s = np.broadcast_to(np.asarray(bd, dtype=u.dtype)[None, None, :], (B, T, D)).copy()
    for k in range(K):
        s += wd[None, None, :, k].astype(u.dtype) * gp[:, k:k + T]
    v = np.where(keep, s * sigmoid(s), 0).astype(u.dtype)
    return s, v, g


def swish_grad(s):
    sg = sigmoid(s)
    return sg * (1 + s * (1 - sg))


def backward(dv, s, u, wd, lens):
    """-> (du, dwd (D,K), dbd) from the output gradient, the SAVED s as given, and u."""
    B, T, D2 = u.shape
    D = D2 // 2
    wd = np.asarray(wd).reshape(D, -1).astype(u.dtype)
    K = wd.shape[1]
    P = (K - 1) // 2
    g, a, gate, keep = glu_masked(u, lens)
    ds = np.where(keep, np.where(keep, dv, 0) * swish_grad(np.where(keep, s, 0)), 0).astype(u.dtype)
    dsp = np.zeros((B, T + 2 * P, D), dtype=u.dtype)
    dsp[:, P:P + T] = ds
    gp = np.zeros((B, T + 2 * P, D), dtype=u.dtype)
    gp[:, P:P + T] = g
    dg = np.zeros((B, T, D), dtype=u.dtype)
    dwd = np.zeros((D, K), dtype=u.dtype)
    for k in range(K):
        dg += wd[None, None, :, k] * dsp[:, 2 * P - k:2 * P - k + T]        # ds[t' + P - k]
        dwd[:, k] = (ds * gp[:, k:k + T]).sum(axis=(0, 1))                  # g[t + k - P]
    dg = np.where(keep, dg, 0)
    sg = sigmoid(gate)
    du = np.concatenate([dg * sg, dg * a * (sg * (1 - sg))], axis=-1).astype(u.dtype)
    return du, dwd, ds.sum(axis=(0, 1))


def torch_core(u, wd, bd, lens):
    """The same forward as a torch composition autograd differentiates: F.glu -> zero fill -> F.conv1d(groups=D, padding=P) -> F.silu ->
    zero fill.  u (B,T,2D), wd (D,1,K), bd (D), lens (B) -> (s, v), both (B,T,D), in u's dtype on u's device."""
    B, T, D2 = u.shape
    D = D2 // 2
    K = wd.shape[-1]
    keep = (torch.arange(T, device=u.device)[None, :] < torch.as_tensor(lens, device=u.device).clamp(0, T)[:, None]).unsqueeze(-1)
    g = torch.where(keep, TF.glu(torch.where(keep, u, torch.zeros((), dtype=u.dtype, device=u.device)), dim=-1),
                    torch.zeros((), dtype=u.dtype, device=u.device))
    s = TF.conv1d(g.transpose(1, 2), wd.reshape(D, 1, K), bd, padding=(K - 1) // 2, groups=D).transpose(1, 2)
    v = torch.where(keep, TF.silu(s), torch.zeros((), dtype=u.dtype, device=u.device))
    return s, v


def torch_module_forward(mod, x, key_len=None, row_keep=None):
    """ConvolutionModule.forward as plain torch ops on the module's own parameters (dropout 0): the autograd composition the model parity
    test swaps in.  x (B,T,D) -> LN(W2 v + b2 + x) * row_keep, in fp32."""
    B, T, D = x.shape
    xf = x.float()
    lens = key_len if key_len is not None else torch.full((B,), T, device=x.device, dtype=torch.int32)
    u = TF.linear(xf, mod.pointwise_1.weight, mod.pointwise_1.bias)
    _, v = torch_core(u, mod.depthwise.weight, mod.depthwise.bias, lens.to(torch.int64))
    y = TF.linear(v, mod.pointwise_2.weight, mod.pointwise_2.bias)
    out = TF.layer_norm(y + xf, (D,), mod.layer_norm.weight, mod.layer_norm.bias, 1e-5)
    if row_keep is not None:
        out = out * row_keep.reshape(B, T, 1).to(out.dtype)
    return out.to(x.dtype)


def random_case(B, T, D, K, lens, seed, dtype=np.float64):
    r = np.random.RandomState(seed)
    u = r.standard_normal((B, T, 2 * D)).astype(dtype)
    wd = (r.standard_normal((D, K)) / np.sqrt(K)).astype(dtype)
    bd = (0.1 * r.standard_normal(D)).astype(dtype)
    dv = r.standard_normal((B, T, D)).astype(dtype)
    return u, wd, bd, dv, np.asarray(lens, dtype=np.int64)


def exact_case(B, T, D, K, lens, seed, dtype=np.float64):
    """The saturated integer case: gate = 40 (sigma = 1 exactly), a in [-2,2], wd in {-1,0,1}, bd = 96, dv in [-2,2].  Then
    s in [96 - 62, 96 + 62] = [34, 158] (sigma(s) = 1, swish' = 1), v = s, ds = dv, the gate half of du is 0 and v, du, dwd, dbd are
    order-free sums of small integers."""
    r = np.random.RandomState(seed)
    a = r.randint(-2, 3, size=(B, T, D))
    u = np.concatenate([a, np.full((B, T, D), 40)], axis=-1).astype(dtype)
    wd = r.randint(-1, 2, size=(D, K)).astype(dtype)
    bd = np.full(D, 96, dtype=dtype)
    dv = r.randint(-2, 3, size=(B, T, D)).astype(dtype)
    return u, wd, bd, dv, np.asarray(lens, dtype=np.int64)
