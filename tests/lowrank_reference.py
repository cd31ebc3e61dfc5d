"""One factor pair of the Low-Rank Transformer (models/common_layers.py LowRankLinear: two asr_hip.functions.LinearActFn calls) restated in
float64 on the CPU, forward and backward, with the roundings of the product and nothing else of it:

    h  = R(x U^T)                         (M, r)    the first projection has no bias
    y  = act(h V^T + b)                   (M, out)  act = ReLU (`relu`) or the identity; the product stores R(y)
    dh = R(dy V)                          (M, r)    dy as LinearActFn.backward receives it: `relu` does NOT mask it here -- the mask of
                                                    a ReLU output is applied by the layer that consumes it (`input_is_relu`)
    dx = (dh U) * (x > 0 if input_is_relu else 1)   (M, in)   the product stores R(dx)
    dU = dh^T x,  dV = dy^T h,  db = column sums of dy        fp32 accumulation targets: never rounded to the compute dtype

R is ONE round-to-nearest-even to the compute dtype (`.to(torch.bfloat16)`), or the identity in fp32 mode.  y and dx are returned
un-rounded: a caller that compares bits rounds them itself (`.to(dtype)`), a caller that chains pairs feeds `R(y)` on.
tests/test_lowrank_chain_host.py holds this file against oracle/asr_oracle.py:proj and float64 autograd with R the identity.
"""
import torch


def rounder(dtype):
    """R of the module docstring for a compute dtype (None / float32: the identity)."""
    if dtype is None or dtype == torch.float32:
        return lambda t: t
    return lambda t: t.to(dtype).double()


def pair_forward(x, U, V, b, relu=False, dtype=None):
    """x (M, in), U (r, in), V (out, r), b (out) or None, all float64 -> (h, y): h = R(x U^T), y = act(h V^T + b) un-rounded."""
    assert x.dtype == U.dtype == V.dtype == torch.float64
    h = rounder(dtype)(x @ U.t())
    y = h @ V.t()
    if b is not None:
        y = y + b
    if relu:
        y = y.clamp_min(0.0)
    return h, y


def pair_backward(x, U, V, h, dy, input_is_relu=False, dtype=None):
    """-> dict(dh, dx, dU, dV, db) of the module docstring; h is pair_forward's (rounded) h, dx is un-rounded."""
    assert dy.dtype == torch.float64
    dh = rounder(dtype)(dy @ V)
    dx = dh @ U
    if input_is_relu:
        dx = dx * (x > 0).to(dx.dtype)
    return {"dh": dh, "dx": dx, "dU": dh.t() @ x, "dV": dy.t() @ h, "db": dy.sum(0)}
