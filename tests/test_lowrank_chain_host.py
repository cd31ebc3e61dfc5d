"""The references tests/test_gpu_lowrank_widths.py compares bits against, checked where there is no GPU: tests/lowrank_reference.py
against oracle/asr_oracle.py:proj and float64 autograd (R the identity), the exactness premise of every case of that file's section 1
(test_gpu_gemm_exact._premise), and the e4m3 decoder / spacing its fp8 section decodes the product's bytes with."""
import pytest
import torch

import lowrank_reference as R
import test_gpu_lowrank_widths as W
from test_gpu_lowrank import _e4m3_decode


def _random_chain(seed, M=37, dims=((24, 40, True, False), (40, 16, False, True)), r=5):
    g = torch.Generator().manual_seed(seed)
    pairs = [{"U": torch.randn(r, din, generator=g, dtype=torch.float64), "V": torch.randn(dout, r, generator=g, dtype=torch.float64),
              "b": torch.randn(dout, generator=g, dtype=torch.float64), "relu": relu, "input_is_relu": inrelu} for din, dout, relu, inrelu in dims]
    return {"x": torch.randn(M, dims[0][0], generator=g, dtype=torch.float64), "dy": torch.randn(M, dims[-1][1], generator=g, dtype=torch.float64),
            "pairs": pairs, "nz": torch.arange(M)}


@pytest.mark.parametrize("dims", [((24, 40, False, False),), ((24, 40, True, False), (40, 16, False, True))], ids=["one-pair", "relu-chain"])
def test_reference_is_the_oracle_projection_and_its_autograd_gradient(dims):
    """R = identity: every pair's forward is oracle.asr_oracle.proj of the same weights, and the chain's dx, dU, dV, db are the float64
    autograd gradients of sum(dy * chain(x)) -- the ReLU of a `relu` pair differentiated by autograd, its mask applied by the consuming
    pair's `input_is_relu` in the reference (as functions.LinearActFn splits it)."""
    from oracle import asr_oracle as O
    data = _random_chain(3, dims=dims)
    ref = W.pair_reference(data, None)
    leaves = {}
    for i, p in enumerate(data["pairs"]):
        leaves.update({"p%d.u.weight" % i: p["U"].clone().requires_grad_(True), "p%d.v.weight" % i: p["V"].clone().requires_grad_(True),
                       "p%d.v.bias" % i: p["b"].clone().requires_grad_(True)})
    x = data["x"].clone().requires_grad_(True)
    t = x
    for i, (p, (xi, h, y)) in enumerate(zip(data["pairs"], ref["acts"])):
        t = O.proj(leaves, "p%d" % i, t)
        if p["relu"]:
            t = torch.relu(t)
        assert torch.allclose(y, t.detach(), rtol=1e-12, atol=1e-12)
        assert torch.allclose(h, xi @ p["U"].t(), rtol=1e-12, atol=1e-12)
    if not data["pairs"][-1]["relu"]:
        (t * data["dy"]).sum().backward()
        assert torch.allclose(ref["dx"], x.grad, rtol=1e-11, atol=1e-11)
        for i, gr in enumerate(ref["grads"]):
            for key, name in (("dU", "u.weight"), ("dV", "v.weight"), ("db", "v.bias")):
                assert torch.allclose(gr[key], leaves["p%d.%s" % (i, name)].grad, rtol=1e-11, atol=1e-11), (i, key)
        assert float(x.grad.abs().max()) > 0


def test_rounding_is_applied_once_per_stored_activation():
    """bf16 mode: h and dh are bf16 numbers; y and dx come back un-rounded (the caller rounds them, as the product stores them)."""
    data = _random_chain(4)
    ref = W.pair_reference(data, torch.bfloat16)
    for (x, h, y), gr in zip(ref["acts"], ref["grads"]):
        assert torch.equal(h.to(torch.bfloat16).double(), h) and torch.equal(gr["dh"].to(torch.bfloat16).double(), gr["dh"])
        assert not torch.equal(y.to(torch.bfloat16).double(), y)
    x1 = ref["acts"][1][0]
    assert torch.equal(x1, ref["acts"][0][2].to(torch.bfloat16).double())            # the second pair reads the ROUNDED output of the first


_PREMISE_CASES = sorted({(s, m, W.route_dtype(r)) for s, m, r in W.pair_cases()}, key=str)


@pytest.mark.parametrize("shape,M,dtype", _PREMISE_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_integer_data_meets_the_exactness_premise(shape, M, dtype):
    """Every (shape, M, compute dtype) the GPU file runs: the seeded integer data keeps every product of the pair -- forward, data
    gradient, weight and bias gradients -- exact in fp32 in any order (W.check_premise; the GPU test asserts the same before it launches)."""
    data = W.pair_data(shape, M)
    ref = W.pair_reference(data, dtype)
    W.check_premise("%s M=%d %s" % (shape, M, dtype), data, ref)
    # and the data is not trivial: every output column carries a value; dy is dense up to the shape's budget, and beyond it every stage of
    # 32 rows holds a non-zero row of dy; the first and the LAST row (the one that opens a tile, stage or slice past a threshold) have a
    # non-zero dy and a non-zero dx, and so has every row dy touches
    assert float((ref["y"] != 0).double().mean()) > 0.2 and bool((ref["grads"][0]["dU"] != 0).any(1).all())
    live = (data["dy"] != 0).any(1)
    if M <= W.NZ_BUDGET[shape]:
        assert bool(live.all())
    pad = torch.zeros((M + 31) // 32 * 32, dtype=torch.bool)
    pad[:M] = live
    assert bool(pad.view(-1, 32).any(1).all()), "a stage of 32 rows without a gradient"
    assert bool(live[0]) and bool(live[M - 1])
    dx_live = (ref["dx"] != 0).any(1)
    assert bool(dx_live[0]) and bool(dx_live[M - 1]) and bool(dx_live[live].all())
    assert torch.equal(live.nonzero().flatten(), data["nz"])


def test_every_threshold_side_is_a_case():
    """The M of the module docstring's threshold table are in the case list, both sides of each."""
    cases = set(W.pair_cases())
    for (shape, route), ms in W.ROUTE_M.items():
        assert len(ms) % 2 == 0 and all(b == a + 1 for a, b in zip(ms[0::2], ms[1::2])), (shape, route, ms)
        for m in tuple(ms) + W.COMMON_M:
            assert (shape, m, route) in cases


def test_kernel_coverage_diff_lists_what_only_the_first_trace_launched(tmp_path, capsys):
    """tools/kernel_coverage.py diff (host only): a kernel the first trace names mangled (with `.kd`) and the second demangled is the same
    kernel; one only the first trace dispatched is listed with its dispatches; --only filters by the demangled name."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(root, "tools", "kernel_coverage.py"))
    kc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kc)
    ring = "_ZN12_GLOBAL__N_116gemm_glds_kernelIttLi64ELi64ELi3EEEvNS_8GemmArgsE"
    fold = "_ZN12_GLOBAL__N_116tn_reduce_kernelEPKfPfliiiii"
    head = '"Kind","Agent_Id","Kernel_Id","Kernel_Name","Start_Timestamp","End_Timestamp"'
    a, b = str(tmp_path / "a.csv"), str(tmp_path / "b.csv")
    with open(a, "w") as fh:
        fh.write("\n".join([head, '"KERNEL_DISPATCH",4,7,"%s.kd",1,2' % ring, '"KERNEL_DISPATCH",4,8,"%s.kd",3,4' % fold,
                            '"KERNEL_DISPATCH",4,8,"%s.kd",5,6' % fold, '"KERNEL_DISPATCH",4,9,"adam_kernel(float*)",7,8']) + "\n")
    with open(b, "w") as fh:
        fh.write("\n".join([head, '"KERNEL_DISPATCH",4,7,"void (anonymous namespace)::gemm_glds_kernel<unsigned short, unsigned short, 64, 64, 3>'
                                  '((anonymous namespace)::GemmArgs)",1,2']) + "\n")
    if kc.demangle([ring])[ring] == ring:
        pytest.skip("no c++filt on this machine: mangled and demangled names cannot be matched")
    assert kc.diff(a, b) == 1
    out = capsys.readouterr().out
    assert "never in the second: 2" in out and "tn_reduce_kernel" in out and "        2  " in out and "gemm_glds_kernel" not in out
    assert kc.diff(a, b, only="gemm|tn_") == 1 and "adam_kernel" not in capsys.readouterr().out
    assert kc.diff(b, a) == 0


def test_e4m3_decoder_and_spacing_agree_with_torch():
    """test_gpu_lowrank._e4m3_decode on all 256 bytes against torch.float8_e4m3fn, and W.e4m3_step (the half-step bound's spacing,
    tests/test_gpu_lowrank.py:112) against the gaps between neighbouring values.  The two NaN codes 0x7f / 0xff: the decoder has no NaN
    (it continues the pattern to +-480), so the GPU tests assert that no quantised operand holds one."""
    if not hasattr(torch, "float8_e4m3fn"):
        pytest.skip("this torch build has no float8_e4m3fn dtype")
    b = torch.arange(256, dtype=torch.uint8)
    want = b.view(torch.float8_e4m3fn).double()
    got = _e4m3_decode(b)
    nan = torch.isnan(want)
    assert nan.nonzero().flatten().tolist() == [0x7F, 0xFF]
    assert torch.equal(got[~nan], want[~nan])
    assert float(want[~nan].max()) == 448.0
    pos = got[:0x7F]                                     # 0 .. 448, increasing
    assert torch.equal(pos[1:] - pos[:-1], W.e4m3_step(pos[:-1]))
