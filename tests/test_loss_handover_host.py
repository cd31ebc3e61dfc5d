"""The two halves of the logit hand-over that the loss Functions share (asr_hip/functions.py: _claim_logits, _hand_back), on the host with a
stub context and a stub backward: no kernel runs.  The expectations restate the protocol written at the helpers, not their code."""
import types

import torch


def _bwd(M, V, calls):
    """A stand-in for ops.*_bwd: records how it was asked and returns what the wrappers return (an (M,V) view of a pad-8 buffer, or the
    whole pad-64 buffer)."""
    def bwd(out_dtype=torch.float32, pad=8):
        calls.append((out_dtype, pad))
        buf = torch.arange(M * ((V + pad - 1) // pad * pad), dtype=torch.float32).reshape(M, -1).to(out_dtype)
        return buf if pad == 64 else buf[:, :V]
    return bwd


def test_with_a_box_the_gradient_goes_into_it_and_a_stride_0_zero_comes_back():
    from asr_hip import functions as Fn
    calls, box = [], {}
    got = Fn._hand_back(types.SimpleNamespace(handover=box), _bwd(6, 37, calls), (2, 3, 37))
    assert calls == [(torch.bfloat16, 64)]                       # ONE backward launch, in the form the data-gradient GEMM reads
    want = _bwd(6, 37, [])(out_dtype=torch.bfloat16, pad=64)
    assert list(box) == ["dy"] and box["dy"].dtype == torch.bfloat16 and box["dy"].shape == (6, 64) and torch.equal(box["dy"], want)
    assert got.shape == (2, 3, 37) and got.stride() == (0, 0, 0) and got.dtype == torch.float32 and not got.any()


def test_without_a_box_the_fp32_gradient_comes_back_in_the_formal_shape():
    from asr_hip import functions as Fn
    calls = []
    got = Fn._hand_back(types.SimpleNamespace(handover=None), _bwd(6, 37, calls), (2, 3, 37))
    assert calls == [(torch.float32, 8)]
    want = _bwd(6, 37, [])()
    assert got.shape == (2, 3, 37) and got.dtype == torch.float32 and torch.equal(got.reshape(6, 37), want)


def test_the_claim_is_made_only_for_an_input_that_needs_a_gradient_and_empties_the_slot(monkeypatch):
    from asr_hip import functions as Fn
    slot = Fn._Handover()
    monkeypatch.setattr(Fn, "_logit_handover", slot)
    logits, box = torch.zeros(4, 5), {}
    slot.leave(logits, logits, box)
    ctx = types.SimpleNamespace(needs_input_grad=(False,))
    Fn._claim_logits(ctx, logits)
    assert ctx.handover is None and slot[0] is not None          # no gradient wanted: the box stays for whoever wants one
    ctx = types.SimpleNamespace(needs_input_grad=(True,))
    Fn._claim_logits(ctx, logits.view(2, 2, 5))
    assert ctx.handover is box and slot[0] is None               # a view of all of it claims; the slot is empty afterwards
    slot.leave(logits, logits, box)
    Fn._claim_logits(ctx, torch.zeros(4, 5))
    assert ctx.handover is None and slot[0] is None              # another tensor finds nothing and still empties the slot
