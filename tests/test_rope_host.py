"""--pos-encoding rope on the host: the float64 restatement the GPU tests measure against (tests/rope_reference.py) held against the
properties that define a rotary embedding, and everything of the flag that needs no GPU -- the table, the flag, the model's keys, the
refused combinations, the checkpoint round trip."""
import os

import pytest
import torch

import rope_reference as R


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("B,T,nheads,d", [(1, 1, 1, 16), (2, 5, 3, 32), (3, 33, 10, 64)])
def test_rotation_keeps_pair_norms_and_inverse_undoes_it(B, T, nheads, d):
    x = _rand(B, T, nheads * d, seed=1)
    cs = R.table64(T, d)
    y = R.rope64(x, cs, nheads, d)
    n = lambda t: t.reshape(B, T, nheads * d // 2, 2).norm(dim=-1)
    assert (n(y) - n(x)).abs().max().item() <= 1e-12
    assert (R.rope64(y, cs, nheads, d, inverse=True) - x).abs().max().item() <= 1e-12
    assert T == 1 or (y - x).abs().max().item() > 0.1                  # (and it is a rotation, not the identity)


def test_pairs_are_interleaved_and_signs_are_the_papers():
    cs = torch.zeros(1, 8, 2, dtype=torch.float64)
    cs[0, :, 1] = 1.0                                                  # a quarter turn: (x0, x1) -> (-x1, x0)
    x = torch.arange(1.0, 33.0, dtype=torch.float64).reshape(1, 1, 32)
    y = R.rope64(x, cs, 2, 16)
    assert torch.equal(y[0, 0, 0::2], -x[0, 0, 1::2]) and torch.equal(y[0, 0, 1::2], x[0, 0, 0::2])
    yi = R.rope64(x, cs, 2, 16, inverse=True)
    assert torch.equal(yi[0, 0, 0::2], x[0, 0, 1::2]) and torch.equal(yi[0, 0, 1::2], -x[0, 0, 0::2])


@pytest.mark.parametrize("d", [16, 64])
def test_score_depends_on_the_offset_only(d):
    """<rope(q, t), rope(k, s)> from table rows (t, s) and from rows (t + delta, s + delta): the relative property."""
    n = 600
    cs = R.table64(n, d)
    q, k = _rand(1, 1, d, seed=2), _rand(1, 1, d, seed=3)
    worst = 0.0
    for t, s in ((0, 0), (3, 17), (40, 2), (99, 98)):
        ref = (R.rope64(q, cs[t:t + 1], 1, d) * R.rope64(k, cs[s:s + 1], 1, d)).sum()
        for delta in (1, 37, 250, 500):
            got = (R.rope64(q, cs[t + delta:t + delta + 1], 1, d) * R.rope64(k, cs[s + delta:s + delta + 1], 1, d)).sum()
            worst = max(worst, (got - ref).abs().item())
    assert worst <= 1e-9, worst


def test_table_row_zero_is_the_identity_and_ops_table_is_its_fp32_cast():
    from asr_hip import ops
    for n, d in ((1, 16), (75, 64), (4000, 32)):
        t64 = R.table64(n, d)
        assert t64.dtype == torch.float64 and tuple(t64.shape) == (n, d // 2, 2)
        assert torch.equal(t64[0, :, 0], torch.ones(d // 2, dtype=torch.float64)) and not t64[0, :, 1].any()
        got = ops.rope_table(n, d)
        assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, t64.to(torch.float32))
    assert abs(R.table64(2, 16)[1, 1, 1].item() - torch.sin(torch.tensor(10000.0 ** (-2 / 16), dtype=torch.float64)).item()) < 1e-15


def _block_case(B, T, H, dk, D, seed):
    x = _rand(B, T, D, seed=seed)
    w = []
    for i, name in enumerate(R.PARAMS):
        rows = D if name.startswith(("output", "layer_norm")) else H * dk
        cols = H * dk if name.startswith("output") else D
        shape = (rows, cols) if name.endswith("linear.weight") else (rows,)
        w.append((1.0 if name == "layer_norm.weight" else 0.0) + 0.3 * _rand(*shape, seed=seed + 1 + i))
    return x, w


def test_block_is_invariant_under_a_shift_of_the_table():
    B, T, H, dk, D = 2, 19, 2, 16, 32
    x, w = _block_case(B, T, H, dk, D, seed=7)
    cs = R.table64(64, dk)
    lens = torch.tensor([19, 11])
    a = R.mha_block64(x, w, cs[:T], H, dk, lens)
    b = R.mha_block64(x, w, cs[37:37 + T], H, dk, lens)
    assert (a - b).abs().max().item() <= 1e-10
    assert (a - R.mha_block64(x, w, None, H, dk, lens)).abs().max().item() > 1e-3          # (the rotation is live in the block)
    assert not a[1, 11:].any() and a[1, :11].abs().min().item() > 0


def test_torch_rope_is_the_restatement_in_fp32():
    x = _rand(2, 5, 96, seed=9).float()
    cs = R.table64(5, 32).float()
    ref = R.rope64(x, cs, 3, 32)
    y = x.clone()
    assert R.torch_rope_(y, cs, 3, 32) is y
    assert (y.double() - ref).abs().max().item() <= 4 * 2.0 ** -24 * x.abs().max().item() * 2
    assert (R.torch_rope_(y, cs, 3, 32, inverse=True) - x).abs().max().item() <= 1e-5


# ------------------------------------------------------------------------------------------------ the feature, without a GPU
TINY = ("--num-layers 2 --num-heads 2 --dim-model 32 --dim-key 16 --dim-value 16 --dim-inner 64 --dim-emb 32 --feat_extractor vgg_cnn "
        "--tgt-max-len 12 --src-max-len 64 --dropout 0.0").split()


def _labels(V=32):
    from utils import constant
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + [chr(0x4E00 + i) for i in range(V - 3)]
    return {c: i for i, c in enumerate(chars)}, {i: c for i, c in enumerate(chars)}


def _model(extra, base=TINY):
    from utils import constant
    from utils.functions import init_transformer_model
    args = constant.parse(list(base) + extra)
    return args, init_transformer_model(args, *_labels())


def _with(flags, **kw):
    flags = list(flags)
    for k, v in kw.items():
        flags[flags.index("--" + k.replace("_", "-")) + 1] = str(v)
    return flags


@pytest.fixture(autouse=True)
def _restore_args():
    from utils import constant
    keep = (constant.args, constant.explicit, constant.USE_CUDA)
    yield
    constant.args, constant.explicit, constant.USE_CUDA = keep


def test_flag_defaults_to_abs_and_has_two_choices():
    from utils import constant
    assert constant.parse([]).pos_encoding == "abs"
    assert constant.parse(["--pos-encoding", "rope"]).pos_encoding == "rope"
    assert constant.parse(["--pos-encoding", "abs"]).pos_encoding == "abs"
    with pytest.raises(SystemExit):
        constant.parse(["--pos-encoding", "relative"])


def test_state_dict_keys_are_the_same_in_both_modes():
    _, plain = _model([])
    _, ab = _model(["--pos-encoding", "abs"])
    _, ro = _model(["--pos-encoding", "rope"])
    base = list(plain.state_dict().keys())
    assert list(ab.state_dict().keys()) == base and list(ro.state_dict().keys()) == base
    assert "encoder.positional_encoding.pe" in base and not any("rope" in k for k in base)
    assert not hasattr(ab.encoder, "rope_cs") and ab.encoder.pos_encoding == "abs" and ro.encoder.pos_encoding == "rope"
    assert ro.encoder.rope_cs.dtype == torch.float32 and tuple(ro.encoder.rope_cs.shape) == (64, 8, 2)
    assert torch.equal(ro.encoder.rope_cs, R.table64(64, 16).float())
    assert not hasattr(ro.decoder, "rope_cs")                          # encoder only


def test_rank_combination_raises_naming_both_flags():
    with pytest.raises(ValueError) as e:
        _model(["--pos-encoding", "rope", "--rank", "8"])
    assert "--pos-encoding" in str(e.value) and "--rank" in str(e.value)


def test_unequal_head_widths_raise_naming_the_flags():
    with pytest.raises(ValueError) as e:
        _model(["--pos-encoding", "rope"], base=_with(TINY, dim_value=32))
    assert "--pos-encoding" in str(e.value) and "--dim-key" in str(e.value) and "--dim-value" in str(e.value)


@pytest.mark.parametrize("width", [8, 24, 128])
def test_head_width_outside_the_kernels_raises_naming_the_flags(width):
    with pytest.raises(ValueError) as e:
        _model(["--pos-encoding", "rope"], base=_with(TINY, dim_key=width, dim_value=width))
    assert "--pos-encoding" in str(e.value) and "--dim-key" in str(e.value)


def test_encoder_and_attention_refuse_what_the_flag_cannot_mean():
    from models.asr.transformer import Encoder
    from models.common_layers import MultiHeadAttention
    with pytest.raises(ValueError):
        Encoder(1, 2, 32, 16, 16, 32, 64, pos_encoding="alibi")
    enc = Encoder(1, 2, 32, 16, 16, 32, 64, src_max_length=8, pos_encoding="rope")
    with pytest.raises(ValueError) as e:
        enc(torch.zeros(1, 9, 32), torch.tensor([9]))
    assert "--src-max-len" in str(e.value)
    mha = MultiHeadAttention(2, 32, 16, 16)
    q, kv = torch.zeros(1, 4, 32), torch.zeros(1, 5, 32)
    with pytest.raises(ValueError):
        mha(q, kv, kv, rope=R.table64(4, 16).float())                   # cross attention


def _save(tmp_path, extra):
    from utils.functions import init_optimizer, save_model
    args, model = _model(extra)
    args.save_folder, args.name = str(tmp_path), "ck"
    opt = init_optimizer(args, model, "noam")
    l2i, i2l = _labels()
    save_model(model, 1, opt, {"valid_loss": 1.0}, l2i, i2l, best_model=False)
    return model, os.path.join(str(tmp_path), "ck", "epoch_1.th")


def test_load_model_rebuilds_the_encoder_from_the_checkpoint(tmp_path):
    from utils import constant
    from utils.functions import load_model
    model, path = _save(tmp_path, ["--pos-encoding", "rope"])
    constant.parse(TINY)                                               # a new run that types no --pos-encoding
    m2, _, _, _, a2, _, _ = load_model(path)
    assert a2.pos_encoding == "rope" and constant.args.pos_encoding == "rope" and m2.encoder.pos_encoding == "rope"
    assert torch.equal(m2.encoder.rope_cs, model.encoder.rope_cs)
    assert list(m2.state_dict().keys()) == list(model.state_dict().keys())
    for (k, a), (_, b) in zip(model.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    constant.parse(TINY + ["--pos-encoding", "rope"])                  # typing the checkpoint's own value is fine
    assert load_model(path)[4].pos_encoding == "rope"


@pytest.mark.parametrize("saved,typed", [("rope", "abs"), ("abs", "rope")])
def test_typed_mismatch_against_the_checkpoint_raises(tmp_path, saved, typed):
    from utils import constant
    from utils.functions import load_model
    _, path = _save(tmp_path, ["--pos-encoding", saved])
    constant.parse(TINY + ["--pos-encoding", typed])
    with pytest.raises(ValueError) as e:
        load_model(path)
    assert "--pos-encoding %s" % typed in str(e.value) and "--pos-encoding %s" % saved in str(e.value)


def test_checkpoint_without_the_field_loads_as_abs(tmp_path):
    from utils import constant
    from utils.functions import load_model
    model, path = _save(tmp_path, [])
    ck = torch.load(path, map_location="cpu", weights_only=False)
    del ck["args"].pos_encoding                                        # as written before the flag existed
    torch.save(ck, path)
    constant.parse(TINY)
    m2, _, _, _, a2, _, _ = load_model(path)
    assert a2.pos_encoding == "abs" and m2.encoder.pos_encoding == "abs" and not hasattr(m2.encoder, "rope_cs")
    assert list(m2.state_dict().keys()) == list(model.state_dict().keys())
