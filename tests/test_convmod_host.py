"""The convolution module on the host: the float64 restatement the GPU tests measure against (tests/convmod_reference.py) held against
torch's own composition and autograd, and everything of --conv-module-kernel that needs no GPU -- the flag, the module's keys, the
refused combinations, the checkpoint round trip.  The first group checks the yardstick and passes without the feature; the second
group fails without it."""
import os

import numpy as np
import pytest
import torch

import convmod_reference as R

CASES = [((3, 5, 8, 31), [5, 3, 1]), ((2, 67, 16, 7), [67, 40]), ((1, 1, 8, 3), [1])]
GPU_SHAPES = [((1, 1, 8, 3), [1]), ((3, 5, 64, 31), [5, 3, 1]), ((2, 67, 192, 7), [67, 40]), ((4, 300, 512, 15), [300, 299, 150, 17])]


def _torch_all(u, wd, bd, dv, lens):
    ut = torch.from_numpy(u).requires_grad_(True)
    wt = torch.from_numpy(wd).reshape(wd.shape[0], 1, -1).requires_grad_(True)
    bt = torch.from_numpy(bd).requires_grad_(True)
    s, v = R.torch_core(ut, wt, bt, torch.from_numpy(lens))
    (v * torch.from_numpy(dv)).sum().backward()
    return s.detach().numpy(), v.detach().numpy(), ut.grad.numpy(), wt.grad.numpy().reshape(wd.shape), bt.grad.numpy()


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("shape,lens", CASES)
def test_restatement_equals_torch_composition_and_autograd(shape, lens):
    u, wd, bd, dv, lens = R.random_case(*shape, lens, seed=11)
    s, v, _ = R.forward(u, wd, bd, lens)
    du, dwd, dbd = R.backward(dv, s, u, wd, lens)
    s_t, v_t, du_t, dwd_t, dbd_t = _torch_all(u, wd, bd, dv, lens)
    assert np.abs(s - s_t).max() <= 1e-12 and np.abs(v - v_t).max() <= 1e-12
    assert np.abs(du - du_t).max() <= 1e-10 and np.abs(dwd - dwd_t).max() <= 1e-10 and np.abs(dbd - dbd_t).max() <= 1e-10


@pytest.mark.parametrize("shape,lens", CASES)
def test_padding_of_u_and_dv_changes_nothing(shape, lens):
    u, wd, bd, dv, lens = R.random_case(*shape, lens, seed=12)
    s, v, g = R.forward(u, wd, bd, lens)
    du, dwd, dbd = R.backward(dv, s, u, wd, lens)
    pad = np.arange(shape[1])[None, :, None] >= lens[:, None, None]
    u2, dv2 = np.where(pad, 1e30, u), np.where(pad, 1e30, dv)
    s2, v2, g2 = R.forward(u2, wd, bd, lens)
    du2, dwd2, dbd2 = R.backward(dv2, s2, u2, wd, lens)
    for a, b in ((s, s2), (v, v2), (g, g2), (du, du2), (dwd, dwd2), (dbd, dbd2)):
        assert np.array_equal(a, b)
    assert not (v2 * pad).any() and not (du2 * pad).any()


@pytest.mark.parametrize("shape,lens", GPU_SHAPES)
def test_saturated_case_is_integer_in_float32_and_float64(shape, lens):
    """gate = 40, bd = 96: s in [34, 158], sigma = 1 in float32, so v = s, ds = dv and every output is an order-free sum of small
    integers (below 2^24, v and du at most 256: exact in bf16 too).  In float64 sigma(34) = 1 - 1.7e-15, so the float64 restatement
    differs from those integers by rounding only and gives them back when rounded to float32."""
    u, wd, bd, dv, lens = R.exact_case(*shape, lens, seed=5, dtype=np.float32)
    s, v, _ = R.forward(u, wd, bd, lens)
    du, dwd, dbd = R.backward(dv, s, u, wd, lens)
    D = shape[2]
    keep = np.arange(shape[1])[None, :, None] < lens[:, None, None]
    assert s.min() >= 34 and s.max() <= 158 and np.array_equal(v, np.where(keep, s, 0))
    for x in (v, du, dwd, dbd):
        assert x.dtype == np.float32 and np.array_equal(x, np.rint(x)) and np.abs(x).max() < 2 ** 24
    assert np.abs(v).max() <= 256 and np.abs(du).max() <= 256 and not du[..., D:].any()
    u6, wd6, bd6, dv6 = (x.astype(np.float64) for x in (u, wd, bd, dv))
    s6, v6, _ = R.forward(u6, wd6, bd6, lens)
    du6, dwd6, dbd6 = R.backward(dv6, s6, u6, wd6, lens)
    for x, x6 in ((v, v6), (du, du6), (dwd, dwd6), (dbd, dbd6)):
        assert np.abs(x6 - x).max() <= 1e-9 and np.array_equal(x6.astype(np.float32), x)


def test_sigmoid_saturates_exactly_in_float32():
    x = np.array([32.0, 40.0, 1e30, -88.0 - 1.0, -1e30], dtype=np.float32)
    sg = R.sigmoid(x)
    assert sg.dtype == np.float32 and list(sg[:3]) == [1.0, 1.0, 1.0] and list(sg[3:]) == [0.0, 0.0]
    assert (np.float32(3.0) * sg[3:] == 0).all()


# ------------------------------------------------------------------------------------------------ the feature, without a GPU
TINY = ("--num-layers 2 --num-heads 2 --dim-model 32 --dim-key 16 --dim-value 16 --dim-inner 64 --dim-emb 32 --feat_extractor vgg_cnn "
        "--tgt-max-len 12 --src-max-len 64 --dropout 0.0").split()
MODULE_KEYS = ["pointwise_1.weight", "pointwise_1.bias", "depthwise.weight", "depthwise.bias", "pointwise_2.weight", "pointwise_2.bias",
               "layer_norm.weight", "layer_norm.bias"]


def _labels(V=32):
    from utils import constant
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + [chr(0x4E00 + i) for i in range(V - 3)]
    return {c: i for i, c in enumerate(chars)}, {i: c for i, c in enumerate(chars)}


def _model(extra):
    from utils import constant
    from utils.functions import init_transformer_model
    args = constant.parse(TINY + extra)
    return args, init_transformer_model(args, *_labels())


@pytest.fixture(autouse=True)
def _restore_args():
    from utils import constant
    keep = (constant.args, constant.explicit, constant.USE_CUDA)
    yield
    constant.args, constant.explicit, constant.USE_CUDA = keep


def test_flag_parses_and_defaults_to_off():
    from utils import constant
    assert constant.parse([]).conv_module_kernel == 0
    assert constant.parse(["--conv-module-kernel", "7"]).conv_module_kernel == 7


def test_module_keys_per_encoder_layer_and_none_when_off():
    _, plain = _model([])
    _, off = _model(["--conv-module-kernel", "0"])
    _, on = _model(["--conv-module-kernel", "7"])
    base = list(plain.state_dict().keys())
    assert list(off.state_dict().keys()) == base and not any("conv_module" in k for k in base)
    assert not any(hasattr(l, "conv_module") for l in off.encoder.layers)
    added = [k for k in on.state_dict().keys() if k not in base]
    assert added == ["encoder.layers.%d.conv_module.%s" % (i, k) for i in range(2) for k in MODULE_KEYS]
    assert [k for k in on.state_dict().keys() if "conv_module" not in k] == base
    sd = on.state_dict()
    assert tuple(sd["encoder.layers.0.conv_module.pointwise_1.weight"].shape) == (64, 32)
    assert tuple(sd["encoder.layers.0.conv_module.depthwise.weight"].shape) == (32, 1, 7)
    assert tuple(sd["encoder.layers.1.conv_module.pointwise_2.weight"].shape) == (32, 32)
    assert not any("conv_module" in k for k in sd if k.startswith("decoder."))


def test_initialisation_matrices_as_the_model_depthwise_as_conv1d():
    _, on = _model(["--conv-module-kernel", "7"])
    cm = on.encoder.layers[0].conv_module
    # every matrix of the model is xavier_uniform_: |w| <= sqrt(6 / (fan_in + fan_out))
    assert cm.pointwise_1.weight.abs().max().item() <= (6.0 / (32 + 64)) ** 0.5 + 1e-6
    assert cm.pointwise_1.weight.abs().max().item() > 0.9 * (6.0 / (32 + 64)) ** 0.5
    # Conv1d's default: kaiming_uniform_(a = sqrt 5) = U(-1/sqrt(fan_in), 1/sqrt(fan_in)), fan_in = K (xavier on (D,1,K) would reach 0.15)
    bound = 1.0 / 7 ** 0.5
    w = cm.depthwise.weight.abs().max().item()
    assert 0.8 * bound < w <= bound + 1e-6


def test_rank_combination_raises_naming_both_flags():
    with pytest.raises(ValueError) as e:
        _model(["--conv-module-kernel", "7", "--rank", "8"])
    assert "--conv-module-kernel" in str(e.value) and "--rank" in str(e.value)


@pytest.mark.parametrize("extra", [["--conv-module-kernel", "4"], ["--conv-module-kernel", "1"], ["--conv-module-kernel", "33"],
                                   ["--conv-module-kernel", "-3"], ["--conv-module-kernel", "7", "--dim-model", "36", "--dim-emb", "36"]])
def test_bad_kernel_sizes_and_widths_raise(extra):
    with pytest.raises(ValueError) as e:
        _model(extra)
    assert "--conv-module-kernel" in str(e.value)


def _save(tmp_path, extra):
    from utils import constant
    from utils.functions import init_optimizer, save_model
    args, model = _model(extra)
    args.save_folder, args.name = str(tmp_path), "ck"
    opt = init_optimizer(args, model, "noam")
    l2i, i2l = _labels()
    save_model(model, 1, opt, {"valid_loss": 1.0}, l2i, i2l, best_model=False)
    return model, os.path.join(str(tmp_path), "ck", "epoch_1.th")


def test_load_model_rebuilds_the_module_from_the_checkpoint(tmp_path):
    from utils import constant
    from utils.functions import load_model
    model, path = _save(tmp_path, ["--conv-module-kernel", "7"])
    constant.parse(TINY)                                      # a new run that types no --conv-module-kernel
    m2, _, _, _, a2, _, _ = load_model(path)
    assert a2.conv_module_kernel == 7 and constant.args.conv_module_kernel == 7
    assert list(m2.state_dict().keys()) == list(model.state_dict().keys())
    for (k, a), (_, b) in zip(model.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    constant.parse(TINY + ["--conv-module-kernel", "7"])      # typing the checkpoint's own value is fine
    assert load_model(path)[4].conv_module_kernel == 7


@pytest.mark.parametrize("saved,typed", [("7", "9"), ("7", "0"), ("0", "7")])
def test_typed_mismatch_against_the_checkpoint_raises(tmp_path, saved, typed):
    from utils import constant
    from utils.functions import load_model
    _, path = _save(tmp_path, ["--conv-module-kernel", saved])
    constant.parse(TINY + ["--conv-module-kernel", typed])
    with pytest.raises(ValueError) as e:
        load_model(path)
    assert "--conv-module-kernel %s" % typed in str(e.value) and "--conv-module-kernel %s" % saved in str(e.value)


def test_checkpoint_without_the_field_loads_without_a_module(tmp_path):
    from utils import constant
    from utils.functions import load_model
    model, path = _save(tmp_path, [])
    ck = torch.load(path, map_location="cpu", weights_only=False)
    del ck["args"].conv_module_kernel                          # as written before the flag existed
    torch.save(ck, path)
    constant.parse(TINY)
    m2, _, _, _, a2, _, _ = load_model(path)
    assert a2.conv_module_kernel == 0 and list(m2.state_dict().keys()) == list(model.state_dict().keys())
