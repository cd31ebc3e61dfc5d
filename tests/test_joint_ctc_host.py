"""Joint CTC / attention training and decoding, the parts that need no GPU: the encoder CTC head exists exactly when --ctc-weight > 0
(state_dict keys, checkpoints), the flag errors, and the best-path collapse rule."""
import pytest
import torch

FLAGS = ("--num-layers 1 --num-heads 2 --dim-model 32 --dim-key 16 --dim-value 16 --dim-inner 64 --dim-emb 32 --tgt-max-len 12 "
         "--src-max-len 64").split()

_ATTN = ["query_linear.weight", "query_linear.bias", "key_linear.weight", "key_linear.bias", "value_linear.weight", "value_linear.bias",
         "layer_norm.weight", "layer_norm.bias", "output_linear.weight", "output_linear.bias"]
_FFN = ["conv_1.weight", "conv_1.bias", "conv_2.weight", "conv_2.bias", "layer_norm.weight", "layer_norm.bias"]
# the state_dict of the model these flags build, written out (one encoder layer, one decoder layer, the vgg_cnn front end)
KEYS_TODAY = (["encoder.input_linear.weight", "encoder.input_linear.bias", "encoder.layer_norm_input.weight",
               "encoder.layer_norm_input.bias", "encoder.positional_encoding.pe"] +
              ["encoder.layers.0.self_attn." + k for k in _ATTN] + ["encoder.layers.0.pos_ffn." + k for k in _FFN] +
              ["decoder.trg_embedding.weight", "decoder.positional_encoding.pe"] +
              ["decoder.layers.0.self_attn." + k for k in _ATTN] + ["decoder.layers.0.encoder_attn." + k for k in _ATTN] +
              ["decoder.layers.0.pos_ffn." + k for k in _FFN] + ["decoder.output_linear.weight"] +
              ["conv.%d.%s" % (i, k) for i in (0, 2, 5, 7) for k in ("weight", "bias")])


@pytest.fixture
def cli():
    """constant.parse with the process-global Namespace put back afterwards."""
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


def _labels():
    from utils import constant
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR, "a", "b", " "]
    l2i = {c: i for i, c in enumerate(chars)}
    return l2i, {i: c for c, i in l2i.items()}


def _model(cli, extra=()):
    from utils.functions import init_transformer_model
    l2i, i2l = _labels()
    return init_transformer_model(cli(FLAGS + list(extra)), l2i, i2l)


def test_default_model_has_exactly_todays_keys(cli):
    assert len(KEYS_TODAY) == 58
    model = _model(cli)
    assert list(model.state_dict().keys()) == KEYS_TODAY and not hasattr(model, "ctc_linear")
    assert list(_model(cli, ["--ctc-weight", "0"]).state_dict().keys()) == KEYS_TODAY


def test_ctc_weight_adds_exactly_the_head(cli):
    model = _model(cli, ["--ctc-weight", "0.3"])
    sd = model.state_dict()
    assert set(sd) - set(KEYS_TODAY) == {"ctc_linear.weight", "ctc_linear.bias"} and set(KEYS_TODAY) <= set(sd)
    V = len(_labels()[0])
    assert tuple(sd["ctc_linear.weight"].shape) == (V, 32) and tuple(sd["ctc_linear.bias"].shape) == (V,)
    # Xavier-uniform like every other matrix of the model: |w| <= sqrt(6 / (fan_in + fan_out)), and not nn.Linear's default bound
    bound = (6.0 / (32 + V)) ** 0.5
    w = sd["ctc_linear.weight"]
    assert w.abs().max().item() <= bound and w.abs().max().item() > 32 ** -0.5


def _save(cli, tmp_path, extra):
    from utils import constant
    from utils.functions import init_optimizer, save_model
    model = _model(cli, ["--save-folder", str(tmp_path), "--name", "ck"] + list(extra))
    opt = init_optimizer(constant.args, model, "noam")
    l2i, i2l = _labels()
    save_model(model, 1, opt, {"valid_loss": 1.0}, l2i, i2l)
    return model, str(tmp_path / "ck" / "epoch_1.th")


def test_checkpoint_round_trip_and_the_weight_rules(cli, tmp_path):
    from utils import constant
    from utils.functions import load_model
    model, path = _save(cli, tmp_path, ["--ctc-weight", "0.3"])
    # test.py needs no flag: the head comes back from the checkpoint's own weight
    cli(["--continue-from", path])
    loaded, _, _, _, largs, _, _ = load_model(path)
    assert largs.ctc_weight == 0.3 and constant.args.ctc_weight == 0.3
    for k, v in model.state_dict().items():
        assert torch.equal(v, loaded.state_dict()[k]), k
    assert "ctc_linear.weight" in loaded.state_dict()
    # positive -> another positive weight: accepted, it only weighs the loss
    cli(["--continue-from", path, "--ctc-weight", "0.5"])
    loaded, _, _, _, largs, _, _ = load_model(path)
    assert largs.ctc_weight == 0.5 and constant.args.ctc_weight == 0.5 and hasattr(loaded, "ctc_linear")
    # positive -> 0 drops the head: an error that names both values
    cli(["--continue-from", path, "--ctc-weight", "0"])
    with pytest.raises(ValueError, match=r"--ctc-weight 0 .*--ctc-weight 0\.3"):
        load_model(path)


def test_checkpoint_without_a_head_loads_unchanged_and_cannot_gain_one(cli, tmp_path):
    from utils.functions import load_model
    model, path = _save(cli, tmp_path, [])
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert list(ck["model_state_dict"].keys()) == KEYS_TODAY
    del ck["args"].ctc_weight                      # a checkpoint written before the flag existed
    torch.save(ck, path)
    cli(["--continue-from", path])
    loaded, _, _, _, largs, _, _ = load_model(path)
    assert list(loaded.state_dict().keys()) == KEYS_TODAY and largs.ctc_weight == 0.0
    cli(["--continue-from", path, "--ctc-weight", "0.3"])
    with pytest.raises(ValueError, match=r"--ctc-weight 0\.3 .*--ctc-weight 0"):
        load_model(path)


def test_training_flag_errors(cli):
    from utils.functions import check_ctc_weight
    with pytest.raises(ValueError, match="--parallel"):
        _model(cli, ["--ctc-weight", "0.3", "--parallel"])
    with pytest.raises(ValueError, match="--loss ctc"):
        _model(cli, ["--ctc-weight", "0.3", "--loss", "ctc"])
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        _model(cli, ["--ctc-weight", "1.5"])
    # train.py refuses them at start-up, before anything is built
    import train
    for bad in (["--parallel"], ["--loss", "ctc"]):
        cli(FLAGS + ["--ctc-weight", "0.3"] + bad)
        with pytest.raises(ValueError):
            train.main()
    assert check_ctc_weight(0.0, cli(FLAGS + ["--parallel", "--loss", "ctc"])) == 0.0      # weight 0: nothing to refuse
    # the hybrid step is eager: the default graph bucket is not turned on for it
    a = cli(FLAGS + ["--cuda", "--ctc-weight", "0.3"])
    assert train.resolve_graph_buckets(a, set()) == 0
    a = cli(FLAGS + ["--cuda"])
    assert train.resolve_graph_buckets(a, set()) == train.DEFAULT_GRAPH_BUCKET


def test_decoding_flag_errors(cli):
    import test as test_mod
    plain, head = _model(cli), _model(cli, ["--ctc-weight", "0.3"])
    with pytest.raises(ValueError, match="CTC head"):
        test_mod.check_ctc_decoding(cli(["--beam-search", "--ctc-decode-weight", "0.3"]), plain)
    with pytest.raises(ValueError, match="CTC head"):
        test_mod.check_ctc_decoding(cli(["--ctc-greedy"]), plain)
    with pytest.raises(ValueError, match="--beam-search"):
        test_mod.check_ctc_decoding(cli(["--ctc-decode-weight", "0.3"]), head)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        test_mod.check_ctc_decoding(cli(["--beam-search", "--ctc-decode-weight", "2"]), head)
    test_mod.check_ctc_decoding(cli(["--beam-search", "--ctc-decode-weight", "0.3", "--ctc-candidates", "6"]), head)
    test_mod.check_ctc_decoding(cli([]), plain)
    # the model's own entry points refuse the same misuse before any device work
    x = torch.zeros(1, 1, 161, 8)
    with pytest.raises(ValueError, match="--beam-search"):
        head.evaluate(x, [8], torch.zeros(1, 2, dtype=torch.int64), ctc_weight=0.3)
    with pytest.raises(ValueError, match="CTC head"):
        plain.ctc_logits(torch.zeros(1, 2, 32))
    with pytest.raises(ValueError, match="ctc_logits"):
        head.decoder.beam_search(torch.zeros(1, 2, 32), beam_width=2, ctc_weight=0.3)
    with pytest.raises(NotImplementedError):
        head.decoder.beam_search(torch.zeros(1, 2, 32), beam_width=2, ctc_weight=0.3, ctc_logits=torch.zeros(1, 2, 6), use_cache=False)
    with pytest.raises(NotImplementedError):
        head.decoder.beam_search(torch.zeros(2, 2, 32), beam_width=2, ctc_weight=0.3, ctc_logits=torch.zeros(2, 2, 6),
                                 use_cache="per_utterance")
    lowrank = _model(cli, ["--ctc-weight", "0.3", "--rank", "8"])
    with pytest.raises(NotImplementedError):
        lowrank.decoder.beam_search(torch.zeros(1, 2, 32), beam_width=2, ctc_weight=0.3, ctc_logits=torch.zeros(1, 2, 6))


def test_best_path_collapse_rule():
    from models.asr.transformer import ctc_collapse, frames_after_cnn
    #        a  a  _  a  b  b  _  _  c  (beyond the utterance's frames:) c  d
    ids = [3, 3, 0, 3, 4, 4, 0, 0, 5, 5, 6]
    assert ctc_collapse(ids, 9) == [3, 3, 4, 5]           # repeats merge, a blank between two equal labels keeps both
    assert ctc_collapse(ids) == [3, 3, 4, 5, 6]
    assert ctc_collapse(ids, 2) == [3] and ctc_collapse(ids, 0) == [] and ctc_collapse([0, 0, 0]) == []
    assert frames_after_cnn(43, "vgg_cnn") == 10 and frames_after_cnn(43, "emb_cnn") == 17 and frames_after_cnn(43, "") == 43
