"""The transducer head, the parts that need no GPU: the float64 restatement (tests/rnnt_reference.py) against
brute-force enumeration, float64 autograd and a closed form; the edge rules of the definition; the flag and entry-point refusals; the
state_dict keys with the flag off and on; the checkpoint round trip of the settings."""
import math

import pytest
import torch

import rnnt_reference as R
from test_joint_ctc_host import FLAGS, KEYS_TODAY, _labels


@pytest.fixture
def cli():
    """constant.parse with the process-global Namespace put back afterwards."""
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


def _model(cli, extra=()):
    from utils.functions import init_transformer_model
    l2i, i2l = _labels()
    return init_transformer_model(cli(FLAGS + list(extra)), l2i, i2l)


# ------------------------------------------------------------------------------------------------ the restatement
def _one(T, U, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, T, U + 1, V), generator=g, dtype=torch.float64) * 1.5
    y = torch.randint(1, V, (1, max(U, 1)), generator=g)
    return x, y


def test_loss_equals_the_sum_over_every_alignment():
    """All T <= 4, U <= 3 at V = 4: C(T - 1 + U, U) alignments each, enumerated."""
    n = 0
    for T in range(1, 5):
        for U in range(0, 4):
            x, y = _one(T, U, 4, 10 * T + U)
            got = R.loss_and_grad(x, y, [T], [U])
            want = R.nll_brute_force(x[0], y[0].tolist()[:U])
            assert abs(float(got["nll"][0]) - want) <= 1e-12 * max(1.0, abs(want)), (T, U, float(got["nll"][0]), want)
            # alpha and beta tell the same story: beta(0,0) is log Z too, and every diagonal's alpha + beta sums to it
            alpha, beta, logz = got["lattice"][0]
            assert abs(float(beta[0, 0]) - float(logz)) <= 1e-12 * max(1.0, abs(float(logz)))
            n += 1
    assert n == 16


@pytest.mark.parametrize("T,U,V", [(1, 0, 3), (1, 3, 4), (4, 0, 4), (4, 3, 4), (5, 4, 7)])
def test_gradient_formula_equals_float64_autograd_through_a_logaddexp_lattice(T, U, V):
    x, y = _one(T, U, V, 100 + T + U)
    got = R.loss_and_grad(x, y, [T], [U], grad_out=0.7)
    xa = x[0].clone().requires_grad_()
    nll = R.nll_autograd(xa, y[0].tolist()[:U])
    (0.7 * nll / max(U, 1)).backward()
    assert abs(float(nll) - float(got["nll"][0])) <= 1e-12 * max(1.0, abs(float(nll)))
    assert float((xa.grad - got["dlogits"][0]).abs().max()) <= 1e-13
    assert float(got["dlogits"].abs().max()) > 1e-3
    assert float(got["dlogits"].sum(-1).abs().max()) <= 1e-13          # every row of a log-softmax gradient sums to zero


def test_uniform_logits_closed_form():
    """Uniform logits: every alignment has probability V^-(T+U) and there are C(T - 1 + U, U) of them."""
    for T, U, V in [(1, 0, 2), (3, 2, 5), (6, 4, 9), (7, 5, 257)]:
        x = torch.full((1, T, U + 1, V), 0.25, dtype=torch.float64)
        y = torch.arange(1, max(U, 1) + 1).view(1, -1) % (V - 1) + 1
        got = float(R.loss_and_grad(x, y, [T], [U])["nll"][0])
        want = (T + U) * math.log(V) - math.log(math.comb(T - 1 + U, U))
        assert abs(got - want) <= 1e-12 * want, (T, U, V, got, want)


def test_edge_rules():
    c = R.case(5)
    ref = R.loss_and_grad(c["logits"], c["targets"], c["frames"], c["lengths"], V=5)
    dl = ref["dlogits"]
    assert torch.isfinite(ref["nll"]).all() and torch.isfinite(dl).all()      # NaN in every dead cell: none was read
    # U_b = 0 is legal: the loss is the blank path
    x1 = c["logits"][1, 0, 0, :5].double()
    assert abs(float(ref["nll"][1]) + float(torch.log_softmax(x1, -1)[0])) <= 1e-14
    # dead cells carry no gradient; live utterances do
    for b, (Tb, Ub) in enumerate(zip(c["frames"].tolist(), c["lengths"].tolist())):
        assert float(dl[b, Tb:].abs().max() if Tb < 7 else 0.0) == 0.0 and float(dl[b, :, Ub + 1:].abs().max() if Ub < 5 else 0.0) == 0.0
        assert float(dl[b, :Tb, :Ub + 1].abs().max()) > 0
    # the batch reduction is the CTC term's: mean over utterances of nll / max(U_b, 1)
    want = sum(float(n) / max(1, u) for n, u in zip(ref["nll"], c["lengths"].tolist())) / 3
    assert abs(float(ref["loss"]) - want) <= 1e-14 * want
    # T_b = 0, a blank label, a label outside [0,V): +inf, zero rows, the neighbours untouched
    for what in ("frames", "blank", "low", "high"):
        frames, tg = c["frames"].clone(), c["targets"].clone()
        if what == "frames":
            frames[2] = 0
        else:
            tg[2, 1] = {"blank": 0, "low": -1, "high": 5}[what]
        bad = R.loss_and_grad(c["logits"], tg, frames, c["lengths"], V=5)
        assert math.isinf(float(bad["nll"][2])) and float(bad["nll"][2]) > 0 and math.isinf(float(bad["loss"])), what
        assert float(bad["dlogits"][2].abs().max()) == 0.0
        assert torch.equal(bad["nll"][:2], ref["nll"][:2]) and torch.equal(bad["dlogits"][:2], dl[:2])
    # lengths beyond the tensor are clamped, negative ones count as 0
    clamped = R.loss_and_grad(c["logits"][:1], c["targets"][:1], [99], [99], V=5)
    assert torch.equal(clamped["nll"], R.loss_and_grad(c["logits"][:1], c["targets"][:1], [7], [5], V=5)["nll"])


def test_joint_and_its_two_reductions_against_autograd():
    g = torch.Generator().manual_seed(5)
    e = torch.randn((2, 5, 8), generator=g, dtype=torch.float64, requires_grad=True)
    p = torch.randn((2, 3, 8), generator=g, dtype=torch.float64, requires_grad=True)
    dz = torch.randn((2, 5, 3, 8), generator=g, dtype=torch.float64)
    z = R.joint(e, p)
    z.backward(dz)
    de, dp = R.joint_bwd(dz, z.detach())
    assert float((de - e.grad).abs().max()) <= 1e-14 and float((dp - p.grad).abs().max()) <= 1e-14


def test_greedy_restatement_on_a_table_by_hand():
    """J = 2: z = tanh of (frame signal, history signal) saturates to +-1, so the logits are a table known by hand.  Frame 0 wants label
    2 until it has just been emitted, frame 1 wants label 3 whatever came before (the max_symbols cut), frame 2 wants blank."""
    big = 20.0
    e = torch.tensor([[[big, 0.0], [-big, 0.0], [0.0, 0.0], [big, 0.0]]])            # frames 0..3; the fourth is beyond the length
    tables = [torch.tensor([[0.0, 0.0], [0.0, -big], [0.0, big], [0.0, -big]])]      # history signal: +1 after label 2, else -1 (SOS: -1)
    #                  z0 (frame)  z1 (history)
    w = torch.tensor([[0.0, 0.0], [0.0, 0.0], [3.0, -3.0], [-4.0, 0.0]])           # blank, SOS, label 2, label 3
    b = torch.tensor([1.0, -9.0, -3.0, 0.0])
    # frame 0 (z0 = 1): hist -1 -> label 2: 3 + 3 - 3 = 3 > blank 1 ; hist +1 -> label 2: 3 - 3 - 3 = -3, label 3: -4, blank 1 wins
    # frame 1 (z0 = -1): label 3 = 4 whatever the history -> emitted until the cut ; frame 2 (z0 = 0): label 2 <= 0 < blank 1
    ids, dec = R.greedy(e, tables, w, b, [3], 2)
    assert ids == [[2, 3, 3]]
    assert [(t, k) for t, k, _ in dec[0]] == [(0, 2), (0, 0), (1, 3), (1, 3), (2, 0)] and min(m for _, _, m in dec[0]) >= 1.0
    assert R.greedy(e, tables, w, b, [3], 4)[0] == [[2, 3, 3, 3, 3]] and R.greedy(e, tables, w, b, [4], 1)[0] == [[2, 3, 2]]
    assert R.greedy(e, tables, w, b, [0], 2)[0] == [[]]
    assert R.decided_prefix(ids[0], dec[0], 0.5) == ([2, 3, 3], True) and R.decided_prefix(ids[0], dec[0], 2.5)[1] is False


# ------------------------------------------------------------------------------------------------ the model and the flags
NEW_KEYS = {"rnnt_enc.weight", "rnnt_enc.bias", "rnnt_embed.0.weight", "rnnt_embed.1.weight", "rnnt_out.weight", "rnnt_out.bias"}


def test_with_the_flag_off_the_keys_are_todays(cli):
    model = _model(cli)
    assert list(model.state_dict().keys()) == KEYS_TODAY and not hasattr(model, "rnnt_out")
    assert list(_model(cli, ["--transducer-weight", "0", "--transducer-dim-joint", "12", "--rank", "0"]).state_dict().keys()) == KEYS_TODAY
    from utils import constant
    assert constant.parser.get_default("transducer_weight") == 0.0 and constant.parser.get_default("transducer_dim_joint") == 256
    assert constant.parser.get_default("transducer_context") == 2 and constant.parser.get_default("transducer_max_symbols") == 5


def test_the_weight_adds_exactly_the_head(cli):
    V = len(_labels()[0])
    sd = _model(cli, ["--transducer-weight", "0.3", "--transducer-dim-joint", "16"]).state_dict()
    assert set(sd) - set(KEYS_TODAY) == NEW_KEYS and set(KEYS_TODAY) <= set(sd)
    assert tuple(sd["rnnt_enc.weight"].shape) == (16, 32) and tuple(sd["rnnt_embed.1.weight"].shape) == (V, 16)
    assert tuple(sd["rnnt_out.weight"].shape) == (V, 16) and tuple(sd["rnnt_out.bias"].shape) == (V,)
    sd = _model(cli, ["--transducer-weight", "1", "--transducer-context", "1", "--ctc-weight", "0.3"]).state_dict()
    assert set(sd) - set(KEYS_TODAY) == (NEW_KEYS - {"rnnt_embed.1.weight"}) | {"ctc_linear.weight", "ctc_linear.bias"}
    assert tuple(sd["rnnt_enc.weight"].shape) == (256, 32)


def test_training_flag_refusals(cli):
    import train
    on = ["--transducer-weight", "0.3"]
    for bad, match in ((["--parallel"], "--parallel"), (["--loss", "ctc"], "--loss ctc"),
                       (["--ctc-weight", "0.3", "--mwer-weight", "0.5"], "--mwer-weight"),
                       (["--distill-from", "teacher.th", "--distill-weight", "0.5"], "--distill-from"), (["--rank", "8"], "--rank"),
                       (["--transducer-dim-joint", "12"], "multiple of 8"), (["--transducer-dim-joint", "0"], "multiple of 8"),
                       (["--transducer-context", "3"], "1 or 2"), (["--transducer-context", "0"], "1 or 2")):
        with pytest.raises(ValueError, match=match):
            _model(cli, on + bad)
        cli(FLAGS + on + bad)
        with pytest.raises(ValueError, match=match):           # train.py refuses them at start-up, before anything is built
            train.main()
    for w in ("1.5", "-0.1"):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            _model(cli, ["--transducer-weight", w])
    from models.asr.transformer import check_transducer
    with pytest.raises(ValueError, match="--dim-model"):
        check_transducer(256, 2, 36)
    assert check_transducer(256, 2, 512) == (256, 2) and check_transducer("8", "1") == (8, 1)
    # the step is eager: the default graph bucket is not turned on for it
    assert train.resolve_graph_buckets(cli(FLAGS + ["--cuda"] + on), set()) == 0
    assert train.resolve_graph_buckets(cli(FLAGS + ["--cuda"]), set()) == train.DEFAULT_GRAPH_BUCKET


def test_the_trainer_refuses_before_any_launch(cli):
    from trainer.asr.trainer import Trainer
    model = _model(cli, ["--transducer-weight", "0.3"])
    data = (torch.zeros(1, 1, 161, 8), torch.zeros(1, 2, dtype=torch.int64), torch.ones(1), torch.tensor([8]), torch.tensor([2]))
    with pytest.raises(ValueError, match="--loss ctc"):
        Trainer()._run_batch(model, data, 0.0, "ctc", model.id2label, None)


def test_decoding_refusals(cli):
    import test as test_mod
    plain, head = _model(cli), _model(cli, ["--transducer-weight", "0.3", "--ctc-weight", "0.3"])
    with pytest.raises(ValueError, match="transducer head"):
        test_mod.check_transducer_decoding(cli(["--transducer-greedy"]), plain)
    for other in (["--beam-search"], ["--ctc-greedy"], ["--ctc-beam-search"], ["--beam-search", "--ctc-decode-weight", "0.3"],
                  ["--ctc-beam-search", "--attention-rescoring-weight", "0.5"], ["--ngram-path", "x"], ["--context-path", "x"],
                  ["--align-out", "x"]):
        with pytest.raises(ValueError, match="cannot be combined with " + other[0]):
            test_mod.check_transducer_decoding(cli(["--transducer-greedy"] + other), head)
    with pytest.raises(ValueError, match="at least 1"):
        test_mod.check_transducer_decoding(cli(["--transducer-greedy", "--transducer-max-symbols", "0"]), head)
    test_mod.check_transducer_decoding(cli(["--transducer-greedy"]), head)
    test_mod.check_transducer_decoding(cli(["--beam-search"]), plain)                  # without the flag nothing is checked
    assert test_mod.transducer_decoding(cli([])) == {}
    assert test_mod.transducer_decoding(cli(["--transducer-greedy", "--transducer-max-symbols", "3"])) == dict(transducer_greedy=True,
                                                                                                             transducer_max_symbols=3)
    # the model's own entry points refuse the same misuse before any device work
    x, y = torch.zeros(1, 1, 161, 8), torch.zeros(1, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="transducer head"):
        plain.evaluate(x, [8], y, transducer_greedy=True)
    for other in (dict(beam_search=True), dict(ctc_greedy=True), dict(ctc_beam=True), dict(align_source="gold")):
        with pytest.raises(ValueError, match="transducer head alone"):
            head.evaluate(x, [8], y, transducer_greedy=True, **other)
    with pytest.raises(ValueError, match="at least 1"):
        head.evaluate(x, [8], y, transducer_greedy=True, transducer_max_symbols=0)
    for call in (lambda: plain.transducer_logits(torch.zeros(1, 2, 32), y, [2]), lambda: plain.transducer_greedy(torch.zeros(1, 2, 32), [2]),
                 lambda: plain.transducer_step(x, [8], y, [2], 0.3, 0.0)):
        with pytest.raises(ValueError, match="transducer head"):
            call()
    with pytest.raises(ValueError, match=r"\(0, 1\]"):
        head.transducer_step(x, [8], y, [2], 0.0, 0.0)
    with pytest.raises(ValueError, match="at least 1"):
        head.transducer_greedy(torch.zeros(1, 2, 32), [2], max_symbols=0)


def test_a_shape_with_2_to_the_31_logit_bytes_is_refused_before_the_first_launch(cli):
    from asr_hip import functions as F_
    F_.check_rnnt_shape(32, 75, 41, 4364)                       # the workload's largest: 1.74e9 bytes
    with pytest.raises(ValueError, match="2\\^31"):
        F_.check_rnnt_shape(32, 75, 51, 4364)
    with pytest.raises(ValueError, match="2\\^31"):
        F_.check_rnnt_shape(64, 75, 41, 4364)
    head = _model(cli, ["--transducer-weight", "0.3"])
    with pytest.raises(ValueError, match="2\\^31"):              # before any launch: the tensors are on the host, nothing could run
        head.transducer_logits(torch.zeros(1).expand(4000, 3000, 32), torch.ones(4000, 40, dtype=torch.int64), [40] * 4000)
    with pytest.raises(ValueError, match="2\\^31"):
        F_.RnntFn.apply(torch.zeros(1).expand(1 << 12, 1 << 10, 1 << 5, 1 << 4), torch.ones(1 << 12, 31, dtype=torch.int64),
                        [1 << 10] * (1 << 12), [31] * (1 << 12), 0)


def _save(cli, tmp_path, extra):
    from utils import constant
    from utils.functions import init_optimizer, save_model
    model = _model(cli, ["--save-folder", str(tmp_path), "--name", "ck"] + list(extra))
    opt = init_optimizer(constant.args, model, "noam")
    l2i, i2l = _labels()
    save_model(model, 1, opt, {"valid_loss": 1.0}, l2i, i2l)
    return model, str(tmp_path / "ck" / "epoch_1.th")


def test_checkpoint_round_trip_of_the_settings(cli, tmp_path):
    from utils import constant
    from utils.functions import load_model
    model, path = _save(cli, tmp_path, ["--transducer-weight", "0.3", "--transducer-dim-joint", "16", "--transducer-context", "1"])
    # test.py and --continue-from need no flag: the head comes back from the checkpoint's own settings
    cli(["--continue-from", path])
    loaded, _, _, _, largs, _, _ = load_model(path)
    assert (largs.transducer_weight, largs.transducer_dim_joint, largs.transducer_context) == (0.3, 16, 1)
    assert (constant.args.transducer_weight, constant.args.transducer_dim_joint, constant.args.transducer_context) == (0.3, 16, 1)
    assert set(loaded.state_dict()) == set(model.state_dict()) and "rnnt_embed.0.weight" in loaded.state_dict()
    for k, v in model.state_dict().items():
        assert torch.equal(v, loaded.state_dict()[k]), k
    # positive -> another positive weight: accepted, it only weighs the loss
    cli(["--continue-from", path, "--transducer-weight", "0.5"])
    loaded, _, _, _, largs, _, _ = load_model(path)
    assert largs.transducer_weight == 0.5 and constant.args.transducer_weight == 0.5 and hasattr(loaded, "rnnt_out")
    # the head cannot be dropped, nor resized
    cli(["--continue-from", path, "--transducer-weight", "0"])
    with pytest.raises(ValueError, match=r"--transducer-weight 0 .*--transducer-weight 0\.3"):
        load_model(path)
    cli(["--continue-from", path, "--transducer-dim-joint", "32"])
    with pytest.raises(ValueError, match=r"--transducer-dim-joint 32 .*--transducer-dim-joint 16"):
        load_model(path)
    cli(["--continue-from", path, "--transducer-context", "2"])
    with pytest.raises(ValueError, match=r"--transducer-context 2 .*--transducer-context 1"):
        load_model(path)


def test_checkpoint_without_a_head_loads_unchanged_and_cannot_gain_one(cli, tmp_path):
    from utils.functions import load_model
    model, path = _save(cli, tmp_path, [])
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert list(ck["model_state_dict"].keys()) == KEYS_TODAY
    for k in ("transducer_weight", "transducer_dim_joint", "transducer_context"):      # a checkpoint written before the flags existed
        delattr(ck["args"], k)
    torch.save(ck, path)
    cli(["--continue-from", path])
    loaded, _, _, _, largs, _, _ = load_model(path)
    assert list(loaded.state_dict().keys()) == KEYS_TODAY and largs.transducer_weight == 0.0
    cli(["--continue-from", path, "--transducer-weight", "0.3"])
    with pytest.raises(ValueError, match=r"--transducer-weight 0\.3 .*--transducer-weight 0"):
        load_model(path)
