"""Pruned transducer training on the host (no GPU): the float64 restatement (tests/rnnt_pruned_reference.py) against independent
statements of the same quantities -- the full loss on the materialised am + lm, float64 autograd, brute-force enumeration of every
alignment inside a band -- the band rule's properties, ties and edge cases, and every new refusal of the flags and of load_model."""
import itertools
import math

import pytest
import torch

import rnnt_pruned_reference as P
import rnnt_reference as R


def _dense(c):
    V = c["V"]
    return torch.nan_to_num(c["am"][..., :V].double(), nan=0.0), torch.nan_to_num(c["lm"][..., :V].double(), nan=0.0)


# ------------------------------------------------------------------------------------------------ the simple loss
@pytest.mark.parametrize("V", [2, 5, 65])
def test_simple_loss_is_the_full_loss_on_the_materialised_joiner(V):
    c = P.simple_case(V)
    am, lm = _dense(c)
    got = P.simple_loss_and_grad(c["am"], c["lm"], c["targets"], c["frames"], c["lengths"], V=V)
    want = R.loss_and_grad(P.materialised(am, lm), c["targets"], c["frames"], c["lengths"], V=V)
    assert torch.allclose(got["nll"], want["nll"], rtol=0, atol=1e-11) and torch.allclose(got["loss"], want["loss"], rtol=0, atol=1e-11)
    # d / d am = the sum over u of the joint gradient, d / d lm the sum over t
    assert torch.allclose(got["dam"], want["dlogits"].sum(2), rtol=0, atol=1e-12)
    assert torch.allclose(got["dlm"], want["dlogits"].sum(1), rtol=0, atol=1e-12)
    assert float(got["dam"].abs().max()) > 1e-3


def test_simple_gradient_is_float64_autograd():
    V = 7
    c = P.simple_case(V, labels={0: [3, 3, 3, 5, 3]})
    am, lm = _dense(c)
    am.requires_grad_(True)
    lm.requires_grad_(True)
    total = 0.0
    for b, (Tb, Ub) in enumerate(zip(c["frames"].tolist(), c["lengths"].tolist())):
        x = am[b, :Tb, None, :] + lm[b, None, :Ub + 1, :]
        total = total + R.nll_autograd(x, c["targets"][b, :Ub].tolist()) / max(Ub, 1)
    (total / 3 * 0.7).backward()
    got = P.simple_loss_and_grad(c["am"], c["lm"], c["targets"], c["frames"], c["lengths"], V=V, grad_out=0.7)
    assert torch.allclose(got["dam"], am.grad, rtol=0, atol=1e-12) and torch.allclose(got["dlm"], lm.grad, rtol=0, atol=1e-12)


def test_simple_loss_edge_rules():
    V = 6
    c = P.simple_case(V)
    base = P.simple_loss_and_grad(c["am"], c["lm"], c["targets"], c["frames"], c["lengths"], V=V)
    assert torch.isfinite(base["nll"]).all()                 # U_b = 0 (utterance 1) is legal
    for what in ("frames", "blank", "low", "high"):
        fr, tg = c["frames"].clone(), c["targets"].clone()
        if what == "frames":
            fr[0] = 0
        else:
            tg[0, 1] = {"blank": 0, "low": -3, "high": V}[what]
        got = P.simple_loss_and_grad(c["am"], c["lm"], tg, fr, c["lengths"], V=V)
        assert math.isinf(float(got["nll"][0])) and not got["dam"][0].any() and not got["dlm"][0].any() and not got["gb"][0].any()
        assert torch.equal(got["nll"][1:], base["nll"][1:])


# ------------------------------------------------------------------------------------------------ the band
def test_band_properties_and_feasibility_on_random_occupancies():
    g = torch.Generator().manual_seed(0)
    for T, U, S in ((7, 5, 2), (7, 5, 3), (3, 2, 2), (12, 9, 4), (40, 30, 5), (4, 9, 4), (2, 7, 5)):
        occ = torch.rand((4, T, U + 1), generator=g, dtype=torch.float64)
        s = P.prune_ranges(occ, [T] * 4, [U] * 4, S)
        assert P.feasible(T, U, S)
        for b in range(4):
            assert P.band_properties(s[b], T, U, S), (T, U, S, s[b])


def test_band_ties_pick_the_lowest_start():
    occ = torch.full((1, 9, 8), 0.25)
    s = P.prune_ranges(occ, [9], [7], 3)
    assert s[0].tolist() == [0, 0, 0, 0, 0, 0, 1, 3, 5]
    occ[0, 4, 3:6] = 0.5                                     # frame 4: windows 1..5 hold 1.0, 1.25, 1.5 (start 3), 1.25, 1.0
    occ[0, 5, 2] = 0.5                                       # frame 5: starts 0, 1 and 2 tie at 1.0 -> 0, then held at s(4) = 2
    s = P.prune_ranges(occ, [9], [7], 3)
    assert s[0].tolist() == [0, 0, 0, 0, 2, 2, 2, 3, 5], s


def test_band_edge_cases():
    occ = torch.rand((5, 6, 5), generator=torch.Generator().manual_seed(1))
    frames, lengths = [6, 0, 1, 6, 3], [4, 4, 4, 1, 4]
    s = P.prune_ranges(occ, frames, lengths, 2)
    assert not s[1].any()                                    # T_b = 0
    assert s[2].tolist() == [3, 0, 0, 0, 0, 0] and not P.feasible(1, 4, 2)       # T_b = 1, U_b = 4, S = 2: s(0) = fin, no band exists
    assert not s[3].any()                                    # U_b + 1 <= W
    assert not s[4, 3:].any()                                # frames t >= T_b
    assert P.band_properties(s[0], 6, 4, 2)
    assert not P.prune_ranges(occ, frames, lengths, 64).any()          # S >= U + 1 everywhere


# ------------------------------------------------------------------------------------------------ the banded loss
def _all_bands(T, U, W):
    """Every s with s(0) = 0, s(T-1) = U + 1 - W and steps in 0 .. W-1."""
    fin = U + 1 - W
    if fin <= 0:
        return [[0] * T]
    out = []
    for steps in itertools.product(range(W), repeat=T - 1):
        s = [0]
        for d in steps:
            s.append(s[-1] + d)
        if s[-1] == fin:
            out.append(s)
    return out


@pytest.mark.parametrize("S", [2, 3])
def test_banded_loss_is_the_enumeration_of_every_alignment_inside_the_band(S):
    V = 4
    g = torch.Generator().manual_seed(S)
    n = 0
    for T in range(1, 5):
        for U in range(0, 4):
            W = min(S, U + 1)
            x = torch.randn((1, T, U + 1, V), generator=g, dtype=torch.float64) * 2
            y = torch.randint(1, V, (1, max(U, 1)), generator=g)
            bands = _all_bands(T, U, W) or [[U + 1 - W] * T]                    # none feasible: any s, the loss must be +inf
            for s in bands:
                st = torch.tensor([s], dtype=torch.int32)
                got = P.pruned_loss_and_grad(P.gather_band(x, st, W), y, [T], [U], st, U, V=V)
                want = P.nll_band_brute_force(x[0], y[0, :U].tolist(), s, W)
                if math.isinf(want):
                    assert math.isinf(float(got["nll"][0])) and not got["dlogits"].any()
                else:
                    assert abs(float(got["nll"][0]) - want) < 1e-11, (T, U, s)
                n += 1
    assert n >= 15


def test_a_band_as_wide_as_the_lattice_reproduces_the_full_loss_and_gradient_exactly():
    V = 9
    c = R.case(V)
    x = torch.nan_to_num(c["logits"], nan=0.0)
    s = torch.zeros((3, 7), dtype=torch.int32)
    for S in (6, 64):
        W = min(S, 6)
        got = P.pruned_loss_and_grad(P.gather_band(x, s, W), c["targets"], c["frames"], c["lengths"], s, 5, V=V, grad_out=0.7)
        want = R.loss_and_grad(x, c["targets"], c["frames"], c["lengths"], V=V, grad_out=0.7)
        assert torch.equal(got["nll"], want["nll"]) and torch.equal(got["loss"], want["loss"])
        assert torch.equal(got["dlogits"], want["dlogits"])


def test_banded_loss_is_never_below_the_full_loss_and_its_gradient_is_autograd():
    V = 6
    c = R.case(V)
    x = torch.nan_to_num(c["logits"], nan=0.0).double()
    full = R.loss_and_grad(x, c["targets"], c["frames"], c["lengths"], V=V)
    occ = torch.rand((3, 7, 6), generator=torch.Generator().manual_seed(3))
    for S in (2, 3, 4):
        s = P.prune_ranges(occ, c["frames"], c["lengths"], S)
        xb = P.gather_band(x, s, S).requires_grad_(True)
        got = P.pruned_loss_and_grad(xb.detach(), c["targets"], c["frames"], c["lengths"], s, 5, V=V)
        assert bool((got["nll"] >= full["nll"] - 1e-12).all()) and float(got["nll"][0]) > float(full["nll"][0])
        # autograd through a cell-by-cell lattice on the scattered band (-1e30 stands for -inf outside)
        total = 0.0
        for b, (Tb, Ub) in enumerate(zip(c["frames"].tolist(), c["lengths"].tolist())):
            lp = torch.full((Tb, Ub + 1, V), -1e30, dtype=torch.float64)
            rows = []
            for t in range(Tb):
                for w in range(S):
                    u = int(s[b, t]) + w
                    if u <= Ub:
                        rows.append((t, u, torch.log_softmax(xb[b, t, w], -1)))
            lp = lp.clone()
            for t, u, r in rows:
                lp[t, u] = r
            total = total + _nll_from_logprobs(lp, c["targets"][b, :Ub].tolist()) / max(Ub, 1)
        (total / 3).backward()
        assert torch.allclose(got["dlogits"], xb.grad, rtol=0, atol=1e-12)


def _nll_from_logprobs(lp, y, blank=0):
    T, U1, _ = lp.shape
    alpha = [[None] * U1 for _ in range(T)]
    for t in range(T):
        for u in range(U1):
            if t == 0 and u == 0:
                alpha[t][u] = lp.new_zeros(())
                continue
            terms = []
            if t > 0:
                terms.append(alpha[t - 1][u] + lp[t - 1, u, blank])
            if u > 0:
                terms.append(alpha[t][u - 1] + lp[t, u - 1, y[u - 1]])
            alpha[t][u] = terms[0] if len(terms) == 1 else torch.logaddexp(terms[0], terms[1])
    return -(alpha[T - 1][U1 - 1] + lp[T - 1, U1 - 1, blank])


def test_the_infeasible_utterance_and_the_edge_rules_of_the_banded_loss():
    V = 5
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 3, 2, V), generator=g, dtype=torch.float64)
    y = torch.tensor([[1, 2, 3, 4], [1, 2, 0, 0]])
    s = torch.tensor([[3, 0, 0], [0, 0, 1]], dtype=torch.int32)
    got = P.pruned_loss_and_grad(x, y, [1, 3], [4, 2], s, 4, V=V)         # utterance 0: T_b = 1, U_b = 4, S = 2
    assert math.isinf(float(got["nll"][0])) and not got["dlogits"][0].any()
    assert math.isfinite(float(got["nll"][1])) and got["dlogits"][1].any()
    for fr, yy in (([0, 3], y), ([1, 3], torch.tensor([[1, 2, 3, 4], [1, 0, 0, 0]])), ([1, 3], torch.tensor([[1, 2, 3, 4], [1, V, 0, 0]]))):
        bad = P.pruned_loss_and_grad(x, yy, fr, [4, 2], s, 4, V=V)
        assert math.isinf(float(bad["nll"][0]))
        if fr[0] == 1:
            assert math.isinf(float(bad["nll"][1])) and not bad["dlogits"].any()


def test_banded_joint_is_the_gathered_full_joint():
    g = torch.Generator().manual_seed(4)
    B, T, U1, W, J = 2, 5, 6, 3, 8
    e, p = torch.randn((B, T, J), generator=g), torch.randn((B, U1, J), generator=g)
    s = torch.tensor([[0, 0, 1, 3, 3], [0, 2, 2, 3, 3]], dtype=torch.int32)
    z = P.joint_pruned(e, p, s, W)
    assert torch.equal(z, P.gather_band(R.joint(e, p), s, W))
    e64, p64 = e.double().requires_grad_(True), p.double().requires_grad_(True)
    dz = torch.randn((B, T, W, J), generator=g, dtype=torch.float64)
    (P.gather_band(torch.tanh(e64[:, :, None] + p64[:, None]), s, W) * dz).sum().backward()
    de, dp = P.joint_pruned_bwd(dz, z, s, U1)
    assert torch.allclose(de, e64.grad, rtol=0, atol=1e-13) and torch.allclose(dp, p64.grad, rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------------ flags, keys, checkpoints
from test_joint_ctc_host import FLAGS, KEYS_TODAY, _labels  # noqa: E402
from test_rnnt_host import cli  # noqa: E402,F401  (fixture)

HEAD = ["--transducer-weight", "0.3", "--transducer-dim-joint", "16"]
SIMPLE_KEYS = {"rnnt_simple_am.weight", "rnnt_simple_am.bias", "rnnt_simple_lm.weight", "rnnt_simple_lm.bias"}


def _model(cli, extra=()):
    from utils.functions import init_transformer_model
    l2i, i2l = _labels()
    return init_transformer_model(cli(FLAGS + list(extra)), l2i, i2l)


def test_with_the_flag_off_the_keys_and_the_initial_weights_are_the_parents(cli):
    from utils import constant
    assert constant.parser.get_default("transducer_prune_range") == 0 and constant.parser.get_default("transducer_simple_scale") == 0.5
    assert list(_model(cli, ["--transducer-prune-range", "0"]).state_dict().keys()) == KEYS_TODAY
    torch.manual_seed(3)
    a = _model(cli, HEAD).state_dict()
    torch.manual_seed(3)
    b = _model(cli, HEAD + ["--transducer-prune-range", "0", "--transducer-simple-scale", "0.25"]).state_dict()
    assert list(a.keys()) == list(b.keys()) and not SIMPLE_KEYS & set(a) and all(torch.equal(a[k], b[k]) for k in a)


def test_the_range_adds_exactly_the_two_simple_layers(cli):
    V = len(_labels()[0])
    plain = _model(cli, HEAD)
    model = _model(cli, HEAD + ["--transducer-prune-range", "3"])
    sd = model.state_dict()
    assert set(sd) - set(plain.state_dict()) == SIMPLE_KEYS and set(plain.state_dict()) <= set(sd)
    assert tuple(sd["rnnt_simple_am.weight"].shape) == (V, 32) and tuple(sd["rnnt_simple_lm.weight"].shape) == (V, 16)
    assert model.rnnt_prune_range == 3 and plain.rnnt_prune_range == 0
    bound = math.sqrt(6.0 / (V + 32))                        # Xavier, like every other matrix
    assert float(sd["rnnt_simple_am.weight"].abs().max()) <= bound and float(sd["rnnt_simple_am.weight"].abs().max()) > 0.5 * bound


def test_new_flag_refusals(cli):
    import train
    for bad, match in ((["--transducer-prune-range", "1"], "2..64"), (["--transducer-prune-range", "65"], "2..64"),
                       (["--transducer-prune-range", "-2"], "2..64"), (["--transducer-prune-range", "3", "--transducer-simple-scale", "-0.1"], ">= 0"),
                       (["--transducer-prune-range", "3", "--parallel"], "--parallel"), (["--transducer-prune-range", "3", "--rank", "8"], "--rank"),
                       (["--transducer-prune-range", "3", "--loss", "ctc"], "--loss ctc")):
        with pytest.raises(ValueError, match=match):
            _model(cli, HEAD + bad)
        cli(FLAGS + HEAD + bad)
        with pytest.raises(ValueError, match=match):           # train.py refuses them at start-up, before anything is built
            train.main()
    with pytest.raises(ValueError, match="needs --transducer-weight > 0"):
        _model(cli, ["--transducer-prune-range", "3"])
    _model(cli, HEAD + ["--transducer-prune-range", "2", "--transducer-simple-scale", "0"])
    _model(cli, HEAD + ["--transducer-prune-range", "64"])
    from models.asr.transformer import Transformer
    plain = _model(cli, HEAD)
    with pytest.raises(ValueError, match="2..64"):
        Transformer(plain.encoder, plain.decoder, feat_extractor=plain.feat_extractor, transducer=dict(dim_joint=16, context=2, prune_range=1))
    # the model's own entry points refuse before any device work
    x, y = torch.zeros(1, 2, 32), torch.ones(1, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="--transducer-prune-range 0"):
        plain.transducer_pruned_loss(x, [8], y, [2])
    with pytest.raises(ValueError, match="transducer head"):
        _model(cli).transducer_pruned_loss(x, [8], y, [2])
    pruned = _model(cli, HEAD + ["--transducer-prune-range", "3"])
    with pytest.raises(ValueError, match=">= 0"):
        pruned.transducer_pruned_loss(x, [8], y, [2], simple_scale=-1.0)
    # the band, not the lattice, meets the 2^31-byte bound: U 60 at the workload's shape is refused in full and passes with S 5
    from asr_hip import functions as F_
    with pytest.raises(ValueError, match="2\\^31"):
        F_.check_rnnt_shape(32, 75, 61, 4364)
    F_.check_rnnt_shape(32, 75, 5, 4364)
    F_.check_rnnt_shape(16, 400, 5, 4364)
    with pytest.raises(ValueError, match="2\\^31"):              # before any launch: the tensors are on the host, nothing could run
        F_.RnntPrunedFn.apply(torch.zeros(1).expand(1 << 12, 1 << 10, 1 << 5, 1 << 4), torch.ones(1 << 12, 40, dtype=torch.int64),
                              [1 << 10] * (1 << 12), [40] * (1 << 12), torch.zeros((1 << 12, 1 << 10), dtype=torch.int32), 40, 0)


def _save(cli, tmp_path, extra):
    from utils import constant
    from utils.functions import init_optimizer, save_model
    model = _model(cli, ["--save-folder", str(tmp_path), "--name", "ck"] + list(extra))
    opt = init_optimizer(constant.args, model, "noam")
    l2i, i2l = _labels()
    save_model(model, 1, opt, {"valid_loss": 1.0}, l2i, i2l)
    return model, str(tmp_path / "ck" / "epoch_1.th")


def test_checkpoint_round_trip_of_the_range_and_the_scale(cli, tmp_path):
    from utils import constant
    from utils.functions import load_model
    model, path = _save(cli, tmp_path, HEAD + ["--transducer-prune-range", "3", "--transducer-simple-scale", "0.25"])
    cli(["--continue-from", path])                           # no flag: the layers come back from the checkpoint's own settings
    loaded, _, _, _, largs, _, _ = load_model(path)
    assert (largs.transducer_prune_range, largs.transducer_simple_scale) == (3, 0.25)
    assert (constant.args.transducer_prune_range, constant.args.transducer_simple_scale) == (3, 0.25)
    assert set(loaded.state_dict()) == set(model.state_dict()) and SIMPLE_KEYS <= set(loaded.state_dict()) and loaded.rnnt_prune_range == 3
    for k, v in model.state_dict().items():
        assert torch.equal(v, loaded.state_dict()[k]), k
    # a positive range may replace a positive one (it only sizes the band), and the scale may change
    cli(["--continue-from", path, "--transducer-prune-range", "5", "--transducer-simple-scale", "0.1"])
    loaded, _, _, _, largs, _, _ = load_model(path)
    assert (largs.transducer_prune_range, largs.transducer_simple_scale) == (5, 0.1) and loaded.rnnt_prune_range == 5
    assert constant.args.transducer_prune_range == 5 and SIMPLE_KEYS <= set(loaded.state_dict())
    # the two layers cannot be dropped; bad values are refused
    cli(["--continue-from", path, "--transducer-prune-range", "0"])
    with pytest.raises(ValueError, match=r"--transducer-prune-range 0 .*--transducer-prune-range 3.*cannot be dropped"):
        load_model(path)
    cli(["--continue-from", path, "--transducer-prune-range", "1"])
    with pytest.raises(ValueError, match="2..64"):
        load_model(path)
    cli(["--continue-from", path, "--transducer-simple-scale", "-1"])
    with pytest.raises(ValueError, match=">= 0"):
        load_model(path)


def test_checkpoint_without_the_simple_layers_loads_unchanged_and_cannot_gain_them(cli, tmp_path):
    from utils.functions import load_model
    model, path = _save(cli, tmp_path, HEAD)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert not SIMPLE_KEYS & set(ck["model_state_dict"])
    for k in ("transducer_prune_range", "transducer_simple_scale"):      # a checkpoint written before the flags existed
        delattr(ck["args"], k)
    torch.save(ck, path)
    cli(["--continue-from", path])
    loaded, _, _, _, largs, _, _ = load_model(path)
    assert list(loaded.state_dict().keys()) == list(model.state_dict().keys())
    assert (largs.transducer_prune_range, largs.transducer_simple_scale) == (0, 0.5)
    cli(["--continue-from", path, "--transducer-prune-range", "3"])
    with pytest.raises(ValueError, match=r"--transducer-prune-range 3 .*--transducer-prune-range 0.*cannot be added"):
        load_model(path)
