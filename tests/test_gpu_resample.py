"""asr_resample on the GPU (csrc/resample.hip) against the restatement of DESIGN.md section 7 (tests/resample_reference.py): bit for bit
on exact data inside a buffer of sentinels, within the fp32 chain's error bound on real tables, sines, batch invariance, repeatability,
the identity, the binding's refusals, the front end with 7-column draws, and train.py --speed-perturb."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resample_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu
SR = 16000
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def ops():
    from asr_hip import ops as o
    torch.cuda.set_device(0)
    return o


def _pad(xs, Lmax=None):
    Lmax = max(max(x.size for x in xs), 1) if Lmax is None else Lmax
    wav = np.zeros((len(xs), Lmax), np.float32)
    for i, x in enumerate(xs):
        wav[i, :x.size] = x
    return torch.from_numpy(wav)


def _dyadic_tables(ps, seed=0, R_of=None):
    """{p: (R, H)}: tables of the definition's shape with values k / 64, |k| <= 128 -- with integer samples |x| <= 64 every partial sum
    of the chain is a multiple of 2^-6 below 2^15: exact in float32."""
    rng = np.random.RandomState(seed)
    out = {}
    for p in ps:
        num, den = RR.ratio(p)
        R = RR.half_width(num, den) if R_of is None else R_of[p]
        out[p] = (R, (rng.randint(-128, 129, (den, 2 * R)) / 64.0).astype(np.float32))
    return out


def _expected_exact(xs, ps, tables):
    exp = []
    for x, p in zip(xs, ps):
        if p in (0, 1000):
            exp.append(x.copy())
        else:
            num, den = RR.ratio(p)
            R, H = tables[p]
            exp.append(RR.resample32_exact(x, num, den, R, H, RR.length(x.size, p)))
    return exp


def _run_in_sentinels(ops, xs, ps, tables, aligned):
    """The batch resampled into the middle of a buffer of sentinels: a guard row before and after, out_stride > out_cols, and out_cols
    beyond the longest output.  aligned: 16-byte loads and stores possible (strides multiples of 4) or not."""
    B = len(xs)
    n_max = max(max(RR.length(x.size, p) if p not in (0, 1000) else x.size for x, p in zip(xs, ps)), 1)
    Lmax = max(max(x.size for x in xs), 1)
    if aligned:
        Lmax, cols = (Lmax + 3) // 4 * 4, (n_max + 3) // 4 * 4 + 8
        stride = cols + 4
    else:
        Lmax, cols = Lmax | 1, n_max + 3
        stride = cols + 5 if (cols + 5) % 4 else cols + 6
    assert (stride % 4 == 0) == aligned and (Lmax % 4 == 0) == aligned
    buf = torch.full((B + 2, stride), SENTINEL, device="cuda")
    out = buf[1:B + 1, :cols]
    got, lens = ops.resample(_pad(xs, Lmax).cuda(), torch.tensor([x.size for x in xs]), torch.tensor(ps), tables=tables, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu()
    assert (host[0] == SENTINEL).all() and (host[B + 1] == SENTINEL).all() and (host[1:B + 1, cols:] == SENTINEL).all()
    return host[1:B + 1, :cols], lens.cpu()


def _check_rows(got, lens, exp, what):
    for b, e in enumerate(exp):
        n = e.size
        assert int(lens[b]) == n, (what, b)
        assert torch.equal(got[b, :n], torch.from_numpy(e)), (what, b, n)
        assert not got[b, n:].numpy().view(np.int32).any(), (what, b, "the tail is +0.0")


RATIOS = [900, 1100, 1000, 997, 1003, 2000, 500, 1500]          # 9/10, 11/10, 1/1 (copied), 997/1000, 1003/1000, 2/1, 1/2, 3/2


@pytest.mark.parametrize("aligned", [False, True])
def test_exact_data_bit_for_bit_inside_sentinels(ops, aligned):
    tile = ops.RESAMPLE_TILE
    tables = _dyadic_tables([p for p in RATIOS if p != 1000])
    assert tables[2000][0] == 13 and tables[900][0] == 7 and tables[997][1].shape == (1000, 14)
    rng = np.random.RandomState(1)
    for rot in range(8):
        xs, ps = [], RATIOS
        for b, p in enumerate(ps):
            R = tables[p][0] if p != 1000 else 7
            n = [0, 1, R - 1, 2 * R, tile - 1, tile, tile + 1, 3 * tile + 5][(b + rot) % 8]
            xs.append(rng.randint(-64, 65, n).astype(np.float32))
        got, lens = _run_in_sentinels(ops, xs, ps, tables, aligned)
        _check_rows(got, lens, _expected_exact(xs, ps, tables), "rotation %d" % rot)
    # output lengths at the tile's edges: inputs of about (tile - 1, tile, tile + 1) num / den samples
    xs = [rng.randint(-64, 65, int(round((tile - 1 + b % 3) * p / 1000.0))).astype(np.float32) for b, p in enumerate(RATIOS)]
    got, lens = _run_in_sentinels(ops, xs, RATIOS, tables, aligned)
    assert {tile - 1, tile, tile + 1} <= set(lens.tolist())
    _check_rows(got, lens, _expected_exact(xs, RATIOS, tables), "tile edges")


def test_a_filter_longer_than_the_staged_span_is_exact_too(ops):
    """2/1 with R = 80: a tile's input span (2 tile + 2R) exceeds the kernel's LDS image, the samples are then read from memory."""
    ps = [2000, 1500, 2000]
    tables = _dyadic_tables([2000, 1500], seed=4, R_of={2000: 80, 1500: 11})
    rng = np.random.RandomState(5)
    xs = [rng.randint(-64, 65, n).astype(np.float32) for n in (4100, 2051, 79)]
    got, lens = _run_in_sentinels(ops, xs, ps, tables, aligned=False)
    _check_rows(got, lens, _expected_exact(xs, ps, tables), "long filter")


def test_a_table_at_an_odd_offset_is_exact_too(ops):
    """An explicit plan whose tables sit at odd offsets with a gap between them: nothing assumes a table's alignment or that the
    tables are packed."""
    tables = _dyadic_tables([900, 1100], seed=6)
    rng = np.random.RandomState(8)
    xs = [rng.randint(-64, 65, n).astype(np.float32) for n in (2100, 1500)]
    flat = [np.zeros(1, np.float32), tables[900][1].reshape(-1), np.zeros(2, np.float32), tables[1100][1].reshape(-1)]
    plan = [[9, 10, 7, 1, RR.length(2100, 900), 0, 0, 0], [11, 10, 7, 1 + 140 + 2, RR.length(1500, 1100), 0, 0, 0]]
    out = torch.full((2, plan[0][4] + 2), SENTINEL, device="cuda")
    ops.resample_launch(_pad(xs).cuda(), [2100, 1500], plan, torch.from_numpy(np.concatenate(flat)).cuda(), out)
    _check_rows(out.cpu(), [r[4] for r in plan], _expected_exact(xs, [900, 1100], tables), "odd offset")


@pytest.fixture(scope="module")
def real_batch(ops):
    """Random fp32 waveforms through the real tables, once: (xs, ps, out, lens)."""
    rng = np.random.RandomState(7)
    ps = [900, 997, 1100, 2000]
    xs = [rng.randn(n).astype(np.float32) for n in (5000, 4999, 4097, 3001)]
    out, lens = ops.resample(_pad(xs).cuda(), torch.tensor([x.size for x in xs]), torch.tensor(ps))
    torch.cuda.synchronize()
    return xs, ps, out.cpu(), lens.cpu()


def test_real_tables_within_the_fp32_chain_bound(ops, real_batch):
    """Against the float64 restatement fed the same float32 table: |y - y64| <= (2R + 1) 2^-24 sum_q |H x|, the standard bound of an
    fp32 multiply-add chain of 2R terms."""
    from utils.audio import resample_table
    xs, ps, out, lens = real_batch
    assert out.shape == (4, max(RR.length(x.size, p) for x, p in zip(xs, ps)))
    for b, (x, p) in enumerate(zip(xs, ps)):
        num, den = RR.ratio(p)
        R, H = resample_table(p)
        n_out = RR.length(x.size, p)
        y64, mag = RR.resample64(x, num, den, R, H, n_out)
        err = np.abs(out[b, :n_out].numpy().astype(np.float64) - y64)
        bound = (2 * R + 1) * 2.0 ** -24 * mag
        print("p %d: max error %.3e, bound there %.3e, smallest bound %.3e" % (p, err.max(), bound[err.argmax()], bound.min()))
        assert int(lens[b]) == n_out and (err <= bound).all()
        assert not out[b, n_out:].numpy().view(np.int32).any()


def test_sines_on_the_device(ops):
    cases = [(p, f) for p in (900, 997, 1100) for f in (200, 1000, 3000)]
    n = 16000
    xs = [np.sin(2 * np.pi * f * np.arange(n) / SR).astype(np.float32) for _, f in cases]
    out, lens = ops.resample(_pad(xs).cuda(), torch.tensor([n] * len(cases)), torch.tensor([p for p, _ in cases]))
    out = out.cpu().numpy()
    for b, (p, f) in enumerate(cases):
        n_out, R = RR.length(n, p), RR.half_width(*RR.ratio(p))
        ideal = np.sin(2 * np.pi * f * (p / 1000.0) * np.arange(n_out) / SR)
        err = np.abs(out[b, :n_out] - ideal)[4 * R:n_out - 4 * R].max()
        print("p %d f %d: max interior error %.3e" % (p, f, err))
        assert int(lens[b]) == n_out and err <= 2e-3


def test_batch_invariance_and_repeatability(ops, real_batch):
    xs, ps, out, lens = real_batch
    again, lens2 = ops.resample(_pad(xs).cuda(), torch.tensor([x.size for x in xs]), torch.tensor(ps))
    assert torch.equal(again.cpu(), out) and torch.equal(lens2.cpu(), lens)
    for b in (1, 3):
        alone, n1 = ops.resample(torch.from_numpy(xs[b])[None].cuda(), torch.tensor([xs[b].size]), torch.tensor([ps[b]]))
        n = int(n1[0])
        assert n == int(lens[b]) and alone.shape == (1, n) and torch.equal(alone.cpu()[0], out[b, :n])


def test_identity_returns_the_input_and_launches_nothing(ops, monkeypatch):
    wav = torch.randn(3, 100).cuda()
    lens = torch.tensor([100, 7, 0], dtype=torch.int32).cuda()

    def no_launch(*a, **k):
        raise AssertionError("an all-identity batch must not launch")
    monkeypatch.setattr(ops.L, "call", no_launch)
    for p in ([1000, 1000, 1000], [0, 1000, 0]):
        out, n = ops.resample(wav, lens, torch.tensor(p))
        assert out is wav and n is lens
    out, n = ops.resample(wav, [100, 7, 0], [0, 0, 0])
    assert out is wav and n.dtype == torch.int32 and n.is_cuda and n.tolist() == [100, 7, 0]


def test_copied_rows_inside_a_mixed_batch(ops):
    rng = np.random.RandomState(9)
    xs = [rng.randn(n).astype(np.float32) for n in (1500, 1029, 3)]
    out, lens = ops.resample(_pad(xs).cuda(), torch.tensor([1500, 1029, 3]), torch.tensor([1000, 900, 0]))
    out = out.cpu()
    assert lens.tolist() == [1500, 1143, 3] and out.shape == (3, 1500)
    assert torch.equal(out[0], torch.from_numpy(xs[0])) and torch.equal(out[2, :3], torch.from_numpy(xs[2])) and not out[2, 3:].any()


def test_binding_refusals(ops):
    from asr_hip import lib as L
    wav = torch.zeros(2, 64).cuda()
    table = torch.zeros(10 * 14).cuda()
    out = torch.zeros(2, 80).cuda()
    good = [[9, 10, 7, 0, 71, 0, 0, 0], [1, 1, 1, 0, 64, 0, 0, 0]]
    ops.resample_launch(wav, [64, 64], good, table, out)
    for what, row in (("den", [1001, 1001 * 2, 7, 0, 10, 0, 0, 0]), ("den", [3, 1001, 7, 0, 10, 0, 0, 0]), ("num", [0, 10, 7, 0, 10, 0, 0, 0]),
                      ("R >= 1", [9, 10, 0, 0, 10, 0, 0, 0]), ("table", [9, 10, 7, 1, 10, 0, 0, 0]), ("table", [9, 10, 8, 0, 10, 0, 0, 0]),
                      ("table", [9, 10, 7, -1, 10, 0, 0, 0]), ("n_out", [9, 10, 7, 0, 81, 0, 0, 0]), ("n_out", [9, 10, 7, 0, -1, 0, 0, 0])):
        with pytest.raises(ValueError, match=what):
            ops.resample_launch(wav, [64, 64], [row, good[1]], table, out)
    with pytest.raises(ValueError, match="table"):
        ops.resample_launch(wav, [64, 64], good, None, out)
    with pytest.raises(ValueError, match="lengths"):
        ops.resample_launch(wav, [65, 64], good, table, out)
    for p in (499, 2001, -900, 1):
        with pytest.raises(ValueError, match="speed factors"):
            ops.resample(wav, [64, 64], [1000, p])
    with pytest.raises(ValueError, match="n_out"):                              # 64 samples at 0.9 are 71: a caller's buffer of 70 columns
        ops.resample(wav, [64, 64], [900, 1000], out=out[:, :70])
    with pytest.raises(ValueError, match="table of factor"):
        ops.resample(wav, [64, 64], [900, 1000], tables={900: (7, np.zeros((10, 12), np.float32))})
    # the entry point itself refuses bad geometry: out_stride < out_cols, a negative count
    plan = torch.tensor(good, dtype=torch.int32).cuda()
    lens = torch.tensor([64, 64], dtype=torch.int32).cuda()
    args = [L.ptr(wav), 64, L.ptr(lens), L.ptr(plan), L.ptr(table), 140, L.ptr(out)]
    for tail in ((79, 80, 2), (80, -1, 2), (80, 80, -1)):
        with pytest.raises(L.AsrHipError):
            L.call("asr_resample", *args, *tail, L.stream())
    L.call("asr_resample", *args, 80, 80, 0, L.stream())                        # B = 0: nothing to do
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ front end
def _spy(monkeypatch, ops, name):
    seen = []
    real = getattr(ops, name)

    def spy(*a, **k):
        seen.append((a, k))
        return real(*a, **k)
    monkeypatch.setattr(ops, name, spy)
    return seen


def _front_end_bound(ops, wav, lens, feat, nfr, kind, window="hamming"):
    """Two launches of the front end normalise the same raw features with statistics whose float atomics add in another order (what
    tests/test_gpu_specaug.py states): a sum of N float32 terms is within (N - 1) 2^-24 sum|x| of the exact one in any order, so the
    means of two launches differ by at most 2 N u mean|x| and the reciprocal deviations by 2 N u relatively; a normalised value y = (x -
    mean) rstd then by at most 2 N u (mean|x| rstd + |y|) (+ 3 u |y| of its own roundings, inside the factor 2).  Per utterance."""
    raw, n_all = ops.log_spectrogram(wav, lens, normalize=False, window=window, **kind)
    raw, y = raw.cpu().numpy().astype(np.float64), feat.cpu().numpy().astype(np.float64)
    tol = []
    for b, n in enumerate(n_all.tolist()):
        x = raw[b, 0, :, :n]
        N = x.size
        tol.append(2 * N * 2.0 ** -24 * (np.abs(x).mean() / x.std(ddof=1) + np.abs(y[b]).max()))
    return tol


@pytest.mark.parametrize("case", ["plain", "tempo gain noise spec", "fbank"])
def test_front_end_with_seven_columns_is_the_front_end_on_the_resampled_batch(ops, tmp_path, monkeypatch, case):
    """gpu_front_end with 7-column draws against gpu_front_end with the corresponding 6-column draws on waveforms pre-resampled by
    ops.resample.  What enters asr_augment_wave and the STFT is compared with torch.equal, and so are the frame counts; the features
    come out of the same kernels on the same bits, but their normalisation adds its statistics with float atomics, so two launches agree
    only up to the order of those sums (_front_end_bound) -- they are compared within that bound, and bit for bit where it is zero."""
    import specaug_reference as SA
    import test_augment_host as H
    from utils.audio import _device_mel_bank, gpu_front_end, spec_frames, tempo_length
    rng = np.random.RandomState(12)
    ns, ps = [9000, 8000, 7001, 6000], [900, 1000, 1100, 997]
    xs = [(rng.randn(n) * 0.1).astype(np.float32) for n in ns]
    mids = [RR.length(n, p) for n, p in zip(ns, ps)]
    full = case == "tempo gain noise spec"
    tempos, gains = ([1.1, 0.0, 0.9, 1.0], [3.0, 0.0, -2.5, 0.0]) if full else ([0.0] * 4, [0.0] * 4)
    clips, starts, levels = ([1, -1, 0, -1], [0.05, 0.0, 0.2, 0.0], [0.3, 0.0, 0.1, 0.0]) if full else ([-1] * 4, [0.0] * 4, [0.0] * 4)
    nd = str(H.noise_dir(tmp_path)) if full else None
    finals = [tempo_length(m, t) if t > 0 else m for m, t in zip(mids, tempos)]
    kw = dict(noise_dir=nd, src_max_len=60 if full else None)
    kind = {}
    if case == "fbank":
        kw.update(features="fbank", num_mel_bins=40)
        kind = dict(features="fbank", mel=_device_mel_bank(40, 320, SR, 20.0, torch.device("cuda", 0)))
    if full:
        kw["spec"] = torch.tensor([SA.row(spec_frames(n, 160, 60), 20, 25, fmasks=[(3, 9)], tmasks=[(5, 6)]) for n in finals], dtype=torch.int32)
    seven = torch.tensor([(n, t, g, c, s, l, p) for n, t, g, c, s, l, p in zip(ns, tempos, gains, clips, starts, levels, ps)], dtype=torch.float64)
    six = torch.tensor([(m, t, g, c, s, l) for m, t, g, c, s, l in zip(mids, tempos, gains, clips, starts, levels)], dtype=torch.float64)
    wav = _pad(xs).cuda()
    pre, pre_lens = ops.resample(wav, torch.tensor(ns), torch.tensor(ps))
    assert pre_lens.tolist() == mids and pre.shape == (4, max(mids))
    seen_aug, seen_stft = _spy(monkeypatch, ops, "augment_wave"), _spy(monkeypatch, ops, "log_spectrogram")
    sizes = torch.tensor(finals, dtype=torch.int32)
    a, na = gpu_front_end(wav[:, None, None, :], sizes, aug=seven, **kw)
    b, nb = gpu_front_end(pre[:, None, None, :].clone(), sizes, aug=six, **kw)
    assert len(seen_aug) == 2 and len(seen_stft) == 2
    (w7, l7, p7, bank7), (w6, l6, p6, bank6) = seen_aug[0][0][:4], seen_aug[1][0][:4]
    assert torch.equal(w7, w6) and torch.equal(w7, pre) and torch.equal(l7, l6) and torch.equal(p7, p6) and bank7 is bank6
    (s7, sl7), (s6, sl6) = seen_stft[0][0][:2], seen_stft[1][0][:2]
    assert torch.equal(s7, s6) and torch.equal(sl7, sl6) and sl7.tolist() == finals
    assert torch.equal(na, nb) and a.shape == b.shape and na.tolist() == [spec_frames(n, 160, kw["src_max_len"]) for n in finals]
    tol = _front_end_bound(ops, s7, sl7, a, na, kind)
    for u in range(4):
        d = (a[u] - b[u]).abs().max().item()
        print("%s utterance %d: max |difference| of two launches %.3e, bound %.3e" % (case, u, d, tol[u]))
        assert d <= tol[u]
        for z in (a[u], b[u]):                                                 # padding and masks: +0.0 in both
            assert not z[..., int(na[u]):].any() and (not full or not (z[:, 3:12].any() or z[..., 5:11].any()))
    with pytest.raises(ValueError, match="input_sizes"):                       # the sizes must count the speed step
        gpu_front_end(wav[:, None, None, :], torch.tensor([n if i else n + 1 for i, n in enumerate(finals)], dtype=torch.int32), aug=seven, **kw)
    with pytest.raises(ValueError, match="input_sizes"):
        gpu_front_end(wav[:, None, None, :], torch.tensor([tempo_length(n, t) if t > 0 else n for n, t in zip(ns, tempos)]), aug=seven, **kw)


# ------------------------------------------------------------------------------------------------ train.py
@pytest.mark.parametrize("buckets", [None, "0"])
def test_train_with_speed_perturbation(tmp_path, monkeypatch, capsys, buckets):
    import test_gpu_train_cli as C
    import trainer.asr.trainer as trainer_mod
    from utils import constant
    from utils.audio import speed_length
    man, lab = C._corpus(tmp_path)
    monkeypatch.chdir(tmp_path)
    argv = ["--train-manifest-list", man, "--valid-manifest-list", man, "--test-manifest-list", man, "--labels-path", lab,
            "--cuda", "--batch-size", "3", "--num-workers", "0", "--epochs", "2", "--save-every", "1", "--name", "tinyspeed",
            "--save-folder", str(tmp_path / "save"), "--num-layers", "1", "--num-heads", "2", "--dim-model", "32", "--dim-key",
            "16", "--dim-value", "16", "--dim-inner", "64", "--dim-emb", "32", "--tgt-max-len", "12", "--src-max-len", "64",
            "--label-smoothing", "0.1", "--dropout", "0.1", "--k-lr", "20", "--warmup", "5", "--clip",
            "--speed-perturb", "0.9", "1.0", "1.1"] + (["--graph-buckets", buckets] if buckets is not None else [])
    seen = []
    real = trainer_mod.gpu_front_end

    def spy(src, sizes, *a, **k):
        seen.append((torch.as_tensor(sizes).tolist(), None if k.get("aug") is None else k["aug"].clone()))
        return real(src, sizes, *a, **k)
    monkeypatch.setattr(trainer_mod, "gpu_front_end", spy)
    old, old_cuda = constant.args, constant.USE_CUDA
    try:
        constant.parse(argv)
        np.random.seed(2)
        random.seed(2)
        import train as train_mod
        train_mod.main()
        assert constant.args.gpu_frontend and "--gpu-frontend turned on" in capsys.readouterr().out
        assert (constant.args.graph_buckets > 0) == (buckets is None)
        state = torch.load(str(tmp_path / "save" / "tinyspeed" / "best_model.th"), map_location="cpu", weights_only=False)
        assert np.isfinite(state["metrics"]["train_loss"]) and state["optimizer_params"]["_step"] >= 4
    finally:
        constant.set_args(old)
        constant.USE_CUDA = old_cuda
    raw = {4000 + 800 * i for i in range(6)}                                   # the corpus' sample counts: what an unperturbed run sees
    train = [(s, a) for s, a in seen if a is not None]
    valid = [s for s, a in seen if a is None]
    assert len(train) == 4 and valid and all(set(s) <= raw for s in valid)     # validation never perturbs
    for sizes, aug in train:
        assert aug.shape == (3, 7) and set(aug[:, 0].long().tolist()) <= raw and set(aug[:, 6].long().tolist()) <= {900, 1000, 1100}
        assert sizes == [speed_length(n, p) for n, p in zip(aug[:, 0].long().tolist(), aug[:, 6].long().tolist())]
        assert sizes == sorted(sizes, reverse=True)
    drawn = {p for _, aug in train for p in aug[:, 6].long().tolist()}
    assert drawn & {900, 1100} and any(not set(s) <= raw for s, _ in train)    # lengths no unperturbed batch has
