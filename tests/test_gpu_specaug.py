"""SpecAugment on the GPU (csrc/spec_augment.hip, asr_spect_finish_aug) against the float64 definition of tests/specaug_reference.py:
masks bit for bit, the time warp within 5 * 2^-24 * max|x| (one rounding each in frac and x1 - x0, each scaled by at most 2 max|x|,
and one in the fma), the fused launcher bit for bit against the separate passes, the front end with loader-drawn rows, and a
trainer step under --graph-buckets."""
import json
import random
import wave

import numpy as np
import pytest
import torch

import specaug_reference as R

pytestmark = pytest.mark.gpu
SHAPES = [(F, T) for F in (5, 161) for T in (37, 64, 257)]
WARP_BOUND = 5 * 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from asr_hip import ops as o
    torch.cuda.set_device(0)
    return o


def _input(F, T, ns, seed=0):
    """(B, 1, F, T) float32 with NaN planted from frame n on: nothing there may reach the output."""
    x = (np.random.RandomState(seed).randn(len(ns), 1, F, T) * 1.5).astype(np.float32)
    for b, n in enumerate(ns):
        x[b, ..., n:] = np.nan
    return x


def _ns(T):
    return [T, T - 5, 2]


def _run(ops, x, rows):
    y = ops.spec_augment(torch.from_numpy(x).cuda(), torch.tensor(rows, dtype=torch.int32))
    torch.cuda.synchronize()
    assert y.shape == x.shape and y.is_contiguous()
    return y.cpu().numpy()


def _check_exact(y, x, rows):
    ref = R.spec_augment_batch(x[:, 0], rows)
    assert np.array_equal(y[:, 0], ref.astype(np.float32)), "values"
    assert not np.signbit(y[:, 0][ref == 0]).any(), "masked values are +0.0"


def _check_warp(y, x, rows, what, slack=0):
    ref = R.spec_augment_batch(x[:, 0], rows)
    for b, r in enumerate(rows):
        n = r[0]
        scale = np.abs(x[b, 0, :, :n]).max()
        err = np.abs(y[b, 0].astype(np.float64) - ref[b]).max()
        print("%s: utterance %d n %d c %d w %d: max err %.3g = %.2f * 2^-24 * max|x| (bound %d)" % (
            what, b, n, r[1], r[2], err, err / scale * 2 ** 24, 5 + slack))
        assert err <= (WARP_BOUND + slack * 2.0 ** -24) * scale, (what, b, r[:3])
        assert not y[b, 0, :, n:].any()


@pytest.mark.parametrize("F,T", SHAPES)
def test_masks_only_are_bit_exact(ops, F, T):
    ns = _ns(T)
    x = _input(F, T, ns)
    variants = {
        "overlapping": lambda n: R.row(n, fmasks=[(1, 3), (2, 2)], tmasks=[(n // 3, 4), (n // 3 + 2, 5)]),
        "width 0": lambda n: R.row(n, fmasks=[(2, 0)], tmasks=[(1, 0), (n - 1, 0)]),
        "all of F": lambda n: R.row(n, fmasks=[(0, F)], tmasks=[(0, 1)]),
        "all of [0, n)": lambda n: R.row(n, fmasks=[(F - 1, 1)], tmasks=[(0, n)]),
        "8 + 8": lambda n: R.row(n, fmasks=[((3 * k) % (F - 1), k % 2) for k in range(8)],
                                 tmasks=[((7 * k) % n, min(1 + k % 3, n - (7 * k) % n)) for k in range(8)]),
        "none": lambda n: R.row(n),
    }
    for name, make in variants.items():
        rows = [make(n) for n in ns]
        _check_exact(_run(ops, x, rows), x, rows)
    rows = [variants["8 + 8"](n) for n in ns]
    assert rows[0][3] == 8 and rows[0][4] == 8


@pytest.mark.parametrize("F,T", SHAPES)
def test_warp_identity_edges_and_general(ops, F, T):
    ns = _ns(T)
    x = _input(F, T, ns, seed=1)
    for c_of in (lambda n: 1, lambda n: n // 2, lambda n: n - 1):          # c == w: the input bits
        rows = [R.row(n, c_of(n), c_of(n)) for n in ns]
        _check_exact(_run(ops, x, rows), x, rows)
    edges = {"w = 0": lambda n: (max(n // 3, 1), 0), "c = n - 1": lambda n: (n - 1, n // 2), "c = 1, w = n - 1": lambda n: (1, n - 1)}
    for name, cw in edges.items():
        rows = [R.row(n, *cw(n)) for n in ns]
        _check_warp(_run(ops, x, rows), x, rows, name)
    rng = np.random.RandomState(T)
    for trial in range(4):
        rows = []
        for n in ns:
            c = int(rng.randint(1, n))
            rows.append(R.row(n, c, int(rng.randint(0, n))))
        _check_warp(_run(ops, x, rows), x, rows, "random %d" % trial)


@pytest.mark.parametrize("F,T", SHAPES)
def test_warp_and_masks_per_utterance(ops, F, T):
    ns = _ns(T)
    x = _input(F, T, ns, seed=2)
    rows = [R.row(ns[0], ns[0] // 2, ns[0] // 2 + 3, fmasks=[(0, 2), (F - 2, 2)], tmasks=[(3, 7)]),
            R.row(ns[1], 5, 2, fmasks=[(1, 1)], tmasks=[(0, 2), (ns[1] - 3, 3), (9, 0)]),
            R.row(ns[2], 1, 0, tmasks=[(1, 1)])]
    y = _run(ops, x, rows)
    _check_warp(y, x, rows, "warp + masks")
    ref = R.spec_augment_batch(x[:, 0], rows)
    assert not y[:, 0][ref == 0].any() and not np.signbit(y[:, 0][ref == 0]).any()
    assert y[0, 0, 2:F - 2, 10:].any()


def test_strided_input_and_long_utterance(ops):
    """A [..., :T] cut of a wider tensor is read in place through its row stride; above 16384 frames the warp's integers are 64-bit."""
    wide = _input(5, 70, [70, 64, 40], seed=3)
    rows = [R.row(64, 30, 35, tmasks=[(60, 4)]), R.row(64, 10, 4), R.row(40, 20, 39, fmasks=[(4, 1)])]
    xw = torch.from_numpy(wide).cuda()
    y = ops.spec_augment(xw[..., :64], torch.tensor(rows, dtype=torch.int32)).cpu().numpy()
    cut = np.ascontiguousarray(wide[..., :64])
    _check_warp(y, cut, rows, "strided")
    assert np.array_equal(y, _run(ops, cut, rows))
    n = 20000
    x = _input(5, n + 4, [n, n - 1, 16385], seed=4)
    rows = [R.row(n, n - 2, 1), R.row(n - 1, 9000, 9080, tmasks=[(100, 50)]), R.row(16385, 16384, 16000)]
    _check_warp(_run(ops, x, rows), x, rows, "long")


def test_binding_refuses_bad_rows(ops):
    x = torch.zeros(1, 1, 5, 16).cuda()
    for bad in (R.row(17), R.row(-1), [16, 0, 0, 9] + [0] * 36, [16, 0, 0, 0, 9] + [0] * 35):
        with pytest.raises(ValueError):
            ops.spec_augment(x, torch.tensor([bad], dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.spec_augment(x, torch.zeros(1, 39, dtype=torch.int32))


def _finish(ops, F, lens, Tmax, hop=160, seed=0):
    """The two launchers on the same random (re, im) rows: separate() -> (spect, statistics), fused() -> (out, raw, statistics), the
    statistics being the (sums, sqdev) that launch accumulated."""
    from asr_hip import lib as L
    B = len(lens)
    ld = (2 * F + 3) // 4 * 4
    reim = torch.from_numpy(np.random.RandomState(seed).randn(B * Tmax, ld).astype(np.float32) * 3).cuda()
    lengths = torch.tensor(lens, dtype=torch.int32).cuda()

    def separate():
        spect = torch.empty((B, 1, F, Tmax), device="cuda")
        sc = torch.zeros((2, B), device="cuda")
        L.call("asr_spect_finish", L.ptr(reim), ld, L.ptr(lengths), L.ptr(spect), L.ptr(sc[0]), L.ptr(sc[1]), B, F, Tmax, hop, 1, L.stream())
        return spect, sc.cpu()

    def fused(rows, T_out):
        raw = torch.empty((B, 1, F, Tmax), device="cuda")
        sc = torch.zeros((2, B), device="cuda")
        out = torch.full((B, 1, F, T_out), float("nan"), device="cuda")
        prm = torch.tensor(rows, dtype=torch.int32).cuda()
        L.call("asr_spect_finish_aug", L.ptr(reim), ld, L.ptr(lengths), L.ptr(raw), L.ptr(sc[0]), L.ptr(sc[1]), L.ptr(out), L.ptr(prm), B,
               F, Tmax, T_out, hop, L.stream())
        return out, raw, sc.cpu()
    return separate, fused


def _normalised(raw, sums, sqdev, nfr, F):
    """What the launch that produced (raw, sums, sqdev) normalises to, restated in float32 numpy with the kernel's expressions:
    mean = sums / (nfr F), rstd = rsqrt(sqdev / (nfr F - 1)), (raw - mean) * rstd.  The divisions and the subtraction are correctly
    rounded on both sides; rstd here is the correctly rounded value, the device's rsqrtf is within 1 ulp of it (NORM_SLACK)."""
    raw, sums, sqdev = (np.asarray(t.cpu(), dtype=np.float32) for t in (raw, sums, sqdev))
    x = np.zeros_like(raw)
    for b, n in enumerate(nfr):
        n_all = np.float32(n) * np.float32(F)
        mean = sums[b] / n_all
        rstd = np.float32(1.0 / np.sqrt(np.float64(sqdev[b] / (n_all - np.float32(1)))))
        x[b] = (raw[b] - mean) * rstd
    return x


# the device's rstd differs from _normalised's by at most 2^-23 (rsqrtf: 1 ulp) + 2^-24 (the rounding of the restated one) relatively,
# and each side rounds its product once more (2^-25 each): a normalised value differs by at most 4 * 2^-24 |x|, and so does any convex
# combination of two (the warp), on top of the warp's own 5 * 2^-24 max|x|
NORM_SLACK = 4


def _check_own_statistics(out, raw, sc, rows, nfr, F, what):
    """The fused launch against the float64 reference of the values ITS OWN statistics normalise to: the issue's warp bound plus
    NORM_SLACK; zeros of the reference (masks, frames from n on) are +0.0 exactly."""
    T_out = out.shape[-1]
    x = _normalised(raw, sc[0], sc[1], nfr, F)[..., :T_out]
    y = out.cpu().numpy()
    _check_warp(y, x, rows, what, slack=NORM_SLACK)
    ref = R.spec_augment_batch(x[:, 0], rows)
    assert not y[:, 0][ref == 0].any() and not np.signbit(y[:, 0][ref == 0]).any(), what


def _equal_where_statistics_agree(a, sa, b, sb, what):
    """a == b bit for bit for every utterance whose two launches accumulated bit-identical statistics; returns how many did."""
    same = 0
    for i in range(a.shape[0]):
        if torch.equal(sa[:, i], sb[:, i]):
            assert torch.equal(a[i], b[i]), (what, i)
            same += 1
        else:
            print("%s: utterance %d: the launches' statistics differ (sums %r / %r): max |a - b| %.3g" % (
                what, i, float(sa[0, i]), float(sb[0, i]), float((a[i].double() - b[i].double()).abs().max())))
    return same


@pytest.mark.parametrize("F", [2, 5, 161])
def test_fused_launcher_against_its_own_statistics_and_the_separate_passes(ops, F):
    """asr_spect_finish_aug normalises with the expressions of spect_normalize_kernel, so it is asr_spec_augment of
    asr_spect_finish(normalize = 1)[..., :T_out] bit for bit GIVEN THE SAME (sums, sqdev).  Those are accumulated with one float
    atomic per workgroup, F per utterance here, in an order that varies from launch to launch (measured at F = 161: sums 16445.0586
    against 16445.0527, outputs then 1.43e-06 apart), so two launches cannot always be compared bit for bit.  Hence two checks:
      * every launch against the float64 reference of what its OWN raw values and statistics normalise to (_normalised), within the
        warp bound plus NORM_SLACK -- independent of the atomics' order, all F, the 16-byte-store and the scalar-store kernel;
      * torch.equal against the separate passes: unconditional at F = 2 (a sum of two terms has no order), and at F = 5 and 161 for
        every utterance whose two launches accumulated the same statistics."""
    hop, Tmax, T_out = 160, 70, 64
    lens = [69 * hop + 3, 39 * hop, 0]                                    # 70, 40 and 1 frames
    nfr = [70, 40, 1]
    separate, fused = _finish(ops, F, lens, Tmax)
    spect, s_sep = separate()
    cases = {"warp + masks": ([R.row(64, 20, 31, fmasks=[(1, 1)], tmasks=[(50, 9)]), R.row(40, 30, 12, tmasks=[(0, 3), (38, 2)]),
                               R.row(1, fmasks=[(0, 1)])], T_out),
             "identity, cut": ([R.row(min(n, T_out)) for n in nfr], T_out),           # asr_spect_finish and the cut
             "identity": ([R.row(n) for n in nfr], Tmax),                             # asr_spect_finish itself
             "T_out 61": ([R.row(61, 20, 31, fmasks=[(1, 1)], tmasks=[(50, 9)]), R.row(40, 30, 12), R.row(1)], 61)}   # scalar stores
    same = 0
    for what, (rows, t_out) in cases.items():
        out, raw, sc = fused(rows, t_out)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and out[0].abs().max() > 0
        _check_own_statistics(out, raw, sc, rows, nfr, F, "%s, F %d" % (what, F))
        if what.startswith("identity"):
            sep = spect[..., :t_out]
        else:
            sep = ops.spec_augment(spect[..., :t_out], torch.tensor(rows, dtype=torch.int32))
        same += _equal_where_statistics_agree(out, sc, sep, s_sep, what)
    print("F %d: %d of 12 comparisons had bit-identical statistics" % (F, same))
    assert F > 2 or same == 12


# ------------------------------------------------------------------------------------------------ loader, front end, trainer
def _corpus(tmp_path, n=6, step=2500):
    rng = np.random.RandomState(0)
    words = ["ab", "ba", "abba", "bab", "aab", "bba"]
    lines = []
    for i in range(n):
        w = tmp_path / ("u%d.wav" % i)
        with wave.open(str(w), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
            f.writeframes((rng.randn(6000 + step * i) * 2000).astype("<i2").tobytes())
        t = tmp_path / ("u%d.txt" % i)
        t.write_text(words[i % len(words)] + "\n")
        lines.append("%s,%s" % (w, t))
    man = tmp_path / "train.csv"
    man.write_text("\n".join(lines))
    lab = tmp_path / "labels.json"
    lab.write_text(json.dumps([" ", "a", "b"]))
    return str(man), str(lab)


CONF = dict(sample_rate=16000, window_size=.02, window_stride=.01, window="hamming", noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))
TINY = ["--cuda", "--batch-size", "3", "--num-workers", "0", "--num-layers", "1", "--num-heads", "2", "--dim-model", "32", "--dim-key",
        "16", "--dim-value", "16", "--dim-inner", "64", "--dim-emb", "32", "--tgt-max-len", "12", "--src-max-len", "64",
        "--label-smoothing", "0.1", "--dropout", "0.0", "--k-lr", "20", "--warmup", "5", "--gpu-frontend", "--graph-buckets", "64",
        "--spec-time-warp", "5", "--spec-time-mask", "10", "--spec-freq-mask", "20"]


def _loader(args, man, l2i, which="train"):
    import train
    from utils.data_loader import AudioDataLoader, BucketingSampler
    args.train_manifest_list, args.valid_manifest_list = [man], [man]
    tr, valid = train.build_datasets(args, CONF, l2i)
    ds = tr if which == "train" else valid[0]
    np.random.seed(21)
    random.seed(21)
    return AudioDataLoader(ds, num_workers=0, batch_sampler=BucketingSampler(ds, batch_size=3))


def test_front_end_with_loader_rows(ops, tmp_path, monkeypatch):
    """gpu_front_end with the rows the loader drew, against the float64 reference of its un-augmented features.  Two runs of the front
    end do not normalise with the same bits (the statistics' atomics; measured 7.55 * 2^-24 * max|x| between two runs), so the
    un-augmented features are those of the SAME launch: ops.log_spectrogram hands back the raw log-magnitudes and the statistics it
    normalised with (stats=), and _normalised restates the normalisation.  Bound: the warp's plus NORM_SLACK; masks +0.0 exactly."""
    from utils import constant
    from utils.audio import gpu_front_end
    man, lab = _corpus(tmp_path)                                           # 38 .. 116 frames, cut to 64
    old = constant.args
    taken = {}
    real = ops.log_spectrogram
    monkeypatch.setattr(ops, "log_spectrogram", lambda *a, **k: real(*a, **dict(k, stats=taken) if k.get("spec") is not None else k))
    try:
        args = constant.parse(TINY + ["--spec-augment"])
        batches = list(_loader(args, man, {"a": 3, "b": 4}))
        assert len(batches) == 2
        for b in batches:
            assert len(b) == 7 and b[5] is None
            rows = b[6]
            plain, nf0 = gpu_front_end(b[0].cuda(), b[3], src_max_len=64)
            taken.clear()
            got, nf = gpu_front_end(b[0].cuda(), b[3], src_max_len=64, spec=rows)
            assert got.shape == plain.shape and got.shape[-1] <= 64 and torch.equal(nf, nf0) and nf.tolist() == rows[:, 0].tolist()
            assert (rows[:, 1] > 0).all() and (rows[:, 3:5] == 2).all()
            nfr = [1 + max(int(v), 2) // 160 for v in b[3]]
            _check_own_statistics(got, taken["raw"], (taken["sums"], taken["sqdev"]), rows.tolist(), nfr, 161, "front end")
            bad = rows.clone()
            bad[1, 0] += 1
            with pytest.raises(ValueError, match="frame counts"):
                gpu_front_end(b[0].cuda(), b[3], src_max_len=64, spec=bad)
        assert max(b[6][:, 0].max().item() for b in batches) == 64
    finally:
        constant.set_args(old)


def test_trainer_step_and_replay_with_spec_augment(ops, tmp_path, monkeypatch):
    from trainer.asr.trainer import Trainer
    from utils import constant
    from utils.functions import init_optimizer, init_transformer_model
    import train
    man, lab = _corpus(tmp_path, step=800)                                 # 38 .. 63 frames: one 64-frame bucket
    l2i, i2l = train.build_labels(lab)
    old, old_cuda = constant.args, constant.USE_CUDA

    def steps(flag, batch):
        args = constant.parse(TINY + (["--spec-augment"] if flag else []))
        torch.manual_seed(7)
        model = init_transformer_model(args, l2i, i2l).cuda().train()
        opt = init_optimizer(args, model, "noam")
        tr = Trainer()
        losses = [tr._run_batch(model, batch, 0.1, "ce", i2l, opt).result()[0] for _ in range(2)]     # eager + capture, then a replay
        assert len(tr._graphs) == 1
        return losses, model

    try:
        args = constant.parse(TINY + ["--spec-augment"])
        b_on = next(iter(_loader(args, man, l2i)))
        vb = next(iter(_loader(args, man, l2i, "valid")))
        assert len(b_on) == 7 and len(vb) == 5
        on, model = steps(True, b_on)
        off, _ = steps(False, b_on[:5])
        print("losses with SpecAugment", on, "without", off)
        assert all(np.isfinite(v) for v in on + off)
        assert on[0] != off[0] and on[1] != off[1]
        # validation is untouched by the flag: the same 5-element batch goes into the front end, bit for bit and without rows, under
        # both settings.  Two front-end runs need not agree in the last bits (the statistics' atomics), and the bf16 model turns a
        # last-bit difference of a feature into 2^-9 ones (measured: losses 1.66765 / 1.66807 from two runs), so the front end runs
        # ONCE and both settings get its features: the results are then those of one model on one input.
        import trainer.asr.trainer as trainer_mod
        model.eval()
        res, seen, feats = [], [], []
        real = trainer_mod.gpu_front_end

        def spy(src, sizes, *a, **k):
            seen.append((src.detach().cpu().clone(), torch.as_tensor(sizes).clone(), a, {q: v for q, v in k.items() if q != "spec"}, k.get("spec")))
            if not feats:
                feats.append(real(src, sizes, *a, **k))
            return feats[0]
        monkeypatch.setattr(trainer_mod, "gpu_front_end", spy)
        for flag in (True, False):
            constant.parse(TINY + (["--spec-augment"] if flag else []))
            with torch.no_grad():
                res.append(Trainer()._run_batch(model, vb, 0.1, "ce", i2l, None))
        assert len(seen) == 2 and seen[0][4] is None and seen[1][4] is None
        assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1]) and seen[0][2:4] == seen[1][2:4]
        # equal text metrics; the loss is an fp32 sum over at most 32 target tokens, equal up to the order of that sum
        assert int(vb[4].sum()) <= 32
        assert res[0][1:] == res[1][1:] and np.isfinite(res[0][0]) and abs(res[0][0] - res[1][0]) <= 2 * 32 * 2.0 ** -24 * abs(res[0][0])
    finally:
        constant.set_args(old)
        constant.USE_CUDA = old_cuda
