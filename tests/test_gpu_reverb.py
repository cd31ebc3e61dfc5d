"""asr_reverb on the GPU (csrc/reverb.hip) against the restatement of DESIGN.md section 7 (tests/reverb_reference.py): bit for bit on
exact data inside a buffer of sentinels, within the fp32 sum's error bound on prepared taps, a lone impulse, batch invariance,
repeatability, the all-copied batch, the binding's refusals, the front end with 8-column draws, and train.py --rir-dir."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import reverb_reference as VR  # noqa: E402

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


def _bank(taps, aligned):
    """(RirBank, index of each response): aligned -- every response starts at a multiple of 4 floats (fillers between them make up
    the difference); otherwise every one starts at an odd offset."""
    from utils.audio import RirBank
    arrays, index, off = [], [], 0
    for h in taps:
        fill = (-off) % 4 if aligned else (off + 1) % 2
        if fill:
            arrays.append(np.full(fill, 99.0, np.float32))                     # never read: a tap from here would show
            off += fill
        index.append(len(arrays))
        arrays.append(h)
        off += h.size
    bank = RirBank.from_arrays(arrays, "cuda")
    offs = bank.offsets.cpu().numpy()[index]
    assert ((offs % 4 == 0) if aligned else (offs % 2 == 1)).all()
    return bank, index


def _run_in_sentinels(ops, xs, rir, bank, aligned):
    """The batch reverberated into the middle of a buffer of sentinels: a guard row before and after, a row stride beyond the columns,
    and more columns than samples.  aligned: 16-byte loads and stores possible (row strides multiples of 4) or not."""
    B = len(xs)
    Lmax = max(max(x.size for x in xs), 1)
    if aligned:
        Lmax = (Lmax + 3) // 4 * 4
        cols, stride = Lmax + 8, Lmax + 12
    else:
        Lmax |= 1
        cols = Lmax + 3
        stride = cols + 5 if (cols + 5) % 4 else cols + 6
    assert (stride % 4 == 0) == aligned and (Lmax % 4 == 0) == aligned
    buf = torch.full((B + 2, stride), SENTINEL, device="cuda")
    out = buf[1:B + 1, :cols]
    wav = _pad(xs, Lmax)
    for b, x in enumerate(xs):                                                  # what lies behind n in the input must not matter
        wav[b, x.size:] = 777.0
    got = ops.reverb(wav.cuda(), torch.tensor([x.size for x in xs]), torch.tensor(rir), bank, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu()
    assert (host[0] == SENTINEL).all() and (host[B + 1] == SENTINEL).all() and (host[1:B + 1, cols:] == SENTINEL).all()
    return host[1:B + 1, :cols]


def _check_rows(got, exp, what):
    for b, e in enumerate(exp):
        n = e.size
        assert torch.equal(got[b, :n], torch.from_numpy(e)), (what, b, n)
        assert not got[b, n:].numpy().view(np.int32).any(), (what, b, "columns from n on are +0.0")


def _exact_case(ops, rng, ns, Ls, copied, aligned, what):
    """Integer taps in [-8, 8] and samples in [-64, 64]: every partial sum stays below 2^24 for L < 32768, so any order is exact."""
    xs = [rng.randint(-64, 65, n).astype(np.float32) for n in ns]
    taps = [rng.randint(-8, 9, L).astype(np.float32) for L in Ls]
    bank, index = _bank(taps, aligned)
    rir = [-1 if b in copied else index[b] for b in range(len(ns))]
    got = _run_in_sentinels(ops, xs, rir, bank, aligned)
    exp = [x.copy() if b in copied else VR.reverb32_exact(x, taps[b], x.size) for b, x in enumerate(xs)]
    _check_rows(got, exp, what)


@pytest.mark.parametrize("aligned", [False, True])
def test_exact_data_bit_for_bit_inside_sentinels(ops, aligned):
    T, C = ops.REVERB_TILE, ops.REVERB_CHUNK
    ns = [0, 1, T - 1, T, T + 1, 2 * T + 3]
    Ls = [1, 2, C - 1, C, C + 1, 1000]
    assert C + 1 <= 1000
    rng = np.random.RandomState(1)
    # every (n, L) pair: row b has n = ns[b] and L = Ls[(b + rot) % 6]; row `rot` is copied instead, its pair comes in the last batch
    for rot in range(6):
        _exact_case(ops, rng, ns, [Ls[(b + rot) % 6] for b in range(6)], {rot}, aligned, "rotation %d" % rot)
    _exact_case(ops, rng, ns, [Ls[(2 * b) % 6] for b in range(6)], set(), aligned, "the pairs of the copied rows")
    # L > n with every n; two copied rows next to each other, first and last row
    _exact_case(ops, rng, [5, 700, T + 1, 0, 999], [6, 1000, 2 * T, 3, 1000], set(), aligned, "L > n")
    _exact_case(ops, rng, [T + 5, 3, 0, 2 * T + 3], [C, 1, 1, 2], {0, 3}, aligned, "copied first and last")


def test_a_response_longer_than_a_tile_and_its_span_is_exact_too(ops):
    """The staged span of one tap chunk is T + C samples, more than the 1000 taps of the cases above (there "longer than a span" can
    only mean more than one chunk); here L exceeds the span itself: the second tile reaches back beyond the first, and in the first
    tile the chunks whose taps all have k > m are skipped.  The data stay exact: L 8 64 < 2^24."""
    T, C = ops.REVERB_TILE, ops.REVERB_CHUNK
    rng = np.random.RandomState(2)
    _exact_case(ops, rng, [2 * T + 3, T + C + 9, T - 1], [T + C + 5, T + C + 5, 3 * C + 2], set(), False, "long response")


def test_a_batch_of_more_rows_than_a_workgroup_has_threads(ops):
    """Up to 256 rows the workgroups take the expensive tiles first; a larger batch is walked as it lies.  Both orders write every row."""
    T = ops.REVERB_TILE
    rng = np.random.RandomState(3)
    for B in (256, 300):
        ns = [(37 * i) % 50 for i in range(B - 2)] + [T + 3, 2 * T]
        _exact_case(ops, rng, ns, [1 + i % 5 for i in range(B)], set(range(0, B, 3)), True, "%d rows" % B)


@pytest.fixture(scope="module")
def real_batch(ops):
    """Gaussian rows and a lone unit impulse through prepared taps of a synthetic decaying-noise response of about 3000 taps, once:
    (xs, rir, taps, bank, out)."""
    from utils.audio import RirBank, prepare_rir
    rng = np.random.RandomState(7)
    raw = rng.randn(3000) * np.exp(-np.arange(3000) / 600.0)
    raw[0] = 6.0
    taps = [prepare_rir(np.concatenate([np.zeros(40), raw]), SR, 500), prepare_rir(raw[:900], SR, 50)]
    assert 2900 <= taps[0].size <= 3000 and 700 <= taps[1].size <= 800
    xs = [rng.randn(n).astype(np.float32) for n in (5000, 4099, 2500)] + [np.zeros(4000, np.float32)]
    xs[3][0] = 1.0
    rir = [0, 1, 0, 0]
    bank = RirBank.from_arrays(taps, "cuda")
    out = ops.reverb(_pad(xs).cuda(), torch.tensor([x.size for x in xs]), torch.tensor(rir), bank)
    torch.cuda.synchronize()
    return xs, rir, taps, bank, out.cpu()


def test_prepared_taps_within_the_fp32_sum_bound(ops, real_batch):
    """|y - y64| <= gamma_{L+1} sum_k |h_k| |x_{m-k}| + L 2^-126 elementwise, gamma_j = j u / (1 - j u), u = 2^-24: the standard bound of
    an fp32 FMA sum of L terms in any order, the right-hand side in float64 from the restatement."""
    xs, rir, taps, bank, out = real_batch
    assert out.shape == (4, 5000) and out.dtype == torch.float32
    for b, x in enumerate(xs):
        h = taps[rir[b]]
        y64, mag = VR.reverb64(x, h, x.size)
        err = np.abs(out[b, :x.size].numpy().astype(np.float64) - y64)
        bound = VR.bound(h.size, mag)
        print("row %d (L %d): max error %.3e, bound there %.3e" % (b, h.size, err.max(), bound[err.argmax()]))
        assert (err <= bound).all()
        assert not out[b, x.size:].numpy().view(np.int32).any()


def test_a_lone_unit_impulse_gives_the_taps_bit_for_bit(ops, real_batch):
    xs, rir, taps, bank, out = real_batch
    h = taps[0]
    assert torch.equal(out[3, :h.size], torch.from_numpy(h)) and not out[3, h.size:].numpy().view(np.int32).any()


def test_batch_invariance_and_repeatability(ops, real_batch):
    xs, rir, taps, bank, out = real_batch
    lens = [x.size for x in xs]
    again = ops.reverb(_pad(xs).cuda(), torch.tensor(lens), torch.tensor(rir), bank)
    assert torch.equal(again.cpu(), out)
    order = [2, 0, 3, 1]
    perm = ops.reverb(_pad([xs[i] for i in order], 5000).cuda(), torch.tensor([lens[i] for i in order]),
                      torch.tensor([rir[i] for i in order]), bank).cpu()
    for row, i in enumerate(order):
        assert torch.equal(perm[row], out[i]), i
    for b in range(4):                                                          # alone: another width, another tile count
        alone = ops.reverb(torch.from_numpy(xs[b])[None].cuda(), torch.tensor([lens[b]]), torch.tensor([rir[b]]), bank).cpu()
        assert alone.shape == (1, lens[b]) and torch.equal(alone[0], out[b, :lens[b]])


def test_all_copied_returns_the_input_and_launches_nothing(ops, monkeypatch):
    from utils.audio import RirBank
    wav = torch.randn(3, 100).cuda()
    bank = RirBank.from_arrays([np.ones(4, np.float32)], "cuda")

    def no_launch(*a, **k):
        raise AssertionError("a batch without a response must not launch")
    monkeypatch.setattr(ops.L, "call", no_launch)
    assert ops.reverb(wav, torch.tensor([100, 7, 0]), torch.tensor([-1, -1, -1]), bank) is wav
    assert ops.reverb(wav, [100, 7, 0], [-1, -1, -1], None) is wav


def test_copied_rows_and_an_empty_row_inside_a_mixed_batch(ops):
    from utils.audio import RirBank
    rng = np.random.RandomState(9)
    xs = [rng.randn(n).astype(np.float32) for n in (2500, 1029, 0, 3)]
    bank = RirBank.from_arrays([np.array([0.5, 0.25], np.float32)], "cuda")
    out = ops.reverb(_pad(xs).cuda(), torch.tensor([2500, 1029, 0, 3]), torch.tensor([-1, 0, 0, -1]), bank).cpu()
    assert out.shape == (4, 2500) and torch.equal(out[0], torch.from_numpy(xs[0]))
    assert torch.equal(out[3, :3], torch.from_numpy(xs[3])) and not out[3, 3:].numpy().view(np.int32).any()
    assert not out[2].numpy().view(np.int32).any()                               # n = 0: all +0.0
    x = xs[1]
    exp = np.float32(0.5) * x + np.float32(0.25) * np.concatenate([[np.float32(0)], x[:-1]])      # both products exact, one rounding
    assert torch.equal(out[1, :1029], torch.from_numpy(exp.astype(np.float32))) and not out[1, 1029:].any()


def test_binding_refusals(ops, monkeypatch):
    from asr_hip import lib as L
    from utils.audio import RirBank
    wav = torch.zeros(2, 64).cuda()
    bank = RirBank.from_arrays([np.ones(3, np.float32), np.ones(5, np.float32)], "cuda")
    ops.reverb(wav, [64, 0], [1, -1], bank)
    launched = []
    real = ops.L.call
    monkeypatch.setattr(ops.L, "call", lambda *a: launched.append(a[0]) or real(*a))
    for lens in ([65, 64], [64, -1]):
        with pytest.raises(ValueError, match="lengths"):
            ops.reverb(wav, lens, [0, 0], bank)
    for rir in ([0, 2], [-2, 0], [5, -1]):
        with pytest.raises(ValueError, match="RIR indices"):
            ops.reverb(wav, [64, 64], rir, bank)
    with pytest.raises(ValueError, match="RIR indices"):
        ops.reverb(wav, [64, 64], [0, -1], None)
    with pytest.raises(ValueError, match="fp32"):
        ops.reverb(wav.double(), [64, 64], [0, 0], bank)
    with pytest.raises(ValueError, match="contiguous"):
        ops.reverb(torch.zeros(2, 128).cuda()[:, ::2], [64, 64], [0, 0], bank)
    with pytest.raises(ValueError, match="contiguous"):
        ops.reverb(torch.zeros(2, 128).cuda()[:, :64], [64, 64], [0, 0], bank)
    with pytest.raises(ValueError, match="bank lives on"):
        ops.reverb(wav, [64, 64], [0, 0], RirBank.from_arrays([np.ones(3, np.float32)], "cpu"))
    with pytest.raises(ValueError, match="out must be"):
        ops.reverb(wav, [64, 64], [0, 0], bank, out=torch.zeros(2, 60).cuda())
    with pytest.raises(ValueError, match="another buffer"):
        ops.reverb(wav, [64, 64], [0, 0], bank, out=wav)
    assert not launched                                                          # every refusal came before any launch
    monkeypatch.setattr(ops.L, "call", real)
    # the entry point itself refuses bad geometry (out_stride < out_cols, negative counts) and clamps bad device data: an index outside
    # the bank, taps that leave it and a length beyond the row are written as zeros or cut, never read
    out = torch.full((3, 64), SENTINEL).cuda()
    wav3 = torch.ones(3, 64).cuda()
    lens = torch.tensor([64, 64, 64], dtype=torch.int32).cuda()
    rir = torch.tensor([0, 1, 0], dtype=torch.int32).cuda()
    args = [L.ptr(wav3), 64, L.ptr(lens), L.ptr(rir), L.ptr(bank.data), 8, L.ptr(bank.offsets), L.ptr(bank.lens), 2, L.ptr(out)]
    for tail in ((63, 64, 3), (64, -1, 3), (64, 64, -1)):
        with pytest.raises(L.AsrHipError):
            L.call("asr_reverb", *args, *tail, L.stream())
    L.call("asr_reverb", *args, 64, 64, 0, L.stream())                          # B = 0: nothing to do
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    bad_rir = torch.tensor([2, -7, 1], dtype=torch.int32).cuda()               # outside the bank twice; the third is fine
    args[3] = L.ptr(bad_rir)
    L.call("asr_reverb", *args, 64, 64, 3, L.stream())
    host = out.cpu()
    assert not host[:2].numpy().view(np.int32).any() and host[2].tolist() == [1.0, 2.0, 3.0, 4.0] + [5.0] * 60
    args[3], args[5] = L.ptr(rir), 7                                            # the bank ends inside the second response
    out.fill_(SENTINEL)
    L.call("asr_reverb", *args, 64, 64, 3, L.stream())
    host = out.cpu()
    assert not host[1].numpy().view(np.int32).any() and host[0].tolist() == [1.0, 2.0] + [3.0] * 62 and torch.equal(host[2], host[0])


# ------------------------------------------------------------------------------------------------ front end
@pytest.mark.parametrize("case", ["plain", "speed", "speed tempo gain noise spec", "fbank"])
def test_front_end_with_eight_columns_is_the_front_end_on_the_reverberated_batch(ops, tmp_path, monkeypatch, case):
    """gpu_front_end with 8-column draws against gpu_front_end with the corresponding draws on waveforms that ops.resample and ops.reverb
    processed first, with and without a speed column.  What enters asr_augment_wave and the STFT is compared with torch.equal, and so
    are the frame counts.  The features themselves come out of the same kernels on the same bits, but the existing normalisation adds
    its statistics with float atomics, so two launches of the SAME front end already differ in the last bits:
    torch.equal on them cannot hold for any correct wiring.  As tests/test_gpu_resample.py does, they are compared within the derived
    reordering bound of those sums (its _front_end_bound), and the largest difference is printed."""
    import specaug_reference as SA
    import test_augment_host as H
    import test_reverb_host as RH
    from test_gpu_resample import _front_end_bound, _spy
    from utils.audio import _device_mel_bank, gpu_front_end, rir_bank, spec_frames, speed_length, tempo_length
    rng = np.random.RandomState(12)
    full = case == "speed tempo gain noise spec"
    ns = [9000, 8000, 7001, 6000]
    ps = [900, 1000, 1100, 997] if case in ("speed", "speed tempo gain noise spec") else [0, 0, 0, 0]
    rirs = [1, -1, 0, 2]
    xs = [(rng.randn(n) * 0.1).astype(np.float32) for n in ns]
    mids = [speed_length(n, p) if p else n for n, p in zip(ns, ps)]
    tempos, gains = ([1.1, 0.0, 0.9, 1.0], [3.0, 0.0, -2.5, 0.0]) if full else ([0.0] * 4, [0.0] * 4)
    clips, starts, levels = ([1, -1, 0, -1], [0.05, 0.0, 0.2, 0.0], [0.3, 0.0, 0.1, 0.0]) if full else ([-1] * 4, [0.0] * 4, [0.0] * 4)
    nd = str(H.noise_dir(tmp_path)) if full else None
    rd = str(RH.rir_dir(tmp_path))
    finals = [tempo_length(m, t) if t > 0 else m for m, t in zip(mids, tempos)]
    kw = dict(noise_dir=nd, src_max_len=60 if full else None)
    kind = {}
    if case == "fbank":
        kw.update(features="fbank", num_mel_bins=40)
        kind = dict(features="fbank", mel=_device_mel_bank(40, 320, SR, 20.0, torch.device("cuda", 0)))
    if full:
        kw["spec"] = torch.tensor([SA.row(spec_frames(n, 160, 60), 20, 25, fmasks=[(3, 9)], tmasks=[(5, 6)]) for n in finals], dtype=torch.int32)
    eight = torch.tensor([(n, t, g, c, s, l, p, r) for n, t, g, c, s, l, p, r in zip(ns, tempos, gains, clips, starts, levels, ps, rirs)],
                         dtype=torch.float64)
    six = torch.tensor([(m, t, g, c, s, l) for m, t, g, c, s, l in zip(mids, tempos, gains, clips, starts, levels)], dtype=torch.float64)
    wav = _pad(xs).cuda()
    bank = rir_bank(rd, SR, 30, wav.device)
    assert len(bank) == 3 and int(bank.lens.max()) <= 480
    pre, pre_lens = ops.resample(wav, torch.tensor(ns), torch.tensor(ps))
    assert pre_lens.tolist() == mids
    pre = ops.reverb(pre, torch.tensor(mids), torch.tensor(rirs), bank)
    assert pre.shape == (4, max(mids)) and torch.equal(pre[1, :mids[1]].cpu(), torch.from_numpy(xs[1]))
    seen_aug, seen_stft = _spy(monkeypatch, ops, "augment_wave"), _spy(monkeypatch, ops, "log_spectrogram")
    sizes = torch.tensor(finals, dtype=torch.int32)
    a, na = gpu_front_end(wav[:, None, None, :], sizes, aug=eight, rir_dir=rd, rir_max_ms=30, **kw)
    b, nb = gpu_front_end(pre[:, None, None, :].clone(), sizes, aug=six, **kw)
    assert len(seen_aug) == 2 and len(seen_stft) == 2
    (w8, l8, p8, bank8), (w6, l6, p6, bank6) = seen_aug[0][0][:4], seen_aug[1][0][:4]
    assert torch.equal(w8, w6) and torch.equal(w8, pre) and torch.equal(l8, l6) and torch.equal(p8, p6) and bank8 is bank6
    (s8, sl8), (s6, sl6) = seen_stft[0][0][:2], seen_stft[1][0][:2]
    assert torch.equal(s8, s6) and torch.equal(sl8, sl6) and sl8.tolist() == finals
    assert torch.equal(na, nb) and a.shape == b.shape and na.tolist() == [spec_frames(n, 160, kw["src_max_len"]) for n in finals]
    tol = _front_end_bound(ops, s8, sl8, a, na, kind)
    for u in range(4):
        d = (a[u] - b[u]).abs().max().item()
        print("%s utterance %d: max |difference| of two launches %.3e, bound %.3e" % (case, u, d, tol[u]))
        assert d <= tol[u]
    # the reverberation is really there: the reverberated rows differ from a front end that leaves the response out
    dry = eight.clone()
    dry[:, 7] = -1
    c, _ = gpu_front_end(wav[:, None, None, :], sizes, aug=dry, rir_dir=rd, rir_max_ms=30, **kw)
    assert (a[0] - c[0]).abs().max().item() > 1e-2 and (a[1] - c[1]).abs().max().item() <= tol[1]
    with pytest.raises(ValueError, match="rir_dir"):
        gpu_front_end(wav[:, None, None, :], sizes, aug=eight, **kw)


# ------------------------------------------------------------------------------------------------ train.py
@pytest.mark.parametrize("buckets", ["0", "64"])
def test_train_with_reverberation(tmp_path, monkeypatch, capsys, buckets):
    import test_gpu_train_cli as C
    import test_reverb_host as RH
    import trainer.asr.trainer as trainer_mod
    from asr_hip import ops
    from utils import constant
    man, lab = C._corpus(tmp_path)
    rd = str(RH.rir_dir(tmp_path))
    monkeypatch.chdir(tmp_path)
    argv = ["--train-manifest-list", man, "--valid-manifest-list", man, "--test-manifest-list", man, "--labels-path", lab,
            "--cuda", "--batch-size", "3", "--num-workers", "0", "--epochs", "2", "--save-every", "1", "--name", "tinyrir",
            "--save-folder", str(tmp_path / "save"), "--num-layers", "1", "--num-heads", "2", "--dim-model", "32", "--dim-key",
            "16", "--dim-value", "16", "--dim-inner", "64", "--dim-emb", "32", "--tgt-max-len", "12", "--src-max-len", "64",
            "--label-smoothing", "0.1", "--dropout", "0.1", "--k-lr", "20", "--warmup", "5", "--clip",
            "--rir-dir", rd, "--rir-prob", "1.0", "--rir-max-ms", "30", "--graph-buckets", buckets]
    seen, reverbs = [], []
    real, real_reverb = trainer_mod.gpu_front_end, ops.reverb

    def spy(src, sizes, *a, **k):
        seen.append((torch.as_tensor(sizes).tolist(), None if k.get("aug") is None else k["aug"].clone()))
        return real(src, sizes, *a, **k)

    def spy_reverb(wav, lens, rir, bank, out=None):
        got = real_reverb(wav, lens, rir, bank, out=out)
        reverbs.append((torch.as_tensor(rir).tolist(), len(bank), not torch.equal(got, wav), bool(torch.isfinite(got).all())))
        return got
    monkeypatch.setattr(trainer_mod, "gpu_front_end", spy)
    monkeypatch.setattr(ops, "reverb", spy_reverb)
    old, old_cuda = constant.args, constant.USE_CUDA
    try:
        constant.parse(argv)
        np.random.seed(2)
        random.seed(2)
        import train as train_mod
        train_mod.main()
        assert constant.args.gpu_frontend and "--gpu-frontend turned on" in capsys.readouterr().out
        assert constant.args.graph_buckets == int(buckets)
        last = torch.load(str(tmp_path / "save" / "tinyrir" / "epoch_2.th"), map_location="cpu", weights_only=False)
        best = torch.load(str(tmp_path / "save" / "tinyrir" / "best_model.th"), map_location="cpu", weights_only=False)
        hist = last["metrics"]["history"]
        assert len(hist) == 2 and all(np.isfinite(h["train_loss"]) and np.isfinite(h["valid_loss"]) for h in hist)
        assert last["optimizer_params"]["_step"] >= 4                           # two epochs of two steps, none skipped
        # the best checkpoint is the epoch with the lowest validation loss: what is kept never gets worse
        assert best["metrics"]["valid_loss"] == min(h["valid_loss"] for h in hist) <= hist[0]["valid_loss"]
    finally:
        constant.set_args(old)
        constant.USE_CUDA = old_cuda
    raw = {4000 + 800 * i for i in range(6)}
    train = [(s, a) for s, a in seen if a is not None]
    valid = [s for s, a in seen if a is None]
    assert len(train) == 4 and valid and all(set(s) <= raw for s in valid)       # validation batches carry no draws: never reverberated
    assert len(reverbs) == 4                                                      # one launch per training batch, none for validation
    for (sizes, aug), (rir, count, changed, finite) in zip(train, reverbs):
        assert aug.shape == (3, 8) and set(aug[:, 0].long().tolist()) <= raw and not aug[:, 6].any()
        assert sizes == aug[:, 0].long().tolist() == sorted(sizes, reverse=True)  # the length does not change
        assert rir == aug[:, 7].long().tolist() and all(0 <= r < 3 for r in rir) and count == 3 and changed and finite
