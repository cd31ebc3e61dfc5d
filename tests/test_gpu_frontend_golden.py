"""The GPU audio front end (csrc/spectrogram.hip, spec_augment.hip, resample.hip, reverb.hip, augment.hip) bit for bit against
tests/golden/frontend.npz, which tools/gen_frontend_golden.py recorded on an MI355X with the library of the commit before csrc/wave_rows.h
and features_finish existed.  The other tests hold these kernels against float64 restatements; a refactor of what they share (the row
copy, the guarded staging load, the 64-lane scan, the frame count, the finish pipeline) has to leave the same BITS.

Inputs are seeded on the CPU (Gaussian samples, taps and tables: any change in the order of a sum shows); only outputs are stored.
  spect_raw / fbank_raw   log_spectrogram(normalize=False), n_fft 64, hop 32 (33 bins), B 4, lengths (0, 1, 20, 8320): 20 <= n_fft / 2 takes
                the zero-padding arm of stft_frames_kernel; Tmax 261 = two 256-frame blocks per row, four whole 64-frame fbank tiles, a
                partial one, and whole tiles past the short utterances' ends.  fbank: 8 overlapping filters.
  fbank_raw_strided       fbank_finish(normalize=False) of random (re, im) rows 12 floats wider than 2 K rounded up.
  specaug_64 / _63 / _strided   spec_augment on (3, 9, 64) (16-byte stores), (2, 9, 63) (scalar stores) and the [..., :64] cut of a
                (3, 1, 5, 70) tensor: warps with c != w and c == w, masks on both axes, a row with n < T, NaN from frame n on.
  resample      exact tables injected (tables=), B 4, L 2500: identity, 900, 1100 and a row of length 0; the 900 row has 2667 outputs (three
                tiles).  compute() runs it into a fresh buffer (2667 columns: scalar stores), into a caller's 2668 columns on a 16-byte base
                (vec_out on), into an out whose row stride is no multiple of 4 and from a wav view one float off 16 bytes (vec_in off), and
                requires the four to agree bit for bit before it returns the first.
  resample_long 900 with R 1200: a tile's span exceeds the kernel's LDS image, the samples are read from memory.
  reverb_a / _b B 5, lengths (2500, 1029, 0, 3, 2048), responses of (1, 2, 3, 515, 1025) taps, assigned two ways (the second with a copied
                row) so that every tail of 1, 2 and 3 taps and three 512-tap chunks are walked; into a fresh buffer and, with the same bits
                required, into a wider out (2507 columns: scalar stores).
  reverb_257    257 rows of 64 samples: more rows than a workgroup has threads, walked as they lie.
  augment       augment_wave(offsets=True): white / chirp / am under a tempo, a row with gain alone, a row with noise alone and one with tempo,
                gain and noise, the noise from a two-clip bank held in memory.
Float outputs are compared as int32 views with torch.equal: 0 and -0 patterns count.

The normalised and the fused forms add their statistics with float atomics in an order that varies between launches; nothing is recorded
for them.  test_normalised_and_fused_forms_against_their_own_statistics takes each launch's own `stats` and requires: raw = the golden
bits; sums within (n - 1) 2^-24 sum |raw| of the float64 sum of the golden raw (the worst case of an fp32 sum of n terms in any order);
sqdev within gamma_{n+2} sum d^2 + n 2^-149 of the float64 sum of d^2, d = raw - mean with the launch's own fp32 mean (one rounding in d,
counted twice in its square, one in the product, n - 1 in the sum; gamma_k = k u / (1 - k u), u = 2^-24; 2^-149 a term for underflow);
the output = the separate passes with those statistics, bit for bit: (raw - mean) * rstd with mean = sums / n and rstd = rsqrt(sqdev /
(n - 1)), then the cut to max_frames and ops.spec_augment.  The divisions and the two roundings of the normalisation are IEEE on either
side; the device's rsqrtf (v_rsq_f32, 1 ulp) is the one operation the host cannot restate, so an utterance has to match, in every bit of
every element, under one of the three values within 1 ulp of the correctly rounded rstd (measured: torch.rsqrt on the device is another
function and differs from rsqrtf by 1 ulp on some arguments)."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import resample_reference as RR
import specaug_reference as SR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend.npz")
N_FFT, HOP, BINS, MEL = 64, 32, 33, 8
FEAT_LENS = (0, 1, 20, 8320)
TMAX = 261
FBANK_TILE = 64                               # kFbankTile of csrc/spectrogram.hip, kernel-local: a change there has to be repeated here
RESAMPLE_LDS = 2304                           # kLds of csrc/resample.hip, likewise (both definitions point back to this file)
SAMPLE_RATE = 16000
NAMES = ["spect_raw", "fbank_raw", "fbank_raw_strided", "specaug_64", "specaug_63", "specaug_strided", "resample", "resample_long",
         "reverb_a", "reverb_b", "reverb_257", "augment"]


def _ops():
    from asr_hip import ops
    torch.cuda.set_device(0)
    return ops


def _frames(n):
    return 1 + max(n, 2) // HOP


# ------------------------------------------------------------------------------------------------ features
@functools.lru_cache(maxsize=None)
def _waves():
    rng = np.random.RandomState(11)
    L = max(FEAT_LENS)
    wav = (rng.randn(len(FEAT_LENS), L) * 0.1).astype(np.float32)
    for b, n in enumerate(FEAT_LENS):
        wav[b, n:] = 0
    assert _frames(L) == TMAX and TMAX > 256 and TMAX % FBANK_TILE and sorted(FEAT_LENS)[2] <= N_FFT // 2 and min(FEAT_LENS) == 0
    assert _frames(sorted(FEAT_LENS)[2]) <= FBANK_TILE < TMAX                   # a whole fbank tile past a short utterance's end
    return torch.from_numpy(wav), torch.tensor(FEAT_LENS, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _mel():
    from utils.audio import MelBank
    first, count = np.array([0, 2, 5, 8, 12, 16, 21, 26], dtype=np.int32), np.array([4, 5, 6, 7, 8, 9, 10, 7], dtype=np.int32)
    assert first.size == MEL and int((first + count).max()) == BINS
    w = np.random.RandomState(12).uniform(0.05, 1.0, int(count.sum())).astype(np.float32)
    return MelBank(first, count, w, BINS)


@functools.lru_cache(maxsize=None)
def _reim():
    """(B * Tmax, ld + 12) random (re, im) rows for fbank_finish; the kernel reads the first 2 K columns of each."""
    ld = (2 * BINS + 3) // 4 * 4 + 12
    return torch.from_numpy((np.random.RandomState(13).randn(len(FEAT_LENS) * TMAX, ld) * 3).astype(np.float32))


def _features(kind, **kw):
    """(features, n_frames) of the front end of `kind` on the feature batch."""
    ops = _ops()
    wav, lens = _waves()
    if kind == "fbank_strided":
        reim = _reim().cuda()[:, :2 * BINS + 2]
        assert reim.stride(0) > reim.shape[1] >= 2 * BINS
        return ops.fbank_finish(reim, lens.cuda(), _mel(), HOP, **kw)
    mel = dict(features="fbank", mel=_mel()) if kind == "fbank" else {}
    return ops.log_spectrogram(wav.cuda(), lens.cuda(), n_fft=N_FFT, hop=HOP, **mel, **kw)


def _feat_raw(kind):
    feat, nf = _features(kind, normalize=False)
    assert feat.shape == (len(FEAT_LENS), 1, MEL if kind.startswith("fbank") else BINS, TMAX)
    assert nf.tolist() == [_frames(n) for n in FEAT_LENS]
    return {"feat": feat, "n_frames": nf}


# ------------------------------------------------------------------------------------------------ SpecAugment
def _spec_input(B, F, T, ns, seed):
    x = (np.random.RandomState(seed).randn(B, 1, F, T) * 1.5).astype(np.float32)
    for b, n in enumerate(ns):
        x[b, ..., n:] = np.nan                                                 # nothing from frame n on may reach the output
    return x


def _specaug(which):
    ops = _ops()
    if which == "64":
        rows = [SR.row(64, 20, 31, fmasks=[(1, 2)], tmasks=[(50, 9)]), SR.row(64, 30, 30, fmasks=[(7, 1), (0, 1)], tmasks=[(3, 4)]),
                SR.row(40, 30, 12, fmasks=[(4, 0)], tmasks=[(0, 3), (38, 2)])]
        x = torch.from_numpy(_spec_input(3, 9, 64, [r[0] for r in rows], 21)).cuda()
    elif which == "63":
        rows = [SR.row(63, 20, 31, fmasks=[(1, 2)], tmasks=[(50, 9)]), SR.row(40, 17, 17, fmasks=[(8, 1)], tmasks=[(5, 2)])]
        x = torch.from_numpy(_spec_input(2, 9, 63, [r[0] for r in rows], 22)).cuda()
    else:                                                                       # test_gpu_specaug.test_strided_input_and_long_utterance
        rows = [SR.row(64, 30, 35, tmasks=[(60, 4)]), SR.row(64, 10, 4), SR.row(40, 20, 39, fmasks=[(4, 1)])]
        x = torch.from_numpy(_spec_input(3, 5, 70, [70, 64, 40], 23)).cuda()[..., :64]
        assert not x.is_contiguous()
    T = x.shape[-1]
    assert any(r[1] != r[2] and r[1] > 0 for r in rows) and any(r[0] < T for r in rows) and (which == "strided" or any(r[1] == r[2] > 0 for r in rows))
    assert any(r[3] for r in rows) and any(r[4] for r in rows) and (T % 4 == 0) == (which != "63")
    return {"out": ops.spec_augment(x, torch.tensor(rows, dtype=torch.int32))}


# ------------------------------------------------------------------------------------------------ waveform rows
def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _resample(long_filter):
    ops = _ops()
    tile = ops.RESAMPLE_TILE
    rng = np.random.RandomState(31 + int(long_filter))
    if long_filter:
        ps, ns, L, R_of = [900, 1000, 900], [2500, 0, 700], 2500, {900: 1200}
        assert tile * 9 // 10 + 2 * R_of[900] > RESAMPLE_LDS                    # the span of a whole tile exceeds the LDS image
    else:
        ps, ns, L, R_of = [1000, 900, 1100, 900], [2500, 2400, 2300, 0], 2500, {}
        assert RR.length(2400, 900) > 2 * tile                                  # a row of three tiles
    tables = {}
    for p in sorted(set(ps) - {1000}):
        num, den = RR.ratio(p)
        R = R_of.get(p, RR.half_width(num, den))
        tables[p] = (R, (rng.randn(den, 2 * R) / np.sqrt(2 * R)).astype(np.float32))
    wav = np.zeros((len(ps), L), np.float32)
    for b, n in enumerate(ns):
        wav[b, :n] = rng.randn(n)
    wav, lens, p = torch.from_numpy(wav), torch.tensor(ns), torch.tensor(ps)
    out, n_out = ops.resample(wav.cuda(), lens, p, tables=tables)
    if not long_filter:
        cols = out.shape[1]
        wide = torch.full((len(ps), (cols + 4) // 4 * 4), 5.0, device="cuda")    # the 16-byte store arm: the fresh (B, 2667) buffer is not
        assert wide.stride(0) % 4 == 0 and wide.data_ptr() % 16 == 0 and cols % 4 and wide.shape[1] > cols
        got = ops.resample(wav.cuda(), lens, p, tables=tables, out=wide)[0]
        assert got.data_ptr() == wide.data_ptr() and _same_bits(wide[:, :cols], out), "an out whose rows are 16-byte aligned"
        assert not wide[:, cols:].contiguous().view(torch.int32).any()
        strided = torch.full((len(ps), cols + 3), 5.0, device="cuda")[:, :cols]
        shifted = torch.zeros(wav.numel() + 4, device="cuda")[1:1 + wav.numel()].view(wav.shape)
        shifted.copy_(wav)
        assert strided.stride(0) % 4 and shifted.data_ptr() % 16 and L % 4 == 0 and wav.cuda().data_ptr() % 16 == 0
        assert _same_bits(ops.resample(wav.cuda(), lens, p, tables=tables, out=strided)[0], out), "an out whose rows are not 16-byte aligned"
        assert _same_bits(ops.resample(shifted, lens, p, tables=tables)[0], out), "a wav that is not 16-byte aligned"
    return {"out": out, "lens": n_out}


REVERB_LENS, REVERB_TAPS = (2500, 1029, 0, 3, 2048), (1, 2, 3, 515, 1025)


def _reverb(which):
    from utils.audio import RirBank
    ops = _ops()
    rng = np.random.RandomState(41)
    if which == "257":
        ns = [64 - (5 * i) % 23 for i in range(257)]
        taps = [(rng.randn(L) * 0.5).astype(np.float32) for L in (1, 2, 3, 4, 5)]
        rir = [-1 if i % 7 == 3 else i % 5 for i in range(257)]
        L = 64
        assert len(ns) > 256
    else:
        ns, L = list(REVERB_LENS), max(REVERB_LENS)
        taps = [(rng.randn(n) / np.sqrt(n)).astype(np.float32) for n in REVERB_TAPS]
        rir = [4, 3, 0, 1, 2] if which == "a" else [0, -1, 2, 2, 3]
    wav = np.full((len(ns), L), 777.0, np.float32)                              # what lies behind n in the input must not matter
    for b, n in enumerate(ns):
        wav[b, :n] = rng.randn(n)
    if which != "257":
        live = [min(taps[r].size, n) for r, n in zip(rir, ns) if r >= 0 and n > 0]          # the taps a row's last tile walks
        chunk = ops.REVERB_CHUNK
        if which == "a":
            assert {t % chunk % 4 for t in live} >= {1, 2, 3} and max(live) > 2 * chunk
        else:
            assert -1 in rir and max(live) > chunk
    bank = RirBank.from_arrays(taps, "cuda")
    wav, lens, idx = torch.from_numpy(wav).cuda(), torch.tensor(ns), torch.tensor(rir)
    out = ops.reverb(wav, lens, idx, bank)
    if which != "257":
        wide = torch.full((len(ns), L + 7), 5.0, device="cuda")
        got = ops.reverb(wav, lens, idx, bank, out=wide)
        assert got.data_ptr() == wide.data_ptr() and wide.stride(0) % 4
        assert _same_bits(wide[:, :L], out) and not wide[:, L:].contiguous().view(torch.int32).any(), "a wider out"
    return {"out": out}


def _signal(kind, n, seed):
    """The signals of tests/test_gpu_augment.py: what load_audio returns for 16-bit pcm."""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / SAMPLE_RATE
    if kind == "white":
        x = rng.randn(n) * 0.2
    elif kind == "chirp":
        x = 0.5 * np.sin(2 * np.pi * (100 * t + 1500 * t * t))
    else:
        x = rng.randn(n) * 0.2 * (0.55 + 0.45 * np.sin(2 * np.pi * 4 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 170 * t))
    return (np.clip(np.rint(x * 32768), -32768, 32767) / 32768).astype(np.float32)


def _augment():
    ops = _ops()
    rng = np.random.RandomState(51)
    clips = [(rng.randn(n) * 4000).clip(-32768, 32767).astype(np.int16) for n in (9000, 1500)]    # the second is read cyclically
    lengths = np.array([c.size for c in clips], dtype=np.int64)
    bank = types.SimpleNamespace(lengths=lengths, data=torch.from_numpy(np.concatenate(clips + [np.zeros(1, np.int16)])).cuda(),
                                 offsets=torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)).cuda(),
                                 lens=torch.from_numpy(lengths).cuda())
    xs = [_signal(k, n, i) for i, (k, n) in enumerate((("white", 5000), ("chirp", 3360), ("am", 6000), ("white", 4000), ("am", 4000),
                                                       ("chirp", 4500)))]
    params = [(0.85, 0.0, -1, 0.0, 0.0), (0.997, 0.0, -1, 0.0, 0.0), (1.15, 0.0, -1, 0.0, 0.0), (1.0, 3.217, -1, 0.0, 0.0),
              (0.0, 0.0, 1, 0.05, 0.25), (0.93, -6.0, 0, 0.2, 0.37)]
    wav = np.zeros((len(xs), max(x.size for x in xs)), np.float32)
    for i, x in enumerate(xs):
        wav[i, :x.size] = x
    out, lens, offs = ops.augment_wave(torch.from_numpy(wav).cuda(), torch.tensor([x.size for x in xs]),
                                       torch.tensor(params, dtype=torch.float64), bank, sample_rate=SAMPLE_RATE, offsets=True)
    assert offs[:3, 1:3].any() and not torch.equal(out[4, :4000].cpu(), torch.from_numpy(xs[4]))       # offsets were searched; noise was mixed
    return {"out": out, "lens": lens, "offsets": offs}


def compute(name):
    """The current library's outputs of case `name` as CPU tensors."""
    kind, _, rest = name.partition("_")
    if kind in ("spect", "fbank"):
        got = _feat_raw(kind + rest[3:])                                        # raw -> "", raw_strided -> "_strided"
    elif kind == "specaug":
        got = _specaug(rest)
    elif kind == "resample":
        got = _resample(rest == "long")
    elif kind == "reverb":
        got = _reverb(rest)
    else:
        got = _augment()
    torch.cuda.synchronize()
    return {k: v.detach().cpu().contiguous() for k, v in got.items()}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _nan_bits(t):
    """The bits of t with every NaN the same one: the silent utterance has no deviation, 0 * inf is a NaN on the device and on the host,
    and the two need not choose the same sign and payload."""
    return torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).view(torch.int32)


def _golden(name):
    z = np.load(GOLDEN)
    return {k.split("/", 1)[1]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "/")}


@pytest.mark.parametrize("name", NAMES)
def test_the_front_end_returns_the_recorded_bits(name):
    want, got = _golden(name), compute(name)
    assert sorted(want) == sorted(got) and want
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (name, k, got[k].dtype, want[k].dtype, got[k].shape, want[k].shape)
        assert torch.equal(_bits(got[k]), _bits(want[k])), (name, k, int((_bits(got[k]) != _bits(want[k])).sum()), "elements differ")


# ------------------------------------------------------------------------------------------------ the forms with float atomics
SPEC_ROWS = {256: [SR.row(1), SR.row(1, fmasks=[(0, 1)]), SR.row(1, tmasks=[(0, 1)]), SR.row(256, 100, 131, fmasks=[(1, 2)], tmasks=[(50, 9), (250, 6)])],
             259: [SR.row(1), SR.row(1), SR.row(1), SR.row(259, 131, 100, fmasks=[(6, 1)], tmasks=[(0, 3)])]}


@pytest.mark.parametrize("form", ["normalize", "spec_256", "spec_259"])
@pytest.mark.parametrize("kind", ["spect", "fbank"])
def test_normalised_and_fused_forms_against_their_own_statistics(kind, form):
    ops = _ops()
    F = MEL if kind == "fbank" else BINS
    nfr = [_frames(n) for n in FEAT_LENS]
    raw_gold = _golden(kind + "_raw")["feat"]
    stats = {}
    if form == "normalize":
        T_out, rows = TMAX, None
        out, nf = _features(kind, normalize=True, stats=stats)
        assert stats["raw"] is None                                             # the normalisation overwrote it
    else:
        T_out = int(form[5:])
        rows = torch.tensor(SPEC_ROWS[T_out], dtype=torch.int32)
        assert (T_out % 4 == 0) == (form == "spec_256") and T_out < TMAX
        out, nf = _features(kind, spec=rows, max_frames=T_out, stats=stats)
        assert torch.equal(_bits(stats["raw"].cpu()), _bits(raw_gold)), "the fused launch's first pass"
    torch.cuda.synchronize()
    assert out.shape == (len(FEAT_LENS), 1, F, T_out) and nf.tolist() == [min(n, T_out) for n in nfr]
    sums, sqdev = stats["sums"].cpu(), stats["sqdev"].cpu()
    n_all = torch.tensor([float(n * F) for n in nfr])                           # fp32: (float)nfr * (float)F, exact
    mean = sums / n_all
    rstd = (1.0 / torch.sqrt((sqdev / (n_all - 1.0)).double())).float()         # correctly rounded; the device's rsqrtf is within 1 ulp
    for b, n in enumerate(nfr):
        term, exact = float(raw_gold[b].double().abs().sum()), float(raw_gold[b].double().sum())
        print("%s %s utterance %d: sums %.9g, float64 %.9g, bound %.3g" % (kind, form, b, float(sums[b]), exact, (n * F - 1) * 2.0 ** -24 * term))
        assert abs(float(sums[b]) - exact) <= (n * F - 1) * 2.0 ** -24 * term, (kind, form, b)
        dev2 = float(((raw_gold[b, ..., :n].double() - float(mean[b])) ** 2).sum())
        k = (n * F + 2) * 2.0 ** -24
        print("%s %s utterance %d: sqdev %.9g, float64 %.9g, bound %.3g" % (kind, form, b, float(sqdev[b]), dev2, k / (1 - k) * dev2))
        assert abs(float(sqdev[b]) - dev2) <= k / (1 - k) * dev2 + n * F * 2.0 ** -149, (kind, form, b)
    have = _nan_bits(out.cpu())
    match = [False] * len(nfr)
    for ulp in (0, -1, 1):
        r = torch.where(torch.isfinite(rstd), (rstd.view(torch.int32) + ulp).view(torch.float32), rstd)
        want = torch.zeros_like(raw_gold)
        for b, n in enumerate(nfr):
            want[b, ..., :n] = (raw_gold[b, ..., :n] - mean[b]) * r[b]
        want = want[..., :T_out]
        if rows is not None:
            want = ops.spec_augment(want.cuda(), rows).cpu()
        want = _nan_bits(want.contiguous())
        for b in range(len(nfr)):
            match[b] = match[b] or torch.equal(have[b], want[b])
    assert all(match), (kind, form, match)
