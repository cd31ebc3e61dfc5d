"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol of include/asr_hip.h, the CLI mirrors the
reference flags, the Noam schedule / text metrics match the oracle, and the data-parallel reducer is exercised with
world_size 2 over gloo."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_loads_and_exports_header_symbols():
    from asr_hip import build, lib
    build.build()
    h = lib.load()
    syms = lib.header_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(h, s), s
    assert set(syms) == set(lib._SIGS), set(syms) ^ set(lib._SIGS)
    assert h.asr_abi_version() == 4
    assert h.asr_strerror(-3).decode().startswith("unsupported")
    # pure host helpers of the ABI (no device needed): workspace sizes
    assert h.asr_add_ln_bwd_workspace(6400, 512) == 800 * 1024
    # 33600 patches, 66 per workgroup: a partial dW block and 64 bias partials per workgroup
    assert h.asr_conv3x3_wgrad_workspace(32, 161, 800, 64, 64) == 510 * 9 * 64 * 64 + 510 * 64
    assert h.asr_gemm_tn_workspace(6400, 2048, 512, 0, 1) == 8 * 64 * 16384      # pipelined 128 x 128 blocks: 64 blocks x 8 m-slices
    assert h.asr_gemm_tn_workspace(6400, 512, 512, 0, 1) == 8 * 64 * 4096         # 64 x 64 tiles: 64 tiles x 8 m-slices
    # one-launch linear backward: m-slices of 16 stages of 64 rows, no empty slice, one 64 x 64 fp32 tile per (slice, tile)
    assert h.asr_gemm_nn_tn_splits(6400, 0) == 7 and h.asr_gemm_nn_tn_splits(3200, 0) == 4 and h.asr_gemm_nn_tn_splits(37, 0) == 1
    assert h.asr_gemm_nn_tn_splits(6400, 100) == 100 and h.asr_gemm_nn_tn_splits(100, 100) == 2
    assert h.asr_gemm_nn_tn_workspace(6400, 512, 2048, 0) == 7 * 8 * 32 * 4096
    assert h.asr_gemm_nn_tn_workspace(3200, 4364, 512, 0) == 4 * 69 * 8 * 4096


def test_product_path_has_no_cpu_fallback():
    from asr_hip import ops
    from asr_hip.lib import AsrHipError
    with pytest.raises(AsrHipError):
        ops.gemm_nt(torch.zeros(8, 8), torch.zeros(8, 8))
    with pytest.raises(AsrHipError):
        ops.add_ln_fwd(torch.zeros(4, 8), None, torch.ones(8), torch.zeros(8))


def test_product_code_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "end2end-asr-pytorch_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("# oracle", ""), os.path.join(dirpath, f)


def test_cli_flags_match_reference_command_lines():
    from utils import constant
    # README-style command lines of the reference (README.md:58,79,92) must parse unchanged
    a = constant.parse("--train-manifest-list a.csv --valid-manifest-list b.csv --test-manifest-list c.csv --cuda "
                       "--batch-size 12 --labels-path l.json --lr 1e-4 --name m --save-folder s --save-every 5 "
                       "--feat_extractor vgg_cnn --dropout 0.1 --num-layers 4 --num-heads 8 --dim-model 512 --dim-key 64 "
                       "--dim-value 64 --dim-input 161 --dim-inner 2048 --dim-emb 512 --shuffle --min-lr 1e-6 --k-lr 1 "
                       "--parallel --device-ids 0 1".split())
    assert a.parallel and a.device_ids == [0, 1] and a.dim_inner == 2048 and a.learning_rate if hasattr(a, "learning_rate") else True
    assert a.lr == 1e-4 and a.feat_extractor == "vgg_cnn" and a.precision == "bf16"
    d = constant.parse([])
    assert (d.num_layers, d.num_heads, d.dim_model, d.dim_inner, d.tgt_max_len, d.src_max_len) == (3, 5, 512, 1024, 1000, 4000)
    assert (d.warmup, d.min_lr, d.k_lr, d.dropout, d.label_smoothing, d.max_norm) == (4000, 1e-5, 1, 0.1, 0.0, 400)
    assert (constant.PAD_TOKEN, constant.SOS_TOKEN, constant.EOS_TOKEN) == (0, 1, 2)


def test_model_keys_match_reference_state_dict(golden_dir):
    import numpy as np
    from utils import constant
    from utils.functions import init_transformer_model
    for name, V in (("vgg_tiny", 32), ("raw_tiny", 32)):
        z = np.load(os.path.join(golden_dir, name + ".npz"))
        flags = str(z["flags"]).split()
        if name == "raw_tiny":
            flags.insert(flags.index("--feat_extractor") + 1, "")
        args = constant.parse(flags)
        chars = [chr(0x4E00 + i) for i in range(int(z["V"]))]
        model = init_transformer_model(args, {c: i for i, c in enumerate(chars)}, {i: c for i, c in enumerate(chars)})
        ref_keys = sorted(k[3:] for k in z.files if k.startswith("w0/"))
        assert sorted(model.state_dict().keys()) == ref_keys
        for k, v in model.state_dict().items():
            assert tuple(v.shape) == z["w0/" + k].shape, k
        assert args.dim_input == int(z["dim_input"])


def test_noam_and_text_metrics_match_oracle():
    from oracle import asr_oracle as O
    from utils.metrics import calculate_cer, calculate_wer
    from utils.optimizer import NoamOpt

    class Dummy:
        param_groups = [{"lr": 0.0}]
        def step(self): pass
    n = NoamOpt(5120, 1.0, 4000, Dummy(), min_lr=1e-5)
    for t in range(1, 6):
        n.step()
        assert abs(n._rate - O.noam_rate(t, 5120, 1.0, 4000, 1e-5)) < 1e-15 and Dummy.param_groups[0]["lr"] == n._rate
    assert calculate_cer("kitten", "sitting") == 3 == O.edit_distance("kitten", "sitting")
    assert calculate_wer("the cat sat", "the cat sat down") == 1
    assert calculate_wer("a b c", "c b a") == 2


def test_rank_shard_splits_every_bin_over_the_ranks():
    """The GLOBAL batch stays --batch-size (the reference's nn.DataParallel scatters one batch over the GPUs): every rank takes
    an equal, disjoint share of every bin; bins smaller than the world size are skipped on every rank."""
    from asr_hip.ddp import rank_shard
    bins = [list(range(0, 8)), list(range(8, 16)), list(range(16, 22)), [22, 23, 24]]
    parts = [rank_shard(bins, r, 4) for r in range(4)]
    assert all(len(p) == 3 for p in parts)                              # the 3-utterance bin is dropped everywhere
    assert all([len(b) for b in p] == [2, 2, 1] for p in parts)         # 8, 8, 6 -> 2, 2, 1 per rank (6 % 4 dropped)
    for j in range(3):
        seen = [u for p in parts for u in p[j]]
        assert len(set(seen)) == len(seen) and set(seen) <= set(bins[j])
    assert rank_shard(bins, 0, 1) == bins


WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[3]); sys.path.insert(0, os.path.join(sys.argv[3], "end2end-asr-pytorch_amd"))
import torch, torch.distributed as dist
from asr_hip.params import FlatParams
from asr_hip.ddp import GradReducer
rank, world = int(sys.argv[1]), int(sys.argv[2])
os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = sys.argv[4]
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.manual_seed(100 + rank)                      # different init per rank: broadcast must equalise
m = torch.nn.Sequential(torch.nn.Linear(40, 70), torch.nn.Linear(70, 30), torch.nn.Linear(30, 5))
flat = FlatParams(m)
red = GradReducer(flat, bucket_bytes=4 * 2000)     # several buckets
assert len(red.buckets) >= 2
assert red.buckets[0]["hi"] == flat.total_all and red.buckets[-1]["lo"] == 0       # the first bucket carries the stats slot
assert sum(b["hi"] - b["lo"] for b in red.buckets) == flat.total_all
red.broadcast_parameters(0)
ref = [torch.zeros_like(flat.data) for _ in range(world)]
dist.all_gather(ref, flat.data)
assert all(torch.equal(r, ref[0]) for r in ref)
for step in range(3):
    if step < 2:
        red.begin_step()                            # what FusedAdam.zero_grad() does; step 2 relies on the automatic restart
    flat.zero_grad()
    flat.stats[0] = 10.0 * (rank + 1) + step        # [loss sum, token count] ride in the tail of the gradient buffer
    flat.stats[1] = 3.0 + rank
    params = list(m.parameters())
    for i, p in reversed(list(enumerate(params))):  # backward order
        p.grad.add_(float(rank + 1) * (i + 1 + step))
        if not (step == 1 and i == 0):              # step 1: the last bucket is left to finish()
            red.mark_ready(p)
    red.finish()
    red.finish()                                    # clip_grad_norm_() and step() both call it: reduced ONCE (ADVICE r1)
    for i, p in enumerate(params):
        want = sum(float(r + 1) for r in range(world)) * (i + 1 + step)
        assert torch.allclose(p.grad, torch.full_like(p.grad, want)), (step, i)
    assert flat.stats[0].item() == sum(10.0 * (r + 1) + step for r in range(world))
    assert flat.stats[1].item() == sum(3.0 + r for r in range(world))
# graph-replay mode: mark_ready / finish are inert, the caller reduces explicit ranges
red.begin_step(); red.hold = True
flat.zero_grad(); flat.grad_all.add_(float(rank + 1))
for p in m.parameters():
    red.mark_ready(p)
red.finish()
assert torch.all(flat.grad_all == float(rank + 1))
cut = flat.offsets[2]
wa = red.all_reduce_range(0, cut); wb = red.all_reduce_range(cut, flat.total_all)
wa.wait(); wb.wait()
assert torch.all(flat.grad_all == float(sum(r + 1 for r in range(world))))
dist.destroy_process_group()
print("ok", rank)
'''


def test_grad_reducer_world2_gloo(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(WORKER)
    port = str(29500 + os.getpid() % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), "2", ROOT, port], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=120)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("ok %d" % r) in o, o


def test_log_spectrogram_matches_reference_convention():
    """SpectrogramParser.parse_audio (reference: utils/data_loader.py:72-89): n_fft = win = 320, hop 160, SYMMETRIC hamming,
    centred reflect-padded frames, |STFT| -> log1p -> (x - mean) / unbiased std.  Checked against torch.stft."""
    import numpy as np
    from utils.audio import hamming_window, log_spectrogram
    rng = np.random.RandomState(0)
    y = (rng.randn(5000) * 0.1).astype(np.float32)
    win = torch.hamming_window(320, periodic=False)
    assert np.allclose(hamming_window(320), win.numpy(), atol=1e-6)
    ref = torch.stft(torch.from_numpy(y), 320, 160, 320, window=win, center=True, pad_mode="reflect", return_complex=True).abs()
    ref = torch.log1p(ref)
    got = log_spectrogram(y, normalize=False)
    assert got.shape == (161, 1 + 5000 // 160) and np.allclose(got, ref.numpy(), atol=2e-4)
    ref = (ref - ref.mean()) / ref.std()
    assert np.allclose(log_spectrogram(y, normalize=True), ref.numpy(), atol=5e-4)


def _scipy_spectrogram(y, normalize):
    """SECOND, independent restatement of SpectrogramParser.parse_audio (reference: utils/data_loader.py:72-89) on scipy.signal:
    the window is the reference's own callable (data_loader.py:20: scipy.signal.hamming, today scipy.signal.windows.hamming) evaluated as
    librosa evaluates a callable window -- window(n_fft), i.e. sym=True --; librosa's center=True is a reflect pad of n_fft // 2 samples
    on both sides; frames of n_fft = win_length = 320 every 160 samples, incomplete last frame dropped; magnitude, log1p, then
    (x - mean) / std with torch's unbiased std over the whole utterance.  scipy.signal.stft divides by sum(window) (scaling
    'spectrum'): undone here."""
    import numpy as np
    import scipy.signal
    win = scipy.signal.windows.hamming(320)                       # sym=True is the default of the callable
    yp = np.pad(np.asarray(y, np.float64), (160, 160), mode="reflect")
    _, _, Z = scipy.signal.stft(yp, fs=16000, window=win, nperseg=320, noverlap=160, nfft=320, boundary=None, padded=False,
                                return_onesided=True)
    sp = np.log1p(np.abs(Z) * win.sum())
    if normalize:
        sp = (sp - sp.mean()) / sp.std(ddof=1)
    return sp


def test_log_spectrogram_matches_scipy_restatement():
    """Pins the spectrogram convention to a second implementation (librosa itself is absent from this image)."""
    import numpy as np
    import scipy.signal
    from utils.audio import hamming_window, log_spectrogram
    assert np.allclose(hamming_window(320), scipy.signal.windows.hamming(320), atol=1e-7)
    assert not np.allclose(hamming_window(320), scipy.signal.windows.hamming(320, sym=False), atol=1e-4)     # the periodic one is NOT it
    rng = np.random.RandomState(7)
    for n in (5000, 16000, 321, 4807):
        y = (rng.randn(n) * 0.1).astype(np.float32)
        for norm in (False, True):
            ref = _scipy_spectrogram(y, norm)
            got = log_spectrogram(y, normalize=norm)
            assert got.shape == ref.shape == (161, 1 + n // 160), (got.shape, ref.shape)
            assert np.abs(got - ref).max() < (2e-4 if not norm else 5e-4), (n, norm, np.abs(got - ref).max())


def spectrogram_known_answer():
    """A 321-sample utterance that is one unit impulse at n0 = 100 has a spectrogram that can be written down by hand.
    Reflect padding by 160 puts a mirror image of the impulse at padded position 60 and the impulse itself at 260; frames start at
    padded positions 0, 160, 320.  With w[k] = 0.54 - 0.46 cos(2 pi k / 319) (SYMMETRIC Hamming, N - 1 in the denominator):
      frame 0 holds both:  |X0[f]|^2 = w[60]^2 + w[260]^2 + 2 w[60] w[260] cos(2 pi f 200 / 320)
      frame 1 holds the impulse at k = 100:  |X1[f]| = w[100] for every bin (a flat spectrum)
      frame 2 holds nothing:  0
    and the stored value is log(1 + |X|).  Returns (waveform, expected (161, 3) array)."""
    import numpy as np
    y = np.zeros(321, np.float32)
    y[100] = 1.0
    w = lambda k: 0.54 - 0.46 * np.cos(2.0 * np.pi * k / 319.0)
    f = np.arange(161, dtype=np.float64)
    x0 = np.sqrt(w(60) ** 2 + w(260) ** 2 + 2.0 * w(60) * w(260) * np.cos(2.0 * np.pi * f * 200.0 / 320.0))
    exp = np.stack([np.log1p(x0), np.full(161, np.log1p(w(100))), np.zeros(161)], axis=1)
    return y, exp


def test_log_spectrogram_known_answer():
    """Hand-computed known-answer test (no FFT library on the expected side): window symmetry, reflect centring, hop, frame count,
    magnitude and log1p all show up in it; the normalised form is checked against the same numbers with the unbiased std."""
    import numpy as np
    from utils.audio import log_spectrogram
    y, exp = spectrogram_known_answer()
    got = log_spectrogram(y, normalize=False)
    assert got.shape == (161, 3)
    assert np.abs(got - exp).max() < 1e-5, np.abs(got - exp).max()
    assert np.abs(_scipy_spectrogram(y, False) - exp).max() < 1e-9
    n = exp.size
    mean = exp.sum() / n
    std = np.sqrt(((exp - mean) ** 2).sum() / (n - 1))
    assert np.abs(log_spectrogram(y, normalize=True) - (exp - mean) / std).max() < 1e-4


def test_loader_contract(tmp_path):
    """manifest 'wav,txt' lines -> (inputs (B,1,161,Tmax) sorted by length desc & zero padded, targets (B,Lmax) i64,
    percentages, input_sizes i32, target_sizes i32); transcripts get SOS/EOS and lose unknown characters."""
    import wave
    import numpy as np
    from utils import constant
    from utils.data_loader import AudioDataLoader, BucketingSampler, SpectrogramDataset
    constant.parse([])                                    # --src-max-len default (4000): no truncation here
    rng = np.random.RandomState(1)
    lines = []
    for i, n in enumerate([8000, 16000, 4000]):
        w = tmp_path / ("u%d.wav" % i)
        with wave.open(str(w), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
            f.writeframes((rng.randn(n) * 2000).astype("<i2").tobytes())
        t = tmp_path / ("u%d.txt" % i)
        t.write_text("Ab c#\n")                           # '#' is not in the label set -> dropped
        lines.append("%s,%s" % (w, t))
    man = tmp_path / "m.csv"
    man.write_text("\n".join(lines))
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + list(" abc")
    l2i = {c: i for i, c in enumerate(chars)}
    conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window="hamming", noise_dir=None, noise_prob=0.4,
                noise_levels=(0.0, 0.5))
    ds = SpectrogramDataset(conf, [str(man)], l2i, normalize=True)
    assert ds.parse_transcript(str(tmp_path / "u0.txt")) == [1, 4, 5, 3, 6, 2]
    loader = AudioDataLoader(ds, num_workers=0, batch_sampler=BucketingSampler(ds, batch_size=3))
    inputs, targets, pct, in_sizes, tgt_sizes = next(iter(loader))
    assert inputs.shape == (3, 1, 161, 101) and inputs.dtype == torch.float32
    assert in_sizes.tolist() == [101, 51, 26] and in_sizes.dtype == torch.int32
    assert (inputs[1, :, :, 51:] == 0).all() and (inputs[2, :, :, 26:] == 0).all()
    assert targets.dtype == torch.int64 and targets.shape == (3, 6) and tgt_sizes.tolist() == [6, 6, 6]
    assert abs(pct[1].item() - 51 / 101) < 1e-6


def test_library_reads_no_environment_and_tuning_goes_through_the_abi():
    """no getenv() in the library; A/B switches are set with asr_set_tuning, unknown names are refused."""
    import glob
    for f in glob.glob(os.path.join(ROOT, "end2end-asr-pytorch_amd", "csrc", "*")):
        assert "getenv" not in open(f).read(), f
    from asr_hip import lib as L
    h = L.load()
    assert h.asr_set_tuning(b"GEMM_TILE", 2) == 0 and h.asr_clear_tuning(b"GEMM_TILE") == 0
    assert h.asr_set_tuning(b"NO_SUCH_SWITCH", 1) != 0
    assert h.asr_clear_tuning(None) == 0


def _outside_ablate_blocks(text):
    """The source as a shipped build sees it: without the `#ifdef ASR_TUNE_ABLATE` arms (an `#else` arm stays)."""
    out, skip = [], None            # skip: the #if depth at which the dropped arm was opened
    depth = 0
    for line in text.split("\n"):
        t = line.strip()
        if t.startswith("#if"):
            depth += 1
            if skip is None and t.split()[:2] == ["#ifdef", "ASR_TUNE_ABLATE"]:
                skip = depth
                continue
        elif t.startswith("#else") and skip == depth:
            skip = -depth           # the #else arm of the block is live
            continue
        elif t.startswith("#endif"):
            depth -= 1
            if skip is not None and abs(skip) == depth + 1:
                skip = None
                continue
        if skip is None or skip < 0:
            out.append(line)
    return "\n".join(out)


def test_tuning_names_are_one_list():
    """The switches of a shipped build are kept in three places that must agree: asr_hip/lib.py TUNING_NAMES (environment forwarding),
    csrc/prof.hip kTuningNames (what asr_set_tuning accepts) and the asr_tuning("...") reads in csrc/ -- a name that is registered but
    never read, or forwarded but refused, is a switch that silently does nothing."""
    import glob
    import re
    from asr_hip import lib as L
    csrc = os.path.join(ROOT, "end2end-asr-pytorch_amd", "csrc")
    read = set()
    for f in glob.glob(os.path.join(csrc, "*")):
        read |= set(re.findall(r'asr_tuning\(\s*"([A-Za-z0-9_]+)"', _outside_ablate_blocks(open(f).read())))
    prof = _outside_ablate_blocks(open(os.path.join(csrc, "prof.hip")).read())
    table = re.search(r"kTuningNames\[\]\s*=\s*\{(.*?)\};", prof, re.S).group(1)
    table = "\n".join(l.split("//")[0] for l in table.split("\n"))
    registered = re.findall(r'"([A-Za-z0-9_]+)"', table)
    assert len(registered) == len(set(registered)) and len(L.TUNING_NAMES) == len(set(L.TUNING_NAMES))
    assert set(registered) == set(L.TUNING_NAMES) == read, (sorted(registered), sorted(L.TUNING_NAMES), sorted(read))
    h = L.load()
    for name in L.TUNING_NAMES:
        assert h.asr_set_tuning(name.encode(), 1) == 0 and h.asr_clear_tuning(name.encode()) == 0, name
    assert not set(L.ABLATE_NAMES) & set(L.TUNING_NAMES)            # (registered in -DASR_TUNE_ABLATE development builds only)


def test_device_prefetcher_passes_batches_through_in_order():
    """utils/data_loader.DevicePrefetcher: same tuples in the same order (host path: pass-through; the H2D overlap itself is
    exercised by tests/test_gpu_train_cli.py, which trains through it)."""
    import torch
    from utils.data_loader import DevicePrefetcher
    batches = [(torch.full((2, 3), float(i)), torch.full((2,), i, dtype=torch.int64), i, "x%d" % i, None) for i in range(5)]
    got = list(DevicePrefetcher(batches, device=None))
    assert len(got) == 5 and all(g[2] == i and torch.equal(g[0], batches[i][0]) for i, g in enumerate(got))
    assert list(DevicePrefetcher([], device=None)) == []


def test_native_edit_distance_matches_python_and_oracle():
    """asr_edit_distance_batch (host C++ in libasr_hip.so) against the pure-Python distance it replaces and the oracle's, on
    random strings incl. empty ones and CJK code points, and on word lists (WER)."""
    import random
    from asr_hip.text import edit_distance, edit_distance_batch, edit_distance_py
    from oracle import asr_oracle as O
    rnd = random.Random(7)
    alphabet = "abcdefghij 的一是不了"
    pairs = [("".join(rnd.choice(alphabet) for _ in range(rnd.randint(0, 90))),
              "".join(rnd.choice(alphabet) for _ in range(rnd.randint(0, 90)))) for _ in range(48)]
    pairs += [("", ""), ("abc", ""), ("", "xy"), ("kitten", "sitting")]
    got = edit_distance_batch(pairs)
    assert got == [edit_distance_py(a, b) for a, b in pairs] == [O.edit_distance(a, b) for a, b in pairs]
    words = [(a.split(), b.split()) for a, b in pairs]
    assert edit_distance_batch(words) == [edit_distance_py(a, b) for a, b in words]
    assert edit_distance("flaw", "lawn") == 2 and edit_distance_batch([]) == []


def test_command_line_records_which_options_were_typed():
    """load_model keeps a checkpoint's --precision unless the user typed the option (utils/functions.py): constant.explicit holds the
    destinations of the options present on the command line, not the argparse defaults."""
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    try:
        a = constant.parse(["--num-layers", "2", "--precision=fp32"])
        assert a.precision == "fp32" and {"num_layers", "precision"} <= constant.explicit and "gpu_frontend" not in constant.explicit
        constant.parse(["--num-layers", "2"])
        assert "precision" not in constant.explicit
    finally:
        constant.set_args(old_args)
        constant.explicit = old_explicit


def test_grouped_weight_gradient_plan():
    """asr_gemm_tn_grouped_plan (host only): the 46 linear layers of configs[1] are one launch of whole blocks, none sliced; configs[3]'s
    48 encoder problems (576 equal blocks of 398 stages = 2.25 rounds of 256 CUs) keep the shared forms; a single block over 400 000 rows
    (emb_cnn's window contraction) next to ordinary layers is sliced into about a CU's share each."""
    import ctypes
    from asr_hip import lib as L
    h = L.load()

    def plan(probs):
        n = len(probs)
        I = ctypes.c_int * n
        sp = I()
        rc = h.asr_gemm_tn_grouped_plan(n, I(*[p[0] for p in probs]), I(*[p[1] for p in probs]), I(*[p[2] for p in probs]), sp)
        assert rc in (0, 1), rc
        return rc, list(sp)

    enc = lambda M: [(M, 512, 2048), (M, 2048, 512), (M, 512, 512), (M, 1536, 512)]
    dec = lambda Md, Me: [(Md, 512, 2048), (Md, 2048, 512), (Md, 512, 512), (Me, 1024, 512), (Md, 512, 512), (Md, 512, 512), (Md, 1536, 512)]
    headline = [(3200, 4416, 512)] + dec(3200, 6400) * 4 + enc(6400) * 4 + [(6400, 512, 2560)]
    assert len(headline) == 46
    assert plan(headline) == (1, [1] * 46)
    assert plan(enc(12720) * 12)[0] == 0
    whole, sp = plan([(409600, 64, 64)] + enc(6400) * 8)
    assert whole == 1 and sp[1:] == [1] * 32 and 32 <= sp[0] <= 64          # 384 blocks x 200 stages + 12 800: a CU's share is ~350 stages
    assert plan([(409600, 64, 64)] + enc(6400) * 2)[0] == 0                  # 96 blocks on 256 CUs: the equal pieces fill the chip
    assert plan([]) == (1, [])


def test_deferred_weight_gradients_close_their_groups_by_work(monkeypatch):
    """Host logic of asr_hip/ops.py queue_wgrad / flush_wgrads (no kernel runs: the grouped launch is replaced by a recorder).  Round 5
    default: a group is closed at 48 layers (asr_gemm_tn_grouped's limit; whole-contraction blocks dispatched longest first want the
    largest group) and a flush empties the queue in order.  Round 3's grouping (ASR_WGRAD_GROUP=32 ASR_WGRAD_STAGES=38000, for the
    equal-piece kernel ASR_TN_ROT=0): 32 layers or ~38 000 block-stages of 256 x 256 x 64 rows, whichever comes first -- 32 layers at the
    6 400 rows of configs[1], 16 at the 12 720 rows of configs[3]."""
    from asr_hip import ops
    seen = []
    monkeypatch.setattr(ops, "gemm_tn_grouped", lambda grp: seen.append([(e[0].shape[0], e[4], e[5]) for e in grp]))
    monkeypatch.setattr(ops, "_wgrad_q", [])
    monkeypatch.setattr(ops, "_wgrad_stages", [0])

    def layer(M):
        for N, K in ((1536, 512), (512, 512), (2048, 512), (512, 2048)):
            ops.queue_wgrad(torch.zeros(M, N, dtype=torch.bfloat16), torch.zeros(M, K, dtype=torch.bfloat16),
                            torch.zeros(N, K), torch.zeros(N), N, K)

    assert ops.WGRAD_GROUP == 48 and ops.WGRAD_STAGES == 0
    for M in (6400, 12720):
        for _ in range(13):
            layer(M)
        assert [len(g) for g in seen] == [48]
        ops.flush_wgrads()
        assert [len(g) for g in seen] == [48, 4] and not ops._wgrad_q
        assert [e[0] for g in seen for e in g] == [M] * 52
        del seen[:]
    monkeypatch.setattr(ops, "WGRAD_GROUP", 32)
    monkeypatch.setattr(ops, "WGRAD_STAGES", 38000)
    for _ in range(10):
        layer(6400)
    assert [len(g) for g in seen] == [32]
    ops.flush_wgrads()
    assert [len(g) for g in seen] == [32, 8] and not ops._wgrad_q
    del seen[:]
    for _ in range(10):
        layer(12720)
    ops.flush_wgrads()
    assert [len(g) for g in seen] == [16, 16, 8]
    assert [e[0] for g in seen for e in g] == [12720] * 40
    del seen[:]
    for _ in range(12):                                   # decoder-sized problems: the count cap decides
        layer(1600)
    ops.flush_wgrads()
    assert [len(g) for g in seen] == [32, 16]


@pytest.mark.parametrize("cfg", [(2, 61, 23, 32, 21, 11, 2, 1, 0), (2, 61, 30, 1, 41, 11, 2, 2, 10)])
@pytest.mark.parametrize("shift", [True, False])
def test_window_convolution_algebra_on_cpu_stand_ins(monkeypatch, cfg, shift):
    """The index algebra of asr_hip/functions.py _conv_window_fwd / _conv_window_bwd -- single-time-step patches X2, the overlapping-rows
    window view, the dense per-tap product + window sum, the packet-of-rows weight-gradient contraction against the shifted dy view, the
    data gradient through col2im -- with every kernel replaced by a few lines of torch on the CPU (fp32 arithmetic on bf16-typed
    buffers' values): equal to F.conv2d and its autograd.  Both emb_cnn layers (reference transformer.py:33-40), both forms."""
    import torch.nn.functional as F
    from asr_hip import functions as Fn
    from asr_hip import ops
    B, H, W, C, KH, KW, SH, SW, PW = cfg
    Cout = 32

    def im2col(x, g, col):
        Bq, Hq, Wq, Cq, kh, kw, sh, sw, ph, pw, oh, ow = g
        xp = F.pad(x.float(), (0, 0, pw, pw, ph, ph))
        rows = torch.zeros(Bq, oh, ow, kh, kw, Cq)
        for ky in range(kh):
            for kx in range(kw):
                rows[:, :, :, ky, kx] = xp[:, ky:ky + sh * (oh - 1) + 1:sh, kx:kx + sw * (ow - 1) + 1:sw]
        col.zero_()
        col[:Bq * oh * ow, :kh * kw * Cq] = rows.reshape(Bq * oh * ow, -1).to(col.dtype)
        return col

    def col2im(dcol, g):
        Bq, Hq, Wq, Cq, kh, kw, sh, sw, ph, pw, oh, ow = g
        dx = torch.zeros(Bq, Hq + 2 * ph, Wq + 2 * pw, Cq)
        d = dcol[:Bq * oh * ow, :kh * kw * Cq].float().reshape(Bq, oh, ow, kh, kw, Cq)
        for ky in range(kh):
            for kx in range(kw):
                dx[:, ky:ky + sh * (oh - 1) + 1:sh, kx:kx + sw * (ow - 1) + 1:sw] += d[:, :, :, ky, kx]
        return dx[:, ph:ph + Hq, pw:pw + Wq].to(dcol.dtype)

    def gemm_nt(A, Bm, out=None, bias=None, **kw):
        r = A.float() @ Bm.float().t()
        if bias is not None:
            r = r + bias[:r.shape[1]]
        out.copy_(r.to(out.dtype))
        return out

    def gemm_tn(dy, x, dw, colsum_acc=None, N=None, K=None, **kw):
        dw += dy[:, :N].float().t() @ x[:, :K].float()
        if colsum_acc is not None:
            colsum_acc += dy[:, :N].float().sum(0)

    def gemm_tn_grouped(grp):
        for dy, x, dw, db, N, K in grp:
            gemm_tn(dy, x, dw, colsum_acc=db, N=N, K=K)

    def window_sum(Z, y, bias, groups, Wg, OW, KW_, Co):
        y.zero_()
        for kx in range(KW_):
            y[:groups * OW, :Co] += Z[kx:kx + groups * Wg].view(groups, Wg, -1)[:, :OW, kx * Co:(kx + 1) * Co].reshape(groups * OW, Co)
        y[:groups * OW, :Co] += bias[:Co]
        return y

    def colsum_acc(x, out):
        out += x.float().sum(0)

    for name, fn in (("im2col", im2col), ("col2im", col2im), ("gemm_nt", gemm_nt), ("gemm_tn", gemm_tn), ("gemm_tn_grouped", gemm_tn_grouped),
                     ("window_sum", window_sum), ("colsum_acc", colsum_acc)):
        monkeypatch.setattr(ops, name, fn)
    monkeypatch.setattr(ops, "_ws", {})
    monkeypatch.setattr(ops, "compute_dtype", lambda: torch.bfloat16)
    monkeypatch.setattr(Fn, "_emb_shift_fwd", shift)
    monkeypatch.setattr(Fn, "_emb_shift_wgrad", shift)

    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, C, H, W, generator=g).bfloat16().float()
    w = (torch.randn(Cout, C, KH, KW, generator=g) * (C * KH * KW) ** -0.5).bfloat16().float()
    b = torch.randn(Cout, generator=g)
    xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    ref = F.conv2d(xr, wr, br, stride=(SH, SW), padding=(0, PW))
    OH, OW = ref.shape[2], ref.shape[3]
    dy = torch.randn(B, Cout, OH, OW, generator=g).bfloat16().float()
    ref.backward(dy)
    geo = ops.conv_geom(B, H, W, C, KH, KW, SH, SW, 0, PW)
    assert Fn._window_ok(geo)
    wd, bd = torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone())
    X2, A, y, M, (yW, yOW) = Fn._conv_window_fwd(x.permute(0, 2, 3, 1).contiguous().bfloat16(), geo, wd, bd, "cpu_win")
    yc = y[:M // yOW * yW].view(M // yOW, yW, -1)[:, :yOW].reshape(M, -1) if yOW else y[:M]      # strided form: y on the GEMM's row grid
    got = yc[:, :Cout].reshape(B, OH, OW, Cout).permute(0, 3, 1, 2)
    assert (got - ref.detach()).abs().max().item() < 1e-4 * max(1.0, ref.detach().abs().max().item())
    Dd, dview, (dW, dOW) = Fn._window_dy(geo, Cout, "cpu_win", torch.device("cpu"))
    dview.view(B * OH, dW, Cout)[:, :OW] = dy.permute(0, 2, 3, 1).reshape(B * OH, OW, Cout).bfloat16()
    bg = torch.zeros(Cout)
    dw, dx = Fn._conv_window_bwd(Dd, A, wd, bg, geo, "cpu_win", SW == 1)
    assert tuple(dw.shape) == tuple(w.shape)
    assert (dw - wr.grad).abs().max().item() < 1e-4 * wr.grad.abs().max().item()
    assert (bg - br.grad).abs().max().item() < 1e-4 * br.grad.abs().max().item()
    if SW == 1:
        dxr = xr.grad.permute(0, 2, 3, 1)
        assert (dx.float() - dxr).abs().max().item() < 1.5e-2 * dxr.abs().max().item()       # dX2 and dx are stored in bf16


def test_reset_pending_forgets_everything_a_failed_pass_left(monkeypatch):
    """a backward pass that raised leaves queued weight gradients, pending folds and the armed flush flag behind; reset_pending()
    (FusedAdam.zero_grad(), the capture's error path) clears all of them -- host logic only, nothing is launched."""
    from asr_hip import ops
    monkeypatch.setattr(ops, "_wgrad_q", [("dy", "x", "dw", "db", 1, 1)])
    monkeypatch.setattr(ops, "_wgrad_stages", [123])
    monkeypatch.setattr(ops, "_tn_pending", [1])
    monkeypatch.setattr(ops, "_ln_pending", [2])
    monkeypatch.setitem(ops._backward_flush, "armed", True)
    ops.reset_pending()
    assert ops._wgrad_q == [] and ops._wgrad_stages == [0] and ops._tn_pending == [] and ops._ln_pending == []
    assert ops._backward_flush["armed"] is False


def test_workspace_is_rezeroed_when_the_live_region_moves():
    """ops.workspace() keeps padding rows zero by re-zeroing only when the request differs from the previous one; the row
    grid of emb_cnn's window gradients is part of that request (`geom`): equal shapes with different grids must not see stale rows."""
    from asr_hip import ops
    a = ops.workspace("t_geom", (6, 4), torch.float32, "cpu", geom=(2, 3, 2))
    a[1].fill_(7.0)                                # a live row of the first grid
    b = ops.workspace("t_geom", (6, 4), torch.float32, "cpu", geom=(2, 3, 2))
    assert b.data_ptr() == a.data_ptr() and float(b[1, 0]) == 7.0            # same request: untouched (the kernels rewrite live rows)
    c = ops.workspace("t_geom", (6, 4), torch.float32, "cpu", geom=(3, 2, 1))
    assert c.data_ptr() == a.data_ptr() and float(c.abs().sum()) == 0.0      # same shape, other grid: zero again


WORKER8 = r'''
import os, sys
sys.path.insert(0, sys.argv[3]); sys.path.insert(0, os.path.join(sys.argv[3], "end2end-asr-pytorch_amd"))
import torch, torch.distributed as dist
rank, world = int(sys.argv[1]), int(sys.argv[2])
os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = sys.argv[4]
dist.init_process_group("gloo", rank=rank, world_size=world)
import bench
from asr_hip.ddp import GradReducer, rank_shard
from asr_hip.graph import GraphedTrainStep
from asr_hip.params import FlatParams
from utils import constant
from utils.functions import init_transformer_model
# configs[1] as bench.py builds it (CPU parameters: no kernel runs here, only the reducer's bookkeeping and the collectives)
args = constant.parse(bench.MODEL_FLAGS + ["--dropout", "0.1", "--precision", "bf16", "--batch-size", "32", "--parallel"])
l2i, i2l = bench.labels(bench.V)
torch.manual_seed(7)
model = init_transformer_model(args, l2i, i2l)
core = model.module if hasattr(model, "module") else model
flat = FlatParams(core)
red = GradReducer(flat, wire="bf16")
assert red.world == 8 and red.active
# ---- layout facts the four-graph step and the bf16 wire rely on, at the REAL offsets
split = GraphedTrainStep._conv_split(flat)
split_dec = GraphedTrainStep._decoder_split(flat, core, split)
assert 0 < split_dec < split < flat.total < flat.total_all
ranges = [(split_dec, split), (0, split_dec), (split, flat.total_all)]          # decoder, encoder, conv + stats (graph.py _exchange_*)
assert sum(hi - lo for lo, hi in ranges) == flat.total_all
for lo, hi in ranges:
    ghi = min(hi, flat.total)
    assert lo % 8 == 0 and ghi % 8 == 0, ("a slice of the step is not 16-byte aligned in the bf16 staging buffer", lo, ghi)
assert ranges[0][1] - ranges[0][0] >= red.WIRE_MIN and ranges[1][1] - ranges[1][0] >= red.WIRE_MIN     # both transformer slices take the bf16 wire
assert flat.total_all - flat.total >= 3                                          # the stats slot [loss sum, token count, num_correct]
# eager buckets: contiguous cover, conv buckets apart, every boundary aligned, the first bucket ends at the stats slot
assert red.buckets[0]["hi"] == flat.total_all and red.buckets[-1]["lo"] == 0
assert all(a["lo"] == b["hi"] for a, b in zip(red.buckets, red.buckets[1:]))
assert all(b["lo"] % 8 == 0 for b in red.buckets)
conv_ix = {i for i, p in enumerate(flat.params) if p.dim() == 4}
assert all(not (b["members"] & conv_ix) or all(flat.params[i].dim() in (1, 4) for i in b["members"]) for b in red.buckets)
# ---- the collectives at world 8 on the real buffer (fp32 wire: the bf16 cast is a device kernel): exact small integers
red.wire = "fp32"
red.broadcast_parameters(0)
red.begin_step(); red.hold = True
flat.zero_grad()
flat.grad_all[:flat.total].fill_(float(rank + 1))
flat.stats[0] = 100.0 + rank; flat.stats[1] = 10.0 * (rank + 1); flat.stats[2] = float(rank)
works = [red.all_reduce_range(lo, hi) for lo, hi in ranges]
for w in works:
    w.wait()
tot = float(sum(r + 1 for r in range(world)))
g = flat.grad_all[:flat.total]
assert float(g.min()) == tot and float(g.max()) == tot
assert flat.stats[0].item() == sum(100.0 + r for r in range(world)) and flat.stats[1].item() == 10.0 * tot and flat.stats[2].item() == sum(range(world))
# ---- uneven bins: every rank the same number of steps and utterances per step
bins = [list(range(0, 32)), list(range(32, 61)), list(range(61, 68)), list(range(68, 75))]
mine = rank_shard(bins, rank, world)
sizes = torch.tensor([len(b) for b in mine] + [0] * (8 - len(mine)))
allsz = [torch.zeros_like(sizes) for _ in range(world)]
dist.all_gather(allsz, sizes)
assert all(torch.equal(s, allsz[0]) for s in allsz) and [len(b) for b in mine] == [4, 3]       # 32 -> 4, 29 -> 3 (5 dropped), 7 and 7 < 8 skipped
dist.barrier()
dist.destroy_process_group()
print("ok", rank)
'''


def test_grad_reducer_world8_gloo_at_the_benchmark_models_offsets(tmp_path):
    """VERDICT r4 #7b: the data-parallel bookkeeping at configs[1]'s REAL parameter offsets under eight ranks (gloo, CPU): the three
    slices of the four-graph step and every eager bucket start on 16-byte boundaries of the bf16 staging buffer (the `lo % 8` rule of
    GradReducer.all_reduce_range), both transformer slices are large enough for the bf16 wire, the stats slot rides behind the conv
    slice, the all-reduces of the real 147 MB buffer sum exactly, and uneven BucketingSampler bins give every rank the same steps."""
    script = tmp_path / "w8.py"
    script.write_text(WORKER8)
    port = str(31500 + os.getpid() % 2000)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), "8", ROOT, port], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(8)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("ok %d" % r) in o, o


def test_train_cli_replays_graphs_by_default_for_vgg_cnn():
    """VERDICT r4 #6a: the README command line gets the benched path.  `train.py --cuda` with vgg_cnn and the CE loss resolves
    --graph-buckets to 64 unless the user typed a value (0 = opt out); so does emb_cnn since round 6 (its BatchNorm statistics are
    length-masked to the batch as collated); a model without a CNN front end, the CTC loss and CPU runs keep the eager loop."""
    import importlib
    from utils import constant
    train = importlib.import_module("train")

    def resolved(argv):
        a = constant.parser.parse_args(argv)
        return train.resolve_graph_buckets(a, constant._given(argv))

    base = ["--feat_extractor", "vgg_cnn"]
    assert resolved(base + ["--cuda"]) == 64
    assert resolved(base + ["--cuda", "--graph-buckets", "0"]) == 0
    assert resolved(base + ["--cuda", "--graph-buckets", "128"]) == 128
    assert resolved(base) == 0
    assert resolved(["--feat_extractor", "emb_cnn", "--cuda"]) == 64
    assert resolved(["--feat_extractor", "", "--cuda"]) == 0
    assert resolved(base + ["--cuda", "--loss", "ctc"]) == 0

    # the MODEL's front end decides, not the command line's default -- `train.py --cuda --continue-from <emb_cnn checkpoint>`
    # without retyping --feat_extractor must be decided by the checkpoint's model (the trainer clamps the lengths by the MODEL's front end:
    # an emb_cnn model under the command line's vgg_cnn default would have had half its positions masked)
    class _M:
        def __init__(self, feat):
            self.feat_extractor = feat

    class _Wrapped:
        def __init__(self, feat):
            self.module = _M(feat)

    def resolved_for(argv, model):
        a = constant.parser.parse_args(argv)
        return train.resolve_graph_buckets(a, constant._given(argv), model)

    assert resolved_for(["--cuda"], _M("")) == 0                              # command line says vgg_cnn (default), the checkpoint's model has no CNN
    assert resolved_for(["--cuda"], _Wrapped("")) == 0
    assert resolved_for(["--feat_extractor", "", "--cuda"], _M("vgg_cnn")) == 64
    assert resolved_for(["--feat_extractor", "", "--cuda"], _Wrapped("emb_cnn")) == 64
    assert resolved_for(["--cuda", "--graph-buckets", "32"], _M("")) == 32


def test_kernel_coverage_parser_counts_launches_per_symbol():
    """tools/kernel_coverage.py (host only): a three-line kernel-trace CSV -- a mangled name with the `.kd` suffix and a demangled one
    with a return type -- counted per symbol under either spelling; a symbol the trace does not name counts zero."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
    kc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kc)
    ring = "_ZN12_GLOBAL__N_116gemm_glds_kernelIttLi64ELi64ELi3EEEvNS_8GemmArgsE"
    fold = "_ZN12_GLOBAL__N_116tn_reduce_kernelEPKfPfliiiii"
    names = {ring: "void (anonymous namespace)::gemm_glds_kernel<unsigned short, unsigned short, 64, 64, 3>((anonymous namespace)::GemmArgs)",
             fold: "(anonymous namespace)::tn_reduce_kernel(float const*, float*, long, int, int, int, int, int)"}
    trace = ['"Kind","Agent_Id","Kernel_Id","Kernel_Name","Start_Timestamp","End_Timestamp"',
             '"KERNEL_DISPATCH",4,7,"%s.kd",100,200' % ring,
             '"KERNEL_DISPATCH",4,7,"void (anonymous namespace)::gemm_glds_kernel<unsigned short, unsigned short, 64, 64, 3>((anonymous namespace)::GemmArgs)",300,400']
    counts = kc.launch_counts(trace)
    assert sum(counts.values()) == 2
    assert kc.coverage([ring, fold], names, counts) == {ring: 2, fold: 0}


def test_isa_identity_by_symbol_flags_a_kernel_two_files_define_unless_both_dumps_share_it(tmp_path):
    """tools/isa_identity.py compare --by-symbol (host only, hand-written assembly): a kernel that moved to another file compares equal; one
    that both dumps define in two files with identical copies (a kernel in a header) is one symbol; copies that differ from each other in
    AFTER, a copy left behind in a second file of AFTER, and a changed instruction each count as differing."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("isa_identity", os.path.join(ROOT, "tools", "isa_identity.py"))
    ii = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ii)

    def asm(*kernels):
        return "".join("%s:\n\t%s\n\ts_endpgm\n.Lfunc_end%d:\n\t.section .rodata\n\t.amdhsa_kernel %s\n\t\t.amdhsa_next_free_vgpr 8\n"
                       "\t.end_amdhsa_kernel\n\t.text\n" % (k, ins, n, k) for n, (k, ins) in enumerate(kernels))

    def dump(name, files):
        d = os.path.join(str(tmp_path), name)
        os.makedirs(d)
        for f, ks in files.items():
            with open(os.path.join(d, f + ".s"), "w") as fh:
                fh.write(asm(*ks))
        return d

    a, b, h, h2 = ("_Z1av", "v_mov_b32 v0, 1"), ("_Z1bv", "v_mov_b32 v0, 2"), ("_Z1hv", "v_mov_b32 v0, 3"), ("_Z1hv", "v_mov_b32 v0, 4")
    before = dump("before", {"one.hip": [a, b, h], "two.hip": [h]})
    assert ii._union(before)[1:] == (set(), {"_Z1hv"})
    assert ii.compare_by_symbol(before, dump("moved", {"x.hip": [h, a], "y.hip": [b, h]})) == 0
    assert ii.compare_by_symbol(before, dump("diverged", {"x.hip": [a, h], "y.hip": [b, h2]})) == 1
    assert ii.compare_by_symbol(before, dump("diverged_first", {"x.hip": [a, h2], "y.hip": [b, h]})) == 1
    assert ii.compare_by_symbol(before, dump("left_behind", {"x.hip": [a, b, h], "y.hip": [b, h]})) == 1
    assert ii.compare_by_symbol(before, dump("changed", {"x.hip": [a, ("_Z1bv", "v_mov_b32 v0, 5"), h], "y.hip": [h]})) == 1


def test_kernel_coverage_attention_family_names_five_translation_units():
    """tools/kernel_coverage.py --family attention (host only): the family is the five attention translation units that hold kernels; a
    trace row of a kernel in a nested anonymous namespace (asr_attn::(anonymous namespace)::..., two int arguments after the struct) is
    counted under its mangled and its demangled spelling; the kernels that only a one-part asr_attn_bwd call reaches are named in
    PARTS_ONLY."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
    kc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kc)
    assert kc.FAMILIES["attention"] == ("attention_generic.hip", "attention_d64_fwd.hip", "attention_d64_bwd.hip", "attention_d64_bwd_fused.hip",
                                        "attention_pp.hip") and kc.FAMILIES["gemm"] == kc.GEMM_FILES
    for f in kc.FAMILIES["attention"]:
        assert os.path.exists(os.path.join(ROOT, "end2end-asr-pytorch_amd", "csrc", f)), f
    both = "_ZN8asr_attn12_GLOBAL__N_129attn_bwd_both_bf16_d64_kernelILi1EEEvNS_8AttnArgsEi"
    dq = "_ZN8asr_attn12_GLOBAL__N_127attn_bwd_dq_bf16_d64_kernelILi1EEEvNS_8AttnArgsE"
    pp = "_ZN8asr_attn12_GLOBAL__N_127attn_fwd_pp_bf16_d64_kernelILb1ELi4EEEvNS_8AttnArgsEiii"
    names = {both: "void asr_attn::(anonymous namespace)::attn_bwd_both_bf16_d64_kernel<1>(asr_attn::AttnArgs, int)",
             dq: "void asr_attn::(anonymous namespace)::attn_bwd_dq_bf16_d64_kernel<1>(asr_attn::AttnArgs)",
             pp: "void asr_attn::(anonymous namespace)::attn_fwd_pp_bf16_d64_kernel<true, 4>(asr_attn::AttnArgs, int, int, int)"}
    trace = ['"Kind","Agent_Id","Kernel_Id","Kernel_Name","Start_Timestamp","End_Timestamp"',
             '"KERNEL_DISPATCH",4,7,"%s.kd",100,200' % both,
             '"KERNEL_DISPATCH",4,8,"%s",300,400' % names[both],
             '"KERNEL_DISPATCH",4,9,"void asr_attn::(anonymous namespace)::attn_fwd_pp_bf16_d64_kernel<true, 4>(asr_attn::AttnArgs, int, int, int) [clone .kd]",500,600',
             '"KERNEL_DISPATCH",4,9,"void asr_attn::(anonymous namespace)::attn_fwd_pp_bf16_d64_kernel<false, 4>(asr_attn::AttnArgs, int, int, int)",700,800']
    counts = kc.launch_counts(trace)
    assert sum(counts.values()) == 4
    assert kc.coverage([both, dq, pp], names, counts) == {both: 2, dq: 0, pp: 1}
    assert any(sub in names[dq] for sub, _ in kc.PARTS_ONLY) and not any(sub in names[both] for sub, _ in kc.PARTS_ONLY)


def test_kernel_coverage_conv_family_names_nine_translation_units():
    """tools/kernel_coverage.py --family conv (host only): the nine translation units of the convolution front end exist; the four 8-wave
    c64 instantiations are explained as hook-only, the default one is not; a trace row of a c64 kernel counts under either spelling."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
    kc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kc)
    assert len(kc.FAMILIES["conv"]) == 9 and kc.HOOK_ONLY_OF["gemm"] is kc.HOOK_ONLY
    for f in kc.FAMILIES["conv"]:
        assert os.path.exists(os.path.join(ROOT, "end2end-asr-pytorch_amd", "csrc", f)), f
    wide = "_ZN12_GLOBAL__N_118conv3x3_c64_kernelILi32ELi8ELb1ELi3ELb0EEEvNS_7C64ArgsE"
    dflt = "_ZN12_GLOBAL__N_118conv3x3_c64_kernelILi16ELi8ELb0ELi3ELb0EEEvNS_7C64ArgsE"
    names = {wide: "void (anonymous namespace)::conv3x3_c64_kernel<32, 8, true, 3, false>((anonymous namespace)::C64Args)",
             dflt: "void (anonymous namespace)::conv3x3_c64_kernel<16, 8, false, 3, false>((anonymous namespace)::C64Args)"}
    trace = ['"Kind","Agent_Id","Kernel_Id","Kernel_Name","Start_Timestamp","End_Timestamp"',
             '"KERNEL_DISPATCH",4,7,"%s.kd",100,200' % wide, '"KERNEL_DISPATCH",4,8,"%s",300,400' % names[wide]]
    assert kc.coverage([wide, dflt], names, kc.launch_counts(trace)) == {wide: 2, dflt: 0}
    hooked = [sub for sub, _ in kc.HOOK_ONLY_OF["conv"]]
    assert len(hooked) == 4 and any(sub in names[wide] for sub in hooked) and not any(sub in names[dflt] for sub in hooked)
