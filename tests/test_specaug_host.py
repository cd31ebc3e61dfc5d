"""SpecAugment without a GPU: the float64 definition (tests/specaug_reference.py) against torch's linear interpolation, the loader's
draws, the 7-element batch, what stays untouched with the flag off, the CLI flags and their start-up checks."""
import random

import numpy as np
import pytest
import torch

import specaug_reference as R
import test_augment_host as H

LD = dict(time_warp=80, freq_mask=27, freq_masks=2, time_mask=100, time_masks=2, time_mask_ratio=1.0)


@pytest.fixture
def front_end_args():
    from utils import constant
    old = constant.args
    constant.parse(["--gpu-frontend", "--spec-augment"])
    yield constant.args
    constant.set_args(old)


def _interp(x, size):
    return torch.nn.functional.interpolate(x[None], size=size, mode="linear", align_corners=False)[0]


@pytest.mark.parametrize("n,c,w", [(37, 16, 20), (37, 16, 11), (64, 5, 0), (64, 5, 10), (33, 32, 27), (257, 100, 1), (4000, 80, 160),
                                   (4000, 3919, 3999)])
def test_reference_warp_is_torch_linear_interpolation(n, c, w):
    x = np.random.RandomState(n + c).randn(3, n + 4)
    xt = torch.from_numpy(x[:, :n])
    parts = ([_interp(xt[:, :c], w)] if w else []) + [_interp(xt[:, c:], n - w)]
    ref = torch.cat(parts, dim=1).numpy()
    got = R.warp(x, n, c, w)
    err = np.abs(got - ref).max()
    print("n %d c %d w %d: max |reference - F.interpolate| = %.3g" % (n, c, w, err))
    assert got.shape == (3, n) and err <= 1e-9


def test_reference_identity_and_masks():
    x = np.random.RandomState(0).randn(5, 40).astype(np.float32)
    for c in (0, 1, 17, 36):
        assert np.array_equal(R.warp(x, 37, c, c).astype(np.float32).view(np.uint32), x[:, :37].view(np.uint32))
    i0, i1, r, den = R.warp_source(37, 16, 20)
    assert (np.diff(i0) >= 0).all() and i0[0] == 0 and i1[-1] == 36 and (i1[:20] <= 15).all() and (i0[20:] >= 16).all()
    y = R.spec_augment(x, R.row(37, fmasks=[(1, 2), (2, 2)], tmasks=[(0, 3), (30, 0), (35, 9)]))
    keep = np.ones((5, 40), bool)
    keep[1:4] = False
    keep[:, :3] = False
    keep[:, 35:] = False
    assert np.array_equal(y[keep], x[keep].astype(np.float64)) and not y[~keep].any()


def test_draws_stay_in_range_and_reach_both_ends(front_end_args):
    from utils.data_loader import SPEC_PARAMS, SpectrogramParser
    pol = dict(time_warp=5, freq_mask=4, freq_masks=2, time_mask=6, time_masks=3, time_mask_ratio=0.2)
    p = SpectrogramParser(H._conf(), normalize=True, spec_augment=pol)
    samples, n, F, W = 25 * 160 + 7, 26, 161, 5
    np.random.seed(11)
    rows = np.array([p.draw_spec(samples) for _ in range(2000)])
    assert rows.shape == (2000, SPEC_PARAMS) and (rows[:, 0] == n).all() and (rows[:, 3] == 2).all() and (rows[:, 4] == 3).all()
    assert not rows[:, 5:8].any() and not rows[:, 12:24].any() and not rows[:, 30:].any()
    c, dw = rows[:, 1], rows[:, 2] - rows[:, 1]
    assert c.min() == W and c.max() == n - W - 1 and dw.min() == -W and dw.max() == W
    fw, f0 = rows[:, [9, 11]], rows[:, [8, 10]]
    assert fw.min() == 0 and fw.max() == 4 and f0.min() == 0 and (f0 + fw <= F).all() and (f0 + fw).max() == F
    cap = min(6, int(np.floor(0.2 * n)))                                  # 5: the ratio binds
    tw, t0 = rows[:, [25, 27, 29]], rows[:, [24, 26, 28]]
    assert tw.min() == 0 and tw.max() == cap and t0.min() == 0 and (t0 + tw <= n).all() and (t0 + tw).max() == n
    short = np.array([p.draw_spec(9 * 160) for _ in range(50)])           # n = 10 = 2 W: no warp
    assert (short[:, 0] == 10).all() and not short[:, 1:3].any()
    front_end_args.src_max_len = 20                                       # n is cut to --src-max-len
    assert p.draw_spec(samples)[0] == 20


def test_draw_order_follows_the_wave_draws(front_end_args):
    from utils.data_loader import SpectrogramParser
    p = SpectrogramParser(H._conf(), normalize=True, augment=True, spec_augment=LD)
    q = SpectrogramParser(H._conf(), normalize=True, augment=True)
    np.random.seed(5)
    d = p.draw(160000)
    row = p.draw_spec(d[6])
    np.random.seed(5)
    assert q.draw(160000) == d
    n = 1 + d[6] // 160
    exp = R.row(n)
    exp[1] = int(np.random.randint(80, n - 80))
    exp[2] = exp[1] + int(np.random.randint(-80, 81))
    exp[3] = exp[4] = 2
    for k in range(2):
        exp[9 + 2 * k] = int(np.random.randint(0, 28))
        exp[8 + 2 * k] = int(np.random.randint(0, 161 - exp[9 + 2 * k] + 1))
    for k in range(2):
        exp[25 + 2 * k] = int(np.random.randint(0, 101))
        exp[24 + 2 * k] = int(np.random.randint(0, n - exp[25 + 2 * k] + 1))
    assert row == exp


def _manifest(tmp_path, n=4):
    lines = []
    rng = np.random.RandomState(0)
    for i in range(n):
        H.write_wav(tmp_path / ("u%d.wav" % i), rng.randn(3000 + 700 * i) * 2000)
        (tmp_path / ("u%d.txt" % i)).write_text("ab\n")
        lines.append("%s,%s" % (tmp_path / ("u%d.wav" % i), tmp_path / ("u%d.txt" % i)))
    (tmp_path / "m.csv").write_text("\n".join(lines))
    return str(tmp_path / "m.csv")


def _batches(ds):
    from utils.data_loader import AudioDataLoader, BucketingSampler
    np.random.seed(3)
    random.seed(3)
    out = list(AudioDataLoader(ds, num_workers=0, batch_sampler=BucketingSampler(ds, batch_size=4)))
    return out, np.random.get_state()


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("augment", [False, True])
def test_flag_off_leaves_batches_and_the_random_stream_alone(tmp_path, front_end_args, augment):
    """The option is a constructor argument: with it absent nothing is drawn and the batch has its 5 or 6 elements, whatever the
    process-wide --spec-augment says; with it present the first six elements are those same tensors and the 7th the rows."""
    from utils.data_loader import SpectrogramDataset
    man, l2i = _manifest(tmp_path), {"a": 3, "b": 4}
    assert front_end_args.spec_augment
    off, st_off = _batches(SpectrogramDataset(H._conf(), [man], l2i, normalize=True, augment=augment))
    front_end_args.spec_augment = False
    off2, st_off2 = _batches(SpectrogramDataset(H._conf(), [man], l2i, normalize=True, augment=augment, spec_augment=None))
    assert _same_state(st_off, st_off2) and len(off) == len(off2) == 1 and len(off[0]) == (6 if augment else 5)
    assert all(torch.equal(u, v) for u, v in zip(off[0], off2[0]))
    # today's stream for these four utterances: the sampler's shuffle, then per utterance the two wave draws
    np.random.seed(3)
    np.random.shuffle(list(range(4)))
    for _ in range(4 * 2 if augment else 0):
        np.random.uniform()
    assert _same_state(st_off, np.random.get_state())
    p = SpectrogramDataset(H._conf(), [man], l2i, normalize=True, augment=augment, spec_augment=None)
    np.random.seed(9)
    d = p.draw(5000)
    st = np.random.get_state()
    np.random.seed(9)
    for _ in range(2 if augment else 0):
        np.random.uniform()
    assert _same_state(st, np.random.get_state()) and d[0] == 5000

    pol = dict(LD, time_warp=3)
    on, st_on = _batches(SpectrogramDataset(H._conf(), [man], l2i, normalize=True, augment=augment, spec_augment=pol))
    assert len(on[0]) == 7 and not _same_state(st_on, st_off)
    rows = on[0][6]
    assert rows.dtype == torch.int32 and rows.shape == (4, 40)
    assert rows[:, 0].tolist() == [1 + max(int(s), 2) // 160 for s in on[0][3]]
    assert (rows[:, 1] > 0).all()
    if augment:
        assert on[0][5].dtype == torch.float64 and on[0][5].shape == (4, 6)
    else:
        assert on[0][5] is None
        assert all(torch.equal(u, v) for u, v in zip(on[0][:5], off[0]))      # no wave draws: the same utterances, order and padding


def test_validation_datasets_never_draw(tmp_path, front_end_args):
    import train
    from utils.data_loader import spec_policy
    man = _manifest(tmp_path)
    a = front_end_args
    a.train_manifest_list, a.valid_manifest_list, a.spec_time_warp = [man], [man, man], 3
    tr, valid = train.build_datasets(a, H._conf(), {"a": 3, "b": 4})
    assert tr.spec == dict(LD, time_warp=3) == spec_policy(a) and len(valid) == 2
    np.random.seed(1)
    random.seed(1)
    st = np.random.get_state()
    for v in valid:
        assert v.spec is None and not v.augmenting
        item = v[0]
        assert len(item) == 2
    assert _same_state(st, np.random.get_state())
    assert len(tr[0]) == 4 and tr[0][2] is None and len(tr[0][3]) == 40
    assert not _same_state(st, np.random.get_state())


def test_flags_parse_with_the_ld_policy_as_default():
    from utils import constant
    from utils.data_loader import spec_policy
    old = constant.args
    try:
        a = constant.parse([])
        assert not a.spec_augment and spec_policy(a) is None
        a = constant.parse(["--spec-augment"])
        assert spec_policy(a) == LD
        a = constant.parse("--spec-augment --spec-time-warp 40 --spec-freq-mask 15 --spec-freq-masks 3 --spec-time-mask 70 "
                           "--spec-time-masks 8 --spec-time-mask-ratio 0.2".split())
        assert spec_policy(a) == dict(time_warp=40, freq_mask=15, freq_masks=3, time_mask=70, time_masks=8, time_mask_ratio=0.2)
    finally:
        constant.set_args(old)


def test_start_up_checks(front_end_args):
    from utils import constant
    from utils.data_loader import SpectrogramParser
    SpectrogramParser(H._conf(), spec_augment=dict(LD, freq_masks=8, time_masks=8))
    for bad in (dict(LD, freq_masks=9), dict(LD, time_masks=9), dict(LD, time_mask=-1), dict(LD, time_mask_ratio=1.5)):
        with pytest.raises(ValueError, match="spec-"):
            SpectrogramParser(H._conf(), spec_augment=bad)
    constant.parse(["--spec-augment"])                                   # no --gpu-frontend
    with pytest.raises(NotImplementedError, match="GPU front end"):
        SpectrogramParser(H._conf(), spec_augment=LD)
    SpectrogramParser(H._conf())                                          # the flag alone asks nothing of a dataset without the option


def test_front_end_refuses_rows_of_other_frame_counts():
    from utils.audio import gpu_front_end, spec_frames
    assert spec_frames(0, 160) == 1 and spec_frames(4000, 160) == 26 and spec_frames(16000, 160, 64) == 64
    with pytest.raises(ValueError, match="frame counts"):
        gpu_front_end(torch.zeros(2, 1, 1, 4000), torch.tensor([4000, 3000]), spec=torch.tensor([R.row(26), R.row(20)]))
