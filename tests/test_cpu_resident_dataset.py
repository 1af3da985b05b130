"""The epoch plan of datacoder.ResidentDataset -- the reference's NB03#cell8 chain `.shuffle(buffer_size=len).map(read_and_encode)
.batch(B).map(augmentation_rgb_channels)` as host lists: a fresh permutation of the samples and a fresh flip draw per sample each
epoch (reference datacoder.py:337-345), one colour draw set per batch (datacoder.py:452-461), the last partial batch kept.  Pure
host work (datacoder._epoch_plan; the pools are allocated on the first write), so no GPU is needed."""
import numpy as np
import pytest

N, B = 11, 4


def _encoder(flip):
    from ssdseglib import datacoder as D
    z = np.zeros(3, np.float32)
    return D.DataEncoderDecoder(4, (6, 8), xmin_boxes_default=z, ymin_boxes_default=z, xmax_boxes_default=z + 1, ymax_boxes_default=z + 1,
                                augmentation_horizontal_flip=flip)


def _dataset(flip=True, **kw):
    """a dataset of N samples that never touches a device: nothing is written, only the sample count is set"""
    from ssdseglib import datacoder as D
    ds = D.ResidentDataset(_encoder(flip), capacity=N, batch_size=B, **kw)
    assert ds.num_samples == 0 and len(ds) == 0 and list(ds) == []
    ds.num_samples = N
    return ds


def _epoch(ds):
    batches = list(ds)
    return batches, np.concatenate([rb.index for rb in batches])


def test_every_epoch_is_a_permutation_cut_into_batches():
    ds = _dataset(seed=3)
    assert len(ds) == 3
    for _ in range(4):
        batches, order = _epoch(ds)
        assert [len(rb) for rb in batches] == [4, 4, 3]
        assert sorted(order.tolist()) == list(range(N))
        assert all(rb.index.dtype == np.int32 and rb.dataset is ds and rb.encoder is ds.encoder for rb in batches)
    dropped = _dataset(seed=3, drop_remainder=True)
    assert len(dropped) == 2
    batches, order = _epoch(dropped)
    assert [len(rb) for rb in batches] == [4, 4]
    assert len(set(order.tolist())) == 8 and set(order.tolist()) <= set(range(N))


def test_epochs_differ_and_a_seed_repeats_them():
    a, b = _dataset(seed=7, rgb_augmentation=True), _dataset(seed=7, rgb_augmentation=True)
    first, second = _epoch(a), _epoch(a)
    assert not np.array_equal(first[1], second[1])
    assert not np.array_equal(np.concatenate([rb.flip for rb in first[0]]), np.concatenate([rb.flip for rb in second[0]]))
    assert first[0][0].rgb_draws != second[0][0].rgb_draws
    for want in (first, second):                   # the same seed: the same two epochs, flips and draws included
        got = _epoch(b)
        assert np.array_equal(got[1], want[1])
        for g, w in zip(got[0], want[0]):
            assert np.array_equal(g.flip, w.flip) and g.rgb_draws == w.rgb_draws
    assert not np.array_equal(_epoch(_dataset(seed=8))[1], first[1])


def test_no_shuffle_keeps_the_order():
    ds = _dataset(shuffle=False, seed=1)
    for _ in range(2):
        batches, order = _epoch(ds)
        assert order.tolist() == list(range(N))
        assert [rb.index.tolist() for rb in batches] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]


def test_flips_follow_the_encoder():
    batches, _ = _epoch(_dataset(flip=False, seed=2))
    assert all(rb.flip is None or not rb.flip.any() for rb in batches)
    flips = np.concatenate([np.concatenate([rb.flip for rb in _epoch(ds)[0]]) for ds in [_dataset(flip=True, seed=2)] for _ in range(8)])
    assert flips.dtype == np.uint8 and set(flips.tolist()) == {0, 1}
    assert 0.25 < flips.mean() < 0.75              # 88 draws of uniform >= 0.5: outside with probability < 1e-5


def test_colour_draws_lie_in_the_reference_ranges():
    assert all(rb.rgb_draws is None for rb in _epoch(_dataset(seed=4))[0])
    ds = _dataset(seed=4, rgb_augmentation=True)
    seen = set()
    for _ in range(5):
        for rb in ds:
            hue, sat, con, bri = rb.rgb_draws
            assert -0.05 <= hue <= 0.05 and 0.95 <= sat <= 1.05 and 0.90 <= con <= 1.10 and -0.10 <= bri <= 0.10
            seen.add(rb.rgb_draws)
    assert len(seen) == 15                         # one draw set per batch, none reused


def test_the_plan_function_itself():
    from ssdseglib import datacoder as D
    plan = D._epoch_plan(np.random.default_rng(5), N, B, True, True, True, False)
    assert [p[0].size for p in plan] == [4, 4, 3] and [p[1].size for p in plan] == [4, 4, 3]
    assert all(len(p[2]) == 4 for p in plan)
    plan = D._epoch_plan(np.random.default_rng(5), N, B, False, False, False, True)
    assert [p[0].tolist() for p in plan] == [[0, 1, 2, 3], [4, 5, 6, 7]] and all(p[1] is None and p[2] is None for p in plan)
    assert D._epoch_plan(np.random.default_rng(5), 0, B, True, True, True, False) == []


def test_explicit_batches_are_checked():
    ds = _dataset(seed=6)
    rb = ds.batch([10, 0, 0], flip=[1, 0, 1], rgb_draws=(0, 1, 1, 0))
    assert rb.index.tolist() == [10, 0, 0] and rb.flip.tolist() == [1, 0, 1] and rb.rgb_draws == (0.0, 1.0, 1.0, 0.0) and len(rb) == 3
    for bad in ([-1], [N], []):
        with pytest.raises((IndexError, ValueError)):
            ds.batch(bad)
    with pytest.raises(ValueError):
        ds.batch([0, 1], flip=[1])
    with pytest.raises(ValueError):
        ds.batch([0], rgb_draws=(0.0, float("nan"), 1.0, 0.0))
    from ssdseglib import datacoder as D
    with pytest.raises(ValueError):
        D.ResidentDataset(ds.encoder, capacity=0)
    with pytest.raises(ValueError):
        D.ResidentDataset(ds.encoder, capacity=4, batch_size=0)
