"""Host half of ssdseglib/_loaders.py: the ground-truth padding every loader shares."""
import numpy as np
import pytest


def _rows(rng, k):
    return rng.uniform(0, 100, (k, 5)).astype(np.float32)


def test_pad_ground_truth():
    from ssdseglib._loaders import _EncodingLoader, _pad_ground_truth
    gmax = _EncodingLoader.GMAX
    assert gmax == 64
    rng = np.random.default_rng(3)
    rows = [_rows(rng, 0), _rows(rng, gmax), _rows(rng, 3)]         # no box at all, a full image, a few
    gt, cnt = _pad_ground_truth(rows, 3, gmax)
    assert gt.shape == (3, gmax, 5) and gt.dtype == np.float32 and gt.flags.c_contiguous
    assert cnt.shape == (3,) and cnt.dtype == np.int32 and cnt.tolist() == [0, gmax, 3]
    assert not gt[0].any()
    np.testing.assert_array_equal(gt[1], rows[1])
    np.testing.assert_array_equal(gt[2, :3], rows[2])
    assert not gt[2, 3:].any()
    gt, cnt = _pad_ground_truth([np.asarray(_rows(rng, 2), np.float64)], 1, 4)      # rows of another float type are cast
    assert gt.dtype == np.float32 and gt.shape == (1, 4, 5) and cnt.tolist() == [2]
    with pytest.raises(ValueError, match=str(gmax)):
        _pad_ground_truth([_rows(rng, 1), _rows(rng, gmax + 1)], 2, gmax)
