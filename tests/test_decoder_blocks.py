"""The decoder-block catalogue (tests/decoder_blocks.py) checked on the CPU
oracle alone, under the default table: the conditions that make the GPU tests
of tests/test_gpu_decoder_input.py meaningful."""
import numpy as np
import pytest

import decoder_blocks as D

DENSE_SPARSE = ["%s-%d" % (k, a) for k in ("dense", "sparse") for a in D.AMPLITUDES]
ALL_CLASSES = ["zero", "dc", "basis", "worst-sign"] + DENSE_SPARSE


@pytest.fixture(scope="module")
def pixels(oracle):
    """(blocks, classes, reference fp32 pixels per block (n, 64))"""
    cat, classes = D.catalogue(oracle.default_transform())
    n = len(cat)
    assert n == D.SIZE and n % 128 == 0
    h, w = n // 128 * 8, 1024
    r = oracle.idct(D.plane_of(cat, h, w))
    return cat, classes, r.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(n, 64)


def test_catalogue_shape_and_classes(oracle, pixels):
    cat, classes, _ = pixels
    assert cat.dtype == np.int16 and cat.shape == (D.SIZE, 64) and D.SIZE <= 1024
    assert set(classes) == set(ALL_CLASSES)
    assert set(classes[:D.FIRST]) == set(ALL_CLASSES)         # the 24 x 1016 frame sees every class
    count = {c: classes.count(c) for c in ALL_CLASSES}
    assert count["zero"] == 1 and count["dc"] == 10 and count["basis"] == 384 and count["worst-sign"] == 2
    # deterministic: a second build gives the same list
    D._memo.clear()
    again, classes2 = D.catalogue(oracle.default_transform())
    assert np.array_equal(again, cat) and classes2 == classes


def test_fixed_classes_hold_what_they_say(pixels):
    cat, classes, _ = pixels
    by = {c: cat[[i for i, k in enumerate(classes) if k == c]] for c in ALL_CLASSES}
    assert not by["zero"].any()
    assert sorted(by["dc"][:, 0].tolist()) == sorted(D.DC_VALUES) and not by["dc"][:, 1:].any()
    assert ((by["basis"] != 0).sum(axis=1) == 1).all()
    seen = {(int(np.flatnonzero(b)[0]), int(b[np.flatnonzero(b)[0]])) for b in by["basis"]}
    assert seen == {(p, v) for p in range(64) for v in D.BASIS_VALUES}
    assert cat.max() == 32767 and cat.min() == -32768
    ws = by["worst-sign"]
    assert np.array_equal(ws[0], -ws[1]) and set(np.abs(ws).reshape(-1).tolist()) <= {0, 32767}
    for a in D.AMPLITUDES:
        d, s = by["dense-%d" % a].astype(np.int64), by["sparse-%d" % a].astype(np.int64)
        assert d.min() >= -a and d.max() < a and s.min() >= -a and s.max() < a
        assert 0.05 < (s != 0).mean() < 0.15


def test_reference_pixels_cover_the_clamp(pixels):
    _, classes, r = pixels
    assert np.isfinite(r).all()                                # the default table overflows nowhere
    inside = ((r > 0) & (r < 255)).mean()
    low, high = (r <= 0).mean(), (r >= 255).mean()
    print("pixels inside (0, 255): %.3f, <= 0: %.3f, >= 255: %.3f" % (inside, low, high))
    assert inside >= 0.20 and low >= 0.20 and high >= 0.20
    assert (r == 254).any() and (r == 256).any()               # DC 63 and 64: either side of the clamp's edge
    assert ((r > 0) & (r < 1e-5)).any()                        # DC -64: 7.6e-6, truncates to 0 without clamping
    for c in DENSE_SPARSE:
        x = r[[i for i, k in enumerate(classes) if k == c]]
        assert (x != np.floor(x)).any(), c
