"""CPU: what polygon_ribbons_device (db_text_minimal_amd.word_crops, dbn_polygon_ribbons_device of csrc/rectify.hip) decides
before it touches a device: the declared signature, the refused inputs of polygon_ribbons, a device that is no GPU, the
ribbons= keyword of rectify_words and recognize_words, and the argument errors of the raw C entry (no launch)."""
import ctypes

import numpy as np
import pytest
import torch

from db_text_minimal_amd import _lib, polygon_ribbons_device, recognize_words, rectify_words
from test_rectify_cpu import rectangle, sector


def test_the_declared_signature():
    assert _lib.SIGNATURES['dbn_polygon_ribbons_device'] == 'ppiliippppp'
    assert 'dbn_polygon_ribbons_device' not in _lib.LONG_RETURN
    assert _lib.lib().dbn_polygon_ribbons_device.restype is ctypes.c_int


def test_refused_inputs_raise_before_any_device_use():
    ok = rectangle(0, 0, 50, 10)
    for bad, kw in [(ok[:2], {}), (np.zeros((257, 2)) + ok[0], {}), (sector(90, side=4)[:7], dict(ends='half')), (ok * np.nan, {}),
                    (np.where(np.eye(4, 2) > 0, np.inf, ok), {}), (ok + 2.0 ** 20, {}), (-ok - 2.0 ** 20 - 1, {}), (ok, dict(segments=3)),
                    (ok, dict(segments=65)), (ok, dict(segments=8.5)), (ok, dict(ends='both')), (ok.reshape(-1), {}), (np.zeros((4, 3)), {})]:
        with pytest.raises(ValueError):
            polygon_ribbons_device([ok, bad], **kw)


def test_a_device_that_is_no_gpu():
    with pytest.raises(ValueError, match='GPU device'):
        polygon_ribbons_device([rectangle(0, 0, 50, 10)], device='cpu')
    with pytest.raises(ValueError, match='GPU device'):
        polygon_ribbons_device([], device='cpu')


def test_the_ribbons_keyword():
    img = torch.zeros((10, 12, 3), dtype=torch.uint8)
    poly = rectangle(1, 1, 8, 4)
    for bad in ('gpu', 1, None, 'Device'):
        with pytest.raises(ValueError, match='ribbons'):
            rectify_words(img, [[poly]], ribbons=bad)
    with pytest.raises(ValueError, match='ribbons'):
        recognize_words(img, None, None, None, polygons=[[poly]], ribbons=1)
    with pytest.raises(ValueError, match='ribbons'):
        recognize_words(img, None, None, None, polygons=[[poly]], ribbons='gpu')
    with pytest.raises(ValueError, match='GPU device'):  # the other checks still come first, on either path
        rectify_words(img, [[poly]], device='cpu', ribbons='device')
    with pytest.raises(ValueError, match='vertices'):
        rectify_words(img, [[poly[:2] + 1]], ribbons='device')


def test_the_raw_entry_refuses_without_a_launch():
    f = _lib.lib().dbn_polygon_ribbons_device
    p = 4096  # never followed: every call below is refused (or has no polygon) before a launch
    assert f(p, p, 1, 4, 3, 0, p, p, p, p, None) == 1    # segments
    assert f(p, p, 1, 4, 65, 0, p, p, p, p, None) == 1
    assert f(p, p, 1, 4, 32, 2, p, p, p, p, None) == 1   # half
    assert f(p, p, 1, 4, 32, -1, p, p, p, p, None) == 1
    assert f(p, p, -1, 4, 32, 0, p, p, p, p, None) == 1  # K
    assert f(p, p, 1, -1, 32, 0, p, p, p, p, None) == 1  # total_vertices
    for null in range(6):  # each pointer in turn
        args = [p] * 6
        args[null] = None
        assert f(args[0], args[1], 1, 4, 32, 0, args[2], args[3], args[4], args[5], None) == 1, null
    assert f(None, None, 0, 0, 32, 0, None, None, None, None, None) == 0  # no polygons: nothing to do
    assert f(None, None, 0, 0, 3, 0, None, None, None, None, None) == 1   # ... but the arguments are still checked
