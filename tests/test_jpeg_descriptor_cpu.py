"""CPU (-m "not gpu"): the one reader of a JPEG descriptor (csrc/jpeg_common.h read_scan), pinned through the two host entry
points that run it, dbn_jpeg_huff_plan and dbn_jpeg_encode_batch: the kernels run the very same function.  Valid descriptors
come from forward_plan (grey, 4:4:4, 4:2:2, 4:2:0 at 1 x 1, 8 x 8, 9 x 17 and 65535 x 1); then one rule is broken at a time and
both entry points must refuse the image with the status they have always given: 1 where the descriptor's own status is not
0, 2 for everything else, except a coefficient offset that is no multiple of 8, which only the device coder's plan minds."""
import numpy as np
import pytest

from db_text_minimal_amd import jpeg as J
from db_text_minimal_amd._lib import check, lib

KINDS = {'grey': (1, '444'), '444': (3, '444'), '422': (3, '422'), '420': (3, '420')}
SIZES = [(1, 1), (8, 8), (9, 17), (65535, 1)]  # (W, H)
COMP, STATUS = 6, 22  # fields of a descriptor: 4 per component {bw, bh, h, v} from 6, the status


@pytest.fixture(scope='module')
def valid():
    """[(name, desc int64 [1, 24], qtabs, coefficients, (hs, vs), blocks the size and the sampling give)], built once and only
    when this file is selected"""
    out = []
    for kind, (nc, sub) in KINDS.items():
        for W, H in SIZES:
            desc, qtabs, total, _, _ = J.forward_plan([(0, H, W, nc)], sub, J.quant_tables(75))
            hs, vs = J.SUBSAMPLING[sub] if nc == 3 else (1, 1)
            blocks = -(-W // (8 * hs)) * -(-H // (8 * vs)) * (hs * vs + 2 if nc == 3 else 1)
            assert total == blocks * 64
            out.append(('%s %dx%d' % (kind, W, H), desc, qtabs, total, (hs, vs), blocks))
    return out


@pytest.fixture(scope='module')
def bufs(valid):
    """(zero coefficients with room for every changed grid below, so that only the broken rule can refuse an image; an output
    buffer: 416 bytes are what a block can take, 704 the header)"""
    return np.zeros(2 * max(v[3] for v in valid), np.int16), np.empty(max(v[5] for v in valid) * 416 + 1024, np.uint8)


def plan(desc, qtabs, coef_elems):
    """dbn_jpeg_huff_plan of one descriptor -> (status, blocks)"""
    blk, ivl, status, sizes = np.zeros(2, np.int64), np.zeros(2, np.int64), np.full(1, -1, np.int32), np.zeros(2, np.int64)
    check(lib().dbn_jpeg_huff_plan(desc.ctypes.data, qtabs.ctypes.data, 1, int(coef_elems), 0, blk.ctypes.data, ivl.ctypes.data,
                                   status.ctypes.data, sizes.ctypes.data), 'jpeg_huff_plan')
    return int(status[0]), int(blk[1])


def encode(bufs, desc, qtabs, coef_elems):
    """dbn_jpeg_encode_batch of one descriptor over zero coefficients -> (status, length of the stream)"""
    coef, out = bufs
    offs, lens, status = np.array([0, out.size], np.int64), np.zeros(1, np.int64), np.full(1, -1, np.int32)
    assert coef_elems <= coef.size
    check(lib().dbn_jpeg_encode_batch(coef.ctypes.data, int(coef_elems), desc.ctypes.data, qtabs.ctypes.data, 1, 0, out.ctypes.data, out.size,
                                      offs.ctypes.data, lens.ctypes.data, status.ctypes.data, 1), 'jpeg_encode_batch')
    return int(status[0]), int(lens[0])


def test_valid_descriptors_are_taken_with_the_blocks_their_size_and_sampling_give(valid, bufs):
    for name, desc, qtabs, total, _, blocks in valid:
        assert plan(desc, qtabs, total) == (0, blocks), name
        s, n = encode(bufs, desc, qtabs, total)
        assert s == 0 and n > 0, name


def _regrid(d, W, H, h, v):
    """the grids a three-component (or, with one, a grey) image would have with luma sampling h x v and 1 x 1 chroma"""
    mcux, mcuy = -(-W // (8 * h)), -(-H // (8 * v))
    d[COMP:COMP + 4] = mcux * h, mcuy * v, h, v
    for c in range(1, int(d[3])):
        d[COMP + 4 * c:COMP + 4 * c + 4] = mcux, mcuy, 1, 1


# name -> (which valid descriptors it applies to, change(d, W, H, total) -> coefficient count to pass (None: all of the buffer), status
#          of the plan, status of the host coder)
def _status(d, W, H, total): d[STATUS] = 3
def _w0(d, W, H, total): d[1] = 0
def _w65536(d, W, H, total): d[1] = 65536
def _nc2(d, W, H, total): d[3] = 2
def _luma22(d, W, H, total): _regrid(d, W, H, 2, 2)
def _luma12(d, W, H, total): _regrid(d, W, H, 1, 2)
def _chroma21(d, W, H, total): d[COMP + 4], d[COMP + 6] = 2 * d[COMP + 4], 2
def _bw(d, W, H, total): d[COMP] += 1
def _bh(d, W, H, total): d[COMP + 1] += 1
def _negative(d, W, H, total): d[0] = -8
def _past_end(d, W, H, total): return total - 1
def _unaligned(d, W, H, total): d[0] = 4


VIOLATIONS = {
    'status not 0': ('all', _status, 1, 1), 'W = 0': ('all', _w0, 2, 2), 'W = 65536': ('all', _w65536, 2, 2),
    'nc = 2': ('all', _nc2, 2, 2), 'luma 2x2 on a grey image': ('grey', _luma22, 2, 2), 'luma 1x2': ('colour', _luma12, 2, 2),
    'chroma 2x1': ('colour', _chroma21, 2, 2), 'bw off by one': ('all', _bw, 2, 2), 'bh off by one': ('all', _bh, 2, 2),
    'coef negative': ('all', _negative, 2, 2), 'coef + blocks * 64 = coef_elems + 1': ('all', _past_end, 2, 2),
    'coef not a multiple of 8': ('all', _unaligned, 2, 0),
}


@pytest.mark.parametrize('violation', list(VIOLATIONS))
def test_one_violation_at_a_time_is_refused_with_its_status(violation, valid, bufs):
    which, change, want_plan, want_host = VIOLATIONS[violation]
    tried = 0
    for name, desc, qtabs, total, _, _ in valid:
        nc = int(desc[0, 3])
        if (which == 'grey' and nc != 1) or (which == 'colour' and nc != 3):
            continue
        d = desc.copy()
        n = change(d[0], int(desc[0, 1]), int(desc[0, 2]), total)
        n = bufs[0].size if n is None else n
        assert plan(d, qtabs, n) == (want_plan, 0), name  # a refused image gets no blocks
        assert encode(bufs, d, qtabs, n)[0] == want_host, name
        tried += 1
    assert tried >= 4
