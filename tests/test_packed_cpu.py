"""CPU (-m "not gpu"): the packed-batch helpers every image-pipeline stage shares (db_text_minimal_amd/packed.py): the layout
arithmetic, the checks with their callers' wording, the collate halves and the base of the two decode-error families."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import jpeg as J
from db_text_minimal_amd import packed as Pk
from db_text_minimal_amd import png as P

SHAPES = [(37, 53), (64, 64), (101, 67)]


def test_offsets_of_empty_single_and_zero_sized_entries():
    for got, want in ((Pk.offsets([]), [0]), (Pk.offsets([7]), [0, 7]), (Pk.offsets([5, 0, 3]), [0, 5, 5, 8])):
        assert got.dtype == np.int64 and got.tolist() == want
    assert Pk.image_offsets([]).tolist() == [0]
    assert Pk.image_offsets([(2, 5)]).tolist() == [0, 30]
    off = Pk.image_offsets([(37, 53), (0, 0), (101, 67)])  # an image that was not decoded takes no bytes
    assert off.dtype == np.int64 and off.tolist() == [0, 37 * 53 * 3, 37 * 53 * 3, 37 * 53 * 3 + 101 * 67 * 3]
    assert Pk.image_offsets([(np.int32(65535), np.int32(65535))] * 2).tolist() == [0, 65535 * 65535 * 3, 2 * 65535 * 65535 * 3]  # past 2^32


def test_check_shape_limits():
    assert Pk.check_shape((1, Pk.MAX_SIDE, 3)) == (1, 65535) and Pk.check_shape(torch.Size([4, 5, 3])) == (4, 5)
    for bad in ((0, 5), (5, 0), (65536, 1)):
        with pytest.raises(ValueError, match='outside 1 .. 65535'):
            Pk.check_shape(bad)


def test_as_images_takes_one_image_or_a_collated_batch():
    one = torch.arange(4 * 5 * 3, dtype=torch.uint8).reshape(4, 5, 3)
    packed, shapes = Pk.as_images(one)
    assert shapes == [(4, 5)] and packed.dim() == 1 and torch.equal(packed, one.reshape(-1))
    packed, shapes = Pk.as_images(one.permute(1, 0, 2))  # a view that is not contiguous: its bytes in [H, W, 3] order
    assert shapes == [(5, 4)] and torch.equal(packed.view(5, 4, 3), one.permute(1, 0, 2))
    need = sum(h * w * 3 for h, w in SHAPES)
    flat = torch.zeros(need, dtype=torch.uint8)
    packed, shapes = Pk.as_images((flat, [np.array(s) for s in SHAPES], [[]] * 3, [[]] * 3))  # image_collate's tuple, extras ignored
    assert packed is flat and shapes == SHAPES and all(type(v) is int for s in shapes for v in s)
    assert Pk.as_images([flat, SHAPES])[1] == SHAPES
    with pytest.raises(ValueError, match='a single image must be a uint8'):
        Pk.as_images(one.float())
    with pytest.raises(ValueError, match='a single image must be a uint8'):
        Pk.as_images(one[..., :2])
    with pytest.raises(ValueError, match='the packed images must be a flat uint8 tensor'):
        Pk.as_images((flat.to(torch.int8), SHAPES))
    with pytest.raises(ValueError, match='the packed images must be a flat uint8 tensor'):
        Pk.as_images((flat.reshape(1, -1), SHAPES))
    for n in (need - 1, need + 1):
        with pytest.raises(ValueError, match='the packed images hold %d bytes, the shapes need %d' % (n, need)):
            Pk.as_images((torch.zeros(n, dtype=torch.uint8), SHAPES))
    with pytest.raises(ValueError, match='images must be .packed uint8 tensor, shapes.'):
        Pk.as_images((flat.numpy(), SHAPES))
    with pytest.raises(ValueError, match='outside 1 .. 65535'):
        Pk.as_images((flat, [(0, 5)]))


def test_the_size_check_speaks_with_its_callers_words():
    Pk.check_bytes(12, 12)
    with pytest.raises(ValueError, match='^packed holds 11 bytes, the shapes need 12$'):
        Pk.check_bytes(11, 12)
    with pytest.raises(ValueError, match='^packed_u8 holds 13 bytes, the shapes need 12$'):
        Pk.check_bytes(13, 12, 'packed_u8 holds')
    with pytest.raises(ValueError, match='^the packed images hold 12 bytes, the shapes need 12$'):
        Pk.check_bytes(12, 12, 'the packed images hold', flat=False)
    need = sum(h * w * 3 for h, w in SHAPES)
    for n in (need - 1, need + 1):
        with pytest.raises(ValueError, match='^packed_u8 holds %d bytes, the shapes need %d$' % (n, need)):
            Pk.packed_on(torch.zeros(n, dtype=torch.uint8), SHAPES, 'cpu')
    with pytest.raises(ValueError, match=r'^packed_u8 must be a flat uint8 tensor \(image_collate\)$'):
        Pk.packed_on(torch.zeros(need, dtype=torch.int16), SHAPES, 'cpu')
    flat = torch.zeros(need, dtype=torch.uint8)
    assert Pk.packed_on(flat, SHAPES, 'cpu') is flat


def test_flat_u8_covers_the_encoders_and_the_device_only_stages():
    a = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    for src in (a, torch.from_numpy(a), torch.from_numpy(a).permute(1, 0, 2), a[:, ::2]):
        got = Pk.flat_u8(src, 'cpu')
        assert got.dim() == 1 and got.dtype == torch.uint8 and got.tolist() == np.asarray(src).reshape(-1).tolist()
    for bad in (a.astype(np.int16), torch.zeros(3), [a]):
        with pytest.raises(ValueError, match='images must be uint8 tensors or arrays'):
            Pk.flat_u8(bad, 'cpu')
    for bad in (a, torch.zeros(4, dtype=torch.uint8)):  # without a device to go to: a host array or tensor has no path
        with pytest.raises(ValueError, match=r'^out must be a tensor on a GPU device \(there is no host path\)$'):
            Pk.flat_u8(bad, what='out')


def test_cuda_device_refuses_what_is_not_a_gpu_in_the_callers_name():
    with pytest.raises(ValueError, match='^rendering runs on a GPU device, not cpu$'):
        Pk.cuda_device('rendering', 'cpu')
    with pytest.raises(ValueError, match='^crop_words runs on a GPU device, not cpu$'):
        Pk.cuda_device('crop_words', torch.device('cpu'), torch.zeros(1))
    assert Pk.cuda_device('x', 'cuda:3') == torch.device('cuda', 3)  # an index given is kept, and no GPU is asked for one
    assert Pk.cuda_device('x', torch.device('cuda', 1), torch.zeros(1)) == torch.device('cuda', 1)


def test_pin_default_and_polys_tags():
    assert Pk.pin_default(True) is True and Pk.pin_default(False) is False and Pk.pin_default(0) is False
    assert Pk.pin_default() is torch.cuda.is_available()  # not a DataLoader worker here
    items = [(None, [[[0, 0], [4, 0], [4, 2], [0, 2]], np.arange(6).reshape(3, 2)], ['a', '###']), (None, [[1, 2, 3, 4, 5, 6]], None), (None, [], None)]
    polys, tags = Pk.polys_tags(items)
    assert [[p.shape for p in ps] for ps in polys] == [[(4, 2), (3, 2)], [(3, 2)], []] and all(p.dtype == np.float64 for ps in polys for p in ps)
    assert polys[1][0].tolist() == [[1, 2], [3, 4], [5, 6]]
    assert tags == [['a', '###'], [None], []]  # tags=None: one None per polygon
    tags[0].append('x')
    assert items[0][2] == ['a', '###']  # a copy, not the item's own list


FAMILIES = [(J.JpegError, J.UnsupportedJpeg, J.CorruptJpeg, J.REASONS, (3, 4, 5, 6, 7, 8, 9, 14)),
            (P.PngError, P.UnsupportedPng, P.CorruptPng, P.REASONS, (20, 21))]


@pytest.mark.parametrize('base, unsupported, corrupt, reasons, refused', FAMILIES, ids=['jpeg', 'png'])
def test_both_decode_error_families_share_one_base(base, unsupported, corrupt, reasons, refused):
    assert issubclass(base, Pk.DecodeError) and issubclass(base, ValueError) and issubclass(unsupported, base) and issubclass(corrupt, base)
    assert tuple(base.refused) == refused
    for code, text in reasons.items():
        e = base.of(code, 2)
        assert type(e) is (unsupported if code in refused else corrupt)
        assert (e.code, e.index, e.reason) == (code, 2, text) and str(e) == 'image 2: ' + text
        again = type(e)(e.code, 5)  # how decode_image_batch re-indexes an error
        assert type(again) is type(e) and (again.code, again.index, again.reason) == (code, 5, text) and str(again) == 'image 5: ' + text
        assert str(base.of(code)) == text and base.of(code).index is None
    e = base.of(99, 0)
    assert type(e) is corrupt and e.reason == 'status 99' and str(e) == 'image 0: status 99'
    assert type(unsupported(np.int32(refused[0]), 1).code) is int


def test_the_multiscan_status_still_resolves():
    e = J.JpegError.of(14, 3)
    assert type(e) is J.UnsupportedJpeg and e.reason == J.MULTISCAN_REASONS[14] and 14 not in J.REASONS
    assert str(type(e)(e.code, 5)) == 'image 5: ' + J.MULTISCAN_REASONS[14]
    assert J.JpegError(3).reason != P.PngError(3).reason and P.PngError.of(14).reason == 'status 14'  # each family reads its own table


def test_decoded_batches_share_shapes_len_and_errors():
    class Obj(Pk.DecodedBatch):
        error, _hw = P.PngError, (1, 0)
        desc, status = np.array([[53, 37], [9, 9], [67, 101]]), np.array([0, 20, 6], np.int32)
    o = Obj()
    assert len(o) == 3 and o.shapes == [(37, 53), (0, 0), (0, 0)] and all(type(v) is int for s in o.shapes for v in s)
    errs = o.errors()
    assert errs[0] is None and type(errs[1]) is P.UnsupportedPng and type(errs[2]) is P.CorruptPng and [e.index for e in errs[1:]] == [1, 2]
    with pytest.raises(P.UnsupportedPng, match='image 1: '):
        o.raise_errors()
    o.status = np.zeros(3, np.int32)
    assert o.raise_errors() is None and o.errors() == [None] * 3
    assert issubclass(J.JpegCoefficients, Pk.DecodedBatch) and issubclass(J.JpegStreams, Pk.DecodedBatch) and issubclass(P.PngScanlines, Pk.DecodedBatch)
    assert J.JpegCoefficients.error is J.JpegError and P.PngScanlines.error is P.PngError
