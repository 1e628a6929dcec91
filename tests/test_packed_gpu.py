"""-m gpu: a stage told to run on a device that is not the current one enters it for its launches (packed.on_device), as the
decode and encode stages always did: the result lies on that device and holds the bytes of the same call made there."""
import numpy as np
import pytest
import torch

from db_text_minimal_amd import augment_images, crop_words, draw_outlines, image_collate, plan_augment

SIZES = [(37, 53), (64, 64), (101, 67)]


def small_batch():
    rng = np.random.RandomState(31)
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]
    quads = [np.array([[[3, 4], [w - 9, 6], [w - 7, h // 2], [5, h // 2 - 3]], [[w // 3, h // 2], [w - 2, h // 2 + 2], [w - 4, h - 3], [w // 3 + 1, h - 5]]],
                      np.int16) for h, w in SIZES]
    packed, shapes, _, _ = image_collate([(im, [], []) for im in images])
    return packed, shapes, quads


@pytest.mark.gpu
@pytest.mark.parametrize('resident', ['host', 'cuda:1'])
def test_stages_run_on_the_device_they_are_given_when_another_is_current(resident):
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two visible devices')
    packed, shapes, quads = small_batch()
    if resident != 'host':
        packed = packed.to(resident)
    plans = plan_augment(shapes, [[q[0].astype(np.float64), q[1].astype(np.float64)] for q in quads], np.random.RandomState(7), 160)
    target = torch.device('cuda:1')
    calls = {'augment_images': lambda: augment_images(packed, shapes, plans, 160, device='cuda:1'),
             'crop_words': lambda: crop_words((packed, shapes), quads, device='cuda:1')[0],
             'draw_outlines': lambda: draw_outlines((packed, shapes), quads, device='cuda:1')}
    with torch.cuda.device(1):
        want = {name: fn() for name, fn in calls.items()}
        torch.cuda.synchronize()
    with torch.cuda.device(0):
        assert torch.cuda.current_device() == 0
        got = {name: fn() for name, fn in calls.items()}
        assert torch.cuda.current_device() == 0  # left as it was found
        torch.cuda.synchronize(1)
    for name in calls:
        assert got[name].device == target and want[name].device == target, name
        assert got[name].numel() > 0 and torch.equal(got[name], want[name]), name
    assert float(want['crop_words'].float().std()) > 0 and not torch.equal(want['draw_outlines'], packed.to(target))  # (something was drawn)
