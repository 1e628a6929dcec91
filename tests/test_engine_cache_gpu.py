"""The engine's cache of derived weights (engine.packs) against an engine that has cached nothing: after every way the parameters can change,
a model that has run before computes bit for bit what a model built fresh from its state computes."""
import pytest
import torch

from gpu_util import DEV
from db_text_minimal_amd import DBLoss, DBTextModel, DBTrainer, FusedAdam
from oracle import dbnet_oracle as O

pytestmark = pytest.mark.gpu

N, SIZE = 2, 128  # (every kind below is eligible at 128 x 128: the host-side dbn_*_eligible queries say so, and the last assertion checks it)


def build(arch, math, state):
    m = DBTextModel() if arch == 'resnet18' else DBTextModel(arch)
    m.load_state_dict(state)
    m = m.to(DEV)
    m.engine.set_conv_math(math)
    return m


def run(model, img, train):
    model.train(train)
    with torch.no_grad():
        return model(img).clone()


@pytest.mark.parametrize('arch,math,trains,kinds', [
    ('resnet18', 'f32', True, {'winograd', 'fold', 'combined'}),
    ('resnet18', 'bf16', True, {'stem16', 'convt16'}),
    ('resnet18', 'fp16', False, {'pw16', 'stem16', 'convt16', 'fold'}),  # (the inference mode: no train step, no train-mode forward)
    ('deformable_resnet18', 'f32', True, {'pad64', 'ohwi'})])
def test_a_cached_engine_equals_a_fresh_one_bit_for_bit(arch, math, trains, kinds):
    """Model A runs an eval forward, two train steps, an eval forward, a load_state_dict of another state and in-place edits of single
    weights (no optimizer step: only the tensors' version counters say so).  After each event model B is built fresh from A's state dict,
    with the same math: the eval maps of both are torch.equal, and so are the preds of one further train-mode forward — A's panels,
    padded / permuted / folded / combined weights were all refilled, B's made for the first time."""
    seed = 29
    img, gts = O.synthetic_batch(N, SIZE, seed=seed)
    img, gts = img.to(DEV), gts.to(DEV)
    A = build(arch, math, O.new_state(seed, arch))
    trainer = DBTrainer(A, DBLoss(), FusedAdam(A, lr=0.005)) if trains else None
    params = dict(A.named_parameters())
    edited = ['backbone.conv1.weight', 'backbone.layer1.0.conv1.weight', 'segmentation_body.reduce_conv_c2.conv.weight',
              'segmentation_body.conv.0.weight', 'segmentation_head.binarize.3.weight']
    if arch.startswith('deformable'):
        edited += ['backbone.layer2.0.conv2.weight', 'backbone.layer2.0.conv2_offset.weight']

    def eval_forward():
        run(A, img, False)

    def train_steps():
        A.train()
        for _ in range(2):
            trainer.step(img, gts)

    def load_other_state():
        A.load_state_dict(O.new_state(seed + 1, arch))

    def edit_in_place():
        with torch.no_grad():
            for k in edited:
                params[k].mul_(0.5)

    events = [eval_forward] + ([train_steps] if trains else []) + [eval_forward, load_other_state, edit_in_place]
    for event in events:
        event()
        B = build(arch, math, A.state_dict())
        for train in ((False, True) if trains else (False, )):
            a, b = run(A, img, train), run(B, img, train)
            assert a.shape == (N, 3 if train else 2, SIZE, SIZE) and bool(torch.isfinite(a).all())
            assert torch.equal(a, b), (event.__name__, 'train' if train else 'eval', float((a - b).abs().max()))
    have = {k[1] for k in A.engine.packs}
    assert kinds <= have, (kinds - have, have)
