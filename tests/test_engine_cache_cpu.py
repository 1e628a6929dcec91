"""Engine._derived / _weight_stamp: the one cache of derived weights (engine.packs[key] = (value, stamp)).  No device call: the engine of
a CPU model, plain CPU tensors and counting make / fill callables."""
import torch

from db_text_minimal_amd import DBTextModel


class Counting:
    def __init__(self, w):
        self.w, self.makes, self.fills = w, 0, 0

    def make(self):
        self.makes += 1
        return torch.zeros_like(self.w)

    def fill(self, value):
        self.fills += 1
        value.copy_(self.w.detach() * 2)

    def counts(self):
        return self.makes, self.fills


def test_derived_weight_cache_makes_once_and_refills_in_place():
    eng = DBTextModel().engine
    w = torch.arange(6.0).reshape(2, 3)
    c = Counting(w)
    key = ('layer', 'doubled')

    def get(version=None):
        return eng._derived(key, eng._weight_stamp(w, version), c.make, c.fill)

    v = get()  # first call: storage made once, filled once
    assert c.counts() == (1, 1) and torch.equal(v, w * 2)
    assert eng.packs[key][0] is v and eng.packs[key][1] == (w._version, eng.param_epoch, w.data_ptr())
    ptr = v.data_ptr()
    assert get() is v and c.counts() == (1, 1)  # same stamp: neither
    w.add_(1)  # the version counter moves: refilled, in the same storage
    v2 = get()
    assert c.counts() == (1, 2) and v2 is v and v2.data_ptr() == ptr and torch.equal(v2, w * 2)
    assert get() is v and c.counts() == (1, 2)
    eng.mark_params_dirty()  # parameters rewritten through raw pointers: refilled, in the same storage
    assert get() is v and c.counts() == (1, 3) and v.data_ptr() == ptr
    assert get() is v and c.counts() == (1, 3)


def test_version_override_replaces_the_version_counter():
    eng = DBTextModel().engine
    w = torch.ones(4)
    c = Counting(w)
    key = ('layer#fold', 'doubled')

    def get(version):
        return eng._derived(key, eng._weight_stamp(w, version), c.make, c.fill)

    v = get(('fold', 1))
    assert c.counts() == (1, 1)
    assert eng._weight_stamp(w, ('fold', 1)) == (('fold', 1), eng.param_epoch, w.data_ptr())
    w.add_(1)  # a derived tensor is rewritten through raw pointers: its own counter says nothing, and is ignored
    assert get(('fold', 1)) is v and c.counts() == (1, 1)
    assert torch.equal(v, torch.full((4, ), 2.0))  # (not refilled)
    assert get(('fold', 2)) is v and c.counts() == (1, 2) and torch.equal(v, w * 2)  # the override moves: refilled in place
    assert get(('fold', 2)) is v and c.counts() == (1, 2)


def test_reset_caches_forgets_the_storage():
    eng = DBTextModel().engine
    w = torch.ones(3)
    c = Counting(w)
    key = ('layer', 'doubled')
    v = eng._derived(key, eng._weight_stamp(w), c.make, c.fill)
    eng.bufs['x'] = torch.zeros(1)
    eng.pack_src[key] = (w, 4)
    eng._reset_caches()
    assert eng.packs == {} and eng.bufs == {} and eng.pack_src == {} and eng._pack_jobs is None
    v2 = eng._derived(key, eng._weight_stamp(w), c.make, c.fill)
    assert c.counts() == (2, 2) and v2 is not v and torch.equal(v2, w * 2)


def test_keys_do_not_share_entries():
    eng = DBTextModel().engine
    w = torch.ones(3)
    a, b = Counting(w), Counting(w)
    va = eng._derived(('layer', 'a'), eng._weight_stamp(w), a.make, a.fill)
    vb = eng._derived(('layer', 'b'), eng._weight_stamp(w), b.make, b.fill)
    assert va is not vb and a.counts() == (1, 1) and b.counts() == (1, 1)
    w.add_(1)
    eng._derived(('layer', 'a'), eng._weight_stamp(w), a.make, a.fill)
    assert a.counts() == (1, 2) and b.counts() == (1, 1)  # only the entry that was asked for is refreshed
