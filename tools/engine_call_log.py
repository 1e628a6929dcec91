"""Record every call an Engine makes into libdbnet_hip.so, in a form two revisions of the host code can be compared by.

One line per call of `engine.L`: the function name, every scalar argument verbatim, every pointer argument replaced by the ordinal of
that address's first appearance in the log ('-' for a null pointer), and the return value.  The ordinals keep which arguments alias
(same buffer, same panel, same stream) and drop the addresses, which differ from process to process.  A host-side refactor of
engine.py must leave these logs identical line for line: same launches, same order, same operands.

    python tools/engine_call_log.py record --root <tree> --out <dir>    # writes <dir>/<case>.log for the four cases below
    python tools/engine_call_log.py compare <dir A> <dir B>             # per-case call counts and the verdict (exit status 1: they differ)

`--root` is the tree whose db_text_minimal_amd package (with its built library) is imported; the oracle comes from this repository.

`--cases pipeline` (record and compare) is a second group for the image pipeline, whose modules all reach the library through
_lib.lib(): one seeded script over three small images (decode, colour jitter, augment, crops, recogniser input, drawing, encode), run
from a host-resident and from a device-resident packed batch.  There the caching allocator decides which addresses alias, not the
host code, so a pointer is logged by null-ness only ('-' or '*'); and after each public call the sha256 of everything it returned.
"""
import argparse
import collections
import ctypes
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

# (case, backbone, conv math, what runs: 'e' an eval forward, 't' a train step); 2 x 3 x 128 x 128, seeded.  The second and third step of
# a case exercise the batched repack of the weight panels.
CASES = [('resnet18_f32', 'resnet18', 'f32', 'ettte'),
         ('resnet18_bf16', 'resnet18', 'bf16', 'ettte'),
         ('resnet18_fp16', 'resnet18', 'fp16', 'ee'),
         ('deformable_resnet50_f32', 'deformable_resnet50', 'f32', 'ttte')]
PIPELINE_CASES = ['pipeline_host', 'pipeline_device']  # where the packed batch lives when the script starts
PIPELINE_SIZES = [(37, 53), (64, 64), (101, 67)]  # odd sizes, rows that are no multiple of 4 bytes


class Recorder:
    """Stands in for the ctypes library object of an Engine."""

    def __init__(self, lib, signatures, out, ordinals=True):
        self._lib, self._sig, self._out, self._ordinal, self._ordinals = lib, signatures, out, {}, ordinals

    def _pointer(self, a):
        if a is None or (not self._ordinals and a == 0):
            return '-'
        if not self._ordinals:
            return '*'
        if not isinstance(a, int):  # ctypes.byref(record): the record's address
            a = ctypes.addressof(a._obj)
        return '#%d' % self._ordinal.setdefault(a, len(self._ordinal))

    def __getattr__(self, name):
        fn, sig = getattr(self._lib, name), self._sig[name]

        def call(*args):
            rc = fn(*args)
            assert len(args) == len(sig), name
            self._out.write('%s(%s) -> %d\n' % (name, ', '.join(self._pointer(a) if k == 'p' else repr(a) for a, k in zip(args, sig)), rc))
            return rc
        self.__dict__[name] = call
        return call


def record(root, out_dir):
    sys.path.insert(0, root)
    sys.path.append(REPO)
    import torch
    from db_text_minimal_amd import DBLoss, DBTextModel, DBTrainer, FusedAdam, _lib
    from oracle import dbnet_oracle as O
    assert os.path.dirname(os.path.abspath(_lib.__file__)) == os.path.join(os.path.abspath(root), 'db_text_minimal_amd'), _lib.__file__
    os.makedirs(out_dir, exist_ok=True)
    for case, arch, math, script in CASES:
        seed = 31
        img, gts = O.synthetic_batch(2, 128, seed=seed)
        img, gts = img.to('cuda:0'), gts.to('cuda:0')
        model = DBTextModel() if arch == 'resnet18' else DBTextModel(arch)
        model.load_state_dict(O.new_state(seed, arch))
        model = model.to('cuda:0')
        eng = model.engine
        eng.set_conv_math(math)
        trainer = DBTrainer(model, DBLoss(), FusedAdam(model, lr=0.005)) if 't' in script else None
        with open(os.path.join(out_dir, case + '.log'), 'w') as f:
            eng.L = Recorder(eng.L, _lib.SIGNATURES, f)
            for what in script:
                f.write('# %s\n' % ('eval forward' if what == 'e' else 'train step'))
                if what == 'e':
                    model.eval()
                    with torch.no_grad():
                        model(img)
                else:
                    model.train()
                    trainer.step(img, gts)
            torch.cuda.synchronize()
        print('recorded', case, flush=True)


def digest(v):
    """sha256 of every tensor, array and byte string in a call's result, in order; anything else verbatim"""
    import numpy as np
    import torch
    if isinstance(v, torch.Tensor):
        a = v.detach().cpu().contiguous()
        v = a.view(torch.uint8).numpy() if a.numel() else np.zeros(0, np.uint8)
        return 'tensor %s %s %s' % (str(a.dtype), list(a.shape), hashlib.sha256(v.tobytes()).hexdigest())
    if isinstance(v, np.ndarray):
        return 'array %s %s %s' % (v.dtype, list(v.shape), hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest())
    if isinstance(v, (bytes, bytearray)):
        return 'bytes %d %s' % (len(v), hashlib.sha256(bytes(v)).hexdigest())
    if isinstance(v, (list, tuple)):
        return '[' + ', '.join(digest(x) for x in v) + ']'
    return repr(v)


def pipeline_script(db, call, resident):
    """The image pipeline end to end on three seeded images; `call(name, fn, *args, **kw)` runs one public function and logs it."""
    import numpy as np
    import torch
    dev = torch.device('cuda:0')
    golden = os.path.join(REPO, 'tests', 'golden')
    jz, pz = np.load(os.path.join(golden, 'jpeg_cases.npz')), np.load(os.path.join(golden, 'png_cases.npz'))
    mixed = [jz['jpeg_12'].tobytes(), pz['png_20'].tobytes(), jz['jpeg_26'].tobytes(), pz['png_0'].tobytes(), jz['jpeg_19'].tobytes()]
    call('decode_image_batch', db.decode_image_batch, mixed, dev)
    rng = np.random.RandomState(31)
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in PIPELINE_SIZES]
    quads = [np.array([[[3, 4], [w - 9, 6], [w - 7, h // 2], [5, h // 2 - 3]], [[w // 3, h // 2], [w - 2, h // 2 + 2], [w - 4, h - 3], [w // 3 + 1, h - 5]],
                       [[0, 0]] * 4], np.int16) for h, w in PIPELINE_SIZES]  # two boxes per image and an all-zero one, which is dropped
    packed, shapes, _, _ = db.image_collate([(im, [], []) for im in images])
    on_dev = packed.to(dev)
    if resident == 'device':
        packed = on_dev
    batch = (packed, shapes)
    with_contrast = [[('brightness', 1.25), ('contrast', 0.75)], [('hue', 0.125)], [('saturation', 1.5), ('contrast', 1.125), ('hue', -0.25)]]
    without = [[('brightness', 0.5)], [], [('hue', 0.25), ('saturation', 0.25)]]
    call('color_jitter_images contrast', db.color_jitter_images, on_dev, shapes, with_contrast)  # (this stage has no host path)
    call('color_jitter_images', db.color_jitter_images, on_dev, shapes, without)
    polys = [[q[0].astype(np.float64), q[1].astype(np.float64)] for q in quads]
    plans = db.plan_augment(shapes, polys, np.random.RandomState(7), 160)
    call('augment_images training', db.augment_images, packed, shapes, plans, 160, device=dev)
    call('augment_images letterbox', db.augment_images, packed, shapes, None, 160, device=dev)
    first = on_dev[:shapes[0][0] * shapes[0][1] * 3].view(shapes[0][0], shapes[0][1], 3)
    call('preprocess_image', db.preprocess_image, first, 96)
    call('preprocess_image pad', db.preprocess_image, first, 96, pad=True)
    crops, _ = call('crop_words', db.crop_words, batch, quads, device=dev)
    call('rectify_words', db.rectify_words, batch, [list(q) for q in quads], device=dev)
    call('rectify_words device ribbons', db.rectify_words, batch, [list(q) for q in quads], device=dev, ribbons='device')
    call('words_to_input', db.words_to_input, crops)
    call('words_to_input rgb', db.words_to_input, crops, rgb=True, dtype=torch.bfloat16)
    labels = [[('word %d' % n, (4, 20 + 9 * n)), ('Qy~', (w // 2, h - 6))] for n, (h, w) in enumerate(PIPELINE_SIZES)]
    dots = [[(5, 5), (w - 3, h // 2)] for h, w in PIPELINE_SIZES]
    prob = torch.from_numpy(np.random.RandomState(5).rand(3, 1, 40, 48).astype(np.float32)).to(dev)
    outlined = call('draw_outlines', db.draw_outlines, batch, quads, device=dev)
    call('draw_outlines thin', db.draw_outlines, batch, quads, (0, 255, 0), 1, device=dev)
    for name, fn, args, kw in (('draw_labels', db.draw_labels, (labels, ), dict(background=(0, 0, 64), height=9)),
                               ('draw_dots', db.draw_dots, (dots, ), {}),
                               ('overlay_heatmap', db.overlay_heatmap, (prob, ), dict(valid_hw=[(40, 48), (33, 48), (40, 31)]))):
        call(name, fn, batch, *args, **kw)
        call(name + ' in place', fn, batch, *args, out=outlined.clone(), **kw)
    call('overlay_heatmap limits', db.overlay_heatmap, batch, prob, vmin=0.25, vmax=0.75, cmap='jet', binary=0.5)
    call('encode_jpeg_batch', db.encode_jpeg_batch, packed, shapes, device=dev)
    call('encode_jpeg_batch device entropy', db.encode_jpeg_batch, packed, shapes, quality=90, subsampling='444', device=dev, entropy='device')
    call('encode_png_batch', db.encode_png_batch, packed, shapes, device=dev)


def record_pipeline(root, out_dir):
    sys.path.insert(0, root)
    import torch
    import db_text_minimal_amd as db
    from db_text_minimal_amd import _lib
    assert os.path.dirname(os.path.abspath(_lib.__file__)) == os.path.join(os.path.abspath(root), 'db_text_minimal_amd'), _lib.__file__
    os.makedirs(out_dir, exist_ok=True)
    real = _lib.lib()
    for case in PIPELINE_CASES:
        with open(os.path.join(out_dir, case + '.log'), 'w') as f:
            def call(name, fn, *args, **kw):
                f.write('# %s\n' % name)
                res = fn(*args, **kw)
                f.write('= %s\n' % digest(res))
                return res
            _lib._lib = Recorder(real, _lib.SIGNATURES, f, ordinals=False)  # every pipeline module calls through _lib.lib()
            try:
                pipeline_script(db, call, case.split('_')[1])
                torch.cuda.synchronize()
            finally:
                _lib._lib = real
        print('recorded', case, flush=True)


def compare(dir_a, dir_b, cases):
    same = True
    print('%-26s %10s %10s %10s  %s' % ('case', 'calls A', 'calls B', 'functions', 'verdict'))
    for case in cases:
        logs = []
        for d in (dir_a, dir_b):
            with open(os.path.join(d, case + '.log')) as f:
                logs.append(f.read().splitlines())
        a, b = logs
        calls = [[ln for ln in log if not ln.startswith(('#', '='))] for log in logs]
        names = collections.Counter(ln.split('(')[0] for ln in calls[0])
        verdict = 'identical'
        if a != b:
            same = False
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            verdict = 'DIFFER at line %d' % (first + 1)
            for log in logs:
                print('    ', log[first] if first < len(log) else '<end of log>')
        print('%-26s %10d %10d %10d  %s' % (case, len(calls[0]), len(calls[1]), len(names), verdict))
    print('verdict: the two logs are %s' % ('identical line for line' if same else 'NOT identical'))
    return 0 if same else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    r = sub.add_parser('record')
    r.add_argument('--root', default=REPO)
    r.add_argument('--out', required=True)
    c = sub.add_parser('compare')
    c.add_argument('dirs', nargs=2)
    for p in (r, c):
        p.add_argument('--cases', choices=('engine', 'pipeline'), default='engine', help='the four engine cases, or the image pipeline')
    a = ap.parse_args()
    if a.cmd == 'record':
        (record if a.cases == 'engine' else record_pipeline)(a.root, a.out)
    else:
        sys.exit(compare(*a.dirs, [c[0] for c in CASES] if a.cases == 'engine' else PIPELINE_CASES))
