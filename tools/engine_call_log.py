"""Record every call an Engine makes into libdbnet_hip.so, in a form two revisions of the host code can be compared by.

One line per call of `engine.L`: the function name, every scalar argument verbatim, every pointer argument replaced by the ordinal of
that address's first appearance in the log ('-' for a null pointer), and the return value.  The ordinals keep which arguments alias
(same buffer, same panel, same stream) and drop the addresses, which differ from process to process.  A host-side refactor of
engine.py must leave these logs identical line for line: same launches, same order, same operands.

    python tools/engine_call_log.py record --root <tree> --out <dir>    # writes <dir>/<case>.log for the four cases below
    python tools/engine_call_log.py compare <dir A> <dir B>             # per-case call counts and the verdict (exit status 1: they differ)

`--root` is the tree whose db_text_minimal_amd package (with its built library) is imported; the oracle comes from this repository.
"""
import argparse
import collections
import ctypes
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


class Recorder:
    """Stands in for the ctypes library object of an Engine."""

    def __init__(self, lib, signatures, out):
        self._lib, self._sig, self._out, self._ordinal = lib, signatures, out, {}

    def _pointer(self, a):
        if a is None:
            return '-'
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


def compare(dir_a, dir_b):
    same = True
    print('%-26s %10s %10s %10s  %s' % ('case', 'calls A', 'calls B', 'functions', 'verdict'))
    for case, _, _, _ in CASES:
        logs = []
        for d in (dir_a, dir_b):
            with open(os.path.join(d, case + '.log')) as f:
                logs.append(f.read().splitlines())
        a, b = logs
        calls = [[ln for ln in log if not ln.startswith('#')] for log in logs]
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
    a = ap.parse_args()
    if a.cmd == 'record':
        record(a.root, a.out)
    else:
        sys.exit(compare(*a.dirs))
