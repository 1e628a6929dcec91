"""ctypes binding of libdbnet_hip.so (the C ABI declared in include/dbnet_hip.h).

The product path has no CPU or PyTorch-op fallback: if the HIP library is
missing or fails to load, importing a compute entry point raises.
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# DBN_LIB_PATH: a test vehicle built from the same sources (make RACE=1 -> libdbnet_hip_race.so, csrc/common.h); the default is the product
LIB_PATH = os.environ.get('DBN_LIB_PATH') or os.path.join(_HERE, 'libdbnet_hip.so')
CSRC = os.path.join(_HERE, 'csrc')

HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'dbnet_hip.h')

# argument kinds: p = device/host pointer, i = int, l = long, f = float, d = double
_KIND = {'p': ctypes.c_void_p, 'i': ctypes.c_int, 'l': ctypes.c_long, 'f': ctypes.c_float, 'd': ctypes.c_double}
_BY_VALUE = {'int': 'i', 'long': 'l', 'float': 'f', 'double': 'd'}


class HipLibraryError(RuntimeError):
    pass


def _declarator(text, where, base=None):
    """'const float* w' -> ('const float', 1, 'w'); with the `base` of an earlier declarator of the same member list, '*b' -> (base, 1, 'b')"""
    toks = re.findall(r'\w+|\S', text)
    words = [t for t in toks if t != '*']
    stars = len(toks) - len(words)
    well_formed = (all(re.fullmatch(r'\w+', w) for w in words)  # type words, then the stars, then the name
                   and (len(words) > 1 if base is None else len(words) == 1) and toks == words[:-1] + ['*'] * stars + words[-1:])
    if not well_formed:
        raise HipLibraryError('%s: cannot split the declaration %r' % (where, ' '.join(text.split())))
    return (' '.join(words[:-1]) if base is None else base), stars, words[-1]


def parse_header(text):
    """The C ABI as include/dbnet_hip.h declares it -> (signatures, long_return, records, spellings):
    signatures   function name -> argument kinds, one letter of _KIND each
    long_return  the names that return long (all others return int)
    records      typedef'd struct name -> [(member, kind)] in declaration order
    spellings    every type spelling met, e.g. 'const float*'
    By value only int, long, float and double are known; a type ending in * is a pointer.  Anything else raises HipLibraryError:
    there is no default kind."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)
    signatures, long_return, records, spellings = {}, set(), {}, set()

    def kind(base, stars, where):
        spellings.add(base + '*' * stars)
        if stars:
            return 'p'
        if base not in _BY_VALUE:
            raise HipLibraryError('%s: by-value type %r is not one of %s' % (where, base, ', '.join(_BY_VALUE)))
        return _BY_VALUE[base]

    def record(m):
        name, fields = m.group(1), []
        if m.group(3) != name:
            raise HipLibraryError('typedef struct %s is named %s' % (name, m.group(3)))
        for member in filter(str.strip, m.group(2).split(';')):
            base = None
            for piece in member.split(','):
                base, stars, field = _declarator(piece, 'struct ' + name, base)
                fields.append((field, kind(base, stars, 'struct ' + name)))
        records[name] = fields
        return ' '

    text = re.sub(r'typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;', record, text)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r'\1', text, flags=re.S)
    for stmt in filter(str.strip, text.split(';')):
        m = re.fullmatch(r'\s*(int|long)\s+(dbn_\w+)\s*\(([^()]*)\)\s*', stmt)
        if m is None:
            raise HipLibraryError('cannot split the declaration %r' % ' '.join(stmt.split()))
        ret, name, params = m.groups()
        if name in signatures:
            raise HipLibraryError('%s is declared twice' % name)
        params = [] if params.strip() in ('', 'void') else params.split(',')
        signatures[name] = ''.join(kind(*_declarator(prm, name)[:2], name) for prm in params)
        if ret == 'long':
            long_return.add(name)
    return signatures, long_return, records, spellings


def _read_header():
    try:
        with open(HEADER) as f:
            return f.read()
    except OSError as e:
        raise HipLibraryError('cannot read the C ABI header %s: %s' % (HEADER, e))


# name -> argument kinds; the names returning long; the members of the ABI's records: all from the one declaration, the header
SIGNATURES, LONG_RETURN, RECORDS, _ = parse_header(_read_header())


def _fields(record):
    return [(member, _KIND[k]) for member, k in RECORDS[record]]


class WgradReduceJob(ctypes.Structure):
    """dbn_wgrad_reduce_job of include/dbnet_hip.h: one layer's slab reduction, for dbn_wgrad_reduce_many."""
    _fields_ = _fields('dbn_wgrad_reduce_job')


class PackJob(ctypes.Structure):
    """dbn_pack_job: one weight panel of dbn_pack_weights_batched's device job table."""
    _fields_ = _fields('dbn_pack_job')


class WinogradPackJob(ctypes.Structure):
    """dbn_winograd_pack_job: one Winograd panel of dbn_winograd_pack_batched's device job table."""
    _fields_ = _fields('dbn_winograd_pack_job')


class WinogradPlan(ctypes.Structure):
    """dbn_winograd_plan of include/dbnet_hip.h: what dbn_winograd_describe reports (forms, rows, groups, splits; nothing is launched)."""
    _fields_ = _fields('dbn_winograd_plan')


class BnbFinal(ctypes.Structure):
    """dbn_bnb_final of include/dbnet_hip.h: the in-kernel finalize of a data gradient's BatchNorm-backward sums."""
    _fields_ = _fields('dbn_bnb_final')


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 into libdbnet_hip.so (hipcc cross-compiles without a GPU)."""
    res = subprocess.run(['make', '-C', CSRC, '-j8'], capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode != 0:
        raise HipLibraryError('building libdbnet_hip.so failed (see output above)')
    return LIB_PATH


def source_stamp():
    """sha256 over the kernel sources (csrc/*.hip, *.h, Makefile, sorted by name): recorded beside profile summaries
    (tools/pmc_traffic.py) so that bench.py can tell whether a committed per-kernel figure still describes these kernels."""
    import hashlib
    h = hashlib.sha256()
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.h')) or name == 'Makefile':
            h.update(name.encode())
            with open(os.path.join(CSRC, name), 'rb') as f:
                h.update(f.read())
    return h.hexdigest()[:16]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError('%s not found: run `python -c "import __graft_entry__ as g; g.build()"` '
                                  '(there is no CPU fallback for the DBNet hot path)' % LIB_PATH)
        try:
            l = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise HipLibraryError('cannot load %s: %s' % (LIB_PATH, e))
        for name, sig in SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if the symbol is missing
            fn.argtypes = [_KIND[k] for k in sig]
            fn.restype = ctypes.c_long if name in LONG_RETURN else ctypes.c_int
        _lib = l
    return _lib


def check(rc, what=''):
    if rc != 0:
        if rc == 1:
            raise RuntimeError('libdbnet_hip: invalid argument in %s' % what)
        raise RuntimeError('libdbnet_hip: %s failed with hipError %d' % (what, rc - 1000))
