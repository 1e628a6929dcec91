"""CPU (-m "not gpu"): host-side logic of the drop-in surface and the C-ABI library itself
(loads, exports every symbol include/dbnet_hip.h declares; no compute calls without a GPU)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

from db_text_minimal_amd import DBLoss, DBTextModel, FusedAdam, _lib
from oracle import dbnet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_decls():
    hdr = open(os.path.join(ROOT, 'include', 'dbnet_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    return re.findall(r'int\s+(dbn_\w+)\s*\(([^)]*)\)\s*;', hdr)


def test_library_builds_loads_and_exports_every_declared_symbol():
    path = _lib.build()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    decls = header_decls()
    assert len(decls) >= 24
    for name, _ in decls:
        assert hasattr(lib, name), 'libdbnet_hip.so does not export ' + name
    hdr_longs = set(re.findall(r'long\s+(dbn_\w+)\s*\(', re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dbnet_hip.h')).read(), flags=re.S)))
    assert set(n for n, _ in decls) | hdr_longs == set(_lib.SIGNATURES), 'ctypes table and header disagree'
    for name in hdr_longs:
        assert hasattr(lib, name)


def test_every_defined_dbn_symbol_is_declared_in_the_header():
    """The reverse direction: an extern "C" dbn_* function that the library defines and the header does not declare
    would be an entry point no compiler compares with anything."""
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.build()], capture_output=True, text=True, check=True).stdout
    defined = {f[2] for f in map(str.split, out.splitlines()) if len(f) == 3 and f[1] in 'TtWw' and f[2].startswith('dbn_')}
    assert len(defined) >= 200, len(defined)
    assert not defined - set(_lib.SIGNATURES), sorted(defined - set(_lib.SIGNATURES))


# one declaration per type spelling of include/dbnet_hip.h, in the forms the header writes them
PARSER_TEXT = """
/* a comment that holds a declaration:  int dbn_in_a_comment(short x);  and spans
 * two lines */
#ifndef SOME_GUARD_H
#define SOME_GUARD_H
#ifdef __cplusplus
extern "C" {
#endif
#define DBN_SOME_CONSTANT 3
typedef struct dbn_rec {
    int* counters;
    float *a, *b;  // two pointers from one base type
    const float* w;
    void* out;
    int O, I;
    float scale;
} dbn_rec;
int dbn_none(void);
long dbn_empty();
int dbn_values(int a, long b, float c, double d);
long dbn_broken(const double* a, double* b,
                const float* c,
                float* d, const int* e, int* f);
int dbn_ints(const long long* a, long long* b, unsigned long long* c, const short* d, short* e, const unsigned short* f,
             unsigned short* g, const unsigned* h, unsigned* i);
int dbn_bytes(const unsigned char* a, unsigned char* b, const void* c, void* d, const dbn_bnb_final* fin);
#ifdef __cplusplus
}
#endif
#endif
"""
PARSER_SPELLINGS = {'int', 'long', 'float', 'double', 'const double*', 'double*', 'const float*', 'float*', 'const int*', 'int*',
                    'const long long*', 'long long*', 'unsigned long long*', 'const short*', 'short*', 'const unsigned short*',
                    'unsigned short*', 'const unsigned*', 'unsigned*', 'const unsigned char*', 'unsigned char*', 'const void*', 'void*',
                    'const dbn_bnb_final*'}


def test_header_parser_on_literal_text():
    sigs, longs, records, spellings = _lib.parse_header(PARSER_TEXT)
    assert sigs == {'dbn_none': '', 'dbn_empty': '', 'dbn_values': 'ilfd', 'dbn_broken': 'pppppp', 'dbn_ints': 'ppppppppp',
                    'dbn_bytes': 'ppppp'}
    assert longs == {'dbn_empty', 'dbn_broken'}
    assert records == {'dbn_rec': [('counters', 'p'), ('a', 'p'), ('b', 'p'), ('w', 'p'), ('out', 'p'), ('O', 'i'), ('I', 'i'),
                                   ('scale', 'f')]}
    assert spellings == PARSER_SPELLINGS and len(PARSER_SPELLINGS) == 24
    # ... and these are the spellings of the real header: a new one there needs a declaration above
    assert _lib.parse_header(open(_lib.HEADER).read())[3] == PARSER_SPELLINGS


@pytest.mark.parametrize('decl', ['int dbn_f(int a, short n);', 'int dbn_f(unsigned n);', 'int dbn_f(size_t n, void* p);',  # unknown by value
                                  'int dbn_f(int);', 'int dbn_f(int a[4]);', 'void dbn_f(int a);', 'int dbn_f(int a) { return a; }',
                                  'typedef struct dbn_r { short n; } dbn_r;', 'typedef struct dbn_r { int n; } dbn_s;'])
def test_header_parser_refuses_what_it_does_not_know(decl):
    with pytest.raises(_lib.HipLibraryError, match='dbn_f|dbn_r'):
        _lib.parse_header('int dbn_before(int a);\n' + decl + '\nint dbn_after(void);\n')


def test_missing_header_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, 'HEADER', str(tmp_path / 'include' / 'dbnet_hip.h'))
    with pytest.raises(_lib.HipLibraryError, match=re.escape(str(tmp_path / 'include' / 'dbnet_hip.h'))):
        _lib._read_header()


def test_real_entries_against_hand_written_expectations():
    """Frozen copies of six rows of the hand-written table this module held before the header became the one declaration,
    and the sizes of the four records."""
    frozen = {'dbn_head_tail_bn_bwd_t': 'ii' + 'p' * 28 + 'iiii' + 'ff' + 'pp',
              'dbn_db_loss_fwd': 'pp' + 'iiii' + 'ffdf' + 'pppp',
              'dbn_jpeg_dhuff_ws_bytes': 'l',
              'dbn_adam_step': 'pppp' + 'l' + 'ffff' + 'i' + 'f' + 'p',
              'dbn_rectify_u8': 'plpppiiiiplp',
              'dbn_head_tail_bwd_ws_floats': ''}
    for name, kinds in frozen.items():
        assert _lib.SIGNATURES[name] == kinds, name
    assert {n for n in frozen if n in _lib.LONG_RETURN} == {'dbn_jpeg_dhuff_ws_bytes'}
    assert [ctypes.sizeof(r) for r in (_lib.WgradReduceJob, _lib.PackJob, _lib.WinogradPackJob, _lib.BnbFinal)] == [72, 48, 32, 72]
    assert [f for f, _ in _lib.PackJob._fields_] == ['w', 'out', 'O', 'I', 'R', 'S', 'mode', 'Cs', 'Cd', 'f']
    L = _lib.lib()
    assert L.dbn_jpeg_dhuff_ws_bytes.restype is ctypes.c_long and L.dbn_adam_step.restype is ctypes.c_int
    assert L.dbn_db_loss_fwd.argtypes[8] is ctypes.c_double and L.dbn_adam_step.argtypes[4] is ctypes.c_long


def test_compiler_compares_the_header_with_the_definitions(tmp_path):
    """csrc/common.h includes the header, so a definition that disagrees with its declaration does not compile: a copy of
    one small unit passes the host syntax check as it is and stops with `conflicting types` once one parameter type of a
    function it defines is changed in the copied header."""
    csrc = tmp_path / 'db_text_minimal_amd' / 'csrc'
    csrc.mkdir(parents=True)
    for f in ('mfma_probe.hip', 'common.h'):
        shutil.copy(os.path.join(_lib.CSRC, f), csrc)
    shutil.copytree(os.path.join(ROOT, 'include'), tmp_path / 'include')
    make = open(os.path.join(_lib.CSRC, 'Makefile')).read()
    hipcc, std = re.search(r'^HIPCC \?= (\S+)', make, re.M).group(1), re.search(r'-std=\S+', make).group(0)

    def syntax_check():
        return subprocess.run([hipcc, '--cuda-host-only', '-fsyntax-only', std, 'mfma_probe.hip'], cwd=csrc, capture_output=True, text=True)

    res = syntax_check()
    assert res.returncode == 0, res.stderr[-2000:]
    hdr = tmp_path / 'include' / 'dbnet_hip.h'
    text = hdr.read_text()
    decl = 'long dbn_mfma_sustained_flops(int kind, int iters);'
    assert text.count(decl) == 1
    hdr.write_text(text.replace(decl, 'long dbn_mfma_sustained_flops(int kind, long iters);'))
    res = syntax_check()
    assert res.returncode != 0 and "conflicting types for 'dbn_mfma_sustained_flops'" in res.stderr, res.stderr[-2000:]


def test_no_module_imports_a_siblings_private_name():
    """What the image-pipeline stages share is public in packed.py: no module of the package brings in an underscore-prefixed name
    from a sibling other than _lib, and packed.py itself imports nothing from the package but _lib, so every stage can import it."""
    import ast
    pkg = os.path.join(ROOT, 'db_text_minimal_amd')
    modules = sorted(f for f in os.listdir(pkg) if f.endswith('.py'))
    assert 'packed.py' in modules and len(modules) >= 15
    seen = 0
    for f in modules:
        for node in ast.walk(ast.parse(open(os.path.join(pkg, f)).read(), f)):
            if isinstance(node, ast.ImportFrom) and node.level >= 1:
                seen += 1
                sibling = node.module or ''  # `from . import x`: the names are the siblings
                private = [a.name for a in node.names if a.name.startswith('_') and not (sibling == '' and a.name == '_lib')]
                assert sibling == '_lib' or not private, '%s: from .%s import %s' % (f, sibling, ', '.join(private))
                if f == 'packed.py':
                    assert sibling == '_lib' or [a.name for a in node.names] == ['_lib'], 'packed.py imports from .%s' % sibling
            elif isinstance(node, (ast.Import, ast.ImportFrom)) and f == 'packed.py':
                names = [node.module] if isinstance(node, ast.ImportFrom) else [a.name for a in node.names]
                assert not any(n.split('.')[0] == 'db_text_minimal_amd' for n in names), names
    assert seen >= 30  # (the walk still finds the relative imports)


def test_size_queries_without_gpu():
    L = _lib.lib()
    assert L.dbn_igemm_packed_floats(7 * 7 * 4, 64) == 208 * 64  # K=196 padded to 208
    assert L.dbn_igemm_panel_floats(64, 3, 7, 7, 0, 2) == 208 * 64
    # 3x3 stride-2 data gradient: parity classes with 4 + 2 + 2 + 1 = 9 taps, no padding waste for Cs=128
    assert L.dbn_igemm_panel_floats(128, 64, 3, 3, 1, 2) == 9 * 128 * 64
    assert L.dbn_igemm_panel_floats(128, 64, 3, 3, 1, 1) == 9 * 128 * 64
    assert L.dbn_reduce_ws_floats(512) == 1024 * 2 * 512
    # bs16 640x640 shapes: FPN conv / head convs use the 128x128 tile, Cout=64 layers 256x64
    assert L.dbn_igemm_tile_config(409600, 256) == 1
    assert L.dbn_igemm_tile_config(409600, 64) in (2, 3, 4)  # (round 3: the 64x64 tile, see dbn_igemm_tile_config)
    sk = L.dbn_wgrad_splitk(16, 160, 160, 64, 64, 3, 3)
    assert 1 <= sk <= 409600 // 256


def test_state_dict_keys_shapes_match_reference_layout():
    m = DBTextModel()
    sd = m.state_dict()
    spec = O.state_spec()
    assert list(sd.keys()) == [k for k, _, _ in spec]  # 211 keys, reference order
    for k, shape, kind in spec:
        assert tuple(sd[k].shape) == tuple(shape), k
    assert sum(p.numel() for p in m.parameters()) == 13306922
    assert m.name == 'resnet18_FPN_DBHead'  # models.py:31-32
    m2 = DBTextModel()
    m2.load_state_dict(O.new_state(3))
    for k, v in O.new_state(3).items():
        assert torch.equal(m2.state_dict()[k], v), k


def test_reference_init_statistics():
    """Init follows the reference: resnet.py:197-203 (conv N(0, sqrt(2/(k*k*Cout))), BN 1/0),
    segmentation_head.py:47-53 (kaiming_normal_, BN w=1 b=1e-4)."""
    torch.manual_seed(0)
    m = DBTextModel()
    w = m.backbone.layer2[0].conv1.weight
    assert abs(float(w.detach().std()) - (2.0 / (9 * 128))**0.5) < 2e-3
    assert float(m.backbone.bn1.weight.min()) == 1 and float(m.backbone.bn1.bias.abs().max()) == 0
    hw = m.segmentation_head.binarize[0].weight
    assert abs(float(hw.std()) - (2.0 / (256 * 9))**0.5) < 1e-3
    ct = m.segmentation_head.thresh[3].weight  # ConvTranspose2d: fan_in = Cout*k*k
    assert abs(float(ct.std()) - (2.0 / (64 * 4))**0.5) < 5e-3
    assert abs(float(m.segmentation_head.binarize[4].bias[0]) - 1e-4) < 1e-9
    assert m.segmentation_head.thresh[0].bias is None and m.segmentation_head.binarize[0].bias is not None


def test_no_cpu_fallback_and_error_surface():
    m = DBTextModel()
    with pytest.raises(RuntimeError, match='HIP device'):
        m(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match='only holds parameters'):
        m.backbone.conv1(torch.zeros(1, 3, 8, 8))
    crit = DBLoss()
    with pytest.raises(RuntimeError, match='MI355X only'):
        crit(torch.rand(1, 3, 8, 8), torch.rand(4, 1, 8, 8))
    with pytest.raises(AssertionError):
        crit(torch.rand(3, 8, 8), torch.rand(4, 1, 8, 8))  # losses.py:113-114
    with pytest.raises(ValueError):
        DBLoss(reduction='bogus')  # F.binary_cross_entropy's error for an unknown reduction string (losses.py:30)
    assert DBLoss(reduction='sum').reduction == 'sum'
    with pytest.raises(NotImplementedError):
        FusedAdam(m, weight_decay=0.1)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'db_text_minimal_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                src = open(os.path.join(dirpath, f)).read()
                assert 'oracle' not in src.replace('the CPU oracle', ''), os.path.join(dirpath, f)


def test_every_environment_name_the_package_reads_is_documented():
    """Every DBN_* name that a module of the package reads through os.environ is listed in INTEGRATION.md."""
    pkg = os.path.join(ROOT, 'db_text_minimal_amd')
    reads = re.compile(r"""os\.environ(?:\.get\(|\.pop\(|\[)\s*['"](DBN_[A-Z0-9_]+)['"]|['"](DBN_[A-Z0-9_]+)['"]\s+(?:not\s+)?in\s+os\.environ""")
    names = set()
    for f in sorted(os.listdir(pkg)):
        if f.endswith('.py'):
            for m in reads.finditer(open(os.path.join(pkg, f)).read()):
                names.add(m.group(1) or m.group(2))
    assert {'DBN_POISON', 'DBN_FOLD_EVAL_BN', 'DBN_LIB_PATH', 'DBN_STEP_GRAPH'} <= names, names  # (the expression still finds the reads)
    documented = set(re.findall(r'DBN_[A-Z0-9_]+', open(os.path.join(ROOT, 'INTEGRATION.md')).read()))
    assert not names - documented, sorted(names - documented)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'nope.so'))
    monkeypatch.setattr(_lib, '_lib', None)
    with pytest.raises(_lib.HipLibraryError):
        _lib.lib()


def test_kernel_selection_logic_without_gpu():
    """Host-side dispatch rules (no device call): which convolutions / weight gradients take the pixel-patch and transposing-read
    kernels, and that the tile configuration reported for a call is the one its BatchNorm partial rows are sized for."""
    L = _lib.lib()
    cfg = lambda at, ns, kmode, N, H, W, Cs, Cd, R, s, p: L.dbn_igemm_kernel_config(at, ns, kmode, N, H, W, Cs, H // s, W // s, Cd, R, R, s, p, 0, 1)
    # 3x3 / stride 1 on whole 8 x 16 patches of 32-channel blocks takes the pixel-patch form in the 16-bit matrix modes; exact fp32
    # (round 4, 128 x 64 tiles) on request only (tile 3 / dbn_set_patch_conv(3): measured, not faster inside the step)
    assert cfg(0, 0, 0, 16, 160, 160, 64, 64, 3, 1, 1) == 4 and cfg(0, 0, 0, 16, 160, 160, 256, 64, 3, 1, 1) == 4
    assert L.dbn_igemm_kernel_config(0, 0, 0, 16, 160, 160, 64, 160, 160, 64, 3, 3, 1, 1, 3, 1) == 19
    for at, ns in ((0, 3), (0, 1), (1, 1), (2, 1)):
        c = cfg(at, ns, 0, 16, 160, 160, 64, 64, 3, 1, 1)
        assert c & 16 and (c & 15) == 3, (at, ns, c)                    # 128 x 64 patch tiles
        assert cfg(at, ns, 1, 16, 80, 80, 128, 128, 3, 1, 1) & 16        # data gradient too
        assert cfg(at, ns, 0, 16, 40, 40, 256, 256, 3, 1, 1) & 16 == 0   # W % 16 != 0
        assert cfg(at, ns, 0, 16, 160, 160, 64, 64, 1, 1, 0) & 16 == 0   # 1x1
        assert cfg(at, ns, 0, 16, 160, 160, 64, 128, 3, 2, 1) & 16 == 0  # stride 2
        assert cfg(at, ns, 0, 16, 160, 160, 16, 64, 3, 1, 1) & 16 == 0   # Cs % 32 != 0
    wcfg = lambda at, ns, O, Cb, R, s, p, H, W: L.dbn_wgrad_kernel_config_hw(at, ns, O, Cb, R, R, s, p, H // s, W // s, H, W)
    assert wcfg(0, 0, 64, 64, 3, 1, 1, 160, 160) & 48 == 0              # exact fp32: the register-transposing kernel
    assert wcfg(1, 1, 64, 64, 3, 1, 1, 160, 160) & 32                   # bf16, 3x3 / stride 1: pixel patches
    assert wcfg(0, 3, 64, 256, 3, 1, 1, 160, 160) & 32                  # bf16x3 on fp32 tensors
    assert wcfg(1, 1, 128, 64, 3, 2, 1, 160, 160) & 48 == 16            # stride 2 on bf16 tensors: LDS-DMA + transposing reads
    assert wcfg(1, 1, 64, 4, 7, 2, 3, 640, 640) & 48 == 0               # the stem (Cb = 4): register-transposing kernel
    assert wcfg(1, 1, 256, 256, 3, 1, 1, 40, 40) & 48 == 16             # W % 16 != 0: no patch form
    assert L.dbn_igemm_kernel_config(0, 0, 0, 16, 160, 160, 64, 160, 160, 64, 3, 3, 1, 1, 4, 1) == 4  # an explicit 64 x 64 tile stays on the gather loop
    try:
        assert L.dbn_set_patch_conv(0) == 1
        assert cfg(1, 1, 0, 16, 160, 160, 64, 64, 3, 1, 1) & 16 == 0 and cfg(0, 0, 0, 16, 160, 160, 64, 64, 3, 1, 1) & 16 == 0
        assert L.dbn_set_patch_conv(2) == 0  # 2: the 16-bit matrix modes only
        assert cfg(1, 1, 0, 16, 160, 160, 64, 64, 3, 1, 1) & 16 and cfg(0, 0, 0, 16, 160, 160, 256, 64, 3, 1, 1) & 16 == 0
        assert L.dbn_set_patch_conv(3) == 2  # 3: exact fp32 on every eligible launch
        assert cfg(0, 0, 0, 16, 160, 160, 64, 64, 3, 1, 1) == 19
    finally:
        L.dbn_set_patch_conv(1)


def _run_bench(*argv, env_drop=('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')):
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in env_drop}
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(argv), env=env, capture_output=True, text=True, timeout=600)


def test_bench_gpus_n_launches_n_ranks_itself():
    """`python bench.py --gpus N` with no torch.distributed.run environment (how the driver may invoke it) must produce an N-rank
    run or fail — round 3 silently ran one rank and printed n_gpus: 1.  The dry run (no GPU work, gloo) exercises exactly the
    self-launch: a fresh `torch.distributed.run --nproc-per-node 2` child, the rendezvous on 127.0.0.1, ONE all-reduce of a
    49 MB flat buffer per step through train.allreduce_flat_grads, rank 0's single JSON line forwarded with the child's code."""
    import json
    r = _run_bench('--gpus', '2', '--steps', '2', '--warmup', '0', '--dry', '--backend', 'gloo')
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout  # exactly one JSON line on stdout
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2 and line['config']['parallelism'] == 'dp2' and line['config']['global_batch'] == 32
    dp = line['data_parallel']
    assert dp['world_seen'] == 2 and dp['allreduce_mean_ok'] and 'self-launched' in dp['launched_by']


def test_bench_refuses_more_gpus_than_visible_and_wrong_world_size():
    """No silent fallback to fewer ranks: this container has no GPU, so --gpus 2 (RCCL) must exit with code 2 before anything is
    launched; an external launch whose WORLD_SIZE disagrees with --gpus must fail as well."""
    r = _run_bench('--gpus', '2', '--steps', '1', '--warmup', '0')
    assert r.returncode == 2 and 'GPU(s) visible' in r.stderr, (r.returncode, r.stderr[-500:])
    assert not r.stdout.strip()
    import subprocess
    env = dict(os.environ, WORLD_SIZE='1', RANK='0', LOCAL_RANK='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--dry', '--backend', 'gloo'], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'WORLD_SIZE=1' in (r.stderr + r.stdout)


def test_bench_dump_outputs_fits_the_budget_and_samples_the_same_elements(tmp_path):
    """bench.py --dump-outputs: float32 .npy files of at most 64 MB in all; maps larger than that (16x3x640x640 fp32) are a sample
    whose indices depend only on the shape, so two runs (two builds) compare element for element; small maps are written whole."""
    import numpy as np
    import bench
    g = torch.Generator().manual_seed(0)
    preds, losses = torch.rand(16, 3, 640, 640, generator=g), torch.rand(5, generator=g)
    info = bench.dump_outputs(str(tmp_path / 'a'), preds, losses)
    bench.dump_outputs(str(tmp_path / 'b'), preds.clone(), losses.clone())
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == ['losses.npy', 'preds.npy'] and info['preds_sampled']
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= 64 * 10**6
    for f in files:
        a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert a.dtype == np.float32 and np.array_equal(a, b)
    p = np.load(tmp_path / 'a' / 'preds.npy')
    assert np.isin(p[:1000], preds.numpy().ravel()).all()
    np.testing.assert_array_equal(np.load(tmp_path / 'a' / 'losses.npy'), losses.numpy())
    small = torch.rand(2, 3, 64, 64, generator=g)
    assert bench.dump_outputs(str(tmp_path / 'c'), small, losses)['preds_sampled'] is None
    np.testing.assert_array_equal(np.load(tmp_path / 'c' / 'preds.npy'), small.numpy().ravel())


def test_bench_refuses_zero_steps():
    r = _run_bench('--steps', '0', '--dry', '--backend', 'gloo')
    assert r.returncode != 0 and '--steps' in r.stderr
