"""The float64 reference of the deformable sampling adjoints (tests/deform_ref.py) pinned without a GPU: adjoint64 (autograd of the oracle)
against an independent loop restatement, the exactness premise of every case that tests/test_deform_adjoint_gpu.py compares bit for bit,
and the conditions that keep those cases from passing on nothing."""
import numpy as np
import pytest
import torch

import deform_ref as D

DT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
EPS64 = 2.0**-52


def stored(t, at):
    return t.to(DT[at]).float()


@pytest.mark.parametrize('shape', [(2, 64, 9, 11, 1), (1, 128, 12, 10, 2)])
def test_adjoint64_agrees_with_the_loops_on_gaussian_data(shape):
    """Two derivations of one sum (autograd of gathers | a scatter loop; d(offset) per corner | from the four corner values): they differ by
    float64 rounding only, |a - b| <= 4 * 2^-52 * sum |addends| per element, the sum taken from the loop version."""
    N, C, H, W, stride = shape
    Ho, Wo = D.out_size(H, W, stride)
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, H, W, C, generator=g)
    off = torch.randn(N, Ho, Wo, 18, generator=g) * 1.5
    dcols = torch.randn(N, Ho, Wo, 9, C, generator=g)
    dx, do = D.adjoint64(x, off, dcols, stride)
    ldx, ldo, sdx, sdo = D.adjoint_loops(x, off, dcols, stride)
    assert float(np.abs(ldx).max()) > 1 and float(np.abs(ldo).max()) > 1
    for name, a, b, s in (('dx', dx, ldx, sdx), ('doffset', do, ldo, sdo)):
        err = np.abs(a.numpy() - b)
        bound = 4 * EPS64 * s
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print('%s %s: max err %.3e, worst err / bound %.3f' % (name, shape, float(err.max()), worst))
        assert bool((err <= bound).all()), (name, shape, worst)


def check_premise(tag, x, off, dcols, stride):
    """adjoint32 == adjoint64 == the loops, bit for bit, and per element 16 sum |dx addends| < 2^24, 4 sum |doffset addends| < 2^24 (the sums
    from the loop version): all partial sums of the 1/16- and 1/4-multiples are float32 numbers, whatever the order."""
    assert bool((x == x.round()).all()) and float(x.abs().max()) <= 4
    assert bool((dcols == dcols.round()).all()) and float(dcols.abs().max()) <= 4
    assert bool((off * 4 == (off * 4).round()).all()), tag + ': an offset is no multiple of 1/4'
    dx64, do64 = D.adjoint64(x, off, dcols, stride)
    dx32, do32 = D.adjoint32(x, off, dcols, stride)
    assert dx32.dtype == torch.float32 and dx64.dtype == torch.float64
    assert torch.equal(dx32.double(), dx64), tag + ': dx differs between float32 and float64'
    assert torch.equal(do32.double(), do64), tag + ': doffset differs between float32 and float64'
    ldx, ldo, sdx, sdo = D.adjoint_loops(x, off, dcols, stride)
    assert np.array_equal(ldx, dx64.numpy()) and np.array_equal(ldo, do64.numpy()), tag + ': the loops differ from adjoint64'
    assert 16 * float(sdx.max()) < 2.0**24 and 4 * float(sdo.max()) < 2.0**24, (tag, float(sdx.max()), float(sdo.max()))
    assert bool((dx64 * 16 == (dx64 * 16).round()).all()) and bool((do64 * 4 == (do64 * 4).round()).all())
    # (the weights are not negative: the loops' sum |w g| is the dx of |dcols|, which is how the grid cases below get it)
    assert np.array_equal(sdx, D.adjoint64(x, off, dcols.abs(), stride)[0].numpy())
    return float(np.abs(ldx).max()), float(np.abs(ldo).max())


@pytest.mark.parametrize('si,name', D.EXACT_CASES)
def test_exactness_premise(si, name):
    """Every (shape, generator) pair the GPU file declares exact, on the offsets as each storage type holds them (rounding to bf16 / fp16
    moves the far offsets and leaves multiples of 1/4)."""
    shape = D.SHAPES[si]
    seen = []
    for at in (0, 1, 2):
        x, off, dcols = D.exact_case(shape, name, at)
        so = stored(off, at)
        assert bool((so * 4 == (so * 4).round()).all()), 'a stored offset is no multiple of 1/4'
        assert torch.equal(stored(x, at), x) and torch.equal(stored(dcols, at), dcols)
        if any(torch.equal(so, t) for t in seen):
            continue  # the same stored case as an earlier storage type
        seen.append(so)
        mdx, mdo = check_premise('%s %s at=%d' % (shape, name, at), x, so, dcols, shape[4])
        print('%s %s at=%d: max |dx| %.4g, max |doffset| %.4g' % (shape, name, at, mdx, mdo))
        assert mdx > 0 and mdo > 0


@pytest.mark.parametrize('shape', D.GRID_CASES)
def test_exactness_premise_of_the_grid_cases(shape):
    """The two 100 x 100 cases (the loops would take minutes there): float32 == float64 bit for bit, image by image;
    16 sum |dx addends| from the dx of |dcols| (equal to the loops' sum: test_exactness_premise asserts that on every small case); and
    every doffset element is a sum of 4 C addends |g v (1 - l | l)| <= 4 * 4 * 1, so 4 sum <= 64 C * 4 < 2^24."""
    N, C, H, W, stride = shape
    x, off, dcols = D.grid_case(shape)
    for at in (0, 1):
        so = stored(off, at)
        assert bool((so * 4 == (so * 4).round()).all())
        assert float(so.abs().max()) < D.emax_of(H, W)  # the finite window
        if at == 1 and torch.equal(so, off):
            continue
        step = max(1, 8 * 64 // (C * 4))  # images per slice (keeps the float64 graph near 1 GB)
        for n in range(0, N, step):
            sl = slice(n, n + step)
            dx64, do64 = D.adjoint64(x[sl], so[sl], dcols[sl], stride)
            dx32, do32 = D.adjoint32(x[sl], so[sl], dcols[sl], stride)
            assert torch.equal(dx32.double(), dx64) and torch.equal(do32.double(), do64), (shape, at, n)
            sdx = D.adjoint64(x[sl], so[sl], dcols[sl].abs(), stride)[0]
            assert 16 * float(sdx.max()) < 2.0**24
    assert 4 * (4 * C * 16) < 2.0**24


# ---- vacuity: the cases hold what they are meant to hold -------------------------------------------------------------------------------
def classes(p, E, far):
    c = {'-1': p == -1, '(-1,0)': (p > -1) & (p < 0), '0': p == 0, 'E-1': p == E - 1, '(E-1,E)': (p > E - 1) & (p < E), 'E': p == E}
    if far:
        c['far'] = p.abs() > 2 * E + 8
    return c


@pytest.mark.parametrize('name', ['edges', 'edges_near'])
@pytest.mark.parametrize('si', range(len(D.SHAPES)))
def test_edges_hold_every_position_class(si, name):
    shape = D.SHAPES[si]
    N, C, H, W, stride = shape
    Ho, Wo = D.out_size(H, W, stride)
    x, off, dcols = D.exact_case(shape, name)
    py, px = D.positions(off, H, W, stride)
    omax = float(off.abs().max())
    if name == 'edges':
        assert omax >= H + W + 3  # the gather searches the whole map
    else:
        assert omax < D.emax_of(H, W)  # the finite window
    if N * Ho * Wo >= 40:
        for p, E in ((py, H), (px, W)):
            for cname, mask in classes(p, E, name == 'edges').items():
                assert bool(mask.any()), (shape, name, E, cname)
    inside = (py > -1) & (py < H) & (px > -1) & (px < W)
    assert float(inside.double().mean()) >= 0.25, float(inside.double().mean())
    dx = D.adjoint64(x, off, dcols, stride)[0]
    assert float((dx != 0).double().mean()) >= 0.5, float((dx != 0).double().mean())


@pytest.mark.parametrize('si', D.ALL_GENERATORS_ON)
def test_traveller_lands(si):
    shape = D.SHAPES[si]
    N, C, H, W, stride = shape
    x, off, dcols = D.exact_case(shape, 'traveller')
    moved = int((off.view(N, -1, 2) != 0).any(-1).sum())
    assert 4 * N <= moved <= 8 * N
    if (H, W) == (21, 19):
        assert float(off.abs().max()) >= 12
    dx = D.adjoint64(x, off, dcols, stride)[0]
    dx0 = D.adjoint64(x, torch.zeros_like(off), dcols, stride)[0]
    changed = (dx != dx0).any(-1).view(N, -1).sum(1)  # pixels per image
    assert bool((changed >= 1).all()), changed
    assert bool((changed <= 8 * 8).all()), changed  # only the pixels the travellers left and reached


@pytest.mark.parametrize('at', [0, 1, 2])
@pytest.mark.parametrize('name', ['rim_below', 'rim_at', 'rim_above', 'rim_far'])
@pytest.mark.parametrize('si', D.ALL_GENERATORS_ON)
def test_rim_sets_the_stored_maximum(si, name, at):
    shape = D.SHAPES[si]
    x, off, dcols = D.exact_case(shape, name, at)
    v = D.rim_value(name, shape, at)
    so = stored(off, at)
    assert float(so.abs().max()) == v
    assert int((so.abs() == v).sum()) == 1
    e = D.emax_of(shape[2], shape[3])
    assert (v < e) == (name == 'rim_below')
    rest = so.clone()
    rest[0, 0, 0, 0] = 0
    assert float(rest.abs().max()) < e - 0.25


def test_pile_and_window_sizes():
    """pile: several hundred addends on one to four pixels; quarter6 on the 21 x 19 map: a 15 x 15 window, three 96-pixel rounds;
    integer: E = 3 exactly, with taps on the window's rim; pile_rows: only input row 0 receives anything."""
    shape = D.SHAPES[0]
    N, C, H, W, stride = shape
    for i, (npix, wsum) in enumerate(((1, 1.0), (1, 0.25), (4, 1.0), (1, 1.0), (1, 0.125))):  # (pixels hit, the in-range corners' weight)
        x, off, dcols = D.exact_case(shape, 'pile%d' % i)
        dx = D.adjoint64(x, off, torch.ones_like(dcols), stride)[0]
        hit = (dx[..., 0] != 0).view(N, -1).sum(1)
        assert hit.tolist() == [npix] * N, (i, hit)
        assert float(dx[0, ..., 0].sum()) == 9 * 11 * 9 * wsum  # every tap of every output pixel
    x, off, dcols = D.exact_case(D.SHAPES[5], 'quarter6')
    assert float(off.abs().max()) == 6.0 and 2 * 96 < 15 * 15 <= 3 * 96
    x, off, dcols = D.exact_case(shape, 'integer')
    assert float(off.abs().max()) == 3.0 and float((off.abs() == 3).double().mean()) > 0.2
    x, off, dcols = D.exact_case(shape, 'pile_rows')
    dx = D.adjoint64(x, off, dcols, stride)[0]
    assert bool((dx[:, 0] != 0).any()) and not bool((dx[:, 1:] != 0).any())
