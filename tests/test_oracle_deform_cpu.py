"""CPU: analytic pins of oracle.deform_sample, the sampling rule of the deformable convolution (torchvision's
bilinear_interpolate, restated in the oracle's docstring).  The oracle is PARITY UNPINNED against torchvision (not installed),
so these pins are what holds the rule in place: the GPU tests (tests/test_train16_ops_gpu.py) compare the HIP kernel with it.

Two probe images make the expected values closed-form:
  ones(H, W)            a sample's value is the summed weight of its in-range corners;
  f(i, j) = a + b i + c j   bilinear interpolation reproduces an affine function exactly where all four corners are in range,
                        and at the edge only the in-range row / column contributes, weighted by its own bilinear weight."""
import pytest
import torch
import torch.nn.functional as F

from oracle import dbnet_oracle as O

D = torch.float64


def sample_at(img, ys, xs):
    """Value of deform_sample at absolute positions (ys[i], xs[i]) of a [H, W] image: a 1 x 1 kernel (R = S = 1, pad 0, stride 1)
    whose output pixel i (row-major) has its offset move the tap from its undeformed position (i // W, i % W) to the target."""
    H, W = img.shape
    n = len(ys)
    assert n <= H * W
    m = torch.arange(n)
    off = torch.zeros(1, 2, H * W, dtype=D)
    off[0, 0, :n] = torch.tensor(ys, dtype=D) - (m // W).to(D)
    off[0, 1, :n] = torch.tensor(xs, dtype=D) - (m % W).to(D)
    col = O.deform_sample(img.view(1, 1, H, W).to(D), off.view(1, 2, H, W), 1, 1, 1, 0)
    assert col.shape == (1, 1, 1, H, W)
    return col.reshape(-1)[:n]


@pytest.mark.parametrize('H,W', [(7, 9), (5, 12)])
def test_deform_sample_boundary_rule_on_a_constant_image(H, W):
    """ones(H, W): exactly -1 and exactly H (W) are outside (0); (-1, 0) keeps the weight 1 + y of row 0; exactly H - 1 is the last
    row at weight 1; (H - 1, H) keeps H - y; far outside is 0; an interior fraction has all four corners (1)."""
    img = torch.ones(H, W, dtype=D)
    x_in = 2.0  # an interior integer column: only the row coordinate decides
    cases = [(-1.0, 0.0), (-0.75, 0.25), (-0.25, 0.75), (-2**-20, 1 - 2**-20), (0.0, 1.0), (H - 1.0, 1.0), (H - 0.75, 0.75),
             (H - 0.25, 0.25), (float(H), 0.0), (H + 0.5, 0.0), (-1e6, 0.0), (1e6, 0.0), (2.5, 1.0), (H - 1.5, 1.0)]
    got = sample_at(img, [c[0] for c in cases], [x_in] * len(cases))
    assert torch.equal(got, torch.tensor([c[1] for c in cases], dtype=D)), (got, cases)
    # the same rule along the columns (the row an interior integer)
    ccases = [(-1.0, 0.0), (-0.5, 0.5), (W - 1.0, 1.0), (W - 0.5, 0.5), (float(W), 0.0), (-3e4, 0.0)]
    got = sample_at(img, [3.0] * len(ccases), [c[0] for c in ccases])
    assert torch.equal(got, torch.tensor([c[1] for c in ccases], dtype=D)), (got, ccases)
    # both coordinates in the edge band: the product of the two one-dimensional weights
    got = sample_at(img, [-0.5, H - 0.25, -0.75], [-0.25, W - 0.5, W - 1.0])
    assert torch.equal(got, torch.tensor([0.5 * 0.75, 0.25 * 0.5, 0.25 * 1.0], dtype=D)), got


def test_deform_sample_reproduces_an_affine_image():
    """f(i, j) = 3 + 2 i - 5 j: interior samples (fractional or not) give f(y, x); in the band (-1, 0) only row 0 contributes, at weight
    1 + y; in (H - 1, H) only row H - 1, at weight H - y; corner bands multiply."""
    H, W = 6, 8
    i = torch.arange(H, dtype=D).view(H, 1)
    j = torch.arange(W, dtype=D).view(1, W)
    img = 3 + 2 * i - 5 * j
    f = lambda y, x: 3 + 2 * y - 5 * x
    ys = [0.0, 0.5, 1.25, 4.75, 5.0, 2.0, -0.25, 5.5, 3.0, 3.0, -0.5]
    xs = [0.0, 0.5, 6.5, 0.125, 7.0, 3.75, 2.5, 4.25, -0.75, 7.25, -0.5]
    want = [f(0, 0), f(0.5, 0.5), f(1.25, 6.5), f(4.75, 0.125), f(5, 7), f(2, 3.75),
            0.75 * f(0, 2.5),        # row band (-1, 0): row 0 at weight 1 + y
            0.5 * f(5, 4.25),        # row band (H-1, H): row H-1 at weight H - y
            0.25 * f(3, 0),          # column band (-1, 0)
            0.75 * f(3, 7),          # column band (W-1, W)
            0.5 * 0.5 * f(0, 0)]     # corner band
    got = sample_at(img, ys, xs)
    assert torch.allclose(got, torch.tensor(want, dtype=D), rtol=0, atol=1e-12), (got, want)


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('dy,dx', [(0, 0), (1, 0), (0, -1), (-2, 3), (4, -5), (40, 0)])
def test_deform_sample_integer_offsets_equal_a_shifted_convolution(stride, dy, dx):
    """The same integer offset (dy, dx) at every tap samples x shifted by (dy, dx) with zeros outside the image: deform_conv2d
    then equals an unpadded F.conv2d of the shifted image on the padded domain (dy = dx = 0: the undeformed convolution)."""
    N, C, H, W, Co = 2, 5, 9, 11, 4
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, C, H, W, generator=g, dtype=D)
    w = torch.randn(Co, C, 3, 3, generator=g, dtype=D)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    off = torch.zeros(N, 18, Ho, Wo, dtype=D)
    off[:, 0::2] = dy
    off[:, 1::2] = dx
    # the shifted image on the PADDED domain rows -1..H, columns -1..W: a tap in the padding samples x wherever its offset takes it
    sp = torch.zeros(N, C, H + 2, W + 2, dtype=D)
    i0, i1 = max(-1, -dy), min(H + 1, H - dy)
    j0, j1 = max(-1, -dx), min(W + 1, W - dx)
    if i0 < i1 and j0 < j1:
        sp[:, :, i0 + 1:i1 + 1, j0 + 1:j1 + 1] = x[:, :, i0 + dy:i1 + dy, j0 + dx:j1 + dx]
    ref = F.conv2d(sp, w, None, stride, 0)
    got = O.deform_conv2d(x, off, w, stride, 1)
    assert torch.allclose(got, ref, rtol=0, atol=1e-12), float((got - ref).abs().max())
    # ... and the columns themselves are the shifted image's 3 x 3 patches, exactly (weights 1 and 0)
    col = O.deform_sample(x, off, 3, 3, stride, 1)
    patches = F.unfold(sp, 3, padding=0, stride=stride).view(N, C, 9, Ho, Wo)
    assert torch.equal(col, patches)


def test_deform_sample_non_finite_offset_stays_in_its_sample():
    """A NaN / +-inf offset makes exactly its own sample's C values NaN; every other sample is what it is without it."""
    N, C, H, W = 1, 3, 6, 7
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, C, H, W, generator=g, dtype=D)
    off = torch.randn(N, 18, H, W, generator=g, dtype=D)
    clean = O.deform_sample(x, off, 3, 3, 1, 1)
    bad = off.clone()
    hits = [(3, 2, 2, float('nan')), (8, 0, 6, float('inf')), (15, 5, 0, -float('inf'))]  # (channel, ho, wo, value)
    for ch, ho, wo, v in hits:
        bad[0, ch, ho, wo] = v
    got = O.deform_sample(x, bad, 3, 3, 1, 1)
    poisoned = torch.zeros(N, 1, 9, H, W, dtype=torch.bool)
    for ch, ho, wo, _ in hits:
        poisoned[0, 0, ch // 2, ho, wo] = True
    poisoned = poisoned.expand_as(got)
    assert torch.isnan(got[poisoned]).all()
    assert torch.equal(got[~poisoned], clean[~poisoned])
