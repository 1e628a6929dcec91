"""-m gpu: on-device pixel metric vs the reference's cal_text_score output (golden)."""
import os

import numpy as np
import pytest
import torch

from gpu_util import DEV
from db_text_minimal_amd.text_metrics import RunningScore, cal_text_score
from oracle import dbnet_oracle as O

pytestmark = pytest.mark.gpu


def test_pixel_metric_matches_reference_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, 'pixel_metrics.npz'))
    rs = RunningScore(2)
    for step in range(2):
        P, G, M = (torch.from_numpy(z['step%d/%s' % (step, k)]).to(DEV) for k in 'PGM')
        preds = torch.stack([P, torch.zeros_like(P), torch.zeros_like(P)], 1).contiguous()  # [N,3,H,W] like the model output
        score = cal_text_score(preds[:, 0, :, :], G, M, rs, thresh=0.25)
        assert np.array_equal(rs.confusion_matrix, z['step%d/hist' % step])  # integer counts: bit-exact
        got = [score[k] for k in ('Overall Acc', 'Mean Acc', 'FreqW Acc', 'Mean IoU')]
        assert np.allclose(got, z['step%d/scores' % step], rtol=1e-12)
    rs.reset()
    assert rs.confusion_matrix.sum() == 0


def test_pixel_metric_full_size_and_edges():
    g = torch.Generator(device=DEV).manual_seed(0)
    N, S = 16, 640
    P = torch.rand(N, 3, S, S, device=DEV, generator=g)
    G = (torch.rand(N, S, S, device=DEV, generator=g) > 0.9).float()
    M = (torch.rand(N, S, S, device=DEV, generator=g) > 0.05).float()
    rs = RunningScore(2)
    cal_text_score(P[:, 0], G, M, rs, thresh=0.5)
    hist = rs.confusion_matrix
    assert hist.sum() == N * S * S  # every pixel is counted exactly once
    ref = O.pixel_confusion(P[:2, 0], G[:2], M[:2], 0.5)
    rs2 = RunningScore(2)
    cal_text_score(P[:2, 0], G[:2], M[:2], rs2, thresh=0.5)
    assert np.array_equal(rs2.confusion_matrix, ref)
    # all masked out -> everything lands in hist[0][0]; threshold is strict (> thresh)
    rs3 = RunningScore(2)
    cal_text_score(torch.full((1, 8, 8), 0.5, device=DEV), torch.ones(1, 8, 8, device=DEV), torch.ones(1, 8, 8, device=DEV), rs3, 0.5)
    assert np.array_equal(rs3.confusion_matrix, np.array([[0, 0], [64, 0]]))
    cal_text_score(torch.ones(1, 8, 8, device=DEV), torch.ones(1, 8, 8, device=DEV), torch.zeros(1, 8, 8, device=DEV), rs3, 0.5)
    assert np.array_equal(rs3.confusion_matrix, np.array([[64, 0], [64, 0]]))


@pytest.mark.parametrize('planes', [2, 3])
@pytest.mark.parametrize('shape', [(3, 7, 9), (2, 33, 31)])
def test_pixel_confusion_kernel_vs_oracle(shape, planes):
    """dbn_pixel_confusion through the C ABI against oracle.pixel_confusion, counts bit-exact: odd sizes (one and several workgroups'
    worth of tail), the probability plane inside 2- and 3-plane predictions (batch_stride), P M exactly at the threshold (strict >:
    not text), fractional G M below 1 (truncates to background), and two calls accumulating into one histogram."""
    from gpu_util import L, stream
    from db_text_minimal_amd import _lib
    N, H, W = shape
    thresh = 0.375  # exact in fp32, and so are the products below
    g = torch.Generator().manual_seed(H)
    hist = torch.zeros(5, dtype=torch.float64, device=DEV)
    ref = np.zeros((2, 2))
    for call in range(2):
        preds = torch.rand(N, planes, H, W, generator=g)
        M = torch.randint(0, 3, (N, H, W), generator=g).float() / 2  # 0, 1/2, 1
        G = torch.randint(0, 3, (N, H, W), generator=g).float() / 2
        i = torch.arange(N * H * W).view(N, H, W)
        P = preds[:, 0]
        P[i % 5 == 0] = 0.375  # at the threshold under M = 1
        M[i % 5 == 0] = 1.0
        P[i % 7 == 1] = 0.75  # at the threshold under M = 1/2
        M[i % 7 == 1] = 0.5
        P[i % 11 == 2] = float(np.nextafter(np.float32(0.375), np.float32(1)))  # the next float above it
        M[i % 11 == 2] = 1.0
        assert int(((P * M) == thresh).sum()) >= 2 * (N * H * W // 7) and int(((G * M > 0) & (G * M < 1)).sum()) > 0
        ref += O.pixel_confusion(P, G, M, thresh)
        pd, gd, md = preds.to(DEV), G.to(DEV), M.to(DEV)
        _lib.check(L().dbn_pixel_confusion(pd.data_ptr(), planes * H * W, gd.data_ptr(), md.data_ptr(), N, H, W, thresh, hist.data_ptr(), stream()),
                   'pixel_confusion')
        _, n01, n10, n11, tot = hist.cpu().tolist()
        got = np.array([[tot - n01 - n10 - n11, n01], [n10, n11]])
        assert np.array_equal(got, ref), (call, got, ref)
    assert ref.sum() == 2 * N * H * W and ref[1, 1] > 0 and ref[0, 1] > 0 and ref[1, 0] > 0
