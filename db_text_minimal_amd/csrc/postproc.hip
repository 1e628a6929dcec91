// Device side of SURVEY §8(f-3): the two array operations of SegDetectorRepresenter (src/postprocess.py) that sit
// between the GPU forward and the (unchanged, host) OpenCV contour code.
//   binarize_u8      postprocess.py:51-52    pred[:, 0] > thresh, as a uint8 bitmap (1 B/px over PCIe instead of 4)
//   box_scores       postprocess.py:186-198  box_score_fast for K boxes/polygons at once: mean of the probability map
//                                            over the cv2.fillPoly mask of each box (one workgroup per box)
// The fillPoly mask is evaluated per pixel in closed form (fillpoly.h, shared with gtmaps.hip).
#include "common.h"
#include "fillpoly.h"

namespace {

constexpr int MAX_PTS = 64;

__global__ void binarize_u8_kernel(const float* __restrict__ pred, long plane_stride, long hw, float thresh, int n_img,
                                   unsigned char* __restrict__ out) {
    const long total4 = (long)n_img * hw / 4;  // hw % 4 == 0
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total4; i += (long)gridDim.x * blockDim.x) {
        const long e = 4 * i, n = e / hw, r = e - n * hw;
        const f32x4 v = *reinterpret_cast<const f32x4*>(pred + n * plane_stride + r);
        uchar4 b;
        b.x = v[0] > thresh; b.y = v[1] > thresh; b.z = v[2] > thresh; b.w = v[3] > thresh;
        reinterpret_cast<uchar4*>(out)[i] = b;
    }
}

__global__ __launch_bounds__(256) void box_score_kernel(const float* __restrict__ bitmap, int H, int W,
                                                        const float* __restrict__ boxes, int P, float* __restrict__ scores) {
    __shared__ int vx[MAX_PTS], vy[MAX_PTS];
    __shared__ int bb[4];
    __shared__ double rs[4], rc[4];
    const float* box = boxes + (long)blockIdx.x * P * 2;
    if (threadIdx.x == 0) {
        float x0 = box[0], x1 = box[0], y0 = box[1], y1 = box[1];
        for (int i = 1; i < P; ++i) {
            x0 = fminf(x0, box[2 * i]); x1 = fmaxf(x1, box[2 * i]);
            y0 = fminf(y0, box[2 * i + 1]); y1 = fmaxf(y1, box[2 * i + 1]);
        }
        bb[0] = min(max((int)floorf(x0), 0), W - 1);
        bb[1] = min(max((int)ceilf(x1), 0), W - 1);
        bb[2] = min(max((int)floorf(y0), 0), H - 1);
        bb[3] = min(max((int)ceilf(y1), 0), H - 1);
    }
    __syncthreads();
    const int xmin = bb[0], xmax = bb[1], ymin = bb[2], ymax = bb[3];
    if (threadIdx.x < P) {  // (box - min).astype(int32): truncation toward zero
        vx[threadIdx.x] = (int)(box[2 * threadIdx.x] - (float)xmin);
        vy[threadIdx.x] = (int)(box[2 * threadIdx.x + 1] - (float)ymin);
    }
    __syncthreads();
    const int bw = xmax - xmin + 1, bh = ymax - ymin + 1;
    double sum = 0.0, cnt = 0.0;
    for (int idx = threadIdx.x; idx < bw * bh; idx += blockDim.x) {
        const int py = idx / bw, px = idx - py * bw;
        const bool in = dbn_fillpoly_hit(px, py, vx, vy, P);
        if (in) {
            sum += (double)bitmap[(long)(ymin + py) * W + xmin + px];
            cnt += 1.0;
        }
    }
    sum = dbn_wave_sum_d(sum);
    cnt = dbn_wave_sum_d(cnt);
    if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = sum; rc[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s = rs[0] + rs[1] + rs[2] + rs[3], c = rc[0] + rc[1] + rc[2] + rc[3];
        scores[blockIdx.x] = c > 0.0 ? (float)(s / c) : 0.f;  // cv2.mean over an empty mask is 0
    }
}

}  // namespace

extern "C" {

// out[n][h*w] = pred[n][0][h][w] > thresh (pred: NCHW with `channels` planes of h*w floats, h*w % 4 == 0)
int dbn_binarize_u8(const float* pred, int N, int channels, int H, int W, float thresh, unsigned char* out, void* stream) {
    DBN_REQUIRE(pred && out && N > 0 && channels > 0 && H > 0 && W > 0 && ((long)H * W) % 4 == 0);
    const long hw = (long)H * W;
    hipLaunchKernelGGL(binarize_u8_kernel, dim3(dbn_grid((long)N * hw / 4)), dim3(256), 0, (hipStream_t)stream, pred, channels * hw,
                       hw, thresh, N, out);
    return dbn_status();
}

// scores[k] = box_score_fast(bitmap[H][W], boxes[k][P][2] (x, y)), P <= 64 vertices per box (pad shorter polygons by
// repeating the last vertex: degenerate edges add nothing)
int dbn_box_scores(const float* bitmap, int H, int W, const float* boxes, int K, int P, float* scores, void* stream) {
    DBN_REQUIRE(bitmap && boxes && scores && H > 0 && W > 0 && K >= 0 && P >= 1 && P <= MAX_PTS);
    if (K == 0) return DBN_OK;
    hipLaunchKernelGGL(box_score_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, bitmap, H, W, boxes, P, scores);
    return dbn_status();
}

}  // extern "C"
