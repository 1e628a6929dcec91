/* C ABI of libdbnet_hip.so — the MI355X (gfx950) DBNet hot path.
 *
 * The reference (huyhoang17/DB_text_minimal) is pure Python/PyTorch and has no FFI
 * layer; its accelerator boundary is the nn.Module call surface of
 *   DBTextModel.forward   /root/reference/src/models.py:34-48
 *   DBLoss.forward        /root/reference/src/losses.py:105-139
 *   the optimizer step    /root/reference/src/train.py:169-172
 * The entry points below are what a binding for that surface calls (see
 * INTEGRATION.md for the ctypes stub).  Conventions:
 *   - all pointers are DEVICE pointers to fp32 unless stated otherwise; the library
 *     never allocates, frees or retains them;
 *   - activations are NHWC ([N,H,W,C], C % 4 == 0); the model input and the three
 *     output maps are NCHW exactly like the reference's tensors;
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on it;
 *   - return value 0 = ok, 1 = invalid argument, 1000+e = hipError_t e at launch.
 */
#ifndef DBNET_HIP_H
#define DBNET_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- convolutions (replaces nn.Conv2d / nn.ConvTranspose2d fwd+bwd:
 *      modules/resnet.py:27-34,70-91,167-172; modules/basic.py:17-25;
 *      modules/segmentation_body.py:22-61; modules/segmentation_head.py:24-29,64-79) */

/* OIHW weights -> GEMM panels [ceil(K/16)*4][Cd][4].  mode 0: forward conv panels
 * (Cs = I rounded up to 4, Cd = O); mode 1: data-gradient / ConvTranspose panels
 * (Cs = O, Cd = I) — for stride f = 2, 4, 8: f*f panels, one per output-parity class (only the
 * taps that reach that class).  `out` holds dbn_igemm_panel_floats(...) floats. */
int dbn_pack_weights(const float* w_oihw, int O, int I, int R, int S, int mode, int stride, float* out, void* stream);
long dbn_igemm_panel_floats(int O, int I, int R, int S, int mode, int stride);
int dbn_igemm_packed_floats(int K, int Cd);

/* dst[N,Hd,Wd,Cd] (+)= gather(src[N,Hs,Ws,Cs]) x panels + bias.
 * mode 0: hs = hd*stride - pad + r (Conv2d forward; ConvTranspose2d data gradient)
 * mode 1: hs = (hd + pad - r)/stride when divisible (Conv2d data gradient;
 *         ConvTranspose2d forward); stride f = 2, 4, 8 runs as f*f parity-class problems in one
 *         launch, so no zero taps are multiplied.  bias may be NULL.  tile_hint 0 = auto.
 * `wpk` must come from dbn_pack_weights with the same (mode, stride).
 * Limits (DBN_ERR_ARG otherwise): Cs % 4 == 0, Cd % 64 == 0, N*Hd*Wd < 2^24 output pixels, the source tensor below
 * 0xF0000000 bytes (raw buffer addressing), N*Hd*Wd*Cd < 2^32 output elements (32-bit epilogue offsets). */
int dbn_igemm_f32(const float* src, const float* wpk, const float* bias, float* dst, int N, int Hs, int Ws, int Cs, int Hd,
                  int Wd, int Cd, int R, int S, int stride, int pad, int mode, int accumulate, int tile_hint, void* stream);

/* The same three operations with the products evaluated on the bf16 matrix pipe (fp32 accumulate,
 * fp32 tensors in and out).  ns = 3: every fp32 operand is split exactly into three bf16 terms and
 * six partial products are accumulated -> fp32-accurate (measured error below a plain fp32 fmaf
 * chain) at 6/16 of the fp32-MFMA cost.  ns = 1: operands rounded to bf16 (BASELINE configs[2]
 * "bf16 compute").  Panels must come from dbn_pack_weights_bf16s with the same (mode, stride, ns). */
int dbn_pack_weights_bf16s(const float* w_oihw, int O, int I, int R, int S, int mode, int stride, int ns, float* out, void* stream);
/* All weight panels of a model in one launch (after an optimizer step every panel is stale: ~80 dbn_pack_weights calls of a
 * few microseconds each otherwise).  jobs: DEVICE array of n dbn_pack_job records (48 bytes each)
 * with Cs = (mode 0 ? I rounded up to 4 : O), Cd = (mode 0 ? O : I), f = (mode 1 && stride > 1 ? stride : 1);
 * out sized by dbn_igemm_panel_floats / dbn_igemm_bf16s_panel_floats.  ns = 0: fp32 panels; 1, 3: split-bf16 panels. */
typedef struct dbn_pack_job {
    const float* w;
    void* out;
    int O, I, R, S, mode, Cs, Cd, f;
} dbn_pack_job;
int dbn_pack_weights_batched(const void* jobs, int n, int ns, void* stream);
long dbn_igemm_bf16s_panel_floats(int O, int I, int R, int S, int mode, int stride, int ns);
int dbn_igemm_bf16s(const float* src, const float* wpk, const float* bias, float* dst, int N, int Hs, int Ws, int Cs, int Hd,
                    int Wd, int Cd, int R, int S, int stride, int pad, int mode, int accumulate, int tile_hint, int ns,
                    void* stream);
int dbn_wgrad_bf16s(const float* sm, const float* big, float* slab, float* grad_oihw, int N, int Ho, int Wo, int O, int H, int W,
                    int Cb, int I, int R, int S, int stride, int pad, float scale, int ns, void* stream);

/* Data gradient (any dbn_igemm_t mode, no split-K) whose epilogue also reduces the two per-channel sums of the BatchNorm
 * backward that consumes its output — the backward of the conv -> BN -> ReLU chain of resnet.py:70-91 / basic.py:32-36 with one
 * pass over dz and y fewer.  dst is the gradient dz of the (ReLU'd) output of a BatchNorm with input y (same shape and storage as
 * dst), saved mean / rstd; ReLU mask: `zmask` > 0 (a saved activation of that shape) or, with zmask NULL, the BatchNorm's own
 * output recomputed as fma(y, mask_scale[c], mask_shift[c]) > 0.  Per output tile (row) and channel:
 *   part[0][c][row] = sum g,   part[1][c][row] = sum g * (y - mean[c]) * rstd[c],   g = dz_final * [mask > 0]
 * over the FINAL dst values (after `accumulate`): the call must be the last writer of dst.  part: [2][Cd][rows] floats with
 * rows = dbn_igemm_bn_rows(same geometry); hand it to dbn_bn_backward_t as `sums` with sums_parts = rows.  fp32 tensors
 * (at = 0, ns = 0 / 1 / 3) and bf16 tensors (at = 1, ns = 1: sums over the stored, rounded values; y / zmask bf16).  y2 / save_mean2 /
 * save_rstd2 / part2 (all NULL, or all given together with zmask): a SECOND BatchNorm consuming the same dst under the same mask
 * (bn2 and the projection shortcut's BatchNorm of a residual block, resnet.py:84-91); part2 like part.  A strided transposed conv (mode 1, stride > 1) must be tap-complete (R, S >= stride: every
 * output pixel is visited). */
int dbn_igemm_bn_rows(int at, int ns, int N, int Hs, int Ws, int Cs, int Hd, int Wd, int Cd, int R, int S, int stride, int pad, int mode,
                      int tile_hint);
/* Optional in-kernel finalize of those sums (`fin` of dbn_igemm_bnsums_t; NULL: the caller hands `part` to dbn_bn_backward_t,
 * which folds it with its own launch).  The last workgroup to finish in each group of 64 partial rows folds the group, the last
 * group-folder of an output-channel tile folds the groups — fixed summation order, integer counters only — and writes, per
 * BatchNorm, c1c2 = [2][Cd] (sum g / M, sum g*xhat / M with M = N*Hd*Wd: hand it to dbn_bn_backward_t as `sums` with sums_parts
 * = -1, which then launches the apply pass only) and the parameter gradients dgamma = grad_scale * sum g*xhat, dbeta =
 * grad_scale * sum g.  counters: dbn_igemm_bn_final_counters(rows, Cd) ints, ZERO before the first call (the kernels leave
 * them zero); group: dbn_igemm_bn_final_group_floats(rows, Cd) floats of scratch.  The *_2 members belong to the second
 * BatchNorm (y2). */
typedef struct dbn_bnb_final {
    int* counters;
    float* group;
    float *c1c2, *dgamma, *dbeta;
    float *c1c2_2, *dgamma_2, *dbeta_2;
    float grad_scale;
} dbn_bnb_final;
long dbn_igemm_bn_final_counters(int rows, int Cd);
long dbn_igemm_bn_final_group_floats(int rows, int Cd);
int dbn_igemm_bnsums_t(int at, int ns, const void* src, const float* wpk, const float* bias, void* dst, int N, int Hs, int Ws, int Cs, int Hd,
                       int Wd, int Cd, int R, int S, int stride, int pad, int mode, int accumulate, int tile_hint, const void* y,
                       const void* zmask, const float* mask_scale, const float* mask_shift, const float* save_mean,
                       const float* save_rstd, float* part, const void* y2, const float* save_mean2, const float* save_rstd2,
                       float* part2, const dbn_bnb_final* fin, void* stream);

/* Convolution whose epilogue also accumulates the train-mode BatchNorm statistics of its output (per-tile pivot,
 * sum, sum of squares; merged in fp64 by a finalize kernel): one call replaces conv + statistics pass.
 * Arguments: dbn_igemm_f32's, ns = 0 (fp32 MFMA) / 3 / 1 (split-bf16), then dbn_bn_train_stats' BN arguments.
 * With accumulate = 1 the statistics are those of the final (previous dst + this conv) values.  ws: dbn_conv_bn_ws_floats(N,Hd,Wd,Cd,mode,stride) floats. */
long dbn_conv_bn_ws_floats(int N, int Hd, int Wd, int Cd, int mode, int stride);
/* Round 6: the NEXT dbn_conv_bn_t / dbn_winograd_conv_bn[_act]_f32 call of the calling thread folds its statistics rows ITSELF — the
 * workgroup that completes a group of 64 partial rows folds the group, the one that completes the last group folds the groups and writes
 * scale / shift / saved mean / rstd / running statistics: no finalize launch behind the conv (32 launches of a ResNet18-FPN train step).
 * counters: dbn_igemm_bn_final_counters(rows, Cd) ints with rows = dbn_igemm_bn_rows(...) / dbn_winograd_rows(...), ZERO before the first
 * use (the kernels leave them zero) and not shared by calls that may be in flight together; group: dbn_conv_bn_final_group_doubles(rows, Cd)
 * doubles of scratch.  Where the launch has no such epilogue (the 2x2 ConvTranspose kernel) the announcement is dropped and the finalize
 * kernel runs as before.  Same results as the finalize kernel up to fp64 summation order.  NULL clears a pending announcement. */
int dbn_conv_bn_set_final(int* counters, double* group);
long dbn_conv_bn_final_group_doubles(int rows, int Cd);
int dbn_conv_bn_f32(const float* src, const float* wpk, const float* bias, float* dst, int N, int Hs, int Ws, int Cs, int Hd, int Wd,
                    int Cd, int R, int S, int stride, int pad, int mode, int accumulate, int tile_hint, int ns,
                    const float* gamma, const float* beta, float eps, float momentum, float* run_mean, float* run_var,
                    float* scale, float* shift, float* save_mean, float* save_rstd, float* ws, void* stream);

/* Split-K variant of dbn_igemm_f32 / dbn_igemm_bf16s (ns selects the math) for convs whose output grid cannot fill
 * 256 CUs but whose reduction is long (the coarse FPN levels' data gradients: 6400 pixels x 64 channels, K = 25600):
 * `ksplit` workgroup rows each reduce a contiguous range of k-tiles into their own slab, a second kernel sums the
 * slabs in fixed order and applies bias / accumulate.  mode 0, or mode 1 with stride 1; Cs % 16 == 0.
 * dbn_igemm_splitk_plan returns the split count the library would pick (1 = do not split);
 * slab: dbn_igemm_splitk_slab_floats(...) = ksplit * (N*Hd*Wd*Cd + 1088) floats (the slabs are padded apart so that consecutive splits
 * land on different HBM channels). */
long dbn_igemm_splitk_slab_floats(int ksplit, int N, int Hd, int Wd, int Cd);
int dbn_igemm_splitk_plan(int M, int Cd, int K, int Cs);
int dbn_igemm_splitk_plan_ns(int M, int Cd, int K, int Cs, int ns); /* ... for matrix math ns (the plan follows the tile choice) */
int dbn_igemm_splitk_f32(const float* src, const float* wpk, const float* bias, float* dst, int N, int Hs, int Ws, int Cs, int Hd,
                         int Wd, int Cd, int R, int S, int stride, int pad, int mode, int accumulate, int tile_hint, int ns,
                         int ksplit, float* slab, void* stream);

/* Pyramid conv — the FPN output conv of segmentation_body.py:75-76 over torch.cat([p2, up2(p3), up4(p4), up8(p5)])
 * (segmentation_body.py:82-87) without building the concatenation:
 *   dst[N,H,W,Cd] = bias + sum_{g=0..3} ConvTranspose2d(k = 2^g + 2, stride 2^g, padding 1)(s_g),  s_g: [N, H>>g, W>>g, Cs]
 * with combined weights from dbn_fpn_combine_weights (level g: [Cs][Cd][k][k]) packed by dbn_pack_weights(mode 1,
 * stride 2^g) into w_g.  One launch; H, W multiples of 8, Cs % 16 == 0, Cd % 128 == 0.  gamma != NULL additionally produces the
 * train-mode BatchNorm coefficients of dst exactly like dbn_conv_bn_f32 (ws: dbn_pyramid_conv_ws_floats floats).
 * tile_hint: 0 | 1 (128x128 is the only tile). */
long dbn_pyramid_conv_ws_floats(int N, int H, int W, int Cd);
int dbn_pyramid_conv_f32(const float* s0, const float* s1, const float* s2, const float* s3, const float* w0, const float* w1,
                         const float* w2, const float* w3, const float* bias, float* dst, int N, int H, int W, int Cs, int Cd,
                         int tile_hint, int ns, const float* gamma, const float* beta, float eps, float momentum, float* run_mean,
                         float* run_var, float* scale, float* shift, float* save_mean, float* save_rstd, float* ws, void* stream);

/* tile configuration chosen for tile_hint 0: 1=128x128, 2=256x64, 3=128x64, 4=64x64 */
int dbn_igemm_tile_config(int M, int Cd);
/* ... for matrix math ns (0 exact fp32, 1 / 3 the bf16 pipe: those modes keep the larger tiles) */
int dbn_igemm_tile_config_ns(int M, int Cd, int ns);

/* grad_oihw[O][I][R][S] = scale * sum_p sm[p][o] * big[pixel(p)+tap][i];
 * sm = [N,Ho,Wo,O] (output-side tensor), big = [N,H,W,Cb] (input-side, Cb >= I).
 * slab: dbn_wgrad_slab_floats(...) floats of scratch (split-K partial sums, reduced deterministically). */
int dbn_wgrad_splitk(int N, int Ho, int Wo, int O, int Cb, int R, int S);
/* the same when the size of X (H x W) is known; a call whose tensors exceed the kernels' index ranges (2^24 pixel rows,
 * 32-bit byte offsets) runs as several launches over image ranges, each with its own slabs */
int dbn_wgrad_splitk_hw(int N, int Ho, int Wo, int O, int H, int W, int Cb, int R, int S);
/* slab floats for a call with X of size H x W stored with `es` bytes per element (4 fp32, 2 bf16): exact under the chunking */
long dbn_wgrad_slab_floats_hw(int N, int Ho, int Wo, int O, int H, int W, int Cb, int R, int S, int es);
/* Test hook: lower the per-launch index ranges (pixel rows, bytes per tensor, output elements; 0 = default) so that the image
 * chunking of the conv / weight-gradient entry points can be exercised at small sizes.  Not thread-safe. */
int dbn_set_index_limits(long pixel_rows, long bytes, long elems);
long dbn_wgrad_slab_floats(int N, int Ho, int Wo, int O, int Cb, int R, int S);
int dbn_wgrad_f32(const float* sm, const float* big, float* slab, float* grad_oihw, int N, int Ho, int Wo, int O, int H, int W,
                  int Cb, int I, int R, int S, int stride, int pad, float scale, void* stream);

/* ---- BatchNorm / ReLU / residual (nn.BatchNorm2d + nn.ReLU: resnet.py:73-91, basic.py:32-36) */
int dbn_reduce_ws_floats(int C);
int dbn_bn_train_stats(const float* y, int M, int C, const float* gamma, const float* beta, float eps, float momentum,
                       float* run_mean, float* run_var, float* scale, float* shift, float* save_mean, float* save_rstd,
                       float* ws, void* stream);
/* Inference (round 5): eval-mode BatchNorm folded into the conv in front of it (basic.py:32-36, resnet.py:70-91 under model.eval();
 * test.py:53-59).  w_out [O][inner] = w * s[o], b_out [o] = beta + (bias - run_mean) * s[o] with s = gamma / sqrt(run_var + eps) (bias may
 * be NULL); feed w_out / b_out to dbn_pack_weights* / dbn_winograd_pack and the *_act_* entry points below: the conv's epilogue then
 * produces relu(bn(conv(x)) [+ residual]) directly and no BatchNorm pass over the activation runs. */
int dbn_fold_bn_eval(const float* w, int O, long inner, const float* bias, const float* gamma, const float* beta, const float* run_mean,
                     const float* run_var, float eps, float* w_out, float* b_out, void* stream);
/* dst = [relu]( conv(src) + bias [+ res] ) in one launch: dbn_igemm_t's contract (mode 0 at any stride, mode 1 at stride 1; no split-K,
 * no accumulate) plus `res` (NULL or a tensor of dst's shape and storage type: a residual connection) and `relu`. */
int dbn_igemm_act_t(int at, int ns, const void* src, const float* wpk, const float* bias, const void* res, int relu, void* dst, int N,
                    int Hs, int Ws, int Cs, int Hd, int Wd, int Cd, int R, int S, int stride, int pad, int mode, int tile_hint,
                    void* stream);
/* ... the Winograd F(2x2,3x3) form (dbn_winograd_conv_bn_f32's tensors, no statistics) */
int dbn_winograd_conv_act_f32(const float* src, const float* upanel, const float* bias, const float* res, int relu, float* dst, int N,
                              int H, int W, int Cs, int Cd, void* stream);
/* ... and the FPN pyramid conv (dbn_pyramid_conv_from_t's tensors, no statistics): dst = [relu]( [dst +] levels first_level..3 + bias ) */
int dbn_pyramid_conv_act_t(int first_level, int at, const void* s0, const void* s1, const void* s2, const void* s3, const float* w0,
                           const float* w1, const float* w2, const float* w3, const float* bias, int relu, void* dst, int N, int H, int W,
                           int Cs, int Cd, int ns, void* stream);
int dbn_bn_eval_coef(int C, const float* gamma, const float* beta, const float* run_mean, const float* run_var, float eps,
                     float* scale, float* shift, void* stream);
/* out = act(y*scale+shift [+ res*res_scale+res_shift | + res]) */
int dbn_bn_apply(const float* y, const float* scale, const float* shift, const float* res, const float* res_scale,
                 const float* res_shift, float* out, long M, int C, int relu, void* stream);
/* g = dout * relu_mask; the mask is (zmask > 0) from a saved activation, or recomputed as
 * (y*mask_scale+mask_shift > 0) from the forward's own BN coefficients, or absent (all NULL).
 * dy = BN backward of g; optional gout (+)= g */
int dbn_bn_backward(const float* y, const float* zmask, const float* mask_scale, const float* mask_shift, const float* dout,
                    const float* save_mean, const float* save_rstd,
                    const float* gamma, float* dy, float* gout, int gout_accumulate, float* dgamma, float* dbeta, int M, int C,
                    float grad_scale, float* ws, void* stream);
/* the same with the two per-channel reductions supplied by the kernel that produced dout (sums[2][C]) */
int dbn_bn_backward_from_sums(const float* sums, const float* y, const float* zmask, const float* mask_scale, const float* mask_shift,
                              const float* dout, const float* save_mean, const float* save_rstd, const float* gamma, float* dy,
                              float* gout, int gout_accumulate, float* dgamma, float* dbeta, int M, int C, float grad_scale,
                              float* ws, void* stream);
/* General form: sums optional ([2][C] as above), dbias_conv optional ([C]: column sums of dy x grad_scale = gradient of the bias
 * of the conv that feeds this BatchNorm, formed in the apply pass; needs 256 % (C/4) == 0). */
int dbn_bn_backward_ex(const float* sums, const float* y, const float* zmask, const float* mask_scale, const float* mask_shift,
                       const float* dout, const float* save_mean, const float* save_rstd, const float* gamma, float* dy, float* gout,
                       int gout_accumulate, float* dgamma, float* dbeta, float* dbias_conv, int M, int C, float grad_scale, float* ws,
                       void* stream);
int dbn_col_sum(const float* x, int M, int C, float* out, float scale, float* ws, void* stream);

/* ---- stem pooling (nn.MaxPool2d(3,2,1) over relu(bn1(.)): resnet.py:233-235) */
int dbn_bnrelu_maxpool_fwd(const float* y, const float* scale, const float* shift, float* out, int N, int H, int W, int C,
                           void* stream);
int dbn_bnrelu_maxpool_bwd(const float* y, const float* scale, const float* shift, const float* pooled, const float* dpool,
                           float* dz, int N, int H, int W, int C, void* stream);

/* ---- FPN nearest upsample + add / concat (segmentation_body.py:79-87) */
int dbn_nearest_up_fwd(const float* src, const float* addend, float* dst, int N, int Hs, int Ws, int C, int H, int W, int Cdst,
                       int coff, void* stream);
int dbn_nearest_up_bwd(const float* dbig, float* dsrc, int N, int Hs, int Ws, int C, int H, int W, int Cbig, int coff,
                       int accumulate, void* stream);

/* ---- final resample of the model (F.interpolate bilinear, align_corners=True: models.py:43-46); the identity
 *      (and elided) when H, W are multiples of 32.  NCHW planes. */
int dbn_bilinear_fwd(const float* src, float* dst, long planes, int Hs, int Ws, int H, int W, void* stream);
int dbn_bilinear_bwd(const float* ddst, float* dsrc, long planes, int Hs, int Ws, int H, int W, void* stream);

/* ---- FPN output conv over [p2 | up2(p3) | up4(p4) | up8(p5)] (segmentation_body.py:55-61,82-87): its data and
 *      weight gradients per upsample group g (factor f = 2^g) are those of a (f+2)x(f+2), stride-f, pad-1 conv with
 *      COMBINED weights (sums of the 3x3 taps that read the same low-resolution pixel): 47 % of the MACs, no concat. */
int dbn_fpn_combine_weights(const float* w, int Co, int Cin, int group, int Cg, float* wd, void* stream);
int dbn_fpn_scatter_wgrad(const float* t0, const float* t1, const float* t2, const float* t3, int Co, int Cg, float* dw,
                          void* stream);

/* ---- layout / misc */
int dbn_nchw3_to_nhwc4(const float* x, float* out, int N, int H, int W, void* stream);
int dbn_add_inplace(const float* x, float* y, long n, void* stream);

/* ---- DB head tail (segmentation_head.py:28-29,35-45,77-79,106-108): last ConvTranspose2d(64,1,2,2) + Sigmoid of both
 * branches, step_function, concat.  With bn_scale/shift (all four [64], or all NULL) xb/xt are the PRE-BatchNorm outputs
 * of the preceding ConvTranspose2d and BN+ReLU (segmentation_head.py:27,74-75) is applied on load, so the post-BN
 * activations of the two largest tensors of the network are never written. */
int dbn_head_tail_fwd(const float* xb, const float* xt, const float* wb, const float* wt, const float* bias_b,
                      const float* bias_t, const float* bn_scale_b, const float* bn_shift_b, const float* bn_scale_t,
                      const float* bn_shift_t, float* out, int N, int Hq, int Wq, int channels, float kstep, void* stream);
int dbn_head_tail_bwd_ws_floats(void);
/* dxb/dxt: gradients w.r.t. the (post-ReLU) inputs of the last ConvTranspose2d; the BatchNorm backward applies the mask.
 * bn_sums (optional, needs the bn_* pointers incl. the saved mean / rstd): [4][64] = per channel sum of the masked
 * gradient and of masked gradient * xhat for branch b, then t — feed each [2][64] half to dbn_bn_backward_from_sums. */
int dbn_head_tail_bwd(const float* xb, const float* xt, const float* wb, const float* wt, const float* preds,
                      const float* dpreds, const float* bn_scale_b, const float* bn_shift_b, const float* bn_scale_t,
                      const float* bn_shift_t, const float* bn_mean_b, const float* bn_rstd_b, const float* bn_mean_t,
                      const float* bn_rstd_t, float* bn_sums, float* dxb, float* dxt, float* dw_b, float* dbias_b, float* dw_t,
                      float* dbias_t, int N, int Hq, int Wq, int channels, float kstep, float grad_scale, float* ws, void* stream);

/* ---- 3x3 / stride 1 / pad 1 forward convolution through the Winograd transform F(2x2, 3x3), fp32 arithmetic (2.25x fewer matrix
 * FLOPs than the direct form; BasicBlock convs resnet.py:70-91, FPN smooth convs segmentation_body.py:55-61, the head's 256 -> 64
 * convs segmentation_head.py:24-25,64-68).  fp32 NHWC tensors of any H x W (worked in 8 x 16 pixel patches; ragged edges are masked;
 * dbn_winograd_eligible says yes when >= 3/4 of the patch area is real), Cs % 16 == 0 channels in the source
 * tensor (I <= Cs of them real), Cd % 64 == 0 (dbn_winograd_eligible).  upanel: the filters transformed once per parameter update
 * (dbn_winograd_pack; dbn_winograd_panel_floats(O, Cs) floats).  gamma non-NULL: the train-mode BatchNorm that follows is folded
 * in exactly as in dbn_conv_bn_f32 (ws: dbn_winograd_ws_floats floats).  Same result as the direct convolution up to fp32 rounding
 * of a different summation order (not bit for bit). */
/* Round 5: winograd_f32_kernel runs with PERSISTENT workgroups — at most two per CU, pulling (patch, channel tile) items from per-XCD
 * counters the library keeps per stream — whenever a launch has more items than the chip has workgroup slots (512).  0 restores one
 * workgroup per item (round 4's form; A/B and test hook).  Results are bit-identical either way. */
int dbn_set_winograd_persistent(int on);
/* ... and the one-time phase stagger between the two persistent workgroups of a CU, in permille of one item's matrix time (0: off) */
int dbn_set_winograd_stagger(int permille);
/* ... and the channel blocks the patch form stages per barrier: 1 (default) or 2 (Cs % 32 == 0 layers; A/B hook) */
int dbn_set_winograd_blocks_per_barrier(int n);
int dbn_winograd_eligible(int N, int H, int W, int Cs, int Cd);
long dbn_winograd_panel_floats(int O, int Cs);
/* dgrad = 0: panel of the forward conv of w [O][I][3][3] over a source with Cs >= I channels.  dgrad = 1: panel of the DATA GRADIENT
 * of the conv with weights w [I][O][3][3] (filters rotated by 180 degrees, channel roles swapped): maps dy (Cs >= I channels) to dx (O). */
int dbn_winograd_pack(const float* w_oihw, int O, int I, int Cs, int dgrad, float* out, void* stream);
/* n dbn_winograd_pack calls in one launch (after an optimizer step every panel is stale).  jobs: DEVICE array of n
 * dbn_winograd_pack_job records (32 bytes each) */
typedef struct dbn_winograd_pack_job {
    const float* w;
    float* out;
    int O, I, Cs, dgrad;
} dbn_winograd_pack_job;
int dbn_winograd_pack_batched(const void* jobs, int n, void* stream);
int dbn_winograd_rows(int N, int H, int W);
/* The data gradient through the same kernel: dx [N,H,W,Cd] = [dx +] conv(dy [N,H,W,Cs]) with the dgrad = 1 panel.  y non-NULL: the
 * epilogue also produces the two per-channel sums of the BatchNorm backward that consumes dx — arguments and semantics of
 * dbn_igemm_bnsums_t, part = [2][Cd][dbn_winograd_rows(N,H,W)] floats, fin = optional in-kernel finalize (counters sized by
 * dbn_igemm_bn_final_counters(rows, Cd)). */
int dbn_winograd_dgrad_bnsums_f32(const float* dy, const float* upanel, float* dx, int N, int H, int W, int Cs, int Cd, int accumulate,
                                  const void* y, const void* zmask, const float* mask_scale, const float* mask_shift,
                                  const float* save_mean, const float* save_rstd, float* part, const void* y2, const float* save_mean2,
                                  const float* save_rstd2, float* part2, const dbn_bnb_final* fin, void* stream);
long dbn_winograd_ws_floats(int N, int H, int W, int Cd);
/* ... with the BatchNorm + ReLU in FRONT of the conv applied on load (basic.py:32-36, resnet.py:77-80): the conv's input is
 * relu(src * in_scale[c] + in_shift[c]) ([Cs] floats each, the coefficients of dbn_bn_apply; both NULL: src itself).  src is that
 * BatchNorm's input; its output tensor is never written.  Bit-identical to dbn_bn_apply followed by dbn_winograd_conv_bn_f32. */
int dbn_winograd_conv_bn_act_f32(const float* src, const float* in_scale, const float* in_shift, const float* upanel, const float* bias,
                                 float* dst, int N, int H, int W, int Cs, int Cd, const float* gamma, const float* beta, float eps,
                                 float momentum, float* run_mean, float* run_var, float* scale, float* shift, float* save_mean,
                                 float* save_rstd, float* ws, void* stream);
int dbn_winograd_conv_bn_f32(const float* src, const float* upanel, const float* bias, float* dst, int N, int H, int W, int Cs, int Cd,
                             const float* gamma, const float* beta, float eps, float momentum, float* run_mean, float* run_var,
                             float* scale, float* shift, float* save_mean, float* save_rstd, float* ws, void* stream);

/* Weight gradient of a 3x3 / stride-1 / pad-1 conv through the Winograd transform F(2x2,3x3) in exact-fp32 arithmetic
 * (csrc/winograd_wgrad_f32.hip; replaces torch.autograd's conv weight gradient for resnet.py:70-91, segmentation_body.py:55-61,
 * segmentation_head.py:24-25,64-68).  x [N][H][W][Cb] (channels >= I are zero padding), dy [N][H][W][O], grad [O][I][3][3] =
 * scale * dW (overwritten).  slab: dbn_winograd_wgrad_slab_floats floats of scratch.  phases: 1 = matrix kernel (-> slab),
 * 2 = slab reduction + G^T . G (-> grad), 3 = both.  Deterministic (fixed-order fp64 reduction, no atomics).  x_scale / x_shift
 * non-NULL ([Cb] each): the conv's input is relu(x * x_scale[c] + x_shift[c]), applied on load (see dbn_winograd_conv_bn_act_f32). */
int dbn_winograd_wgrad_eligible(int N, int H, int W, int O, int Cb, int I);
int dbn_winograd_wgrad_linear(int H, int W); /* 1: small map, consecutive-tile form (kernel <true> in a trace) */
long dbn_winograd_wgrad_slab_floats(int N, int H, int W, int O, int Cb);
int dbn_winograd_wgrad_f32(int phases, const float* dy, const float* x, const float* x_scale, const float* x_shift, float* slab, float* grad,
                           int N, int H, int W, int O, int Cb, int I, float scale, void* stream);
/* What the Winograd kernels do on an N x H x W map with O output-gradient channels and Cb stored input channels, DESCRIBED
 * instead of launched (host only: no device call): fills `plan` (host memory, dbn_winograd_plan) with the plans that
 * dbn_winograd_conv_bn[_act]_f32 / dbn_winograd_dgrad_bnsums_f32 (fwd_*) and dbn_winograd_wgrad_f32 (wgrad_*) take — for the tests
 * that prove which form a shape reaches.  fwd_lin / wgrad_lin: 1 = the consecutive-tile form, 0 = 8 x 16 pixel patches; fwd_rows =
 * dbn_winograd_rows; wgrad_groups: patches or 32-tile groups of the whole batch, shared among wgrad_nsplit workgroups per
 * wgrad_nsub = (O / 64) (Cb / 64) channel blocks (workgroup `split` takes groups split * groups / nsplit up to the next split's
 * first); wgrad_wide: 1 = the slab reduction is winograd_wgrad_reduce_kernel<32>, 0 = the serial one.  Eligibility is not checked
 * here (dbn_winograd_eligible, dbn_winograd_wgrad_eligible). */
typedef struct dbn_winograd_plan {
    int fwd_lin, fwd_rows;
    int wgrad_lin, wgrad_groups, wgrad_nsub, wgrad_nsplit, wgrad_wide;
} dbn_winograd_plan;
int dbn_winograd_describe(int N, int H, int W, int O, int Cb, void* plan);

/* ---- DBLoss (losses.py:18-40,48-66,75-82,105-139); preds [N,3|2,H,W], gts [4,N,H,W].
 * One launch: the workgroup that finishes last folds every workgroup's partial sums (fixed order) and writes losses[5] and
 * coef[8].  ws: dbn_db_loss_ws_bytes() bytes of scratch, no initialisation required (it ends with the arrival counter of that
 * hand-over, which the library clears on `stream` in front of every launch); not shared between calls that may run concurrently.
 * negative_ratio is a double in all four forward entry points: n_neg = min(int(n_pos * negative_ratio), ...) is taken in doubles like
 * the reference's Python (losses.py:26); rounded to float first, 0.7, 2.3 or 3.3 truncate one lower at n_pos = 10, 20, ... */
int dbn_db_loss_ws_bytes(void);
int dbn_db_loss_fwd(const float* preds, const float* gts, int N, int H, int W, int channels, float alpha, float beta,
                    double negative_ratio, float eps, float* losses, float* coef, void* ws, void* stream);
int dbn_db_loss_bwd(const float* preds, const float* gts, const float* coef, const float* grad_losses, float alpha, float beta,
                    int N, int H, int W, int channels, float* dpreds, void* stream);
/* DBLoss(reduction='sum'): losses.py:30 forwards the reduction string to F.binary_cross_entropy, so the scalar BCE of the
 * OHEM term is summed instead of averaged; everything else as dbn_db_loss_fwd (same ws; backward: dbn_db_loss_bwd). */
int dbn_db_loss_sum_fwd(const float* preds, const float* gts, int N, int H, int W, int channels, float alpha, float beta,
                        double negative_ratio, float eps, float* losses, float* coef, void* ws, void* stream);
/* The two entry points above evaluate losses.py:33-39's `topk(loss * negative, n_neg).sum()` (loss a SCALAR in these reductions)
 * in closed form, bce * n_neg — exact for binary prob_gt / supervision_mask maps (what data_loaders.py:112-134 produces) and
 * only for those.  coef[7] receives the number of pixels whose gt or mask is neither 0 nor 1 (the host side refuses such maps,
 * db_text_minimal_amd/losses.py).  dbn_db_loss_frac_fwd evaluates the expression literally for ANY maps:
 * bce * (sum(positive) + sum of the n_neg largest negative_i) / (n_pos + n_neg + eps), top-k sum by the device radix select of
 * the per-pixel path below.  sum != 0: reduction='sum'.  ws: dbn_db_loss_ohem_ws_bytes(N,H,W) bytes; backward: dbn_db_loss_bwd. */
int dbn_db_loss_frac_fwd(const float* preds, const float* gts, int N, int H, int W, int channels, float alpha, float beta,
                         double negative_ratio, float eps, int sum, float* losses, float* coef, void* ws, void* stream);

/* DBLoss(reduction='none') — true per-pixel OHEM (losses.py:30-39 with a per-pixel BCE): the n_neg largest
 * negative losses are found by a 3-pass radix select on device (no sort, no host sync).  `ws` holds
 * dbn_db_loss_ohem_ws_bytes(N,H,W) bytes (no initialisation required, as above) and must stay untouched between _fwd and _bwd. */
long dbn_db_loss_ohem_ws_bytes(int N, int H, int W);
int dbn_db_loss_ohem_fwd(const float* preds, const float* gts, int N, int H, int W, int channels, float alpha, float beta,
                         double negative_ratio, float eps, float* losses, float* coef, void* ws, void* stream);
int dbn_db_loss_ohem_bwd(const float* preds, const float* gts, const float* coef, const float* grad_losses, const void* ws,
                         float alpha, float beta, int N, int H, int W, int channels, float* dpreds, void* stream);

/* ---- per-step pixel metric (cal_text_score / RunningScore._fast_hist, text_metrics.py:14-24,63-82):
 *      2x2 confusion matrix of (P*M > thresh) vs int(G*M), accumulated on device into 5 doubles
 *      [unused, n01, n10, n11, total] (index = 2*gt + pred) — replaces 3 D2H copies + np.bincount per step */
int dbn_pixel_confusion(const float* preds, long batch_stride, const float* gt, const float* mask, int N, int H, int W, float thresh,
                        double* hist, void* stream);

/* ---- optimizer (torch.optim.Adam, train.py:114-117,172) over one flat buffer */
int dbn_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps, int step,
                  float grad_scale, void* stream);

/* ---- optimizer extensions (csrc/optim.hip): gradient accumulation, the global gradient norm, and Adam with AMSGrad, L2 weight decay
 *      and norm clipping.  Nothing here crosses to the host: the norm stays in device memory and the Adam launch reads it there.
 * dbn_grad_accumulate: acc = g when `first`, else acc += g (one fp32 add per element, the k micro-batches of one update in pass order).
 * dbn_grad_sqnorm: out[0] = sum of g[i]^2 in float64.  Workgroup b sums the fixed chunk [b C, (b + 1) C) of g into partials[b]
 *      (C is a compile-time constant, so the partition depends on n alone); a second launch of one workgroup adds the partials in index
 *      order.  No atomics: the same bits on every run.  `partials` holds dbn_grad_sqnorm_ws_doubles(n) doubles and needs no clearing.
 * dbn_adam_step_ex: with s = grad_scale,
 *      coef = sqnorm ? min(1, max_norm / (|s| sqrt(*sqnorm) + 1e-6)) : 1        (torch.nn.utils.clip_grad_norm_; a NaN norm gives NaN)
 *      gg = (coef s) g + weight_decay p                                          (torch's L2 form: the decay enters after the clip)
 *      then dbn_adam_step's update on gg, with vmax = max(vmax, v) in place of v under the square root when vmax != NULL (AMSGrad).
 *      With vmax == NULL, sqnorm == NULL and weight_decay == 0 the results are bit-identical to dbn_adam_step's. */
int dbn_grad_accumulate(float* acc, const float* g, long n, int first, void* stream);
long dbn_grad_sqnorm_ws_doubles(long n);
int dbn_grad_sqnorm(const float* g, long n, double* partials, double* out, void* stream);
int dbn_adam_step_ex(float* p, const float* g, float* m, float* v, float* vmax, long n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int step, float grad_scale, const double* sqnorm, float max_norm, void* stream);

/* ---- optimizer family (csrc/optim_groups.hip): SGD with momentum and AdamW over one flat buffer, with per-group
 *      learning rate and weight decay, the clip coefficient of dbn_adam_step_ex (same formula, same device value) and an optional
 *      exponential moving average of the weights.
 * Groups: `lr` and `weight_decay` are HOST arrays of `ngroups` floats (1 .. dbn_optim_max_groups() = 8), copied into the kernel arguments:
 *      nothing is uploaded when a schedule changes them.  `run_end` / `run_group` are DEVICE arrays of `nruns` int32: run r covers the
 *      quads (4 consecutive floats of the flat buffer) [run_end[r - 1], run_end[r]) and belongs to group run_group[r]; run_end ascends
 *      and its last entry covers n / 4.  Elements past the last whole quad take the last run's group.  nruns = 0 (tables may be NULL)
 *      means one group: that launch has no table, no LDS and no search.  nruns > dbn_optim_max_runs() = 1024 returns DBN_ERR_ARG.
 * EMA: with shadow != NULL the thread that formed p' also writes shadow' = ema_decay shadow + ema_one_minus p' (the caller rounds d and
 *      1 - d to fp32 once each); NULL moves no extra bytes.
 * dbn_sgd_step, as torch.optim.SGD with clip_grad_norm_ in front (G: the element's group, s = grad_scale, coef as in dbn_adam_step_ex):
 *      g = (coef s) acc + weight_decay[G] p;   buf' = g when `first`, else momentum buf + (1 - dampening) g
 *      d = g + momentum buf' (nesterov) | buf' (momentum != 0) | g (momentum == 0: `buf` may be NULL and is not touched)
 *      p' = p - lr[G] d
 * dbn_adamw_step: the update of dbn_adam_step_ex (vmax != NULL: AMSGrad) with lr[G] / bc1.  decoupled = 0: g + weight_decay[G] p after the
 *      clip (torch.optim.Adam(weight_decay); one group, shadow NULL: the bits of dbn_adam_step_ex).  decoupled = 1 (torch.optim.AdamW):
 *      p <- p fp32(1 - lr[G] weight_decay[G]) first, then the update with the undecayed gradient. */
int dbn_optim_max_groups(void);
int dbn_optim_max_runs(void);
int dbn_sgd_step(float* p, const float* g, float* buf, long n, const float* lr, const float* weight_decay, int ngroups, const int* run_end,
                 const int* run_group, int nruns, float momentum, float dampening, int nesterov, int first, float grad_scale,
                 const double* sqnorm, float max_norm, float* shadow, float ema_decay, float ema_one_minus, void* stream);
int dbn_adamw_step(float* p, const float* g, float* m, float* v, float* vmax, long n, const float* lr, const float* weight_decay, int ngroups,
                   const int* run_end, const int* run_group, int nruns, float beta1, float beta2, float eps, int decoupled, int step,
                   float grad_scale, const double* sqnorm, float max_norm, float* shadow, float ema_decay, float ema_one_minus,
                   void* stream);

/* 1 when the library was built with -DDBN_EXPERIMENTS (make -C csrc EXP=1): adds the variants that were measured and rejected —
 * pre-split bf16 planes (at = 3, dbn_split3), the LDS-DMA fp32 weight gradient (dbn_set_wgrad_variant(1)), DBN_* environment
 * overrides of the tile / split heuristics.  The product library (default) has none of them: no getenv anywhere. */
int dbn_has_experiments(void);

/* ---- measurement aid (bench.py, no reference counterpart): one wave samples the shader clock (s_memtime) against the constant
 * reference clock (s_memrealtime) over `microseconds`; out2 = {shader cycles, reference ticks} (two uint64 in device memory).
 * dbn_wall_clock_khz: the reference clock's rate.  sustained MHz = cycles / ticks * khz / 1000 */
int dbn_clock_probe(void* out2, int microseconds, void* stream);
int dbn_wall_clock_khz(void);

/* ---- deformable convolution of the DCN backbones (resnet.py:54-65,81-82,111-124,145-146: conv2_offset ->
 * torchvision.ops.DeformConv2d, deformable_groups = 1), lowered to sampling + GEMM:
 *   cols = dbn_deform_im2col(x, offset);  y = dbn_igemm_f32(cols as [N,Ho,Wo,R*S*C], 1x1 panels of the permuted weight)
 * backward: dcols = 1x1 data gradient, dW = 1x1 weight gradient of (dy, cols) permuted back, then dbn_deform_col2im.
 * offset: [N*Ho*Wo][off_stride] floats, channel 2k = dy and 2k+1 = dx of tap k = r*S + s (torchvision layout);
 * off_stride >= 2*R*S lets the offsets live in the 64-channel output of the (zero-padded) offset conv. */
int dbn_deform_im2col(const float* x, const float* offset, float* cols, int N, int H, int W, int C, int Ho, int Wo, int R, int S,
                      int stride, int pad, int off_stride, void* stream);
/* dx = [dx +] adjoint of the sampling applied to dcols; doffset is written (channels >= 2*R*S zeroed).  DETERMINISTIC since
 * round 3: every contribution is accumulated in 64-bit fixed point (scale from max |dcols| of the call: resolution 2^-43 of the
 * largest column gradient), so LDS / global integer atomics give the same bits in any order.  ws: dbn_deform_col2im_ws_bytes(...)
 * bytes of scratch; accumulate = 1 adds to the gradient dx already holds; off_stride % 4 == 0. */
long dbn_deform_col2im_ws_bytes(int N, int H, int W, int C, int Ho, int Wo, int R, int S);
int dbn_deform_col2im(const float* dcols, const float* x, const float* offset, float* dx, float* doffset, int accumulate, void* ws, int N,
                      int H, int W, int C, int Ho, int Wo, int R, int S, int stride, int pad, int off_stride, void* stream);
/* to_ohwi = 1: dst[O][T][C] = scale * src[O][C][T]; 0: dst[O][C][T] = scale * src[O][T][C] */
int dbn_permute_weight(const float* src, float* dst, int O, int C, int T, int to_ohwi, float scale, void* stream);

/* ---- array work of SegDetectorRepresenter ahead of the (host, unchanged) OpenCV contour code ---- */
/* postprocess.py:51-52 `pred > thresh` on channel 0 of pred[N][channels][H][W], as a uint8 {0,1} bitmap out[N][H][W]
 * (H*W % 4 == 0): the D2H copy the contour tracer needs shrinks 4x. */
int dbn_binarize_u8(const float* pred, int N, int channels, int H, int W, float thresh, unsigned char* out, void* stream);
/* postprocess.py:186-198 box_score_fast for K boxes at once: scores[k] = mean of bitmap[H][W] over the cv2.fillPoly
 * mask of boxes[k][P][2] (x, y; float, as produced by get_mini_boxes / approxPolyDP), P <= 64.  Polygons with fewer
 * vertices are padded by repeating the last vertex. */
int dbn_box_scores(const float* bitmap, int H, int W, const float* boxes, int K, int P, float* scores, void* stream);

/* ---- ground truth of data_loaders.py:87-172 on the device (csrc/gtmaps.hip, db_text_minimal_amd/gt_maps.py) ---- */
/* The four maps of train.py GT_KEYS for N images of S x S pixels: out[4][N][S][S] fp32 (prob_map, supervision_mask,
 * thresh_map, text_area_map).  P polygons, image by image: polygons img_off[n] .. img_off[n+1]-1 belong to image n.
 * meta[P][20] int32 per polygon: 0 first vertex in verts (fp64 (x, y) pairs), 1 vertex count (<= 64), 2 ignored flag,
 * 3/4 first point / count in ixy (int32 (x, y) pairs) of the shrunk polygon (the truncated source polygon if ignored),
 * 5/6 first point / count in ixy of the padded polygon, 7-10 the box x0 x1 y0 y1 of pixels the polygon may touch
 * (clamped to the image; empty if x1 < x0), 11-14 the padded polygon's bbox xmin xmax ymin ymax, 15-18 the bbox of
 * the shrunk (or truncated) polygon, 19 unused.  dist[P] = D of each polygon (fp64).  max_verts / max_off_pts: bounds
 * on the vertex counts (meta 1) and ixy counts (meta 4, 6) of every polygon, refused above 64 / 1024.  Precondition: no
 * count exceeds them (the Python layer passes the batch's maxima and refuses larger polygons before the call); the kernel
 * draws nothing for a polygon that breaks it, it never clips one.  thresh_map = canvas * scale + tmin in fp32. */
int dbn_gt_maps(const double* verts, const double* dist, const int* meta, const int* img_off, const int* ixy, int N, int P, int S,
                int max_verts, int max_off_pts, float scale, float tmin, float* out, void* stream);
/* uint8 in[N][H][W][3] -> fp32 out[N][3][H][W] = (float)in - m_c (data_loaders.py:161-167; the reference's means in
 * image channel order) */
int dbn_normalize_u8(const unsigned char* in, int N, int H, int W, float m0, float m1, float m2, float* out, void* stream);
/* host: Clipper 6 ClipperOffset (JT_ROUND, ET_CLOSEDPOLYGON, ArcTolerance 0.25) of the closed path xy[n][2] by *delta
 * (fp64, by pointer), coordinates cast to integers toward zero as pyclipper converts them.  Writes the piece of largest
 * area to out_xy[*out_n][2] (*out_n = 0: the offset vanished); returns 1 with *out_n = the needed count if it exceeds
 * cap.  PARITY UNPINNED against pyclipper. */
int dbn_poly_offset(const double* xy, int n, const double* delta, int* out_xy, int cap, int* out_n);
/* host: dbn_poly_offset, and *out_paths = the number of paths Clipper's Execute returns (outer loops and holes; 0 when
 * the offset vanishes).  dbn_poly_offset's own result is unchanged by it. */
int dbn_poly_offset_paths(const double* xy, int n, const double* delta, int* out_xy, int cap, int* out_n, int* out_paths);

/* ---- the loader's geometric stage on the device: flip + rotate, cubic resize of a crop window, letterbox + normalise
 *      (csrc/resample.hip, db_text_minimal_amd/augment.py).  PARITY UNPINNED against cv2 / imgaug. ---- */
/* uint8 HWC images, 3 channels, packed: image n is described by desc[n][12] int64 — 0 byte offset of its source in src,
 * 1/2 source height / width, 3 offset of its output in dst (bytes; elements of out for the linear stage, which needs 0),
 * 4/5 height / width of the whole resized image (the source size for the warp), 6/7 row / column of the window's origin in
 * it, 8/9 window height / width (what is computed and stored, row-major, at dst + 3); 10 flip (warp only), 11 unused — and
 * coef[n][6] fp64: the inverse affine map (warp), or scale_x, scale_y = 1 / ((double)dst / src) as cv2.resize computes
 * them.  A descriptor whose regions leave src_bytes / dst_bytes, or whose window leaves the resized image, is skipped.
 * max_h / max_w bound the windows (the grid).  All sizes <= 65535. */
/* cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) of the image (flipped left-right first if flip), output the size of
 * the input (window = the whole image). */
int dbn_warp_affine_u8(const unsigned char* src, long src_bytes, const long long* desc, const double* coef, int N, int max_h, int max_w,
                       unsigned char* dst, long dst_bytes, void* stream);
/* cv2.resize(INTER_CUBIC) of the image to desc 4 x 5, only the window 6-9. */
int dbn_resize_cubic_u8(const unsigned char* src, long src_bytes, const long long* desc, const double* coef, int N, int max_h, int max_w,
                        unsigned char* dst, long dst_bytes, void* stream);
/* cv2.resize(INTER_LINEAR) of the image to desc 4 x 5 (window 0, 0, desc 4, desc 5), written normalised into the top-left
 * corner of out[n][3][CH][CW] = (float)u8 - m_c, and -m_c over the rest of the canvas: every element written once. */
int dbn_resize_linear_norm_u8(const unsigned char* src, long src_bytes, const long long* desc, const double* coef, int N, int CH, int CW,
                              float m0, float m1, float m2, float* out, void* stream);

/* ---- word crops of detected boxes: test_ocr.py:160-177 (cv2.getPerspectiveTransform + cv2.warpPerspective per box;
 *      csrc/resample.hip, db_text_minimal_amd/word_crops.py).  PARITY UNPINNED against cv2. ---- */
/* host: for K quads quads[K][4][2] (fp32 (x, y), the corners mapped to (0, 0), (out_w, 0), (out_w, out_h), (0, out_h)),
 * fwd[K][9] = getPerspectiveTransform (fp64, row-major; a singular system gives zeros with fwd[8] = 1) and inv[K][9] = its
 * inverse as warpPerspective computes it (invert, DECOMP_LU: the zero matrix when the determinant is 0). */
int dbn_perspective_maps(const float* quads, int K, int out_h, int out_w, double* fwd, double* inv);
/* cv2.warpPerspective(INTER_LINEAR, BORDER_CONSTANT 0) of K crops into dst[K][out_h][out_w][3] uint8 (every byte
 * written; dst_bytes >= K * out_h * out_w * 3): crop k samples the uint8 HWC image desc[k][3] int64 = {byte offset in
 * src, height, width} through inv[k][9] (fp64, dbn_perspective_maps).  A descriptor that leaves src_bytes or whose sides
 * leave 1 .. 65535 gives a zero crop.  K > 0, sides <= 65535. */
int dbn_warp_perspective_u8(const unsigned char* src, long src_bytes, const long long* desc, const double* inv, int K, int out_h, int out_w,
                            unsigned char* dst, long dst_bytes, void* stream);

/* ---- word images of text polygons: a curved word straightened into out_h x out_w (csrc/rectify.hip,
 *      db_text_minimal_amd/word_crops.py).  THIS PROJECT'S DEFINITION, the reference crops boxes only. ---- */
/* host: the ribbons of K polygons, on min(K, 16, threads) threads.  Polygon k has the vertices xy[offs[k] .. offs[k + 1])
 * (fp64 (x, y), border order, either orientation; offs[0] = 0), 3 .. 256 of them, finite and within +-2^20; half = 1 needs
 * an even count.  Its 2n boundary points are the vertices and the edge midpoints (point 2i = vertex i).  half = 0: the ends
 * are the non-adjacent pair i < j whose two chains, sampled at segments + 1 equal arclength fractions, have the smallest
 * mean squared distance E (ties: the smallest (i, j)); half = 1: points 2n - 1 and n - 1.  knots[k][segments + 1][4] int32 =
 * round(1024 (Cx, Cy, W Nx, W Ny)): the centre line resampled at equal arclength, W the largest chain distance, N the unit
 * normal (-Ty, Tx); with half = 0 the knots start at the end with the smaller x (y, if the line is taller than wide).
 * valid[k] = 0 and zero knots: a centre line of no length, W = 0, no area, or a value beyond int32.  ends[k][2] = (i, j) as
 * found, info[k][3] = {E, W, length of the centre line}.  segments 4 .. 64; 1 for any argument outside its range. */
int dbn_polygon_ribbons(const double* xy, const long long* offs, int K, int segments, int half, int threads, int* knots,
                        unsigned char* valid, int* ends, double* info);
/* device: the same ribbons with the same bits, one launch (none for K = 0), one workgroup per polygon.  All
 * pointers are device pointers with dbn_polygon_ribbons' layouts; xy holds total_vertices vertices.  The call checks K,
 * segments, half, total_vertices >= 0 and the pointers; the kernel checks what they hold: a polygon with offs[k] < 0,
 * offs[k + 1] > total_vertices, a vertex count outside 3 .. 256 (odd with half = 1) or a coordinate that is not within
 * +-2^20 gets valid 0, zero knots, ends (-1, -1) and info 0, and nothing outside xy is read.  Every output byte of every
 * polygon is written. */
int dbn_polygon_ribbons_device(const double* xy, const long long* offs, int K, long total_vertices, int segments, int half, int* knots,
                               unsigned char* valid, int* ends, double* info, void* stream);
/* K crops into dst[K][out_h][out_w][3] uint8 (every byte written; dst_bytes >= K * out_h * out_w * 3), one launch (none
 * for K = 0): crop q samples the uint8 HWC image desc[q][3] int64 = {byte offset in src, height, width} along the ribbon
 * knots[q][segments + 1][4] (dbn_polygon_ribbons' layout; any int32 values).  Pixel (x, y): k = x segments div out_w, r = x
 * segments mod out_w, c = out_w c_k + r (c_k+1 - c_k), n likewise, P = floor((2 out_h c + (2 y - out_h) n + out_h out_w) /
 * (2 out_h out_w)) per axis in 64-bit integers, P5 = (P + 16) >> 5, tap P5 >> 5 with the weights (32 - f | f), f = P5 & 31,
 * of the 2 x 2 taps (outside the image: 0), (sum + 512) >> 10.  valid[q] = 0, or a descriptor that leaves src_bytes or
 * 1 .. 65535 a side, gives a zero crop.  Sides <= 65535 and out_h * out_w <= 2^30, which keeps every term below 2^63. */
int dbn_rectify_u8(const unsigned char* src, long src_bytes, const long long* desc, const int* knots, const unsigned char* valid, int K,
                   int segments, int out_h, int out_w, unsigned char* dst, long dst_bytes, void* stream);

/* ---- showing a detection result: utils.draw_bbox + the heat-map overlay of utils.visualize_polygon / visualize_heatmap
 *      (utils.py:110-113,202-283; csrc/render.hip, db_text_minimal_amd/render.py).  Thick strokes are this project's
 *      definition, the resize is PARITY UNPINNED against cv2. ---- */
/* cv2.polylines(isClosed) of E edges, one colour: dst = src (bytes bytes of packed uint8 HWC images; src may be dst, then
 * nothing is copied), then every pixel of image edges[e][0] within thickness / 2 of the closed segment edges[e][1..4] =
 * (xa, ya, xb, yb) is set to (c0, c1, c2); thickness 1 paints the 8-connected line of fillPoly's border instead.
 * desc[n][3] int64 = {byte offset of image n, height, width}.  Vertices within +-2^20, 1 <= thickness <= 255; an edge
 * whose image, descriptor or vertices break this is skipped.  E may be 0. */
int dbn_draw_strokes(const unsigned char* src, unsigned char* dst, long bytes, const long long* desc, int N, const int* edges, long E,
                     int thickness, int c0, int c1, int c2, void* stream);
/* Labels: the cv2.putText step of test_ocr.py:197-210, as filled glyph outlines (THIS PROJECT'S DEFINITION: DejaVu Sans,
 * non-zero winding at pixel centres in exact integers, on or off; PARITY UNPINNED against cv2's Hershey strokes, DESIGN.md
 * 29).  dst = src (as dbn_draw_strokes; src may be dst), then for each of R instances recs[r][5] = {image, glyph, pen,
 * org x, org y} every pixel (px, py) of the image whose centre has a non-zero winding number about the glyph's contours is
 * set to (c0, c1, c2).  On the lattice of 1 / (64 * 2048) pixel a vertex v sits at v * size64 and the centre at
 * (((64 px + 32) - 64 org x) * 2048 - pen * size64, (64 org y - (64 py + 32)) * 2048); edge a -> b counts +1 if
 * ay <= Py < by and cr > 0, -1 if by <= Py < ay and cr < 0, cr = (bx - ax)(Py - ay) - (by - ay)(Px - ax).
 * edges[E][4] = {ax, ay, bx, by} and glyphs[G][6] = {first edge, edges, xmin, ymin, xmax, ymax} in font units (the box
 * holds every edge of the glyph; only pixels with their centre inside it are tested); desc as dbn_draw_strokes.
 * 0 <= pen <= 2^20, |org| <= 2^20, at most 512 edges per glyph, (xmax - xmin) size64 < 2^35, (ymax - ymin) size64 < 2^27:
 * an instance whose image, descriptor, glyph or numbers break this is skipped.  rows: an upper bound of the pixel rows
 * of a glyph's box (sizes the grid; any value 1 .. 65535 gives the same bytes).  R may be 0.  No float arithmetic. */
int dbn_draw_glyphs(const unsigned char* src, unsigned char* dst, long bytes, const long long* desc, int N, const int* edges, long E,
                    const int* glyphs, int G, const int* recs, long R, int size64, int rows, int c0, int c1, int c2, void* stream);
/* The heat map.  desc[n][5] int64 = {first pixel of image n in the packed run of n_px pixels, height, width, valid map
 * rows, valid map columns}; coef[n][4] fp64 = {scale_x, scale_y (1 / ((double)dst / src), as cv2.resize), vmin, vmax}.
 * Image n's map is prob + n * img_stride, rows row_stride floats apart, map_elems floats in all.  binary != 0: a tap
 * reads 1 where the map is > thresh, else 0.
 * dbn_render_minmax: mm[n] (8 bytes per image) = ordered keys of the minimum and maximum of the map resized to image n
 * (float INTER_LINEAR); the resized values are not stored. */
int dbn_render_minmax(const long long* desc, const double* coef, int N, long n_px, const float* prob, long map_elems, long img_stride,
                      int row_stride, int binary, float thresh, void* mm, void* stream);
/* dst pixel = rint(src pixel * (1 - alpha) + lut[index] * alpha), index = matplotlib's Normalize + Colormap index of the
 * resized map value with the limits of mm (dbn_render_minmax) or, mm NULL, of coef.  lut: 256 x (r | g << 8 | b << 16).
 * Every byte of dst is written once; src may be dst; 0 <= alpha <= 1. */
int dbn_render_paint(const unsigned char* src, unsigned char* dst, const long long* desc, const double* coef, int N, long n_px, const float* prob,
                     long map_elems, long img_stride, int row_stride, int binary, float thresh, const void* mm, const void* lut, float alpha,
                     void* stream);
/* utils.minmax_scaler_img: x [N][3][H][W] fp32 -> out [N][H][W][3] = (uint8)((x - min) * (1 / (max - min) * 255)) in
 * float32 per image, truncated; a constant image gives zeros.  mm: 8 bytes per image of workspace. */
int dbn_minmax_scale_u8(const float* x, int N, int H, int W, void* mm, unsigned char* out, void* stream);

/* ---- around a text recogniser: rec_preprocess and predict() of test_ocr.py:59-108,179-200, batched (csrc/recognise.hip,
 *      db_text_minimal_amd/recognise.py).  at: storage type of the floating tensor (0 fp32, 1 bf16, 2 fp16). ---- */
/* crops [K][h][w][3] uint8 (n_px = K * h * w pixels, hw = h * w) -> out [K][1][h][w] (rgb = 0: PIL's convert('L') in
 * integers, (19595 c0 + 38470 c1 + 7471 c2 + 32768) >> 16; bgr != 0 swaps the weights of c0 and c2) or [K][3][h][w]
 * (rgb != 0, planar, the crop's channel order), each value lut[byte]: lut = 256 fp32 on the device, (g / 255 - 0.5) / 0.5
 * as the caller rounds it; the 16-bit types store its round-to-nearest-even conversion.  Every element written. */
int dbn_words_to_input(int at, const unsigned char* crops, long n_px, long hw, int rgb, int bgr, const float* lut, void* out, void* stream);
/* bytes of workspace dbn_greedy_decode needs (8 per step) */
long dbn_greedy_decode_ws_bytes(int B, int T);
/* Greedy decode of logits [B][T][C] (contiguous, widened to fp32 exactly), two launches, no host synchronisation.  Per step
 * t < len_b (lengths[b] clamped to 0 .. T; lengths NULL: T): m = max_c x, k_t = the smallest index with x == m,
 * p_t = 1 / sum_c expf(x_c - m) in fp32; a row with a NaN gives k_t = the index of its first NaN and p_t = NaN.
 * mode 0 (CTC): step t is kept iff k_t != 0 and (t == 0 or k_t != k_{t-1}); score = the product of p_t over all len_b steps.
 * mode 1 (attention): the steps before the first k_t == 1 are kept; score = the product of their p_t (1.0 for none).
 * The product is formed in fp32 in ascending t.  codes [B][T]: the kept k_t packed to the left, then -1; count [B];
 * score [B]; every element written.  ws: dbn_greedy_decode_ws_bytes(B, T) bytes, any contents. */
int dbn_greedy_decode(int at, const void* logits, int B, int T, int C, const int* lengths, int mode, void* ws, int* codes, int* count,
                      float* score, void* stream);

/* ---- edit distances between strings of classes: text scoring and lexicon correction (csrc/lexicon.hip,
 *      db_text_minimal_amd/spotting.py).  A string is a run of bytes, one class 0 .. 254 each; class 255
 *      matches nothing, not even itself.  Distance: unit-cost Levenshtein (insert, delete, substitute), exact. ---- */
/* P independent pairs, one launch, one wave per pair.  Pair p: the pattern is row p of pattern [P][T] (1 <= T <= 64), its
 * first pat_len[p] classes (clamped to 0 .. T); the text is the text_len[p] bytes (text_len NULL: text_off[p + 1] -
 * text_off[p]) from byte text_off[p] of text, of any length.  text holds n_text bytes, and no byte outside it is read
 * whatever the two tables hold (offset and length are clamped).  dist [P]: every element written. */
int dbn_edit_distance_pairs(const unsigned char* pattern, int T, const int* pat_len, const unsigned char* text, long n_text, const int* text_off,
                            const int* text_len, int P, int* dist, void* stream);
/* bytes of workspace dbn_lexicon_nearest needs (8 per query) */
long dbn_lexicon_ws_bytes(int K);
/* K queries against a lexicon on the device, three launches, no host synchronisation.  Query k: row k of query [K][T]
 * (1 <= T <= 64), its first qlen[k] classes (clamped to 0 .. T), searched in group group[k] (group NULL: group 0).
 * The lexicon: NB blocks of 64 entry slots, ordered by (group, length); group g owns the blocks grp_blk[g] ..
 * grp_blk[g + 1] - 1 (grp_blk [G + 1]; max_blocks = the largest such count).  Block b holds a multiple of four positions
 * of 64 bytes each from byte blk_off[b] of data, position-major: byte blk_off[b] + pos * 64 + lane is class pos of slot
 * b * 64 + lane; ent_len [NB * 64] is the slot's length (at most the block's positions; -1: a padding slot) and ent_idx
 * [NB * 64] its index in the caller's order.  index [K], dist [K]: the entry of the group with the smallest distance and,
 * among equals, the smallest ent_idx, and that distance; (-1, -1) where the group is empty or outside 0 .. G - 1.  Every
 * element written; two runs agree in every bit.  ws: dbn_lexicon_ws_bytes(K) bytes, 8-byte aligned, any contents. */
int dbn_lexicon_nearest(const unsigned char* query, int T, const int* qlen, const int* group, int K, const unsigned char* data, const int* blk_off,
                        const int* ent_len, const int* ent_idx, const int* grp_blk, int G, int NB, int max_blocks, void* ws, int* index, int* dist,
                        void* stream);

/* ---- text boxes from probability maps: boxes_from_bitmap of postprocess.py:105-141 (csrc/detect.hip,
 *      db_text_minimal_amd/postprocess.py detect_boxes).  PARITY UNPINNED against cv2 / pyclipper. ---- */
/* One record per candidate (72 bytes):
 *   struct dbn_detect_rec { int root, hull_n, ex, ey; long long dmin, dmax, cmin, cmax, sum_hi, sum_lo, count; };
 * root: raster index y*W+x of the component's first pixel (-1: empty slot); hull_n: vertices of the convex hull of its
 * pixel centres (-1: hull buffer overflow); the min-area rectangle R1 of that hull has a side along the integer edge
 * vector (ex, ey) and spans dot((ex, ey), v) over [dmin, dmax], cross((ex, ey), v) over [cmin, cmax]; the sum of pred
 * over the filled component is sum_hi * 2^-24 + sum_lo * 2^-56 over `count` pixels (fixed point; pred clamped to
 * [-127, 127], bits below 2^-56 dropped). */
/* bytes of workspace dbn_detect needs */
long dbn_detect_ws_bytes(int N, int H, int W, int max_candidates);
/* Device stage for pred[N][channels][H][W] (fp32, channel 0 used), bitmap = pred > thresh, H, W <= 16384:
 * labels[N][H][W] int32 = root (raster index of the first pixel) of each pixel's component, foreground 8-connected,
 * background 4-connected; counts[n] = number of foreground components; recs[N][max_candidates] dbn_detect_rec, slot k
 * of image n = the foreground component with the k-th LARGEST root (k < min(counts[n], max_candidates)).  No float
 * atomics: bitwise reproducible.  ws: dbn_detect_ws_bytes(...) bytes, any contents. */
int dbn_detect(const float* pred, int N, int channels, int H, int W, float thresh, int max_candidates, void* ws, int* labels, void* recs,
               int* counts, void* stream);
/* host: postprocess.py:118-140 on the records of dbn_detect (host memory).  params = {box_thresh, unclip_ratio} (fp64),
 * dest_hw[N][2] = (height, width) to scale to.  Writes, for k < min(counts[n], max_candidates), boxes[n][k][4][2] int16
 * and scores[n][k] fp32 (zero for a skipped candidate); info (NULL or [N][max_candidates][10] fp32): R1's four corners,
 * min side of R1, score of every candidate. */
int dbn_detect_host(const void* recs, const int* counts, int N, int max_candidates, int H, int W, const double* params, const int* dest_hw,
                    short* boxes, float* scores, float* info);

/* ---- text polygons: polygons_from_bitmap of postprocess.py:54-103 (csrc/detect.hip, db_text_minimal_amd/postprocess.py
 *      detect_polygons).  PARITY UNPINNED against cv2 / pyclipper. ---- */
/* bytes of the contour workspace dbn_detect_poly needs besides dbn_detect's (about 71 B per pixel) */
long dbn_detect_poly_ws_bytes(int N, int H, int W, int max_candidates);
/* capacity of the packed vertex buffer, in (x, y) int16 pairs: N * (2 H W + H + W), the unit edges of the pixel grid */
long dbn_detect_poly_verts_cap(int N, int H, int W);
/* Device stage: dbn_detect (ws: dbn_detect_ws_bytes, labels as there), then the outer border of every kept candidate,
 * traced in parallel (cracks, successors, Wyllie pointer jumping, CHAIN_APPROX_SIMPLE compression).
 * table: recs [N][max_candidates] dbn_detect_rec | counts [N] int | nv [N][max_candidates] int (compressed vertices of
 * the candidate's outer border, 0 for an empty slot) | voff [N][max_candidates] int (offset of its first vertex in
 * verts) | info [4] int {total vertices, cracks, pointer-jumping rounds run, rounds launched}.
 * verts: dbn_detect_poly_verts_cap pairs; the first info[0] are written, (x, y) int16, per candidate from its
 * raster-first pixel, counter-clockwise on screen.  poly_ws: dbn_detect_poly_ws_bytes, any contents. */
int dbn_detect_poly(const float* pred, int N, int channels, int H, int W, float thresh, int max_candidates, void* ws, void* poly_ws,
                    int* labels, void* table, short* verts, void* stream);
/* host: postprocess.py:72-101 on the table and vertices of dbn_detect_poly (host memory).  params = {box_thresh,
 * unclip_ratio} (fp64), dest_hw[N][2] = (height, width) to scale to.  Per slot: poly_n (0: skipped), poly_off (first
 * vertex in poly_xy), the scaled unclipped polygon as int32 (x, y) pairs in poly_xy, scores fp64 (0: skipped).
 * Returns 1 with *poly_total = the vertices needed when they exceed poly_cap.  info (NULL or [N][max_candidates][4]
 * fp64): score, approxPolyDP vertices, offset paths, shorter side of the unclipped min-area rectangle (-1: not reached);
 * approx_xy (NULL or info[0] int32 pairs): the approxPolyDP vertices, at voff. */
int dbn_detect_poly_host(const void* recs, const int* counts, const int* nv, const int* voff, const short* verts, int N, int max_candidates,
                         int H, int W, const double* params, const int* dest_hw, int* poly_n, int* poly_off, int* poly_xy, int poly_cap,
                         int* poly_total, double* scores, double* info, int* approx_xy);

/* ---- Text-detection scoring (csrc/det_eval.hip): the overlap matrices of the reference's evaluators
 *      (src/iou.py, src/deteval.py) and their matching protocols.  Polygons are oriented so that their shoelace signed area is
 *      >= 0; area = |signed area|; overlap(A, B) = the integral of w_A * w_B (winding numbers), exactly area(A n B) for simple
 *      polygons, a winding-weighted overlap for non-simple ones (flagged).  Exact predicates with symbolic perturbation. ---- */
/* bytes of the dbn_det_eval_overlaps workspace (48 per polygon) */
long dbn_det_eval_ws_bytes(int n_polys);
/* verts: (x, y) fp64 pairs of every polygon of the batch, packed; poff [n_polys + 1] int: polygon k is verts[poff[k] ..
 * poff[k + 1]), at least 3 vertices; img [N][5] int64 = {first GT polygon, G, first detection polygon, D, pair offset} with
 * pair offset = sum over earlier images of G * D; n_pairs = the sum over all images.  Outputs: inter [n_pairs] fp64, per image the
 * row-major G x D overlap matrix at its pair offset; area [n_polys] fp64; nonsimple [n_polys] int (1: two non-adjacent edges
 * touch or cross, two adjacent edges overlap collinearly, or fewer than 3 non-zero edges).  cull = 0 computes pairs with
 * disjoint bounding boxes too (measurement only; the product culls).  ws: dbn_det_eval_ws_bytes, any contents. */
int dbn_det_eval_overlaps(const double* verts, const int* poff, int n_polys, const long long* img, int N, long n_pairs, int cull, void* ws,
                          double* inter, double* area, int* nonsimple, void* stream);
/* host: per image what the reference's evaluate_image computes from the overlaps (host memory).  protocol 0: iou.py
 * (params {iou_constraint, area_precision_constraint}), 1: deteval.py (params {area_recall_constraint,
 * area_precision_constraint, ev_param_ind_center_diff_thr, mtype_oo_o, mtype_om_o, mtype_om_m}).  sizes [N][2] = (G, D);
 * inter as dbn_det_eval_overlaps writes it; gt_area / gt_ignore / gt_cd packed over the images' GT polygons, det_area / det_cd
 * over the detections; *_cd [.][3] = vertex mean x, y and bounding-box diagonal as deteval.py computes them (protocol 1 only).
 * Outputs: stats [N][8] = {precision, recall, hmean, gtCare, detCare, detMatched, recallAccum, precisionAccum}; det_dc [D]
 * (1: don't care); rows: per image from 2 * sum over earlier images of (G + D), n_rows[n] records {pair, kind, gt, det}
 * (kind 0: one-to-one, 1: one-to-many (gt, its dets; det -1 for an empty list), 2: many-to-one (gts -1 likewise)). */
int dbn_det_eval_match_host(int protocol, int N, const int* sizes, const double* inter, const double* gt_area, const double* det_area,
                            const unsigned char* gt_ignore, const double* gt_cd, const double* det_cd, const double* params, double* stats,
                            unsigned char* det_dc, int* rows, int* n_rows);


/* =====================================================================================================================
 * Activation storage types (BASELINE configs[2]-[4]).  Every entry point above that moves activation tensors has a `_t`
 * form with the storage type first: DBN_AT_F32 (0, the fp32 contract above), DBN_AT_BF16 (1: activations, their gradients
 * and the weight panels are stored in bf16 in HBM; bf16 MFMA, fp32 accumulators / BatchNorm statistics / loss sums / weight
 * gradients / master weights), DBN_AT_F16 (2: fp16 inference).  Tensors typed `void*` are stored in that type; everything
 * typed `float*` stays fp32.  The reference has one dtype (fp32, src/train.py:96-98); these are the native data paths of the
 * reduced-precision configurations.
 * ===================================================================================================================== */
#define DBN_AT_F32 0
#define DBN_AT_BF16 1
#define DBN_AT_F16 2
/* conv / weight-gradient entry points only, with ns = 3 (bf16x3): the source operand(s) are PRE-SPLIT fp32 tensors — three
 * bf16 planes [3][N,H,W,C] with a0 + a1 + a2 == a exactly, made by dbn_split3 — gathered without conversion; dst stays fp32 */
#define DBN_AT_SPLIT3 3
int dbn_split3(const float* src, void* planes, long n, void* stream);

/* weight panels: kind 0 fp32, 1 bf16, 3 bf16x3 (three bf16 planes), 2 fp16.  cs: channels of the source tensor for mode 0
 * (0: I rounded up to 4; the 16-bit model input is stored with 16 channels) */
long dbn_igemm_panel_floats_t(int kind, int O, int I, int R, int S, int mode, int stride, int cs);
int dbn_pack_weights_t(int kind, const float* w_oihw, int O, int I, int R, int S, int mode, int stride, int cs, float* out, void* stream);

/* dbn_igemm_f32 / _bf16s / _splitk_f32 in one: at = storage of src / dst (16-bit storage: ns = 1, Cs % 16 == 0), ns = matrix math
 * (0 exact fp32, 1 one 16-bit plane, 3 bf16x3), ksplit > 1 with `slab` (ksplit * (N*Hd*Wd*Cd + 1088) floats) = split-K */
int dbn_igemm_t(int at, int ns, const void* src, const float* wpk, const float* bias, void* dst, int N, int Hs, int Ws, int Cs, int Hd,
                int Wd, int Cd, int R, int S, int stride, int pad, int mode, int accumulate, int tile_hint, int ksplit, float* slab,
                void* stream);
/* dbn_conv_bn_f32 with typed tensors; the BatchNorm statistics are those of the fp32 accumulators (before the storage rounding) */
int dbn_conv_bn_t(int at, const void* src, const float* wpk, const float* bias, void* dst, int N, int Hs, int Ws, int Cs, int Hd, int Wd,
                  int Cd, int R, int S, int stride, int pad, int mode, int accumulate, int tile_hint, int ns,
                  const float* gamma, const float* beta, float eps, float momentum, float* run_mean, float* run_var,
                  float* scale, float* shift, float* save_mean, float* save_rstd, float* ws, void* stream);
int dbn_pyramid_conv_t(int at, const void* s0, const void* s1, const void* s2, const void* s3, const float* w0, const float* w1,
                       const float* w2, const float* w3, const float* bias, void* dst, int N, int H, int W, int Cs, int Cd,
                       int tile_hint, int ns, const float* gamma, const float* beta, float eps, float momentum, float* run_mean,
                       float* run_var, float* scale, float* shift, float* save_mean, float* save_rstd, float* ws, void* stream);
/* first_level = 1 (at = 0 with ns = 0, or 16-bit storage with ns = 1): dst already holds level 0's part (the 3x3 conv of s0 with the bias —
 * dbn_winograd_conv_bn_f32, or dbn_igemm_t in mode 1 with the level-0 panel, which takes the 16-bit pixel-patch kernel);
 * the launch adds levels 1-3 (s0, w0, bias unused).  first_level = 0: dbn_pyramid_conv_t. */
int dbn_pyramid_conv_from_t(int first_level, int at, const void* s0, const void* s1, const void* s2, const void* s3, const float* w0,
                            const float* w1, const float* w2, const float* w3, const float* bias, void* dst, int N, int H, int W, int Cs,
                            int Cd, int tile_hint, int ns, const float* gamma, const float* beta, float eps, float momentum,
                            float* run_mean, float* run_var, float* scale, float* shift, float* save_mean, float* save_rstd, float* ws,
                            void* stream);
/* weight gradient with typed dY (sm) and X (big): at = 0 (any ns) or 1 (bf16, ns = 1); slabs and the gradient stay fp32 */
int dbn_wgrad_t(int at, int ns, const void* sm, const void* big, float* slab, float* grad_oihw, int N, int Ho, int Wo, int O, int H, int W,
                int Cb, int I, int R, int S, int stride, int pad, float scale, void* stream);

/* weight-gradient kernel selection (same results up to the summation order inside a split): 0 = defaults — fp32 tensors: the
 * register-transposing kernel; bf16 tensors: LDS-DMA panels + transposing LDS reads (wgrad_tr_kernel); 1 = LDS-DMA kernel for
 * exact-fp32 math on fp32 tensors (pixel-major LDS image, three-stage ring); 2 = the register-transposing kernel also where the
 * defaults take wgrad_tr_kernel or wgrad_patch_kernel (3x3 / stride-1 layers in the 16-bit matrix modes); 3 = the defaults with
 * the general per-pixel gather also where the block-wise k-tiles apply (measurements, tests) */
int dbn_set_wgrad_variant(int variant);
/* ConvTranspose2d(2x2, stride 2, padding 0) forward in exact fp32 (dbn_igemm_f32 / dbn_conv_bn_f32 with mode 1, stride 2, R = S = 2,
 * Cs in {16, 32, 48, 64}, no accumulate, tile_hint 0) runs as convt2x2_f32_kernel<Cs>: the input tile stays in LDS and the four output
 * parity classes are walked inside the workgroup.  0 routes these calls through the general parity-class launch again (tests, A/B);
 * returns the previous setting. */
int dbn_set_convt_kernel(int on);
/* tile variant as dbn_wgrad_tile_config, + 16 when the matrix kernel is wgrad_tr_kernel<BM,BN,2,2> (its rocprofv3 symbol) */
int dbn_wgrad_kernel_config(int at, int ns, int O, int J, int Cb);
/* ... with the layer geometry: + 32 when the matrix kernel is wgrad_patch_kernel<ns, at> (3x3 / stride 1, 16-bit matrix modes);
 * + 64 when wgrad_f32_kernel<BM,BN,2,2,ns,at,ROW> runs with ROW = 1: fp32 tensors whose output map tiles into 16x1, 8x2 or 4x4 pixel
 * blocks — the reduction then walks such blocks with scalar-offset addressing (same sum; 16x1 blocks: bit-identical to ROW = 0) */
int dbn_wgrad_kernel_config_hw(int at, int ns, int O, int Cb, int R, int S, int stride, int pad, int Ho, int Wo, int H, int W);
/* 0: route 3x3 / stride-1 convolutions of the 16-bit matrix modes through the generic gather loop instead of the pixel-patch
   form (A/B and test hook; returns the previous setting) */
int dbn_set_patch_conv(int on);
/* 1 (default): the 3x3 / stride-1 convolutions of the 16-bit storage types with 64 -> 64, 128 -> 128 or 256 -> 64 channels run in the
 * weight-resident kernel (csrc/wres16.hip: the panel in registers, the activations streamed row by row); 0: the pixel-patch kernel
 * again (test / A-B hook); 2: as 1, and also maps whose width is not a multiple of the kernel's 32-column strip (by default those stay
 * on the pixel-patch kernel, which is faster there; the tests of the ragged last strip use 2).  Returns the previous setting.
 * dbn_igemm_kernel_config reports such a launch with bit 64. */
int dbn_set_wres16(int on);
/* The 128 x 256 tile of the 16-bit storage types (Cd % 256 == 0; one column tile for the FPN output conv's 256 channels: half the gathered
 * activation bytes per output).  0: off (128 x 128); 1 (default): the pyramid conv on launches of >= 4096 such tiles (BASELINE configs[4]:
 * 25 600); 2: also plain forward / stride-1 data-gradient launches of the generic loop; 3: as 2 whatever the size (tests).  Per output
 * element the same products in the same order: bit-identical results.  Returns the previous setting (DBN_PYR_WIDE in the environment sets
 * the initial one). */
int dbn_set_pyramid_wide(int on);
int dbn_pyramid_wide_would_run(int at, int N, int H, int W, int Cs, int Cd); /* 1: such a pyramid conv call launches the 128 x 256 tile */
int dbn_wres16_would_run(int at, int mode, int N, int H, int W, int Cs, int Cd, int bnb, int y2); /* 1: such a call launches that kernel */

/* ---- measurement infrastructure (bench.py: roofline.peak_sustained): what the matrix pipe sustains on this box with non-zero
 * operands — the chip clocks to its power budget, far below the 2.4 GHz of the nominal peaks under back-to-back MFMAs (csrc/mfma_probe.hip).
 * kind 0: v_mfma_f32_32x32x2_f32, 1: ..._32x32x16_bf16, 2: ..._32x32x16_f16.  operands: 65536 bytes of values of that type; out: 524288
 * floats of scratch.  One launch (1024 workgroups x 8 waves, iters x 16 MFMAs per wave) of dbn_mfma_sustained_flops(kind, iters) FLOPs. */
int dbn_mfma_sustained(int kind, const void* operands, float* out, int iters, void* stream);
long dbn_mfma_sustained_flops(int kind, int iters);
/* First-round stagger of the exact-fp32 implicit-GEMM launches (workgroups sharing a CU start out of phase so that their prologues /
 * epilogues overlap other workgroups' MFMA loops), in permille of the nominal delay; 0 = off.  Returns the previous setting. */
int dbn_set_stagger(int permille);
/* 1: the implicit-GEMM workgroups run their prologue and epilogue at raised wave priority (s_setprio), so that they do not wait behind
 * the MFMA loops of the other workgroups on their CU; 0: everything at the default priority.  Returns the previous setting. */
int dbn_set_phase_priority(int on);
/* Diagnostic builds only (make TRACE=1: per-workgroup phase timestamps of the exact-fp32 implicit-GEMM kernels, tools/trace_probe.py);
 * the product library ignores the buffer and returns 0. */
int dbn_set_trace(void* buf, long max_blocks);
/* what one (unchunked) dbn_igemm_t call launches: tile configuration as dbn_igemm_tile_config, + 16 for the pixel-patch kernel
   (kmode: 0 forward, 1 stride-1 data gradient, 2 parity classes, 3 pyramid) — the template arguments of its rocprofv3 symbol */
int dbn_igemm_kernel_config(int at, int ns, int kmode, int N, int Hs, int Ws, int Cs, int Hd, int Wd, int Cd, int R, int S, int stride,
                            int pad, int tile_hint, int ksplit);
/* The slab reductions (phase 2) of many dbn_wgrad_phase_t calls in ONE launch.  dbn_wgrad_reduce_describe takes phase 2's
 * arguments and fills a host-side job record instead of launching (DBN_ERR_ARG for layers without the 64-channel reduction form:
 * the stem); the caller uploads the records and the prefix table of their `blocks` and calls dbn_wgrad_reduce_many.  Same sums
 * in the same order as the per-layer launches.  (A training step's side stream otherwise carries one small reduction behind
 * every weight-gradient kernel; conv / ConvTranspose weight gradients of resnet.py:70-91, basic.py:32-36, segmentation_head.py:24-29.) */
typedef struct dbn_wgrad_reduce_job {
    const float* slab;
    float* grad;
    int splitk, O, J, Jp, BM, BN, Cb, I, RS, G, natural, blocks;
    float scale;
    int smem_bytes;
} dbn_wgrad_reduce_job;
int dbn_wgrad_reduce_describe(int at, int ns, const void* sm, const void* big, float* slab, float* grad_oihw, int N, int Ho, int Wo, int O,
                              int H, int W, int Cb, int I, int R, int S, int stride, int pad, float scale, void* job);
int dbn_wgrad_reduce_many(const void* jobs, const int* first, int n_jobs, int total_blocks, int max_smem, void* stream);
/* tile variant of the weight-gradient kernel for O output channels, J = R*S*Cb columns: 1 = 64x192, 2 = 128x128, 3 = 64x128, 4 = 64x64 */
int dbn_wgrad_tile_config(int O, int J);
/* dbn_wgrad_t in two calls: phase 1 = matrix kernels (-> slabs), phase 2 = slab reduction (-> grad_oihw) */
int dbn_wgrad_phase_t(int phase, int at, int ns, const void* sm, const void* big, float* slab, float* grad_oihw, int N, int Ho, int Wo,
                      int O, int H, int W, int Cb, int I, int R, int S, int stride, int pad, float scale, void* stream);

/* deformable conv (resnet.py:54-65,111-124) on typed tensors: dcols, x, offset, dx and doffset all in the activation type `at` */
int dbn_deform_im2col_t(int at, const void* x, const void* offset, void* cols, int N, int H, int W, int C, int Ho, int Wo, int R, int S,
                        int stride, int pad, int off_stride, void* stream);
int dbn_deform_col2im_t(int at, const void* dcols, const void* x, const void* offset, void* dx, void* doffset, int accumulate, void* ws,
                        int N, int H, int W, int C, int Ho, int Wo, int R, int S, int stride, int pad, int off_stride, void* stream);
/* The same adjoint (the backward of torchvision.ops.DeformConv2d's sampling, resnet.py:61-65,119-124) as a GATHER in plain fp32 (round 5):
 * a team per input pixel searches the taps whose undeformed position lies within ceil(max |offset|) of it (the maximum is taken on the
 * device: no host synchronisation, larger offsets only widen the window) and adds their corner contributions in candidate order;
 * doffset is a per-sample reduction over the channels.  One fixed summation order: bit-reproducible; equal to dbn_deform_col2im_t up to
 * the fp32 rounding of the sums; non-finite dcols values reach exactly the elements their samples touch.  ws:
 * dbn_deform_col2im_gather_ws_bytes(N, Ho, Wo) bytes, no initialisation needed.  C <= 512, off_stride % 4 == 0, 9 <= R * S <= 32. */
long dbn_deform_col2im_gather_ws_bytes(int N, int Ho, int Wo);
int dbn_deform_col2im_gather_t(int at, const void* dcols, const void* x, const void* offset, void* dx, void* doffset, int accumulate,
                               void* ws, int N, int H, int W, int C, int Ho, int Wo, int R, int S, int stride, int pad, int off_stride,
                               void* stream);
/* out_bits[0] = bit pattern of max |offset| (0x7FC00000 if an element is not finite): what bounds the gather's window (n % 4 == 0) */
int dbn_deform_offset_absmax_t(int at, const void* offset, long n, unsigned* out_bits, void* stream);
int dbn_cast_f32(int at, const float* src, void* dst, long n, void* stream);

int dbn_bn_train_stats_t(int at, const void* y, int M, int C, const float* gamma, const float* beta, float eps, float momentum,
                         float* run_mean, float* run_var, float* scale, float* shift, float* save_mean, float* save_rstd,
                         float* ws, void* stream);
int dbn_bn_apply_t(int at, const void* y, const float* scale, const float* shift, const void* res, const float* res_scale,
                   const float* res_shift, void* out, long M, int C, int relu, void* stream);
/* The general BatchNorm backward: `sums` optional — [2*C][sums_parts] partial sums (or [2][C] with sums_parts = 1) of the masked
 * gradient and of masked gradient * xhat produced by the kernel that wrote dout (dbn_head_tail_bwd, dbn_bnrelu_maxpool_bwd_t,
 * dbn_igemm_bnsums_t); sums_parts = -1: `sums` is the FINALIZED pair [2][C] (sum / M, sum_xhat / M) of a dbn_bnb_final, dgamma /
 * dbeta are already written: only the apply pass runs.  dbias_conv optional as in dbn_bn_backward_ex */
int dbn_bn_backward_t(int at, const float* sums, int sums_parts, const void* y, const void* zmask, const float* mask_scale,
                      const float* mask_shift, const void* dout, const float* save_mean, const float* save_rstd, const float* gamma,
                      void* dy, void* gout, int gout_accumulate, float* dgamma, float* dbeta, float* dbias_conv, int M, int C,
                      float grad_scale, float* ws, void* stream);
int dbn_col_sum_t(int at, const void* x, int M, int C, float* out, float scale, float* ws, void* stream);
int dbn_bnrelu_maxpool_fwd_t(int at, const void* y, const float* scale, const float* shift, void* out, int N, int H, int W, int C,
                             void* stream);
/* bn_mean / bn_rstd / bn_part optional (all or none): also emit the partial sums of the BatchNorm backward that consumes dz,
 * bn_part = [2*C][dbn_maxpool_bwd_parts(N,H,W,C)] floats (needs 256 % (C/4) == 0) */
int dbn_maxpool_bwd_parts(int N, int H, int W, int C);
int dbn_bnrelu_maxpool_bwd_t(int at, const void* y, const float* scale, const float* shift, const void* pooled, const void* dpool,
                             void* dz, int N, int H, int W, int C, const float* bn_mean, const float* bn_rstd, float* bn_part,
                             void* stream);
/* The stem's pool with a RECORDED argmax (replaces nn.MaxPool2d(3, 2, 1) over relu(bn1(conv1(x))) and its autograd,
 * /root/reference/src/modules/resnet.py:167-172,231-235).  Forward: out as dbn_bnrelu_maxpool_fwd_t, plus idx [N,Ho,Wo,C] bytes — the position
 * 3 r + q of the window's FIRST maximum in scan order (PyTorch's rule), 15 where the pooled value is 0 — and ypool [N,Ho,Wo,C] (storage type),
 * the pre-BatchNorm value y at that position.  Backward: dy [N,H,W,C] = gradient at y given dpool, through pool, ReLU and the train-mode
 * BatchNorm, in one pass over y (the BatchNorm's two channel sums come from the pooled tensors); dgamma / dbeta are written (x grad_scale).
 * Needs 256 % (C/4) == 0; ws: dbn_maxpool_bn_backward_ws_floats(N,H,W,C) floats. */
int dbn_bnrelu_maxpool_fwd_arg_t(int at, const void* y, const float* scale, const float* shift, void* out, void* idx, void* ypool, int N, int H,
                                 int W, int C, void* stream);
long dbn_maxpool_bn_backward_ws_floats(int N, int H, int W, int C);
int dbn_maxpool_bn_backward_t(int at, const void* y, const void* dpool, const void* idx, const void* ypool, const float* save_mean,
                              const float* save_rstd, const float* gamma, void* dy, float* dgamma, float* dbeta, int N, int H, int W, int C,
                              float grad_scale, float* ws, void* stream);
int dbn_nearest_up_fwd_t(int at, const void* src, const void* addend, void* dst, int N, int Hs, int Ws, int C, int H, int W, int Cdst,
                         int coff, void* stream);
int dbn_nearest_up_bwd_t(int at, const void* dbig, void* dsrc, int N, int Hs, int Ws, int C, int H, int W, int Cbig, int coff,
                         int accumulate, void* stream);
/* x [N,3,H,W] fp32 -> [N,H,W,4] fp32 (at = 0) or [N,H,W,16] in the 16-bit type (channels 3.. zero) */
int dbn_nchw3_to_nhwc4_t(int at, const float* x, void* out, int N, int H, int W, void* stream);
/* ---- The stem convolution in 16-bit storage on a PACKED input (round 5; csrc/stem16.hip): Conv2d(3 -> 64, 7x7, stride 2, pad 3, no bias) of
 * modules/resnet.py:167-172,231-235.  The image is stored as xp [N][dbn_stem16_padded_h(H)][dbn_stem16_padded_w(W)][4] in the 16-bit type —
 * (r, g, b, 0) per pixel at offset (3, 3) inside a ZERO border the caller provides once (dbn_nchw3_to_padded4_t rewrites the interior only;
 * x4 non-NULL: also the packed [N][H][W][4] form, the X operand of the stem's weight gradient) — so the conv needs no bounds tests and
 * K = 7 x 8 x 4 = 224 instead of the 7 x 7 x 16 = 784 of the 16-channel-block form.  wpk: dbn_stem16_panel_bytes() bytes from
 * dbn_stem16_pack(kind 1 bf16 | 2 fp16, w [64][3][7][7] fp32).  y [N][(H-1)/2+1][(W-1)/2+1][64] in the 16-bit type.  gamma non-NULL: + the
 * train-mode BatchNorm that follows, as dbn_conv_bn_t (ws: (3 * 64 + 1) * dbn_stem16_rows() floats). */
int dbn_stem16_padded_h(int H);
int dbn_stem16_padded_w(int W);
int dbn_stem16_rows(void);
long dbn_stem16_panel_bytes(void);
int dbn_stem16_eligible(int at, int N, int H, int W);
int dbn_stem16_pack(int kind, const float* w_oihw, void* out, void* stream);
int dbn_nchw3_to_padded4_t(int at, const float* x, void* xp, void* x4, int N, int H, int W, void* stream);
int dbn_stem16_conv_bn_t(int at, const void* xp, const void* wpk, void* y, int N, int H, int W, const float* gamma, const float* beta, float eps,
                         float momentum, float* run_mean, float* run_var, float* scale, float* shift, float* save_mean, float* save_rstd,
                         float* ws, void* stream);
/* inference (round 5): out [N][Hq][Wq][64] = MaxPool2d(3, 2, 1)(relu(conv7x7/2 (xp) * scale + shift)) in ONE launch — the stem of
 * modules/resnet.py:231-235 in eval mode; scale / shift: the eval-mode BatchNorm coefficients (dbn_bn_eval_coef).  The 64-channel conv
 * output is never written.  Eligible: dbn_stem16_eligible and an even conv height Ho = (H - 1) / 2 + 1; Hq = (Ho - 1) / 2 + 1. */
int dbn_stem16_pool_eligible(int at, int N, int H, int W);
int dbn_stem16_conv_bn_relu_pool_t(int at, const void* xp, const void* wpk, const float* scale, const float* shift, void* out, int N, int H, int W,
                                   void* stream);
/* ---- ConvTranspose2d(64 -> 64, 2x2, stride 2) forward in 16-bit storage (round 5; csrc/convt16.hip): the head's up-sampling layers,
 * modules/segmentation_head.py:27-29,74-76.  x [N][H][W][64], y [N][2H][2W][64] in the 16-bit type; wpk: dbn_convt16_panel_bytes() bytes from
 * dbn_convt16_pack(kind 1 bf16 | 2 fp16, w [64][64][2][2] fp32 — the module's own [Cin][Cout][kh][kw] layout); bias [64] fp32 or NULL.
 * gamma non-NULL: + the train-mode BatchNorm that follows, as dbn_conv_bn_t (ws: (3 * 64 + 1) * dbn_convt16_rows() floats). */
int dbn_convt16_rows(void);
long dbn_convt16_panel_bytes(void);
int dbn_convt16_eligible(int at, int N, int H, int W, int Cin, int Cout);
int dbn_convt16_pack(int kind, const float* w_iohw, void* out, void* stream);
int dbn_convt16_bn_t(int at, const void* x, const void* wpk, const float* bias, void* y, int N, int H, int W, const float* gamma, const float* beta,
                     float eps, float momentum, float* run_mean, float* run_var, float* scale, float* shift, float* save_mean, float* save_rstd,
                     float* ws, void* stream);
/* ... and the same kernel as a pointwise conv 64 -> 64 | 256 on 16-bit storage, inference form (round 5): y [N][H][W][Cout] =
 * [relu](conv1x1(x [N][H][W][64]) + bias) — nn.Conv2d(64, Cout, 1) with the eval-mode BatchNorm folded into weight / bias (dbn_fold_bn_eval)
 * and the ReLU of modules/basic.py:32-36; the FPN lateral reduce_conv_c2 of resnet18, modules/segmentation_body.py:46,68.  Panel:
 * dbn_pw16_panel_bytes() bytes from the OIHW weight [Cout][64][1][1] (dbn_pw16_pack; kind 1 bf16, 2 fp16). */
int dbn_pw16_eligible(int at, int N, int H, int W, int Cin, int Cout);
long dbn_pw16_panel_bytes(void);
int dbn_pw16_pack(int kind, const float* w_oihw, int Cout, void* out, void* stream);
int dbn_pw16_act_t(int at, const void* x, const void* wpk, const float* bias, int relu, void* y, int N, int H, int W, int Cout, void* stream);
/* inference (round 5): the DB head's tail of BOTH branches in one launch — per branch ConvTranspose2d(64, 64, 2, 2) -> eval-mode BatchNorm ->
 * ReLU -> ConvTranspose2d(64, 1, 2, 2) -> Sigmoid (modules/segmentation_head.py:27-29,35-45,74-79): out [N][2][4 Hq][4 Wq] fp32 (channel 0 the
 * binarize branch, 1 the threshold branch); x_*: [N][Hq][Wq][64] in the activation type; panel_*: dbn_convt16_pack of the first ConvT;
 * scale / shift: dbn_bn_eval_coef of the BatchNorm behind it; w2_*: the second ConvT's weight [64][1][2][2], bias2_*: [1]. */
int dbn_head16_eligible(int at, int N, int Hq, int Wq);
int dbn_head16_tail_eval_t(int at, const void* x_b, const void* x_t, const void* panel_b, const void* panel_t, const float* bias1_b,
                           const float* bias1_t, const float* scale_b, const float* shift_b, const float* scale_t, const float* shift_t,
                           const float* w2_b, const float* w2_t, const float* bias2_b, const float* bias2_t, float* out, int N, int Hq, int Wq,
                           void* stream);

/* ... 16-bit storage: the 16-channel form and (out4 non-NULL) the packed 4-channel form of dbn_nchw3_to_nhwc4_packed_t in ONE launch */
int dbn_nchw3_to_nhwc16_and_4_t(int at, const float* x, void* out16, void* out4, int N, int H, int W, void* stream);
/* the same into [N,H,W,4] of the storage type (16-bit: 4 channels, not a 16-channel block): X operand of the stem weight gradient */
int dbn_nchw3_to_nhwc4_packed_t(int at, const float* x, void* out, int N, int H, int W, void* stream);
/* head tail with typed 64-channel inputs / input gradients; the maps, dpreds and the ConvT parameter gradients are fp32 */
int dbn_head_tail_fwd_t(int at, const void* xb, const void* xt, const float* wb, const float* wt, const float* bias_b,
                        const float* bias_t, const float* bn_scale_b, const float* bn_shift_b, const float* bn_scale_t,
                        const float* bn_shift_t, float* out, int N, int Hq, int Wq, int channels, float kstep, void* stream);
/* test / A-B hook: the 16-bit forward's lane layout — 0 by size (eight lanes x eight channels per pixel from 2^22 quarter pixels), 1 always,
 * -1 never; returns the previous setting */
int dbn_set_head_tail_wide(int mode);
int dbn_head_tail_bwd_t(int at, const void* xb, const void* xt, const float* wb, const float* wt, const float* preds,
                        const float* dpreds, const float* bn_scale_b, const float* bn_shift_b, const float* bn_scale_t,
                        const float* bn_shift_t, const float* bn_mean_b, const float* bn_rstd_b, const float* bn_mean_t,
                        const float* bn_rstd_t, float* bn_sums, void* dxb, void* dxt, float* dw_b, float* dbias_b, float* dw_t,
                        float* dbias_t, int N, int Hq, int Wq, int channels, float kstep, float grad_scale, float* ws, void* stream);
/* dbn_head_tail_bwd_t (with bn_sums) and the dbn_bn_backward_t of both branches' BatchNorm in front of the last ConvT (sums given, ReLU
 * mask recomputed from scale / shift, dbias_conv) as ONE call with the same results bit for bit: the two [N Hq Wq][64] gradients between
 * them are formed again inside the BatchNorm apply pass and never stored.  yb / yt: the BatchNorm inputs, dyb / dyt their gradients
 * (storage type `at`); dbias_conv_b / _t optional [64] (both or neither); ws: dbn_head_tail_bn_bwd_ws_floats() floats.
 * phases: 3 = the whole; 1 (sums pass, folds, finalize) then 2 (apply pass, bias fold) with the same arguments and workspace = the same
 * launches as two calls, for a caller that times the two passes separately. */
int dbn_head_tail_bn_bwd_ws_floats(void);
int dbn_head_tail_bn_bwd_t(int at, int phases, const void* yb, const void* yt, const float* wb, const float* wt, const float* preds, const float* dpreds,
                           const float* bn_scale_b, const float* bn_shift_b, const float* bn_scale_t, const float* bn_shift_t,
                           const float* bn_mean_b, const float* bn_rstd_b, const float* bn_mean_t, const float* bn_rstd_t,
                           const float* bn_gamma_b, const float* bn_gamma_t, void* dyb, void* dyt, float* dgamma_b, float* dbeta_b,
                           float* dgamma_t, float* dbeta_t, float* dbias_conv_b, float* dbias_conv_t, float* dw_b, float* dbias_b, float* dw_t,
                           float* dbias_t, int N, int Hq, int Wq, int channels, float kstep, float grad_scale, float* ws, void* stream);

/* ---- JPEG decode for the device pipeline (csrc/jpeg.hip): in the place of cv2.imread(path)[:, :, ::-1] (data_loaders.py:78, utils.py:179).
 * The entropy stage runs on the host, the rest (dequantise, libjpeg's slow-integer IDCT, fancy chroma upsampling, YCbCr -> RGB) on the device.
 * Status / support codes: 0 ok, 1 not a JPEG, 2 truncated, 3 progressive (SOF2), 4 arithmetic coding, 5 lossless / hierarchical, 6 sample
 * precision not 8 bits (12-bit), 7 4-component / Adobe-transform, 8 unsupported sampling factors, 9 non-interleaved multi-scan, 10 malformed
 * header or missing table, 11 invalid Huffman code, 12 coefficient run past index 63, 13 entropy data and markers disagree, 14 scan
 * script incomplete or longer than 100 scans (multiscan only).
 * dbn_jpeg_info: out[24] = {status, width, height, components, restart interval, Exif orientation (0: none), h0, v0, h1, v1, h2, v2, h3, v3,
 * SOF type, int16 coefficients needed (0 unless status 0), JFIF seen, Adobe transform (-1: no marker), precision, 0...}; reads data[0 .. len) only.
 * dbn_jpeg_coef_elems: streams n = blob[offs[n] .. offs[n + 1]); per_image[n] (may be NULL) and the returned sum count int16 coefficients.
 * dbn_jpeg_entropy_batch: Huffman-decodes the N streams on min(N, 16, threads) threads.  coef: per image and component the blocks of the
 * MCU-padded grid in raster order, 64 coefficients each in NATURAL order; desc int64 [N][24] = {coefficient offset (elements), width, height,
 * components, output byte offset, table offset (elements of qtabs), then per component c < 3 {block columns, block rows, h, v}, hmax, vmax,
 * MCU columns, MCU rows, status, restart interval}; qtabs uint16 [N][3][64] natural order, one per component; status int [N].  A stream that
 * fails keeps its (zeroed) slots and fails alone.
 * dbn_jpeg_pixels: the device stage, two launches on `stream`: packed uint8 [H][W][3] RGB per image at its output byte offset (grey replicated).
 * tab_idct int32 [n_idct][4] = {image, component, first block, 0}, one entry per 32 blocks; tab_rgb int32 [n_rgb][4] = {image, chunk of 1024
 * pixels, 0, 0}; planes: coef_elems bytes of workspace; coef and qtabs 16-byte aligned, planes 8-byte aligned.  Descriptors that would leave a
 * buffer are skipped.
 * The _ex forms take a flags word and the Exif orientation; with flags 0 and no oriented image they are the plain forms, which keep their
 * results.  flags 1 (multiscan): SOF2 progressive Huffman streams and SOF0 / SOF1 streams whose components come in several scans are decoded
 * too, into the same layout: a scan of one component walks that component's real block grid ceil(ceil(W h / hmax) / 8) x ceil(ceil(H v / vmax) / 8)
 * (its restart interval counts blocks), a scan of several walks MCUs; blocks no scan sends stay zero; a component's quantisation table is the
 * one in force at its first scan.  A scan header that breaks T.81's rules is status 10; status 14: the scan script is incomplete at EOI (a
 * coefficient never sent, or not refined to Al = 0) or longer than 100 scans.  dbn_jpeg_info_ex: out[19] = scans (multiscan only), SOF type 2
 * = progressive.  dbn_jpeg_entropy_batch_ex: orientation int [N] (may be NULL) receives every header's Exif tag.
 * dbn_jpeg_pixels_ex: orientation int32 [N] on the device; the images whose tag is 2 .. 8 are listed by the host in tab_tile int32 [n_tile][4] =
 * {image, tile row, tile column, 0} (32 x 32 tiles of the ORIENTED image) and not in tab_rgb, and are written turned as cv2.imread turns them,
 * [W][H][3] for tags 5 .. 8, in the same packed layout; one more launch on `stream`.  n_rgb or n_tile may be 0. */
int dbn_jpeg_info(const unsigned char* data, long len, long long* out);
int dbn_jpeg_info_ex(const unsigned char* data, long len, int flags, long long* out);
long dbn_jpeg_coef_elems_ex(const unsigned char* blob, const long long* offs, int N, int flags, long long* per_image);
int dbn_jpeg_entropy_batch_ex(const unsigned char* blob, const long long* offs, int N, short* coef, long coef_elems, long long* desc,
                              unsigned short* qtabs, int* status, int* orientation, int threads, int flags);
int dbn_jpeg_pixels_ex(const short* coef, long coef_elems, const long long* desc, const unsigned short* qtabs, int N, const int* tab_idct,
                       int n_idct, const int* tab_rgb, int n_rgb, const int* orientation, const int* tab_tile, int n_tile,
                       unsigned char* planes, unsigned char* out, long out_bytes, void* stream);
long dbn_jpeg_coef_elems(const unsigned char* blob, const long long* offs, int N, long long* per_image);
int dbn_jpeg_entropy_batch(const unsigned char* blob, const long long* offs, int N, short* coef, long coef_elems, long long* desc,
                           unsigned short* qtabs, int* status, int threads);
int dbn_jpeg_pixels(const short* coef, long coef_elems, const long long* desc, const unsigned short* qtabs, int N, const int* tab_idct,
                    int n_idct, const int* tab_rgb, int n_rgb, unsigned char* planes, unsigned char* out, long out_bytes, void* stream);

/* ---- JPEG encode behind the device pipeline (csrc/jpeg_enc.hip): in the place of the reference's imageio / Pillow writes (utils.py:225,272,280,
 * test_ocr.py:176,210, ts_request.py:38-39).  The decoder turned round: colour conversion, edge replication, chroma downsampling, libjpeg's
 * slow-integer forward DCT and quantisation on the device, Huffman coding (Annex K tables) on the host; the coefficient layout, the descriptor
 * and the tables of dbn_jpeg_entropy_batch are the hand-over.
 * dbn_jpeg_forward: two launches on `stream`.  pixels: in_bytes bytes that hold every image; desc int64 [N][24] as above, field 4 being the byte
 * offset of the image's first pixel in `pixels` (any alignment) and `components` 1 for uint8 [H][W] grey, 3 for uint8 [H][W][3] RGB; sampling
 * 1x1, 2x1 or 2x2 luma with 1x1 chroma, and the grids the size and the sampling give; qtabs uint16 [N][3][64] natural order (entries 1 .. 255).
 * tab_planes int32 [n_planes][4] = {image, chunk of 256 cells, 0, 0} over the image's 8 * MCU columns x 8 * MCU rows cells (a cell: hmax x vmax
 * pixels); tab_fdct int32 [n_fdct][4] = {image, component, first block, 0}, one entry per 32 blocks of the padded grid; planes: coef_elems bytes
 * of workspace, 8-byte aligned; coef (coef_elems int16) and qtabs 16-byte aligned.  Every block of the padded grid is written: a dummy block has
 * zero AC and the DC of the previous block in MCU order, as libjpeg codes it.  Entries that would leave a buffer are skipped.
 * dbn_jpeg_encode_bound: per_image[n] (may be NULL) and the returned sum: bytes a stream can need at most (header, 416 per block, 4 per
 * restart); 0 for a descriptor that cannot be encoded, -1 for bad arguments.  restart_interval: MCUs, 0 .. 65535.
 * dbn_jpeg_encode_batch: host; codes N images on min(N, 16, threads) threads.  Image n's stream (SOI, JFIF APP0, DQT, SOF0, DHT, DRI, SOS, one
 * interleaved scan, EOI) goes to out[offs[n] .. offs[n + 1]) (offs int64 [N + 1] ascending, offs[N] <= out_bytes), its length to lens[n]; no
 * byte outside an image's slot is written.  status[n]: 0 coded, 1 the descriptor's own status is not 0, 2 bad descriptor, 3 a quantisation
 * value outside 1 .. 255, 4 a DC difference of more than 11 bits, 5 an AC coefficient of more than 10 bits, 6 the slot is too small.  An image
 * that is not coded has length 0 and fails alone.  Coefficients are taken as given, dummy blocks included. */
int dbn_jpeg_forward(const unsigned char* pixels, long in_bytes, const long long* desc, const unsigned short* qtabs, int N,
                     const int* tab_planes, int n_planes, const int* tab_fdct, int n_fdct, unsigned char* planes, short* coef, long coef_elems,
                     void* stream);
long dbn_jpeg_encode_bound(const long long* desc, int N, int restart_interval, long long* per_image);
int dbn_jpeg_encode_batch(const short* coef, long coef_elems, const long long* desc, const unsigned short* qtabs, int N, int restart_interval,
                          unsigned char* out, long out_bytes, const long long* offs, long long* lens, int* status, int threads);
/* dbn_jpeg_optimal_table: freq int64 [256] -> bits uint8 [16], vals uint8 [256], *nvals: libjpeg's jpeg_gen_optimal_table (pseudo-symbol 256
 * of count 1, ties to the larger symbol, lengths limited to 16, symbols by length then value): the DHT of Pillow's optimize=True.
 * dbn_jpeg_encode_batch_opt: dbn_jpeg_encode_batch with `optimize`: not 0, each image is walked twice and carries its own tables in its DHT
 * segments; status 7: libjpeg's builder would give up (a code of more than 32 bits).  optimize 0 gives dbn_jpeg_encode_batch's bytes. */
int dbn_jpeg_optimal_table(const long long* freq, unsigned char* bits, unsigned char* vals, int* nvals);
int dbn_jpeg_encode_batch_opt(const short* coef, long coef_elems, const long long* desc, const unsigned short* qtabs, int N, int restart_interval,
                              unsigned char* out, long out_bytes, const long long* offs, long long* lens, int* status, int threads, int optimize);

/* ---- Huffman coding on the device (csrc/jpeg_huff.hip): the scans of dbn_jpeg_encode_batch(_opt) from coefficients in device memory, parallel
 * over the blocks of the batch in scan order; headers and EOI are the host's.  Tables travel as specs uint16 [4][273] (DC 0, AC 0, DC 1, AC 1:
 * symbols per length [16], symbol count, symbols [256]) and codes uint32 [4][256] (code | length << 16).
 * dbn_jpeg_huff_plan (host): status [N] (0, or the host coder's 1 / 2 / 3; such an image gets no blocks), blk_base / int_base int64 [N + 1] (first
 * scan block / restart interval of each image over the batch), sizes int64 [2] = bytes of workspace and of output dbn_jpeg_huff_code wants.
 * dbn_jpeg_huff_hist (device, one launch): hist uint32 [N][4][256], the symbol counts of each image's scan; errkey uint64 [N], all ones before
 * the first call, lowered to (first failing scan block << 3 | status 4 / 5, or 2 for a descriptor the kernel did not follow).
 * dbn_jpeg_huff_annex_k / dbn_jpeg_huff_tables (host): the Annex K set, or every image's own set from its histogram (status 7 as above).
 * dbn_jpeg_huff_code (device, nine launches, no synchronisation): res uint64 [2 N + 1] = errkey [N], offs [N + 1]; image n's entropy-coded
 * segment (stuffed, RSTn between intervals, ones-padded) is out[offs[n] .. offs[n + 1]).  coef, ws 16-byte aligned.
 * dbn_jpeg_huff_headers (host): SOI .. SOS of image n into out[704 n ..], lens[n] its length (0 where status[n] is not 0). */
int dbn_jpeg_huff_plan(const long long* desc, const unsigned short* qtabs, int N, long coef_elems, int restart_interval, long long* blk_base,
                       long long* int_base, int* status, long long* sizes);
int dbn_jpeg_huff_hist(const short* coef, long coef_elems, const long long* desc, int N, const long long* blk_base, long total_blocks,
                       int restart_interval, unsigned* hist, unsigned long long* errkey, void* stream);
int dbn_jpeg_huff_annex_k(unsigned short* specs, unsigned* codes);
int dbn_jpeg_huff_tables(const unsigned* hist, const long long* desc, int N, int* status, unsigned short* specs, unsigned* codes, int threads);
int dbn_jpeg_huff_code(const short* coef, long coef_elems, const long long* desc, int N, const long long* blk_base, const long long* int_base,
                       long total_blocks, long total_intervals, int restart_interval, const unsigned* codes, int per_image, void* ws, long ws_bytes,
                       unsigned char* out, long out_bytes, unsigned long long* res, void* stream);
int dbn_jpeg_huff_headers(const long long* desc, const unsigned short* qtabs, int N, int restart_interval, const unsigned short* specs, int per_image,
                          const int* status, unsigned char* out, long long* lens);

/* ---- Huffman decoding on the device (csrc/jpeg_dhuff.hip; host plan in csrc/jpeg.hip; shared layouts in csrc/jpeg_dhuff.h): the coefficients
 * of dbn_jpeg_entropy_batch from the compressed bytes in device memory, by subsequences of 1024 bits with the decoder state propagated to
 * a fixed point.
 * dbn_jpeg_stream_plan (host; reads no bit of the entropy data): desc / qtabs / status as dbn_jpeg_entropy_batch writes them from the headers
 * (same kinds, same codes); hspec uint8 [N][8][273] (DC 0 .. 3, AC 0 .. 3: present, symbols per length [16], symbols [256]); info int64 [N][8] =
 * {table ids (DC of component c in bits 8c .. 8c + 3, AC in 8c + 4 .. 8c + 7), host-only (the scan's markers are not the ones the header calls
 * for: a missing or extra marker, a wrong RSTn, fill bytes, the end of the data), first / end byte of the stream in the blob, first segment,
 * segments, first subsequence, subsequences}; seg int64 [segments][6] = {image, first byte, end byte (the FF of the marker behind it), first MCU,
 * MCUs, n of the RSTn in front or -1}, one row per restart interval; sub_base int64 [segments + 1], the first subsequence of each segment over
 * the batch; wgtab int32 [workgroups][4] = {image, first subsequence, count <= 256, 0}; counts int64 [4] = {segments, subsequences, workgroups,
 * int16 coefficients}.  seg == NULL: counts only (call twice).
 * dbn_jpeg_dhuff_ws_bytes: workspace for that many subsequences (two state buffers, block counts and their scan).
 * dbn_jpeg_dhuff (device; rounds + 5 launches and three memsets, no synchronisation): everything above in device memory, desc with the status in
 * field 22.  coef is zeroed and every planned image's slice written.  res uint64 [(rounds + 2) N]: res[n] all ones, or lowered to (subsequence
 * << 4 | reason) when image n's data or plan rows were not followed; res[(1 + r) N + n] != 0 when propagation launch r changed a state of image
 * n.  Image n is decoded when res[n] is all ones and res[(1 + rounds) N + n] == 0; any other image (and every host-only one) is the host
 * decoder's, whose status is the one to report.  ws 8-byte aligned. */
int dbn_jpeg_stream_plan(const unsigned char* blob, const long long* offs, int N, long long* desc, unsigned short* qtabs, int* status,
                         unsigned char* hspec, long long* info, long long* seg, long seg_cap, long long* sub_base, int* wgtab, long wg_cap,
                         long long* counts);
long dbn_jpeg_dhuff_ws_bytes(long nsub);
int dbn_jpeg_dhuff(const unsigned char* blob, long blob_len, const long long* desc, const unsigned char* hspec, const long long* info,
                   const long long* seg, const long long* sub_base, const int* wgtab, int N, long nseg, long nsub, int nwg, int rounds, short* coef,
                   long coef_elems, void* ws, long ws_bytes, unsigned long long* res, void* stream);

/* ---- PNG at both ends of the device pipeline (csrc/png.hip): zlib's inflate and deflate stay on the host (db_text_minimal_amd/png.py); the
 * scanline filters, Adam7, the sample conversions and the packing run on the device.  Pixels are cv2.imread's IMREAD_COLOR ones, as RGB.
 * desc int64 [N][32] per image = {width, height, bit depth, colour type, interlace, output byte offset, palette entries, status (not 0: the
 * image takes no bytes anywhere), src[8], raw[8], 0 ...}: src[s] / raw[s] are the byte offsets of sub-image s in the blob of filtered scanlines
 * and in the workspace of reconstructed ones; s = 0 is the whole image of a file that is not interlaced, s = 1 .. 7 the Adam7 passes of one
 * that is.  A sub-image of ph rows of rb bytes takes ph (rb + 1) bytes in the blob (a type byte, at most 4, in front of every row) and ph rows of
 * rb rounded up to 16 in the workspace; the sub-images lie end to end in both, in image and pass order, and the blob holds nothing else.  Output
 * offsets are packed in image order.  subs int32 [n_subs][2] =
 * {image, s}: the sub-images that hold bytes, one workgroup each.  Every entry point takes the descriptors twice, in host memory (hdesc,
 * hsubs), which it checks against the buffer lengths before anything is launched, and in device memory, which the kernels read.
 * dbn_png_check (host): the checks alone.  dbn_png_unfilter (one launch): blob is 4-byte aligned and blob_cap >= blob_len + 32 bytes are
 * allocated.  dbn_png_pixels (one launch): palettes uint8 [N][256][3]; packed uint8 [H][W][3] per image.
 * dbn_png_filter_rows (encode, one launch): desc int64 [N][8] = {input byte offset, H, W, channels (1 or 3), output byte offset, first row over
 * the batch, 0, 0}; out receives H rows of 1 + W channels bytes per image: the type byte and the filtered row.  filter 0 .. 4: that type for
 * every row; -1: per row the type whose sum of min(f, 256 - f) is lowest, the lowest type of equal ones. */
int dbn_png_check(const long long* hdesc, int N, const int* hsubs, int n_subs, long blob_len, long raw_bytes, long out_bytes);
int dbn_png_unfilter(const unsigned char* blob, long blob_len, long blob_cap, const long long* hdesc, const long long* desc, int N,
                     const int* hsubs, const int* subs, int n_subs, unsigned char* raw, long raw_bytes, long out_bytes, void* stream);
int dbn_png_pixels(const unsigned char* raw, long raw_bytes, const long long* hdesc, const long long* desc, const unsigned char* palettes, int N,
                   long blob_len, unsigned char* out, long out_bytes, void* stream);
int dbn_png_filter_rows(const unsigned char* pixels, long in_bytes, const long long* hdesc, const long long* desc, int N, int filter,
                        unsigned char* out, long out_bytes, void* stream);

/* ---- Photometric augmentation (csrc/photometric.hip, csrc/photometric.h; db_text_minimal_amd/photometric.py): torchvision's ColorJitter as
 * it acts on PIL images (Pillow's Image.blend, convert('L'), convert('HSV') and back), bit for bit, on packed uint8 [H][W][3] RGB images.
 * desc int64 [N][8] per image = {byte offset of its first pixel (any alignment; ascending, images do not overlap), H, W, first chunk over the
 * batch (an image takes ceil(H W / 1024) chunks; images in order), ops, f01, f23, 0}.  ops = steps (0 .. 4) | code of step k << 4 (k + 1), codes
 * 1 brightness, 2 contrast, 3 colour (torchvision's saturation), 4 hue, each at most once, in the order they are applied; f01 / f23 hold 32 bits
 * per step (step 0 in the low half of f01): the bits of the float32 factor (finite), or for hue the shift 0 .. 255 added to H mod 256.
 * 1 <= N <= 65535, 1 <= H, W <= 16384.  The records are taken twice: in host memory (hdesc), checked against `bytes` before anything is
 * launched, and in device memory (desc), which the kernels read.
 * dbn_color_jitter_u8 (a memset and a launch for the grey sums when a plan holds contrast, then one launch): sums uint64 [N] of workspace
 * (may be NULL when no plan holds contrast).  out == in works in place; bytes of `out` that belong to no image are not written.
 * dbn_color_jitter_host: TEST SUPPORT, not a product path (no Python function calls it, and the package refuses host tensors): the same
 * arithmetic (csrc/photometric.h compiled for the host) walked over host buffers without a launch, so that the tests that run without a
 * device hold what this library compiles, not only its numpy restatement, against Pillow.  It is declared here because every dbn_* symbol
 * the library defines is (tests/test_host_cpu.py), and the ctypes side is derived from this header alone. */
int dbn_color_jitter_u8(const unsigned char* in, unsigned char* out, long bytes, const long long* hdesc, const long long* desc, int N,
                        unsigned long long* sums, void* stream);
int dbn_color_jitter_host(const unsigned char* in, unsigned char* out, long bytes, const long long* hdesc, int N);

/* ---- Degradation augmentation (csrc/degrade.hip; db_text_minimal_amd/degrade.py): a Gaussian blur with a per-image radius, then additive
 * Gaussian noise on the blurred byte, in exact integers, on packed uint8 [H][W][3] RGB images (the definition: DESIGN.md section 40).
 * desc int64 [N][25] per image = {byte offset of its first pixel (any alignment; ascending, images do not overlap), H, W, first tile over the
 * batch, r (0 .. 32; 0: no blur), S8 | per_channel << 32 (S8 = round(256 scale), 0 .. 16384; 0: no noise), the 64-bit seed, 0, then q_0 ..
 * q_32 as 32-bit values, two to a field, the lower index in the low half}.  With r > 0 the weights q_0 .. q_r are below 65536, q_0 + 2 (q_1 +
 * ... + q_r) = 65536, and those behind q_r are 0.  tiles int32 [T][3] = {image, y0, x0}: 32 rows x 64 columns from (y0, x0) of an image with
 * r > 0 (cut at the image's edges), or {image, first pixel, 0}: a run of 3072 pixels in row-major order of an image with r = 0; per image in
 * row-major order, images in order, every pixel in exactly one tile (the entry point refuses any other list).  normal int16 [4096]:
 * round(4096 Phi^-1((k + 0.5) / 4096)).  1 <= N <= 65535, 1 <= H, W <= 16384.  Records and tiles are taken twice: in host memory (hdesc,
 * htiles), checked against `bytes` before anything is launched, and in device memory (desc, tiles), which the kernel reads.  One launch, LDS
 * sized by the largest r of the batch.  `out` must not overlap `in`; bytes of `out` that belong to no image are not written. */
int dbn_degrade_u8(const unsigned char* in, unsigned char* out, long bytes, const long long* hdesc, const long long* desc, int N, const int* htiles,
                   const int* tiles, long T, const short* normal, void* stream);

/* ---- Synthetic scene text (csrc/synth.hip; db_text_minimal_amd/synth.py): a background and over it glyph instances under any affine map,
 * anti-aliased by 16 samples per pixel, in exact integers, written as packed uint8 [H][W][3] RGB images (the definition: DESIGN.md section
 * 41; THIS PROJECT'S DEFINITION, PARITY UNPINNED against SynthText or any renderer).  One launch, one workgroup per tile of 32 x 32 pixels.
 * desc int64 [N][8] per image = {byte offset of its first pixel (any alignment; ascending, images do not overlap), H, W, first tile over the
 * batch, base colour r | g << 8 | b << 16, amplitudes A_0 | A_1 << 8 | A_2 << 16 (0 .. 64 each; octave o has cells of 64 >> 2 o pixels), the
 * 64-bit seed of the noise, 0}.  backgrounds: NULL (the procedural background of desc) or a packed batch of the same layout, read instead;
 * `out` must not overlap it.
 * recs int64 [R][9] per glyph instance = {image, glyph, a00, a01, a10, a11, tx, ty, colour r | g << 8 | b << 16}: font vertex v sits at (a00 vx +
 * a01 vy, a10 vx + a11 vy) + t on the lattice of 2^20 units per pixel (font y points up: an upright glyph has a11 < 0).  Sample (i, j), i, j =
 * 0 .. 3, of pixel (px, py) sits at (2^20 px + (2 i + 1) 2^17, 2^20 py + (2 j + 1) 2^17); it is inside when the winding sum of
 * dbn_draw_glyphs' rule about the transformed edges is not 0; cov = the samples inside; per channel cur = (cov fg + (16 - cov) cur + 8) >> 4,
 * instance after instance in ascending record order.  An instance is evaluated only if |a| < 2^19, |t| <= 2^35, its glyph has 1 .. 512 edges
 * and the transformed glyph box spans less than 2^30 per axis (then every cross product is below 2^62); any other is skipped.
 * edges int32 [E][4] = {ax, ay, bx, by} in font units, EVERY edge of the closed contours (one that is horizontal after the transform never
 * counts); glyphs int32 [G][6] = {first edge, edges, xmin, ymin, xmax, ymax}, the box holding every edge of the glyph, |.| <= 2^14.
 * bins int32 [B]: T rows {image, y0, x0, end} of the tiles, per image in row-major order, images in order, every tile once; then the lists:
 * tile k lists bins[end of tile k - 1 (4 T for k = 0) .. end of tile k), record indices of its image in strictly ascending order; the last
 * end is B.  A tile lists (at least) the evaluated instances whose box meets it.
 * Descriptors, records, bins and glyphs are taken twice: in host memory (hdesc, hrecs, hbins, hglyphs), checked before anything is
 * launched (descriptors against `bytes`, the tile list, glyph ranges against E, image and glyph indices and colours of the records, bins
 * in range, ascending and of their tile's image), and in device memory, which the kernel reads; an instance whose device record disagrees
 * with its tile's image, G or E is skipped.  1 <= N <= 65535, 1 <= H, W <= 16384; R may be 0 (hrecs, recs NULL): the background alone.
 * Every byte of every image is stored exactly once; bytes of `out` that belong to no image are not written.  No atomics, no float arithmetic. */
int dbn_synth_text_u8(const unsigned char* backgrounds, unsigned char* out, long bytes, const long long* hdesc, const long long* desc, int N,
                      const long long* hrecs, const long long* recs, long R, const int* hbins, const int* bins, long T, long B, const int* edges,
                      long E, const int* hglyphs, const int* glyphs, int G, void* stream);

#ifdef __cplusplus
}
#endif
#endif
