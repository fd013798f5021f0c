/*
 * sis_hip.h -- C ABI of libsis_hip.so: the MI355X (gfx950) kernels behind the
 * synthesis-in-style hot path (StyleGAN2 generator forward + segmentation training step).
 *
 * Drop-in boundary.  Every entry point takes plain device pointers, sizes and a HIP stream
 * (passed as void*, i.e. a hipStream_t; NULL = the legacy default stream).  No torch types.
 * Inputs are borrowed and must be contiguous; outputs are caller-allocated.  Nothing here
 * synchronises the host.  Return value: 0 on success, non-zero on error (message from
 * sis_last_error(), thread-local).  The reference interface each function replaces is cited
 * as file:line relative to /root/reference/stylegan_code_finder/.
 *
 * dtype codes: 0 = float32, 1 = float64, 2 = float16, 3 = bfloat16.
 */
#ifndef SIS_HIP_H
#define SIS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIS_F32 0
#define SIS_F64 1
#define SIS_F16 2
#define SIS_BF16 3

/* library version (major*1000 + minor) and last error text of the calling thread */
int sis_version(void);
const char* sis_last_error(void);
/* Name of the device kernel the calling thread's last sis_modconv2d / sis_modconv2d_up call dispatched to (the
 * dispatch depends on shape and alignment); bench.py uses it so that its per-kernel timings carry the names
 * rocprofv3 reports. */
const char* sis_last_kernel(void);

/* ------------------------------------------------------------------------------------------
 * K1  fused bias + activation.
 * Replaces the pybind entry `fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale)`
 *   networks/stylegan2/op/fused_bias_act.cpp:11-21, launcher fused_bias_act_kernel.cu:52-99,
 *   element formula fused_bias_act_kernel.cu:25-47.
 * out[i] = f(x[i] + bias[(i / step_b) % size_b]) * scale, mode = act*10+grad:
 *   10/11 linear; 30 leaky-relu(alpha); 31 leaky-relu gradient gated on ref[i] > 0; 12/32 zero.
 * bias == NULL (or size_b == 0) means "no bias", ref == NULL means "no ref" (the reference
 * passes empty tensors, fused_bias_act_kernel.cu:62-63).  step_b = product of dims[2:].
 */
int sis_fused_bias_act(void* out, const void* x, const void* bias, const void* ref, int dtype,
                       int64_t numel, int64_t step_b, int64_t size_b, int act, int grad,
                       float alpha, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * K2  upfirdn2d: zero-insert upsample, pad/crop, 2-D FIR with the flipped taps, decimate.
 * Replaces the pybind entry `upfirdn2d_op.upfirdn2d(input, kernel, up_x, up_y, down_x, down_y,
 *   pad_x0, pad_x1, pad_y0, pad_y1)`  networks/stylegan2/op/upfirdn2d.cpp:12-23,
 *   launcher/dispatch upfirdn2d_kernel.cu:140-272, kernel :52-137.
 * in  [major, in_h, in_w, minor], taps [kh, kw] (same dtype as in), out [major, out_h, out_w, minor]
 * with out = (in*up + pad0 + pad1 - k + down) / down  (upfirdn2d_kernel.cu:167-168).
 * Unlike the reference (which silently returns uninitialised memory for an up/down/tap
 * combination outside its 6 modes, upfirdn2d_kernel.cu:172-175) every combination is computed.
 */
int sis_upfirdn2d_out_size(int in_size, int up, int down, int pad0, int pad1, int k);
int sis_upfirdn2d(void* out, const void* in, const void* taps, int dtype, int major, int in_h,
                  int in_w, int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                  int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* ------------------------------------------------------------------------------------------
 * Generator building blocks (float32).  Together they replace the composite PyTorch code of
 * networks/stylegan2/model.py cited per function.
 */

/* PixelNorm, model.py:19-20: out[b,:] = x[b,:] * rsqrt(mean(x[b,:]^2) + 1e-8). */
int sis_pixel_norm(float* out, const float* x, int batch, int dim, void* stream);

/* Output features per workgroup of the three head GEMMs below (EqualLinear, batched modulation, batched demodulation:
 * 32 batch rows x this many outputs on the fp32 matrix cores); the batched launches' tables count blocks in this unit. */
int sis_head_gemm_tile(void);

/* EqualLinear, model.py:152-162: out[b,o] = sum_i x[b,i] * w[o,i] * scale + bias[o]*lr_mul, then
 * (activation != 0) leaky-relu(0.2) * sqrt(2) as fused_leaky_relu does (fused_act.py:85-86).
 * x rows are x_row_stride floats apart (lets a [B, n_latent, D] latent be indexed in place).
 * sis_last_kernel() names the kernel in_dim picked: equal_linear_full_kernel<8> (512), equal_linear_full_kernel<4> (256),
 * equal_linear_kernel (up to 1024), head_gemm_kernel<0> (wider). */
int sis_equal_linear(float* out, const float* x, int64_t x_row_stride, const float* w,
                     const float* bias, int batch, int in_dim, int out_dim, float scale,
                     float lr_mul, int activation, void* stream);

/* Every modulation EqualLinear of one Generator.forward in ONE launch (20 layers at 256^2; model.py:240 per
 * layer): out_base[row.out_offset + b*out_dim + o] = scale * <latent[b, row.latent_index, :], w[o, :]> + bias[o].
 * latent is [B, n_latent, dim]; table is a device array of n_layers rows of 8 int64:
 * {weight ptr, bias ptr, out offset (floats), latent index, out_dim, first_block, 0, 0}, first_block = running
 * sum of ceil(out_dim / sis_head_gemm_tile()); total_blocks = the final sum. */
int sis_modulation_batch(float* out_base, const float* latent, const int64_t* table, int n_layers,
                         int total_blocks, int batch, int n_latent, int dim, float scale, void* stream);

/* Every demodulation-coefficient row of one forward in ONE launch (see sis_modconv_demod); table rows of 8
 * int64: {wsq ptr, float bits of the conv scale, s offset, dscale offset, cout, first_block, cin, demodulate},
 * first_block = running sum of ceil(cout / sis_head_gemm_tile()). */
int sis_demod_batch(float* dscale_base, const float* s_base, const int64_t* table, int n_layers,
                    int total_blocks, int batch, void* stream);

/* Truncation trick, model.py:502-510: out = mean + psi * (w - mean); mean is [dim]. */
int sis_truncate(float* out, const float* w, const float* mean, float psi, int batch, int dim,
                 void* stream);

/* Weight prepack for the modulated convolution (once per checkpoint):
 *   wpk[ci][tap][co] = w[co][ci][tap]            (tap = kh*ks + kw)
 *   wsq[co][ci]      = sum_tap w[co][ci][tap]^2  (feeds the demodulation, model.py:243-245)
 * w is the ModulatedConv2d.weight parameter [1, Cout, Cin, ks, ks] (model.py:223-225). */
int sis_modconv_prepack(float* wpk, float* wsq, const float* w, int cout, int cin, int ksize,
                        void* stream);

/* dscale[b,co] = scale * rsqrt(scale^2 * sum_ci s[b,ci]^2 * wsq[co,ci] + 1e-8) when demodulate,
 * else scale  (model.py:241-245 with the style factored out of the weights; scale = 1/sqrt(Cin*ks^2),
 * model.py:219-220). */
int sis_modconv_demod(float* dscale, const float* s, const float* wsq, int batch, int cin,
                      int cout, float scale, int demodulate, void* stream);

/* Modulated convolution, stride 1, "same" padding, ks in {1,3}: model.py:272-276 (+ :287-292,
 * fused_act.py:85-86 when fuse_act != 0):
 *   y[b,co,h,w] = dscale[b,co] * sum_{ci,kh,kw} wpk[ci][kh*ks+kw][co] * s[b,ci] * x[b,ci,h+kh-p,w+kw-p]
 *   fuse_act:  y = lrelu_{0.2}(y + noise_weight[0]*noise[nb,0,h,w] + bias[co]) * sqrt(2)
 * noise is [1,1,H,W] (noise_batch_stride 0) or [B,1,H,W] (stride H*W) or NULL; noise_weight is a
 * DEVICE pointer to one float (the NoiseInjection.weight parameter).  MFMA fp32 (v_mfma_f32_32x32x2_f32).
 * workspace (optional, may be NULL): device scratch for split-K partial sums of launch-starved small
 * layers; without it those layers run unsplit.  Contents need not be preserved between calls. */
int sis_modconv2d(float* out, const float* x, const float* wpk, const float* s,
                  const float* dscale, const float* noise, int64_t noise_batch_stride,
                  const float* noise_weight, const float* bias, int batch, int cin, int cout,
                  int h, int w, int ksize, int fuse_act, const float* wino_u, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* Winograd F(2x2,3x3) weight transform for sis_modconv2d's optional `wino_u` argument (ksize 3, even H and W,
 * Cin % 8 == 0): cin * 16 * cout floats holding (G w[co,ci] G^T)[xi], xi = 0..15, in the kernels' private operand order
 * [ci][q][ih][co][il][jj] with xi = 4 (2 ih + il) + 2 q + jj (opaque to the caller: only these kernels read it).  With
 * wino_u the stride-1 3x3 layers run 16 multiplies per 2x2 output tile instead of 36 (2.25x fewer MFMA FLOPs); NULL
 * selects the direct kernel. */
int sis_modconv_prepack_wino(float* u, const float* w, int cout, int cin, void* stream);

/* The same layers in Winograd F(2x4,3x3) form (csrc/modconv_wino24.h): 24 multiplies per 2 x 4 output tile, 24/72 of the
 * direct form.  sis_modconv_prepack_wino24 writes cin * 24 * cout floats, (G2 w[co,ci] G4^T)[xi] with F(2,3) on the row axis and
 * F(4,3) (points 0, +-1, +-2, inf) on the column axis, in the kernel's private order [ci][q][g][co][4] (plane 3 i + jj = 4 g + k
 * of column half q, xi = 6 i + 3 q + jj).  sis_modconv_wino24_eligible depends on (cin, cout, h, w) only, never on the batch:
 * cin % 8 == 0, cout % 64 == 0, h % 2 == 0, w % 4 == 0, w > 16 and a map of at least 512 pixels.  sis_modconv2d_wino24 is
 * sis_modconv2d for such a layer (same operands and fused tail; u24 in place of wpk / wino_u; no workspace: never split-K);
 * tiles_per_wg = 0 lets the launcher choose how many 512-pixel tiles a workgroup walks (> 0: the tests' override, must divide
 * the tile count; the results do not depend on it). */
int sis_modconv_prepack_wino24(float* u, const float* w, int cout, int cin, void* stream);
int sis_modconv_wino24_eligible(int cin, int cout, int h, int w);
int sis_modconv2d_wino24(float* out, const float* x, const float* u24, const float* s, const float* dscale,
                         const float* noise, int64_t noise_batch_stride, const float* noise_weight, const float* bias,
                         int batch, int cin, int cout, int h, int w, int fuse_act, int tiles_per_wg, void* stream);

/* sis_modconv2d_wino24 that also leaves the following ToRGB's channel sum, in blocks of 64 output channels:
 * rgb_part[cb][b][c][y][x] = sum_{co in [64 cb, 64 cb + 64)} rgb_scale * rgb_w[c][co] * rgb_s[b][co] * out[b][co][y][x], c = 0..2,
 * a [cout / 64][B][3][H][W] buffer (16-byte aligned) that is written in full.  out is what sis_modconv2d_wino24 writes, bit for
 * bit; a sample's sums do not depend on the batch or on tiles_per_wg.  sis_rgb_finish completes the ToRGB layer:
 * out[b][c] = sum_cb part[cb][b][c] (cb ascending) + bias[c] + upsample(skip)[b][c], skip / taps / pads as in sis_to_rgb. */
int sis_modconv2d_wino24_rgb(float* out, float* rgb_part, const float* x, const float* u24, const float* s, const float* dscale,
                             const float* noise, int64_t noise_batch_stride, const float* noise_weight, const float* bias,
                             const float* rgb_w, const float* rgb_s, float rgb_scale, int batch, int cin, int cout, int h, int w,
                             int fuse_act, int tiles_per_wg, void* stream);

/* The same layers in Winograd F(4x4,3x3) form (csrc/modconv_wino44.h): 36 multiplies per 4 x 4 output tile, 36/144 of the direct
 * form.  sis_modconv_prepack_wino44 writes cin * 36 * cout floats, (G4 w[co,ci] G4^T)[i][j] with F(4,3) (points 0, +-1, +-2, inf)
 * on both axes, in the kernel's private order [ci][9 rows][co][4] (head of csrc/modconv_wino44.h).  sis_modconv_wino44_eligible
 * is sis_modconv_wino24_eligible's rule with h % 4 == 0 in place of h % 2 == 0.  sis_modconv2d_wino44 and
 * sis_modconv2d_wino44_rgb take the operands of their wino24 twins with u44 in place of u24 and write the same things: rgb_part
 * has the layout that sis_rgb_finish reads; the stored activation of the _rgb entry is that of the plain entry bit for bit, and a
 * sample's results do not depend on the batch or on tiles_per_wg. */
int sis_modconv_prepack_wino44(float* u, const float* w, int cout, int cin, void* stream);
int sis_modconv_wino44_eligible(int cin, int cout, int h, int w);
int sis_modconv2d_wino44(float* out, const float* x, const float* u44, const float* s, const float* dscale,
                         const float* noise, int64_t noise_batch_stride, const float* noise_weight, const float* bias,
                         int batch, int cin, int cout, int h, int w, int fuse_act, int tiles_per_wg, void* stream);
int sis_modconv2d_wino44_rgb(float* out, float* rgb_part, const float* x, const float* u44, const float* s, const float* dscale,
                             const float* noise, int64_t noise_batch_stride, const float* noise_weight, const float* bias,
                             const float* rgb_w, const float* rgb_s, float rgb_scale, int batch, int cin, int cout, int h, int w,
                             int fuse_act, int tiles_per_wg, void* stream);
int sis_rgb_finish(float* out, const float* part, const float* bias, const float* skip, const float* taps, int batch, int blocks,
                   int cout, int h, int width, int kh, int kw, int pad0, int pad1, void* stream);

/* The same stride-1 3x3 layers with bf16 operands on the bf16 matrix cores (csrc/modconv_bf16.h; opt-in, the default route is
 * fp32): model.py:272-276 (+ :287-292, fused_act.py:85-86 when fuse_act != 0) with both operands rounded,
 *   y[b,co,h,w] = dscale[b,co] * sum_{ci,kh,kw} bf16(w[co,ci,kh,kw]) * bf16(fl32(s[b,ci] * x[b,ci,h+kh-1,w+kw-1]))
 *   fuse_act:  y = lrelu_{0.2}(y + noise_weight[0]*noise[nb,0,h,w] + bias[co]) * sqrt(2)      (as sis_modconv2d, in fp32)
 * Both conversions round to nearest even; the style product is formed in fp32 and rounded once; the weight is the raw
 * parameter rounded once (the conv scale stays in dscale); accumulation, dscale, noise, bias and the tail are fp32; x and out
 * are fp32.  No atomics, no split-K: a sample's result depends on neither the batch nor the launch plan.
 * sis_modconv_bf16_eligible (model.py:272-276, :287-292) depends on (cin, cout, h, w) only, never on the batch: cin % 8 == 0
 * (a last half-empty chunk of 16 channels is padded with zeros), cin <= 1024, cout % 64 == 0, w % 4 == 0 (16-byte row loads),
 * w >= 32 and h * w >= 256 (one whole tile of 256 pixels: 4 x 64, or 8 x 32 on maps up to 32 wide; h itself is free) and fewer than 2^31
 * elements per sample on either side.
 * sis_modconv_bf16_packed_elems (model.py:272-276, :287-292): bf16 elements of the packed weight image of a cin -> cout layer
 * (-1: no such layer); sis_modconv_prepack_bf16 (model.py:272-276, :287-292) writes it from w [cout][cin][3][3], once per
 * checkpoint: [cout tile of 128 (cout >= 128) or 64][chunk of 16 channels][tap][row][swizzled 8-channel unit][8], private to
 * the kernel.  sis_modconv2d_bf16 (model.py:272-276, :287-292): the operands of sis_modconv2d_wino24 with that image in place
 * of u24; x and packed 16-byte aligned. */
int sis_modconv_bf16_eligible(int cin, int cout, int h, int w);
int64_t sis_modconv_bf16_packed_elems(int cin, int cout);
int sis_modconv_prepack_bf16(void* packed, const float* w, int cout, int cin, void* stream);
int sis_modconv2d_bf16(float* out, const float* x, const void* packed, const float* s, const float* dscale,
                       const float* noise, int64_t noise_batch_stride, const float* noise_weight, const float* bias,
                       int batch, int cin, int cout, int h, int w, int fuse_act, void* stream);

/* Modulated transposed convolution, stride 2, no padding, ks = 3: model.py:251-261 up to (not
 * including) the Blur: t[b,co,p,q] = dscale[b,co] * sum_{ci, 2h+kh=p, 2w+kw=q} wpk[ci][kh*3+kw][co]
 * * s[b,ci] * x[b,ci,h,w];  t is [B, Cout, 2H+1, t_row_stride] with the first 2W+1 floats of every row
 * meaningful (t_row_stride 0 = dense 2W+1; an even stride lets the kernel store output phase pairs as 8 bytes). */
int sis_modconv2d_up(float* t, const float* x, const float* wpk, const float* s,
                     const float* dscale, int batch, int cin, int cout, int h, int w,
                     int t_row_stride, void* workspace, int64_t workspace_bytes, void* stream);

/* The same transposed convolution in its fast-FIR form (csrc/modconv_upfir.hip): 25 instead of 36 multiplies per 2 x 2 input
 * positions (F(2,2) of the 2-tap even phases per axis), on v_mfma_f32_16x16x4_f32.  `u` = the 16 transformed weight planes,
 * [cin][8 plane pairs][cout][2], written by sis_modconv_up_fir_prepack from the layer's weight [cout][cin][3][3] (once per
 * checkpoint).
 * t: [batch][cout][2h+1][t_row_stride] with t_row_stride % 4 == 0 and >= 2w + 4 (columns beyond 2w are padding and receive
 * unspecified finite values).  sis_modconv_up_fir_supported: h, w >= 32, h even, w % 4 == 0, cin % 8 == 0, cout % 64 == 0,
 * operands below 2 GiB. */
int sis_modconv_up_fir_supported(int batch, int cin, int cout, int h, int w, int t_row_stride);
int sis_modconv_up_fir_prepack(float* u, const float* w, int cout, int cin, void* stream);
int sis_modconv2d_up_fir(float* t, const float* x, const float* u, const float* s, const float* dscale, int batch, int cin, int cout,
                         int h, int w, int t_row_stride, void* stream);

/* Blur (upfirdn2d up=1 down=1, model.py:89-92 / :262) fused with NoiseInjection + FusedLeakyReLU
 * (model.py:338-340): in [B,C,IH,IW] -> out [B,C,OH,OW], OH = IH + pad0 + pad1 - kh + 1.
 * fuse_act == 0 gives the plain blur. taps [kh,kw] float32 device pointer.  in_row_stride (floats, 0 = in_w)
 * lets the input rows be padded; sis_modconv2d_up writes rows of 2W+4 floats so that the 4x4 / pad-1 case
 * streams aligned 16-byte rows. */
int sis_blur_noise_act(float* out, const float* in, const float* taps, const float* noise,
                       int64_t noise_batch_stride, const float* noise_weight, const float* bias,
                       int batch, int channels, int in_h, int in_w, int in_row_stride, int kh, int kw,
                       int pad0, int pad1, int fuse_act, void* stream);

/* ToRGB, model.py:355-364: out[b,c,y,x] = scale * sum_ci w[c,ci]*s[b,ci]*x[b,ci,y,x] + bias[c]
 * + upfirdn2d(skip, taps, up=2, pad=(pad0,pad1))[b,c,y,x]   (skip == NULL: first ToRGB).
 * w is the [1,3,Cin,1,1] parameter, skip is [B,3,H/2,W/2], taps [kh,kw]. out channels fixed to
 * `cout` <= 4.  sis_last_kernel() names the kernel that ran: to_rgb_kernel<4> (h * w a multiple of 4, at least 256,
 * x and out 16-byte aligned), else to_rgb_kernel<1>. */
int sis_to_rgb(float* out, const float* x, const float* w, const float* s, const float* bias,
               const float* skip, const float* taps, int batch, int cin, int cout, int h, int width,
               int kh, int kw, int pad0, int pad1, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Segmentation training step (float32): the non-convolution ends of EMANetUpdater.update_core /
 * TransUNetUpdater.update_core (updater/segmentation_updater.py:47-73, :83-106).
 */

/* EMANet loss tail, networks/ema_net/network.py:305-311 + CrossEntropyLoss2d :319-327:
 *   pred = bilinear(logits [B,C,h,w] -> [B,C,out_h,out_w], align_corners=True)
 *   loss[b] = mean_{y,x} NLL(log_softmax(pred)[b,:,y,x], labels[b,y,x]), ignore_index pixels count as 0.
 * workspace: sis_upsample_ce_workspace(batch, out_h, out_w) floats.  labels are int64 [B,out_h,out_w]. */
int sis_upsample_ce_workspace(int batch, int out_h, int out_w);
int sis_upsample_ce_fwd(float* loss, float* workspace, const float* logits, const int64_t* labels,
                        int batch, int classes, int h, int w, int out_h, int out_w,
                        int64_t ignore_index, void* stream);
/* grad_logits[b,c,i,j] = d(sum_b grad_loss[b] * loss[b]) / d logits[b,c,i,j] (deterministic gather). */
int sis_upsample_ce_bwd(float* grad_logits, const float* grad_loss, const float* logits,
                        const int64_t* labels, int batch, int classes, int h, int w, int out_h,
                        int out_w, int64_t ignore_index, void* stream);

/* torch.optim.SGD(momentum, dampening 0, no nesterov) for every tensor of an optimizer in one launch
 * (training_builder/ema_net_train_builder.py:27-48).  `table` is a device array of n_chunks rows of FIVE
 * int64: {param ptr, grad ptr, momentum-buffer ptr, count | (group << 48), bf16 shadow ptr or 0}, count <=
 * sis_sgd_chunk_elems().
 *   d = grad + wd[group]*p;  buf = first_step ? d : momentum*buf + d;  p -= lr[group]*buf;  shadow = bf16(p) if given
 * (the shadow is the bfloat16 copy of the fp32 master weight that bf16 layers read: no per-forward cast kernels)
 * lr / weight_decay are HOST arrays of n_groups (<= 4) floats. */
int sis_sgd_chunk_elems(void);
int sis_sgd_momentum(const int64_t* table, int n_chunks, const float* lr, const float* weight_decay,
                     int n_groups, float momentum, int first_step, void* stream);

/* The same step (not the first one: momentum buffers exist) with the hyper-parameters in DEVICE memory,
 * hyper = {lr[0..3], weight_decay[0..3], momentum}: the launch carries only pointers, so it can be captured in a
 * hipGraph and still follow a per-iteration LR schedule (the host rewrites `hyper` between replays). */
int sis_sgd_momentum_dev(const int64_t* table, int n_chunks, const float* hyper, void* stream);

/* emau.mu[i] = mu[i]*momentum + mean_b(mu_batch[b,i])*one_minus_momentum
 * (updater/segmentation_updater.py:56-66; in-place on the buffer, outside autograd). */
int sis_ema_update(float* mu, const float* mu_batch, float momentum, float one_minus_momentum,
                   int batch, int numel, void* stream);

/* A 3x3 convolution whose dilation (= padding) is half the image side (EMANet's dilation-16 bottleneck on 32 x 32 maps,
 * networks/ema_net/network.py:82-86) is one dense [4 Cin] -> [4 Cout] map per position of the half-size grid:
 * taps [4 cout][4 cin], rows (u, v, co), columns (u', v', ci), = weight[co][ci][u' - u + 1][v' - v + 1] (csrc/dilation_taps.hip);
 * the product itself runs on sis_conv1x1_f32*.  _bwd: dweight [cout][cin][3][3] from dtaps, fixed summation order. */
int sis_half_dilation_taps(float* taps, const float* weight, int cout, int cin, void* stream);
int sis_half_dilation_taps_bwd(float* dweight, const float* dtaps, int cout, int cin, void* stream);

/* EMANet's Expectation-Maximisation Attention Unit between its two 1x1 convolutions (networks/ema_net/network.py:219-249,
 * the no_grad block and the reconstruction):  mu <- mu0 (shared [channels][bases]) for every sample; `stages` rounds of
 * z = softmax_k(x^T mu), z_ = z / (1e-6 + sum_n z), mu = l2norm_c(x z_) (eps 1e-6);  x_out = relu(mu z^T), mu_out = mu.
 * x, x_out: [batch][channels][pixels] float32; mu_out: [batch][channels][bases].  fp32 MFMA products, 2 * stages + 1 launches,
 * no atomics (csrc/emau.hip).  bases must be 64, channels % 64 == 0, pixels % 128 == 0 (sis_emau_supported);
 * workspace: sis_emau_workspace_floats(...) floats (z, un-normalised bases, partial sums). */
int sis_emau_supported(int batch, int channels, int pixels, int bases);
int64_t sis_emau_workspace_floats(int batch, int channels, int pixels, int bases);
int sis_emau_forward(float* x_out, float* mu_out, const float* x, const float* mu0, float* workspace, int batch, int channels,
                     int pixels, int bases, int stages, void* stream);

/* Batch normalisation (training: batch statistics; F.batch_norm semantics incl. the unbiased running_var update)
 * fused with an optional residual add and ReLU, fp32 NCHW with H*W % 4 == 0
 * (networks/ema_net/network.py:37-56 bottleneck tail, :169-184 ConvBNReLU; bn_lib/nn/modules/batchnorm.py:51-56).
 * workspace: sis_bn_workspace_floats(batch, channels, hw) floats.  running_* may be NULL (no update).
 *   sis_bn_stats    mean[c], invstd[c] = 1/sqrt(var_biased + eps)   (+ running stats with `momentum`)
 *   sis_bn_act_fwd  y = [relu]( gamma*(x-mean)*invstd + beta [+ residual] )     (eval: pass running statistics)
 *   sis_bn_act_bwd  dy' = dy*[y>0] (when relu); dbeta = sum dy'; dgamma = sum dy'*xhat;
 *                   dx = gamma*invstd*(dy' - mean(dy') - xhat*mean(dy'*xhat)); dresidual = dy' (when not NULL).
 * relu_mask (may be NULL): sis_bn_mask_words(batch, channels, hw) 64-bit words, one sign bit per element of y, written by
 * sis_bn_act_fwd (relu != 0) and read by sis_bn_act_bwd INSTEAD of y (y may then be NULL): 1/8 byte per element for the ReLU
 * gate in both backward passes instead of 4. */
int64_t sis_bn_workspace_floats(int batch, int channels, int hw);
int64_t sis_bn_mask_words(int batch, int channels, int hw);
int sis_bn_stats(float* mean, float* invstd, float* running_mean, float* running_var, const float* x,
                 float* workspace, int batch, int channels, int hw, float eps, float momentum, void* stream);
int sis_bn_act_fwd(float* y, const float* x, const float* residual, const float* mean, const float* invstd,
                   const float* gamma, const float* beta, int batch, int channels, int hw, int relu, void* relu_mask,
                   void* stream);
int sis_bn_act_bwd(float* dx, float* dresidual, float* dgamma, float* dbeta, const float* dy, const float* y,
                   const float* x, const float* mean, const float* invstd, const float* gamma, float* workspace,
                   int batch, int channels, int hw, int relu, const void* relu_mask, void* stream);
/* Statistics + apply of the training-mode batch norm in ONE launch when a channel's batch * hw elements fit one workgroup's
 * registers (sis_bn_fused_supported: batch * hw <= 16 384 and hw % 256 == 0 -- every 32 x 32 layer of EMANet at batch 16 -- or, with
 * one workgroup of 1 024 threads per channel, batch * hw <= 65 536: the 64 x 64 layers; statistics then within 1e-6, not bitwise):
 * x is read once instead of twice; mean / invstd / running statistics as sis_bn_stats, y (and relu_mask) as sis_bn_act_fwd,
 * bitwise the same values.  sis_bn_act_bwd takes its single-pass form (dy and x read once; results to an ulp of the
 * three-launch form) under the same condition. */
int sis_bn_fused_supported(int batch, int channels, int hw);
int sis_bn_fused_fwd(float* y, float* mean, float* invstd, float* running_mean, float* running_var, const float* x,
                     const float* residual, const float* gamma, const float* beta, int batch, int channels, int hw, float eps,
                     float momentum, int relu, void* relu_mask, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dataset-loop neighbours of Generator.forward (SURVEY.md §8f "next" rows 1 and 2).
 */

/* Nearest k-means centre per pixel: labels[b,p] = argmin_k sum_c (x[b,c,p] - centres[k,c])^2, ties to the lowest
 * k (segmentation/gan_local_edit/factor_catalog.py:47-62 + :69-75: FactorCatalog.predict on [B,C,H,W]).
 * x [B,C,HW] float32, centres [K,C] float32 (K <= 64, 8 <= C < 8192), labels int64 [B,HW].
 * Bit-exact contract: the fp32 adds are associated exactly as torch's CPU ``.sum(dim=-1)`` associates them (the
 * reference's evaluation); the order is written out in csrc/dataset_ops.hip and oracle/kmeans_ref.py. */
int sis_kmeans_assign(int64_t* labels, const float* x, const float* centres, int batch, int channels,
                      int hw, int n_centres, void* stream);
/* The same with a workspace of sis_kmeans_workspace_ints(batch, hw) ints: the pixels the fast first pass leaves open are
 * listed there and the exact-order pass revisits exactly those, one per lane (without it: every 512-pixel workgroup that holds
 * one).  Same labels either way. */
int64_t sis_kmeans_workspace_ints(int batch, int hw);
int sis_kmeans_assign_ws(int64_t* labels, const float* x, const float* centres, int batch, int channels, int hw, int n_centres,
                         int* workspace, int64_t workspace_ints, void* stream);

/* float32 NCHW image in [-1,1] -> uint8 NHWC: clamp, (x+1)/2*255, truncating cast (the third-party make_image
 * called at create_dataset_for_segmentation.py:135; its rounding is not pinned by the reference). */
int sis_make_image_u8(uint8_t* out, const float* x, int batch, int channels, int hw, void* stream);

/* ------------------------------------------------------------------------------------------
 * Plain 3x3 convolution (stride 1, padding 1, no bias) of the segmentation networks on the Winograd F(2x2,3x3)
 * MFMA kernel -- replaces F.conv2d / cuDNN for networks/ema_net/network.py's 3x3 layers (ConvBNReLU :169-184, the
 * deep stem :71-79, Bottleneck.conv2 :27-28 where stride = dilation = 1), forward and data gradient.
 * sis_conv3x3_prepack: w [Cout_w][Cin_w][3][3] -> u, the transformed weights the kernel streams.  adjoint = 0: the
 *   forward convolution (cout = Cout_w, cin = Cin_w).  adjoint = 1: the convolution that maps dL/dy to dL/dx
 *   (cout = Cin_w, cin = Cout_w, taps rotated by 180 degrees).  u holds cin * 16 * cout floats.
 * sis_conv3x3: out [B,cout,H,W] = conv(x [B,cin,H,W], u).  Needs W % 4 == 0, H % 2 == 0, cin % 8 == 0,
 *   cout % 4 == 0; workspace as for sis_modconv2d (split-K scratch, may be NULL). */
int sis_conv3x3_eligible(int batch, int cin, int cout, int h, int w); /* 1 if sis_conv3x3 takes this shape */
/* Weight gradient of the same convolution in the Winograd domain (csrc/conv_wgrad_wino.hip):
 *   dw [Cout][Cin][3][3] = d/dw of <gy, conv(x, w)>,  x [B,Cin,H,W], gy [B,Cout,H,W].
 * Needs even H and W, (B*H*W/4) % 8 == 0, Cin % 64 == 0, Cout % 64 == 0, tensors below 2^29 elements (32-bit byte offsets of
 * the masked buffer loads), fewer than 2^24 2x2 tiles and a workspace of >= 64 * Cin * Cout bytes (split-K slabs, added in
 * slice order: deterministic).  sis_conv3x3_wgrad_eligible returns 1 when the call would be taken. */
int sis_conv3x3_wgrad_eligible(int batch, int cin, int cout, int h, int w, int64_t workspace_bytes);
int sis_conv3x3_wgrad(float* dw, const float* x, const float* gy, int batch, int cin, int cout, int h, int w,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* n_jobs layers of ONE shape (EMANet's repeated bottleneck units) through one tile launch + one finish launch: `dw`, `x`, `gy` are
 * HOST arrays of n_jobs device pointers; the K slices are planned for the layers' joint tile count. */
int sis_conv3x3_wgrad_multi(float* const* dw, const float* const* x, const float* const* gy, int n_jobs, int batch, int cin, int cout,
                            int h, int w, void* workspace, int64_t workspace_bytes, void* stream);
int sis_conv3x3_prepack(float* u, const float* w, int cout, int cin, int adjoint, void* stream);
/* forward and adjoint images of w [cout][cin][3][3] from one launch (training: the backward of the same step needs the adjoint):
 * u [cin][16][cout], u_adjoint [cout][16][cin]. */
int sis_conv3x3_prepack_both(float* u, float* u_adjoint, const float* w, int cout, int cin, void* stream);
/* Forward and adjoint images of SEVERAL layers from one launch.  `table`: device array of n_layers rows of 6 int64 --
 * (w pointer [cout][cin][3][3] float32, u pointer, u_adjoint pointer, cout, cin, first block of the layer) with
 * blocks per layer = ceil(cout * cin / 256); total_blocks = their sum. */
int sis_conv3x3_prepack_multi(const void* table, int n_layers, int total_blocks, void* stream);
int sis_conv3x3(float* out, const float* x, const float* u, int batch, int cin, int cout, int h, int w,
                void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weight standardisation of StdConv2d (networks/trans_u_net/vit_seg_modeling_resnet_skip.py:20-27), one launch per
 * direction.  w [rows][n] float32 (rows = Cout, n = Cin*kh*kw).
 * fwd: w_hat (dtype out_dtype = SIS_F32 / SIS_F16 / SIS_BF16) = (w - mean_row) / sqrt(var_row + eps), biased variance;
 *      invstd [rows] = 1 / sqrt(var_row + eps).
 * bwd: dw [rows][n] float32 = invstd * (g - mean(g) - w_hat * mean(g * w_hat)), g = dL/dw_hat in grad_dtype. */
int sis_weight_std_fwd(void* w_hat, float* invstd, const float* w, int out_dtype, int rows, int n, float eps,
                       void* stream);
int sis_weight_std_bwd(float* dw, const void* grad_w_hat, const float* w, const float* invstd, int grad_dtype,
                       int rows, int n, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * nn.GroupNorm (+ optional ReLU) of TransUNet's ResNetV2 trunk (vit_seg_modeling_resnet_skip.py:40-75,114-126),
 * x [B][C][hw] in x_dtype (SIS_F32 / SIS_F16 / SIS_BF16), fp32 arithmetic, affine gamma / beta [C] float32.
 * fwd: y (y_dtype = x_dtype or SIS_F32) = relu?((x - mean_g) * rstd_g * gamma_c + beta_c); mean / rstd [B*groups] kept.
 * residual (float32, may be NULL; needs y_dtype = SIS_F32): y = relu?(norm(x) + residual), the bottleneck's shortcut sum.
 * bwd: dx (x_dtype), dgamma / dbeta [C]; grad_y in g_dtype (= x_dtype or SIS_F32); the ReLU mask is recomputed from x, or
 *      taken from y_mask (the saved float32 output) when a residual was added; dresidual (float32, may be NULL) = masked grad;
 *      workspace (both directions): sis_group_norm_workspace_floats(B, C, hw) floats.
 *      y_lp (may be NULL; needs a float32 y of a 16-bit x): the same output also rounded to x's dtype in the same pass --
 *      the fp32 residual stream and the 16-bit tensor the next convolution reads; grad_y_lp (may be NULL): the gradient
 *      that came back through that copy, added to grad_y on load.
 *      counters (may be NULL): B*groups ints, ZERO on entry and left zero, private to the stream -- the per-group merge
 *      of the plane statistics then runs inside the statistics launch (the workgroup that completes a group does it, in
 *      channel order) and d(gamma) / d(beta) inside the apply launch: 2 launches per direction instead of 3 / 4; same
 *      values either way.
 *      relu_bits (may be NULL; fwd: with relu; sis_group_norm_gate_bytes bytes, 8-byte aligned): the forward leaves one bit per
 *      element ([y > 0], bit i of a flat bit array) and the backward gates on it instead of y_mask -- the residual form's
 *      backward then reads 1/8 byte instead of 4 per element and pass for the gate. */
int64_t sis_group_norm_workspace_floats(int batch, int channels, int hw);
int sis_group_norm_fwd(void* y, void* y_lp, float* mean, float* rstd, float* workspace, const void* x, const float* residual,
                       const float* gamma, const float* beta, int x_dtype, int y_dtype, int batch, int channels, int hw,
                       int groups, float eps, int relu, int* counters, void* relu_bits, void* stream);
int sis_group_norm_bwd(void* dx, float* dresidual, float* dgamma, float* dbeta, float* workspace, const void* grad_y,
                       const void* grad_y_lp, const void* x, const float* y_mask, const float* mean, const float* rstd, const float* gamma,
                       const float* beta, int x_dtype, int g_dtype, int batch, int channels, int hw, int groups, int relu,
                       int* counters, const void* relu_bits, void* stream);
int64_t sis_group_norm_gate_bytes(int batch, int channels, int hw);
/* nn.BatchNorm2d in training mode (+ optional ReLU) with 16-bit or fp32 tensors -- the TransUNet decoder's Conv2dReLU
 * blocks (networks/trans_u_net/vit_seg_modeling.py:265-287).  Arguments as for group norm; statistics per channel over
 * (B, hw); mean / rstd [C]; running_mean / running_var (float32 [C], may both be NULL) are updated with `momentum`
 * (unbiased variance).  Workspace: sis_group_norm_workspace_floats(B, C, hw) floats.  `counters`: NULL, or C ints that are
 * zero before the call and zero again after it (private to the stream, as for group norm): the per-channel merge then
 * happens inside the statistics launch, by the workgroup that completes the channel, instead of in a launch of its own. */
int sis_batch_norm_fwd(void* y, float* mean, float* rstd, float* running_mean, float* running_var, float* workspace,
                       const void* x, const float* gamma, const float* beta, int x_dtype, int y_dtype, int batch,
                       int channels, int hw, float eps, float momentum, int relu, int* counters, void* stream);
int sis_batch_norm_bwd(void* dx, float* dgamma, float* dbeta, float* workspace, const void* grad_y, const void* x,
                       const float* mean, const float* rstd, const float* gamma, const float* beta, int x_dtype,
                       int g_dtype, int batch, int channels, int hw, int relu, int* counters, void* stream);

/* ------------------------------------------------------------------------------------------
 * Column sums out[c] = sum_r x[r][c] of a [rows][n] matrix (n % 4 == 0; x SIS_F32 / SIS_F16 / SIS_BF16, out float32): the
 * bias gradient of the encoder's Linear layers (networks/trans_u_net/vit_seg_modeling.py:53-110, what autograd computes as
 * grad_output.sum(0)); deterministic two-stage reduction.  workspace: sis_column_sum_workspace_floats(n) floats. */
int64_t sis_column_sum_workspace_floats(int n);
int sis_column_sum(float* out, float* workspace, const void* x, int x_dtype, int rows, int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * nn.LayerNorm over the last dimension (TransUNet encoder, networks/trans_u_net/vit_seg_modeling.py:171-190,233-250),
 * x [rows][n], n in {256, 512, 768, 1024}, x / y / grad dtypes SIS_F32 or SIS_BF16 (fp32 arithmetic), gamma / beta [n].
 * fwd: y = (x - mean_row) * rstd_row * gamma + beta; mean / rstd [rows] kept.
 * bwd: dx (x's dtype), dgamma / dbeta [n]; workspace: sis_layer_norm_workspace_floats(n) floats. */
int sis_layer_norm_workspace_floats(int n);
int sis_layer_norm_fwd(void* y, float* mean, float* rstd, const void* x, const float* gamma, const float* beta, int x_dtype,
                       int y_dtype, int rows, int n, float eps, void* stream);
int sis_layer_norm_bwd(void* dx, float* dgamma, float* dbeta, float* workspace, const void* grad_y, const void* x,
                       const float* mean, const float* rstd, const float* gamma, int x_dtype, int g_dtype, int rows, int n,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * nn.UpsamplingBilinear2d (align_corners=True) of the TransUNet decoder
 * (networks/trans_u_net/vit_seg_modeling.py:290-329), forward and backward, f32 / f16 / bf16 (dtype = SIS_*).
 * backward = 0: out [planes][out_h][out_w] from x [planes][h][w].
 * backward = 1: out = grad_x [planes][h][w] from x = grad_out [planes][out_h][out_w] (gather, deterministic). */
int sis_upsample_bilinear(void* out, const void* x, int dtype, int64_t planes, int h, int w, int out_h, int out_w,
                          int backward, void* stream);
/* The same with an image stride on the UPSAMPLED-size tensor (elements between consecutive images; >= channels*out_h*out_w):
 * forward writes its result into the leading channels of a wider tensor, backward reads grad_out from there -- the decoder's
 * torch.cat([up(x), skip], dim=1) (vit_seg_modeling.py:300-303) then costs one copy of the skip feature only.  Strided
 * tensors need the x2 case (out_h = 2h, out_w = 2w). */
int sis_upsample_bilinear_strided(void* out, const void* x, int dtype, int batch, int channels, int h, int w, int out_h, int out_w,
                                  int64_t image_stride, int backward, void* stream);

/* Weight gradient of the same 1x1 convolutions (networks/hip_conv.py::_Pointwise.backward; reference layers as for
 * sis_conv1x1_f32): dw[co][ci] = sum_{b, p} gy[b][co][p] * x[b][ci][p], fp32 on the matrix cores, NCHW rows straight from
 * HBM by LDS-DMA, split-K over the (sample, pixel) stream with an ordered (deterministic) reduction through `workspace`
 * (sis_conv1x1_wgrad_f32_workspace bytes; fewer bytes = fewer slices, NULL = one).  Supported: hw % 64 == 0 and
 * (cout % 128 == 0 and cin % 64 == 0) or (cout % 64 == 0 and cin % 128 == 0) or (cout % 256 == 0 and cin % 32 == 0). */
int sis_conv1x1_wgrad_f32_supported(int batch, int cin, int cout, int hw);
int64_t sis_conv1x1_wgrad_f32_workspace(int batch, int cin, int cout, int hw);
int sis_conv1x1_wgrad_f32(float* dw, const float* gy, const float* x, int batch, int cin, int cout, int hw,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* (as sis_conv3x3_wgrad_multi; workspace: any size, the slices adapt -- sis_conv1x1_wgrad_f32_workspace x n_jobs is plenty) */
int sis_conv1x1_wgrad_f32_multi(float* const* dw, const float* const* gy, const float* const* x, int n_jobs, int batch, int cin, int cout,
                                int hw, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * nn.MaxPool2d / F.max_pool2d of the segmentation backbones (ceil_mode false, dilation 1): EMANet stem (3, 2, 1)
 * (networks/ema_net/network.py:66), TransUNet root (3, 2, 0) (vit_seg_modeling_resnet_skip.py:146); f32 / f16 / bf16.
 * backward = 0: out [planes][out_h][out_w] and argmax (one byte per output: kh * kernel + kw of the FIRST maximum in
 *               row-major window order, ATen's tie rule) from x [planes][h][w].
 * backward = 1: out = grad_x [planes][h][w] from x = grad_out [planes][out_h][out_w] and the forward's argmax (gather,
 *               deterministic, bit-equal to ATen's max_pool2d_with_indices_backward). */
int sis_max_pool2d(void* out, unsigned char* argmax, const void* x, int dtype, int64_t planes, int h, int w, int out_h,
                   int out_w, int kernel, int stride, int padding, int backward, void* stream);

/* ------------------------------------------------------------------------------------------
 * Patch-wise page inference.  The patch grid is the product of `nx` left edges `xs` and
 * `ny` top edges `ys` (device int32 arrays, ascending), patch n = yi * nx + xi, as
 * segmentation/analysis_segmenter.py:83-113 enumerates them.
 * sis_crop_patches_u8: image uint8 [height][width][channels] -> out float32 [ny*nx][channels][patch][patch] =
 *   ((u8 / 255) - 0.5) / 0.5 with zeros read outside the image (PIL crop + ToTensor + Normalize, :115-130).
 * sis_assemble_max: pred float32 [ny*nx][classes][patch][patch] -> out [classes][height][width] = maximum over
 *   the covering patches (:147-167); labels (uint8 [height][width], may be NULL) = first maximal class
 *   (networks/base_segmenter.py:59-62).  classes / channels <= 16. */
int sis_crop_patches_u8(float* out, const unsigned char* image, const int* xs, const int* ys, int nx, int ny,
                        int height, int width, int channels, int patch, void* stream);
int sis_assemble_max(float* out, unsigned char* labels, const float* pred, const int* xs, const int* ys, int nx,
                     int ny, int classes, int height, int width, int patch, void* stream);

/* ------------------------------------------------------------------------------------------
 * bf16 convolutions of the segmentation training step on the matrix cores, direct on NCHW tensors (csrc/conv_bf16.hip):
 * TransUNet under bf16 autocast -- StdConv2d 3x3 / 1x1 (networks/trans_u_net/vit_seg_modeling_resnet_skip.py:20-37,40-75),
 * decoder Conv2dReLU and segmentation head (vit_seg_modeling.py:265-287,324-329), patch embedding (:125-168).
 * Kernel sizes 1 and 3 (padding ksize/2), strides 1 and 2, Cin % 16 == 0 (% 64 for 1x1 stride 1); x / y bf16 NCHW,
 * fp32 accumulation, optional fp32 bias[cout] added before the rounding to bf16.
 *   sis_conv_bf16_supported     1 when a tile plan exists for the layer.
 *   sis_conv_bf16_packed_elems  bf16 elements of the packed weight image (-1: unsupported).
 *   sis_conv_bf16_pack          weight [cout][cin][k][k] (SIS_F32 or SIS_BF16) -> the kernel's LDS image, per output
 *                               channel tile / input channel chunk / tap / row, 16-byte units XOR-swizzled.
 *                               adjoint = 1 packs the convolution that takes dL/dy to dL/dx of a stride-1 layer
 *                               (channel roles swapped, taps rotated by 180 degrees); it is then used with
 *                               sis_conv_bf16(cin = the layer's cout, cout = the layer's cin).
 *   sis_conv_bf16               y [batch][cout][ho][wo] = conv(x [batch][cin][h][w], packed) (+ bias). */
int sis_conv_bf16_supported(int cin, int cout, int h, int w, int ksize, int stride);
int64_t sis_conv_bf16_packed_elems(int cin, int cout, int h, int w, int ksize, int stride, int adjoint);
int sis_conv_bf16_pack(void* packed, const void* weight, int weight_dtype, int cin, int cout, int h, int w, int ksize,
                       int stride, int adjoint, void* stream);
int sis_conv_bf16(void* y, const void* x, const void* packed, const float* bias, int batch, int cin, int cout, int h, int w,
                  int ksize, int stride, void* stream);
/* All StdConv2d layers of a network in ONE launch: standardise every filter (as sis_weight_std_fwd, bf16 result) and write it
 * into w_hat, into the forward image and (stride-1 layers) into the adjoint image of its layer
 * (networks/trans_u_net/vit_seg_modeling_resnet_skip.py:20-27: the reference standardises every weight in every forward).
 * `table`: device array of 14 int64 per layer -- pointers w (float32 [cout][cin][k][k]), w_hat (bf16), invstd (float32 [cout]),
 * packed, adjoint (0 = none), then cout, cin, k, mt, kc, mt2 (from sis_weight_std_pack_plan), rows = ceil(cout / mt) * mt,
 * row_begin = sum of the previous layers' rows, filter_begin = sum of the previous layers' cout; total_rows = sum of rows.  sis_weight_std_pack_plan returns 0 for a layer the
 * bf16 convolution kernels have no plan for. */
int sis_weight_std_pack_plan(int cin, int cout, int ksize, int stride, int* mt, int* kc, int* mt2, int64_t* packed_elems,
                             int64_t* adjoint_elems);
int sis_weight_std_pack_multi(const void* table, int n_layers, int total_rows, float eps, void* stream);
/* ... and its backward for all layers in one launch (per 64 layers): grads[i] = dL/dw_hat of layer i (bf16, device pointer, NULL =
 * no gradient for that layer), dw[i] = float32 result of the layer's weight shape; `grads`, `dw`, `couts` are HOST arrays of
 * n_layers entries in the table's layer order. */
int sis_weight_std_bwd_multi(const void* table, const void* const* grads, void* const* dw, const int* couts, int n_layers,
                             void* stream);
/* forward and adjoint packing of a stride-1 layer's weight in one launch (training: both are needed every step) */
int sis_conv_bf16_pack_both(void* packed, void* packed_adjoint, const void* weight, int weight_dtype, int cin, int cout, int h,
                            int w, int ksize, void* stream);

/* Weight gradient of a stride-1, padding-1 3x3 bf16 convolution (csrc/conv_bf16_wgrad.hip):
 * dw [cout][cin][3][3] (SIS_F32 or SIS_BF16) = sum_{n,y,x} grad_y[n][co][y][x] * x[n][ci][y+ky-1][x+kx-1], x / grad_y bf16
 * NCHW, fp32 accumulation; split-K partial tiles go through `workspace` and are added in a fixed order (deterministic).
 * sis_conv_bf16_wgrad_supported: 1 when a tile plan exists (cin, cout >= 32) and its slabs fit `workspace_bytes`. */
int sis_conv_bf16_wgrad_supported(int batch, int cin, int cout, int h, int w, int64_t workspace_bytes);
int sis_conv_bf16_wgrad(void* dw, int dw_dtype, const void* x, const void* grad_y, int batch, int cin, int cout, int h, int w,
                        void* workspace, int64_t workspace_bytes, void* stream);
/* The 1x1 stride-1 layers (conv1x1 / StdConv2d 1x1 of every bottleneck, vit_seg_modeling_resnet_skip.py:30-37,40-75; the
 * reference's autograd runs convolution_backward): dw [cout][cin] (SIS_F32 or SIS_BF16) = sum_{n,p} grad_y[n][co][p] * x[n][ci][p],
 * x [batch][cin][pixels] / grad_y [batch][cout][pixels] bf16 (NCHW with the plane flattened; any plane size, odd ones take a
 * funnel-shift load path), fp32 accumulation, unit slabs through `workspace` added in unit order (deterministic). */
int sis_conv1x1_bf16_wgrad_supported(int batch, int cin, int cout, int pixels, int64_t workspace_bytes);
int sis_conv1x1_bf16_wgrad(void* dw, int dw_dtype, const void* x, const void* grad_y, int batch, int cin, int cout, int pixels,
                           void* workspace, int64_t workspace_bytes, void* stream);
/* Both weight-gradient kernels for n_jobs layers of ONE shape (the trunk's repeated bottleneck units, queued during the
 * backward): `dw`, `x`, `grad_y` are HOST arrays of n_jobs device pointers; one tile launch (grid.z = layer) and one reduction
 * launch per <= 16 layers.  The tile plan counts the layers' workgroups together: each layer is cut into fewer, longer units than
 * it would be alone (less slab traffic, fewer prologues).  Results are those of the single-layer calls up to the order of the
 * fp32 partial sums. */
int sis_conv_bf16_wgrad_multi(void* const* dw, int dw_dtype, const void* const* x, const void* const* grad_y, int n_jobs, int batch,
                              int cin, int cout, int h, int w, void* workspace, int64_t workspace_bytes, void* stream);
int sis_conv1x1_bf16_wgrad_multi(void* const* dw, int dw_dtype, const void* const* x, const void* const* grad_y, int n_jobs, int batch,
                                 int cin, int cout, int pixels, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The root convolution of the hybrid trunk (networks/trans_u_net/vit_seg_modeling_resnet_skip.py:115-125: StdConv2d(3, 64,
 * kernel_size=7, stride=2, padding=3) on the image) on the bf16 matrix cores: forward and weight gradient (the image needs no
 * gradient).  x [B][3][h][w] float32 or bfloat16 (converted while staged), y / grad_y [B][64][ho][wo] bfloat16 with
 * ho = (h - 1) / 2 + 1.  `packed`: sis_stem_conv_packed_elems() bf16 elements written by sis_stem_conv_pack from the
 * (standardised) weight [64][3][7][7] (float32 or bfloat16).  dw [64][3][7][7] float32 or bfloat16; the partial sums of the
 * workgroups go through `workspace` (sis_stem_conv_wgrad_workspace_bytes) and are added in a fixed order. */
int sis_stem_conv_supported(int cin, int cout, int ksize, int stride, int padding, int h, int w);
int64_t sis_stem_conv_packed_elems(void);
int sis_stem_conv_pack(void* packed, const void* weight, int weight_dtype, void* stream);
int sis_stem_conv_fwd(void* y, const void* x, int x_dtype, const void* packed, int batch, int h, int w, void* stream);
int64_t sis_stem_conv_wgrad_workspace_bytes(int batch, int h, int w);
int sis_stem_conv_wgrad(void* dw, int dw_dtype, const void* x, int x_dtype, const void* grad_y, int batch, int h, int w, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * fp32 pointwise (1x1, stride 1) convolution of the EMANet training step (csrc/conv1x1_f32.hip;
 * networks/ema_net/network.py:24,29,106-107 Bottleneck conv1 / conv3 / downsample, :219-249 EMAU, :271-289 fc0 / fc1),
 * exact fp32 on v_mfma_f32_32x32x2_f32, NCHW in and out.
 *   data_gradient = 0:  y [batch][cout][hw] = weight [cout][cin] . x [batch][cin][hw] (+ bias[cout])
 *   data_gradient = 1:  y = dL/dx [batch][cin][hw] = weight^T . x, x = dL/dy [batch][cout][hw] (the weight tensor itself is
 *                       read as the k-major operand: no transposed copy)
 * Contraction length % 32 == 0, output channels % 4 == 0, hw % 4 == 0, 16-byte aligned pointers. */
int sis_conv1x1_f32_supported(int cin, int cout, int hw);
int sis_conv1x1_f32(float* y, const float* x, const float* weight, const float* bias, int batch, int cin, int cout, int hw,
                    int data_gradient, void* stream);
/* dx [batch][cin][hw] = weight^T . dy + skip_grad: the data gradient of a bottleneck's first 1x1 convolution with the gradient
 * that arrives over the identity shortcut (networks/ema_net/network.py:37-56: out = relu(bn3(...) + x)) added in the epilogue
 * instead of by a separate element-wise pass. */
int sis_conv1x1_f32_dgrad_add(float* dx, const float* dy, const float* weight, const float* skip_grad, int batch, int cin, int cout,
                              int hw, void* stream);

/* ------------------------------------------------------------------------------------------
 * bf16 GEMM with the Linear layers' element-wise tail fused into the epilogue (csrc/gemm_bf16.hip): the ViT encoder of
 * TransUNet under bf16 autocast -- Attention.query/key/value/out (networks/trans_u_net/vit_seg_modeling.py:60-67,76-96),
 * Mlp fc1 / GELU / dropout / fc2 / dropout (:104-122), the Block residual adds (:181-189); replaces F.linear (a library
 * GEMM) + separate bias / GELU / dropout / add / cast kernels, forward and backward.
 *   C[m][n] = epilogue( sum_k opA[m][k] * opB[k][n] ),  bf16 operands, fp32 accumulation, row-major C with leading dim ldc
 *   layout 0 (NT): A [m][k] (lda), B [n][k] (ldb)        forward:          y  = x W^T
 *   layout 1 (NN): A [m][k] (lda), B [k][n] (ldb)        data gradient:    dx = g W
 *   layout 2 (TN): A [k][m] (lda), B [k][n] (ldb)        weight gradient:  dW = g^T x   (k = tokens; any k >= 1)
 * epilogue:
 *   SIS_GEMM_EPI_NONE             C bf16 = acc
 *   SIS_GEMM_EPI_BIAS             C bf16 = acc + bias[n]
 *   SIS_GEMM_EPI_BIAS_GELU_DROP   with h = acc + bias:  C bf16 = dropout(gelu(h))  (erf GELU);  C2 bf16 = d C / d h = gelu'(h) * the same
 *                                 dropout factor -- what SIS_GEMM_EPI_GELU_BWD of the backward multiplies by (round 5: it was h, and the
 *                                 backward recomputed erf, exp and the dropout hash per element)
 *   SIS_GEMM_EPI_BIAS_DROP_RESID  C fp32 = resid[m][n] + dropout(acc + bias)      (resid fp32, leading dim ldc)
 *   SIS_GEMM_EPI_GELU_BWD         C bf16 = acc * pre[m][n]   (pre bf16, leading dim ldc: the C2 of the forward's SIS_GEMM_EPI_BIAS_GELU_DROP;
 *                                 seed / site / drop_p are not read)
 *   SIS_GEMM_EPI_F32              C fp32 = acc; with splits > 1 the K range is cut into `splits` slices whose partial results
 *                                 go through `workspace` and are added in slice order (deterministic)
 * dropout: element (m, n) of site `site` is dropped iff hash(seed word, site, m * n_cols + n) < drop_p * 2^32, else scaled by
 * 1 / (1 - drop_p); the forward and the backward launch of a site evaluate the same function (no stored mask).  `seed`
 * points to a 64-bit device word (sis_dropout_advance steps it once per iteration).  drop_p = 0: no dropout.
 * bias_seg > 0: the bias is three vectors of bias_seg = n / 3 entries (bias, bias1, bias2: the query | key | value biases of the
 * fused projection stay three parameters); bias_seg = 0: one vector `bias`.
 * tile (BM x BN x BK, LDS stages): 0 = 128x128x64 / 2, 1 = 256x128x64 / 2, 2 = 128x256x64 / 2, 3 = 256x256x64 / 2,
 * 4 = 128x128x32 / 3, 5 = 128x128x32 / 4, 6 = 128x128x64 / 3, 7 = 256x128x64 / 3 (one wave per 64x64 sub-tile),
 * 8 = 128x96x64 / 2 (NT only; waves of 64x48: n = 768 / 2304 give 512 / 1536 tiles = whole rounds of 2 workgroups per CU).  NT / NN need k % 64 == 0; n, ldc % 4 == 0;
 * lda, ldb % 8 == 0; 16-byte aligned pointers.  m (and k for TN) need not be tile multiples. */
#define SIS_GEMM_EPI_NONE 0
#define SIS_GEMM_EPI_BIAS 1
#define SIS_GEMM_EPI_BIAS_GELU_DROP 2
#define SIS_GEMM_EPI_BIAS_DROP_RESID 3
#define SIS_GEMM_EPI_GELU_BWD 4
#define SIS_GEMM_EPI_F32 5
/* tile codes 9..11: 256 x 96 / 256 x 192 / 256 x 288 output tiles, one 8-wave workgroup per compute unit, register-double-
 * buffered fragments over four LDS stages (csrc/gemm256_bf16.hip): layout NT only, splits == 1, k % 64 == 0, k >= 128, every
 * epilogue except SIS_GEMM_EPI_F32.  8 192-token GEMMs of width 768 / 3072 / 2304 give 256 / 512 / 256 such tiles. */
#define SIS_GEMM_TILE_256X96 9
#define SIS_GEMM_TILE_256X192 10
#define SIS_GEMM_TILE_256X288 11
int64_t sis_gemm_bf16_workspace_bytes(int m, int n, int splits);
int sis_gemm_bf16(void* c, void* c2, const void* a, const void* b, int layout, int epilogue, int m, int n, int k, int lda,
                  int ldb, int ldc, const float* bias, const float* bias1, const float* bias2, int bias_seg, const float* resid,
                  const void* pre, const void* seed, int site, float drop_p, int splits, void* workspace,
                  int64_t workspace_bytes, int tile, void* stream);
/* Weight gradient AND bias gradient of a Linear layer (what autograd computes as grad.t() @ x and grad.sum(0)) in the two
 * launches of the split-K weight gradient: dw [m][n] float32 (TN layout: grad [k][m], x [k][n], splits > 1), db [m] float32 =
 * column sums of grad by extra workgroups of the GEMM launch (dispatched last: they fill the slots its final, partly filled round
 * of tiles leaves idle) and of the slab reduction; sis_column_sum's summation order.
 * workspace: sis_gemm_bf16_workspace_bytes(m, n, splits) + 64 * m * 4 bytes; tile 0 or 4..6. */
int sis_gemm_bf16_wgrad_bias(void* dw, float* db, const void* grad, const void* x, int m, int n, int k, int lda, int ldb, int splits,
                             void* workspace, int64_t workspace_bytes, int tile, void* stream);
/* The same for n_jobs Linear layers of ONE shape (the encoder's twelve blocks, queued during the backward): one launch for the
 * n_jobs products -- every problem contracts its whole K per tile: no split-K, no slabs, no reduction launch -- and one for the
 * column sums.  `dw`, `db`, `grad`, `x`: HOST arrays of n_jobs device pointers (dw[j] [m][n] float32, db[j] [m] float32, grad[j]
 * bf16 [k][lda], x[j] bf16 [k][ldb]).  tile: a 128 x 128 four-wave tile code (0, 4, 5, 6).  workspace:
 * sis_gemm_bf16_wgrad_multi_workspace_bytes(n_jobs, m, k) bytes. */
int64_t sis_gemm_bf16_wgrad_multi_workspace_bytes(int n_jobs, int m, int k);
int sis_gemm_bf16_wgrad_bias_multi(void* const* dw, float* const* db, const void* const* grad, const void* const* x, int n_jobs, int m,
                                   int n, int k, int lda, int ldb, void* workspace, int64_t workspace_bytes, int tile, void* stream);

/* Transposed bf16 copies of `n_tensors` matrices by one launch (csrc/vit_elementwise.hip): dst_i [cols_i][rows_i] =
 * src_i [rows_i][cols_i]^T.  `table`: DEVICE array of n_tensors rows of 5 int64 {src, dst, rows, cols, first_tile} with
 * first_tile = running sum of ceil(rows / 64) * ceil(cols / 64); total_tiles = the final sum.  Used for the transposed
 * weight shadows that turn a Linear layer's data gradient into an NT product (sis_gemm_bf16 tiles 9..11). */
int sis_transpose_bf16_multi(const void* table, int n_tensors, int total_tiles, void* stream);
/* dst[b][c][r] = src[b][r][c] for 2- or 4-byte elements: `x.flatten(2).transpose(-1, -2)` of the patch embeddings
 * (networks/trans_u_net/vit_seg_modeling.py:151-153), `hidden_states.permute(0, 2, 1).contiguous()` of DecoderCup.forward
 * (:341-344), and the gradients of both (the same operation). */
int sis_transpose_batched(void* dst, const void* src, int elem_bytes, int batch, int rows, int cols, void* stream);

/* The same kernel over `batches` problems (grid.y): A / B / C of entry i start i * {a,b,c}_batch_stride elements after the base
 * pointers (stride 0 = shared operand).  With sum_over_batches != 0 the entries are the K slices of ONE result instead
 * (C fp32 [m][n] = sum_i op(A_i) op(B_i), ordered slab reduction through `workspace`; batches must be 1, 2, 4 or a multiple
 * of 8).  This is how the bf16 1x1 convolutions of TransUNet's ResNetV2 trunk run on NCHW tensors
 * (networks/trans_u_net/vit_seg_modeling_resnet_skip.py:30-37 conv1x1 / StdConv2d): per image
 *   forward          y_i [cout][hw] = W [cout][cin] . x_i [cin][hw]        layout NN, A shared
 *   data gradient    dx_i [cin][hw] = W^T . dy_i                           layout TN, A = W read K-major, shared
 *   weight gradient  dW [cout][cin] = sum_i dy_i [cout][hw] . x_i^T        layout NT, summed over the images
 * epilogue: SIS_GEMM_EPI_NONE (bf16) or SIS_GEMM_EPI_F32. */
int sis_gemm_bf16_batched(void* c, const void* a, const void* b, int layout, int epilogue, int m, int n, int k, int lda, int ldb,
                          int ldc, int batches, int64_t a_batch_stride, int64_t b_batch_stride, int64_t c_batch_stride,
                          int sum_over_batches, void* workspace, int64_t workspace_bytes, int tile, void* stream);

/* Dropout stream of the fused ViT-encoder kernels (csrc/vit_elementwise.hip; nn.Dropout of vit_seg_modeling.py:70-71,108,138).
 *   sis_dropout_advance   steps the 64-bit device seed word once per training iteration (graph-capturable).
 *   sis_dropout_bwd_cast  out bf16[numel] = grad fp32[numel] * dropout_factor(seed, site, element index): the gradient of
 *                         `resid + dropout(y)` w.r.t. y for a site whose forward ran as SIS_GEMM_EPI_BIAS_DROP_RESID with the
 *                         same site id and a dense [m][n] output (element index = m * n_cols + n). */
int sis_dropout_advance(void* seed, void* stream);
int sis_dropout_bwd_cast(void* out, const float* grad, int64_t numel, const void* seed, int site, float drop_p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused multi-head self-attention of the ViT encoder, head size 64 (csrc/attention_bf16.hip).
 * Replaces Attention.forward's  softmax(q k^T / sqrt(d)) v  with its transposes / permutes
 * (networks/trans_u_net/vit_seg_modeling.py:71-74,83-94; attention dropout rate 0.0, vit_seg_configs.py:16) and its backward.
 *   qkv    bf16 [batch][n][3 * heads * 64]   the fused query | key | value projection, read in place (head h = columns h*64..)
 *   ctx    bf16 [batch][n][heads * 64]       context, heads merged (what Attention.out consumes)
 *   lse    fp32 [batch][heads][n]            log-sum-exp of the scaled scores (saved for the backward)
 *   d_qkv  bf16, layout of qkv; d_ctx bf16, layout of ctx; delta fp32 [batch][heads][n] scratch (rowsum(d_ctx o ctx))
 * No [n][n] tensor is written; the backward accumulates nothing across workgroups (no atomics: bitwise reproducible). */
/* LayerNorm backward (csrc/layer_norm.hip) with the residual-block fusions of the ViT encoder (vit_seg_modeling.py:181-189):
 * dx = residual_grad + LN'(grad_y) (residual_grad fp32 or NULL), and optionally cast_out bf16 = dx * dropout factor of the
 * dropout site the previous residual add used (what sis_dropout_bwd_cast computes, without its pass over memory). */
int sis_layer_norm_bwd_fused(void* dx, float* dgamma, float* dbeta, float* workspace, const void* grad_y, const void* x,
                             const float* mean, const float* rstd, const float* gamma, int x_dtype, int g_dtype, int rows, int n,
                             const float* residual_grad, void* cast_out, const void* seed, int site, float drop_p, void* stream);
/* Deferred form of the LayerNorm parameter gradients (a ViT encoder has 25 norms; nothing reads d(gamma) / d(beta) before the
 * optimizer or the gradient exchange): sis_layer_norm_bwd_fused_partial = sis_layer_norm_bwd_fused without its reduction launch
 * (the sis_layer_norm_bwd_parts(rows) partial rows stay in `workspace`), sis_layer_norm_param_reduce_multi = the reductions of
 * `count` such jobs in one launch per 32 jobs (HOST arrays of device pointers / ints), bitwise the results of the undeferred call. */
int sis_layer_norm_bwd_fused_partial(void* dx, float* workspace, const void* grad_y, const void* x, const float* mean,
                                     const float* rstd, const float* gamma, int x_dtype, int g_dtype, int rows, int n,
                                     const float* residual_grad, void* cast_out, const void* seed, int site, float drop_p,
                                     void* stream);
int sis_layer_norm_bwd_parts(int rows);
int sis_layer_norm_param_reduce_multi(void* const* dgamma, void* const* dbeta, const void* const* part, const int* n_part,
                                      const int* n, int count, void* stream);
int sis_attention_fwd(void* ctx, float* lse, const void* qkv, int batch, int n, int heads, void* stream);
int sis_attention_bwd(void* d_qkv, float* delta, const void* d_ctx, const void* qkv, const void* ctx, const float* lse, int batch,
                      int n, int heads, void* stream);

/* ------------------------------------------------------------------------------------------
 * TransUNet objective, fused (csrc/loss_ops.hip):  0.5 * CrossEntropy + 0.5 * Dice(softmax)  of
 * updater/segmentation_updater.py:95-102 with networks/trans_u_net/utils.py:7-42 (DiceLoss, smooth 1e-5, sums over the batch).
 *   logits [batch][classes][hw] (SIS_F32 or SIS_BF16), labels int64 [batch][hw]; 2 <= classes <= 8, hw % 4 == 0.
 *   fwd: out3 = {combined, cross entropy, dice}; stats (1 + 2 * classes floats) = constants for the backward;
 *        workspace: sis_ce_dice_workspace_floats(classes) floats (per-workgroup partial sums, added in order: deterministic).
 *   bwd: grad_logits (dtype of logits) = d combined / d logits * grad_loss[0] (grad_loss NULL = 1).
 * Labels outside [0, classes) are ignored by the cross entropy and are an all-zero one-hot row for the Dice sums. */
int sis_ce_dice_workspace_floats(int classes);
int sis_ce_dice_fwd(float* out3, float* stats, float* workspace, const void* logits, int dtype, const int64_t* labels, int batch,
                    int classes, int hw, void* stream);
int sis_ce_dice_bwd(void* grad_logits, const void* logits, int dtype, const int64_t* labels, const float* stats,
                    const float* grad_loss, int batch, int classes, int hw, void* stream);

/* ---- DocUFCN segmenter (networks/doc_ufcn/doc_ufcn.py:11-101, training_builder/doc_ufcn_train_builder.py:18-33), fp32 NCHW
 * (csrc/doc_ufcn.hip).
 *   sis_dconv3x3           out [B][Cout][H][W] = conv2d(x, weight [Cout][Cin][3][3], bias or NULL, stride 1, padding = dilation,
 *                          dilation); any Cin, Cout >= 1.  Data gradient: the same call on sis_dconv3x3_adjoint's weights
 *                          (wa [Cin][Cout][3][3] = weight with the channel axes swapped and the taps rotated by 180 degrees).
 *   sis_dconv3x3_wgrad     dw [Cout][Cin][taps] from grad_output [B][Cout][H][W] and x [B][Cin][H][W]: taps 9 = the dilated 3x3
 *                          convolution above, taps 1 = a 1x1 product.  Fixed pixel slices summed in order.
 *   sis_channel_sum        out [C] = sum over batch and pixels of x [B][C][HW] (bias gradients), fixed order.
 *   sis_pixel_shuffle2     out [B][C][2H][2W] from in [B][4C][H][W] (nn.PixelShuffle(2) order) + bias [C] or NULL; inverse = 1:
 *                          out [B][4C][H][W] from in [B][C][2H][2W] (its gradient).  The wide map's samples are
 *                          wide_batch_stride floats apart (a channel slice of a wider buffer).
 *   sis_transpose2d        out [cols][rows] = in [rows][cols]^T.
 *   sis_bn_drop_fwd        y = dropout(relu(gamma * (x - mean) * invstd + beta)), y written with a batch stride (a channel slice of
 *                          a wider buffer); train mode: mean / invstd from sis_bn_stats, dropout of element e drawn from the
 *                          counter stream (seed word, site, quad e / 4), mask (sis_bn_mask_words int64 words, or NULL) = one bit
 *                          per element: (relu output > 0) & kept.  eval = 1: invstd_or_var is the running variance, no dropout.
 *   sis_bn_drop_bwd        dx, dgamma, dbeta from dy (batch stride dy_batch_stride) + dy2 (contiguous, or NULL) and the mask.
 *                          workspace: sis_bn_drop_bwd_workspace_floats floats, 16-byte aligned (the per-channel sums are kept in double).
 *   sis_weighted_ce_fwd    loss[0] = sum w[y] nll / sum w[y] (nn.CrossEntropyLoss(weight=w)); stats[0] = sum w[y]; weight NULL = 1.
 *   sis_weighted_ce_bwd    grad_logits = grad_loss[0] * d loss / d logits.
 *   sis_adam_clip_step     clip_grad_norm_(all gradients of the table, max_norm) then torch.optim.Adam (L2 weight decay added to the
 *                          gradient), one norm launch + one update launch.  table rows: param, grad, exp_avg, exp_avg_sq,
 *                          count | group << 48 (chunks of sis_adam_chunk_elems); hyper float[21]: {lr, beta1, beta2, eps,
 *                          weight_decay} per group (<= 4), max_norm; step: device int32 counter, incremented by the call;
 *                          partial: float[n_chunks]. */
int sis_dconv3x3(float* out, const float* x, const float* weight, const float* bias, int batch, int cin, int cout, int h, int w,
                 int dilation, void* stream);
int sis_dconv3x3_adjoint(float* wa, const float* weight, int cin, int cout, void* stream);
int64_t sis_dconv3x3_wgrad_workspace_floats(int batch, int cin, int cout, int h, int w, int taps);
int sis_dconv3x3_wgrad(float* dw, const float* grad_output, const float* x, float* workspace, int64_t workspace_floats, int batch,
                       int cin, int cout, int h, int w, int dilation, int taps, void* stream);
int sis_channel_sum(float* out, const float* x, int batch, int channels, int hw, void* stream);
int sis_pixel_shuffle2(float* out, const float* in, const float* bias, int batch, int channels, int h, int w,
                       int64_t wide_batch_stride, int inverse, void* stream);
int sis_transpose2d(float* out, const float* in, int rows, int cols, void* stream);
int64_t sis_bn_drop_bwd_workspace_floats(int batch, int channels, int hw);
int sis_bn_drop_fwd(float* y, int64_t y_batch_stride, const float* x, const float* mean, const float* invstd_or_var,
                    const float* gamma, const float* beta, int batch, int channels, int hw, int eval, float eps, const void* seed,
                    int site, float drop_p, void* mask, void* stream);
int sis_bn_drop_bwd(float* dx, float* dgamma, float* dbeta, const float* dy, int64_t dy_batch_stride, const float* dy2,
                    const float* x, const float* mean, const float* invstd, const float* gamma, const void* mask, float drop_p,
                    float* workspace, int batch, int channels, int hw, void* stream);
int sis_weighted_ce_workspace_floats(void);
int sis_weighted_ce_fwd(float* loss, float* stats, float* workspace, const float* logits, const int64_t* labels, const float* weight,
                        int batch, int classes, int hw, void* stream);
int sis_weighted_ce_bwd(float* grad_logits, const float* grad_loss, const float* logits, const int64_t* labels, const float* weight,
                        const float* stats, int batch, int classes, int hw, void* stream);
int sis_adam_chunk_elems(void);
int sis_adam_clip_step(const int64_t* table, int n_chunks, float* partial, const float* hyper, int* step, void* stream);

/* ------------------------------------------------------------------------------------------
 * DatasetGAN labelling (csrc/pixel_ensemble.hip): PixelEnsembleClassifier.predict_classes on the bilinearly upsampled
 * generator activations (reference segmentation/dataset_gan_segmenter.py, data/dataset_gan_dataset.py:12-34,
 * networks/pixel_classifier/model.py:13-121), eval mode, fp32, without the [B, S, S, F] feature tensor.
 * _project: for each of `ngroups` activation resolutions r below the output size, out[B][r*r][m] = wt[K][m]^T . act,
 *   where act is the K range over one or two layers [B][c][r*r]; `groups` is a HOST array of 7 int64 per group:
 *   {r, wt, out, act0, act1, c0, c1} (c1 = 0: one layer; c0, c1 multiples of 32; m a multiple of 128).
 * _head: labels[B][S*S] (int64) = the members' majority vote (ties: torch.mode on the device) of argmax over classes of
 *   W3 relu(W2 relu(W1f . act_full + sum_r up(P_r) + b1) + b2) + b3, BatchNorm folded into W2 / W3 by the caller.
 *   `full`: HOST {act0, act1, c0, c1} of the full-resolution layers (c0 = 0: none); `proj`: HOST {P_r, r} pairs.
 *   w1f [Kf][members*hidden1], b1 [members*hidden1], w2t [members][hidden1][H2], b2 [members][H2],
 *   w3t [members][H2][CP], b3 [members][CP] with (hidden1, H2, CP) = (128, 32, 32) for 2..31 classes, (256, 128, 64) for 32..64.
 *   rgb (optional) [B][S*S][3] = lut[label]; logits (optional, tests) [members][B][S*S][classes]. */
int sis_pixel_ensemble_project(const int64_t* groups, int ngroups, int batch, int m, void* stream);
int sis_pixel_ensemble_head(const int64_t* full, const int64_t* proj, int nproj, const float* w1f, const float* b1,
                            const float* w2t, const float* b2, const float* w3t, const float* b3, const uint8_t* lut,
                            int64_t* labels, uint8_t* rgb, float* logits, int batch, int size, int members, int classes,
                            int hidden1, void* stream);

/* ------------------------------------------------------------------------------------------
 * DatasetGAN training (csrc/pixel_ensemble_train.h): one step of every member of a narrow PixelEnsembleClassifier
 * (hidden widths 128 and 32, 2..31 classes, 1..10 members) on `npix` >= 2 pixels; fp32, deterministic (fixed summation orders,
 * no atomics).  The members are batched along the column axis: w1 [members*128][features], b1 / g1 / be1 [members*128],
 * w2 [members][32][128], b2 / g2 / be2 [members*32], w3 [members][classes][32], b3 [members][classes].
 * _workspace_bytes: bytes of `workspace` for _tail (piece 0) or _l1_wgrad (piece 1); -1 for an unsupported shape.
 * _gather: x[npix][features] from `layers` resident activation layers [images][c][res][res]; the table holds 4 int64 per layer
 *   {pointer, c, res, first column}, once on the HOST (checked) and once on the DEVICE (read by the kernel); pixels int32
 *   [npix][3] = (image, y, x); bilinear, align_corners=False, the source indices of _head; res == size is a plain read.
 * _l1_forward: a1[npix][members*128] = relu(x w1^T + b1).
 * _tail: BatchNorm 1 (batch statistics), layer 2, BatchNorm 2, layer 3, mean cross-entropy and their backward.
 *   params {g1, be1, w2, b2, g2, be2, w3, b3}; running {mean1, var1, mean2, var2, tracked1, tracked2} (entries may be null;
 *   momentum 0.1, unbiased variance; tracked: int64 [members], += 1); grads {dg1, dbe1, dw2, db2, dg2, dbe2, dw3, db3} (the order of params);
 *   dz1[npix][members*128] = d loss / d (x w1^T + b1); loss[members]; logits (optional, tests) [members][npix][classes].
 * _l1_wgrad: dw1[members*128][features] = dz1^T x (npix in slabs added in slab order), db1 = the column sums of dz1. */
int64_t sis_pe_train_workspace_bytes(int piece, int pixels, int features, int members);
int sis_pe_train_gather(const int64_t* table_host, const int64_t* table_dev, int layers, const int32_t* pixels, float* x, int npix,
                        int features, int size, int images, void* stream);
int sis_pe_train_l1_forward(const float* x, const float* w1, const float* b1, float* a1, int npix, int features, int members,
                            void* stream);
int sis_pe_train_tail(const float* a1, const int64_t* labels, const void* const* params, void* const* running, void* const* grads,
                      float* dz1, float* loss, float* logits, void* workspace, int npix, int members, int classes, void* stream);
int sis_pe_train_l1_wgrad(const float* dz1, const float* x, float* dw1, float* db1, void* workspace, int npix, int features,
                          int members, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fitting spherical k-means activation catalogs (csrc/spherical_kmeans.hip): the arithmetic of
 * MiniBatchSphericalKMeans.fit (reference segmentation/gan_local_edit/spherical_kmeans.py:161-312) as called by
 * FactorCatalog.fit_predict (factor_catalog.py:64-67) from create_semantic_segmentation.py:114-129, on the NCHW activation
 * x [B][C][HW] as the generator wrote it.  Row n = b*HW + p of the reference's partial_flat(x) is pixel p of sample b.
 * Envelope: C a multiple of 8 up to 512, at most 32 centres, batch_size at most 256, B*HW below 2^31.  All fp32 data; counts,
 * sums over members, norms and the stop rule in double; no floating-point atomics (same bytes on every run).
 * _gather: out[i][0..C) = x_row(idx[i]) / |x_row(idx[i])| (a zero row stays zero), replacing the normalize(X) of the whole
 *   matrix (spherical_kmeans.py:201) for the few rows a plan uses.
 * _loop: one workgroup per fit runs up to `iters` mini-batch iterations (spherical_kmeans.py:262-296, the step :36-156) and
 *   stops early on the no-improvement rule; fits whose state says done are skipped.  state [n_fits][sis_skm_state_doubles()]:
 *   {ewa, ewa_min, iteration, no_improvement, done, last mini-batch inertia, k, has_ewa, counts[32]}; centres [n_fits][32][C]
 *   (rows 0..k-1 used); last_labels [n_fits][256]: labels of the last mini-batch it ran; rows [iters][batch_size][C]: the unit
 *   rows of this chunk's planned mini-batches (shared by all fits); picks [iters][32]: distinct mini-batch positions per
 *   iteration for the reassignment rule.  alpha: the EWA factor min(2*batch_size/(N+1), 1).
 * _label: labels[n] = argmax_k (x_n.c_k/|x_n| - |c_k|^2/2) (= argmin |xhat_n - c_k|^2, lowest k on ties), result[0] = inertia =
 *   sum_n |xhat_n - c_label|^2, result[1+k] = pixels of centre k (spherical_kmeans.py:298-300 _labels_inertia); workspace
 *   sis_skm_label_workspace_doubles(B*HW) doubles, result 33 doubles. */
int sis_skm_state_doubles(void);
int sis_skm_gather(float* out, const float* x, const int* idx, int64_t n_rows, int batch, int channels, int hw, void* stream);
int sis_skm_loop(double* state, float* centres, int* last_labels, const float* rows, const int* picks, int n_fits, int channels,
                 int batch_size, int iters, double alpha, int max_no_improvement, double reassignment_ratio, int64_t max_iterations,
                 void* stream);
int64_t sis_skm_label_workspace_doubles(int64_t n_pixels);
int sis_skm_label(int64_t* labels, double* result, double* workspace, const float* x, const float* centres, int batch, int channels,
                  int hw, int n_centres, void* stream);

/* ------------------------------------------------------------------------------------------
 * Page evaluation (csrc/page_ops.hip, csrc/contour_ops.hip): what the reference's
 * segmentation/evaluation/analyze_image_segments.py does per page besides running the network.
 * sis_assemble_vote: VotingAssemblySegmenter.assemble_predictions (segmentation/analysis_segmenter.py:198-223); arguments as
 *   sis_assemble_max.  out[c][y][x] = (sum over the covering patches, row-major) / (sum of that over c), 0 where the divisor
 *   is 0; labels (optional) uint8 first maximal class of out.
 * sis_confusion_matrix: matrix[t][p] += #{pixels with ground truth t and predicted class p} (int64 [classes][classes] on the
 *   device, accumulated: the caller zeroes it once per run).  prediction: confidences [classes][pixels] (first maximal class)
 *   or null, then labels uint8 [pixels] is read.  classes <= 16.
 * sis_color_to_class: out[i] = id of the LAST of `count` colours equal to image[i] (uint8 [pixels][3]), else background_id;
 *   colors / ids are HOST arrays ([count][3] r, g, b; [count]), count <= 64.
 * sis_remove_small_contours: BaseSegmenter.postprocess (networks/base_segmenter.py:25-52) on pred [batch][classes][p][p]:
 *   confidence threshold, then every region of a non-background plane whose contour area is below min_contour_area is zeroed.
 *   Exact definition (mask, 5x5 closing, outside, regions, area through 2x2 blocks): DESIGN.md §10.  p <= 1024; workspace of
 *   sis_contour_workspace_bytes(batch*classes, p) bytes, 4-byte aligned; fixed launch sequence, no host sync, bit-reproducible. */
int sis_assemble_vote(float* out, uint8_t* labels, const float* pred, const int* xs, const int* ys, int nx, int ny, int classes,
                      int height, int width, int patch, void* stream);
int sis_confusion_matrix(int64_t* matrix, const float* prediction, const uint8_t* labels, const uint8_t* ground_truth,
                         int64_t pixels, int classes, void* stream);
int sis_color_to_class(uint8_t* out, const uint8_t* image, int64_t pixels, int background_id, const uint8_t* colors,
                       const uint8_t* ids, int count, void* stream);
int64_t sis_contour_workspace_bytes(int planes, int p);
int sis_remove_small_contours(float* out, const float* pred, void* workspace, int64_t workspace_bytes, int batch, int classes,
                              int p, float min_confidence, int min_contour_area, int background_class_id, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cluster-based dataset labelling (csrc/cluster_segment.hip): what the reference's
 * BlackWhiteHandwrittenPrintedTextDatasetSegmenter.create_segmentation_image does per batch after FactorCatalog.predict
 * (segmentation/black_white_handwritten_printed_text_segmenter.py:31-99 on top of
 * segmentation/base_cluster_based_dataset_segmenter.py:119-450: class merging, nearest resize, keys_to_merge, dilation,
 * external contours, merging across layers, classification of the fine-grained contours, area filter, drop decision,
 * rendering), instead of Python loops over OpenCV calls on the host.
 * sis_cluster_segment: cluster_maps is a HOST array of num_keys device pointers (int64 [batch][resolutions[k]]^2, a cluster id
 *   outside 0..255 belongs to no class), lut is on the DEVICE ([num_keys][256], bit c: the cluster belongs to non-background
 *   class c).  determination_sources / fine_sources (HOST, one byte per key of the step): bit k set = cluster map k is OR-ed
 *   into that key's masks (keys_to_merge resolved by the caller).  class_ids / colours (HOST, [classes + 1] / [classes + 1][3]):
 *   entry 0 is the background, entry 1 + c non-background class c.  Outputs class_map uint8 [batch][size]^2, colour uint8
 *   [batch][size]^2[3], drop uint8 [batch].  size <= 1024, num_keys and keys per step <= 8, classes <= 7; workspace of
 *   sis_cluster_segment_workspace_bytes(...) bytes, 16-byte aligned; fixed launch sequence, no host sync, bit-reproducible. */
int64_t sis_cluster_segment_workspace_bytes(int batch, int size, int num_determination, int num_fine, int classes);
int sis_cluster_segment(uint8_t* class_map, uint8_t* colour, uint8_t* drop, const int64_t* const* cluster_maps,
                        const int* resolutions, int num_keys, const uint8_t* lut, const uint8_t* determination_sources,
                        int num_determination, const uint8_t* fine_sources, int num_fine, int classes, int fine_class,
                        const uint8_t* class_ids, const uint8_t* colours, int batch, int size, int only_keep_overlapping,
                        int min_class_contour_area, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-time augmentation of a device-resident [image | label] dataset (csrc/augment.hip): what the
 * reference's augment_image (utils/augment_dataset.py:33-59: SomeOf(elastic, ShearX, CropAndPad, translate), Rot90 / Rotate,
 * GammaContrast / Invert) and AugmentedSegmentationDataset.__getitem__ (data/segmentation_dataset.py:80-107: augment, ToTensor,
 * Normalize(0.5, 0.5), colours -> class ids, resize to image_size) do per sample with imgaug and PIL on the host, for a batch.
 * The augmentation is stated exactly in DESIGN.md §12 and is NOT pinned against imgaug.
 * sis_augment_warp (utils/augment_dataset.py:33-59, data/segmentation_dataset.py:80-107): one launch per batch.  pixels uint8
 *   [n_samples][height][width][3] and classes uint8 [n_samples][height][width] are the resident dataset; slot b of the batch
 *   reads sample index[b] (an id outside 0..n_samples-1 yields a zero image / background).  For output pixel (x, y) of slot b:
 *   q = minv[b] (row-major 2x3) * (x, y, 1); with f = field_slot[b] in 0..num_fields-1, s = q + (field[f][0], field[f][1])
 *   sampled bilinearly at q with edge clamp (field [num_fields][2][height][width], component 0 = x), else s = q; image value =
 *   sum over the four bilinear taps around s of w * lut[b][source byte], a tap outside the source contributing 0; with
 *   `quantize` rounded half-to-even to a byte; then / 255, - 0.5, / 0.5 in true divisions (as sis_crop_patches_u8) into images
 *   float32 [batch][3][out_h][out_w]; segmented int64 [batch][1][out_h][out_w] = the source class at (floor(s_x + 0.5),
 *   floor(s_y + 0.5)), background_id outside.  All device pointers; no host sync.
 * sis_elastic_field (utils/augment_dataset.py:35, iaa.ElasticTransformation): field[f][c] = alpha[f] * (G * noise[f][c]), G the
 *   separable Gaussian of sigma[f] with radius floor(4 sigma + 0.5), weights normalised to sum 1, mirror boundary
 *   (scipy.ndimage.gaussian_filter(mode="mirror", truncate=4.0)).  noise (device, [num_fields][2][height][width]) when given,
 *   else uniform in [-1, 1) from the counter hash of (seeds[f], c, y * width + x) stated in DESIGN.md §12; noise_out (optional,
 *   same shape) receives the noise used.  alpha / sigma / seeds are HOST arrays; sigma in (0, 9], num_fields <= 64, height and
 *   width above the radius; workspace: num_fields * 2 * height * width floats. */
int sis_augment_warp(float* images, int64_t* segmented, const uint8_t* pixels, const uint8_t* classes, const int* index,
                     const float* minv, const uint8_t* lut, const int* field_slot, const float* field, int64_t n_samples,
                     int batch, int height, int width, int num_fields, int background_id, int out_h, int out_w, int quantize,
                     void* stream);
int sis_elastic_field(float* field, float* workspace, float* noise_out, const float* noise, const float* alpha, const float* sigma,
                      const uint32_t* seeds, int num_fields, int height, int width, void* stream);

/* ------------------------------------------------------------------------------------------
 * Projection encoders, inference path (csrc/encoder_ops.h): the layers of the reference's U-Net-like W+
 * encoders (networks/encoder/u_net_like_encoder.py:28-63 torchvision BasicBlocks, :73-78 the 1x1 heads, :94-114
 * WPlusEncoder.forward) that sis_conv3x3 and sis_bn_act_fwd do not take.  fp32 NCHW; eval-mode BatchNorm enters folded:
 * scale = gamma / sqrt(var + eps), shift = beta - mean * scale.  No host sync, no atomics, bit-reproducible.
 * sis_enc_conv3x3_s2 (u_net_like_encoder.py:42-50, a stride-2 BasicBlock's conv1 + bn1 + relu and its downsample =
 *   Conv2d(1x1, stride 2) + BatchNorm2d): y_main = relu(scale1 * conv3x3_s2_p1(x, w1) + shift1) and, when y_short is given,
 *   y_short = scale_d * conv1x1_s2(x, wd) + shift_d (a convolution bias folded into shift_d), both [batch][cout][h/2][w/2],
 *   from one read of x.  `packed` comes from sis_enc_conv3x3_s2_pack (w1 [cout][cin][3][3], wd [cout][cin] or null) and holds
 *   sis_enc_conv3x3_s2_packed_floats floats; y_short needs an image packed with wd.  cin % 8 == 0, h and w even, and
 *   the staged tile within 64 KiB of LDS: 32 * (640 + (2 r + 1) * (w + 1)) <= 65536 bytes with r = min(h / 2, 128 / (w / 2) if
 *   w / 2 divides 128, else 128 / (w / 2) + 2) output rows per 128-pixel tile -- every power-of-two width up to 256, other
 *   widths up to about 200 (sis_enc_conv3x3_s2_supported answers for a shape).
 * sis_enc_stem (u_net_like_encoder.py:28-35, the start block from the image): y_main = relu(scale1 * conv3x3_p1(x, w1) + shift1),
 *   y_short = scale_d * (conv1x1(x, wd) + bias_d) + shift_d (bias_d may be null), stride 1, 1 <= cin <= 4.
 * sis_enc_block_tail (BasicBlock.forward's out = relu(bn2(conv2) + identity); u_net_like_encoder.py:102,106 to_noise /
 *   intermediate_to_noise, :101,104 the adaptive_avg_pool2d): y = relu(scale * c + shift + residual) (residual may be null);
 *   noise [batch][1][hw] = sum_c noise_w[c] * y[.][c][.] + noise_b[0] when noise is given; partial [batch][channels][tiles],
 *   tiles = sis_enc_block_tail_tiles(hw), = the sums of y over 256-pixel tiles when partial is given.  hw % 4 == 0.  The
 *   channels are split over workgroups (a split that depends on channels and hw only, not on the batch); the noise output
 *   then needs noise_workspace of sis_enc_block_tail_workspace_floats(batch, channels, hw) floats (0: none needed), 16-byte
 *   aligned, for the slices' sums, which a second launch adds in slice order.
 * sis_enc_latent_heads (u_net_like_encoder.py:101,104 to_latent on the pooled map, :108-110 reverse + stack; :161 WEncoder;
 *   :175,240 the sums of WWPlusEncoder / WNoNoiseEncoder): table (device) holds n_heads rows of 8 int64 {partial pointer,
 *   weight pointer [latent][C], bias pointer [latent], C, tiles, hw, slot, 0}; out[b][slot][:] = W * (sum of the tile
 *   partials / hw) + bias, out being [batch][n_slots][latent]; with sum_heads (n_slots = 1) out[b][0][:] = the sum of all heads
 *   in table order.  The CALLER guarantees max_channels >= every C of the table and 0 <= slot < n_slots (the table is
 *   device memory the entry cannot read; sis_hip.enc_heads_table builds and checks both); (max_channels + latent) * 4 <= 48 KiB. */
int sis_enc_conv3x3_s2_supported(int cin, int cout, int h, int w);
int64_t sis_enc_conv3x3_s2_packed_floats(int cin, int cout, int with_shortcut);
int sis_enc_conv3x3_s2_pack(float* packed, const float* w1, const float* wd, int cin, int cout, void* stream);
int sis_enc_conv3x3_s2(float* y_main, float* y_short, const float* x, const float* packed, const float* scale1,
                       const float* shift1, const float* scale_d, const float* shift_d, int batch, int cin, int cout, int h,
                       int w, void* stream);
int sis_enc_stem_supported(int cin, int cout, int h, int w);
int sis_enc_stem(float* y_main, float* y_short, const float* x, const float* w1, const float* wd, const float* bias_d,
                 const float* scale1, const float* shift1, const float* scale_d, const float* shift_d, int batch, int cin,
                 int cout, int h, int w, void* stream);
int sis_enc_block_tail_supported(int channels, int hw);
int sis_enc_block_tail_tiles(int hw);
int64_t sis_enc_block_tail_workspace_floats(int batch, int channels, int hw);
int sis_enc_block_tail(float* y, float* noise, float* partial, const float* c, const float* residual, const float* scale,
                       const float* shift, const float* noise_w, const float* noise_b, float* noise_workspace, int batch,
                       int channels, int hw, void* stream);
int sis_enc_latent_heads_supported(int max_channels, int latent);
int sis_enc_latent_heads(float* out, const int64_t* table, int n_heads, int batch, int latent, int n_slots, int sum_heads,
                         int max_channels, void* stream);

/* ------------------------------------------------------------------------------------------
 * GAN training from an image list (csrc/gan_train_ops.h).  fp32 NCHW; no host sync, no atomics, every sum in a
 * fixed order: bit-reproducible.
 * sis_gan_image_batch (utils/data_loading.py:38-42, transforms.ToTensor + Normalize((0.5,) * 3, (0.5,) * 3) of a batch the
 *   DataLoader collates): images uint8 [n_images][3][size][size] resident on the device, ids int32 [batch] (device) ->
 *   out float32 [batch][3][size][size] = (v / 255 - 0.5) / 0.5 with true fp32 divisions in that order, bit-equal to the
 *   reference's transform.  An id outside 0 .. n_images - 1 yields a NaN sample and reads nothing.  16-byte stores when
 *   3 * size * size % 4 == 0 (every even size), out 16-byte and images 4-byte aligned; one element per thread otherwise.
 * sis_phase_split / sis_phase_merge (F.pixel_unshuffle / F.pixel_shuffle by 2; the reference has no counterpart: it runs
 *   networks/stylegan2/model.py:564-609 ConvLayer(downsample=True) as Blur + stride-2 conv2d): x [batch][channels][h][w] <->
 *   phases [batch][4 channels][h/2][w/2], phases[b][4 c + 2 py + px][i][j] = x[b][c][2 i + py][2 j + px]; `channels`, h, w are
 *   those of x in both calls.  h and w even (sis_phase_split_supported).  The two are inverses and mutual adjoints.  16-byte
 *   accesses on both sides when w % 8 == 0 and both pointers are 16-byte aligned.
 * sis_down_weight_compose (model.py:564-609 with :55-73 Blur, :94-131 EqualConv2d): Blur(pad = (2, 2), fir [4][4]) followed by
 *   conv2d(stride 2, padding 0) with scale * w, w [cout][cin][3][3], is ONE 6 x 6 stride-2 kernel
 *   K[m][n] = scale * sum_{i,j} w[i][j] * fir[3 - (m - i)][3 - (n - j)], which over the phases of its input is the 3 x 3 stride-1
 *   padding-1 convolution with w_phases [cout][4 cin][3][3], w_phases[co][4 ci + 2 py + px][a][b] = K[co][ci][2 a + py][2 b + px].
 *   fir is device memory, NORMALISED taps as Blur holds them.  Only a 4 x 4 fir (sis_down_weight_compose_supported).
 * sis_down_weight_compose_adjoint: the transpose of that linear map, dw_phases [cout][4 cin][3][3] -> dw [cout][cin][3][3],
 *   scale included.  w_phases / dw_phases 16-byte aligned. */
int sis_gan_image_batch(float* out, const uint8_t* images, const int* ids, int64_t n_images, int batch, int size, void* stream);
int sis_phase_split_supported(int h, int w);
int sis_phase_split(float* phases, const float* x, int batch, int channels, int h, int w, void* stream);
int sis_phase_merge(float* x, const float* phases, int batch, int channels, int h, int w, void* stream);
int sis_down_weight_compose_supported(int fir_h, int fir_w);
int sis_down_weight_compose(float* w_phases, const float* w, const float* fir, int fir_h, int fir_w, float scale, int cout, int cin,
                            void* stream);
int sis_down_weight_compose_adjoint(float* dw, const float* dw_phases, const float* fir, int fir_h, int fir_w, float scale, int cout,
                                    int cin, void* stream);

/* ------------------------------------------------------------------------------------------
 * PNG files of the dataset's [image | label] pairs, encoded on the device (csrc/png_encode.h).  Integer
 * arithmetic only; two encodes of the same input give the same bytes.
 * sis_png_capacity (create_dataset_for_segmentation.py:84-90, save_image): the per-image stride of the output buffer in bytes
 *   for files of `height` rows and `width_total` = image width + label width pixels: with F = height * (1 + 3 * width_total)
 *   filtered bytes, 57 + 2 + ceil((10 + 9 F) / 8) + 4 rounded up to a multiple of 16.  Host query; 0 for a size < 1.
 * sis_png_encode_pairs_workspace_bytes (:84-90, save_image): bytes of device workspace of one call (row offsets, checksums).
 * sis_png_encode_pairs (:84-90, save_image; :62-67 the concatenation of image and label, here never materialised): image
 *   uint8 [n][height][image_width][3], label uint8 [n][height][label_width][3] or null with label_width 0 (device) ->
 *   out[i * out_stride ...] the complete PNG file of pair i (8-bit RGB, width image_width + label_width, one IDAT: filter
 *   Sub on every row, one deflate block with the fixed Huffman codes, run-length matches at distance 1; the byte format is
 *   stated in DESIGN.md §14) and sizes[i] its length in bytes (int32, device).  The entry clears all n * out_stride bytes
 *   itself.  ihdr_crc: CRC-32 of "IHDR" + its 13 data bytes (it depends on the two sizes only; the caller computes it).
 *   Declines with an error code and launches nothing when n, height or image_width is < 1, label_width < 0 (or not 0 without
 *   a label, or 0 with one), image_width + label_width > 4096, n > 65535, out_stride < sis_png_capacity or no multiple of 16,
 *   out not 16-byte aligned, or the workspace smaller than the query says. */
int64_t sis_png_capacity(int height, int width_total);
int64_t sis_png_encode_pairs_workspace_bytes(int n, int height);
int sis_png_encode_pairs(uint8_t* out, int* sizes, const uint8_t* image, const uint8_t* label, int n, int height, int image_width,
                         int label_width, int64_t out_stride, uint32_t ihdr_crc, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Reconstruction metrics and the denoising loader (csrc/eval_ops.h).  No host sync, no atomics, every sum in a
 * fixed order: bit-reproducible and capturable.
 * sis_psnr_ssim_tile: the tile edge of the SSIM kernel (tests size a shape around it).
 * sis_psnr_ssim_workspace_bytes: bytes of device workspace of one sis_psnr_ssim call (tile partials, partial minima).
 * sis_psnr_ssim (evaluation/psnr_ssim.py:14-39, PSNRSSIMEvaluator.unnormalize / psnr / ssim of every sample of a batch; the
 *   reference calls kornia once per image at batch size 1): image, target float32 [batch][channels][height][width] ->
 *   psnr[b] = 10 log10(max_val^2 / mse_b), the POSITIVE metric (kornia.psnr_loss changed sign between versions; what is reported
 *   is the metric), +inf where mse_b == 0; ssim[b] = mean over the sample of clamp(s, 0, 1), the value of the reference's
 *   (1 - 2 ssim_loss(..., reduction='none')).mean() with ssim_loss = clamp(1 - s, 0, 1) / 2; and, where ssim_map is not null,
 *   ssim_map [batch][channels][height][width] = the unclamped s.  s = (2 mu_x mu_y + C1)(2 sigma_xy + C2) / ((mu_x^2 + mu_y^2 +
 *   C1)(sigma_x^2 + sigma_y^2 + C2)), mu = the image filtered with the normalised separable Gaussian of `window` taps and sigma
 *   1.5 under reflect padding that does not repeat the edge, sigma_x^2 = G(x^2) - mu_x^2, sigma_xy = G(xy) - mu_x mu_y,
 *   C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2.  mode 0: per sample, a tensor whose minimum is < 0 is first mapped by
 *   x <- (clamp(x, -1, 1) + 1) / 2 (pytorch_training's clamp_and_unnormalize), image and target decided independently, as
 *   `unnormalize` does at batch size 1; mode 1: both always; mode 2: neither.  Moments and sums are accumulated in double.
 *   window odd in 3..11, height and width > window / 2, batch <= 65535, a sample < 2^31 elements; workspace 8-byte aligned.
 * sis_autoencoder_batch (data/autoencoder_dataset.py:21-36 __getitem__, :44-54 iaa.AdditiveGaussianNoise, :59-67 the grey
 *   conversion, with the DataLoader's collate): images uint8 [n_images][3][size][size] resident on the device, ids int32 [batch],
 *   per-sample scale float [batch], per_channel int32 [batch], seed uint32 [batch], grey int32 [batch] (all device) ->
 *   output_image = (p / 255 - 0.5) / 0.5, bit-equal to sis_gan_image_batch, and input_image = the same map of
 *   q = clip(rint(p + scale * z), 0, 255) (half to even), z a standard normal by Box-Muller from a counter hash of (seed,
 *   component, pixel) (bit recipe: DESIGN.md §15), one z per pixel shared by the three channels unless per_channel; with grey,
 *   after the noise, all three channels become (19595 R + 38470 G + 7471 B + 32768) >> 16 (PIL's convert('L').convert('RGB')).
 *   Both outputs float32 [batch][3][size][size], written in one launch.  scale == 0 reproduces p.  An id outside 0 .. n_images - 1
 *   yields NaN samples and reads nothing.  16-byte stores when size * size % 4 == 0. */
int sis_psnr_ssim_tile(void);
int64_t sis_psnr_ssim_workspace_bytes(int batch, int channels, int height, int width);
int sis_psnr_ssim(float* psnr, float* ssim, float* ssim_map, const float* image, const float* target, int batch, int channels,
                  int height, int width, int window, float max_val, int mode, void* workspace, int64_t workspace_bytes, void* stream);
int sis_autoencoder_batch(float* input_image, float* output_image, const uint8_t* images, const int* ids, const float* scale,
                          const int* per_channel, const uint32_t* seed, const int* grey, int64_t n_images, int batch, int size,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * Dataset ground truth: per-image class listing and COCO annotations (csrc/coco_gt.h; the reference's
 * segmentation/evaluation/coco_gt.py:38-92 and create_dataset_for_segmentation.py:151-206).  Integers only, fixed launch
 * sequence, no host sync, the same bytes on every run.  Stated in DESIGN.md §16 and tested against an independent restatement;
 * NOT pinned against OpenCV's findContours or pycocotools.
 * sis_label_regions_workspace_bytes (coco_gt.py:38-92): bytes of device workspace of one call; 0 for a size < 1 or p > 1024.
 * sis_label_regions (coco_gt.py:38-92 extract_rle / determine_classes_in_image / build_annotations_for_image;
 *   create_dataset_for_segmentation.py:151-206 the has_<class> keys and coco_gt.json): label uint8 [batch][p][p][3] (device),
 *   colours uint8 [classes][3] on the HOST (the annotated classes' colours).  Per plane (b, k): M = (label[b] == colours[k]) on
 *   all three bytes; the regions are the 8-connected components of everything the 4-connected background of M cannot reach
 *   from outside the plane (outermost contours, holes filled), in ascending order of root = the smallest y * p + x of the
 *   region.  regions [batch][classes][max_regions][8] int32 = root, x0, y0, w, h (tight box), area (pixels), run_offset,
 *   run_count; a region whose pixels all lie on one horizontal, vertical or diagonal line has run_count 0 and no runs.
 *   runs [batch][classes][max_runs] int32: from run_offset, the region's COCO uncompressed RLE over the whole plane in
 *   column-major order (position x * p + y; the first count is the number of leading zeros; the counts sum to p * p).
 *   has [batch][classes] uint8: 1 iff the plane has a region with runs.  region_count, run_total [batch][classes] int32: the true
 *   numbers, also above the capacities; rows and counts beyond max_regions / max_runs are not stored.  runs == NULL: no counts
 *   are emitted and max_runs is ignored (run_offset, run_count and run_total are still filled); regions == NULL: no rows are
 *   stored and max_regions is ignored.  1 <= classes <= 8, p <= 1024, batch * classes <= 65535; workspace 4-byte aligned.
 *   Declines with an error code and launches nothing otherwise. */
int64_t sis_label_regions_workspace_bytes(int batch, int classes, int p);
int sis_label_regions(uint8_t* has, int32_t* region_count, int32_t* regions, int32_t* run_total, int32_t* runs, const uint8_t* label,
                      const uint8_t* colours, int classes, int batch, int p, int max_regions, int max_runs, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Page visualisation: regions and boxes of a whole assembled page, the colour-coded page, its overlay on the scan, box
 * outlines and cut-out regions (csrc/page_visual.h; the visual half of the reference's
 * segmentation/evaluation/analyze_image_segments.py).  A page is pred float32 [classes][height][width] on the device with
 * 1 <= height, width <= 8192 and 2 <= classes <= 16; every entry declines anything else with an error code and launches
 * nothing.  Integers and bytes only, launch sequence fixed by the arguments, caller's stream, no host sync, the same bytes
 * on every run.  Stated in DESIGN.md §17 and tested against an independent restatement; NOT pinned against OpenCV's
 * findContours / boundingRect / drawContours.
 * sis_page_regions_workspace_bytes (segmentation_utils.py:88-121): bytes of device workspace of one call (9 per pixel and
 *   class); 0 for a shape outside the limits.
 * sis_page_regions (segmentation_utils.py:88-121 get_contours_from_prediction / find_class_contours;
 *   segmentation_visualization.py:35-45 get_bounding_boxes): per plane k other than background_class_id and the classes whose
 *   bit is set in filter_classes: M0 = (pred * 255.0f) >= 1.0f, M = 5x5 closing of M0, regions = the
 *   8-connected components of everything the 4-connected background of M cannot reach from outside the plane (step 4),
 *   twice_area by the 2x2-block rule (step 5).  regions [classes][max_regions][8] int32 = root (the smallest y * width + x of
 *   the region), x0, y0, w, h (tight box), twice_area, kept (twice_area >= 2 * min_contour_area; the reference's default is
 *   10), 0; rows in ascending root order.  The reference lists contours in OpenCV's order, so a region's position in this
 *   table is not the `i` of the reference's file names.  region_count, kept_count [classes] int32: the true numbers, also
 *   above max_regions; rows beyond max_regions are not stored, rows between the count and max_regions are left as they were.
 *   region_labels (may be NULL) [classes][height][width] int32: root + 1 of the pixel's region, 0 outside any region.  Skipped
 *   planes get zero counts and a zero label plane.  regions may be NULL with max_regions == 0.  workspace 4-byte aligned.
 * sis_page_render (visualization/utils.py:9-68 linear_gradient / network_output_to_color_image;
 *   segmentation_visualization.py:22-78 save_overlayed_segmentation_image / draw_bounding_boxes / draw_segmentation): up to
 *   four uint8 [height][width][3] outputs, a NULL pointer skips one.  page uint8 [height][width][page_channels], 1 (grey,
 *   replicated) or 3 channels; colours uint8 [classes][3] on the HOST.  segmented: confidence_table == NULL: the colour of the
 *   FIRST maximal class (all-zero pixels: class 0's).  Otherwise confidence_table is uint8 [classes][100][3] on the device
 *   (entry t = int(255 + (t / 99) * (c - 255))): a pixel whose float32 sum of the non-background planes, in class order, is
 *   > 0 takes table[first maximal class of ALL classes][(int)(100.0 * (double)max) - 1], where index -1 is entry 99 (the
 *   reference's negative list index) and so is an index above 99 (the reference raises); other pixels the background colour.
 *   overlay: the page where segmented equals the background colour on all three bytes, segmented elsewhere.  boxes_on_page /
 *   boxes_on_segmented: the page / segmented with outlines.  First, in (0,255,0) and stroke 3, every row of regions
 *   [classes][max_regions][8] below min(region_count[k], max_regions) with `kept` set, as the box x0, y0, x0 + w, y0 + h with
 *   both ends INCLUSIVE (the reference's BBox(x, y, x + w, y + h) handed to PIL); then, in (255,0,0) and stroke 1, the
 *   `patches` rows x0, y0, x1, y1 (inclusive) of patch_boxes int32 [patches][4] on the device.  A pixel is painted iff it lies
 *   in [x0,x1] x [y0,y1], within the image, and one of x-x0, x1-x, y-y0, y1-y is < stroke: ImageDraw.rectangle's outline
 *   whenever both extents are >= stroke; thinner boxes are filled, where PIL paints outside the box.
 * sis_page_crops (segmentation_visualization.py:81-133 extract_and_save_bounding_boxes / extract_and_save_contours): table
 *   int64 [rows][7] on the device = plane, root, x0, y0, w, h, byte offset; every crop is written as uint8 [h][w][3] at its
 *   offset of out (out_bytes long).  mode 0 (bbox): the page's pixels; mode 1 (contour): the page's pixel where
 *   region_labels == root + 1, (255,255,255) elsewhere -- the filled outer contour, holes and islands included.  A row whose
 *   box leaves the page, whose plane does not exist or whose crop does not fit into out is not written. */
int64_t sis_page_regions_workspace_bytes(int classes, int height, int width);
int sis_page_regions(int32_t* regions, int32_t* region_count, int32_t* kept_count, int32_t* region_labels, const float* pred,
                     int classes, int height, int width, int background_class_id, uint32_t filter_classes, int min_contour_area,
                     int max_regions, void* workspace, int64_t workspace_bytes, void* stream);
int sis_page_render(uint8_t* segmented, uint8_t* overlay, uint8_t* boxes_on_page, uint8_t* boxes_on_segmented, const float* pred,
                    const uint8_t* page, int page_channels, const uint8_t* colours, const uint8_t* confidence_table,
                    const int32_t* regions, const int32_t* region_count, int max_regions, const int32_t* patch_boxes, int patches,
                    int classes, int height, int width, int background_class_id, void* stream);
int sis_page_crops(uint8_t* out, int64_t out_bytes, const int64_t* table, int rows, const uint8_t* page, int page_channels,
                   const int32_t* region_labels, int classes, int height, int width, int mode, void* stream);

/* ------------------------------------------------------------------------------------------
 * GAN training patches cut from document scans (csrc/scan_patches.h).  Pages are uint8 [height][width][3] on the
 * device with 1 <= height, width <= 16384.  Integer arithmetic only, no atomics: two calls give the same bytes, and for 8-bit
 * RGB they are Pillow's bytes.  Every entry declines with an error code and launches nothing outside its stated range.
 * sis_scan_reduce (scripts/create_stylegan_train_dataset.py:45, random_resize: the reduce step inside Image.thumbnail, :167 the
 *   same for --max-size): Pillow's reduce((fx, fy)) over the whole page -> out uint8 [ceil(height / fy)][ceil(width / fx)][3],
 *   every output ((sum + n / 2) * m(n)) >> 24 in uint32 over the n pixels of its box that exist, m(n) = (uint32)(2^32 /
 *   (float)(256 n)) in float arithmetic.  fx, fy >= 1, fx * fy <= 65536.
 * sis_scan_resample_workspace_bytes (scripts/create_stylegan_train_dataset.py:45, random_resize): bytes of device workspace of
 *   one two-pass call: in_h rows of out_w pixels, each row padded to a multiple of 4 bytes.  0 for a side outside 1..16384.
 * sis_scan_resample (scripts/create_stylegan_train_dataset.py:45, random_resize: the resample step inside Image.thumbnail,
 *   :167): the two-pass antialiased resample, horizontal pass first, from host-built tables on the device: per axis coef int32
 *   [out][ksize], first int32 [out] (first source index) and count int32 [out] (taps, <= ksize).  Every output is
 *   clip8((2^21 + sum_j source[first + j] * coef[j]) >> 22) in tap order.  ksize odd and <= 67; ksize 0 with three NULL tables
 *   skips that axis' pass, whose size must then not change (both skipped: a copy).  The horizontal result is uint8 in the
 *   caller's workspace (4-byte aligned, used only when both passes run).  A table entry that would leave the page is clamped.
 * sis_scan_patches (scripts/create_stylegan_train_dataset.py:18-34, crop_patches): n windows of size x size at origins int32
 *   [n][2] = (x, y) on the device -> out uint8 [n][size][size][3], 0 where a window leaves the page (Image.crop's black).
 *   1 <= n <= 65535, 1 <= size <= 4096 (what sis_png_encode_pairs takes); out and origins 4-byte aligned. */
int sis_scan_reduce(uint8_t* out, const uint8_t* page, int height, int width, int fx, int fy, void* stream);
int64_t sis_scan_resample_workspace_bytes(int in_h, int in_w, int out_h, int out_w);
int sis_scan_resample(uint8_t* out, const uint8_t* page, int in_h, int in_w, int out_h, int out_w, const int32_t* coef_x,
                      const int32_t* first_x, const int32_t* count_x, int ksize_x, const int32_t* coef_y, const int32_t* first_y,
                      const int32_t* count_y, int ksize_y, void* workspace, int64_t workspace_bytes, void* stream);
int sis_scan_patches(uint8_t* out, const uint8_t* page, const int32_t* origins, int n, int size, int height, int width, void* stream);

/* Scanner-margin removal (csrc/scan_margin.h): the content box of an analysis image uint8 [height][width][3] on
 * the device, 3 <= height, width <= 4096.  The reference calls OpenCV's blur, Canny, dilate, erode, findContours and
 * boundingRect; §20 states that sequence in integers from OpenCV's documented behaviour -- nothing was compared with OpenCV.
 * Integer arithmetic, sums, minima and maxima only: two calls give the same bytes.  Fixed launch sequence on `stream`, nothing
 * read back.
 * sis_scan_content_box_workspace_bytes (scripts/create_stylegan_train_dataset.py:49, get_content_box): bytes of device workspace
 *   of one call; 0 for a side outside 3..4096.
 * sis_scan_content_box (scripts/create_stylegan_train_dataset.py:49-111, get_content_box with edge_detect=True; :114-138 scale
 *   the box and crop on the host): 3x3 box blur, Sobel gradients of the strongest channel, non-maximum suppression, hysteresis
 *   between `low` and `high` (20 and 150 in the tool), closing with the 3x3 cross, one contour per 8-connected component of
 *   the result E and per hole of E, then the reference's "largest gap of the sorted box areas" cut.
 *   box int32 [4] = x0, y0, x1, y1 with exclusive ends (the whole image unless info[4] is 0);
 *   info int32 [8] = contours, outer contours, largest box area, contours kept, decision (0 cut, 1 at most one contour, 2 largest
 *     area below 0.6 of the image), T (kept: area >= T; 0 unless the decision is 0), pixels of E, 0;
 *   edges uint8 [height][width] = E as 0 / 255, or NULL;
 *   contours int32 [max_contours][6] = kind (0 outer, 1 hole), root (smallest y * width + x), x0, y0, w, h: outers by ascending
 *     root, then holes by ascending root; rows from min(count, max_contours) on are not written; NULL: no table.  Neither box
 *     nor info depends on max_contours.
 *   box, info, contours and workspace 4-byte aligned.  Declines with an error code and launches nothing: a null pointer (box,
 *   info, page, workspace), an unaligned one, a workspace below sis_scan_content_box_workspace_bytes, a side outside 3..4096,
 *   low < 0, high < low, max_contours < 0. */
int64_t sis_scan_content_box_workspace_bytes(int height, int width);
int sis_scan_content_box(int32_t* box, int32_t* info, uint8_t* edges, int32_t* contours, int max_contours, const uint8_t* page,
                         int height, int width, int low, int high, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Validation pass of the segmenters (csrc/seg_eval.h).  The reference leaves its evaluator hook empty for them
 * (training_builder/base_train_builder.py:64-65); the scores are those of evaluation/segmentation_metric_calculation.py:71-94
 * (confusion matrix) and networks/trans_u_net/utils.py:7-42 (Dice sums), the cross entropy is nn.CrossEntropyLoss's.
 * sis_seg_eval: logits [batch][classes][h][w] (SIS_F32, or SIS_BF16 when h == out_h and w == out_w), labels int64
 *   [batch][out_h][out_w]; 2 <= classes <= 16, 1 <= h <= out_h, 1 <= w <= out_w, out_h * out_w <= 2^30,
 *   batch * out_h * out_w <= 2^39, no alignment rule.
 *   Per output pixel the values v[c] are the stored elements widened to float (h == out_h and w == out_w) or the align-corners
 *   bilinear values with the scales and the function of sis_upsample_ce_fwd; the prediction is the first maximal class
 *   (torch.argmax for finite logits; a NaN never wins, and non-finite logits make `sums` NaN).
 *   ACCUMULATES (the caller zeroes both once per validation run) into
 *     counts int64 [classes * classes + 2]: matrix[label][prediction] as sis_confusion_matrix lays it out, then `counted` (labels
 *       in [0, classes)), then `ignored` (every other label: in no cell, not in the cross entropy);
 *     sums double [1 + 3 * classes]: sum of -log softmax(v)[label] over the counted pixels, then per class c at 1 + 3c:
 *       I_c = sum p_c [label == c], P_c = sum p_c^2, T_c = sum [label == c] over ALL pixels (an ignored label is an all-zero one-hot
 *       row, sis_ce_dice_fwd's rule).
 *   counts are exact and independent of any order; sums are added in a fixed order (two calls give the same bits).
 *   workspace: sis_seg_eval_workspace_bytes(batch, classes, out_h, out_w) bytes, 8-byte aligned (0 for sizes out of range).
 *   Everything else declines with an error code and launches nothing. */
int64_t sis_seg_eval_workspace_bytes(int batch, int classes, int out_h, int out_w);
int sis_seg_eval(int64_t* counts, double* sums, void* workspace, const void* logits, int dtype, const int64_t* labels, int batch,
                 int classes, int h, int w, int out_h, int out_w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIS_HIP_H */
