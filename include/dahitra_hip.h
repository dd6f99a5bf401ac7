/* dahitra_hip.h -- C ABI of libdahitra_hip.so, the MI355X (gfx950) kernel library behind
 * dahitra_amd's drop-in replacement of the DAHiTra change-detection hot path.
 *
 * The reference (nka77/DAHiTra) owns no native code: its hot path issues stock torch operators.
 * Each entry point below therefore cites the reference call site(s) whose torch operator it
 * replaces (paths relative to the reference root).  A maintainer binds these with ctypes exactly as
 * dahitra_amd/_lib.py does.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; dh_last_error() gives the message
 *   - all pointers are DEVICE pointers (hipMalloc / torch CUDA tensors) unless stated otherwise;
 *     buffers are caller-allocated, no ownership is transferred, nothing is allocated inside
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); calls are async
 *   - `dtype`: DH_F32 (parity mode, exact-fp32 MFMA) or DH_BF16 (throughput mode, bf16 MFMA with
 *     fp32 accumulation) selects the ACTIVATION type "T"; parameters, statistics, optimizer state
 *     and weight gradients are always fp32
 *   - activations are NHWC: [N][H][W][C], C contiguous; "rows x C" tensors are the same thing
 *   - `*_workspace_size` twins return the bytes of scratch the call needs (contents undefined)
 */
#ifndef DAHITRA_HIP_H
#define DAHITRA_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define DH_F32 0
#define DH_BF16 1
#define DH_ACT_NONE 0
#define DH_ACT_RELU 1
#define DH_ACT_GELU 2

int dh_abi_version(void);
const char* dh_last_error(void);
void dh_set_error(const char* msg);

/* ---- convolution / linear on the matrix cores ------------------------------------------------
 * replaces F.conv2d / nn.Linear at: models/resnet.py:24-32,150 (trunk), models/networks.py:215
 * (conv_pred), models/help_funcs.py:7-15 (TwoLayerConv2d), :52-63 (FeedForward), :86-88,111
 * (to_q/k/v/out), models/networks.py:1178-1185,1196-1199,1235-1243 (squeeze / decode / top-down
 * convs); with transposed+flipped weights it is also their input gradient (autograd
 * convolution_backward), and with w_image_stride != 0 the per-image attention products
 * (help_funcs.py:92,109) in re-associated form.
 * y[n,oy,ox,co] = act( sum_{kh,kw,ci} x[n, oy*stride-pad+kh, ox*stride-pad+kw, ci] * w[kh*ks+kw][co][ci]
 *                      + bias[co] + residual[n,oy,ox,co] )
 * w_packed: [ks*ks][CoutPad][Cin] T (dh_pack_weight).  Cin*sizeof(T) must be a multiple of 64.
 * y_preact (optional): receives the value before `act`.  stats_partial (optional):
 * [2][CoutPad][dh_conv2d_fwd_num_tiles(dtype,N,OH,OW,Cin,ks,stride)] fp32 per-tile (sum, sum of squares) of y for BatchNorm
 * (channel-major: the per-channel combine reads contiguous runs).
 * npix_valid > 0: treat each image as a row list with that many valid rows (H*W >= npix_valid). */
int dh_conv2d_fwd(int dtype, const void* x, const void* w_packed, void* y, const float* bias,
                  const void* residual, float* stats_partial, int N, int H, int W, int Cin, int OH, int OW,
                  int Cout, int CoutPad, int ks, int stride, int pad, int act, int npix_valid,
                  long w_image_stride, void* y_preact, int dilation, const void* gate_out, const void* gate_y,
                  const float* gate_mean, const float* gate_invstd, int gate_groups, const float* in_scale,
                  const float* in_shift, int in_groups, int phase_mode, const void* w_frag, void* stream);
/* w_frag (optional; bf16 3x3 only): the SAME weights in fragment order [CoutPad / 16][Cin / 32][9][64][8] (what
 * dh_pack_weights_multi writes for jobs with dtype | 0x200): lane l of a wavefront finds the 8 reduction channels
 * 32 c + 8 (l >> 4) .. of output channel 16 r + (l & 15) at [r][c][tap][l], i.e. one MFMA weight fragment is 1 KiB
 * contiguous.  Read only where the register-resident-weights kernel runs (dh_conv_wreg_mode); NULL = it loads w_packed. */
/* phase_mode (0 = off; ks = 2, pad = 1 only): conv3x3(nearest-upsample-x2(x)) -- models/networks.py:251-256, upsamplex2 +
 * conv_pred -- as four 2x2 convolutions on x, one per output parity, weights from dh_pack_phase_weights (2.25x fewer
 * FLOPs, the upsampled tensor is never written).  1: forward, logical Cout = 4 * 32, y is the [N][2 OH][2 OW][32] output
 * (depth-to-space store), bias tiled 4 x.  2: data gradient, x is the [N][2 H][2 W][32] gradient (space-to-depth gather),
 * logical Cin = 4 * 32, y = [N][H][W][Cout]. */
/* in_scale / in_shift ([in_groups][Cin] fp32, NULL = off; 3x3 stride-1 convolutions): BatchNorm-apply + ReLU on LOAD.  x is
 * then the PRE-normalisation output of the previous convolution and the kernel consumes relu(x * in_scale[g][ci] +
 * in_shift[g][ci]), g = n / (N / in_groups); zero padding applies to that post-activation tensor.  Replaces the separate
 * F.batch_norm + ReLU pass between two convolutions (models/resnet.py:60-65, models/help_funcs.py:11-13). */
/* gate_* (all NULL / 0 = off): BatchNorm-backward gating of a data-gradient launch.  gate_y / gate_out are the
 * pre-normalisation input and the post-ReLU output (NULL: no ReLU) of the BN layer whose output gradient this launch
 * produces ([N][OH][OW][Cout] like y), gate_mean / gate_invstd its batch statistics [gate_groups][Cout].  The
 * epilogue then stores g = dout * (gate_out > 0) and writes stats_partial[tile] = (sum g, sum g * xhat), which
 * dh_bn_bwd_from_partials consumes (replaces the reduction pass of dh_bn_bwd; torch autograd's native_batch_norm
 * backward + threshold_backward, called from models/resnet.py:58-73 via loss.backward()). */
int dh_conv2d_fwd_num_tiles(int dtype, int N, int OH, int OW, int Cin, int ks, int stride);   /* dtype: of the launch that fills the buffer */
/* Host only (no launch, no device, no tensor is read): the launch plan of a forward / data-gradient convolution call under the
 * thread's current dh_set_f32_mma_mode and dh_conv_wreg_mode, on a device of `cus` compute units.  entry: 0 dh_conv2d_fwd (every
 * scalar argument as there), 1 dh_conv3x3_head_fwd (dtype, N, H, W, Cin, Cout, in_groups), 2 dh_conv3x3_split_fwd (N, H, W, Cin, Cout),
 * 3 dh_conv3x3_up4_fwd (N, H, W, act), 4 dh_conv3x3_dgrad_up4 (dtype, N, H, W, Cin = K), 5 dh_conv3x3_res_bits_fwd (dtype, N, H, W, Cin,
 * Cout, CoutPad; flag 32); the other arguments are ignored.  flags: which
 * of the tensors the decision depends on are given -- 1 residual, 2 stats_partial, 4 y_preact, 8 the gate_* tensors, 16 in_scale /
 * in_shift, 32 w_frag, 64 x_split_bytes, 128 y_split_bytes.
 * out[30], unused fields 0:
 *   [0]      family: 0 tap kernel bf16, 1 exact fp32, 2 / 3 / 4 its split forms bf16x3 / bf16x6 / fp16x3, 5 the 1x1 GEMM, 6 / 7 / 8 the
 *            weights-resident stream at 64 / 128 / 256 input channels, 9 its 32 -> 32 form, 10 that with the bilinear x4 on load
 *   [1..9]   tap kernel: KS, STRIDE, NT, RW, DIL, PF, FAST, INBN, INUP4
 *   [10..12] GEMM: BN, BM, XDEEP
 *   [13..21] stream: NCH, D, PFD, WPS, INBN, RES, RELU (those its kernel has), workgroups per channel block J, channel blocks
 *   [22..25] grid x, grid y, threads, dynamic LDS bytes
 *   [26..28] tilesX, tilesY, rows per wavefront rw (tile height 4 rw)
 *   [29]     rows of stats_partial the kernel indexes (= dh_conv2d_fwd_num_tiles of the launch)
 * Returns non-zero, with dh_last_error set, where the call itself would be refused. */
int dh_conv2d_fwd_describe(int entry, int dtype, int N, int H, int W, int Cin, int OH, int OW, int Cout, int CoutPad, int ks, int stride,
                           int pad, int act, int npix_valid, long w_image_stride, int dilation, int gate_groups, int in_groups,
                           int phase_mode, int flags, int cus, int* out);
/* bf16 3x3 / stride-1 / pad-1 convolutions with 64 / 128 / 256 input channels and Cout % 64 == 0 on whole 8x16 tiles run,
 * inside dh_conv2d_fwd, on the register-resident-weights kernel (csrc/conv_wreg.hip: persistent workgroups, the weights of
 * a wavefront's output channels stay in its registers, only the input halo is staged) -- same products in the same order as
 * the tap-oriented kernel, i.e. bit-identical outputs.  mode -1 (default): on the shapes where it is the faster kernel; 0: never
 * (everything through the tap-oriented kernel); 1: wherever it can run.  Returns the previous mode.  Same reference call sites as dh_conv2d_fwd
 * (models/resnet.py:24-73: BasicBlock conv1 / conv2 and their input gradients). */
int dh_conv_wreg_mode(int mode);
/* 3x3 / stride-1 / pad-1 convolution + MASKED residual: y = conv(x) + (bit ? residual : 0), the bits taken from res_bits in the
 * layout of dh_bn_apply_bits's relu_bits for the [N][H][W][Cout] residual (byte i = its 16-byte piece i, bit j = element j).  It is
 * the data gradient of conv1 of a residual block without a downsample (models/resnet.py:56-71) fed the gradient of the block's
 * output and the ReLU mask of that output, so that the masked copy `dres` of dh_bn_bwd* need not be written: bit-identical to
 * dh_conv2d_fwd with that copy as residual.  No bias, activation or statistics; w_frag optional (bf16).  Served by the
 * weights-resident stream at 64 / 128 / 256 input channels and by the tap kernel; dh_conv3x3_res_bits_supported returns 1
 * where one of them takes the shape, 0 where the call would be refused (the 32 -> 32 stream form, which has no mask path,
 * among them): callers keep the masked copy there.  The mask is never silently ignored. */
int dh_conv3x3_res_bits_supported(int dtype, int N, int H, int W, int Cin, int Cout, int CoutPad, int has_frag);
int dh_conv3x3_res_bits_fwd(int dtype, const void* x, const void* w_packed, const void* w_frag, const void* residual,
                            const unsigned char* res_bits, void* y, int N, int H, int W, int Cin, int Cout, int CoutPad, void* stream);
/* How the matrix products of DH_F32 launches are computed (dh_conv2d_fwd, dh_conv3x3_head_fwd, dh_conv2d_wgrad* and the
 * kernels that call them), per host thread, read when a launch is issued:
 *   0 (default)  exact fp32: v_mfma_f32_16x16x4_f32;
 *   1            split-bf16, two planes: while an operand tile is staged every fp32 element x becomes hi = bf16(x),
 *                lo = bf16(x - hi) and a product is ah*bh + al*bh + ah*bl on v_mfma_f32_16x16x32_bf16 with fp32 accumulation
 *                (unit roundoff 2^-17 against fp32's 2^-24; 3/16 of the exact form's matrix-core cycles);
 *   2            split-bf16, three planes (x = p0 + p1 + p2, 8 mantissa bits each): the six products a_i*b_j, i + j < 3
 *                (unit roundoff 2^-23; 6/16 of the cycles).  Convolution / linear launches only: a weight-gradient launch
 *                issued in mode 2 or 3 runs form 1.
 *   3            split-fp16, two planes (hi = fp16(x), lo = fp16(x - hi), 11 mantissa bits each): three products on
 *                v_mfma_f32_16x16x32_f16, ~2^-21 at the cycles of form 1 -- for operands inside fp16's RANGE: |x| < 65504, and
 *                |w| < 255 for the weights, which are staged times 2^8 (exact; undone on the accumulators) so that weights of
 *                size 1e-2 keep a normal lo plane.  The forward's form (activations are O(1)); not for gradients.
 * Tensors, accumulators, statistics, everything that is not a matrix product, launches with Cin % 32 != 0 and launches
 * whose staging planes would not fit the LDS are unchanged, so DH_F32 buffers, packs and workspaces are interchangeable
 * between the modes.  The reference computes these products in fp32 (models/networks.py:358-392,
 * models/help_funcs.py:66-114, loss.backward()): compute_dtype="bf16x3" (form 3 in the forward, form 1 in the backward)
 * is the parity mode's fast form. */
int dh_set_f32_mma_mode(int mode);
int dh_get_f32_mma_mode(void);
/* The backward of |a - b| -> nn.Upsample(4, 'bilinear') -> conv3x3 (models/networks.py:383-389; autograd's
 * upsample_bilinear2d_backward + convolution_backward input gradient) WITHOUT the fine-grid gradient tensor: the data-gradient
 * launch of the 3x3 convolution (dy [N][H][W][K] bf16, w_packed = its data-gradient pack [9][32][K]) reduces each 8x16 tile
 * to the 4 x 6 coarse pixels it interpolates from and writes fp32 partials (dh_conv3x3_dgrad_up4_partial_floats of them);
 * dh_absdiff_up4_combine sums the <= 4 tiles of every coarse pixel of the [N][H/4][W/4][32] maps a, b and applies
 * sign(a - b): da, db.  bf16 mode; H % 8 == 0, W % 16 == 0. */
long dh_conv3x3_dgrad_up4_partial_floats(int N, int H, int W);
int dh_conv3x3_dgrad_up4(int dtype, const void* dy, const void* w_packed, int N, int H, int W, int K, float* partial, void* stream);
int dh_absdiff_up4_combine(const float* partial, const void* a, const void* b, void* da, void* db, int N, int H, int W, void* stream);
/* The class head -- classifier[-1]: nn.Conv2d(32, n_class, 3, padding 1) (models/networks.py:201-204, 1121-1129) -- with the
 * fp32 NCHW logits [N][Cout][H][W] (the reference's output layout) written by the convolution itself: no NHWC logits tensor,
 * no layout pass.  w_packed: dh_pack_weight with OPad = 16; in_scale / in_shift (optional): BatchNorm-apply + ReLU on load. */
int dh_conv3x3_head_fwd(int dtype, const void* x, const void* w_packed, const float* bias, int N, int H, int W, int Cin,
                        int Cout, const float* in_scale, const float* in_shift, int in_groups, float* logits_nchw, void* stream);

/* weight gradient (autograd convolution_backward / mm for nn.Linear): groups == 1 writes the
 * torch OIHW layout [Cout_real][Cin][ks][ks]; groups == N (ks == 1) one [Cout][Cin] per image. */
int dh_conv2d_wgrad(int dtype, const void* x, const void* dy, float* dw_oihw, int accumulate, int N, int H,
                    int W, int Cin, int OH, int OW, int Cout, int ks, int stride, int pad, int groups,
                    int npix_valid, int use_tr, int Cout_real, int cin_pitch, int dilation, void* workspace, void* stream);
/* > 0: a plain bf16 1x1 / stride-1 weight gradient of this shape runs in the block form (wgrad1x1_kernel: a 256 x 128 / 128 x 256 /
 * 256 x 64 / 64 x 256 block of dW per workgroup over flat pixels, all blocks of a pixel split on one XCD); the value = blocks per
 * split.  0: the 64 x 64-slab kernel (too few pixels to fill the chip with fat blocks, a small layer, or a launch that goes
 * direct: split-K 1 -- a handful of pixel tiles -- writes dW itself, whatever the channel counts). */
int dh_conv2d_wgrad_1x1_blocks(int N, int H, int W, int Cin, int Cout);
/* Host only (no launch, no device): the launch plan of a dh_conv2d_wgrad / _partial call with these arguments, of dh_conv2d_wgrad_bn_in
 * (has_in_scale, in_groups), of dh_conv2d_wgrad_split (split_input: cin_pitch is Cin / 2) and, with ks == 2, of
 * dh_conv2d_wgrad_phase(dtype, N, H, W, Cin, use_tr); batch_open: as a deferred call between dh_wgrad_batch_begin and _end.
 * out[12] = family (0 wgrad1x1_kernel, 1 the wave-specialised 3x3 kernel, 2 / 3 recorded into the wave-specialised / the 32-wide
 * job-table launch, 4 conv_wgrad_kernel, 5 its 2x2 phase form), co tile, ci channels per workgroup, ci wave groups, ci tiles,
 * split-K factor, direct, grid x, y, z, threads, dynamic LDS bytes.  Returns non-zero where the launch itself would be refused. */
int dh_conv2d_wgrad_describe(int dtype, int accumulate, int N, int H, int W, int Cin, int OH, int OW, int Cout, int ks, int stride,
                             int pad, int groups, int npix_valid, int use_tr, int Cout_real, int cin_pitch, int dilation,
                             int in_groups, int has_in_scale, int split_input, int batch_open, int* out);
long dh_conv2d_wgrad_workspace_size(int N, int OH, int OW, int Cin, int Cout, int ks, int groups);
/* The weight gradient with its split-K reduce deferred: only the partial slabs are written into `workspace` (which
 * must stay alive until the batched reduce) and *splitk_out receives their count (0: the single-slab 1x1 case wrote
 * dW directly).  dh_wgrad_reduce_multi then sums every deferred layer of a backward pass in one launch.  jobs_dev:
 * njobs records {const float* part; float* dw; int splitk, taps, Oslab, O, I, accumulate, first_block, nblocks;}
 * (dh_wgrad_reduce_job_size() bytes each) sorted by first_block, nblocks = ceil(O*I*taps / dh_wgrad_reduce_outputs_per_block(I)), Oslab = the Cout the
 * kernel was launched with, O = Cout_real.  (autograd convolution_backward's weight term, as dh_conv2d_wgrad.) */
int dh_conv2d_wgrad_partial(int dtype, const void* x, const void* dy, float* dw_oihw, int accumulate, int N, int H,
                            int W, int Cin, int OH, int OW, int Cout, int ks, int stride, int pad, int groups,
                            int npix_valid, int use_tr, int Cout_real, int cin_pitch, int dilation, void* workspace,
                            int* splitk_out, void* stream);
/* dh_conv2d_wgrad (splitk_out == NULL) / dh_conv2d_wgrad_partial (splitk_out != NULL) against
 * relu(x * in_scale[g][ci] + in_shift[g][ci]) computed on load (see dh_conv2d_fwd's in_scale) */
int dh_conv2d_wgrad_bn_in(int dtype, const void* x, const void* dy, float* dw_oihw, int accumulate, int N, int H, int W,
                          int Cin, int OH, int OW, int Cout, int ks, int stride, int pad, int use_tr, int Cout_real,
                          int dilation, const float* in_scale, const float* in_shift, int in_groups, void* workspace,
                          int* splitk_out, void* stream);
/* Channel concatenation without the concatenated tensor (bf16, 3x3 / stride 1 / pad 1): models/networks.py:1344,
 * conv_layer2_0(torch.cat([a_128, b_128], 1)) -- here the two temporal streams are the two halves of ONE [2N]-image tensor.
 *   dh_conv3x3_split_fwd   x_split_bytes != 0: the input is cat([A, B], channel) of two [N][H][W][Cin / 2] tensors, A at x, B
 *                          at x + x_split_bytes; y_split_bytes != 0: the output's channel halves go to two
 *                          [N][H][W][Cout / 2] tensors, y and y + y_split_bytes (the data gradient of such a layer, with
 *                          w_packed / w_frag its data-gradient packs).  No bias / residual / activation; stats_partial as
 *                          dh_conv2d_fwd (rows = dh_conv2d_fwd_num_tiles).  w_frag (fragment-order pack) is required.
 *   dh_conv2d_wgrad_split  dh_conv2d_wgrad_partial against such an input (joins an open weight-gradient batch).
 *   dh_conv3x3_split_supported  1 when all three run for a layer Cin -> Cout on N x H x W pixels; callers otherwise
 *                          materialise the concatenation with dh_copy_channels.
 * (replaces torch.cat + F.conv2d and their autograd terms; the copies were 4 x 134 MB per step at batch 32) */
int dh_conv3x3_split_supported(int N, int H, int W, int Cin, int Cout);
int dh_conv3x3_split_fwd(const void* x, long x_split_bytes, const void* w_packed, const void* w_frag, void* y, long y_split_bytes,
                         float* stats_partial, int N, int H, int W, int Cin, int Cout, void* stream);
int dh_conv2d_wgrad_split(const void* x, long x_split_bytes, const void* dy, float* dw_oihw, int accumulate, int N, int H, int W,
                          int Cin, int Cout, void* workspace, int* splitk_out, void* stream);
/* classifier.0 on nn.Upsample(4, 'bilinear')(abs(x1 - x2)) WITHOUT that map (models/networks.py:383-389, models/help_funcs.py:9;
 * bf16): a, b [N][H / 4][W / 4][32] are the two streams' decoder outputs, H x W the fine size (multiples of 4).
 *   dh_conv3x3_up4_fwd   y [N][H][W][32] = act(conv3x3(upsample4(|a - b|)) + bias), act 0 / ReLU; w_packed [9][32][32]
 *                        (dh_pack_weight forward form); stats_partial as dh_conv2d_fwd, dh_conv2d_fwd_num_tiles(DH_DTYPE_BF16, N, H, W, 32, 3, 1)
 *                        rows.  The 8 x 16-pixel tile's haloed input is interpolated from its 4 x 6 coarse footprint with the
 *                        terms and order of dh_absdiff_upsample4_fwd: equal to dh_conv2d_fwd on that kernel's output, bit for bit.
 * (the data gradient through the upsample is dh_conv3x3_dgrad_up4; the weight gradient still reads the materialised map:
 * F.interpolate + abs + F.conv2d.  Measured slower than dh_absdiff_upsample4_fwd + the register-resident-weights kernel -- 121
 * against 32 + 76 us at batch 32 -- and therefore not the default path) */
int dh_conv3x3_up4_fwd(const void* a, const void* b, const void* w_packed, const float* bias, int act, void* y, float* stats_partial,
                       int N, int H, int W, void* stream);
/* Batched weight gradients: the 3x3 stride-1 bf16 layers of one backward pass as ONE launch per kernel family (the
 * wave-specialised 64co x 64ci form: Cin and Cout multiples of 64; the 32-wide output tile: 16 < Cout <= 32).  Between dh_wgrad_batch_begin() and dh_wgrad_batch_end(), dh_conv2d_wgrad_partial /
 * dh_conv2d_wgrad_bn_in (with splitk_out) only RECORD an eligible layer -- *splitk_out is its in-batch slice count, smaller
 * than a launch of its own would take -- and every other layer launches as before; dh_wgrad_batch_launch(stream) issues what
 * has been recorded (x / dy / scale / shift / workspace must stay alive and unchanged until then; a 17th layer issues the
 * first 16), dh_wgrad_batch_pending() counts the recorded layers.  The reduce (dh_wgrad_reduce_multi) follows as before.
 * The state is per host thread.  Replaces nothing in the reference (autograd computes each layer's gradient on its own):
 * it exists because a launch per layer needs 256 workgroups each to fill the chip. */
int dh_wgrad_batch_begin(void);
int dh_wgrad_batch_pending(void);
int dh_wgrad_batch_launch(void* stream);
int dh_wgrad_batch_end(void* stream);
int dh_wgrad_batch_abort(void);        /* closes the batch without launching (an aborted pass) */
int dh_wgrad_reduce_multi(const void* jobs_dev, int njobs, int total_blocks, void* stream);
/* ---- the 2x2 phase form of conv3x3(nearest-upsample-x2(x)) with 32 output channels (dh_conv2d_fwd's phase_mode) ----
 * dh_pack_phase_weights: OIHW fp32 [32][Cin][3][3] (+ bias [32]) -> fwd [4 taps][4 * 32][Cin] T, data-gradient form
 * [4 taps][Cin][4 * 32] T, bias4 [128] fp32; W_ab[t][u] = sum of the 3x3 taps that read the same source pixel.
 * dh_conv2d_wgrad_phase: per-phase weight gradients, x [N][H][W][Cin], dy [N][2H][2W][32] -> partial slabs in `workspace`
 * ([4 phases][splitk][4 taps][32][Cin] fp32, *splitk_out slabs per phase; reduce each phase with dh_wgrad_reduce_multi /
 * the returned layout into dwab [4][32][Cin][2][2]).  dh_phase_wgrad_combine: dw_oihw [32][Cin][3][3] (+)= the sums of the
 * phase gradients that share a 3x3 tap.  (autograd of F.interpolate(nearest) + conv2d's weight.) */
int dh_pack_phase_weights(int dtype, const float* w_oihw, const float* bias, int Cin, void* fwd, void* dgrad, float* bias4,
                          void* stream);
long dh_conv2d_wgrad_phase_workspace_size(int N, int H, int W, int Cin);
int dh_conv2d_wgrad_phase(int dtype, const void* x, const void* dy, int N, int H, int W, int Cin, int use_tr, void* workspace,
                          int* splitk_out, void* stream);
int dh_phase_wgrad_combine(const float* dwab, float* dw_oihw, int Cin, int accumulate, void* stream);
/* Data gradient of a 3x3 / stride-2 / pad-1 convolution (models/resnet.py:24-27 with stride 2; autograd convolution_backward)
 * WITHOUT the zero-inserted gradient: dh_conv2d_fwd(phase_mode = 1, ks = 2, x = dY [N][OH][OW][Co], logical Cout = 4 * Ci,
 * y = dX [N][2 OH][2 OW][Ci], residual = coarse [N][OH][OW][Ci] gradient of the 1x1 stride-2 shortcut or NULL) over the
 * weights packed here: [4 taps][4 * Ci][Co] T from OIHW fp32 [Co][Ci][3][3]; Ci = 32 or 64. */
int dh_pack_s2_dgrad_phase_weights(int dtype, const float* w_oihw, int Co, int Ci, void* out, void* stream);
int dh_wgrad_reduce_job_size(void);
int dh_wgrad_reduce_outputs_per_block(int Cin);
int dh_conv2d_wgrad_splitk(int N, int OH, int OW, int Cin, int Cout, int ks, int groups);

/* OIHW fp32 master weight -> kernel layouts: fwd [ks*ks][OPad][I] T and (optional) the data-gradient
 * form [ks*ks flipped][IPad][max(O, dgrad_inner)] T.  out_scale (optional, [O]) multiplies the forward form per
 * output channel: eval-mode BatchNorm folded into the convolution (its shift then goes in as `bias`). */
int dh_pack_weight(int dtype, const float* w_oihw, const float* out_scale, int O, int I, int ks, int OPad, void* fwd, int IPad,
                   int dgrad_inner, void* dgrad, void* stream);
/* every weight of a net in one launch.  jobs_dev: njobs records {const float* w; void* fwd; void* dgrad; int O, I, KS,
 * OPad, IPad, OK, dtype (| 0x200: fragment-order destinations, see dh_conv2d_fwd), first_block, nblocks;} (dh_pack_job_size() bytes each) in device memory, sorted by
 * first_block; record k is served by workgroups [first_block, first_block + nblocks). */
int dh_pack_weights_multi(const void* jobs_dev, int njobs, int total_blocks, void* stream);
int dh_pack_job_size(void);
/* z[n,2y,2x,c] = dy[n,y,x,c] (zero elsewhere): stride-2 data gradients as stride-1 convolutions */
int dh_zero_insert2(int dtype, const void* dy, void* z, int N, int OH, int OW, int H, int W, int C, void* stream);
/* x [N][H][W][C] (+)= coarse [N][(H+1)/2][(W+1)/2][C] at the even-even positions: the data gradient of a 1x1 stride-2 convolution
 * (the shortcut of a stride-2 Bottleneck, models/resnet.py:106-118) computed on its own coarse grid and added where it lives,
 * instead of zero insertion + a 1x1 convolution on the fine grid. */
int dh_add_coarse(int dtype, void* x, const void* coarse, int N, int OH, int OW, int H, int W, int C, void* stream);

/* stem nn.Conv2d(3,64,7,2,3) (models/resnet.py:150) as a 4x4/stride-1 conv on a space-to-depth image */
int dh_stem_space_to_depth(int dtype, const float* x_nchw, void* y, int N, int H, int W, int CP, void* stream);
int dh_stem_pack_weight(int dtype, const float* w_oihw, const float* out_scale, void* packed, int O, int CP, void* stream);
int dh_stem_unpack_grad(const float* dw2, float* dw_oihw, int O, int CP, int accumulate, void* stream);
/* The same stem (models/resnet.py:150, applied to both images by forward_single, models/networks.py:215-224) as one bf16
 * kernel on the NCHW fp32 images themselves: images [0, B) from xa, [B, N) from xb (xb may be NULL when B == N).
 * w_oihw fp32 [64][3][7][7]; out_scale / bias (optional, per cout): eval-mode BatchNorm folded in; relu: 0 / 1.
 * y: bf16 NHWC [N][H/2][W/2][64].  stats (optional, raw convolution only): [2][64][dh_stem7_fwd_num_slots] sum / sum of
 * squares per workgroup for dh_bn_finalize (ntiles = slots); a workgroup stays inside one of the `groups` equal image
 * ranges, slots of group 0 first.  xs16 (optional): the space-to-depth image [N][H/2][W/2][16] bf16 (channel (ry*2+rx)*3 + c, 4 zero
 * channels) the weight gradient reads (dh_conv2d_wgrad with ks = 4, Cin = 16, pitch 16 + dh_stem_unpack_grad). */
int dh_stem7_fwd(const float* xa, const float* xb, int B, int N, int H, int W, const float* w_oihw, const float* out_scale,
                 const float* bias, int relu, void* y, float* stats, int groups, void* xs16, void* stream);
int dh_stem7_fwd_num_slots(int N, int H, int W, int groups);
/* Backward of the stem's tail maxpool(relu(bn1(conv1(x)))) (models/resnet.py:150-153,198-201) without a BatchNorm pass of its
 * own (bf16).  dh_stem_pool_bn_bwd: max-pool backward from the saved arg-max, the ReLU mask recomputed from y
 * (y * mask_scale + mask_shift > 0) and the BatchNorm-backward sums in ONE pass over the 128x128 map: d [N][H][W][C] = masked
 * gradient of the BatchNorm output, dgamma / dbeta (+)=, coef [groups][3][C] = per-channel (A, B, C) of
 * dconv = A * d + B * y + C.  dh_stem_wgrad_bn: the weight gradient against the space-to-depth image xs16 with that
 * expression applied while d and y are loaded; dw2 [64][16][4][4] is assigned (then dh_stem_unpack_grad). */
long dh_stem_pool_bn_bwd_workspace_size(int C, int groups);
int dh_stem_pool_bn_bwd(const unsigned char* argmax, const void* dpool, const void* y, const float* mask_scale,
                        const float* mask_shift, const float* mean, const float* invstd, const float* gamma, int N, int H, int W,
                        int C, int groups, void* d, float* coef, float* dgamma, float* dbeta, int accumulate, void* workspace,
                        void* stream);
/* dh_stem_pool_bn_bwd with a second gradient of the same pre-pool activation, extra [N][H][W][C] (or NULL), added before the
 * mask: the hierarchical model reads the stem's output twice (models/networks.py:1118-1128 max-pool -> layer1, :1344
 * cat([a_128, b_128]) -> conv_layer2_0), so the add, the max-pool backward and both BatchNorm-backward passes are this one. */
int dh_stem_pool_bn_bwd_plus(const unsigned char* argmax, const void* dpool, const void* extra, const void* y,
                             const float* mask_scale, const float* mask_shift, const float* mean, const float* invstd,
                             const float* gamma, int N, int H, int W, int C, int groups, void* d, float* coef, float* dgamma,
                             float* dbeta, int accumulate, void* workspace, void* stream);
int dh_stem_wgrad_bn(const void* xs16, const void* d, const void* y, const float* coef, int groups, int N, int OH, int OW,
                     float* dw2, int use_tr, void* workspace, void* stream);

/* ---- BatchNorm2d (models/resnet.py:152,40-44; help_funcs.py:11) and LayerNorm(32) (help_funcs.py:34-49)
 * groups (statistics groups of equal size, image order): 1, 2 or 4 in dh_bn_finalize / dh_bn_apply* / dh_bn_bwd* alike */
int dh_bn_finalize(const float* partial, int ntiles, int CP, int C, int groups, double count, const float* gamma,
                   const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                   float* mean, float* invstd, float* scale, float* shift, long long* num_batches_tracked,
                   void* stream);   /* partial: [2][CP][ntiles]; num_batches_tracked (optional) += groups */
int dh_bn_eval_params(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      float eps, int C, float* scale, float* shift, void* stream);
int dh_bn_apply(int dtype, const void* x, const void* residual, void* y, const float* scale, const float* shift,
                long npix, int C, int groups, int act, void* stream);
int dh_bn_bwd(int dtype, const void* dout, const void* out_relu, const void* x, const float* mean,
              const float* invstd, const float* gamma, long npix, int C, int groups, void* dx, void* dres,
              float* dgamma, float* dbeta, int accumulate, const float* mask_scale, const float* mask_shift,
              void* workspace, void* stream);
/* ReLU mask of the layer: out_relu (its post-activation output) OR mask_scale / mask_shift [groups][C] (the forward's
 * scale / shift: mask = x * scale + shift > 0, for layers without a residual input) OR neither (no ReLU) */
long dh_bn_bwd_workspace_size(long npix, int C, int groups);
/* dh_bn_bwd as ONE persistent launch (csrc/bn_bwd_persist.hip): 256 workgroups hold dout (registers) and x (LDS) on chip
 * across a device-wide barrier, so each tensor is read once.  bf16 only; dh_bn_bwd_persist_supported() tells whether the
 * layer fits (otherwise call dh_bn_bwd).  sync: 8192 zero-initialised uint32 words owned by the caller and reused by every
 * call on ONE stream.  The barrier needs all 256 workgroups resident: never launch it where a kernel of another stream
 * (a collective, a side-stream launch) may hold CUs.  Error word sync[2]: bit 0 = the bounded barrier spin timed out, bit 1 =
 * a non-finite / out-of-range partial sum; when it is set dgamma / dbeta come out NaN.  dh_bn_bwd_persist_status() returns
 * and clears the word (synchronises the stream; < 0: the copy failed).  workspace: as dh_bn_bwd.  Same autograd call site. */
int dh_bn_bwd_persist_supported(int dtype, long npix, int C, int groups);
int dh_bn_bwd_persist_preferred(int dtype, long npix, int C, int groups);   /* supported AND large enough to be faster */
int dh_bn_bwd_persist(const void* dout, const void* out_relu, const void* x, const float* mean, const float* invstd,
                      const float* gamma, long npix, int C, int groups, void* dx, void* dres, float* dgamma, float* dbeta,
                      int accumulate, const float* mask_scale, const float* mask_shift, void* workspace, unsigned* sync,
                      void* stream);
/* The ReLU mask of a BatchNorm + residual + ReLU layer (models/resnet.py:56-71, 104-121: out = relu(bn(y) + identity)) as BYTES
 * instead of the post-activation tensor: dh_bn_apply_bits = dh_bn_apply that also writes relu_bits [npix * C / V] (V = 8 bf16 /
 * 4 fp32 elements per 16-byte piece) -- byte i holds the mask of piece i of y, bit j = (y[V i + j] > 0) -- and dh_bn_bwd_bits /
 * dh_bn_bwd_persist_bits (bf16) =
 * dh_bn_bwd / dh_bn_bwd_persist reading those bytes where the latter read out_relu: one sixteenth of a tensor pass instead of
 * one (persistent form) or two (two-pass form).  Same results bit for bit.  Replaces the same autograd nodes as dh_bn_bwd
 * (native_batch_norm_backward + threshold_backward). */
int dh_bn_apply_bits(int dtype, const void* x, const void* residual, void* y, const float* scale, const float* shift, long npix,
                     int C, int groups, int act, unsigned char* relu_bits, void* stream);
/* dh_bn_apply / dh_bn_apply_bits (relu_bits optional) whose residual is the BatchNorm output of a block's shortcut, given as
 * that BatchNorm's INPUT `residual` + its res_scale / res_shift [groups][C]: the value added is T(residual * res_scale +
 * res_shift), rounded through the tensor's dtype exactly as dh_bn_apply(residual, res_scale, res_shift) would have stored it.
 * Same y and relu_bits bit for bit; the shortcut's normalised tensor is never written or read back. */
int dh_bn_apply_res_affine(int dtype, const void* x, const void* residual, const float* res_scale, const float* res_shift, void* y,
                           const float* scale, const float* shift, long npix, int C, int groups, int act,
                           unsigned char* relu_bits, void* stream);
int dh_bn_bwd_bits(int dtype, const void* dout, const unsigned char* relu_bits, const void* x, const float* mean, const float* invstd,
                   const float* gamma, long npix, int C, int groups, void* dx, void* dres, float* dgamma, float* dbeta, int accumulate,
                   void* workspace, void* stream);
int dh_bn_bwd_persist_bits(const void* dout, const unsigned char* relu_bits, const void* x, const float* mean, const float* invstd,
                           const float* gamma, long npix, int C, int groups, void* dx, void* dres, float* dgamma, float* dbeta,
                           int accumulate, void* workspace, unsigned* sync, void* stream);
int dh_bn_bwd_persist_status(unsigned* sync, void* stream);
int dh_bn_bwd_persist_test_spin_limit(unsigned limit);   /* tests: limit > 0 forces the timeout path (0 restores 2^22 spins) */
int dh_bn_bwd_from_partials(int dtype, const void* g, const void* x, const float* partial, int ntiles, const float* mean,
                            const float* invstd, const float* gamma, long npix, int C, int groups, void* dx,
                            float* dgamma, float* dbeta, int accumulate, void* workspace, void* stream);
int dh_layernorm_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* y, float* stats,
                     long rows, int C, float eps, void* stream);
int dh_layernorm_bwd(int dtype, const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                     const void* dx_add, float* dgamma, float* dbeta, int accumulate, long rows, int C,
                     void* workspace, void* stream);
long dh_layernorm_bwd_workspace_size(long rows);
int dh_reduce_partials(const float* partial, long nt, long n, float scale, float* out, int accumulate, void* stream);

/* ---- pointwise / resampling / layout (models/resnet.py:154; networks.py:199-200,384,1312,1348) ---- */
/* input pipeline on the device (replaces the per-sample PIL work of datasets/data_utils.py:55-111 -- crop window, h / v
 * flip, ToTensor + Normalize(0.5, 0.5) -- for pre-decoded pairs): a, b [S][H][W][3] uint8, l [S][H][W] uint8 (or NULL);
 * output sample n takes source pair idx[n] with params[n] = {x0, y0, hflip, vflip}; out_a / out_b fp32 [N][3][h][w],
 * out_l uint8 [N][1][h][w]. */
int dh_augment_pairs_u8(const unsigned char* a, const unsigned char* b, const unsigned char* l, const int* idx,
                        const int* params, int N, int H, int W, int h, int w, float* out_a, float* out_b,
                        unsigned char* out_l, void* stream);
/* The same batch with the reference's random Gaussian blur on A and B (PIL ImageFilter.GaussianBlur(radius), radius < sqrt(2),
 * datasets/data_utils.py:99-102), byte-exact: three 3-tap box passes along the rows, then three along the columns, on uint8 with
 * the window's edge pixel replicated in every pass, out = (in * ww + (left + right) * fw + (1 << 23)) >> 24.  blur [N][2] int32 =
 * sample n's (ww, fw), 0 < ww <= 1 << 24, fw >= 0, ww + 2 fw <= 1 << 24 (the caller checks them where it writes the table:
 * the 32-bit accumulator relies on it); (1 << 24, 0) is the unblurred result bit for bit.  Labels are not blurred. */
int dh_augment_pairs_blur_u8(const unsigned char* a, const unsigned char* b, const unsigned char* l, const int* idx,
                             const int* params, const int* blur, int N, int H, int W, int h, int w, float* out_a,
                             float* out_b, unsigned char* out_l, void* stream);
/* Input pipeline of the xBD step (TrainData / ValData.__getitem__, xBD_code/train.py:99-183, 194-244, for pre-decoded samples):
 * pre, post [n_src][H][W][3] uint8, pre_mask (0 / 255; NULL in train mode, which overwrites it) and post_label (0 .. 4)
 * [n_src][H][W] uint8.  Output sample n takes source idx[n] with params[n] = {x0, y0, hflip, vflip, resize, top, left, height,
 * width}: the S x S crop at (x0, y0), the flips, then -- if `resize` -- TF.resized_crop(img, top, left, height, width, (S, S)) on
 * all four arrays (train.py:132-136), byte-exact: PIL's img.crop(box).resize((S, S), Image.BILINEAR), two fixed-point passes
 * (rows, then columns) that each round to uint8.  The box lies inside the crop, 1 <= height, width <= S.  coef [N][2][S][4] int32
 * = (first source index, k0, k1, k2) of every output index, axis 0 along x (`width` source pixels) and axis 1 along y (`height`),
 * as datasets/xbd_pipeline.resize_coeffs writes it.  The caller guarantees 0 <= k and k0 + k1 + k2 <= (1 << 22) + 8192: a pass's
 * byte is then in range without a clip.  Rows of samples without the flag are not read, and coef == NULL means that no sample
 * resizes (the flag is then ignored).  Then the masks: mode 0 (train) msk[k] = (label == k)
 * for k = 1 .. 4 and msk[0] = any of them; mode 1 (val) msk[0] = (pre_mask > 127) instead, and out_lbl = label - 1 where label is
 * 1 .. 4, else 0.  out_img fp32 [N][6][S][S] = preprocess_inputs(concat(pre, post)) = x / 127 - 1; out_msk uint8 [N][5][S][S],
 * 0 / 1; out_lbl uint8 [N][S][S], written in mode 1 only (NULL allowed in mode 0). */
int dh_xbd_augment_u8(const unsigned char* pre, const unsigned char* post, const unsigned char* pre_mask,
                      const unsigned char* post_label, const int* idx, const int* params, const int* coef, int N, int H, int W,
                      int S, int mode, float* out_img, unsigned char* out_msk, unsigned char* out_lbl, void* stream);
/* The same batch with the reference's ColorJitter(brightness, contrast, saturation) on the pre and post images of the samples
 * that draw it (train.py:138-139), byte-exact against PIL's ImageEnhance chain, after the resize and before preprocess_inputs;
 * masks and labels are not touched.  jitter_host [N][2][8] int32 in HOST memory (the entry checks it, then copies it into the
 * workspace on `stream`; it is read before the call returns): row (n, image) = {enabled 0 / 1, the three operations in applied
 * order (0 brightness, 1 contrast, 2 saturation, each once), the float32 bits of the brightness, contrast and saturation
 * factors, 0}; image 0 is pre, 1 is post.  An operation is Image.blend(degenerate, image, factor) per byte, (float)d + factor *
 * (float)(i - d) in two float32 roundings (not fused), clipped to 0 .. 255 and truncated; d = 0 (brightness), L of the pixel
 * (saturation) or int(mean + 0.5) of L over the whole S x S image as it stands when contrast is applied.  That mean takes a launch
 * of its own before the apply launch (exact integer partial sums per tile, in the workspace; none when no row is enabled).
 * workspace: device memory, 4-byte aligned, N * 2 * (8 + dh_xbd_augment_jitter_tiles(S)) * 4 bytes (tiles: the workgroups of an
 * S x S image; 0 for an S the entry refuses).  S <= 4096 (32-bit sums), 2 N <= 65535.  A sample whose rows are both disabled gets
 * dh_xbd_augment_u8's bytes. */
int dh_xbd_augment_jitter_tiles(int S);
int dh_xbd_augment_jitter_u8(const unsigned char* pre, const unsigned char* post, const unsigned char* pre_mask,
                             const unsigned char* post_label, const int* idx, const int* params, const int* coef,
                             const int* jitter_host, int N, int H, int W, int S, int mode, float* out_img, unsigned char* out_msk,
                             unsigned char* out_lbl, void* workspace, long workspace_bytes, void* stream);
/* Input pipeline of DAHiTra's own training script (TrainData.__getitem__, xBD_code/train_unettransformer.py:109-167, 206-209,
 * 255-279, for pre-decoded samples) in one launch: pre, post [n_src][H][W][3] uint8 RGB and post_label (0 .. 4) [n_src][H][W]
 * uint8 (the pre mask is not an argument: the script overwrites its channel, line 264).  Output sample n takes source idx[n] with
 * params[n] = 12 int32 {x0, y0, vflip, rot, sx, sy, warp, chan, dR, dG, dB, 0}: the S x S crop at (x0, y0); rows reversed if
 * `vflip`; np.rot90(., rot), rot = 0 .. 3 (1 is counter-clockwise: out[i][j] = in[j][S-1-i]); shift_image by (sx, sy), i.e.
 * dst(x, y) = src(x - sx, y - sy) with cv2.BORDER_REFLECT_101 (0, 0: none); if `warp`, rotate_image = cv2.warpAffine(INTER_LINEAR,
 * BORDER_REFLECT_101) in OpenCV's fixed-point arithmetic for CV_8U (4.x up to 4.10) from tab [N][4][S] int32 = adelta[x],
 * bdelta[x], X0[y], Y0[y] as datasets/xbd_pipeline.unet_warp_table writes them: X = (X0[y] + adelta[x]) >> 5, Y likewise, taps at
 * (X >> 5, Y >> 5) and its right / lower neighbours, fractions X & 31 and Y & 31, weights (32 - fx)(32 - fy) 32 .. fx fy 32, byte
 * = (sum w v + 16384) >> 15; then shift_channels: dR, dG, dB added to the planes of the pre (chan 1) or post (chan 2) image and
 * clipped to 0 .. 255 (chan 0: nobody).  All of it is one gather from the sources: no intermediate image.  Rows of `tab` of
 * samples without the flag are not read, and tab == NULL means that no sample warps.  Every tap index is reflected into the crop
 * and clamped into the image whatever the rows and tables hold.  out_img fp32 [N][6][S][S] = preprocess_inputs(concat(pre,
 * post)) = x / 127 - 1; out_msk uint8 [N][5][S][S], 0 / 1: channel c = 1 .. 4 is the warped 0 / 255 plane of (label == c)
 * thresholded > 127, ((255 * (weights of the taps whose label == c) + 16384) >> 15) > 127, channel 0 any of them.  A row of zeros
 * but for (x0, y0) gives dh_xbd_augment_u8's train-mode bytes.
 * Refused (nothing is written, non-zero, dh_last_error begins with xbd_augment_warp): a null pointer other than tab, S < 1,
 * S > H, S > W, N < 1 or beyond the launch grid (65535).
 * dh_xbd_augment_warp_tile_h / _w: the output tile of a workgroup. */
int dh_xbd_augment_warp_tile_h(void);
int dh_xbd_augment_warp_tile_w(void);
int dh_xbd_augment_warp_u8(const unsigned char* pre, const unsigned char* post, const unsigned char* post_label, const int* idx,
                           const int* params, const int* tab, int N, int H, int W, int S, float* out_img, unsigned char* out_msk,
                           void* stream);
/* The colour stage of the same script (xBD_code/train_unettransformer.py:211-244) IN PLACE on img fp32 [N][6][S][S], the batch
 * dh_xbd_augment_warp_u8 wrote: a value decodes to its byte as rint((f + 1) 127) and encodes as x / 127 - 1 again.  jobs [J][12]
 * int32 (device), one row per (sample, image) that drew anything, in any order, at most one per pair: {sample, image (0 pre,
 * 1 post), hsv flag, h, s, v, op, the float64 bits of the factor (low word, high word), noise plane, 0, 0}.  First change_hsv if
 * flagged: 8-bit COLOR_BGR2HSV in OpenCV's integer form (hsv_shift 12: V = max, d = V - min, S = (d sdiv[V] + 2048) >> 12, H0 =
 * g - b / b - r + 2 d / r - g + 4 d where V is r / g / b, H = (H0 hdiv[d] + 2048) >> 12, + 180 if negative), h, s, v added and
 * clipped to 0 .. 255 each, and 8-bit COLOR_HSV2BGR in OpenCV's scalar float32 form (h = H (6 / 180), s = S / 255, v = V / 255 as
 * products with float32 constants; h = fmod(h, 6), k = floor(h), f = h - k; t = {v, v (1 - s), v (1 - s f), v (1 - s (1 - f))}
 * selected by sector; s == 0 is the grey v; byte = rint(255 x), saturated; every operation rounded on its own).  Then op: 0 none;
 * 1 gauss_noise, min(byte + noise, 255) with noise [K][S][S][3] uint8 in the script's B, G, R order; 2 cv2.blur(3 x 3),
 * (2 sum + 9) / 18 of the window under BORDER_REFLECT_101; 3 saturation, 4 brightness, 5 contrast = clip(byte * factor +
 * (1 - factor) * gs, 0, 255) in float64, truncated, with gs = (0.114 b + 0.587 g) + 0.299 r of the pixel, 0, or that grey of the
 * exact channel sums over S * S.  No operation is contracted into a fused multiply-add.  Two launches whatever the jobs; samples
 * without a row are not touched; the result is deterministic.  The sample and noise indices are clamped, the image is one bit,
 * the shifts are clamped to +-255 and an unknown op is none: no table content makes the kernels read or write outside img, noise
 * and the workspace.  workspace: device memory, 4-byte aligned, dh_xbd_unet_colour_ws_bytes(J, S) bytes (the bytes of the jobs'
 * images and one integer sum per tile and channel).
 * Refused (nothing is written, non-zero, dh_last_error begins with xbd_unet_colour): a null img, jobs or workspace, noise NULL
 * with K > 0 or not NULL with K == 0, N < 1, S < 1 or > 4096, J < 1 or > 65535, K < 0, a workspace that is too small or not
 * aligned.  dh_xbd_unet_colour_tile: the side of a workgroup's square tile. */
int dh_xbd_unet_colour_tile(void);
int dh_xbd_unet_colour_ws_bytes(int J, int S, long* bytes);
int dh_xbd_unet_colour_u8(float* img, const int* jobs, const unsigned char* noise, int N, int S, int J, int K, void* workspace,
                          long workspace_bytes, void* stream);
int dh_nchw_to_nhwc(int dtype, const float* src, void* dst, int N, int C, long HW, int CP, void* stream);
/* data gradient of the class head (3x3 / s1 / p1, 32 -> n_class <= 8 channels; help_funcs.py:13-14, networks.py:1247):
 * dy [N][H][W][CP] (CP = 8 bf16 / 4 or 8 fp32 channels per pixel, the first NC real), w_oihw [NC][32][3][3] fp32,
 * dx [N][H][W][32] */
int dh_head_dgrad3x3(int dtype, const void* dy, int CP, const float* w_oihw, int NC, void* dx, int N, int H, int W,
                     void* stream);
/* The same data gradient for a head whose 32 input channels are the output of a ReLU (classifier(conv_layer2(...)),
 * models/networks.py:1351-1355; bf16, n_class <= 2, CP = 8): relu_out [N][H][W][32] is that output and
 * dx = gradient * (relu_out > 0) -- the activation's backward pass (3 x 134 MB at batch 32) folded into this kernel. */
int dh_head_dgrad3x3_relu(const void* dy, const float* w_oihw, int NC, const void* relu_out, void* dx, int N, int H, int W,
                          void* stream);
/* The same data gradient GATED for the BatchNorm + ReLU behind the 32 channels (classifier[0..2], models/help_funcs.py:7-15; bf16,
 * n_class <= 2): g = gradient * (y * mask_scale + mask_shift > 0) and the per-workgroup partials [2][32][blocks] (sum g,
 * sum g * xhat) for dh_bn_bwd_from_partials -- that BatchNorm's reduction pass disappears. */
int dh_head_dgrad3x3_bn_blocks(int N, int H, int W, int groups);
int dh_head_dgrad3x3_bn(const void* dy, const float* w_oihw, int NC, const void* y, const float* mask_scale, const float* mask_shift,
                        const float* mean, const float* invstd, int groups, void* g, float* partial, int N, int H, int W,
                        void* stream);
/* The head's data gradient AND the backward of the BatchNorm + ReLU behind its 32 channels in two passes that never write the
 * gradient in between (n_class <= 8; the autograd of Conv2d(32, n_class, 3) <- ReLU <- BatchNorm2d(32),
 * models/help_funcs.py:7-15): each pass forms g = (y * mask_scale + mask_shift > 0) * (W^T (*) dlogits) on the matrix cores from
 * dlp, the dlogits as [N][H + 2][W + 2] class pieces inside a border of zeros (dh_head_dlogits_pack from the loss kernel's
 * [N][n_class][H][W] fp32: a piece = 2 classes in one word for n_class <= 2, 8 classes in 16 bytes for 3 .. 8 -- the five-class
 * heads of the xBD nets; a tap is one load, no bounds test); pass 1 reduces (sum g, sum g y), pass 2 writes dx = gamma invstd (g - (s1 + xhat s2) / M).  y
 * [N][H][W][32] pre-BatchNorm, statistics [groups][32] as dh_bn_finalize left them; dgamma / dbeta [32] (+)= when accumulate. */
int dh_head_bn_bwd_blocks(int N, int H, int W, int groups);
long dh_head_bn_bwd_workspace_size(int N, int H, int W, int groups);
/* dw [n_class][32][3][3] / db [n_class] (both or NULL): the head convolution's own weight and bias gradient (input =
 * relu(BatchNorm(y)) as bf16), taken by pass 1 from the loads it makes anyway -- pixels are the K dimension of an MFMA through
 * wave-private LDS tiles read back transposed; (+)= when accumulate. */
/* dtype DH_DTYPE_BF16: dlp one word per pixel; DH_DTYPE_F32 (the fp32 pipeline under dh_set_f32_mma_mode != 0): y / dx fp32, dlp two
 * words per pixel (bf16 heads, bf16 remainders) and every product as the three split bf16 products of that mode. */
int dh_head_dlogits_pack(int dtype, const float* dlogits_nchw, int N, int NC, int H, int W, void* dlp, void* stream);
int dh_head_bn_bwd(int dtype, const void* dlp, const float* w_oihw, int NC, const void* y, const float* mask_scale, const float* mask_shift,
                   const float* mean, const float* invstd, const float* gamma, int groups, void* dx, float* dgamma, float* dbeta,
                   float* dw, float* db, int accumulate, int N, int H, int W, void* workspace, void* stream);
/* The class head behind a ReLU (classifier(conv_layer2(...)), models/networks.py:1351-1355; n_class <= 8): the data gradient
 * dx = (relu_out > 0) * (W^T (*) dlogits) of dh_head_dgrad3x3_relu, from the pair map dlp (dh_head_dlogits_pack), AND the head's
 * own weight / bias gradient dw [n_class][32][3][3] / db [n_class] ((+)= when accumulate) from the same loads of relu_out --
 * the head's input.  workspace: dh_head_bn_bwd_workspace_size(N, H, W, 1) bytes. */
int dh_head_relu_bwd(int dtype, const void* dlp, const float* w_oihw, int NC, const void* relu_out, void* dx, float* dw, float* db,
                     int accumulate, int N, int H, int W, void* workspace, void* stream);
/* The class head's forward (nn.Conv2d(32, n_class, 3, padding=1): models/help_funcs.py:13-14, networks.py:1247 / 1355) for
 * n_class <= 2 and bf16 activations: x [N][H][W][32] (pre-BatchNorm when in_scale / in_shift [in_groups][32] are given: the
 * head's input is relu(x * scale + shift)), w_oihw [n_class][32][3][3] fp32, bias [n_class] or NULL -> logits [N][n_class][H][W]
 * fp32.  The contraction over the input channels is done once per input pixel for all nine taps (M = (tap, class) = 18), the
 * convolution is a nine-term gather from a ring of rows in LDS: no halo, no padded output channels.  dh_head_fwd_supported:
 * whether (n_class, W) is this kernel's shape (else dh_conv3x3_head_fwd). */
int dh_head_fwd_supported(int NC, int W);
/* dtype DH_DTYPE_F32: x fp32 and every product as three fp16-plane products -- the arithmetic of dh_set_f32_mma_mode(3), for
 * callers in that mode only. */
int dh_head_fwd(int dtype, const void* x, const float* w_oihw, const float* bias, int NC, const float* in_scale, const float* in_shift,
                int in_groups, float* logits_nchw, int N, int H, int W, void* stream);
/* A job table of small element-wise kernels in ONE launch (no reference counterpart: autograd runs one op at a time): the three
 * levels of _forward_trans_module (models/networks.py:1297-1318) each issue a positional add, the channel concatenation of the two
 * streams, |token2 - token1| and their gradients between the launches they share; the independent ones of a round go out together.
 * n <= 12 jobs that must not depend on each other; per job an op and its operands (see csrc/pointwise.hip dh_ew_multi):
 * ADD_POS = dh_add_pos (bf16, C % 8 == 0), CAT_HALVES / SPLIT_HALVES = dh_cat_halves (bf16), ABSDIFF_HALVES(_BWD) =
 * dh_absdiff_halves(_bwd) (fp32), ADD_POS_BWD = dh_add_pos_bwd (bf16, C = 32). */
enum { DH_EW_ADD_POS = 1, DH_EW_CAT_HALVES = 2, DH_EW_SPLIT_HALVES = 3, DH_EW_ABSDIFF_HALVES = 4, DH_EW_ABSDIFF_HALVES_BWD = 5,
       DH_EW_ADD_POS_BWD = 6 };
int dh_ew_multi(int n, const int* op, const void* const* a, const void* const* b, void* const* c, const int* i0, const int* i1,
                const long* l0, void* stream);
int dh_nhwc_to_nchw(int dtype, const void* src, float* dst, int N, int C, long HW, void* stream);
int dh_copy_channels(int dtype, const void* src, int Cs, int sc0, void* dst, int Cd, int dc0, int Cn, long P, void* stream);
/* torch.cat([x1, x2], 1) of the two temporal streams (models/networks.py:1309, 1344), which are the two batch halves of
 * t [2 P][C] here: cat [P][2 C] <- t (inverse = 0), or t <- cat (inverse = 1: the concatenation's gradient back to the
 * streams); both halves in one launch.  C a multiple of the 16-byte piece (8 bf16 / 4 fp32). */
int dh_cat_halves(int dtype, void* t, void* cat, int C, long P, int inverse, void* stream);
int dh_add(int dtype, const void* a, const void* b, void* y, long n, void* stream);
int dh_add_pos(int dtype, const void* x, const float* pos, void* y, int N, long HW, int C, void* stream);
int dh_add_pos_bwd(int dtype, const void* dy, float* dpos, int N, long HW, int C, int accumulate, void* stream);
int dh_act_bwd(int dtype, const void* dy, const void* ref, void* dx, long n, int act, void* stream);
/* argmax (optional, [N][OH][OW][C] bytes): window position 0..8 of the first maximum, consumed by the backward */
int dh_maxpool3x3s2_fwd(int dtype, const void* x, void* y, unsigned char* argmax, int N, int H, int W, int C,
                        const float* bn_scale, const float* bn_shift, int groups, void* stream);
/* bn_scale / bn_shift [groups][C] (optional): x is the PRE-normalisation input of a train-mode BatchNorm + ReLU whose
 * only consumer is this pool (the ResNet stem, models/resnet.py:207-210): relu(x * scale + shift) is applied on load */
int dh_maxpool3x3s2_bwd(int dtype, const unsigned char* argmax, const void* dy, void* dx, int N, int H, int W, int C, void* stream);
int dh_upsample2_nearest_fwd(int dtype, const void* x, void* y, int N, int H, int W, int C, void* stream);
int dh_upsample2_nearest_bwd(int dtype, const void* dy, void* dx, int N, int H, int W, int C, void* stream);
int dh_absdiff_upsample4_fwd(int dtype, const void* a, const void* b, void* y, int N, int H, int W, int C, void* stream);
int dh_absdiff_upsample4_bwd(int dtype, const void* a, const void* b, const void* dy, void* da, void* db, int N, int H, int W, int C, void* stream);
int dh_absdiff(int dtype, const void* a, const void* b, void* y, long n, void* stream);
int dh_absdiff_bwd(int dtype, const void* a, const void* b, const void* dy, void* da, void* db, long n, int accumulate, void* stream);
int dh_colsum(int dtype, const void* x, long P, int C, float* out, int accumulate, void* workspace, void* stream);  /* workspace: 1024 * C floats */
int dh_cast_from_f32(int dtype, const float* src, void* dst, long n, void* stream);
int dh_cast_to_f32(int dtype, const void* src, float* dst, long n, int accumulate, void* stream);

/* ---- token side (models/networks.py:312-336,457-488; help_funcs.py:66-114) --------------------
 * xattn_prep: wq / wk / wv / wo are the fp32 masters ([inner][32] resp. [32][inner]); wkT, wvT, wqT ([32][inner])
 * and woT ([inner][32]) are their transposes in T as produced by dh_pack_weight's data-gradient form. */
int dh_tokenizer_fwd(int dtype, const void* x, const float* wa, const float* pos, int S, int B, int HW, int L,
                     float* logits, float* stats, float* pooled, float* tok_cat, void* workspace, void* stream);
long dh_tokenizer_fwd_workspace_size(int S, int HW, int L);
int dh_tokenizer_bwd(int dtype, const void* x, const float* wa, int S, int B, int HW, int L, const float* logits,
                     const float* stats, const float* pooled, const float* dtok_cat, void* dx_accum, float* dwa,
                     float* dpos, int accumulate, void* workspace, void* stream);
long dh_tokenizer_bwd_workspace_size(int S, int HW, int L);
int dh_xattn_prep_fwd(int dtype, const void* tok, long tok_bstride, long tok_sstride, int B, int S, int L, int heads,
                      int dim_head, int HLP, float scale, float eps, const float* ln_g, const float* ln_b,
                      const float* wq, const void* wkT, const void* wvT, const void* woT, float* mn, float* mstats,
                      float* k, float* v, void* kq, void* kqT, void* vo, void* voT, void* stream);
/* stacked forms: ONE launch prepares all `layers` of a decoder stack (they read the same tokens).  Parameter /
 * gradient pointers are the first layer's, consecutive layers lie param_stride floats apart (the net's flat arena);
 * wkT / wvT / woT / wqT and every saved / output tensor are stacked [layers][single-layer shape]. */
int dh_xattn_prep_fwd_stack(int dtype, const void* tok, long tok_bstride, long tok_sstride, int B, int S, int L, int heads,
                            int dim_head, int HLP, float scale, float eps, int layers, long param_stride,
                            const float* ln_g, const float* ln_b, const float* wq, const void* wkT, const void* wvT,
                            const void* woT, float* mn, float* mstats, float* k, float* v, void* kq, void* kqT, void* vo,
                            void* voT, void* stream);
/* The same preparation on the matrix cores (csrc/tokens.hip: four images = the 16 columns of one MFMA per workgroup, heads over
 * the waves) for bf16 nets with L = 4, S a multiple of 4, dim_head 32 / 64, HLP = 32 (dh_xattn_prep_mfma_supported).  wk / wv
 * ([inner][32]) and wo ([32][inner]) are the first layer's fp32 masters, wqT the stacked bf16 transposes [layers][32][inner]. */
int dh_xattn_prep_mfma_supported(int dtype, int S, int L, int heads, int dim_head, int HLP);
int dh_xattn_prep_fwd_stack_mfma(const void* tok, long tok_bstride, long tok_sstride, int B, int S, int heads, int dim_head,
                                 int HLP, float scale, float eps, int layers, long param_stride, const float* ln_g,
                                 const float* ln_b, const float* wk, const float* wv, const float* wo, const void* wqT,
                                 float* mn, float* mstats, float* k, float* v, void* kq, void* kqT, void* vo, void* voT,
                                 void* stream);
int dh_xattn_prep_bwd_stack_mfma(const void* tok, void* dtok_accum, long tok_bstride, long tok_sstride, int B, int S, int heads,
                                 int dim_head, int HLP, float scale, int layers, long param_stride, const float* ln_g,
                                 const float* wq, const void* woT, const void* wkT, const void* wvT, const float* mn,
                                 const float* mstats, const float* k, const float* v, const float* dkq, const float* dvoT,
                                 float* dk, float* dv, float* dln_g, float* dln_b, float* dwq, float* dwk, float* dwv,
                                 float* dwo, int accumulate, void* workspace, void* stream);
int dh_xattn_prep_bwd_stack(int dtype, const void* tok, void* dtok_accum, long tok_bstride, long tok_sstride, int B, int S,
                            int L, int heads, int dim_head, int HLP, float scale, int layers, long param_stride,
                            const float* ln_g, const void* wqT, const float* wk, const float* wv, const float* wo,
                            const float* mn, const float* mstats, const float* k, const float* v, const float* dkq,
                            const float* dvoT, float* dk, float* dv, float* dln_g, float* dln_b, float* dwq, float* dwk,
                            float* dwv, float* dwo, int accumulate, void* workspace, void* stream);
long dh_xattn_prep_bwd_stack_workspace_size(int S, int L, int layers);
int dh_xattn_prep_bwd(int dtype, const void* tok, void* dtok_accum, long tok_bstride, long tok_sstride, int B, int S,
                      int L, int heads, int dim_head, int HLP, float scale, const float* ln_g, const void* wqT,
                      const float* wk, const float* wv, const float* wo, const float* mn, const float* mstats,
                      const float* k, const float* v, const float* dkq, const float* dvoT, float* dk, float* dv,
                      float* dln_g, float* dln_b, float* dwq, float* dwk, float* dwv, float* dwo, int accumulate,
                      void* workspace, void* stream);
long dh_xattn_prep_bwd_workspace_size(int S);
int dh_softmax_groups_fwd(int dtype, const void* x, void* y, long rows, int heads, int L, int HLP, void* stream);
int dh_softmax_groups_bwd(int dtype, const void* y, const void* dy, void* dx, long rows, int heads, int L, int HLP, void* stream);
int dh_self_attn_fwd(int dtype, const void* qkv, void* o, float* attn, int B, int n, int heads, int dim_head, float scale, void* stream);
int dh_self_attn_bwd(int dtype, const void* qkv, const float* attn, const void* dout, void* dqkv, int B, int n, int heads, int dim_head, float scale, void* stream);

/* Fused token encoder stack (models/networks.py:457-512, help_funcs.py:117-167) on the 2*token_len <= 8 tokens of an
 * image pair, fp32: one workgroup per image and direction + one launch for all parameter gradients.  x, y, dy, dx:
 * [B][n][32]; parameters are the first layer's pointers in torch layouts (to_qkv [3*inner][32], to_out [32][inner],
 * net.0 [mlp][32], net.3 [32][mlp]), consecutive layers param_stride floats apart; gradients are accumulated.
 * dh_encoder_supported: 1 when the shape fits the kernels (n <= 8, mlp <= 64, dim_head % 16 == 0, heads*n*n and n*mlp multiples
 * of 4 -- every LDS buffer and saved record 16-byte aligned --, working set within the 160 KB LDS). */
int dh_encoder_supported(int n, int heads, int dim_head, int mlp);
int dh_encoder_fwd(const float* x, float* y, float* saved_inputs, int B, int n, int depth, int heads, int dim_head,
                   int mlp, float scale, float eps, long param_stride, const float* ln1_g, const float* ln1_b,
                   const float* wqkv, const float* wo, const float* bo, const float* ln2_g, const float* ln2_b,
                   const float* w1, const float* b1, const float* w2, const float* b2, void* stream);
int dh_encoder_bwd(const float* dy, float* dx, const float* saved_inputs, int B, int n, int depth, int heads,
                   int dim_head, int mlp, float scale, float eps, long param_stride, const float* ln1_g,
                   const float* ln1_b, const float* wqkv, const float* wo, const float* bo, const float* ln2_g,
                   const float* ln2_b, const float* w1, const float* b1, const float* w2, const float* b2,
                   float* dln1_g, float* dln1_b, float* dwqkv, float* dwo, float* dbo, float* dln2_g, float* dln2_b,
                   float* dw1, float* db1, float* dw2, float* db2, void* workspace, void* stream);
/* Batched encoder stacks (csrc/encoder_fused.hip): a stack runs one workgroup per image, i.e. a launch of its own keeps B of
 * the 256 CUs busy; the three levels of the hierarchical model are independent, so their stacks can share a launch.  Between
 * dh_encoder_batch_begin() and _end(), dh_encoder_fwd / dh_encoder_bwd only RECORD (up to four of each direction; a fifth
 * issues the first four); dh_encoder_batch_launch(stream) issues the recorded forward stacks as one launch and / or the
 * recorded backward stacks as one data-gradient + one parameter-gradient launch.  Every buffer of a recorded call (its
 * workspace included: one per call) must stay alive and unchanged until then.  State per host thread; _abort drops the
 * recorded calls without launching. */
int dh_encoder_batch_begin(void);
int dh_encoder_batch_pending(void);
int dh_encoder_batch_launch(void* stream);
int dh_encoder_batch_end(void* stream);
int dh_encoder_batch_abort(void);
/* The same for the fused decoder layers (csrc/decoder_fused.hip): between _begin and _end, dh_decoder_layer_fwd and the
 * data-gradient-only form of dh_decoder_layer_bwd (dw1 == NULL) only RECORD (up to four per direction and MLP width);
 * dh_decoder_batch_launch issues the recorded layers -- of INDEPENDENT stacks: never two layers of one stack -- as one launch
 * per direction and width. */
int dh_decoder_batch_begin(void);
int dh_decoder_batch_pending(void);
int dh_decoder_batch_launch(void* stream);
int dh_decoder_batch_end(void* stream);
int dh_decoder_batch_abort(void);
/* And for the cross-attention operand preparation of a decoder stack (csrc/tokens.hip; models/help_funcs.py:118-160, the
 * token side of Cross_Attention): between _begin and _end, dh_xattn_prep_fwd_stack_mfma and dh_xattn_prep_bwd_stack_mfma with
 * dim_head 64 only RECORD (up to four each).  _launch_fwd issues the recorded preparations as ONE launch; _launch_bwd the
 * recorded gradients as one launch per kernel of the family (operand gradients, token-gradient reduction, projection weight
 * gradients, LayerNorm gradients).  A recorded backward needs a workspace and dk / dv of its OWN until then.
 * dh_decoder_stack_bwd_finalize is recorded by the decoder batch in the same way and issued after its backward launches, so
 * the order `dh_xprep_batch_launch_fwd, dh_decoder_batch_launch, dh_xprep_batch_launch_bwd` is right for calls recorded
 * in program order.  _pause(1): calls launch at once although a batch is open; _pause(0) records again. */
int dh_xprep_batch_begin(void);
int dh_xprep_batch_pending(void);
int dh_xprep_batch_pause(int paused);
int dh_xprep_batch_launch_fwd(void* stream);
int dh_xprep_batch_launch_bwd(void* stream);
int dh_xprep_batch_end(void* stream);
int dh_xprep_batch_abort(void);
long dh_encoder_bwd_workspace_size(int B, int n, int depth, int heads, int dim_head, int mlp);
/* floats of `saved_inputs` (non-null in training): per (layer, image) the forward's intermediates -- layer input, LayerNorm
 * outputs and statistics, qkv, attention probabilities and output, MLP activations -- which dh_encoder_bwd reads back
 * instead of recomputing the layer */
long dh_encoder_saved_floats(int B, int n, int depth, int heads, int dim_head, int mlp);

/* Fused cross-attention decoder layer (help_funcs.py:170-186: Residual2(PreNorm2(Cross_Attention)) + Residual(PreNorm(
 * FeedForward))) in one kernel per direction; bf16, token_len 4, heads*4 <= 32, rows per image % 128 == 0.
 * kq / voT / vo / kqT are the per-image operands of dh_xattn_prep_fwd; w1 [mlp][32], w2 [32][mlp] (+ transposes). */
int dh_decoder_layer_fwd(const void* x, void* y, const void* kq, const void* voT, const float* ln1_g,
                         const float* ln1_b, const float* bo, const float* ln2_g, const float* ln2_b, const void* w1,
                         const float* b1, const void* w2, const float* b2, long rows, int rows_per_image, int mlp,
                         float eps, void* stream);
/* the same layer with OCP fp8 (e4m3) operands in its two ATTENTION products (BASELINE configs[4] "fp8 MFMA attention"): Kq /
 * VoT quantised per output row (absmax / 448) while they are staged, LN(x) / softmax probabilities converted at scale 1,
 * fp32 accumulation; output within ~3e-2 (relative L2) of dh_decoder_layer_fwd.  Forward only: the backward runs
 * dh_decoder_layer_bwd. */
int dh_decoder_layer_fwd_fp8(const void* x, void* y, const void* kq, const void* voT, const float* ln1_g,
                         const float* ln1_b, const float* bo, const float* ln2_g, const float* ln2_b, const void* w1,
                         const float* b1, const void* w2, const float* b2, long rows, int rows_per_image, int mlp,
                         float eps, void* stream);
int dh_decoder_layer_bwd(const void* x, const void* dy, void* dx, const void* kq, const void* voT, const void* vo,
                         const void* kqT, const float* ln1_g, const float* ln1_b, const float* bo, const float* ln2_g,
                         const float* ln2_b, const void* w1, const void* w1T, const float* b1, const void* w2,
                         const void* w2T, const float* b2, float* dw1, float* dw2, float* db1, float* db2, float* dbo,
                         float* dln1_g, float* dln1_b, float* dln2_g, float* dln2_b, float* dkq, float* dvoT, long rows,
                         int rows_per_image, int mlp, float eps, void* workspace, void* stream);
/* A whole fused decoder stack -- `depth` layers of the same shapes attending to ONE set of tokens (TransformerDecoder,
 * models/help_funcs.py:170-186: x = attn(x, m); x = ff(x) per layer with m fixed) -- in ONE launch per direction: a pixel row
 * only ever meets the tokens of its image, so a workgroup takes its rows through all layers, re-staging the layer's weights,
 * with no synchronisation between workgroups.  x [rows][32] bf16; ys [depth][rows][32] receives every layer's output
 * (ys[depth - 1] = the stack's; the backward recomputes each layer from its input).  Layer l's operands: kq / voT / vo / kqT
 * + l * kq_lstride elements (the dh_xattn_prep_fwd_stack outputs), packed MLP weights + l * w_lstride elements, fp32
 * parameter vectors + l * par_lstride floats.  dh_decoder_stack_bwd: dy = gradient of ys[depth - 1], dx = gradient of x, dwork
 * [rows][32] bf16 scratch; partials of layer l at workspace + l * dh_decoder_layer_bwd_workspace_size bytes, for
 * dh_decoder_stack_bwd_finalize.  Bit-identical to `depth` dh_decoder_layer_fwd / _bwd calls; both join an open decoder batch.
 * depth <= 8 (a workgroup keeps every layer's parameter vectors in LDS).  A launch of SEVERAL recorded jobs sizes the pixel
 * blocks of each for the launch as a whole (csrc/decoder_fused.hip dec_plan_launch; DAHITRA_DEC_BALANCE=0: the per-job rule): y / dx
 * do not depend on it, the partial sums -- hence the parameter gradients -- to fp32 summation order.  The workspace of
 * dh_decoder_layer_bwd_workspace_size holds the smallest blocks such a launch may choose (only the blocks written are read).
 * The finalize of a workspace sums exactly the blocks the LAST backward on it wrote, or fails: an eager backward always writes
 * the default plan's blocks (a function of rows, rows_per_image and mlp alone); a batch launch that chose others keeps them,
 * per host thread, until that workspace's finalize (on the same thread, eager or recorded, in that round or a later one)
 * takes them, a later backward on the workspace replaces them, or dh_decoder_batch_abort drops them.  At most 64 such
 * launches may wait for their finalize; a finalize whose rows, rows_per_image or mlp differ from its backward's is refused. */
int dh_decoder_stack_fwd(const void* x, void* ys, const void* kq, const void* voT, const float* ln1_g, const float* ln1_b,
                         const float* bo, const float* ln2_g, const float* ln2_b, const void* w1, const float* b1, const void* w2,
                         const float* b2, int depth, long kq_lstride, long w_lstride, long par_lstride, long rows,
                         int rows_per_image, int mlp, float eps, void* stream);
int dh_decoder_stack_bwd(const void* x, const void* ys, const void* dy, void* dx, void* dwork, const void* kq, const void* voT,
                         const void* vo, const void* kqT, const float* ln1_g, const float* ln1_b, const float* bo,
                         const float* ln2_g, const float* ln2_b, const void* w1, const void* w1T, const float* b1, const void* w2,
                         const void* w2T, const float* b2, int depth, long kq_lstride, long w_lstride, long par_lstride, long rows,
                         int rows_per_image, int mlp, float eps, void* workspace, void* stream);
/* dh_decoder_layer_bwd with dw1 == NULL leaves its per-workgroup partials in `workspace`; this sums the partials of the `depth`
 * layers of one decoder stack (same shapes; layer l's workspace at + l * dh_decoder_layer_bwd_workspace_size bytes, its gradients
 * at + l * grad_stride floats from layer 0's, its dkq / dvoT at + l * images * 1024 floats) in ONE launch. */
int dh_decoder_stack_bwd_finalize(const void* workspace, int depth, long rows, int rows_per_image, int mlp, float* dw1, float* dw2,
                                  float* db1, float* db2, float* dbo, float* dln1_g, float* dln1_b, float* dln2_g, float* dln2_b,
                                  long grad_stride, float* dkq, float* dvoT, void* stream);
long dh_decoder_layer_bwd_workspace_size(long rows, int rows_per_image, int mlp);
/* Host only (no launch, no device): the plan of ONE fused-decoder launch on a device of `cus` compute units.  backward: 0
 * dh_decoder_layer_fwd / _stack_fwd, 1 _layer_bwd / _stack_bwd; stack: the layer-fused form; batch_open: the njobs (<= 4) calls
 * recorded between dh_decoder_batch_begin and _launch, else one eager call (njobs == 1).  Job j has rows[j] pixel rows,
 * rows_per_image[j] and (stacks) depth[j] layers.  out[41], unused fields 0:
 *   [0]          kernel: (mlp == 64) + 2 * stack + 4 * (the multi-job form, which every launch of a batch takes)
 *   [1..4]       grid, threads, dynamic LDS bytes, jobs
 *   [5 + 5 j..]  job j in ISSUE order: its index as given, upb (64-row units per workgroup), bpi (workgroups per image), first
 *                workgroup, workgroups
 *   [25 + 4 j..] backward, the same job: bytes of one layer's workspace (dh_decoder_layer_bwd_workspace_size), and the nblk, bpi
 *                and grid of its dh_decoder_stack_bwd_finalize over max(depth[j], 1) layers
 * Returns non-zero, with dh_last_error set, where the calls themselves would be refused. */
int dh_decoder_plan_describe(int backward, int stack, int mlp, int batch_open, int njobs, const long* rows, const int* rows_per_image,
                             const int* depth, int cus, long* out);

/* ---- loss, mask, optimizer (models/losses.py:106-196; trainer.py:39-40,170) ------------------- */
int dh_focal_loss(const float* logits_nchw, const long long* target, int B, int C, long HW, float alpha,
                  float grad_scale, float* loss_out, float* dlogits_nchw, void* workspace, void* stream);
int dh_argmax_nchw(const float* logits_nchw, long long* mask, int B, int C, long HW, void* stream);
/* batch-size-1 branch of the trainer (models/trainer.py:260-261 -> losses.py:9-26): F.cross_entropy with class
 * weights [1, 1], ignore_index, mean over the contributing pixels.  out_dev[0] = loss, out_dev[1] = pixel count.
 * workspace: 16 KiB. */
int dh_cross_entropy_fwd(const float* logits_nchw, const long long* target, int B, int C, long HW, int ignore_index,
                         float* out_dev, void* workspace, void* stream);
int dh_cross_entropy_bwd(const float* logits_nchw, const long long* target, int B, int C, long HW, int ignore_index,
                         const float* fwd_out_dev, const float* upstream_dev, float* dlogits_nchw, void* stream);
/* the gradient-free dice term of models/trainer.py:256-259 (losses.py:333-339): binary DiceLoss of
 * segmentation_models_pytorch applied to the arg-max mask (third party, not vendored: see oracle dice_constant).
 * workspace: 24 KiB. */
int dh_dice_argmax_constant(const float* logits_nchw, const long long* target, int B, int C, long HW, float eps,
                            float* loss_out, void* workspace, void* stream);
/* HIP-graph-capturable form: hyper_dev = [lr, beta1, beta2, eps, weight_decay, grad_scale, bc1, bc2_sqrt] and the
 * step counter live on the device; every call (or graph replay) advances the counter and the bias correction */
int dh_adamw_step_graph(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n,
                        float* hyper_dev, int* step_dev, void* stream);
/* arg-max over classes (first maximum wins) + confusion counts[gt*C+pred] (int64, accumulated); mask optional */
int dh_confusion_matrix(const float* logits_nchw, const long long* target, int B, int C, long HW, long long* mask,
                        long long* counts, void* stream);
int dh_scale_by_scalar(const float* src, const float* scalar_dev, float* dst, long n, void* stream);
/* |tok[b][1] - tok[b][0]| over [B][2][n] token sets (models/networks.py:1311) and its gradient */
int dh_absdiff_halves(int dtype, const void* tok, void* out, int B, long n, void* stream);
int dh_absdiff_halves_bwd(int dtype, const void* tok, const void* dout, void* dtok_accum, int B, long n, void* stream);
int dh_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);


/* ---- xBD train step (csrc/xbd_step.hip) -------------------------------------------
 * ComboLoss{dice, focal} per output channel on sigmoid(logits) (xBD_code/losses.py:24-34, 95-126, 273-288) with the
 * per-channel weights of xBD_code/train.py:348-353.  logits / masks are [B][C][HW] fp32.  fwd writes the channel
 * totals sums_out [C][4] = {sum s*t, sum s, sum t, sum focal} (needed by bwd), channel_loss_out [C] and loss_out [1]. */
long dh_combo_loss_workspace_size(int C);
int dh_combo_loss_fwd(const float* logits, const float* masks, int B, int C, long HW, const float* weights_dev,
                      float dice_weight, float focal_weight, float* sums_out, float* channel_loss_out, float* loss_out,
                      void* workspace, void* stream);
int dh_combo_loss_bwd(const float* logits, const float* masks, const float* sums, const float* weights_dev,
                      const float* upstream_dev, float dice_weight, float focal_weight, int B, int C, long HW,
                      float* dlogits, void* stream);
/* torch.nn.utils.clip_grad_norm_(params, max_norm) over the flat gradient arena (xBD_code/train.py:373):
 * out_dev[0] = total L2 norm, out_dev[1] = min(1, max_norm / (norm + 1e-6)); the optimizer reads out_dev + 1 */
long dh_grad_norm_workspace_size(void);
int dh_grad_norm_clip_coef(const float* grad, long n, float max_norm, float* out_dev, void* workspace, void* stream);
/* xBD_code/adamw.py:37-86: like dh_adamw_step but denom = sqrt(v) + eps (eps before the bias correction) and the
 * gradient scale is read from device memory (NULL = 1) */
int dh_adamw_xbd_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int step, const float* grad_scale_dev, void* stream);
/* HIP-graph form: hyper_dev = [lr, beta1, beta2, eps, weight_decay, (unused), step_size (out)]; every call / replay
 * advances the device step counter */
int dh_adamw_xbd_step_graph(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float* hyper_dev,
                            int* step_dev, const float* grad_scale_dev, void* stream);

/* ---- loss of xBD_code/train_unettransformer.py's step (lines 438-461; csrc/xbd_script_loss.hip) -----------------
 * loss = sum_c cw_c * ComboLoss{dice, focal}(logits[:, c], msk[:, c]) + ce_weight * CrossEntropyLoss(weight=w)(z, y) with
 * z = logits * (y > 0), in ONE pass over the pixels plus a finalize launch.  logits fp32 [B][5][HW]; msk uint8 [B][5][HW]
 * (bytes 0 / 1, the loader's); label_mode 0: y = lbl [B][HW] uint8; label_mode 1 ("damage"): y = the first set channel among
 * 1 .. 4 of msk, 0 if none, and lbl may be null.  weights_dev: the 5 channel weights cw, then the 5 class weights w.
 * The combo sums and channel losses are dh_combo_loss_fwd's float expressions; ce = (sum w_y nll) / (sum w_y) over ALL pixels
 * (torch's weighted mean), nll = logsumexp(z) - z_y.  A label byte above 4 adds nothing to the two cross-entropy sums, has no
 * cross-entropy gradient and is counted.  fwd writes loss_out [1], parts_out [8] = the five channel losses, ce, the script's
 * Dice meter (2 I + 1e-6) / (S + T + 1e-6) on sigmoid(z_0), the bad-label count; sums_out [24] = [c][4] combo sums, sum w_y,
 * sum w_y nll, the meter's I and S (what bwd reads).  Sums in fp64 through a fixed tree: deterministic.  The 4-pixel form
 * (16-byte logit loads) runs where HW % 4 == 0 and the planes are aligned, the one-pixel form otherwise.
 * dh_xbd_unet_loss_grid_pass: the lanes of one forward grid pass (pixels in the one-pixel form, quads in the other).
 * bwd: dlogits [B][5][HW] = upstream * (cw_c * combo gradient + ce_weight * [y > 0] * w_y / (sum w_y) * (softmax(z)_c - [c == y])),
 * upstream_dev a device scalar or NULL for 1.  Refused (nothing is launched): a null pointer, an empty input, label_mode
 * outside {0, 1}, label_mode 0 without lbl, a workspace smaller than dh_xbd_unet_loss_workspace_size answers. */
int dh_xbd_unet_loss_workspace_size(long* bytes);
int dh_xbd_unet_loss_grid_pass(void);
int dh_xbd_unet_loss_fwd(const float* logits, const unsigned char* msk, const unsigned char* lbl, int label_mode, int B, long HW,
                         const float* weights_dev, float dice_weight, float focal_weight, float ce_weight, float* sums_out,
                         float* parts_out, float* loss_out, void* workspace, long workspace_bytes, void* stream);
int dh_xbd_unet_loss_bwd(const float* logits, const unsigned char* msk, const unsigned char* lbl, int label_mode,
                         const float* sums, const float* weights_dev, const float* upstream_dev, float dice_weight,
                         float focal_weight, float ce_weight, int B, long HW, float* dlogits, void* stream);

/* ---- loss of xBD_code/train_adapt.py's step (lines 332-342; csrc/xbd_script_loss.hip) --------------------------------
 * The four-output sibling of dh_xbd_unet_loss_*: loss = sum_c cw_c * ComboLoss{dice, focal}(logits[:, c], msk[:, c]) + ce_weight *
 * CrossEntropyLoss(weight=w)(logits, y), in ONE pass over the pixels plus a finalize launch.  logits fp32 [B][4][HW]; msk uint8
 * [B][4][HW] (bytes 0 / 1, the loader's), read in place.  y is derived from the mask bytes in the kernel: the FIRST maximum of
 * (1 - m0, m1, m2, m3) as integers, torch.argmax after the script's msks[:, 0] = 1 - msks[:, 0].  The cross-entropy is taken of
 * the raw logits, nothing is masked: every pixel has a cross-entropy gradient.  weights_dev: the 4 channel weights cw, then the 4
 * class weights w.  The combo sums and channel losses are dh_combo_loss_fwd's float expressions; ce = (sum w_y nll) / (sum w_y)
 * over all pixels (torch's weighted mean), nll = logsumexp(x) - x_y.  fwd writes loss_out [1], parts_out [6] = the four channel
 * losses, ce, 0; sums_out [18] = [c][4] combo sums, sum w_y, sum w_y nll (what bwd reads).  Sums in fp64 through a fixed tree:
 * deterministic.  The 4-pixel form (16-byte logit loads) runs where HW % 4 == 0 and the planes are aligned, the one-pixel form
 * otherwise.  dh_xbd_adapt_loss_grid_pass: the lanes of one forward grid pass (pixels in the one-pixel form, quads in the other).
 * bwd: dlogits [B][4][HW] = upstream * (cw_c * combo gradient + ce_weight * w_y / (sum w_y) * (softmax(x)_c - [c == y])),
 * upstream_dev a device scalar or NULL for 1.  Refused (nothing is launched): a null pointer, an empty input, logits or dlogits
 * that are not 4-byte aligned, a workspace smaller than dh_xbd_adapt_loss_workspace_size answers or not 8-byte aligned. */
int dh_xbd_adapt_loss_workspace_size(long* bytes);
int dh_xbd_adapt_loss_grid_pass(void);
int dh_xbd_adapt_loss_fwd(const float* logits, const unsigned char* msk, int B, long HW, const float* weights_dev,
                          float dice_weight, float focal_weight, float ce_weight, float* sums_out, float* parts_out,
                          float* loss_out, void* workspace, long workspace_bytes, void* stream);
int dh_xbd_adapt_loss_bwd(const float* logits, const unsigned char* msk, const float* sums, const float* weights_dev,
                          const float* upstream_dev, float dice_weight, float focal_weight, float ce_weight, int B, long HW,
                          float* dlogits, void* stream);

/* ---- loader of xBD_code/train_adapt.py (TrainData lines 97-184, ValData 196-245; csrc/xbd_adapt.hip) -------------------
 * One launch per batch.  pre, post [n_src][H][W][3] uint8, pre_mask and post_label [n_src][H][W] uint8, resident.  Output sample
 * n takes source idx[n] and the S x S window at origins[n] = {x0, y0} (origins NULL: every window at (0, 0)); both are clamped
 * into the sources, so nothing outside them is read whatever the tables hold.  out_img fp32 [N][6][S][S] =
 * preprocess_inputs(concat(pre, post)) = x / 127 - 1; out_msk uint8 [N][4][S][S], 0 / 1, from the post label byte l:
 * m1 = (l == 1), m2 = (l == 2), m3 = (l == 3 or l == 4), and m0 = m1 | m2 | m3 in mode 0 (TrainData: the pre mask is cleared and
 * not read, pre_mask may be NULL) or pre_mask > 127 in mode 1 (ValData); out_lbl uint8 [N][S][S] = argmax(m1, m2, m3): 1 where
 * l == 2, 2 where l is 3 or 4, else 0.  A label byte above 4 sets no plane.  16-byte image stores and dword mask stores where
 * S % 4 == 0 and the outputs are aligned, byte stores otherwise; the same bytes either way.
 * Refused (nothing is written): a null pointer other than origins (and pre_mask in mode 0), mode outside {0, 1}, N outside
 * 1..65535, n_src < 1, S < 1, S > H, S > W, H * W >= 2^31. */
int dh_xbd_adapt_batch_u8(const unsigned char* pre, const unsigned char* post, const unsigned char* pre_mask,
                          const unsigned char* post_label, const int* idx, const int* origins, int N, int n_src, int H, int W,
                          int S, int mode, float* out_img, unsigned char* out_msk, unsigned char* out_lbl, void* stream);

/* ---- xBD validation count (xBD_code/train.py:258-279; csrc/xbd_eval.hip) -------------------------------
 * One pass over logits [B][5][H][W] fp32: s = sigmoid in fp32, loc = s[0] > thr (strict, in float32), pred = argmax(s[1:]) * loc
 * with the first maximum of the fp32 sigmoids winning.  msk0: image j's ground-truth localisation plane [H][W] (nonzero = set) at
 * msk0 + j * msk0_image_stride bytes (5 * H * W reads channel 0 of a [B][5][H][W] mask in place); lbl [B][H][W]: classes 0 .. 3.
 * image_counts [B][3] = |gt0|, |loc|, |gt0 & loc| is WRITTEN; class_counts [4][3] = tp, fn, fp of each class is ACCUMULATED over the selected
 * pixels: select 0 = the reference's boolean index by the first row (row r with all its columns iff lbl[j][0][r] > 0; needs
 * H == W), select 1 = pixel p iff msk0[j][p] > 0.  All counting is integer: exact, independent of the order of the sums.
 * Refused (nothing is written): a null pointer, B < 1, thr outside (0, 1), select 0 with H != W, H * W >= 2^31. */
int dh_xbd_val_count(const float* logits, const unsigned char* msk0, long msk0_image_stride, const unsigned char* lbl, int B,
                     int H, int W, float thr, int select, long long* image_counts, long long* class_counts, void* stream);
/* dh_xbd_val_count for n_damage damage classes: logits [B][n_damage + 1][H][W], lbl classes 0 .. n_damage - 1, class_counts
 * [n_damage][3].  n_damage 4 is dh_xbd_val_count; 3 is the pass of xBD_code/train_adapt.py:262-280, whose net has four outputs
 * (destroyed merged with class 3).  Refused besides what dh_xbd_val_count refuses: n_damage outside {3, 4}. */
int dh_xbd_val_count_n(const float* logits, const unsigned char* msk0, long msk0_image_stride, const unsigned char* lbl,
                       int n_damage, int B, int H, int W, float thr, int select, long long* image_counts,
                       long long* class_counts, void* stream);
/* The same pass for a whole grid of localisation thresholds: thr is a HOST pointer to T float32 values, 1 <= T <= 64, each
 * inside (0, 1), strictly ascending; they are read during the call and travel by value in the kernel's arguments (a recorded
 * graph owns its copy; there is no device table).  Per pixel: bin = the number of k with s0 > thr[k] (strict, float32), 0 .. T;
 * arg = the first maximum of the fp32 sigmoids of channels 1 .. 4, 0 .. 3; g0 = msk0 != 0; t = min(lbl, 4) (a label above 3 is
 * "other": never a tp or fn, an fp of the predicted class, as dh_xbd_val_count's comparisons have it).  Same sigmoid, loads
 * and selection code as dh_xbd_val_count, so loc = (bin > k) is that call's s0 > thr[k] bit for bit.
 * image_hist [B][T + 1][4][2], indexed [j][bin][arg][g0] over every pixel of image j, is WRITTEN (cleared by a kernel, no memset
 * node); class_hist [T + 1][4][5], indexed [bin][arg][t] over the selected pixels, is ACCUMULATED.  All integer, exact.
 * Refused (nothing is launched or written): whatever dh_xbd_val_count refuses, thr NULL, T outside 1..64, a threshold outside
 * (0, 1) or NaN, thresholds that do not ascend strictly. */
int dh_xbd_val_sweep(const float* logits, const unsigned char* msk0, long msk0_image_stride, const unsigned char* lbl, int B,
                     int H, int W, const float* thr, int T, int select, long long* image_hist, long long* class_hist,
                     void* stream);

/* ---- xBD prediction: the 4-flip test-time augmentation (xBD_code/predict_test_cls.py:60-94; csrc/xbd_predict.hip) ----------
 * flip_0 = identity, flip_1 reverses the rows, flip_2 the columns, flip_3 both (each its own inverse).
 * dh_xbd_tta_pack_u8: pre, post [N][H][W][3] uint8 -> inp [4N][6][H][W] fp32, inp[4n + k] = flip_k(concat(pre_n, post_n)) with
 * every byte v normalised as (float)v / 127.f - 1.f (both operations rounded to float32).  bgr != 0 reverses each image's RGB
 * triple (what cv2.imread gives the reference script), bgr == 0 keeps the stored order.  Every byte of inp is written.
 * dh_xbd_tta_merge_u8: logits [4N][5][H][W] fp32 -> out [N][H][W][5] uint8 (channels last):
 *   s_k = sigmoid(logits[4n + k]) in fp32, u_k = flip_k(s_k), mean = (((u_0 + u_1) + u_2) + u_3) / 4 in fp32, added in that
 *   order (numpy's float32 mean over the stack), out = uint8(trunc(float32(mean * 255))).  A NaN logit gives 0 (the
 *   reference's astype of a NaN is undefined).  Every byte of out is written.
 * Both launch one kernel and nothing else (no memset or copy node in a recorded step).  pre / post / out may start at any byte;
 * pointers that are not aligned to their vector, or a W that is no multiple of 4, take a scalar path with the same result.
 * Refused (nothing is written): a null pointer, N < 1, 4 N > 65535, H < 1, W < 1, H * W >= 2^31. */
int dh_xbd_tta_pack_u8(const unsigned char* pre, const unsigned char* post, int N, int H, int W, int bgr, float* inp,
                       void* stream);
int dh_xbd_tta_merge_u8(const float* logits, int N, int H, int W, unsigned char* out, void* stream);

/* ---- xBD prediction for M snapshots and V = 4 or 8 views (predict_test_cls.py:38-55, 81-91; csrc/xbd_ensemble.hip) ---------
 * view_v = flip_v for v < 4; view_{4+k}(x)[c][i][j] = flip_k(x)[c][j][i], the transpose of flip_k: with V = 8 the eight
 * symmetries of the square, each once.  Undoing view 4 + k on an output s is flip_k(transpose(s)).  V = 8 needs H == W.
 * dh_xbd_tta_pack_views_u8: pre, post [N][H][W][3] uint8 -> inp [V N][6][H][W] fp32, inp[V n + v] = view_v(concat(pre_n, post_n)),
 *   bytes normalised and `bgr` as in dh_xbd_tta_pack_u8; with V = 4 the same bytes as that call.
 * dh_xbd_tta_merge_multi_u8: logits_host_table is a HOST array of M device pointers, each to one model's contiguous
 *   [V N][5][H][W] fp32 logits; the entry reads and checks the table and hands the pointers to the kernel by value.
 *   u_{m,v} = un-view_v(sigmoid(logits_m[V n + v])) in fp32; t = (((u_{0,0} + u_{0,1}) + ...) + u_{M-1,V-1}), model-major and
 *   view-minor, one fp32 add after the other (numpy's float32 mean over the script's stack); mean = t / (float)(M V), a true
 *   division; out [N][H][W][5] uint8 = uint8(trunc(float32(mean * 255))), channels last; a NaN gives 0.  With M = 1 and V = 4
 *   the same bytes as dh_xbd_tta_merge_u8.
 * Both work on 32 x 32 pixel tiles staged in LDS (row pitch 33 floats), so the transposed views are read and written as row
 * segments too; both launch one kernel and nothing else and write every byte of their output.  pre / post / out may start at any
 * byte; pointers not aligned to their vector, or a W that is no multiple of 4, take a scalar path with the same result.
 * Refused (nothing is written): a null pointer or table entry, V not 4 or 8, N < 1, V N > 65535, H < 1, W < 1, H * W >= 2^31,
 * V = 8 with H != W, M outside 1..8, a float pointer that is not 4-byte aligned. */
int dh_xbd_tta_pack_views_u8(const unsigned char* pre, const unsigned char* post, int N, int H, int W, int bgr, int V, float* inp,
                             void* stream);
int dh_xbd_tta_merge_multi_u8(const float* const* logits_host_table, int M, int V, int N, int H, int W, unsigned char* out,
                              void* stream);

/* ---- xBD damage map and the 4-panel visual grid (xBD_code/visualize_results.py:204-220; csrc/xbd_visual.hip) ---------------
 * msk [N][H][W][5] uint8, channels last: what dh_xbd_tta_merge_u8 writes.  All integer.
 *   class: dmg = 1 + index of the first maximum of msk[1..4] (a tie goes to the lowest channel): 1 .. 4.
 *   rule (use_loc != 0): keep = m0 >= b0 || (m0 >= b1 && 1 < dmg < 4) || (m0 >= b2 && dmg > 1) with m0 = msk[0]; the class is
 *     keep ? dmg : 0.  b_i is the smallest byte v with v / 255 > the script's _thr[i] in float64, 256 if there is none; the caller
 *     derives it.  use_loc == 0 applies no rule (the script as executed); the b_i are range-checked all the same.
 *   colour: class 0 .. 4 -> RGB (0,0,0), (0,255,0), (255,255,0), (255,127,0), (255,0,0); any other byte -> (255,0,255).
 * dh_xbd_damage_map_u8: out [N][H][W] uint8 = the class.
 * dh_xbd_vis_grid_u8: pre, post [N][H][W][3] uint8, gt [N][H][W] uint8 -> grid [N][H][4W][3] uint8, RGB as pre and post store it:
 *   columns [0, W) pre, [W, 2W) post, [2W, 3W) colour(gt), [3W, 4W) colour(class).  The class is computed in registers; no class
 *   map is written.  (The script's BGR array is this one with the last axis reversed.)
 * Both launch one kernel and nothing else and write every byte of their output.  Every pointer may start at any byte; sources
 * that are not 16-byte aligned, an output not aligned to its vector store or a W that is no multiple of 4 (grid) take a
 * pixel-by-pixel path with the same result.
 * Refused (nothing is written): a null pointer, N < 1, H < 1, W < 1, H * W >= 2^31, a bound outside 0..256 and, for the grid,
 * 4 * W * 3 * H >= 2^31. */
int dh_xbd_damage_map_u8(const unsigned char* msk, int N, int H, int W, int use_loc, int b0, int b1, int b2, unsigned char* out,
                         void* stream);
int dh_xbd_vis_grid_u8(const unsigned char* pre, const unsigned char* post, const unsigned char* gt, const unsigned char* msk,
                       int N, int H, int W, int use_loc, int b0, int b1, int b2, unsigned char* grid, void* stream);

/* ---- xBD buildings: connected components, statistics, vote and the painted map (csrc/xbd_buildings.hip) ----------------------
 * Beyond the reference (which stops at pixels).  All integer, bit-exact, independent of launch order and scheduling.
 * dh_xbd_cc_label: key [N][H][W] uint8 -> labels [N][H][W] int32, count [N] int32.  Two pixels that are neighbours (conn 4:
 *   left / right / up / down; conn 8: and the diagonals) belong together when both keys are nonzero (keyed == 0), or nonzero and
 *   equal (keyed == 1).  labels is 0 where key == 0, elsewhere 1 .. K_n per image, the components numbered in raster order of
 *   their first pixel (minimum linear index): scipy.ndimage.label's numbering; count[n] = K_n.  Images are independent.
 *   Union-find with union-by-minimum-index in six launches, their number and grids fixed by the shape: a tile pass in LDS
 *   (dh_xbd_cc_tile_h() x dh_xbd_cc_tile_w() pixels per workgroup), a pass that unites across tile borders with agent-scope
 *   atomicMin (parents read with agent-scope relaxed atomic loads), a flatten pass that also counts the roots per block of 1024
 *   pixels, a one-workgroup-per-image scan of those counts, root ids, and the write of every label.  No workgroup waits for
 *   another and nothing is read back to the host: the sequence can be captured in a graph.
 *   ws: the caller's workspace of at least 4 N (H W + ceil(H W / 1024)) bytes (dh_xbd_cc_ws_bytes writes that number to
 *   *bytes, a host pointer), 4-byte aligned
 *   (parents [N][H W] int32, then block counts); its content before and after the call is meaningless, nothing needs clearing.
 * dh_xbd_cc_stats: labels, vote [N][H][W] uint8, cap >= 1 -> table [N][cap][10] int32; row i describes label i + 1:
 *   area, h0 .. h4 (pixels with vote == 0 .. 4; a vote byte above 4 counts in area only), y0, x0, y1, x1 (inclusive box).
 *   A row whose label does not exist is area = 0, h = 0, y0 = H, x0 = W, y1 = x1 = -1.  Labels above cap (or below 1) are
 *   ignored.  Two launches: one writes every int of the table, one accumulates with integer atomics (add, min, max), reduced
 *   per wave and label with ballots and per workgroup (one tile of the local pass) in LDS before the table is touched.
 * dh_xbd_cc_vote: table, min_area >= 0, mode -> cls [N][cap] uint8.  mode 0 (damage): 1 + the first maximum of h1 .. h4, 0 when
 *   all four are zero; mode 1 (all): the first maximum of h0 .. h4.  A tie goes to the lowest class.  A row with area == 0 or
 *   area < min_area gets 0.  One launch.
 * dh_xbd_cc_paint: out [N][H][W] uint8 = cls[n][l - 1] for a pixel with label l, 0 when l < 1 or l > cap.  One launch, every byte
 *   written.
 * key, vote, cls and out may start at any byte; labels, count, table and ws are 4-byte aligned.
 * Refused (nothing is written, non-zero, dh_last_error begins with xbd_cc_label / xbd_cc_stats / xbd_cc_vote / xbd_cc_paint):
 * a null pointer, N < 1, N > 65535, H < 1, W < 1, H * W >= 2^31, conn outside {4, 8}, keyed or mode outside {0, 1}, cap < 1,
 * cap > 2^24, N * cap > 2^28, min_area < 0, ws_bytes below the query, a misaligned int32 pointer.  dh_xbd_cc_ws_bytes refuses
 * the same shapes (its message begins with xbd_cc_ws_bytes). */
int dh_xbd_cc_tile_h(void);
int dh_xbd_cc_tile_w(void);
int dh_xbd_cc_ws_bytes(int N, int H, int W, long* bytes);
int dh_xbd_cc_label(const unsigned char* key, int N, int H, int W, int conn, int keyed, int* labels, int* count, void* ws,
                    long ws_bytes, void* stream);
int dh_xbd_cc_stats(const int* labels, const unsigned char* vote, int N, int H, int W, int cap, int* table, void* stream);
int dh_xbd_cc_vote(const int* table, int N, int cap, int min_area, int mode, unsigned char* cls, void* stream);
int dh_xbd_cc_paint(const int* labels, const unsigned char* cls, int N, int H, int W, int cap, unsigned char* out, void* stream);

/* ---- xBD buildings: two label maps matched by IoU (csrc/xbd_buildings.hip) ---------------------------------------------------
 * dh_xbd_cc_match: labels_a (the predicted buildings, labels 1 .. cap_a) and labels_b (the true ones, 1 .. cap_b), both
 *   [N][H][W] int32 as dh_xbd_cc_label writes them; a label below 1 or above its cap is background on that side.  Images are
 *   independent.  For a label a: area(a) = pixels with A == a; inter(a, b) = pixels with A == a and B == b;
 *     maj(a)   = the b >= 1 with 2 inter(a, b) > area(a), 0 when there is none;
 *     inter    = inter(a, maj), maj_area = area_B(maj), both 0 when maj == 0;
 *     match(a) = maj if inter * iou_den > iou_num * (area + maj_area - inter) (strict, in 64-bit integers), else 0.
 *   1 <= iou_num <= iou_den <= 32768 and 2 iou_num >= iou_den: above one half a match is one-to-one with no tie rule (the
 *   shared pixels are more than half of a and more than half of b).
 *   -> match_a [N][cap_a][5] int32, row i describes label i + 1 of A: area, maj, inter, maj_area, match;
 *      match_b [N][cap_b] int32: the label of A matched to label j + 1 of B, or 0.
 *   Rows of labels that do not exist are all 0.  Every int of both outputs is written by every call.
 *   No table of pairs and no hash: with NB = bit_length(cap_b) <= 25, a first pass over the pixels counts per label a its area
 *   and, for every bit k < NB, its pixels whose B label has bit k set (and the areas of B); cand(a) = OR_k (2 ones_k > area) << k
 *   is maj(a) whenever maj(a) != 0 (each set bit of maj is counted more than area / 2 times, each clear bit fewer) and anything
 *   otherwise, so a second pass over the pixels counts inter(a, cand(a)) and the candidate stands only if that is more than half
 *   of the area.  Five launches whose number and grids depend on the shapes alone (zero, count, candidate, verify, decide); the
 *   pixel passes reduce per wave and label with ballots and per workgroup in LDS, as dh_xbd_cc_stats does, and sum across
 *   workgroups with agent-scope integer atomics.  No workgroup waits for another; the same bits on every run.
 *   ws: the caller's workspace of at least 4 N (cap_a (NB + 3) + cap_b) bytes (dh_xbd_cc_match_ws_bytes writes that number to
 *   *bytes, a host pointer), 4-byte aligned; every word that is read is written first by the same call, so nothing needs clearing
 *   and the sequence replays from a captured graph.  All five device pointers are 4-byte aligned.
 * Refused (nothing is written, non-zero, dh_last_error begins with xbd_cc_match): a null pointer, N < 1, N > 65535, H < 1, W < 1,
 * H * W >= 2^31, a cap < 1 or > 2^24, N * cap > 2^28 (either cap), iou_num < 1, iou_num > iou_den, iou_den > 32768,
 * 2 iou_num < iou_den, a misaligned pointer, ws_bytes below the query.  dh_xbd_cc_match_ws_bytes refuses the same N and caps. */
int dh_xbd_cc_match_ws_bytes(int N, int cap_a, int cap_b, long* bytes);
int dh_xbd_cc_match(const int* labels_a, const int* labels_b, int N, int H, int W, int cap_a, int cap_b, int iou_num, int iou_den,
                    int* match_a, int* match_b, void* ws, long ws_bytes, void* stream);

/* ---- xBD masks: square-window morphology, the dilated training masks, hole filling (csrc/xbd_morph.hip) -----------------------
 * All integer, bit-exact.  k is the side of the square window: odd, 1 .. 31; r = k / 2.
 * dh_xbd_morph_u8: src [N][H][W] uint8 (nonzero = set) -> dst [N][H][W] uint8, 0 / 1.
 *   op 0 (dilate): dst = 1 where any pixel of the k x k window centred on it is set, everything outside the image clear:
 *     scipy.ndimage.binary_dilation(a, structure=ones((k, k))), skimage.morphology.dilation(a, square(k)).
 *   op 1 (erode): dst = 1 where every pixel of the window is set, everything outside the image SET:
 *     binary_erosion(a, structure=ones((k, k)), border_value=1), skimage's erosion.
 *   One launch.  A workgroup owns a dh_xbd_morph_tile_h() x dh_xbd_morph_tile_w() tile of dst and stages it with its halo in LDS,
 *   four pixels to a dword; the window is separable (rows, then columns) and each pass doubles (widths 1, 2, 4, .. then the two
 *   overlapping windows that make k), so the cost grows with log k.  Erosion is the dilation of the complement (De Morgan).
 * dh_xbd_msk_dilate_u8: msk [N][5][H][W] uint8 mask channels (dh_xbd_augment_u8's out_msk; nonzero = set) -> out [N][5][H][W],
 *   0 / 1: with d_c = dilate(msk[c], k) for c = 1 .. 4 (channel 0 is not read), the priority rule of
 *   xBD_code/train_unettransformer.py:262-273,
 *     out[2] = d2, out[3] = d3 & ~d2, out[4] = d4 & ~d2 & ~d3, out[1] = d1 & ~(d2 | d3 | d4), out[0] = out[1] | .. | out[4].
 *   One launch of the same kernel: the four channels are four bit planes of the staged byte.
 * dh_xbd_fill_holes_u8: src [N][H][W] uint8 (nonzero = set) -> dst [N][H][W] uint8, 0 / 1: src != 0, plus every component of
 *   src == 0 (background connectivity 4 or 8) that has no pixel on the image border:
 *   scipy.ndimage.binary_fill_holes(a, structure=generate_binary_structure(2, 1 for 4, 2 for 8)).
 *   Nine launches whatever the data, nothing read back: the key src == 0 and the cleared marks, dh_xbd_cc_label's six, one thread
 *   per border pixel that stores mark[label] = 1 (plain byte stores of one value: no atomic, no order), the write of dst.  The
 *   marks are bytes [N][H W + 1] indexed by the label, so there is no cap on the number of holes.
 *   ws: the caller's workspace of at least dh_xbd_fill_holes_ws_bytes bytes (written to *bytes, a host pointer), 4-byte aligned:
 *   labels and count, the labelling's workspace, the key and the marks.  Nothing needs clearing; the sequence replays from a
 *   captured graph.
 * Any H, W >= 1; W % 4 == 0 with 4-byte aligned pointers takes dword loads and stores, anything else goes byte by byte with the
 * same result.  Every output byte is written and nothing outside the source is read.
 * Refused (nothing is written, non-zero, dh_last_error begins with xbd_morph / xbd_msk_dilate / xbd_fill_holes): a null pointer,
 * N < 1, N > 65535, H < 1, W < 1, H * W >= 2^31, an even k or one outside 1 .. 31, op outside {0, 1}, background outside {4, 8},
 * an output that overlaps its input, a misaligned or short workspace. */
int dh_xbd_morph_tile_h(void);
int dh_xbd_morph_tile_w(void);
int dh_xbd_morph_u8(const unsigned char* src, int N, int H, int W, int k, int op, unsigned char* dst, void* stream);
int dh_xbd_msk_dilate_u8(const unsigned char* msk, int N, int H, int W, int k, unsigned char* out, void* stream);
int dh_xbd_fill_holes_ws_bytes(int N, int H, int W, long* bytes);
int dh_xbd_fill_holes_u8(const unsigned char* src, int N, int H, int W, int background, unsigned char* dst, void* ws,
                         long ws_bytes, void* stream);

/* ---- xBD class table: the bytes of every class in every resident label (csrc/xbd_classes.hip) --------------------------------
 * dh_xbd_class_table_u8: labels [n][hw] uint8, contiguous (the pipeline's post_label stack, or a slice of it: no alignment is
 * asked of the pointer or of hw) -> counts [n][6] int32: columns 0 .. 4 the number of bytes of file f equal to 0 .. 4, column 5
 * the number above 4; a row sums to hw.  `file_classes` of xBD_code/train.py:397-407 and train_unettransformer.py:499-506
 * (fl[c - 1] = c in msk1) is counts[:, 1:5] > 0.  All 6 n words are written whatever they held: a memset node on the stream
 * clears them, then one launch adds.  A workgroup counts dh_xbd_class_table_chunk() bytes of one file: the bytes in front of the
 * first 16-byte aligned address and behind the last whole piece one by one, the body with 16-byte loads; counts are kept in
 * 32-bit registers (never in packed narrow lanes), summed across the wave and then across the workgroup through LDS, and reach
 * memory as at most one integer atomic per class and workgroup.  Integer adds only: exact, and the same bits on every call.
 * Nothing outside labels is read and labels is not written.
 * Refused (nothing is written, non-zero, dh_last_error begins with xbd_class_table): a null pointer, n < 1, hw < 1,
 * hw > 2^31 - 1. */
int dh_xbd_class_table_chunk(void);
int dh_xbd_class_table_u8(const unsigned char* labels, long n, long hw, int* counts, void* stream);

/* ---- the change-detection evaluator's picture (models/evaluator.py:118-131; csrc/cd_visual.hip) ------------------------------
 * dh_cd_eval_vis_u8: A, B [N][3][H][W] fp32 (as the net receives them), logits [N][C][H][W] fp32, label [N][H][W] int64 ->
 * out [4 * rows * H][cols * W][3] uint8 RGB, cols = min(8, N), rows = ceil(N / cols) (make_grid, padding 0): four bands of
 * rows * H lines, image n at tile (n / cols, n % cols) of each:
 *   A and B: t = x * 0.5f + 0.5f in fp32, clipped to [0, 1], byte = trunc(t * 255) (the float64 product's truncation);
 *   prediction: 255 on all three channels where dh_argmax_nchw's class (first maximum, a later one only if strictly greater)
 *     is >= 1, else 0;  ground truth: 255 where label >= 1, else 0.  A tile position >= N is 0 in all four bands.
 * One kernel and nothing else; it writes every byte of out.  W % 4 == 0 with A, B, logits, label 16-byte aligned and out 4-byte
 * aligned takes 16-byte loads and dword stores; anything else goes pixel by pixel with the same result.  A NaN paints 0.
 * Refused (nothing is written): a null pointer, N < 1, C < 1, H < 1, W < 1, H * W >= 2^31, 2^31 or more units of 1024 pixels. */
int dh_cd_eval_vis_u8(const float* A, const float* B, const float* logits, const long long* label, int N, int C, int H, int W,
                      unsigned char* out, void* stream);

/* ---- whole-tile change maps (dahitra_amd/tiles.py TilePlan; csrc/cd_tile.hip) ------------------------------------------------
 * dh_cd_tile_stitch: logits [P][C][h][w] fp32, the net's answer to the P = ny * nx * nf views of one H x W tile, view
 * p = (iy * nx + ix) * nf + f the window at (ys[iy], xs[ix]) under flip code flips[f] (bit 0: rows reversed, bit 1: columns
 * reversed), still flipped -> out_logits [C][H][W] fp32 (or NULL) and out_mask [H][W] uint8.  Per pixel (Y, X) and class, over
 * the covering iy ascending, ix ascending, f in table order: ly = Y - ys[iy], lx = X - xs[ix], g = wy[ly] * wx[lx],
 * v = the view's element at (bit 0 ? h - 1 - ly : ly, bit 1 ? w - 1 - lx : lx), acc = acc + g * v, ws = ws + g, each operation
 * rounded to fp32 on its own (no fused multiply-add); out = acc / ws, correctly rounded.  out_mask is dh_argmax_nchw's rule on
 * out (first maximum).  One thread per pixel (or per 4 columns) gathers: no floating-point atomics, the same bits on every run.
 * Tables, all in DEVICE memory and trusted as the plan built them: ys [ny], xs [nx] ascending origins with origin + window
 * inside the tile; flips [nf] codes 0 .. 3; wy [h], wx [w]; row_cover [H][2] = (first iy, count) of the windows over a row,
 * col_cover [W][2] the same per column.  x_align: 4 states that W, w and every xs[ix] are multiples of 4 (then, with logits and
 * out_logits 16-byte and out_mask / label 4-byte aligned, a thread takes 4 columns with 16-byte loads and stores), else 1.
 * label [H][W] uint8 with counts [C][C] int64 (both or neither): counts[label * C + class] += 1 per pixel, a label >= C counts
 * nowhere.  label_index (device int, or NULL): label is then [S][H][W] and plane label_index[0] is read, so that a recorded
 * graph follows the tile it is aimed at.
 * Refused (nothing is launched): a null pointer among the required ones, label without counts or the reverse, C outside
 * 1 .. 8, a window larger than the tile, H * W >= 2^31, P != ny * nx * nf, nf outside 1 .. 4, x_align not 1 or 4.
 * dh_cd_view_counts: logits [P][C][h][w] fp32, labels [P][h][w] uint8 -> counts [P][C][C] int64,
 * counts[p][label * C + class] += 1 with the same arg-max rule: P confusion matrices in one launch.  Refused: a null pointer,
 * C outside 1 .. 8, P outside 1 .. 65535, an empty view, h * w >= 2^31. */
int dh_cd_tile_stitch(const float* logits, int P, int C, int h, int w, const int* ys, int ny, const int* xs, int nx,
                      const int* flips, int nf, const float* wy, const float* wx, const int* row_cover, const int* col_cover,
                      int x_align, int H, int W, float* out_logits, unsigned char* out_mask, const unsigned char* label,
                      const int* label_index, long long* counts, void* stream);
int dh_cd_view_counts(const float* logits, const unsigned char* labels, int P, int C, int h, int w, long long* counts,
                      void* stream);

/* ---- xBD losses: the Lovasz, Jaccard and BCE terms of xBD_code/losses.py's ComboLoss (csrc/xbd_seg_losses.hip) --------------
 * x fp32 [B][C][HW]; target of the same shape, fp32 (target_kind 0) or uint8 (target_kind 1); n = B * C * HW.
 * dh_xbd_lovasz_fwd: lovasz_hinge / lovasz_sigmoid (losses.py:129-225) of every channel, and its gradient, in one call.
 *   mode 0: hinge on logits, e = fl32(1 - x (2 t - 1)), weight max(e, 0); mode 1: e = |t - x| on probabilities x; mode 2: the same
 *   on p = 1 / (1 + expf(-x)), the gradient taken through p (1 - p).
 *   per_image 0: one segment per channel over the whole batch (segment c); per_image 1: one per plane (segment b * C + c), a
 *   channel's loss the mean over its B images, an image without a valid element counting 0.
 *   ignore: -1, or the target value (0 .. 255) whose elements are dropped: no key, no count, zero gradient.  Any other target
 *   that is neither 0 nor 1 is dropped too and counted in bad_out [1] (int32, may be NULL).
 *   Within a segment the elements are sorted by descending e as floats (+0 == -0), equal errors in flat index order (a stable
 *   least-significant-digit radix sort; dropped elements last, in index order).  With G the segment's ones and c1 / c0 the ones /
 *   zeros up to and including an element: I = G - c1, U = G + c0, g = 1 - I / U for the segment's first element, 1 / U at a
 *   label 1, I / ((U - 1) U) at a label 0, formed in fp64 from the integers.  Segment loss = sum weight * g in fp64 through a
 *   fixed tree.  loss_out [1] = sum_c w_c channel_loss_c with w = seg_weights_dev [C] or 1 when NULL; channel_loss_out [C];
 *   dx_out [B][C][HW] = d loss_out / d x, every element written.  NaN inputs are outside the contract and stay in bounds.
 * dh_xbd_lovasz_order: order_out [n] int32 = the flat indices in sorted order, segment after segment, and nothing else.
 * workspace: dh_xbd_lovasz_workspace_size(n, segments) bytes (segments = C or B * C; *bytes is a host pointer), 16-byte aligned;
 *   every word that is read is written first by the same call.  The launches depend on (n, segments) alone, nothing is read by the
 *   host or allocated, no workgroup waits for another: the call can be recorded in a HIP graph.  The same bits on every call.
 * dh_xbd_lovasz_tile: the elements a workgroup takes per pass.
 * Refused (nothing is launched, non-zero, dh_last_error begins with xbd_lovasz): a null x, target, output or workspace, an empty
 *   input, n > 2^30, more than 256 segments, mode outside 0 .. 2, target_kind or per_image outside {0, 1}, ignore outside
 *   -1 .. 255, a short or misaligned workspace. */
int dh_xbd_lovasz_tile(void);
int dh_xbd_lovasz_workspace_size(long n, int segments, long* bytes);
int dh_xbd_lovasz_fwd(const float* x, const void* target, int target_kind, int B, int C, long HW, int mode, int per_image,
                      int ignore, const float* seg_weights_dev, float* loss_out, float* channel_loss_out, float* dx_out,
                      int* bad_out, void* workspace, long workspace_bytes, void* stream);
int dh_xbd_lovasz_order(const float* x, const void* target, int target_kind, int B, int C, long HW, int mode, int per_image,
                        int ignore, int* order_out, void* workspace, long workspace_bytes, void* stream);
/* The terms that need no sort, per channel over the whole batch, on s = 1 / (1 + expf(-x)) (probs 0: x are logits) or s = x
 * (probs 1: x are probabilities, what the reference's stand-alone classes take) and t = the target's value:
 *   jaccard      1 - (I + 1e-6) / (S + T - I + 1e-6), I = sum s t, S = sum s, T = sum t             (losses.py:36-45)
 *   bce          mean(max(x, 0) - x t + log(1 + exp(-|x|))), x always read as a logit               (StableBCELoss, :70-80)
 *   mask_bceavg  mean(-(t max(log s, -100) + (1 - t) max(log(1 - s), -100)))                        (MaskLoss, :82-92)
 *   dice         1 - (2 I + 1e-6) / (S + T + 1e-6)                                                  (soft_dice_loss, :24-33)
 *   focal        mean over t != 255 of -(1 - pt)^2 log pt, pt on s and t clamped to [1e-6, 1 - 1e-6] (FocalLoss2d, :273-289)
 * dh_combo_loss_* stays the path of ComboLoss's dice and focal; the last two serve the stand-alone classes.
 * fwd: one pass and a finalize launch; sums_out [C][4] = I, S, T, focal's element count (what bwd reads), terms_out [C][5] = the
 * terms in the order above, loss_out [1] = sum_c w_c sum_k weight_k term_kc over the terms whose weight is not 0, w =
 * chan_weights_dev [C] or 1 when NULL.  Sums in fp64 through a fixed tree.  bwd: dx [B][C][HW] = upstream * d loss_out / d x in
 * one pass (upstream_dev a device scalar or NULL for 1); a term whose weight is 0 is not evaluated.
 * workspace: dh_xbd_seg_terms_workspace_size(C) bytes, 8-byte aligned.
 * Refused (nothing is launched): a null pointer, an empty input, C > 65535, target_kind or probs outside {0, 1}, a short
 * workspace. */
int dh_xbd_seg_terms_workspace_size(int C, long* bytes);
int dh_xbd_seg_terms_fwd(const float* x, const void* target, int target_kind, int probs, int B, int C, long HW,
                         const float* chan_weights_dev, float w_jaccard, float w_bce, float w_mask, float w_dice, float w_focal,
                         float* sums_out, float* terms_out, float* loss_out, void* workspace, long workspace_bytes, void* stream);
int dh_xbd_seg_terms_bwd(const float* x, const void* target, int target_kind, int probs, const float* sums,
                         const float* chan_weights_dev, const float* upstream_dev, float w_jaccard, float w_bce, float w_mask,
                         float w_dice, float w_focal, int B, int C, long HW, float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif
