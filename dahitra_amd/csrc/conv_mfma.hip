// C ABI of the MFMA direct convolution (kernel: conv_mfma_impl.h).  The bf16 and fp32 instantiations are compiled in
// separate translation units (conv_mfma_bf16.hip / conv_mfma_f32.hip): each is minutes of device code generation.
#include "conv_mfma_impl.h"

int dh_conv_launch_bf16(const ConvArgs& a, const ConvPlan& p, hipStream_t st);
int dh_conv_launch_f32(const ConvArgs& a, const ConvPlan& p, hipStream_t st);
int dh_conv_launch_x3(const ConvArgs& a, const ConvPlan& p, hipStream_t st);      // conv_mfma_x3.hip
int dh_conv_launch_x6(const ConvArgs& a, const ConvPlan& p, hipStream_t st);      // conv_mfma_x6.hip
int dh_conv_launch_h3(const ConvArgs& a, const ConvPlan& p, hipStream_t st);      // conv_mfma_h3.hip
// K-deep GEMM form of the 1x1 convolutions with >= 64 input channels (conv1x1_gemm.hip)
bool dh_conv1x1_gemm_plan(const ConvArgs& a, int ks, int stride, int dtype, ConvPlan& p);
int dh_conv1x1_gemm_launch(const ConvArgs& a, const ConvPlan& p, hipStream_t st);
// 3x3 stride-1 convolutions with the weights resident in registers, persistent workgroups (conv_wreg.hip)
bool dh_conv_wreg_plan(const ConvArgs& a, int ks, int stride, int dtype, int cus, ConvPlan& p);
int dh_conv_wreg_launch(const ConvArgs& a, const ConvPlan& p, hipStream_t st);

// How the matrix products of fp32 (DH_DTYPE_F32) launches are computed -- per host thread, read at launch time (so a recorded
// graph keeps the form it was captured with):
//   0  exact fp32 on v_mfma_f32_16x16x4_f32 (default);
//   1  split-bf16, two planes (common.h f32x3): three v_mfma_f32_16x16x32_bf16 products per operand pair on (hi, lo) bf16
//      splits formed while staging, unit roundoff 2^-17 -- tensors, accumulation and everything that is not a matrix product
//      stay fp32;
//   2  split-bf16, three planes (f32x6): six products, unit roundoff 2^-23 (convolutions / linears only; weight-gradient
//      launches issued in this mode run form 1).
// Launches whose input-channel count is not a multiple of 32 (the 16-channel space-to-depth stem) or whose planes do not fit
// the LDS (form 2 at stride 2 with 3x3 taps) keep the exact form.
// (DAHITRA_F32_MMA=bf16x3 makes mode 1 the initial value: the whole fp32 test suite can then run on the split form)
// Split-bf16 launches take 16-row tiles for every 3x3 stride-1 layer with enough tiles, not only from 128 input channels on:
// they run one workgroup per CU whatever the tile (the planes), and a 16-row tile stages -- and splits -- the weight tile once
// per 256 pixels instead of once per 128 (bf16x3 step 3043 / 3020 -> 3100 pairs/s same-box; from 64 channels on only: 3064).
// DAHITRA_X_RW4=<min Cin> moves the threshold, 0 switches it off.
static int x_rw4_cin_min() {
    const char* e = getenv("DAHITRA_X_RW4");
    return e ? atoi(e) : 32;
}
// modes: 0 exact fp32 MFMA; 1 split-bf16, two planes / three products (2^-17: the backward of compute_dtype "bf16x3"); 2 split-bf16,
// three planes / six products (2^-23: the forward's fallback); 3 split-fp16, two planes / three products (~2^-21, fp16's range:
// the forward's default).  DAHITRA_F32_MMA sets the thread default (bf16x3 -> 1, bf16x6 -> 2); engines set the mode per pass.
static int f32_mma_env_default() {
    const char* e = getenv("DAHITRA_F32_MMA");
    return e && !strcmp(e, "bf16x3") ? 1 : (e && !strcmp(e, "bf16x6") ? 2 : 0);
}
static thread_local int g_f32_mma_mode = f32_mma_env_default();
extern "C" int dh_set_f32_mma_mode(int mode) {
    DH_REQUIRE(mode >= 0 && mode <= 3, "set_f32_mma_mode: mode %d (0 = exact fp32 MFMA, 1 / 2 = split-bf16 three- / six-product form, 3 = split-fp16 three-product form)", mode);
    g_f32_mma_mode = mode;
    return 0;
}
extern "C" int dh_get_f32_mma_mode(void) { return g_f32_mma_mode; }
// THE tile rule: rows per wavefront (tile height 4 * rw), for the launch and for dh_conv2d_fwd_num_tiles alike.  dtype, and for
// fp32 the thread's current MMA mode, decide; the two bilinear-x4 entry points (up4) run 8-row tiles whatever the shape.
static inline int conv_rw(int dtype, int N, int OH, int OW, int Cin, int ks, int stride, bool up4 = false) {
    static const int cmin = x_rw4_cin_min();
    if (up4) return 2;
    if (cmin && dtype == DH_DTYPE_F32 && g_f32_mma_mode != 0 && Cin % 32 == 0 && Cin >= cmin && ks == 3 && stride == 1 && OH >= 16 &&
        (long)N * dh_cdiv(OH, 16) * dh_cdiv(OW, TW) >= 256)
        return 4;
    return pick_rw(N, OH, OW, Cin, ks, stride);
}
// The ConvArgs every entry point starts from: zero, the shape, whole images, one BatchNorm group on either side, the tile rule
static ConvArgs conv_args(int dtype, int N, int H, int W, int Cin, int OH, int OW, int Cout, int CoutPad, int ks, int stride, int pad,
                          int act, int dil = 1, bool up4 = false) {
    static const int no_remap = getenv("DAHITRA_NO_XCD_REMAP") ? 1 : 0;
    ConvArgs a = {};
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.OH = OH; a.OW = OW; a.Cout = Cout; a.CoutPad = CoutPad;
    a.pad = pad; a.act = act; a.dil = dil;
    a.npix = OH * OW; a.in_npix = H * W;
    a.gate_groups = a.in_groups = 1;
    a.no_xcd_remap = no_remap;
    a.rw = conv_rw(dtype, N, OH, OW, Cin, ks, stride, up4);
    a.tilesX = dh_cdiv(OW, TW); a.tilesY = dh_cdiv(OH, 4 * a.rw);
    return a;
}
// The tap kernel (conv_mfma_impl.h) serves every launch the other families leave.  Split-precision fit: the NPL planes of halo +
// weights (+ the BatchNorm-on-load table) must fit 160 KB of LDS; the widest output tile that does is taken, 16-wide tiles only
// for layers that ARE that narrow (64 -> 128 at stride 2 fits three planes at 16 channels and then takes 165 us where the exact
// fp32 kernel takes 97); where nothing fits the launch runs the exact fp32 family.  DESIGN.md section 5.
static int tap_plan(const ConvArgs& a, int ks, int stride, int dtype, ConvPlan& p) {
    const bool s1d1 = ks == 3 && stride == 1 && a.dil == 1;
    if (!((ks == 3 || ks == 1) && (stride == 1 || stride == 2)) && !(ks == 4 && stride == 1) && !(ks == 2 && stride == 1 && a.phase_mode))
        DH_FAIL("conv_mfma: unsupported kernel %dx%d stride %d", ks, ks, stride);
    if (a.in_scale && !s1d1)
        DH_FAIL("conv_mfma: BatchNorm-on-load is built for 3x3 stride-1 dilation-1 convolutions (got %dx%d s%d d%d)", ks, ks, stride, a.dil);
    p.family = dtype == DH_DTYPE_BF16 ? CONV_TAP_BF16
             : g_f32_mma_mode == 0 || a.Cin % 32 ? CONV_TAP_F32
             : g_f32_mma_mode == 3 ? CONV_TAP_H3 : (g_f32_mma_mode == 2 ? CONV_TAP_X6 : CONV_TAP_X3);
    p.KS = ks; p.STRIDE = stride; p.RW = a.rw; p.DIL = a.dil;
    p.INBN = a.in_scale != nullptr;
    const int esz = dtype == DH_DTYPE_BF16 ? 2 : 4;
    // bytes staged per channel chunk: NPL planes of (haloed input tile + the weights of all taps), the on-load tables
    auto staging = [&](int npl, int nt, bool up4) {
        const int hh = (4 * a.rw - 1) * stride + (ks - 1) * a.dil + 1, hwd = (TW - 1) * stride + (ks - 1) * a.dil + 1;
        return npl * ((size_t)hh * hwd * (stride == 1 ? HaloLayout<1>::PITCH : HaloLayout<2>::PITCH) + (size_t)ks * ks * nt * WPITCH) +
               (p.INBN ? (size_t)2 * a.Cin * sizeof(float) : 0) + (up4 ? (size_t)4 * 6 * 32 * sizeof(float) : 0);
    };
    int npl = p.family == CONV_TAP_X6 ? 3 : (p.family == CONV_TAP_X3 || p.family == CONV_TAP_H3 ? 2 : 1);
    if (ks == 2) {      // the phase convolutions: forward = one cout block (32 or 64 channels) per phase; data gradient: Cout = the 3x3's Cin
        p.NT = (a.phase_mode == 1 ? a.Cout == 128 : a.Cout % 64 != 0) ? 32 : 64;
    } else {
        auto fits = [&](int nt) { return npl == 1 || staging(npl, nt, false) <= (size_t)160 * 1024; };
        p.NT = a.CoutPad % 64 == 0 && fits(64) ? 64 : (a.CoutPad % 32 == 0 && fits(32) ? 32 : (a.CoutPad % 32 != 0 && fits(16) ? 16 : 0));
        if (!p.NT) {
            p.family = CONV_TAP_F32;
            npl = 1;
            p.NT = a.CoutPad % 64 == 0 ? 64 : (a.CoutPad % 32 == 0 ? 32 : 16);
        }
    }
    const int ck = npl > 1 ? 32 : 64 / esz;                 // channels of one 64-byte LDS row
    // layers with 1-2 channel chunks have nothing to pipeline (but split-bf16 forms run one workgroup per CU, so their two-chunk
    // layers prefetch the second chunk under the first one's MFMAs: +2.9 % on the bf16x3 step, same-box)
    p.PF = !(a.rw == 2 && ks == 3 && a.dil == 1 && a.Cin <= 2 * ck && !(npl > 1 && a.Cin == 2 * ck));
    // compact-epilogue instantiation: 16-byte output pieces, no gating / pre-activation copy / GELU
    p.FAST = ((a.Cout % (16 / esz)) == 0 || a.y_nchw) && !a.gate_y && !a.y2 && a.act != DH_ACT_GELU;
    if (a.up4_a && !p.INBN) {
        if (!(s1d1 && p.NT == 32 && a.rw == 2 && !p.PF && esz == 2))
            DH_FAIL("conv_mfma: bilinear x4 on load is built for the bf16 3x3 / stride 1, 32 -> 32 channel convolution on 8-row tiles");
        if (!p.FAST) DH_FAIL("conv_mfma: the bilinear-x4-on-load form has the compact epilogue and no BatchNorm on load");
        p.INUP4 = 1;
    }
    const size_t st = staging(npl, p.NT, p.INUP4), otile = (size_t)4 * 2 * p.NT * 4 + (size_t)4 * a.rw * TW * (p.NT * esz + 16);
    p.lds = (int)(st > otile ? st : otile);                 // (otile: the epilogue's stats scratch + transposed tile)
    p.grid_x = a.N * a.tilesX * a.tilesY;
    p.grid_y = a.CoutPad / p.NT;
    p.threads = 256;
    p.stats_rows = p.grid_x;
    return 0;
}
// The plan of a launch: 1x1 GEMM, then weights-resident stream, then tap kernel, among the families the entry point admits (a bit
// per ConvFamily), under the thread's current modes, for `cus` compute units.  CONV_NO_FAMILY: none serves it (no error text).
// Whatever the family, p.stats_rows equals dh_conv2d_fwd_num_tiles: the stream and the GEMM take whole 8x16 tiles only.
constexpr unsigned CONV_TAP = 0x1f, CONV_WREG = 0x1f << CONV_WREG64, CONV_ANY = ~0u;
constexpr int CONV_NO_FAMILY = -1;
static int conv_plan(const ConvArgs& a, int ks, int stride, int dtype, int cus, unsigned admit, ConvPlan& p) {
    p = ConvPlan{};
    p.tilesX = a.tilesX; p.tilesY = a.tilesY; p.rw = a.rw;
    // ConvArgs::res_bits: the 64 / 128 / 256-channel stream kernels and the tap kernel's compact epilogue at 3x3 / stride 1 apply
    // the mask; no other family reads it, so every other plan is refused rather than served with an unmasked sum
    if (a.res_bits && (!a.res || ks != 3 || stride != 1 || a.phase_mode)) return CONV_NO_FAMILY;
    if ((admit >> CONV_GEMM1X1 & 1) && dh_conv1x1_gemm_plan(a, ks, stride, dtype, p)) return a.res_bits ? CONV_NO_FAMILY : 0;
    if ((admit & CONV_WREG) && dh_conv_wreg_plan(a, ks, stride, dtype, cus, p))
        return a.res_bits && (p.family == CONV_WREG32 || p.family == CONV_WREG32_UP4) ? CONV_NO_FAMILY : 0;
    if (!(admit & CONV_TAP)) return CONV_NO_FAMILY;
    if (int e = tap_plan(a, ks, stride, dtype, p)) return e;
    return a.res_bits && !p.FAST ? CONV_NO_FAMILY : 0;
}
// the CU count the persistent grids are sized for: asked once, 256 where there is no answer
static int device_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    }
    return cus;
}
// Set by dh_conv2d_fwd_describe around its call of an entry point, which then runs its checks and the plan as ever but launches
// nothing: the plan for `cus` compute units goes to out.  CONTRACT: the pointers it passes stand for tensors and lead nowhere, so
// an entry point may test them for null but must neither read through one nor make a HIP call before conv_issue.
struct ConvDescribe { int cus; int* out; };
static thread_local const ConvDescribe* t_describe = nullptr;
// plan, then launch (or describe)
static int conv_issue(const ConvArgs& a, int ks, int stride, int dtype, unsigned admit, void* stream) {
    ConvPlan p;
    if (int e = conv_plan(a, ks, stride, dtype, t_describe ? t_describe->cus : device_cus(), admit, p)) return e;
    if (t_describe) {
        memcpy(t_describe->out, &p, sizeof(p));
        return 0;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (p.family) {
        case CONV_TAP_BF16: return dh_conv_launch_bf16(a, p, st);
        case CONV_TAP_F32: return dh_conv_launch_f32(a, p, st);
        case CONV_TAP_X3: return dh_conv_launch_x3(a, p, st);
        case CONV_TAP_X6: return dh_conv_launch_x6(a, p, st);
        case CONV_TAP_H3: return dh_conv_launch_h3(a, p, st);
        case CONV_GEMM1X1: return dh_conv1x1_gemm_launch(a, p, st);
        default: return dh_conv_wreg_launch(a, p, st);
    }
}

// C ABI: see include/dahitra_hip.h
extern "C" int dh_conv2d_fwd(int dtype, const void* x, const void* w_packed, void* y, const float* bias,
                             const void* residual, float* stats_partial, int N, int H, int W, int Cin,
                             int OH, int OW, int Cout, int CoutPad, int ks, int stride, int pad, int act,
                             int npix_valid, long w_image_stride, void* y_preact, int dilation, const void* gate_out,
                             const void* gate_y, const float* gate_mean, const float* gate_invstd, int gate_groups,
                             const float* in_scale, const float* in_shift, int in_groups, int phase_mode, const void* w_frag,
                             void* stream) {
    const int esz = dtype == DH_DTYPE_BF16 ? 2 : 4;
    DH_REQUIRE(dtype == DH_DTYPE_F32 || dtype == DH_DTYPE_BF16, "conv2d_fwd: bad dtype %d", dtype);
    DH_REQUIRE((Cin * esz) % 64 == 0, "conv2d_fwd: Cin=%d must be a multiple of %d", Cin, 64 / esz);
    DH_REQUIRE(CoutPad % 16 == 0 && CoutPad >= Cout, "conv2d_fwd: CoutPad=%d invalid for Cout=%d", CoutPad, Cout);
    DH_REQUIRE(N > 0 && OH > 0 && OW > 0, "conv2d_fwd: empty output");
    DH_REQUIRE(dilation == 1 || (dilation == 2 && ks == 3 && stride == 1), "conv2d_fwd: dilation %d unsupported here", dilation);
    ConvArgs a = conv_args(dtype, N, H, W, Cin, OH, OW, Cout, CoutPad, ks, stride, pad, act, dilation);
    a.x = x; a.w = w_packed; a.y = y; a.bias = bias; a.res = residual; a.stats = stats_partial; a.y2 = y_preact;
    if (npix_valid > 0) a.npix = a.in_npix = npix_valid;
    a.w_nstride = w_image_stride;
    a.gate_out = gate_out; a.gate_y = gate_y; a.gate_mean = gate_mean; a.gate_invstd = gate_invstd;
    if (gate_groups > 0) a.gate_groups = gate_groups;
    if (gate_y) {
        DH_REQUIRE(stats_partial && gate_mean && gate_invstd && Cout % 4 == 0 && act == DH_ACT_NONE && N % a.gate_groups == 0,
                   "conv2d_fwd: BN-backward gating needs stats_partial, mean/invstd, Cout %% 4 == 0, no activation");
    }
    a.in_scale = in_scale; a.in_shift = in_shift;
    if (in_groups > 0) a.in_groups = in_groups;
    if (in_scale) DH_REQUIRE(in_shift && N % a.in_groups == 0 && w_image_stride == 0,
                             "conv2d_fwd: BatchNorm-on-load needs in_shift and N %% in_groups == 0");
    a.phase_mode = phase_mode;
    a.w_frag = w_frag;
    DH_REQUIRE(!w_frag || (ks == 3 && w_image_stride == 0 && !phase_mode && dtype == DH_DTYPE_BF16 && Cin % 32 == 0 && CoutPad % 16 == 0),
               "conv2d_fwd: fragment-order weights exist for the bf16 3x3 layers only");
    if (phase_mode) {
        DH_REQUIRE(ks == 2 && stride == 1 && pad == 1 && dilation == 1 && (!residual || phase_mode == 1) && !stats_partial && !y_preact && !gate_y &&
                   !in_scale && w_image_stride == 0 && npix_valid == 0 && H == OH && W == OW && act != DH_ACT_GELU,
                   "conv2d_fwd: phase mode is a plain 2x2 pad-1 convolution on equal input / output grids");
        DH_REQUIRE(phase_mode == 1 ? ((Cout == 128 || Cout == 256) && CoutPad == Cout) : (phase_mode == 2 && Cin == 128 && (Cout % 64 == 0 || Cout == 32)),
                   "conv2d_fwd: phase mode %d with Cin=%d Cout=%d", phase_mode, Cin, Cout);
    }
    return conv_issue(a, ks, stride, dtype, CONV_ANY, stream);
}

// 3x3 / stride 1 / pad 1 convolution (bf16) over a channel concatenation that is never materialised, see ConvArgs::x_split /
// y_split: conv_layer2_0 of the hierarchical model reads torch.cat([a_128, b_128], 1) (models/networks.py:1344) -- the two
// temporal streams' stem outputs, which here are the two halves of one [2 N]-image tensor -- and its data gradient writes
// the two halves of that tensor's gradient.  Without this the concatenation and its gradient cost four channel-copy passes
// of 134 MB each per step at batch 32.  x_split_bytes / y_split_bytes: byte distance from the first to the second tensor
// (0: plain tensor on that side).  No bias, residual or activation; stats_partial as dh_conv2d_fwd.  Served by the
// register-resident-weights kernel only: dh_conv3x3_split_supported says whether a shape is (callers fall back to
// dh_copy_channels + dh_conv2d_fwd otherwise).
static ConvArgs split_conv_args(long x_split, const void* w_frag, long y_split, int N, int H, int W, int Cin, int Cout) {
    ConvArgs a = conv_args(DH_DTYPE_BF16, N, H, W, Cin, H, W, Cout, Cout, 3, 1, 1, DH_ACT_NONE);
    a.w_frag = w_frag; a.x_split = x_split; a.y_split = y_split;
    return a;
}
bool dh_wgrad_split_supported(int N, int H, int W, int Cin, int Cout);      // conv_wgrad.hip
extern "C" int dh_conv3x3_split_supported(int N, int H, int W, int Cin, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin % 128 || Cout % 64) return 0;
    ConvPlan p;
    // forward (split input), data gradient (split output, channel counts exchanged); both need the fragment-order weights, of
    // which only the presence is planned: &p stands for them
    if (conv_plan(split_conv_args(16, &p, 0, N, H, W, Cin, Cout), 3, 1, DH_DTYPE_BF16, 256, CONV_WREG, p)) return 0;
    if (conv_plan(split_conv_args(0, &p, 16, N, H, W, Cout, Cin), 3, 1, DH_DTYPE_BF16, 256, CONV_WREG, p)) return 0;
    return dh_wgrad_split_supported(N, H, W, Cin, Cout) ? 1 : 0;
}
extern "C" int dh_conv3x3_split_fwd(const void* x, long x_split_bytes, const void* w_packed, const void* w_frag, void* y,
                                    long y_split_bytes, float* stats_partial, int N, int H, int W, int Cin, int Cout, void* stream) {
    DH_REQUIRE(x && w_packed && y && N > 0 && (x_split_bytes || y_split_bytes), "conv3x3_split_fwd: bad arguments");
    DH_REQUIRE((!x_split_bytes || Cin % 128 == 0) && (!y_split_bytes || Cout % 128 == 0) && x_split_bytes % 16 == 0 && y_split_bytes % 16 == 0,
               "conv3x3_split_fwd: a split side needs a multiple of 128 channels (Cin=%d Cout=%d) and 16-byte aligned tensors", Cin, Cout);
    ConvArgs a = split_conv_args(x_split_bytes, w_frag, y_split_bytes, N, H, W, Cin, Cout);
    a.x = x; a.w = w_packed; a.y = y; a.stats = stats_partial;
    const int e = conv_issue(a, 3, 1, DH_DTYPE_BF16, CONV_WREG, stream);
    if (e == CONV_NO_FAMILY)
        DH_FAIL("conv3x3_split_fwd: %d x %dx%d, %d -> %d channels is outside the register-resident-weights kernel "
                "(dh_conv3x3_split_supported)", N, H, W, Cin, Cout);
    return e;
}

// 3x3 / stride 1 / pad 1 convolution + MASKED residual, y = conv(x) + (bit ? residual : 0) with the bits in res_bits (ConvArgs::
// res_bits: the relu_bits of dh_bn_apply_bits for the [N][H][W][Cout] residual).  The data gradient of conv1 of a residual block
// without a downsample: residual = the gradient of the block's output, res_bits = the ReLU mask of that output -- the masked
// copy of the gradient (dres of dh_bn_bwd*) is then never written.  Same bits as dh_conv2d_fwd with that copy as residual.
// No bias, activation or statistics.  dh_conv3x3_res_bits_supported: 1 where a kernel family applies the mask for this shape
// (and the shape would not otherwise run the 32-channel stream kernel, which does not); callers keep the copy elsewhere.
static ConvArgs res_bits_conv_args(int dtype, const void* w_frag, int N, int H, int W, int Cin, int Cout, int CoutPad) {
    ConvArgs a = conv_args(dtype, N, H, W, Cin, H, W, Cout, CoutPad, 3, 1, 1, DH_ACT_NONE);
    a.w_frag = dtype == DH_DTYPE_BF16 && Cin % 32 == 0 ? w_frag : nullptr;
    return a;
}
extern "C" int dh_conv3x3_res_bits_supported(int dtype, int N, int H, int W, int Cin, int Cout, int CoutPad, int has_frag) {
    const int esz = dtype == DH_DTYPE_BF16 ? 2 : 4;
    if ((dtype != DH_DTYPE_F32 && dtype != DH_DTYPE_BF16) || N <= 0 || H <= 0 || W <= 0 || (Cin * esz) % 64 || CoutPad % 16 ||
        CoutPad < Cout || Cout % (16 / esz))
        return 0;
    ConvPlan p;
    ConvArgs a = res_bits_conv_args(dtype, has_frag ? &p : nullptr, N, H, W, Cin, Cout, CoutPad);     // (&p: presence only)
    a.res = &p; a.res_bits = reinterpret_cast<const unsigned char*>(&p);
    return conv_plan(a, 3, 1, dtype, device_cus(), CONV_WREG | CONV_TAP, p) == 0 ? 1 : 0;
}
extern "C" int dh_conv3x3_res_bits_fwd(int dtype, const void* x, const void* w_packed, const void* w_frag, const void* residual,
                                       const unsigned char* res_bits, void* y, int N, int H, int W, int Cin, int Cout, int CoutPad,
                                       void* stream) {
    const int esz = dtype == DH_DTYPE_BF16 ? 2 : 4;
    DH_REQUIRE(dtype == DH_DTYPE_F32 || dtype == DH_DTYPE_BF16, "conv3x3_res_bits_fwd: bad dtype %d", dtype);
    DH_REQUIRE(x && w_packed && residual && res_bits && y && N > 0 && H > 0 && W > 0, "conv3x3_res_bits_fwd: bad arguments");
    DH_REQUIRE((Cin * esz) % 64 == 0 && CoutPad % 16 == 0 && CoutPad >= Cout && Cout % (16 / esz) == 0,
               "conv3x3_res_bits_fwd: Cin=%d Cout=%d CoutPad=%d", Cin, Cout, CoutPad);
    ConvArgs a = res_bits_conv_args(dtype, w_frag, N, H, W, Cin, Cout, CoutPad);
    a.x = x; a.w = w_packed; a.y = y; a.res = residual; a.res_bits = res_bits;
    const int e = conv_issue(a, 3, 1, dtype, CONV_WREG | CONV_TAP, stream);
    if (e == CONV_NO_FAMILY)
        DH_FAIL("conv3x3_res_bits_fwd: no kernel family applies the residual's mask bytes for %d x %dx%d, %d -> %d channels "
                "(dh_conv3x3_res_bits_supported)", N, H, W, Cin, Cout);
    return e;
}

// The class head (3x3, pad 1, <= 16 classes) with fp32 NCHW logits written by the convolution itself: see ConvArgs::y_nchw.
extern "C" int dh_conv3x3_head_fwd(int dtype, const void* x, const void* w_packed, const float* bias, int N, int H, int W, int Cin,
                                   int Cout, const float* in_scale, const float* in_shift, int in_groups,
                                   float* logits_nchw, void* stream) {
    const int esz = dtype == DH_DTYPE_BF16 ? 2 : 4;
    DH_REQUIRE(dtype == DH_DTYPE_F32 || dtype == DH_DTYPE_BF16, "conv3x3_head_fwd: bad dtype %d", dtype);
    DH_REQUIRE((Cin * esz) % 64 == 0 && Cout >= 1 && Cout <= 16 && logits_nchw && N > 0 && H > 0 && W > 0,
               "conv3x3_head_fwd: Cin=%d Cout=%d", Cin, Cout);
    ConvArgs a = conv_args(dtype, N, H, W, Cin, H, W, Cout, 16, 3, 1, 1, DH_ACT_NONE);
    a.x = x; a.w = w_packed; a.bias = bias;
    a.in_scale = in_scale; a.in_shift = in_shift;
    if (in_groups > 0) a.in_groups = in_groups;
    if (in_scale) DH_REQUIRE(in_shift && N % a.in_groups == 0, "conv3x3_head_fwd: BatchNorm-on-load needs in_shift and N %% in_groups == 0");
    a.y_nchw = logits_nchw;
    return conv_issue(a, 3, 1, dtype, CONV_TAP, stream);
}

// Data gradient of a 3x3 / pad-1 convolution whose INPUT is a bilinear x4 upsampled map (models/networks.py:387-389:
// classifier.0 behind nn.Upsample(4, 'bilinear')), taken straight to the COARSE grid: dy [N][H][W][K] (K = the conv's output
// channels, a multiple of the 64-byte chunk), w_packed = the data-gradient pack [9][32][K]; the kernel reduces every 8x16 tile
// of the fine-grid gradient to the 4 x 6 coarse pixels it touches and writes partial [N * (H/8) * (W/16)][4][6][32] fp32.
// The fine-grid gradient (32 channels x H x W) is never stored.  dh_absdiff_up4_combine finishes (sum of <= 4 tiles, sign).
extern "C" long dh_conv3x3_dgrad_up4_partial_floats(int N, int H, int W) { return (long)N * (H / 8) * (W / 16) * 4 * 6 * 32; }
extern "C" int dh_conv3x3_dgrad_up4(int dtype, const void* dy, const void* w_packed, int N, int H, int W, int K, float* partial,
                                    void* stream) {
    DH_REQUIRE(dtype == DH_DTYPE_BF16, "conv3x3_dgrad_up4: bf16 only (the fp32 mode keeps the two-kernel path)");
    DH_REQUIRE(K % 32 == 0 && H % 8 == 0 && W % 16 == 0 && partial && N > 0, "conv3x3_dgrad_up4: K=%d H=%d W=%d", K, H, W);
    ConvArgs a = conv_args(dtype, N, H, W, K, H, W, 32, 32, 3, 1, 1, DH_ACT_NONE, 1, true);
    a.x = dy; a.w = w_packed;
    a.up4_partial = partial;
    return conv_issue(a, 3, 1, dtype, CONV_TAP, stream);
}

// classifier.0 on the bilinear-x4 upsampled |A - B| map WITHOUT that map (ConvArgs::up4_a; models/networks.py:383-389,
// models/help_funcs.py:9): a, b [N][H / 4][W / 4][32] bf16 (the two streams' decoder outputs), y [N][H][W][32] bf16 =
// act(conv3x3(upsample4(|a - b|)) + bias); stats_partial as dh_conv2d_fwd with dh_conv2d_fwd_num_tiles(DH_DTYPE_BF16, N, H, W, 32, 3, 1) rows.
// The interpolation is dh_absdiff_upsample4_fwd's (same terms, same order, rounded to bf16 as that kernel's output is), so the
// result equals dh_conv2d_fwd on its output bit for bit.
extern "C" int dh_conv3x3_up4_fwd(const void* a, const void* b, const void* w_packed, const float* bias, int act, void* y,
                                  float* stats_partial, int N, int H, int W, void* stream) {
    DH_REQUIRE(a && b && w_packed && y && N > 0 && H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0, "conv3x3_up4_fwd: N=%d H=%d W=%d", N, H, W);
    DH_REQUIRE(act == DH_ACT_NONE || act == DH_ACT_RELU, "conv3x3_up4_fwd: activation %d", act);
    ConvArgs c = conv_args(DH_DTYPE_BF16, N, H, W, 32, H, W, 32, 32, 3, 1, 1, act, 1, true);
    c.w = w_packed; c.y = y; c.bias = bias; c.stats = stats_partial;
    c.up4_a = a; c.up4_b = b;
    // the persistent register-resident-weights stream with the interpolation in LDS (csrc/conv_wreg.hip) where it serves the shape;
    // else (ragged tiles, ReLU, few tiles) the tap kernel with the interpolation on its load path
    return conv_issue(c, 3, 1, DH_DTYPE_BF16, CONV_WREG | CONV_TAP, stream);
}

// number of workgroup tiles along the pixel dimension (= rows of the stats_partial buffer): the tile rule of the launch that will
// WRITE the buffer
extern "C" int dh_conv2d_fwd_num_tiles(int dtype, int N, int OH, int OW, int Cin, int ks, int stride) {
    return N * dh_cdiv(OW, TW) * dh_cdiv(OH, 4 * conv_rw(dtype, N, OH, OW, Cin, ks, stride));
}

// the plan of such a call, for tests and tools (see dahitra_hip.h).  Host only
extern "C" int dh_conv2d_fwd_describe(int entry, int dtype, int N, int H, int W, int Cin, int OH, int OW, int Cout, int CoutPad, int ks,
                                      int stride, int pad, int act, int npix_valid, long w_image_stride, int dilation, int gate_groups,
                                      int in_groups, int phase_mode, int flags, int cus, int* out) {
    static float present[1] = {0.f};        // stands for every tensor: only their presence is planned
    static_assert(sizeof(ConvPlan) == 30 * sizeof(int), "dh_conv2d_fwd_describe documents 30 ints");
    DH_REQUIRE(out && cus > 0, "conv2d_fwd_describe: out missing, or cus=%d", cus);
    const ConvDescribe d{cus, out};
    void* const on = present;
    auto has = [&](int bit) { return flags >> bit & 1 ? present : nullptr; };
    float *res = has(0), *stats = has(1), *preact = has(2), *gate = has(3), *scale = has(4), *frag = has(5);
    const long xs = flags >> 6 & 1 ? 16 : 0, ys = flags >> 7 & 1 ? 16 : 0;
    t_describe = &d;
    int e = 1;
    switch (entry) {
        case 0: e = dh_conv2d_fwd(dtype, on, on, on, present, res, stats, N, H, W, Cin, OH, OW, Cout, CoutPad, ks, stride, pad, act, npix_valid,
                                  w_image_stride, preact, dilation, gate, gate, gate, gate, gate_groups, scale, scale, in_groups, phase_mode,
                                  frag, nullptr); break;
        case 1: e = dh_conv3x3_head_fwd(dtype, on, on, present, N, H, W, Cin, Cout, scale, scale, in_groups, present, nullptr); break;
        case 2: e = dh_conv3x3_split_fwd(on, xs, on, frag, on, ys, stats, N, H, W, Cin, Cout, nullptr); break;
        case 3: e = dh_conv3x3_up4_fwd(on, on, on, present, act, on, stats, N, H, W, nullptr); break;
        case 4: e = dh_conv3x3_dgrad_up4(dtype, on, on, N, H, W, Cin, present, nullptr); break;
        case 5: e = dh_conv3x3_res_bits_fwd(dtype, on, on, frag, on, reinterpret_cast<const unsigned char*>(present), on, N, H, W, Cin, Cout,
                                            CoutPad, nullptr); break;
        default: dh_set_error("conv2d_fwd_describe: entry (0 dh_conv2d_fwd, 1 head, 2 split, 3 up4 fwd, 4 dgrad up4, 5 res_bits fwd)");
    }
    t_describe = nullptr;
    return e;
}
