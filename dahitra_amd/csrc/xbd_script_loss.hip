// Losses of the two xBD training scripts, one source for both:
//   xBD_code/train_unettransformer.py (lines 438-461), the script that trains DAHiTra proper ("unet", five outputs):
//     five ComboLoss{dice:1, focal:8} terms, one per output channel ... xBD_code/losses.py:24-34, 95-126, 273-288
//     + ce_w * CrossEntropyLoss(weight)(out * (lbl > 0), lbl) .......... train_unettransformer.py:445-449, 563-564
//     + the Dice meter of line 460-461 on the MASKED channel 0
//   xBD_code/train_adapt.py (lines 332-342), the four-output DAHiTra fine-tuned on Ida-BD ("adapt"):
//     four ComboLoss terms + ce_w * CrossEntropyLoss(weight)(out, y), y = argmax(1 - m0, m1, m2, m3) ... train_adapt.py:338-340
// The masks are the loader's uint8 bytes (no float copy of them exists), the label is a byte per pixel or is derived from the
// mask bytes in the kernel.  HBM-streaming work: ONE pass over the pixels for all NQ sums (xbd_step.hip's combo kernels make one
// pass per channel), one small finalize launch, and one pass for the gradient.  16-byte logit loads per lane where HW % 4 == 0.
// Every sum is carried in fp64 through a fixed two-stage tree (dh_block_sum_f64's, all NQ sums behind one barrier; then a
// fixed-order finalize), so the results are deterministic.
// A form struct per script holds what differs, and that is four things: the label of a pixel, whether the cross-entropy reads
// the logits masked by y > 0 (unet) or raw (adapt), the meter and bad-label sums, and the tail of parts.
#include "common.h"

namespace {

constexpr int SL_THREADS = 256;
constexpr int SL_MAX_BLOCKS = 1024;       // forward grid cap: one grid pass covers SL_MAX_BLOCKS * SL_THREADS lanes
constexpr int SL_BWD_MAX_BLOCKS = 2048;
constexpr float XEPS = 1e-6f;             // xBD_code/losses.py:12

struct UnetForm {
    static constexpr int NC = 5;
    static constexpr int NQ = 25;         // sums per workgroup: [c][4] combo, sum w_y, sum w_y nll, meter I, meter S, bad labels
    static constexpr int SUMS = 24;       // of which the backward and the caller get the first 24 as floats
    static constexpr int PARTS = 8;       // five channel losses, ce, Dice meter, bad labels
    static constexpr bool MASKED_CE = true, HAS_LBL = true, HAS_METER = true, COUNTS_BAD = true;
    static constexpr const char* FWD = "xbd_unet_loss_fwd";
    static constexpr const char* FINALIZE = "xbd_unet_loss_finalize";
    static constexpr const char* BWD = "xbd_unet_loss_bwd";
    // the label of a pixel: the byte of `lbl`, or ("damage") the first set channel among 1 .. 4 of the mask, 0 if none
    static __device__ __forceinline__ unsigned label(int label_mode, const unsigned char (&t)[5], unsigned char lbl) {
        if (label_mode == 0) return lbl;
        return t[1] ? 1u : t[2] ? 2u : t[3] ? 3u : t[4] ? 4u : 0u;
    }
    // tot[22], tot[23]: the meter's I and S; tot[24]: the labels no class has
    static __device__ __forceinline__ void parts_tail(const double* tot, float* __restrict__ parts) {
        const float mI = (float)tot[22], mS = (float)tot[23], T0 = (float)tot[2];
        parts[6] = (2.f * mI + XEPS) / (mS + T0 + XEPS);      // 1 - soft_dice_loss(sigmoid(masked channel 0), msk[:, 0])
        parts[7] = (float)tot[24];
    }
};

struct AdaptForm {
    static constexpr int NC = 4;
    static constexpr int NQ = 18;         // sums per workgroup: [c][4] combo, sum w_y, sum w_y nll
    static constexpr int SUMS = 18;
    static constexpr int PARTS = 6;       // four channel losses, ce, 0
    static constexpr bool MASKED_CE = false, HAS_LBL = false, HAS_METER = false, COUNTS_BAD = false;
    static constexpr const char* FWD = "xbd_adapt_loss_fwd";
    static constexpr const char* FINALIZE = "xbd_adapt_loss_finalize";
    static constexpr const char* BWD = "xbd_adapt_loss_bwd";
    // torch.argmax(msks, dim=1) after msks[:, 0] = 1 - msks[:, 0] (train_adapt.py:338-339) on the integers the bytes stand for:
    // the FIRST maximum of (1 - t0, t1, t2, t3)
    static __device__ __forceinline__ unsigned label(int, const unsigned char (&t)[4], unsigned char) {
        int best = 1 - (int)t[0];
        unsigned y = 0;
#pragma unroll
        for (int c = 1; c < 4; ++c)
            if ((int)t[c] > best) { best = (int)t[c]; y = (unsigned)c; }
        return y;
    }
    static __device__ __forceinline__ void parts_tail(const double*, float* __restrict__ parts) { parts[5] = 0.f; }
};

__device__ __forceinline__ float sl_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// a[y] for y in 0 .. NC - 1 without a runtime-indexed register array
template <int NC>
__device__ __forceinline__ float sl_sel(const float (&a)[NC], unsigned y) {
    float r = a[0];
#pragma unroll
    for (int c = 1; c < NC; ++c) r = y == (unsigned)c ? a[c] : r;
    return r;
}

// the maximum of the NC logits, in the order of a pairwise tree over the first four
template <int NC>
__device__ __forceinline__ float sl_max(const float (&z)[NC]) {
    static_assert(NC >= 4, "sl_max pairs the first four");
    float mx = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
#pragma unroll
    for (int c = 4; c < NC; ++c) mx = fmaxf(mx, z[c]);
    return mx;
}

// logits, mask bytes and (where the form has one) label byte of V consecutive pixels of image b, starting at pixel p
template <class Form, int V>
struct SlPixels {
    float x[Form::NC][V];
    unsigned char t[Form::NC][V];
    unsigned char y[V];
};

template <class Form, int V>
__device__ __forceinline__ void sl_load(SlPixels<Form, V>& px, const float* __restrict__ logits,
                                        const unsigned char* __restrict__ msk, const unsigned char* __restrict__ lbl,
                                        int label_mode, long b, long p, long HW) {
#pragma unroll
    for (int c = 0; c < Form::NC; ++c) {
        const long at = (b * Form::NC + c) * HW + p;
        if constexpr (V == 4) {
            const float4 v = *reinterpret_cast<const float4*>(logits + at);
            const uchar4 m = *reinterpret_cast<const uchar4*>(msk + at);
            px.x[c][0] = v.x; px.x[c][1] = v.y; px.x[c][2] = v.z; px.x[c][3] = v.w;
            px.t[c][0] = m.x; px.t[c][1] = m.y; px.t[c][2] = m.z; px.t[c][3] = m.w;
        } else {
            px.x[c][0] = logits[at];
            px.t[c][0] = msk[at];
        }
    }
    if constexpr (Form::HAS_LBL) {
        if (label_mode == 0) {
            if constexpr (V == 4) {
                const uchar4 l = *reinterpret_cast<const uchar4*>(lbl + b * HW + p);
                px.y[0] = l.x; px.y[1] = l.y; px.y[2] = l.z; px.y[3] = l.w;
            } else {
                px.y[0] = lbl[b * HW + p];
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) px.y[j] = 0;
}

// partial[blk][NQ] over the pixels this workgroup visits; n = B * HW / V lanes of V pixels, HWV = HW / V
template <class Form, int V>
__global__ __launch_bounds__(SL_THREADS) void sl_fwd_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ msk,
                                                            const unsigned char* __restrict__ lbl, int label_mode,
                                                            const float* __restrict__ weights, long n, long HWV, long HW,
                                                            double* __restrict__ partial) {
    constexpr int NC = Form::NC, NQ = Form::NQ;
    __shared__ double sh[SL_THREADS / 64][NQ];
    float cw[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) cw[c] = weights[NC + c];
    const float lnc = logf((float)NC);
    double acc[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) acc[k] = 0.0;
    for (long i = (long)blockIdx.x * SL_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * SL_THREADS) {
        const long b = i / HWV, p = (i - b * HWV) * V;
        SlPixels<Form, V> px;
        sl_load<Form, V>(px, logits, msk, lbl, label_mode, b, p, HW);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            unsigned char tb[NC];
            float z[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) tb[c] = px.t[c][j];
            const unsigned y = Form::label(label_mode, tb, px.y[j]);
            const bool m = !Form::MASKED_CE || y > 0;      // the pixel's logits reach the cross-entropy
            float s0 = 0.5f;                // sigmoid(0): the masked channel 0 of a background pixel
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                // the float expressions of combo_partial_kernel (xbd_step.hip)
                const float s = sl_sigmoid(px.x[c][j]);
                const float t = (float)tb[c];
                const float o = fminf(fmaxf(s, XEPS), 1.f - XEPS), tt = fminf(fmaxf(t, XEPS), 1.f - XEPS);
                const float pt = (1.f - tt) * (1.f - o) + tt * o;
                acc[c * 4 + 0] += (double)s * t;
                acc[c * 4 + 1] += s;
                acc[c * 4 + 2] += t;
                acc[c * 4 + 3] += -(double)((1.f - pt) * (1.f - pt)) * (double)logf(pt);
                z[c] = m ? px.x[c][j] : 0.f;
                if (c == 0 && m) s0 = s;
            }
            // cross-entropy of the (masked) logits: nll = logsumexp(z) - z_y with the maximum subtracted.  Where z is all zero
            // (background of the masked form) that is logf(NC) - 0 -- expf(0) is 1 and the sum NC, exactly -- and the expf are
            // skipped.
            float nll = lnc;
            if (m) {
                const float mx = sl_max(z);
                float se = 0.f;
#pragma unroll
                for (int c = 0; c < NC; ++c) se += expf(z[c] - mx);
                nll = logf(se) - (sl_sel(z, y) - mx);
            }
            if (!Form::COUNTS_BAD || y <= NC - 1) {
                const float wy = sl_sel(cw, y);
                acc[NC * 4 + 0] += wy;
                acc[NC * 4 + 1] += (double)wy * (double)nll;
            } else if constexpr (Form::COUNTS_BAD) {
                acc[NC * 4 + 4] += 1.0;     // a label no class has: no cross-entropy term, counted
            }
            if constexpr (Form::HAS_METER) {
                // the script's Dice meter reads channel 0 AFTER the in-place masking (line 460)
                acc[NC * 4 + 2] += (double)s0 * (float)tb[0];
                acc[NC * 4 + 3] += s0;
            }
        }
    }
    // dh_block_sum_f64's tree for all NQ sums behind ONE barrier: the shuffle sum of each wave, then the waves in order
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) sh[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        double t = 0.0;
        for (int w = 0; w < SL_THREADS / 64; ++w) t += sh[w][threadIdx.x];
        partial[(long)blockIdx.x * NQ + threadIdx.x] = t;
    }
}

// totals in a fixed order: 32 strided part sums per quantity, then those 32 in turn.  sums[SUMS] (floats, for the backward),
// parts[PARTS] = the channel losses, ce, then the form's tail; *loss = sum_c w_c channel_loss[c] + ce_w * ce
template <class Form>
__global__ __launch_bounds__(1024) void sl_finalize_kernel(const double* __restrict__ partial, int nblk, double npix,
                                                          const float* __restrict__ weights, float dice_w, float focal_w,
                                                          float ce_w, float* __restrict__ sums, float* __restrict__ parts,
                                                          float* __restrict__ loss) {
    constexpr int NC = Form::NC, NQ = Form::NQ;
    __shared__ double part[32][32];
    __shared__ double tot[32];
    const int k = threadIdx.x & 31, j = threadIdx.x >> 5;
    double a = 0.0;
    if (k < NQ)
        for (int b = j; b < nblk; b += 32) a += partial[(long)b * NQ + k];
    part[j][k] = a;
    __syncthreads();
    if (threadIdx.x < NQ) {
        double t = 0.0;
        for (int jj = 0; jj < 32; ++jj) t += part[jj][threadIdx.x];
        tot[threadIdx.x] = t;
        if (threadIdx.x < Form::SUMS) sums[threadIdx.x] = (float)t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = 0.f;
        for (int c = 0; c < NC; ++c) {
            // float arithmetic in the reference's order, as combo_finalize_kernel: 1 - (2 I + eps) / (S + T + eps); focal mean
            const float I = (float)tot[c * 4 + 0], S = (float)tot[c * 4 + 1], T = (float)tot[c * 4 + 2];
            const float dice = 1.f - (2.f * I + XEPS) / (S + T + XEPS);
            const float focal = (float)(tot[c * 4 + 3] / npix);
            const float l = dice_w * dice + focal_w * focal;
            parts[c] = l;
            total += weights[c] * l;
        }
        const float ce = (float)(tot[NC * 4 + 1] / tot[NC * 4 + 0]);          // torch's weighted mean over ALL pixels
        parts[NC] = ce;
        Form::parts_tail(tot, parts);
        *loss = total + ce_w * ce;
    }
}

// dlogits = upstream * [ w_c * combo gradient (combo_bwd_kernel's expressions) + ce_w * m * w_y / (sum w_y) * (softmax(z)_c - [c == y]) ]
// with m = [y > 0] in the masked form and 1 in the raw one
template <class Form, int V>
__global__ __launch_bounds__(SL_THREADS) void sl_bwd_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ msk,
                                                            const unsigned char* __restrict__ lbl, int label_mode,
                                                            const float* __restrict__ sums, const float* __restrict__ weights,
                                                            const float* __restrict__ upstream, float dice_w, float focal_w,
                                                            float ce_w, float inv_n, long n, long HWV, long HW,
                                                            float* __restrict__ dlogits) {
    constexpr int NC = Form::NC;
    const float up = upstream ? *upstream : 1.f;
    float w[NC], cw[NC], I[NC], U[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        w[c] = weights[c];
        cw[c] = weights[NC + c];
        I[c] = sums[c * 4 + 0];
        U[c] = sums[c * 4 + 1] + sums[c * 4 + 2] + XEPS;
    }
    const float den = sums[NC * 4 + 0];
    const float ce_coef = den > 0.f ? ce_w / den : 0.f;
    for (long i = (long)blockIdx.x * SL_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * SL_THREADS) {
        const long b = i / HWV, p = (i - b * HWV) * V;
        SlPixels<Form, V> px;
        sl_load<Form, V>(px, logits, msk, lbl, label_mode, b, p, HW);
        float g[NC][V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            unsigned char tb[NC];
            float z[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) tb[c] = px.t[c][j];
            const unsigned y = Form::label(label_mode, tb, px.y[j]);
            const bool m = !Form::MASKED_CE || y > 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float s = sl_sigmoid(px.x[c][j]);
                const float t = (float)tb[c];
                const float ddice = -(2.f * t * U[c] - (2.f * I[c] + XEPS)) / (U[c] * U[c]);
                float dfocal = 0.f;
                if (s > XEPS && s < 1.f - XEPS) {          // clamp passes the gradient strictly inside only
                    const float tt = fminf(fmaxf(t, XEPS), 1.f - XEPS);
                    const float pt = (1.f - tt) * (1.f - s) + tt * s;
                    const float q = 1.f - pt;
                    dfocal = (2.f * q * logf(pt) - q * q / pt) * (2.f * tt - 1.f) * inv_n;
                }
                g[c][j] = w[c] * (dice_w * ddice + focal_w * dfocal) * s * (1.f - s);
                z[c] = px.x[c][j];
            }
            if (m && (!Form::COUNTS_BAD || y <= NC - 1)) { // z == x here; a masked pixel or a bad label has no cross-entropy gradient
                const float mx = sl_max(z);
                float e[NC], se = 0.f;
#pragma unroll
                for (int c = 0; c < NC; ++c) { e[c] = expf(z[c] - mx); se += e[c]; }
                const float k = ce_coef * sl_sel(cw, y), inv = 1.f / se;
#pragma unroll
                for (int c = 0; c < NC; ++c) g[c][j] += k * (e[c] * inv - ((unsigned)c == y ? 1.f : 0.f));
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const long at = (b * NC + c) * HW + p;
            if constexpr (V == 4) {
                *reinterpret_cast<float4*>(dlogits + at) = make_float4(up * g[c][0], up * g[c][1], up * g[c][2], up * g[c][3]);
            } else {
                dlogits[at] = up * g[c][0];
            }
        }
    }
}

inline hipStream_t ST(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline bool sl_aligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }

// How a pass is launched: the 4-pixel form needs whole quads per plane and every plane's first byte on the load's boundary
// (a null lbl or dlogits counts as aligned); n lanes of V pixels, HWV = HW / V, and the grid under the pass's cap.
struct SlLaunch {
    bool vec;
    long n, HWV;
    int grid;
};

inline SlLaunch sl_launch(const float* logits, const unsigned char* msk, const unsigned char* lbl, const float* dlogits, int B,
                          long HW, int max_blocks) {
    SlLaunch L;
    L.vec = HW % 4 == 0 && sl_aligned(logits, 16) && sl_aligned(msk, 4) && sl_aligned(lbl, 4) && sl_aligned(dlogits, 16);
    L.HWV = L.vec ? HW / 4 : HW;
    L.n = (long)B * L.HWV;
    long g = (L.n + SL_THREADS - 1) / SL_THREADS;
    L.grid = (int)(g > max_blocks ? max_blocks : g);
    return L;
}

template <class Form>
inline int sl_check(const char* what, const float* logits, const unsigned char* msk, const unsigned char* lbl, int label_mode,
                    int B, long HW, const float* weights_dev) {
    DH_REQUIRE(logits != nullptr && msk != nullptr && weights_dev != nullptr, "%s: logits, msk and weights must be given", what);
    if constexpr (Form::HAS_LBL) {
        DH_REQUIRE(label_mode == 0 || label_mode == 1, "%s: label_mode=%d is neither 0 (lbl) nor 1 (damage)", what, label_mode);
        DH_REQUIRE(label_mode == 1 || lbl != nullptr, "%s: label_mode 0 reads lbl, which is null", what);
    }
    DH_REQUIRE(B > 0 && HW > 0, "%s: empty input (B=%d, HW=%ld)", what, B, HW);
    DH_REQUIRE(sl_aligned(logits, 4), "%s: logits are not 4-byte aligned", what);
    return 0;
}

template <class Form>
constexpr long sl_workspace_bytes() { return (long)SL_MAX_BLOCKS * Form::NQ * (long)sizeof(double); }

template <class Form>
int sl_fwd(const float* logits, const unsigned char* msk, const unsigned char* lbl, int label_mode, int B, long HW,
           const float* weights_dev, float dice_weight, float focal_weight, float ce_weight, float* sums_out, float* parts_out,
           float* loss_out, void* workspace, long workspace_bytes, void* stream) {
    if (sl_check<Form>(Form::FWD, logits, msk, lbl, label_mode, B, HW, weights_dev) != 0) return 1;
    DH_REQUIRE(sums_out != nullptr && parts_out != nullptr && loss_out != nullptr, "%s: an output is null", Form::FWD);
    DH_REQUIRE(workspace != nullptr && sl_aligned(workspace, 8) && workspace_bytes >= sl_workspace_bytes<Form>(),
               "%s: the workspace holds %ld bytes, %ld 8-byte aligned ones are needed", Form::FWD, workspace_bytes,
               sl_workspace_bytes<Form>());
    double* partial = reinterpret_cast<double*>(workspace);
    const SlLaunch L = sl_launch(logits, msk, lbl, nullptr, B, HW, SL_MAX_BLOCKS);
    const auto fwd = L.vec ? sl_fwd_kernel<Form, 4> : sl_fwd_kernel<Form, 1>;
    hipLaunchKernelGGL(fwd, dim3(L.grid), dim3(SL_THREADS), 0, ST(stream), logits, msk, lbl, label_mode, weights_dev, L.n, L.HWV,
                       HW, partial);
    DH_CHECK_LAUNCH(Form::FWD);
    hipLaunchKernelGGL(sl_finalize_kernel<Form>, dim3(1), dim3(1024), 0, ST(stream), partial, L.grid, (double)B * (double)HW,
                       weights_dev, dice_weight, focal_weight, ce_weight, sums_out, parts_out, loss_out);
    DH_CHECK_LAUNCH(Form::FINALIZE);
    return 0;
}

template <class Form>
int sl_bwd(const float* logits, const unsigned char* msk, const unsigned char* lbl, int label_mode, const float* sums,
           const float* weights_dev, const float* upstream_dev, float dice_weight, float focal_weight, float ce_weight, int B,
           long HW, float* dlogits, void* stream) {
    if (sl_check<Form>(Form::BWD, logits, msk, lbl, label_mode, B, HW, weights_dev) != 0) return 1;
    DH_REQUIRE(sums != nullptr && dlogits != nullptr, "%s: sums and dlogits must be given", Form::BWD);
    DH_REQUIRE(sl_aligned(dlogits, 4), "%s: dlogits are not 4-byte aligned", Form::BWD);
    const SlLaunch L = sl_launch(logits, msk, lbl, dlogits, B, HW, SL_BWD_MAX_BLOCKS);
    const float inv_n = 1.f / (float)((double)B * (double)HW);
    const auto bwd = L.vec ? sl_bwd_kernel<Form, 4> : sl_bwd_kernel<Form, 1>;
    hipLaunchKernelGGL(bwd, dim3(L.grid), dim3(SL_THREADS), 0, ST(stream), logits, msk, lbl, label_mode, sums, weights_dev,
                       upstream_dev, dice_weight, focal_weight, ce_weight, inv_n, L.n, L.HWV, HW, dlogits);
    DH_CHECK_LAUNCH(Form::BWD);
    return 0;
}

}  // namespace

// ---- train_unettransformer.py's loss ----
extern "C" int dh_xbd_unet_loss_workspace_size(long* bytes) {
    DH_REQUIRE(bytes != nullptr, "xbd_unet_loss: null size pointer");
    *bytes = sl_workspace_bytes<UnetForm>();
    return 0;
}

// lanes of one forward grid pass: that many pixels in the one-pixel form, four times as many in the 4-pixel form
extern "C" int dh_xbd_unet_loss_grid_pass(void) { return SL_MAX_BLOCKS * SL_THREADS; }

// logits fp32 [B][5][HW]; msk uint8 [B][5][HW]; lbl uint8 [B][HW] or null; weights_dev: 5 channel weights, then 5 class weights.
// sums_out [24], parts_out [8], loss_out [1].
extern "C" int dh_xbd_unet_loss_fwd(const float* logits, const unsigned char* msk, const unsigned char* lbl, int label_mode, int B,
                                    long HW, const float* weights_dev, float dice_weight, float focal_weight, float ce_weight,
                                    float* sums_out, float* parts_out, float* loss_out, void* workspace, long workspace_bytes,
                                    void* stream) {
    return sl_fwd<UnetForm>(logits, msk, lbl, label_mode, B, HW, weights_dev, dice_weight, focal_weight, ce_weight, sums_out,
                            parts_out, loss_out, workspace, workspace_bytes, stream);
}

extern "C" int dh_xbd_unet_loss_bwd(const float* logits, const unsigned char* msk, const unsigned char* lbl, int label_mode,
                                    const float* sums, const float* weights_dev, const float* upstream_dev, float dice_weight,
                                    float focal_weight, float ce_weight, int B, long HW, float* dlogits, void* stream) {
    return sl_bwd<UnetForm>(logits, msk, lbl, label_mode, sums, weights_dev, upstream_dev, dice_weight, focal_weight, ce_weight, B,
                            HW, dlogits, stream);
}

// ---- train_adapt.py's loss: no lbl, the label always comes from the mask bytes ----
extern "C" int dh_xbd_adapt_loss_workspace_size(long* bytes) {
    DH_REQUIRE(bytes != nullptr, "xbd_adapt_loss: null size pointer");
    *bytes = sl_workspace_bytes<AdaptForm>();
    return 0;
}

extern "C" int dh_xbd_adapt_loss_grid_pass(void) { return SL_MAX_BLOCKS * SL_THREADS; }

// logits fp32 [B][4][HW]; msk uint8 [B][4][HW]; weights_dev: 4 channel weights, then 4 class weights.
// sums_out [18], parts_out [6], loss_out [1].
extern "C" int dh_xbd_adapt_loss_fwd(const float* logits, const unsigned char* msk, int B, long HW, const float* weights_dev,
                                     float dice_weight, float focal_weight, float ce_weight, float* sums_out, float* parts_out,
                                     float* loss_out, void* workspace, long workspace_bytes, void* stream) {
    return sl_fwd<AdaptForm>(logits, msk, nullptr, 1, B, HW, weights_dev, dice_weight, focal_weight, ce_weight, sums_out, parts_out,
                             loss_out, workspace, workspace_bytes, stream);
}

extern "C" int dh_xbd_adapt_loss_bwd(const float* logits, const unsigned char* msk, const float* sums, const float* weights_dev,
                                     const float* upstream_dev, float dice_weight, float focal_weight, float ce_weight, int B,
                                     long HW, float* dlogits, void* stream) {
    return sl_bwd<AdaptForm>(logits, msk, nullptr, 1, sums, weights_dev, upstream_dev, dice_weight, focal_weight, ce_weight, B, HW,
                             dlogits, stream);
}
