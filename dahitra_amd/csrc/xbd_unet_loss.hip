// Loss of the xBD step of xBD_code/train_unettransformer.py (lines 438-461), the script that trains DAHiTra proper:
//   five ComboLoss{dice:1, focal:8} terms, one per output channel ... xBD_code/losses.py:24-34, 95-126, 273-288
//   + ce_w * CrossEntropyLoss(weight)(out * (lbl > 0), lbl) .......... train_unettransformer.py:445-449, 563-564
//   + the Dice meter of line 460-461 on the MASKED channel 0
// The masks are the loader's uint8 bytes (no float copy of them exists), the label is a byte per pixel or is derived from the
// mask bytes in the kernel.  HBM-streaming work: ONE pass over the pixels for all 25 sums (the parent's combo kernels make one
// pass per channel), one small finalize launch, and one pass for the gradient.  16-byte logit loads per lane where HW % 4 == 0.
// Every sum is carried in fp64 through a fixed two-stage tree (dh_block_sum_f64's, all 25 sums behind one barrier; then a
// fixed-order finalize), so the results are deterministic.
#include "common.h"

namespace {

constexpr int UL_THREADS = 256;
constexpr int UL_MAX_BLOCKS = 1024;       // forward grid cap: one grid pass covers UL_MAX_BLOCKS * UL_THREADS lanes
constexpr int UL_BWD_MAX_BLOCKS = 2048;
constexpr int UL_NQ = 25;                 // sums per workgroup: [c][4] combo, sum w_y, sum w_y nll, meter I, meter S, bad labels
constexpr int UL_SUMS = 24;               // of which the backward and the caller get the first 24 as floats
constexpr float XEPS = 1e-6f;             // xBD_code/losses.py:12

__device__ __forceinline__ float ul_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// a[y] for y in 0 .. 4 without a runtime-indexed register array
__device__ __forceinline__ float ul_sel5(const float (&a)[5], unsigned y) {
    float r = a[0];
    r = y == 1 ? a[1] : r;
    r = y == 2 ? a[2] : r;
    r = y == 3 ? a[3] : r;
    r = y == 4 ? a[4] : r;
    return r;
}

// the label of a pixel: the byte of `lbl`, or ("damage") the first set channel among 1 .. 4 of the mask, 0 if none
__device__ __forceinline__ unsigned ul_label(int label_mode, const unsigned char (&t)[5], unsigned char lbl) {
    if (label_mode == 0) return lbl;
    return t[1] ? 1u : t[2] ? 2u : t[3] ? 3u : t[4] ? 4u : 0u;
}

// logits, mask bytes and label byte of V consecutive pixels of image b, starting at pixel p
template <int V>
struct UlPixels {
    float x[5][V];
    unsigned char t[5][V];
    unsigned char y[V];
};

template <int V>
__device__ __forceinline__ void ul_load(UlPixels<V>& px, const float* __restrict__ logits, const unsigned char* __restrict__ msk,
                                        const unsigned char* __restrict__ lbl, int label_mode, long b, long p, long HW) {
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const long at = (b * 5 + c) * HW + p;
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
    if (label_mode == 0) {
        if constexpr (V == 4) {
            const uchar4 l = *reinterpret_cast<const uchar4*>(lbl + b * HW + p);
            px.y[0] = l.x; px.y[1] = l.y; px.y[2] = l.z; px.y[3] = l.w;
        } else {
            px.y[0] = lbl[b * HW + p];
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) px.y[j] = 0;
    }
}

// partial[blk][25] over the pixels this workgroup visits; n = B * HW / V lanes of V pixels, HWV = HW / V
template <int V>
__global__ __launch_bounds__(UL_THREADS) void ul_fwd_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ msk,
                                                            const unsigned char* __restrict__ lbl, int label_mode,
                                                            const float* __restrict__ weights, long n, long HWV, long HW,
                                                            double* __restrict__ partial) {
    __shared__ double sh[UL_THREADS / 64][UL_NQ];
    float cw[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) cw[c] = weights[5 + c];
    const float ln5 = logf(5.f);
    double acc[UL_NQ];
#pragma unroll
    for (int k = 0; k < UL_NQ; ++k) acc[k] = 0.0;
    for (long i = (long)blockIdx.x * UL_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * UL_THREADS) {
        const long b = i / HWV, p = (i - b * HWV) * V;
        UlPixels<V> px;
        ul_load<V>(px, logits, msk, lbl, label_mode, b, p, HW);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            unsigned char tb[5];
            float z[5];
#pragma unroll
            for (int c = 0; c < 5; ++c) tb[c] = px.t[c][j];
            const unsigned y = ul_label(label_mode, tb, px.y[j]);
            const bool m = y > 0;
            float s0 = 0.5f;                // sigmoid(0): the masked channel 0 of a background pixel
#pragma unroll
            for (int c = 0; c < 5; ++c) {
                // the float expressions of combo_partial_kernel (xbd_step.hip)
                const float s = ul_sigmoid(px.x[c][j]);
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
            // cross-entropy of the masked logits: nll = logsumexp(z) - z_y with the maximum subtracted.  Where z is all zero
            // (background) that is logf(5) - 0 -- expf(0) is 1 and the sum 5, exactly -- and the five expf are skipped.
            float nll = ln5;
            if (m) {
                const float mx = fmaxf(fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3])), z[4]);
                float se = 0.f;
#pragma unroll
                for (int c = 0; c < 5; ++c) se += expf(z[c] - mx);
                nll = logf(se) - (ul_sel5(z, y) - mx);
            }
            if (y <= 4) {
                const float wy = ul_sel5(cw, y);
                acc[20] += wy;
                acc[21] += (double)wy * (double)nll;
            } else {
                acc[24] += 1.0;             // a label no class has: no cross-entropy term, counted
            }
            // the script's Dice meter reads channel 0 AFTER the in-place masking (line 460)
            acc[22] += (double)s0 * (float)tb[0];
            acc[23] += s0;
        }
    }
    // dh_block_sum_f64's tree for all 25 sums behind ONE barrier: the shuffle sum of each wave, then the waves in order
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < UL_NQ; ++k) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) sh[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < UL_NQ) {
        double t = 0.0;
        for (int w = 0; w < UL_THREADS / 64; ++w) t += sh[w][threadIdx.x];
        partial[(long)blockIdx.x * UL_NQ + threadIdx.x] = t;
    }
}

// totals in a fixed order: 32 strided part sums per quantity, then those 32 in turn.  sums[24] (floats, for the backward),
// parts[8] = five channel losses, ce, Dice meter, bad labels; *loss = sum_c w_c channel_loss[c] + ce_w * ce
__global__ __launch_bounds__(1024) void ul_finalize_kernel(const double* __restrict__ partial, int nblk, double npix,
                                                          const float* __restrict__ weights, float dice_w, float focal_w,
                                                          float ce_w, float* __restrict__ sums, float* __restrict__ parts,
                                                          float* __restrict__ loss) {
    __shared__ double part[32][32];
    __shared__ double tot[32];
    const int k = threadIdx.x & 31, j = threadIdx.x >> 5;
    double a = 0.0;
    if (k < UL_NQ)
        for (int b = j; b < nblk; b += 32) a += partial[(long)b * UL_NQ + k];
    part[j][k] = a;
    __syncthreads();
    if (threadIdx.x < UL_NQ) {
        double t = 0.0;
        for (int jj = 0; jj < 32; ++jj) t += part[jj][threadIdx.x];
        tot[threadIdx.x] = t;
        if (threadIdx.x < UL_SUMS) sums[threadIdx.x] = (float)t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = 0.f;
        for (int c = 0; c < 5; ++c) {
            // float arithmetic in the reference's order, as combo_finalize_kernel: 1 - (2 I + eps) / (S + T + eps); focal mean
            const float I = (float)tot[c * 4 + 0], S = (float)tot[c * 4 + 1], T = (float)tot[c * 4 + 2];
            const float dice = 1.f - (2.f * I + XEPS) / (S + T + XEPS);
            const float focal = (float)(tot[c * 4 + 3] / npix);
            const float l = dice_w * dice + focal_w * focal;
            parts[c] = l;
            total += weights[c] * l;
        }
        const float ce = (float)(tot[21] / tot[20]);          // torch's weighted mean over ALL pixels
        const float mI = (float)tot[22], mS = (float)tot[23], T0 = (float)tot[2];
        parts[5] = ce;
        parts[6] = (2.f * mI + XEPS) / (mS + T0 + XEPS);      // 1 - soft_dice_loss(sigmoid(masked channel 0), msk[:, 0])
        parts[7] = (float)tot[24];
        *loss = total + ce_w * ce;
    }
}

// dlogits = upstream * [ w_c * combo gradient (combo_bwd_kernel's expressions) + ce_w * m * w_y / (sum w_y) * (softmax(z)_c - [c == y]) ]
template <int V>
__global__ __launch_bounds__(UL_THREADS) void ul_bwd_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ msk,
                                                            const unsigned char* __restrict__ lbl, int label_mode,
                                                            const float* __restrict__ sums, const float* __restrict__ weights,
                                                            const float* __restrict__ upstream, float dice_w, float focal_w,
                                                            float ce_w, float inv_n, long n, long HWV, long HW,
                                                            float* __restrict__ dlogits) {
    const float up = upstream ? *upstream : 1.f;
    float w[5], cw[5], I[5], U[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        w[c] = weights[c];
        cw[c] = weights[5 + c];
        I[c] = sums[c * 4 + 0];
        U[c] = sums[c * 4 + 1] + sums[c * 4 + 2] + XEPS;
    }
    const float den = sums[20];
    const float ce_coef = den > 0.f ? ce_w / den : 0.f;
    for (long i = (long)blockIdx.x * UL_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * UL_THREADS) {
        const long b = i / HWV, p = (i - b * HWV) * V;
        UlPixels<V> px;
        ul_load<V>(px, logits, msk, lbl, label_mode, b, p, HW);
        float g[5][V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            unsigned char tb[5];
            float z[5];
#pragma unroll
            for (int c = 0; c < 5; ++c) tb[c] = px.t[c][j];
            const unsigned y = ul_label(label_mode, tb, px.y[j]);
            const bool m = y > 0;
#pragma unroll
            for (int c = 0; c < 5; ++c) {
                const float s = ul_sigmoid(px.x[c][j]);
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
            if (m && y <= 4) {                             // z == x here; a masked pixel or a bad label has no cross-entropy gradient
                const float mx = fmaxf(fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3])), z[4]);
                float e[5], se = 0.f;
#pragma unroll
                for (int c = 0; c < 5; ++c) { e[c] = expf(z[c] - mx); se += e[c]; }
                const float k = ce_coef * ul_sel5(cw, y), inv = 1.f / se;
#pragma unroll
                for (int c = 0; c < 5; ++c) g[c][j] += k * (e[c] * inv - ((unsigned)c == y ? 1.f : 0.f));
            }
        }
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const long at = (b * 5 + c) * HW + p;
            if constexpr (V == 4) {
                *reinterpret_cast<float4*>(dlogits + at) = make_float4(up * g[c][0], up * g[c][1], up * g[c][2], up * g[c][3]);
            } else {
                dlogits[at] = up * g[c][0];
            }
        }
    }
}

inline hipStream_t ST(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline bool ul_aligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }

// the 4-pixel form needs whole quads per plane and every plane's first byte on the load's boundary
inline bool ul_vector(const float* logits, const unsigned char* msk, const unsigned char* lbl, const float* dlogits, long HW) {
    return HW % 4 == 0 && ul_aligned(logits, 16) && ul_aligned(msk, 4) && ul_aligned(lbl, 4) && ul_aligned(dlogits, 16);
}

inline int ul_check(const char* what, const float* logits, const unsigned char* msk, const unsigned char* lbl, int label_mode,
                    int B, long HW, const float* weights_dev) {
    DH_REQUIRE(logits != nullptr && msk != nullptr && weights_dev != nullptr, "%s: logits, msk and weights must be given", what);
    DH_REQUIRE(label_mode == 0 || label_mode == 1, "%s: label_mode=%d is neither 0 (lbl) nor 1 (damage)", what, label_mode);
    DH_REQUIRE(label_mode == 1 || lbl != nullptr, "%s: label_mode 0 reads lbl, which is null", what);
    DH_REQUIRE(B > 0 && HW > 0, "%s: empty input (B=%d, HW=%ld)", what, B, HW);
    DH_REQUIRE(ul_aligned(logits, 4), "%s: logits are not 4-byte aligned", what);
    return 0;
}

}  // namespace

extern "C" int dh_xbd_unet_loss_workspace_size(long* bytes) {
    DH_REQUIRE(bytes != nullptr, "xbd_unet_loss: null size pointer");
    *bytes = (long)UL_MAX_BLOCKS * UL_NQ * sizeof(double);
    return 0;
}

// lanes of one forward grid pass: that many pixels in the one-pixel form, four times as many in the 4-pixel form
extern "C" int dh_xbd_unet_loss_grid_pass(void) { return UL_MAX_BLOCKS * UL_THREADS; }

// logits fp32 [B][5][HW]; msk uint8 [B][5][HW]; lbl uint8 [B][HW] or null; weights_dev: 5 channel weights, then 5 class weights.
// sums_out [24], parts_out [8], loss_out [1].
extern "C" int dh_xbd_unet_loss_fwd(const float* logits, const unsigned char* msk, const unsigned char* lbl, int label_mode, int B,
                                    long HW, const float* weights_dev, float dice_weight, float focal_weight, float ce_weight,
                                    float* sums_out, float* parts_out, float* loss_out, void* workspace, long workspace_bytes,
                                    void* stream) {
    if (ul_check("xbd_unet_loss_fwd", logits, msk, lbl, label_mode, B, HW, weights_dev) != 0) return 1;
    DH_REQUIRE(sums_out != nullptr && parts_out != nullptr && loss_out != nullptr, "xbd_unet_loss_fwd: an output is null");
    DH_REQUIRE(workspace != nullptr && ul_aligned(workspace, 8) &&
                   workspace_bytes >= (long)UL_MAX_BLOCKS * UL_NQ * (long)sizeof(double),
               "xbd_unet_loss_fwd: the workspace holds %ld bytes, %ld 8-byte aligned ones are needed", workspace_bytes,
               (long)UL_MAX_BLOCKS * UL_NQ * (long)sizeof(double));
    double* partial = reinterpret_cast<double*>(workspace);
    const bool vec = ul_vector(logits, msk, lbl, nullptr, HW);
    const long n = vec ? (long)B * (HW / 4) : (long)B * HW;
    long g = (n + UL_THREADS - 1) / UL_THREADS;
    if (g > UL_MAX_BLOCKS) g = UL_MAX_BLOCKS;
    if (vec)
        hipLaunchKernelGGL(ul_fwd_kernel<4>, dim3((int)g), dim3(UL_THREADS), 0, ST(stream), logits, msk, lbl, label_mode,
                           weights_dev, n, HW / 4, HW, partial);
    else
        hipLaunchKernelGGL(ul_fwd_kernel<1>, dim3((int)g), dim3(UL_THREADS), 0, ST(stream), logits, msk, lbl, label_mode,
                           weights_dev, n, HW, HW, partial);
    DH_CHECK_LAUNCH("xbd_unet_loss_fwd");
    hipLaunchKernelGGL(ul_finalize_kernel, dim3(1), dim3(1024), 0, ST(stream), partial, (int)g, (double)B * (double)HW, weights_dev,
                       dice_weight, focal_weight, ce_weight, sums_out, parts_out, loss_out);
    DH_CHECK_LAUNCH("xbd_unet_loss_finalize");
    return 0;
}

extern "C" int dh_xbd_unet_loss_bwd(const float* logits, const unsigned char* msk, const unsigned char* lbl, int label_mode,
                                    const float* sums, const float* weights_dev, const float* upstream_dev, float dice_weight,
                                    float focal_weight, float ce_weight, int B, long HW, float* dlogits, void* stream) {
    if (ul_check("xbd_unet_loss_bwd", logits, msk, lbl, label_mode, B, HW, weights_dev) != 0) return 1;
    DH_REQUIRE(sums != nullptr && dlogits != nullptr, "xbd_unet_loss_bwd: sums and dlogits must be given");
    DH_REQUIRE(ul_aligned(dlogits, 4), "xbd_unet_loss_bwd: dlogits are not 4-byte aligned");
    const bool vec = ul_vector(logits, msk, lbl, dlogits, HW);
    const long n = vec ? (long)B * (HW / 4) : (long)B * HW;
    long g = (n + UL_THREADS - 1) / UL_THREADS;
    if (g > UL_BWD_MAX_BLOCKS) g = UL_BWD_MAX_BLOCKS;
    const float inv_n = 1.f / (float)((double)B * (double)HW);
    if (vec)
        hipLaunchKernelGGL(ul_bwd_kernel<4>, dim3((int)g), dim3(UL_THREADS), 0, ST(stream), logits, msk, lbl, label_mode, sums,
                           weights_dev, upstream_dev, dice_weight, focal_weight, ce_weight, inv_n, n, HW / 4, HW, dlogits);
    else
        hipLaunchKernelGGL(ul_bwd_kernel<1>, dim3((int)g), dim3(UL_THREADS), 0, ST(stream), logits, msk, lbl, label_mode, sums,
                           weights_dev, upstream_dev, dice_weight, focal_weight, ce_weight, inv_n, n, HW, HW, dlogits);
    DH_CHECK_LAUNCH("xbd_unet_loss_bwd");
    return 0;
}
