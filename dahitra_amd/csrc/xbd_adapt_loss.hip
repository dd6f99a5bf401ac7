// Loss of the xBD adaptation step, xBD_code/train_adapt.py (lines 332-342), the four-output DAHiTra fine-tuned on Ida-BD:
//   four ComboLoss{dice:1, focal:8} terms, one per output channel ..... xBD_code/losses.py:24-34, 95-126, 273-288
//   + ce_w * CrossEntropyLoss(weight)(out, y), y = argmax(1 - m0, m1, m2, m3) ... train_adapt.py:338-340
// The sibling of xbd_unet_loss.hip, with its structure: the masks are the loader's uint8 bytes read in place, ONE pass over the
// pixels for all 18 sums, one small finalize launch, one pass for the gradient; 16-byte logit loads per lane where HW % 4 == 0;
// every sum in fp64 through the fixed two-stage tree, so the results are deterministic.  What differs: four channels, the label
// is always derived from the mask bytes here, and the cross-entropy is taken of the RAW logits -- nothing is masked, so every
// pixel has a cross-entropy gradient.
#include "common.h"

namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_MAX_BLOCKS = 1024;       // forward grid cap: one grid pass covers AL_MAX_BLOCKS * AL_THREADS lanes
constexpr int AL_BWD_MAX_BLOCKS = 2048;
constexpr int AL_NQ = 18;                 // sums per workgroup: [c][4] combo, sum w_y, sum w_y nll
constexpr float XEPS = 1e-6f;             // xBD_code/losses.py:12

__device__ __forceinline__ float al_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// a[y] for y in 0 .. 3 without a runtime-indexed register array
__device__ __forceinline__ float al_sel4(const float (&a)[4], unsigned y) {
    float r = a[0];
    r = y == 1 ? a[1] : r;
    r = y == 2 ? a[2] : r;
    r = y == 3 ? a[3] : r;
    return r;
}

// torch.argmax(msks, dim=1) after msks[:, 0] = 1 - msks[:, 0] (train_adapt.py:338-339) on the integers the bytes stand for:
// the FIRST maximum of (1 - t0, t1, t2, t3)
__device__ __forceinline__ unsigned al_label(const unsigned char (&t)[4]) {
    int best = 1 - (int)t[0];
    unsigned y = 0;
#pragma unroll
    for (int c = 1; c < 4; ++c)
        if ((int)t[c] > best) { best = (int)t[c]; y = (unsigned)c; }
    return y;
}

// logits and mask bytes of V consecutive pixels of image b, starting at pixel p
template <int V>
struct AlPixels {
    float x[4][V];
    unsigned char t[4][V];
};

template <int V>
__device__ __forceinline__ void al_load(AlPixels<V>& px, const float* __restrict__ logits, const unsigned char* __restrict__ msk,
                                        long b, long p, long HW) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const long at = (b * 4 + c) * HW + p;
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
}

// partial[blk][18] over the pixels this workgroup visits; n = B * HW / V lanes of V pixels, HWV = HW / V
template <int V>
__global__ __launch_bounds__(AL_THREADS) void al_fwd_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ msk,
                                                            const float* __restrict__ weights, long n, long HWV, long HW,
                                                            double* __restrict__ partial) {
    __shared__ double sh[AL_THREADS / 64][AL_NQ];
    float cw[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) cw[c] = weights[4 + c];
    double acc[AL_NQ];
#pragma unroll
    for (int k = 0; k < AL_NQ; ++k) acc[k] = 0.0;
    for (long i = (long)blockIdx.x * AL_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * AL_THREADS) {
        const long b = i / HWV, p = (i - b * HWV) * V;
        AlPixels<V> px;
        al_load<V>(px, logits, msk, b, p, HW);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            unsigned char tb[4];
            float z[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) tb[c] = px.t[c][j];
            const unsigned y = al_label(tb);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                // the float expressions of combo_partial_kernel (xbd_step.hip), as ul_fwd_kernel has them
                const float s = al_sigmoid(px.x[c][j]);
                const float t = (float)tb[c];
                const float o = fminf(fmaxf(s, XEPS), 1.f - XEPS), tt = fminf(fmaxf(t, XEPS), 1.f - XEPS);
                const float pt = (1.f - tt) * (1.f - o) + tt * o;
                acc[c * 4 + 0] += (double)s * t;
                acc[c * 4 + 1] += s;
                acc[c * 4 + 2] += t;
                acc[c * 4 + 3] += -(double)((1.f - pt) * (1.f - pt)) * (double)logf(pt);
                z[c] = px.x[c][j];
            }
            // cross-entropy of the raw logits: nll = logsumexp(z) - z_y with the maximum subtracted
            const float mx = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
            float se = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) se += expf(z[c] - mx);
            const float nll = logf(se) - (al_sel4(z, y) - mx);
            const float wy = al_sel4(cw, y);
            acc[16] += wy;
            acc[17] += (double)wy * (double)nll;
        }
    }
    // dh_block_sum_f64's tree for all 18 sums behind ONE barrier: the shuffle sum of each wave, then the waves in order
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < AL_NQ; ++k) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) sh[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < AL_NQ) {
        double t = 0.0;
        for (int w = 0; w < AL_THREADS / 64; ++w) t += sh[w][threadIdx.x];
        partial[(long)blockIdx.x * AL_NQ + threadIdx.x] = t;
    }
}

// totals in a fixed order: 32 strided part sums per quantity, then those 32 in turn.  sums[18] (floats, for the backward),
// parts[6] = four channel losses, ce, 0; *loss = sum_c w_c channel_loss[c] + ce_w * ce
__global__ __launch_bounds__(1024) void al_finalize_kernel(const double* __restrict__ partial, int nblk, double npix,
                                                          const float* __restrict__ weights, float dice_w, float focal_w,
                                                          float ce_w, float* __restrict__ sums, float* __restrict__ parts,
                                                          float* __restrict__ loss) {
    __shared__ double part[32][32];
    __shared__ double tot[32];
    const int k = threadIdx.x & 31, j = threadIdx.x >> 5;
    double a = 0.0;
    if (k < AL_NQ)
        for (int b = j; b < nblk; b += 32) a += partial[(long)b * AL_NQ + k];
    part[j][k] = a;
    __syncthreads();
    if (threadIdx.x < AL_NQ) {
        double t = 0.0;
        for (int jj = 0; jj < 32; ++jj) t += part[jj][threadIdx.x];
        tot[threadIdx.x] = t;
        sums[threadIdx.x] = (float)t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = 0.f;
        for (int c = 0; c < 4; ++c) {
            // float arithmetic in the reference's order, as combo_finalize_kernel: 1 - (2 I + eps) / (S + T + eps); focal mean
            const float I = (float)tot[c * 4 + 0], S = (float)tot[c * 4 + 1], T = (float)tot[c * 4 + 2];
            const float dice = 1.f - (2.f * I + XEPS) / (S + T + XEPS);
            const float focal = (float)(tot[c * 4 + 3] / npix);
            const float l = dice_w * dice + focal_w * focal;
            parts[c] = l;
            total += weights[c] * l;
        }
        const float ce = (float)(tot[17] / tot[16]);          // torch's weighted mean over ALL pixels
        parts[4] = ce;
        parts[5] = 0.f;
        *loss = total + ce_w * ce;
    }
}

// dlogits = upstream * [ w_c * combo gradient (combo_bwd_kernel's expressions) + ce_w * w_y / (sum w_y) * (softmax(x)_c - [c == y]) ]
template <int V>
__global__ __launch_bounds__(AL_THREADS) void al_bwd_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ msk,
                                                            const float* __restrict__ sums, const float* __restrict__ weights,
                                                            const float* __restrict__ upstream, float dice_w, float focal_w,
                                                            float ce_w, float inv_n, long n, long HWV, long HW,
                                                            float* __restrict__ dlogits) {
    const float up = upstream ? *upstream : 1.f;
    float w[4], cw[4], I[4], U[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        w[c] = weights[c];
        cw[c] = weights[4 + c];
        I[c] = sums[c * 4 + 0];
        U[c] = sums[c * 4 + 1] + sums[c * 4 + 2] + XEPS;
    }
    const float den = sums[16];
    const float ce_coef = den > 0.f ? ce_w / den : 0.f;
    for (long i = (long)blockIdx.x * AL_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * AL_THREADS) {
        const long b = i / HWV, p = (i - b * HWV) * V;
        AlPixels<V> px;
        al_load<V>(px, logits, msk, b, p, HW);
        float g[4][V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            unsigned char tb[4];
            float z[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) tb[c] = px.t[c][j];
            const unsigned y = al_label(tb);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float s = al_sigmoid(px.x[c][j]);
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
            const float mx = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
            float e[4], se = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) { e[c] = expf(z[c] - mx); se += e[c]; }
            const float k = ce_coef * al_sel4(cw, y), inv = 1.f / se;
#pragma unroll
            for (int c = 0; c < 4; ++c) g[c][j] += k * (e[c] * inv - ((unsigned)c == y ? 1.f : 0.f));
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long at = (b * 4 + c) * HW + p;
            if constexpr (V == 4) {
                *reinterpret_cast<float4*>(dlogits + at) = make_float4(up * g[c][0], up * g[c][1], up * g[c][2], up * g[c][3]);
            } else {
                dlogits[at] = up * g[c][0];
            }
        }
    }
}

inline hipStream_t ST(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline bool al_aligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }

// the 4-pixel form needs whole quads per plane and every plane's first byte on the load's boundary
inline bool al_vector(const float* logits, const unsigned char* msk, const float* dlogits, long HW) {
    return HW % 4 == 0 && al_aligned(logits, 16) && al_aligned(msk, 4) && al_aligned(dlogits, 16);
}

inline int al_check(const char* what, const float* logits, const unsigned char* msk, int B, long HW, const float* weights_dev) {
    DH_REQUIRE(logits != nullptr && msk != nullptr && weights_dev != nullptr, "%s: logits, msk and weights must be given", what);
    DH_REQUIRE(B > 0 && HW > 0, "%s: empty input (B=%d, HW=%ld)", what, B, HW);
    DH_REQUIRE(al_aligned(logits, 4), "%s: logits are not 4-byte aligned", what);
    return 0;
}

}  // namespace

extern "C" int dh_xbd_adapt_loss_workspace_size(long* bytes) {
    DH_REQUIRE(bytes != nullptr, "xbd_adapt_loss: null size pointer");
    *bytes = (long)AL_MAX_BLOCKS * AL_NQ * sizeof(double);
    return 0;
}

// lanes of one forward grid pass: that many pixels in the one-pixel form, four times as many in the 4-pixel form
extern "C" int dh_xbd_adapt_loss_grid_pass(void) { return AL_MAX_BLOCKS * AL_THREADS; }

// logits fp32 [B][4][HW]; msk uint8 [B][4][HW]; weights_dev: 4 channel weights, then 4 class weights.
// sums_out [18], parts_out [6], loss_out [1].
extern "C" int dh_xbd_adapt_loss_fwd(const float* logits, const unsigned char* msk, int B, long HW, const float* weights_dev,
                                     float dice_weight, float focal_weight, float ce_weight, float* sums_out, float* parts_out,
                                     float* loss_out, void* workspace, long workspace_bytes, void* stream) {
    if (al_check("xbd_adapt_loss_fwd", logits, msk, B, HW, weights_dev) != 0) return 1;
    DH_REQUIRE(sums_out != nullptr && parts_out != nullptr && loss_out != nullptr, "xbd_adapt_loss_fwd: an output is null");
    DH_REQUIRE(workspace != nullptr && al_aligned(workspace, 8) &&
                   workspace_bytes >= (long)AL_MAX_BLOCKS * AL_NQ * (long)sizeof(double),
               "xbd_adapt_loss_fwd: the workspace holds %ld bytes, %ld 8-byte aligned ones are needed", workspace_bytes,
               (long)AL_MAX_BLOCKS * AL_NQ * (long)sizeof(double));
    double* partial = reinterpret_cast<double*>(workspace);
    const bool vec = al_vector(logits, msk, nullptr, HW);
    const long n = vec ? (long)B * (HW / 4) : (long)B * HW;
    long g = (n + AL_THREADS - 1) / AL_THREADS;
    if (g > AL_MAX_BLOCKS) g = AL_MAX_BLOCKS;
    if (vec)
        hipLaunchKernelGGL(al_fwd_kernel<4>, dim3((int)g), dim3(AL_THREADS), 0, ST(stream), logits, msk, weights_dev, n, HW / 4, HW,
                           partial);
    else
        hipLaunchKernelGGL(al_fwd_kernel<1>, dim3((int)g), dim3(AL_THREADS), 0, ST(stream), logits, msk, weights_dev, n, HW, HW,
                           partial);
    DH_CHECK_LAUNCH("xbd_adapt_loss_fwd");
    hipLaunchKernelGGL(al_finalize_kernel, dim3(1), dim3(1024), 0, ST(stream), partial, (int)g, (double)B * (double)HW, weights_dev,
                       dice_weight, focal_weight, ce_weight, sums_out, parts_out, loss_out);
    DH_CHECK_LAUNCH("xbd_adapt_loss_finalize");
    return 0;
}

extern "C" int dh_xbd_adapt_loss_bwd(const float* logits, const unsigned char* msk, const float* sums, const float* weights_dev,
                                     const float* upstream_dev, float dice_weight, float focal_weight, float ce_weight, int B,
                                     long HW, float* dlogits, void* stream) {
    if (al_check("xbd_adapt_loss_bwd", logits, msk, B, HW, weights_dev) != 0) return 1;
    DH_REQUIRE(sums != nullptr && dlogits != nullptr, "xbd_adapt_loss_bwd: sums and dlogits must be given");
    DH_REQUIRE(al_aligned(dlogits, 4), "xbd_adapt_loss_bwd: dlogits are not 4-byte aligned");
    const bool vec = al_vector(logits, msk, dlogits, HW);
    const long n = vec ? (long)B * (HW / 4) : (long)B * HW;
    long g = (n + AL_THREADS - 1) / AL_THREADS;
    if (g > AL_BWD_MAX_BLOCKS) g = AL_BWD_MAX_BLOCKS;
    const float inv_n = 1.f / (float)((double)B * (double)HW);
    if (vec)
        hipLaunchKernelGGL(al_bwd_kernel<4>, dim3((int)g), dim3(AL_THREADS), 0, ST(stream), logits, msk, sums, weights_dev,
                           upstream_dev, dice_weight, focal_weight, ce_weight, inv_n, n, HW / 4, HW, dlogits);
    else
        hipLaunchKernelGGL(al_bwd_kernel<1>, dim3((int)g), dim3(AL_THREADS), 0, ST(stream), logits, msk, sums, weights_dev,
                           upstream_dev, dice_weight, focal_weight, ce_weight, inv_n, n, HW, HW, dlogits);
    DH_CHECK_LAUNCH("xbd_adapt_loss_bwd");
    return 0;
}
