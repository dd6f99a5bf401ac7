// The xBD validation count (xBD_code/train.py:258-279) in one pass over the logits:
//   s = sigmoid(out) in fp32; loc = s[0] > thr; pred = argmax(s[1:]) * loc (first maximum of the fp32 SIGMOIDS wins, so two
//   logits that both saturate to 1.0f pick the lower channel); per image |gt0|, |loc|, |gt0 & loc| for dice(msks[j, 0], loc);
//   per class tp / fn / fp over the selected pixels.
// Selection 0 ("reference") is what train.py:271-274 executes: lbl_msk[j][lbl_msk[j, 0] > 0] is a boolean index on axis 0 by
// the image's first ROW, so row r counts with all its columns iff lbl[j][0][r] > 0 (needs H == W).  Selection 1 ("building")
// counts pixel p iff msk0[j][p] > 0.
// HBM-bound: 5 fp32 planes + 2 byte planes = 22 bytes per pixel, read once with 16-byte / 4-byte lanes.  After the sigmoid all
// arithmetic is on integers: per-thread counts, a wave reduction, one LDS step over the workgroup's waves, one 64-bit integer
// atomic per counter and workgroup -- the counts are exact and independent of the order of the partial sums.
#include "common.h"

namespace {

constexpr int VC_THREADS = 256;
constexpr int VC_WAVES = VC_THREADS / 64;
constexpr int VC_MAX_WORKGROUPS = 512;      // over the whole batch: two workgroups per CU, the rest is the grid-stride loop
constexpr int VC_NCOUNT = 15;               // 3 image counters, then (tp, fn, fp) of each of the 4 classes

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// 4 consecutive values of a plane from pixel p0; `vec`: the address is aligned to the vector and all four are inside the plane
__device__ __forceinline__ void load4(const float* __restrict__ p, bool vec, int n, float (&o)[4]) {
    if (vec) {
        ld4(p, o);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = k < n ? p[k] : 0.f;
    }
}
__device__ __forceinline__ void load4(const unsigned char* __restrict__ p, bool vec, int n, unsigned (&o)[4]) {
    if (vec) {
        const unsigned v = *reinterpret_cast<const unsigned*>(p);
        o[0] = v & 255u; o[1] = (v >> 8) & 255u; o[2] = (v >> 16) & 255u; o[3] = v >> 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = k < n ? p[k] : 0u;
    }
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(VC_THREADS) void xbd_val_clear_kernel(unsigned long long* __restrict__ image_counts, int n) {
    const int i = blockIdx.x * VC_THREADS + threadIdx.x;
    if (i < n) image_counts[i] = 0;
}

// grid (gx, B): image blockIdx.y, groups of 4 pixels strided over gx workgroups
__global__ __launch_bounds__(VC_THREADS) void xbd_val_count_kernel(const float* __restrict__ logits,
                                                                   const unsigned char* __restrict__ msk0, long msk0_stride,
                                                                   const unsigned char* __restrict__ lbl, int W, long HW,
                                                                   float thr, int select,
                                                                   unsigned long long* __restrict__ image_counts,
                                                                   unsigned long long* __restrict__ class_counts) {
    __shared__ unsigned red[VC_WAVES][VC_NCOUNT];
    const int j = blockIdx.y;
    const float* lg = logits + (long)j * 5 * HW;
    const unsigned char* m0 = msk0 + (long)j * msk0_stride;
    const unsigned char* lb = lbl + (long)j * HW;
    // plane c starts at lg + c * HW: with HW % 4 != 0 the planes are aligned differently, so each one decides for itself
    bool vl[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) vl[c] = (reinterpret_cast<uintptr_t>(lg + c * HW) & 15) == 0;
    const bool vm = (reinterpret_cast<uintptr_t>(m0) & 3) == 0, vb = (reinterpret_cast<uintptr_t>(lb) & 3) == 0;

    unsigned cnt[VC_NCOUNT];
#pragma unroll
    for (int i = 0; i < VC_NCOUNT; ++i) cnt[i] = 0;

    const long groups = (HW + 3) >> 2;
#pragma unroll 2
    for (long g = (long)blockIdx.x * VC_THREADS + threadIdx.x; g < groups; g += (long)gridDim.x * VC_THREADS) {
        const long p0 = g << 2;
        const int n = HW - p0 >= 4 ? 4 : (int)(HW - p0);
        const bool full = n == 4;
        float x[5][4];
        unsigned gt[4], tg[4];
#pragma unroll
        for (int c = 0; c < 5; ++c) load4(lg + c * HW + p0, full && vl[c], n, x[c]);
        load4(m0 + p0, full && vm, n, gt);
        load4(lb + p0, full && vb, n, tg);
        int row = 0, col = 0;
        if (select == 0) {
            row = (int)(p0 / W);
            col = (int)(p0 - (long)row * W);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < n) {
                const bool loc = sigmoidf_(x[0][k]) > thr;
                float best = sigmoidf_(x[1][k]);
                unsigned arg = 0;
#pragma unroll
                for (int c = 2; c < 5; ++c) {
                    const float s = sigmoidf_(x[c][k]);
                    if (s > best) { best = s; arg = c - 1; }
                }
                const unsigned pred = loc ? arg : 0u;
                const bool g0 = gt[k] != 0;
                cnt[0] += g0;
                cnt[1] += loc;
                cnt[2] += g0 && loc;
                bool sel;
                if (select == 0) {
                    while (col >= W) { col -= W; ++row; }
                    sel = lb[row] != 0;          // lbl[j][0][row]: H == W, so row < W
                    ++col;
                } else {
                    sel = g0;
                }
                if (sel) {
                    const unsigned t = tg[k];
#pragma unroll
                    for (unsigned c = 0; c < 4; ++c) {
                        cnt[3 + 3 * c] += pred == c && t == c;
                        cnt[4 + 3 * c] += pred != c && t == c;
                        cnt[5 + 3 * c] += pred == c && t != c;
                    }
                }
            }
        }
    }

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < VC_NCOUNT; ++i) {
        const unsigned s = wave_sum_u32(cnt[i]);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < VC_NCOUNT) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < VC_WAVES; ++w) s += red[w][threadIdx.x];
        if (s) {
            unsigned long long* dst = threadIdx.x < 3 ? image_counts + (long)j * 3 + threadIdx.x : class_counts + (threadIdx.x - 3);
            atomicAdd(dst, (unsigned long long)s);
        }
    }
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int dh_xbd_val_count(const float* logits, const unsigned char* msk0, long msk0_image_stride,
                                const unsigned char* lbl, int B, int H, int W, float thr, int select, long long* image_counts,
                                long long* class_counts, void* stream) {
    DH_REQUIRE(logits && msk0 && lbl && image_counts && class_counts, "xbd_val_count: null pointer");
    DH_REQUIRE(B >= 1 && B <= 65535, "xbd_val_count: B=%d must be in 1..65535", B);
    DH_REQUIRE(H >= 1 && W >= 1, "xbd_val_count: empty image %dx%d", H, W);
    const long HW = (long)H * W;
    DH_REQUIRE(HW <= 0x7fffffffL, "xbd_val_count: %dx%d: a workgroup's 32-bit partial counts hold 2^31 - 1 pixels", H, W);
    DH_REQUIRE(thr > 0.f && thr < 1.f, "xbd_val_count: thr=%g must lie inside (0, 1)", (double)thr);      // (a nan fails too)
    DH_REQUIRE(select == 0 || select == 1, "xbd_val_count: select=%d (0 reference rows, 1 building pixels)", select);
    DH_REQUIRE(select != 0 || H == W,
               "xbd_val_count: the reference's row selection indexes axis 0 by the first row and needs H == W, got %dx%d", H, W);
    DH_REQUIRE(msk0_image_stride >= HW, "xbd_val_count: msk0_image_stride=%ld is less than one %dx%d plane", msk0_image_stride, H,
               W);
    DH_REQUIRE((reinterpret_cast<size_t>(logits) & 3) == 0 && (reinterpret_cast<size_t>(image_counts) & 7) == 0 &&
                   (reinterpret_cast<size_t>(class_counts) & 7) == 0, "xbd_val_count: misaligned pointer");
    // image_counts is written, not accumulated: cleared by a kernel of our own, so that a recorded step holds kernel nodes only
    // (a memset node in front of the count gave stale image rows on a later replay of the captured graph)
    hipLaunchKernelGGL(xbd_val_clear_kernel, dim3(dh_cdiv((long)B * 3, VC_THREADS)), dim3(VC_THREADS), 0, ST(stream),
                       reinterpret_cast<unsigned long long*>(image_counts), B * 3);
    DH_CHECK_LAUNCH("xbd_val_clear");
    int gx = dh_cdiv((HW + 3) / 4, VC_THREADS);
    const int cap = VC_MAX_WORKGROUPS / B > 0 ? VC_MAX_WORKGROUPS / B : 1;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(xbd_val_count_kernel, dim3(gx, B), dim3(VC_THREADS), 0, ST(stream), logits, msk0, msk0_image_stride, lbl, W,
                       HW, thr, select, reinterpret_cast<unsigned long long*>(image_counts),
                       reinterpret_cast<unsigned long long*>(class_counts));
    DH_CHECK_LAUNCH("xbd_val_count");
    return 0;
}
