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

// grid (gx, B): image blockIdx.y, groups of 4 pixels strided over gx workgroups.  ND: the damage classes -- logits [B][ND + 1][HW],
// counters 3 + 3 ND (4: train.py; 3: train_adapt.py, whose net merges destroyed into class 3)
template <int ND>
__global__ __launch_bounds__(VC_THREADS) void xbd_val_count_kernel(const float* __restrict__ logits,
                                                                   const unsigned char* __restrict__ msk0, long msk0_stride,
                                                                   const unsigned char* __restrict__ lbl, int W, long HW,
                                                                   float thr, int select,
                                                                   unsigned long long* __restrict__ image_counts,
                                                                   unsigned long long* __restrict__ class_counts) {
    constexpr int NCOUNT = 3 + 3 * ND;
    __shared__ unsigned red[VC_WAVES][NCOUNT];
    const int j = blockIdx.y;
    const float* lg = logits + (long)j * (ND + 1) * HW;
    const unsigned char* m0 = msk0 + (long)j * msk0_stride;
    const unsigned char* lb = lbl + (long)j * HW;
    // plane c starts at lg + c * HW: with HW % 4 != 0 the planes are aligned differently, so each one decides for itself
    bool vl[ND + 1];
#pragma unroll
    for (int c = 0; c < ND + 1; ++c) vl[c] = (reinterpret_cast<uintptr_t>(lg + c * HW) & 15) == 0;
    const bool vm = (reinterpret_cast<uintptr_t>(m0) & 3) == 0, vb = (reinterpret_cast<uintptr_t>(lb) & 3) == 0;

    unsigned cnt[NCOUNT];
#pragma unroll
    for (int i = 0; i < NCOUNT; ++i) cnt[i] = 0;

    const long groups = (HW + 3) >> 2;
#pragma unroll 2
    for (long g = (long)blockIdx.x * VC_THREADS + threadIdx.x; g < groups; g += (long)gridDim.x * VC_THREADS) {
        const long p0 = g << 2;
        const int n = HW - p0 >= 4 ? 4 : (int)(HW - p0);
        const bool full = n == 4;
        float x[ND + 1][4];
        unsigned gt[4], tg[4];
#pragma unroll
        for (int c = 0; c < ND + 1; ++c) load4(lg + c * HW + p0, full && vl[c], n, x[c]);
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
                for (int c = 2; c < ND + 1; ++c) {
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
                    for (unsigned c = 0; c < (unsigned)ND; ++c) {
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
    for (int i = 0; i < NCOUNT; ++i) {
        const unsigned s = wave_sum_u32(cnt[i]);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < NCOUNT) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < VC_WAVES; ++w) s += red[w][threadIdx.x];
        if (s) {
            unsigned long long* dst = threadIdx.x < 3 ? image_counts + (long)j * 3 + threadIdx.x : class_counts + (threadIdx.x - 3);
            atomicAdd(dst, (unsigned long long)s);
        }
    }
}

// ---- the threshold sweep: the same pass, binned by a grid of localisation thresholds -------------------------------------------
// Per pixel: bin = #{k : s0 > thr[k]} (0 .. T; the thresholds ascend, so s0 > thr[k] iff bin > k), arg as above, g0, and over the
// selected pixels t = min(lbl, 4).  A workgroup counts into ONE u32 LDS histogram: (T + 1) * 8 image cells [bin][arg][g0], then
// (T + 1) * 20 class cells [bin][arg][t]; one 64-bit integer atomic per non-zero cell and workgroup at the end.
// Real masks are mostly background: most lanes of a wave hit one cell, and an LDS add of 64 lanes on one address is 64 adds
// in a row.  So a thread first merges its own 4 pixels that share its first cell, and the wave merges every lane that shares
// the first active lane's cell into one add by a wave sum; what is left adds for itself.
constexpr int VS_MAX_T = 64;
constexpr int VS_ICELL = 8, VS_CCELL = 20;
constexpr int VS_MAX_CELLS = (VS_MAX_T + 1) * (VS_ICELL + VS_CCELL);

struct SweepThr { float v[VS_MAX_T]; };          // by value in the kernel arguments: a recorded graph owns its thresholds

// c[k]: the cell of pixel k, or -1.  Called by every lane of the wave (the shuffles read all 64).
__device__ __forceinline__ void sweep_add4(unsigned* __restrict__ h, const int (&c)[4], int lane) {
    int head = -1;
#pragma unroll
    for (int k = 3; k >= 0; --k) head = c[k] >= 0 ? c[k] : head;          // the first valid cell
    unsigned cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt += c[k] == head;
    const unsigned long long live = __ballot(head >= 0);
    if (live == 0) return;                                                // wave-uniform
    const int leader = __ffsll((long long)live) - 1;
    const int lead = __shfl(head, leader, 64);
    const bool match = head == lead;
    const unsigned total = wave_sum_u32(match ? cnt : 0u);
    if (lane == leader) atomicAdd(&h[lead], total);
    else if (!match && head >= 0) atomicAdd(&h[head], cnt);
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (c[k] >= 0 && c[k] != head) atomicAdd(&h[c[k]], 1u);
}

// grid (gx, B) as xbd_val_count_kernel; the loop's trip count is the same for every lane of a workgroup
__global__ __launch_bounds__(VC_THREADS) void xbd_val_sweep_kernel(const float* __restrict__ logits,
                                                                   const unsigned char* __restrict__ msk0, long msk0_stride,
                                                                   const unsigned char* __restrict__ lbl, int W, long HW,
                                                                   SweepThr thr, int T, int select,
                                                                   unsigned long long* __restrict__ image_hist,
                                                                   unsigned long long* __restrict__ class_hist) {
    __shared__ unsigned hist[VS_MAX_CELLS];
    const int ni = (T + 1) * VS_ICELL, ncell = (T + 1) * (VS_ICELL + VS_CCELL);
    for (int i = threadIdx.x; i < ncell; i += VC_THREADS) hist[i] = 0;
    __syncthreads();
    const int j = blockIdx.y, lane = threadIdx.x & 63;
    const float* lg = logits + (long)j * 5 * HW;
    const unsigned char* m0 = msk0 + (long)j * msk0_stride;
    const unsigned char* lb = lbl + (long)j * HW;
    bool vl[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) vl[c] = (reinterpret_cast<uintptr_t>(lg + c * HW) & 15) == 0;
    const bool vm = (reinterpret_cast<uintptr_t>(m0) & 3) == 0, vb = (reinterpret_cast<uintptr_t>(lb) & 3) == 0;

    const long groups = (HW + 3) >> 2;
    for (long gb = (long)blockIdx.x * VC_THREADS; gb < groups; gb += (long)gridDim.x * VC_THREADS) {
        const long g = gb + threadIdx.x;
        const long p0 = g << 2;
        const int n = g >= groups ? 0 : (HW - p0 >= 4 ? 4 : (int)(HW - p0));          // 0: a lane past the plane loads nothing
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
        float s0[4];
        int ci[4], cc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ci[k] = cc[k] = -1;
            s0[k] = 0.f;
            if (k < n) {
                s0[k] = sigmoidf_(x[0][k]);
                float best = sigmoidf_(x[1][k]);
                unsigned arg = 0;
#pragma unroll
                for (int c = 2; c < 5; ++c) {
                    const float s = sigmoidf_(x[c][k]);
                    if (s > best) { best = s; arg = c - 1; }
                }
                const bool g0 = gt[k] != 0;
                bool sel;
                if (select == 0) {
                    while (col >= W) { col -= W; ++row; }
                    sel = lb[row] != 0;          // lbl[j][0][row]: H == W, so row < W
                    ++col;
                } else {
                    sel = g0;
                }
                const unsigned t = tg[k] < 4u ? tg[k] : 4u;
                ci[k] = (int)(arg * 2 + g0);                       // + bin * 8 below
                cc[k] = sel ? ni + (int)(arg * 5 + t) : -1;        // + bin * 20 below
            }
        }
        int bin[4] = {0, 0, 0, 0};
#pragma unroll 4
        for (int q = 0; q < T; ++q) {
            const float th = thr.v[q];
#pragma unroll
            for (int k = 0; k < 4; ++k) bin[k] += s0[k] > th;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (ci[k] >= 0) ci[k] += bin[k] * VS_ICELL;
            if (cc[k] >= 0) cc[k] += bin[k] * VS_CCELL;
        }
        sweep_add4(hist, ci, lane);
        sweep_add4(hist, cc, lane);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ncell; i += VC_THREADS) {
        const unsigned s = hist[i];
        if (s) atomicAdd(i < ni ? image_hist + (long)j * ni + i : class_hist + (i - ni), (unsigned long long)s);
    }
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

namespace {
template <int ND>
int xbd_val_count_impl(const float* logits, const unsigned char* msk0, long msk0_image_stride, const unsigned char* lbl, int B, int H,
                       int W, float thr, int select, long long* image_counts, long long* class_counts, void* stream) {
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
    hipLaunchKernelGGL(xbd_val_count_kernel<ND>, dim3(gx, B), dim3(VC_THREADS), 0, ST(stream), logits, msk0, msk0_image_stride, lbl, W,
                       HW, thr, select, reinterpret_cast<unsigned long long*>(image_counts),
                       reinterpret_cast<unsigned long long*>(class_counts));
    DH_CHECK_LAUNCH("xbd_val_count");
    return 0;
}
}  // namespace

extern "C" int dh_xbd_val_count(const float* logits, const unsigned char* msk0, long msk0_image_stride,
                                const unsigned char* lbl, int B, int H, int W, float thr, int select, long long* image_counts,
                                long long* class_counts, void* stream) {
    return xbd_val_count_impl<4>(logits, msk0, msk0_image_stride, lbl, B, H, W, thr, select, image_counts, class_counts, stream);
}

// dh_xbd_val_count for logits [B][n_damage + 1][H][W] and class_counts [n_damage][3]: n_damage 4 is that call, 3 the pass of
// xBD_code/train_adapt.py:262-280 (three damage classes, lbl 0 .. 2)
extern "C" int dh_xbd_val_count_n(const float* logits, const unsigned char* msk0, long msk0_image_stride, const unsigned char* lbl,
                                  int n_damage, int B, int H, int W, float thr, int select, long long* image_counts,
                                  long long* class_counts, void* stream) {
    DH_REQUIRE(n_damage == 3 || n_damage == 4, "xbd_val_count: n_damage=%d is neither 3 nor 4", n_damage);
    if (n_damage == 3)
        return xbd_val_count_impl<3>(logits, msk0, msk0_image_stride, lbl, B, H, W, thr, select, image_counts, class_counts, stream);
    return xbd_val_count_impl<4>(logits, msk0, msk0_image_stride, lbl, B, H, W, thr, select, image_counts, class_counts, stream);
}

extern "C" int dh_xbd_val_sweep(const float* logits, const unsigned char* msk0, long msk0_image_stride,
                                const unsigned char* lbl, int B, int H, int W, const float* thr, int T, int select,
                                long long* image_hist, long long* class_hist, void* stream) {
    DH_REQUIRE(logits && msk0 && lbl && thr && image_hist && class_hist, "xbd_val_sweep: null pointer");
    DH_REQUIRE(B >= 1 && B <= 65535, "xbd_val_sweep: B=%d must be in 1..65535", B);
    DH_REQUIRE(H >= 1 && W >= 1, "xbd_val_sweep: empty image %dx%d", H, W);
    const long HW = (long)H * W;
    DH_REQUIRE(HW <= 0x7fffffffL, "xbd_val_sweep: %dx%d: a workgroup's 32-bit partial counts hold 2^31 - 1 pixels", H, W);
    DH_REQUIRE(T >= 1 && T <= VS_MAX_T, "xbd_val_sweep: T=%d thresholds, must be in 1..%d", T, VS_MAX_T);
    SweepThr th;
    for (int k = 0; k < VS_MAX_T; ++k) th.v[k] = 2.f;          // past T: never read
    for (int k = 0; k < T; ++k) {          // thr is host memory
        DH_REQUIRE(thr[k] > 0.f && thr[k] < 1.f, "xbd_val_sweep: thr[%d]=%g must lie inside (0, 1)", k, (double)thr[k]);      // (nan too)
        DH_REQUIRE(k == 0 || thr[k] > thr[k - 1], "xbd_val_sweep: thr[%d]=%g is not above thr[%d]=%g: the grid ascends strictly", k,
                   (double)thr[k], k - 1, (double)thr[k - 1]);
        th.v[k] = thr[k];
    }
    DH_REQUIRE(select == 0 || select == 1, "xbd_val_sweep: select=%d (0 reference rows, 1 building pixels)", select);
    DH_REQUIRE(select != 0 || H == W,
               "xbd_val_sweep: the reference's row selection indexes axis 0 by the first row and needs H == W, got %dx%d", H, W);
    DH_REQUIRE(msk0_image_stride >= HW, "xbd_val_sweep: msk0_image_stride=%ld is less than one %dx%d plane", msk0_image_stride, H,
               W);
    DH_REQUIRE((reinterpret_cast<size_t>(logits) & 3) == 0 && (reinterpret_cast<size_t>(image_hist) & 7) == 0 &&
                   (reinterpret_cast<size_t>(class_hist) & 7) == 0, "xbd_val_sweep: misaligned pointer");
    // image_hist is written, not accumulated: cleared by the kernel dh_xbd_val_count clears with, for the same reason
    const int ni = B * (T + 1) * VS_ICELL;
    hipLaunchKernelGGL(xbd_val_clear_kernel, dim3(dh_cdiv(ni, VC_THREADS)), dim3(VC_THREADS), 0, ST(stream),
                       reinterpret_cast<unsigned long long*>(image_hist), ni);
    DH_CHECK_LAUNCH("xbd_val_sweep clear");
    int gx = dh_cdiv((HW + 3) / 4, VC_THREADS);
    const int cap = VC_MAX_WORKGROUPS / B > 0 ? VC_MAX_WORKGROUPS / B : 1;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(xbd_val_sweep_kernel, dim3(gx, B), dim3(VC_THREADS), 0, ST(stream), logits, msk0, msk0_image_stride, lbl, W,
                       HW, th, T, select, reinterpret_cast<unsigned long long*>(image_hist),
                       reinterpret_cast<unsigned long long*>(class_hist));
    DH_CHECK_LAUNCH("xbd_val_sweep");
    return 0;
}
