// The 4-flip test-time augmentation of the xBD predictor (xBD_code/predict_test_cls.py:60-94) around the model's forward.
// flip_0 = identity, flip_1 reverses the rows, flip_2 the columns, flip_3 both; each is its own inverse.
//   pack:   x = concat(pre, post) over channels, [H][W][6] uint8; preprocess_inputs = (float)v / 127.f - 1.f, each operation
//           rounded to float32; inp[4n + k] = flip_k(x_n) as [6][H][W] fp32.  bgr = 1 reverses each RGB triple (what cv2.imread
//           hands the script), bgr = 0 keeps the stored order.  Every source byte is read once and written to its 4 destinations.
//   merge:  s_k = sigmoid(logits[4n + k]) in fp32, u_k = flip_k(s_k), mean = (((u_0 + u_1) + u_2) + u_3) / 4 in fp32 in THAT
//           order (numpy's mean over axis 0 of a float32 stack adds the slices one after the other),
//           out[n][y][x][c] = uint8(trunc(float32(mean * 255))), channels last.  The reference's astype('uint8') of a NaN is
//           undefined; here a NaN logit gives 0.
// Both are HBM-bound (pack: 6 B read, 96 B written per pixel; merge: 80 B read, 5 B written per pixel) and write every byte of
// their output, so a recorded step holds kernel nodes only: no memset, no copy node (see xbd_eval.hip).
#include "common.h"

namespace {

constexpr int TT_THREADS = 256;
constexpr int TT_MAX_WORKGROUPS = 512;      // over the whole batch: two workgroups per CU, the rest is the grid-stride loop

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }      // the sigmoid of xbd_eval.hip

// grid (gx, N): image blockIdx.y; groups of 4 consecutive pixels of one row, strided over gx workgroups.
// vec: W % 4 == 0, pre / post 4-byte aligned and inp 16-byte aligned -- then every group is three dwords per source and one
// float4 per destination plane (the column-reversed destination is the aligned vector at W - 4 - x0, reversed in registers).
__global__ __launch_bounds__(TT_THREADS) void xbd_tta_pack_kernel(const unsigned char* __restrict__ pre,
                                                                  const unsigned char* __restrict__ post, int H, int W, int bgr,
                                                                  int vec, float* __restrict__ inp) {
    __shared__ float lut[256];
    lut[threadIdx.x] = (float)threadIdx.x / 127.f - 1.f;      // preprocess_inputs: x /= 127, x -= 1, each rounded to float32
    __syncthreads();
    const long HW = (long)H * W;
    const int n = blockIdx.y;
    const unsigned char* src[2] = {pre + (long)n * HW * 3, post + (long)n * HW * 3};
    float* dst = inp + (long)n * 4 * 6 * HW;
    const int wg = (W + 3) >> 2;                               // groups per row
    const int groups = H * wg;                                 // (H * W < 2^31)
    for (long gl = (long)blockIdx.x * TT_THREADS + threadIdx.x; gl < groups; gl += (long)gridDim.x * TT_THREADS) {
        const int g = (int)gl, y = g / wg, x0 = (g - y * wg) << 2;
        const int cnt = W - x0 >= 4 ? 4 : W - x0;
        const long row = (long)y * W, rowf = (long)(H - 1 - y) * W;
#pragma unroll
        for (int im = 0; im < 2; ++im) {
            float v[3][4];                                     // [stored channel][pixel]
            const unsigned char* s = src[im] + (row + x0) * 3;
            if (vec) {
                const unsigned* s4 = reinterpret_cast<const unsigned*>(s);
                const unsigned d0 = s4[0], d1 = s4[1], d2 = s4[2];
                v[0][0] = lut[d0 & 255u];         v[1][0] = lut[(d0 >> 8) & 255u];  v[2][0] = lut[(d0 >> 16) & 255u];
                v[0][1] = lut[d0 >> 24];          v[1][1] = lut[d1 & 255u];         v[2][1] = lut[(d1 >> 8) & 255u];
                v[0][2] = lut[(d1 >> 16) & 255u]; v[1][2] = lut[d1 >> 24];          v[2][2] = lut[d2 & 255u];
                v[0][3] = lut[(d2 >> 8) & 255u];  v[1][3] = lut[(d2 >> 16) & 255u]; v[2][3] = lut[d2 >> 24];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) v[ch][j] = j < cnt ? lut[s[j * 3 + ch]] : 0.f;
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float(&a)[4] = v[ch];
                float* plane = dst + (long)(im * 3 + (bgr ? 2 - ch : ch)) * HW;      // flip k: + k * 6 * HW
                if (vec) {
                    const float r[4] = {a[3], a[2], a[1], a[0]};
                    const int xr = W - 4 - x0;
                    st4(plane + row + x0, a);
                    st4(plane + 6 * HW + rowf + x0, a);
                    st4(plane + 12 * HW + row + xr, r);
                    st4(plane + 18 * HW + rowf + xr, r);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (j < cnt) {
                            const int x = x0 + j, xr = W - 1 - x;
                            plane[row + x] = a[j];
                            plane[6 * HW + rowf + x] = a[j];
                            plane[12 * HW + row + xr] = a[j];
                            plane[18 * HW + rowf + xr] = a[j];
                        }
                    }
                }
            }
        }
    }
}

// 4 consecutive sigmoids of one plane's row, from column x (rev: the pixels x0 .. x0 + 3 seen through the column flip, that is
// columns W - 1 - x0 down to W - 4 - x0: the vector at W - 4 - x0, reversed in registers)
__device__ __forceinline__ void load_sig4(const float* __restrict__ rowp, int x0, int W, bool rev, bool vec, int cnt, float (&o)[4]) {
    if (vec) {
        float t[4];
        ld4(rowp + (rev ? W - 4 - x0 : x0), t);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = sigmoidf_(t[rev ? 3 - j : j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = j < cnt ? sigmoidf_(rowp[rev ? W - 1 - (x0 + j) : x0 + j]) : 0.f;
    }
}

__device__ __forceinline__ unsigned quantise(float mean) {
    const float v = mean * 255.f;
    return v >= 0.f ? (v < 255.f ? (unsigned)v : 255u) : 0u;      // a NaN compares false: 0
}

// grid (gx, N): image blockIdx.y; groups of 4 consecutive pixels of one row, strided over gx workgroups.  out_vec: W % 4 == 0
// and `out` 4-byte aligned, then a group's 20 output bytes are five dwords.
__global__ __launch_bounds__(TT_THREADS) void xbd_tta_merge_kernel(const float* __restrict__ logits, int H, int W, int out_vec,
                                                                   unsigned char* __restrict__ out) {
    const long HW = (long)H * W;
    const int n = blockIdx.y;
    const float* lg = logits + (long)n * 4 * 5 * HW;
    unsigned char* o = out + (long)n * HW * 5;
    // plane (k, c) starts at lg + (k * 5 + c) * HW: each one decides for itself whether its rows are aligned to the vector
    unsigned vl = 0;
    if ((W & 3) == 0) {
#pragma unroll
        for (int p = 0; p < 20; ++p) vl |= (unsigned)((reinterpret_cast<uintptr_t>(lg + p * HW) & 15) == 0) << p;
    }
    const int wg = (W + 3) >> 2;
    const int groups = H * wg;
    for (long gl = (long)blockIdx.x * TT_THREADS + threadIdx.x; gl < groups; gl += (long)gridDim.x * TT_THREADS) {
        const int g = (int)gl, y = g / wg, x0 = (g - y * wg) << 2;
        const int cnt = W - x0 >= 4 ? 4 : W - x0;
        const long row = (long)y * W, rowf = (long)(H - 1 - y) * W;
        unsigned q[5][4];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            float u[4][4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                load_sig4(lg + (long)(k * 5 + c) * HW + ((k & 1) ? rowf : row), x0, W, (k & 2) != 0, (vl >> (k * 5 + c)) & 1u, cnt,
                          u[k]);
#pragma unroll
            for (int j = 0; j < 4; ++j) q[c][j] = quantise((((u[0][j] + u[1][j]) + u[2][j]) + u[3][j]) * 0.25f);
        }
        unsigned char* po = o + (row + x0) * 5;
        if (out_vec) {
            unsigned d[5] = {0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 5; ++c) {
                    const int b = j * 5 + c;
                    d[b >> 2] |= q[c][j] << (8 * (b & 3));
                }
            unsigned* p4 = reinterpret_cast<unsigned*>(po);
#pragma unroll
            for (int i = 0; i < 5; ++i) p4[i] = d[i];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) {
#pragma unroll
                    for (int c = 0; c < 5; ++c) po[j * 5 + c] = (unsigned char)q[c][j];
                }
        }
    }
}

int grid_x(int N, int H, int W) {
    int gx = dh_cdiv((long)H * ((W + 3) / 4), TT_THREADS);
    const int cap = TT_MAX_WORKGROUPS / N > 0 ? TT_MAX_WORKGROUPS / N : 1;
    return gx > cap ? cap : gx;
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int dh_xbd_tta_pack_u8(const unsigned char* pre, const unsigned char* post, int N, int H, int W, int bgr, float* inp,
                                  void* stream) {
    DH_REQUIRE(pre && post && inp, "xbd_tta_pack: null pointer");
    DH_REQUIRE(N >= 1 && 4L * N <= 65535, "xbd_tta_pack: N=%d: the batch 4 N must be in 4..65535", N);
    DH_REQUIRE(H >= 1 && W >= 1, "xbd_tta_pack: empty image %dx%d", H, W);
    DH_REQUIRE((long)H * W <= 0x7fffffffL, "xbd_tta_pack: %dx%d: pixels of an image are indexed in 32 bits", H, W);
    DH_REQUIRE((reinterpret_cast<size_t>(inp) & 3) == 0, "xbd_tta_pack: misaligned pointer");
    const int vec = (W & 3) == 0 && (reinterpret_cast<size_t>(pre) & 3) == 0 && (reinterpret_cast<size_t>(post) & 3) == 0 &&
                    (reinterpret_cast<size_t>(inp) & 15) == 0;
    hipLaunchKernelGGL(xbd_tta_pack_kernel, dim3(grid_x(N, H, W), N), dim3(TT_THREADS), 0, ST(stream), pre, post, H, W,
                       bgr != 0, vec, inp);
    DH_CHECK_LAUNCH("xbd_tta_pack");
    return 0;
}

extern "C" int dh_xbd_tta_merge_u8(const float* logits, int N, int H, int W, unsigned char* out, void* stream) {
    DH_REQUIRE(logits && out, "xbd_tta_merge: null pointer");
    DH_REQUIRE(N >= 1 && 4L * N <= 65535, "xbd_tta_merge: N=%d: the batch 4 N must be in 4..65535", N);
    DH_REQUIRE(H >= 1 && W >= 1, "xbd_tta_merge: empty image %dx%d", H, W);
    DH_REQUIRE((long)H * W <= 0x7fffffffL, "xbd_tta_merge: %dx%d: pixels of an image are indexed in 32 bits", H, W);
    DH_REQUIRE((reinterpret_cast<size_t>(logits) & 3) == 0, "xbd_tta_merge: misaligned pointer");
    const int out_vec = (W & 3) == 0 && (reinterpret_cast<size_t>(out) & 3) == 0;
    hipLaunchKernelGGL(xbd_tta_merge_kernel, dim3(grid_x(N, H, W), N), dim3(TT_THREADS), 0, ST(stream), logits, H, W, out_vec,
                       out);
    DH_CHECK_LAUNCH("xbd_tta_merge");
    return 0;
}
