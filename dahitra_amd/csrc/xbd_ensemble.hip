// The xBD predictor (xBD_code/predict_test_cls.py:38-55, 81-91) for a list of M snapshots and V = 4 or 8 views of each pair.
// flip_k, k = 0..3, as in xbd_predict.hip: bit 0 reverses the rows, bit 1 the columns.  view_v = flip_v for v < 4, and
// view_{4+k}(x)[c][i][j] = flip_k(x)[c][j][i], the transpose of flip_k: the eight symmetries of the square (train_unettransformer.py
// trains with np.rot90 on top of the flips).  Undoing view 4 + k on an output s is flip_k(transpose(s)).  V = 8 needs H == W.
//   pack:   inp[V n + v] = view_v(concat(pre_n, post_n)) as [6][H][W] fp32, every byte b as (float)b / 127.f - 1.f.
//   merge:  u_{m,v} = un-view_v(sigmoid(logits_m[V n + v])), t = (((u_{0,0} + u_{0,1}) + ...) + u_{M-1,V-1}), model-major and
//           view-minor, one fp32 add after the other (the script's pred.append order under numpy's mean(axis=0)),
//           mean = t / (float)(M V), a true division, out[n][y][x][c] = uint8(trunc(mean * 255)), channels last, NaN -> 0.
// A transposed plane read row by row is a stride-W access, so both kernels work on 32 x 32 pixel tiles staged in LDS:
//   pack   one workgroup converts the tile's six planes into t[6][32][33] and writes its 32 rows of every view's destination tile:
//          a straight view reads LDS rows, a transposed one LDS columns.
//   merge  a thread owns 4 consecutive pixels of a tile row and keeps their 20 running sums in registers.  The straight views are
//          read from global memory as row segments; a transposed view's source tile (its 5 planes, sigmoid applied) is staged
//          in tt[5][32][33] in the source's own order and read by columns.
// Pitch 33: thread (r, q) = (tid / 8, tid % 8) touches dword (+-(4 q + e)) * 33 +- r or +-r * 33 +- (4 q + e); over the 32 lanes
// of a ds_read_b32 / ds_write_b32 group (4 values of r, 8 of q) the banks (+-r +- 4 q + const) mod 32 are all different.
// Traffic per pixel: pack 6 B read, 24 V B written; merge 20 M V B read, 5 B written.  Both write every byte of their output, so
// a recorded step holds kernel nodes only.
#include "common.h"

namespace {

constexpr int EN_THREADS = 256;
constexpr int EN_TILE = 32;                  // pixels per tile side; EN_THREADS = EN_TILE rows x EN_TILE / 4 groups of 4
constexpr int EN_PITCH = EN_TILE + 1;
constexpr int EN_MAX_MODELS = 8;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }      // the sigmoid of xbd_predict.hip

__device__ __forceinline__ unsigned quantise(float mean) {
    const float v = mean * 255.f;
    return v >= 0.f ? (v < 255.f ? (unsigned)v : 255u) : 0u;      // a NaN compares false: 0
}

__device__ __forceinline__ float norm_byte(unsigned b) { return (float)b / 127.f - 1.f; }      // preprocess_inputs, two roundings

// grid (tiles, N): tile blockIdx.x of image blockIdx.y.  VEC: W % 4 == 0 (and H % 4 == 0 when V == 8: H == W), pre / post 4-byte
// and inp 16-byte aligned: then a tile's sides are multiples of 4 and every group of 4 is three dwords in and one float4 out.
template <bool VEC>
__global__ __launch_bounds__(EN_THREADS) void xbd_pack_views_kernel(const unsigned char* __restrict__ pre,
                                                                    const unsigned char* __restrict__ post, int H, int W, int bgr,
                                                                    int V, float* __restrict__ inp) {
    __shared__ float t[6][EN_TILE][EN_PITCH];
    const long HW = (long)H * W;
    const int n = blockIdx.y;
    const int tiles_x = (W + EN_TILE - 1) / EN_TILE;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * EN_TILE, x0 = tx * EN_TILE;
    const int th = H - y0 < EN_TILE ? H - y0 : EN_TILE, tw = W - x0 < EN_TILE ? W - x0 : EN_TILE;
    const int r = threadIdx.x >> 3, q4 = (threadIdx.x & 7) << 2;
    if (r < th && q4 < tw) {
        const long at = ((long)(y0 + r) * W + x0 + q4) * 3;
#pragma unroll
        for (int im = 0; im < 2; ++im) {
            const unsigned char* s = (im ? post : pre) + (long)n * HW * 3 + at;
            unsigned b[12];
            if (VEC) {
                const unsigned* s4 = reinterpret_cast<const unsigned*>(s);
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const unsigned w = s4[d];
#pragma unroll
                    for (int k = 0; k < 4; ++k) b[4 * d + k] = (w >> (8 * k)) & 255u;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) b[k] = q4 + k / 3 < tw ? s[k] : 0u;
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float* row = t[im * 3 + (bgr ? 2 - ch : ch)][r];
#pragma unroll
                for (int j = 0; j < 4; ++j) row[q4 + j] = norm_byte(b[j * 3 + ch]);
            }
        }
    }
    __syncthreads();
    float* dst = inp + (long)n * V * 6 * HW;
    for (int v = 0; v < V; ++v) {
        const bool fr = v & 1, fc = v & 2, tr = v >= 4;
        // the destination tile: dh x dw, from (dy0, dx0), in a plane of `pitch` columns
        const int dh = tr ? tw : th, dw = tr ? th : tw, pitch = tr ? H : W;
        const int by = fr ? H - y0 - th : y0, bx = fc ? W - x0 - tw : x0;
        const int dy0 = tr ? bx : by, dx0 = tr ? by : bx;
        if (r >= dh || q4 >= dw) continue;
        // destination (r, q4 + e) holds the tile's pixel (ly, lx)
        const int a = (tr ? fc : fr) ? dh - 1 - r : r;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int bb = q4 + e;
                if (!VEC && bb >= dw) bb = dw - 1;
                bb = (tr ? fr : fc) ? dw - 1 - bb : bb;
                o[e] = tr ? t[c][bb][a] : t[c][a][bb];
            }
            float* p = dst + (long)(v * 6 + c) * HW + (long)(dy0 + r) * pitch + dx0 + q4;
            if (VEC) {
                st4(p, o);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (q4 + e < dw) p[e] = o[e];
            }
        }
    }
}

struct MergeTable {
    const float* lg[EN_MAX_MODELS];
};

// grid (tiles, N).  IN_VEC: W % 4 == 0 (so is H when V == 8) and every model's logits 16-byte aligned; out_vec: W % 4 == 0 and
// `out` 4-byte aligned, then a thread's 20 output bytes are five dwords.
template <bool IN_VEC>
__global__ __launch_bounds__(EN_THREADS) void xbd_merge_multi_kernel(MergeTable tab, int M, int V, int H, int W, int out_vec,
                                                                     unsigned char* __restrict__ out) {
    __shared__ float tt[5][EN_TILE][EN_PITCH];
    const long HW = (long)H * W;
    const int n = blockIdx.y;
    const int tiles_x = (W + EN_TILE - 1) / EN_TILE;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * EN_TILE, x0 = tx * EN_TILE;
    const int th = H - y0 < EN_TILE ? H - y0 : EN_TILE, tw = W - x0 < EN_TILE ? W - x0 : EN_TILE;
    const int r = threadIdx.x >> 3, q4 = (threadIdx.x & 7) << 2;
    const bool own = r < th && q4 < tw;                    // this thread has pixels (y0 + r, x0 + q4 ..)
    const int cnt = own ? (tw - q4 >= 4 ? 4 : tw - q4) : 0;
    float acc[5][4];
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[c][j] = 0.f;        // 0.f + u is u: a sigmoid is never -0
    for (int m = 0; m < M; ++m) {
        const float* lg = tab.lg[m] + (long)n * V * 5 * HW;
        // the straight views: row segments of the source, the column flip undone in registers
        for (int v = 0; v < 4; ++v) {
            if (!own) continue;
            const bool fr = v & 1, fc = v & 2;
            const long row = (long)(fr ? H - 1 - (y0 + r) : y0 + r) * W;
#pragma unroll
            for (int c = 0; c < 5; ++c) {
                const float* rowp = lg + (long)(v * 5 + c) * HW + row;
                if (IN_VEC) {
                    float s[4];
                    ld4(rowp + (fc ? W - 4 - (x0 + q4) : x0 + q4), s);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[c][j] += sigmoidf_(s[fc ? 3 - j : j]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < cnt) acc[c][j] += sigmoidf_(rowp[fc ? W - 1 - (x0 + q4 + j) : x0 + q4 + j]);
                }
            }
        }
        // the transposed views (H == W): u[y][x] = s[fc ? W - 1 - x : x][fr ? H - 1 - y : y].  The source tile has tw rows from
        // sy0 and th columns from sx0 and is staged as it lies; the owner of (ly = r, lx = q4 + j) reads tt[c][a][b].
        for (int v = 4; v < V; ++v) {
            const bool fr = v & 1, fc = v & 2;
            const int sy0 = fc ? W - x0 - tw : x0, sx0 = fr ? H - y0 - th : y0;
            __syncthreads();                               // the previous view's reads are done
            if (r < tw && q4 < th) {
                const long at = (long)(sy0 + r) * W + sx0 + q4;
#pragma unroll
                for (int c = 0; c < 5; ++c) {
                    const float* p = lg + (long)(v * 5 + c) * HW + at;
                    if (IN_VEC) {
                        float s[4];
                        ld4(p, s);
#pragma unroll
                        for (int e = 0; e < 4; ++e) tt[c][r][q4 + e] = sigmoidf_(s[e]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (q4 + e < th) tt[c][r][q4 + e] = sigmoidf_(p[e]);
                    }
                }
            }
            __syncthreads();
            if (own) {
                const int b = fr ? th - 1 - r : r;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j < cnt) {
                        const int a = fc ? tw - 1 - (q4 + j) : q4 + j;
#pragma unroll
                        for (int c = 0; c < 5; ++c) acc[c][j] += tt[c][a][b];
                    }
                }
            }
        }
    }
    if (!own) return;
    const float count = (float)(M * V);
    unsigned qv[5][4];
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) qv[c][j] = quantise(acc[c][j] / count);
    unsigned char* po = out + ((long)n * HW + (long)(y0 + r) * W + x0 + q4) * 5;
    if (out_vec) {
        unsigned d[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 5; ++c) {
                const int b = j * 5 + c;
                d[b >> 2] |= qv[c][j] << (8 * (b & 3));
            }
        unsigned* p4 = reinterpret_cast<unsigned*>(po);
#pragma unroll
        for (int i = 0; i < 5; ++i) p4[i] = d[i];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) {
#pragma unroll
                for (int c = 0; c < 5; ++c) po[j * 5 + c] = (unsigned char)qv[c][j];
            }
    }
}

// what both entries refuse about the shape; 0 when it is fine
int check_shape(const char* who, int V, int N, int H, int W) {
    DH_REQUIRE(V == 4 || V == 8, "%s: V=%d views: 4 (the flips) or 8 (with their transposes)", who, V);
    DH_REQUIRE(N >= 1 && (long)V * N <= 65535, "%s: N=%d: the batch V N must be in %d..65535", who, N, V);
    DH_REQUIRE(H >= 1 && W >= 1, "%s: empty image %dx%d", who, H, W);
    DH_REQUIRE((long)H * W <= 0x7fffffffL, "%s: %dx%d: pixels of an image are indexed in 32 bits", who, H, W);
    DH_REQUIRE(V == 4 || H == W, "%s: %dx%d: the transposed views need a square image", who, H, W);
    return 0;
}

int tiles(int H, int W) { return dh_cdiv(H, EN_TILE) * dh_cdiv(W, EN_TILE); }

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int dh_xbd_tta_pack_views_u8(const unsigned char* pre, const unsigned char* post, int N, int H, int W, int bgr, int V,
                                        float* inp, void* stream) {
    const char* who = "xbd_tta_pack_views";
    DH_REQUIRE(pre && post && inp, "%s: null pointer", who);
    if (check_shape(who, V, N, H, W)) return 1;
    DH_REQUIRE((reinterpret_cast<size_t>(inp) & 3) == 0, "%s: misaligned pointer", who);
    const bool vec = (W & 3) == 0 && (reinterpret_cast<size_t>(pre) & 3) == 0 && (reinterpret_cast<size_t>(post) & 3) == 0 &&
                     (reinterpret_cast<size_t>(inp) & 15) == 0;
    const dim3 grid(tiles(H, W), N);
    if (vec)
        hipLaunchKernelGGL(xbd_pack_views_kernel<true>, grid, dim3(EN_THREADS), 0, ST(stream), pre, post, H, W, bgr != 0, V, inp);
    else
        hipLaunchKernelGGL(xbd_pack_views_kernel<false>, grid, dim3(EN_THREADS), 0, ST(stream), pre, post, H, W, bgr != 0, V, inp);
    DH_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int dh_xbd_tta_merge_multi_u8(const float* const* logits_host_table, int M, int V, int N, int H, int W,
                                         unsigned char* out, void* stream) {
    const char* who = "xbd_tta_merge_multi";
    DH_REQUIRE(logits_host_table && out, "%s: null pointer", who);
    DH_REQUIRE(M >= 1 && M <= EN_MAX_MODELS, "%s: M=%d models: 1..%d", who, M, EN_MAX_MODELS);
    if (check_shape(who, V, N, H, W)) return 1;
    MergeTable tab;
    bool vec = (W & 3) == 0;
    for (int m = 0; m < EN_MAX_MODELS; ++m) {
        tab.lg[m] = m < M ? logits_host_table[m] : nullptr;
        if (m >= M) continue;
        DH_REQUIRE(tab.lg[m], "%s: the table's entry %d is null", who, m);
        DH_REQUIRE((reinterpret_cast<size_t>(tab.lg[m]) & 3) == 0, "%s: misaligned pointer (entry %d)", who, m);
        vec = vec && (reinterpret_cast<size_t>(tab.lg[m]) & 15) == 0;
    }
    const int out_vec = (W & 3) == 0 && (reinterpret_cast<size_t>(out) & 3) == 0;
    const dim3 grid(tiles(H, W), N);
    if (vec)
        hipLaunchKernelGGL(xbd_merge_multi_kernel<true>, grid, dim3(EN_THREADS), 0, ST(stream), tab, M, V, H, W, out_vec, out);
    else
        hipLaunchKernelGGL(xbd_merge_multi_kernel<false>, grid, dim3(EN_THREADS), 0, ST(stream), tab, M, V, H, W, out_vec, out);
    DH_CHECK_LAUNCH(who);
    return 0;
}
