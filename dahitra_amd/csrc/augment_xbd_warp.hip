// Input pipeline of DAHiTra's own xBD training script on the device (gfx950): TrainData.__getitem__ of
// xBD_code/train_unettransformer.py:109-167, 206-209 and 255-279 for pre-decoded samples.  Per sample: the S x S crop, the
// vertical flip, np.rot90(., k), shift_image (cv2.warpAffine with an integer translation, BORDER_REFLECT_101), rotate_image
// (cv2.warpAffine, INTER_LINEAR, BORDER_REFLECT_101), shift_channels on one of the two images, preprocess_inputs and the five
// mask channels.  One launch per batch, no intermediate image.
//
// Everything between the crop and the bytes is ONE gather.  An output pixel (x, y) has four taps (u, v), (u + 1, v), (u, v + 1),
// (u + 1, v + 1) in the image the warp reads, and a tap is an index chain back to the source, each coordinate on its own:
//   1. reflect-101 into 0 .. S - 1                          (the warp's border)
//   2. minus the shift (sx along x, sy along y)             (shift_image: dst(x, y) = src(x - sx, y - sy), fractions 0)
//   3. reflect-101 again                                    (the shift's border; its result is the S x S image the warp reads)
//   4. undo rot90: with (r, c) the row and column so far, k = 1: (c, S-1-r), 2: (S-1-r, S-1-c), 3: (S-1-c, r)
//   5. undo the vertical flip on the row
//   6. plus the crop origin, clamped into the image
// reflect-101 is closed form: m = 2 (S - 1), p mod m (non-negative), p >= S ? m - p : p; 0 for S == 1.
//
// The warp is OpenCV's fixed-point path (4.x up to 4.10, imgwarp.cpp, CV_8U): the host inverts the matrix in float64 and writes
// tab [N][4][S] int32 = adelta[x], bdelta[x], X0[y], Y0[y] (datasets/xbd_pipeline.unet_warp_table); here
//   X = (X0[y] + adelta[x]) >> 5, Y = (Y0[y] + bdelta[x]) >> 5, (u, v) = (X >> 5, Y >> 5), fx = X & 31, fy = Y & 31,
//   weights (32 - fx)(32 - fy) 32, fx (32 - fy) 32, (32 - fx) fy 32, fx fy 32 (their sum is 32768),
//   byte = (sum_k w_k v_k + 16384) >> 15.
// A sample without the warp flag is the single tap (x, y) at weight 32768, which returns the byte itself: the same code with one
// tap, so a crop / flip / rot90 / shift sample costs a quarter of the loads.  A tap of weight 0 is still read: every chain ends
// inside 0 .. S - 1 and every source coordinate is clamped into the image, so no table or row makes the kernel read outside.
//
// Masks: the script warps the 0 / 255 indicator plane of every class and thresholds > 127, so channel c = 1 .. 4 is
// ((255 * (weights of the taps whose label == c) + 16384) >> 15) > 127, each on its own (two classes at weight 1/2 are both
// set), and channel 0 is any of them (the script clears the warped pre mask, line 264).
//
// Layout: a workgroup owns a WT_W x WT_H tile of one sample's output, a lane four pixels of a row: 6 float4 and 5 dword stores.
// The taps are gathered straight from global memory.  The tile is square so that its source footprint is the same ~ (WT + 2)^2
// pixels whichever way rot90 turns it (7 bytes a pixel: 8 KiB, a quarter of a CU's vector L1): a quarter turn makes a lane's
// four pixels and a wave's 32 columns walk down source rows, but the lines they touch are the ones the tile's other rows touch
// too.  Measured on the script's own parameter distribution the launch takes 1.06 x the time of augment_xbd.hip's kernel, whose
// reads run along rows through LDS: staging the footprint in LDS was not built ("xBD loader: the DAHiTra
// script's geometry", has the times).
#include "common.h"

#ifndef DH_XBD_WARP_TW
#define DH_XBD_WARP_TW 32
#endif
#ifndef DH_XBD_WARP_TH
#define DH_XBD_WARP_TH 32
#endif

namespace {

constexpr int XW_PW = 12;              // int32 words of a parameter row
constexpr int XW_MAX_SHIFT = 1 << 20;  // a shift beyond it is clamped: the chain's subtraction stays inside int32

// cv2.BORDER_REFLECT_101 of any p into 0 .. S - 1; m = 2 (S - 1)
__device__ __forceinline__ int reflect101(int p, int S, int m) {
    if (m == 0) return 0;
    p %= m;
    if (p < 0) p += m;
    return p >= S ? m - p : p;
}

template <int TW, int TH>
__global__ __launch_bounds__(256) void xbd_augment_warp_kernel(
    const unsigned char* __restrict__ pre, const unsigned char* __restrict__ post, const unsigned char* __restrict__ label,
    const int* __restrict__ idx, const int* __restrict__ params, const int* __restrict__ tab, int H, int W, int S,
    float* __restrict__ out_img, unsigned char* __restrict__ out_msk, int vec4, int mvec4) {
    constexpr int CG = TW / 4;             // lanes (groups of four columns) of a row
    static_assert(TW % 4 == 0 && CG * TH == 256, "a lane takes four pixels of a row and 256 lanes take the tile");
    __shared__ float lut[256];
    const int tid = threadIdx.x, n = blockIdx.z;
    // preprocess_inputs: x /= 127, x -= 1, each rounded to float32 (augment_xbd.hip's table)
    lut[tid] = (float)tid / 127.f - 1.f;
    __syncthreads();
    const int oy = blockIdx.y * TH + tid / CG, ox = blockIdx.x * TW + 4 * (tid % CG);
    if (oy >= S || ox >= S) return;

    const int* pr = params + (long)n * XW_PW;
    const int x0 = pr[0], y0 = pr[1], vf = pr[2] != 0, rot = pr[3] & 3;
    const int sx = min(max(pr[4], -XW_MAX_SHIFT), XW_MAX_SHIFT), sy = min(max(pr[5], -XW_MAX_SHIFT), XW_MAX_SHIFT);
    const bool warp = pr[6] != 0 && tab != nullptr;
    const int chan = pr[7];                // shift_channels: 0 nobody, 1 the pre image, 2 the post image
    const int dch[3] = {pr[8], pr[9], pr[10]};                             // added to planes R, G, B
    const int m = 2 * (S - 1);
    const int* tb = tab + (long)n * 4 * S;
    const long sbase = (long)idx[n] * H * W;
    const long plane = (long)S * S;

    // pixel offset in the source image of (row r, column c) of the image the warp reads, both in 0 .. S - 1 already
    auto source = [&](int r, int c) {
        const int a = rot == 0 ? r : rot == 1 ? c : rot == 2 ? S - 1 - r : S - 1 - c;
        const int b = rot == 0 ? c : rot == 1 ? S - 1 - r : rot == 2 ? S - 1 - c : r;
        const int y = min(max(y0 + (vf ? S - 1 - a : a), 0), H - 1), x = min(max(x0 + b, 0), W - 1);
        return sbase + (long)y * W + x;
    };
    auto col = [&](int u) { return reflect101(reflect101(u, S, m) - sx, S, m); };
    auto row = [&](int v) { return reflect101(reflect101(v, S, m) - sy, S, m); };

    unsigned img[6] = {0, 0, 0, 0, 0, 0}, msk[5] = {0, 0, 0, 0, 0};        // four packed bytes each
    const int tY0 = warp ? tb[3 * S + oy] : 0, tX0 = warp ? tb[2 * S + oy] : 0;
    const int ntap = warp ? 4 : 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = min(ox + j, S - 1);                                   // a column past S repeats the last one; it is not stored
        int u = x, v = oy, fx = 0, fy = 0;
        if (warp) {
            const int X = (int)((unsigned)tX0 + (unsigned)tb[x]) >> 5, Y = (int)((unsigned)tY0 + (unsigned)tb[S + x]) >> 5;
            u = X >> 5, v = Y >> 5, fx = X & 31, fy = Y & 31;
        }
        const int c0 = col(u), r0 = row(v);
        const int c1 = warp ? col(u + 1) : c0, r1 = warp ? row(v + 1) : r0;
        const long at[4] = {source(r0, c0), source(r0, c1), source(r1, c0), source(r1, c1)};
        const int w[4] = {(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32};
        int acc[6] = {0, 0, 0, 0, 0, 0}, wc[4] = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t >= ntap) break;                                           // uniform over the workgroup
            const unsigned char* a = pre + at[t] * 3;
            const unsigned char* b = post + at[t] * 3;
            const int l = label[at[t]];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[ch] += w[t] * (int)a[ch], acc[3 + ch] += w[t] * (int)b[ch];
#pragma unroll
            for (int c = 0; c < 4; ++c) wc[c] += l == c + 1 ? w[t] : 0;
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            int byte = (acc[p] + 16384) >> 15;
            if (chan == 1 + p / 3) byte = min(max(byte + dch[p % 3], 0), 255);
            img[p] |= ((unsigned)byte & 255u) << (8 * j);
        }
        unsigned any = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned on = ((255 * wc[c] + 16384) >> 15) > 127 ? 1u : 0u;
            msk[1 + c] |= on << (8 * j);
            any |= on;
        }
        msk[0] |= any << (8 * j);
    }

    const long at = (long)oy * S + ox;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        float* dst = out_img + ((long)n * 6 + p) * plane + at;
        const unsigned d = img[p];
        if (vec4) {                                                         // S % 4 == 0 and a 16-byte aligned output
            *reinterpret_cast<float4*>(dst) = make_float4(lut[d & 255u], lut[(d >> 8) & 255u], lut[(d >> 16) & 255u], lut[d >> 24]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ox + j < S) dst[j] = lut[(d >> (8 * j)) & 255u];
        }
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        unsigned char* dst = out_msk + ((long)n * 5 + c) * plane + at;
        if (mvec4) {                                                        // S % 4 == 0 and a 4-byte aligned output
            *reinterpret_cast<unsigned*>(dst) = msk[c];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ox + j < S) dst[j] = (unsigned char)((msk[c] >> (8 * j)) & 255u);
        }
    }
}

}  // namespace

extern "C" int dh_xbd_augment_warp_tile_h(void) { return DH_XBD_WARP_TH; }
extern "C" int dh_xbd_augment_warp_tile_w(void) { return DH_XBD_WARP_TW; }

extern "C" int dh_xbd_augment_warp_u8(const unsigned char* pre, const unsigned char* post, const unsigned char* post_label,
                                      const int* idx, const int* params, const int* tab, int N, int H, int W, int S,
                                      float* out_img, unsigned char* out_msk, void* stream) {
    constexpr int TW = DH_XBD_WARP_TW, TH = DH_XBD_WARP_TH;
    const char* who = "xbd_augment_warp";
    DH_REQUIRE(N > 0 && S > 0 && S <= H && S <= W, "%s: bad sizes N=%d %dx%d -> %d", who, N, H, W, S);
    DH_REQUIRE(N <= 65535 && dh_cdiv(S, TH) <= 65535, "%s: N=%d S=%d exceed the launch grid", who, N, S);
    DH_REQUIRE(pre != nullptr && post != nullptr && post_label != nullptr && idx != nullptr && params != nullptr,
               "%s: a source or table pointer is NULL", who);
    DH_REQUIRE(out_img != nullptr && out_msk != nullptr, "%s: an output pointer is NULL", who);
    const int vec4 = S % 4 == 0 && (uintptr_t)out_img % 16 == 0;
    const int mvec4 = S % 4 == 0 && (uintptr_t)out_msk % 4 == 0;
    hipLaunchKernelGGL((xbd_augment_warp_kernel<TW, TH>), dim3(dh_cdiv(S, TW), dh_cdiv(S, TH), N), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), pre, post, post_label, idx, params, tab, H, W, S, out_img, out_msk,
                       vec4, mvec4);
    DH_CHECK_LAUNCH(who);
    return 0;
}
