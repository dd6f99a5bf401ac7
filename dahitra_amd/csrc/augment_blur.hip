// Input pipeline on the device, with the reference's random Gaussian blur (gfx950).
// CDDataAugmentation.transform (datasets/data_utils.py:55-111) in training mode: crop window, horizontal / vertical flip,
// img.filter(ImageFilter.GaussianBlur(radius=random.random())) on both images (data_utils.py:99-102), ToTensor +
// Normalize(0.5, 0.5).  augment_pairs_u8_kernel (pointwise.hip) is the same pass without the blur; this one is byte-exact
// against Pillow's filter.
//
// Pillow's GaussianBlur is three box-blur passes along the rows, then three along the columns, each pass in integer arithmetic
// on uint8 with a rounding to uint8 at its end and the line's edge pixel replicated (BoxBlur.c).  For radius < sqrt(2) the box
// has integer radius 0 and a fractional part, so a pass is the 3-tap filter
//     out[x] = (in[x] * ww + (in[x - 1] + in[x + 1]) * fw + (1 << 23)) >> 24        (unsigned 32 bits: 255 ww + 510 fw + 2^23 > 2^31)
// with per-sample 8.24 fixed-point weights (ww, fw), ww + 2 fw <= 1 << 24, derived on the host (gpu_pipeline.box_blur_weights).
// The filter is symmetric, so it commutes with the flips: the tile is loaded already flipped and blurred in output orientation.
//
// A workgroup owns a TW x TH tile of one image (A or B) of one sample.  It stages the tile plus a 3-pixel halo as interleaved RGB
// bytes in LDS -- the arithmetic does not care about channels: along a row the neighbours of byte i are bytes i - 3 and i + 3,
// along a column the same byte of the rows above and below -- runs the six passes between two LDS images, four bytes (one dword)
// per lane and step, and stores the normalised fp32 planes, 16 bytes per lane and channel.
//   * Replication is per pass and at the border of the CROP WINDOW: a tap that would leave the window reads the centre byte
//     instead (byte masks along x, the row index along y).  Source pixels outside the window are never loaded; LDS bytes outside
//     it hold arbitrary values that no in-window result depends on.
//   * At tile borders inside the window the halo supplies real neighbours: after pass k the outermost k halo pixels are stale,
//     after three passes exactly the tile is valid.  The row passes run on the halo rows too (the column passes read them).
//   * Normalisation: augment_pairs_u8_kernel's expression, evaluated once per byte value into a 256-entry table (an IEEE
//     division per output value is about ten vector instructions, against about six per byte and pass for the blur), so
//     (ww, fw) = (1 << 24, 0) gives that kernel's bits.
#include "common.h"

// tile of a workgroup ("Device loader: the random Gaussian blur": tile shape and measured rate)
#ifndef DH_BLUR_TW
#define DH_BLUR_TW 64
#endif
#ifndef DH_BLUR_TH
#define DH_BLUR_TH 32
#endif

namespace {

// one pass on four packed bytes: centre C, the two neighbours L / R byte for byte.  ww < 2^24 and fw < 2^23 (s <= 510), so both
// products are exact 24-bit multiplies and the sum stays below 2^32.
__device__ __forceinline__ unsigned blur_tap4(unsigned C, unsigned L, unsigned R, unsigned ww, unsigned fw) {
    unsigned o = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned c = (C >> (8 * k)) & 255u;
        const unsigned s = ((L >> (8 * k)) & 255u) + ((R >> (8 * k)) & 255u);
        const unsigned acc = __umul24(c, ww) + __umul24(s, fw) + (1u << 23);
        o |= (acc >> 24) << (8 * k);
    }
    return o;
}

template <int TW, int TH>
__global__ __launch_bounds__(256) void augment_pairs_blur_u8_kernel(
    const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, const unsigned char* __restrict__ l,
    const int* __restrict__ idx, const int* __restrict__ params, const int* __restrict__ blur, int H, int W, int h, int w,
    float* __restrict__ oa, float* __restrict__ ob, unsigned char* __restrict__ ol, int vec) {
    static_assert(TW % 4 == 0, "a lane stores 4 pixels");
    constexpr int RB = 3 * TW + 24;        // bytes of an LDS row: 3 pad, 9 halo, 3 TW tile (starts dword-aligned at 12), 9 halo, 3 pad
    constexpr int RWD = RB / 4;            // ... in dwords
    constexpr int ROWS = TH + 6;
    constexpr int LB = 3 * (TW + 6);       // loaded bytes of a row, at byte 3
    constexpr int CW = 3 * TW / 4;         // dwords of the tile proper, at dword 3
    __shared__ unsigned s[2][ROWS * RWD];
    __shared__ float lut[256];
    const int tid = threadIdx.x;
    const int n = blockIdx.z >> 1, img = blockIdx.z & 1;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const int* pr = params + n * 4;
    const int x0 = pr[0], y0 = pr[1], hf = pr[2], vf = pr[3];
    // ww = 1 << 24 (the identity; then fw = 0) does not fit a 24-bit multiply: (c * (2^24 - 1) + 2^23) >> 24 is c as well
    const unsigned ww = min((unsigned)blur[2 * n], (1u << 24) - 1u), fw = (unsigned)blur[2 * n + 1];
    const long sbase = (long)idx[n] * H * W;
    const unsigned char* src = (img ? b : a) + sbase * 3;
    const long plane = (long)h * w;

    lut[tid] = ((float)tid / 255.f - 0.5f) / 0.5f;       // ToTensor then Normalize: same roundings
    unsigned char* sb = reinterpret_cast<unsigned char*>(s[0]);
    // thread t < LB owns byte column t of the staged rows: its source column is fixed.  All of its loads are issued before the
    // first LDS write, so the thread waits for memory once and not once per few rows (ROWS byte registers per lane; the lanes
    // past LB idle here); a staged row outside the window takes the nearest row inside it -- never a source row outside the
    // window -- and is not used by any in-window result.
    static_assert(LB <= 256, "one thread per staged byte column");
    const int rlo = max(0, 3 - ty0), rhi = min(ROWS, h - ty0 + 3);      // staged rows inside the window: rlo < rhi
    const int ox = tx0 - 3 + tid / 3;
    if (tid < LB && (unsigned)ox < (unsigned)w) {
        const unsigned char* sc = src + (long)(x0 + (hf ? w - 1 - ox : ox)) * 3 + tid % 3;
        unsigned char v[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int oy = ty0 - 3 + min(max(r, rlo), rhi - 1);
            v[r] = sc[(long)(y0 + (vf ? h - 1 - oy : oy)) * W * 3];
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) sb[r * RB + 3 + tid] = v[r];
    }
    if (img == 0 && l != nullptr && ol != nullptr) {
        for (int j = tid; j < TH * TW; j += 256) {
            const int oy = ty0 + j / TW, ox = tx0 + j % TW;
            if (oy < h && ox < w) {
                const int sx = x0 + (hf ? w - 1 - ox : ox), sy = y0 + (vf ? h - 1 - oy : oy);
                ol[(long)n * plane + (long)oy * w + ox] = l[sbase + (long)sy * W + sx];
            }
        }
    }
    __syncthreads();

    int cur = 0;
    // ---- three passes along the rows, on every staged row ----
    const bool edge_x = tx0 == 0 || tx0 + TW + 3 >= w;      // the tile or its halo touches the window's left / right border
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const unsigned* in = s[cur];
        unsigned* out = s[cur ^ 1];
        for (int u = tid; u < ROWS * RWD; u += 256) {
            const int col = u % RWD;
            if (col == 0 || col == RWD - 1) continue;         // pad dwords: no neighbour dword on one side
            const unsigned C = in[u];
            unsigned L = __builtin_amdgcn_alignbyte(C, in[u - 1], 1);        // bytes i - 3 .. i
            unsigned R = __builtin_amdgcn_alignbyte(in[u + 1], C, 3);        // bytes i + 3 .. i + 6
            if (edge_x) {
                const int gb = 3 * tx0 - 12 + 4 * col;       // byte index of the dword's byte 0 in the window's row
                const int nl = 3 - gb;                        // bytes k < nl are pixel 0 (or left of it): left tap = centre
                const int nr = 3 * w - 3 - gb;                // bytes k >= nr are pixel w - 1 (or right of it): right tap = centre
                const unsigned mL = nl <= 0 ? 0u : (nl >= 4 ? ~0u : (1u << (8 * nl)) - 1u);
                const unsigned mR = nr <= 0 ? ~0u : (nr >= 4 ? 0u : ~((1u << (8 * nr)) - 1u));
                L = (C & mL) | (L & ~mL);
                R = (C & mR) | (R & ~mR);
            }
            out[u] = blur_tap4(C, L, R, ww, fw);
        }
        __syncthreads();
        cur ^= 1;
    }
    // ---- three passes along the columns, on the tile's own bytes; the rows still needed shrink by one per pass.  A thread keeps
    // its dword column and strides over the rows (a flat index over rows x columns needs a division and a multiply per tap
    // address in every step) ----
    constexpr int NRG = 256 / CW;                              // row groups; the threads past NRG * CW idle in these passes
    const int ccol = 3 + tid % CW, rg = tid / CW;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const unsigned* in = s[cur];
        unsigned* out = s[cur ^ 1];
        if (rg < NRG) {
            for (int r = 1 + pass + rg; r < ROWS - 1 - pass; r += NRG) {
                const int oy = ty0 - 3 + r;
                const unsigned* q = in + r * RWD + ccol;
                out[r * RWD + ccol] = blur_tap4(q[0], q[oy == 0 ? 0 : -RWD], q[oy == h - 1 ? 0 : RWD], ww, fw);
            }
        }
        __syncthreads();
        cur ^= 1;
    }

    // ---- normalise and store: a lane takes 4 pixels = 12 bytes = 3 dwords and writes 4 consecutive floats of each plane ----
    const unsigned* fin = s[cur];
    float* o = (img ? ob : oa) + (long)n * 3 * plane;
    for (int u = tid; u < TH * (TW / 4); u += 256) {
        const int r = u / (TW / 4), g = u % (TW / 4);
        const int oy = ty0 + r, ox = tx0 + 4 * g;
        if (oy >= h || ox >= w) continue;
        const unsigned* q = fin + (r + 3) * RWD + 3 + 3 * g;
        const unsigned d[3] = {q[0], q[1], q[2]};
        float v[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j] = lut[(d[j >> 2] >> (8 * (j & 3))) & 255u];
        float* dst = o + (long)oy * w + ox;
        if (vec) {                                              // w % 4 == 0 and 16-byte aligned outputs
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *reinterpret_cast<float4*>(dst + c * plane) = make_float4(v[c], v[3 + c], v[6 + c], v[9 + c]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ox + k < w) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) dst[c * plane + k] = v[3 * k + c];
                }
        }
    }
}

}  // namespace

extern "C" int dh_augment_pairs_blur_u8(const unsigned char* a, const unsigned char* b, const unsigned char* l, const int* idx,
                                        const int* params, const int* blur, int N, int H, int W, int h, int w, float* out_a,
                                        float* out_b, unsigned char* out_l, void* stream) {
    constexpr int TW = DH_BLUR_TW, TH = DH_BLUR_TH;
    DH_REQUIRE(N > 0 && h > 0 && w > 0 && h <= H && w <= W, "augment_pairs_blur_u8: bad sizes N=%d %dx%d -> %dx%d", N, H, W, h, w);
    DH_REQUIRE(2 * (long)N <= 65535 && dh_cdiv(h, TH) <= 65535, "augment_pairs_blur_u8: N=%d h=%d exceed the launch grid", N, h);
    DH_REQUIRE(blur != nullptr, "augment_pairs_blur_u8: no (ww, fw) table");
    const int vec = w % 4 == 0 && (uintptr_t)out_a % 16 == 0 && (uintptr_t)out_b % 16 == 0;
    hipLaunchKernelGGL((augment_pairs_blur_u8_kernel<TW, TH>), dim3(dh_cdiv(w, TW), dh_cdiv(h, TH), 2 * N), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), a, b, l, idx, params, blur, H, W, h, w, out_a, out_b, out_l, vec);
    DH_CHECK_LAUNCH("augment_pairs_blur_u8");
    return 0;
}
