// The picture the change-detection evaluator writes per batch (models/evaluator.py:118-131 of the reference: make_grid with
// padding 0 of de_norm(A), de_norm(B), argmax * 255 and the label, concatenated top to bottom, clipped to [0, 1], saved as
// uint8(vis * 255)) in one pass, all bytes.
// A, B [N][3][H][W] fp32, logits [N][C][H][W] fp32, label [N][H][W] int64 -> out [4 rows H][cols W][3] uint8 RGB with
// cols = min(8, N), rows = ceil(N / cols): image n is the tile (n / cols, n % cols) of each of the four bands
//   band 0, 1: t = x * 0.5f + 0.5f in fp32, clipped to [0, 1], byte = trunc(t * 255)
//   band 2:    255 where the first maximum of the C logits is not class 0 (dh_argmax_nchw's rule: a later class wins only if
//              strictly greater), else 0, on all three channels
//   band 3:    255 where label >= 1, else 0
//   a tile position >= N: 0 in all four bands.
// Arithmetic.  x * 0.5f is exact (a power of two; a subnormal x that loses its last bit is far below the rounding of the sum),
// so a fused multiply-add gives the same t as the two roundings and no contraction pragma is needed.  The reference's byte is
// the truncated float64 product t * 255, which is the exact real product (24 x 8 bits).  Here it is the truncated fp32 product.
// Both products increase with t, so the two can differ only if, for some k in 1 .. 255, the largest fp32 t below k / 255 has an
// fp32 product that rounds up to k; that t is fl(k / 255) or the fp32 value below it, 510 candidates, and none rounds up
// (tests/test_cd_visual_cpu.py goes through them).  A NaN paints 0.
// Work.  A unit is 1024 consecutive pixels of one image in one band: band and image are uniform per workgroup and pass, a
// thread owns 4 pixels.  Vector form (W % 4 == 0, sources 16-byte aligned, out 4-byte aligned): the 4 pixels are consecutive in
// one row, every plane is one 16-byte load (a label two), the 12 output bytes are assembled in registers and stored as three
// dwords.  Any other W or alignment: the same unit pixel by pixel, 256 consecutive pixels per pass of the workgroup.  Units are
// walked with a grid-stride loop; every byte of out is written, the empty tiles included, by this one launch.
#include "common.h"

namespace {

constexpr int CV_THREADS = 256;
constexpr int CV_PX = 4;                              // pixels per thread and unit
constexpr int CV_UNIT = CV_THREADS * CV_PX;           // pixels per unit
constexpr int CV_MAX_WORKGROUPS = 2048;               // 8 workgroups per CU; the rest is the grid-stride loop
constexpr int CV_COLS = 8;                            // make_grid's nrow

__device__ __forceinline__ unsigned byte_of(float x) {
    float t = x * 0.5f + 0.5f;
    t = fminf(fmaxf(t, 0.f), 1.f);                    // fmaxf(NaN, 0) = 0
    return (unsigned)(t * 255.f);
}

__device__ __forceinline__ unsigned grey(bool on) { return on ? 0xffffffu : 0u; }

// 4 colours (R | G << 8 | B << 16) -> the 12 bytes of 4 RGB pixels
__device__ __forceinline__ void pack_rgb4(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned* d) {
    d[0] = c0 | (c1 << 24);
    d[1] = (c1 >> 8) | (c2 << 16);
    d[2] = (c2 >> 16) | (c3 << 8);
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

struct Shape {
    int N, C, H, W, rows, cols;
    int chunks;                                       // units of an image
    long HW;                                          // pixels of an image, < 2^31
};

// the colour of pixel p of image n in `band` (n < N)
__device__ __forceinline__ unsigned colour1(const float* __restrict__ A, const float* __restrict__ B, const float* __restrict__ logits,
                                            const long long* __restrict__ label, int band, long n, long p, const Shape& s) {
    if (band < 2) {
        const float* src = (band == 0 ? A : B) + n * 3 * s.HW + p;
        return byte_of(src[0]) | (byte_of(src[s.HW]) << 8) | (byte_of(src[2 * s.HW]) << 16);
    }
    if (band == 2) {
        const float* src = logits + n * s.C * s.HW + p;
        float best = src[0];
        bool on = false;
        for (int c = 1; c < s.C; ++c) {
            const float v = src[c * s.HW];
            if (v > best) { best = v; on = true; }
        }
        return grey(on);
    }
    return grey(label[n * s.HW + p] >= 1);
}

template <bool VEC>
__global__ __launch_bounds__(CV_THREADS) void cd_eval_vis_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                                 const float* __restrict__ logits,
                                                                 const long long* __restrict__ label, Shape s,
                                                                 unsigned char* __restrict__ out) {
    const unsigned per_band = (unsigned)(s.rows * s.cols) * (unsigned)s.chunks;          // the host checked: 4 per_band < 2^31
    const unsigned units = 4u * per_band;
    const long line = (long)s.cols * s.W * 3;         // bytes of one line of out
    for (unsigned u = blockIdx.x; u < units; u += gridDim.x) {
        const int band = (int)(u / per_band);
        const unsigned rem = u - band * per_band;
        const long n = rem / (unsigned)s.chunks;      // the tile, and the image if n < N
        const long p0 = (long)(rem - (unsigned)n * (unsigned)s.chunks) * CV_UNIT;
        const int r = (int)((unsigned)n / (unsigned)s.cols), c = (int)n - r * s.cols;
        unsigned char* tile = out + ((long)band * s.rows + r) * s.H * line + (long)c * s.W * 3;
        const bool empty = n >= s.N;
        if (VEC) {
            const long p = p0 + (long)threadIdx.x * CV_PX;          // HW % 4 == 0: the 4 pixels are all inside or all outside
            if (p >= s.HW) continue;
            unsigned col[CV_PX] = {0, 0, 0, 0};
            if (empty) {
            } else if (band < 2) {
                const float* src = (band == 0 ? A : B) + n * 3 * s.HW + p;
                const float4 cr = ld4(src), cg = ld4(src + s.HW), cb = ld4(src + 2 * s.HW);
                col[0] = byte_of(cr.x) | (byte_of(cg.x) << 8) | (byte_of(cb.x) << 16);
                col[1] = byte_of(cr.y) | (byte_of(cg.y) << 8) | (byte_of(cb.y) << 16);
                col[2] = byte_of(cr.z) | (byte_of(cg.z) << 8) | (byte_of(cb.z) << 16);
                col[3] = byte_of(cr.w) | (byte_of(cg.w) << 8) | (byte_of(cb.w) << 16);
            } else if (band == 2) {
                const float* src = logits + n * s.C * s.HW + p;
                float4 best = ld4(src);
                bool on[CV_PX] = {false, false, false, false};
                for (int k = 1; k < s.C; ++k) {
                    const float4 v = ld4(src + k * s.HW);
                    if (v.x > best.x) { best.x = v.x; on[0] = true; }          // strict: the first maximum keeps its place
                    if (v.y > best.y) { best.y = v.y; on[1] = true; }
                    if (v.z > best.z) { best.z = v.z; on[2] = true; }
                    if (v.w > best.w) { best.w = v.w; on[3] = true; }
                }
#pragma unroll
                for (int j = 0; j < CV_PX; ++j) col[j] = grey(on[j]);
            } else {
                const longlong2* src = reinterpret_cast<const longlong2*>(label + n * s.HW + p);
                const longlong2 l0 = src[0], l1 = src[1];
                col[0] = grey(l0.x >= 1); col[1] = grey(l0.y >= 1); col[2] = grey(l1.x >= 1); col[3] = grey(l1.y >= 1);
            }
            const long y = (unsigned)p / (unsigned)s.W;             // p < H W < 2^31
            const int x = (int)(p - y * s.W);                       // x and W are multiples of 4: the 4 pixels lie in line y
            unsigned d[3];
            pack_rgb4(col[0], col[1], col[2], col[3], d);
            unsigned* dst = reinterpret_cast<unsigned*>(tile + y * line + (long)x * 3);
            dst[0] = d[0]; dst[1] = d[1]; dst[2] = d[2];
        } else {
            for (int j = 0; j < CV_PX; ++j) {
                const long p = p0 + j * CV_THREADS + threadIdx.x;
                if (p >= s.HW) break;
                const unsigned col = empty ? 0u : colour1(A, B, logits, label, band, n, p, s);
                const long y = (unsigned)p / (unsigned)s.W;
                const int x = (int)(p - y * s.W);
                unsigned char* dst = tile + y * line + (long)x * 3;
                dst[0] = (unsigned char)col; dst[1] = (unsigned char)(col >> 8); dst[2] = (unsigned char)(col >> 16);
            }
        }
    }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int dh_cd_eval_vis_u8(const float* A, const float* B, const float* logits, const long long* label, int N, int C, int H,
                                 int W, unsigned char* out, void* stream) {
    DH_REQUIRE(A && B && logits && label && out, "cd_eval_vis: null pointer");
    DH_REQUIRE(N >= 1, "cd_eval_vis: N=%d: an empty batch", N);
    DH_REQUIRE(C >= 1, "cd_eval_vis: C=%d: the logits hold at least one class", C);
    DH_REQUIRE(H >= 1 && W >= 1, "cd_eval_vis: empty image %dx%d", H, W);
    DH_REQUIRE((long)H * W <= 0x7fffffffL, "cd_eval_vis: %dx%d: an image holds fewer than 2^31 pixels", H, W);
    Shape s;
    s.N = N; s.C = C; s.H = H; s.W = W;
    s.cols = N < CV_COLS ? N : CV_COLS;
    s.rows = (N + s.cols - 1) / s.cols;
    s.HW = (long)H * W;
    s.chunks = (int)((s.HW + CV_UNIT - 1) / CV_UNIT);
    const long units = 4L * s.rows * s.cols * s.chunks;
    DH_REQUIRE(units <= 0x7fffffffL, "cd_eval_vis: N=%d at %dx%d: %ld units of 1024 pixels, the kernel counts fewer than 2^31", N, H, W, units);
    const int grid = units > CV_MAX_WORKGROUPS ? CV_MAX_WORKGROUPS : (int)units;
    const bool vec = (W & 3) == 0 && aligned(A, 16) && aligned(B, 16) && aligned(logits, 16) && aligned(label, 16) && aligned(out, 4);
    if (vec)
        hipLaunchKernelGGL(cd_eval_vis_kernel<true>, dim3(grid), dim3(CV_THREADS), 0, ST(stream), A, B, logits, label, s, out);
    else
        hipLaunchKernelGGL(cd_eval_vis_kernel<false>, dim3(grid), dim3(CV_THREADS), 0, ST(stream), A, B, logits, label, s, out);
    DH_CHECK_LAUNCH("cd_eval_vis");
    return 0;
}
