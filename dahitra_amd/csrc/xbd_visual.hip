// The damage map of the xBD visualiser (xBD_code/visualize_results.py:204-220) from the predictor's bytes, all in integers.
// msk [N][H][W][5] uint8, channels last (what dh_xbd_tta_merge_u8 writes).
//   class:  dmg = 1 + index of the FIRST maximum of msk[1..4] (numpy's argmax: a tie goes to the lowest channel), 1 .. 4.
//   rule:   use_loc != 0: keep = m0 >= b0 || (m0 >= b1 && 1 < dmg < 4) || (m0 >= b2 && dmg > 1), out = keep ? dmg : 0, with m0 = msk[0]
//           and b_i the smallest byte whose value / 255 exceeds the script's threshold _thr[i] (256: none does).  The caller
//           derives the b_i; the kernel compares bytes.  use_loc == 0 is the script as executed (its line 211 is commented out).
//   colour: class 0 .. 4 -> RGB (0,0,0) (0,255,0) (255,255,0) (255,127,0) (255,0,0); any other byte -> (255,0,255).
//   map:    out[N][H][W] = the class.
//   grid:   grid[N][H][4W][3] RGB = pre | post | colour(gt) | colour(class), the class computed in registers.
// Both stream (map: 5 B read, 1 B written per pixel; grid: 12 B read, 12 B written) over runs of 16 consecutive pixels of the
// flat [N H W] index: 80 bytes of msk are five 16-byte loads, 48 bytes of an image three, 16 labels one.  The map stores its
// 16 classes as one 16-byte vector.  The grid stores each panel's 48 bytes as three 16-byte vectors where a run lies in one row
// at a 16-byte address (W % 16 == 0), and otherwise as 4 x 3 dwords, each 4 pixels of one row (W % 4 == 0).  Sources that are
// not 16-byte aligned, an output that is not aligned to its store, a W that is no multiple of 4 (grid) and the last partial run
// go pixel by pixel through the same class function.  Every output byte is written; nothing else is launched.
#include "common.h"

namespace {

constexpr int VS_THREADS = 256;
constexpr int VS_MAX_WORKGROUPS = 512;      // two workgroups per CU, the rest is the grid-stride loop
constexpr int VS_RUN = 16;                  // pixels per thread and pass

struct LocRule {
    int use, b0, b1, b2;
};

__device__ __forceinline__ unsigned damage_class(unsigned m0, unsigned m1, unsigned m2, unsigned m3, unsigned m4, LocRule r) {
    unsigned d = 1, best = m1;
    if (m2 > best) { best = m2; d = 2; }      // strict: the first maximum keeps its place
    if (m3 > best) { best = m3; d = 3; }
    if (m4 > best) d = 4;
    if (r.use) {
        const int m = (int)m0;
        const bool keep = m >= r.b0 || (m >= r.b1 && d > 1 && d < 4) || (m >= r.b2 && d > 1);
        d = keep ? d : 0u;
    }
    return d;
}

// R | G << 8 | B << 16
__device__ __forceinline__ unsigned colour(unsigned c) {
    return c == 0 ? 0x000000u : c == 1 ? 0x00ff00u : c == 2 ? 0x00ffffu : c == 3 ? 0x007fffu : c == 4 ? 0x0000ffu : 0xff00ffu;
}

__device__ __forceinline__ unsigned byte_of(const unsigned* v, int i) { return (v[i >> 2] >> (8 * (i & 3))) & 255u; }

__device__ __forceinline__ void ld16(const unsigned char* p, unsigned* o) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
__device__ __forceinline__ void st16(unsigned char* p, const unsigned* o) {
    *reinterpret_cast<uint4*>(p) = make_uint4(o[0], o[1], o[2], o[3]);
}

// the 16 classes of the run whose 80 msk bytes lie in m[20]
__device__ __forceinline__ void classes16(const unsigned (&m)[20], LocRule r, unsigned (&c)[VS_RUN]) {
#pragma unroll
    for (int j = 0; j < VS_RUN; ++j)
        c[j] = damage_class(byte_of(m, 5 * j), byte_of(m, 5 * j + 1), byte_of(m, 5 * j + 2), byte_of(m, 5 * j + 3),
                            byte_of(m, 5 * j + 4), r);
}

// 4 colours -> the 12 bytes of 4 RGB pixels
__device__ __forceinline__ void pack_rgb4(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned* d) {
    d[0] = c0 | (c1 << 24);
    d[1] = (c1 >> 8) | (c2 << 16);
    d[2] = (c2 >> 16) | (c3 << 8);
}

// total = N * H * W pixels; vec: msk and out 16-byte aligned
__global__ __launch_bounds__(VS_THREADS) void xbd_damage_map_kernel(const unsigned char* __restrict__ msk, long total, LocRule r,
                                                                    int vec, unsigned char* __restrict__ out) {
    const long runs = (total + VS_RUN - 1) / VS_RUN;
    for (long g = (long)blockIdx.x * VS_THREADS + threadIdx.x; g < runs; g += (long)gridDim.x * VS_THREADS) {
        const long p0 = g * VS_RUN;
        if (vec && p0 + VS_RUN <= total) {
            unsigned m[20], c[VS_RUN], d[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 5; ++i) ld16(msk + p0 * 5 + 16 * i, m + 4 * i);
            classes16(m, r, c);
#pragma unroll
            for (int j = 0; j < VS_RUN; ++j) d[j >> 2] |= c[j] << (8 * (j & 3));
            st16(out + p0, d);
        } else {
            const int cnt = total - p0 >= VS_RUN ? VS_RUN : (int)(total - p0);
            for (int j = 0; j < cnt; ++j) {
                const unsigned char* s = msk + (p0 + j) * 5;
                out[p0 + j] = (unsigned char)damage_class(s[0], s[1], s[2], s[3], s[4], r);
            }
        }
    }
}

// total = N * H * W pixels, rows of the grid are the N * H rows of the batch, each 4 W pixels of 3 bytes.
// mode 2: sources 16-byte aligned, W % 16 == 0, grid 16-byte aligned: a run is 16 pixels of one row, every panel three 16-byte stores
// mode 1: sources 16-byte aligned, W % 4 == 0, grid 4-byte aligned: a run is four groups of 4 pixels of one row each, three dwords
// mode 0: pixel by pixel
__global__ __launch_bounds__(VS_THREADS) void xbd_vis_grid_kernel(const unsigned char* __restrict__ pre,
                                                                  const unsigned char* __restrict__ post,
                                                                  const unsigned char* __restrict__ gt,
                                                                  const unsigned char* __restrict__ msk, long total, int W, LocRule r,
                                                                  int mode, unsigned char* __restrict__ grid) {
    const long runs = (total + VS_RUN - 1) / VS_RUN;
    const long panel = (long)W * 3;      // bytes of one panel's row
    for (long g = (long)blockIdx.x * VS_THREADS + threadIdx.x; g < runs; g += (long)gridDim.x * VS_THREADS) {
        const long p0 = g * VS_RUN;
        long row = p0 / W;
        int x = (int)(p0 - row * W);
        if (mode && p0 + VS_RUN <= total) {
            unsigned m[20], a[12], b[12], t[4], c[VS_RUN], cg[12], cp[12];
#pragma unroll
            for (int i = 0; i < 5; ++i) ld16(msk + p0 * 5 + 16 * i, m + 4 * i);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                ld16(pre + p0 * 3 + 16 * i, a + 4 * i);
                ld16(post + p0 * 3 + 16 * i, b + 4 * i);
            }
            ld16(gt + p0, t);
            classes16(m, r, c);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                pack_rgb4(colour(byte_of(t, 4 * q)), colour(byte_of(t, 4 * q + 1)), colour(byte_of(t, 4 * q + 2)),
                          colour(byte_of(t, 4 * q + 3)), cg + 3 * q);
                pack_rgb4(colour(c[4 * q]), colour(c[4 * q + 1]), colour(c[4 * q + 2]), colour(c[4 * q + 3]), cp + 3 * q);
            }
            if (mode == 2) {
                unsigned char* dst = grid + (row * 4 * W + x) * 3;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    st16(dst + 16 * i, a + 4 * i);
                    st16(dst + panel + 16 * i, b + 4 * i);
                    st16(dst + 2 * panel + 16 * i, cg + 4 * i);
                    st16(dst + 3 * panel + 16 * i, cp + 4 * i);
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    unsigned char* dst = grid + (row * 4 * W + x) * 3;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        reinterpret_cast<unsigned*>(dst)[i] = a[3 * q + i];
                        reinterpret_cast<unsigned*>(dst + panel)[i] = b[3 * q + i];
                        reinterpret_cast<unsigned*>(dst + 2 * panel)[i] = cg[3 * q + i];
                        reinterpret_cast<unsigned*>(dst + 3 * panel)[i] = cp[3 * q + i];
                    }
                    x += 4;                     // x and W are multiples of 4: the next group starts in this row or opens the next
                    if (x == W) { x = 0; ++row; }
                }
            }
        } else {
            const int cnt = total - p0 >= VS_RUN ? VS_RUN : (int)(total - p0);
            for (int j = 0; j < cnt; ++j) {
                const long p = p0 + j;
                const unsigned char* s = msk + p * 5;
                const unsigned cols[2] = {colour(gt[p]), colour(damage_class(s[0], s[1], s[2], s[3], s[4], r))};
                unsigned char* dst = grid + (row * 4 * W + x) * 3;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    dst[ch] = pre[p * 3 + ch];
                    dst[panel + ch] = post[p * 3 + ch];
                    dst[2 * panel + ch] = (unsigned char)(cols[0] >> (8 * ch));
                    dst[3 * panel + ch] = (unsigned char)(cols[1] >> (8 * ch));
                }
                if (++x == W) { x = 0; ++row; }
            }
        }
    }
}

int grid_x(long total) {
    const long gx = ((total + VS_RUN - 1) / VS_RUN + VS_THREADS - 1) / VS_THREADS;
    return gx > VS_MAX_WORKGROUPS ? VS_MAX_WORKGROUPS : (int)gx;
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define VS_REQUIRE_SHAPE(what)                                                                                                   \
    DH_REQUIRE(N >= 1, what ": N=%d: an empty batch", N);                                                                        \
    DH_REQUIRE(H >= 1 && W >= 1, what ": empty image %dx%d", H, W);                                                              \
    DH_REQUIRE((long)H * W <= 0x7fffffffL, what ": %dx%d: an image holds fewer than 2^31 pixels", H, W);                         \
    DH_REQUIRE(b0 >= 0 && b0 <= 256 && b1 >= 0 && b1 <= 256 && b2 >= 0 && b2 <= 256,                                              \
               what ": bounds %d, %d, %d: each is a byte 0..255, or 256 for a threshold no byte exceeds", b0, b1, b2)

extern "C" int dh_xbd_damage_map_u8(const unsigned char* msk, int N, int H, int W, int use_loc, int b0, int b1, int b2,
                                    unsigned char* out, void* stream) {
    DH_REQUIRE(msk && out, "xbd_damage_map: null pointer");
    VS_REQUIRE_SHAPE("xbd_damage_map");
    const long total = (long)N * H * W;
    const LocRule r = {use_loc != 0, b0, b1, b2};
    const int vec = aligned(msk, 16) && aligned(out, 16);
    hipLaunchKernelGGL(xbd_damage_map_kernel, dim3(grid_x(total)), dim3(VS_THREADS), 0, ST(stream), msk, total, r, vec, out);
    DH_CHECK_LAUNCH("xbd_damage_map");
    return 0;
}

extern "C" int dh_xbd_vis_grid_u8(const unsigned char* pre, const unsigned char* post, const unsigned char* gt,
                                  const unsigned char* msk, int N, int H, int W, int use_loc, int b0, int b1, int b2,
                                  unsigned char* grid, void* stream) {
    DH_REQUIRE(pre && post && gt && msk && grid, "xbd_vis_grid: null pointer");
    VS_REQUIRE_SHAPE("xbd_vis_grid");
    DH_REQUIRE(12L * W * H <= 0x7fffffffL, "xbd_vis_grid: %dx%d: the grid of an image, 12 W H bytes, stays below 2^31", H, W);
    const long total = (long)N * H * W;
    const LocRule r = {use_loc != 0, b0, b1, b2};
    int mode = 0;
    if (aligned(pre, 16) && aligned(post, 16) && aligned(gt, 16) && aligned(msk, 16)) {
        if ((W & 15) == 0 && aligned(grid, 16)) mode = 2;
        else if ((W & 3) == 0 && aligned(grid, 4)) mode = 1;
    }
    hipLaunchKernelGGL(xbd_vis_grid_kernel, dim3(grid_x(total)), dim3(VS_THREADS), 0, ST(stream), pre, post, gt, msk, total, W, r,
                       mode, grid);
    DH_CHECK_LAUNCH("xbd_vis_grid");
    return 0;
}
