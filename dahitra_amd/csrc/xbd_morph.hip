// xBD masks: square-window morphology on bytes, the dilated training masks and the hole fill.  All integer, bit-exact.
//
// morph_kernel<KIND>: out[y][x] = OR over the k x k window centred on (y, x) of in, k odd, 1 <= k <= 31, r = k / 2, everything
// outside the image clear.  A workgroup owns a MT_H x MT_W tile of the output and stages rows y0 - r .. y0 + MT_H - 1 + r and the
// columns x0 - 16 .. x0 + MT_W + 15 (a fixed halo of 16 >= r columns, so a staged row starts on a multiple of four columns) in
// LDS, four pixels to a dword, byte 0 the lowest column; out-of-image positions are staged as 0.  A byte carries up to eight
// independent bit planes and the kernel never looks at how many are in use.  The window is separable, along the rows first and
// then along the columns, and each pass doubles: with f_m[x] = OR in[x .. x + m - 1],
//     f_2m[x] = f_m[x] | f_m[x + m]                      m = 1, 2, 4, .. while 2 m <= k
//     out[x]  = f_m[x - r] | f_m[x + r - m + 1]          m the largest power of two <= k: the two windows cover x - r .. x + r
// so a pass costs floor(log2 k) + 1 steps of two reads each whatever k is.  Along the rows a read at a byte offset that is no
// multiple of four is two dwords and one v_alignbyte_b32; along the columns a shift is a row offset.  The steps alternate between
// two LDS images with a barrier between them; consecutive threads take consecutive dwords, so no step has a bank conflict.
// Erosion is the same kernel by De Morgan: the load stages "clear" (in-image pixels only, so that out-of-image stays 0 in the
// complemented domain, which is border_value = 1), the store inverts.
//   KIND MORPH_DILATE / MORPH_ERODE   [N][H][W] uint8 (nonzero = set) -> [N][H][W] uint8 (0 / 1)
//   KIND MORPH_MSK                    [N][5][H][W] uint8 mask channels -> [N][5][H][W]: channel c = 1 .. 4 is bit c - 1 of the
//                                     staged byte (channel 0 is not read); the store applies the priority rule of
//                                     xBD_code/train_unettransformer.py:262-273 to the four dilated bits d1 .. d4,
//                                         m2 = d2, m3 = d3 & ~d2, m4 = d4 & ~d2 & ~d3, m1 = d1 & ~(d2 | d3 | d4), m0 = any,
//                                     and writes all five channels.
// Any H, W >= 1: W % 4 == 0 with 4-byte aligned pointers takes dword loads and stores, anything else goes byte by byte with the
// same result.  Every output byte is written, nothing outside the source is read.
//
// Hole fill: dst = (src != 0) | (a component of src == 0 that owns no pixel on the image border).  Nine launches whatever the
// data: one writes the key src == 0 and clears the marks, dh_xbd_cc_label's six label the key (4- or 8-connected), one thread per
// border pixel stores mark[label] = 1 -- a plain byte store of the same value from every writer, no atomic -- and one writes dst.
// The marks are bytes [N][H W + 1], indexed by the label: a complement cannot have more components than pixels, so there is no cap.
#include "common.h"

extern "C" int dh_xbd_cc_ws_bytes(int N, int H, int W, long* bytes);
extern "C" int dh_xbd_cc_label(const unsigned char* key, int N, int H, int W, int conn, int keyed, int* labels, int* count,
                               void* ws, long ws_bytes, void* stream);

namespace {

constexpr int MT_H = 32, MT_W = 64;          // the output tile: the tile of the component labelling
constexpr int MT_THREADS = 256;
constexpr int MT_HALO = 16;                  // staged columns on each side: >= the largest r, a multiple of four
constexpr int MT_MAX_K = 31;
constexpr int MT_SW = (MT_W + 2 * MT_HALO) / 4;            // dwords of a staged row: 24
constexpr int MT_SH = MT_H + MT_MAX_K - 1;                 // staged rows at the largest window: 62
constexpr int MT_OW = MT_W / 4, MT_O0 = MT_HALO / 4;       // the output columns of a staged row: dwords 4 .. 19
static_assert(MT_HALO % 4 == 0 && MT_HALO >= MT_MAX_K / 2 && MT_W % 4 == 0, "a staged row starts on a multiple of four columns");

enum { MORPH_DILATE = 0, MORPH_ERODE = 1, MORPH_MSK = 2 };
constexpr unsigned ONES = 0x01010101u;

// 0x01 in every byte of v that is not zero
__device__ __forceinline__ unsigned nonzero_bytes(unsigned v) { return ((((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) >> 7) & ONES; }

// the four bytes at byte offset b of a staged row (b may lie before or beyond it: those bytes are 0)
__device__ __forceinline__ unsigned row_read(const unsigned* row, int b) {
    const int q = b >> 2;
    const unsigned lo = (q >= 0 && q < MT_SW) ? row[q] : 0u;
    const unsigned hi = (q + 1 >= 0 && q + 1 < MT_SW) ? row[q + 1] : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, (unsigned)(b & 3));
}

// four pixels of one plane at columns gx .. gx + 3 of row gy (gx a multiple of four, possibly outside the image) as a dword;
// inside = 0x01 in the bytes that lie in the image
__device__ __forceinline__ unsigned load4(const unsigned char* __restrict__ plane, int H, int W, int gy, int gx, bool fast,
                                         unsigned& inside) {
    inside = 0;
    if (gy < 0 || gy >= H || gx + 3 < 0 || gx >= W) return 0u;
    const unsigned char* p = plane + (long)gy * W + gx;
    if (fast) {                                  // W % 4 == 0 and gx % 4 == 0: the dword is inside or outside as a whole
        inside = ONES;
        return *reinterpret_cast<const unsigned*>(p);
    }
    unsigned v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (gx + b >= 0 && gx + b < W) {
            v |= (unsigned)p[b] << (8 * b);
            inside |= 1u << (8 * b);
        }
    return v;
}

__device__ __forceinline__ void store4(unsigned char* __restrict__ plane, int W, int gy, int gx, bool fast, unsigned v) {
    unsigned char* p = plane + (long)gy * W + gx;
    if (fast) {
        *reinterpret_cast<unsigned*>(p) = v;
        return;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (gx + b < W) p[b] = (unsigned char)(v >> (8 * b));
}

// grid (tiles of an image, N)
template <int KIND>
__global__ __launch_bounds__(MT_THREADS) void morph_kernel(const unsigned char* __restrict__ src, int H, int W, int tiles_x, int k,
                                                           int fast, unsigned char* __restrict__ dst) {
    __shared__ unsigned img[2][MT_SH * MT_SW];
    const long hw = (long)H * W;
    constexpr int PLANES = KIND == MORPH_MSK ? 5 : 1;
    const unsigned char* simg = src + (long)blockIdx.y * PLANES * hw;
    unsigned char* dimg = dst + (long)blockIdx.y * PLANES * hw;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * MT_H, x0 = tx * MT_W;
    const int r = k >> 1;
    const int rows = MT_H + 2 * r;
    const int q_lo = (MT_HALO - r) >> 2, q_hi = (MT_HALO + MT_W - 1 + r) >> 2;       // the staged dwords a window can reach
    // stage
    for (int i = threadIdx.x; i < rows * MT_SW; i += MT_THREADS) {
        const int ry = i / MT_SW, q = i - ry * MT_SW;
        const int gy = y0 - r + ry, gx = x0 - MT_HALO + 4 * q;
        unsigned v = 0;
        if (q >= q_lo && q <= q_hi) {
            unsigned in;
            if constexpr (KIND == MORPH_MSK) {
#pragma unroll
                for (int c = 1; c < 5; ++c) v |= nonzero_bytes(load4(simg + c * hw, H, W, gy, gx, fast, in)) << (c - 1);
            } else {
                v = nonzero_bytes(load4(simg, H, W, gy, gx, fast, in));
                if constexpr (KIND == MORPH_ERODE) v = (v ^ ONES) & in;
            }
        }
        img[0][i] = v;
    }
    __syncthreads();
    int cur = 0, m = 1;
    // along the rows
    for (; 2 * m <= k; m <<= 1) {
        for (int i = threadIdx.x; i < rows * MT_SW; i += MT_THREADS) {
            const int ry = i / MT_SW, q = i - ry * MT_SW;
            const unsigned* row = img[cur] + ry * MT_SW;
            img[cur ^ 1][i] = row[q] | row_read(row, 4 * q + m);
        }
        cur ^= 1;
        __syncthreads();
    }
    for (int i = threadIdx.x; i < rows * MT_OW; i += MT_THREADS) {       // the window centred, the output columns only
        const int ry = i / MT_OW, q = MT_O0 + i - ry * MT_OW;
        const unsigned* row = img[cur] + ry * MT_SW;
        img[cur ^ 1][ry * MT_SW + q] = row_read(row, 4 * q - r) | row_read(row, 4 * q + r - m + 1);
    }
    cur ^= 1;
    __syncthreads();
    // along the columns: staged row ry is image row y0 - r + ry, so output row oy is the OR of staged rows oy .. oy + k - 1
    for (m = 1; 2 * m <= k; m <<= 1) {
        for (int i = threadIdx.x; i < rows * MT_OW; i += MT_THREADS) {
            const int ry = i / MT_OW, q = MT_O0 + i - ry * MT_OW;
            const unsigned a = img[cur][ry * MT_SW + q];
            img[cur ^ 1][ry * MT_SW + q] = ry + m < rows ? a | img[cur][(ry + m) * MT_SW + q] : a;
        }
        cur ^= 1;
        __syncthreads();
    }
    for (int i = threadIdx.x; i < MT_H * MT_OW; i += MT_THREADS) {
        const int oy = i / MT_OW, oq = i - oy * MT_OW;
        const int gy = y0 + oy, gx = x0 + 4 * oq;
        if (gy >= H || gx >= W) continue;
        const unsigned v = img[cur][oy * MT_SW + MT_O0 + oq] | img[cur][(oy + k - m) * MT_SW + MT_O0 + oq];
        if constexpr (KIND == MORPH_MSK) {
            const unsigned d1 = v & ONES, d2 = (v >> 1) & ONES, d3 = (v >> 2) & ONES, d4 = (v >> 3) & ONES;
            store4(dimg, W, gy, gx, fast, d1 | d2 | d3 | d4);
            store4(dimg + hw, W, gy, gx, fast, d1 & ~(d2 | d3 | d4));
            store4(dimg + 2 * hw, W, gy, gx, fast, d2);
            store4(dimg + 3 * hw, W, gy, gx, fast, d3 & ~d2);
            store4(dimg + 4 * hw, W, gy, gx, fast, d4 & ~(d2 | d3));
        } else {
            store4(dimg, W, gy, gx, fast, KIND == MORPH_ERODE ? (v ^ ONES) & ONES : v & ONES);
        }
    }
}

// ---- hole fill -------------------------------------------------------------------------------------------------------------
constexpr int FH_BLOCK = 1024;               // pixels per workgroup of the flat passes: 4 per thread, strided by 256

// grid (nblk, N): key = (src == 0), and the marks of the image cleared: mark [N][H W + 1]
__global__ __launch_bounds__(MT_THREADS) void fill_key_kernel(const unsigned char* __restrict__ src, long hw,
                                                              unsigned char* __restrict__ key, unsigned char* __restrict__ mark) {
    const unsigned char* s = src + (long)blockIdx.y * hw;
    unsigned char* kimg = key + (long)blockIdx.y * hw;
    unsigned char* mimg = mark + (long)blockIdx.y * (hw + 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) mimg[0] = 0;
#pragma unroll
    for (int j = 0; j < FH_BLOCK / MT_THREADS; ++j) {
        const long p = (long)blockIdx.x * FH_BLOCK + j * MT_THREADS + threadIdx.x;
        if (p >= hw) continue;
        kimg[p] = s[p] == 0;
        mimg[p + 1] = 0;
    }
}

// grid (ceil((2 W + 2 H) / 256), N): one thread per pixel of the image's border (a corner is taken twice)
__global__ __launch_bounds__(MT_THREADS) void fill_mark_kernel(const int* __restrict__ labels, int H, int W,
                                                               unsigned char* __restrict__ mark) {
    const long hw = (long)H * W;
    const long i = (long)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= 2L * W + 2L * H) return;
    long p;
    if (i < W) p = i;
    else if (i < 2L * W) p = (long)(H - 1) * W + (i - W);
    else if (i < 2L * W + H) p = (i - 2L * W) * W;
    else p = (i - 2L * W - H) * W + (W - 1);
    const int l = labels[(long)blockIdx.y * hw + p];
    if (l > 0 && l <= hw) mark[(long)blockIdx.y * (hw + 1) + l] = 1;      // every writer stores the same byte
}

// grid (nblk, N)
__global__ __launch_bounds__(MT_THREADS) void fill_write_kernel(const unsigned char* __restrict__ src, const int* __restrict__ labels,
                                                                const unsigned char* __restrict__ mark, long hw,
                                                                unsigned char* __restrict__ dst) {
    const unsigned char* s = src + (long)blockIdx.y * hw;
    const int* L = labels + (long)blockIdx.y * hw;
    const unsigned char* mimg = mark + (long)blockIdx.y * (hw + 1);
    unsigned char* d = dst + (long)blockIdx.y * hw;
#pragma unroll
    for (int j = 0; j < FH_BLOCK / MT_THREADS; ++j) {
        const long p = (long)blockIdx.x * FH_BLOCK + j * MT_THREADS + threadIdx.x;
        if (p >= hw) continue;
        const int l = L[p];
        d[p] = (s[p] != 0) || (l > 0 && l <= hw && mimg[l] == 0);
    }
}

bool aligned4(const void* p) { return (reinterpret_cast<size_t>(p) & 3) == 0; }
long pad4(long b) { return (b + 3) & ~3L; }

bool overlap(const void* a, const void* b, long bytes) {
    const size_t x = reinterpret_cast<size_t>(a), y = reinterpret_cast<size_t>(b);
    return x < y + (size_t)bytes && y < x + (size_t)bytes;
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define MORPH_REQUIRE_SHAPE(what)                                                                                                \
    DH_REQUIRE(N >= 1, what ": N=%d: an empty batch", N);                                                                        \
    DH_REQUIRE(N <= 65535, what ": N=%d: at most 65535 images per call", N);                                                     \
    DH_REQUIRE(H >= 1 && W >= 1, what ": empty image %dx%d", H, W);                                                              \
    DH_REQUIRE((long)H * W <= 0x7fffffffL, what ": %dx%d: an image holds fewer than 2^31 pixels", H, W)
#define MORPH_REQUIRE_K(what)                                                                                                    \
    DH_REQUIRE(k >= 1 && k <= MT_MAX_K && (k & 1), what ": k=%d: the window is odd, 1 .. %d", k, MT_MAX_K)

extern "C" int dh_xbd_morph_tile_h(void) { return MT_H; }
extern "C" int dh_xbd_morph_tile_w(void) { return MT_W; }

extern "C" int dh_xbd_morph_u8(const unsigned char* src, int N, int H, int W, int k, int op, unsigned char* dst, void* stream) {
    DH_REQUIRE(src && dst, "xbd_morph: null pointer");
    MORPH_REQUIRE_SHAPE("xbd_morph");
    MORPH_REQUIRE_K("xbd_morph");
    DH_REQUIRE(op == 0 || op == 1, "xbd_morph: op %d is neither 0 (dilate) nor 1 (erode)", op);
    DH_REQUIRE(!overlap(src, dst, (long)N * H * W), "xbd_morph: dst overlaps src (a window reads its neighbours)");
    const int tiles_x = dh_cdiv(W, MT_W), tiles_y = dh_cdiv(H, MT_H);
    const int fast = W % 4 == 0 && aligned4(src) && aligned4(dst);
    const dim3 grid(tiles_x * tiles_y, N), thr(MT_THREADS);
    if (op == 0) hipLaunchKernelGGL(morph_kernel<MORPH_DILATE>, grid, thr, 0, ST(stream), src, H, W, tiles_x, k, fast, dst);
    else hipLaunchKernelGGL(morph_kernel<MORPH_ERODE>, grid, thr, 0, ST(stream), src, H, W, tiles_x, k, fast, dst);
    DH_CHECK_LAUNCH("xbd_morph");
    return 0;
}

extern "C" int dh_xbd_msk_dilate_u8(const unsigned char* msk, int N, int H, int W, int k, unsigned char* out, void* stream) {
    DH_REQUIRE(msk && out, "xbd_msk_dilate: null pointer");
    MORPH_REQUIRE_SHAPE("xbd_msk_dilate");
    MORPH_REQUIRE_K("xbd_msk_dilate");
    DH_REQUIRE(!overlap(msk, out, 5L * N * H * W), "xbd_msk_dilate: out overlaps msk (a window reads its neighbours)");
    const int tiles_x = dh_cdiv(W, MT_W), tiles_y = dh_cdiv(H, MT_H);
    const int fast = W % 4 == 0 && ((long)H * W) % 4 == 0 && aligned4(msk) && aligned4(out);
    hipLaunchKernelGGL(morph_kernel<MORPH_MSK>, dim3(tiles_x * tiles_y, N), dim3(MT_THREADS), 0, ST(stream), msk, H, W, tiles_x, k,
                       fast, out);
    DH_CHECK_LAUNCH("xbd_msk_dilate");
    return 0;
}

// workspace: labels int32 [N][H W], count int32 [N], the labelling's own workspace, key uint8 [N][H W], mark uint8 [N][H W + 1]
static long fill_ws_bytes(int N, int H, int W, long cc_bytes) {
    const long hw = (long)H * W;
    return 4L * N * hw + 4L * N + pad4(cc_bytes) + pad4((long)N * hw) + pad4((long)N * (hw + 1));
}

extern "C" int dh_xbd_fill_holes_ws_bytes(int N, int H, int W, long* bytes) {
    DH_REQUIRE(bytes, "xbd_fill_holes_ws_bytes: null pointer");
    MORPH_REQUIRE_SHAPE("xbd_fill_holes_ws_bytes");
    long cc = 0;
    if (dh_xbd_cc_ws_bytes(N, H, W, &cc) != 0) return 1;
    *bytes = fill_ws_bytes(N, H, W, cc);
    return 0;
}

extern "C" int dh_xbd_fill_holes_u8(const unsigned char* src, int N, int H, int W, int background, unsigned char* dst, void* ws,
                                    long ws_bytes, void* stream) {
    DH_REQUIRE(src && dst && ws, "xbd_fill_holes: null pointer");
    MORPH_REQUIRE_SHAPE("xbd_fill_holes");
    DH_REQUIRE(background == 4 || background == 8, "xbd_fill_holes: background connectivity %d is neither 4 nor 8", background);
    DH_REQUIRE(aligned4(ws), "xbd_fill_holes: the workspace holds int32");
    const long hw = (long)H * W;
    DH_REQUIRE(!overlap(src, dst, N * hw), "xbd_fill_holes: dst overlaps src");
    long cc = 0;
    if (dh_xbd_cc_ws_bytes(N, H, W, &cc) != 0) return 1;
    const long need = fill_ws_bytes(N, H, W, cc);
    DH_REQUIRE(ws_bytes >= need, "xbd_fill_holes: a workspace of %ld bytes, %ld are needed", ws_bytes, need);
    unsigned char* base = reinterpret_cast<unsigned char*>(ws);
    int* labels = reinterpret_cast<int*>(base);
    int* count = labels + (long)N * hw;
    unsigned char* ccws = reinterpret_cast<unsigned char*>(count + N);
    unsigned char* key = ccws + pad4(cc);
    unsigned char* mark = key + pad4((long)N * hw);
    const dim3 flat(dh_cdiv(hw, FH_BLOCK), N), thr(MT_THREADS);
    hipLaunchKernelGGL(fill_key_kernel, flat, thr, 0, ST(stream), src, hw, key, mark);
    DH_CHECK_LAUNCH("xbd_fill_holes");
    if (dh_xbd_cc_label(key, N, H, W, background, 0, labels, count, ccws, cc, stream) != 0) return 1;
    hipLaunchKernelGGL(fill_mark_kernel, dim3(dh_cdiv(2L * W + 2L * H, MT_THREADS), N), thr, 0, ST(stream), labels, H, W, mark);
    hipLaunchKernelGGL(fill_write_kernel, flat, thr, 0, ST(stream), src, labels, mark, hw, dst);
    DH_CHECK_LAUNCH("xbd_fill_holes");
    return 0;
}
