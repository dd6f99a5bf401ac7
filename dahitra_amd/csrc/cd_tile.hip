// Whole-tile change maps: the per-window logits of a net of fixed input size put back together (dahitra_amd/tiles.py TilePlan).
//
// dh_cd_tile_stitch.  logits [P][C][h][w] fp32 is the net's answer to the P views of one H x W tile, view
// p = (iy * nx + ix) * nf + f being the window at (ys[iy], xs[ix]) under flip code flips[f] (bit 0: rows reversed, bit 1: columns
// reversed), still flipped.  GATHER form: one thread computes an output pixel from everything that covers it, so there is no
// floating-point atomic and every run gives the same bits.  For pixel (Y, X) and class c, over the covering iy ascending, then
// ix ascending, then f in plan order:
//     ly = Y - ys[iy], lx = X - xs[ix], g = wy[ly] * wx[lx]
//     v  = logits[p][c][bit 0 ? h - 1 - ly : ly][bit 1 ? w - 1 - lx : lx]
//     acc = acc + g * v;  ws = ws + g                         every operation rounded to fp32 on its own
//     out = acc / ws                                          the correctly rounded fp32 division
// Contraction is off for the whole file: a fused multiply-add would skip the rounding of g * v, and whether the compiler fuses
// differs between the two forms below (loss_optim.hip keeps AdamW unfused for the same reason).  The class map is
// dh_argmax_nchw's rule on `out` (a later class wins only if strictly greater), so mask == argmax(out) by construction; with a
// label tile, counts[label * C + class] += 1 per pixel (integer atomics on LDS, then one 64-bit atomic per cell and workgroup,
// as dh_confusion_matrix).
// Cover.  Nothing scans the P views: rowc[Y] = (first iy, count) and colc[X] = (first ix, count), built on the host from the
// plan, name the windows over a row and over a column (up to three per axis once the last window is clamped to the edge).
// Work.  The kernel is bound by its reads, P C h w 4 bytes.  Quad form (the caller states x_align == 4: W, w and every xs[ix]
// are multiples of 4; the library checks W, w and that logits / out are 16-byte, mask / label 4-byte aligned): a thread owns 4
// consecutive columns of one row.  They share their cover, and in every view their sources are 4 consecutive floats at a
// multiple of 4 -- also under reversed columns, where the run starts at w - 4 - lx and is read forwards, then reversed in
// registers -- so a wave reads 1 KiB per instruction, each class plane of `out` is stored 16 bytes per lane, the mask as one
// dword.  Any other plan or alignment: one pixel per thread, dword loads, still contiguous across the wave in both directions.
// Units are walked with a grid-stride loop in 64-bit indices.
//
// dh_cd_view_counts.  counts[p][label * C + class] += 1 for every pixel of view p, class by the same arg-max rule: the P confusion
// matrices of P evaluators (eval_cd.py:49-55 keeps sixteen) in one launch, against the uint8 labels the cut kernel wrote.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAXC = 8;
constexpr int TS_THREADS = 256;
constexpr int TS_MAX_WORKGROUPS = 2048;               // 8 workgroups per CU; the rest is the grid-stride loop
constexpr int VC_MAX_X = 64;                          // workgroups per view of dh_cd_view_counts

struct Stitch {
    const float* logits;
    const int *ys, *xs, *flips, *rowc, *colc;
    const float *wy, *wx;
    float* out;                                       // [C][H][W] or null
    unsigned char* mask;                              // [H][W]
    const unsigned char* label;                       // [H][W] (or [S][H][W] with label_index) or null
    const int* label_index;                           // device scalar or null
    unsigned long long* counts;                       // [C][C] or null
    int C, h, w, nx, nf, H, W;
};

template <int PX> struct Vec;
template <> struct Vec<1> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[1]) { v[0] = *p; }
    static __device__ __forceinline__ void store(float* p, const float (&v)[1]) { *p = v[0]; }
};
template <> struct Vec<4> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) { ld4(p, v); }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) { st4(p, v); }
};

// PX: columns per thread (4: quad form).  CT: the class count if > 0, else s.C <= MAXC predicated slots.
template <int PX, int CT>
__global__ __launch_bounds__(TS_THREADS) void cd_tile_stitch_kernel(Stitch s) {
    constexpr int NC = CT > 0 ? CT : MAXC;
    const int C = CT > 0 ? CT : s.C;
    __shared__ unsigned int hist[MAXC * MAXC];
    const bool counting = s.counts != nullptr;        // uniform
    if (counting) {
        for (int i = threadIdx.x; i < C * C; i += TS_THREADS) hist[i] = 0;
        __syncthreads();
    }
    const unsigned char* label = s.label;
    if (counting && s.label_index) label += (long)s.label_index[0] * s.H * s.W;
    const int qw = s.W / PX;
    const long total = (long)s.H * qw, plane = (long)s.h * s.w, HW = (long)s.H * s.W;
    for (long i = (long)blockIdx.x * TS_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * TS_THREADS) {
        const int Y = (int)(i / qw), X = (int)(i - (long)Y * qw) * PX;
        const int iy0 = s.rowc[2 * Y], iy1 = iy0 + s.rowc[2 * Y + 1];
        const int ix0 = s.colc[2 * X], ix1 = ix0 + s.colc[2 * X + 1];
        float acc[NC][PX], ws[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            ws[j] = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c][j] = 0.f;
        }
        for (int iy = iy0; iy < iy1; ++iy) {
            const int ly = Y - s.ys[iy];
            const float gy = s.wy[ly];
            for (int ix = ix0; ix < ix1; ++ix) {
                const int lx = X - s.xs[ix];
                float g[PX];
#pragma unroll
                for (int j = 0; j < PX; ++j) g[j] = gy * s.wx[lx + j];
                const long view0 = (long)(iy * s.nx + ix) * s.nf;
                for (int f = 0; f < s.nf; ++f) {
                    const int k = s.flips[f];
                    const int sy = (k & 1) ? s.h - 1 - ly : ly;
                    const bool rev = (k & 2) != 0;
                    const int sx = rev ? s.w - PX - lx : lx;                      // where the run starts in memory
                    const float* src = s.logits + (view0 + f) * C * plane + (long)sy * s.w + sx;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        if (CT > 0 || c < C) {
                            float v[PX];
                            Vec<PX>::load(src + c * plane, v);
#pragma unroll
                            for (int j = 0; j < PX; ++j) {
                                const float t = rev ? v[PX - 1 - j] : v[j];
                                acc[c][j] = acc[c][j] + g[j] * t;
                            }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < PX; ++j) ws[j] = ws[j] + g[j];
                }
            }
        }
        const long o = (long)Y * s.W + X;
        float best[PX];
        int arg[PX];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (CT > 0 || c < C) {
                float r[PX];
#pragma unroll
                for (int j = 0; j < PX; ++j) {
                    r[j] = acc[c][j] / ws[j];
                    if (c == 0) { best[j] = r[j]; arg[j] = 0; }
                    else if (r[j] > best[j]) { best[j] = r[j]; arg[j] = c; }      // strict: the first maximum keeps its place
                }
                if (s.out) Vec<PX>::store(s.out + c * HW + o, r);
            }
        }
        unsigned packed = 0;                              // the PX class bytes, column j in byte j
#pragma unroll
        for (int j = 0; j < PX; ++j) packed |= (unsigned)arg[j] << (8 * j);
        if constexpr (PX == 4) *reinterpret_cast<unsigned*>(s.mask + o) = packed;
        else s.mask[o] = (unsigned char)packed;
        if (counting) {
            unsigned lab;
            if constexpr (PX == 4) lab = *reinterpret_cast<const unsigned*>(label + o);
            else lab = label[o];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const int t = (int)((lab >> (8 * j)) & 0xffu);
                if (t < C) atomicAdd(&hist[t * C + arg[j]], 1u);
            }
        }
    }
    if (counting) {
        __syncthreads();
        for (int i = threadIdx.x; i < C * C; i += TS_THREADS)
            if (hist[i]) atomicAdd(&s.counts[i], (unsigned long long)hist[i]);
    }
}

// grid (x, P): workgroup (bx, p) walks the pixels of view p
__global__ __launch_bounds__(TS_THREADS) void cd_view_counts_kernel(const float* __restrict__ logits,
                                                                    const unsigned char* __restrict__ labels, int C, long hw,
                                                                    unsigned long long* __restrict__ counts) {
    __shared__ unsigned int hist[MAXC * MAXC];
    for (int i = threadIdx.x; i < C * C; i += TS_THREADS) hist[i] = 0;
    __syncthreads();
    const long p = blockIdx.y;
    const float* src = logits + p * C * hw;
    const unsigned char* lab = labels + p * hw;
    for (long i = (long)blockIdx.x * TS_THREADS + threadIdx.x; i < hw; i += (long)gridDim.x * TS_THREADS) {
        float best = src[i];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float v = src[c * hw + i];
            if (v > best) { best = v; arg = c; }
        }
        const int t = lab[i];
        if (t < C) atomicAdd(&hist[t * C + arg], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += TS_THREADS)
        if (hist[i]) atomicAdd(&counts[p * C * C + i], (unsigned long long)hist[i]);
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }

template <int PX>
void launch_stitch(const Stitch& s, int grid, hipStream_t stream) {
    if (s.C == 2)
        hipLaunchKernelGGL((cd_tile_stitch_kernel<PX, 2>), dim3(grid), dim3(TS_THREADS), 0, stream, s);
    else
        hipLaunchKernelGGL((cd_tile_stitch_kernel<PX, 0>), dim3(grid), dim3(TS_THREADS), 0, stream, s);
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int dh_cd_tile_stitch(const float* logits, int P, int C, int h, int w, const int* ys, int ny, const int* xs, int nx,
                                 const int* flips, int nf, const float* wy, const float* wx, const int* row_cover,
                                 const int* col_cover, int x_align, int H, int W, float* out_logits, unsigned char* out_mask,
                                 const unsigned char* label, const int* label_index, long long* counts, void* stream) {
    DH_REQUIRE(logits && ys && xs && flips && wy && wx && row_cover && col_cover && out_mask, "cd_tile_stitch: null pointer");
    DH_REQUIRE((label != nullptr) == (counts != nullptr), "cd_tile_stitch: a label tile and counts come together");
    DH_REQUIRE(label || !label_index, "cd_tile_stitch: a label index without labels");
    DH_REQUIRE(C >= 1 && C <= MAXC, "cd_tile_stitch: n_class=%d unsupported (max %d)", C, MAXC);
    DH_REQUIRE(h >= 1 && w >= 1 && H >= h && W >= w, "cd_tile_stitch: window %dx%d in a %dx%d tile", h, w, H, W);
    DH_REQUIRE((long)H * W <= 0x7fffffffL, "cd_tile_stitch: %dx%d: a tile holds fewer than 2^31 pixels", H, W);
    DH_REQUIRE(ny >= 1 && nx >= 1 && nf >= 1 && nf <= 4, "cd_tile_stitch: %d x %d windows under %d flips", ny, nx, nf);
    DH_REQUIRE(ny <= H && nx <= W, "cd_tile_stitch: %d x %d windows in a %dx%d tile", ny, nx, H, W);
    DH_REQUIRE((long)ny * nx * nf == (long)P, "cd_tile_stitch: P=%d is not %d x %d windows under %d flips", P, ny, nx, nf);
    DH_REQUIRE(x_align == 1 || x_align == 4, "cd_tile_stitch: x_align=%d is neither 1 nor 4", x_align);
    Stitch s;
    s.logits = logits; s.ys = ys; s.xs = xs; s.flips = flips; s.rowc = row_cover; s.colc = col_cover; s.wy = wy; s.wx = wx;
    s.out = out_logits; s.mask = out_mask; s.label = label; s.label_index = label_index;
    s.counts = reinterpret_cast<unsigned long long*>(counts);
    s.C = C; s.h = h; s.w = w; s.nx = nx; s.nf = nf; s.H = H; s.W = W;
    const bool quad = x_align == 4 && (W & 3) == 0 && (w & 3) == 0 && aligned(logits, 16) && aligned(out_logits, 16) &&
                      aligned(out_mask, 4) && aligned(label, 4);
    const long units = ((long)H * (quad ? W / 4 : W) + TS_THREADS - 1) / TS_THREADS;
    const int grid = units > TS_MAX_WORKGROUPS ? TS_MAX_WORKGROUPS : (int)units;
    if (quad) launch_stitch<4>(s, grid, ST(stream));
    else launch_stitch<1>(s, grid, ST(stream));
    DH_CHECK_LAUNCH("cd_tile_stitch");
    return 0;
}

extern "C" int dh_cd_view_counts(const float* logits, const unsigned char* labels, int P, int C, int h, int w, long long* counts,
                                 void* stream) {
    DH_REQUIRE(logits && labels && counts, "cd_view_counts: null pointer");
    DH_REQUIRE(C >= 1 && C <= MAXC, "cd_view_counts: n_class=%d unsupported (max %d)", C, MAXC);
    DH_REQUIRE(P >= 1 && P <= 65535, "cd_view_counts: P=%d views (1 .. 65535)", P);
    DH_REQUIRE(h >= 1 && w >= 1, "cd_view_counts: empty view %dx%d", h, w);
    DH_REQUIRE((long)h * w <= 0x7fffffffL, "cd_view_counts: %dx%d: a view holds fewer than 2^31 pixels", h, w);
    const long hw = (long)h * w;
    long gx = (hw + TS_THREADS - 1) / TS_THREADS;
    if (gx > VC_MAX_X) gx = VC_MAX_X;
    hipLaunchKernelGGL(cd_view_counts_kernel, dim3((unsigned)gx, (unsigned)P), dim3(TS_THREADS), 0, ST(stream), logits, labels, C,
                       hw, reinterpret_cast<unsigned long long*>(counts));
    DH_CHECK_LAUNCH("cd_view_counts");
    return 0;
}
