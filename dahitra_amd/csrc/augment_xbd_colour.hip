// Colour stage of DAHiTra's own xBD training script on the device (gfx950): lines 211-244 of TrainData.__getitem__ in
// xBD_code/train_unettransformer.py -- change_hsv, then ONE of gauss_noise, cv2.blur(3 x 3), saturation, brightness, contrast per
// image -- applied IN PLACE to the [N][6][S][S] float32 batch dh_xbd_augment_warp_u8 wrote.  clahe and imgaug's elastic transform
// are not built.  datasets/xbd_pipeline.unet_colour_reference_u8 states the bytes; the header states the arithmetic.
//
// About one sample in thirty draws any of this, so the input is a compact job table, one row per (sample, image) that drew
// something, and a workgroup of the grid (tiles x tiles x J) works on one 32 x 32 tile of one job's three planes.  Samples
// without a job are never touched.  Two launches whatever the jobs:
//   1. decode the floats to bytes (byte = rint((f + 1) 127), which inverts the 256-entry table x / 127 - 1 exactly), change_hsv
//      where the job has it, bytes to a scratch [J][3][S][S], and the tile's three channel sums as integers to sums[J][tiles][3];
//   2. the block operation from the scratch -- blur gathers its 3 x 3 window under reflect-101 there, across tile borders, which
//      is why the bytes cannot stay in the batch; contrast adds up the tile sums of its image -- then encode and store.
// No floating-point sum crosses lanes, no atomics and no workspace to zero: the result does not depend on the schedule.
//
// The float64 blends and the float32 HSV return are stated product by product: nothing in this file may be contracted into a
// fused multiply-add (hipcc contracts by default), hence the pragma below and -ffp-contract=off on this file in the Makefile.
//
// Bounds: whatever the table holds, the sample and the noise plane are clamped, the image is one bit, the shifts are clamped to
// +-255, an unknown op code is none, every decoded byte is clamped before it indexes a table, and reflect-101 is closed form.
// Two rows that name the same (sample, image) race on its bytes; the pipeline writes at most one.
#include "common.h"

#pragma clang fp contract(off)

#ifndef DH_XBD_COLOUR_TILE
#define DH_XBD_COLOUR_TILE 32
#endif

namespace {

constexpr int XC_JW = 12;                       // int32 words of a job row
constexpr int XC_T = DH_XBD_COLOUR_TILE;        // the tile is square, a lane takes four pixels of a row
constexpr int XC_CG = XC_T / 4;
constexpr int XC_MAX_S = 4096;                  // 32-bit channel sums of a whole image: 4096^2 * 255 < 2^32
static_assert(XC_T % 4 == 0 && XC_CG * XC_T == 256, "256 lanes take the tile, four pixels of a row each");

enum { OP_NONE = 0, OP_NOISE = 1, OP_BLUR = 2, OP_SATURATION = 3, OP_BRIGHTNESS = 4, OP_CONTRAST = 5 };

struct Job {
    int n, im, hsv, dh, ds, dv, op, noise;
    double alpha;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ Job read_job(const int* __restrict__ jobs, int j, int N, int K) {
    const int* r = jobs + (long)j * XC_JW;
    Job jb;
    jb.n = clampi(r[0], 0, N - 1);
    jb.im = r[1] & 1;
    jb.hsv = r[2] != 0;
    jb.dh = clampi(r[3], -255, 255), jb.ds = clampi(r[4], -255, 255), jb.dv = clampi(r[5], -255, 255);
    jb.op = r[6] >= OP_NOISE && r[6] <= OP_CONTRAST ? r[6] : OP_NONE;
    if (jb.op == OP_NOISE && K <= 0) jb.op = OP_NONE;
    const unsigned long long bits = (unsigned long long)(unsigned)r[7] | ((unsigned long long)(unsigned)r[8] << 32);
    jb.alpha = __longlong_as_double((long long)bits);
    jb.noise = clampi(r[9], 0, max(K - 1, 0));
    return jb;
}

// cv2.BORDER_REFLECT_101 of any p into 0 .. S - 1; m = 2 (S - 1)
__device__ __forceinline__ int reflect101(int p, int S, int m) {
    if (m == 0) return 0;
    p %= m;
    if (p < 0) p += m;
    return p >= S ? m - p : p;
}

// rint(a / d), half to even, of positive integers: what float64 gives for OpenCV's sdiv / hdiv tables (the quotient of integers
// this small is never within a rounding error of a tie it is not on)
__device__ __forceinline__ int rint_div(int a, int d) {
    const int q = a / d, r = a % d;
    return q + ((2 * r > d || (2 * r == d && (q & 1))) ? 1 : 0);
}

// the (b, g, r) of OpenCV's sector table {1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}, two bits a sector
constexpr unsigned pack6(int a, int b, int c, int d, int e, int f) {
    return (unsigned)a | (unsigned)b << 2 | (unsigned)c << 4 | (unsigned)d << 6 | (unsigned)e << 8 | (unsigned)f << 10;
}
constexpr unsigned SEL_B = pack6(1, 1, 3, 0, 0, 2), SEL_G = pack6(3, 0, 0, 2, 1, 1), SEL_R = pack6(0, 2, 1, 1, 3, 0);

__device__ __forceinline__ int byte_of(float x) { return (int)rintf(fminf(fmaxf(x * 255.f, 0.f), 255.f)); }

// utils.change_hsv on one pixel: 8-bit COLOR_BGR2HSV (integer, hsv_shift 12), the clipped shifts, 8-bit COLOR_HSV2BGR (float32)
__device__ __forceinline__ void change_hsv(int& r, int& g, int& b, const Job& jb, const int* sdiv, const int* hdiv) {
    const int V = max(max(b, g), r), d = V - min(min(b, g), r);
    int Sx = (d * sdiv[V] + 2048) >> 12;
    const int H0 = V == r ? g - b : V == g ? b - r + 2 * d : r - g + 4 * d;
    int Hx = (H0 * hdiv[d] + 2048) >> 12;
    if (Hx < 0) Hx += 180;
    Hx = clampi(clampi(Hx, 0, 255) + jb.dh, 0, 255);
    Sx = clampi(clampi(Sx, 0, 255) + jb.ds, 0, 255);
    const int Vx = clampi(V + jb.dv, 0, 255);
    float h = (float)Hx * (float)(6.0 / 180.0);
    const float s = (float)Sx * (float)(1.0 / 255.0), v = (float)Vx * (float)(1.0 / 255.0);
    float fb = v, fg = v, fr = v;
    if (s != 0.f) {
        h = h >= 6.f ? h - 6.f : h;                  // fmod(h, 6): h <= 255 * 6 / 180 < 12, and the difference is exact
        const float k = floorf(h);
        float f = h - k;
        int sector = (int)k;
        if ((unsigned)sector >= 6u) sector = 0, f = 0.f;
        const float t0 = v, t1 = v * (1.f - s), t2 = v * (1.f - s * f), t3 = v * (1.f - s * (1.f - f));
        auto pick = [&](unsigned sel) {
            const unsigned i = (sel >> (2 * sector)) & 3u;
            return i == 0 ? t0 : i == 1 ? t1 : i == 2 ? t2 : t3;
        };
        fb = pick(SEL_B), fg = pick(SEL_G), fr = pick(SEL_R);
    }
    b = byte_of(fb), g = byte_of(fg), r = byte_of(fr);
}

// launch 1: floats -> bytes, change_hsv, scratch and tile sums
__global__ __launch_bounds__(256) void xbd_colour_hsv_kernel(const float* __restrict__ img, const int* __restrict__ jobs, int N,
                                                             int S, unsigned char* __restrict__ scratch,
                                                             unsigned* __restrict__ sums, int vec4) {
    __shared__ int sdiv[256], hdiv[256];
    __shared__ unsigned red[4][3];
    const int tid = threadIdx.x, j = blockIdx.z;
    const Job jb = read_job(jobs, j, N, 0);
    if (jb.hsv) {                                                           // uniform over the workgroup
        sdiv[tid] = tid ? rint_div(255 << 12, tid) : 0;
        hdiv[tid] = tid ? rint_div(180 << 12, 6 * tid) : 0;
        __syncthreads();
    }
    const int oy = blockIdx.y * XC_T + tid / XC_CG, ox = blockIdx.x * XC_T + 4 * (tid % XC_CG);
    const long plane = (long)S * S, at = (long)oy * S + ox;
    unsigned sum[3] = {0, 0, 0};
    if (oy < S && ox < S) {
        const float* src = img + ((long)jb.n * 6 + 3 * jb.im) * plane + at;
        float val[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (vec4) {                                                     // S % 4 == 0 and a 16-byte aligned batch
                const float4 q = *reinterpret_cast<const float4*>(src + c * plane);
                val[c][0] = q.x, val[c][1] = q.y, val[c][2] = q.z, val[c][3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) val[c][k] = ox + k < S ? src[c * plane + k] : -1.f;
            }
        }
        unsigned pk[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (ox + k >= S) break;
            int px[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = (int)rintf(fminf(fmaxf((val[c][k] + 1.f) * 127.f, 0.f), 255.f));
            if (jb.hsv) change_hsv(px[0], px[1], px[2], jb, sdiv, hdiv);
#pragma unroll
            for (int c = 0; c < 3; ++c) pk[c] |= (unsigned)px[c] << (8 * k), sum[c] += (unsigned)px[c];
        }
        unsigned char* dst = scratch + (long)j * 3 * plane + at;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (S % 4 == 0) {                                               // the scratch is 4-byte aligned
                *reinterpret_cast<unsigned*>(dst + c * plane) = pk[c];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (ox + k < S) dst[c * plane + k] = (unsigned char)((pk[c] >> (8 * k)) & 255u);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        unsigned v = sum[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((tid & 63) == 0) red[tid >> 6][c] = v;
    }
    __syncthreads();
    if (tid < 3) {
        const long tile = (long)blockIdx.y * gridDim.x + blockIdx.x;
        sums[((long)j * gridDim.x * gridDim.y + tile) * 3 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    }
}

// launch 2: the block operation from the scratch, encode, store
__global__ __launch_bounds__(256) void xbd_colour_apply_kernel(float* __restrict__ img, const int* __restrict__ jobs,
                                                               const unsigned char* __restrict__ noise, int N, int S, int K,
                                                               const unsigned char* __restrict__ scratch,
                                                               const unsigned* __restrict__ sums, int vec4) {
    __shared__ float lut[256];
    __shared__ unsigned long long red[4][3];
    const int tid = threadIdx.x, j = blockIdx.z;
    // preprocess_inputs: x /= 127, x -= 1, each rounded to float32 (augment_xbd_warp.hip's table)
    lut[tid] = (float)tid / 127.f - 1.f;
    const Job jb = read_job(jobs, j, N, noise != nullptr ? K : 0);
    const double alpha = jb.alpha, oma = 1.0 - alpha;
    if (jb.op == OP_CONTRAST) {                                             // uniform over the workgroup
        const int tiles = gridDim.x * gridDim.y;
        unsigned long long part[3] = {0, 0, 0};
        for (int t = tid; t < tiles; t += 256)
#pragma unroll
            for (int c = 0; c < 3; ++c) part[c] += sums[((long)j * tiles + t) * 3 + c];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            unsigned long long v = part[c];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if ((tid & 63) == 0) red[tid >> 6][c] = v;
        }
    }
    __syncthreads();
    double term = 0.0;                                                      // contrast: (1 - alpha) * mean
    if (jb.op == OP_CONTRAST) {
        const double sr = (double)(red[0][0] + red[1][0] + red[2][0] + red[3][0]);
        const double sg = (double)(red[0][1] + red[1][1] + red[2][1] + red[3][1]);
        const double sb = (double)(red[0][2] + red[1][2] + red[2][2] + red[3][2]);
        const double mean = ((0.114 * sb + 0.587 * sg) + 0.299 * sr) / (double)((long)S * S);
        term = oma * mean;
    }
    const int oy = blockIdx.y * XC_T + tid / XC_CG, ox = blockIdx.x * XC_T + 4 * (tid % XC_CG);
    if (oy >= S || ox >= S) return;
    const long plane = (long)S * S, at = (long)oy * S + ox;
    const unsigned char* sc = scratch + (long)j * 3 * plane;

    int px[3][4];
    if (jb.op == OP_BLUR) {
        const int m = 2 * (S - 1);
        int rows[3], cols[6];
#pragma unroll
        for (int i = 0; i < 3; ++i) rows[i] = reflect101(oy - 1 + i, S, m);
#pragma unroll
        for (int i = 0; i < 6; ++i) cols[i] = reflect101(ox - 1 + i, S, m);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int cs[6];
#pragma unroll
            for (int i = 0; i < 6; ++i)
                cs[i] = (int)sc[c * plane + (long)rows[0] * S + cols[i]] + (int)sc[c * plane + (long)rows[1] * S + cols[i]] +
                        (int)sc[c * plane + (long)rows[2] * S + cols[i]];
#pragma unroll
            for (int k = 0; k < 4; ++k) px[c][k] = (2 * (cs[k] + cs[k + 1] + cs[k + 2]) + 9) / 18;     // nearest ninth, no ties
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) px[c][k] = (int)sc[c * plane + at + min(k, S - 1 - ox)];
    }
    if (jb.op == OP_NOISE) {
        const unsigned char* nz = noise + ((long)jb.noise * plane + at) * 3;    // [K][S][S][3] in the script's order: B, G, R
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long o = 3L * min(k, S - 1 - ox);
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c][k] = min(px[c][k] + (int)nz[o + 2 - c], 255);
        }
    } else if (jb.op == OP_SATURATION || jb.op == OP_BRIGHTNESS || jb.op == OP_CONTRAST) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double r = (double)px[0][k], g = (double)px[1][k], b = (double)px[2][k];
            double add = term;
            if (jb.op == OP_SATURATION) add = oma * ((0.114 * b + 0.587 * g) + 0.299 * r);
            if (jb.op == OP_BRIGHTNESS) add = oma * 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c)                                     // np.clip(img * alpha + (1 - alpha) * gs, 0, 255), truncated
                px[c][k] = (int)fmin(fmax((double)px[c][k] * alpha + add, 0.0), 255.0);
        }
    }

    float* dst = img + ((long)jb.n * 6 + 3 * jb.im) * plane + at;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (vec4) {
            *reinterpret_cast<float4*>(dst + c * plane) = make_float4(lut[px[c][0] & 255], lut[px[c][1] & 255], lut[px[c][2] & 255],
                                                                     lut[px[c][3] & 255]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ox + k < S) dst[c * plane + k] = lut[px[c][k] & 255];
        }
    }
}

long colour_scratch_bytes(int J, int S) { return ((3L * J * S * S + 3) / 4) * 4; }
long colour_ws_bytes(int J, int S) {
    const long tiles = (long)dh_cdiv(S, XC_T) * dh_cdiv(S, XC_T);
    return colour_scratch_bytes(J, S) + 4L * J * tiles * 3;
}

}  // namespace

extern "C" int dh_xbd_unet_colour_tile(void) { return XC_T; }

extern "C" int dh_xbd_unet_colour_ws_bytes(int J, int S, long* bytes) {
    const char* who = "xbd_unet_colour_ws_bytes";
    DH_REQUIRE(bytes != nullptr, "%s: null pointer", who);
    DH_REQUIRE(J > 0 && J <= 65535 && S > 0 && S <= XC_MAX_S, "%s: bad sizes J=%d S=%d (J <= 65535, S <= %d)", who, J, S, XC_MAX_S);
    *bytes = colour_ws_bytes(J, S);
    return 0;
}

extern "C" int dh_xbd_unet_colour_u8(float* img, const int* jobs, const unsigned char* noise, int N, int S, int J, int K,
                                     void* workspace, long workspace_bytes, void* stream) {
    const char* who = "xbd_unet_colour";
    DH_REQUIRE(N > 0 && S > 0 && S <= XC_MAX_S && J > 0 && J <= 65535 && K >= 0,
               "%s: bad sizes N=%d S=%d J=%d K=%d (S <= %d, 1 <= J <= 65535, K >= 0)", who, N, S, J, K, XC_MAX_S);
    DH_REQUIRE(img != nullptr && jobs != nullptr && workspace != nullptr, "%s: the batch, the job table or the workspace is NULL", who);
    DH_REQUIRE((noise != nullptr) == (K > 0), "%s: %d noise planes with a %s noise pointer", who, K, noise ? "non-NULL" : "NULL");
    DH_REQUIRE((uintptr_t)workspace % 4 == 0 && (uintptr_t)img % 4 == 0, "%s: the batch and the workspace hold 32-bit words", who);
    const long need = colour_ws_bytes(J, S);
    DH_REQUIRE(workspace_bytes >= need, "%s: a workspace of %ld bytes, %ld are needed", who, workspace_bytes, need);
    unsigned char* scratch = reinterpret_cast<unsigned char*>(workspace);
    unsigned* sums = reinterpret_cast<unsigned*>(scratch + colour_scratch_bytes(J, S));
    const int vec4 = S % 4 == 0 && (uintptr_t)img % 16 == 0;
    const dim3 grid(dh_cdiv(S, XC_T), dh_cdiv(S, XC_T), J);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(xbd_colour_hsv_kernel, grid, dim3(256), 0, st, img, jobs, N, S, scratch, sums, vec4);
    DH_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(xbd_colour_apply_kernel, grid, dim3(256), 0, st, img, jobs, noise, N, S, K, scratch, sums, vec4);
    DH_CHECK_LAUNCH(who);
    return 0;
}
