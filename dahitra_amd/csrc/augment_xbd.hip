// Input pipeline of the xBD step on the device (gfx950): TrainData / ValData.__getitem__ (xBD_code/train.py:99-183, 194-244) for
// pre-decoded samples.  Per sample: crop window, horizontal / vertical flip, TF.resized_crop(img, top, left, height, width,
// (S, S)) on both images, the pre mask and the post label (train.py:132-136), the five mask channels (train.py:144-172 / 215-233)
// and preprocess_inputs (utils.py:112-116).  One launch per batch, byte-exact against Pillow.
//
// TF.resized_crop on a PIL image is img.crop(box).resize((S, S), Image.BILINEAR).  Pillow's resize of an 8-bit image is two
// passes, each in 32-bit fixed point with a rounding to uint8 at its end (Resample.c): along the rows first, then along the columns
// of the horizontally resized rows.  An output index o of an axis has a first source index lo and coefficients k[t] in 2.22 fixed
// point; out = clip8(((1 << 21) + sum_t in[lo + t] * k[t]) >> 22).  The box only ever shrinks the source (in <= out), so the
// bilinear filter's support is 1 and an output index has three taps: the coefficient table is [n][2 axes][S][4] int32 =
// (lo, k0, k1, k2), axis 0 along x and axis 1 along y, written on the host in float64 as Pillow derives it
// (datasets/xbd_pipeline.resize_coeffs).  in == out gives (o, 1 << 22, 0, 0), the identity: the pass Pillow skips then needs no
// special case, and a sample without the resize flag takes the same path with these coefficients made up in the kernel.
//
// A workgroup owns a TW x TH tile of one sample's output.
//   1. Horizontal pass from global memory into LDS, as uint8 planes: pre R G B, post R G B, the label and (val mode) the pre mask,
//      for the source rows lo(ty0) .. lo(ty0 + TH - 1) + 2 the tile's output rows read -- at most TH + 2, because lo(o) =
//      int((o + 0.5) * in / out - 0.5) advances by at most one per output row.  A thread keeps its four output columns over all of
//      its rows (their coefficients and source offsets stay in registers) and writes their four bytes as one dword.  Crop origin,
//      flips and box are index arithmetic on these loads.
//   2. Vertical pass from LDS: four output bytes of three rows per lane, normalised through a 256-entry table ((float)v / 127.f -
//      1.f is an IEEE division per value otherwise) and stored as one float4 per lane; the label (and pre mask) 16 bytes per
//      lane, turned into the mask channels and stored 16 bytes per lane and channel.
// A tap whose coefficient is 0 by construction (at or beyond Pillow's xmax) may lie outside the box: every tap index is clamped
// into the box, every LDS row index into the rows staged, and every source coordinate into the image, so no table or parameter
// row makes the kernel read outside its sources.
//
// ColorJitter (train.py:138-139; dh_xbd_augment_jitter_u8) runs on the resized uint8 images, before the normalisation.  Each of
// its operations is PIL's Image.blend(degenerate, image, factor) per byte (jitter_blend8 below); contrast's degenerate image is
// the rounded mean of L over the WHOLE S x S image as it stands when contrast is applied, so a jittered batch takes two launches
// that share the tile code below (xbd_tile):
//   statistics  one workgroup per tile of every jittered (sample, image): the same two passes on that image's three planes, the
//               operations that precede contrast, and the integer sum of L over the tile's pixels inside S x S -> one partial per
//               workgroup, [N][2][tiles].  Integer sums are exact in any order: no atomics, no fill.
//   apply       the plain kernel with one change: a lane of the vertical image loop takes the four columns of all THREE planes
//               of an image (saturation needs R, G and B of a pixel together), applies the operations and looks the bytes up in
//               the normalisation table.  Every workgroup first adds up its sample's partials into the two means.
// The plain kernel is the instantiation without either: its code and registers do not depend on the jitter's.
#include "common.h"

// tile of a workgroup ("Device loader for the xBD step": tile shape and measured rate)
#ifndef DH_XBD_TW
#define DH_XBD_TW 64
#endif
#ifndef DH_XBD_TH
#define DH_XBD_TH 32
#endif

namespace {

// Pillow's clip8((1 << 21) + sum) of one pass.  0 <= k and k0 + k1 + k2 <= (1 << 22) + 8192 (the host checks both where it writes
// the table), so 0 <= acc < 256 << 22 and the clip never acts: a mask keeps the byte in range for a table that breaks the rule.
// It is a mask and not min / max on purpose: for two such clamps side by side hipcc (ROCm 7.2) picks v_ashr_pk_u8_i32 and ORs the
// other two bytes into its result as if that instruction cleared the upper 16 bits of its destination; gfx950 leaves them as they
// were.  Nothing but the byte-exact tests (tests/test_xbd_loader_gpu.py) keeps the compiler from choosing the packed form for
// another spelling of this: they are the guard.
__device__ __forceinline__ unsigned clip8(int acc) { return ((unsigned)acc >> 22) & 255u; }

// three taps on four packed bytes: out byte j = clip8((1 << 21) + a_j k.y + b_j k.z + c_j k.w); the products are exact 24-bit
// multiplies and the sum stays below 2^30
__device__ __forceinline__ unsigned vtap4(unsigned a, unsigned b, unsigned c, int4 k) {
    unsigned o = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int acc = (1 << 21) + __mul24((a >> (8 * j)) & 255u, k.y) + __mul24((b >> (8 * j)) & 255u, k.z) +
                        __mul24((c >> (8 * j)) & 255u, k.w);
        o |= clip8(acc) << (8 * j);
    }
    return o;
}

// what an instantiation of the tile code does
enum { XBD_PLAIN = 0, XBD_JITTER = 1, XBD_STATS = 2 };
constexpr int XBD_JW = 8;              // int32 words of a jitter row: enabled, the three operations in applied order, the factors' bits
constexpr int XBD_JITTER_MAX_S = 4096; // sum of L + S * S / 2 stays below 2^32

// one ColorJitter call: `on`, the operations in applied order (0 brightness, 1 contrast, 2 saturation; anything else is taken
// for saturation, so no row selects an address) and the factors of brightness, contrast and saturation.  Scalars passed by
// value, so that a row stays in (scalar) registers.
struct JitterRow {
    int on, op0, op1, op2;
    float fb, fc, fs;
};
__device__ __forceinline__ JitterRow jitter_row(const int* __restrict__ t) {
    return JitterRow{t[0] != 0, t[1], t[2], t[3], __int_as_float(t[4]), __int_as_float(t[5]), __int_as_float(t[6])};
}

// PIL's convert("L") of an RGB pixel (Convert.c, L24 >> 16 with rounding)
__device__ __forceinline__ unsigned luma(unsigned r, unsigned g, unsigned b) {
    return (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16;
}

// PIL's Image.blend(degenerate, image, alpha) of one byte (Blend.c): t = (float)d + alpha * (float)(i - d), the product rounded
// to float32 and then the sum -- NOT fused: fma(alpha, i - d, d) differs from Pillow for about one factor in 300, then for some
// hundred (d, i) pairs, so contraction is off here (tests/test_xbd_jitter_*.py pin two such factors).  0 <= alpha <= 1 keeps t
// between d and i and Pillow truncates; otherwise it clips to 0 .. 255 first: one clamp serves both.  The byte is masked like
// clip8's, and for the same reason.
__device__ __forceinline__ unsigned jitter_blend8(unsigned d, unsigned i, float alpha) {
#pragma clang fp contract(off)
    const float prod = alpha * (float)((int)i - (int)d);
    const float t = (float)(int)d + prod;
    return (unsigned)(int)fminf(fmaxf(t, 0.f), 255.f) & 255u;
}

// the operations of `j` on four packed pixels (byte q of r, g, b is pixel q), in applied order; `mean` is contrast's degenerate
// byte.  UNTIL_CONTRAST stops in front of contrast: the image whose L the statistics phase sums.
template <bool UNTIL_CONTRAST>
__device__ __forceinline__ void jitter4(const JitterRow j, unsigned mean, unsigned& r, unsigned& g, unsigned& b) {
    bool live = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int op = k == 0 ? j.op0 : k == 1 ? j.op1 : j.op2;
        if (UNTIL_CONTRAST && op == 1) live = false;
        if (!live) continue;                                               // uniform over the workgroup
        const float alpha = op == 0 ? j.fb : op == 1 ? j.fc : j.fs;
        unsigned nr = 0, ng = 0, nb = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned R = (r >> (8 * q)) & 255u, G = (g >> (8 * q)) & 255u, B = (b >> (8 * q)) & 255u;
            const unsigned d = op == 0 ? 0u : op == 1 ? mean : luma(R, G, B);
            nr |= jitter_blend8(d, R, alpha) << (8 * q);
            ng |= jitter_blend8(d, G, alpha) << (8 * q);
            nb |= jitter_blend8(d, B, alpha) << (8 * q);
        }
        r = nr, g = ng, b = nb;
    }
}

// sum over the workgroup's 256 threads (4 waves); every thread gets it.  `red` is 4 words of LDS the caller does not reuse
// before its next barrier.
__device__ __forceinline__ unsigned block_sum_u32(unsigned v, unsigned* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// KIND == XBD_PLAIN is dh_xbd_augment_u8's kernel: blockIdx.z is the sample, `jit` and `partial` are not read.  XBD_JITTER: the
// same with the rows `jit` [N][2][XBD_JW] applied to the images and `partial` [N][2][tiles] summed into contrast's means.
// XBD_STATS: blockIdx.z is 2 * sample + image; that image alone, nothing stored but partial[sample][image][tile] (the mask
// arguments and the outputs are not touched).
// (One kernel template and not a device function shared by three kernels: hipcc of ROCm 7.2 crashes while it inlines that.)
template <int TW, int TH, int KIND>
__global__ __launch_bounds__(256) void xbd_augment_u8_kernel(
    const unsigned char* __restrict__ pre, const unsigned char* __restrict__ post, const unsigned char* __restrict__ pmask,
    const unsigned char* __restrict__ label, const int* __restrict__ idx, const int* __restrict__ params,
    const int4* __restrict__ coef, int H, int W, int S, int mode, float* __restrict__ out_img,
    unsigned char* __restrict__ out_msk, unsigned char* __restrict__ out_lbl, int vec4, int vec16,
    const int* __restrict__ jit, unsigned* __restrict__ partial) {
    const int n = KIND == XBD_STATS ? blockIdx.z >> 1 : blockIdx.z, im = KIND == XBD_STATS ? blockIdx.z & 1 : 0;
    static_assert(TW % 16 == 0 && 256 % (TW / 4) == 0, "a lane stores 4 image pixels or 16 mask pixels; a thread keeps its columns");
    constexpr int ROWS = TH + 2;           // source rows of a tile
    constexpr int CG = TW / 4;             // dwords (groups of four columns) of a row
    constexpr int NP = KIND == XBD_STATS ? 3 : 8;      // planes staged
    __shared__ __attribute__((aligned(16))) unsigned hs[NP][ROWS][CG];
    __shared__ float lut[KIND == XBD_STATS ? 1 : 256];
    __shared__ unsigned red[KIND == XBD_PLAIN ? 1 : 2][4];
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const int tiles = gridDim.x * gridDim.y, tile = blockIdx.y * gridDim.x + blockIdx.x;
    JitterRow jr0 = {}, jr1 = {};                                           // pre and post; the statistics phase's image in jr0
    if constexpr (KIND == XBD_STATS) {
        jr0 = jitter_row(jit + (long)(2 * n + im) * XBD_JW);
        if (!jr0.on) return;                                                // the whole workgroup: this image is not jittered
    }
    if constexpr (KIND == XBD_JITTER) {
        // contrast's means, first half: this thread's share of the partial sums of an image (finished after the barrier below)
        auto share = [&](int i, const JitterRow j) {
            unsigned v = 0;
            if (j.on)
                for (int t = tid; t < tiles; t += 256) v += partial[(long)(2 * n + i) * tiles + t];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if ((tid & 63) == 0) red[i][tid >> 6] = v;
        };
        jr0 = jitter_row(jit + (long)(2 * n) * XBD_JW), jr1 = jitter_row(jit + (long)(2 * n + 1) * XBD_JW);
        share(0, jr0), share(1, jr1);
    }
    const int* pr = params + n * 9;
    const int x0 = pr[0], y0 = pr[1], hf = pr[2], vf = pr[3];
    const bool rs = pr[4] != 0 && coef != nullptr;
    const int top = rs ? pr[5] : 0, left = rs ? pr[6] : 0;
    const int bh = rs ? min(max(pr[7], 1), S) : S, bw = rs ? min(max(pr[8], 1), S) : S;
    const int4* cx = coef + (long)(2 * n) * S;
    const int4* cy = cx + S;
    const long sbase = (long)idx[n] * H * W;
    const long plane = (long)S * S;

    // (lo, k0, k1, k2) of output index o < S of an axis with `in` source pixels, lo inside the box
    auto tap_at = [&](const int4* c, int o, int in) {
        int4 t = rs ? c[o] : make_int4(o, 1 << 22, 0, 0);
        t.x = min(max(t.x, 0), in - 1);
        return t;
    };

    // preprocess_inputs: x /= 127, x -= 1, each rounded to float32
    if constexpr (KIND != XBD_STATS) lut[tid] = (float)tid / 127.f - 1.f;

    // ---- horizontal pass: global -> LDS ----
    const int cg = tid % CG;
    int4 kx[4];
    int sx[4][3];                                // source column of tap t of output column j: crop origin + flip + box, in the image
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        kx[j] = tap_at(cx, min(tx0 + 4 * cg + j, S - 1), bw);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int fx = left + min(kx[j].x + t, bw - 1);
            sx[j][t] = min(max(x0 + (hf ? S - 1 - fx : fx), 0), W - 1);
        }
    }
    const int r0 = tap_at(cy, ty0, bh).x;
    // rows staged: up to the last tap of the tile's last output row; without a resize only tap 0 of a row has a weight
    const int rlast = tap_at(cy, min(ty0 + TH - 1, S - 1), bh).x + (rs ? 3 : 1);
    const int nrows = max(min(min(rlast, bh) - r0, ROWS), 1);
    const int nplanes = KIND == XBD_STATS ? 3 : mode ? 8 : 7;
    for (int item = tid; item < nplanes * nrows * CG; item += 256) {       // item % CG == cg: 256 is a multiple of CG
        const int lp = item / (nrows * CG), row = (item / CG) % nrows;
        const int p = KIND == XBD_STATS ? 3 * im + lp : lp;                 // the statistics phase stages one image's planes
        const unsigned char* src;
        int ps;                                                             // bytes from a pixel to the next
        if (p < 3) src = pre + sbase * 3 + p, ps = 3;
        else if (p < 6) src = post + sbase * 3 + (p - 3), ps = 3;
        else if (p == 6) src = label + sbase, ps = 1;
        else src = pmask + sbase, ps = 1;
        const int fy = top + r0 + row;
        src += (long)min(max(y0 + (vf ? S - 1 - fy : fy), 0), H - 1) * W * ps;
        unsigned v[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 3; ++t) v[j][t] = src[sx[j][t] * ps];
        unsigned o = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o |= clip8((1 << 21) + __mul24(v[j][0], kx[j].y) + __mul24(v[j][1], kx[j].z) + __mul24(v[j][2], kx[j].w)) << (8 * j);
        hs[lp][row][cg] = o;
    }
    __syncthreads();

    // LDS rows of the three taps of output row oy
    auto rows_of = [&](int4 k, int* i) {
#pragma unroll
        for (int t = 0; t < 3; ++t) i[t] = min(max(k.x - r0 + t, 0), nrows - 1);
    };

    if constexpr (KIND == XBD_STATS) {
        // ---- vertical pass of one image, the operations in front of contrast, and the sum of L inside S x S ----
        unsigned sum = 0;
        for (int u = tid; u < TH * CG; u += 256) {
            const int g = u % CG, r = u / CG;
            const int oy = ty0 + r, ox = tx0 + 4 * g;
            if (oy >= S || ox >= S) continue;
            const int4 k = tap_at(cy, oy, bh);
            int i[3];
            rows_of(k, i);
            unsigned c[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] = vtap4(hs[ch][i[0]][g], hs[ch][i[1]][g], hs[ch][i[2]][g], k);
            jitter4<true>(jr0, 0u, c[0], c[1], c[2]);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (ox + q < S) sum += luma((c[0] >> (8 * q)) & 255u, (c[1] >> (8 * q)) & 255u, (c[2] >> (8 * q)) & 255u);
        }
        sum = block_sum_u32(sum, red[0]);
        if (tid == 0) partial[(long)(2 * n + im) * tiles + tile] = sum;
        return;
    }

    // one dword of plane p (four columns at (oy, ox)): normalised, 4 floats per lane
    auto store4 = [&](int p, int oy, int ox, unsigned d) {
        float* dst = out_img + ((long)n * 6 + p) * plane + (long)oy * S + ox;
        if (vec4) {                                                         // S % 4 == 0 and a 16-byte aligned output
            *reinterpret_cast<float4*>(dst) =
                make_float4(lut[d & 255u], lut[(d >> 8) & 255u], lut[(d >> 16) & 255u], lut[d >> 24]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ox + j < S) dst[j] = lut[(d >> (8 * j)) & 255u];
        }
    };

    if constexpr (KIND == XBD_JITTER) {
        // ---- vertical pass, images: a lane takes the three planes of an image, for the operations that need R, G and B ----
        const unsigned npx = (unsigned)S * (unsigned)S;
        auto image = [&](int m, const JitterRow j) {
            // int(mean + 0.5) of L = (2 sum + npx) / (2 npx) = (sum + npx / 2) / npx for either parity of npx
            const unsigned mean = (red[m][0] + red[m][1] + red[m][2] + red[m][3] + npx / 2) / npx;
            for (int u = tid; u < TH * CG; u += 256) {
                const int g = u % CG, r = u / CG;
                const int oy = ty0 + r, ox = tx0 + 4 * g;
                if (oy >= S || ox >= S) continue;
                const int4 k = tap_at(cy, oy, bh);
                int i[3];
                rows_of(k, i);
                unsigned c[3];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    c[ch] = vtap4(hs[3 * m + ch][i[0]][g], hs[3 * m + ch][i[1]][g], hs[3 * m + ch][i[2]][g], k);
                if (j.on) jitter4<false>(j, mean, c[0], c[1], c[2]);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) store4(3 * m + ch, oy, ox, c[ch]);
            }
        };
        image(0, jr0), image(1, jr1);
    } else {
        // ---- vertical pass, images: normalise and store 4 floats per lane ----
        for (int u = tid; u < 6 * TH * CG; u += 256) {
            const int g = u % CG, r = (u / CG) % TH, p = u / (CG * TH);
            const int oy = ty0 + r, ox = tx0 + 4 * g;
            if (oy >= S || ox >= S) continue;
            const int4 k = tap_at(cy, oy, bh);
            int i[3];
            rows_of(k, i);
            store4(p, oy, ox, vtap4(hs[p][i[0]][g], hs[p][i[1]][g], hs[p][i[2]][g], k));
        }
    }

    // ---- vertical pass, label (and pre mask): the mask channels, 16 pixels per lane ----
    // train (train.py:144-172): msk[k] = (label == k), k = 1 .. 4; msk[0] = any of them (the pre mask is overwritten).
    // val (train.py:215-235): msk[0] = (pre mask > 127); lbl_msk = argmax(msk[1:]) = label - 1 on 1 .. 4, else 0.
    for (int u = tid; u < TH * (TW / 16); u += 256) {
        const int g = u % (TW / 16), r = u / (TW / 16);
        const int oy = ty0 + r, ox = tx0 + 16 * g;
        if (oy >= S || ox >= S) continue;
        const int4 k = tap_at(cy, oy, bh);
        int i[3];
        rows_of(k, i);
        unsigned m[5][4], lb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = 4 * g + q;
            const unsigned L = vtap4(hs[6][i[0]][c], hs[6][i[1]][c], hs[6][i[2]][c], k);
            const unsigned M = mode ? vtap4(hs[7][i[0]][c], hs[7][i[1]][c], hs[7][i[2]][c], k) : 0u;
#pragma unroll
            for (int ch = 0; ch < 5; ++ch) m[ch][q] = 0;
            lb[q] = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned l = (L >> (8 * j)) & 255u;
                const unsigned any = (l >= 1u && l <= 4u) ? 1u : 0u;
                m[0][q] |= (mode ? (((M >> (8 * j)) & 255u) > 127u ? 1u : 0u) : any) << (8 * j);
#pragma unroll
                for (int ch = 1; ch < 5; ++ch) m[ch][q] |= (l == (unsigned)ch ? 1u : 0u) << (8 * j);
                lb[q] |= (any ? l - 1u : 0u) << (8 * j);
            }
        }
        const long at = (long)oy * S + ox;
        unsigned char* dm = out_msk + (long)n * 5 * plane + at;
        if (vec16) {                                                        // S % 16 == 0 and 16-byte aligned outputs
#pragma unroll
            for (int ch = 0; ch < 5; ++ch)
                *reinterpret_cast<uint4*>(dm + ch * plane) = make_uint4(m[ch][0], m[ch][1], m[ch][2], m[ch][3]);
            if (mode) *reinterpret_cast<uint4*>(out_lbl + (long)n * plane + at) = make_uint4(lb[0], lb[1], lb[2], lb[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (ox + j < S) {
#pragma unroll
                    for (int ch = 0; ch < 5; ++ch) dm[ch * plane + j] = (unsigned char)((m[ch][j >> 2] >> (8 * (j & 3))) & 255u);
                    if (mode) out_lbl[(long)n * plane + at + j] = (unsigned char)((lb[j >> 2] >> (8 * (j & 3))) & 255u);
                }
        }
    }
}


}  // namespace

// the checks both entries share
static int xbd_check_args(const char* who, const unsigned char* pre, const unsigned char* post, const unsigned char* pre_mask,
                          const unsigned char* post_label, const int* idx, const int* params, const int* coef, int N, int H, int W,
                          int S, int mode, float* out_img, unsigned char* out_msk, unsigned char* out_lbl) {
    DH_REQUIRE(N > 0 && S > 0 && S <= H && S <= W, "%s: bad sizes N=%d %dx%d -> %d", who, N, H, W, S);
    DH_REQUIRE(N <= 65535 && dh_cdiv(S, DH_XBD_TH) <= 65535, "%s: N=%d S=%d exceed the launch grid", who, N, S);
    DH_REQUIRE(mode == 0 || mode == 1, "%s: mode %d is neither 0 (train) nor 1 (val)", who, mode);
    DH_REQUIRE(pre != nullptr && post != nullptr && post_label != nullptr && idx != nullptr && params != nullptr,
               "%s: a source or table pointer is NULL", who);
    DH_REQUIRE(out_img != nullptr && out_msk != nullptr, "%s: an output pointer is NULL", who);
    DH_REQUIRE(mode == 0 || (pre_mask != nullptr && out_lbl != nullptr), "%s: val mode needs pre_mask and out_lbl", who);
    DH_REQUIRE((uintptr_t)coef % 16 == 0, "%s: the coefficient table is read 16 bytes at a time", who);
    return 0;
}

extern "C" int dh_xbd_augment_u8(const unsigned char* pre, const unsigned char* post, const unsigned char* pre_mask,
                                 const unsigned char* post_label, const int* idx, const int* params, const int* coef, int N, int H,
                                 int W, int S, int mode, float* out_img, unsigned char* out_msk, unsigned char* out_lbl,
                                 void* stream) {
    constexpr int TW = DH_XBD_TW, TH = DH_XBD_TH;
    if (xbd_check_args("xbd_augment_u8", pre, post, pre_mask, post_label, idx, params, coef, N, H, W, S, mode, out_img, out_msk,
                       out_lbl))
        return 1;
    const int vec4 = S % 4 == 0 && (uintptr_t)out_img % 16 == 0;
    const int vec16 = S % 16 == 0 && (uintptr_t)out_msk % 16 == 0 && (mode == 0 || (uintptr_t)out_lbl % 16 == 0);
    hipLaunchKernelGGL((xbd_augment_u8_kernel<TW, TH, XBD_PLAIN>), dim3(dh_cdiv(S, TW), dh_cdiv(S, TH), N), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), pre, post, pre_mask, post_label, idx, params,
                       reinterpret_cast<const int4*>(coef), H, W, S, mode, out_img, out_msk, out_lbl, vec4, vec16,
                       (const int*)nullptr, (unsigned*)nullptr);
    DH_CHECK_LAUNCH("xbd_augment_u8");
    return 0;
}

// tiles (workgroups) of an S x S image.  dh_xbd_augment_jitter_u8's workspace holds the device copy of the jitter table, then one
// partial sum per tile and image: N * 2 * (8 + tiles) * 4 bytes.
extern "C" int dh_xbd_augment_jitter_tiles(int S) {
    if (S <= 0 || S > XBD_JITTER_MAX_S) return 0;
    return dh_cdiv(S, DH_XBD_TW) * dh_cdiv(S, DH_XBD_TH);
}

extern "C" int dh_xbd_augment_jitter_u8(const unsigned char* pre, const unsigned char* post, const unsigned char* pre_mask,
                                        const unsigned char* post_label, const int* idx, const int* params, const int* coef,
                                        const int* jitter_host, int N, int H, int W, int S, int mode, float* out_img,
                                        unsigned char* out_msk, unsigned char* out_lbl, void* workspace, long workspace_bytes,
                                        void* stream) {
    constexpr int TW = DH_XBD_TW, TH = DH_XBD_TH;
    const char* who = "xbd_augment_jitter_u8";
    if (xbd_check_args(who, pre, post, pre_mask, post_label, idx, params, coef, N, H, W, S, mode, out_img, out_msk, out_lbl)) return 1;
    DH_REQUIRE(2 * N <= 65535, "%s: N=%d exceeds the statistics launch grid", who, N);
    DH_REQUIRE(S <= XBD_JITTER_MAX_S, "%s: S=%d: the 32-bit sum of L holds images up to %d x %d", who, S, XBD_JITTER_MAX_S,
               XBD_JITTER_MAX_S);
    DH_REQUIRE(jitter_host != nullptr && workspace != nullptr, "%s: the jitter table or the workspace is NULL", who);
    const long need = (long)N * 2 * (XBD_JW + dh_xbd_augment_jitter_tiles(S)) * 4;
    DH_REQUIRE((uintptr_t)workspace % 4 == 0 && workspace_bytes >= need, "%s: a workspace of %ld bytes, %ld needed (4-byte aligned)",
               who, workspace_bytes, need);
    int any = 0;
    for (int r = 0; r < 2 * N; ++r) {
        const int* t = jitter_host + (long)r * XBD_JW;
        DH_REQUIRE(t[0] == 0 || t[0] == 1, "%s: row %d: the enabled flag is %d", who, r, t[0]);
        if (!t[0]) continue;
        any = 1;
        for (int k = 0; k < 3; ++k)
            DH_REQUIRE(t[1 + k] >= 0 && t[1 + k] <= 2, "%s: row %d: operation %d is none of 0 (brightness), 1 (contrast), 2 (saturation)",
                       who, r, t[1 + k]);
        DH_REQUIRE(t[1] != t[2] && t[1] != t[3] && t[2] != t[3], "%s: row %d: an operation occurs twice", who, r);
        for (int k = 0; k < 3; ++k)
            DH_REQUIRE((t[4 + k] & 0x7f800000) != 0x7f800000, "%s: row %d: factor %d is not finite", who, r, k);
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int* jit = static_cast<int*>(workspace);
    unsigned* partial = reinterpret_cast<unsigned*>(jit + (long)N * 2 * XBD_JW);
    const hipError_t e = hipMemcpyAsync(jit, jitter_host, (size_t)N * 2 * XBD_JW * 4, hipMemcpyHostToDevice, st);
    DH_REQUIRE(e == hipSuccess, "%s: copying the jitter table: %s", who, hipGetErrorString(e));
    const int vec4 = S % 4 == 0 && (uintptr_t)out_img % 16 == 0;
    const int vec16 = S % 16 == 0 && (uintptr_t)out_msk % 16 == 0 && (mode == 0 || (uintptr_t)out_lbl % 16 == 0);
    const int4* coef4 = reinterpret_cast<const int4*>(coef);
    if (any) {
        hipLaunchKernelGGL((xbd_augment_u8_kernel<TW, TH, XBD_STATS>), dim3(dh_cdiv(S, TW), dh_cdiv(S, TH), 2 * N), dim3(256), 0, st,
                           pre, post, pre_mask, post_label, idx, params, coef4, H, W, S, mode, out_img, out_msk, out_lbl, vec4,
                           vec16, (const int*)jit, partial);
        DH_CHECK_LAUNCH("xbd_jitter_stats");
    }
    hipLaunchKernelGGL((xbd_augment_u8_kernel<TW, TH, XBD_JITTER>), dim3(dh_cdiv(S, TW), dh_cdiv(S, TH), N), dim3(256), 0, st, pre,
                       post, pre_mask, post_label, idx, params, coef4, H, W, S, mode, out_img, out_msk, out_lbl, vec4, vec16,
                       (const int*)jit, partial);
    DH_CHECK_LAUNCH(who);
    return 0;
}
