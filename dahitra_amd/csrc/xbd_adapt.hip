// The loader of the xBD adaptation script, xBD_code/train_adapt.py: TrainData (lines 97-184) and ValData (196-245) as executed.
// One launch per batch: the S x S crop at (x0, y0) of the resident pre / post images as preprocess_inputs(concat(pre, post)) =
// x / 127 - 1, the script's FOUR mask planes and its label byte.  The script's augmentation sits inside a string literal
// (lines 115-146) and is not executed, so there is no geometry beyond the crop.  The planes are a pure function of the post
// label byte l (lines 147-175, 216-236):
//   m1 = l == 1, m2 = l == 2, m3 = l == 3 or 4 (destroyed merged with class 3)
//   m0 = m1 | m2 | m3 (train: line 165 clears the pre mask, line 172 sets the union) or pre_mask > 127 (val)
//   lbl = argmax(m1, m2, m3) = 1 where l == 2, 2 where l is 3 or 4, else 0
// A label byte above 4 sets no plane.  HBM-streaming: 8 bytes read and 29 written per pixel.  Where S % 4 == 0 a lane owns four
// pixels of a row and writes six 16-byte image stores, four mask dwords and one label dword (the sources as three dwords per
// image where their address allows, bytes otherwise); any other S goes pixel by pixel with byte stores.
#include "common.h"

namespace {

constexpr int AB_THREADS = 256;
constexpr int AB_MAX_BLOCKS_X = 1024;

// preprocess_inputs (xBD_code/utils.py): x /= 127, x -= 1, each rounded to float32 -- dh_xbd_augment_u8's expression
__device__ __forceinline__ float ab_norm(unsigned v) { return (float)v / 127.f - 1.f; }

// V consecutive bytes from p; one dword where V == 4 and the address allows
template <int V>
__device__ __forceinline__ void ab_bytes(const unsigned char* __restrict__ p, unsigned (&o)[V]) {
    if constexpr (V == 4) {
        if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
            const unsigned v = *reinterpret_cast<const unsigned*>(p);
            o[0] = v & 255u; o[1] = (v >> 8) & 255u; o[2] = (v >> 16) & 255u; o[3] = v >> 24;
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) o[k] = p[k];
}

// the 3 V bytes of V RGB pixels from p as rgb[channel][pixel]
template <int V>
__device__ __forceinline__ void ab_rgb(const unsigned char* __restrict__ p, unsigned (&rgb)[3][V]) {
    unsigned b[3 * V];
    if (V == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
#pragma unroll
        for (int q = 0; q < 3 * V / 4; ++q) {
            const unsigned v = reinterpret_cast<const unsigned*>(p)[q];
            b[4 * q] = v & 255u; b[4 * q + 1] = (v >> 8) & 255u; b[4 * q + 2] = (v >> 16) & 255u; b[4 * q + 3] = v >> 24;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3 * V; ++k) b[k] = p[k];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        rgb[0][k] = b[3 * k]; rgb[1][k] = b[3 * k + 1]; rgb[2][k] = b[3 * k + 2];
    }
}

template <int V>
__device__ __forceinline__ void ab_store(float* __restrict__ p, const unsigned (&v)[V]) {
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(ab_norm(v[0]), ab_norm(v[1]), ab_norm(v[2]), ab_norm(v[3]));
    } else {
        p[0] = ab_norm(v[0]);
    }
}

template <int V>
__device__ __forceinline__ void ab_store(unsigned char* __restrict__ p, const unsigned (&v)[V]) {
    if constexpr (V == 4) {
        *reinterpret_cast<unsigned*>(p) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
        p[0] = (unsigned char)v[0];
    }
}

// grid (gx, N): sample blockIdx.y, lanes of V pixels strided over gx workgroups; SV = S / V lanes per row
template <int V>
__global__ __launch_bounds__(AB_THREADS) void adapt_batch_kernel(const unsigned char* __restrict__ pre,
                                                                 const unsigned char* __restrict__ post,
                                                                 const unsigned char* __restrict__ pre_mask,
                                                                 const unsigned char* __restrict__ post_label,
                                                                 const int* __restrict__ idx, const int* __restrict__ origins,
                                                                 int n_src, int H, int W, int S, int mode,
                                                                 float* __restrict__ out_img, unsigned char* __restrict__ out_msk,
                                                                 unsigned char* __restrict__ out_lbl) {
    const int n = blockIdx.y;
    // whatever the tables hold, nothing outside the sources is read: the sample and the window are clamped into them
    const long src = min(max(idx[n], 0), n_src - 1);
    const int x0 = origins ? min(max(origins[2 * n], 0), W - S) : 0;
    const int y0 = origins ? min(max(origins[2 * n + 1], 0), H - S) : 0;
    const int SV = S / V;
    const long SS = (long)S * S, lanes = (long)S * SV;
    for (long i = (long)blockIdx.x * AB_THREADS + threadIdx.x; i < lanes; i += (long)gridDim.x * AB_THREADS) {
        const int y = (int)(i / SV), x = (int)(i - (long)y * SV) * V;
        const long at = (src * H + (y0 + y)) * W + (x0 + x);          // the source pixel
        const long o = (long)y * S + x;                               // the output pixel of a plane
        unsigned a[3][V], b[3][V], l[V], m0[V], m1[V], m2[V], m3[V], lb[V];
        ab_rgb<V>(pre + at * 3, a);
        ab_rgb<V>(post + at * 3, b);
        ab_bytes<V>(post_label + at, l);
        if (mode) {
            ab_bytes<V>(pre_mask + at, m0);
#pragma unroll
            for (int k = 0; k < V; ++k) m0[k] = m0[k] > 127u;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            m1[k] = l[k] == 1u;
            m2[k] = l[k] == 2u;
            m3[k] = l[k] == 3u || l[k] == 4u;
            if (!mode) m0[k] = m1[k] | m2[k] | m3[k];
            lb[k] = m2[k] ? 1u : m3[k] ? 2u : 0u;
        }
        float* img = out_img + (long)n * 6 * SS + o;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ab_store<V>(img + c * SS, a[c]);
            ab_store<V>(img + (3 + c) * SS, b[c]);
        }
        unsigned char* msk = out_msk + (long)n * 4 * SS + o;
        ab_store<V>(msk, m0);
        ab_store<V>(msk + SS, m1);
        ab_store<V>(msk + 2 * SS, m2);
        ab_store<V>(msk + 3 * SS, m3);
        ab_store<V>(out_lbl + (long)n * SS + o, lb);
    }
}

inline bool ab_aligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int dh_xbd_adapt_batch_u8(const unsigned char* pre, const unsigned char* post, const unsigned char* pre_mask,
                                     const unsigned char* post_label, const int* idx, const int* origins, int N, int n_src, int H,
                                     int W, int S, int mode, float* out_img, unsigned char* out_msk, unsigned char* out_lbl,
                                     void* stream) {
    DH_REQUIRE(pre && post && post_label && idx && out_img && out_msk && out_lbl, "xbd_adapt_batch: null pointer");
    DH_REQUIRE(mode == 0 || mode == 1, "xbd_adapt_batch: mode=%d is neither 0 (TrainData) nor 1 (ValData)", mode);
    DH_REQUIRE(mode == 0 || pre_mask, "xbd_adapt_batch: mode 1 (ValData) reads pre_mask, which is null");
    DH_REQUIRE(N >= 1 && N <= 65535, "xbd_adapt_batch: N=%d must be in 1..65535", N);
    DH_REQUIRE(n_src >= 1, "xbd_adapt_batch: n_src=%d sources", n_src);
    DH_REQUIRE(S >= 1 && S <= H && S <= W, "xbd_adapt_batch: crop %d does not fit the %dx%d image", S, H, W);
    DH_REQUIRE((long)H * W <= 0x7fffffffL, "xbd_adapt_batch: %dx%d: H * W must stay below 2^31", H, W);
    DH_REQUIRE(ab_aligned(out_img, 4), "xbd_adapt_batch: out_img is not 4-byte aligned");
    const bool vec = S % 4 == 0 && ab_aligned(out_img, 16) && ab_aligned(out_msk, 4) && ab_aligned(out_lbl, 4);
    const long lanes = vec ? (long)S * (S / 4) : (long)S * S;
    int gx = dh_cdiv(lanes, AB_THREADS);
    if (gx > AB_MAX_BLOCKS_X) gx = AB_MAX_BLOCKS_X;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(adapt_batch_kernel<4>, dim3(gx, N), dim3(AB_THREADS), 0, st, pre, post, pre_mask, post_label, idx, origins,
                           n_src, H, W, S, mode, out_img, out_msk, out_lbl);
    else
        hipLaunchKernelGGL(adapt_batch_kernel<1>, dim3(gx, N), dim3(AB_THREADS), 0, st, pre, post, pre_mask, post_label, idx, origins,
                           n_src, H, W, S, mode, out_img, out_msk, out_lbl);
    DH_CHECK_LAUNCH("xbd_adapt_batch");
    return 0;
}
