// The terms of xBD_code/losses.py's ComboLoss that csrc/xbd_step.hip does not compute:
//   lovasz, lovasz_sigmoid ... lovasz_hinge / lovasz_sigmoid_flat (losses.py:129-225): a stable segmented sort of the errors, a
//                              scan over the sorted labels and the gradient of the Lovasz extension in closed form
//   jaccard, bce, mask_bceavg  (losses.py:36-45, 70-92): one pass, a finalize launch and one gradient pass
//
// ---- Lovasz ----
// x [B][C][HW] fp32, targets fp32 or uint8.  A SEGMENT is what the reference sorts on its own: a channel over the whole batch
// (per_image 0, segment = c) or one plane (per_image 1, segment = b * C + c).  Every segment has L = n / segments elements.
//   error     e = fl32(1 - x (2 t - 1))             mode 0, weight max(e, 0)
//             e = |t - x|                           mode 1
//             e = |t - p|, p = 1 / (1 + expf(-x))   mode 2
//   key       the order-preserving unsigned image of e, inverted so that ascending keys are descending errors; -0 is keyed as
//             +0.  An element whose target is `ignore` or no label at all takes the key 0xffffffff, behind every valid element
//             of its segment (a valid key is at most 0xfffffffe).
//   payload   the flat index (30 bits, n <= 2^30) with the label in bit 31
//   sort      least-significant-digit radix sort, 8 bits a pass: four passes over the key and, with more than one segment, a
//             fifth over the segment id.  A pass is three launches -- per-workgroup digit histogram, scan, scatter -- and no
//             workgroup ever waits for another one.  Every pass is stable, so equal errors keep flat index order.
//               histogram: counts[digit][workgroup] (LDS integer atomics) and totals[pass][digit] (one global integer atomic
//                          per digit and workgroup)
//               scan:      workgroup d takes the sum of totals[pass][< d] and runs along its row counts[d][:] with a carry
//               scatter:   a wave ranks its 64 keys by __ballot on the eight digit bits (lanes of one digit, in lane order),
//                          eight rounds per wave, four waves per tile in index order
//   after it  the sorted payloads lie segment after segment.  Per tile of a segment: the ones and the valid elements
//             (lv_tile_count_kernel), their exclusive prefix along the segment and the segment's G (lv_seg_scan_kernel), then
//             per element, with c1 / c0 the ones / zeros up to and including it, I = G - c1, U = G + c0:
//               g = 1 - I / U        first element of the segment
//               g = 1 / U            label 1
//               g = I / ((U - 1) U)  label 0
//             in fp64 from the integers.  dx[index] = fl32(coef_c * g * d weight / dx), coef_c = w_c or w_c / B (per image);
//             the tile's sum of weight * g in fp64 through a fixed tree; lv_finalize_kernel adds the tiles in a fixed order.
// All scratch is the caller's workspace; the launch sequence depends on (n, segments) alone; nothing is read by the host.
#include "common.h"

namespace {

constexpr int LV_THREADS = 256;
constexpr int LV_WAVES = LV_THREADS / 64;
constexpr int LV_ITEMS = 8;                         // keys per thread and pass
constexpr int LV_TILE = LV_THREADS * LV_ITEMS;      // keys per workgroup and pass
constexpr int LV_RADIX = 256;
constexpr int LV_MAX_PASSES = 5;
constexpr int LV_MAX_SEGMENTS = 256;
constexpr long LV_MAX_N = 1L << 30;
constexpr int LV_KEYGEN_MAX_BLOCKS = 2048;
constexpr unsigned LV_IGNORED_KEY = 0xffffffffu;
constexpr unsigned LV_LABEL_BIT = 0x80000000u;
constexpr unsigned LV_INDEX_MASK = 0x3fffffffu;
static_assert(LV_RADIX == LV_THREADS, "a thread per digit");

inline hipStream_t ST(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline bool lv_aligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }

__device__ __forceinline__ float lv_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }      // xbd_step.hip's sigmoidf_

// 0 / 1: the label; 2: the ignored value; 3: no label at all (ignored and counted)
template <class T>
__device__ __forceinline__ int lv_label(T t, int ignore) {
    if (t == (T)0) return 0;
    if (t == (T)1) return 1;
    return (ignore >= 0 && (float)t == (float)ignore) ? 2 : 3;
}

__device__ __forceinline__ float lv_error(float x, int label, int mode) {
    const float t = (float)label;
    if (mode == 0) return 1.f - x * (2.f * t - 1.f);         // the product is exact: one rounding, fused or not
    return fabsf(t - (mode == 2 ? lv_sigmoid(x) : x));
}

__device__ __forceinline__ unsigned lv_key(float e) {
    unsigned u = __float_as_uint(e);
    if ((u << 1) == 0u) u = 0u;                              // -0 sorts as +0
    const unsigned ascending = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    const unsigned k = ~ascending;
    return k == LV_IGNORED_KEY ? LV_IGNORED_KEY - 1u : k;    // (a NaN's bits; outside the contract, kept in range)
}

__device__ __forceinline__ unsigned lv_segment(unsigned index, unsigned HW, unsigned C, int per_image) {
    const unsigned plane = index / HW;
    return per_image ? plane : plane % C;
}

__device__ __forceinline__ unsigned lv_digit(unsigned key, unsigned pay, int pass, unsigned HW, unsigned C, int per_image) {
    if (pass < 4) return (key >> (8 * pass)) & 255u;
    return lv_segment(pay & LV_INDEX_MASK, HW, C, per_image);          // < segments <= 256
}

// inclusive scan of v over the workgroup's 256 threads in thread order; *total = the sum.  `sh`: LV_WAVES + 1 words.
__device__ __forceinline__ unsigned lv_block_scan(unsigned v, unsigned* sh, unsigned* total) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    __syncthreads();                                          // the last call's readers are done with sh
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < LV_WAVES; ++w) {
        const unsigned s = sh[w];
        before += w < wave ? s : 0u;
        all += s;
    }
    *total = all;
    return v + before;
}

// keys and payloads in flat order; totals[5][256] cleared for the histogram launches that follow; bad_partial[block] = the targets
// of this workgroup that are no label at all
template <class T>
__global__ __launch_bounds__(LV_THREADS) void lv_keygen_kernel(const float* __restrict__ x, const T* __restrict__ target, int mode,
                                                              int ignore, long n, unsigned* __restrict__ keys,
                                                              unsigned* __restrict__ pay, unsigned* __restrict__ totals,
                                                              int* __restrict__ bad_partial) {
    __shared__ unsigned sh[LV_WAVES + 1];
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < LV_MAX_PASSES * LV_RADIX; i += LV_THREADS) totals[i] = 0u;
    unsigned bad = 0;
    for (long i = (long)blockIdx.x * LV_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * LV_THREADS) {
        const int lab = lv_label(target[i], ignore);
        unsigned k = LV_IGNORED_KEY, p = (unsigned)i;
        if (lab < 2) {
            k = lv_key(lv_error(x[i], lab, mode));
            p |= lab ? LV_LABEL_BIT : 0u;
        } else if (lab == 3) {
            ++bad;
        }
        keys[i] = k;
        pay[i] = p;
    }
    unsigned total;
    lv_block_scan(bad, sh, &total);
    if (threadIdx.x == 0) bad_partial[blockIdx.x] = (int)total;
}

__global__ __launch_bounds__(LV_THREADS) void lv_hist_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ pay,
                                                            int pass, long n, unsigned HW, unsigned C, int per_image,
                                                            unsigned nblk, unsigned* __restrict__ counts,
                                                            unsigned* __restrict__ totals) {
    __shared__ unsigned h[LV_RADIX];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const long base = (long)blockIdx.x * LV_TILE;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const long i = base + j * LV_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&h[lv_digit(keys[i], pay[i], pass, HW, C, per_image)], 1u);
    }
    __syncthreads();
    const unsigned c = h[threadIdx.x];
    counts[(long)threadIdx.x * nblk + blockIdx.x] = c;
    if (c) atomicAdd(&totals[pass * LV_RADIX + threadIdx.x], c);
}

// counts[d][blk] -> where workgroup blk's first key of digit d goes.  Workgroup d alone walks row d.
__global__ __launch_bounds__(LV_THREADS) void lv_scan_kernel(unsigned* __restrict__ counts, const unsigned* __restrict__ totals,
                                                            int pass, unsigned nblk) {
    __shared__ unsigned sh[LV_WAVES + 1];
    const unsigned d = blockIdx.x;
    unsigned carry;
    lv_block_scan(threadIdx.x < d ? totals[pass * LV_RADIX + threadIdx.x] : 0u, sh, &carry);
    unsigned* row = counts + (long)d * nblk;
    for (unsigned j0 = 0; j0 < nblk; j0 += LV_THREADS) {
        const unsigned j = j0 + threadIdx.x;
        const unsigned c = j < nblk ? row[j] : 0u;
        unsigned total;
        const unsigned incl = lv_block_scan(c, sh, &total);
        if (j < nblk) row[j] = carry + incl - c;
        carry += total;
    }
}

__global__ __launch_bounds__(LV_THREADS) void lv_scatter_kernel(const unsigned* __restrict__ keys_in, const unsigned* __restrict__ pay_in,
                                                               unsigned* __restrict__ keys_out, unsigned* __restrict__ pay_out,
                                                               int pass, long n, unsigned HW, unsigned C, int per_image,
                                                               unsigned nblk, const unsigned* __restrict__ offsets) {
    __shared__ unsigned cnt[LV_WAVES][LV_RADIX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int w = 0; w < LV_WAVES; ++w) cnt[w][threadIdx.x] = 0u;
    __syncthreads();
    // the wave's 512 consecutive keys, 64 a round: rank = keys of the same digit before this one in the wave's part
    const long base = (long)blockIdx.x * LV_TILE + (long)wave * (LV_TILE / LV_WAVES);
    const unsigned long long below_me = (1ull << lane) - 1ull;
    unsigned k[LV_ITEMS], p[LV_ITEMS], rank[LV_ITEMS], dg[LV_ITEMS];
#pragma unroll
    for (int r = 0; r < LV_ITEMS; ++r) {
        const long i = base + r * 64 + lane;
        const bool valid = i < n;
        k[r] = valid ? keys_in[i] : 0u;
        p[r] = valid ? pay_in[i] : 0u;
        const unsigned d = valid ? lv_digit(k[r], p[r], pass, HW, C, per_image) & 255u : 0u;
        dg[r] = d;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const unsigned long long before = same & below_me;
        rank[r] = cnt[wave][d] + (unsigned)__popcll(before);
        __builtin_amdgcn_wave_barrier();
        if (valid && before == 0ull) cnt[wave][d] += (unsigned)__popcll(same);     // the digit's first lane; the row is this wave's own
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {   // thread d: the tile's offset of digit d, then wave after wave
        unsigned off = offsets[(long)threadIdx.x * nblk + blockIdx.x];
#pragma unroll
        for (int w = 0; w < LV_WAVES; ++w) {
            const unsigned c = cnt[w][threadIdx.x];
            cnt[w][threadIdx.x] = off;
            off += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < LV_ITEMS; ++r) {
        const long i = base + r * 64 + lane;
        if (i < n) {
            const unsigned at = cnt[wave][dg[r]] + rank[r];
            if ((long)at < n) {                               // always, when the histogram saw these keys
                keys_out[at] = k[r];
                pay_out[at] = p[r];
            }
        }
    }
}

__global__ __launch_bounds__(LV_THREADS) void lv_order_kernel(const unsigned* __restrict__ pay, long n, int* __restrict__ order) {
    for (long i = (long)blockIdx.x * LV_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * LV_THREADS)
        order[i] = (int)(pay[i] & LV_INDEX_MASK);
}

// ones | valid << 16 of tile t of segment s (a tile holds at most 2048 of either)
__global__ __launch_bounds__(LV_THREADS) void lv_tile_count_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ pay,
                                                                  long L, unsigned tps, unsigned* __restrict__ tile_ones,
                                                                  unsigned* __restrict__ tile_valid) {
    __shared__ unsigned sh[LV_WAVES + 1];
    const unsigned s = blockIdx.x / tps, t = blockIdx.x % tps;
    const long seg0 = (long)s * L, first = (long)t * LV_TILE;
    unsigned v = 0;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const long q = first + j * LV_THREADS + threadIdx.x;
        if (q < L && keys[seg0 + q] != LV_IGNORED_KEY) v += 0x10000u + (pay[seg0 + q] >> 31);
    }
    unsigned total;
    lv_block_scan(v, sh, &total);
    if (threadIdx.x == 0) {
        tile_ones[blockIdx.x] = total & 0xffffu;
        tile_valid[blockIdx.x] = total >> 16;
    }
}

// per segment: the tiles' counts -> exclusive prefixes, in place; seg_ones[s] = G
__global__ __launch_bounds__(LV_THREADS) void lv_seg_scan_kernel(unsigned* __restrict__ tile_ones, unsigned* __restrict__ tile_valid,
                                                                unsigned tps, unsigned* __restrict__ seg_ones) {
    __shared__ unsigned sh[LV_WAVES + 1];
    unsigned* ones = tile_ones + (long)blockIdx.x * tps;
    unsigned* valid = tile_valid + (long)blockIdx.x * tps;
    unsigned carry1 = 0, carryv = 0;
    for (unsigned j0 = 0; j0 < tps; j0 += LV_THREADS) {
        const unsigned j = j0 + threadIdx.x;
        const unsigned a = j < tps ? ones[j] : 0u, b = j < tps ? valid[j] : 0u;
        unsigned ta, tb;
        const unsigned ia = lv_block_scan(a, sh, &ta);
        const unsigned ib = lv_block_scan(b, sh, &tb);
        if (j < tps) {
            ones[j] = carry1 + ia - a;
            valid[j] = carryv + ib - b;
        }
        carry1 += ta;
        carryv += tb;
    }
    if (threadIdx.x == 0) seg_ones[blockIdx.x] = carry1;
}

// the gradient of every element of tile t of segment s, and the tile's sum of weight * g
__global__ __launch_bounds__(LV_THREADS) void lv_grad_kernel(const float* __restrict__ x, const unsigned* __restrict__ keys,
                                                            const unsigned* __restrict__ pay, int mode, int per_image, unsigned B,
                                                            unsigned C, unsigned HW, long n, long L, unsigned tps,
                                                            const unsigned* __restrict__ tile_ones,
                                                            const unsigned* __restrict__ tile_valid,
                                                            const unsigned* __restrict__ seg_ones, const float* __restrict__ seg_weights,
                                                            float* __restrict__ dx, double* __restrict__ loss_partial) {
    __shared__ unsigned sh[LV_WAVES + 1];
    __shared__ unsigned spay[LV_TILE];
    __shared__ unsigned char sval[LV_TILE];
    __shared__ double shd[16];
    const unsigned s = blockIdx.x / tps, t = blockIdx.x % tps;
    const long seg0 = (long)s * L, first = (long)t * LV_TILE;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const int at = j * LV_THREADS + threadIdx.x;
        const long q = first + at;
        spay[at] = q < L ? pay[seg0 + q] : 0u;
        sval[at] = q < L && keys[seg0 + q] != LV_IGNORED_KEY;
    }
    __syncthreads();
    // a thread takes LV_ITEMS consecutive sorted elements
    unsigned mine = 0;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const int at = threadIdx.x * LV_ITEMS + j;
        if (sval[at]) mine += 0x10000u + (spay[at] >> 31);
    }
    unsigned total;
    const unsigned incl = lv_block_scan(mine, sh, &total);
    unsigned c1 = tile_ones[blockIdx.x] + ((incl - mine) & 0xffffu);          // ones before this thread's first element
    unsigned cv = tile_valid[blockIdx.x] + ((incl - mine) >> 16);             // valid elements before it
    const double G = (double)seg_ones[s];
    const unsigned c = per_image ? s % C : s;
    const double coef = (double)(seg_weights ? seg_weights[c] : 1.f) / (per_image ? (double)B : 1.0);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const int at = threadIdx.x * LV_ITEMS + j;
        if (first + at >= L) break;
        const unsigned p = spay[at], index = p & LV_INDEX_MASK;
        if ((long)index >= n) continue;                       // never, when the sort saw these payloads
        float grad = 0.f;
        if (sval[at]) {
            const int label = (int)(p >> 31);
            c1 += (unsigned)label;
            cv += 1u;
            const double I = G - (double)c1, U = G + (double)(cv - c1);
            const double g = cv == 1u ? 1.0 - I / U : label ? 1.0 / U : I / ((U - 1.0) * U);
            const float xi = x[index];
            const float tf = (float)label;
            double weight, slope;                             // the element's weight in the loss and d weight / dx
            if (mode == 0) {
                const float sgn = 2.f * tf - 1.f;
                const float e = 1.f - xi * sgn;
                weight = e > 0.f ? (double)e : 0.0;
                slope = e > 0.f ? -(double)sgn : 0.0;
            } else {
                const float pr = mode == 2 ? lv_sigmoid(xi) : xi;
                const float d = tf - pr;
                weight = (double)fabsf(d);
                slope = d > 0.f ? -1.0 : d < 0.f ? 1.0 : 0.0;
                if (mode == 2) slope *= (double)pr * (1.0 - (double)pr);
            }
            acc += weight * g;
            grad = (float)(coef * g * slope);
        }
        dx[index] = grad;
    }
    const double tile = dh_block_sum_f64(acc, shd);
    if (threadIdx.x == 0) loss_partial[blockIdx.x] = tile;
}

// segment losses (the tiles in order: a strided sum per thread, then the workgroup's tree), channel losses, the weighted sum,
// the bad-label count
__global__ __launch_bounds__(LV_THREADS) void lv_finalize_kernel(const double* __restrict__ loss_partial, unsigned tps, int segments,
                                                                int per_image, int B, int C, const float* __restrict__ seg_weights,
                                                                const int* __restrict__ bad_partial, int nbad,
                                                                float* __restrict__ loss_out, float* __restrict__ channel_loss_out,
                                                                int* __restrict__ bad_out) {
    __shared__ double shd[16];
    __shared__ double seg_loss[LV_MAX_SEGMENTS];
    __shared__ unsigned sh[LV_WAVES + 1];
    for (int s = 0; s < segments; ++s) {
        double a = 0.0;
        for (unsigned j = threadIdx.x; j < tps; j += LV_THREADS) a += loss_partial[(long)s * tps + j];
        const double v = dh_block_sum_f64(a, shd);
        if (threadIdx.x == 0) seg_loss[s] = v;
    }
    unsigned bad = 0;
    for (int j = threadIdx.x; j < nbad; j += LV_THREADS) bad += (unsigned)bad_partial[j];
    unsigned bad_total;
    lv_block_scan(bad, sh, &bad_total);                       // (its barriers also publish seg_loss)
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int c = 0; c < C; ++c) {
            double l = 0.0;
            if (per_image) {
                for (int b = 0; b < B; ++b) l += seg_loss[b * C + c];
                l /= (double)B;
            } else {
                l = seg_loss[c];
            }
            channel_loss_out[c] = (float)l;
            total += (double)(seg_weights ? seg_weights[c] : 1.f) * l;
        }
        *loss_out = (float)total;
        if (bad_out) *bad_out = (int)bad_total;
    }
}

// ---- host side: the workspace's regions and the launch sequence ----
struct LvPlan {
    long n, L;
    int segments, passes, keygen_blocks;
    unsigned nblk, tps;
    long keys[2], pay[2], counts, totals, bad, tile_ones, tile_valid, seg_ones, loss_partial, bytes;
};

inline long lv_up(long v) { return (v + 255) & ~255L; }

inline LvPlan lv_plan(long n, int segments) {
    LvPlan p;
    p.n = n;
    p.segments = segments;
    p.L = n / segments;
    p.passes = segments > 1 ? 5 : 4;
    p.nblk = (unsigned)((n + LV_TILE - 1) / LV_TILE);
    p.tps = (unsigned)((p.L + LV_TILE - 1) / LV_TILE);
    const long kb = (n + LV_THREADS - 1) / LV_THREADS;
    p.keygen_blocks = (int)(kb > LV_KEYGEN_MAX_BLOCKS ? LV_KEYGEN_MAX_BLOCKS : kb);
    long at = 0;
    const auto take = [&at](long bytes) { const long r = at; at += lv_up(bytes); return r; };
    const long tiles = (long)segments * p.tps;
    for (int i = 0; i < 2; ++i) p.keys[i] = take(4 * n);
    for (int i = 0; i < 2; ++i) p.pay[i] = take(4 * n);
    p.counts = take(4L * LV_RADIX * p.nblk);
    p.totals = take(4L * LV_MAX_PASSES * LV_RADIX);
    p.bad = take(4L * LV_KEYGEN_MAX_BLOCKS);
    p.tile_ones = take(4 * tiles);
    p.tile_valid = take(4 * tiles);
    p.seg_ones = take(4L * LV_MAX_SEGMENTS);
    p.loss_partial = take(8 * tiles);
    p.bytes = at;
    return p;
}

struct LvInput {
    const float* x;
    const void* target;
    int target_kind, B, C, mode, per_image, ignore;
    long HW;
};

// what both entries refuse; on success *plan is the call's plan
inline int lv_check(const char* what, const LvInput& in, const void* workspace, long workspace_bytes, LvPlan* plan) {
    DH_REQUIRE(in.x != nullptr && in.target != nullptr, "%s: x and target must be given", what);
    DH_REQUIRE(in.B > 0 && in.C > 0 && in.HW > 0, "%s: empty input (B=%d, C=%d, HW=%ld)", what, in.B, in.C, in.HW);
    DH_REQUIRE(in.target_kind == 0 || in.target_kind == 1, "%s: target_kind=%d is neither 0 (fp32) nor 1 (uint8)", what, in.target_kind);
    DH_REQUIRE(in.mode >= 0 && in.mode <= 2, "%s: mode=%d is not 0 (hinge), 1 (probabilities) or 2 (sigmoid of logits)", what, in.mode);
    DH_REQUIRE(in.per_image == 0 || in.per_image == 1, "%s: per_image=%d is neither 0 nor 1", what, in.per_image);
    DH_REQUIRE(in.ignore >= -1 && in.ignore <= 255, "%s: ignore=%d is neither -1 (none) nor a byte", what, in.ignore);
    DH_REQUIRE(in.HW <= LV_MAX_N && (long)in.B * in.C <= LV_MAX_N && (long)in.B * in.C * in.HW <= LV_MAX_N,
               "%s: n = B * C * HW = %d * %d * %ld is above 2^30", what, in.B, in.C, in.HW);
    const long segments = in.per_image ? (long)in.B * in.C : (long)in.C;
    DH_REQUIRE(segments <= LV_MAX_SEGMENTS, "%s: %ld segments, at most %d are sorted", what, segments, LV_MAX_SEGMENTS);
    DH_REQUIRE(lv_aligned(in.x, 4) && (in.target_kind == 1 || lv_aligned(in.target, 4)), "%s: x or target is not 4-byte aligned", what);
    *plan = lv_plan((long)in.B * in.C * in.HW, (int)segments);
    DH_REQUIRE(workspace != nullptr && lv_aligned(workspace, 16) && workspace_bytes >= plan->bytes,
               "%s: the workspace holds %ld bytes, %ld 16-byte aligned ones are needed", what, workspace_bytes, plan->bytes);
    return 0;
}

template <class T>
inline T* lv_at(void* workspace, long offset) { return reinterpret_cast<T*>(reinterpret_cast<char*>(workspace) + offset); }

// keys and payloads, sorted: returns the index (0 / 1) of the buffers that hold the result, or -1 with the error set
inline int lv_sort(const char* what, const LvInput& in, const LvPlan& P, void* ws, hipStream_t st) {
    unsigned* keys[2] = {lv_at<unsigned>(ws, P.keys[0]), lv_at<unsigned>(ws, P.keys[1])};
    unsigned* pay[2] = {lv_at<unsigned>(ws, P.pay[0]), lv_at<unsigned>(ws, P.pay[1])};
    unsigned* counts = lv_at<unsigned>(ws, P.counts);
    unsigned* totals = lv_at<unsigned>(ws, P.totals);
    int* bad = lv_at<int>(ws, P.bad);
    if (in.target_kind == 0)
        hipLaunchKernelGGL(lv_keygen_kernel<float>, dim3(P.keygen_blocks), dim3(LV_THREADS), 0, st, in.x,
                           reinterpret_cast<const float*>(in.target), in.mode, in.ignore, P.n, keys[0], pay[0], totals, bad);
    else
        hipLaunchKernelGGL(lv_keygen_kernel<unsigned char>, dim3(P.keygen_blocks), dim3(LV_THREADS), 0, st, in.x,
                           reinterpret_cast<const unsigned char*>(in.target), in.mode, in.ignore, P.n, keys[0], pay[0], totals, bad);
    if (hipGetLastError() != hipSuccess) { dh_set_error("xbd_lovasz keygen launch failed"); return -1; }
    int cur = 0;
    const unsigned HW = (unsigned)in.HW, C = (unsigned)in.C;
    for (int pass = 0; pass < P.passes; ++pass) {
        hipLaunchKernelGGL(lv_hist_kernel, dim3(P.nblk), dim3(LV_THREADS), 0, st, keys[cur], pay[cur], pass, P.n, HW, C, in.per_image,
                           P.nblk, counts, totals);
        hipLaunchKernelGGL(lv_scan_kernel, dim3(LV_RADIX), dim3(LV_THREADS), 0, st, counts, totals, pass, P.nblk);
        hipLaunchKernelGGL(lv_scatter_kernel, dim3(P.nblk), dim3(LV_THREADS), 0, st, keys[cur], pay[cur], keys[cur ^ 1], pay[cur ^ 1],
                           pass, P.n, HW, C, in.per_image, P.nblk, counts);
        if (hipGetLastError() != hipSuccess) {
            char b[128];
            snprintf(b, sizeof(b), "%s: a launch of sort pass %d failed", what, pass);
            dh_set_error(b);
            return -1;
        }
        cur ^= 1;
    }
    return cur;
}

}  // namespace

extern "C" int dh_xbd_lovasz_tile(void) { return LV_TILE; }

extern "C" int dh_xbd_lovasz_workspace_size(long n, int segments, long* bytes) {
    DH_REQUIRE(bytes != nullptr, "xbd_lovasz_workspace_size: null size pointer");
    DH_REQUIRE(n > 0 && n <= LV_MAX_N, "xbd_lovasz_workspace_size: n=%ld is outside 1 .. 2^30", n);
    DH_REQUIRE(segments > 0 && segments <= LV_MAX_SEGMENTS && n % segments == 0,
               "xbd_lovasz_workspace_size: %d segments (1 .. %d, dividing n=%ld)", segments, LV_MAX_SEGMENTS, n);
    *bytes = lv_plan(n, segments).bytes;
    return 0;
}

extern "C" int dh_xbd_lovasz_order(const float* x, const void* target, int target_kind, int B, int C, long HW, int mode,
                                   int per_image, int ignore, int* order_out, void* workspace, long workspace_bytes, void* stream) {
    const LvInput in = {x, target, target_kind, B, C, mode, per_image, ignore, HW};
    LvPlan P;
    if (lv_check("xbd_lovasz_order", in, workspace, workspace_bytes, &P) != 0) return 1;
    DH_REQUIRE(order_out != nullptr && lv_aligned(order_out, 4), "xbd_lovasz_order: order_out is null or not 4-byte aligned");
    const int cur = lv_sort("xbd_lovasz_order", in, P, workspace, ST(stream));
    if (cur < 0) return 1;
    hipLaunchKernelGGL(lv_order_kernel, dim3(P.keygen_blocks), dim3(LV_THREADS), 0, ST(stream), lv_at<unsigned>(workspace, P.pay[cur]),
                       P.n, order_out);
    DH_CHECK_LAUNCH("xbd_lovasz_order");
    return 0;
}

extern "C" int dh_xbd_lovasz_fwd(const float* x, const void* target, int target_kind, int B, int C, long HW, int mode, int per_image,
                                 int ignore, const float* seg_weights_dev, float* loss_out, float* channel_loss_out, float* dx_out,
                                 int* bad_out, void* workspace, long workspace_bytes, void* stream) {
    const LvInput in = {x, target, target_kind, B, C, mode, per_image, ignore, HW};
    LvPlan P;
    if (lv_check("xbd_lovasz_fwd", in, workspace, workspace_bytes, &P) != 0) return 1;
    DH_REQUIRE(loss_out != nullptr && channel_loss_out != nullptr && dx_out != nullptr, "xbd_lovasz_fwd: an output is null");
    DH_REQUIRE(lv_aligned(dx_out, 4) && lv_aligned(bad_out, 4), "xbd_lovasz_fwd: dx_out or bad_out is not 4-byte aligned");
    const int cur = lv_sort("xbd_lovasz_fwd", in, P, workspace, ST(stream));
    if (cur < 0) return 1;
    const unsigned* keys = lv_at<unsigned>(workspace, P.keys[cur]);
    const unsigned* pay = lv_at<unsigned>(workspace, P.pay[cur]);
    unsigned* tile_ones = lv_at<unsigned>(workspace, P.tile_ones);
    unsigned* tile_valid = lv_at<unsigned>(workspace, P.tile_valid);
    unsigned* seg_ones = lv_at<unsigned>(workspace, P.seg_ones);
    double* loss_partial = lv_at<double>(workspace, P.loss_partial);
    const unsigned tiles = (unsigned)P.segments * P.tps;
    hipLaunchKernelGGL(lv_tile_count_kernel, dim3(tiles), dim3(LV_THREADS), 0, ST(stream), keys, pay, P.L, P.tps, tile_ones, tile_valid);
    hipLaunchKernelGGL(lv_seg_scan_kernel, dim3(P.segments), dim3(LV_THREADS), 0, ST(stream), tile_ones, tile_valid, P.tps, seg_ones);
    hipLaunchKernelGGL(lv_grad_kernel, dim3(tiles), dim3(LV_THREADS), 0, ST(stream), x, keys, pay, mode, per_image, (unsigned)B,
                       (unsigned)C, (unsigned)HW, P.n, P.L, P.tps, tile_ones, tile_valid, seg_ones, seg_weights_dev, dx_out, loss_partial);
    hipLaunchKernelGGL(lv_finalize_kernel, dim3(1), dim3(LV_THREADS), 0, ST(stream), loss_partial, P.tps, P.segments, per_image, B, C,
                       seg_weights_dev, lv_at<int>(workspace, P.bad), P.keygen_blocks, loss_out, channel_loss_out, bad_out);
    DH_CHECK_LAUNCH("xbd_lovasz_fwd");
    return 0;
}


// ---- jaccard, bce, mask_bceavg (and, for the module's stand-alone classes on probabilities, dice and focal) ----
namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_MAX_BLOCKS = 256;        // workgroups per channel: the finalize launch gives each a thread
constexpr int ST_BWD_MAX_BLOCKS = 2048;
constexpr int ST_NQ = 7;                  // sum s t, sum s, sum t, sum bce, sum mask bce, sum focal, focal's elements
constexpr int ST_TERMS = 5;               // jaccard, bce, mask_bceavg, dice, focal
constexpr int ST_SUMS = 4;                // I, S, T, focal's elements
constexpr float ST_EPS = 1e-6f;           // xBD_code/losses.py:12

struct StWeights { float w[ST_TERMS]; };

template <class T>
__global__ __launch_bounds__(ST_THREADS) void st_fwd_kernel(const float* __restrict__ x, const T* __restrict__ target, int probs,
                                                           long per_channel, int C, long HW, double* __restrict__ partial) {
    __shared__ double sh[ST_THREADS / 64][ST_NQ];
    const int c = blockIdx.y;
    double acc[ST_NQ];
#pragma unroll
    for (int k = 0; k < ST_NQ; ++k) acc[k] = 0.0;
    for (long j = (long)blockIdx.x * ST_THREADS + threadIdx.x; j < per_channel; j += (long)gridDim.x * ST_THREADS) {
        const long b = j / HW, at = (b * C + c) * HW + (j - b * HW);
        const float xi = x[at], t = (float)target[at];
        const float s = probs ? xi : lv_sigmoid(xi);
        acc[0] += (double)s * t;
        acc[1] += s;
        acc[2] += t;
        // StableBCELoss, always of x as a logit: max(x, 0) - x t + log(1 + exp(-|x|))
        acc[3] += (double)(fmaxf(xi, 0.f) - xi * t + logf(1.f + expf(-fabsf(xi))));
        // F.binary_cross_entropy(s, t): each log clamped at -100
        acc[4] += -((double)t * (double)fmaxf(logf(s), -100.f) + (double)(1.f - t) * (double)fmaxf(logf(1.f - s), -100.f));
        // FocalLoss2d (gamma 2): the elements whose target is 255 are left out; combo_partial_kernel's float expressions
        if (t != 255.f) {
            const float o = fminf(fmaxf(s, ST_EPS), 1.f - ST_EPS), tt = fminf(fmaxf(t, ST_EPS), 1.f - ST_EPS);
            const float pt = (1.f - tt) * (1.f - o) + tt * o;
            acc[5] += -(double)((1.f - pt) * (1.f - pt)) * (double)logf(pt);
            acc[6] += 1.0;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < ST_NQ; ++k) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) sh[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < ST_NQ) {
        double t = 0.0;
        for (int w = 0; w < ST_THREADS / 64; ++w) t += sh[w][threadIdx.x];
        partial[((long)c * gridDim.x + blockIdx.x) * ST_NQ + threadIdx.x] = t;
    }
}

// sums [C][4] = I, S, T, focal's elements as floats (what bwd reads); terms [C][5]; *loss = sum_c w_c (weighted terms)
__global__ __launch_bounds__(ST_THREADS) void st_finalize_kernel(const double* __restrict__ partial, int nblk, int C, double count,
                                                                const float* __restrict__ weights, StWeights tw,
                                                                float* __restrict__ sums, float* __restrict__ terms,
                                                                float* __restrict__ loss) {
    __shared__ double shd[16];
    float total = 0.f;
    for (int c = 0; c < C; ++c) {
        double tot[ST_NQ];
        for (int k = 0; k < ST_NQ; ++k) {
            const double a = (int)threadIdx.x < nblk ? partial[((long)c * nblk + threadIdx.x) * ST_NQ + k] : 0.0;
            tot[k] = dh_block_sum_f64(a, shd);
        }
        if (threadIdx.x == 0) {
            const float I = (float)tot[0], S = (float)tot[1], T = (float)tot[2];
            float v[ST_TERMS];
            v[0] = 1.f - (I + ST_EPS) / (S + T - I + ST_EPS);
            v[1] = (float)(tot[3] / count);
            v[2] = (float)(tot[4] / count);
            v[3] = 1.f - (2.f * I + ST_EPS) / (S + T + ST_EPS);
            v[4] = (float)(tot[5] / tot[6]);
            sums[c * ST_SUMS + 0] = I; sums[c * ST_SUMS + 1] = S; sums[c * ST_SUMS + 2] = T; sums[c * ST_SUMS + 3] = (float)tot[6];
            float l = 0.f;
            for (int k = 0; k < ST_TERMS; ++k) {
                terms[c * ST_TERMS + k] = v[k];
                if (tw.w[k] != 0.f) l += tw.w[k] * v[k];      // a term without weight may be NaN (focal of nothing) and stays out
            }
            total += (weights ? weights[c] : 1.f) * l;
        }
    }
    if (threadIdx.x == 0) *loss = total;
}

template <class T>
__global__ __launch_bounds__(ST_THREADS) void st_bwd_kernel(const float* __restrict__ x, const T* __restrict__ target, int probs,
                                                           const float* __restrict__ sums, const float* __restrict__ weights,
                                                           const float* __restrict__ upstream, StWeights tw, float inv_n, long n,
                                                           int C, long HW, float* __restrict__ dx) {
    // in fp64 from x: the gradient is held to the float64 reference more tightly than float32 sigmoids allow
    const double up = upstream ? (double)*upstream : 1.0, eps = (double)ST_EPS;
    // the fp64 sigmoid is taken only where something reads it: bce always does, the other terms when x are logits
    const bool on_s = tw.w[0] != 0.f || tw.w[2] != 0.f || tw.w[3] != 0.f || tw.w[4] != 0.f;
    const bool want_sg = tw.w[1] != 0.f || (!probs && on_s);
    for (long i = (long)blockIdx.x * ST_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * ST_THREADS) {
        const int c = (int)((i / HW) % C);
        const double xi = (double)x[i], t = (double)(float)target[i];
        const double sg = want_sg ? 1.0 / (1.0 + exp(-xi)) : 0.0;
        const double s = probs ? xi : sg, sp = s * (1.0 - s), ds = probs ? 1.0 : sp;
        const double I = (double)sums[c * ST_SUMS + 0], SpT = (double)sums[c * ST_SUMS + 1] + (double)sums[c * ST_SUMS + 2];
        double g = 0.0;
        if (tw.w[0] != 0.f) {
            // J = 1 - (I + eps) / U, U = S + T - I + eps: dJ/ds = -(t U - (I + eps) (1 - t)) / U^2
            const double U = SpT - I + eps;
            g += (double)tw.w[0] * (-(t * U - (I + eps) * (1.0 - t)) / (U * U)) * ds;
        }
        if (tw.w[1] != 0.f) g += (double)tw.w[1] * (sg - t) * (double)inv_n;
        if (tw.w[2] != 0.f) g += (double)tw.w[2] * ((s - t) / fmax(sp, 1e-12)) * ds * (double)inv_n;      // torch's backward: / max(s (1 - s), 1e-12)
        if (tw.w[3] != 0.f) {
            const double U = SpT + eps;                       // combo_bwd_kernel's expression
            g += (double)tw.w[3] * (-(2.0 * t * U - (2.0 * I + eps)) / (U * U)) * ds;
        }
        if (tw.w[4] != 0.f && t != 255.0 && s > eps && s < (double)(1.f - ST_EPS)) {      // clamp passes the gradient strictly inside only
            const double tt = fmin(fmax(t, eps), (double)(1.f - ST_EPS));
            const double pt = (1.0 - tt) * (1.0 - s) + tt * s;
            const double q = 1.0 - pt;
            g += (double)tw.w[4] * (2.0 * q * log(pt) - q * q / pt) * (2.0 * tt - 1.0) / (double)sums[c * ST_SUMS + 3] * ds;
        }
        dx[i] = (float)(up * (double)(weights ? weights[c] : 1.f) * g);
    }
}

inline int st_check(const char* what, const float* x, const void* target, int target_kind, int probs, int B, int C, long HW) {
    DH_REQUIRE(x != nullptr && target != nullptr, "%s: x and target must be given", what);
    DH_REQUIRE(B > 0 && C > 0 && HW > 0, "%s: empty input (B=%d, C=%d, HW=%ld)", what, B, C, HW);
    DH_REQUIRE(C <= 65535, "%s: C=%d is beyond the launch grid (65535)", what, C);
    DH_REQUIRE(target_kind == 0 || target_kind == 1, "%s: target_kind=%d is neither 0 (fp32) nor 1 (uint8)", what, target_kind);
    DH_REQUIRE(probs == 0 || probs == 1, "%s: probs=%d is neither 0 (x are logits) nor 1 (x are probabilities)", what, probs);
    DH_REQUIRE(lv_aligned(x, 4) && (target_kind == 1 || lv_aligned(target, 4)), "%s: x or target is not 4-byte aligned", what);
    return 0;
}

inline long st_workspace_bytes(int C) { return (long)C * ST_MAX_BLOCKS * ST_NQ * (long)sizeof(double); }

}  // namespace

extern "C" int dh_xbd_seg_terms_workspace_size(int C, long* bytes) {
    DH_REQUIRE(bytes != nullptr, "xbd_seg_terms_workspace_size: null size pointer");
    DH_REQUIRE(C > 0 && C <= 65535, "xbd_seg_terms_workspace_size: C=%d is outside 1 .. 65535", C);
    *bytes = st_workspace_bytes(C);
    return 0;
}

extern "C" int dh_xbd_seg_terms_fwd(const float* x, const void* target, int target_kind, int probs, int B, int C, long HW,
                                    const float* chan_weights_dev, float w_jaccard, float w_bce, float w_mask, float w_dice,
                                    float w_focal, float* sums_out, float* terms_out, float* loss_out, void* workspace,
                                    long workspace_bytes, void* stream) {
    if (st_check("xbd_seg_terms_fwd", x, target, target_kind, probs, B, C, HW) != 0) return 1;
    DH_REQUIRE(sums_out != nullptr && terms_out != nullptr && loss_out != nullptr, "xbd_seg_terms_fwd: an output is null");
    DH_REQUIRE(workspace != nullptr && lv_aligned(workspace, 8) && workspace_bytes >= st_workspace_bytes(C),
               "xbd_seg_terms_fwd: the workspace holds %ld bytes, %ld 8-byte aligned ones are needed", workspace_bytes,
               st_workspace_bytes(C));
    const long per_channel = (long)B * HW;
    const long g = (per_channel + ST_THREADS - 1) / ST_THREADS;
    const int grid = (int)(g > ST_MAX_BLOCKS ? ST_MAX_BLOCKS : g);
    const StWeights tw = {{w_jaccard, w_bce, w_mask, w_dice, w_focal}};
    double* partial = reinterpret_cast<double*>(workspace);
    if (target_kind == 0)
        hipLaunchKernelGGL(st_fwd_kernel<float>, dim3(grid, C), dim3(ST_THREADS), 0, ST(stream), x, reinterpret_cast<const float*>(target),
                           probs, per_channel, C, HW, partial);
    else
        hipLaunchKernelGGL(st_fwd_kernel<unsigned char>, dim3(grid, C), dim3(ST_THREADS), 0, ST(stream), x,
                           reinterpret_cast<const unsigned char*>(target), probs, per_channel, C, HW, partial);
    DH_CHECK_LAUNCH("xbd_seg_terms_fwd");
    hipLaunchKernelGGL(st_finalize_kernel, dim3(1), dim3(ST_THREADS), 0, ST(stream), partial, grid, C, (double)per_channel,
                       chan_weights_dev, tw, sums_out, terms_out, loss_out);
    DH_CHECK_LAUNCH("xbd_seg_terms_finalize");
    return 0;
}

extern "C" int dh_xbd_seg_terms_bwd(const float* x, const void* target, int target_kind, int probs, const float* sums,
                                    const float* chan_weights_dev, const float* upstream_dev, float w_jaccard, float w_bce,
                                    float w_mask, float w_dice, float w_focal, int B, int C, long HW, float* dx, void* stream) {
    if (st_check("xbd_seg_terms_bwd", x, target, target_kind, probs, B, C, HW) != 0) return 1;
    DH_REQUIRE(sums != nullptr && dx != nullptr && lv_aligned(dx, 4), "xbd_seg_terms_bwd: sums and dx must be given, dx 4-byte aligned");
    const long n = (long)B * C * HW;
    const long g = (n + ST_THREADS - 1) / ST_THREADS;
    const int grid = (int)(g > ST_BWD_MAX_BLOCKS ? ST_BWD_MAX_BLOCKS : g);
    const float inv_n = 1.f / (float)((double)B * (double)HW);
    const StWeights tw = {{w_jaccard, w_bce, w_mask, w_dice, w_focal}};
    if (target_kind == 0)
        hipLaunchKernelGGL(st_bwd_kernel<float>, dim3(grid), dim3(ST_THREADS), 0, ST(stream), x, reinterpret_cast<const float*>(target),
                           probs, sums, chan_weights_dev, upstream_dev, tw, inv_n, n, C, HW, dx);
    else
        hipLaunchKernelGGL(st_bwd_kernel<unsigned char>, dim3(grid), dim3(ST_THREADS), 0, ST(stream), x,
                           reinterpret_cast<const unsigned char*>(target), probs, sums, chan_weights_dev, upstream_dev, tw, inv_n, n, C,
                           HW, dx);
    DH_CHECK_LAUNCH("xbd_seg_terms_bwd");
    return 0;
}
