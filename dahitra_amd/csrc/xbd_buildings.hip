// Buildings from an xBD class map: connected components, per-component statistics, the vote and the painted map.  All integer.
//   key [N][H][W] uint8 -> labels [N][H][W] int32 (0 background, 1 .. K_n in raster order of each component's first pixel: the
//   numbering of scipy.ndimage.label) and count [N] = K_n; then table [N][cap][10], cls [N][cap], out [N][H][W] (contracts:
//   include/dahitra_hip.h).  Further down: two label maps matched by IoU, match_a [N][cap_a][5] and match_b [N][cap_b].
//
// Labelling is union-find with union-by-minimum-index in SIX launches whose number and grids depend on the shape alone:
//   1 cc_tile_kernel     one workgroup per CC_TH x CC_TW tile, in LDS.  A wave holds one tile row: the horizontal runs come from
//                        one ballot (parent = first pixel of the run), the vertical and diagonal adjacencies are united with
//                        LDS atomicMin, and every pixel's root goes to P as the image's linear index of that pixel (-1: background).
//   2 cc_border_kernel   one thread per pixel on a tile edge: its left / upper neighbours that lie in ANOTHER tile are united in P
//                        with agent-scope atomicMin; every read of P is an agent-scope relaxed atomic load (an XCD's L2 is not
//                        coherent with the others' for plain loads).  Paths are compressed with atomicMin as they are walked.
//   3 cc_flatten_kernel  P[p] = root(p); counts the roots (P[p] == p) of each block of 1024 pixels.
//   4 cc_scan_kernel     one workgroup per image: exclusive scan of the block counts in place, count[n] = their sum.
//   5 cc_rootid_kernel   the r-th root of the image (raster order) gets P[root] = -(r + 1), r = 1 .. K: ballot ranks inside a block
//                        plus the block's scanned base.
//   6 cc_write_kernel    labels[p] = 0 (background), the id of P[p] if p is a root, else the id of P[P[p]].  Writes every label.
// No workgroup waits for another: there is no flag, ticket or spin.  Every loop of find / unite ends by itself: a parent is never
// larger than its child and only ever decreases (atomicMin), and stays inside the component, so a stale read is still an ancestor
// and each step of a walk, and each retry of a unite (whose larger end strictly decreases), moves towards index 0.  The root of a
// component is its minimum index whatever the order of the unions, so every output is the same on every run.
// Workspace (caller's): P [N][H*W] int32, then the block counts [N][ceil(H*W / 1024)] int32; every word that is read is written
// first by the same call, so the sequence needs no memset and replays in a captured graph.
#include "common.h"

namespace {

constexpr int CC_TH = 32, CC_TW = 64;        // the tile of the local pass: a tile row is one wavefront
constexpr int CC_THREADS = 256;
constexpr int CC_BLOCK = 1024;               // pixels per workgroup of the flat passes: 4 per thread, strided by 256
constexpr int CC_COLS = 10;
static_assert(CC_TW == 64 && CC_THREADS % 64 == 0 && (CC_TH * CC_TW) % CC_THREADS == 0, "a tile row is one wavefront");

__device__ __forceinline__ bool adjacent(unsigned a, unsigned b, int keyed) { return a != 0 && b != 0 && (!keyed || a == b); }

// ---- LDS union-find (workgroup scope) ------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(int* par, int x) {
    int q;
    while ((q = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x) x = q;      // q < x
    return x;
}
__device__ __forceinline__ void lds_unite(int* par, int a, int b) {
    a = lds_find(par, a);
    b = lds_find(par, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) break;                  // a was a root and hangs under b now
        a = lds_find(par, old);               // a had a parent already: old < a, max(a, b) decreases every turn
        b = lds_find(par, b);
    }
}

// ---- global union-find on one image's P (agent scope) --------------------------------------------------------------------
__device__ __forceinline__ int ldp(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(int* P, int x) {
    int q;
    while ((q = ldp(P + x)) != x) x = q;
    return x;
}
// find with the walked path hung under the root it found (an ancestor of every node on it, smaller than each)
__device__ __forceinline__ int g_find_compress(int* P, int x) {
    const int r = g_find(P, x);
    int q;
    while (x != r && (q = ldp(P + x)) > r) {
        __hip_atomic_fetch_min(P + x, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = q;
    }
    return r;
}
__device__ __forceinline__ void g_unite(int* P, int a, int b) {
    a = g_find_compress(P, a);
    b = g_find_compress(P, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) break;
        a = g_find(P, old);
        b = g_find(P, b);
    }
}

// grid (tiles of an image, N)
__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const unsigned char* __restrict__ key, int H, int W, int tiles_x,
                                                             int conn8, int keyed, int* __restrict__ P) {
    __shared__ int par[CC_TH * CC_TW];
    __shared__ unsigned char kk[CC_TH * CC_TW];
    const long hw = (long)H * W;
    const unsigned char* kimg = key + (long)blockIdx.y * hw;
    int* Pimg = P + (long)blockIdx.y * hw;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * CC_TH, x0 = tx * CC_TW;
    const int lane = threadIdx.x & 63;
    // rows: the runs of a row from one ballot of their first pixels
    for (int i = threadIdx.x; i < CC_TH * CC_TW; i += CC_THREADS) {
        const int ly = i / CC_TW, lx = i - ly * CC_TW;          // lx == lane
        const int gy = y0 + ly, gx = x0 + lx;
        const unsigned kv = (gy < H && gx < W) ? kimg[(long)gy * W + gx] : 0u;
        const unsigned kl = __shfl_up(kv, 1, 64);
        const bool first = kv != 0 && (lane == 0 || !adjacent(kv, kl, keyed));
        const unsigned long long starts = __ballot(first);
        const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
        kk[i] = (unsigned char)kv;
        par[i] = kv ? ly * CC_TW + (63 - __clzll((long long)(starts & upto))) : i;
    }
    __syncthreads();
    // columns and diagonals
    for (int i = threadIdx.x; i < CC_TH * CC_TW; i += CC_THREADS) {
        const int ly = i / CC_TW, lx = i - ly * CC_TW;
        const unsigned kv = kk[i];
        if (kv == 0 || ly == 0) continue;
        const unsigned ku = kk[i - CC_TW];
        if (adjacent(kv, ku, keyed)) lds_unite(par, i, i - CC_TW);
        if (conn8 && (keyed || ku == 0)) {                      // unkeyed with the upper pixel set: both diagonals join through it
            if (lx > 0 && adjacent(kv, kk[i - CC_TW - 1], keyed)) lds_unite(par, i, i - CC_TW - 1);
            if (lx < CC_TW - 1 && adjacent(kv, kk[i - CC_TW + 1], keyed)) lds_unite(par, i, i - CC_TW + 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CC_TH * CC_TW; i += CC_THREADS) {
        const int ly = i / CC_TW, lx = i - ly * CC_TW;
        const int gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        int v = -1;
        if (kk[i]) {
            const int r = lds_find(par, i);
            const int ry = r / CC_TW;
            v = (y0 + ry) * W + x0 + (r - ry * CC_TW);          // < H * W < 2^31
        }
        Pimg[(long)gy * W + gx] = v;
    }
}

// grid (ceil(H W / 1024), N): the pixels on a tile's first row, first column or last column
__global__ __launch_bounds__(CC_THREADS) void cc_border_kernel(const unsigned char* __restrict__ key, int H, int W, int conn8,
                                                               int keyed, int* P) {
    const long hw = (long)H * W;
    const unsigned char* kimg = key + (long)blockIdx.y * hw;
    int* Pimg = P + (long)blockIdx.y * hw;
#pragma unroll
    for (int j = 0; j < CC_BLOCK / CC_THREADS; ++j) {
        const long p = (long)blockIdx.x * CC_BLOCK + j * CC_THREADS + threadIdx.x;
        if (p >= hw) continue;
        const int y = (int)(p / W), x = (int)(p - (long)y * W);
        const int ly = y % CC_TH, lx = x % CC_TW;
        const bool top = ly == 0 && y > 0, lft = lx == 0 && x > 0, rgt = lx == CC_TW - 1 && x < W - 1;
        if (!(top || lft || (conn8 && rgt && y > 0))) continue;
        const unsigned kv = kimg[p];
        if (kv == 0) continue;
        const unsigned ku = y > 0 ? kimg[p - W] : 0u;
        if (lft && adjacent(kv, kimg[p - 1], keyed)) g_unite(Pimg, (int)p, (int)p - 1);
        if (top && adjacent(kv, ku, keyed)) g_unite(Pimg, (int)p, (int)p - W);
        if (conn8 && y > 0 && (keyed || ku == 0)) {
            if (x > 0 && (top || lft) && adjacent(kv, kimg[p - W - 1], keyed)) g_unite(Pimg, (int)p, (int)p - W - 1);
            if (x < W - 1 && (top || rgt) && adjacent(kv, kimg[p - W + 1], keyed)) g_unite(Pimg, (int)p, (int)p - W + 1);
        }
    }
}

// grid (nblk, N): P[p] = root(p), bc[n][blk] = roots in the block
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int H, int W, int* P, int* __restrict__ bc) {
    __shared__ int wsum[CC_THREADS / 64];
    const long hw = (long)H * W;
    int* Pimg = P + (long)blockIdx.y * hw;
    int roots = 0;
#pragma unroll
    for (int j = 0; j < CC_BLOCK / CC_THREADS; ++j) {
        const long p = (long)blockIdx.x * CC_BLOCK + j * CC_THREADS + threadIdx.x;
        bool root = false;
        if (p < hw) {
            const int q = ldp(Pimg + p);
            if (q == (int)p) root = true;
            else if (q >= 0) {
                const int r = g_find(Pimg, q);
                if (r != q) __hip_atomic_store(Pimg + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        roots += __popcll(__ballot(root));
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = roots;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < CC_THREADS / 64; ++w) t += wsum[w];
        bc[(long)blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
}

// grid (N): bc[n][*] becomes its exclusive prefix sum, count[n] the total
__global__ __launch_bounds__(CC_THREADS) void cc_scan_kernel(int* __restrict__ bc, int nblk, int* __restrict__ count) {
    __shared__ int wsum[CC_THREADS / 64];
    int* b = bc + (long)blockIdx.x * nblk;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nblk; base += CC_THREADS) {
        const int i = base + threadIdx.x;
        const int v = i < nblk ? b[i] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int off = 0, tot = 0;
        for (int k = 0; k < CC_THREADS / 64; ++k) {
            if (k < w) off += wsum[k];
            tot += wsum[k];
        }
        if (i < nblk) b[i] = carry + off + inc - v;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) count[blockIdx.x] = carry;
}

// grid (nblk, N): P[root] = -(id + 1), id = 1 .. K in raster order
__global__ __launch_bounds__(CC_THREADS) void cc_rootid_kernel(int H, int W, int* __restrict__ P, const int* __restrict__ bc) {
    constexpr int NJ = CC_BLOCK / CC_THREADS, NW = CC_THREADS / 64;
    __shared__ int wsum[NJ * NW];
    const long hw = (long)H * W;
    int* Pimg = P + (long)blockIdx.y * hw;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    bool root[NJ];
    int rank[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const long p = (long)blockIdx.x * CC_BLOCK + j * CC_THREADS + threadIdx.x;
        root[j] = p < hw && Pimg[p] == (int)p;
        const unsigned long long m = __ballot(root[j]);
        rank[j] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[j * NW + w] = __popcll(m);
    }
    __syncthreads();
    const int base = bc[(long)blockIdx.y * gridDim.x + blockIdx.x];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (!root[j]) continue;
        int off = 0;
        for (int k = 0; k < j * NW + w; ++k) off += wsum[k];
        const long p = (long)blockIdx.x * CC_BLOCK + j * CC_THREADS + threadIdx.x;
        Pimg[p] = -(base + off + rank[j] + 1 + 1);
    }
}

// grid (nblk, N)
__global__ __launch_bounds__(CC_THREADS) void cc_write_kernel(int H, int W, const int* __restrict__ P, int* __restrict__ labels) {
    const long hw = (long)H * W;
    const int* Pimg = P + (long)blockIdx.y * hw;
    int* L = labels + (long)blockIdx.y * hw;
#pragma unroll
    for (int j = 0; j < CC_BLOCK / CC_THREADS; ++j) {
        const long p = (long)blockIdx.x * CC_BLOCK + j * CC_THREADS + threadIdx.x;
        if (p >= hw) continue;
        int v = Pimg[p];
        if (v >= 0) v = Pimg[v];               // a flattened pixel points at its root, which holds -(id + 1)
        L[p] = v == -1 ? 0 : -v - 1;
    }
}

// ---- statistics ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_THREADS) void cc_table_init_kernel(int* __restrict__ table, long rows, int H, int W) {
    const long i = (long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= rows * CC_COLS) return;
    const int c = (int)(i % CC_COLS);
    table[i] = c < 6 ? 0 : c == 6 ? H : c == 7 ? W : -1;
}

// One partial row of the table: area, h0 .. h4 and the box of some pixels of one label
struct StatsPart {
    int area, h[5], ya, xa, yb, xb;
};
constexpr int CC_SLOTS = 128;                 // labels a workgroup gathers in LDS before it touches the table

__device__ __forceinline__ void part_to_global(int* row, const StatsPart& s) {
    if (s.area) __hip_atomic_fetch_add(row, s.area, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int k = 0; k < 5; ++k)
        if (s.h[k]) __hip_atomic_fetch_add(row + 1 + k, s.h[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(row + 6, s.ya, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(row + 7, s.xa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(row + 8, s.yb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(row + 9, s.xb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void part_to_lds(int* row, const StatsPart& s) {
    atomicAdd(row, s.area);
#pragma unroll
    for (int k = 0; k < 5; ++k)
        if (s.h[k]) atomicAdd(row + 1 + k, s.h[k]);
    atomicMin(row + 6, s.ya);
    atomicMin(row + 7, s.xa);
    atomicMax(row + 8, s.yb);
    atomicMax(row + 9, s.xb);
}

// grid (tiles of an image, N), the tiles of cc_tile_kernel.  A wave holds 64 consecutive pixels of ONE image row.  For every
// distinct label among them (a loop of at most 64 turns, one per label, the same for all lanes) ballots give the area and the
// class counts, and the first and last lane of the label its columns: one partial row per wave and label, no shuffle reduction.
// The lane that leads the label adds the partial row to the workgroup's LDS slot of that label (claimed with ONE compare-and-swap,
// never retried: a slot taken by another label sends the partial row straight to the table), and the slots go to the table with
// integer atomics at the end: a building that fills the tile costs ten global atomics per tile, not per pixel.
__global__ __launch_bounds__(CC_THREADS) void cc_stats_kernel(const int* __restrict__ labels, const unsigned char* __restrict__ vote,
                                                              int H, int W, int tiles_x, int cap, int* table) {
    __shared__ int tag[CC_SLOTS];
    __shared__ int acc[CC_SLOTS][CC_COLS];
    const long hw = (long)H * W;
    const int* L = labels + (long)blockIdx.y * hw;
    const unsigned char* V = vote + (long)blockIdx.y * hw;
    int* T = table + (long)blockIdx.y * cap * CC_COLS;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * CC_TH, x0 = tx * CC_TW;
    const int lane = threadIdx.x & 63;
    for (int s = threadIdx.x; s < CC_SLOTS; s += CC_THREADS) {
        tag[s] = 0;
#pragma unroll
        for (int c = 0; c < CC_COLS; ++c) acc[s][c] = c < 6 ? 0 : c < 8 ? 0x7fffffff : -1;
    }
    __syncthreads();
#pragma unroll 1
    for (int i = threadIdx.x; i < CC_TH * CC_TW; i += CC_THREADS) {
        const int y = y0 + i / CC_TW, x = x0 + lane;            // i % CC_TW == lane
        const bool in = y < H && x < W;
        int l = in ? L[(long)y * W + x] : 0;
        if (l < 0 || l > cap) l = 0;
        const unsigned v = l ? V[(long)y * W + x] : 255u;
        unsigned long long rest = __ballot(l > 0);
        while (rest) {                                          // one turn per distinct label; `rest` is the same in every lane
            const int leader = __ffsll((long long)rest) - 1;
            const int lead = __shfl(l, leader, 64);
            const bool mine = l == lead;
            const unsigned long long mm = __ballot(mine);
            StatsPart s;
            s.area = __popcll(mm);
#pragma unroll
            for (int k = 0; k < 5; ++k) s.h[k] = __popcll(__ballot(mine && v == (unsigned)k));
            s.ya = s.yb = y;
            s.xa = x0 + leader;                                 // the lanes of a label: first = leader, last = the top bit
            s.xb = x0 + 63 - __clzll((long long)mm);
            if (lane == leader) {
                const int slot = lead & (CC_SLOTS - 1);
                const int old = atomicCAS(&tag[slot], 0, lead);
                if (old == 0 || old == lead) part_to_lds(acc[slot], s);
                else part_to_global(T + (long)(lead - 1) * CC_COLS, s);
            }
            rest &= ~mm;
        }
    }
    __syncthreads();
    for (int sl = threadIdx.x; sl < CC_SLOTS; sl += CC_THREADS) {
        const int lab = tag[sl];
        if (lab == 0) continue;
        StatsPart s;
        s.area = acc[sl][0];
#pragma unroll
        for (int k = 0; k < 5; ++k) s.h[k] = acc[sl][1 + k];
        s.ya = acc[sl][6]; s.xa = acc[sl][7]; s.yb = acc[sl][8]; s.xb = acc[sl][9];
        part_to_global(T + (long)(lab - 1) * CC_COLS, s);
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_vote_kernel(const int* __restrict__ table, long rows, int min_area, int mode,
                                                             unsigned char* __restrict__ cls) {
    const long i = (long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= rows) return;
    const int* r = table + i * CC_COLS;
    const int area = r[0];
    int c = 0;
    if (area > 0 && area >= min_area) {
        if (mode == 0) {
            int best = r[2];
            c = 1;
            for (int k = 2; k <= 4; ++k)
                if (r[1 + k] > best) { best = r[1 + k]; c = k; }        // strict: the first maximum keeps its place
            if (best == 0) c = 0;
        } else {
            int best = r[1];
            for (int k = 1; k <= 4; ++k)
                if (r[1 + k] > best) { best = r[1 + k]; c = k; }
        }
    }
    cls[i] = (unsigned char)c;
}

// grid (nblk, N)
__global__ __launch_bounds__(CC_THREADS) void cc_paint_kernel(const int* __restrict__ labels, const unsigned char* __restrict__ cls,
                                                              int H, int W, int cap, unsigned char* __restrict__ out) {
    const long hw = (long)H * W;
    const int* L = labels + (long)blockIdx.y * hw;
    const unsigned char* C = cls + (long)blockIdx.y * cap;
    unsigned char* O = out + (long)blockIdx.y * hw;
#pragma unroll
    for (int j = 0; j < CC_BLOCK / CC_THREADS; ++j) {
        const long p = (long)blockIdx.x * CC_BLOCK + j * CC_THREADS + threadIdx.x;
        if (p >= hw) continue;
        const int l = L[p];
        O[p] = (l >= 1 && l <= cap) ? C[l - 1] : (unsigned char)0;
    }
}

// ---- matching two label maps -----------------------------------------------------------------------------------------------
// A [N][H][W] (labels 1 .. cap_a) against B (1 .. cap_b): for every label a the label of B that covers more than half of it, and
// whether the two match above an IoU of num / den.  No table of pairs: with NB = bit_length(cap_b), a row of NB + 1 counters per
// label a (its area, and for every bit k the pixels of a whose B label has bit k set) names the ONLY label that can cover more
// than half of a -- each of its set bits is counted more than area / 2 times, each of its clear bits fewer -- and a second pass
// counts the pixels of a that carry that candidate, which is what decides.  Five launches, grids fixed by the shapes:
//   1 match_init_kernel    zeroes the workspace and match_b
//   2 match_count_kernel   the pixels, once: rows [area, ones_0 .. ones_NB-1] of A and the areas of B
//   3 match_cand_kernel    cand(a) = OR_k (2 ones_k > area) << k
//   4 match_verify_kernel  the pixels again: inter(a) = pixels with A == a, B == cand(a)
//   5 match_decide_kernel  the five columns of match_a, and match_b[match - 1] = a (one writer: the match is one-to-one)
// The two pixel passes have the tile and wave shape of cc_stats_kernel, and its LDS slots.
// Workspace, int32: rows [N][cap_a][NB + 1], area_b [N][cap_b], cand [N][cap_a], inter [N][cap_a].
constexpr int MATCH_COLS = 5;
constexpr int MATCH_MAX_BITS = 25;            // bit_length(CC_MAX_CAP)
constexpr int MATCH_ROW = MATCH_MAX_BITS + 1;
static_assert(MATCH_ROW <= 32, "the count pass flushes a slot with 32 lanes");

__host__ __device__ inline int match_bits(int cap_b) {
    int nb = 0;
    while (nb < 31 && (cap_b >> nb)) ++nb;
    return nb;
}
__host__ __device__ inline long match_ws_words(long N, long cap_a, long cap_b) {
    return N * (cap_a * (match_bits((int)cap_b) + 3) + cap_b);
}

__global__ __launch_bounds__(CC_THREADS) void match_init_kernel(int* __restrict__ ws, long ws_words, int* __restrict__ match_b,
                                                                long b_words) {
    const long i = (long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i < ws_words) ws[i] = 0;
    else if (i - ws_words < b_words) match_b[i - ws_words] = 0;
}

// grid (tiles of an image, N).  A wave holds 64 consecutive pixels of one image row.  Once per row, lane k + 1 takes the ballot of
// bit k of the 64 B labels and lane 0 all ones.  Then one turn per distinct label of A among the pixels: the ballot of the
// label's lanes, ANDed with what a lane holds and counted, is the area in lane 0 and ones_k in lane k + 1, so a turn costs one
// popcount whatever NB is, and the NB + 1 counters of the partial row go to the LDS slot (or, when the slot is another label's,
// straight to the table) in ONE atomic instruction of NB + 1 lanes.  Then one turn per distinct label of B for its area,
// through a second slot array.
__global__ __launch_bounds__(CC_THREADS) void match_count_kernel(const int* __restrict__ la, const int* __restrict__ lb, int H, int W,
                                                                 int tiles_x, int cap_a, int cap_b, int nb, int* rows, int* area_b) {
    __shared__ int tag_a[CC_SLOTS], tag_b[CC_SLOTS];
    __shared__ int acc_a[CC_SLOTS][MATCH_ROW];
    __shared__ int acc_b[CC_SLOTS];
    const long hw = (long)H * W;
    const int* A = la + (long)blockIdx.y * hw;
    const int* B = lb + (long)blockIdx.y * hw;
    const int rw = nb + 1;
    int* R = rows + (long)blockIdx.y * cap_a * rw;
    int* AB = area_b + (long)blockIdx.y * cap_b;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * CC_TH, x0 = tx * CC_TW;
    const int lane = threadIdx.x & 63;
    for (int s = threadIdx.x; s < CC_SLOTS; s += CC_THREADS) tag_a[s] = tag_b[s] = acc_b[s] = 0;
    for (int j = threadIdx.x; j < CC_SLOTS * MATCH_ROW; j += CC_THREADS) (&acc_a[0][0])[j] = 0;
    __syncthreads();
#pragma unroll 1
    for (int i = threadIdx.x; i < CC_TH * CC_TW; i += CC_THREADS) {
        const int y = y0 + i / CC_TW, x = x0 + lane;            // i % CC_TW == lane
        const bool in = y < H && x < W;
        int a = in ? A[(long)y * W + x] : 0;
        int b = in ? B[(long)y * W + x] : 0;
        if (a < 0 || a > cap_a) a = 0;
        if (b < 0 || b > cap_b) b = 0;
        unsigned long long rest = __ballot(a > 0);
        unsigned long long bits = lane == 0 ? ~0ull : 0ull;     // lane k + 1: the lanes whose B label has bit k set
        if (rest) {
#pragma unroll 1
            for (int k = 0; k < nb; ++k) {
                const unsigned long long bk = __ballot((b >> k) & 1);
                if (lane == k + 1) bits = bk;
            }
        }
        while (rest) {                                          // one turn per distinct label of A; `rest` is the same in every lane
            const int leader = __ffsll((long long)rest) - 1;
            const int lead = __shfl(a, leader, 64);
            const unsigned long long mm = __ballot(a == lead);
            const int val = __popcll(bits & mm);
            const int slot = lead & (CC_SLOTS - 1);
            int old = 0;
            if (lane == leader) old = atomicCAS(&tag_a[slot], 0, lead);
            old = __shfl(old, leader, 64);
            if (lane < rw && val) {
                if (old == 0 || old == lead) atomicAdd(&acc_a[slot][lane], val);
                else __hip_atomic_fetch_add(R + (long)(lead - 1) * rw + lane, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            rest &= ~mm;
        }
        rest = __ballot(b > 0);
        while (rest) {                                          // and per distinct label of B
            const int leader = __ffsll((long long)rest) - 1;
            const int lead = __shfl(b, leader, 64);
            const unsigned long long mm = __ballot(b == lead);
            if (lane == leader) {
                const int slot = lead & (CC_SLOTS - 1);
                const int old = atomicCAS(&tag_b[slot], 0, lead);
                if (old == 0 || old == lead) atomicAdd(&acc_b[slot], __popcll(mm));
                else __hip_atomic_fetch_add(AB + (lead - 1), __popcll(mm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            rest &= ~mm;
        }
    }
    __syncthreads();
    for (int sl = threadIdx.x >> 5; sl < CC_SLOTS; sl += CC_THREADS >> 5) {         // 32 lanes per slot: MATCH_ROW <= 32
        const int c = threadIdx.x & 31;
        const int lab = tag_a[sl], v = c < rw ? acc_a[sl][c] : 0;
        if (lab && v) __hip_atomic_fetch_add(R + (long)(lab - 1) * rw + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int sl = threadIdx.x; sl < CC_SLOTS; sl += CC_THREADS)
        if (tag_b[sl]) __hip_atomic_fetch_add(AB + (tag_b[sl] - 1), acc_b[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread per row of A, all images
__global__ __launch_bounds__(CC_THREADS) void match_cand_kernel(const int* __restrict__ rows, long nrows, int nb, int* __restrict__ cand) {
    const long i = (long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= nrows) return;
    const int* r = rows + i * (nb + 1);
    const long area = r[0];
    int c = 0;
    for (int k = 0; k < nb; ++k) c |= (2L * r[1 + k] > area) << k;
    cand[i] = c;                                                // may exceed cap_b, or name a label that merely touches: verified next
}

// grid (tiles of an image, N): inter[a - 1] += the pixels with A == a and B == cand(a), B a label of 1 .. cap_b
__global__ __launch_bounds__(CC_THREADS) void match_verify_kernel(const int* __restrict__ la, const int* __restrict__ lb, int H, int W,
                                                                  int tiles_x, int cap_a, int cap_b, const int* __restrict__ cand,
                                                                  int* inter) {
    __shared__ int tag[CC_SLOTS], acc[CC_SLOTS];
    const long hw = (long)H * W;
    const int* A = la + (long)blockIdx.y * hw;
    const int* B = lb + (long)blockIdx.y * hw;
    const int* C = cand + (long)blockIdx.y * cap_a;
    int* I = inter + (long)blockIdx.y * cap_a;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * CC_TH, x0 = tx * CC_TW;
    const int lane = threadIdx.x & 63;
    for (int s = threadIdx.x; s < CC_SLOTS; s += CC_THREADS) tag[s] = acc[s] = 0;
    __syncthreads();
#pragma unroll 1
    for (int i = threadIdx.x; i < CC_TH * CC_TW; i += CC_THREADS) {
        const int y = y0 + i / CC_TW, x = x0 + lane;
        const bool in = y < H && x < W;
        int a = in ? A[(long)y * W + x] : 0;
        const int b = in ? B[(long)y * W + x] : 0;
        if (a < 0 || a > cap_a) a = 0;
        const bool hit = a > 0 && b >= 1 && b <= cap_b && b == C[a - 1];
        unsigned long long rest = __ballot(hit);
        while (rest) {
            const int leader = __ffsll((long long)rest) - 1;
            const int lead = __shfl(a, leader, 64);
            const unsigned long long mm = __ballot(hit && a == lead);
            if (lane == leader) {
                const int slot = lead & (CC_SLOTS - 1);
                const int old = atomicCAS(&tag[slot], 0, lead);
                if (old == 0 || old == lead) atomicAdd(&acc[slot], __popcll(mm));
                else __hip_atomic_fetch_add(I + (lead - 1), __popcll(mm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            rest &= ~mm;
        }
    }
    __syncthreads();
    for (int sl = threadIdx.x; sl < CC_SLOTS; sl += CC_THREADS)
        if (tag[sl]) __hip_atomic_fetch_add(I + (tag[sl] - 1), acc[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (ceil(cap_a / 256), N): one thread per row of A
__global__ __launch_bounds__(CC_THREADS) void match_decide_kernel(const int* __restrict__ rows, const int* __restrict__ area_b,
                                                                  const int* __restrict__ cand, const int* __restrict__ inter,
                                                                  int cap_a, int cap_b, int nb, int num, int den,
                                                                  int* __restrict__ match_a, int* __restrict__ match_b) {
    const int i = blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= cap_a) return;
    const long row = (long)blockIdx.y * cap_a + i;
    const int area = rows[row * (nb + 1)];
    int it = inter[row];
    int maj = 2L * it > area ? cand[row] : 0;                   // a verified candidate is a label of 1 .. cap_b
    int maj_area = 0;
    if (maj) maj_area = area_b[(long)blockIdx.y * cap_b + maj - 1];
    else it = 0;
    const int match = (long)it * den > (long)num * ((long)area + maj_area - it) ? maj : 0;
    int* o = match_a + row * MATCH_COLS;
    o[0] = area; o[1] = maj; o[2] = it; o[3] = maj_area; o[4] = match;
    if (match) match_b[(long)blockIdx.y * cap_b + match - 1] = i + 1;
}

bool aligned4(const void* p) { return (reinterpret_cast<size_t>(p) & 3) == 0; }
long blocks_of(int H, int W) { return ((long)H * W + CC_BLOCK - 1) / CC_BLOCK; }
constexpr int CC_MAX_CAP = 1 << 24;
static_assert(MATCH_MAX_BITS == 25 && (CC_MAX_CAP >> 24) == 1 && (CC_MAX_CAP >> 25) == 0, "a row of the count pass holds every bit of a label");

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define CC_REQUIRE_SHAPE(what)                                                                                                   \
    DH_REQUIRE(N >= 1, what ": N=%d: an empty batch", N);                                                                        \
    DH_REQUIRE(N <= 65535, what ": N=%d: at most 65535 images per call", N);                                                     \
    DH_REQUIRE(H >= 1 && W >= 1, what ": empty image %dx%d", H, W);                                                              \
    DH_REQUIRE((long)H * W <= 0x7fffffffL, what ": %dx%d: an image holds fewer than 2^31 pixels", H, W)
#define CC_REQUIRE_CAP(what)                                                                                                     \
    DH_REQUIRE(cap >= 1 && cap <= CC_MAX_CAP, what ": cap=%d: 1 .. %d table rows per image", cap, CC_MAX_CAP);                  \
    DH_REQUIRE((long)N * cap <= (1L << 28), what ": N * cap = %ld: at most 2^28 table rows per call", (long)N * cap)

extern "C" int dh_xbd_cc_tile_h(void) { return CC_TH; }
extern "C" int dh_xbd_cc_tile_w(void) { return CC_TW; }

static long cc_ws_bytes(int N, int H, int W) { return 4L * N * ((long)H * W + blocks_of(H, W)); }

extern "C" int dh_xbd_cc_ws_bytes(int N, int H, int W, long* bytes) {
    DH_REQUIRE(bytes, "xbd_cc_ws_bytes: null pointer");
    CC_REQUIRE_SHAPE("xbd_cc_ws_bytes");
    *bytes = cc_ws_bytes(N, H, W);
    return 0;
}

extern "C" int dh_xbd_cc_label(const unsigned char* key, int N, int H, int W, int conn, int keyed, int* labels, int* count,
                               void* ws, long ws_bytes, void* stream) {
    DH_REQUIRE(key && labels && count && ws, "xbd_cc_label: null pointer");
    CC_REQUIRE_SHAPE("xbd_cc_label");
    DH_REQUIRE(conn == 4 || conn == 8, "xbd_cc_label: connectivity %d is neither 4 nor 8", conn);
    DH_REQUIRE(keyed == 0 || keyed == 1, "xbd_cc_label: keyed=%d is neither 0 nor 1", keyed);
    DH_REQUIRE(aligned4(labels) && aligned4(count) && aligned4(ws), "xbd_cc_label: labels, count and the workspace hold int32");
    DH_REQUIRE(ws_bytes >= cc_ws_bytes(N, H, W), "xbd_cc_label: a workspace of %ld bytes, %ld are needed", ws_bytes,
               cc_ws_bytes(N, H, W));
    const int nblk = (int)blocks_of(H, W);
    const int tiles_x = dh_cdiv(W, CC_TW), tiles_y = dh_cdiv(H, CC_TH);
    int* P = reinterpret_cast<int*>(ws);
    int* bc = P + (long)N * H * W;
    const dim3 flat(nblk, N), thr(CC_THREADS);
    hipLaunchKernelGGL(cc_tile_kernel, dim3(tiles_x * tiles_y, N), thr, 0, ST(stream), key, H, W, tiles_x, conn == 8, keyed, P);
    hipLaunchKernelGGL(cc_border_kernel, flat, thr, 0, ST(stream), key, H, W, conn == 8, keyed, P);
    hipLaunchKernelGGL(cc_flatten_kernel, flat, thr, 0, ST(stream), H, W, P, bc);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(N), thr, 0, ST(stream), bc, nblk, count);
    hipLaunchKernelGGL(cc_rootid_kernel, flat, thr, 0, ST(stream), H, W, P, bc);
    hipLaunchKernelGGL(cc_write_kernel, flat, thr, 0, ST(stream), H, W, P, labels);
    DH_CHECK_LAUNCH("xbd_cc_label");
    return 0;
}

extern "C" int dh_xbd_cc_stats(const int* labels, const unsigned char* vote, int N, int H, int W, int cap, int* table,
                               void* stream) {
    DH_REQUIRE(labels && vote && table, "xbd_cc_stats: null pointer");
    CC_REQUIRE_SHAPE("xbd_cc_stats");
    CC_REQUIRE_CAP("xbd_cc_stats");
    DH_REQUIRE(aligned4(labels) && aligned4(table), "xbd_cc_stats: labels and table hold int32");
    const long rows = (long)N * cap;
    hipLaunchKernelGGL(cc_table_init_kernel, dim3(dh_cdiv(rows * CC_COLS, CC_THREADS)), dim3(CC_THREADS), 0, ST(stream), table, rows,
                       H, W);
    const int tiles_x = dh_cdiv(W, CC_TW), tiles_y = dh_cdiv(H, CC_TH);
    hipLaunchKernelGGL(cc_stats_kernel, dim3(tiles_x * tiles_y, N), dim3(CC_THREADS), 0, ST(stream), labels, vote, H, W, tiles_x,
                       cap, table);
    DH_CHECK_LAUNCH("xbd_cc_stats");
    return 0;
}

extern "C" int dh_xbd_cc_vote(const int* table, int N, int cap, int min_area, int mode, unsigned char* cls, void* stream) {
    DH_REQUIRE(table && cls, "xbd_cc_vote: null pointer");
    DH_REQUIRE(N >= 1 && N <= 65535, "xbd_cc_vote: N=%d: 1 .. 65535 images", N);
    CC_REQUIRE_CAP("xbd_cc_vote");
    DH_REQUIRE(min_area >= 0, "xbd_cc_vote: min_area=%d is negative", min_area);
    DH_REQUIRE(mode == 0 || mode == 1, "xbd_cc_vote: mode %d is neither 0 (damage) nor 1 (all)", mode);
    DH_REQUIRE(aligned4(table), "xbd_cc_vote: table holds int32");
    const long rows = (long)N * cap;
    hipLaunchKernelGGL(cc_vote_kernel, dim3(dh_cdiv(rows, CC_THREADS)), dim3(CC_THREADS), 0, ST(stream), table, rows, min_area, mode,
                       cls);
    DH_CHECK_LAUNCH("xbd_cc_vote");
    return 0;
}

extern "C" int dh_xbd_cc_paint(const int* labels, const unsigned char* cls, int N, int H, int W, int cap, unsigned char* out,
                               void* stream) {
    DH_REQUIRE(labels && cls && out, "xbd_cc_paint: null pointer");
    CC_REQUIRE_SHAPE("xbd_cc_paint");
    CC_REQUIRE_CAP("xbd_cc_paint");
    DH_REQUIRE(aligned4(labels), "xbd_cc_paint: labels hold int32");
    hipLaunchKernelGGL(cc_paint_kernel, dim3((int)blocks_of(H, W), N), dim3(CC_THREADS), 0, ST(stream), labels, cls, H, W, cap, out);
    DH_CHECK_LAUNCH("xbd_cc_paint");
    return 0;
}

extern "C" int dh_xbd_cc_match_ws_bytes(int N, int cap_a, int cap_b, long* bytes) {
    DH_REQUIRE(bytes, "xbd_cc_match_ws_bytes: null pointer");
    DH_REQUIRE(N >= 1 && N <= 65535, "xbd_cc_match_ws_bytes: N=%d: 1 .. 65535 images", N);
    {
        const int cap = cap_a;
        CC_REQUIRE_CAP("xbd_cc_match_ws_bytes");
    }
    {
        const int cap = cap_b;
        CC_REQUIRE_CAP("xbd_cc_match_ws_bytes");
    }
    *bytes = 4L * match_ws_words(N, cap_a, cap_b);
    return 0;
}

extern "C" int dh_xbd_cc_match(const int* labels_a, const int* labels_b, int N, int H, int W, int cap_a, int cap_b, int iou_num,
                               int iou_den, int* match_a, int* match_b, void* ws, long ws_bytes, void* stream) {
    DH_REQUIRE(labels_a && labels_b && match_a && match_b && ws, "xbd_cc_match: null pointer");
    CC_REQUIRE_SHAPE("xbd_cc_match");
    {
        const int cap = cap_a;
        CC_REQUIRE_CAP("xbd_cc_match");
    }
    {
        const int cap = cap_b;
        CC_REQUIRE_CAP("xbd_cc_match");
    }
    DH_REQUIRE(iou_num >= 1 && iou_num <= iou_den && iou_den <= 32768 && 2L * iou_num >= iou_den,
               "xbd_cc_match: iou %d / %d: 1 <= num <= den <= 32768 and num / den >= 1 / 2", iou_num, iou_den);
    DH_REQUIRE(aligned4(labels_a) && aligned4(labels_b) && aligned4(match_a) && aligned4(match_b) && aligned4(ws),
               "xbd_cc_match: both label maps, match_a, match_b and the workspace hold int32");
    const long words = match_ws_words(N, cap_a, cap_b);
    DH_REQUIRE(ws_bytes >= 4 * words, "xbd_cc_match: a workspace of %ld bytes, %ld are needed", ws_bytes, 4 * words);
    const int nb = match_bits(cap_b);
    const long nrows = (long)N * cap_a, b_words = (long)N * cap_b;
    int* rows = reinterpret_cast<int*>(ws);
    int* area_b = rows + nrows * (nb + 1);
    int* cand = area_b + b_words;
    int* inter = cand + nrows;
    const int tiles_x = dh_cdiv(W, CC_TW), tiles_y = dh_cdiv(H, CC_TH);
    const dim3 tiles(tiles_x * tiles_y, N), thr(CC_THREADS);
    hipLaunchKernelGGL(match_init_kernel, dim3(dh_cdiv(words + b_words, CC_THREADS)), thr, 0, ST(stream), rows, words, match_b, b_words);
    hipLaunchKernelGGL(match_count_kernel, tiles, thr, 0, ST(stream), labels_a, labels_b, H, W, tiles_x, cap_a, cap_b, nb, rows, area_b);
    hipLaunchKernelGGL(match_cand_kernel, dim3(dh_cdiv(nrows, CC_THREADS)), thr, 0, ST(stream), rows, nrows, nb, cand);
    hipLaunchKernelGGL(match_verify_kernel, tiles, thr, 0, ST(stream), labels_a, labels_b, H, W, tiles_x, cap_a, cap_b, cand, inter);
    hipLaunchKernelGGL(match_decide_kernel, dim3(dh_cdiv(cap_a, CC_THREADS), N), thr, 0, ST(stream), rows, area_b, cand, inter, cap_a,
                       cap_b, nb, iou_num, iou_den, match_a, match_b);
    DH_CHECK_LAUNCH("xbd_cc_match");
    return 0;
}
