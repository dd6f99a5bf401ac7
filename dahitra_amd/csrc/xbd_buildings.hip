// Buildings from an xBD class map: connected components, per-component statistics, the vote and the painted map.  All integer.
//   key [N][H][W] uint8 -> labels [N][H][W] int32 (0 background, 1 .. K_n in raster order of each component's first pixel: the
//   numbering of scipy.ndimage.label) and count [N] = K_n; then table [N][cap][10], cls [N][cap], out [N][H][W] (contracts:
//   include/dahitra_hip.h).
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

bool aligned4(const void* p) { return (reinterpret_cast<size_t>(p) & 3) == 0; }
long blocks_of(int H, int W) { return ((long)H * W + CC_BLOCK - 1) / CC_BLOCK; }
constexpr int CC_MAX_CAP = 1 << 24;

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
