// xBD class table: how many bytes of every resident post-disaster label equal 0, 1, 2, 3, 4 or lie above 4 -- the numbers the
// training scripts' `file_classes` scan (c in msk1) is read from.  All integer, exact, the same on every call.
//
// labels [n][hw] uint8 -> counts [n][6] int32.  The call clears the 6 n words with a memset node on the stream, then ONE launch:
// grid (chunks of a file, files); a workgroup of 256 threads counts one chunk of CT_CHUNK bytes of one file and adds its six
// numbers to the file's row, at most one integer atomic per class (a class the chunk does not hold adds nothing).
//   * A file starts at byte f * hw of the stack, so neither a file nor a chunk need start on a 16-byte boundary.  The chunk's
//     bytes up to the first 16-byte aligned ADDRESS (at most 15) are its head, those after the last aligned piece its tail; one
//     thread takes one of them.  The aligned body is read with 16-byte loads, consecutive threads on consecutive pieces, four
//     loads in flight per thread.  The chunks of a file partition it, so every byte is counted once and no byte outside the
//     file is read.
//   * A dword w holds four labels.  For k = 1 .. 5, ((w | 0x80808080) - k * 0x01010101) cannot borrow across bytes (every byte
//     of the minuend is >= 0x80 > k) and leaves bit 7 of a byte set where its low seven bits are >= k; OR-ing w's own bit 7 back
//     in gives 0x80 in exactly the bytes that are >= k.  v_sad_u8 against zero adds those four bytes to a 32-bit register: the
//     thread's count of bytes >= k, times 128.  Nothing is counted in packed 8- or 16-bit lanes, so nothing can wrap: a thread
//     sees at most CT_CHUNK / 256 + 1 bytes and its register holds 128 times that.
//   * The five threshold counts are summed across the wave (shuffles), then across the four waves through LDS; with the chunk's
//     length L the classes are c0 = L - g1, c_k = g_k - g_(k+1), c5 = g5.
// Integer adds commute: the order in which workgroups arrive cannot change a word.
#include "common.h"

namespace {

constexpr int CT_THREADS = 256;
constexpr long CT_CHUNK = 65536;             // bytes of one file that one workgroup counts: 16 aligned loads per thread
constexpr int CT_CLASSES = 6;
constexpr int CT_MAX_GRID_Y = 65535;
constexpr unsigned CT_HI = 0x80808080u, CT_ONES = 0x01010101u;

__device__ __forceinline__ void count_dword(unsigned w, unsigned (&g)[5]) {
    const unsigned u = w | CT_HI, top = w & CT_HI;
#pragma unroll
    for (int k = 1; k <= 5; ++k) g[k - 1] = __builtin_amdgcn_sad_u8(((u - k * CT_ONES) & CT_HI) | top, 0u, g[k - 1]);
}

__device__ __forceinline__ void count_piece(const uint4& v, unsigned (&g)[5]) {
    count_dword(v.x, g);
    count_dword(v.y, g);
    count_dword(v.z, g);
    count_dword(v.w, g);
}

// grid (chunks, min(n, 65535)): blockIdx.y strides over the files
__global__ __launch_bounds__(CT_THREADS) void class_table_kernel(const unsigned char* __restrict__ labels, long n, long hw,
                                                                 int* __restrict__ counts) {
    __shared__ unsigned part[CT_THREADS / 64][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long c0 = (long)blockIdx.x * CT_CHUNK;
    const long len = (hw - c0 < CT_CHUNK) ? hw - c0 : CT_CHUNK;          // 1 .. CT_CHUNK: the grid has ceil(hw / CT_CHUNK) chunks
    for (long f = blockIdx.y; f < n; f += gridDim.y) {
        const unsigned char* p = labels + f * hw + c0;
        // head: the bytes in front of the first 16-byte aligned address, tail: those behind the last whole piece
        long head = (long)((16 - (reinterpret_cast<size_t>(p) & 15)) & 15);
        if (head > len) head = len;
        const long nvec = (len - head) >> 4;
        const long tail0 = head + (nvec << 4);
        const uint4* body = reinterpret_cast<const uint4*>(p + head);
        unsigned g[5] = {0u, 0u, 0u, 0u, 0u};
        long i = tid;
        for (; i + 3 * CT_THREADS < nvec; i += 4 * CT_THREADS) {
            const uint4 a = body[i], b = body[i + CT_THREADS], c = body[i + 2 * CT_THREADS], d = body[i + 3 * CT_THREADS];
            count_piece(a, g);
            count_piece(b, g);
            count_piece(c, g);
            count_piece(d, g);
        }
        for (; i < nvec; i += CT_THREADS) count_piece(body[i], g);
#pragma unroll
        for (int k = 0; k < 5; ++k) g[k] >>= 7;
        // one byte per thread: threads 0 .. 14 the head, threads 16 .. 30 the tail
        long at = -1;
        if (tid < head) at = tid;
        else if (tid >= 16 && tail0 + (tid - 16) < len) at = tail0 + (tid - 16);
        if (at >= 0) {
            const unsigned b = p[at];
#pragma unroll
            for (int k = 1; k <= 5; ++k) g[k - 1] += b >= (unsigned)k;
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            unsigned v = g[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            g[k] = v;
        }
        __syncthreads();                                    // the previous file's reads of `part`
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) part[wave][k] = g[k];
        }
        __syncthreads();
        if (tid < CT_CLASSES) {
            // ge(k) = bytes >= k: ge(0) = len, ge(6) = 0
            unsigned lo = 0, hi = 0;                        // ge(tid), ge(tid + 1)
            if (tid == 0) lo = (unsigned)len;
            else lo = part[0][tid - 1] + part[1][tid - 1] + part[2][tid - 1] + part[3][tid - 1];
            if (tid < 5) hi = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
            const unsigned c = lo - hi;
            if (c) atomicAdd(counts + f * CT_CLASSES + tid, (int)c);
        }
    }
}

}  // namespace

extern "C" int dh_xbd_class_table_chunk(void) { return (int)CT_CHUNK; }

extern "C" int dh_xbd_class_table_u8(const unsigned char* labels, long n, long hw, int* counts, void* stream) {
    DH_REQUIRE(labels && counts, "xbd_class_table: null pointer");
    DH_REQUIRE(n >= 1, "xbd_class_table: n=%ld: no file", n);
    DH_REQUIRE(hw >= 1, "xbd_class_table: hw=%ld: an empty file", hw);
    DH_REQUIRE(hw <= 0x7fffffffL, "xbd_class_table: hw=%ld: a file holds fewer than 2^31 bytes (the counts are int32)", hw);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int) * CT_CLASSES * (size_t)n, st);
    if (e != hipSuccess) DH_FAIL("xbd_class_table: clearing the counts: %s", hipGetErrorString(e));
    const dim3 grid((unsigned)((hw + CT_CHUNK - 1) / CT_CHUNK), (unsigned)(n < CT_MAX_GRID_Y ? n : CT_MAX_GRID_Y));
    hipLaunchKernelGGL(class_table_kernel, grid, dim3(CT_THREADS), 0, st, labels, n, hw, counts);
    DH_CHECK_LAUNCH("xbd_class_table");
    return 0;
}
