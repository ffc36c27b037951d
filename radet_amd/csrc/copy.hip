// Segmented copy between arbitrary device byte addresses: one launch moves every row {source, destination, bytes} of a
// descriptor table.  The sample cache (radet_amd/datasets/sample_cache.py) uses it in both directions: decoded images from
// its HBM arena into a batch's packed source buffer, and a batch's newly decoded images from that buffer into the arena.
//
// Work is cut into tiles of COPY_TILE_BYTES of the DESTINATION, counted from the destination rounded down to 16 bytes, so
// every 16-byte piece of a tile is an aligned global_store_dwordx4.  A row owns ceil(((dst & 15) + bytes) / COPY_TILE_BYTES)
// consecutive tiles starting at the row's `first tile` word (the host's exclusive prefix sum); a workgroup finds its row
// by binary search over that column, so a table may mix rows of any sizes: the grid is the tile total, not rows x the
// longest row.  The column only distributes work: whatever it holds, a workgroup moves bytes of its row's own range.
//
// Source side: the 16 bytes of a piece start at any byte.  They are read as one dword-aligned global_load_dwordx4 (multi-
// dword global loads need dword alignment only) plus, when the source is not dword-aligned against the destination, the
// next dword, and shifted into place with v_alignbyte_b32 -- no byte-unaligned vector load, whose legality depends on the
// alignment mode the driver configured.  The fast path is taken only where those dwords lie inside the row's source range;
// the few pieces at a row's two ends (and rows shorter than that) go byte by byte.  Nothing outside [src, src + bytes) is
// read and nothing outside [dst, dst + bytes) is written.
#include "common.h"
#include "radet_hip.h"

#define COPY_THREADS 256
#define COPY_PIECES (COPY_TILE_BYTES / 16 / COPY_THREADS)

typedef uint32_t copy_u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t copy_u32x4 __attribute__((ext_vector_type(4)));
// the addresses arrive as integers: say that they are global memory, or the compiler has to emit flat_ instructions
#define COPY_GLOBAL __attribute__((address_space(1)))

static_assert(COPY_TILE_BYTES % (16 * COPY_THREADS) == 0, "a tile is whole 16-byte pieces per thread");

__global__ __launch_bounds__(COPY_THREADS) void copy_segments_kernel(const int* __restrict__ desc, int n) {
    const int tile = blockIdx.x;
    // the last row whose first tile is <= tile (rows without bytes own no tile and are passed over)
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(size_t)mid * COPY_DESC_INTS + 5] <= tile) lo = mid; else hi = mid - 1;
    }
    const int* d = desc + (size_t)lo * COPY_DESC_INTS;
    const uint64_t src = (uint64_t)(uint32_t)d[0] | ((uint64_t)(uint32_t)d[1] << 32);
    const uint64_t dst = (uint64_t)(uint32_t)d[2] | ((uint64_t)(uint32_t)d[3] << 32);
    const int64_t nbytes = d[4];
    const int64_t t = (int64_t)tile - d[5];
    if (nbytes <= 0 || t < 0) return;
    const int64_t head = (int64_t)(dst & 15);                  // the row's first byte inside its first 16-byte piece
    // positions below are relative to the row's first destination byte: piece p covers [p * 16 - head, p * 16 - head + 16)
    const int64_t tile_lo = t * COPY_TILE_BYTES - head;
    if (tile_lo >= nbytes) return;
    const unsigned sh = (unsigned)((src - head) & 3);           // byte offset of a piece's source inside its first dword
    const COPY_GLOBAL uint8_t* sp = (const COPY_GLOBAL uint8_t*)src;
    COPY_GLOBAL uint8_t* dp = (COPY_GLOBAL uint8_t*)dst;
#pragma unroll
    for (int k = 0; k < COPY_PIECES; ++k) {
        const int64_t o = tile_lo + ((int64_t)k * COPY_THREADS + threadIdx.x) * 16;
        if (o >= nbytes) break;
        // dword-aligned source span of the piece: [a, a + 16) and one more dword when sh != 0
        const int64_t a = o - sh;
        if (o >= 0 && o + 16 <= nbytes && a >= 0 && a + (sh ? 20 : 16) <= nbytes) {
            const copy_u32x4_a4 w = *(const COPY_GLOBAL copy_u32x4_a4*)(sp + a);
            copy_u32x4 v;
            if (sh) {
                const uint32_t w4 = *(const COPY_GLOBAL uint32_t*)(sp + a + 16);
                v.x = __builtin_amdgcn_alignbyte(w.y, w.x, sh);
                v.y = __builtin_amdgcn_alignbyte(w.z, w.y, sh);
                v.z = __builtin_amdgcn_alignbyte(w.w, w.z, sh);
                v.w = __builtin_amdgcn_alignbyte(w4, w.w, sh);
            } else {
                v.x = w.x; v.y = w.y; v.z = w.z; v.w = w.w;
            }
            *(COPY_GLOBAL copy_u32x4*)(dp + o) = v;
        } else {
            const int64_t b0 = o < 0 ? 0 : o, b1 = o + 16 < nbytes ? o + 16 : nbytes;
            for (int64_t b = b0; b < b1; ++b) dp[b] = sp[b];
        }
    }
}

extern "C" int radet_copy_segments(const int* desc, int n, int n_tiles, void* stream) {
    if (n < 0 || n_tiles < 0 || (n > 0 && !desc)) return RADET_ERR_ARG;
    if (n == 0 || n_tiles == 0) return RADET_OK;
    hipLaunchKernelGGL(copy_segments_kernel, dim3(n_tiles), dim3(COPY_THREADS), 0, (hipStream_t)stream, desc, n);
    return radet_check_launch();
}
