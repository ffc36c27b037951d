// Tiled inference, the step between the rows' decode launches and the one NMS over their union: radet_merge_tiles drops the
// candidates that a tile border cut, maps the others back into the frame and packs them per image, in ONE launch.
//
// A batch of B frames has R rows, image-major (row_start i32 [B + 1]): per image the full-frame row (if any), then its tiles.
// The rows' lists lie in one pool; a row's descriptor (include/radet_hip.h, TILE_DESC_INTS) says where, how the row maps
// into the frame and which of its sides are cuts through the frame (edge mask).  Unlike radet_merge_views this is a
// compaction, not a copy: which slot a candidate gets depends on every candidate in front of it.  One workgroup of 512
// threads (8 wavefronts) per image walks the image's candidates -- its rows in order, inside a row in candidate order -- 512
// at a time: the inclusive prefix of the rows' clamped counts lies in LDS (one wave scan over at most TILE_MAX_ROWS rows),
// a thread finds the row of its candidate by bisection in it, so chunks are dense whatever the rows' fill.  The keep flag goes
// through a 64-lane ballot, popcount below the lane gives the rank in the wavefront, the 8 wave totals go through LDS
// (two sets, alternating: ONE barrier per chunk) and every thread keeps the running base in a register.  No atomics decide
// a position, so the output order is the input order whatever the scheduling.  The box moves as one 16-byte load and one
// 16-byte store; 260 + 64 bytes of LDS, no scratch.
//
// Arithmetic: fp32, each operation rounded once -- the file is built with -ffp-contract=off, the division is the correctly
// rounded one (__fdiv_rn, bbox_mapping_back's true division), then one add of the tile's offset.
#include "common.h"
#include "radet_hip.h"

#include <math.h>

#define TILE_THREADS 512
#define TILE_WAVES (TILE_THREADS / 64)

__device__ __forceinline__ float tdesc_f(const int* d, int k) { return __int_as_float(d[k]); }

__global__ __launch_bounds__(TILE_THREADS) void merge_tiles_kernel(
    const int* __restrict__ desc, const int* __restrict__ row_start, size_t pool, const float4* __restrict__ pool_boxes,
    const float* __restrict__ pool_scores, const float* __restrict__ pool_ctr, const int64_t* __restrict__ pool_labels,
    const int* __restrict__ counts, float margin, int cap_out, float4* __restrict__ out_boxes, float* __restrict__ out_scores,
    float* __restrict__ out_ctr, int64_t* __restrict__ out_labels, int* __restrict__ out_count, int* __restrict__ out_dropped) {
    __shared__ int pre[TILE_MAX_ROWS + 1];                      // pre[k] = clamped candidates of the image's rows 0 .. k - 1
    __shared__ int wcnt[2][TILE_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r0 = row_start[b];
    int nr = row_start[b + 1] - r0;
    nr = nr < 0 ? 0 : (nr > TILE_MAX_ROWS ? TILE_MAX_ROWS : nr);  // (the host checked 1..TILE_MAX_ROWS: cannot happen)
    if (wv == 0) {
        int n = 0;
        if (lane < nr) {
            const int cap = desc[(size_t)TILE_DESC_INTS * (size_t)(r0 + lane) + 10];
            n = counts[r0 + lane];
            n = n < 0 ? 0 : (n > cap ? cap : n);
        }
        for (int d = 1; d < 64; d <<= 1) {                      // inclusive scan over the wavefront
            const int up = __shfl_up(n, d, 64);
            if (lane >= d) n += up;
        }
        pre[lane + 1] = n;
        if (lane == 0) pre[0] = 0;
    }
    __syncthreads();
    int total = pre[nr];
    if (total > cap_out) total = cap_out;                       // (the host checked the capacities: cannot happen)
    int base = 0, par = 0;
    for (int c0 = 0; c0 < total; c0 += TILE_THREADS, par ^= 1) {
        const int i = c0 + tid;
        bool keep = false;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        size_t src = 0;
        if (i < total) {
            int lo = 0, hi = nr;                                // the row of candidate i: the last k with pre[k] <= i
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (pre[mid] <= i) lo = mid; else hi = mid;
            }
            const int* d = desc + (size_t)TILE_DESC_INTS * (size_t)(r0 + lo);
            src = (size_t)(unsigned)d[9] + (size_t)(i - pre[lo]);
            if (d[9] >= 0 && src < pool) {                      // (a row outside the pool: checked on the host as well)
                q = pool_boxes[src];
                const float h = tdesc_f(d, 0), w = tdesc_f(d, 1);
                const int edge = d[8];
                const bool cut = ((edge & TILE_EDGE_L) && q.x <= margin) || ((edge & TILE_EDGE_T) && q.y <= margin) ||
                                 ((edge & TILE_EDGE_R) && q.z >= __fsub_rn(w, margin)) ||
                                 ((edge & TILE_EDGE_B) && q.w >= __fsub_rn(h, margin));
                keep = !cut;
                if (keep) {
                    q.x = __fadd_rn(__fdiv_rn(q.x, tdesc_f(d, 2)), tdesc_f(d, 6));
                    q.y = __fadd_rn(__fdiv_rn(q.y, tdesc_f(d, 3)), tdesc_f(d, 7));
                    q.z = __fadd_rn(__fdiv_rn(q.z, tdesc_f(d, 4)), tdesc_f(d, 6));
                    q.w = __fadd_rn(__fdiv_rn(q.w, tdesc_f(d, 5)), tdesc_f(d, 7));
                }
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wcnt[par][wv] = __popcll(m);
        __syncthreads();                                        // (the other set is written next: one barrier per chunk)
        int off = base, tot = 0;
        for (int k = 0; k < TILE_WAVES; ++k) {
            const int c = wcnt[par][k];
            if (k < wv) off += c;
            tot += c;
        }
        off += __popcll(m & ((1ull << lane) - 1ull));
        if (keep && off < cap_out) {
            const size_t dst = (size_t)b * cap_out + off;
            out_boxes[dst] = q;
            out_scores[dst] = pool_scores[src];
            out_ctr[dst] = pool_ctr[src];
            out_labels[dst] = pool_labels[src];
        }
        base += tot;
    }
    if (tid == 0) {
        out_count[b] = base;
        out_dropped[b] = total - base;
    }
}

extern "C" int radet_merge_tiles(const int* desc_host, const int* desc, const int* row_start_host, const int* row_start, int B,
                                 size_t pool, const float* pool_boxes, const float* pool_scores, const float* pool_ctr,
                                 const int64_t* pool_labels, const int* counts, float edge_margin, int cap_out, float* out_boxes,
                                 float* out_scores, float* out_ctr, int64_t* out_labels, int* out_count, int* out_dropped,
                                 void* stream) {
    if (B < 0 || B > 65535 || cap_out < 1 || cap_out > 65536 || !isfinite(edge_margin) || edge_margin < 0.f) return RADET_ERR_ARG;
    if (B == 0) return RADET_OK;
    if (!desc_host || !desc || !row_start_host || !row_start || !pool_boxes || !pool_scores || !pool_ctr || !pool_labels ||
        !counts || !out_boxes || !out_scores || !out_ctr || !out_labels || !out_count || !out_dropped)
        return RADET_ERR_ARG;
    if (((uintptr_t)pool_boxes | (uintptr_t)out_boxes) & 15) return RADET_ERR_ARG;
    if (row_start_host[0] != 0) return RADET_ERR_ARG;
    for (int b = 0; b < B; ++b) {
        const long long r0 = row_start_host[b], nr = (long long)row_start_host[b + 1] - r0;
        if (nr < 1 || nr > TILE_MAX_ROWS) return RADET_ERR_ARG;
        long long total = 0;
        for (long long r = r0; r < r0 + nr; ++r) {
            const int* d = desc_host + (size_t)TILE_DESC_INTS * (size_t)r;
            const int edge = d[8], start = d[9], cap = d[10];
            if (edge < 0 || edge > 15 || cap < 0 || start < 0 || (unsigned long long)start + (unsigned long long)cap > pool)
                return RADET_ERR_ARG;
            total += cap;
        }
        if (total > cap_out) return RADET_ERR_ARG;
    }
    hipLaunchKernelGGL(merge_tiles_kernel, dim3(B), dim3(TILE_THREADS), 0, (hipStream_t)stream, desc, row_start, pool,
                       (const float4*)pool_boxes, pool_scores, pool_ctr, pool_labels, counts, edge_margin, cap_out,
                       (float4*)out_boxes, out_scores, out_ctr, out_labels, out_count, out_dropped);
    return radet_check_launch();
}
