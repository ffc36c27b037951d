// Test-time augmentation, the step between the views' decode launches and the one NMS over their union
// (radet/models/dense_heads/dense_test_mixins.py aug_test_bboxes: per-view candidates -> bbox_mapping_back -> torch.cat in
// view order): radet_merge_views maps the candidates of V * B (view, image) rows back into the frame and packs them per
// image, in ONE launch.
//
// The rows' lists lie in one pool; a row's descriptor (include/radet_hip.h, MERGE_DESC_INTS) says where, so views of
// different scales keep their own capacities.  Image b's output list is view 0's valid candidates, then view 1's, ...: an
// output slot j finds its view by walking the (at most TTA_MAX_VIEWS) counts of its image, which every lane of a wavefront
// reads from the same addresses.  grid (ceil(cap_out / 256), B): one slot per thread, one 16-byte load and store for the
// box, 4 + 4 + 8 bytes for the scores and the label -- memory-bound and tiny next to a forward pass.  No LDS, no scratch.
//
// Arithmetic (bbox_flip, then the division of bbox_mapping_back): fp32, each operation rounded once -- the file is built
// with -ffp-contract=off and the division is the correctly rounded one (__fdiv_rn: no reciprocal).
#include "common.h"
#include "radet_hip.h"

__device__ __forceinline__ float desc_f(const int* d, int k) { return __int_as_float(d[k]); }

__global__ __launch_bounds__(256) void merge_views_kernel(const int* __restrict__ desc, int V, int B, size_t pool,
                                                          const float4* __restrict__ pool_boxes,
                                                          const float* __restrict__ pool_scores,
                                                          const float* __restrict__ pool_ctr,
                                                          const int64_t* __restrict__ pool_labels,
                                                          const int* __restrict__ counts, int cap_out,
                                                          float4* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                          float* __restrict__ out_ctr, int64_t* __restrict__ out_labels,
                                                          int* __restrict__ out_count) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    // the view that fills slot j: the first whose running total exceeds j
    int before = 0, view = -1, k = 0;
    for (int v = 0; v < V; ++v) {
        const int* d = desc + (size_t)MERGE_DESC_INTS * ((size_t)v * B + b);
        int n = counts[(size_t)v * B + b];
        n = n < 0 ? 0 : (n > d[8] ? d[8] : n);
        if (view < 0 && j < before + n) { view = v; k = j - before; }
        before += n;
    }
    if (before > cap_out) before = cap_out;                     // (the host checked the capacities: cannot happen)
    if (j == 0) out_count[b] = before;
    if (view < 0 || j >= before) return;
    const int* d = desc + (size_t)MERGE_DESC_INTS * ((size_t)view * B + b);
    const size_t src = (size_t)(unsigned)d[7] + (size_t)k;
    if (d[7] < 0 || src >= pool) return;                        // (a row outside the pool: checked on the host as well)
    const size_t dst = (size_t)b * cap_out + j;
    float4 q = pool_boxes[src];
    const float h = desc_f(d, 0), w = desc_f(d, 1);
    const int flip = d[6];
    if (flip & 1) { const float x1 = w - q.z, x2 = w - q.x; q.x = x1; q.z = x2; }
    if (flip & 2) { const float y1 = h - q.w, y2 = h - q.y; q.y = y1; q.w = y2; }
    q.x = __fdiv_rn(q.x, desc_f(d, 2));
    q.y = __fdiv_rn(q.y, desc_f(d, 3));
    q.z = __fdiv_rn(q.z, desc_f(d, 4));
    q.w = __fdiv_rn(q.w, desc_f(d, 5));
    out_boxes[dst] = q;
    out_scores[dst] = pool_scores[src];
    out_ctr[dst] = pool_ctr[src];
    out_labels[dst] = pool_labels[src];
}

extern "C" int radet_merge_views(const int* desc_host, const int* desc, int V, int B, size_t pool, const float* pool_boxes,
                                 const float* pool_scores, const float* pool_ctr, const int64_t* pool_labels,
                                 const int* counts, int cap_out, float* out_boxes, float* out_scores, float* out_ctr,
                                 int64_t* out_labels, int* out_count, void* stream) {
    if (V < 1 || V > TTA_MAX_VIEWS || B < 0 || B > 65535 || cap_out < 1 || cap_out > 65536) return RADET_ERR_ARG;
    if (B == 0) return RADET_OK;
    if (!desc_host || !desc || !pool_boxes || !pool_scores || !pool_ctr || !pool_labels || !counts || !out_boxes ||
        !out_scores || !out_ctr || !out_labels || !out_count)
        return RADET_ERR_ARG;
    if (((uintptr_t)pool_boxes | (uintptr_t)out_boxes) & 15) return RADET_ERR_ARG;
    for (int b = 0; b < B; ++b) {
        long long total = 0;
        for (int v = 0; v < V; ++v) {
            const int* d = desc_host + (size_t)MERGE_DESC_INTS * ((size_t)v * B + b);
            const int flip = d[6], start = d[7], cap = d[8];
            if (flip < 0 || flip > 3 || cap < 0 || start < 0 || (unsigned long long)start + (unsigned long long)cap > pool)
                return RADET_ERR_ARG;
            total += cap;
        }
        if (total > cap_out) return RADET_ERR_ARG;
    }
    hipLaunchKernelGGL(merge_views_kernel, dim3((cap_out + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, desc, V, B, pool,
                       (const float4*)pool_boxes, pool_scores, pool_ctr, pool_labels, counts, cap_out, (float4*)out_boxes,
                       out_scores, out_ctr, out_labels, out_count);
    return radet_check_launch();
}
