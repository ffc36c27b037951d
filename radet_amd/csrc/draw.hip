// Detections drawn on frames in one launch (radet_draw_detections): box outlines and "name|score" labels over B frames of
// mixed sizes that are already in HBM (the PREP_DESC_INTS rows of radet_preprocess_frames: any byte address, any row stride),
// out of place (copy + overlay in one pass) or in place.  The pixel rules are written out in include/radet_hip.h.
//
// Gather form: one workgroup of 256 threads per DRAW_TW x DRAW_TH (128 x 8) pixel tile and frame, every pixel computed and stored by
// exactly one thread -- no atomics, no byte stored twice, so crossing outlines and overlapping labels come out the same on
// every run and in place is safe.  The workgroup
//   1. walks the frame's detections in chunks of 256 (one per thread): validity, the integer box, the rank among the valid
//      ones by ballot + popcount with running offsets across the 4 wavefronts (rank order kept, as crop_plan_kernel), the cut
//      at max_dets;
//   2. culls the drawn ones against its tile (outline rectangle or label rectangle) with a second ordered ballot compaction
//      and stores only the hits -- box, colour, label origin, the text as strip ids and the column where each strip ends --
//      in LDS (80 bytes each, at most DRAW_MAX_DETS);
//   3. each thread then owns 4 consecutive pixels (12 bytes) of one row: three dword loads and stores where the 12 bytes
//      start on a dword in that row, byte accesses otherwise (an unaligned base or row stride, the frame's right edge); it
//      walks the hit list twice from the last rank down (outlines: the lowest rank stays on top; labels: background then
//      text), every hit read from LDS at one address by the whole wavefront (a broadcast).
// A tile without hits is a plain copy out of place and stores nothing in place.  Memory-bound: 3 bytes read and 3 stored per
// pixel; the detections and the glyph atlas stay in L2.  The launch's time is the time of its densest tile (the blends of a
// pixel under several labels are a serial chain), which is why the tile is low: fewer pixels per thread.
#include "common.h"
#include "radet_hip.h"

#ifndef DRAW_ROWS
#define DRAW_ROWS 1                    // rows per thread (measured: 1 -> 43 / 18 us, 2 -> 57 / 25 us, 4 -> 98 / 41 us)
#endif
#define DRAW_TW 128                    // tile: 32 threads x 4 pixels wide,
#define DRAW_TH (8 * DRAW_ROWS)        //       8 thread rows x DRAW_ROWS rows high
#define DRAW_STRIP_DOT 10              // strips of the atlas: '0'..'9', '.', '|', 'class ', then one per class name
#define DRAW_STRIP_BAR 11
#define DRAW_STRIP_CLASS 12
#define DRAW_STRIP_NAME0 13
#define DRAW_MAX_STRIPS 11             // 'class ' + 5 digits + '|' + "d.dd"
#define DRAW_BATCH 8                   // label hits whose atlas loads are in flight together

struct DrawHit {
    int x1, y1, x2, y2;                // the integer box
    int lx, ly, wt;                    // the label rectangle's origin, the text's width
    unsigned colour;                   // the outline's b | g << 8 | r << 16
    unsigned short ids[DRAW_MAX_STRIPS + 1];   // strip ids (0 beyond the text); [DRAW_MAX_STRIPS] = their number
    unsigned short ends[DRAW_MAX_STRIPS + 1];  // the text column where each strip ends
};

// the reference's astype(int32) of a finite coordinate, after the clamp to +-2^20: truncation toward zero
__device__ __forceinline__ int draw_coord(float v) {
    return (int)fminf(fmaxf(v, -1048576.f), 1048576.f);
}

// out = (colour * a + pixel * (65025 - a) + 32512) / 65025 per channel, a in [0, 65025]
__device__ __forceinline__ unsigned draw_blend(unsigned px, unsigned colour, int a) {
    unsigned out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int p = (int)((px >> (8 * c)) & 0xFFu), q = (int)((colour >> (8 * c)) & 0xFFu);
        out |= (unsigned)((q * a + p * (65025 - a) + 32512) / 65025) << (8 * c);
    }
    return out;
}

// The text of a detection as strips: with names  <name> | d . d d ; without  'class ' <the label's nd digits> | d . d d
__device__ __forceinline__ int draw_text_strips(int n_names, int nd) { return n_names > 0 ? 6 : 6 + nd; }

__device__ __forceinline__ int draw_strip_id(int k, int n_names, int label, int nd, int cents) {
    if (n_names > 0) {
        if (k == 0) return DRAW_STRIP_NAME0 + label;
        k -= 1;
    } else {
        if (k == 0) return DRAW_STRIP_CLASS;
        if (k <= nd) {
            const int e = nd - k, div = e == 4 ? 10000 : e == 3 ? 1000 : e == 2 ? 100 : e == 1 ? 10 : 1;
            return (label / div) % 10;
        }
        k -= 1 + nd;
    }
    return k == 0 ? DRAW_STRIP_BAR : k == 1 ? cents / 100 : k == 2 ? DRAW_STRIP_DOT : k == 3 ? (cents / 10) % 10 : cents % 10;
}

struct DrawArgs {
    const int* src_desc;
    const int* dst_desc;
    const float* boxes;
    const float* scores;
    const int64_t* labels;
    const int* counts;
    const uint8_t* palette;
    const uint8_t* atlas;
    const int* widths;
    int K, thickness, box_colour, n_palette, text_colour, a_bg, max_dets, n_names, pad, inplace, S, Hc, Wa;
    float score_thr;
};

// The coverage of hit H's text at the 4 pixels x0 .. x0 + 3 of row y, one byte per pixel (0 outside the text).  The strip of
// a text column is the number of strips that end at or before it (the ends ascend), counted without a data-dependent loop.
__device__ __forceinline__ unsigned draw_text_cov(const DrawHit& H, int y, int x0, int p, const DrawArgs& A) {
    const int tv = y - H.ly - p, wt = H.wt, tu0 = x0 - H.lx - p;
    if (tv < 0 || tv >= A.Hc || tu0 + 3 < 0 || tu0 >= wt) return 0u;
    const int n = H.ids[DRAW_MAX_STRIPS];
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int tu = tu0 + k;
        if (tu < 0 || tu >= wt) continue;
        int q = 0;
#pragma unroll
        for (int j = 0; j < DRAW_MAX_STRIPS - 1; ++j) q += (j < n - 1 && tu >= (int)H.ends[j]) ? 1 : 0;
        const int off = tu - (q > 0 ? (int)H.ends[q - 1] : 0), id = H.ids[q];
        if (off < A.Wa && id < A.S) out |= (unsigned)A.atlas[((size_t)id * A.Hc + tv) * A.Wa + off] << (8 * k);
    }
    return out;
}

__global__ __launch_bounds__(256) void draw_detections_kernel(DrawArgs A) {
    __shared__ DrawHit hits[DRAW_MAX_DETS];
    __shared__ int wvalid[4], whit[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.z;
    const int* sd = A.src_desc + (size_t)PREP_DESC_INTS * b;
    const int* dd = A.dst_desc + (size_t)PREP_DESC_INTS * b;
    const int h = sd[3], w = sd[4];
    const int tx0 = blockIdx.x * DRAW_TW, ty0 = blockIdx.y * DRAW_TH;
    if (h <= 0 || w <= 0 || tx0 >= w || ty0 >= h || dd[3] != h || dd[4] != w) return;   // (uniform: before any barrier)
    const uint8_t* src = (const uint8_t*)(((uint64_t)(uint32_t)sd[1] << 32) | (uint64_t)(uint32_t)sd[0]);
    uint8_t* dst = (uint8_t*)(((uint64_t)(uint32_t)dd[1] << 32) | (uint64_t)(uint32_t)dd[0]);
    const size_t sstride = (size_t)(uint32_t)sd[2], dstride = (size_t)(uint32_t)dd[2];
    const int tx1 = min(tx0 + DRAW_TW, w) - 1, ty1 = min(ty0 + DRAW_TH, h) - 1;          // the tile, inclusive
    const int t = A.thickness, lo = t / 2, hi = (t - 1) / 2, p = A.pad, Hc = A.Hc;
    const int limit = A.n_names > 0 ? A.n_names : 100000;

    // ---- 1 + 2: the frame's drawn detections, the ones that touch this tile into LDS in rank order
    int cnt = A.counts[b];
    cnt = cnt < 0 ? 0 : cnt < A.K ? cnt : A.K;
    int n_drawn = 0, nh = 0;
    for (int c0 = 0; c0 < cnt && n_drawn < A.max_dets; c0 += 256) {
        const int j = c0 + tid;
        bool valid = false;
        int x1 = 0, y1 = 0, x2 = 0, y2 = 0, label = 0;
        float score = 0.f;
        if (j < cnt) {
            const size_t i = (size_t)b * A.K + j;
            const float4 bx = reinterpret_cast<const float4*>(A.boxes)[i];
            score = A.scores[i];
            const int64_t l64 = A.labels[i];
            if (isfinite(bx.x) && isfinite(bx.y) && isfinite(bx.z) && isfinite(bx.w) && isfinite(score) && score > A.score_thr &&
                l64 >= 0 && l64 < (int64_t)limit && (A.box_colour >= 0 || l64 < (int64_t)A.n_palette)) {
                label = (int)l64;
                x1 = draw_coord(bx.x); y1 = draw_coord(bx.y); x2 = draw_coord(bx.z); y2 = draw_coord(bx.w);
                valid = x2 >= x1 && y2 >= y1;
            }
        }
        const unsigned long long mv = __ballot(valid);
        if (lane == 0) wvalid[wv] = __popcll(mv);
        __syncthreads();
        int rank = n_drawn + __popcll(mv & ((1ull << lane) - 1ull));
        for (int k = 0; k < wv; ++k) rank += wvalid[k];
        const bool drawn = valid && rank < A.max_dets;
        bool hit = false;
        DrawHit H = {};
        if (drawn) {
            H.x1 = x1; H.y1 = y1; H.x2 = x2; H.y2 = y2;
            H.lx = H.ly = H.wt = 0;
            // the outline touches the tile: its outer rectangle does, and the tile is not wholly inside the hole
            hit = x1 - lo <= tx1 && x2 + hi >= tx0 && y1 - lo <= ty1 && y2 + hi >= ty0 &&
                  !(tx0 > x1 + hi && tx1 < x2 - lo && ty0 > y1 + hi && ty1 < y2 - lo);
            int n = 0;
            // the label's rows follow from y1 alone: most detections miss the tile's rows, and only the others need the text
            const int ly = max(0, min(y1, h - (Hc + 2 * p)));
            if (Hc > 0 && (hit || (ly <= ty1 && ly + Hc + 2 * p - 1 >= ty0))) {
                int nd = 0;
                if (A.n_names == 0) nd = label >= 10000 ? 5 : label >= 1000 ? 4 : label >= 100 ? 3 : label >= 10 ? 2 : 1;
                // the score as d.dd: ties round up (floor(x + 0.5) in double), not Python's round-half-even
                const double cd = floor((double)score * 100.0 + 0.5);
                const int cents = cd < 0.0 ? 0 : cd > 100.0 ? 100 : (int)cd;
                n = draw_text_strips(A.n_names, nd);
                int wt = 0;
#pragma unroll
                for (int k = 0; k < DRAW_MAX_STRIPS; ++k) {
                    int id = 0;
                    if (k < n) {
                        id = draw_strip_id(k, A.n_names, label, nd, cents);
                        int sw = A.widths[id];
                        sw = sw < 0 ? 0 : sw > A.Wa ? A.Wa : sw;
                        wt = min(wt + sw, DRAW_MAX_TEXT_W);
                    }
                    H.ids[k] = (unsigned short)id;
                    H.ends[k] = (unsigned short)wt;
                }
                const int lw = wt + 2 * p, lh = Hc + 2 * p;
                H.wt = wt;
                H.lx = max(0, min(x1, w - lw));
                H.ly = ly;
                hit = hit || (H.lx <= tx1 && H.lx + lw - 1 >= tx0 && H.ly <= ty1 && H.ly + lh - 1 >= ty0);
            }
            H.ids[DRAW_MAX_STRIPS] = (unsigned short)n;
            if (A.box_colour >= 0) {
                H.colour = (unsigned)A.box_colour;
            } else {
                const uint8_t* c = A.palette + (size_t)label * 3;
                H.colour = (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16;
            }
        }
        const unsigned long long mh = __ballot(hit);
        if (lane == 0) whit[wv] = __popcll(mh);
        __syncthreads();
        if (hit) {
            int pos = nh + __popcll(mh & ((1ull << lane) - 1ull));
            for (int k = 0; k < wv; ++k) pos += whit[k];
            hits[pos] = H;                                      // (pos < the number drawn <= max_dets <= DRAW_MAX_DETS)
        }
        n_drawn += wvalid[0] + wvalid[1] + wvalid[2] + wvalid[3];
        nh += whit[0] + whit[1] + whit[2] + whit[3];
        __syncthreads();                                        // the counters are reused, the hits are read below
    }
    // in place: every frame with DRAW_INPLACE, else a frame whose destination row names its source
    if (nh == 0 && (A.inplace || (src == dst && sstride == dstride))) return;   // a tile that nothing covers stores nothing

    // ---- 3: the pixels
    const int x0 = tx0 + 4 * (tid & 31);
    if (x0 >= w) return;
    const int npx = min(4, w - x0);
    const int a_bg = A.a_bg * 255, lh = Hc + 2 * p;
#pragma unroll
    for (int rr = 0; rr < DRAW_ROWS; ++rr) {
        const int y = ty0 + (tid >> 5) + 8 * rr;
        if (y >= h) break;
        const uint8_t* s = src + (size_t)y * sstride + (size_t)x0 * 3;
        uint8_t* d = dst + (size_t)y * dstride + (size_t)x0 * 3;
        unsigned px[4] = {0, 0, 0, 0};
        if (npx == 4 && ((uintptr_t)s & 3) == 0) {
            const unsigned w0 = ((const unsigned*)s)[0], w1 = ((const unsigned*)s)[1], w2 = ((const unsigned*)s)[2];
            px[0] = w0 & 0xFFFFFFu;
            px[1] = (w0 >> 24) | (w1 & 0xFFFFu) << 8;
            px[2] = (w1 >> 16) | (w2 & 0xFFu) << 16;
            px[3] = w2 >> 8;
        } else {
            for (int k = 0; k < npx; ++k) px[k] = (unsigned)s[3 * k] | (unsigned)s[3 * k + 1] << 8 | (unsigned)s[3 * k + 2] << 16;
        }
        // outlines, opaque: from the last rank down, so the lowest rank that covers a pixel stays
        for (int i = nh - 1; i >= 0; --i) {
            const DrawHit& H = hits[i];
            if (y < H.y1 - lo || y > H.y2 + hi) continue;
            const bool yin = y > H.y1 + hi && y < H.y2 - lo;
            const int ox1 = H.x1 - lo, ox2 = H.x2 + hi, ix1 = H.x1 + hi, ix2 = H.x2 - lo;
            const unsigned colour = H.colour;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = x0 + k;
                if (x >= ox1 && x <= ox2 && !(yin && x > ix1 && x < ix2)) px[k] = colour;
            }
        }
        // labels above all outlines, from the last rank down: the background, then the text.  In batches of DRAW_BATCH hits:
        // first every atlas byte the batch needs is requested (the loads do not depend on the pixels), then the blends run
        // in paint order -- one load latency per batch in the dependent chain of a pixel, not one per label that covers it
        if (Hc > 0) {
            for (int base = nh - 1; base >= 0; base -= DRAW_BATCH) {
                unsigned cov[DRAW_BATCH];
#pragma unroll
                for (int j = 0; j < DRAW_BATCH; ++j) cov[j] = base - j >= 0 ? draw_text_cov(hits[base - j], y, x0, p, A) : 0u;
#pragma unroll
                for (int j = 0; j < DRAW_BATCH; ++j) {
                    if (base - j < 0) break;
                    const DrawHit& H = hits[base - j];
                    const int v = y - H.ly;
                    if (v < 0 || v >= lh) continue;
                    const int u0 = x0 - H.lx, lw = H.wt + 2 * p;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (u0 + k < 0 || u0 + k >= lw) continue;
                        px[k] = draw_blend(px[k], 0u, a_bg);
                        const int c = (int)((cov[j] >> (8 * k)) & 0xFFu);
                        if (c) px[k] = draw_blend(px[k], (unsigned)A.text_colour, 255 * c);
                    }
                }
            }
        }
        if (npx == 4 && ((uintptr_t)d & 3) == 0) {
            ((unsigned*)d)[0] = px[0] | px[1] << 24;
            ((unsigned*)d)[1] = px[1] >> 8 | px[2] << 16;
            ((unsigned*)d)[2] = px[2] >> 16 | px[3] << 8;
        } else {
            for (int k = 0; k < npx; ++k) {
                d[3 * k] = (uint8_t)px[k]; d[3 * k + 1] = (uint8_t)(px[k] >> 8); d[3 * k + 2] = (uint8_t)(px[k] >> 16);
            }
        }
    }
}

extern "C" int radet_draw_detections(const int* src_desc, const int* dst_desc, int B, int max_h, int max_w, const float* boxes,
                                     const float* scores, const int64_t* labels, const int* counts, int K, int thickness,
                                     int box_colour, const uint8_t* palette, int n_palette, int text_colour, int a_bg,
                                     float score_thr, int max_dets, int n_names, int pad, int flags, const uint8_t* atlas,
                                     const int* widths, int S, int Hc, int Wa, void* stream) {
    if (B < 0 || B > 65535 || K < 0 || max_h < 0 || max_w < 0 || (flags & ~DRAW_INPLACE)) return RADET_ERR_ARG;
    if (thickness < 1 || thickness > DRAW_MAX_THICKNESS || max_dets < 0 || max_dets > DRAW_MAX_DETS) return RADET_ERR_ARG;
    if (a_bg < 0 || a_bg > 255 || text_colour < 0 || text_colour > 0xFFFFFF || box_colour > 0xFFFFFF) return RADET_ERR_ARG;
    if (box_colour < 0 && (!palette || n_palette < 1)) return RADET_ERR_ARG;
    if (n_names < 0 || n_names > 65535 - DRAW_STRIP_NAME0 || pad < 0 || pad > DRAW_MAX_PAD || std::isnan(score_thr))
        return RADET_ERR_ARG;
    if (Hc < 0 || Hc > DRAW_MAX_GLYPH_H) return RADET_ERR_ARG;
    if (Hc > 0 && (!atlas || !widths || Wa < 1 || Wa > DRAW_MAX_TEXT_W || S < DRAW_STRIP_NAME0 + n_names)) return RADET_ERR_ARG;
    if (B == 0 || max_h == 0 || max_w == 0) return RADET_OK;
    if (!src_desc || !dst_desc || !counts) return RADET_ERR_ARG;
    if (K > 0 && (!boxes || !scores || !labels || ((uintptr_t)boxes & 15))) return RADET_ERR_ARG;
    const long long gy = ((long long)max_h + DRAW_TH - 1) / DRAW_TH;
    if (gy > 65535) return RADET_ERR_ARG;
    DrawArgs A;
    A.src_desc = src_desc; A.dst_desc = dst_desc; A.boxes = boxes; A.scores = scores; A.labels = labels; A.counts = counts;
    A.palette = palette; A.atlas = atlas; A.widths = widths;
    A.K = K; A.thickness = thickness; A.box_colour = box_colour; A.n_palette = n_palette; A.text_colour = text_colour;
    A.a_bg = a_bg; A.max_dets = max_dets; A.n_names = n_names; A.pad = pad; A.inplace = (flags & DRAW_INPLACE) ? 1 : 0;
    A.S = S; A.Hc = Hc; A.Wa = Wa; A.score_thr = score_thr;
    const dim3 grid((max_w + DRAW_TW - 1) / DRAW_TW, (unsigned)gy, B), block(256);
    hipLaunchKernelGGL(draw_detections_kernel, grid, block, 0, (hipStream_t)stream, A);
    return radet_check_launch();
}
