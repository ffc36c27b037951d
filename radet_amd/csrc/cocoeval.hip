// COCO-protocol bounding-box evaluation on the device: the matching of radet_amd/datasets/cocoeval.py:COCOeval._evaluate_img
// and the precision / recall tables of COCOeval.accumulate, bit for bit (IEEE fp64 + - * / and comparisons only; the
// Makefile's -ffp-contract=off keeps every product and sum a rounding of its own).  The host evaluator is the yardstick:
// tests/test_gpu_cocoeval.py compares the uint64 views of the three tables.
//
// radet_coco_match: one wave per segment = (category, image) pair (one per image with useCats = 0).  Detections of a segment
// arrive in descending-score order, cut to maxDets[-1]; they are visited one after the other (the greedy matching is serial
// in them).  For each, all 64 lanes compute its IoU row over the segment's ground truths into LDS; then lane c = a * T + t
// walks that row for its own (area range, IoU threshold) in the evaluator's gt order (non-ignored first, stable; the order
// depends on the area range) with its matched-gt set as a bit mask in LDS.
// radet_coco_accumulate: one thread per (category, area range, maxDets entry, IoU threshold).  The detections of a category
// arrive stable-sorted by descending score over all images.  One forward pass counts tp / fp, one backward pass forms
// precision, its right-to-left envelope (a running maximum) and hands the envelope value to every recall threshold whose
// left-sided search lands on the current index.
#include "common.h"
#include "radet_hip.h"

#define COCO_CAP RADET_COCO_MAX_GT
#define COCO_MAXA 8
#define ORD_IDX 0x1ff            // gt index inside the segment (COCO_CAP <= 512)
#define ORD_CROWD 0x4000
#define ORD_IGN 0x8000

static_assert(COCO_CAP <= 512 && COCO_CAP % 64 == 0, "s_ord packs the gt index into 9 bits");

__global__ __launch_bounds__(64) void coco_match_kernel(
    const float* __restrict__ dt, const int* __restrict__ dt_off, const double* __restrict__ gbox,
    const double* __restrict__ garea, const uint8_t* __restrict__ gflags, const int* __restrict__ gt_off,
    const double* __restrict__ thrs, int T, const double* __restrict__ rng, int A,
    int* __restrict__ dt_match, uint8_t* __restrict__ dt_flag, int* __restrict__ gt_match, uint8_t* __restrict__ gt_ignore) {
    __shared__ double s_iou[COCO_CAP];
    __shared__ unsigned short s_ord[COCO_MAXA][COCO_CAP];
    __shared__ unsigned long long s_mask[COCO_CAP / 64][64];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int g0 = gt_off[s], ng = gt_off[s + 1] - g0, d0 = dt_off[s], nd = dt_off[s + 1] - d0;
    if (ng > COCO_CAP || ng < 0 || nd < 0 || (ng == 0 && nd == 0)) return;      // (oversize: the launcher has refused already)
    const int AT = A * T;
    const unsigned long long below = (1ull << lane) - 1ull;

    // gtIgnore per area range and the evaluator's visiting order: a stable partition, non-ignored first
    for (int a = 0; a < A; ++a) {
        const double lo = rng[2 * a], hi = rng[2 * a + 1];
        int nreg = 0;
        for (int base = 0; base < ng; base += 64) {
            const int j = base + lane;
            bool reg = false;
            if (j < ng) {
                const double ar = garea[g0 + j];
                reg = !((gflags[g0 + j] & 1) || ar < lo || ar > hi);
            }
            nreg += __popcll(__ballot(reg));
        }
        int creg = 0, cign = nreg;
        for (int base = 0; base < ng; base += 64) {
            const int j = base + lane;
            const bool valid = j < ng;
            bool ign = false, crowd = false;
            if (valid) {
                const double ar = garea[g0 + j];
                crowd = gflags[g0 + j] & 1;
                ign = crowd || ar < lo || ar > hi;
            }
            const unsigned long long breg = __ballot(valid && !ign), bign = __ballot(valid && ign);
            if (valid) {
                const int pos = ign ? cign + __popcll(bign & below) : creg + __popcll(breg & below);
                s_ord[a][pos] = (unsigned short)(j | (crowd ? ORD_CROWD : 0) | (ign ? ORD_IGN : 0));
                gt_ignore[(size_t)(g0 + j) * A + a] = ign ? 1 : 0;
            }
            creg += __popcll(breg);
            cign += __popcll(bign);
        }
    }
    for (int w = 0; w < (ng + 63) / 64; ++w) s_mask[w][lane] = 0ull;
    __syncthreads();

    const bool active = lane < AT;
    const int a = active ? lane / T : 0, t = active ? lane % T : 0;
    const double thr = thrs[t] < 1 - 1e-10 ? thrs[t] : 1 - 1e-10;              // min(t, 1 - 1e-10)
    const double lo = rng[2 * a], hi = rng[2 * a + 1];

    for (int d = 0; d < nd; ++d) {
        const float* b = dt + (size_t)(d0 + d) * 4;
        // BOPDataset.xyxy2xywh + COCO.loadRes: the fp32 corners widened, extents and area formed in fp64
        const double dx = (double)b[0], dy = (double)b[1];
        const double dw = (double)b[2] - dx, dh = (double)b[3] - dy;
        const double da = dw * dh;
        for (int j = lane; j < ng; j += 64) {                                     // cocoeval.bbox_iou, one row
            const double* g = gbox + (size_t)(g0 + j) * 4;
            const double gx = g[0], gy = g[1], gw = g[2], gh = g[3];
            const double ga = gw * gh;
            const double xr = dx + dw, gxr = gx + gw, yb = dy + dh, gyb = gy + gh;
            const double iw = (xr < gxr ? xr : gxr) - (dx > gx ? dx : gx);
            const double ih = (yb < gyb ? yb : gyb) - (dy > gy ? dy : gy);
            const double inter = (iw <= 0 || ih <= 0) ? 0.0 : iw * ih;
            const double uni = (gflags[g0 + j] & 1) ? da : da + ga - inter;
            s_iou[j] = inter / uni;
        }
        __syncthreads();
        if (active) {
            double iou = thr;
            int m = -1, mj = -1, mign = 0;
            for (int pos = 0; pos < ng; ++pos) {
                const unsigned o = s_ord[a][pos];
                const int j = o & ORD_IDX, ign = (o & ORD_IGN) ? 1 : 0;
                if (((s_mask[j >> 6][lane] >> (j & 63)) & 1ull) && !(o & ORD_CROWD)) continue;   // matched (crowds match repeatedly)
                if (m > -1 && mign == 0 && ign == 1) break;             // matched a regular gt and only ignored ones remain
                const double v = s_iou[j];
                if (v < iou) continue;                                  // (equality matches, and passes an equal IoU on to the later gt)
                iou = v;
                m = pos;
                mj = j;
                mign = ign;
            }
            // the host keeps the gt's annotation id in dtMatches and reads "== 0" as unmatched: an id of 0 counts as no match
            const bool matched = m > -1 && !(gflags[g0 + mj] & 2);
            const bool ignore = (m > -1 && mign) || (!matched && (da < lo || da > hi));
            if (m > -1) {
                s_mask[mj >> 6][lane] |= 1ull << (mj & 63);
                gt_match[(size_t)(g0 + mj) * AT + lane] = d;
            }
            dt_match[(size_t)(d0 + d) * AT + lane] = mj;
            dt_flag[(size_t)(d0 + d) * AT + lane] = (uint8_t)((matched ? 1 : 0) | (ignore ? 2 : 0));
        }
        __syncthreads();
    }
}

int radet_coco_match(const float* dt_xyxy, const int* dt_off, const double* gt_xywh, const double* gt_area,
                     const uint8_t* gt_flags, const int* gt_off, int nseg, int max_seg_gt, const double* iou_thrs, int T,
                     const double* area_rng, int A, int* dt_match, uint8_t* dt_flag, int* gt_match, uint8_t* gt_ignore,
                     void* stream) {
    if (nseg < 0 || T < 1 || A < 1 || A > COCO_MAXA || A * T > 64 || max_seg_gt < 0) return RADET_ERR_ARG;
    if (max_seg_gt > COCO_CAP) return RADET_ERR_COCO_OVERSIZE;
    if (nseg == 0) return RADET_OK;
    hipLaunchKernelGGL(coco_match_kernel, dim3(nseg), dim3(64), 0, (hipStream_t)stream, dt_xyxy, dt_off, gt_xywh, gt_area,
                       gt_flags, gt_off, iou_thrs, T, area_rng, A, dt_match, dt_flag, gt_match, gt_ignore);
    return radet_check_launch();
}

__global__ __launch_bounds__(64) void coco_accumulate_kernel(
    const uint8_t* __restrict__ flags, const int* __restrict__ rank, const float* __restrict__ score,
    const int* __restrict__ cat_off, const uint8_t* __restrict__ gt_ignore, const int* __restrict__ gt_cat_off,
    const int* __restrict__ max_dets, const double* __restrict__ rec, int T, int R, int K, int A, int M,
    double* __restrict__ precision, double* __restrict__ recall, double* __restrict__ scores) {
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= K * A * M * T) return;
    const int t = idx % T, m = (idx / T) % M, a = (idx / (T * M)) % A, k = idx / (T * M * A);
    int npig = 0;
    for (int g = gt_cat_off[k]; g < gt_cat_off[k + 1]; ++g) npig += gt_ignore[(size_t)g * A + a] == 0;
    if (npig == 0) return;                                              // the tables keep their -1
    const int md = max_dets[m], b = cat_off[k], e = cat_off[k + 1], AT = A * T, col = a * T + t;
    long long tp = 0, fp = 0, n = 0;
    for (int i = b; i < e; ++i) {
        if (rank[i] >= md) continue;
        const unsigned f = flags[(size_t)i * AT + col];
        tp += f == 1;                                                   // matched and not ignored
        fp += f == 0;                                                   // unmatched and not ignored
        ++n;
    }
    const size_t KAM = (size_t)K * A * M, at = ((size_t)k * A + a) * M + m;
    double* q = precision + (size_t)t * R * KAM + at;                   // [T, R, K, A, M]: entry r at q[r * KAM]
    double* ss = scores + (size_t)t * R * KAM + at;
    const double rc_last = n ? (double)tp / npig : 0.0;
    recall[(size_t)t * KAM + at] = rc_last;
    int r = R - 1;
    for (; r >= 0 && (n == 0 || rec[r] > rc_last); --r) {               // searchsorted(...) >= nd: the host leaves 0
        q[r * KAM] = 0.0;
        ss[r * KAM] = 0.0;
    }
    double env = 0.0;                                                   // precision is >= 0
    for (int i = e - 1; i >= b && r >= 0; --i) {
        if (rank[i] >= md) continue;
        const unsigned f = flags[(size_t)i * AT + col];
        const double pr = (double)tp / ((double)fp + (double)tp + 2.220446049250313e-16);       // np.spacing(1) = 2^-52
        if (pr > env) env = pr;
        tp -= f == 1;
        fp -= f == 0;
        --n;
        const double rc_prev = (double)tp / npig;
        // recall thresholds whose left-sided search lands on i: rc[i] >= thr (invariant) and rc[i - 1] < thr, or i is the first
        for (; r >= 0 && (n == 0 || rc_prev < rec[r]); --r) {
            q[r * KAM] = env;
            ss[r * KAM] = (double)score[i];
        }
    }
}

int radet_coco_accumulate(const uint8_t* dt_flag_sorted, const int* dt_rank_sorted, const float* dt_score_sorted,
                          const int* dt_cat_off, const uint8_t* gt_ignore, const int* gt_cat_off, const int* max_dets,
                          const double* rec_thrs, int T, int R, int K, int A, int M, double* precision, double* recall,
                          double* scores, void* stream) {
    if (T < 1 || R < 1 || K < 0 || A < 1 || M < 1) return RADET_ERR_ARG;
    const long long n = (long long)K * A * M * T;
    if (n == 0) return RADET_OK;
    if (n > 0x7fffffffLL) return RADET_ERR_ARG;
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       dt_flag_sorted, dt_rank_sorted, dt_score_sorted, dt_cat_off, gt_ignore, gt_cat_off, max_dets, rec_thrs,
                       T, R, K, A, M, precision, recall, scores);
    return radet_check_launch();
}
