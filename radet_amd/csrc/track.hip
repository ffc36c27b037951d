// Detections tracked across frames: greedy IoU association in rank order against a constant-velocity prediction, one wave per
// sequence (camera), one launch per batch of consecutive frames.  The rules are this project's own: include/radet_hip.h,
// radet_track_update; tests/_track_ref.py restates them in NumPy and the tests pin the two bit for bit.
//
// The 256 slots of a sequence live in registers, four per lane (slot = 4 * lane + j), loaded once and stored once.  The frames
// of a batch run one after the other -- that is the dependence itself.  A frame's detections are read 64 at a time, one per
// lane; eligibility is decided for all 64 at once and a ballot leaves the eligible ones, which are visited in rank order with
// their fields broadcast by v_readlane.  Per detection: the lane-local best of four IoUs, one wave maximum over the IoU bits
// (qualifying IoUs are positive, so their bit patterns order like the floats), a ballot for the lowest lane that holds it.
// The lowest free slot is a ballot too.  No LDS, no barriers, no atomics.
#include <cmath>
#include "common.h"
#include "radet_hip.h"

struct TrackArgs {
    const float* boxes; const float* scores; const int64_t* labels; const int* counts;
    char* state; int* ids; int* hits;
    int B, cap, max_age, max_tracks, motion, class_aware;
    float iou_thr, track_thr, new_thr;
};

__device__ __forceinline__ float track_lane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ bool track_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ float track_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float track_max(float a, float b) { return a > b ? a : b; }

__global__ __launch_bounds__(64) void track_update_kernel(TrackArgs A) {
    const int lane = threadIdx.x;
    const size_t seq = blockIdx.x;
    char* st = A.state + seq * TRACK_STATE_BYTES;
    float4* s_box = (float4*)st;
    float4* s_vel = (float4*)(st + 4096);
    int4* s_label = (int4*)(st + 8192);
    int4* s_id = (int4*)(st + 9216);
    int4* s_misses = (int4*)(st + 10240);
    int4* s_hits = (int4*)(st + 11264);
    float4* s_score = (float4*)(st + 12288);
    int* s_head = (int*)(st + 13312);

    float4 box[4], vel[4], pred[4];
    int label[4], id[4], misses[4], hits[4];
    float score[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { box[j] = s_box[lane * 4 + j]; vel[j] = s_vel[lane * 4 + j]; }
    {
        const int4 l = s_label[lane], i = s_id[lane], m = s_misses[lane], h = s_hits[lane];
        const float4 s = s_score[lane];
        label[0] = l.x; label[1] = l.y; label[2] = l.z; label[3] = l.w;
        id[0] = i.x; id[1] = i.y; id[2] = i.z; id[3] = i.w;
        misses[0] = m.x; misses[1] = m.y; misses[2] = m.z; misses[3] = m.w;
        hits[0] = h.x; hits[1] = h.y; hits[2] = h.z; hits[3] = h.w;
        score[0] = s.x; score[1] = s.y; score[2] = s.z; score[3] = s.w;
    }
    int next_id = __builtin_amdgcn_readfirstlane(s_head[0]);
    int frames = __builtin_amdgcn_readfirstlane(s_head[1]);
    int refused = __builtin_amdgcn_readfirstlane(s_head[2]);
    const bool constant = A.motion == TRACK_MOTION_CONSTANT;

    for (int f = 0; f < A.B; ++f) {
        const size_t frame = seq * (size_t)A.B + f, base = frame * (size_t)A.cap;
        int cnt = __builtin_amdgcn_readfirstlane(A.counts[frame]);
        cnt = cnt < 0 ? 0 : (cnt > A.cap ? A.cap : cnt);
        // 1. predict
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pred[j] = box[j];
            if (constant) { pred[j].x = box[j].x + vel[j].x; pred[j].y = box[j].y + vel[j].y;
                            pred[j].z = box[j].z + vel[j].z; pred[j].w = box[j].w + vel[j].w; }
        }
        unsigned matched = 0;                                   // bit j: slot 4 * lane + j was matched or started in this frame
        for (int c0 = 0; c0 < A.cap; c0 += 64) {
            const int i = c0 + lane;
            int out_id = 0, out_hits = 0;
            if (c0 < cnt) {
                // 2. the 64 detections of this chunk, one per lane
                const bool have = i < cnt;
                float4 db = make_float4(0.f, 0.f, 0.f, 0.f);
                float ds = 0.f;
                long long dl = -1;
                if (have) { db = ((const float4*)A.boxes)[base + i]; ds = A.scores[base + i]; dl = A.labels[base + i]; }
                const bool elig = have && track_finite(db.x) && track_finite(db.y) && track_finite(db.z) && track_finite(db.w) &&
                                  track_finite(ds) && ds >= A.track_thr && dl >= 0 && dl < 2147483648LL;
                const float darea = (db.z - db.x) * (db.w - db.y);
                unsigned long long todo = __ballot(elig);
                while (todo) {
                    const int d = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    const float x1 = track_lane_f(db.x, d), y1 = track_lane_f(db.y, d), x2 = track_lane_f(db.z, d),
                                y2 = track_lane_f(db.w, d), sc = track_lane_f(ds, d), area_b = track_lane_f(darea, d);
                    const int lab = __builtin_amdgcn_readlane((int)dl, d);
                    // 3. match: the lane's best of four, then the wave's
                    unsigned best = 0;
                    int bj = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool cand = id[j] != 0 && !((matched >> j) & 1u) && lane * 4 + j < A.max_tracks &&
                                          (!A.class_aware || label[j] == lab);
                        const float4 p = pred[j];
                        const float iw = track_max(track_min(p.z, x2) - track_max(p.x, x1), 0.f);
                        const float ih = track_max(track_min(p.w, y2) - track_max(p.y, y1), 0.f);
                        const float inter = iw * ih;
                        const float area_a = (p.z - p.x) * (p.w - p.y);
                        const float uni = (area_a + area_b) - inter;
                        const float iou = inter / uni;
                        const unsigned bits = (cand && iou >= A.iou_thr) ? __float_as_uint(iou) : 0u;
                        if (bits > best) { best = bits; bj = j; }
                    }
                    const unsigned top = radet_amax_reduce(best);
                    int got_id = 0, got_hits = 0;
                    if (top != 0u) {
                        const int L = __builtin_ctzll(__ballot(best == top));
                        int my_id = 0, my_hits = 0;
                        if (lane == L) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                if (j != bj) continue;
                                if (constant) vel[j] = make_float4(x1 - box[j].x, y1 - box[j].y, x2 - box[j].z, y2 - box[j].w);
                                box[j] = make_float4(x1, y1, x2, y2);
                                score[j] = sc;
                                misses[j] = 0;
                                hits[j] += 1;
                                matched |= 1u << j;
                                my_id = id[j];
                                my_hits = hits[j];
                            }
                        }
                        got_id = __builtin_amdgcn_readlane(my_id, L);
                        got_hits = __builtin_amdgcn_readlane(my_hits, L);
                    } else if (sc >= A.new_thr) {
                        // 4. start a track in the lowest free slot
                        unsigned free_bits = 0;
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (id[j] == 0 && lane * 4 + j < A.max_tracks) free_bits |= 1u << j;
                        const unsigned long long free_lanes = __ballot(free_bits != 0u);
                        if (free_lanes) {
                            const int L = __builtin_ctzll(free_lanes);
                            next_id += 1;
                            if (lane == L) {
                                const int j0 = __builtin_ctz(free_bits);
#pragma unroll
                                for (int j = 0; j < 4; ++j) {
                                    if (j != j0) continue;
                                    box[j] = make_float4(x1, y1, x2, y2);
                                    vel[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                                    label[j] = lab;
                                    id[j] = next_id;
                                    score[j] = sc;
                                    hits[j] = 1;
                                    misses[j] = 0;
                                    matched |= 1u << j;
                                }
                            }
                            got_id = next_id;
                            got_hits = 1;
                        } else {
                            refused += 1;
                        }
                    }
                    if (lane == d) { out_id = got_id; out_hits = got_hits; }
                }
            }
            if (i < A.cap) { A.ids[base + i] = out_id; A.hits[base + i] = out_hits; }
        }
        // 5. age the slots nothing matched
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (id[j] != 0 && !((matched >> j) & 1u)) {
                misses[j] += 1;
                if (misses[j] > A.max_age) id[j] = 0;
                else box[j] = pred[j];
            }
        }
        frames += 1;                                            // 6.
    }

#pragma unroll
    for (int j = 0; j < 4; ++j) { s_box[lane * 4 + j] = box[j]; s_vel[lane * 4 + j] = vel[j]; }
    s_label[lane] = make_int4(label[0], label[1], label[2], label[3]);
    s_id[lane] = make_int4(id[0], id[1], id[2], id[3]);
    s_misses[lane] = make_int4(misses[0], misses[1], misses[2], misses[3]);
    s_hits[lane] = make_int4(hits[0], hits[1], hits[2], hits[3]);
    s_score[lane] = make_float4(score[0], score[1], score[2], score[3]);
    if (lane < 3) s_head[lane] = lane == 0 ? next_id : (lane == 1 ? frames : refused);
}

extern "C" size_t radet_track_state_bytes(int nseq) { return nseq < 1 ? 0 : (size_t)nseq * TRACK_STATE_BYTES; }

extern "C" int radet_track_update(const float* boxes, const float* scores, const int64_t* labels, const int* counts, int nseq,
                                  int B, int cap, void* state, float iou_thr, float track_thr, float new_thr, int max_age,
                                  int max_tracks, int motion, int class_aware, int* ids, int* hits, void* stream) {
    if (nseq < 1 || B < 1 || cap < 1 || cap > TRACK_MAX_DETS) return RADET_ERR_ARG;
    if (max_tracks < 1 || max_tracks > TRACK_MAX_TRACKS || max_age < 0) return RADET_ERR_ARG;
    if (!std::isfinite(iou_thr) || !std::isfinite(track_thr) || !std::isfinite(new_thr)) return RADET_ERR_ARG;
    if (!(iou_thr > 0.f && iou_thr <= 1.f)) return RADET_ERR_ARG;
    if ((motion != TRACK_MOTION_NONE && motion != TRACK_MOTION_CONSTANT) || (class_aware != 0 && class_aware != 1)) return RADET_ERR_ARG;
    if (!boxes || !scores || !labels || !counts || !state || !ids || !hits) return RADET_ERR_ARG;
    if (((uintptr_t)boxes & 15) || ((uintptr_t)state & 15)) return RADET_ERR_ARG;
    TrackArgs A;
    A.boxes = boxes; A.scores = scores; A.labels = labels; A.counts = counts; A.state = (char*)state; A.ids = ids; A.hits = hits;
    A.B = B; A.cap = cap; A.max_age = max_age; A.max_tracks = max_tracks; A.motion = motion; A.class_aware = class_aware;
    A.iou_thr = iou_thr; A.track_thr = track_thr; A.new_thr = new_thr;
    hipLaunchKernelGGL(track_update_kernel, dim3(nseq), dim3(64), 0, (hipStream_t)stream, A);
    return radet_check_launch();
}
