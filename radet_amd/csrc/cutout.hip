// CutOut (radet/datasets/pipelines/transforms.py:1734-1804: `img[y1:y2, x1:x2, :] = fill_in` per hole) for a batch of
// images in ONE launch, in place: radet_cutout_u8 on the packed u8 HWC BGR buffer the resize, the warp and the
// augmentation kernels share (a CutOut in the block after Resize), radet_cutout_f32 on the finished f32 [B, 3, Hp, Wp]
// batch (a CutOut behind the photometric stages: the holes keep fill_in through the Pillow blends, which run inside
// radet_augment_finish, so they are cut after it and hold what finish writes for a u8 pixel equal to the fill with no
// blend active -- the same norm_store, the same operands).
//
// One row of CUTOUT_DESC_INTS ints per image and one table of hole rectangles {x1, y1, x2, y2} (half open, unflipped
// image coordinates) for the whole batch (include/radet_hip.h).  grid (ceil(largest hole area / 256), most holes of any
// image, images): one thread per hole pixel, so the work follows the hole area, not the image area.  Every rectangle is
// clipped to its image here again; a row whose image would leave its buffer, or whose holes would leave the table,
// stores nothing (as radet_warp_affine_u8).  Overlapping holes of one image store identical bytes, so their order does
// not matter.  Bytes outside the holes are never written.  Pure stores, memory-bound: 3 bytes (u8) or 3 dwords (f32) per
// thread.  No LDS, no scratch.
#include "common.h"
#include "pixel_ops.h"
#include "../../include/radet_hip.h"

struct CutHole { int x1, y1, w, h; };             // the clipped rectangle: origin and extent (w, h <= 0: nothing to store)

// hole blockIdx.y of the image of row d, clipped to the h x w image; false for a row or hole that stores nothing
__device__ __forceinline__ bool cut_hole(const int* __restrict__ d, const int* __restrict__ holes, int nholes, CutHole* r) {
    const int h = d[CUTOUT_DESC_H], w = d[CUTOUT_DESC_W], first = d[CUTOUT_DESC_FIRST], count = d[CUTOUT_DESC_COUNT];
    if ((d[CUTOUT_DESC_FLAGS] & CUTOUT_SKIP) || h <= 0 || w <= 0 || count <= 0 || first < 0) return false;
    if ((long long)first + count > nholes) return false;          // (a row whose holes leave the table is not touched)
    if ((int)blockIdx.y >= count) return false;
    const int* q = holes + 4 * ((size_t)first + blockIdx.y);
    // (all four into [0, w] / [0, h]: the differences cannot overflow whatever the table holds)
    const int x1 = min(max(q[0], 0), w), y1 = min(max(q[1], 0), h), x2 = max(min(q[2], w), 0), y2 = max(min(q[3], h), 0);
    r->x1 = x1; r->y1 = y1; r->w = x2 - x1; r->h = y2 - y1;
    return r->w > 0 && r->h > 0;
}

__global__ __launch_bounds__(256) void cutout_u8_kernel(uint8_t* __restrict__ img, long long img_px, const int* __restrict__ desc,
                                                        const int* __restrict__ holes, int nholes) {
    const int* d = desc + (size_t)CUTOUT_DESC_INTS * blockIdx.z;
    CutHole r;
    if (!cut_hole(d, holes, nholes, &r)) return;
    const int off = d[CUTOUT_DESC_OFF], w = d[CUTOUT_DESC_W];
    if (off < 0 || (long long)off + (long long)d[CUTOUT_DESC_H] * w > img_px) return;      // (the image leaves the buffer)
    const unsigned p = blockIdx.x * 256u + threadIdx.x;             // (< 2^31: the host bounds the grid by max_area)
    if ((long long)p >= (long long)r.w * r.h) return;
    const int yy = (int)(p / (unsigned)r.w), xx = (int)(p - (unsigned)yy * (unsigned)r.w);
    uint8_t* o = img + ((size_t)off + (size_t)(r.y1 + yy) * w + (size_t)(r.x1 + xx)) * 3;
    const unsigned fill = (unsigned)d[CUTOUT_DESC_FILL];
    o[0] = (uint8_t)(fill & 0xFFu);
    o[1] = (uint8_t)((fill >> 8) & 0xFFu);
    o[2] = (uint8_t)((fill >> 16) & 0xFFu);
}

__global__ __launch_bounds__(256) void cutout_f32_kernel(float* __restrict__ out, int nbatch, int Hp, int Wp,
                                                         const int* __restrict__ desc, const int* __restrict__ holes, int nholes,
                                                         float m0, float m1, float m2, float s0, float s1, float s2) {
    const int* d = desc + (size_t)CUTOUT_DESC_INTS * blockIdx.z;
    CutHole r;
    if (!cut_hole(d, holes, nholes, &r)) return;
    const int n = d[CUTOUT_DESC_OFF], w = d[CUTOUT_DESC_W];
    if (n < 0 || n >= nbatch || d[CUTOUT_DESC_H] > Hp || w > Wp) return;                     // (the image leaves the batch)
    const unsigned p = blockIdx.x * 256u + threadIdx.x;             // (< 2^31: the host bounds the grid by max_area)
    if ((long long)p >= (long long)r.w * r.h) return;
    const int yy = (int)(p / (unsigned)r.w), xx = (int)(p - (unsigned)yy * (unsigned)r.w);
    // a flipped sample: finish wrote source column c to column w - 1 - c, so the hole's columns x1 .. x2 - 1 lie at
    // w - x2 .. w - x1 - 1
    const int x0 = (d[CUTOUT_DESC_FLAGS] & CUTOUT_FLIP) ? w - (r.x1 + r.w) : r.x1;
    const size_t plane = (size_t)Hp * Wp;
    float* o = out + (size_t)n * 3 * plane + (size_t)(r.y1 + yy) * Wp + (size_t)(x0 + xx);
    const unsigned fill = (unsigned)d[CUTOUT_DESC_FILL];
    const int v[3] = {(int)(fill & 0xFFu), (int)((fill >> 8) & 0xFFu), (int)((fill >> 16) & 0xFFu)};
    norm_store(o, plane, v, d[CUTOUT_DESC_FLAGS] & CUTOUT_TO_RGB, m0, m1, m2, s0, s1, s2);
}

static int cutout_args(const void* buf, const int* desc, int nimg, const int* holes, int nholes, int max_holes, int max_area) {
    if (nimg < 0 || nholes < 0 || max_holes < 0 || max_area < 0 || nimg > 65535 || max_holes > 65535) return RADET_ERR_ARG;
    if (nimg == 0 || nholes == 0 || max_holes == 0 || max_area == 0) return RADET_OK;
    if (!buf || !desc || !holes || ((uintptr_t)desc & 3) || ((uintptr_t)holes & 3) || max_area > 0x7FFFFFFF - 255) return RADET_ERR_ARG;
    return 1;                                                       // (launch)
}

extern "C" int radet_cutout_u8(uint8_t* img, size_t img_px, const int* desc, int nimg, const int* holes, int nholes, int max_holes,
                               int max_area, int channels, void* stream) {
    if (channels != 3) return RADET_ERR_ARG;
    const int rc = cutout_args(img, desc, nimg, holes, nholes, max_holes, max_area);
    if (rc != 1) return rc;
    if (img_px > 0x7FFFFFFFull) return RADET_ERR_ARG;               // (pixel offsets are ints)
    hipLaunchKernelGGL(cutout_u8_kernel, dim3((max_area + 255) / 256, max_holes, nimg), dim3(256), 0, (hipStream_t)stream, img,
                       (long long)img_px, desc, holes, nholes);
    return radet_check_launch();
}

extern "C" int radet_cutout_f32(float* out, int nbatch, int Hp, int Wp, const int* desc, int nimg, const int* holes, int nholes,
                                int max_holes, int max_area, float m0, float m1, float m2, float s0, float s1, float s2,
                                void* stream) {
    if (nbatch < 0 || Hp < 0 || Wp < 0) return RADET_ERR_ARG;
    const int rc = cutout_args(out, desc, nimg, holes, nholes, max_holes, max_area);
    if (rc != 1) return rc;
    if (nbatch == 0 || Hp == 0 || Wp == 0) return RADET_OK;
    hipLaunchKernelGGL(cutout_f32_kernel, dim3((max_area + 255) / 256, max_holes, nimg), dim3(256), 0, (hipStream_t)stream, out,
                       nbatch, Hp, Wp, desc, holes, nholes, m0, m1, m2, s0, s1, s2);
    return radet_check_launch();
}
