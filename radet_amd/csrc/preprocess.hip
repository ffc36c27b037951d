// Test-time preparation of in-memory frames (LoadImageFromWebcam -> Resize -> Normalize -> Pad of the reference's test
// pipeline, radet/datasets/pipelines/loading.py:88, transforms.py) in ONE launch: a batch of u8 HWC BGR frames of
// arbitrary, mixed sizes -> the network input f32 [nimg, 3, Hp, Wp].
//
// One row of PREP_DESC_INTS ints per frame (include/radet_hip.h) holds the frame's own byte address and row stride, so a
// frame that already lives on the device -- a view into a larger tensor included -- is read where it is; the source is
// read byte by byte and nothing is assumed about its alignment.  The arithmetic is the file pipeline's, from the same
// helpers (pixel_ops.h): resize_u8_kernel's taps and fixed-point blend, then aug_finish_kernel's BGR->RGB, (q - mean) *
// stdinv and zeros outside the frame's h x w -- bit-equal to radet_resize_linear_u8 -> radet_augment_finish, without the
// packed u8 temporaries and the three pass-through launches between them.  A row may ask for the flipped image
// (PREP_FLIP_H / PREP_FLIP_V, test-time augmentation): the mirror is taken inside the destination h x w, the padding stays
// on the right and at the bottom.
//
// grid (ceil(Hp * Wp / 256), nimg): one output pixel (3 planes) per thread, as aug_finish_kernel; stores along x are
// coalesced per plane.  Memory-bound: 12 source bytes (mostly shared with the neighbouring lanes) and 12 stored bytes
// per pixel.  No LDS, no scratch.
#include "common.h"
#include "pixel_ops.h"
#include "radet_hip.h"

// the addresses arrive as integers: say that they are global memory, or the compiler has to emit flat_ instructions
#define PREP_GLOBAL __attribute__((address_space(1)))

__global__ __launch_bounds__(256) void preprocess_frames_kernel(const int* __restrict__ desc, float* __restrict__ out, int Hp,
                                                                int Wp, float m0, float m1, float m2, float s0, float s1,
                                                                float s2) {
    const int* d = desc + (size_t)PREP_DESC_INTS * blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Hp * Wp) return;
    const int y = p / Wp, x = p - y * Wp;
    const size_t plane = (size_t)Hp * Wp;
    float* o = out + (size_t)blockIdx.y * 3 * plane + p;
    const int sh = d[3], sw = d[4], dh = d[5], dw = d[6];
    if (y >= dh || x >= dw || sh <= 0 || sw <= 0) {            // (a row without source pixels is all padding)
        zero_store(o, plane);
        return;
    }
    const PREP_GLOBAL uint8_t* src = (const PREP_GLOBAL uint8_t*)(((uint64_t)(uint32_t)d[1] << 32) | (uint64_t)(uint32_t)d[0]);
    const size_t stride = (size_t)(uint32_t)d[2];
    // a flipped row (mmcv.imflip of the resized image): pixel (y, x) is the unflipped row's pixel at the mirrored place
    const int fy = (d[7] & PREP_FLIP_V) ? dh - 1 - y : y, fx = (d[7] & PREP_FLIP_H) ? dw - 1 - x : x;
    const LinTaps t = lin_taps_u8(fy, fx, sh, sw, dh, dw);
    const PREP_GLOBAL uint8_t* r0 = src + (size_t)t.y0 * stride;
    const PREP_GLOBAL uint8_t* r1 = src + (size_t)t.y1 * stride;
    const size_t c0 = (size_t)t.sx * 3, c1 = (size_t)t.x1 * 3;
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = lin_blend_u8(r0[c0 + c], r0[c1 + c], r1[c0 + c], r1[c1 + c], t);
    norm_store(o, plane, v, d[7] & PREP_TO_RGB, m0, m1, m2, s0, s1, s2);
}

extern "C" int radet_preprocess_frames(const int* desc, int nimg, int Hp, int Wp, float m0, float m1, float m2, float s0,
                                       float s1, float s2, float* out, void* stream) {
    if (nimg < 0 || Hp < 0 || Wp < 0 || nimg > 65535) return RADET_ERR_ARG;
    if (nimg == 0 || Hp == 0 || Wp == 0) return RADET_OK;
    if (!desc || !out || (long long)Hp * Wp > 0x7FFFFFFFll - 255) return RADET_ERR_ARG;
    hipLaunchKernelGGL(preprocess_frames_kernel, dim3((Hp * Wp + 255) / 256, nimg), dim3(256), 0, (hipStream_t)stream, desc, out,
                       Hp, Wp, m0, m1, m2, s0, s1, s2);
    return radet_check_launch();
}
