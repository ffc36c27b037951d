// Instance-mask path feeding the visibility-guided assigner, on the GPU: nearest resize -> flip -> pad of a stack
// of u8 bitmaps in ONE pass, plus the loader's per-mask normalisation (mask / mask.max()).
// Replaces radet/core/mask/structures.py:253-303 (BitmapMasks.rescale / resize / flip / pad, i.e. mmcv.imresize
// (cv2.INTER_NEAREST) / np.flip / np.pad per mask on the host) and radet/datasets/pipelines/loading.py:419-422.
// HBM-bound byte work: every output byte is written once (4 per thread, one 32-bit store when the row allows),
// every source byte is read at most ~once (rows are walked contiguously).
// radet_rle_masks produces the same bytes from run-length annotations: no bitmap is uploaded, no maximum is taken.
#include "pixel_ops.h"

__global__ __launch_bounds__(256) void mask_max_kernel(const uint8_t* __restrict__ m, unsigned* __restrict__ mx, size_t hw) {
    const int g = blockIdx.y;
    const uint8_t* p = m + (size_t)g * hw;
    unsigned v = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (size_t)gridDim.x * 256) v = max(v, (unsigned)p[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    if ((threadIdx.x & 63) == 0 && v) atomicMax(mx + g, v);
}

// cv2.resize(INTER_NEAREST): src index = min(floor(dst index * (1 / (dst / src))), src - 1), in double
__device__ __forceinline__ int nn_src(int d, double inv, int n) {
    const int s = (int)floor((double)d * inv);
    return s < n - 1 ? s : n - 1;
}

// A mask's view row (pixel_ops.h View; masks read 0 outside the source: BitmapMasks.expand pads with zeros).  A row with bad
// geometry, or whose output window does not fit the destination, becomes an empty window: the mask is pad_val only.
__device__ __forceinline__ View load_mask_view(const int* __restrict__ view, int g, int Hd, int Wd) {
    View v;
    if (!load_view(view, g, &v) || v.h > Hd || v.w > Wd) {
        v.Hr = v.Wr = v.wh = v.ww = 1;
        v.wy0 = v.wx0 = v.oy = v.ox = v.h = v.w = 0;
    }
    return v;
}

// 4 adjacent bytes of a destination row of Wd bytes at x0 (a multiple of 4): one 32-bit store when every row is aligned
__device__ __forceinline__ void store4(uint8_t* __restrict__ row, int x0, int Wd, unsigned v) {
    if ((Wd & 3) == 0) {
        *reinterpret_cast<unsigned*>(row + x0) = v;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < Wd) row[x0 + j] = (uint8_t)(v >> (8 * j));
    }
}

// VIEW: the geometry comes per mask from `view` (the kernel arguments Hr, Wr, ify, ifx, flip are not used): nearest sampling
// over the wh x ww source window resized to Hr x Wr, each sample fetched at (wy0 + sy, wx0 + sx) of the source mask or 0
// outside it, the flip inside the h x w output window (it follows the crop).  norm_max stays the maximum of the whole
// source mask (the reference normalises at load time).  Otherwise: the whole source to the whole Hr x Wr at the origin.
template <bool VIEW>
__global__ __launch_bounds__(256) void mask_transform_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                             const unsigned* __restrict__ norm_max, const int* __restrict__ view,
                                                             int Hs, int Ws, int Hr, int Wr, int Hd, int Wd, double ify,
                                                             double ifx, int flip, int pad_val) {
    const int g = blockIdx.z, y = blockIdx.y;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= Wd) return;
    View m = {};
    if (VIEW) {
        m = load_mask_view(view, g, Hd, Wd);
        flip = m.flip & 3;
        // OpenCV computes inv_scale = dsize / ssize and then 1. / inv_scale (not ssize / dsize)
        ify = 1.0 / ((double)m.Hr / (double)m.wh); ifx = 1.0 / ((double)m.Wr / (double)m.ww);
        Hr = m.h; Wr = m.w;                                   // (from here on: the output window's size)
    }
    const uint8_t* sp = src + (size_t)g * Hs * Ws;
    const unsigned mx = norm_max ? norm_max[g] : 0u;
    unsigned out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        unsigned v = (unsigned)pad_val & 0xFFu;
        if (y < Hr && x < Wr) {
            const int yr = (flip & 2) ? Hr - 1 - y : y;       // flip acts on the resized image
            const int xr = (flip & 1) ? Wr - 1 - x : x;
            if (VIEW) {
                const int sy = m.wy0 + nn_src(m.oy + yr, ify, m.wh), sx = m.wx0 + nn_src(m.ox + xr, ifx, m.ww);
                v = ((unsigned)sy < (unsigned)Hs && (unsigned)sx < (unsigned)Ws) ? sp[(size_t)sy * Ws + sx] : 0u;
            } else {
                v = sp[(size_t)nn_src(yr, ify, Hs) * Ws + nn_src(xr, ifx, Ws)];
            }
            // (mask / mask.max()).astype(u8): 1 where the value equals the mask's maximum, else 0; an all-zero mask
            // is 0 / 0 = NaN -> 0 after the cast
            if (norm_max) v = (mx != 0u && v == mx) ? 1u : 0u;
        }
        out |= v << (8 * j);
    }
    store4(dst + ((size_t)g * Hd + y) * Wd, x0, Wd, out);
}

// Number of run ends <= p among ends[lo, n) (ends ascending): the index of the run that holds position p.
__device__ __forceinline__ int rle_run_of(const uint32_t* __restrict__ ends, int lo, int n, uint32_t p) {
    int hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ends[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One workgroup per destination row of one mask.  A thread owns 4 adjacent pixels: their source positions sx * Hs + sy
// ascend with x, so each part is searched once (binary, over its run ends) and the search for the next pixel starts at the
// run found last -- one compare when it is the same run.  The packed row goes to LDS; from there the mirrored copy is
// composed, so both orientations leave as aligned 32-bit stores and the runs are looked up once.
// VIEW: per mask the geometry of its `view` row (as above; its flip word is not read, the flip is mask_desc's); the mirrored
// copy is composed inside the output window.  A sample that falls outside the source image decodes as 0 -- it is not
// looked up, so it cannot land in a neighbouring column's run; the positions that are looked up still ascend with x.
#define RLE_MAX_W 8192
template <bool VIEW>
__global__ __launch_bounds__(256) void rle_masks_kernel(const uint32_t* __restrict__ run_ends, int n_ends,
                                                        const int* __restrict__ part_desc, int n_parts,
                                                        const int* __restrict__ mask_desc, const int* __restrict__ view,
                                                        uint8_t* __restrict__ dst, uint8_t* __restrict__ dst_plain, int Hr,
                                                        int Wr, int Hd, int Wd, int pad_val) {
    __shared__ unsigned row[RLE_MAX_W / 4 + 1];
    const int g = blockIdx.y, y = blockIdx.x;
    const int* md = mask_desc + (size_t)g * RLE_MASK_INTS;
    const int first = md[0], Hs = md[2], Ws = md[3], flip = md[4] & 1;
    int np = md[1];
    if (first < 0 || np < 0 || first > n_parts - np || Hs <= 0 || Ws <= 0) np = 0;         // (a row that points outside the part table: no parts)
    View m = {Hr, Wr, 0, 0, Hs, Ws, 0, 0, Hr, Wr, 0, 0u};
    if (VIEW) m = load_mask_view(view, g, Hd, Wd);
    // OpenCV computes inv_scale = dsize / ssize and then 1. / inv_scale (not ssize / dsize)
    const double ify = 1.0 / ((double)m.Hr / (double)m.wh), ifx = 1.0 / ((double)m.Wr / (double)m.ww);
    Hr = m.h; Wr = m.w;                                           // (from here on: the output window's size)
    const unsigned pad = (unsigned)pad_val & 0xFFu;
    const int nwords = (Wd + 3) >> 2;
    const bool inside = y < Hr;
    const int sy = inside ? m.wy0 + nn_src(m.oy + y, ify, m.wh) : 0;
    const bool row_in = np > 0 && (unsigned)sy < (unsigned)Hs;   // (only VIEW can leave the source)
    for (int wd = threadIdx.x; wd < nwords; wd += blockDim.x) {
        const int x0 = wd * 4;
        unsigned out[4] = {pad, pad, pad, pad};
        if (inside && x0 < Wr) {
            uint32_t pos[4];
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                out[j] = x0 + j < Wr ? 0u : pad;
                const int sx = m.wx0 + nn_src(m.ox + min(x0 + j, Wr - 1), ifx, m.ww);
                ok[j] = x0 + j < Wr && (!VIEW || (row_in && (unsigned)sx < (unsigned)Ws));
                pos[j] = !VIEW || ok[j] ? (uint32_t)sx * (uint32_t)Hs + (uint32_t)sy : 0u;
            }
            for (int k = 0; k < np; ++k) {
                const int off = part_desc[(size_t)(first + k) * RLE_PART_INTS], n = part_desc[(size_t)(first + k) * RLE_PART_INTS + 1];
                if (off < 0 || n <= 0 || off > n_ends - n) continue;
                const uint32_t* e = run_ends + off;
                int r = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (VIEW && !ok[j]) continue;
                    if (r < n && e[r] <= pos[j]) r = rle_run_of(e, r + 1, n, pos[j]);
                    if (ok[j]) out[j] |= (unsigned)r & 1u;
                }
            }
        }
        row[wd] = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
    }
    __syncthreads();
    const uint8_t* rb = reinterpret_cast<const uint8_t*>(row);
    uint8_t* dp = dst + ((size_t)g * Hd + y) * Wd;
    uint8_t* pp = (dst_plain && flip) ? dst_plain + ((size_t)g * Hd + y) * Wd : nullptr;
    for (int wd = threadIdx.x; wd < nwords; wd += blockDim.x) {
        const int x0 = wd * 4;
        unsigned v = row[wd];
        if (pp) store4(pp, x0, Wd, v);
        if (flip && inside) {                                        // flip acts on the resized image; the pad stays right
            v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + j;
                v |= (unsigned)(x < Wr ? rb[Wr - 1 - x] : (uint8_t)pad) << (8 * j);
            }
        }
        store4(dp, x0, Wd, v);
    }
}

extern "C" int radet_mask_max(const uint8_t* masks, uint32_t* maxes, int G, size_t hw, void* stream) {
    if (G <= 0 || hw == 0) return RADET_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(maxes, 0, sizeof(uint32_t) * G, st) != hipSuccess) return RADET_ERR_LAUNCH;
    int bx = (int)((hw + 256 * 16 - 1) / (256 * 16));
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(mask_max_kernel, dim3(bx, G), dim3(256), 0, st, masks, maxes, hw);
    return radet_check_launch();
}

extern "C" int radet_mask_transform(const uint8_t* src, uint8_t* dst, const uint32_t* norm_max, const int* view_desc, int G, int Hs,
                                    int Ws, int Hr, int Wr, int Hd, int Wd, int flip, int pad_val, void* stream) {
    if (G <= 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0 || Hd > 65535) return RADET_ERR_ARG;
    const dim3 grid((Wd + 1023) / 1024, Hd, G);
    if (view_desc) {
        hipLaunchKernelGGL(mask_transform_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, norm_max, view_desc, Hs, Ws,
                           0, 0, Hd, Wd, 0.0, 0.0, 0, pad_val);
        return radet_check_launch();
    }
    if (Hr <= 0 || Wr <= 0 || Hd < Hr || Wd < Wr || flip < 0 || flip > 3) return RADET_ERR_ARG;
    // OpenCV computes inv_scale = dsize / ssize and then 1. / inv_scale (not ssize / dsize)
    const double ify = 1.0 / ((double)Hr / (double)Hs), ifx = 1.0 / ((double)Wr / (double)Ws);
    hipLaunchKernelGGL(mask_transform_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, dst, norm_max, view_desc, Hs, Ws, Hr,
                       Wr, Hd, Wd, ify, ifx, flip, pad_val);
    return radet_check_launch();
}

extern "C" int radet_rle_masks(const uint32_t* run_ends, int n_ends, const int* part_desc, int n_parts, const int* mask_desc,
                               const int* view_desc, int G, uint8_t* dst, uint8_t* dst_plain, int Hr, int Wr, int Hd, int Wd,
                               int pad_val, void* stream) {
    if (G <= 0 || G > 65535 || n_ends < 0 || n_parts < 0 || Hd <= 0 || Wd <= 0 || Wd > RLE_MAX_W) return RADET_ERR_ARG;
    if (!view_desc && (Hr <= 0 || Wr <= 0 || Hd < Hr || Wd < Wr)) return RADET_ERR_ARG;
    const int nwords = (Wd + 3) / 4;
    const int threads = nwords >= 256 ? 256 : ((nwords + 63) / 64) * 64;
    if (view_desc)
        hipLaunchKernelGGL(rle_masks_kernel<true>, dim3(Hd, G), dim3(threads), 0, (hipStream_t)stream, run_ends, n_ends, part_desc,
                           n_parts, mask_desc, view_desc, dst, dst_plain, 0, 0, Hd, Wd, pad_val);
    else
        hipLaunchKernelGGL(rle_masks_kernel<false>, dim3(Hd, G), dim3(threads), 0, (hipStream_t)stream, run_ends, n_ends, part_desc,
                           n_parts, mask_desc, view_desc, dst, dst_plain, Hr, Wr, Hd, Wd, pad_val);
    return radet_check_launch();
}
