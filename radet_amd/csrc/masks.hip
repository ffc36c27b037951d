// Instance-mask path feeding the visibility-guided assigner, on the GPU: nearest resize -> flip -> pad of a stack
// of u8 bitmaps in ONE pass, plus the loader's per-mask normalisation (mask / mask.max()).
// Replaces radet/core/mask/structures.py:253-303 (BitmapMasks.rescale / resize / flip / pad, i.e. mmcv.imresize
// (cv2.INTER_NEAREST) / np.flip / np.pad per mask on the host) and radet/datasets/pipelines/loading.py:419-422.
// HBM-bound byte work: every output byte is written once (4 per thread, one 32-bit store when the row allows),
// every source byte is read at most ~once (rows are walked contiguously).
// radet_rle_masks produces the same bytes from run-length annotations: no bitmap is uploaded, no maximum is taken.
#include "common.h"
#include "radet_hip.h"

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

// A window row (WIN, include/radet_hip.h MASK_WIN_INTS) of mask g: {Hr, Wr, oy, ox, h, w, flip}.  The h x w window at
// (oy, ox) of the virtual Hr x Wr resized mask; a window that does not lie inside its virtual mask or the destination is empty.
struct MaskWin { int Hr, Wr, oy, ox, h, w, flip; };

__device__ __forceinline__ MaskWin load_mask_win(const int* __restrict__ win, int g, int Hd, int Wd) {
    const int* d = win + (size_t)g * MASK_WIN_INTS;
    MaskWin m = {d[0], d[1], d[2], d[3], d[4], d[5], d[6]};
    if (m.Hr <= 0 || m.Wr <= 0 || m.oy < 0 || m.ox < 0 || m.h < 0 || m.w < 0 || m.h > Hd || m.w > Wd || m.oy > m.Hr - m.h ||
        m.ox > m.Wr - m.w) {
        m.Hr = m.Wr = 1;
        m.oy = m.ox = m.h = m.w = 0;
    }
    return m;
}

// WIN: the resized geometry comes per mask from `win` (the kernel arguments Hr, Wr, ify, ifx, flip are not used) and the
// flip acts inside the window; otherwise the window is the whole resized mask at the origin.
template <bool WIN>
__global__ __launch_bounds__(256) void mask_transform_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                             const unsigned* __restrict__ norm_max, const int* __restrict__ win,
                                                             int Hs, int Ws, int Hr, int Wr, int Hd, int Wd, double ify,
                                                             double ifx, int flip, int pad_val) {
    const int g = blockIdx.z, y = blockIdx.y;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= Wd) return;
    int oy = 0, ox = 0;
    if (WIN) {
        const MaskWin m = load_mask_win(win, g, Hd, Wd);
        oy = m.oy; ox = m.ox; flip = m.flip & 3;
        ify = 1.0 / ((double)m.Hr / (double)Hs); ifx = 1.0 / ((double)m.Wr / (double)Ws);
        Hr = m.h; Wr = m.w;                                   // (from here on: the window's size)
    }
    const uint8_t* sp = src + (size_t)g * Hs * Ws;
    const unsigned mx = norm_max ? norm_max[g] : 0u;
    unsigned out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        unsigned v = (unsigned)pad_val & 0xFFu;
        if (y < Hr && x < Wr) {
            const int yr = (flip & 2) ? Hr - 1 - y : y;       // flip acts on the resized image
            const int xr = (flip & 1) ? Wr - 1 - x : x;
            v = sp[(size_t)nn_src(oy + yr, ify, Hs) * Ws + nn_src(ox + xr, ifx, Ws)];
            // (mask / mask.max()).astype(u8): 1 where the value equals the mask's maximum, else 0; an all-zero mask
            // is 0 / 0 = NaN -> 0 after the cast
            if (norm_max) v = (mx != 0u && v == mx) ? 1u : 0u;
        }
        out[j] = v;
    }
    uint8_t* dp = dst + ((size_t)g * Hd + y) * Wd + x0;
    if ((Wd & 3) == 0) {
        *reinterpret_cast<unsigned*>(dp) = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < Wd) dp[j] = (uint8_t)out[j];
    }
}

// A source-window row (include/radet_hip.h MASK_SRC_WIN_INTS) of mask g: {Hr, Wr, wy0, wx0, wh, ww, flip}.  The mask that
// is resized to Hr x Wr is the wh x ww window at (wy0, wx0) of the source mask in the source's coordinates (Expand /
// MinIoURandomCrop in front of Resize); the window may overhang the source, what lies outside is 0 (BitmapMasks.expand
// pads with zeros).  A row without a window, or whose Hr x Wr does not fit the destination, is empty.
struct MaskSrcWin { int Hr, Wr, wy0, wx0, wh, ww, flip; };

__device__ __forceinline__ MaskSrcWin load_mask_src_win(const int* __restrict__ win, int g, int Hd, int Wd) {
    const int* d = win + (size_t)g * MASK_SRC_WIN_INTS;
    MaskSrcWin m = {d[0], d[1], d[2], d[3], d[4], d[5], d[6]};
    if (m.Hr <= 0 || m.Wr <= 0 || m.Hr > Hd || m.Wr > Wd || m.wh <= 0 || m.ww <= 0 || (long long)m.wy0 + m.wh > 0x7FFFFFFFLL ||
        (long long)m.wx0 + m.ww > 0x7FFFFFFFLL) {
        m.Hr = m.Wr = 0;
        m.wy0 = m.wx0 = 0;
        m.wh = m.ww = 1;
    }
    return m;
}

// mask_transform_kernel over source windows: nearest sampling over the wh x ww window grid, each sample fetched at
// (wy0 + sy, wx0 + sx) of the source mask or 0 outside it; norm_max stays the maximum of the whole source mask (the
// reference normalises at load time, before Expand); flip and pad as there.
__global__ __launch_bounds__(256) void mask_transform_src_window_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                        const unsigned* __restrict__ norm_max,
                                                                        const int* __restrict__ win, int Hs, int Ws, int Hd, int Wd,
                                                                        int pad_val) {
    const int g = blockIdx.z, y = blockIdx.y;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= Wd) return;
    const MaskSrcWin m = load_mask_src_win(win, g, Hd, Wd);
    const int Hr = m.Hr, Wr = m.Wr, flip = m.flip & 3;
    // OpenCV computes inv_scale = dsize / ssize and then 1. / inv_scale (not ssize / dsize)
    const double ify = Hr > 0 ? 1.0 / ((double)Hr / (double)m.wh) : 0.0, ifx = Wr > 0 ? 1.0 / ((double)Wr / (double)m.ww) : 0.0;
    const uint8_t* sp = src + (size_t)g * Hs * Ws;
    const unsigned mx = norm_max ? norm_max[g] : 0u;
    unsigned out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        unsigned v = (unsigned)pad_val & 0xFFu;
        if (y < Hr && x < Wr) {
            const int yr = (flip & 2) ? Hr - 1 - y : y;       // flip acts on the resized image
            const int xr = (flip & 1) ? Wr - 1 - x : x;
            const int sy = m.wy0 + nn_src(yr, ify, m.wh), sx = m.wx0 + nn_src(xr, ifx, m.ww);
            v = ((unsigned)sy < (unsigned)Hs && (unsigned)sx < (unsigned)Ws) ? sp[(size_t)sy * Ws + sx] : 0u;
            if (norm_max) v = (mx != 0u && v == mx) ? 1u : 0u;
        }
        out[j] = v;
    }
    uint8_t* dp = dst + ((size_t)g * Hd + y) * Wd + x0;
    if ((Wd & 3) == 0) {
        *reinterpret_cast<unsigned*>(dp) = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < Wd) dp[j] = (uint8_t)out[j];
    }
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
// WIN: per mask the h x w window at (oy, ox) of its virtual resized mask (`win`, as above; its flip word is not read, the
// flip is mask_desc's); the mirrored copy is composed inside the window.
#define RLE_MAX_W 8192
template <bool WIN>
__global__ __launch_bounds__(256) void rle_masks_kernel(const uint32_t* __restrict__ run_ends, int n_ends,
                                                        const int* __restrict__ part_desc, int n_parts,
                                                        const int* __restrict__ mask_desc, const int* __restrict__ win,
                                                        uint8_t* __restrict__ dst, uint8_t* __restrict__ dst_plain, int Hr,
                                                        int Wr, int Hd, int Wd, int pad_val) {
    __shared__ unsigned row[RLE_MAX_W / 4 + 1];
    const int g = blockIdx.y, y = blockIdx.x;
    const int* md = mask_desc + (size_t)g * RLE_MASK_INTS;
    const int first = md[0], Hs = md[2], Ws = md[3], flip = md[4] & 1;
    int np = md[1];
    if (first < 0 || np < 0 || first > n_parts - np || Hs <= 0 || Ws <= 0) np = 0;         // (a row that points outside the part table: no parts)
    int oy = 0, ox = 0, wh = Hr, ww = Wr;
    if (WIN) {
        const MaskWin m = load_mask_win(win, g, Hd, Wd);
        oy = m.oy; ox = m.ox; wh = m.h; ww = m.w;
        Hr = m.Hr; Wr = m.Wr;
    }
    // OpenCV computes inv_scale = dsize / ssize and then 1. / inv_scale (not ssize / dsize)
    const double ify = 1.0 / ((double)Hr / (double)Hs), ifx = 1.0 / ((double)Wr / (double)Ws);
    Hr = wh; Wr = ww;                                             // (from here on: the window's size)
    const unsigned pad = (unsigned)pad_val & 0xFFu;
    const int nwords = (Wd + 3) >> 2;
    const bool inside = y < Hr;
    const uint32_t sy = inside ? (uint32_t)nn_src(oy + y, ify, Hs) : 0u;
    for (int wd = threadIdx.x; wd < nwords; wd += blockDim.x) {
        const int x0 = wd * 4;
        unsigned out[4] = {pad, pad, pad, pad};
        if (inside && x0 < Wr) {
            uint32_t pos[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                out[j] = x0 + j < Wr ? 0u : pad;
                pos[j] = (uint32_t)nn_src(ox + min(x0 + j, Wr - 1), ifx, Ws) * (uint32_t)Hs + sy;
            }
            for (int k = 0; k < np; ++k) {
                const int off = part_desc[(size_t)(first + k) * RLE_PART_INTS], n = part_desc[(size_t)(first + k) * RLE_PART_INTS + 1];
                if (off < 0 || n <= 0 || off > n_ends - n) continue;
                const uint32_t* e = run_ends + off;
                int r = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (r < n && e[r] <= pos[j]) r = rle_run_of(e, r + 1, n, pos[j]);
                    if (x0 + j < Wr) out[j] |= (unsigned)r & 1u;
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
        if (pp) {
            if ((Wd & 3) == 0) {
                *reinterpret_cast<unsigned*>(pp + x0) = v;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j < Wd) pp[x0 + j] = (uint8_t)(v >> (8 * j));
            }
        }
        if (flip && inside) {                                        // flip acts on the resized image; the pad stays right
            v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + j;
                v |= (unsigned)(x < Wr ? rb[Wr - 1 - x] : (uint8_t)pad) << (8 * j);
            }
        }
        if ((Wd & 3) == 0) {
            *reinterpret_cast<unsigned*>(dp + x0) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < Wd) dp[x0 + j] = (uint8_t)(v >> (8 * j));
        }
    }
}

// rle_masks_kernel over source windows (`win` rows as for mask_transform_src_window_kernel; the flip is mask_desc's): a
// sample that falls outside the source image decodes as 0 -- it is not looked up, so it cannot land in a neighbouring
// column's run.  The positions of the samples that are looked up still ascend with x.
__global__ __launch_bounds__(256) void rle_masks_src_window_kernel(const uint32_t* __restrict__ run_ends, int n_ends,
                                                                   const int* __restrict__ part_desc, int n_parts,
                                                                   const int* __restrict__ mask_desc, const int* __restrict__ win,
                                                                   uint8_t* __restrict__ dst, uint8_t* __restrict__ dst_plain,
                                                                   int Hd, int Wd, int pad_val) {
    __shared__ unsigned row[RLE_MAX_W / 4 + 1];
    const int g = blockIdx.y, y = blockIdx.x;
    const int* md = mask_desc + (size_t)g * RLE_MASK_INTS;
    const int first = md[0], Hs = md[2], Ws = md[3], flip = md[4] & 1;
    int np = md[1];
    if (first < 0 || np < 0 || first > n_parts - np || Hs <= 0 || Ws <= 0) np = 0;         // (a row that points outside the part table: no parts)
    const MaskSrcWin m = load_mask_src_win(win, g, Hd, Wd);
    const int Hr = m.Hr, Wr = m.Wr;
    const double ify = Hr > 0 ? 1.0 / ((double)Hr / (double)m.wh) : 0.0, ifx = Wr > 0 ? 1.0 / ((double)Wr / (double)m.ww) : 0.0;
    const unsigned pad = (unsigned)pad_val & 0xFFu;
    const int nwords = (Wd + 3) >> 2;
    const bool inside = y < Hr;
    const int sy = inside ? m.wy0 + nn_src(y, ify, m.wh) : -1;
    const bool row_in = np > 0 && (unsigned)sy < (unsigned)Hs;
    for (int wd = threadIdx.x; wd < nwords; wd += blockDim.x) {
        const int x0 = wd * 4;
        unsigned out[4] = {pad, pad, pad, pad};
        if (inside && x0 < Wr) {
            uint32_t pos[4];
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                out[j] = x0 + j < Wr ? 0u : pad;
                const int sx = m.wx0 + nn_src(min(x0 + j, Wr - 1), ifx, m.ww);
                ok[j] = row_in && x0 + j < Wr && (unsigned)sx < (unsigned)Ws;
                pos[j] = ok[j] ? (uint32_t)sx * (uint32_t)Hs + (uint32_t)sy : 0u;
            }
            for (int k = 0; k < np; ++k) {
                const int off = part_desc[(size_t)(first + k) * RLE_PART_INTS], n = part_desc[(size_t)(first + k) * RLE_PART_INTS + 1];
                if (off < 0 || n <= 0 || off > n_ends - n) continue;
                const uint32_t* e = run_ends + off;
                int r = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!ok[j]) continue;
                    if (r < n && e[r] <= pos[j]) r = rle_run_of(e, r + 1, n, pos[j]);
                    out[j] |= (unsigned)r & 1u;
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
        if (pp) {
            if ((Wd & 3) == 0) {
                *reinterpret_cast<unsigned*>(pp + x0) = v;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j < Wd) pp[x0 + j] = (uint8_t)(v >> (8 * j));
            }
        }
        if (flip && inside) {                                        // flip acts on the resized image; the pad stays right
            v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + j;
                v |= (unsigned)(x < Wr ? rb[Wr - 1 - x] : (uint8_t)pad) << (8 * j);
            }
        }
        if ((Wd & 3) == 0) {
            *reinterpret_cast<unsigned*>(dp + x0) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < Wd) dp[x0 + j] = (uint8_t)(v >> (8 * j));
        }
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

extern "C" int radet_mask_transform(const uint8_t* src, uint8_t* dst, const uint32_t* norm_max, int G, int Hs, int Ws,
                                    int Hr, int Wr, int Hd, int Wd, int flip, int pad_val, void* stream) {
    if (G <= 0 || Hs <= 0 || Ws <= 0 || Hr <= 0 || Wr <= 0 || Hd < Hr || Wd < Wr || flip < 0 || flip > 3 || Hd > 65535)
        return RADET_ERR_ARG;
    // OpenCV computes inv_scale = dsize / ssize and then 1. / inv_scale (not ssize / dsize)
    const double ify = 1.0 / ((double)Hr / (double)Hs), ifx = 1.0 / ((double)Wr / (double)Ws);
    hipLaunchKernelGGL(mask_transform_kernel<false>, dim3((Wd + 1023) / 1024, Hd, G), dim3(256), 0, (hipStream_t)stream, src, dst,
                       norm_max, (const int*)nullptr, Hs, Ws, Hr, Wr, Hd, Wd, ify, ifx, flip, pad_val);
    return radet_check_launch();
}

extern "C" int radet_mask_transform_window(const uint8_t* src, uint8_t* dst, const uint32_t* norm_max, const int* win_desc, int G,
                                           int Hs, int Ws, int Hd, int Wd, int pad_val, void* stream) {
    if (G <= 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0 || Hd > 65535 || !win_desc) return RADET_ERR_ARG;
    hipLaunchKernelGGL(mask_transform_kernel<true>, dim3((Wd + 1023) / 1024, Hd, G), dim3(256), 0, (hipStream_t)stream, src, dst,
                       norm_max, win_desc, Hs, Ws, 0, 0, Hd, Wd, 0.0, 0.0, 0, pad_val);
    return radet_check_launch();
}

extern "C" int radet_rle_masks(const uint32_t* run_ends, int n_ends, const int* part_desc, int n_parts, const int* mask_desc,
                               int G, uint8_t* dst, uint8_t* dst_plain, int Hr, int Wr, int Hd, int Wd, int pad_val,
                               void* stream) {
    if (G <= 0 || G > 65535 || n_ends < 0 || n_parts < 0 || Hr <= 0 || Wr <= 0 || Hd < Hr || Wd < Wr || Wd > RLE_MAX_W)
        return RADET_ERR_ARG;
    const int nwords = (Wd + 3) / 4;
    const int threads = nwords >= 256 ? 256 : ((nwords + 63) / 64) * 64;
    hipLaunchKernelGGL(rle_masks_kernel<false>, dim3(Hd, G), dim3(threads), 0, (hipStream_t)stream, run_ends, n_ends, part_desc,
                       n_parts, mask_desc, (const int*)nullptr, dst, dst_plain, Hr, Wr, Hd, Wd, pad_val);
    return radet_check_launch();
}

extern "C" int radet_rle_masks_window(const uint32_t* run_ends, int n_ends, const int* part_desc, int n_parts, const int* mask_desc,
                                      const int* win_desc, int G, uint8_t* dst, uint8_t* dst_plain, int Hd, int Wd, int pad_val,
                                      void* stream) {
    if (G <= 0 || G > 65535 || n_ends < 0 || n_parts < 0 || Hd <= 0 || Wd <= 0 || Wd > RLE_MAX_W || !win_desc) return RADET_ERR_ARG;
    const int nwords = (Wd + 3) / 4;
    const int threads = nwords >= 256 ? 256 : ((nwords + 63) / 64) * 64;
    hipLaunchKernelGGL(rle_masks_kernel<true>, dim3(Hd, G), dim3(threads), 0, (hipStream_t)stream, run_ends, n_ends, part_desc,
                       n_parts, mask_desc, win_desc, dst, dst_plain, 0, 0, Hd, Wd, pad_val);
    return radet_check_launch();
}

extern "C" int radet_mask_transform_src_window(const uint8_t* src, uint8_t* dst, const uint32_t* norm_max, const int* win_desc, int G,
                                               int Hs, int Ws, int Hd, int Wd, int pad_val, void* stream) {
    if (G <= 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0 || Hd > 65535 || !win_desc) return RADET_ERR_ARG;
    hipLaunchKernelGGL(mask_transform_src_window_kernel, dim3((Wd + 1023) / 1024, Hd, G), dim3(256), 0, (hipStream_t)stream, src, dst,
                       norm_max, win_desc, Hs, Ws, Hd, Wd, pad_val);
    return radet_check_launch();
}

extern "C" int radet_rle_masks_src_window(const uint32_t* run_ends, int n_ends, const int* part_desc, int n_parts,
                                          const int* mask_desc, const int* win_desc, int G, uint8_t* dst, uint8_t* dst_plain, int Hd,
                                          int Wd, int pad_val, void* stream) {
    if (G <= 0 || G > 65535 || n_ends < 0 || n_parts < 0 || Hd <= 0 || Wd <= 0 || Wd > RLE_MAX_W || !win_desc) return RADET_ERR_ARG;
    const int nwords = (Wd + 3) / 4;
    const int threads = nwords >= 256 ? 256 : ((nwords + 63) / 64) * 64;
    hipLaunchKernelGGL(rle_masks_src_window_kernel, dim3(Hd, G), dim3(threads), 0, (hipStream_t)stream, run_ends, n_ends, part_desc,
                       n_parts, mask_desc, win_desc, dst, dst_plain, Hd, Wd, pad_val);
    return radet_check_launch();
}
