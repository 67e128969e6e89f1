// Tissue mask of a slide thumbnail on the device: the pixel stages of reference misc/utils.py:195-244 (stain_entropy_otsu; the morphology chain of
// get_tissue_mask is at the end of this file: cerb_tissue_morphology, on the labeller of pp_label.hip) and of the third-party routines they call
// (skimage.color.rgb2hed, skimage.filters.rank.entropy over disk(4), numpy.histogram behind skimage.filters.threshold_otsu).  Byte and integer work
// plus table look-ups of doubles: LDS / latency bound, no MFMA.
//
//   tm_hed_kernel       RGB -> three stain bytes.  rgb2hed is log(max(v / 255, 1e-6)) / log(1e-6) per channel times a 3 x 3 matrix, and the reference
//                       keeps (hed * 255).astype(uint8): per stain two adds of table entries lut[channel][value][stain], one multiply by 255, truncation
//                       toward zero and wrap-around modulo 256 (x86 numpy).  The host fills the table (cerberus_amd/tissue.py: stain_table) with the
//                       library's own arithmetic, so no logarithm is taken here.
//   tm_entropy_kernel   rank.entropy of the three planes in one launch and their combination (H + E) - D in the reference's order.  A block stages its
//                       32 x 4 tile and the 4-pixel halo of all three planes in LDS; a thread owns one pixel and a private 256-bin byte histogram in LDS
//                       (bin-major, one bank per thread): 49 increments, one ascending walk over the 64 words of the histogram that adds
//                       term[pop][count] for every bin in use -- skimage's `e -= p * log(p) / log(2)` in ascending bin order, with the products looked
//                       up in a host-filled table of at most 50 x 50 doubles -- and 49 stores that clear the bins again.  Pixels outside the image are
//                       left out of pop.  Every block also leaves the minimum and maximum of its outputs; tm_minmax_kernel folds them (min / max do not
//                       depend on the order, nothing here is a floating-point atomic).
//   tm_hist_kernel      numpy's uniform-bin assignment against the host's 257 edges (np.linspace(min, max, 257)): the scaled position truncated, the
//                       last edge closed, then one step down / up where the value lies outside [edge[i], edge[i + 1]).  Integer counts: LDS atomics per
//                       block, one 64-bit integer atomic per bin and block.  The counts do not depend on the launch geometry.
//   tm_threshold_kernel mask = entropy > threshold.
// The Otsu arithmetic on the 256 counts is host numpy (cerberus_amd/tissue.py: otsu_threshold).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "pp_common.h"

namespace {

constexpr int TM_TW = 32, TM_TH = 4, TM_R = 4;            // output tile, footprint radius (disk(4))
constexpr int TM_NT = TM_TW * TM_TH;                      // threads per block: one per output pixel
constexpr int TM_LW = TM_TW + 2 * TM_R, TM_LH = TM_TH + 2 * TM_R;
constexpr int TM_TERM = 50;                               // term table: [pop 0 .. 49][count 0 .. 49]

__global__ __launch_bounds__(256) void tm_hed_kernel(const uint8_t* __restrict__ rgb, long long row_stride, int H, int W, const double* __restrict__ lut,
                                                     uint8_t* __restrict__ planes) {
    __shared__ double sl[3 * 256 * 3];
    for (int i = threadIdx.x; i < 3 * 256 * 3; i += blockDim.x) sl[i] = lut[i];
    __syncthreads();
    const long long n = (long long)H * W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        const long long y = p / W, x = p - y * W;
        const uint8_t* px = rgb + y * row_stride + x * 3;
        const int r = px[0], g = px[1], b = px[2];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const double v = ((sl[r * 3 + s] + sl[(256 + g) * 3 + s]) + sl[(512 + b) * 3 + s]) * 255.0;
            planes[(long long)s * n + p] = (uint8_t)((long long)v & 255);  // toward zero, then modulo 256
        }
    }
}

// half-width of the disk(4) footprint in row dy (dx^2 + dy^2 <= 16): 49 pixels
__device__ __forceinline__ int tm_halfw(int dy) {
    const int a = dy < 0 ? -dy : dy;
    return a == 0 ? 4 : a <= 2 ? 3 : a == 3 ? 2 : 0;
}

__global__ __launch_bounds__(TM_NT) void tm_entropy_kernel(const uint8_t* __restrict__ planes, int H, int W, const double* __restrict__ term,
                                                           double* __restrict__ ent, double* __restrict__ part) {
    __shared__ uint8_t tile[3][TM_LH][TM_LW];
    __shared__ uint32_t hist[64 * TM_NT];  // hist[(bin >> 2) * TM_NT + thread]: four byte counters per word, a bank of its own per thread
    __shared__ double sterm[TM_TERM * TM_TERM];
    __shared__ double smin[TM_NT / 64], smax[TM_NT / 64];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TM_TW, y0 = blockIdx.y * TM_TH;
    const long long n = (long long)H * W;
    for (int i = tid; i < 3 * TM_LH * TM_LW; i += TM_NT) {
        const int s = i / (TM_LH * TM_LW), r = (i / TM_LW) % TM_LH, c = i % TM_LW;
        const int y = y0 + r - TM_R, x = x0 + c - TM_R;
        tile[s][r][c] = (y >= 0 && y < H && x >= 0 && x < W) ? planes[(long long)s * n + (long long)y * W + x] : 0;
    }
    for (int i = tid; i < TM_TERM * TM_TERM; i += TM_NT) sterm[i] = term[i];
    for (int i = 0; i < 64; ++i) hist[i * TM_NT + tid] = 0;
    __syncthreads();
    const int lx = tid % TM_TW, ly = tid / TM_TW;
    const int x = x0 + lx, y = y0 + ly;
    const bool live = x < W && y < H;
    double out = 0.0;
    if (live) {
        int pop = 0;
        for (int dy = -TM_R; dy <= TM_R; ++dy) {
            if (y + dy < 0 || y + dy >= H) continue;
            const int hw = tm_halfw(dy);
            const int a = x - hw < 0 ? 0 : x - hw, b = x + hw > W - 1 ? W - 1 : x + hw;
            pop += b - a + 1;
        }
        const double* trow = sterm + pop * TM_TERM;
        double e3[3];
        for (int s = 0; s < 3; ++s) {
            for (int dy = -TM_R; dy <= TM_R; ++dy) {
                if (y + dy < 0 || y + dy >= H) continue;
                const int hw = tm_halfw(dy);
                for (int dx = -hw; dx <= hw; ++dx) {
                    if (x + dx < 0 || x + dx >= W) continue;
                    const int v = tile[s][ly + TM_R + dy][lx + TM_R + dx];
                    hist[(v >> 2) * TM_NT + tid] += 1u << ((v & 3) * 8);  // (a counter holds at most 49)
                }
            }
            double e = 0.0;
            for (int wd = 0; wd < 64; ++wd) {  // ascending bins
                const uint32_t c4 = hist[wd * TM_NT + tid];
                if (!c4) continue;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = (c4 >> (8 * k)) & 255;
                    if (c) e -= trow[c];
                }
            }
            e3[s] = e;
            for (int dy = -TM_R; dy <= TM_R; ++dy) {
                if (y + dy < 0 || y + dy >= H) continue;
                const int hw = tm_halfw(dy);
                for (int dx = -hw; dx <= hw; ++dx) {
                    if (x + dx < 0 || x + dx >= W) continue;
                    hist[(tile[s][ly + TM_R + dy][lx + TM_R + dx] >> 2) * TM_NT + tid] = 0;
                }
            }
        }
        out = (e3[0] + e3[1]) - e3[2];  // np.sum([h, e], axis=0) - d
        ent[(long long)y * W + x] = out;
    }
    // block minimum / maximum (every block holds at least its pixel (x0, y0))
    double mn = live ? out : __builtin_inf(), mx = live ? out : -__builtin_inf();
    for (int d = 32; d >= 1; d >>= 1) {
        const double a = __shfl_xor(mn, d), b = __shfl_xor(mx, d);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((tid & 63) == 0) {
        smin[tid >> 6] = mn;
        smax[tid >> 6] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < TM_NT / 64; ++w) {
            mn = smin[w] < mn ? smin[w] : mn;
            mx = smax[w] > mx ? smax[w] : mx;
        }
        const long long blk = (long long)blockIdx.y * gridDim.x + blockIdx.x;
        part[2 * blk] = mn;
        part[2 * blk + 1] = mx;
    }
}

__global__ __launch_bounds__(256) void tm_minmax_kernel(const double* __restrict__ part, long long n_part, double* __restrict__ minmax) {
    __shared__ double smin[4], smax[4];
    double mn = __builtin_inf(), mx = -__builtin_inf();
    for (long long i = threadIdx.x; i < n_part; i += 256) {
        const double a = part[2 * i], b = part[2 * i + 1];
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const double a = __shfl_xor(mn, d), b = __shfl_xor(mx, d);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        smin[threadIdx.x >> 6] = mn;
        smax[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            mn = smin[w] < mn ? smin[w] : mn;
            mx = smax[w] > mx ? smax[w] : mx;
        }
        minmax[0] = mn;
        minmax[1] = mx;
    }
}

__global__ __launch_bounds__(256) void tm_hist_kernel(const double* __restrict__ ent, long long n, const double* __restrict__ edges,
                                                      unsigned long long* __restrict__ counts) {
    __shared__ double se[257];
    __shared__ unsigned int sc[256];
    for (int i = threadIdx.x; i < 257; i += 256) se[i] = edges[i];
    sc[threadIdx.x] = 0;
    __syncthreads();
    const double first = se[0], denom = se[256] - se[0];
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        const double a = ent[p];
        if (!(a >= first && a <= se[256])) continue;  // numpy keeps first <= a <= last (NaN falls out here too)
        int i = (int)(((a - first) / denom) * 256.0);
        i = i < 0 ? 0 : i > 255 ? 255 : i;  // (the last edge belongs to the last bin)
        if (a < se[i]) i = i > 0 ? i - 1 : 0;
        else if (a >= se[i + 1] && i != 255) ++i;
        atomicAdd(&sc[i], 1u);
    }
    __syncthreads();
    if (sc[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)sc[threadIdx.x]);
}

__global__ void tm_threshold_kernel(const double* __restrict__ ent, long long n, double thr, uint8_t* __restrict__ mask) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) mask[p] = ent[p] > thr ? 1 : 0;
}

inline unsigned tm_grid(long long n) {
    long long b = (n + 255) / 256;
    return (unsigned)(b > 4096 ? 4096 : b < 1 ? 1 : b);
}
inline long long tm_blocks(int h, int w) { return (long long)((w + TM_TW - 1) / TM_TW) * ((h + TM_TH - 1) / TM_TH); }
inline bool tm_bad_size(int h, int w) { return h <= 0 || w <= 0 || (long long)h * w >= (1ll << 31) || (h + TM_TH - 1) / TM_TH > 65535; }

}  // namespace

// per pixel: the labelling of cerb_tissue_morphology (two int32 maps, two byte maps); per entropy block: its minimum and maximum
extern "C" size_t cerb_tissue_workspace_bytes(int h, int w) {
    if (h <= 0 || w <= 0) return 0;
    const size_t n = (size_t)h * (size_t)w;
    return n * 10 + (size_t)tm_blocks(h, w) * 16 + (1u << 20);
}

extern "C" int cerb_tissue_hed(const uint8_t* rgb, long long row_stride, int h, int w, const double* lut, uint8_t* planes_out, void* hip_stream) {
    if (!rgb || !lut || !planes_out || tm_bad_size(h, w) || row_stride < 3ll * w) return cerb_set_error("cerb_tissue_hed: bad arguments");
    hipLaunchKernelGGL(tm_hed_kernel, dim3(tm_grid((long long)h * w)), dim3(256), 0, (hipStream_t)hip_stream, rgb, row_stride, h, w, lut, planes_out);
    KCHECK();
    return 0;
}

extern "C" int cerb_tissue_entropy(const uint8_t* planes, int h, int w, const double* term_table, double* ent_out, double* minmax_out, void* ws,
                                   size_t ws_bytes, void* hip_stream) {
    if (!planes || !term_table || !ent_out || !minmax_out || !ws || tm_bad_size(h, w)) return cerb_set_error("cerb_tissue_entropy: bad arguments");
    if (ws_bytes < cerb_tissue_workspace_bytes(h, w)) return cerb_set_error("cerb_tissue_entropy: workspace too small");
    if (((uintptr_t)ws & 7) != 0) return cerb_set_error("cerb_tissue_entropy: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)hip_stream;
    double* part = (double*)ws;
    const dim3 grid((w + TM_TW - 1) / TM_TW, (h + TM_TH - 1) / TM_TH);
    hipLaunchKernelGGL(tm_entropy_kernel, grid, dim3(TM_NT), 0, st, planes, h, w, term_table, ent_out, part);
    hipLaunchKernelGGL(tm_minmax_kernel, dim3(1), dim3(256), 0, st, (const double*)part, tm_blocks(h, w), minmax_out);
    KCHECK();
    return 0;
}

extern "C" int cerb_tissue_histogram(const double* ent, int h, int w, const double* edges257, int64_t* counts256_out, void* hip_stream) {
    if (!ent || !edges257 || !counts256_out || tm_bad_size(h, w)) return cerb_set_error("cerb_tissue_histogram: bad arguments");
    hipStream_t st = (hipStream_t)hip_stream;
    PP_OK(hipMemsetAsync(counts256_out, 0, 256 * sizeof(int64_t), st));
    hipLaunchKernelGGL(tm_hist_kernel, dim3(tm_grid((long long)h * w)), dim3(256), 0, st, ent, (long long)h * w, edges257, (unsigned long long*)counts256_out);
    KCHECK();
    return 0;
}

extern "C" int cerb_tissue_threshold(const double* ent, int h, int w, double thr, uint8_t* mask_out, void* hip_stream) {
    if (!ent || !mask_out || tm_bad_size(h, w)) return cerb_set_error("cerb_tissue_threshold: bad arguments");
    hipLaunchKernelGGL(tm_threshold_kernel, dim3(tm_grid((long long)h * w)), dim3(256), 0, (hipStream_t)hip_stream, ent, (long long)h * w, thr, mask_out);
    KCHECK();
    return 0;
}

// =================================================================================================================
// Tissue-mask morphology (misc/utils.py:216-235 `morphology`, the second half of get_tissue_mask :238-244):
//     binary_erosion(disk(3)) -> remove_small_holes(2000) -> remove_small_objects(2000) -> binary_dilation(disk(3)) -> remove_small_holes(2000)
//     -> binary_fill_holes, connectivity 1 throughout.
// The erosion and the dilation are scipy.ndimage's (misc/utils.py:16-19), whose border_value defaults to 0: pixels outside the image count as CLEAR
// for both, so the erosion removes a 3-pixel rim of anything that touches the image border.  remove_small_objects drops 4-connected components with
// area < min_size; remove_small_holes is the same on the complement -- border-touching background included, so a mask of fewer than 2000 pixels
// always ends full.  binary_fill_holes sets the background components that do not reach the image border.  Labelling and areas are
// pp_label.hip's (pp_ccl_run); the other stages are here.
// =================================================================================================================
// disk(3): dx^2 + dy^2 <= 9, 29 pixels.  ERODE: set iff every footprint pixel is inside the image and set; else (dilation): set iff one is.
template <bool ERODE>
__global__ void tm_morph_disk3_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W) {
    const long long n = (long long)H * W;
    const double invW = 1.0 / (double)W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        int y, x;
        pix_yx(p, W, invW, y, x);
        bool r = ERODE;
        for (int dy = -3; dy <= 3; ++dy) {
            const int hw = dy == 0 ? 3 : (dy == 3 || dy == -3) ? 0 : 2;
            const int yy = y + dy;
            for (int dx = -hw; dx <= hw; ++dx) {
                const int xx = x + dx;
                const bool v = yy >= 0 && yy < H && xx >= 0 && xx < W && in[(long long)yy * W + xx] != 0;
                r = ERODE ? (r && v) : (r || v);
            }
        }
        out[p] = r ? 1 : 0;
    }
}
// pixels of colour `val` whose component (L: flattened roots, area at the roots) is smaller than min_size take the other colour
__global__ void tm_flip_small_kernel(uint8_t* __restrict__ m, uint8_t val, const int* __restrict__ L, const int* __restrict__ area, int min_size, int n) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x)
        if (m[p] == val && area[L[p]] < min_size) m[p] = val ? 0 : 1;
}
// flag[root] = 1 for the background components that reach the image border (flag zeroed by the caller; every writer stores the same value)
__global__ void tm_border_bg_kernel(const uint8_t* __restrict__ m, const int* __restrict__ L, int* __restrict__ flag, int H, int W) {
    const int per = 2 * (H + W);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < per; i += gridDim.x * blockDim.x) {
        const long long p = perimeter_pixel(i, H, W);
        if (!m[p]) flag[L[p]] = 1;
    }
}
__global__ void tm_fill_holes_kernel(const uint8_t* __restrict__ m, const int* __restrict__ L, const int* __restrict__ flag, uint8_t* __restrict__ out, int n) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) out[p] = (m[p] || !flag[L[p]]) ? 1 : 0;
}
static int tm_remove_small(uint8_t* m, uint8_t val, int* L, int* area, int min_size, int H, int W, hipStream_t st) {
    const int n = H * W;
    PP_OK(hipMemsetAsync(area, 0, (size_t)n * 4, st));
    if (pp_ccl_run(m, val, L, H, W, st, area)) return 1;
    hipLaunchKernelGGL(tm_flip_small_kernel, dim3(grid_for(n)), dim3(256), 0, st, m, val, (const int*)L, (const int*)area, min_size, n);
    KCHECK();
    return 0;
}
extern "C" int cerb_tissue_morphology(const uint8_t* mask_in, int H, int W, uint8_t* mask_out, void* ws, size_t ws_bytes, void* hip_stream) {
    if (int rc = pp_check_map("cerb_tissue_morphology", mask_in && mask_out && ws, H, W, ws_bytes, cerb_tissue_workspace_bytes(H, W))) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const int n = H * W;
    Carve cv{(char*)ws, ws_bytes};
    int* L = (int*)cv.take((size_t)n * 4);
    int* area = (int*)cv.take((size_t)n * 4);  // component areas; then the border flags of the hole filling
    uint8_t* a = (uint8_t*)cv.take(n);
    uint8_t* b = (uint8_t*)cv.take(n);
    if (!b) return cerb_set_error("cerb_tissue_morphology: workspace carve failed");
    const unsigned g = grid_for(n);
    const int min_size = 2000;  // misc/utils.py:224-230
    hipLaunchKernelGGL(tm_morph_disk3_kernel<true>, dim3(g), dim3(256), 0, st, mask_in, a, H, W);
    if (tm_remove_small(a, 0, L, area, min_size, H, W, st)) return 1;  // remove_small_holes
    if (tm_remove_small(a, 1, L, area, min_size, H, W, st)) return 1;  // remove_small_objects
    hipLaunchKernelGGL(tm_morph_disk3_kernel<false>, dim3(g), dim3(256), 0, st, (const uint8_t*)a, b, H, W);
    if (tm_remove_small(b, 0, L, area, min_size, H, W, st)) return 1;  // remove_small_holes
    if (pp_ccl_run(b, 0, L, H, W, st)) return 1;                       // binary_fill_holes
    PP_OK(hipMemsetAsync(area, 0, (size_t)n * 4, st));
    hipLaunchKernelGGL(tm_border_bg_kernel, dim3(nblk(2 * ((long long)H + W), 256)), dim3(256), 0, st, (const uint8_t*)b, (const int*)L, area, H, W);
    hipLaunchKernelGGL(tm_fill_holes_kernel, dim3(g), dim3(256), 0, st, (const uint8_t*)b, (const int*)L, (const int*)area, mask_out, n);
    KCHECK();
    return 0;
}
