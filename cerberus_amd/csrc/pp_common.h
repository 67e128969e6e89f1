// What the post-processing units share (pp_label.hip, pp_nuclei.hip, pp_gland.hip, and the labelling users tissue_mask.hip and slide_kernels.hip):
// the host-side error macros, launch-size helpers, workspace carving and entry-point checks; the device-side primitives (pixel index -> (row, column),
// lock-free union-find, 256-thread block scan, perimeter walk), all __forceinline__; and the declarations of the host launchers that cross units.
// No kernel lives here: a kernel that two units need is reached through its unit's launcher, so the library carries every kernel once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/cerberus_hip.h"
#include "cerb_dev.h"

int cerb_set_error(const std::string& m);  // cerb_api.hip
#define PP_OK(expr)                                                                                   \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return cerb_set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define KCHECK() PP_OK(hipGetLastError())

typedef unsigned long long u64;
typedef unsigned int u32;

#define SCAN_ITEMS 1024  // the scans of pp_label.hip, per block: 256 threads x 4

// =================================================================================================================
// Host side
// =================================================================================================================
static inline unsigned nblk(long long n, int per) { return (unsigned)((n + per - 1) / per); }
static inline unsigned grid_for(long long n) {
    long long b = (n + 255) / 256;
    if (b > 256 * 16) b = 256 * 16;
    if (b < 1) b = 1;
    return (unsigned)b;
}
struct Carve {
    char* p;
    size_t left;
    void* take(size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        if (bytes > left) return nullptr;
        void* r = p;
        p += bytes;
        left -= bytes;
        return r;
    }
};
// What an entry point that works on one map below 2^31 pixels out of a caller's workspace opens with (0, or the error code)
static inline int pp_check_map(const std::string& who, bool pointers_ok, int H, int W, size_t ws_bytes, size_t ws_needed) {
    if (!pointers_ok || H <= 0 || W <= 0) return cerb_set_error(who + ": bad arguments");
    if (ws_bytes < ws_needed) return cerb_set_error(who + ": workspace too small");
    if ((long long)H * W >= (1ll << 31)) return cerb_set_error(who + ": map too large (H*W must be < 2^31)");
    return 0;
}

// ---- launchers of pp_label.hip that other units call (every one returns 0, or the error code with cerb_set_error's message set) ----------------
// out = exclusive prefix sum of in; tmp must hold at least n/1024 + n/1024^2 + ... + 4 ints
int pp_scan_exclusive(const int* in, int* out, int n, int* tmp, hipStream_t st);
// wpre[w] (+ (*block_offsets)[w >> 10] when that is not nullptr) = number of set bits in the words before w; count_out (optional, a device int): the
// number of set bits, or -1 when `any` is given and *any == 0
int pp_scan_exclusive_popc(const u64* bits, int* wpre, int nw, int* tmp, hipStream_t st, const int** block_offsets, int* count_out, const int* any);
// 4-connected components of fg == val: L[p] = the component's smallest raster index (-1 elsewhere); area (optional, zeroed by the caller): pixels per root
int pp_ccl_run(const uint8_t* fg, uint8_t val, int* L, int H, int W, hipStream_t st, int* area = nullptr);
// pp_ccl_run on fg == 1, then out[p] = 1 + the rank of p's component among the kept ones in raster order of their roots (scipy's label ids), 0 elsewhere, and
// *n_out = their number.  area != nullptr: it receives the areas and components below min_size are dropped; nullptr: every component is kept.
int pp_label_ranked(const uint8_t* fg, int* L, int* area, int min_size, int* flag, int* rank, int* scantmp, int* out, int* n_out, int H, int W, hipStream_t st);
// The nuclei mask: components of msk == 1, msk &= "the component has min_size pixels", L[p] = root of a kept pixel, bits = bitmap of the kept roots,
// area at the roots.  wide: the tile labelling with its root list (roots: H * W ints, n_roots: one per tile) and four pixels per thread (W % 4 == 0,
// 16-byte aligned maps); else pp_ccl_run and one pixel per thread.  colbuf: 2 x (tiles_x - 1) x H ints for the seam columns.
int pp_label_mask_min_area(uint8_t* msk, int* L, int* area, int min_size, int H, int W, hipStream_t st, u64* root_bits, bool wide, int* roots, int* n_roots,
                           int* colbuf);
// The nuclei markers: label -> drop components below min_size -> fill holes -> label, as edits of ONE two-colour forest (see pp_label.hip)
int pp_markers_two_colour(uint8_t* mrk, int* L, int* area, int* border, int* roots, int* n_roots, int min_size, int H, int W, hipStream_t st, u64* root_bits,
                          bool wide, int* colbuf);
// entries of n_roots above: the number of labelling tiles of an H x W map
int pp_label_tiles(int H, int W);

// =================================================================================================================
// Device side
// =================================================================================================================
// (row, column) of a linear pixel index p < 2^31 without the 64-bit integer division a per-pixel `p / W`, `p % W` costs (~100 VALU
// instructions): one fp64 multiply by a per-thread reciprocal, exact after a one-step fix-up.
__device__ __forceinline__ void pix_yx(long long p, int W, double invW, int& y, int& x) {
    int q = (int)((double)p * invW);
    int r = (int)(p - (long long)q * W);
    if (r < 0) {
        --q;
        r += W;
    } else if (r >= W) {
        ++q;
        r -= W;
    }
    y = q;
    x = r;
}
// pixel i of the map's perimeter walk, i < 2 (H + W): top row, bottom row, left column, right column (corners come twice)
__device__ __forceinline__ long long perimeter_pixel(int i, int H, int W) {
    if (i < W) return i;
    if (i < 2 * W) return (long long)(H - 1) * W + (i - W);
    if (i < 2 * W + H) return (long long)(i - 2 * W) * W;
    return (long long)(i - 2 * W - H) * W + (W - 1);
}

// ---- union-find on an implicit grid: lock-free (atomicMin on roots), root = smallest index of the set ----------------------------------------
// Three finds.  Agent-scope loads; IDX = int for maps below 2^31 pixels, long long above (slide_kernels.hip: cc8_*):
template <typename IDX>
__device__ __forceinline__ IDX uf_find(const IDX* L, IDX x) {
    IDX p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        x = p;
        p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return x;
}
// the forest of one tile in LDS:
__device__ __forceinline__ int lds_find(volatile int* L, int x) {
    int p = L[x];
    while (p != x) {
        x = p;
        p = L[x];
    }
    return x;
}
// CACHED finds (0.27 -> 0.17 ms for the marker image's seams at 8192^2 against uf_union): uf_find's agent-scope
// loads go past the L2 on every step; a plain load may be
// stale, but a stale parent is still an ancestor (links only ever move towards smaller indices inside one set) and the returning atomicMin that
// closes a union validates the root it acts on -- a root that was no root any more hands back its real parent and the loop continues from there.
// Every step also pulls the node it leaves one level up (path halving by a non-returning atomicMin).
__device__ __forceinline__ int uf_find_relaxed(int* L, int x) {
    int p = L[x];
    while (p != x) {
        const int gp = L[p];
        if (gp != p) atomicMin(&L[x], gp);
        x = p;
        p = gp;
    }
    return x;
}
// One union: find both roots, atomicMin the larger under the smaller, retry from what the atomic handed back when it was no root any more
template <typename IDX, typename FIND>
__device__ __forceinline__ void uf_union_by(FIND find, IDX* L, IDX a, IDX b) {
    bool done;
    do {
        a = find(L, a);
        b = find(L, b);
        if (a < b) {
            const IDX old = atomicMin(&L[b], a);
            done = (old == b);
            b = old;
        } else if (b < a) {
            const IDX old = atomicMin(&L[a], b);
            done = (old == a);
            a = old;
        } else
            done = true;
    } while (!done);
}
template <typename IDX>
__device__ __forceinline__ void uf_union(IDX* L, IDX a, IDX b) {
    uf_union_by([](IDX* l, IDX x) { return uf_find<IDX>(l, x); }, L, a, b);
}
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
    uf_union_by([](int* l, int x) { return lds_find(l, x); }, L, a, b);
}
__device__ __forceinline__ void uf_union_relaxed(int* L, int a, int b) {
    uf_union_by([](int* l, int x) { return uf_find_relaxed(l, x); }, L, a, b);
}

// Exclusive scan of one int per thread over a 256-thread block (every thread calls it): returns the sum of the threads before this one; `total` is
// the block's sum in the LAST thread (tid 255) and a partial sum elsewhere.
__device__ __forceinline__ int block_exclusive_scan_256(int tsum, int& total) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = tsum;  // inclusive scan across the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    total = woff + inc;
    return woff + inc - tsum;
}
