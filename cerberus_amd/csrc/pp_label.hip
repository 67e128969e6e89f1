// The labelling stage of the instance post-processing on gfx950 (overview: pp_nuclei.hip; shared primitives and the launchers declared for the other
// units: pp_common.h): the prefix scans, the 4-connected one-colour labeller (tile-local union-find in LDS, seams through the global one), the
// two-colour labeller of the nuclei markers with its root bitmaps, and cerb_label_mask.
#include <climits>

#include "pp_common.h"

// =================================================================================================================
// Exclusive prefix sum over int32 (three-kernel, recursive on the block sums)
// =================================================================================================================
__global__ __launch_bounds__(256) void scan_block_kernel(const int* __restrict__ in, int* __restrict__ out, int* __restrict__ sums, int n) {
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * SCAN_ITEMS + tid * 4;
    int v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (base + i < n) ? in[base + i] : 0;
    const int tsum = v[0] + v[1] + v[2] + v[3];
    int total;
    int run = block_exclusive_scan_256(tsum, total);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
    if (tid == 255 && sums) sums[blockIdx.x] = total;
}
__global__ void scan_add_kernel(int* __restrict__ out, const int* __restrict__ sums, int n) {
    const long long i = (long long)blockIdx.x * SCAN_ITEMS + threadIdx.x;
    const int add = sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long j = i + k * 256;
        if (j < n) out[j] += add;
    }
}
int pp_scan_exclusive(const int* in, int* out, int n, int* tmp, hipStream_t st) {
    const int nb = (n + SCAN_ITEMS - 1) / SCAN_ITEMS;
    if (nb <= 1) {
        hipLaunchKernelGGL(scan_block_kernel, dim3(1), dim3(256), 0, st, in, out, (int*)nullptr, n);
        KCHECK();
        return 0;
    }
    hipLaunchKernelGGL(scan_block_kernel, dim3(nb), dim3(256), 0, st, in, out, tmp, n);
    KCHECK();
    if (pp_scan_exclusive(tmp, tmp, nb, tmp + ((nb + 3) & ~3), st)) return 1;
    hipLaunchKernelGGL(scan_add_kernel, dim3(nb), dim3(256), 0, st, out, tmp, n);
    KCHECK();
    return 0;
}

// ---- root bitmaps (round 5) -------------------------------------------------------------------------------------
// The roots of a labelling are ~1 pixel in 1000; the passes that only want THEM (ranks = scipy's label ids, per-component setup, heap offsets, work
// lists) used to scan the whole pixel map (0.12 - 0.19 ms each at 8192^2).  The last per-pixel pass of a labelling leaves one bit per pixel instead
// ("is a kept root": a wave ballot, one 8-byte store per 64 pixels), and those passes walk n / 64 words.
//   rank of root r = wpre[r >> 6] (+ block offset) + popcount(bits[r >> 6] below bit r & 63)
__global__ __launch_bounds__(256) void scan_block_popc_kernel(const u64* __restrict__ bits, int* __restrict__ out, int* __restrict__ sums, int nw) {
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * SCAN_ITEMS + tid * 4;
    int v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (base + i < nw) ? __popcll(bits[base + i]) : 0;
    const int tsum = v[0] + v[1] + v[2] + v[3];
    int total;
    int run = block_exclusive_scan_256(tsum, total);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (base + i < nw) out[base + i] = run;
        run += v[i];
    }
    if (tid == 255 && sums) sums[blockIdx.x] = total;
}
__global__ void count_roots_from_bits_kernel(const u64* __restrict__ bits, const int* __restrict__ wpre, const int* __restrict__ boff, int nw, int* __restrict__ out,
                                             const int* __restrict__ any) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *out = (any && !*any) ? -1 : (nw > 0 ? wpre[nw - 1] + (boff ? boff[(nw - 1) / SCAN_ITEMS] : 0) + __popcll(bits[nw - 1]) : 0);
}
int pp_scan_exclusive_popc(const u64* bits, int* wpre, int nw, int* tmp, hipStream_t st, const int** block_offsets, int* count_out, const int* any) {
    const int nb = (nw + SCAN_ITEMS - 1) / SCAN_ITEMS;
    *block_offsets = nullptr;
    hipLaunchKernelGGL(scan_block_popc_kernel, dim3(nb), dim3(256), 0, st, bits, wpre, nb > 1 ? tmp : (int*)nullptr, nw);
    KCHECK();
    if (nb > 1) {
        if (pp_scan_exclusive(tmp, tmp, nb, tmp + ((nb + 3) & ~3), st)) return 1;
        *block_offsets = tmp;
    }
    if (count_out) {
        hipLaunchKernelGGL(count_roots_from_bits_kernel, dim3(1), dim3(1), 0, st, bits, (const int*)wpre, *block_offsets, nw, count_out, any);
        KCHECK();
    }
    return 0;
}

// =================================================================================================================
// Union-find connected components (4-connectivity) on an implicit grid
// =================================================================================================================
__global__ void ccl_flatten_kernel(int* L, int n) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        if (L[p] < 0) continue;
        L[p] = uf_find(L, (int)p);
    }
}
// flatten + component areas in one pass over L: area[root] += the length of each RUN of equal roots inside the wave (64 consecutive pixels of a
// row hold a few runs; a separate area pass would re-read all of L for the same atomics).  `area` is zeroed by the caller.
__global__ void ccl_flatten_area_kernel(int* L, int* __restrict__ area, int n) {
    const int lane = threadIdx.x & 63;
    for (long long base = (blockIdx.x * (long long)blockDim.x + threadIdx.x) - lane; base < n; base += (long long)gridDim.x * blockDim.x) {
        const long long p = base + lane;
        int r = -1;
        if (p < n && L[p] >= 0) {
            r = uf_find(L, (int)p);
            L[p] = r;
        }
        const int prev = __shfl_up(r, 1);
        const bool head = r >= 0 && (lane == 0 || prev != r);
        const unsigned long long bounds = __ballot(head || r < 0);
        if (head) {
            const unsigned long long after = lane == 63 ? 0ull : (bounds >> (lane + 1));
            atomicAdd(&area[r], after ? __ffsll((long long)after) : 64 - lane);
        }
    }
}
// Tile-local labelling (round 2): a workgroup labels a 64 x 32-pixel tile with its union-find in LDS (an LDS atomic is ~20x cheaper than
// the L2 round trips of a global uf_union, and a run-pair union of the global merge pass cost 2-3 us of serial latency), writes every
// pixel's tile root as a GLOBAL index, and only the pixel pairs across tile borders (1/32 of the rows, 1/64 of the columns) go through
// the global union-find.  Roots stay "smallest raster index of the component".
constexpr int CT_W = 64, CT_H = 32;
// first slot of a tile's range in the root list: the pixels of the tile rows above it + of the tiles to its left in its own tile row
// (a tile gets as many slots as it has pixels, the list as many as the map)
__device__ __forceinline__ int tile_list_base(int tx0, int ty0, int H, int W) {
    const int rows = H - ty0 < CT_H ? H - ty0 : CT_H;
    return ty0 * W + tx0 * rows;
}
// ROOTS (round 5): every tile-local root is appended to a compact list (one atomic per tile) and area[root] = the pixels of its tile-local set (counted
// per run in LDS) -- with the list flattened after the seam unions (ccl2_flatten_roots_kernel) L[L[p]] is a pixel's root and roots_area_merge_kernel
// adds the merged sets' counts up over the LIST: no pass over the pixel map for the flatten, none for the areas, no zero fill of `area`.
template <bool ROOTS>
__global__ __launch_bounds__(256) void ccl_tile_kernel(const uint8_t* __restrict__ fg, uint8_t val, int* __restrict__ L, int H, int W, int tiles_x, int n_tiles,
                                                       int* __restrict__ roots, int* __restrict__ cnt, int* __restrict__ area, int* __restrict__ colbuf = nullptr) {
    __shared__ int sl[CT_H * CT_W];
    __shared__ u64 smask[CT_H];
    __shared__ int scnt[ROOTS ? CT_H * CT_W : 1];
    __shared__ int swtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int tx0 = (tile % tiles_x) * CT_W, ty0 = (tile / tiles_x) * CT_H;
        const int x = tx0 + lane;
        // rows wave*8 .. +7: every pixel points at the first pixel of its horizontal run inside the tile (ballot, no atomics)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = wave * 8 + i, y = ty0 + r;
            const bool f = x < W && y < H && fg[(long long)y * W + x] == val;
            const u64 m = __ballot(f);
            const u64 starts = m & ~(m << 1);
            sl[r * CT_W + lane] = f ? r * CT_W + 63 - __clzll((long long)(starts & ((2ull << lane) - 1))) : -1;
            if (ROOTS) scnt[r * CT_W + lane] = 0;
            if (lane == 0) smask[r] = m;
        }
        __syncthreads();
        // one union per pair of vertically adjacent runs: at the first column where they overlap
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = wave * 8 + i;
            if (r == 0) continue;
            const u64 m = smask[r], up = smask[r - 1];
            const u64 both = m & up;
            const u64 first = both & (~(m << 1) | ~(up << 1));  // the lower run starts here, or the upper one does
            if ((first >> lane) & 1) lds_union(sl, r * CT_W + lane, (r - 1) * CT_W + lane);
        }
        __syncthreads();
        u64 rmv[8] = {};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = wave * 8 + i, y = ty0 + r;
            bool is_root = false;
            if (x < W && y < H) {
                const int l = sl[r * CT_W + lane];
                int g = -1;
                if (l >= 0) {
                    const int root = lds_find(sl, l);
                    g = (ty0 + (root >> 6)) * W + tx0 + (root & 63);
                    if (ROOTS) {
                        is_root = root == r * CT_W + lane;
                        const u64 mrow = smask[r];
                        if (((mrow & ~(mrow << 1)) >> lane) & 1ull) {  // first pixel of a run: the run's length goes to the set's counter
                            const u64 rest = ~(mrow >> lane);
                            atomicAdd(&scnt[root], rest ? __ffsll((long long)rest) - 1 : 64 - lane);
                        }
                    }
                }
                L[(long long)y * W + x] = g;
                // the tile's border columns, compactly: what the seam pass wants of this tile (seam_cols: [right-of-seam | left-of-seam][seam k][y])
                if (colbuf) {
                    if (lane == 0 && tx0 > 0) colbuf[(long long)(tx0 / CT_W - 1) * H + y] = g;
                    if (lane == CT_W - 1 && tx0 + CT_W < W) colbuf[(long long)(tiles_x - 1) * H + (long long)(tx0 / CT_W) * H + y] = g;
                }
            }
            if (ROOTS) rmv[i] = __ballot(is_root);
        }
        if (ROOTS) {
            __syncthreads();  // every set's counter is complete
            {   // the tile's roots go to the tile's OWN range of the list (tile_list_base: as many slots as the tile has pixels) and their number to
                // cnt[tile] -- a shared list head took one returning atomic per tile on ONE address: 33 k of them cost 0.1 ms, 131 k (one per wave) 0.4 ms
                int tot = 0;
#pragma unroll
                for (int i = 0; i < 8; ++i) tot += __popcll(rmv[i]);
                if (lane == 0) swtot[wave] = tot;
                __syncthreads();
                int base = tile_list_base(tx0, ty0, H, W);
                for (int w = 0; w < wave; ++w) base += swtot[w];
                if (tid == 0) cnt[tile] = swtot[0] + swtot[1] + swtot[2] + swtot[3];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int r = wave * 8 + i, y = ty0 + r;
                    if ((rmv[i] >> lane) & 1ull) {
                        roots[base + __popcll(rmv[i] & ((1ull << lane) - 1))] = y * W + x;
                        area[(long long)y * W + x] = scnt[r * CT_W + lane];
                    }
                    base += __popcll(rmv[i]);
                }
            }
            __syncthreads();  // (sl / scnt / swtot are rewritten by the next tile)
        } else {
            __syncthreads();
        }
    }
}
// The list kernels: one wave per tile walks the tile's range of the root list (cnt[tile] entries from tile_list_base).
// area[root] += the counts of the tile-local sets that were united into it (needs the flattened list: L[t] is t's root)
__global__ void roots_area_merge_kernel(const int* __restrict__ L, const int* __restrict__ roots, const int* __restrict__ cnt, int n_tiles, int tiles_x, int H,
                                        int W, int* __restrict__ area) {
    const int lane = threadIdx.x & 63, nwaves = gridDim.x * (blockDim.x >> 6);
    for (int tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); tile < n_tiles; tile += nwaves) {
        const int c = cnt[tile], base = tile_list_base((tile % tiles_x) * CT_W, (tile / tiles_x) * CT_H, H, W);
        for (int k = lane; k < c; k += 64) {
            const int t = roots[base + k];
            const int f = L[t];
            if (f != t) {
                const int a = area[t];
                if (a) atomicAdd(&area[f], a);
            }
        }
    }
}
// unions across tile borders: vertical seams (x a multiple of 64: the run continues), horizontal seams (y a multiple of 32: one union per
// pair of tile-clipped runs, at the first column where they overlap)
// cols (round 6): the tile kernel's compact copy of its border columns -- [0, nv): the label RIGHT of seam k at row y (the right tile's first
// column), [nv, 2 nv): left of it (the left tile's last column); -1 = not `val`.  A vertical seam then reads two coalesced ints per pixel pair instead of two
// bytes and two labels out of four different 64-byte lines (4 B/px of HBM traffic for 3 % of the pixels: profiles/r06_postproc_nuclei_8192_bytes_per_pass.txt).
// What a column entry holds is the pixel's tile root as the tile pass left it: an ancestor of the pixel whatever unions have happened since -- the same
// starting point L[pixel] gives.
// The tail of a seam kernel: the lane's pair is (a, b), two pixels, or (ca, cb), their tile roots out of the compact columns; -1 = none.
// A component that crosses many seams (the background of a marker image is ONE component) would hammer one root with atomics:
// the tile pass left every pixel pointing at its tile root, so neighbouring lanes mostly ask for the same (root, root) pair --
// only the first lane of each run of equal pairs performs the union.  Every lane of the wave calls this (shuffles).
template <typename UNION>
__device__ __forceinline__ void seam_union_runs(int* L, int a, int b, int ca, int cb, int lane, UNION unite) {
    const int ra = ca >= 0 ? ca : a >= 0 ? L[a] : -1, rb = ca >= 0 ? cb : b >= 0 ? L[b] : -2;
    const int pa = __shfl_up(ra, 1), pb = __shfl_up(rb, 1);
    if ((a >= 0 || ca >= 0) && ra != rb && !(lane > 0 && pa == ra && pb == rb)) unite(L, ra, rb);
}
__global__ void ccl_seam_kernel(const uint8_t* __restrict__ fg, uint8_t val, int* L, int H, int W, int tiles_x, int tiles_y, const int* __restrict__ cols = nullptr) {
    const unsigned sx = (unsigned)(tiles_x - 1), sy = (unsigned)(tiles_y - 1);
    const unsigned nv = sx * (unsigned)H, nh = sy * (unsigned)W;  // < 2^31 / 32
    const unsigned total = nv + nh, stride = gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (unsigned i0 = blockIdx.x * blockDim.x + threadIdx.x - lane; i0 < total; i0 += stride) {  // wave-uniform trip count (shuffles below)
        const unsigned i = i0 + lane;
        int a = -1, b = -1;
        int ca = -1, cb = -1;  // vertical seam through the compact columns: the two roots themselves
        if (i < nv && cols) {
            ca = cols[i];
            cb = cols[nv + i];
            if (ca < 0 || cb < 0) ca = cb = -1;
        } else if (i < nv) {  // consecutive threads walk down one seam (a row-major order was 2.6x slower)
            const unsigned k = i / (unsigned)H, y = i - k * (unsigned)H, x = (k + 1) * CT_W;
            const long long p = (long long)y * W + x;
            if (fg[p] == val && fg[p - 1] == val) {
                a = (int)p;
                b = (int)p - 1;
            }
        } else if (i < total) {  // consecutive threads: consecutive pixels of one seam row
            const unsigned j = i - nv;
            const unsigned k = j / (unsigned)W, x = j - k * (unsigned)W, y = (k + 1) * CT_H;
            const long long p = (long long)y * W + x;
            if (fg[p] == val && fg[p - W] == val) {
                const bool edge = (x % CT_W) == 0;
                const bool low_starts = edge || fg[p - 1] != val, up_starts = edge || fg[p - W - 1] != val;
                if (low_starts || up_starts) {
                    a = (int)p;
                    b = (int)(p - W);
                }
            }
        }
        seam_union_runs(L, a, b, ca, cb, lane, [](int* l, int x, int y) { uf_union(l, x, y); });
    }
}
int pp_ccl_run(const uint8_t* fg, uint8_t val, int* L, int H, int W, hipStream_t st, int* area) {
    const int n = H * W;
    const int tiles_x = (W + CT_W - 1) / CT_W, tiles_y = (H + CT_H - 1) / CT_H;
    const int n_tiles = tiles_x * tiles_y;
    hipLaunchKernelGGL(ccl_tile_kernel<false>, dim3(n_tiles < 256 * 16 ? n_tiles : 256 * 16), dim3(256), 0, st, fg, val, L, H, W, tiles_x, n_tiles, (int*)nullptr,
                       (int*)nullptr, (int*)nullptr);
    const long long seams = (long long)(tiles_x - 1) * H + (long long)(tiles_y - 1) * W;
    if (seams > 0) hipLaunchKernelGGL(ccl_seam_kernel, dim3(grid_for(seams)), dim3(256), 0, st, fg, val, L, H, W, tiles_x, tiles_y);
    if (area) hipLaunchKernelGGL(ccl_flatten_area_kernel, dim3(grid_for(n)), dim3(256), 0, st, L, area, n);
    else hipLaunchKernelGGL(ccl_flatten_kernel, dim3(grid_for(n)), dim3(256), 0, st, L, n);
    KCHECK();
    return 0;
}

// =================================================================================================================
// Two-colour labelling of the nuclei MARKER image (round 5).  loader/postproc.py:370-377 is
//     label(inner > 0.5) -> remove_small_objects(4) -> binary_fill_holes -> label
// which round 4 ran as THREE union-find labellings (markers; their background, for the holes; the filled markers).  Here the marker image is
// labelled ONCE in both colours (a pixel is united with its 4-neighbours of the SAME colour), and the two later steps are edits of that one forest:
//   * a foreground component smaller than min_size turns into background: its pixels are united with their background neighbours;
//   * a background component that does not touch the image border is a hole: its pixels turn into foreground and are united with their
//     foreground neighbours (this is also what merges two markers that only touched diagonally around a hole).
// Roots stay "smallest raster index of the set", so the rank of a final root among all roots is scipy's label id as before.
// =================================================================================================================
// `roots` / `cnt`: every pixel that is the root of its tile-local set goes to its tile's range of a root list (tile_list_base; cnt[tile] entries).  All later unions link
// roots under roots, so the nodes of the forest above the pixel level are exactly these: flattening the LIST (ccl2_flatten_roots_kernel) makes
// L[L[p]] the set's root for every pixel p -- two loads, no pointer chase, no pass that walks 67 M background pixels up to one giant root.
__global__ __launch_bounds__(256) void ccl2_tile_kernel(const uint8_t* __restrict__ fg, int* __restrict__ L, int H, int W, int tiles_x, int n_tiles,
                                                        int* __restrict__ roots, int* __restrict__ cnt, int* __restrict__ area, int* __restrict__ colbuf) {
    __shared__ int swtot[4];
    __shared__ int sl[CT_H * CT_W];
    __shared__ int scnt[CT_H * CT_W];  // FOREGROUND pixels of every tile-local set (background sets stay at 0: ccl2_drop_small_kernel relies on it)
    __shared__ u64 sc[CT_H], sv[CT_H], ss[CT_H];  // per row: colour bits, valid bits, run starts
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int tx0 = (tile % tiles_x) * CT_W, ty0 = (tile / tiles_x) * CT_H;
        const int x = tx0 + lane;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = wave * 8 + i, y = ty0 + r;
            const bool v = x < W && y < H;
            const bool f = v && fg[(long long)y * W + x] != 0;
            const u64 c = __ballot(f), vm = __ballot(v);
            const u64 starts = ((c ^ (c << 1)) | 1ull) & vm;  // a run starts where the colour changes (pixels beyond the image sit at the right end only)
            sl[r * CT_W + lane] = v ? r * CT_W + 63 - __clzll((long long)(starts & ((2ull << lane) - 1))) : -1;
            scnt[r * CT_W + lane] = 0;
            if (lane == 0) {
                sc[r] = c;
                sv[r] = vm;
                ss[r] = starts;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = wave * 8 + i;
            if (r == 0) continue;
            const u64 both = ~(sc[r] ^ sc[r - 1]) & sv[r] & sv[r - 1];
            const u64 first = both & (ss[r] | ss[r - 1]);  // the lower run starts here, or the upper one does
            if ((first >> lane) & 1) lds_union(sl, r * CT_W + lane, (r - 1) * CT_W + lane);
        }
        __syncthreads();
        u64 rmv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = wave * 8 + i, y = ty0 + r;
            bool is_root = false;
            if (x < W && y < H) {
                const int root = lds_find(sl, sl[r * CT_W + lane]);
                const int g = (ty0 + (root >> 6)) * W + tx0 + (root & 63);
                L[(long long)y * W + x] = g;
                is_root = root == r * CT_W + lane;
                const u64 c = sc[r];
                // border columns for the seam pass (see ccl_seam_kernel): the tile root, the pixel's colour in bit 31 (indices stay below 2^31)
                const int gc = g | (int)(((c >> lane) & 1ull) << 31);
                if (lane == 0 && tx0 > 0) colbuf[(long long)(tx0 / CT_W - 1) * H + y] = gc;
                if (lane == CT_W - 1 && tx0 + CT_W < W) colbuf[(long long)(tiles_x - 1) * H + (long long)(tx0 / CT_W) * H + y] = gc;
                if (((c & ss[r]) >> lane) & 1ull) {  // first pixel of a foreground run: its length (the colour bits beyond the image are 0)
                    const u64 rest = ~(c >> lane);
                    atomicAdd(&scnt[root], rest ? __ffsll((long long)rest) - 1 : 64 - lane);
                }
            }
            rmv[i] = __ballot(is_root);
        }
        __syncthreads();  // every set's counter is complete
        {   // the tile's roots go to the tile's OWN range of the list (tile_list_base: as many slots as the tile has pixels) and their number to
            // cnt[tile] -- a shared list head took one returning atomic per tile on ONE address: 33 k of them cost 0.1 ms, 131 k (one per wave) 0.4 ms
            int tot = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) tot += __popcll(rmv[i]);
            if (lane == 0) swtot[wave] = tot;
            __syncthreads();
            int base = tile_list_base(tx0, ty0, H, W);
            for (int w = 0; w < wave; ++w) base += swtot[w];
            if (tid == 0) cnt[tile] = swtot[0] + swtot[1] + swtot[2] + swtot[3];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int r = wave * 8 + i, y = ty0 + r;
                if ((rmv[i] >> lane) & 1ull) {
                    roots[base + __popcll(rmv[i] & ((1ull << lane) - 1))] = y * W + x;
                    area[(long long)y * W + x] = scnt[r * CT_W + lane];
                }
                base += __popcll(rmv[i]);
            }
        }
        __syncthreads();  // (sl / scnt / swtot are rewritten by the next tile)
    }
}
// L[r] = root of r for every node of the forest above the pixel level (see ccl2_tile_kernel)
// zero (optional): an int map that is only ever read at roots (the border flags of the two-colour labelling) is cleared at the LIST's entries here -- every
// root there will ever be is one of them -- instead of by a whole-map fill (4 B/px of a call's 82: round 6)
__global__ void ccl2_flatten_roots_kernel(int* L, const int* __restrict__ roots, const int* __restrict__ cnt, int n_tiles, int tiles_x, int H, int W,
                                          int* __restrict__ zero = nullptr) {
    const int lane = threadIdx.x & 63, nwaves = gridDim.x * (blockDim.x >> 6);
    for (int tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); tile < n_tiles; tile += nwaves) {
        const int c = cnt[tile], base = tile_list_base((tile % tiles_x) * CT_W, (tile / tiles_x) * CT_H, H, W);
        for (int k = lane; k < c; k += 64) {
            const int r = roots[base + k];
            if (zero) zero[r] = 0;
            const int f = uf_find(L, r);
            if (f != r) __hip_atomic_store(&L[r], f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
__global__ void ccl2_seam_kernel(const uint8_t* __restrict__ fg, int* L, int H, int W, int tiles_x, int tiles_y, const int* __restrict__ cols) {
    const unsigned sx = (unsigned)(tiles_x - 1), sy = (unsigned)(tiles_y - 1);
    const unsigned nv = sx * (unsigned)H, nh = sy * (unsigned)W;
    const unsigned total = nv + nh, stride = gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (unsigned i0 = blockIdx.x * blockDim.x + threadIdx.x - lane; i0 < total; i0 += stride) {
        const unsigned i = i0 + lane;
        int a = -1, b = -1;
        int ca = -1, cb = -1;  // vertical seam through the compact columns (two colours: bit 31)
        if (i < nv) {
            const int va = cols[i], vb = cols[nv + i];
            if ((va ^ vb) >= 0) {  // same colour
                ca = va & 0x7fffffff;
                cb = vb & 0x7fffffff;
            }
        } else if (i < total) {
            const unsigned j = i - nv;
            const unsigned k = j / (unsigned)W, x = j - k * (unsigned)W, y = (k + 1) * CT_H;
            const long long p = (long long)y * W + x;
            const bool c = fg[p] != 0;
            if (c == (fg[p - W] != 0)) {
                const bool edge = (x % CT_W) == 0;
                const bool low_starts = edge || (fg[p - 1] != 0) != c, up_starts = edge || (fg[p - W - 1] != 0) != c;
                if (low_starts || up_starts) {
                    a = (int)p;
                    b = (int)(p - W);
                }
            }
        }
        seam_union_runs(L, a, b, ca, cb, lane, [](int* l, int x, int y) { uf_union_relaxed(l, x, y); });
    }
}
// unite pixel p = (y, x) with those of its four neighbours whose byte reads as colour c (true: not 0)
__device__ __forceinline__ void unite_with_neighbours(const uint8_t* m, int* L, long long p, int y, int x, int H, int W, bool c) {
    if (x > 0 && (m[p - 1] != 0) == c) uf_union(L, (int)p, (int)p - 1);
    if (x < W - 1 && (m[p + 1] != 0) == c) uf_union(L, (int)p, (int)p + 1);
    if (y > 0 && (m[p - W] != 0) == c) uf_union(L, (int)p, (int)(p - W));
    if (y < H - 1 && (m[p + W] != 0) == c) uf_union(L, (int)p, (int)(p + W));
}
// foreground components below min_size turn into background and join the background sets around them
__global__ void ccl2_drop_small_kernel(uint8_t* m, int* L, const int* __restrict__ area, int min_size, int H, int W) {
    const long long n = (long long)H * W;
    const double invW = 1.0 / (double)W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        if (!m[p]) continue;
        const int r = L[L[p]];  // the component's root as the area merge saw it -- or, once this small component has been united away, a
        if (area[r] >= min_size) continue;  // background index, whose area is 0: "small" either way
        int y, x;
        pix_yx(p, W, invW, y, x);
        m[p] = 0;
        // (a neighbour that reads as background is background or a pixel of this same small component: uniting with either is right)
        unite_with_neighbours(m, L, p, y, x, H, W, false);
    }
}
__global__ void ccl2_mark_border_kernel(const uint8_t* __restrict__ m, const int* L, int* __restrict__ border, int H, int W) {
    const int per = 2 * (H + W);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < per; i += gridDim.x * blockDim.x) {
        const long long p = perimeter_pixel(i, H, W);
        if (!m[p]) border[uf_find(L, (int)p)] = 1;
    }
}
// background sets that do not reach the border are holes: their pixels become foreground and join the foreground sets around them
// (border[] is 1 only at the roots of border-touching background sets, which nothing is united with here; every other index reads 0)
__global__ void ccl2_fill_kernel(uint8_t* m, int* L, const int* __restrict__ border, int H, int W) {
    const long long n = (long long)H * W;
    const double invW = 1.0 / (double)W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        if (m[p]) continue;
        if (border[uf_find(L, (int)p)]) continue;
        int y, x;
        pix_yx(p, W, invW, y, x);
        m[p] = 1;
        // (a neighbour that reads as foreground is foreground or a pixel of this same hole that was filled a moment ago: uniting with either is right)
        unite_with_neighbours(m, L, p, y, x, H, W, true);
    }
}
// final marker labels: root for foreground pixels, -1 for the background, and bits[p >> 6] |= "p is the root of a marker" (whole waves step
// together: the ballot covers 64 consecutive pixels)
__global__ void ccl2_final_bits_kernel(int* L, const uint8_t* __restrict__ m, int n, u64* __restrict__ bits) {
    // (flattened roots: L[L[p]] is the root; a foreground node that other pixels still point at keeps the value it already holds)
    const int lane = threadIdx.x & 63;
    for (long long base = (blockIdx.x * (long long)blockDim.x + threadIdx.x) - lane; base < n; base += (long long)gridDim.x * blockDim.x) {
        const long long p = base + lane;
        int r = -1;
        if (p < n) {
            r = m[p] ? L[L[p]] : -1;
            L[p] = r;
        }
        const u64 b = __ballot(r == (int)p && p < n);
        if (lane == 0) bits[base >> 6] = b;
    }
}
// ---- four pixels per thread (see nuc_marker_out4_kernel for why) -------------------------------------------------
// 16 consecutive lanes hold 64 consecutive pixels: their 4-bit root flags make one bitmap word (every lane of the wave calls this)
__device__ __forceinline__ void store_root_bits4(u64* __restrict__ bits, long long q, long long nq, unsigned nib, int lane) {
    u64 v = (u64)nib << (4 * (lane & 15));
    v |= __shfl_xor(v, 1);
    v |= __shfl_xor(v, 2);
    v |= __shfl_xor(v, 4);
    v |= __shfl_xor(v, 8);
    if ((lane & 15) == 0 && q < nq) bits[q >> 4] = v;
}
__global__ void ccl2_drop_small4_kernel(uint32_t* m4, int4* L4, const int* __restrict__ area, int min_size, int H, int W) {
    const long long nq = (long long)H * W / 4;
    const int qw = W / 4;
    const double invQ = 1.0 / (double)qw;
    uint8_t* m = (uint8_t*)m4;
    int* L = (int*)L4;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
        const uint32_t mw = m4[q];
        if (!mw) continue;
        const int4 l = L4[q];
        const int t[4] = {l.x, l.y, l.z, l.w};
        int pt = -1;
        bool small = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!((mw >> (8 * i)) & 0xffu)) continue;
            if (t[i] != pt) {  // (pixels of one tile-local set share the decision; see ccl2_drop_small_kernel for the races that do not matter)
                pt = t[i];
                small = area[L[pt]] < min_size;
            }
            if (!small) continue;
            int y, xq;
            pix_yx(q, qw, invQ, y, xq);
            const int x = xq * 4 + i;
            const long long p = q * 4 + i;
            m[p] = 0;
            unite_with_neighbours(m, L, p, y, x, H, W, false);
        }
    }
}
// The fill with four pixels per thread, gated per TILE (round 6): a hole is a background set that does not reach the border, and every pixel of it belongs to a tile-local set whose
// tile root sits in that tile's range of the root list -- so a tile none of whose list entries is background with an unflagged root holds no hole pixel and is
// skipped without touching its labels (holes are rare: 5.0 -> ~0.5 B/px of a call, the pass 0.155 -> ~0.03 ms at 8192^2).  One wave per tile; the list is flat
// here (ccl2_flatten_roots_kernel ran after the last unions), so L[entry] is the entry's root.
__global__ void ccl2_fill_tiles4_kernel(uint32_t* m4, int4* L4, const int* __restrict__ border, const int* __restrict__ roots, const int* __restrict__ cnt, int n_tiles,
                                        int tiles_x, int H, int W) {
    const int lane = threadIdx.x & 63, nwaves = gridDim.x * (blockDim.x >> 6);
    const int qw = W / 4;
    uint8_t* m = (uint8_t*)m4;
    int* L = (int*)L4;
    for (int tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); tile < n_tiles; tile += nwaves) {
        const int tx0 = (tile % tiles_x) * CT_W, ty0 = (tile / tiles_x) * CT_H;
        const int c = cnt[tile], base = tile_list_base(tx0, ty0, H, W);
        bool any = false;
        for (int k0 = 0; k0 < c; k0 += 64) {  // (wave-uniform trip count)
            const int k = k0 + lane;
            bool h = false;
            if (k < c) {
                const int r = roots[base + k];
                h = !m[r] && !border[L[r]];
            }
            any = any || (__ballot(h) != 0ull);
        }
        if (!any) continue;
        const int rows = H - ty0 < CT_H ? H - ty0 : CT_H, qpr = (W - tx0 < CT_W ? W - tx0 : CT_W) / 4;  // quads per tile row (W % 4 == 0)
        for (int idx = lane; idx < rows * qpr; idx += 64) {
            const int y = ty0 + idx / qpr, xq = tx0 / 4 + idx % qpr;
            const long long q = (long long)y * qw + xq;
            const uint32_t mw = m4[q];
            if (mw == 0x01010101u) continue;
            const int4 l = L4[q];
            const int t[4] = {l.x, l.y, l.z, l.w};
            int pt = -1;
            bool hole = false;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if ((mw >> (8 * i)) & 0xffu) continue;
                if (t[i] != pt) {
                    pt = t[i];
                    hole = !border[uf_find(L, pt)];
                }
                if (!hole) continue;
                const int x = xq * 4 + i;
                const long long p = q * 4 + i;
                m[p] = 1;
                unite_with_neighbours(m, L, p, y, x, H, W, true);
            }
        }
    }
}
__global__ void ccl2_final_bits4_kernel(int4* L4, const uint32_t* __restrict__ m4, long long nq, u64* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int* L = (const int*)L4;
    for (long long q0 = (blockIdx.x * (long long)blockDim.x + threadIdx.x) - lane; q0 < nq; q0 += (long long)gridDim.x * blockDim.x) {
        const long long q = q0 + lane;
        unsigned nib = 0;
        if (q < nq) {
            const uint32_t mw = m4[q];
            int r[4] = {-1, -1, -1, -1};
            if (mw) {
                const int4 l = L4[q];
                const int t[4] = {l.x, l.y, l.z, l.w};
                int pt = -1, pr = -1;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (!((mw >> (8 * i)) & 0xffu)) continue;
                    if (t[i] != pt) {
                        pt = t[i];
                        pr = L[pt];
                    }
                    r[i] = pr;
                    if (pr == (int)(q * 4 + i)) nib |= 1u << i;
                }
                L4[q] = make_int4(r[0], r[1], r[2], r[3]);  // (round 6: quads without a marker pixel keep whatever they held -- nuc_marker_out4_kernel asks the marker bytes first)
            }
        }
        store_root_bits4(bits, q, nq, nib, lane);
    }
}
// mask side: m = "the pixel's component has at least min_size pixels", L[p] <- its root (the list is flat: L[L[p]]), bitmap of the kept roots
__global__ void apply_min_area_bits4_kernel(uint32_t* __restrict__ m4, int4* L4, const int* __restrict__ area, int min_size, long long nq, u64* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int* L = (const int*)L4;
    for (long long q0 = (blockIdx.x * (long long)blockDim.x + threadIdx.x) - lane; q0 < nq; q0 += (long long)gridDim.x * blockDim.x) {
        const long long q = q0 + lane;
        unsigned nib = 0;
        if (q < nq && m4[q]) {  // (round 6: the eroded mask's own bytes say where the labelling has labels -- the int32 map is read for those quads only)
            const int4 l = L4[q];
            uint32_t mw = 0;
            if (l.x >= 0 || l.y >= 0 || l.z >= 0 || l.w >= 0) {
                const int t[4] = {l.x, l.y, l.z, l.w};
                int r[4] = {-1, -1, -1, -1};
                int pt = -1, pr = -1;
                bool keep = false;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (t[i] < 0) continue;
                    if (t[i] != pt) {
                        pt = t[i];
                        pr = L[pt];
                        keep = area[pr] >= min_size;
                    }
                    r[i] = pr;
                    if (keep) {
                        mw |= 1u << (8 * i);
                        if (pr == (int)(q * 4 + i)) nib |= 1u << i;
                    }
                }
                L4[q] = make_int4(r[0], r[1], r[2], r[3]);
            }
            m4[q] = mw;
        }
        store_root_bits4(bits, q, nq, nib, lane);
    }
}
// (pp_common.h) roots: H * W ints (every tile its own range), n_roots: one int per tile
// root_bits: bitmap of the final markers' roots; colbuf: 2 x (tiles_x - 1) x H ints for the seam columns; wide: four pixels per thread (W % 4 == 0)
int pp_markers_two_colour(uint8_t* mrk, int* L, int* area, int* border, int* roots, int* n_roots, int min_size, int H, int W, hipStream_t st,
                              u64* root_bits, bool wide, int* colbuf) {
    const int n = H * W;
    const int tiles_x = (W + CT_W - 1) / CT_W, tiles_y = (H + CT_H - 1) / CT_H, n_tiles = tiles_x * tiles_y;
    const unsigned g = grid_for(n);
    // (area: written by the tile kernel at every tile-local root, read at roots only -- no zero fill; border: read at roots only as well, cleared at the
    //  root list's entries by the first flatten pass below)
    hipLaunchKernelGGL(ccl2_tile_kernel, dim3(n_tiles < 256 * 16 ? n_tiles : 256 * 16), dim3(256), 0, st, mrk, L, H, W, tiles_x, n_tiles, roots, n_roots, area, colbuf);
    const long long seams = (long long)(tiles_x - 1) * H + (long long)(tiles_y - 1) * W;
    if (seams > 0) hipLaunchKernelGGL(ccl2_seam_kernel, dim3(grid_for(seams)), dim3(256), 0, st, mrk, L, H, W, tiles_x, tiles_y, (const int*)colbuf);
    const unsigned gl = nblk(n_tiles, 4) < 4096 ? nblk(n_tiles, 4) : 4096;  // one wave per tile
    auto flatten_roots = [&]() { hipLaunchKernelGGL(ccl2_flatten_roots_kernel, dim3(gl), dim3(256), 0, st, L, (const int*)roots, (const int*)n_roots, n_tiles, tiles_x, H, W, (int*)nullptr); };
    hipLaunchKernelGGL(ccl2_flatten_roots_kernel, dim3(gl), dim3(256), 0, st, L, (const int*)roots, (const int*)n_roots, n_tiles, tiles_x, H, W, border);
    hipLaunchKernelGGL(roots_area_merge_kernel, dim3(gl), dim3(256), 0, st, (const int*)L, (const int*)roots, (const int*)n_roots, n_tiles, tiles_x, H, W, area);
    const unsigned g4 = grid_for(n / 4);
    if (wide) hipLaunchKernelGGL(ccl2_drop_small4_kernel, dim3(g4), dim3(256), 0, st, (uint32_t*)mrk, (int4*)L, area, min_size, H, W);
    else hipLaunchKernelGGL(ccl2_drop_small_kernel, dim3(g), dim3(256), 0, st, mrk, L, area, min_size, H, W);
    flatten_roots();
    hipLaunchKernelGGL(ccl2_mark_border_kernel, dim3(nblk(2 * (H + W), 256)), dim3(256), 0, st, mrk, L, border, H, W);
    if (wide) hipLaunchKernelGGL(ccl2_fill_tiles4_kernel, dim3(gl), dim3(256), 0, st, (uint32_t*)mrk, (int4*)L, border, (const int*)roots, (const int*)n_roots, n_tiles, tiles_x, H, W);
    else hipLaunchKernelGGL(ccl2_fill_kernel, dim3(g), dim3(256), 0, st, mrk, L, border, H, W);
    flatten_roots();
    if (wide) hipLaunchKernelGGL(ccl2_final_bits4_kernel, dim3(g4), dim3(256), 0, st, (int4*)L, (const uint32_t*)mrk, (long long)n / 4, root_bits);
    else hipLaunchKernelGGL(ccl2_final_bits_kernel, dim3(g), dim3(256), 0, st, L, mrk, n, root_bits);
    KCHECK();
    return 0;
}

// flag[p] = 1 for roots of components with area >= min_size (0 otherwise / non-roots)
__global__ void ccl_keep_roots_kernel(const int* __restrict__ L, const int* __restrict__ area, int min_size, int* __restrict__ flag, int n) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x)
        flag[p] = (L[p] == (int)p && area[p] >= min_size) ? 1 : 0;
}
// out[p] = 1 + rank[root] for pixels of kept components (rank = exclusive scan of the root flags), 0 elsewhere
__global__ void ccl_relabel_kernel(const int* __restrict__ L, const int* __restrict__ flag, const int* __restrict__ rank, int* __restrict__ out, int n) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x) {
        const int r = L[p];
        out[p] = (r >= 0 && flag[r]) ? rank[r] + 1 : 0;
    }
}
__global__ void count_from_scan_kernel(const int* __restrict__ flag, const int* __restrict__ rank, int n, int* __restrict__ out,
                                       const int* __restrict__ any) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = (any && !*any) ? -1 : (n > 0 ? rank[n - 1] + flag[n - 1] : 0);
}
// m[p] &= area[root(p)] >= min_size, and bits[p >> 6] |= "p is the root of a kept component"
__global__ void apply_min_area_bits_kernel(uint8_t* __restrict__ m, const int* __restrict__ L, const int* __restrict__ area, int min_size, int n,
                                           u64* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    for (long long base = (blockIdx.x * (long long)blockDim.x + threadIdx.x) - lane; base < n; base += (long long)gridDim.x * blockDim.x) {
        const long long p = base + lane;
        bool root = false;
        if (p < n) {
            const int r = L[p];
            const bool keep = r >= 0 && area[r] >= min_size;
            m[p] = keep ? 1 : 0;
            root = keep && r == (int)p;
        }
        const u64 b = __ballot(root);
        if (lane == 0) bits[base >> 6] = b;
    }
}

int pp_label_tiles(int H, int W) { return ((W + CT_W - 1) / CT_W) * ((H + CT_H - 1) / CT_H); }
int pp_label_mask_min_area(uint8_t* msk, int* L, int* area, int min_size, int H, int W, hipStream_t st, u64* root_bits, bool wide, int* roots, int* n_roots,
                           int* colbuf) {
    const int n = H * W;
    if (!wide) {
        PP_OK(hipMemsetAsync(area, 0, (size_t)n * 4, st));
        if (pp_ccl_run(msk, 1, L, H, W, st, area)) return 1;
        hipLaunchKernelGGL(apply_min_area_bits_kernel, dim3(grid_for(n)), dim3(256), 0, st, msk, (const int*)L, (const int*)area, min_size, n, root_bits);
        return 0;
    }
    // tile labelling with the root list + per-set counts, flatten and areas over the LIST, then one pass: min-area, root of every pixel, bitmap
    const int tiles_x = (W + CT_W - 1) / CT_W, tiles_y = (H + CT_H - 1) / CT_H, n_tiles = tiles_x * tiles_y;
    hipLaunchKernelGGL(ccl_tile_kernel<true>, dim3(n_tiles < 256 * 16 ? n_tiles : 256 * 16), dim3(256), 0, st, (const uint8_t*)msk, (uint8_t)1, L, H, W, tiles_x, n_tiles,
                       roots, n_roots, area, colbuf);
    const long long seams = (long long)(tiles_x - 1) * H + (long long)(tiles_y - 1) * W;
    if (seams > 0) hipLaunchKernelGGL(ccl_seam_kernel, dim3(grid_for(seams)), dim3(256), 0, st, (const uint8_t*)msk, (uint8_t)1, L, H, W, tiles_x, tiles_y, (const int*)colbuf);
    const unsigned gl = nblk(n_tiles, 4) < 4096 ? nblk(n_tiles, 4) : 4096;
    hipLaunchKernelGGL(ccl2_flatten_roots_kernel, dim3(gl), dim3(256), 0, st, L, (const int*)roots, (const int*)n_roots, n_tiles, tiles_x, H, W);
    hipLaunchKernelGGL(roots_area_merge_kernel, dim3(gl), dim3(256), 0, st, (const int*)L, (const int*)roots, (const int*)n_roots, n_tiles, tiles_x, H, W, area);
    hipLaunchKernelGGL(apply_min_area_bits4_kernel, dim3(grid_for(n / 4)), dim3(256), 0, st, (uint32_t*)msk, (int4*)L, (const int*)area, min_size, (long long)n / 4, root_bits);
    KCHECK();
    return 0;
}
int pp_label_ranked(const uint8_t* fg, int* L, int* area, int min_size, int* flag, int* rank, int* scantmp, int* out, int* n_out, int H, int W, hipStream_t st) {
    const int n = H * W;
    const unsigned g = grid_for(n);
    if (area) PP_OK(hipMemsetAsync(area, 0, (size_t)n * 4, st));
    if (pp_ccl_run(fg, 1, L, H, W, st, area)) return 1;
    if (area) hipLaunchKernelGGL(ccl_keep_roots_kernel, dim3(g), dim3(256), 0, st, (const int*)L, (const int*)area, min_size, flag, n);
    else hipLaunchKernelGGL(ccl_keep_roots_kernel, dim3(g), dim3(256), 0, st, (const int*)L, (const int*)L, INT_MIN, flag, n);  // every root: area test always true
    if (pp_scan_exclusive(flag, rank, n, scantmp, st)) return 1;
    hipLaunchKernelGGL(ccl_relabel_kernel, dim3(g), dim3(256), 0, st, (const int*)L, (const int*)flag, (const int*)rank, out, n);
    hipLaunchKernelGGL(count_from_scan_kernel, dim3(1), dim3(1), 0, st, (const int*)flag, (const int*)rank, n, n_out, (const int*)nullptr);
    KCHECK();
    return 0;
}

// =================================================================================================================
// Tissue-mask regions (infer/wsi.py:724 `measurements.label(wsi_mask)`): 4-connected components of mask != 0,
// ids in raster order of each component's first pixel (scipy.ndimage.label's order).
// =================================================================================================================
__global__ void binarize_kernel(const uint8_t* __restrict__ m, long long row_stride, int H, int W, uint8_t* __restrict__ fg) {
    const long long n = (long long)H * W;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n; p += (long long)gridDim.x * blockDim.x)
        fg[p] = m[(p / W) * row_stride + (p % W)] != 0 ? 1 : 0;
}
extern "C" int cerb_label_mask(const uint8_t* mask, long long row_stride, int H, int W, int32_t* labels_out, int32_t* n_out, void* ws,
                               size_t ws_bytes, void* hip_stream) {
    if (int rc = pp_check_map("cerb_label_mask", mask && labels_out && n_out && ws, H, W, ws_bytes, cerb_pp_workspace_bytes(H, W))) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const int n = H * W;
    Carve cv{(char*)ws, ws_bytes};
    int* L = (int*)cv.take((size_t)n * 4);
    int* flag = (int*)cv.take((size_t)n * 4);
    int* rank = (int*)cv.take((size_t)n * 4);
    uint8_t* fg = (uint8_t*)cv.take(n);
    int* scantmp = (int*)cv.take((size_t)(n / SCAN_ITEMS + 4096) * 4 * 2);
    if (!scantmp) return cerb_set_error("cerb_label_mask: workspace carve failed");
    hipLaunchKernelGGL(binarize_kernel, dim3(grid_for(n)), dim3(256), 0, st, mask, row_stride, H, W, fg);
    return pp_label_ranked(fg, L, nullptr, 0, flag, rank, scantmp, labels_out, n_out, H, W, st);
}
