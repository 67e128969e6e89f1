// Instance morphometry and gland-level relations on gfx950 (include/cerberus_hip.h: cerb_inst_shape, cerb_inst_hull_rows, cerb_inst_relate,
// cerb_points_knn; cerberus_amd/inst_features.py).  The second segmented reduction over a label map, after cerb_inst_table's:
//   cerb_inst_shape      raw second moments about the box corner, crack length and border pixels per instance.  Lanes of a wave are consecutive
//                        pixels, so equal labels form RUNS along a row; the run heads are balloted and ONE lane per run issues the atomics:
//                        the three moments of a run are closed forms of (first x, length, row), crack and border are popcounts of five ballots
//                        under the run's lane mask -- no shuffle, no per-pixel atomic.  The wave-uniform case of inst_table_kernel is one run.
//   cerb_inst_hull_rows  pass 1: leftmost / rightmost x of every instance in every row of its box (one atomicMin + one atomicMax per run);
//                        pass 2: one thread per instance, monotone chains over the left and the right ends, in place.
//   cerb_inst_relate     one thread per child instance: the parent under its integer centroid, counters per parent.
//   cerb_points_knn      brute force: candidate tiles through LDS, k best per thread in registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>
#include <string>

#include "../../include/cerberus_hip.h"
#include "cerb_dev.h"

int cerb_set_error(const std::string& m);

#define IF_CHECK()                                                                                    \
    do {                                                                                              \
        hipError_t e_ = hipGetLastError();                                                            \
        if (e_ != hipSuccess) return cerb_set_error(std::string("kernel launch: ") + hipGetErrorString(e_)); \
    } while (0)

static unsigned if_grid(long long n, int block = 256, long long cap = 256 * 16) {
    long long b = (n + block - 1) / block;
    if (b > cap) b = cap;
    return (unsigned)(b < 1 ? 1 : b);
}

__global__ void if_fill_ll_kernel(long long* __restrict__ p, long long n, long long v) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = v;
}

// One wave = 64 consecutive pixels in raster order.  -> the pixel's validated label, its (y, x), whether this lane starts a run (first lane, first
// pixel of a row, or a label other than the lane before) and the lane mask [lane, end) of the run it starts.
struct RunLane {
    int y, x, l;
    bool head;
    unsigned long long mask;
    int len;
};
__device__ __forceinline__ RunLane run_lane(const int* __restrict__ lab, long long stride, int W, int n_inst, long long p, long long n, int lane) {
    RunLane r;
    r.y = 0;
    r.x = 1;  // (a lane past the map: background, never a row start)
    r.l = 0;
    if (p < n) {
        r.y = (int)(p / W);
        r.x = (int)(p % W);
        const int v = lab[(long long)r.y * stride + r.x];
        r.l = (v < 0 || v > n_inst) ? 0 : v;
    }
    const int prev = __shfl_up(r.l, 1);
    r.head = lane == 0 || r.x == 0 || prev != r.l;
    const unsigned long long heads = __ballot(r.head);
    const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
    const int end = rest ? lane + 1 + (__ffsll((long long)rest) - 1) : 64;
    r.len = end - lane;
    r.mask = (end == 64 ? ~0ull : ((1ull << end) - 1ull)) & ~((1ull << lane) - 1ull);
    return r;
}

// PER_PIXEL: the naive form, every foreground pixel issuing its own atomics -- the developers' library only (CERB_INST_SHAPE_PER_PIXEL), as the other
// side of scripts/dev_inst_features_time.py's A/B.
template <bool PER_PIXEL>
__global__ void inst_shape_kernel(const int* __restrict__ lab, long long stride, int H, int W, int n_inst, const long long* __restrict__ table,
                                  unsigned long long* __restrict__ shape) {
    const long long n = (long long)H * W;
    const int lane = threadIdx.x & 63;
    for (long long p0 = (blockIdx.x * (long long)blockDim.x + threadIdx.x) - lane; p0 < n; p0 += (long long)gridDim.x * blockDim.x) {
        const RunLane r = run_lane(lab, stride, W, n_inst, p0 + lane, n, lane);
        if (!__ballot(r.l != 0)) continue;
        bool up = false, down = false, left = false, right = false;
        if (r.l) {
            auto other = [&](int yy, int xx) {
                if (yy < 0 || yy >= H || xx < 0 || xx >= W) return true;
                const int v = lab[(long long)yy * stride + xx];
                return ((v < 0 || v > n_inst) ? 0 : v) != r.l;
            };
            up = other(r.y - 1, r.x);
            down = other(r.y + 1, r.x);
            left = other(r.y, r.x - 1);
            right = other(r.y, r.x + 1);
        }
        if (PER_PIXEL) {
            if (r.l) {
                const long long* t = table + 16ll * (r.l - 1);
                const long long dx = r.x - t[5], dy = r.y - t[3];
                const int crack = (int)up + (int)down + (int)left + (int)right;
                unsigned long long* s = shape + 8ll * (r.l - 1);
                atomicAdd(s + 0, (unsigned long long)(dx * dx));
                atomicAdd(s + 1, (unsigned long long)(dy * dy));
                atomicAdd(s + 2, (unsigned long long)(dx * dy));
                if (crack) {
                    atomicAdd(s + 3, (unsigned long long)crack);
                    atomicAdd(s + 4, 1ull);
                }
            }
            continue;
        }
        const unsigned long long bu = __ballot(up), bd = __ballot(down), bl = __ballot(left), br = __ballot(right);
        if (r.head && r.l) {
            const long long* t = table + 16ll * (r.l - 1);
            const long long len = r.len, a = r.x - t[5], dy = r.y - t[3];
            // sum over k < len of (a + k), (a + k)^2
            const long long s1 = len * a + len * (len - 1) / 2;
            const long long s2 = len * a * a + a * len * (len - 1) + (len - 1) * len * (2 * len - 1) / 6;
            const int crack = __popcll(bu & r.mask) + __popcll(bd & r.mask) + __popcll(bl & r.mask) + __popcll(br & r.mask);
            const int border = __popcll((bu | bd | bl | br) & r.mask);
            unsigned long long* s = shape + 8ll * (r.l - 1);
            atomicAdd(s + 0, (unsigned long long)s2);
            atomicAdd(s + 1, (unsigned long long)(len * dy * dy));
            atomicAdd(s + 2, (unsigned long long)(dy * s1));
            if (crack) {
                atomicAdd(s + 3, (unsigned long long)crack);
                atomicAdd(s + 4, (unsigned long long)border);
            }
        }
    }
}

extern "C" int cerb_inst_shape(const int32_t* labels, long long lab_row_stride, int h, int w, int n_inst, const long long* table, long long* shape,
                               void* hip_stream) {
    if (!labels || h <= 0 || w <= 0 || n_inst < 0 || (n_inst > 0 && (!table || !shape))) return cerb_set_error("cerb_inst_shape: bad arguments");
    if (n_inst == 0) return 0;
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(if_fill_ll_kernel, dim3(if_grid(8ll * n_inst)), dim3(256), 0, st, shape, 8ll * n_inst, 0ll);
    // developer A/B, read at every call so that one process can alternate the two forms; folds to false in the product library
    const bool per_pixel = cerb_dev_getenv("CERB_INST_SHAPE_PER_PIXEL") != nullptr;
    if (per_pixel)
        hipLaunchKernelGGL(inst_shape_kernel<true>, dim3(if_grid((long long)h * w)), dim3(256), 0, st, labels, lab_row_stride, h, w, n_inst, table,
                           (unsigned long long*)shape);
    else
        hipLaunchKernelGGL(inst_shape_kernel<false>, dim3(if_grid((long long)h * w)), dim3(256), 0, st, labels, lab_row_stride, h, w, n_inst, table,
                           (unsigned long long*)shape);
    IF_CHECK();
    return 0;
}

// ---- hull ------------------------------------------------------------------------------------------------------------------------------------------
// box height of a table row; 0 for an absent id (cerb_inst_table leaves y1 = h, y2 = 0 there)
__device__ __forceinline__ long long box_rows(const long long* t) { return t[0] > 0 && t[4] > t[3] ? t[4] - t[3] : 0; }

__global__ void hull_clear_kernel(int n_inst, const long long* __restrict__ table, const long long* __restrict__ row_offsets, int* __restrict__ ext) {
    const int lane = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6, waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long i = wave; i < n_inst; i += waves) {
        const long long rows = box_rows(table + 16 * i);
        int* e = ext + 2 * row_offsets[i];
        for (long long r = lane; r < rows; r += 64) {
            e[2 * r] = INT_MAX;
            e[2 * r + 1] = INT_MIN;
        }
    }
}

__global__ void hull_extent_kernel(const int* __restrict__ lab, long long stride, int H, int W, int n_inst, const long long* __restrict__ table,
                                   const long long* __restrict__ row_offsets, int* __restrict__ ext) {
    const long long n = (long long)H * W;
    const int lane = threadIdx.x & 63;
    for (long long p0 = (blockIdx.x * (long long)blockDim.x + threadIdx.x) - lane; p0 < n; p0 += (long long)gridDim.x * blockDim.x) {
        const RunLane r = run_lane(lab, stride, W, n_inst, p0 + lane, n, lane);
        if (r.head && r.l) {
            const long long* t = table + 16ll * (r.l - 1);
            const long long dy = r.y - t[3];
            if (dy >= 0 && dy < box_rows(t)) {  // (a table that is not this map's: no row outside the instance's own slots)
                int* e = ext + 2 * (row_offsets[r.l - 1] + dy);
                atomicMin(e, r.x);
                atomicMax(e + 1, r.x + r.len - 1);
            }
        }
    }
}

// One thread per instance.  The extents of row r are read before anything is written to slot r, and each chain's stack never holds more entries than
// rows read, so both stacks live in the extents themselves: entry k of the left chain in ext[2k], of the right chain in ext[2k + 1], each packed as
// (row << 16) | (x - x1) -- box sides below 2^16.
__global__ void hull_chain_kernel(int n_inst, const long long* __restrict__ table, const long long* __restrict__ row_offsets, int* __restrict__ ext,
                                  int* __restrict__ pts_out, long long* __restrict__ shape) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_inst; i += gridDim.x * blockDim.x) {
        const long long* t = table + 16ll * i;
        long long* s = shape + 8ll * i;
        const long long rows = box_rows(t);
        if (rows == 0) {
            s[5] = s[6] = s[7] = 0;
            continue;
        }
        const long long x1 = t[5], y1 = t[3];
        if (rows >= 65536 || t[6] - x1 >= 65536) {  // outside the stated bound: flagged, not computed
            s[5] = s[6] = s[7] = -1;
            continue;
        }
        int* e = ext + 2 * row_offsets[i];
        auto px = [](int v) { return (long long)(v & 0xFFFF); };
        auto py = [](int v) { return (long long)((unsigned)v >> 16); };
        auto cross = [&](int a, int b, long long cx, long long cy) { return (px(b) - px(a)) * (cy - py(a)) - (py(b) - py(a)) * (cx - px(a)); };
        int nl = 0, nr = 0, filled = 0;
        for (long long r = 0; r < rows; ++r) {
            const int lo = e[2 * r], hi = e[2 * r + 1];
            if (lo > hi) continue;  // an empty row: the instance has several pieces
            ++filled;
            const long long lx = lo - x1, rx = hi - x1;
            while (nl >= 2 && cross(e[2 * (nl - 2)], e[2 * (nl - 1)], lx, r) >= 0) --nl;  // the left chain turns left going down; collinear points go
            e[2 * nl++] = (int)((r << 16) | lx);
            while (nr >= 2 && cross(e[2 * (nr - 2) + 1], e[2 * (nr - 1) + 1], rx, r) <= 0) --nr;
            e[2 * nr++ + 1] = (int)((r << 16) | rx);
        }
        // counter-clockwise on the screen (y down): down the left chain, then up the right chain; the chains share their ends when the top or the
        // bottom row holds one pixel
        const bool same_bottom = e[2 * (nl - 1)] == e[2 * (nr - 1) + 1], same_top = e[0] == e[1];
        const int r_hi = nr - 1 - (same_bottom ? 1 : 0), r_lo = (same_top ? 1 : 0);
        const int n_pts = nl + (r_hi >= r_lo ? r_hi - r_lo + 1 : 0);
        int* out = pts_out ? pts_out + 4 * row_offsets[i] : nullptr;
        long long area2 = 0;
        int first = e[0], prev = first;
        for (int k = 0; k < n_pts; ++k) {
            const int v = k < nl ? e[2 * k] : e[2 * (r_hi - (k - nl)) + 1];
            if (out) {
                out[2 * k] = (int)(x1 + px(v));
                out[2 * k + 1] = (int)(y1 + py(v));
            }
            if (k) area2 += px(prev) * py(v) - px(v) * py(prev);
            prev = v;
        }
        area2 += px(prev) * py(first) - px(first) * py(prev);
        s[5] = area2 < 0 ? -area2 : area2;
        s[6] = n_pts;
        s[7] = filled;
    }
}

extern "C" int cerb_inst_hull_rows(const int32_t* labels, long long lab_row_stride, int h, int w, int n_inst, const long long* table,
                                   const long long* row_offsets, int32_t* extents, int32_t* hull_pts_out, long long* shape, void* hip_stream) {
    if (!labels || h <= 0 || w <= 0 || n_inst < 0 || (n_inst > 0 && (!table || !row_offsets || !extents || !shape)))
        return cerb_set_error("cerb_inst_hull_rows: bad arguments");
    if (n_inst == 0) return 0;
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(hull_clear_kernel, dim3(if_grid(64ll * n_inst)), dim3(256), 0, st, n_inst, table, row_offsets, extents);
    hipLaunchKernelGGL(hull_extent_kernel, dim3(if_grid((long long)h * w)), dim3(256), 0, st, labels, lab_row_stride, h, w, n_inst, table, row_offsets,
                       extents);
    hipLaunchKernelGGL(hull_chain_kernel, dim3(if_grid(n_inst, 64)), dim3(64), 0, st, n_inst, table, row_offsets, extents, hull_pts_out, shape);
    IF_CHECK();
    return 0;
}

// ---- relation ----------------------------------------------------------------------------------------------------------------------------------------
__global__ void inst_relate_kernel(const long long* __restrict__ child, int n_child, const int* __restrict__ child_type, const int* __restrict__ plab,
                                   long long pstride, int PH, int PW, int shift, int n_parent, int* __restrict__ parent_of,
                                   unsigned long long* __restrict__ rows) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_child; i += gridDim.x * blockDim.x) {
        const long long* t = child + 16ll * i;
        const long long area = t[0];
        int p = 0;
        if (area > 0) {
            const long long cx = (t[1] / area) >> shift, cy = (t[2] / area) >> shift;
            if (cx >= 0 && cx < PW && cy >= 0 && cy < PH) {
                p = plab[cy * pstride + cx];
                if (p < 0 || p > n_parent) p = 0;
            }
        }
        parent_of[i] = p;
        if (p) {
            unsigned long long* r = rows + 10ll * (p - 1);
            atomicAdd(r + 0, 1ull);
            atomicAdd(r + 1, (unsigned long long)area);
            if (child_type) atomicAdd(r + 2 + (child_type[i] & 7), 1ull);
        }
    }
}

extern "C" int cerb_inst_relate(const long long* child_table, int n_child, const int32_t* child_type, const int32_t* parent_labels,
                                long long parent_row_stride, int ph, int pw, int shift, int n_parent, int32_t* parent_of, long long* parent_rows,
                                void* hip_stream) {
    if (!parent_labels || ph <= 0 || pw <= 0 || n_child < 0 || n_parent < 0 || shift < 0 || shift > 30 || (n_child > 0 && (!child_table || !parent_of)) ||
        (n_parent > 0 && !parent_rows))
        return cerb_set_error("cerb_inst_relate: bad arguments");
    hipStream_t st = (hipStream_t)hip_stream;
    if (n_parent > 0) hipLaunchKernelGGL(if_fill_ll_kernel, dim3(if_grid(10ll * n_parent)), dim3(256), 0, st, parent_rows, 10ll * n_parent, 0ll);
    if (n_child > 0)
        hipLaunchKernelGGL(inst_relate_kernel, dim3(if_grid(n_child)), dim3(256), 0, st, child_table, n_child, child_type, parent_labels, parent_row_stride,
                           ph, pw, shift, n_parent, parent_of, (unsigned long long*)parent_rows);
    IF_CHECK();
    return 0;
}

// ---- k nearest neighbours ------------------------------------------------------------------------------------------------------------------------------
#define KNN_BLOCK 64
#define KNN_TILE 256
// Candidates are visited in ascending index order and a newcomer only passes entries that are STRICTLY farther, so equal distances stay in index order.
template <int K>
__global__ __launch_bounds__(KNN_BLOCK) void points_knn_kernel(const int2* __restrict__ xy, int n, int* __restrict__ idx_out, long long* __restrict__ d2_out) {
    __shared__ int2 tile[KNN_TILE];
    const int i = blockIdx.x * KNN_BLOCK + threadIdx.x;
    const int2 q = i < n ? xy[i] : make_int2(0, 0);
    long long bd[K];
    int bi[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
        bd[t] = LLONG_MAX;
        bi[t] = -1;
    }
    for (int j0 = 0; j0 < n; j0 += KNN_TILE) {
        __syncthreads();
        for (int t = threadIdx.x; t < KNN_TILE; t += KNN_BLOCK)
            if (j0 + t < n) tile[t] = xy[j0 + t];
        __syncthreads();
        const int m = min(KNN_TILE, n - j0);
        for (int t = 0; t < m; ++t) {
            const int2 c = tile[t];
            const long long dx = (long long)c.x - q.x, dy = (long long)c.y - q.y;
            const long long d = dx * dx + dy * dy;
            if (d < bd[K - 1] && j0 + t != i) {
                bd[K - 1] = d;
                bi[K - 1] = j0 + t;
#pragma unroll
                for (int u = K - 1; u > 0; --u) {
                    if (bd[u] < bd[u - 1]) {
                        const long long td = bd[u];
                        bd[u] = bd[u - 1];
                        bd[u - 1] = td;
                        const int ti = bi[u];
                        bi[u] = bi[u - 1];
                        bi[u - 1] = ti;
                    }
                }
            }
        }
    }
    if (i < n) {
#pragma unroll
        for (int t = 0; t < K; ++t) {
            idx_out[(long long)i * K + t] = bi[t];
            d2_out[(long long)i * K + t] = bi[t] < 0 ? -1 : bd[t];
        }
    }
}

extern "C" int cerb_points_knn(const int32_t* xy, int n, int k, int32_t* idx_out, long long* d2_out, void* hip_stream) {
    if (n < 0 || k < 1 || k > 8 || (n > 0 && (!xy || !idx_out || !d2_out))) return cerb_set_error("cerb_points_knn: bad arguments (1 <= k <= 8)");
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)hip_stream;
    const dim3 grid((n + KNN_BLOCK - 1) / KNN_BLOCK), block(KNN_BLOCK);
    const int2* p = (const int2*)xy;
    switch (k) {
        case 1: hipLaunchKernelGGL(points_knn_kernel<1>, grid, block, 0, st, p, n, idx_out, d2_out); break;
        case 2: hipLaunchKernelGGL(points_knn_kernel<2>, grid, block, 0, st, p, n, idx_out, d2_out); break;
        case 3: hipLaunchKernelGGL(points_knn_kernel<3>, grid, block, 0, st, p, n, idx_out, d2_out); break;
        case 4: hipLaunchKernelGGL(points_knn_kernel<4>, grid, block, 0, st, p, n, idx_out, d2_out); break;
        case 5: hipLaunchKernelGGL(points_knn_kernel<5>, grid, block, 0, st, p, n, idx_out, d2_out); break;
        case 6: hipLaunchKernelGGL(points_knn_kernel<6>, grid, block, 0, st, p, n, idx_out, d2_out); break;
        case 7: hipLaunchKernelGGL(points_knn_kernel<7>, grid, block, 0, st, p, n, idx_out, d2_out); break;
        default: hipLaunchKernelGGL(points_knn_kernel<8>, grid, block, 0, st, p, n, idx_out, d2_out); break;
    }
    IF_CHECK();
    return 0;
}
